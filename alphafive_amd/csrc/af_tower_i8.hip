// af_tower_i8.hip — the residual blocks of the tower in int8 (W8A8) for gfx950, 11x11 boards (C ABI: the af_tower_i8_* part of
// include/af_tower_bf16.h; the arithmetic, the fragment map and the layouts are specified by alphafive_amd/tower_i8.py, which the
// tests hold these kernels to).  Part of libaf_tower.so: the handle, its one allocation and the pack paths are af_tower_bf16.hip's.
//
// af_tower_conv_i8<PROJ, OBF, DEPTH> is af_tower_conv's convolution — 3x3, 128 -> 128, implicit GEMM, weight-stationary and
// persistent, a position's planes double-buffered in LDS by LDS-DMA, B fragments one ds_read_b128 at lane base + compile-time
// offset, the zero region for a row's missing neighbours — on v_mfma_i32_32x32x32_i8: M = 32 couts, N = 32 pixels, K = 32 cin of
// one tap, the same 16 bytes per lane and the same cycles as the bf16 MFMA at twice the K.  A unit is still 16 bytes = one lane's
// B operand, now 16 int8 channels ("C16": int8 [batch][8][144][16], pixel (y, x) at unit 11 (y + 1) + x).  Per convolution: 36
// k-steps instead of 72 (+4 instead of +8 for the projection, PROJ), 18 KB staged per plane instead of 36.
//
// What the halved weights are spent on: TWO COUT TILES PER WAVE.  A wave keeps the A fragments of 64 couts — 2 x 36 [40] fragments
// of 16 int8 = 288 [320] registers, the bf16 kernel's budget, the upper part pinned in accumulator registers as there — and
// computes them for two of the position's four pixel tiles: wave w = cout half w & 1, pixel tiles 2 (w >> 1) and + 1.  A B
// fragment read from LDS then feeds two MFMAs, so a position costs a wave 72 [80] ds_read_b128 for 144 [160] MFMAs where the bf16
// kernel reads 288 [320] for 288 [320]: LDS operand bytes per MFMA, which is what the bf16 tower spends its power cap on, are
// halved once by the data type and once more by this.  Four live accumulator sets (2 cout tiles x 2 pixel tiles), as before.
//
// Staging: a plane is 18,432 B = 4.5 LDS-DMA rounds of 256 lanes x 16 B.  PADDED PLANE: a plane owns a 20,480-byte slot in LDS
// and is staged in five whole rounds; the upper 128 lanes of the fifth re-read the plane's first unit (an address inside the
// position, whatever the batch) and land in the slot's last 2 KB, which no tap reaches (static_assert below).  Positions are
// never paired, so every batch walks the same code.
//
// Epilogue, in tower_i8.py's order: pre = fmaf(float(acc), m[c], b[c]) — explicit, the library is built with contraction on —
// y = elu1(pre), then either q = clamp(rint(y * r_out), -127, 127), one 16-byte store of a lane's 16 consecutive couts = one C16
// unit, or (OBF, the last block's second convolution) y rounded to bf16, two C8 units as af_tower_conv stores them.  m and b wait
// in LDS (1 KB, read once per position and accumulator set); r_out is read from device memory at the top.  Scales and multipliers
// never travel by value, so a captured launch follows a re-pack.
//
// af_tower_conv_i8_small<PROJ, OBF> is the same layer for a handful of positions, one workgroup per pixel tile with the weights
// streamed (af_tower_forward_i8_small; its own comment, behind the kernel above; the same bits).
//
// The packers (af_tower_pack_i8_kernel), the entry quantiser (af_tower_quantize_i8_kernel) and the kernels of the device
// calibration (af_tower_absmax_kernel, af_tower_i8_finalize_kernel) are at the end, with the host part.
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include <vector>

#include "af_tower_common.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

namespace {

using G = Geo<11>;
constexpr uint32_t kPlane16 = 8u * G::PIX * 16u;                        // bytes per position in memory, C16: 18,432
constexpr uint32_t kPlane8 = 16u * G::PIX * 16u;                        // ... and of the bf16 C8 layout: 36,864
constexpr int kRounds = 5;                                              // LDS-DMA rounds per plane: 4.5, padded
constexpr uint32_t kSlot = kRounds * 4096u;                             // a plane's slot in LDS: 20,480
constexpr uint32_t kZero16 = 14592u;                                    // the zero region: largest tap offset + a lane's bank offset + one unit, rounded up
constexpr uint32_t kMbBytes = 2u * 128u * 4u;                           // m[128], b[128]
constexpr uint32_t zero_off(bool proj) { return kLds0 + (proj ? 3u : 2u) * kSlot; }     // LDS: [256 B][g0][g1]([h])[zero region][m, b]
constexpr uint32_t mb_off(bool proj) { return zero_off(proj) + kZero16; }
constexpr uint32_t lds_bytes(bool proj) { return mb_off(proj) + kMbBytes; }              // 56,832 / 77,312
// the farthest unit a lane can form inside a plane — past-board lanes keep pixel 0's base — is channel group 7 (kg = 1, cc = 3),
// the last pixel, tap (2, 2): inside the plane proper, so the slot's pad behind it is never read
static_assert((G::LPIX + G::NPIX - 2) + 6 * G::LPIX + 2 * G::S + 2 < 8 * G::LPIX, "largest tap offset against the end of the plane");
static_assert(255u + (6u * G::LPIX + 2u * G::S + 2u) * 16u + 16u <= kZero16 && kZero16 % 16 == 0, "largest tap offset against the end of the zero region");
static_assert(kPlane16 <= kSlot && kSlot - kPlane16 == 2048u, "four and a half rounds in a slot of five");
static_assert(lds_bytes(true) <= 160u * 1024u, "a gfx950 workgroup has 163,840 bytes of LDS");

struct I8Args {
    const char* in;       // C16 int8: input of the 3x3 convolution
    const char* in2;      // PROJ: the block input (1x1 projection), C16
    const uint4* w;       // [2 cout halves][NS][64 lanes] A fragments of 16 int8
    const float* mb;      // m[128] then b[128]
    const float* r_out;   // reciprocal scale of the int8 tensor written (one word in device memory); unused when OBF
    char* out;            // C16 int8, or C8 bf16 (OBF)
    int batch;
};

// 4 KB piece r of position pos's plane -> LDS at byte offset off behind lds0 (wave wv's 1 KB of it)
__device__ __forceinline__ void stage_round16(uint32_t lds0, uint32_t wv, const char* src, int pos, uint32_t off, int r) {
    uint32_t o = threadIdx.x * 16u + (uint32_t)r * 4096u;
    if (r == kRounds - 1) o = o < kPlane16 ? o : 0u;                    // the fifth round's upper half: the plane's first unit again
    const uint32_t ld = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds0 + off + wv * 1024u + (uint32_t)r * 4096u));
    glds16(src + (size_t)pos * kPlane16 + o, ld);
}

constexpr int kVSlack16 = 88;    // architectural VGPRs left to everything that is not a weight fragment or the B-fragment ring (as af_tower_bf16.hip)

template <bool PROJ, bool OBF, int DEPTH>
__global__ __launch_bounds__(256, 1) void af_tower_conv_i8_kernel(I8Args A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NK = PROJ ? 40 : 36, NS = 2 * NK, NPK = PROJ ? 4 : 0;  // k-steps, A fragments per wave, projection k-steps
    const int lane = threadIdx.x & 63, kg = lane >> 5, nn = lane & 31;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t cp = wv & 1u, pp = wv >> 1;                          // cout half, pixel-tile pair
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem + kLds0;
    int pos = first_position();
    if (pos >= A.batch) return;

    // the zero region, m and b, and the planes of the first position on their way
    for (uint32_t u = threadIdx.x; u < kZero16 / 16; u += 256) *reinterpret_cast<uint4*>(smem + zero_off(PROJ) + u * 16) = uint4{0, 0, 0, 0};
    reinterpret_cast<float*>(smem + mb_off(PROJ))[threadIdx.x] = A.mb[threadIdx.x];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) stage_round16(lds0, wv, A.in, pos, 0u, r);
    if (PROJ) {
#pragma unroll
        for (int r = 0; r < kRounds; ++r) stage_round16(lds0, wv, A.in2, pos, 2u * kSlot, r);
    }
    // resident weights: fragment f = 2 * k-step + cout tile
    i32x4 W[NS];
    {
        const uint4* wp = A.w + ((size_t)cp * NS * 64 + lane);
#pragma unroll
        for (int f = 0; f < NS; ++f) {
            const uint4 v = wp[f * 64];
            __builtin_memcpy(&W[f], &v, 16);
        }
    }
    float rq = 0.0f;
    if (!OBF) rq = A.r_out[0];
    // the lane's pixel in its two pixel tiles: LDS byte base of tap (0, 0), output unit, zero-region base (af_tower_bf16.hip: pixel_bases)
    uint32_t lb[2], ob[2], zb[2];
    bool ok[2], edgeL[2], edgeR[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int n = 32 * (2 * (int)pp + jj) + nn;
        ok[jj] = n < G::NPIX;
        const int nc = ok[jj] ? n : 0;
        const int x = nc % G::S;
        edgeL[jj] = x == 0; edgeR[jj] = x == G::S - 1;
        lb[jj] = kLds0 + (uint32_t)(kg * G::LPIX + nc + G::S - (G::S + 1)) * 16u;
        ob[jj] = (uint32_t)(nc + G::S) * 16u;
        zb[jj] = zero_off(PROJ) + (lb[jj] & 255u);
    }
    // pin the weight loads' completion in front of the position loop, the upper fragments in accumulator registers (af_tower_bf16.hip: pin_and_sync)
    {
        constexpr int kNVfit = (256 - 4 * DEPTH - kVSlack16) / 4, kNVmin = NS - (256 - 64) / 4;
        constexpr int NV = kNVfit > kNVmin ? kNVfit : kNVmin;
#pragma unroll
        for (int f = 0; f < NS; ++f) {
            if (f < NV) asm volatile("" : "+v"(W[f]));
            else asm volatile("" : "+a"(W[f]));
        }
        asm volatile("" : "+v"(rq));
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     // first planes landed; zero region, m and b written
        __builtin_amdgcn_s_barrier();
    }
    const float* const mbs = reinterpret_cast<const float*>(smem + mb_off(PROJ));

    for (int it = 0; pos < A.batch; pos += gridDim.x, ++it) {
        const uint32_t gcur = (it & 1) ? kSlot : 0u, gnxt = kSlot - gcur;
        const int nxt = pos + (int)gridDim.x;
        const bool more = nxt < A.batch;
        uint32_t bC[2], bL[2], bR[2];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            bC[jj] = !ok[jj] ? zb[jj] : gcur + lb[jj];
            bL[jj] = edgeL[jj] ? zb[jj] : bC[jj];
            bR[jj] = edgeR[jj] ? zb[jj] : bC[jj];
        }
        i32x16 acc[4];                                                  // [2 * pixel tile + cout tile]
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0;
        // B read q of the position: pixel tile q & 1 of k-step q >> 1 (PROJ: its 4 projection steps, block-input plane, first);
        // it feeds MFMAs 2q and 2q + 1, one per cout tile.  The reads ride a DEPTH-deep register ring: read q + DEPTH is issued
        // right behind the MFMAs of read q, so it has 2 DEPTH MFMAs to land.
        constexpr int NB = 2 * NK;
        auto rd = [&](int q) -> i32x4 {
            const int jj = q & 1, s = q >> 1;
            if (s < NPK) return *reinterpret_cast<const i32x4*>(smem + 2u * kSlot + lb[jj] + (uint32_t)(2 * s * G::LPIX + G::S + 1) * 16u);
            const int s_ = s - NPK, t = s_ >> 2, cc = s_ & 3;
            const uint32_t base = t % 3 == 0 ? bL[jj] : (t % 3 == 2 ? bR[jj] : bC[jj]);
            return *reinterpret_cast<const i32x4*>(smem + base + (uint32_t)(2 * cc * G::LPIX + (t / 3) * G::S + (t % 3)) * 16u);
        };
        i32x4 ring[DEPTH];
#pragma unroll
        for (int q = 0; q < DEPTH; ++q) ring[q] = rd(q);
#pragma clang loop unroll(full)
        for (int q = 0; q < NB; ++q) {
            const int jj = q & 1, s = q >> 1, ws = s < NPK ? 36 + s : s - NPK;
            acc[2 * jj] = __builtin_amdgcn_mfma_i32_32x32x32_i8(W[2 * ws], ring[q % DEPTH], acc[2 * jj], 0, 0, 0);
            acc[2 * jj + 1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(W[2 * ws + 1], ring[q % DEPTH], acc[2 * jj + 1], 0, 0, 0);
            if (q + DEPTH < NB) ring[q % DEPTH] = rd(q + DEPTH);
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);   // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
            // the next position's planes, one 4 KB piece every 16 MFMAs (in one burst they would stall the matrix pipe)
            if (q % 8 == 0 && q / 8 < kRounds && more) stage_round16(lds0, wv, A.in, nxt, gnxt, q / 8);
            if (PROJ && q >= 2 * NPK && (q - 2 * NPK) % 8 == 4 && (q - 2 * NPK) / 8 < kRounds && more)
                stage_round16(lds0, wv, A.in2, nxt, 2u * kSlot, (q - 2 * NPK) / 8);
            if (PROJ && q == 2 * NPK - 1) {
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();                    // every wave is done with the projection plane
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // the next position's planes have landed ...
        __builtin_amdgcn_s_barrier();                                   // ... for every wave, and all are done with this one
        // epilogue.  A lane's 16 accumulator rows are the 16 consecutive couts 64 cp + 32 ct + 16 kg + r: channel group
        // 4 cp + 2 ct + kg of the C16 layout (one 16-byte unit per pixel), channel octets twice that and + 1 of C8.
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const uint32_t grp = 4u * cp + 2u * ct + (uint32_t)kg;
                const float* const mr = mbs + 16u * grp;
                float y[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) y[r] = elu1(__fmaf_rn((float)acc[2 * jj + ct][r], mr[r], mr[128 + r]));
                if (OBF) {
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        bf16x8_t v;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = (__bf16)y[8 * hf + e];
                        if (ok[jj]) *reinterpret_cast<bf16x8_t*>(A.out + (size_t)pos * kPlane8 + (uint32_t)((2 * grp + hf) * G::PIX) * 16u + ob[jj]) = v;
                    }
                } else {
                    uint32_t d[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        d[k] = 0u;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float q = fminf(fmaxf(__builtin_rintf(__fmul_rn(y[4 * k + e], rq)), -127.0f), 127.0f);
                            d[k] |= ((uint32_t)(int)q & 255u) << (8 * e);
                        }
                    }
                    if (ok[jj]) *reinterpret_cast<uint4*>(A.out + (size_t)pos * kPlane16 + (uint32_t)(grp * G::PIX) * 16u + ob[jj]) = uint4{d[0], d[1], d[2], d[3]};
                }
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// af_tower_conv_i8_small<PROJ, OBF>: the same layer for a handful of positions (af_tower_forward_i8_small), after
// af_tower_bf16.hip's af_tower_conv_small.  The kernel above is weight-stationary: a workgroup loads its 147 / 164 KB of A
// fragments before its first MFMA and then walks positions, which at batch 1 is one workgroup on one CU.  Here the work is split
// the other way:
//   - one workgroup per (position, pixel tile): grid = batch * 4, workgroup b = tile b & 3 of position b >> 2; its 4 waves are
//     the 4 cout tiles of 32: wave w = cout tile w & 1 of cout half w >> 1, i.e. fragments f = 2 * k-step + (w & 1) of half
//     w >> 1 of the stream [2][NS][64][16] the kernel above keeps resident — no other packer, no other buffer;
//   - the workgroup stages the position's plane (PROJ: and the block-input plane) once, single-buffered, with stage_round16 into
//     the LDS layout above (the second slot stays unused), so the zero region, the edge bases and the tap offsets are the same;
//   - a wave runs its tile's 36 / 40 MFMAs into ONE accumulator — a single chain of v_mfma_i32_32x32x32_i8, in the order above
//     (PROJ: the four projection steps first, then tap major, cin step minor);
//   - the A fragments are not resident: fragment i of that order streams through a ring of kSmallA8 register sets, its load
//     issued kSmallA8 MFMAs before its use, so the first MFMA waits for the planes and ONE fragment, not for all of them.  The
//     prefill is issued behind the staging loads and in front of the wait that counts them out: loads return in order, so
//     vmcnt(kSmallA8) means every LDS-DMA piece has landed;
//   - the epilogue is the one above for the lane's 16 couts: fmaf(float(acc), m, b), elu1, then multiply by r_out, rint, clamp
//     and one 16-byte C16 store, or (OBF) the bf16 rounding and the two C8 stores.  m, b and r_out are read from device memory
//     (a lane's 16 + 16 + 1 words, behind the barrier), never passed by value: a captured launch follows a re-pack.
// The int32 accumulator is exact in any order and the epilogue is the same sequence on the same operands: bit-identical to
// af_tower_conv_i8_kernel.  Workgroups are independent: no hand-over, no waiting on each other, no atomics.
// IN PLACE.  A block's second convolution runs in place (out = in2 = xq), and the four tile workgroups of a position run
// concurrently, so a workgroup may stage units of xq that a sibling has already overwritten.  xq is read only through the 1x1
// projection, at the lane's OWN pixel: the centre unit of a pixel this workgroup computes, which nobody else writes and which
// this workgroup writes after its own staging has landed (the wait and the barrier below are in front of every store).  The 3x3
// window reads gq, which this launch does not write.  A lane whose pixel does not exist reads pixel 0's unit of another tile
// in the projection (whatever it finds) and the zero region in the window, and never stores.  The padded fifth staging round
// re-reads the plane's first unit into the slot's pad, which no tap reaches (the static_asserts above).
// Ring depth by measurement (profiles/tower_int8_small.md): 8, 12 and 16 are level, 24, 32 (af_tower_conv_small's) and 36 (all of
// them in front) each a little slower at batches 1, 8 and 64; 16 is the deepest of the level ones.
constexpr int kSmallA8 = 16;     // A-fragment ring: 16 KB per wave in flight
constexpr int kSmallB8 = 8;      // B-fragment ring, as af_tower_conv_small's
template <bool PROJ, bool OBF>
__global__ __launch_bounds__(256) void af_tower_conv_i8_small(I8Args A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];         // [256 B][g][-]([h])[zero region][-]: the layout above
    constexpr int NK = PROJ ? 40 : 36, NS = 2 * NK, NPK = PROJ ? 4 : 0;  // MFMAs of the chain, fragments per cout half of the stream, projection steps
    static_assert(kSmallA8 <= 63 && kSmallA8 <= NK, "the ring's prefill is counted on vmcnt");
    const int lane = threadIdx.x & 63, kg = lane >> 5, nn = lane & 31;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem + kLds0;
    const int pos = (int)(blockIdx.x >> 2), j = (int)(blockIdx.x & 3);  // position (< batch by the grid), pixel tile
    for (uint32_t u = threadIdx.x; u < kZero16 / 16; u += 256) *reinterpret_cast<uint4*>(smem + zero_off(PROJ) + u * 16) = uint4{0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < kRounds; ++r) stage_round16(lds0, wv, A.in, pos, 0u, r);
    if (PROJ) {
#pragma unroll
        for (int r = 0; r < kRounds; ++r) stage_round16(lds0, wv, A.in2, pos, 2u * kSlot, r);
    }
    // A fragment of MFMA i: the projection's (k-steps 36..39 of the stream) first
    const uint4* wp = A.w + ((size_t)(wv >> 1) * NS * 64 + (wv & 1u) * 64 + lane);
    auto frag = [&](int i) -> i32x4 {
        const uint4 v = wp[(i < NPK ? 36 + i : i - NPK) * 128];
        i32x4 f;
        __builtin_memcpy(&f, &v, 16);
        return f;
    };
    i32x4 ra[kSmallA8];
#pragma unroll
    for (int i = 0; i < kSmallA8; ++i) ra[i] = frag(i);
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(kSmallA8) : "memory");   // planes landed, zero region written
    __builtin_amdgcn_s_barrier();
    // the lane's 16 couts 32 wv + 16 kg + r: channel group 2 wv + kg of C16
    const uint32_t grp = 2u * wv + (uint32_t)kg;
    float m_r[16], b_r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { m_r[r] = A.mb[16u * grp + r]; b_r[r] = A.mb[128u + 16u * grp + r]; }
    float rq = 0.0f;
    if (!OBF) rq = A.r_out[0];
    // the lane's pixel of tile j: bases as in the kernel above, for that one tile
    const int n = 32 * j + nn;
    const bool ok = n < G::NPIX;
    const int nc = ok ? n : 0;
    const int px = nc % G::S;
    const uint32_t lb = kLds0 + (uint32_t)(kg * G::LPIX + nc + G::S - (G::S + 1)) * 16u;
    const uint32_t ob = (uint32_t)(nc + G::S) * 16u;
    const uint32_t zb = zero_off(PROJ) + (lb & 255u);
    const uint32_t bC = !ok ? zb : lb, bL = px == 0 ? zb : bC, bR = px == G::S - 1 ? zb : bC;
    auto rd = [&](int i) -> i32x4 {
        if (i < NPK) return *reinterpret_cast<const i32x4*>(smem + 2u * kSlot + lb + (uint32_t)(2 * i * G::LPIX + G::S + 1) * 16u);
        const int s_ = i - NPK, t = s_ >> 2, cc = s_ & 3;
        const uint32_t base = t % 3 == 0 ? bL : (t % 3 == 2 ? bR : bC);
        return *reinterpret_cast<const i32x4*>(smem + base + (uint32_t)(2 * cc * G::LPIX + (t / 3) * G::S + (t % 3)) * 16u);
    };
    i32x4 rb[kSmallB8];
#pragma unroll
    for (int i = 0; i < kSmallB8; ++i) rb[i] = rd(i);
    i32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    __builtin_amdgcn_sched_barrier(0);                       // the ring's first reads stay in front: the groups below would take them one by one
#pragma clang loop unroll(full)
    for (int i = 0; i < NK; ++i) {
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ra[i % kSmallA8], rb[i % kSmallB8], acc, 0, 0, 0);
        if (i + kSmallB8 < NK) rb[i % kSmallB8] = rd(i + kSmallB8);
        if (i + kSmallA8 < NK) ra[i % kSmallA8] = frag(i + kSmallA8);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
    }
    float y[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) y[r] = elu1(__fmaf_rn((float)acc[r], m_r[r], b_r[r]));
    if (OBF) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            bf16x8_t v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (__bf16)y[8 * hf + e];
            if (ok) *reinterpret_cast<bf16x8_t*>(A.out + (size_t)pos * kPlane8 + (uint32_t)((2 * grp + hf) * G::PIX) * 16u + ob) = v;
        }
    } else {
        uint32_t d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[k] = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float q = fminf(fmaxf(__builtin_rintf(__fmul_rn(y[4 * k + e], rq)), -127.0f), 127.0f);
                d[k] |= ((uint32_t)(int)q & 255u) << (8 * e);
            }
        }
        if (ok) *reinterpret_cast<uint4*>(A.out + (size_t)pos * kPlane16 + (uint32_t)(grp * G::PIX) * 16u + ob) = uint4{d[0], d[1], d[2], d[3]};
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Entry quantiser: bf16 C8 -> int8 C16, q = clamp(rint(fp32(x) * r), -127, 127).  A thread owns one C16 unit of a board pixel: two
// 16-byte loads (channel octets 2k, 2k + 1 of the pixel), one 16-byte vector store.  The zero rows are not touched.
__global__ __launch_bounds__(256) void af_tower_quantize_i8_kernel(const char* x, char* xq, const float* r, int batch) {
    const float rq = r[0];
    const int64_t total = (int64_t)batch * 8 * G::NPIX;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int pos = (int)(i / (8 * G::NPIX)), rem = (int)(i - (int64_t)pos * (8 * G::NPIX));
        const int k = rem / G::NPIX, n = rem - k * G::NPIX;             // k < 8, n < 121
        uint32_t d[4];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const uint4 v = *reinterpret_cast<const uint4*>(x + (size_t)pos * kPlane8 + (uint32_t)((2 * k + hf) * G::PIX + G::S + n) * 16u);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                uint32_t o = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t word = w[2 * p + (e >> 1)];
                    const float f = __uint_as_float((e & 1) ? (word & 0xffff0000u) : (word << 16));
                    const float q = fminf(fmaxf(__builtin_rintf(__fmul_rn(f, rq)), -127.0f), 127.0f);
                    o |= ((uint32_t)(int)q & 255u) << (8 * e);
                }
                d[2 * hf + p] = o;
            }
        }
        *reinterpret_cast<uint4*>(xq + (size_t)pos * kPlane16 + (uint32_t)(k * G::PIX + G::S + n) * 16u) = uint4{d[0], d[1], d[2], d[3]};
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Packer: fp32 weights in device memory (the six tensors of a block, af_tower_update_device's order) -> the int8 A-fragment
// streams, m and b, per tower_i8.py.  One workgroup per (cout, convolution of the block, block): it loads the cout's 1152 weights
// (second convolution: and its 128 projection weights times ratio = a_h / a_g) into LDS, reduces their absmax, and thread i < NS
// then quantises and writes fragment row (k-step i >> 1, lane half i & 1) of that cout: 16 int8, one vector store.  Thread 0
// writes m[c] = s[c] * a_in and b[c].  The same workgroup copies what it read into the handle's fp32 keep (unless it is reading
// the keep itself): the sources a later change of scales re-packs from.  Every index is in range by construction: grid (128, 2, nb).
constexpr int kPackI8Blocks = 8;
constexpr int64_t kKeepFloats = 2 * 147456 + 16384 + 3 * 128;           // a block's six tensors, back to back
__host__ __device__ constexpr int64_t keep_off(int k) {              // where tensor k of the six starts
    return k == 0 ? 0 : k == 1 ? 147456 : k == 2 ? 147456 + 128 : k == 3 ? 2 * 147456 + 128 : k == 4 ? 2 * 147456 + 256 : 2 * 147456 + 256 + 16384;
}
struct PackI8Args {
    const float* src[kPackI8Blocks][6];  // c1_w, c1_b, c2_w, c2_b, res_w, res_b
    float* keep[kPackI8Blocks];
    uint4* wq[kPackI8Blocks][2];
    float* mb[kPackI8Blocks][2];
    const float* act;                    // the scales a[2 * blocks]
    int b0;
};

__device__ __forceinline__ uint32_t quant8(float w, float inv) {
    const float q = fminf(fmaxf(__builtin_rintf(__fmul_rn(w, inv)), -127.0f), 127.0f);
    return (uint32_t)(int)q & 255u;
}

__global__ __launch_bounds__(256) void af_tower_pack_i8_kernel(PackI8Args A) {
    __shared__ float row[1280];
    __shared__ float red[256];
    const int c = blockIdx.x, second = blockIdx.y, j = blockIdx.z, tid = threadIdx.x;
    const int b = A.b0 + j, n = second ? 1280 : 1152, NS = second ? 80 : 72;
    const float a_h = A.act[2 * b], a_g = A.act[2 * b + 1];
    const float ratio = __fdiv_rn(a_h, a_g);
    const float* w3 = A.src[j][second ? 2 : 0] + (size_t)c * 1152;
    const float* wp = A.src[j][4] + (size_t)c * 128;
    float* const keep = A.keep[j];
    const bool copy = keep != A.src[j][0];                              // (the keep is one piece: reading it means all six come from it)
    float amax = 0.0f;
    for (int e = tid; e < n; e += 256) {
        float v;
        if (e < 1152) {
            v = w3[e];
            if (copy) keep[keep_off(second ? 2 : 0) + (size_t)c * 1152 + e] = v;
        } else {
            const float p = wp[e - 1152];
            if (copy) keep[keep_off(4) + (size_t)c * 128 + (e - 1152)] = p;
            v = __fmul_rn(p, ratio);
        }
        row[e] = v;
        amax = fmaxf(amax, fabsf(v));
    }
    red[tid] = amax;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) red[tid] = fmaxf(red[tid], red[tid + k]);
        __syncthreads();
    }
    const float absmax = red[0];
    const bool zero = absmax == 0.0f;
    const float s = zero ? 1.0f : __fdiv_rn(absmax, 127.0f);
    const float inv = __fdiv_rn(127.0f, zero ? 1.0f : absmax);
    if (tid < NS) {
        const int ks = tid >> 1, h = tid & 1;                           // k-step < 40, lane half
        uint32_t d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[k] = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ci = 16 * h + 4 * k + e;                      // < 32
                const float v = ks < 36 ? row[(32 * (ks & 3) + ci) * 9 + (ks >> 2)] : row[1152 + 32 * (ks - 36) + ci];
                d[k] |= quant8(v, inv) << (8 * e);
            }
        }
        const int o = c & 31, m = (o & 3) | (((o >> 4) & 1) << 2) | (((o >> 2) & 1) << 3) | (((o >> 3) & 1) << 4);    // pack_perm(m) = o
        const int half = c >> 6, ct = (c >> 5) & 1;
        A.wq[j][second][((size_t)half * NS + 2 * ks + ct) * 64 + 32 * h + m] = uint4{d[0], d[1], d[2], d[3]};
    }
    if (tid == 0) {
        float bias;
        if (second) {
            const float b2 = A.src[j][3][c], br = A.src[j][5][c];
            if (copy) { keep[keep_off(3) + c] = b2; keep[keep_off(5) + c] = br; }
            bias = __fadd_rn(b2, br);
        } else {
            bias = A.src[j][1][c];
            if (copy) keep[keep_off(1) + c] = bias;
        }
        A.mb[j][second][c] = __fmul_rn(s, second ? a_g : a_h);
        A.mb[j][second][128 + c] = bias;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Device calibration (af_tower_i8_calibrate; specified by tower_i8.scales_from_absmax / calibration_ok).
//
// Absmax of a bf16 C8 buffer over the BOARD pixels — units S .. S + NPIX - 1 of every channel octet, so the result does not rest
// on the zero rows being zero — as the largest magnitude bit pattern: bits & 0x7fff orders bf16 values by magnitude as unsigned
// integers, with the infinities (0x7f80) above every finite value and every NaN above them, so a NaN anywhere is seen.  A thread
// takes one 16-byte unit per pass, kAbsUnroll passes of the grid in flight; the maximum is reduced per lane, per wave
// (__shfl_xor), per workgroup (4 words of LDS) and leaves as ONE atomicMax per workgroup into the caller's word.  A maximum
// does not depend on the order it is taken in: deterministic.  Every address is inside the first `batch` positions by
// construction (i < batch * 16 * NPIX).
constexpr int kAbsUnroll = 4;
constexpr int kAbsMaxBlocks = 1024;
__global__ __launch_bounds__(256) void af_tower_absmax_kernel(const char* x, uint32_t* word, int batch) {
    __shared__ uint32_t red[4];
    const int64_t total = (int64_t)batch * 16 * G::NPIX, stride = (int64_t)gridDim.x * 256;
    uint32_t m = 0u;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < total; i0 += kAbsUnroll * stride) {
        uint4 v[kAbsUnroll];
#pragma unroll
        for (int u = 0; u < kAbsUnroll; ++u) {
            const int64_t i = i0 + u * stride;
            v[u] = uint4{0u, 0u, 0u, 0u};
            if (i < total) {
                const int pos = (int)(i / (16 * G::NPIX)), rem = (int)(i - (int64_t)pos * (16 * G::NPIX));
                const int k = rem / G::NPIX, n = rem - k * G::NPIX;     // k < 16, n < 121
                v[u] = *reinterpret_cast<const uint4*>(x + (size_t)pos * kPlane8 + (uint32_t)(k * G::PIX + G::S + n) * 16u);
            }
        }
#pragma unroll
        for (int u = 0; u < kAbsUnroll; ++u) {
            const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t lo = w[e] & 0x7fffu, hi = (w[e] >> 16) & 0x7fffu;
                m = m > lo ? m : lo;
                m = m > hi ? m : hi;
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, d, 64);
        m = m > o ? m : o;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
        atomicMax(word, a > b ? a : b);
    }
}

// the head of a calibration: its n absmax words start from 0
__global__ __launch_bounds__(64) void af_tower_i8_clear_kernel(uint32_t* words, int n) {
    for (int i = threadIdx.x; i < n; i += 64) words[i] = 0u;
}

// Its tail: one wave turns the n = 2 * blocks words into scales, in tower_i8.scales_from_absmax's operations — a = (absmax *
// margin) / 127, 1 for an absmax of exactly 0, r = 1 / a — and installs them ALL OR NOT AT ALL: only if every absmax is finite and
// every a finite and positive (calibration_ok) are act[0 .. n) = a and act[n .. 2n) = r written, status[0] = 0 and the counter
// status[1] bumped; otherwise act stays as it was and status[0] = 1.  The vote is one __all over the wave, in front of any store.
__global__ __launch_bounds__(64) void af_tower_i8_finalize_kernel(const uint32_t* words, float* act, int32_t* status, int n, float margin) {
    bool ok = true;
    for (int i = threadIdx.x; i < n; i += 64) {
        const uint32_t bits = words[i];
        const float amax = __uint_as_float(bits << 16);
        const float a = bits == 0u ? 1.0f : __fdiv_rn(__fmul_rn(amax, margin), 127.0f);
        ok = ok && bits < 0x7f80u && a > 0.0f && a < __builtin_inff();
    }
    const bool all_ok = __all(ok) != 0;
    if (all_ok)
        for (int i = threadIdx.x; i < n; i += 64) {
            const uint32_t bits = words[i];
            const float a = bits == 0u ? 1.0f : __fdiv_rn(__fmul_rn(__uint_as_float(bits << 16), margin), 127.0f);
            act[i] = a;
            act[n + i] = __fdiv_rn(1.0f, a);
        }
    if (threadIdx.x == 0) {
        status[0] = all_ok ? 0 : 1;
        if (all_ok) status[1] = status[1] + 1;
    }
}

// ------------------------------------------------------------------ host ------------------------------------------------------------------
enum { kW1q, kW2q, kMb1, kMb2 };
constexpr int64_t kQBytes[4] = {2 * 72 * 64 * 16, 2 * 80 * 64 * 16, 2 * 128 * 4, 2 * 128 * 4};
constexpr int kConvDepth = 4;

struct I8Kernel {
    void (*fn)(I8Args);
    bool proj, obf;
};
constexpr I8Kernel kI8[4] = {
    {af_tower_conv_i8_kernel<false, false, kConvDepth>, false, false}, {af_tower_conv_i8_kernel<false, true, kConvDepth>, false, true},
    {af_tower_conv_i8_kernel<true, false, kConvDepth>, true, false},   {af_tower_conv_i8_kernel<true, true, kConvDepth>, true, true},
};

// af_tower_forward_i8_small's kernels, by (PROJ, OBF) as kI8
constexpr I8Kernel kI8Small[4] = {
    {af_tower_conv_i8_small<false, false>, false, false}, {af_tower_conv_i8_small<false, true>, false, true},
    {af_tower_conv_i8_small<true, false>, true, false},   {af_tower_conv_i8_small<true, true>, true, true},
};
// af_tower_i8_small_batch: the largest batch up to which the whole evaluation was measured faster on af_tower_forward_i8_small
// than on af_tower_forward_i8 (profiles/tower_int8_small.md: medians apart by more than both forms' min..max spreads together;
// measured at 1, 2, 4, ... 256: the small form wins by 62 us of 186 at 64; at 128 it is 14 us ahead, inside the spreads, and at
// 256 it loses).
constexpr int32_t kSmallBatchI8 = 64;

size_t padded(int64_t bytes) { return (size_t)((bytes + 255) & ~(int64_t)255); }
int64_t act_bytes(const af_tower* t) { return (int64_t)4 * t->blocks * 4; }
int64_t cal_bytes(const af_tower* t) { return (int64_t)(2 * t->blocks + 2) * 4; }       // the absmax words, status, count

bool ready(const af_tower* t) {
    if (!t->i8) return false;
    for (int b = 0; b < t->blocks; ++b) if (!t->qset[b]) return false;
    return true;
}

int launch_conv(af_tower* t, hipStream_t st, int b, bool second, const void* in, const void* in2, void* out, bool obf, int batch) {
    I8Args a;
    a.in = static_cast<const char*>(in); a.in2 = static_cast<const char*>(in2);
    a.w = reinterpret_cast<const uint4*>(t->qbuf[4 * b + (second ? kW2q : kW1q)]);
    a.mb = reinterpret_cast<const float*>(t->qbuf[4 * b + (second ? kMb2 : kMb1)]);
    a.r_out = t->act + 2 * t->blocks + (obf ? 0 : 2 * b + 1 + (second ? 1 : 0));     // r of g_b, or of h_{b+1}
    a.out = static_cast<char*>(out); a.batch = batch;
    const int over = af_tower_grid_override();
    const int ncu = over > 0 ? over : t->ncu;
    const int grid = batch < ncu ? batch : ncu;
    for (const I8Kernel& k : kI8)
        if (k.proj == second && k.obf == obf) hipLaunchKernelGGL(k.fn, dim3(grid), dim3(256), lds_bytes(second), st, a);
    return AF_TOWER_OK;
}

// the tile-parallel form: one workgroup per pixel tile of a position, whatever the chip and tune key 1
void launch_conv_small(af_tower* t, hipStream_t st, int b, bool second, const void* in, const void* in2, void* out, bool obf, int batch) {
    I8Args a;
    a.in = static_cast<const char*>(in); a.in2 = static_cast<const char*>(in2);
    a.w = reinterpret_cast<const uint4*>(t->qbuf[4 * b + (second ? kW2q : kW1q)]);
    a.mb = reinterpret_cast<const float*>(t->qbuf[4 * b + (second ? kMb2 : kMb1)]);
    a.r_out = t->act + 2 * t->blocks + (obf ? 0 : 2 * b + 1 + (second ? 1 : 0));
    a.out = static_cast<char*>(out); a.batch = batch;
    for (const I8Kernel& k : kI8Small)
        if (k.proj == second && k.obf == obf) hipLaunchKernelGGL(k.fn, dim3((unsigned)batch * 4u), dim3(256), lds_bytes(second), st, a);
}

void launch_quantize(af_tower* t, hipStream_t st, const void* x, void* xq, int batch) {
    const int64_t blocks = ((int64_t)batch * 8 * G::NPIX + 255) / 256;
    hipLaunchKernelGGL(af_tower_quantize_i8_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st,
                       static_cast<const char*>(x), static_cast<char*>(xq), t->act + 2 * t->blocks, batch);
}

// the grid from the batch, capped as launch_quantize's: a thread takes kAbsUnroll units per pass
void launch_absmax(hipStream_t st, const void* x, uint32_t* word, int batch) {
    const int64_t blocks = ((int64_t)batch * 16 * G::NPIX + 256 * kAbsUnroll - 1) / (256 * kAbsUnroll);
    hipLaunchKernelGGL(af_tower_absmax_kernel, dim3((unsigned)(blocks < kAbsMaxBlocks ? blocks : kAbsMaxBlocks)), dim3(256), 0, st,
                       static_cast<const char*>(x), word, batch);
}

}  // namespace

size_t af_tower_i8_arena_bytes(const af_tower* t) {
    if (t->S != 11) return 0;
    size_t total = padded(act_bytes(t)) + padded(cal_bytes(t)) + padded(kKeepFloats * 4) * (size_t)t->blocks;
    for (int k = 0; k < 4; ++k) total += padded(kQBytes[k]) * (size_t)t->blocks;
    return total;
}

int af_tower_i8_carve(af_tower* t, char* p) {
    if (t->S != 11) return AF_TOWER_OK;
    for (const I8Kernel& k : kI8)
        TW_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    for (const I8Kernel& k : kI8Small)
        TW_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(k.proj)));
    for (int b = 0; b < t->blocks; ++b)
        for (int k = 0; k < 4; ++k) { t->qbuf.push_back(p); p += padded(kQBytes[k]); }
    t->act = reinterpret_cast<float*>(p); p += padded(act_bytes(t));
    t->cal = reinterpret_cast<uint32_t*>(p); p += padded(cal_bytes(t));
    TW_HIP_OK(hipMemset(t->cal, 0, (size_t)cal_bytes(t)));              // status 0, no calibration counted yet
    t->keep = reinterpret_cast<float*>(p);
    t->qset.assign(t->blocks, 0);
    return AF_TOWER_OK;
}

static float* keep_of(const af_tower* t, int b) { return t->keep + (size_t)b * (padded(kKeepFloats * 4) / 4); }

void af_tower_i8_pack(const af_tower* t, hipStream_t st, int b0, int nb, const float* const* src) {
    for (int at = 0; at < nb; at += kPackI8Blocks) {
        const int n = nb - at < kPackI8Blocks ? nb - at : kPackI8Blocks;
        PackI8Args a = {};
        for (int j = 0; j < n; ++j) {
            const int b = b0 + at + j;
            for (int k = 0; k < 6; ++k) a.src[j][k] = src[6 * (at + j) + k];
            a.keep[j] = keep_of(t, b);
            a.wq[j][0] = reinterpret_cast<uint4*>(t->qbuf[4 * b + kW1q]); a.wq[j][1] = reinterpret_cast<uint4*>(t->qbuf[4 * b + kW2q]);
            a.mb[j][0] = reinterpret_cast<float*>(t->qbuf[4 * b + kMb1]); a.mb[j][1] = reinterpret_cast<float*>(t->qbuf[4 * b + kMb2]);
            t->qset[b] = 1;
        }
        a.act = t->act; a.b0 = b0 + at;
        hipLaunchKernelGGL(af_tower_pack_i8_kernel, dim3(128, 2, n), dim3(256), 0, st, a);
    }
}

extern "C" {

int af_tower_i8_enable(af_tower* t, const float* act_scales_host, int32_t n) {
    if (!t || !act_scales_host || t->S != 11 || n != 2 * t->blocks) return AF_TOWER_ERR_ARG;
    std::vector<float> h(2 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        const float a = act_scales_host[i];
        if (!(a > 0.0f) || !std::isfinite(a)) return AF_TOWER_ERR_ARG;
        h[i] = a; h[n + i] = 1.0f / a;
    }
    TW_HIP_OK(hipSetDevice(t->device));
    TW_HIP_OK(hipDeviceSynchronize());                                   // forwards in flight read the scales
    TW_HIP_OK(hipMemcpy(t->act, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    t->i8 = true;
    // re-pack, in place, every block whose fp32 sources the handle kept: those set or updated since the first enable
    for (int b = 0; b < t->blocks; ++b)
        if (t->qset[b]) {
            const float* k = keep_of(t, b);
            const float* src[6];
            for (int i = 0; i < 6; ++i) src[i] = k + keep_off(i);
            af_tower_i8_pack(t, nullptr, b, 1, src);
        }
    TW_HIP_OK(hipGetLastError());
    TW_HIP_OK(hipDeviceSynchronize());
    return AF_TOWER_OK;
}

int64_t af_tower_i8_plane_bytes(const af_tower* t) { return t && t->S == 11 ? (int64_t)kPlane16 : 0; }

int af_tower_quantize_i8(af_tower* t, void* stream, const void* x_dev, void* xq_dev, int32_t batch) {
    if (!t || t->S != 11 || !x_dev || !xq_dev || batch < 1) return AF_TOWER_ERR_ARG;
    if (!t->i8) return AF_TOWER_ERR_STATE;
    launch_quantize(t, static_cast<hipStream_t>(stream), x_dev, xq_dev, batch);
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int af_tower_conv_i8(af_tower* t, void* stream, int32_t block, int32_t second, const void* in_dev, const void* in2_dev, void* out_dev,
                     int32_t out_is_bf16, int32_t batch) {
    if (!t || t->S != 11 || block < 0 || block >= t->blocks || !in_dev || (second && !in2_dev) || !out_dev || batch < 1) return AF_TOWER_ERR_ARG;
    if (second && !out_is_bf16 && block == t->blocks - 1) return AF_TOWER_ERR_ARG;      // the last block's output has no int8 scale
    if (!t->i8 || !t->qset[block]) return AF_TOWER_ERR_STATE;
    launch_conv(t, static_cast<hipStream_t>(stream), block, second != 0, in_dev, in2_dev, out_dev, out_is_bf16 != 0, batch);
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int af_tower_forward_i8(af_tower* t, void* stream, void* x_dev, void* xq_dev, void* gq_dev, int32_t batch) {
    if (!t || t->S != 11 || !x_dev || !xq_dev || !gq_dev || batch < 1) return AF_TOWER_ERR_ARG;
    if (!ready(t)) return AF_TOWER_ERR_STATE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    launch_quantize(t, st, x_dev, xq_dev, batch);
    for (int b = 0; b < t->blocks; ++b) {
        const bool last = b == t->blocks - 1;
        launch_conv(t, st, b, false, xq_dev, nullptr, gq_dev, false, batch);
        launch_conv(t, st, b, true, gq_dev, xq_dev, last ? x_dev : xq_dev, last, batch);
    }
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int af_tower_conv_i8_small(af_tower* t, void* stream, int32_t block, int32_t second, const void* in_dev, const void* in2_dev, void* out_dev,
                           int32_t out_is_bf16, int32_t batch) {
    if (!t || t->S != 11 || block < 0 || block >= t->blocks || !in_dev || (second && !in2_dev) || !out_dev || batch < 1) return AF_TOWER_ERR_ARG;
    if (second && !out_is_bf16 && block == t->blocks - 1) return AF_TOWER_ERR_ARG;      // the last block's output has no int8 scale
    if (!t->i8 || !t->qset[block]) return AF_TOWER_ERR_STATE;
    launch_conv_small(t, static_cast<hipStream_t>(stream), block, second != 0, in_dev, in2_dev, out_dev, out_is_bf16 != 0, batch);
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int af_tower_forward_i8_small(af_tower* t, void* stream, void* x_dev, void* xq_dev, void* gq_dev, int32_t batch) {
    if (!t || t->S != 11 || !x_dev || !xq_dev || !gq_dev || batch < 1) return AF_TOWER_ERR_ARG;
    if (!ready(t)) return AF_TOWER_ERR_STATE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    launch_quantize(t, st, x_dev, xq_dev, batch);
    for (int b = 0; b < t->blocks; ++b) {
        const bool last = b == t->blocks - 1;
        launch_conv_small(t, st, b, false, xq_dev, nullptr, gq_dev, false, batch);
        launch_conv_small(t, st, b, true, gq_dev, xq_dev, last ? x_dev : xq_dev, last, batch);
    }
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int32_t af_tower_i8_small_batch(const af_tower* t) { return t && t->S == 11 ? kSmallBatchI8 : 0; }

// ---- activation scales without the host ----
int af_tower_i8_calibrate(af_tower* t, void* stream, void* x_dev, void* g_dev, int32_t batch, float margin) {
    if (!t || t->S != 11 || !x_dev || !g_dev || batch < 1 || !(margin > 0.0f) || !std::isfinite(margin)) return AF_TOWER_ERR_ARG;
    if (!ready(t)) return AF_TOWER_ERR_STATE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = 2 * t->blocks;
    hipLaunchKernelGGL(af_tower_i8_clear_kernel, dim3(1), dim3(64), 0, st, t->cal, n);
    // the bf16 tower's own forward, every stored activation measured on its way: h_b in front of block b, g_b between its layers
    for (int b = 0; b < t->blocks; ++b) {
        launch_absmax(st, x_dev, t->cal + 2 * b, batch);
        int rc = af_tower_launch_layer(t, st, b, false, x_dev, g_dev, batch);
        if (rc) return rc;
        launch_absmax(st, g_dev, t->cal + 2 * b + 1, batch);
        rc = af_tower_launch_layer(t, st, b, true, x_dev, g_dev, batch);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(af_tower_i8_finalize_kernel, dim3(1), dim3(64), 0, st, t->cal, t->act, reinterpret_cast<int32_t*>(t->cal + n), n, margin);
    // ... and every block again from the sources the handle kept, under the scales now in place (a refused calibration: the
    // same bytes once more)
    std::vector<const float*> src(6 * (size_t)t->blocks);
    for (int b = 0; b < t->blocks; ++b)
        for (int i = 0; i < 6; ++i) src[6 * b + i] = keep_of(t, b) + keep_off(i);
    af_tower_i8_pack(t, st, 0, t->blocks, src.data());
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int af_tower_i8_calibration_status(af_tower* t, int32_t* status, int32_t* count) {
    if (!t || t->S != 11 || !status || !count) return AF_TOWER_ERR_ARG;
    if (!t->i8) return AF_TOWER_ERR_STATE;
    int32_t h[2];
    TW_HIP_OK(hipSetDevice(t->device));
    TW_HIP_OK(hipDeviceSynchronize());
    TW_HIP_OK(hipMemcpy(h, t->cal + 2 * t->blocks, sizeof(h), hipMemcpyDeviceToHost));
    *status = h[0]; *count = h[1];
    return AF_TOWER_OK;
}

int af_tower_i8_absmax(af_tower* t, void* stream, const void* x_dev, int32_t batch, uint32_t* word_dev) {
    if (!t || t->S != 11 || !x_dev || !word_dev || batch < 1) return AF_TOWER_ERR_ARG;
    launch_absmax(static_cast<hipStream_t>(stream), x_dev, word_dev, batch);
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int64_t af_tower_i8_debug_weights(af_tower* t, int32_t index, void* host_out, int64_t cap_bytes) {
    if (!t || t->S != 11 || index < 0 || index > 4 * t->blocks) return AF_TOWER_ERR_ARG;
    const bool is_act = index == 4 * t->blocks;
    if (!t->i8 || (!is_act && !t->qset[index / 4])) return AF_TOWER_ERR_STATE;
    const int64_t bytes = is_act ? act_bytes(t) : kQBytes[index % 4];
    if (!host_out) return bytes;
    if (cap_bytes < bytes) return AF_TOWER_ERR_ARG;
    TW_HIP_OK(hipSetDevice(t->device));
    TW_HIP_OK(hipDeviceSynchronize());
    TW_HIP_OK(hipMemcpy(host_out, is_act ? reinterpret_cast<const char*>(t->act) : t->qbuf[index], (size_t)bytes, hipMemcpyDeviceToHost));
    return bytes;
}

}  // extern "C"
