// af_tower_bf16.hip — bf16 residual tower for gfx950 (C ABI: include/af_tower_bf16.h).
//
// Three kernels compute the same 3x3 convolution: af_tower_conv<G, PROJ, DEPTH> and af_tower_conv3<G, PROJ, DEPTH>, weight-stationary
// and persistent, which af_tower_forward launches, and af_tower_conv_small<G, PROJ>, one workgroup per pixel tile with the weights
// streamed, which af_tower_forward_small launches for a handful of positions (its own comment, behind af_tower_conv3; the same
// bits).  The first two are described here: they compute the 3x3 convolution 128 -> 128 over
// 11x11 boards (G = Geo<11>; what follows describes that geometry — Geo<15>, which af_tower_conv alone runs, on half boards, is
// described at the geometry types) as an implicit GEMM
//   out[cout][pixel] = sum_{tap, cin} W[cout][cin][tap] * in[cin][pixel + tap offset]
// on v_mfma_f32_32x32x16_bf16 (M = 32 couts, N = 32 pixels, K = 16 cin of one tap), plus, for the second
// convolution of a block (PROJ), 8 more k-steps that fold the block's 1x1 projection of the block input in.
// They share everything described below — set-up, staging, LDS layout, tap addresses: the functions in front of them, which
// af_tower_conv_small calls too — and differ in their position loops only: af_tower_conv runs a position's MFMAs over four accumulator sets and then its epilogue;
// af_tower_conv3 runs two phases of two pixel tiles and issues the finished pair's epilogue inside the other pair's MFMA stream
// (see its own comment).  Which one runs where is tune key 3 (kConv / pick in the host part): by default af_tower_conv3 for a
// block's first convolution and af_tower_conv for its second (PROJ); 0 = af_tower_conv for both, at the ring depth of key 0;
// 2 = af_tower_conv3 for both.
//
// Work split (weight-stationary, persistent): a workgroup = 4 waves = the 4 cout tiles of 32; each wave keeps
// ALL its weights — 32 couts x (9*128 [+128]) k = 72 [80] A fragments of 8 bf16 = 288 [320] registers — resident
// for the whole launch (one wave per SIMD, 512-register budget) and the workgroup walks over positions with
// stride gridDim.x.  A position's activations (36 KB in the C8 layout, include/af_tower_bf16.h) are copied
// global -> LDS by LDS-DMA (global_load_lds_dwordx4: contiguous, no staging registers), double buffered:
// position i+1 lands while position i multiplies.  In C8, a B fragment (32 pixels x 16 cin) is one
// ds_read_b128 per lane at lane_base + compile-time offset (pixel units are 16 bytes, consecutive pixels are
// consecutive units => conflict-free; for a row's missing left/right neighbours the edge lanes read an all-zero LDS
// region at the same bank offset instead), so the inner loop is ds_read_b128 + MFMA only.
// Epilogue: bias, ELU, round to bf16, two 16-byte stores per pixel tile (the MFMA rows are permuted at pack time so a
// lane holds 16 consecutive couts); the 32 lanes of a k half cover 512 contiguous bytes.
//
// Roofline: 2*128*128*9*121 = 35.7 MFLOP per position and convolution on 2.5 PFLOP/s dense bf16 MFMA;
// per position a workgroup reads 36 KB (+36 KB PROJ) and writes 31 KB of HBM: 8192 positions x 16 convolutions
// = 4.7 TFLOP and ~11 GB per tower pass, i.e. MFMA-bound (1.9 ms) over HBM (1.4 ms at 8 TB/s) by a small margin.
//
// The handle struct and the device helpers the int8 residual blocks (af_tower_i8.hip) share with this file — LDS-DMA, elu1, the
// first position of a persistent workgroup, Geo<S>, pack_perm — are in af_tower_common.h.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <stdint.h>

#include <vector>

#include "af_tower_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// (r3 A/B record, profiles/r3_18_tower_ab.txt; both were build-time switches until nothing built them any other way: the nt hint on
//  the LDS-DMA loads: 5.29 -> 5.17 ms per 8192-position tower pass; lanes past the board read zeros: within noise, 5.16-5.17 with both)
constexpr int kVSlack = 88;      // architectural VGPRs left to everything that is not a weight fragment or the B-fragment ring
#ifndef AF_TOWER_ABL_NOLDS
#define AF_TOWER_ABL_NOLDS 0     // profiling build: af_tower_conv without its B-fragment reads (results wrong by design)
#endif

// (glds16, the LDS-DMA, and elu1, the ELU as max(x, min(exp(x), 1) - 1): af_tower_common.h)
// elu1 two at a time on 2-vectors, which keeps the bias add in front and the "- 1" as v_pk_add_f32 (hipcc's SLP vectoriser pairs them
// in the compare / select form but not in the max form): 3 + v_exp_f32 instead of 4 + v_exp_f32 issue slots per element
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 elu2(f32x2 x) {
    const f32x2 t = x * 1.44269504088896341f;
    f32x2 e;
    e.x = fminf(fmaxf(__builtin_amdgcn_exp2f(t.x), 0.0f), 1.0f);
    e.y = fminf(fmaxf(__builtin_amdgcn_exp2f(t.y), 0.0f), 1.0f);
    const f32x2 em1 = e - 1.0f;
    return f32x2{fmaxf(x.x, em1.x), fmaxf(x.y, em1.y)};
}

struct TowerArgs {
    const char* in;      // C8 bf16 [batch][16][PIX][8]: input of the 3x3 convolution
    const char* in2;     // PROJ: block input (1x1 projection), same layout
    const uint4* w;      // [4 waves][NS][64 lanes] A fragments (8 bf16)
    const float* bias;   // [128]
    char* out;           // C8 bf16
    int batch;
    int abl;             // profiling: bit 0 = stage only the first position, bit 1 = no stores, bit 2 = no ELU
    char* dump;          // af_tower_conv3: 4 KB the lanes past the board store to (an unconditional store keeps the epilogue out of a branch)
};

// Board geometry Geo<S> — 11x11 whole positions, 15x15 as two half boards — and kLds0: af_tower_common.h.
template <class G> struct Lay {
    static constexpr uint32_t kPlaneB = 16u * G::PIX * 16u;             // bytes per position in memory: 36,864 / 65,536
    static constexpr uint32_t kPlaneL = 16u * G::LPIX * 16u;            // bytes per (half-)plane in LDS: 36,864 / 40,960
    static constexpr int kRounds = kPlaneL / (256 * 16);                // 9 / 10 LDS-DMA rounds of 256 lanes x 16 B
    static constexpr uint32_t zero_off(bool proj) { return kLds0 + (proj ? 3u : 2u) * kPlaneL; }      // LDS: [256 B][g0][g1]([h])[zero region]
    static constexpr uint32_t lds_bytes(bool proj) { return zero_off(proj) + G::kZeroB; }            // a launch's dynamic LDS
    static_assert(kPlaneL % 4096 == 0 && G::kZeroB % 16 == 0, "whole LDS-DMA rounds, whole zero units");
    static_assert(lds_bytes(true) <= 160u * 1024u, "a gfx950 workgroup has 163,840 bytes of LDS");
    // the farthest unit a lane can form inside a plane — past-board lanes included (they keep pixel 0's base for the projection tap):
    // channel octet 15 (kg = 1, cc = 7), the last pixel of the larger half, tap (2, 2) — is still inside that plane
    static_assert((G::LPIX + G::HPIX0 - 2) + 14 * G::LPIX + 2 * G::S + 2 < 16 * G::LPIX, "largest tap offset against the end of the plane");
    // ... and the farthest one inside the zero region: bank offset (< 256) + the largest tap offset + the 16 bytes read
    static_assert(255u + (14u * G::LPIX + 2u * G::S + 2u) * 16u + 16u <= G::kZeroB, "largest tap offset against the end of the zero region");
    static_assert(G::HPIX0 <= 128 && G::HPIX1 <= 128 && G::HPIX0 >= G::HPIX1, "a half fits four pixel tiles");
    static_assert(G::HOFF + G::LIVE1 <= G::PIX && G::LIVE0 <= G::LPIX, "what a half stages lies inside the plane");
};

#ifdef AF_TOWER_TIMING
// profiling build only (tools/probe_tower_timing.py): per wave and position, cycles of MFMA loop | wait for the next planes | barrier | epilogue
__device__ unsigned long long g_tower_cyc[2][256][4][5];
#define TT(v) const unsigned long long v = __builtin_readcyclecounter()
#else
#define TT(v)
#endif

// ---- what both convolution kernels are made of.  Free functions over the kernels' own register arrays, taken BY REFERENCE: gathered
// into a struct that a member function fills, the same code made hipcc park values in accumulator registers and read them back inside
// af_tower_conv3's steady-state MFMA blocks (+2 to +8 v_accvgpr_read_b32 per 16-MFMA block: profiles/tower_conv_shared_setup.md).
// lane, kg = lane >> 5 and nn = lane & 31 are the kernel's, computed at its top (derived again in here they cost registers) ----

// 4 KB piece r of a position's plane -> LDS at byte offset off behind lds0 (wave wv's 1 KB of it).  HALVES = 2: pos is a
// pseudo-position (board pos >> 1, half pos & 1) and the piece is gathered: LDS unit u = 256 r + thread = (octet u / LPIX, unit w of
// the half-plane) comes from plane unit HOFF * half + w of that octet.  The LDS-DMA writes all 256 units of a piece whatever the
// lane's address, so a lane whose unit the half does not stage (w >= LIVE: the pad of the half-plane, and half 1's tenth row,
// which would lie past the plane) re-reads the half's first unit; no tap of a live pixel reaches those units.
template <class G>
__device__ __forceinline__ void stage_round(uint32_t lds0, uint32_t wv, const char* src, int pos, uint32_t off, int r) {
    const char* gp;
    if constexpr (G::HALVES == 1) {
        gp = src + (size_t)pos * Lay<G>::kPlaneB + threadIdx.x * 16u + r * 4096;
    } else {
        const uint32_t half = (uint32_t)pos & 1u, u = (uint32_t)r * 256u + threadIdx.x, oct = u / (uint32_t)G::LPIX, w = u - oct * G::LPIX;
        const uint32_t wl = w < (half ? (uint32_t)G::LIVE1 : (uint32_t)G::LIVE0) ? w : 0u;
        gp = src + (size_t)(pos >> 1) * Lay<G>::kPlaneB + (oct * G::PIX + half * G::HOFF + wl) * 16u;
    }
    const uint32_t ld = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds0 + off + wv * 1024u + r * 4096u));
    glds16(gp, ld);
}

// the zero region, and the planes of the workgroup's first position on their way
template <class G, bool PROJ>
__device__ __forceinline__ void stage_first(const TowerArgs& A, char* smem, uint32_t lds0, uint32_t wv, int pos) {
    for (uint32_t u = threadIdx.x; u < G::kZeroB / 16; u += 256) *reinterpret_cast<uint4*>(smem + Lay<G>::zero_off(PROJ) + u * 16) = uint4{0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < Lay<G>::kRounds; ++r) stage_round<G>(lds0, wv, A.in, pos, 0u, r);
    if (PROJ) {
#pragma unroll
        for (int r = 0; r < Lay<G>::kRounds; ++r) stage_round<G>(lds0, wv, A.in2, pos, 2u * Lay<G>::kPlaneL, r);
    }
}

// resident weights and bias
template <int NS>
__device__ __forceinline__ void load_weights(const TowerArgs& A, uint32_t wv, int lane, int kg, bf16x8 (&W)[NS], float (&bias_r)[16]) {
    const uint4* wp = A.w + ((size_t)wv * NS * 64 + lane);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint4 v = wp[s * 64];
        __builtin_memcpy(&W[s], &v, 16);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) bias_r[r] = A.bias[32 * wv + 16 * kg + r];   // MFMA rows are permuted at pack time: see pack_perm
}

// the lane's pixel in each of the 4 pixel tiles: LDS byte base of tap (0,0) (one row up, one pixel left).  Rows are
// stored back to back (no pad columns: consecutive lanes read consecutive 16-byte units, which is what keeps
// ds_read_b128 conflict-free); for the left / right taps of the first / last pixel of a row the lane reads zeros
// from a dedicated LDS region (a different base register, no per-read VALU).
template <class G>
__device__ __forceinline__ void pixel_bases(uint32_t zoff, int kg, int nn, uint32_t (&lb)[4], uint32_t (&ob)[4], uint32_t (&zb)[4],
                                            bool (&ok)[4], bool (&edgeL)[4], bool (&edgeR)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = 32 * j + nn;
        ok[j] = n < G::HPIX0;                                           // (HALVES = 2: half 1 has fewer, see the position loop)
        const int nc = ok[j] ? n : 0;
        const int x = nc % G::S;
        edgeL[j] = x == 0; edgeR[j] = x == G::S - 1;
        lb[j] = kLds0 + (uint32_t)(kg * G::LPIX + nc + G::S - (G::S + 1)) * 16u;
        ob[j] = (uint32_t)(nc + G::S) * 16u;                            // output unit of the pixel (HALVES = 2: behind the half's first unit)
        zb[j] = zoff + (lb[j] & 255u);                                  // same banks as the lane's own unit: stays conflict-free
    }
}

// Pin the weight / bias loads' completion HERE, in front of the position loop: hipcc otherwise sinks its counted vmcnt waits to
// the first use of each fragment inside the loop, where they would also wait for the (to hipcc invisible) LDS-DMA of the
// next position that is issued at the top of every iteration.  Then wait for the first planes and meet the other waves.
template <int NS, int DEPTH>
__device__ __forceinline__ void pin_and_sync(bf16x8 (&W)[NS], float (&bias_r)[16]) {
    constexpr int kNVfit = (256 - 4 * DEPTH - kVSlack) / 4, kNVmin = NS - (256 - 64) / 4;   // fragments kept in VGPRs
    constexpr int NV = kNVfit > kNVmin ? kNVfit : kNVmin;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        // 288 [320] weight registers do not fit the 256 architectural VGPRs: the upper half is pinned into accumulator registers,
        // which the MFMA reads as its A operand directly ("+v" for all of them made hipcc park them there anyway and copy each
        // fragment back with four v_accvgpr_read before use: one VALU instruction per MFMA in the hot loop)
        if (s < NV) asm volatile("" : "+v"(W[s]));
        else asm volatile("" : "+a"(W[s]));
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(bias_r[r]));
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // first planes landed, zero region written
    __builtin_amdgcn_s_barrier();
}

// a position's read bases for the centre / left / right tap columns: its plane (LDS buffer gcur), or the zero region for lanes
// past the board and for the neighbour a row does not have
__device__ __forceinline__ void tap_bases(uint32_t gcur, const uint32_t (&lb)[4], const uint32_t (&zb)[4], const bool (&ok)[4],
                                          const bool (&edgeL)[4], const bool (&edgeR)[4], uint32_t (&bC)[4], uint32_t (&bL)[4], uint32_t (&bR)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bC[j] = !ok[j] ? zb[j] : gcur + lb[j];
        bL[j] = edgeL[j] ? zb[j] : bC[j];
        bR[j] = edgeR[j] ? zb[j] : bC[j];
    }
}

// B fragment of projection k-step cc (block-input plane, the pixel itself) ...
template <class G>
__device__ __forceinline__ bf16x8 proj_tap(const char* smem, uint32_t lbj, int cc) {
    return *reinterpret_cast<const bf16x8*>(smem + 2u * Lay<G>::kPlaneL + lbj + (uint32_t)(2 * cc * G::LPIX + G::S + 1) * 16u);
}
// ... and of tap t (0..8, row-major), cin step cc of the 3x3 convolution, from the base of the tap's column: bL / bC / bR for
// t % 3 = 0 / 1 / 2.  The caller picks the column with a conditional of its own: with that choice in here — as a select, through
// a helper or as a table indexed by t % 3 — hipcc allocates af_tower_conv<true, *> differently (504 -> 496 VGPRs at depth 8, other
// spills at 12 and 16), and this file's kernels are held to the code they had (profiles/tower_conv_shared_setup.md).
template <class G>
__device__ __forceinline__ bf16x8 conv_tap(const char* smem, uint32_t base, int t, int cc) {
    return *reinterpret_cast<const bf16x8*>(smem + base + (uint32_t)(2 * cc * G::LPIX + (t / 3) * G::S + (t % 3)) * 16u);
}

// One convolution layer over this workgroup's (pseudo-)positions.
// HALVES = 2 and the block's second convolution, which runs in place (out = in2 = the block input x, in = the mid activation g):
// a half stages rows of x that its sibling half — in another workgroup, or in this one an iteration earlier or later — may already
// have overwritten: board row 8 for half 0, row 7 for half 1.  That is safe because x is read only through the 1x1 projection, at the
// half's OWN pixels (proj_tap: the centre unit of rows it computes and nobody else writes); the 3x3 window, which does reach the
// neighbouring row, reads g, which this launch does not write.  The sibling's row is staged and never multiplied.
template <class G, bool PROJ, int DEPTH>
__device__ __forceinline__ void tower_layer(const TowerArgs& A, char* smem) {
    constexpr int NS = PROJ ? 80 : 72;
    const int lane = threadIdx.x & 63, kg = lane >> 5, nn = lane & 31;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem + kLds0;
    using L = Lay<G>;
    const int npos = G::HALVES == 1 ? A.batch : G::HALVES * A.batch;    // pseudo-positions: board pos >> 1, half pos & 1
    int pos = first_position();
    if (pos >= npos) return;
    stage_first<G, PROJ>(A, smem, lds0, wv, pos);
    bf16x8 W[NS];
    float bias_r[16];
    load_weights(A, wv, lane, kg, W, bias_r);
    uint32_t lb[4], ob[4], zb[4];
    bool ok[4], edgeL[4], edgeR[4];
    pixel_bases<G>(L::zero_off(PROJ), kg, nn, lb, ob, zb, ok, edgeL, edgeR);
    pin_and_sync<NS, DEPTH>(W, bias_r);

#ifdef AF_TOWER_TIMING
    unsigned long long tacc[5] = {0, 0, 0, 0, 0};
#endif
    for (int it = 0; pos < npos; pos += gridDim.x, ++it) {
        const uint32_t gcur = (it & 1) ? L::kPlaneL : 0u, gnxt = L::kPlaneL - gcur;
        const int nxt = pos + (int)gridDim.x;
        const bool more = nxt < npos && !(A.abl & 1);
        uint32_t bC[4], bL[4], bR[4];
        bool okh[4];                                                    // HALVES = 2: the lane's pixel exists in THIS half
        if constexpr (G::HALVES == 1) {
            tap_bases(gcur, lb, zb, ok, edgeL, edgeR, bC, bL, bR);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) okh[j] = ok[j] && (!(pos & 1) || 32 * j + nn < G::HPIX1);
            tap_bases(gcur, lb, zb, okh, edgeL, edgeR, bC, bL, bR);
        }
        auto live = [&](int j) -> bool { if constexpr (G::HALVES == 1) return ok[j]; else return okh[j]; };
        TT(t0);
        f32x16 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
        // MFMA i of the position: pixel tile j = i % 4 of k-step i / 4; PROJ runs its 8 projection steps (block-input
        // plane) first.  B fragments ride a DEPTH-deep register ring: the ds_read_b128 of MFMA i + DEPTH is issued
        // right after MFMA i, so an LDS read has DEPTH MFMAs (32 cycles each) to land.
        constexpr int NM = NS * 4, NPJ = PROJ ? 32 : 0;
        auto rd = [&](int i) -> bf16x8 {
            const int j = i & 3;
            if (i < NPJ) return proj_tap<G>(smem, lb[j], i >> 2);
            const int s_ = (i - NPJ) >> 2, t = s_ >> 3;
            return conv_tap<G>(smem, t % 3 == 0 ? bL[j] : (t % 3 == 2 ? bR[j] : bC[j]), t, s_ & 7);
        };
        bf16x8 ring[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) ring[i] = rd(i);
#pragma clang loop unroll(full)
        for (int i = 0; i < NM; ++i) {
            const int ws = i < NPJ ? 72 + (i >> 2) : (i - NPJ) >> 2;
            acc[i & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W[ws], ring[i % DEPTH], acc[i & 3], 0, 0, 0);
            // (no run-time condition here: a profiling bit tested at this point cost a branch and four register moves per MFMA,
            // r2 -> r3_37; the "no LDS reads" ablation is the build-time macro AF_TOWER_ABL_NOLDS)
            if (i + DEPTH < NM && !AF_TOWER_ABL_NOLDS) ring[i % DEPTH] = rd(i + DEPTH);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
            // the next position's planes are requested one 4 KB piece every 16 MFMAs (an LDS-DMA costs ~5 issue slots:
            // in one burst they would stall the matrix pipe for the whole burst)
            if (i % 16 == 0 && i / 16 < L::kRounds && more) stage_round<G>(lds0, wv, A.in, nxt, gnxt, i / 16);
            if (PROJ && i >= NPJ && i % 16 == 8 && (i - NPJ) / 16 < L::kRounds && more) stage_round<G>(lds0, wv, A.in2, nxt, 2u * L::kPlaneL, (i - NPJ) / 16);
            if (PROJ && i == NPJ - 1) {
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();                    // every wave is done with the projection plane
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        TT(t1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // the next position's planes have landed ...
        TT(t2);
        __builtin_amdgcn_s_barrier();                                   // ... for every wave, and all are done with this one
        TT(t3);
        // epilogue: bias, ELU, bf16, store.  The weight rows are packed so that a lane's 16 accumulator rows are the 16
        // consecutive couts 32*wave + 16*kg + r: two whole 8-channel units = two 16-byte stores per pixel tile, and the
        // 32 lanes of a k half cover 512 contiguous bytes.
        // (HALVES = 2: the board's full plane, from the half's first unit on — pixel (y, x) lands at unit S * (y + 1) + x)
        char* const o = G::HALVES == 1 ? A.out + (size_t)pos * L::kPlaneB
                                       : A.out + (size_t)(pos >> 1) * L::kPlaneB + (uint32_t)((pos & 1) * G::HOFF) * 16u;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                bf16x8 v;
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const f32x2 y = elu2(f32x2{acc[j][8 * hf + e], acc[j][8 * hf + e + 1]} + f32x2{bias_r[8 * hf + e], bias_r[8 * hf + e + 1]});
                    v[e] = (__bf16)y.x; v[e + 1] = (__bf16)y.y;
                }
                if (live(j) && !(A.abl & 2)) *reinterpret_cast<bf16x8*>(o + (uint32_t)((4 * wv + 2 * kg + hf) * G::PIX) * 16u + ob[j]) = v;
            }
#ifdef AF_TOWER_TIMING
        { TT(t4); tacc[0] += t1 - t0; tacc[1] += t2 - t1; tacc[2] += t3 - t2; tacc[3] += t4 - t3; tacc[4] += 1; }
#endif
    }
#ifdef AF_TOWER_TIMING
    if (lane == 0 && blockIdx.x < 256) for (int q = 0; q < 5; ++q) g_tower_cyc[PROJ ? 1 : 0][blockIdx.x][wv][q] = tacc[q];
#endif
}

template <class G, bool PROJ, int DEPTH>
__global__ __launch_bounds__(256, 1) void af_tower_conv(TowerArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];         // [256 B][g0][g1]([h])
    tower_layer<G, PROJ, DEPTH>(A, smem);
}

// (r4 A/B record, removed from the source in r6: the whole tower as ONE launch — af_tower_persist, a workgroup keeping its 32 positions
//  from layer to layer with no grid barrier — was bit-identical and bought nothing: 4.217 vs 4.198 ms per 8192-position pass,
//  profiles/r4_36; 98 % of a position's MFMA loop already runs at the MFMA issue rate and the late workgroups are the same in every layer)

// ---------------------------------------------------------------------------------------------------------------
// af_tower_conv3<PROJ, DEPTH> (r4): af_tower_conv with its epilogue taken off the critical path.  In af_tower_conv a position is
// 288 [320] MFMAs over FOUR live accumulator sets (pixel tile = MFMA index mod 4) followed by ~300 VALU instructions of bias / ELU /
// bf16 / stores during which the matrix pipe idles (one wave per SIMD: nobody else can use it) — 0.65 of 4.2 ms per tower pass.
// Here the position runs as two PHASES of two pixel tiles each (tiles 0,1 then tiles 2,3: 144 [160] MFMAs per phase, still alternating
// accumulators), and the finished pair's epilogue is issued in 48 small pieces (a third of a two-element chunk: 3-5 VALU) inside the OTHER pair's MFMA
// stream — pair A's under phase B of the same position, pair B's under phase A of the next one — where a wave's VALU work costs a
// fraction of its serial price (tools/probes/mfma_valu_coissue.hip: 4 VALU per MFMA add ~7 cycles to its 32).  Live accumulators:
// the accumulating pair + the pair in its epilogue = the same 64 registers as before.
// PROJ: the 16 projection MFMAs of a phase sit at the END of phase A and at the START of phase B, so the single-buffered block-input
// plane is needed for one 32-MFMA window in the middle of a position and the next position's copy of it streams in behind that
// window (9 pieces, one every 16 MFMAs) with 144 MFMAs to land.  Same MFMAs on the same operands in the same per-accumulator order
// as af_tower_conv (k-steps ascending per tile; PROJ: projection steps last for tiles 0,1 and first for tiles 2,3 — af_tower_conv
// runs them first for all four), so tiles 2,3 of the PROJ layers and every tile of the others are bit-identical to af_tower_conv.
// One position per iteration: instantiated for the geometries with HALVES = 1 only (a 15x15 handle runs af_tower_conv for both).
template <class G, bool PROJ, int DEPTH>
__global__ __launch_bounds__(256, 1) void af_tower_conv3(TowerArgs A) {
    static_assert(G::HALVES == 1, "af_tower_conv3 walks whole positions");
    constexpr uint32_t kPlaneB = Lay<G>::kPlaneB;
    constexpr int kPIX = G::PIX, kRounds = Lay<G>::kRounds;
    extern __shared__ __attribute__((aligned(16))) char smem[];         // [256 B][g0][g1]([h])
    constexpr int NS = PROJ ? 80 : 72;
    const int lane = threadIdx.x & 63, kg = lane >> 5, nn = lane & 31;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem + kLds0;
    int pos = first_position();
    if (pos >= A.batch) return;
    stage_first<G, PROJ>(A, smem, lds0, wv, pos);
    bf16x8 W[NS];
    float bias_r[16];
    load_weights(A, wv, lane, kg, W, bias_r);
    uint32_t lb[4], ob[4], zb[4];
    bool ok[4], edgeL[4], edgeR[4];
    pixel_bases<G>(Lay<G>::zero_off(PROJ), kg, nn, lb, ob, zb, ok, edgeL, edgeR);
    pin_and_sync<NS, DEPTH>(W, bias_r);

    // MFMA m of a position -> (pixel tile j, projection step?, k-step index): phase A = m < NH (tiles 0,1), phase B = tiles 2,3
    constexpr int NM = NS * 4, NH = NM / 2, NP = PROJ ? 16 : 0;          // per phase: NH MFMAs of which NP are projection steps
    struct MI { int j, proj, s; };
    auto mi = [](int m) constexpr -> MI {
        constexpr int NM_ = (PROJ ? 80 : 72) * 4, NH_ = NM_ / 2, NP_ = PROJ ? 16 : 0;
        const int ph = m >= NH_, q = m - ph * NH_, j = 2 * ph + (q & 1);
        // phase A: 144 3x3 steps then NP projection steps; phase B: NP projection steps then 144 3x3 steps
        const bool proj = ph ? q < NP_ : q >= NH_ - NP_;
        const int s = proj ? (ph ? q : q - (NH_ - NP_)) >> 1 : (ph ? q - NP_ : q) >> 1;
        return MI{j, proj ? 1 : 0, s};
    };
    f32x16 acc[4];
    const f32x16 kZero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    char* o_prev = nullptr;

    // epilogue of pixel-tile pair jp0 as 16 chunks (tile jp0 + (c >> 3), elements 2*(c & 7), +1) of kEpiK = 8 stages of TWO
    // single-issue VALU instructions each — accumulator read + bias, twice | scale + exp2 + clamp, twice | - 1 + max, twice | bf16 |
    // a 16-byte store after every fourth chunk — so that one stage fits the shadow of one MFMA; stage k of chunk c is issued behind
    // MFMA 8c + k + 3 of the other pair's phase (128 of its 144 [160]), fenced so that hipcc keeps it there (unfenced it gathers four
    // chunks in front of their store and reads a whole accumulator set in one burst).  The accumulators are read where they are used:
    // left to itself hipcc copies the whole finished set out of the accumulator registers in one burst at the top of the phase.
    // (r4 A/B record, removed from the source: the same epilogue as 16 chunks x 3 stages of 3-5 VALU on 2-vectors — v_pk_add_f32 /
    //  v_pk_mul_f32 — one stage every second MFMA.  A packed fp32 instruction beside an MFMA costs ~+22-26 cycles of a 32-cycle gap
    //  (MI355X_MICROARCH.md, "price of one filler beside MFMAs"), i.e. 48 stages x ~20 cycles per phase gave back what hiding the
    //  epilogue had won (254.5 vs 258.3 us per layer), which is why r5 made the stages scalar.)  Plain v_add / v_mul / v_exp / v_max /
    // v_cvt_pk_bf16 fillers are hidden up to ~5 per gap.  The opaque asm("" : "+v") after each result keeps hipcc's SLP vectoriser
    // from re-packing the two elements of a chunk.
    bf16x8 vst;
    float e0_[16], e1_[16], t0_[16], t1_[16];
    auto epi_stage = [&](int jp0, int c, int k, char* o) {
        const int j = jp0 + (c >> 3), q = c & 7, hf = q >> 2, e = 2 * (q & 3);
#define AF_OPAQUE(x) asm volatile("" : "+v"(x))
        if (k == 0) {
            float a0;
            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(a0) : "a"(acc[j][8 * hf + e]));
            e0_[c] = a0 + bias_r[8 * hf + e]; AF_OPAQUE(e0_[c]);
        } else if (k == 1) {
            float a1;
            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(a1) : "a"(acc[j][8 * hf + e + 1]));
            e1_[c] = a1 + bias_r[8 * hf + e + 1]; AF_OPAQUE(e1_[c]);
        } else if (k == 2) {
            float t = e0_[c] * 1.44269504088896341f; AF_OPAQUE(t);
            t0_[c] = fminf(fmaxf(__builtin_amdgcn_exp2f(t), 0.0f), 1.0f); AF_OPAQUE(t0_[c]);
        } else if (k == 3) {
            float t = e1_[c] * 1.44269504088896341f; AF_OPAQUE(t);
            t1_[c] = fminf(fmaxf(__builtin_amdgcn_exp2f(t), 0.0f), 1.0f); AF_OPAQUE(t1_[c]);
        } else if (k == 4) {
            // (v_max_f32 by hand: fmaxf() comes with a canonicalising v_max x, x, x of each input in IEEE mode — three instructions)
            const float m = t0_[c] - 1.0f;
            asm volatile("v_max_f32 %0, %1, %2" : "=v"(e0_[c]) : "v"(e0_[c]), "v"(m));
        } else if (k == 5) {
            const float m = t1_[c] - 1.0f;
            asm volatile("v_max_f32 %0, %1, %2" : "=v"(e1_[c]) : "v"(e1_[c]), "v"(m));
        } else if (k == 6) {
            vst[e] = (__bf16)e0_[c]; vst[e + 1] = (__bf16)e1_[c];
        } else if ((q & 3) == 3) {
            char* dst = o + (uint32_t)((4 * wv + 2 * kg + hf) * kPIX) * 16u + ob[j];
            if (j == 3) dst = ok[3] ? dst : A.dump + threadIdx.x * 16u;            // (only tile 3 has lanes past the board)
            *reinterpret_cast<bf16x8*>(dst) = vst;
        }
#undef AF_OPAQUE
    };
    constexpr int kEpiK = 8;                                             // stages per chunk
    constexpr int kEpiStride = 1;                                        // one stage every kEpiStride MFMAs, from the 4th of a phase on

    auto position = [&](auto first_tag, int it, int pos_) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const uint32_t gcur = (it & 1) ? kPlaneB : 0u, gnxt = kPlaneB - gcur;
        const int nxt = pos_ + (int)gridDim.x;
        const bool more = nxt < A.batch && !(A.abl & 1);
        char* const o = A.out + (size_t)pos_ * kPlaneB;
        uint32_t bC[4], bL[4], bR[4];
        tap_bases(gcur, lb, zb, ok, edgeL, edgeR, bC, bL, bR);
        auto rd = [&](int m) -> bf16x8 {
            const MI x = mi(m);
            if (x.proj) return proj_tap<G>(smem, lb[x.j], x.s);
            const int t = x.s >> 3;
            return conv_tap<G>(smem, t % 3 == 0 ? bL[x.j] : (t % 3 == 2 ? bR[x.j] : bC[x.j]), t, x.s & 7);
        };
        bf16x8 ring[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) ring[i] = rd(i);
#pragma clang loop unroll(full)
        for (int m = 0; m < NM; ++m) {
            const MI x = mi(m);
            const int ws = x.proj ? 72 + x.s : x.s;
            // the first MFMA of a tile starts from zero: the accumulator is not cleared while the pair is still in its epilogue
            // (srcC = the constant 0: the accumulator registers are not touched before this MFMA writes them)
            const bool fresh = (m < NH ? m : m - NH) < 2;
            if (fresh) acc[x.j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W[ws], ring[m % DEPTH], kZero16, 0, 0, 0);
            else acc[x.j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W[ws], ring[m % DEPTH], acc[x.j], 0, 0, 0);
            if (m + DEPTH < NM && !AF_TOWER_ABL_NOLDS) ring[m % DEPTH] = rd(m + DEPTH);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
            // the other pair's epilogue, one chunk every 8 MFMAs from the 5th on (16 chunks inside the phase's first 132 MFMAs)
            {
                const int q = m < NH ? m : m - NH;
                if (q >= 3 && (q - 3) % kEpiStride == 0 && (q - 3) / kEpiStride < 16 * kEpiK && (m >= NH || !FIRST)) {
                    const int st_ = (q - 3) / kEpiStride;
                    __builtin_amdgcn_sched_barrier(0);
                    if (m >= NH) epi_stage(0, st_ / kEpiK, st_ % kEpiK, o);        // pair A of this position, under phase B
                    else epi_stage(2, st_ / kEpiK, st_ % kEpiK, o_prev);           // pair B of the previous position, under phase A
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // the next position's planes: one 4 KB piece every 16 MFMAs from the start of the position
            if (m % 16 == 0 && m / 16 < kRounds && more) stage_round<G>(lds0, wv, A.in, nxt, gnxt, m / 16);
            if (PROJ) {
                constexpr int kAfter = NH + NP;                  // first MFMA after the projection window
                if (m == kAfter - 1) {
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();                // every wave is done with the block-input plane
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (m >= kAfter && (m - kAfter) % 16 == 8 && (m - kAfter) / 16 < kRounds && more)
                    stage_round<G>(lds0, wv, A.in2, nxt, 2u * kPlaneB, (m - kAfter) / 16);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // the next position's planes have landed ...
        __builtin_amdgcn_s_barrier();                                   // ... for every wave, and all are done with this one
        o_prev = o;
    };

    position(std::true_type{}, 0, pos);
    pos += gridDim.x;
    for (int it = 1; pos < A.batch; pos += gridDim.x, ++it) position(std::false_type{}, it, pos);
    // the last position's second pair
#pragma unroll
    for (int c = 0; c < 16; ++c)
#pragma unroll
        for (int k = 0; k < kEpiK; ++k) epi_stage(2, c, k, o_prev);
}

// ---------------------------------------------------------------------------------------------------------------
// af_tower_conv_small<G, PROJ>: the same convolution for a handful of positions (af_tower_forward_small).  The two kernels above
// are weight-stationary: a workgroup loads its 295 / 328 KB of A fragments before its first MFMA and then walks positions, which at
// batch 1 is one workgroup on one CU doing 288 / 320 MFMAs per wave behind that load.  Here the work is split the other way:
//   - one workgroup per (pseudo-position, pixel tile): grid = batch * HALVES * 4, workgroup b = tile b & 3 of pseudo-position b >> 2;
//     its 4 waves are the 4 cout tiles of 32, as above;
//   - the workgroup stages its pseudo-position's plane (PROJ: and the block-input plane) once, single-buffered, into the same LDS
//     layout with the same stage_first / stage_round, so proj_tap / conv_tap and the edge / zero-region bases are the ones above;
//   - a wave runs its ONE pixel tile's 72 / 80 MFMAs into ONE accumulator, in tower_layer's per-accumulator order (PROJ: projection
//     steps 0..7, then tap 0..8 major, cin step 0..7 minor) — a single chain of v_mfma_f32_32x32x16_bf16 issues at the MFMA rate;
//   - the A fragments are not resident: fragment i of that order streams from the packed buffer (the very stream load_weights
//     reads) through a ring of kSmallA register sets, its load issued kSmallA MFMAs before its use, so the first MFMA waits for the
//     planes and ONE fragment, not for all of them.  The prefill is issued behind the staging loads and in front of the wait, which
//     counts them out: loads return in order, so vmcnt(kSmallA) means every LDS-DMA piece has landed;
//   - the epilogue is tower_layer's for that tile: elu2(acc + bias), bf16, the same two 16-byte stores at the same addresses, for
//     the lanes whose pixel exists in this (half-)board.
// Same MFMAs on the same operands in the same order, the same epilogue arithmetic: bit-identical to af_tower_conv (and, where that
// is, to af_tower_conv3).  Workgroups are independent: no hand-over, no waiting on each other, no atomics.
// The block's second convolution runs in place (out = in2 = x), and the four tile workgroups of a position (times two halves) run
// concurrently, so a workgroup may stage units of x that a sibling has already overwritten.  This is the situation argued above
// tower_layer for the two halves, one level finer: x is read only through the 1x1 projection at the lane's OWN pixel (proj_tap: the
// centre unit of a pixel this workgroup computes and nobody else writes); the 3x3 window reads g, which this launch does not
// write.  A lane whose pixel does not exist reads another tile's unit (pixel 0's, or a row of the other half): whatever it finds,
// its result is never stored.
constexpr int kSmallA = 32;      // A-fragment ring: 32 KB per wave in flight (a CU's share of the bandwidth x the latency of a miss)
constexpr int kSmallB = 8;       // B-fragment ring, as af_tower_conv's at depth 8
template <class G, bool PROJ>
__global__ __launch_bounds__(256) void af_tower_conv_small(TowerArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];         // [256 B][g][-]([h])[zero region]: Lay<G>'s, one plane unused
    constexpr int NS = PROJ ? 80 : 72, NPJ = PROJ ? 8 : 0;
    static_assert(kSmallA <= 63 && kSmallA <= NS, "the ring's prefill is counted on vmcnt");
    using L = Lay<G>;
    const int lane = threadIdx.x & 63, kg = lane >> 5, nn = lane & 31;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem + kLds0;
    const int pos = (int)(blockIdx.x >> 2), j = (int)(blockIdx.x & 3);  // pseudo-position (< batch * HALVES by the grid), pixel tile
    stage_first<G, PROJ>(A, smem, lds0, wv, pos);
    // A fragment of MFMA i: the projection's (72..79 of the stream) first
    const uint4* wp = A.w + ((size_t)wv * NS * 64 + lane);
    auto frag = [&](int i) -> bf16x8 {
        const uint4 v = wp[(i < NPJ ? 72 + i : i - NPJ) * 64];
        bf16x8 f;
        __builtin_memcpy(&f, &v, 16);
        return f;
    };
    bf16x8 ra[kSmallA];
#pragma unroll
    for (int i = 0; i < kSmallA; ++i) ra[i] = frag(i);
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(kSmallA) : "memory");    // planes landed, zero region written
    __builtin_amdgcn_s_barrier();
    float bias_r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bias_r[r] = A.bias[32 * wv + 16 * kg + r];
    // the lane's pixel of tile j: pixel_bases and tap_bases for that one tile
    const int n = 32 * j + nn;
    const bool ok = n < G::HPIX0;
    const int nc = ok ? n : 0;
    const bool live = ok && (G::HALVES == 1 || !(pos & 1) || n < G::HPIX1);
    const int px = nc % G::S;
    const uint32_t lb = kLds0 + (uint32_t)(kg * G::LPIX + nc + G::S - (G::S + 1)) * 16u;
    const uint32_t ob = (uint32_t)(nc + G::S) * 16u;
    const uint32_t zb = L::zero_off(PROJ) + (lb & 255u);
    const uint32_t bC = !live ? zb : lb, bL = px == 0 ? zb : bC, bR = px == G::S - 1 ? zb : bC;
    auto rd = [&](int i) -> bf16x8 {
        if (i < NPJ) return proj_tap<G>(smem, lb, i);
        const int s_ = i - NPJ, t = s_ >> 3;
        return conv_tap<G>(smem, t % 3 == 0 ? bL : (t % 3 == 2 ? bR : bC), t, s_ & 7);
    };
    bf16x8 rb[kSmallB];
#pragma unroll
    for (int i = 0; i < kSmallB; ++i) rb[i] = rd(i);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    __builtin_amdgcn_sched_barrier(0);                       // the ring's first reads stay in front: the groups below would take them one by one
#pragma clang loop unroll(full)
    for (int i = 0; i < NS; ++i) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[i % kSmallA], rb[i % kSmallB], acc, 0, 0, 0);
        if (i + kSmallB < NS) rb[i % kSmallB] = rd(i + kSmallB);
        if (i + kSmallA < NS) ra[i % kSmallA] = frag(i + kSmallA);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
    }
    char* const o = G::HALVES == 1 ? A.out + (size_t)pos * L::kPlaneB
                                   : A.out + (size_t)(pos >> 1) * L::kPlaneB + (uint32_t)((pos & 1) * G::HOFF) * 16u;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            const f32x2 y = elu2(f32x2{acc[8 * hf + e], acc[8 * hf + e + 1]} + f32x2{bias_r[8 * hf + e], bias_r[8 * hf + e + 1]});
            v[e] = (__bf16)y.x; v[e + 1] = (__bf16)y.y;
        }
        if (live) *reinterpret_cast<bf16x8*>(o + (uint32_t)((4 * wv + 2 * kg + hf) * G::PIX) * 16u + ob) = v;
    }
}

// (r2 A/B record, removed from the source in r6: af_tower_conv2, the same convolution on af_conv_f16s.hip's slab-ring structure —
//  5.37 ms per tower pass against 4.2: its 32-channel slabs give a wave only 36 MFMAs between barriers)

// ---------------------------------------------------------------------------------------------------------------
// af_tower_stem: the 5x5 stem (3 -> 128, SAME) + bias + ELU, planes fp32 [B][3][S][S] -> C8 bf16, on the same MFMA.
// K = 3 planes x 5 rows x (5 taps padded to 8) = 15 groups of 8 = 8 k-steps; a B fragment (pixel n, group (cin, ky))
// is the 8-wide input window starting at column x-2 of row y+ky-2, pre-expanded into LDS once per position as
// 3 x (S + 4) x S entries of 8 bf16 ("im2row"), so it is one aligned ds_read_b128.  Weights (8 A fragments) stay in
// registers; workgroups are persistent over positions.
struct StemArgs {
    const float* planes;
    const uint4* w;      // [4 waves][8][64] A fragments
    const float* bias;   // [128]
    char* out;           // C8 bf16
    int batch;
};

// Geometry: the image has rows -2..S+1 (SR = S + 4) of IW = S + 5 columns (-2..S+2), an entry row per image row; a wave runs all
// NT pixel tiles of the position (4 / 8 accumulator sets — 8 weight fragments leave room), a thread loads NL = 2 / 3 of the
// position's 3 * NPIX plane values.
template <class G>
__global__ __launch_bounds__(256) void af_tower_stem_kernel(StemArgs A) {
    constexpr int kS = G::S, kNPIX = G::NPIX, kPIX = G::PIX, NT = G::NT, SR = G::S + 4, IW = G::S + 5, NL = (3 * G::NPIX + 255) / 256;
    constexpr uint32_t kPlaneB = Lay<G>::kPlaneB;
    static_assert(3 * G::NPIX > 256 && NL <= 3, "plane values per thread");
    __shared__ __attribute__((aligned(16))) uint4 ent[3 * SR * kS + 1];      // entry (cin, yy, x) = window x-2..x+5 of row yy-2
    const int lane = threadIdx.x & 63, kg = lane >> 5, nn = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    bf16x8 W[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const uint4 v = A.w[((size_t)wv * 8 + s) * 64 + lane];
        __builtin_memcpy(&W[s], &v, 16);
    }
    float bias_r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bias_r[r] = A.bias[32 * wv + 16 * kg + r];
    uint32_t lb[NT], ob[NT];
    bool ok[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = 32 * j + nn;
        ok[j] = n < kNPIX;
        const int nc = ok[j] ? n : 0;
        lb[j] = (uint32_t)nc;                                            // entry index of (cin 0, yy = y, x)
        ob[j] = (uint32_t)(nc + kS) * 16u;
    }
    // r3 (as in af_stem_mfma_f16s): the planes go through a zero-bordered bf16 image in LDS (rows -2..S+1, columns -2..S+2) filled from
    // registers loaded one position ahead; the im2row entries are built from it instead of five scattered global loads each
    __shared__ __bf16 img[3 * SR * IW];
    for (int i = threadIdx.x; i < 3 * SR * IW; i += 256) img[i] = (__bf16)0.0f;
    auto img_at = [](int i) -> int { const int c = i / kNPIX, p = i - c * kNPIX, y = p / kS, x = p - y * kS; return (c * SR + y + 2) * IW + x + 2; };
    int tq[NL], aq[NL];
    bool hq[NL];
    float nx[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        tq[q] = (int)threadIdx.x + 256 * q;
        hq[q] = q == 0 || tq[q] < 3 * kNPIX;                             // (3 * NPIX > 256: every thread has a first value)
        aq[q] = img_at(hq[q] ? tq[q] : 0);
        nx[q] = 0.0f;
    }
    if ((int)blockIdx.x < A.batch) {
        const float* pl = A.planes + (size_t)blockIdx.x * 3 * kNPIX;
#pragma unroll
        for (int q = 0; q < NL; ++q) if (q == 0 || hq[q]) nx[q] = pl[tq[q]];
    }
    for (int pos = blockIdx.x; pos < A.batch; pos += gridDim.x) {
        __syncthreads();                                                 // the previous position's reads are done
#pragma unroll
        for (int q = 0; q < NL; ++q) if (q == 0 || hq[q]) img[aq[q]] = (__bf16)nx[q];
        if (pos + (int)gridDim.x < A.batch) {
            const float* pl = A.planes + (size_t)(pos + gridDim.x) * 3 * kNPIX;
#pragma unroll
            for (int q = 0; q < NL; ++q) if (q == 0 || hq[q]) nx[q] = pl[tq[q]];
        }
        __syncthreads();
        for (int en = threadIdx.x; en < 3 * SR * kS; en += 256) {
            const int cin = en / (SR * kS), rem = en - cin * SR * kS, yy = rem / kS, x = rem - yy * kS;
            const __bf16* src = img + (cin * SR + yy) * IW + x;
            const bf16x8 v = {src[0], src[1], src[2], src[3], src[4], (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f};
            __builtin_memcpy(&ent[en], &v, 16);
        }
        __syncthreads();
        f32x16 acc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            // group g = 2s + kg -> (cin, ky); g = 15 is the zero pad of K (its weights are zero: any entry will do)
            const int ga = 2 * s, gb = 2 * s + 1 < 15 ? 2 * s + 1 : 0;
            const uint32_t offa = (uint32_t)((ga / 5) * SR + ga % 5) * kS, offb = (uint32_t)((gb / 5) * SR + gb % 5) * kS;
            const uint32_t off = kg ? offb : offa;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                bf16x8 b;
                __builtin_memcpy(&b, &ent[lb[j] + off], 16);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W[s], b, acc[j], 0, 0, 0);
            }
        }
        char* const o = A.out + (size_t)pos * kPlaneB;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                bf16x8 v;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (__bf16)elu1(acc[j][8 * hf + e] + bias_r[8 * hf + e]);
                if (ok[j]) *reinterpret_cast<bf16x8*>(o + (uint32_t)((4 * wv + 2 * kg + hf) * kPIX) * 16u + ob[j]) = v;
            }
    }
}

// af_tower_heads_kernel: the two heads' 1x1 convolutions (128 -> 4 value, 128 -> 16 policy) + bias + ELU straight from the
// C8 tower output into the flattened NCHW rows the dense layers take: vin [B][4*121], pin [B][16*121] (bf16).
// 0.3 MMAC per position against 36 KB of input: HBM-bound, plain VALU (thread = pixel x half of the 20 couts, the
// weights broadcast from LDS).
struct HeadsArgs {
    const char* x;       // C8 bf16
    const float* w;      // [20][128] fp32 (bf16-rounded values): rows 0-3 value conv, 4-19 policy conv
    const float* b;      // [20]
    __bf16* vin;         // [B][484]
    __bf16* pin;         // [B][1936]
    int batch;
};

// (thread = pixel x half of the couts needs 2 * NPIX <= 256 threads: the geometries with a single half only; a 15x15 handle runs
//  the MFMA kernel below whatever tune key 4 says)
template <class G>
__global__ __launch_bounds__(256) void af_tower_heads_kernel(HeadsArgs A) {
    static_assert(2 * G::NPIX <= 256, "one thread per pixel and half of the output channels");
    constexpr int kS = G::S, kNPIX = G::NPIX, kPIX = G::PIX;
    constexpr uint32_t kPlaneB = Lay<G>::kPlaneB;
    __shared__ __attribute__((aligned(16))) float wl[20 * 128];
    __shared__ float bl[20];
    for (int i = threadIdx.x; i < 20 * 128; i += 256) wl[i] = A.w[i];
    if (threadIdx.x < 20) bl[threadIdx.x] = A.b[threadIdx.x];
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= 2 * kNPIX) return;
    const int grp = t / kNPIX, p = t - grp * kNPIX;
    for (int pos = blockIdx.x; pos < A.batch; pos += gridDim.x) {
        const char* xp = A.x + (size_t)pos * kPlaneB + (uint32_t)(p + kS) * 16u;
        float acc[10];
#pragma unroll
        for (int c = 0; c < 10; ++c) acc[c] = bl[10 * grp + c];
#pragma unroll 4
        for (int cb = 0; cb < 16; ++cb) {
            bf16x8 v;
            const uint4 raw = *reinterpret_cast<const uint4*>(xp + (size_t)cb * kPIX * 16);
            __builtin_memcpy(&v, &raw, 16);
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
#pragma unroll
            for (int c = 0; c < 10; ++c) {
                const float4 w0 = *reinterpret_cast<const float4*>(&wl[(10 * grp + c) * 128 + cb * 8]);
                const float4 w1 = *reinterpret_cast<const float4*>(&wl[(10 * grp + c) * 128 + cb * 8 + 4]);
                acc[c] += f[0] * w0.x + f[1] * w0.y + f[2] * w0.z + f[3] * w0.w + f[4] * w1.x + f[5] * w1.y + f[6] * w1.z + f[7] * w1.w;
            }
        }
#pragma unroll
        for (int c = 0; c < 10; ++c) {
            const int co = 10 * grp + c;
            const __bf16 y = (__bf16)elu1(acc[c]);
            if (co < 4) A.vin[(size_t)pos * (4 * kNPIX) + co * kNPIX + p] = y;
            else A.pin[(size_t)pos * (16 * kNPIX) + (co - 4) * kNPIX + p] = y;
        }
    }
}

// af_tower_heads_mfma_kernel (r4): the same 1x1 convolutions on the matrix cores.  The VALU kernel above re-reads its 20 x 128 weights
// from LDS for every pixel (320 16-byte LDS reads per thread) and takes 198 us per 8192 positions against a 75-us HBM bound.  Here a
// wave = one 32-pixel tile of a position: M = 32 output rows (4 value + 16 policy channels, the rest zero weights), K = 128 channels =
// 8 k-steps whose B fragment is exactly one 16-byte C8 unit per lane (8 channels of the lane's pixel: straight from global memory,
// 512 contiguous bytes per half wave), A fragments (8 x 16 bytes per lane) resident.  The weight rows are permuted at pack time like
// the tower's, so a lane holds outputs 16 kg + r: bias, ELU, bf16, 2-byte stores that are contiguous over the 32 pixels of a tile.
struct HeadsMfmaArgs {
    const char* x;       // C8 bf16
    const uint4* a;      // [8 k-steps][64 lanes] A fragments (8 bf16)
    const float* b;      // [32]: bias of output o (0 for o >= 20)
    __bf16* vin;         // [B][484]
    __bf16* pin;         // [B][1936]
    int batch;
};

// NT = 8 tiles (15x15): a workgroup is one half of a position's tiles, pseudo-position pp -> position pp >> 1, tiles 4 (pp & 1) + wave;
// the host launches an even grid there, so a workgroup keeps its half and the lane its pixel.
template <class G>
__global__ __launch_bounds__(256) void af_tower_heads_mfma_kernel(HeadsMfmaArgs A) {
    constexpr int kS = G::S, kNPIX = G::NPIX, kPIX = G::PIX, NH = G::NT / 4;     // workgroups per position
    constexpr uint32_t kPlaneB = Lay<G>::kPlaneB;
    const int lane = threadIdx.x & 63, kg = lane >> 5, nn = lane & 31;
    const int j = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (NH == 1 ? 0 : 4 * (int)(blockIdx.x & 1));       // pixel tile
    const int p = 32 * j + nn, pc = p < kNPIX ? p : 0;
    bf16x8 W[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) { const uint4 v = A.a[s * 64 + lane]; __builtin_memcpy(&W[s], &v, 16); }
    float bias_r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bias_r[r] = A.b[16 * kg + r];
    const uint32_t off = (uint32_t)(kg * kPIX + pc + kS) * 16u;                   // the lane's unit inside channel-group plane kg
    uint4 cur[8], nxt[8];
    const int npos = NH == 1 ? A.batch : NH * A.batch;
    auto board = [](int pp) -> int { return NH == 1 ? pp : pp >> 1; };
    int pp = blockIdx.x;
    if (pp >= npos) return;
#pragma unroll
    for (int s = 0; s < 8; ++s) cur[s] = *reinterpret_cast<const uint4*>(A.x + (size_t)board(pp) * kPlaneB + off + (uint32_t)(2 * s * kPIX) * 16u);
    for (; pp < npos; pp += gridDim.x) {
        const int pos = board(pp);
        const int np = board(pp + (int)gridDim.x < npos ? pp + (int)gridDim.x : pp);
#pragma unroll
        for (int s = 0; s < 8; ++s) nxt[s] = *reinterpret_cast<const uint4*>(A.x + (size_t)np * kPlaneB + off + (uint32_t)(2 * s * kPIX) * 16u);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            bf16x8 y;
            __builtin_memcpy(&y, &cur[s], 16);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W[s], y, acc, 0, 0, 0);
        }
        if (p < kNPIX) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 16 * kg + r;                                            // (kg = 1: only o = 16..19 exist)
                if (o < 20) {
                    const __bf16 yv = (__bf16)elu1(acc[r] + bias_r[r]);
                    if (o < 4) A.vin[(size_t)pos * (4 * kNPIX) + o * kNPIX + p] = yv;
                    else A.pin[(size_t)pos * (16 * kNPIX) + (o - 4) * kNPIX + p] = yv;
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) cur[s] = nxt[s];
    }
}

// af_tower_dense_kernel: the three dense layers and the softmax behind the heads' 1x1 convolutions (network.py:73-76,85-88)
// for 32 positions per workgroup on the same MFMA: D[out][position] = sum_k W^T[out][k] * in[position][k].
//   policy: 1936 -> 121 (+ bias) -> softmax: wave w owns outputs 32w..32w+31 (121 padded to 128 with zero weights), 121 k-steps
//   value : 484 -> 64 (+ bias, ELU) on waves 0 and 1 (31 k-steps, K padded to 496), then 64 -> 1 (+ bias), tanh(x/2)
// A fragments (weights) are pre-packed [k-step][out tile][lane][8] and stream from L2; a B fragment is 16 bytes of one
// position's input row per lane, read straight from global memory (consecutive k-steps reuse the same lines).
struct DenseArgs {
    const __bf16* vin;    // [B][484]
    const __bf16* pin;    // [B][1936]
    const uint4* wp;      // [121][4][64] policy A fragments
    const uint4* wv;      // [31][2][64] value fc1 A fragments
    const float* pb;      // [128] policy bias (padded with -inf-like for the 7 dead outputs)
    const float* vb1;     // [64]
    const float* vw2;     // [64]
    const float* vb2;     // [1]: a device word, not a by-value argument — a replayed graph must see the value an update wrote
    float* policy;        // fp32 [B][121]
    float* value;         // fp32 [B]
    int batch;
};

// Geometry: NPIX outputs in NT tiles of 32 (the dead ones carry zero weights and a bias of -1e30), wave w owns the TW = NT / 4 tiles
// TW w .. TW w + TW - 1, one accumulator set each, on the same B fragment; KP = 16 NPIX / 16 policy k-steps, KV value k-steps.
template <class G>
__global__ __launch_bounds__(256) void af_tower_dense_kernel(DenseArgs A) {
    constexpr int kNPIX = G::NPIX, NT = G::NT, TW = G::NT / 4, KP = G::KP, KV = G::KV, VIN = 4 * G::NPIX;
    constexpr int kPinRowB = 16 * G::NPIX * 2, kPinUnits = kPinRowB / 16;      // a policy input row: 3872 / 7200 bytes = 242 / 450 units
    __shared__ float s_red[4][2][32];         // [wave][lane half][position]: partial max / sum / dot
    constexpr int kStageBuf = 32 * 528;
    __shared__ __attribute__((aligned(16))) char s_stage[2 * kStageBuf];      // policy rows of the 32 positions, 16 k-steps at a time
    const int lane = threadIdx.x & 63, kg = lane >> 5, nn = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    typedef uint32_t u32x4d __attribute__((ext_vector_type(4)));
    for (int p0 = blockIdx.x * 32; p0 < A.batch; p0 += gridDim.x * 32) {
        const int pos = p0 + nn < A.batch ? p0 + nn : A.batch - 1;      // dead lanes of a ragged tail recompute the last position
        // ---------------- policy ----------------
        f32x16 acc[TW];
#pragma unroll
        for (int i = 0; i < TW; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
        // B operands through LDS (r4): read straight from global memory a B fragment is one 16-byte piece of a DIFFERENT position's row
        // per lane — 32 rows = 64 cache lines per load instruction; staged, 32 consecutive threads copy 512 contiguous bytes of one row
        // (chunks of 16 k-steps, double buffered, rows 528 bytes apart in LDS: an odd number of 16-byte units, conflict-free
        // ds_read_b128) and the fragment is one LDS read.  A operands (weights, L2) stay on the kRing-deep register ring.  Same k order.
        constexpr int kRing = 8, kChunks = (KP + 15) / 16;                       // 7 x 16 + 9 k-steps at 11x11, 14 x 16 + 1 at 15x15
        u32x4d stg[4];
        auto stage_load = [&](int c) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int u = 256 * i + (int)threadIdx.x, row = u >> 5, col = u & 31;
                const int prw = p0 + row < A.batch ? p0 + row : A.batch - 1;
                stg[i] = u32x4d{0u, 0u, 0u, 0u};
                if (32 * c + col < kPinUnits) stg[i] = *reinterpret_cast<const u32x4d*>(reinterpret_cast<const char*>(A.pin) + (size_t)prw * kPinRowB + (size_t)c * 512 + col * 16);
            }
        };
        auto stage_store = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int u = 256 * i + (int)threadIdx.x, row = u >> 5, col = u & 31;
                *reinterpret_cast<u32x4d*>(s_stage + buf * kStageBuf + row * 528 + col * 16) = stg[i];
            }
        };
        u32x4d ra[kRing][TW];
#pragma unroll
        for (int q = 0; q < kRing; ++q)
#pragma unroll
            for (int i = 0; i < TW; ++i) ra[q][i] = *reinterpret_cast<const u32x4d*>(A.wp + ((size_t)q * NT + TW * wv + i) * 64 + lane);
        stage_load(0);
        stage_store(0);
        __syncthreads();
        for (int c = 0; c < kChunks; ++c) {
            if (c + 1 < kChunks) stage_load(c + 1);
            const char* bb = s_stage + (c & 1) * kStageBuf + nn * 528 + kg * 16;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int k = 16 * c + q;
                if (k < KP) {
                    bf16x8 y;
                    const u32x4d yb = *reinterpret_cast<const u32x4d*>(bb + q * 32);
                    __builtin_memcpy(&y, &yb, 16);
                    const int kn = k + kRing < KP ? k + kRing : KP - 1;        // (past the end: the last step again, never used)
#pragma unroll
                    for (int i = 0; i < TW; ++i) {
                        bf16x8 x;
                        __builtin_memcpy(&x, &ra[q % kRing][i], 16);
                        ra[q % kRing][i] = *reinterpret_cast<const u32x4d*>(A.wp + ((size_t)kn * NT + TW * wv + i) * 64 + lane);
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, acc[i], 0, 0, 0);
                    }
                }
            }
            if (c + 1 < kChunks) stage_store((c + 1) & 1);
            __syncthreads();
        }
        // a lane holds the outputs 32*(TW*wv + i) + 16*kg + r of position nn (rows permuted at pack time)
        float mx = -3.0e38f;
#pragma unroll
        for (int i = 0; i < TW; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][r] += A.pb[32 * (TW * wv + i) + 16 * kg + r]; mx = acc[i][r] > mx ? acc[i][r] : mx; }
        s_red[wv][kg][nn] = mx;
        __syncthreads();
        float gmx = -3.0e38f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int h = 0; h < 2; ++h) { const float v = s_red[w][h][nn]; gmx = v > gmx ? v : gmx; }
        __syncthreads();
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < TW; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][r] = __expf(acc[i][r] - gmx); sum += acc[i][r]; }
        s_red[wv][kg][nn] = sum;
        __syncthreads();
        float gs = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int h = 0; h < 2; ++h) gs += s_red[w][h][nn];
        __syncthreads();
        const float inv = 1.0f / gs;
        if (p0 + nn < A.batch) {
#pragma unroll
            for (int i = 0; i < TW; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = 32 * (TW * wv + i) + 16 * kg + r;
                    if (o < kNPIX) A.policy[(size_t)pos * kNPIX + o] = acc[i][r] * inv;
                }
        }
        // ---------------- value ----------------
        float part = 0.0f;
        if (wv < 2) {
            f32x16 av;
#pragma unroll
            for (int r = 0; r < 16; ++r) av[r] = 0.0f;
            const __bf16* vrow = A.vin + (size_t)pos * VIN + 8 * kg;
            auto load_b = [&](int k) -> u32x4d {
                u32x4d b = {0u, 0u, 0u, 0u};
                if (16 * k + 8 * kg + 8 <= VIN) b = *reinterpret_cast<const u32x4d*>(vrow + 16 * k);
                else if (16 * k + 8 * kg < VIN) {                          // the last, partial 8-group: 484 = 30*16 + 4, 900 = 56*16 + 4
                    __bf16 t8[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) t8[e] = 16 * k + 8 * kg + e < VIN ? vrow[16 * k + e] : (__bf16)0.0f;
                    __builtin_memcpy(&b, t8, 16);
                }
                return b;
            };
            u32x4d va[kRing], vb[kRing];                                   // the same register ring as the policy loop
#pragma unroll
            for (int q = 0; q < kRing; ++q) {
                va[q] = *reinterpret_cast<const u32x4d*>(A.wv + ((size_t)q * 2 + wv) * 64 + lane);
                vb[q] = load_b(q);
            }
            for (int k0 = 0; k0 < KV; k0 += kRing) {
#pragma unroll
                for (int q = 0; q < kRing; ++q) {
                    const int k = k0 + q;
                    if (k < KV) {
                        bf16x8 x, y;
                        __builtin_memcpy(&x, &va[q], 16);
                        __builtin_memcpy(&y, &vb[q], 16);
                        const int kn = k + kRing < KV ? k + kRing : KV - 1;
                        va[q] = *reinterpret_cast<const u32x4d*>(A.wv + ((size_t)kn * 2 + wv) * 64 + lane);
                        vb[q] = load_b(kn);
                        av = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, av, 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 32 * wv + 16 * kg + r;
                part += elu1(av[r] + A.vb1[o]) * A.vw2[o];
            }
        }
        s_red[wv][kg][nn] = part;
        __syncthreads();
        if (wv == 0 && kg == 0 && p0 + nn < A.batch) {
            const float z = s_red[0][0][nn] + s_red[0][1][nn] + s_red[1][0][nn] + s_red[1][1][nn] + A.vb2[0];
            A.value[pos] = tanhf(0.5f * z);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Weight packers, the only ones: fp32 weights in device memory (OIHW convolutions, [in][out] dense layers) -> every
// weight-derived buffer of the handle, in place.  af_tower_update_device runs them over the caller's device tensors; the host
// setters (af_tower_set_block / _set_stem / _set_heads / _set_dense) copy their fp32 arrays into the handle's staging area
// and run them over that, one block or one range of the ends kernel each.  The layout is specified by oracle/tower_pack.py, a
// numpy restatement tied to the bytes of the former host packers (tests/golden/tower_packed_digests.json);
// tests/test_gpu_tower_update.py holds both paths to it buffer by buffer.  A thread owns one 16-byte fragment row (8 bf16, one
// vector store) or one fp32 word; the thread index is decoded by div / mod with compile-time region sizes, so every source and
// destination index is in range by construction for the element counts the callers have validated or staged.  No scales, no
// reductions: nothing here has to come back to the host, which is why the update is launches only.
//
// pack_bf16: round to nearest even on the bit pattern (ties both ways, carry into the exponent up to inf, denormals and -0 as
// they are; NaN keeps its sign and upper payload and gets a quiet bit).  Not a conversion instruction: the bytes are the
// specification's on every class of input.
__device__ __forceinline__ uint32_t pack_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return ((u >> 16) | 0x40u) & 0xffffu;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ __forceinline__ float pack_bf16_f32(float f) { return __uint_as_float(pack_bf16(f) << 16); }
// (pack_perm, MFMA row -> output, so that a lane's 16 accumulator rows are 16 consecutive outputs: af_tower_common.h)
__device__ __forceinline__ uint4 pack_row(const uint32_t (&h)[8]) {
    return uint4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
}

constexpr int kPackBlocks = 8;                                          // residual blocks per launch (their pointers are kernel arguments)
constexpr int kRowsW1 = 4 * 72 * 64, kRowsW2 = 4 * 80 * 64;             // fragment rows of a block's two convolutions
constexpr int kPackBlockThreads = kRowsW1 + kRowsW2 + 128 + 128;        // + b1 + b2 words: 39,168 = 153 x 256
struct PackBlocksArgs {
    const float* src[kPackBlocks][6];    // c1_w, c1_b, c2_w, c2_b, res_w, res_b
    uint4* w1[kPackBlocks];
    uint4* w2[kPackBlocks];
    float* b1[kPackBlocks];
    float* b2[kPackBlocks];
};

// grid (153, blocks of this launch): blockIdx.y picks the residual block
__global__ __launch_bounds__(256) void af_tower_pack_blocks_kernel(PackBlocksArgs A) {
    const int b = blockIdx.y;
    int r = (int)(blockIdx.x * 256 + threadIdx.x);
    if (r < kRowsW1 + kRowsW2) {
        const bool second = r >= kRowsW1;
        const int q = second ? r - kRowsW1 : r, NS = second ? 80 : 72;            // q < 4 * NS * 64
        const int lane = q & 63, s = (q >> 6) % NS, wv = (q >> 6) / NS;           // wv < 4
        const int co = 32 * wv + pack_perm(lane & 31);                            // < 128
        const int cc = s < 72 ? s % 8 : s - 72;                                   // < 8
        const int ci = 16 * cc + 8 * (lane >> 5);                                 // ci + 7 < 128
        uint32_t h[8];
        if (s < 72) {
            const float* p = A.src[b][second ? 2 : 0] + ((size_t)co * 128 + ci) * 9 + s / 8;      // tap s / 8 < 9
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = pack_bf16(p[9 * e]);
        } else {
            const float* p = A.src[b][4] + (size_t)co * 128 + ci;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = pack_bf16(p[e]);
        }
        (second ? A.w2[b] : A.w1[b])[q] = pack_row(h);
        return;
    }
    r -= kRowsW1 + kRowsW2;
    if (r < 128) { A.b1[b][r] = A.src[b][1][r]; return; }
    r -= 128;
    if (r < 128) A.b2[b][r] = A.src[b][3][r] + A.src[b][5][r];
}

// stem, the heads' 1x1 convolutions and the dense layers: the thread index r walks the regions below in order, stem in
// [0, kPackEndsStem), heads up to kPackEndsHeads, the dense layers in the rest.  A launch covers [first, end): all of it for
// af_tower_update_device, one group's range for a host setter, which leaves the other groups' pointers null (never reached).
// Stem and heads are the same for every board size; the dense regions are sized by the geometry (Ends<G>).
constexpr int kRowsStem = 4 * 8 * 64, kRowsHeadsA = 8 * 64;
constexpr int kPackEndsStem = kRowsStem + 128, kPackEndsHeads = kPackEndsStem + 20 * 128 + 20 + kRowsHeadsA + 32;
template <class G> struct Ends {
    static constexpr int kRowsWp = G::KP * G::NT * 64, kRowsWv = G::KV * 2 * 64;    // 121 x 4 / 225 x 8 policy, 31 / 57 value-fc1 fragment sets
    static constexpr int kPbWords = 32 * G::NT;                                     // policy bias, padded to whole tiles: 128 / 256
    static constexpr int kThreads = kPackEndsHeads + kRowsWp + kRowsWv + G::NPIX + 64 + 64 + 1;
    static_assert(16 * G::KP == 16 * G::NPIX && G::KVPAD == 16 * G::KV && G::KVPAD >= 4 * G::NPIX, "k-steps cover the dense layers' inputs");
};
struct PackEndsArgs {
    int first, end;
    const float *stem_w, *stem_b, *vconv_w, *vconv_b, *pconv_w, *pconv_b, *vfc1_w, *vfc1_b, *vfc2_w, *vfc2_b, *pfc_w, *pfc_b;
    uint4* o_stem_w;
    float* o_stem_b;
    float *o_heads_w, *o_heads_b;
    uint4* o_heads_a;
    float* o_heads_b32;
    uint4 *o_dense_wp, *o_dense_wv;
    float *o_dense_pb, *o_dense_vb1, *o_dense_vw2, *o_dense_vb2;
};

template <class G>
__global__ __launch_bounds__(256) void af_tower_pack_ends_kernel(PackEndsArgs A) {
    constexpr int kRowsWp = Ends<G>::kRowsWp, kRowsWv = Ends<G>::kRowsWv, kNPIX = G::NPIX, NT = G::NT;
    int r = A.first + (int)(blockIdx.x * 256 + threadIdx.x);
    if (r >= A.end) return;
    if (r < kRowsStem) {                         // [wave][k-step][lane]: group g = 2 s + (lane >> 5) = (cin, ky), 5 taps + 3 zeros; g = 15 is zero
        const int lane = r & 63, s = (r >> 6) & 7, wv = r >> 9;                   // wv < 4
        const int co = 32 * wv + pack_perm(lane & 31), g = 2 * s + (lane >> 5);
        uint32_t h[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (g < 15) {
            const float* p = A.stem_w + (((size_t)co * 3 + g / 5) * 5 + g % 5) * 5;
#pragma unroll
            for (int e = 0; e < 5; ++e) h[e] = pack_bf16(p[e]);
        }
        A.o_stem_w[r] = pack_row(h);
        return;
    }
    r -= kRowsStem;
    if (r < 128) { A.o_stem_b[r] = A.stem_b[r]; return; }
    r -= 128;
    if (r < 20 * 128) {                          // heads_w [20][128]: rows 0-3 value conv, 4-19 policy conv, bf16 values held in fp32
        const int c = r >> 7, k = r & 127;
        A.o_heads_w[r] = pack_bf16_f32(c < 4 ? A.vconv_w[c * 128 + k] : A.pconv_w[(c - 4) * 128 + k]);
        return;
    }
    r -= 20 * 128;
    if (r < 20) { A.o_heads_b[r] = r < 4 ? A.vconv_b[r] : A.pconv_b[r - 4]; return; }
    r -= 20;
    if (r < kRowsHeadsA) {                       // [k-step][lane]: output o = perm(lane & 31) (zero rows for o >= 20), channels 16 step + 8 (lane >> 5) + e
        const int lane = r & 63, step = r >> 6;                                   // step < 8
        const int o = pack_perm(lane & 31), ch = 16 * step + 8 * (lane >> 5);     // ch + 7 < 128
        uint32_t h[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (o < 20) {
            const float* p = (o < 4 ? A.vconv_w + o * 128 : A.pconv_w + (o - 4) * 128) + ch;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = pack_bf16(p[e]);
        }
        A.o_heads_a[r] = pack_row(h);
        return;
    }
    r -= kRowsHeadsA;
    if (r < 32) { A.o_heads_b32[r] = r < 4 ? A.vconv_b[r] : (r < 20 ? A.pconv_b[r - 4] : 0.0f); return; }
    r -= 32;
    if (r < kRowsWp) {                           // [k-step][out tile][lane]: pfc [16 NPIX][NPIX], outputs NPIX..32 NT - 1 are zero rows
        const int lane = r & 63, tile = (int)((uint32_t)(r >> 6) % NT), k = (int)((uint32_t)(r >> 6) / NT);       // k < KP
        const int o = 32 * tile + pack_perm(lane & 31), ki = 16 * k + 8 * (lane >> 5);    // ki + 7 < 16 NPIX
        uint32_t h[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (o < kNPIX) {
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = pack_bf16(A.pfc_w[(size_t)(ki + e) * kNPIX + o]);
        }
        A.o_dense_wp[r] = pack_row(h);
        return;
    }
    r -= kRowsWp;
    if (r < kRowsWv) {                           // [k-step][out tile][lane]: vfc1 [4 NPIX][64], K padded to KVPAD (496 / 912) with zeros
        const int lane = r & 63, tile = (r >> 6) & 1, k = r >> 7;                 // k < KV
        const int o = 32 * tile + pack_perm(lane & 31), ki = 16 * k + 8 * (lane >> 5);    // o < 64
        uint32_t h[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (ki + e < 4 * kNPIX) h[e] = pack_bf16(A.vfc1_w[(size_t)(ki + e) * 64 + o]);
        A.o_dense_wv[r] = pack_row(h);
        return;
    }
    r -= kRowsWv;
    if (r < kNPIX) { A.o_dense_pb[r] = pack_bf16_f32(A.pfc_b[r]); return; }      // (the words behind keep the -1e30 af_tower_create wrote)
    r -= kNPIX;
    if (r < 64) { A.o_dense_vb1[r] = pack_bf16_f32(A.vfc1_b[r]); return; }
    r -= 64;
    if (r < 64) { A.o_dense_vw2[r] = pack_bf16_f32(A.vfc2_w[r]); return; }
    r -= 64;
    if (r < 1) A.o_dense_vb2[0] = pack_bf16_f32(A.vfc2_b[0]);
}

// ------------------------------------------------------------------ host ------------------------------------------------------------------
// The handle's weight-derived buffers, in af_tower_debug_weights' order: the four of every block, then the twelve of the ends.
enum { kW1, kW2, kB1, kB2 };        // w1 / w2: A fragments of a block's two convolutions [wave][s][lane][e], s = 8 tap + cin / 16, then the 1x1 projection
enum { kStemW, kStemB, kHeadsW, kHeadsB, kHeadsA, kHeadsB32, kDenseWp, kDenseWv, kDensePb, kDenseVb1, kDenseVw2, kDenseVb2, kEnds };

// Dims, what the host needs of a geometry as plain numbers, filled once in af_tower_create from Geo<S> (dims_of): af_tower_common.h.
template <class G> static Dims dims_of() {
    return Dims{G::S, G::NPIX, G::PIX, G::HALVES, Ends<G>::kRowsWp, Ends<G>::kRowsWv, Ends<G>::kPbWords, Ends<G>::kThreads};
}

static int64_t buffer_bytes(int i, int blocks, const Dims& d) {
    static const int64_t kBlock[4] = {(int64_t)kRowsW1 * 16, (int64_t)kRowsW2 * 16, 128 * 4, 128 * 4};
    const int64_t kEnd[kEnds] = {(int64_t)kRowsStem * 16, 128 * 4, 20 * 128 * 4, 20 * 4, (int64_t)kRowsHeadsA * 16, 32 * 4,
                                 (int64_t)d.rows_wp * 16, (int64_t)d.rows_wv * 16, (int64_t)d.pb_words * 4, 64 * 4, 64 * 4, 4};
    return i < 4 * blocks ? kBlock[i % 4] : kEnd[i - 4 * blocks];
}

// A group is what one host setter fills: block b is group b, then stem, heads and dense.
enum { kStem, kHeads, kDense, kEndGroups };
static int group_of(int i, int blocks) {
    if (i < 4 * blocks) return i / 4;
    const int e = i - 4 * blocks;
    return blocks + (e < kHeadsW ? kStem : e < kDenseWp ? kHeads : kDense);
}

// element counts of af_tower_update_device's tensors, in its order (include/af_tower_bf16.h); a host setter takes a run of them
static int64_t update_count(int i, int blocks, const Dims& d) {
    static const int64_t kBlock[6] = {147456, 128, 147456, 128, 16384, 128};
    const int64_t C = d.npix;       // vfc1_w [4C][64], pfc_w [16C][C], pfc_b [C]: 30976 / 234256 / 121 at 11, 57600 / 810000 / 225 at 15
    const int64_t kTail[10] = {512, 4, 2048, 16, 4 * C * 64, 64, 64, 1, 16 * C * C, C};
    if (i == 0) return 9600;
    if (i == 1) return 128;
    if (i < 2 + 6 * blocks) return kBlock[(i - 2) % 6];
    return kTail[i - 2 - 6 * blocks];
}

// the staging area holds the largest setter's tensors, each rounded up to 64 floats: a block's six (1.25 MB) or — 15x15 — the dense six
static int64_t stage_floats(const Dims& d) {
    const int64_t r64 = 63, C = d.npix;
    const int64_t block = 2 * 147456 + 16384 + 3 * 128;
    const int64_t dense = ((4 * C * 64 + r64) & ~r64) + 3 * 64 + 64 + ((16 * C * C + r64) & ~r64) + ((C + r64) & ~r64);
    return block > dense ? block : dense;
}
constexpr int64_t kDumpBytes = 4096;                                // TowerArgs::dump

// (struct af_tower, the handle: af_tower_common.h)

// The one fork between the geometries: f(Geo<11>{}) or f(Geo<15>{}) (af_tower_create admits no other size).
template <class F>
static int with_geo(const af_tower* t, F&& f) { return t->S == 11 ? f(Geo<11>{}) : f(Geo<15>{}); }

static bool all_set(const af_tower* t) {
    for (char c : t->set) if (!c) return false;
    return true;
}

// blocks b0 .. b0 + nb - 1 (nb <= kPackBlocks) from src: six device tensors per block, af_tower_update_device's order
static void pack_blocks(const af_tower* t, hipStream_t st, int b0, int nb, const float* const* src) {
    PackBlocksArgs a = {};
    for (int j = 0; j < nb; ++j) {
        for (int k = 0; k < 6; ++k) a.src[j][k] = src[6 * j + k];
        a.w1[j] = t->block<uint4>(b0 + j, kW1); a.w2[j] = t->block<uint4>(b0 + j, kW2);
        a.b1[j] = t->block<float>(b0 + j, kB1); a.b2[j] = t->block<float>(b0 + j, kB2);
    }
    hipLaunchKernelGGL(af_tower_pack_blocks_kernel, dim3(kPackBlockThreads / 256, nb), dim3(256), 0, st, a);
    if (t->i8) af_tower_i8_pack(t, st, b0, nb, src);             // an int8-enabled handle: its packers follow, from the same sources
}

// range [first, end) of the ends kernel from src: stem_w, stem_b, then the ten device tensors behind the blocks in
// af_tower_update_device's order; the entries of a group the range stays out of may be null
static void pack_ends(const af_tower* t, hipStream_t st, const float* const* src, int first, int end) {
    PackEndsArgs a;
    a.first = first; a.end = end;
    a.stem_w = src[0]; a.stem_b = src[1]; a.vconv_w = src[2]; a.vconv_b = src[3]; a.pconv_w = src[4]; a.pconv_b = src[5];
    a.vfc1_w = src[6]; a.vfc1_b = src[7]; a.vfc2_w = src[8]; a.vfc2_b = src[9]; a.pfc_w = src[10]; a.pfc_b = src[11];
    a.o_stem_w = t->end<uint4>(kStemW); a.o_stem_b = t->end<float>(kStemB);
    a.o_heads_w = t->end<float>(kHeadsW); a.o_heads_b = t->end<float>(kHeadsB);
    a.o_heads_a = t->end<uint4>(kHeadsA); a.o_heads_b32 = t->end<float>(kHeadsB32);
    a.o_dense_wp = t->end<uint4>(kDenseWp); a.o_dense_wv = t->end<uint4>(kDenseWv); a.o_dense_pb = t->end<float>(kDensePb);
    a.o_dense_vb1 = t->end<float>(kDenseVb1); a.o_dense_vw2 = t->end<float>(kDenseVw2); a.o_dense_vb2 = t->end<float>(kDenseVb2);
    with_geo(t, [&](auto g) {
        hipLaunchKernelGGL(af_tower_pack_ends_kernel<decltype(g)>, dim3((end - first + 255) / 256), dim3(256), 0, st, a);
        return 0;
    });
}

// A host setter, first half: wait for the device (forwards in flight read the buffers), then copy the caller's n fp32 arrays —
// entries first .. first + n - 1 of af_tower_update_device's table, with its counts — into the staging area as they are.
// dev[k]: where array k landed (256-byte aligned).
static int stage(af_tower* t, int first, int n, const float* const* host, const float** dev) {
    TW_HIP_OK(hipSetDevice(t->device));
    TW_HIP_OK(hipDeviceSynchronize());
    int64_t at = 0;
    for (int k = 0; k < n; ++k) {
        const int64_t count = update_count(first + k, t->blocks, t->d);
        if (at + count > stage_floats(t->d)) return AF_TOWER_ERR_ARG;   // (no setter's arrays are larger than the area)
        TW_HIP_OK(hipMemcpy(t->stage + at, host[k], (size_t)count * 4, hipMemcpyHostToDevice));
        dev[k] = t->stage + at;
        at += (count + 63) & ~(int64_t)63;
    }
    return AF_TOWER_OK;
}

// ... and second half, behind the packer's launch on the null stream: when this returns the weights are in place and both the
// caller's arrays and the staging area are free again
static int packed(af_tower* t, int group) {
    TW_HIP_OK(hipGetLastError());
    TW_HIP_OK(hipDeviceSynchronize());
    t->set[group] = 1;
    return AF_TOWER_OK;
}

static int g_depth = 0;     // B-fragment ring depth (A/B knob; 0 = per-kernel default)
static int g_abl = 0;       // profiling ablations (results wrong by design)
static int g_grid = 0;      // persistent workgroups (0 = one per CU)
int af_tower_grid_override() { return g_grid; }
static int g_heads = 1;     // heads' 1x1 convolutions: 1 = af_tower_heads_mfma_kernel (r4), 0 = the VALU kernel (A/B)
static int g_engine = 3;    // 3 (default, r4): af_tower_conv3 for a block's first convolution + af_tower_conv for its second (bit-identical to 0,
                            //    4.143 vs 4.167 ms per 8192-position tower pass); 0: af_tower_conv for both; 2: af_tower_conv3 for both (its
                            //    PROJ form is slower: 4.224 ms)

// Every convolution instantiation the library launches: allocate() raises their LDS limit, pick() chooses among them.
struct ConvKernel {
    void (*fn)(TowerArgs);
    int S;                  // board side of the geometry
    bool conv3, proj;       // af_tower_conv3 or af_tower_conv; PROJ = a block's second convolution
    int depth;              // B-fragment ring
    uint32_t lds;           // dynamic LDS of a launch
};
using G11 = Geo<11>;
using G15 = Geo<15>;
constexpr ConvKernel kConv[15] = {
    {af_tower_conv<G11, false, 8>, 11, false, false, 8, Lay<G11>::lds_bytes(false)},   {af_tower_conv<G11, true, 8>, 11, false, true, 8, Lay<G11>::lds_bytes(true)},
    {af_tower_conv<G11, false, 12>, 11, false, false, 12, Lay<G11>::lds_bytes(false)}, {af_tower_conv<G11, true, 12>, 11, false, true, 12, Lay<G11>::lds_bytes(true)},
    {af_tower_conv<G11, false, 16>, 11, false, false, 16, Lay<G11>::lds_bytes(false)}, {af_tower_conv<G11, true, 16>, 11, false, true, 16, Lay<G11>::lds_bytes(true)},
    {af_tower_conv3<G11, false, 8>, 11, true, false, 8, Lay<G11>::lds_bytes(false)},   {af_tower_conv3<G11, true, 8>, 11, true, true, 8, Lay<G11>::lds_bytes(true)},
    {af_tower_conv<G15, false, 8>, 15, false, false, 8, Lay<G15>::lds_bytes(false)},   {af_tower_conv<G15, true, 8>, 15, false, true, 8, Lay<G15>::lds_bytes(true)},
    {af_tower_conv<G15, false, 12>, 15, false, false, 12, Lay<G15>::lds_bytes(false)}, {af_tower_conv<G15, true, 12>, 15, false, true, 12, Lay<G15>::lds_bytes(true)},
    {af_tower_conv<G15, false, 16>, 15, false, false, 16, Lay<G15>::lds_bytes(false)}, {af_tower_conv<G15, true, 16>, 15, false, true, 16, Lay<G15>::lds_bytes(true)},    {af_tower_conv<G15, true, 6>, 15, false, true, 6, Lay<G15>::lds_bytes(true)},
};

// The kernel of a block's first or second convolution.  Engine 3: af_tower_conv3 then af_tower_conv, engine 2: af_tower_conv3 for
// both — at depth 8 whatever key 0 says; engine 0: af_tower_conv at the depth of key 0, or by default the deepest ring that hipcc
// allocates without scratch, 12 / 8 (a scratch reload's vmcnt(0) would also wait for the LDS-DMA of the next position: measured
// 400 vs 230 us per launch).
// 15x15: af_tower_conv for both convolutions whatever the engine (af_tower_conv3 walks whole positions), at the depth of key 0 or,
// by the same rule, 12 / 6: the gather addresses of the staging rounds cost the PROJ form the registers of a fourth of its ring
// (depth 8: 36 bytes of scratch; depth 6: none).
static const ConvKernel* pick(int S, int engine, bool second, int depth) {
    if (S != 11) engine = 0;
    const bool conv3 = engine == 2 || (engine == 3 && !second);
    const int d = engine != 0 ? 8 : depth ? depth : !second ? 12 : S == 11 ? 8 : 6;
    for (const ConvKernel& k : kConv)
        if (k.S == S && k.conv3 == conv3 && k.proj == second && k.depth == d) return &k;
    return nullptr;         // (not reached with the values af_tower_tune accepts)
}

// af_tower_forward_small's kernels: one per geometry and convolution of a block, in Lay<G>'s LDS layout.
struct SmallKernel {
    void (*fn)(TowerArgs);
    int S;
    bool proj;
    uint32_t lds;
};
constexpr SmallKernel kSmall[4] = {
    {af_tower_conv_small<G11, false>, 11, false, Lay<G11>::lds_bytes(false)}, {af_tower_conv_small<G11, true>, 11, true, Lay<G11>::lds_bytes(true)},
    {af_tower_conv_small<G15, false>, 15, false, Lay<G15>::lds_bytes(false)}, {af_tower_conv_small<G15, true>, 15, true, Lay<G15>::lds_bytes(true)},
};
// af_tower_small_batch: the largest batch up to which the whole forward was measured faster on af_tower_forward_small than on
// af_tower_forward, per board size (profiles/tower_small_batch.md: medians apart by more than both forms' min..max spread; measured
// at 1, 2, 4, ... 256: at 11x11 the small form wins by 45 us of 211 at 64 and loses at 128, at 15x15 it wins by 37 of 245 at 32 and
// loses at 64 — where its grid passes one workgroup per CU)
constexpr int32_t kSmallBatch11 = 64, kSmallBatch15 = 32;

static TowerArgs layer_args(const af_tower* t, int b, bool second, void* x, void* g, int batch) {
    TowerArgs a;
    a.in = static_cast<const char*>(second ? g : x);
    a.in2 = second ? static_cast<const char*>(x) : nullptr;
    a.w = t->block<uint4>(b, second ? kW2 : kW1);
    a.bias = t->block<float>(b, second ? kB2 : kB1);
    a.out = static_cast<char*>(second ? x : g);
    a.batch = batch; a.abl = g_abl; a.dump = t->dump;
    return a;
}

// One layer on the persistent kernels: what af_tower_forward is a loop over, and the hook of af_tower_i8.hip's device calibration.
int af_tower_launch_layer(af_tower* t, hipStream_t st, int b, bool second, void* x_dev, void* g_dev, int batch) {
    if (!t->set[b]) return AF_TOWER_ERR_STATE;
    const int ncu = g_grid > 0 ? g_grid : t->ncu;
    const int64_t units = (int64_t)batch * t->d.halves;      // what the persistent loop walks: positions, or their halves at 15x15
    const int grid = units < ncu ? (int)units : ncu;
    const ConvKernel* k = pick(t->S, g_engine, second, g_depth);
    if (!k) return AF_TOWER_ERR_ARG;
    hipLaunchKernelGGL(k->fn, dim3(grid), dim3(256), k->lds, st, layer_args(t, b, second, x_dev, g_dev, batch));
    return AF_TOWER_OK;
}

extern "C" {

int af_tower_tune(int32_t key, int32_t value) {
    // only the values include/af_tower_bf16.h documents; a rejected call leaves the setting as it was
    if (key == 0) { if (value != 0 && value != 8 && value != 12 && value != 16) return AF_TOWER_ERR_ARG; g_depth = value; return AF_TOWER_OK; }
    if (key == 1) { if (value < 0) return AF_TOWER_ERR_ARG; g_grid = value; return AF_TOWER_OK; }
    if (key == 2) { if (value < 0 || value > 7) return AF_TOWER_ERR_ARG; g_abl = value; return AF_TOWER_OK; }
    if (key == 3) { if (value != 0 && value != 2 && value != 3) return AF_TOWER_ERR_ARG; g_engine = value; return AF_TOWER_OK; }
    if (key == 4) { if (value != 0 && value != 1) return AF_TOWER_ERR_ARG; g_heads = value; return AF_TOWER_OK; }
    return AF_TOWER_ERR_ARG;
}

const char* af_tower_strerror(int code) {
    switch (code) {
        case AF_TOWER_OK: return "ok";
        case AF_TOWER_ERR_ARG: return "bad argument";
        case AF_TOWER_ERR_HIP: return "HIP runtime error";
        case AF_TOWER_ERR_STATE: return "not every weight set has been given";
        default: return "unknown error";
    }
}

static int allocate(af_tower* t) {
    TW_HIP_OK(hipSetDevice(t->device));
    TW_HIP_OK(hipDeviceGetAttribute(&t->ncu, hipDeviceAttributeMultiprocessorCount, t->device));
    for (const ConvKernel& k : kConv)
        TW_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    for (const SmallKernel& k : kSmall)
        TW_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const int n = 4 * t->blocks + kEnds;
    auto padded = [](int64_t bytes) { return (size_t)((bytes + 255) & ~(int64_t)255); };
    const int64_t stage_bytes = stage_floats(t->d) * 4;
    size_t total = padded(stage_bytes) + padded(kDumpBytes) + af_tower_i8_arena_bytes(t);
    for (int i = 0; i < n; ++i) total += padded(buffer_bytes(i, t->blocks, t->d));
    { void* q = nullptr; TW_HIP_OK(hipMalloc(&q, total)); t->arena = static_cast<char*>(q); }
    char* p = t->arena;
    for (int i = 0; i < n; ++i) { t->buf.push_back(p); p += padded(buffer_bytes(i, t->blocks, t->d)); }
    t->stage = reinterpret_cast<float*>(p); p += padded(stage_bytes);
    t->dump = p; p += padded(kDumpBytes);
    { const int rc = af_tower_i8_carve(t, p); if (rc) return rc; }   // the int8 path's buffers: the rest of the allocation
    t->set.assign(t->blocks + kEndGroups, 0);
    // dense_pb's words behind the last pixel (121..127 / 225..255) — policy outputs that do not exist — are -1e30 for good: no packer writes them
    const std::vector<float> tail(t->d.pb_words - t->d.npix, -1.0e30f);
    TW_HIP_OK(hipMemcpy(t->end<float>(kDensePb) + t->d.npix, tail.data(), tail.size() * sizeof(float), hipMemcpyHostToDevice));
    return AF_TOWER_OK;
}

int af_tower_create(int32_t S, int32_t width, int32_t blocks, int32_t device, af_tower** out) {
    if (!out || (S != 11 && S != 15) || width != 128 || blocks < 1) return AF_TOWER_ERR_ARG;
    af_tower* t = new af_tower();
    t->S = S; t->width = width; t->blocks = blocks; t->device = device;
    with_geo(t, [&](auto g) { t->d = dims_of<decltype(g)>(); return 0; });
    const int rc = allocate(t);
    if (rc) { af_tower_destroy(t); return rc; }
    *out = t;
    return AF_TOWER_OK;
}

void af_tower_destroy(af_tower* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->arena) (void)hipFree(t->arena);
    delete t;
}

int af_tower_set_block(af_tower* t, int32_t b, const float* c1_w, const float* c1_b, const float* c2_w, const float* c2_b,
                       const float* res_w, const float* res_b) {
    if (!t || b < 0 || b >= t->blocks || !c1_w || !c1_b || !c2_w || !c2_b || !res_w || !res_b) return AF_TOWER_ERR_ARG;
    const float* const host[6] = {c1_w, c1_b, c2_w, c2_b, res_w, res_b};
    const float* dev[6];
    const int rc = stage(t, 2 + 6 * b, 6, host, dev);
    if (rc) return rc;
    pack_blocks(t, nullptr, b, 1, dev);
    return packed(t, b);
}

int af_tower_set_stem(af_tower* t, const float* w, const float* b) {
    if (!t || !w || !b) return AF_TOWER_ERR_ARG;
    const float* const host[2] = {w, b};
    const float* dev[12] = {};
    const int rc = stage(t, 0, 2, host, dev);
    if (rc) return rc;
    pack_ends(t, nullptr, dev, 0, kPackEndsStem);
    return packed(t, t->blocks + kStem);
}

int af_tower_set_heads(af_tower* t, const float* vconv_w, const float* vconv_b, const float* pconv_w, const float* pconv_b) {
    if (!t || !vconv_w || !vconv_b || !pconv_w || !pconv_b) return AF_TOWER_ERR_ARG;
    const float* const host[4] = {vconv_w, vconv_b, pconv_w, pconv_b};
    const float* dev[12] = {};
    const int rc = stage(t, 2 + 6 * t->blocks, 4, host, dev + 2);
    if (rc) return rc;
    pack_ends(t, nullptr, dev, kPackEndsStem, kPackEndsHeads);
    return packed(t, t->blocks + kHeads);
}

// dense layers (network.py:73-76,85): vfc1 [484][64] + [64], vfc2 [64] + [1], pfc [1936][121] + [121], all [in][out] fp32
int af_tower_set_dense(af_tower* t, const float* vfc1_w, const float* vfc1_b, const float* vfc2_w, const float* vfc2_b,
                       const float* pfc_w, const float* pfc_b) {
    if (!t || !vfc1_w || !vfc1_b || !vfc2_w || !vfc2_b || !pfc_w || !pfc_b) return AF_TOWER_ERR_ARG;
    const float* const host[6] = {vfc1_w, vfc1_b, vfc2_w, vfc2_b, pfc_w, pfc_b};
    const float* dev[12] = {};
    const int rc = stage(t, 2 + 6 * t->blocks + 4, 6, host, dev + 6);
    if (rc) return rc;
    pack_ends(t, nullptr, dev, kPackEndsHeads, t->d.ends_threads);
    return packed(t, t->blocks + kDense);
}

int af_tower_dense(af_tower* t, void* stream, const void* vin_dev, const void* pin_dev, float* policy_dev, float* value_dev,
                   int32_t batch) {
    if (!t || !vin_dev || !pin_dev || !policy_dev || !value_dev || batch < 1) return AF_TOWER_ERR_ARG;
    if (!t->set[t->blocks + kDense]) return AF_TOWER_ERR_STATE;
    DenseArgs a;
    a.vin = static_cast<const __bf16*>(vin_dev); a.pin = static_cast<const __bf16*>(pin_dev);
    a.wp = t->end<uint4>(kDenseWp); a.wv = t->end<uint4>(kDenseWv); a.pb = t->end<float>(kDensePb);
    a.vb1 = t->end<float>(kDenseVb1); a.vw2 = t->end<float>(kDenseVw2); a.vb2 = t->end<float>(kDenseVb2);
    a.policy = policy_dev; a.value = value_dev; a.batch = batch;
    const int blocks = (batch + 31) / 32;
    with_geo(t, [&](auto g) {
        hipLaunchKernelGGL(af_tower_dense_kernel<decltype(g)>, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, static_cast<hipStream_t>(stream), a);
        return 0;
    });
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int af_tower_stem(af_tower* t, void* stream, const float* planes_dev, void* x_dev, int32_t batch) {
    if (!t || !planes_dev || !x_dev || batch < 1) return AF_TOWER_ERR_ARG;
    if (!t->set[t->blocks + kStem]) return AF_TOWER_ERR_STATE;
    StemArgs a;
    a.planes = planes_dev; a.w = t->end<uint4>(kStemW); a.bias = t->end<float>(kStemB); a.out = static_cast<char*>(x_dev); a.batch = batch;
    const int grid = batch < 1024 ? batch : 1024;
    with_geo(t, [&](auto g) {
        hipLaunchKernelGGL(af_tower_stem_kernel<decltype(g)>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
        return 0;
    });
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int af_tower_heads(af_tower* t, void* stream, const void* x_dev, void* vin_dev, void* pin_dev, int32_t batch) {
    if (!t || !x_dev || !vin_dev || !pin_dev || batch < 1) return AF_TOWER_ERR_ARG;
    if (!t->set[t->blocks + kHeads]) return AF_TOWER_ERR_STATE;
    HeadsArgs a;
    a.x = static_cast<const char*>(x_dev); a.w = t->end<float>(kHeadsW); a.b = t->end<float>(kHeadsB);
    a.vin = static_cast<__bf16*>(vin_dev); a.pin = static_cast<__bf16*>(pin_dev); a.batch = batch;
    const int grid = batch < 2048 ? batch : 2048;
    if (g_heads == 0 && t->S == 11) {                // (the VALU kernel exists at 11x11 only: key 4 has no effect on a 15x15 handle)
        hipLaunchKernelGGL(af_tower_heads_kernel<G11>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    } else {
        HeadsMfmaArgs m;
        m.x = a.x; m.a = t->end<uint4>(kHeadsA); m.b = t->end<float>(kHeadsB32); m.vin = a.vin; m.pin = a.pin; m.batch = batch;
        // 15x15: two workgroups per position, and an even grid, so that a workgroup keeps its half of the tiles
        with_geo(t, [&](auto g) {
            using G = decltype(g);
            hipLaunchKernelGGL(af_tower_heads_mfma_kernel<G>, dim3(grid * (G::NT / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), m);
            return 0;
        });
    }
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int32_t af_tower_pix(const af_tower* t) { return t ? t->d.pix : 0; }
int64_t af_tower_plane_elems(const af_tower* t) { return t ? (int64_t)128 * t->d.pix : 0; }

int af_tower_forward(af_tower* t, void* stream, void* x_dev, void* g_dev, int32_t batch) {
    if (!t || !x_dev || !g_dev || batch < 1) return AF_TOWER_ERR_ARG;
    for (int b = 0; b < t->blocks; ++b) if (!t->set[b]) return AF_TOWER_ERR_STATE;
    for (int b = 0; b < t->blocks; ++b)
        for (int second = 0; second < 2; ++second) {
            const int rc = af_tower_launch_layer(t, static_cast<hipStream_t>(stream), b, second != 0, x_dev, g_dev, batch);
            if (rc) return rc;
        }
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int af_tower_forward_small(af_tower* t, void* stream, void* x_dev, void* g_dev, int32_t batch) {
    if (!t || !x_dev || !g_dev || batch < 1) return AF_TOWER_ERR_ARG;
    for (int b = 0; b < t->blocks; ++b) if (!t->set[b]) return AF_TOWER_ERR_STATE;
    const int64_t grid = (int64_t)batch * t->d.halves * 4;    // one workgroup per pixel tile of a (half-)position
    if (grid > INT32_MAX) return AF_TOWER_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int b = 0; b < t->blocks; ++b)
        for (int second = 0; second < 2; ++second)
            for (const SmallKernel& k : kSmall)
                if (k.S == t->S && k.proj == (second != 0))
                    hipLaunchKernelGGL(k.fn, dim3((unsigned)grid), dim3(256), k.lds, st, layer_args(t, b, second != 0, x_dev, g_dev, batch));
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int32_t af_tower_small_batch(const af_tower* t) { return !t ? 0 : t->S == 11 ? kSmallBatch11 : kSmallBatch15; }

#ifdef AF_TOWER_TIMING
int af_tower_debug_cycles(unsigned long long* host) {
    TW_HIP_OK(hipDeviceSynchronize());
    TW_HIP_OK(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_tower_cyc), sizeof(unsigned long long) * 2 * 256 * 4 * 5));
    return AF_TOWER_OK;
}
#endif

// ---- weights without the host ----
int af_tower_update_device(af_tower* t, void* stream, const float* const* dev_ptrs, const int64_t* counts, int32_t n) {
    // all or nothing: everything is checked before the first launch
    if (!t || !dev_ptrs || !counts || n != 12 + 6 * t->blocks) return AF_TOWER_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!dev_ptrs[i] || counts[i] != update_count(i, t->blocks, t->d)) return AF_TOWER_ERR_ARG;
    if (!all_set(t)) return AF_TOWER_ERR_STATE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int b0 = 0; b0 < t->blocks; b0 += kPackBlocks)
        pack_blocks(t, st, b0, t->blocks - b0 < kPackBlocks ? t->blocks - b0 : kPackBlocks, dev_ptrs + 2 + 6 * b0);
    const float* ends[12] = {dev_ptrs[0], dev_ptrs[1]};
    for (int k = 0; k < 10; ++k) ends[2 + k] = dev_ptrs[2 + 6 * t->blocks + k];
    pack_ends(t, st, ends, 0, t->d.ends_threads);
    TW_HIP_OK(hipGetLastError());
    return AF_TOWER_OK;
}

int64_t af_tower_debug_weights(af_tower* t, int32_t index, void* host_out, int64_t cap_bytes) {
    if (!t || index < 0 || index >= 4 * t->blocks + kEnds) return AF_TOWER_ERR_ARG;
    if (!t->set[group_of(index, t->blocks)]) return AF_TOWER_ERR_STATE;          // its host setter has not run yet
    const int64_t bytes = buffer_bytes(index, t->blocks, t->d);
    if (!host_out) return bytes;
    if (cap_bytes < bytes) return AF_TOWER_ERR_ARG;
    TW_HIP_OK(hipSetDevice(t->device));
    TW_HIP_OK(hipDeviceSynchronize());
    TW_HIP_OK(hipMemcpy(host_out, t->buf[index], (size_t)bytes, hipMemcpyDeviceToHost));
    return bytes;
}

int64_t af_tower_flops_per_position(const af_tower* t) {
    return (int64_t)2 * t->blocks * (128 * 128 * 9 * 2 + 128 * 128) * t->d.npix;
}

}  // extern "C"
