// af_net.hip — hand-written gfx950 forward pass of the alphaFive policy/value net
// (genData/network.py:52-97,163-165), fp32 on the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32
// products, fp32 accumulate).  C ABI: include/af_net.h.
//
// Activations live in zero-padded planes [batch][channel][WP*WP (+pad)], WP = 2*ceil(S/2)+2, so a
// convolution tap is a constant address shift and no kernel needs bounds checks; every layer writes
// straight into the next layer's padded layout.  Kernels:
//   af_conv_wino         (97 % of this path's algorithmic FLOPs) Winograd F(2x2,3x3) for every 3x3
//                        layer with the block's 1x1 projection folded into the Winograd domain; 16
//                        accumulators in AGPRs, on-the-fly input transform, fused output transform +
//                        bias + residual + ELU.  3.5 ms per 4096 positions at 11x11 (profiles/r6_02).
//   af_stem_conv, af_value_head, af_policy_head<PPB>, af_policy_head_mfma   5x5 stem and the two heads.
// This is the fp32-operand path (af_net_tune(0, 1)): every board size other than 11x11 / 15x15, and the 24-bit
// leg of bench.py.  The product path on 11x11 / 15x15 is af_conv_f16s.hip (af_net_tune(0, 5), default), which
// this file's af_net_forward dispatches to.  The variants that lost their A/B (U through LDS, LDS-DMA staging,
// persistent grid, direct implicit GEMM, sub-batch streams) were removed from the source in r6; their records
// are in DESIGN_HISTORY.md and profiles/.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "af_net.h"
#include "af_conv_f16s.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // 4 floats, only 4-byte aligned
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
typedef float f2a __attribute__((ext_vector_type(2)));               // 8-byte aligned pair (LDS reads)

// ELU(alpha=1).  exp(x)-1 through the hardware exp2 (absolute error ~1e-7 at x -> 0-, far inside the
// 1e-5 parity budget); expm1f costs ~30 VALU ops per element and sat un-overlapped in the epilogue.
__device__ __forceinline__ float elu1(float x) { return x > 0.0f ? x : __expf(x) - 1.0f; }

// ----------------------------------------------------------------------------------------------
// Winograd F(2x2,3x3) on the matrix cores: Y = A^T [ (G g G^T) (.) (B^T d B) ] A per 2x2 output
// tile, the 16 element-wise products becoming 16 independent [cout x cin] x [cin x tile] GEMMs:
// 16 MFMA k-steps per cin pair cover 32 tiles = 128 output pixels (direct: 9 k-steps cover 32
// pixels) => 2.25x fewer MFMA instructions for the layers that hold 97 % of the FLOPs.
//   * one wave = 32 tiles x 32 couts; all 16 Winograd-domain accumulators M[xi][nu] stay in
//     registers (256 AGPRs), so nothing is staged through memory: the input transform B^T d B
//     (32 adds on the lane's own 4x4 patch, loaded as 16 dwords) happens between the loads and the
//     MFMAs, the output transform A^T M A (24 adds per cout row) in the epilogue, fused with bias,
//     the residual projection, ELU and the store into the next layer's padded layout.
//   * the block's 1x1 projection is a 3x3 kernel with only the centre tap set; in the Winograd
//     domain only (xi,nu) in {1,2}^2 are non-zero, so it is 4 extra k-steps per cin pair into
//     M[1][1], M[1][2], M[2][1], M[2][2] and needs only the 2x2 centre of the patch.
//   * U = G g G^T is computed once per weight set (af_update_wino: fp64, rounded to fp32) and packed k-pair-major
//     [cin/2][2][cout][16] (a lane's 16 values = 4 dwordx4 loads); the 4 waves of a workgroup take 4 tile blocks of the SAME cout tile so
//     the weight stream is shared in L1.
// Plane layout: tiles need rows/cols 2t-1 .. 2t+2, so planes are padded to (2*ceil(S/2)+2)^2.
struct WinoArgs {
    const float* in;     // [batch][cin][PP]   input of the 3x3 convolution
    const float* u;      // [cin/2][2][cout][16]
    const float* in2;    // [batch][cin2][PP]  input of the 1x1 projection (or nullptr)
    const float* u2;     // [cin2/2][2][cout][4]
    const float* bias;   // [cout]
    float* out;          // [batch][cout][PP]
    int cin, cin2, cout, ntiles, T, S, WP, PP;
};

// (r1-r3 A/B records, removed from the source in r6: U through LDS — 6 % slower; both operands through LDS by LDS-DMA; a persistent grid;
//  a direct implicit-GEMM kernel af_conv_mfma — 5.2 ms against 3.5 per 4096 positions: profiles/r6_02_arith_width.json, DESIGN_HISTORY.md)
__device__ __forceinline__ void wino_task(const WinoArgs& A, const int bid) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, kh = lane >> 5;
    const int nct = A.cout >> 5;
    // XCD-aware block -> task map: workgroup b is observed to run on XCD b % 8 and each XCD has its own L2.
    // The nct workgroups that read the SAME activations (same tile-block group, different cout tile) get the
    // block ids g8, g8+8, g8+16, ... so they share one XCD's L2 instead of fetching the planes nct times.
    const int xcd = bid & 7, rest = bid >> 3;
    const int ct = rest % nct;
    const int tb = ((rest / nct) * 8 + xcd) * 4 + wave;
    if (tb * 32 >= A.ntiles) return;
    const int q = tb * 32 + col;
    const bool valid = q < A.ntiles;
    const int qq = valid ? q : 0;
    const int TT = A.T * A.T;
    const int pos = qq / TT;
    const int t_ = qq - pos * TT;
    const int ty = t_ / A.T, tx = t_ - ty * A.T;
    const int WP = A.WP, PP = A.PP, cout = A.cout;
    const int poff0 = 2 * ty * WP + 2 * tx;

    f32x16 M[16];
#pragma unroll
    for (int x = 0; x < 16; ++x)
#pragma unroll
        for (int r = 0; r < 16; ++r) M[x][r] = 0.0f;

    float bias_r[16];                                    // requested now, consumed in the epilogue
#pragma unroll
    for (int r = 0; r < 16; ++r) bias_r[r] = A.bias[ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh];
    const uint32_t wlane = (uint32_t)(kh * cout + ct * 32 + col);
    // k loops: operands ride a 4-deep register ring — the loads of phase p+3 are requested while phase p
    // computes (16 MFMAs = 1024 cycles per phase => >= 3072 cycles to land) — and the wide loads + the
    // transform adds of a phase are spread between its MFMAs by sched_group_barrier.
    {   // ---- 3x3 segment: phase = one cin pair (16 MFMAs) ----
        const char* __restrict__ inb = reinterpret_cast<const char*>(A.in);
        const uint32_t boff = (uint32_t)(pos * A.cin * PP + poff0 + kh * PP) * 4u;
        const int npairs = A.cin / 2;                    // multiple of 4
        f4u d0[4] = {}, d1[4] = {}, d2[4] = {}, d3[4] = {};
        auto load_d = [&](int c, f4u (&d)[4]) {
            c = c < npairs ? c : npairs - 1;             // tail: harmless re-load instead of a branch
            const char* ip = inb + (ptrdiff_t)(2 * c) * PP * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r)                  // one patch row = 4 consecutive floats (4-byte aligned)
                d[r] = *reinterpret_cast<const f4u*>(ip + (ptrdiff_t)(r * WP) * 4 + (size_t)boff);
        };
        {
            const char* __restrict__ ub = reinterpret_cast<const char*>(A.u);
            const uint32_t woff = wlane * 64u;           // 16 floats per (kh, cout)
            float4 u0[4] = {}, u1[4] = {}, u2[4] = {}, u3[4] = {};
            auto load_u = [&](int c, float4 (&u)[4]) {
                    c = c < npairs ? c : npairs - 1;
                const char* up = ub + (size_t)c * 2 * cout * 64;
#pragma unroll
                for (int r = 0; r < 4; ++r) u[r] = *reinterpret_cast<const float4*>(up + (size_t)r * 16 + (size_t)woff);
            };
            // the input transform runs ONE PHASE AHEAD of the MFMAs that consume it (v of pair c+1 is computed
            // while pair c multiplies), so no MFMA waits on a VALU result issued just before it
            auto transform = [&](f4u (&d)[4], float (&v)[16]) {
                float t[16];
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) {
                    t[0 + s_] = d[0][s_] - d[2][s_];
                    t[4 + s_] = d[1][s_] + d[2][s_];
                    t[8 + s_] = d[2][s_] - d[1][s_];
                    t[12 + s_] = d[1][s_] - d[3][s_];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i * 4 + 0] = t[i * 4 + 0] - t[i * 4 + 2];
                    v[i * 4 + 1] = t[i * 4 + 1] + t[i * 4 + 2];
                    v[i * 4 + 2] = t[i * 4 + 2] - t[i * 4 + 1];
                    v[i * 4 + 3] = t[i * 4 + 1] - t[i * 4 + 3];
                }
            };
            auto mfma16 = [&](float4 (&u)[4], float (&v)[16]) {
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    M[4 * x + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[x].x, v[4 * x + 0], M[4 * x + 0], 0, 0, 0);
                    M[4 * x + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[x].y, v[4 * x + 1], M[4 * x + 1], 0, 0, 0);
                    M[4 * x + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[x].z, v[4 * x + 2], M[4 * x + 2], 0, 0, 0);
                    M[4 * x + 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[x].w, v[4 * x + 3], M[4 * x + 3], 0, 0, 0);
                }
            };
            float vA[16], vB[16];
            auto phase = [&](int c_load, f4u (&dl)[4], float4 (&ul)[4], f4u (&dn)[4], float (&vn)[16], float4 (&uc)[4],
                             float (&vc)[16]) {
                load_d(c_load + 1, dl);        // a patch slot is free one phase earlier than a U slot: 4-phase lead
                load_u(c_load, ul);
                transform(dn, vn);
                mfma16(uc, vc);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);   // VALU
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            load_d(0, d0); load_u(0, u0);
            load_d(1, d1); load_u(1, u1);
            load_d(2, d2); load_u(2, u2);
            __builtin_amdgcn_sched_barrier(0);
            load_d(3, d3);
            transform(d0, vA);
            __builtin_amdgcn_sched_barrier(0);
            for (int c = 0; c < npairs; c += 4) {
                phase(c + 3, d0, u3, d1, vB, u0, vA);     // multiply pair c, transform pair c+1, load U c+3 / patch c+4
                phase(c + 4, d1, u0, d2, vA, u1, vB);
                phase(c + 5, d2, u1, d3, vB, u2, vA);
                phase(c + 6, d3, u2, d0, vA, u3, vB);
            }
        }
    }
    if (A.in2) {   // ---- 1x1 projection segment: phase = 4 cin pairs (16 MFMAs) ----
        const char* __restrict__ inb = reinterpret_cast<const char*>(A.in2);
        const char* __restrict__ ub = reinterpret_cast<const char*>(A.u2);
        const uint32_t boff = (uint32_t)(pos * A.cin2 * PP + poff0 + kh * PP + WP + 1) * 4u;   // patch centre (1,1)
        const uint32_t woff = wlane * 16u;               // 4 floats per (kh, cout)
        const int nph = A.cin2 / 8;                      // multiple of 4
        f2u d0[4][2], d1[4][2], d2[4][2], d3[4][2];
        float4 u0[4], u1[4], u2[4], u3[4];
        auto load_ph = [&](int q, f2u (&d)[4][2], float4 (&u)[4]) {
            q = q < nph ? q : nph - 1;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const char* ip = inb + (ptrdiff_t)(2 * (4 * q + h)) * PP * 4;
                const char* up = ub + (size_t)(4 * q + h) * 2 * cout * 16;
                d[h][0] = *reinterpret_cast<const f2u*>(ip + (size_t)boff);
                d[h][1] = *reinterpret_cast<const f2u*>(ip + (ptrdiff_t)WP * 4 + (size_t)boff);
                u[h] = *reinterpret_cast<const float4*>(up + (size_t)woff);
            }
        };
        auto compute_ph = [&](f2u (&d)[4][2], float4 (&u)[4]) {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const float t11 = d[h][0][0] + d[h][1][0], t12 = d[h][0][1] + d[h][1][1];   // (B^T d) rows 1,2, cols 1,2
                const float t21 = d[h][1][0] - d[h][0][0], t22 = d[h][1][1] - d[h][0][1];
                M[5] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[h].x, t11 + t12, M[5], 0, 0, 0);
                M[6] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[h].y, t12 - t11, M[6], 0, 0, 0);
                M[9] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[h].z, t21 + t22, M[9], 0, 0, 0);
                M[10] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[h].w, t22 - t21, M[10], 0, 0, 0);
            }
        };
        auto phase = [&](int q_load, f2u (&dl)[4][2], float4 (&ul)[4], f2u (&dc)[4][2], float4 (&uc)[4]) {
            load_ph(q_load, dl, ul);
            compute_ph(dc, uc);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        load_ph(0, d0, u0);
        load_ph(1, d1, u1);
        load_ph(2, d2, u2);
        __builtin_amdgcn_sched_barrier(0);
        for (int q = 0; q < nph; q += 4) {
            phase(q + 3, d3, u3, d0, u0);
            phase(q + 4, d0, u0, d1, u1);
            phase(q + 5, d1, u1, d2, u2);
            phase(q + 6, d2, u2, d3, u3);
        }
    }
    // ---- output transform Y = A^T M A, bias, ELU, store the 2x2 tile ----
    // (bias values were requested before the k loops; each tile row goes out as one 8-byte store, so the
    // lanes of a board row write one contiguous run)
    const bool ok1y = 2 * ty + 1 < A.S, ok1x = 2 * tx + 1 < A.S;      // rows/cols 2t are always inside the board
    float* const obase = A.out + (size_t)pos * cout * PP + poff0 + WP + 1;  // output pixel (2ty, 2tx) of cout 0
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const float bv = bias_r[r];
        float s0[4], s1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s0[j] = M[0 + j][r] + M[4 + j][r] + M[8 + j][r];
            s1[j] = M[4 + j][r] - M[8 + j][r] - M[12 + j][r];
        }
        f2u y0, y1;
        y0[0] = elu1(s0[0] + s0[1] + s0[2] + bv); y0[1] = elu1(s0[1] - s0[2] - s0[3] + bv);
        y1[0] = elu1(s1[0] + s1[1] + s1[2] + bv); y1[1] = elu1(s1[1] - s1[2] - s1[3] + bv);
        float* o = obase + (size_t)co * PP;
        if (valid) {
            if (ok1x) {
                *reinterpret_cast<f2u*>(o) = y0;
                if (ok1y) *reinterpret_cast<f2u*>(o + WP) = y1;
            } else {
                o[0] = y0[0];
                if (ok1y) o[WP] = y1[0];
            }
        }
    }
}

__global__ __launch_bounds__(256, 1) void af_conv_wino(WinoArgs A) { wino_task(A, (int)blockIdx.x); }

// (r1 experiment, removed: af_conv_wino2 split the 16 Winograd-domain accumulators over a wave pair —
// 128 AGPRs per wave, two waves per SIMD, partial outputs swapped through LDS.  Correct, but hipcc spilled
// 288 B/lane at the 256-register budget and the pair doubles the patch loads: 4.94 ms vs 3.96 ms.)

// stem: conv 5x5 SAME 3->32 + ELU (network.py:63), one block per position, one thread per pixel
__global__ __launch_bounds__(256) void af_stem_conv(const float* __restrict__ planes, const float* __restrict__ w /*[75][32]*/,
                                                    const float* __restrict__ bias, float* __restrict__ out, int S, int WP, int PP) {
    __shared__ float sx[3 * 20 * 20];
    __shared__ float sw[75 * 32];
    __shared__ float sb[32];
    const int b = blockIdx.x, t = threadIdx.x, HW = S * S, XP = S + 4;
    for (int i = t; i < 3 * XP * XP; i += blockDim.x) sx[i] = 0.0f;
    for (int i = t; i < 75 * 32; i += blockDim.x) sw[i] = w[i];
    if (t < 32) sb[t] = bias[t];
    __syncthreads();
    for (int i = t; i < 3 * HW; i += blockDim.x) {
        const int c = i / HW, p = i - c * HW, y = p / S, x = p - y * S;
        sx[c * XP * XP + (y + 2) * XP + x + 2] = planes[(size_t)b * 3 * HW + i];
    }
    __syncthreads();
    if (t >= HW) return;
    const int y = t / S, x = t - y * S;
    float acc[32];
#pragma unroll
    for (int co = 0; co < 32; ++co) acc[co] = sb[co];
    for (int ky = 0; ky < 5; ++ky)
        for (int kx = 0; kx < 5; ++kx)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float xv = sx[c * XP * XP + (y + ky) * XP + x + kx];
                const float* wr = sw + ((ky * 5 + kx) * 3 + c) * 32;
#pragma unroll
                for (int co = 0; co < 32; ++co) acc[co] = fmaf(xv, wr[co], acc[co]);
            }
    float* o = out + (size_t)b * 32 * PP + (y + 1) * WP + x + 1;
#pragma unroll
    for (int co = 0; co < 32; ++co) o[(size_t)co * PP] = elu1(acc[co]);
}

// value head: 1x1 conv 32->4 + ELU, fc 4*HW->64 + ELU, fc 64->1, tanh(x/2)  (network.py:70-76,163).
// VPB positions per workgroup: the fc1 weights (4*HW x 64 floats = 124 KB at 11x11) are streamed from L2 once per
// workgroup, not once per position (r1: one position per block = 0.5 GB of L2 reads per forward for 0.2 GMAC).
constexpr int VPB = 8;
__global__ __launch_bounds__(256) void af_value_head(const float* __restrict__ in /*[b][32][PP]*/, const float* __restrict__ wc /*[32][4]*/,
                                                     const float* __restrict__ bc, const float* __restrict__ w1 /*[4HW][64]*/,
                                                     const float* __restrict__ b1, const float* __restrict__ w2 /*[64]*/,
                                                     const float* __restrict__ b2, float* __restrict__ value, int batch, int S, int WP, int PP) {
    __shared__ float sh[VPB][4 * 256];
    __shared__ float swc[32 * 4];
    __shared__ float s64[VPB][64];
    const int b0 = blockIdx.x * VPB, t = threadIdx.x, HW = S * S;
    if (t < 128) swc[t] = wc[t];
    __syncthreads();
    for (int it = t; it < VPB * HW; it += 256) {                     // 1x1 conv + ELU: item = (position q, pixel)
        const int q = it / HW, px = it - q * HW, y = px / S, x = px - y * S;
        const int b = b0 + q < batch ? b0 + q : batch - 1;
        const float* p = in + (size_t)b * 32 * PP + (y + 1) * WP + x + 1;
        float a0 = bc[0], a1 = bc[1], a2 = bc[2], a3 = bc[3];
#pragma unroll 8
        for (int c = 0; c < 32; ++c) {
            const float xv = p[(size_t)c * PP];
            a0 = fmaf(xv, swc[c * 4 + 0], a0); a1 = fmaf(xv, swc[c * 4 + 1], a1);
            a2 = fmaf(xv, swc[c * 4 + 2], a2); a3 = fmaf(xv, swc[c * 4 + 3], a3);
        }
        sh[q][0 * HW + px] = elu1(a0); sh[q][1 * HW + px] = elu1(a1); sh[q][2 * HW + px] = elu1(a2); sh[q][3 * HW + px] = elu1(a3);
    }
    __syncthreads();
    {                                                                // fc1: thread = (output o, pair of positions pg)
        const int o = t & 63, pg = t >> 6;
        float acc0 = b1[o], acc1 = acc0;
        const float* x0 = sh[2 * pg];
        const float* x1 = sh[2 * pg + 1];
        for (int k = 0; k < 4 * HW; ++k) {                           // same k order as one-position-per-block: same bits
            const float w = w1[(size_t)k * 64 + o];
            acc0 = fmaf(x0[k], w, acc0);
            acc1 = fmaf(x1[k], w, acc1);
        }
        s64[2 * pg][o] = elu1(acc0) * w2[o];
        s64[2 * pg + 1][o] = elu1(acc1) * w2[o];
    }
    __syncthreads();
    if (t < VPB && b0 + t < batch) {
        float s = b2[0];
        for (int j = 0; j < 64; ++j) s += s64[t][j];
        value[b0 + t] = tanhf(s * 0.5f);
    }
}

// policy head: 1x1 conv 32->16 + ELU, fc 16*HW->HW, softmax  (network.py:82-88); PPB positions per block
template <int PPB>
__global__ __launch_bounds__(256) void af_policy_head(const float* __restrict__ in /*[b][32][PP]*/, const float* __restrict__ wc /*[32][16]*/,
                                                      const float* __restrict__ bc, const float* __restrict__ wf /*[16HW][HW]*/,
                                                      const float* __restrict__ bf, float* __restrict__ policy, int batch, int S, int WP, int PP) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int HW = S * S, t = threadIdx.x, b0 = blockIdx.x * PPB;
    float* sh = smem;                       // [16*HW][PPB]
    float* swc = smem + 16 * HW * PPB;      // [32][16]
    float* red = swc + 512;                 // [4 waves][PPB]
    for (int i = t; i < 512; i += blockDim.x) swc[i] = wc[i];
    __syncthreads();
    if (t < HW) {
        const int y = t / S, x = t - y * S;
        for (int p = 0; p < PPB; ++p) {
            const int b = b0 + p < batch ? b0 + p : batch - 1;
            const float* src = in + (size_t)b * 32 * PP + (y + 1) * WP + x + 1;
            float a[16];
#pragma unroll
            for (int co = 0; co < 16; ++co) a[co] = bc[co];
            for (int c = 0; c < 32; ++c) {
                const float xv = src[(size_t)c * PP];
#pragma unroll
                for (int co = 0; co < 16; ++co) a[co] = fmaf(xv, swc[c * 16 + co], a[co]);
            }
#pragma unroll
            for (int co = 0; co < 16; ++co) sh[(co * HW + t) * PPB + p] = elu1(a[co]);
        }
    }
    __syncthreads();
    // dense layer: thread (ks, tj) accumulates logit tj over the ks-th slice of the 16*HW inputs for PPB
    // positions at once (weights streamed once per block); slices are summed through LDS in fixed order
    const int JW = HW <= 128 ? 128 : 256, KS = blockDim.x / JW;
    const int ks = t / JW, tj = t - ks * JW;
    const bool owner = ks == 0 && tj < HW;
    float acc[PPB];
    const int j = tj < HW ? tj : HW - 1;
#pragma unroll
    for (int p = 0; p < PPB; ++p) acc[p] = ks == 0 ? bf[j] : 0.0f;
    const int K = 16 * HW, k0 = ks * (K / KS), k1 = ks == KS - 1 ? K : k0 + K / KS;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) {
        const float wv = wf[(size_t)k * HW + j];
        const float4* xr = reinterpret_cast<const float4*>(sh + (size_t)k * PPB);
#pragma unroll
        for (int q = 0; q < PPB / 4; ++q) {
            const float4 xv = xr[q];
            acc[4 * q + 0] = fmaf(xv.x, wv, acc[4 * q + 0]); acc[4 * q + 1] = fmaf(xv.y, wv, acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(xv.z, wv, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(xv.w, wv, acc[4 * q + 3]);
        }
    }
    if (KS > 1) {
        __syncthreads();                                  // everyone is done reading sh: reuse it for the partials
        if (ks > 0) {
#pragma unroll
            for (int p = 0; p < PPB; ++p) sh[((ks - 1) * PPB + p) * JW + tj] = acc[p];
        }
        __syncthreads();
        if (ks == 0) {
            for (int s_ = 1; s_ < KS; ++s_)
#pragma unroll
                for (int p = 0; p < PPB; ++p) acc[p] += sh[((s_ - 1) * PPB + p) * JW + tj];
        }
    }
    // softmax over the HW logits of each position
    const int wave = t >> 6, lane = t & 63, nw = blockDim.x >> 6;
    float m[PPB];
#pragma unroll
    for (int p = 0; p < PPB; ++p) {
        float v = owner ? acc[p] : -3.0e38f;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
        if (lane == 0) red[wave * PPB + p] = v;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < PPB; ++p) {
        float v = red[p];
        for (int w_ = 1; w_ < nw; ++w_) v = fmaxf(v, red[w_ * PPB + p]);
        m[p] = v;
    }
    __syncthreads();
    float e[PPB];
#pragma unroll
    for (int p = 0; p < PPB; ++p) {
        e[p] = owner ? expf(acc[p] - m[p]) : 0.0f;
        float v = e[p];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
        if (lane == 0) red[wave * PPB + p] = v;
    }
    __syncthreads();
    if (owner) {
#pragma unroll
        for (int p = 0; p < PPB; ++p) {
            float s_ = red[p];
            for (int w_ = 1; w_ < nw; ++w_) s_ += red[w_ * PPB + p];
            if (b0 + p < batch) policy[(size_t)(b0 + p) * HW + tj] = e[p] / s_;
        }
    }
}

// policy head on the matrix cores (boards up to 11x11), 16 positions per workgroup = one workgroup per CU
// at 4096 leaves.  All three phases are matrix shaped, v_mfma_f32_16x16x4_f32 throughout:
//   phase 1  1x1 conv 32->16 + ELU: D[co][item] = sum_ci wc[ci][co] x[ci][item] over tiles of 16 items
//            (item = position*HW + pixel); A = the lane's 8 weights (registers), B = one dword per k-step
//            straight from the padded planes, two tiles in flight; result -> X[pos][co*HW + pix] in LDS
//            (the NCHW flatten order of network.py:83-84; row stride = 2 mod 32: conflict-free B reads later)
//   phase 2  logits^T[j][pos] = sum_k Wfc[k][j] X[pos][k]: A = 16 logits x 4 k from global (64-byte runs,
//            requested 16 k-steps = 1024 MFMA cycles ahead), B = 4 k x 16 positions from LDS; each wave owns
//            two 16-logit tiles
//   phase 3  logits -> LDS, softmax by 16-lane groups, store
typedef float f32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void af_policy_head_mfma(const float* __restrict__ in /*[b][32][PP]*/, const float* __restrict__ wc /*[32][16]*/,
                                                           const float* __restrict__ bc, const float* __restrict__ wf /*[16HW][HW]*/,
                                                           const float* __restrict__ bf, float* __restrict__ policy, int batch, int S, int WP, int PP) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int HW = S * S, K = 16 * HW, t = threadIdx.x, b0 = blockIdx.x * 16;
    const int KS = K + ((2 - K % 32) + 32) % 32;
    float* X = smem;                                       // [16][KS]
    const int lane = t & 63, wave = t >> 6, i16 = lane & 15, kq = lane >> 4;
    {   // ---- phase 1 ----
        float aw[8];                                       // A fragments: wc[ci = 4s+kq][co = i16]
#pragma unroll
        for (int s_ = 0; s_ < 8; ++s_) aw[s_] = wc[(4 * s_ + kq) * 16 + i16];
        float bias4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bias4[r] = bc[kq * 4 + r];
        const int nitems = 16 * HW, ntiles = (nitems + 15) / 16;
        auto item_src = [&](int tile, int& p, int& pix) -> const float* {
            int it = tile * 16 + i16;
            it = it < nitems ? it : nitems - 1;
            p = it / HW;
            pix = it - p * HW;
            const int y = pix / S, x = pix - y * S;
            const int b = b0 + p < batch ? b0 + p : batch - 1;
            return in + (size_t)b * 32 * PP + (size_t)kq * PP + (y + 1) * WP + x + 1;
        };
        for (int tile = wave; tile < ntiles; tile += 8) {   // two tiles (this one and tile+4) in flight
            int p0, x0, p1, x1;
            const float* s0 = item_src(tile, p0, x0);
            const bool has1 = tile + 4 < ntiles;
            const float* s1 = item_src(has1 ? tile + 4 : tile, p1, x1);
            float bx0[8], bx1[8];
#pragma unroll
            for (int s_ = 0; s_ < 8; ++s_) { bx0[s_] = s0[(size_t)(4 * s_) * PP]; bx1[s_] = s1[(size_t)(4 * s_) * PP]; }
            f32x4 d0 = {0, 0, 0, 0}, d1 = {0, 0, 0, 0};
#pragma unroll
            for (int s_ = 0; s_ < 8; ++s_) {
                d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[s_], bx0[s_], d0, 0, 0, 0);
                d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[s_], bx1[s_], d1, 0, 0, 0);
            }
            const bool ok0 = tile * 16 + i16 < nitems, ok1 = has1 && (tile + 4) * 16 + i16 < nitems;
#pragma unroll
            for (int r = 0; r < 4; ++r) {                  // D: col = lane&15 (item), row = kq*4 + r (co)
                if (ok0) X[p0 * KS + (kq * 4 + r) * HW + x0] = elu1(d0[r] + bias4[r]);
                if (ok1) X[p1 * KS + (kq * 4 + r) * HW + x1] = elu1(d1[r] + bias4[r]);
            }
        }
    }
    __syncthreads();
    // ---- phase 2 ----
    const int j0 = wave * 32 + i16, j1 = j0 + 16;
    const float* w0 = wf + (size_t)kq * HW + (j0 < HW ? j0 : HW - 1);
    const float* w1 = wf + (size_t)kq * HW + (j1 < HW ? j1 : HW - 1);
    const float* xb = X + i16 * KS + kq;
    f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
    constexpr int PF = 16;
    float a0[PF], a1[PF];
    const int nsteps = K / 4;                              // = 4*HW (484 at 11x11: not a multiple of PF -> tail below)
#pragma unroll
    for (int q = 0; q < PF; ++q) { a0[q] = w0[(size_t)q * 4 * HW]; a1[q] = w1[(size_t)q * 4 * HW]; }
    int s0 = 0;
    for (; s0 + PF <= nsteps; s0 += PF) {
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            const int s_ = s0 + q;
            const float bx = xb[s_ * 4];
            const float ca0 = a0[q], ca1 = a1[q];
            const int sn = s_ + PF < nsteps ? s_ + PF : nsteps - 1;   // ring slot q now waits for step s_+PF
            a0[q] = w0[(size_t)sn * 4 * HW];
            a1[q] = w1[(size_t)sn * 4 * HW];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca0, bx, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca1, bx, acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int q = 0; q < PF; ++q) {                         // tail: slots 0..rem-1 hold steps s0..nsteps-1
        if (s0 + q < nsteps) {
            const float bx = xb[(s0 + q) * 4];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[q], bx, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[q], bx, acc1, 0, 0, 0);
        }
    }
    __syncthreads();                                       // X is dead: reuse it for the logits [16 pos][128]
    float* Lg = smem;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                          // D: col = lane&15 (position), row = kq*4 + r
        const int ja = wave * 32 + kq * 4 + r, jb = ja + 16;
        Lg[i16 * 128 + ja] = acc0[r] + (ja < HW ? bf[ja] : 0.0f);
        Lg[i16 * 128 + jb] = acc1[r] + (jb < HW ? bf[jb] : 0.0f);
    }
    __syncthreads();
    // ---- phase 3 ----
    const int p = t >> 4, sub = t & 15;                    // 16 threads per position, 8 logits each
    float v[8], m = -3.0e38f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int j = sub + 16 * q;
        v[q] = j < HW ? Lg[p * 128 + j] : -3.0e38f;
        m = fmaxf(m, v[q]);
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    float sum = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) { v[q] = (sub + 16 * q) < HW ? expf(v[q] - m) : 0.0f; sum += v[q]; }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if (b0 + p < batch) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = sub + 16 * q;
            if (j < HW) policy[(size_t)(b0 + p) * HW + j] = v[q] / sum;
        }
    }
}

// ----------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------
#define NET_HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "[af_net] %s failed: %s\n", #x, hipGetErrorString(e_)); return AF_NET_ERR_HIP; } } while (0)

// (the five blocks and the 42 variables: kBlocks, kNetVars and their indices in af_conv_f16s.h)
static int var_index(const char* name) {
    for (int i = 0; i < kVars; ++i) if (!strcmp(kNetVars[i].name, name)) return i;
    return -1;
}
static size_t var_count(int i, int HW) { const NetVar& v = kNetVars[i]; return v.c0 + (size_t)v.c1 * HW + (size_t)v.c2 * HW * HW; }
static size_t var_offset(int i, int HW) {        // in floats; var_offset(kVars, HW) = the size of the staging area
    size_t at = 0;
    for (int k = 0; k < i; ++k) at += var_count(k, HW);
    return at;
}

// The fp32 path's weight-derived buffers in af_net_debug_weights' order (the split-operand path's follow: f16s_weight_buffer): stem
// kernel and bias; per block the padded conv1 bias, the padded conv2 + projection bias and the Winograd-domain conv1 / conv2 /
// projection kernels; the heads' ten tensors as they are, in the variables' order.
enum { kStemW, kStemB, kConv1B, kSumB = kConv1B + 5, kWino1 = kSumB + 5, kWino2 = kWino1 + 5, kWinoR = kWino2 + 5, kHeadW = kWinoR + 5,
       kVcW = kHeadW, kVcB, kV1W, kV1B, kV2W, kV2B, kPcW, kPcB, kPfW, kPfB, kWeightBufs };
static size_t weight_count(int i, int HW) {
    if (i < kConv1B) return var_count(i, HW);
    if (i >= kHeadW) return var_count(kVarHeads + i - kHeadW, HW);
    const NetBlock& b = kBlocks[(i - kConv1B) % 5];
    if (i < kWino1) return (b.cout + 31) / 32 * 32;          // biases are padded to a multiple of 32 couts
    if (i < kWino2) return (size_t)b.cin * b.cout * 16;
    return i < kWinoR ? (size_t)b.cout * b.cout * 16 : (size_t)b.cin * b.cout * 4;
}
// ... and its activation buffers [max_batch][C][PP]: the stem's output, then per block g (conv1's output) and o (the block's)
enum { kF0, kG, kO, kActs = 1 + 2 * 5 };
static int act_channels(int i) { return i == kF0 ? 32 : kBlocks[(i - kG) / 2].cout; }

// Everything a handle owns is made by af_net_create and lives until af_net_destroy; no call in between allocates or frees.
struct af_net {
    int S, HW, WP, PP, T, max_batch, device;
    // state.  set: af_net_set_variable marks a variable, af_net_update_device clears them all (the host image is stale then);
    // packed and ready: pack_from_device sets both, af_net_set_variable takes ready back until the next af_net_finalize
    bool set[kVars] = {}, packed = false, ready = false;
    std::vector<float> image;     // host image of the staging area
    float* arena = nullptr;       // one allocation: stage, upd_max_dev and w[] at 256-byte offsets
    float* stage = nullptr;       // the 42 fp32 variables as af_net_finalize uploads them: what its pack kernels read
    float *upd_max_dev = nullptr, *upd_max_host = nullptr;      // max|w| per scale group of the split-operand path, device and pinned host
    float* w[kWeightBufs] = {};
    float* act[kActs] = {};       // zero-filled once: no kernel writes their borders
    hipStream_t branch_stream = nullptr;
    hipEvent_t ev_trunk = nullptr, ev_value = nullptr;
    f16s_net* f16s = nullptr;     // 11x11 and 15x15 boards: the fp16 split-operand convolution path (af_conv_f16s.hip)
};

// Winograd weights U = G g G^T per (cin, cout), G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]], packed [cin/2][2][cout][npos] (one
// lane's npos values contiguous).  taps == 9: all 16 (xi,nu); taps == 1: the centre-tap kernel of a 1x1 projection, whose only
// non-zero positions are (1,1),(1,2),(2,1),(2,2).  A thread per (cin, cout) pair reads the pair's taps (HWIO, device memory) and
// writes its npos values: fp64, summed over i then j, no contraction, then rounded to fp32.
struct WinoPackDesc { const float* w; float* out; int taps, cin, cout; };
constexpr int kWinoBufs = 15, kWinoPackBlocks = 64;
struct WinoPackTable { WinoPackDesc d[kWinoBufs]; };
__global__ __launch_bounds__(256) void af_update_wino(WinoPackTable T) {
#pragma clang fp contract(off)
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const WinoPackDesc& D = T.d[blockIdx.y];
    for (int q = blockIdx.x * 256 + threadIdx.x; q < D.cin * D.cout; q += kWinoPackBlocks * 256) {
        const int c = q / D.cout, co = q - c * D.cout;
        double g[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        if (D.taps == 9) {
#pragma unroll
            for (int t = 0; t < 9; ++t) g[t / 3][t % 3] = D.w[((size_t)t * D.cin + c) * D.cout + co];
        } else {
            g[1][1] = D.w[(size_t)c * D.cout + co];
        }
        float u16[16];
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int xi = x / 4, nu = x % 4;
            double u = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) u += G[xi][i] * g[i][j] * G[nu][j];
            u16[x] = (float)u;
        }
        if (D.taps == 9) {
            float4* o = reinterpret_cast<float4*>(D.out + (size_t)q * 16);       // ((c/2)*2 + (c&1)) * cout + co = q
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = make_float4(u16[4 * r], u16[4 * r + 1], u16[4 * r + 2], u16[4 * r + 3]);
        } else {
            *reinterpret_cast<float4*>(D.out + (size_t)q * 4) = make_float4(u16[5], u16[6], u16[9], u16[10]);
        }
    }
}

// Packs every weight-derived buffer of the handle, in place, from the 42 fp32 TF-layout tensors src names in device memory
// (kNetVars' order): the one packer behind af_net_finalize and af_net_update_device.  Asynchronous on st but for ONE wait: the
// scales of the split-operand path need max|w| per group, reduced on the device and brought to the host as 80 bytes.
static int pack_from_device(af_net* n, hipStream_t st, const float* const* src) {
    if (n->f16s) {
        if (f16s_update_absmax(n->f16s, st, src, n->upd_max_dev)) return AF_NET_ERR_HIP;
        NET_HIP_OK(hipMemcpyAsync(n->upd_max_host, n->upd_max_dev, kF16sScaleGroups * sizeof(float), hipMemcpyDeviceToHost, st));
        NET_HIP_OK(hipStreamSynchronize(st));
        if (f16s_update_pack(n->f16s, st, src, n->upd_max_host)) return AF_NET_ERR_HIP;
    }
    WinoPackTable W = {};
    UpdCopy C[22];
    int ncp = 0;
    auto copy = [&](int buf, int v, const float* b, int sum) {
        C[ncp++] = UpdCopy{n->w[buf], src[v], b, (int)weight_count(buf, n->HW), (int)var_count(v, n->HW), sum};
    };
    copy(kStemW, kVarStemK, nullptr, 0); copy(kStemB, kVarStemB, nullptr, 0);
    for (int i = 0; i < 5; ++i) {
        const NetBlock& b = kBlocks[i];
        // biases padded with zeros to a multiple of 32 couts; conv1's is bias + 0.0f, conv2's the sum with the projection's
        copy(kConv1B + i, var(i, kC1B), nullptr, 1);
        copy(kSumB + i, var(i, kC2B), src[var(i, kResB)], 1);
        W.d[3 * i] = WinoPackDesc{src[var(i, kC1K)], n->w[kWino1 + i], 9, b.cin, b.cout};
        W.d[3 * i + 1] = WinoPackDesc{src[var(i, kC2K)], n->w[kWino2 + i], 9, b.cout, b.cout};
        W.d[3 * i + 2] = WinoPackDesc{src[var(i, kResK)], n->w[kWinoR + i], 1, b.cin, b.cout};
    }
    for (int j = 0; j < 10; ++j) copy(kHeadW + j, kVarHeads + j, nullptr, 0);
    hipLaunchKernelGGL(af_update_wino, dim3(kWinoPackBlocks, kWinoBufs), dim3(256), 0, st, W);
    NET_HIP_OK(hipGetLastError());
    if (upd_launch_copies(st, C, ncp)) return AF_NET_ERR_HIP;
    n->packed = n->ready = true;
    return AF_NET_OK;
}

// af_net_create's device half (no forward runs before an af_net_finalize, which waits for the device: the zero-fills have finished by then)
static int allocate(af_net* n) {
    NET_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(af_policy_head_mfma), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024));
    auto pad64 = [](size_t count) { return (count + 63) & ~(size_t)63; };       // floats: every buffer of the arena starts at a 256-byte offset
    n->image.resize(var_offset(kVars, n->HW));
    size_t total = pad64(n->image.size()) + pad64(kF16sScaleGroups);
    for (int i = 0; i < kWeightBufs; ++i) total += pad64(weight_count(i, n->HW));
    NET_HIP_OK(hipMalloc((void**)&n->arena, total * sizeof(float)));
    n->stage = n->arena;
    n->upd_max_dev = n->stage + pad64(n->image.size());
    float* p = n->upd_max_dev + pad64(kF16sScaleGroups);
    for (int i = 0; i < kWeightBufs; ++i) { n->w[i] = p; p += pad64(weight_count(i, n->HW)); }
    NET_HIP_OK(hipHostMalloc((void**)&n->upd_max_host, kF16sScaleGroups * sizeof(float), hipHostMallocDefault));
    for (int i = 0; i < kActs; ++i) {
        const size_t bytes = (size_t)n->max_batch * n->PP * act_channels(i) * sizeof(float);
        NET_HIP_OK(hipMalloc((void**)&n->act[i], bytes));
        NET_HIP_OK(hipMemset(n->act[i], 0, bytes));
    }
    NET_HIP_OK(hipStreamCreateWithFlags(&n->branch_stream, hipStreamNonBlocking));
    NET_HIP_OK(hipEventCreateWithFlags(&n->ev_trunk, hipEventDisableTiming));
    NET_HIP_OK(hipEventCreateWithFlags(&n->ev_value, hipEventDisableTiming));
    if (f16s_supported(n->S) && f16s_create(&n->f16s, n->S, n->max_batch, n->device) != 0) return AF_NET_ERR_HIP;
    return AF_NET_OK;
}

extern "C" {

const char* af_net_strerror(int code) {
    switch (code) {
        case AF_NET_OK: return "ok";
        case AF_NET_ERR_ARG: return "bad argument";
        case AF_NET_ERR_HIP: return "HIP runtime error";
        case AF_NET_ERR_NAME: return "unknown variable name or wrong element count";
        case AF_NET_ERR_STATE: return "network not finalized or variables missing";
        default: return "unknown error";
    }
}

int af_net_create(int32_t S, int32_t max_batch, int32_t device, af_net** out) {
    if (!out || S < 3 || S > 16 || max_batch < 1) return AF_NET_ERR_ARG;
    NET_HIP_OK(hipSetDevice(device));
    af_net* n = new af_net();
    n->S = S; n->HW = S * S;
    n->T = (S + 1) / 2;                      // 2x2 output tiles per board side (Winograd)
    n->WP = 2 * n->T + 2;                    // plane padded so every tile's 4x4 patch is in bounds
    n->PP = (n->WP * n->WP + 15) / 16 * 16;
    n->max_batch = max_batch; n->device = device;
    // the conv kernels address activations with 32-bit byte offsets: the widest buffer must stay below 4 GiB
    if ((uint64_t)max_batch * 128u * (uint64_t)n->PP * 4u >= (1ull << 32)) { delete n; return AF_NET_ERR_ARG; }
    const int rc = allocate(n);
    if (rc) { af_net_destroy(n); return rc; }
    *out = n;
    return AF_NET_OK;
}

void af_net_destroy(af_net* n) {
    if (!n) return;
    (void)hipSetDevice(n->device);
    f16s_destroy(n->f16s);
    (void)hipFree(n->arena);
    for (float* a : n->act) (void)hipFree(a);
    if (n->upd_max_host) (void)hipHostFree(n->upd_max_host);
    if (n->branch_stream) (void)hipStreamDestroy(n->branch_stream);
    if (n->ev_trunk) (void)hipEventDestroy(n->ev_trunk);
    if (n->ev_value) (void)hipEventDestroy(n->ev_value);
    delete n;
}

int af_net_set_variable(af_net* n, const char* name, const float* data, int64_t count) {
    if (!n || !name || !data) return AF_NET_ERR_ARG;
    const int v = var_index(name);
    if (v < 0 || (int64_t)var_count(v, n->HW) != count) return AF_NET_ERR_NAME;
    memcpy(n->image.data() + var_offset(v, n->HW), data, (size_t)count * sizeof(float));
    n->set[v] = true;
    n->ready = false;
    return AF_NET_OK;
}

int af_net_finalize(af_net* n) {
    if (!n) return AF_NET_ERR_ARG;
    for (bool s : n->set) if (!s) return AF_NET_ERR_STATE;
    NET_HIP_OK(hipSetDevice(n->device));
    NET_HIP_OK(hipDeviceSynchronize());          // forwards in flight, on any stream, still read the buffers
    if (n->f16s && f16s_reset_roles(n->f16s)) return AF_NET_ERR_HIP;
    NET_HIP_OK(hipMemcpy(n->stage, n->image.data(), n->image.size() * sizeof(float), hipMemcpyHostToDevice));
    const float* src[kVars];
    for (int i = 0; i < kVars; ++i) src[i] = n->stage + var_offset(i, n->HW);
    const int rc = pack_from_device(n, nullptr, src);
    if (rc) return rc;
    NET_HIP_OK(hipStreamSynchronize(nullptr));   // every pack kernel has finished: a forward on any stream finds the weights
    return AF_NET_OK;
}

int af_net_update_device(af_net* n, void* stream, const char* const* tf_names, const float* const* dev_ptrs, const int64_t* counts,
                         int32_t nvars) {
    if (!n || !tf_names || !dev_ptrs || !counts) return AF_NET_ERR_ARG;            // (before any HIP call)
    if (!n->packed) return AF_NET_ERR_STATE;                                       // never finalized
    // all or nothing: every name known, every count right, all variables present exactly once — before anything is launched
    if (nvars != kVars) return AF_NET_ERR_ARG;
    const float* src[kVars] = {};
    for (int i = 0; i < nvars; ++i) {
        if (!tf_names[i] || !dev_ptrs[i]) return AF_NET_ERR_ARG;
        const int v = var_index(tf_names[i]);
        if (v < 0 || (int64_t)var_count(v, n->HW) != counts[i]) return AF_NET_ERR_NAME;
        if (src[v]) return AF_NET_ERR_ARG;                                         // a name twice (so another one is missing)
        src[v] = dev_ptrs[i];
    }
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    NET_HIP_OK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return AF_NET_ERR_STATE;                // this call waits for the stream once: not capturable
    NET_HIP_OK(hipSetDevice(n->device));
    const int rc = pack_from_device(n, st, src);
    if (rc) return rc;
    for (bool& s : n->set) s = false;        // the host image is stale: af_net_finalize needs all 42 variables set again
    return AF_NET_OK;
}

int64_t af_net_debug_weights(af_net* n, int32_t index, void* host_out, int64_t cap_bytes) {
    if (!n || index < 0 || !n->packed) return AF_NET_ERR_ARG;
    const void* p = nullptr;
    size_t bytes = 0;
    if (index < kWeightBufs) { p = n->w[index]; bytes = weight_count(index, n->HW) * sizeof(float); }
    else if (!n->f16s || f16s_weight_buffer(n->f16s, index - kWeightBufs, &p, &bytes)) return AF_NET_ERR_ARG;
    if (!host_out) return (int64_t)bytes;
    if (cap_bytes < (int64_t)bytes) return AF_NET_ERR_ARG;
    NET_HIP_OK(hipSetDevice(n->device));
    NET_HIP_OK(hipDeviceSynchronize());
    NET_HIP_OK(hipMemcpy(host_out, p, bytes, hipMemcpyDeviceToHost));
    return (int64_t)bytes;
}

int32_t af_net_debug_scales(af_net* n, float* host_out, int32_t cap) {
    if (!n || !host_out || cap < 0) return AF_NET_ERR_ARG;
    return n->f16s ? f16s_scales(n->f16s, host_out, cap) : 0;
}

}  // extern "C"

// The process-global knobs, by af_net_tune key
static struct {
    int conv = 5;        // 0: 5 = fp16 split-operand implicit GEMM on 11x11 / 15x15 boards (default; other sizes run 1); 1 = af_conv_wino (fp32 MFMA, Winograd)
    int branch = 1;      // 4: value branch on a side stream (fp32 path: 1/0; 2 forces it on path 5)
    int phead = 1;       // 5: 1 = af_policy_head_mfma for boards up to 11x11; 0 = VALU head
    int f16s_bits = 0;   // 7: A/B and profiling bits of af_conv_f16s.hip (F16sBits)
    int fhead = 1;       // 9: 1 = the split-operand path computes the heads itself (fused 1x1 conv + MFMA dense layers); 0 = af_value_head / af_policy_head_mfma
} g_tune;

extern "C" int af_net_tune(int32_t key, int32_t value) {
    if (key == 0) { if (value != 1 && value != 5) return AF_NET_ERR_ARG; g_tune.conv = value; return AF_NET_OK; }
    if (key == 4) { g_tune.branch = value; return AF_NET_OK; }
    if (key == 5) { g_tune.phead = value; return AF_NET_OK; }
    if (key == 7) { g_tune.f16s_bits = value; return AF_NET_OK; }
    if (key == 9) { g_tune.fhead = value ? 1 : 0; return AF_NET_OK; }
    return AF_NET_ERR_ARG;
}

static void launch_wino(hipStream_t st, const af_net* n, int batch, const float* in, const float* u, int cin,
                        const float* in2, const float* u2, int cin2, const float* bias, float* out, int cout) {
    WinoArgs a;
    a.in = in; a.u = u; a.in2 = in2; a.u2 = u2; a.bias = bias; a.out = out;
    a.cin = cin; a.cin2 = cin2; a.cout = cout; a.T = n->T; a.S = n->S; a.WP = n->WP; a.PP = n->PP;
    a.ntiles = batch * n->T * n->T;
    const int ntb = (a.ntiles + 31) / 32;
    const int ngrp8 = (((ntb + 3) / 4) + 7) / 8 * 8;      // tile-block groups, padded to the 8-XCD interleave
    hipLaunchKernelGGL(af_conv_wino, dim3(ngrp8 * (cout / 32)), dim3(256), 0, st, a);
}
// block i of the fp32 path, in -> act[kO + 2 * i]: conv1 3x3 + ELU (network.py:54); conv2 3x3 (+) 1x1 projection, add, ELU (network.py:53,55,56)
static void launch_wino_block(hipStream_t st, const af_net* n, int batch, int i, const float* in) {
    const NetBlock& b = kBlocks[i];
    float *g = n->act[kG + 2 * i], *o = n->act[kO + 2 * i];
    launch_wino(st, n, batch, in, n->w[kWino1 + i], b.cin, nullptr, nullptr, 0, n->w[kConv1B + i], g, b.cout);
    launch_wino(st, n, batch, g, n->w[kWino2 + i], b.cout, in, n->w[kWinoR + i], b.cin, n->w[kSumB + i], o, b.cout);
}

// the fp32 heads, on the fp32 planes [batch][32][PP] a branch ends in
static void launch_value_head(hipStream_t st, const af_net* n, int batch, const float* o3, float* value) {
    hipLaunchKernelGGL(af_value_head, dim3((batch + VPB - 1) / VPB), dim3(256), 0, st, o3, n->w[kVcW], n->w[kVcB], n->w[kV1W], n->w[kV1B],
                       n->w[kV2W], n->w[kV2B], value, batch, n->S, n->WP, n->PP);
}
// boards up to 11x11: af_policy_head_mfma (16 positions per workgroup) or, with af_net_tune(5, 0), the VALU head at 8; larger boards: the VALU head at 4
static void launch_policy_head(hipStream_t st, const af_net* n, int batch, const float* o5, float* policy) {
    const int HW = n->HW, K = 16 * HW, KS = K + ((2 - K % 32) + 32) % 32;
    const bool mfma = HW <= 128 && g_tune.phead;
    const int ppb = mfma ? 16 : HW <= 128 ? 8 : 4;
    const size_t lds = mfma ? (size_t)16 * KS * 4 : ((size_t)16 * HW * ppb + 512 + 4 * ppb) * 4;
    const auto head = mfma ? af_policy_head_mfma : HW <= 128 ? af_policy_head<8> : af_policy_head<4>;
    hipLaunchKernelGGL(head, dim3((batch + ppb - 1) / ppb), dim3(256), lds, st, o5, n->w[kPcW], n->w[kPcB], n->w[kPfW], n->w[kPfB], policy,
                       batch, n->S, n->WP, n->PP);
}

// The value branch (block3 + head) only depends on the trunk output o2: on the handle's side stream it runs concurrently with the
// policy branch (blocks 4,5 + head), filling the SIMDs the 32/64-wide layers leave idle.  vs is the value branch's stream: with
// vs == st there is no side stream and nothing to do.  The fork, behind the trunk:
static int fork_value(af_net* n, hipStream_t st, hipStream_t vs) {
    if (vs != st) { NET_HIP_OK(hipEventRecord(n->ev_trunk, st)); NET_HIP_OK(hipStreamWaitEvent(vs, n->ev_trunk, 0)); }
    return AF_NET_OK;
}
// ... and the join: the record behind the value branch's last launch; the wait behind the policy branch's, which ends the forward
static int value_done(af_net* n, hipStream_t st, hipStream_t vs) { if (vs != st) NET_HIP_OK(hipEventRecord(n->ev_value, vs)); return AF_NET_OK; }
static int join_value(af_net* n, hipStream_t st, hipStream_t vs) {
    if (vs != st) NET_HIP_OK(hipStreamWaitEvent(st, n->ev_value, 0));
    NET_HIP_OK(hipGetLastError());        // every launch of the forward
    return AF_NET_OK;
}

// fp32 Winograd path: stem, five blocks, both fp32 heads
static int forward_wino(af_net* n, hipStream_t st, const float* planes, int batch, float* policy, float* value) {
    float *f0 = n->act[kF0], *o1 = n->act[kO], *o2 = n->act[kO + 2], *o3 = n->act[kO + 4], *o4 = n->act[kO + 6], *o5 = n->act[kO + 8];   // block1 .. block5's outputs
    hipLaunchKernelGGL(af_stem_conv, dim3(batch), dim3(256), 0, st, planes, n->w[kStemW], n->w[kStemB], f0, n->S, n->WP, n->PP);
    launch_wino_block(st, n, batch, 0, f0);
    launch_wino_block(st, n, batch, 1, o1);
    const hipStream_t vs = g_tune.branch ? n->branch_stream : st;
    if (const int rc = fork_value(n, st, vs)) return rc;
    launch_wino_block(vs, n, batch, 2, o2);
    launch_value_head(vs, n, batch, o3, value);
    if (const int rc = value_done(n, st, vs)) return rc;
    launch_wino_block(st, n, batch, 3, o2);
    launch_wino_block(st, n, batch, 4, o4);
    launch_policy_head(st, n, batch, o5, policy);
    return join_value(n, st, vs);
}

// fp16 split-operand path (af_conv_f16s.hip)
static int forward_f16s(af_net* n, hipStream_t st, const float* planes, int batch, float* policy, float* value) {
    const bool fhead = g_tune.fhead;        // heads fused into the path; otherwise the branches end in o3 / o5 for the fp32 head kernels
    const F16sPlan plan = f16s_plan(n->f16s, batch, g_tune.f16s_bits, fhead);
    // 11x11 with fused heads: <= 8 positions as one launch of dataflow roles instead of nine dependent launches (r6); otherwise the
    // trunk, then both branches paired on this stream (fork and join of a side stream cost more than the value branch's kernels)
    if (plan.form != kF16sBranches) return f16s_forward(n->f16s, plan, st, planes, value, policy) ? AF_NET_ERR_HIP : AF_NET_OK;
    float *o3 = n->act[kO + 4], *o5 = n->act[kO + 8];
    if (f16s_trunk(n->f16s, plan, st, planes)) return AF_NET_ERR_HIP;
    // (r5: on this path the side stream is used by neither board size any more — 11x11 runs the value branch as workgroup classes of the
    //  policy branch's launches (kF16sPaired above); 15x15 serialised is 0.7 % faster than forked, 2.653 vs 2.672 ms: fork and join cost
    //  more than the tail filling returns.  af_net_tune(4, 2) forces the side stream for A/B.)
    const hipStream_t vs = g_tune.branch == 2 ? n->branch_stream : st;
    if (const int rc = fork_value(n, st, vs)) return rc;
    if (f16s_value_branch(n->f16s, plan, vs, o3, n->WP, n->PP, value)) return AF_NET_ERR_HIP;
    if (!fhead) launch_value_head(vs, n, batch, o3, value);
    if (const int rc = value_done(n, st, vs)) return rc;
    if (f16s_policy_branch(n->f16s, plan, st, o5, n->WP, n->PP, policy)) return AF_NET_ERR_HIP;
    if (!fhead) launch_policy_head(st, n, batch, o5, policy);
    return join_value(n, st, vs);
}

extern "C" {

int af_net_forward(af_net* n, void* stream, const float* planes, int32_t batch, float* policy, float* value) {
    if (!n || !planes || !policy || !value || batch < 1 || batch > n->max_batch) return AF_NET_ERR_ARG;
    if (!n->ready) return AF_NET_ERR_STATE;
    // (r1-r5 A/B records, removed from the source in r6: concurrent sub-batches on side streams and sequential sub-batches that keep a
    //  layer's output inside the Infinity Cache — 1.415 / 1.621 ms per 4096 positions as 2 / 4 sub-batches against 1.330: profiles/r5_41)
    if (g_tune.conv == 5 && n->f16s) return forward_f16s(n, (hipStream_t)stream, planes, batch, policy, value);
    return forward_wino(n, (hipStream_t)stream, planes, batch, policy, value);      // (also: board sizes without the split-operand path)
}

int af_net_debug_activation(af_net* n, int32_t which, int32_t batch, float* host_out) {
    if (!n || !host_out) return AF_NET_ERR_ARG;
    if (which >= 16) {       // the fp32 planes act[]: 16 + i the interior [batch][C][S*S], 32 + i the buffer as stored [batch][C][PP]
        const bool stored = which >= 32;
        const int i = which - (stored ? 32 : 16);
        if (i >= kActs || batch < 1 || batch > n->max_batch) return AF_NET_ERR_ARG;
        const int C = act_channels(i), S = n->S, WP = n->WP, PP = n->PP;
        const size_t count = (size_t)batch * C * PP;
        NET_HIP_OK(hipSetDevice(n->device));
        NET_HIP_OK(hipDeviceSynchronize());
        if (stored) { NET_HIP_OK(hipMemcpy(host_out, n->act[i], count * sizeof(float), hipMemcpyDeviceToHost)); return C; }
        std::vector<float> h(count);
        NET_HIP_OK(hipMemcpy(h.data(), n->act[i], count * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t bc = 0; bc < (size_t)batch * C; ++bc)
            for (int y = 0; y < S; ++y) memcpy(host_out + (bc * S + y) * S, h.data() + bc * PP + (y + 1) * WP + 1, S * sizeof(float));
        return C;
    }
    if (!n->f16s) return AF_NET_ERR_ARG;
    const int c = f16s_read_activation(n->f16s, which, batch, host_out);
    return c < 0 ? AF_NET_ERR_ARG : c;
}

int af_net_small_forward_error(af_net* n) {
    if (!n || !n->f16s) return AF_NET_ERR_ARG;
    return f16s_small_forward_error(n->f16s);
}

int64_t af_net_flops_per_position(const af_net* n) {
    const int64_t HW = n->HW;
    int64_t mac = 75 * 32 * HW;
    for (const NetBlock& b : kBlocks) mac += ((int64_t)9 * b.cin * b.cout + (int64_t)9 * b.cout * b.cout + (int64_t)b.cin * b.cout) * HW;
    mac += 32 * 4 * HW + 4 * HW * 64 + 64 + 32 * 16 * HW + 16 * HW * HW;
    return 2 * mac;
}

}  // extern "C"
