// af_train.hip — the trainer's fused kernels (C ABI and the arithmetic, operator by operator: include/af_train.h).
// Three launches around torch.autograd.grad: the loss head with its gradient (one wavefront per row, the row stays in
// registers), Adam over every variable with the L2 gradient and the L2 sum folded in (table by value in the kernel arguments),
// and the reduction of the logged scalars.  Built with -ffp-contract=off; wave64, gfx950; no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "af_train.h"

#define TR_HIP_OK(expr)                                     \
    do {                                                    \
        hipError_t err_ = (expr);                           \
        if (err_ != hipSuccess) return AF_TRAIN_ERR_HIP;    \
    } while (0)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxPerLane = AF_TRAIN_MAX_C / 64;                    // at most 16 logits of a row per lane
constexpr int kPerThread = AF_TRAIN_ADAM_CHUNK / kThreads;          // 8 elements of a chunk per thread
static_assert(kMaxPerLane == 16 && AF_TRAIN_ADAM_CHUNK % kThreads == 0, "tile sizes");

// butterfly: every lane ends with the same bits (a + b == b + a), whatever the lane
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}

// all 256 threads call it; the four waves are added in order
template <typename T>
__device__ __forceinline__ T block_sum(T x, T* lds) {
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    const T r = ((lds[0] + lds[1]) + lds[2]) + lds[3];
    __syncthreads();
    return r;
}

struct LossArgs {
    const float *logits, *value, *pi, *winner, *weight;
    float *dlogits, *dvalue;
    double* row_terms;
    int B, C;
};

// kPerLane: logits of a row per lane, C <= 64 * kPerLane (the host picks the smallest power of two that holds the row, so the
// 121-cell board runs the 2-per-lane kernel, not one that keeps 16 slots and their exp() live).
// The arithmetic is fp64 from the loaded fp32 values to the one rounding of each stored fp32 result: a row is a few hundred
// elements, so the wider exp/log cost nothing that shows, and the logged scalars and gradients carry the rounding of their own
// format only (a row of logits spread over +-40 has |logsm| up to 80: in fp32 every one of them would be off by up to 4e-6).
template <int kPerLane>
__global__ __launch_bounds__(kThreads) void af_train_loss_head_kernel(LossArgs A) {
    const int lane = threadIdx.x & 63, row = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
    if (row >= A.B) return;                                         // whole waves leave; nothing below synchronises the block
    const int C = A.C;
    const float* z = A.logits + (size_t)row * C;
    const float* pi = A.pi + (size_t)row * C;
    double zr[kPerLane], pr[kPerLane], sr[kPerLane];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        const int c = lane + 64 * k;
        zr[k] = 0.0; pr[k] = 0.0; sr[k] = 0.0;
        if (c < C) {
            const float zc = z[c];
            zr[k] = (double)zc;
            pr[k] = (double)pi[c];
            mx = fmaxf(mx, zc);
        }
    }
    const double dmx = (double)wave_max(mx);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k)
        if (lane + 64 * k < C) {
            zr[k] = zr[k] - dmx;
            s = s + exp(zr[k]);
        }
    const double lse = log(wave_sum(s));
    double xent = 0.0, ent = 0.0, psum = 0.0;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k)
        if (lane + 64 * k < C) {
            zr[k] = zr[k] - lse;                                    // logsm
            sr[k] = exp(zr[k]);
            xent = xent + pr[k] * zr[k];
            ent = ent + sr[k] * zr[k];
            psum = psum + pr[k];
        }
    xent = wave_sum(xent);
    ent = wave_sum(ent);
    psum = wave_sum(psum);
    const double w = (double)A.weight[row], dB = (double)A.B;
    const double wb = w / dB;
    float* dl = A.dlogits + (size_t)row * C;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k)
        if (lane + 64 * k < C) dl[lane + 64 * k] = (float)(-wb * (pr[k] - sr[k] * psum));
    if (lane == 0) {
        const double d = (double)A.value[row] - (double)A.winner[row], vsq = d * d;
        A.dvalue[row] = (float)(((4.0 * w) / dB) * d);
        double* t = A.row_terms + (size_t)row * AF_TRAIN_ROW_TERMS;
        t[0] = w * xent;
        t[1] = w * vsq;
        t[2] = xent;
        t[3] = vsq;
        t[4] = -ent;
    }
}

// the table of one launch, by value in the kernel-argument segment (2.6 KB of the 4 KB there are)
struct AdamTable {
    float* p[AF_TRAIN_MAX_VARS];
    const float* g[AF_TRAIN_MAX_VARS];
    float* m[AF_TRAIN_MAX_VARS];
    float* v[AF_TRAIN_MAX_VARS];
    int32_t n[AF_TRAIN_MAX_VARS];
    int32_t first[AF_TRAIN_MAX_VARS + 1];       // first chunk (= workgroup) of variable k; first[nvars] = the grid
    uint32_t decay[AF_TRAIN_MAX_VARS / 32];     // bit k: variable k is under the L2 penalty
    int32_t nvars;
};

__global__ __launch_bounds__(kThreads) void af_train_adam_kernel(AdamTable T, float lr_t, float beta1, float beta2, float eps,
                                                                 float l2_coef, float* l2_partials) {
    __shared__ float lds[kWaves];
    const int w = (int)blockIdx.x;
    int lo = 0, hi = T.nvars;                   // first[lo] <= w, and hi == nvars or first[hi] > w; w < first[nvars] by the grid
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (T.first[mid] <= w) lo = mid; else hi = mid;
    }
    const int k = lo;
    float* const p = T.p[k];
    const float* const g = T.g[k];
    float* const m = T.m[k];
    float* const v = T.v[k];
    const int n = T.n[k];
    const bool decay = (T.decay[k >> 5] >> (k & 31)) & 1u;
    const float c1 = 1.0f - beta1, c2 = 1.0f - beta2;
    const int64_t base = (int64_t)(w - T.first[k]) * AF_TRAIN_ADAM_CHUNK + threadIdx.x;
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int64_t i = base + (int64_t)j * kThreads;
        if (i < n) {
            const float pi = p[i];
            float gi = g[i];
            if (decay) {
                gi = gi + l2_coef * pi;
                acc = acc + pi * pi;
            }
            const float mi = m[i] * beta1 + gi * c1;
            const float vi = v[i] * beta2 + (gi * gi) * c2;
            m[i] = mi;
            v[i] = vi;
            p[i] = pi - (lr_t * mi) / (sqrtf(vi) + eps);
        }
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) l2_partials[w] = acc;                    // 0 for a variable without decay
}

struct FinalizeArgs {
    const double* row_terms;
    const float* l2_partials;
    float* terms;
    int B, n_partials;
    float l2_coef;
};

__global__ __launch_bounds__(kThreads) void af_train_finalize_kernel(FinalizeArgs A) {
    __shared__ double lds[kWaves];
    double s[AF_TRAIN_ROW_TERMS];
#pragma unroll
    for (int j = 0; j < AF_TRAIN_ROW_TERMS; ++j) {
        double a = 0.0;
        for (int b = threadIdx.x; b < A.B; b += kThreads) a = a + A.row_terms[(size_t)b * AF_TRAIN_ROW_TERMS + j];
        s[j] = block_sum(a, lds);
    }
    double a = 0.0;
    for (int i = threadIdx.x; i < A.n_partials; i += kThreads) a = a + (double)A.l2_partials[i];
    const double L = block_sum(a, lds);
    if (threadIdx.x == 0) {
        const double dB = (double)A.B;
        A.terms[0] = (float)((-(s[0] / dB) + 2.0 * (s[1] / dB)) + (double)A.l2_coef * (L / 2.0));
        A.terms[1] = (float)(-(s[2] / dB));
        A.terms[2] = (float)(s[3] / dB);
        A.terms[3] = (float)(s[4] / dB);
    }
}

// chunks of a variable of n elements; n checked by the caller
inline int64_t chunks_of(int64_t n) { return (n + AF_TRAIN_ADAM_CHUNK - 1) / AF_TRAIN_ADAM_CHUNK; }

}  // namespace

extern "C" {

int af_train_loss_head(void* stream, int32_t B, int32_t C, const float* logits, const float* value, const float* pi,
                       const float* winner, const float* weight, float* dlogits, float* dvalue, double* row_terms) {
    if (B < 1 || C < 1 || !logits || !value || !pi || !winner || !weight || !dlogits || !dvalue || !row_terms)
        return AF_TRAIN_ERR_ARG;
    if (C > AF_TRAIN_MAX_C) return AF_TRAIN_ERR_RANGE;
    LossArgs A{logits, value, pi, winner, weight, dlogits, dvalue, row_terms, B, C};
    const dim3 grid((unsigned)(((int64_t)B + kWaves - 1) / kWaves)), block(kThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (C <= 64) hipLaunchKernelGGL(af_train_loss_head_kernel<1>, grid, block, 0, st, A);
    else if (C <= 128) hipLaunchKernelGGL(af_train_loss_head_kernel<2>, grid, block, 0, st, A);
    else if (C <= 256) hipLaunchKernelGGL(af_train_loss_head_kernel<4>, grid, block, 0, st, A);
    else if (C <= 512) hipLaunchKernelGGL(af_train_loss_head_kernel<8>, grid, block, 0, st, A);
    else hipLaunchKernelGGL(af_train_loss_head_kernel<kMaxPerLane>, grid, block, 0, st, A);
    TR_HIP_OK(hipGetLastError());
    return AF_TRAIN_OK;
}

int af_train_adam_partials(int32_t nvars, const int64_t* n) {
    if (nvars < 0 || (nvars > 0 && !n)) return AF_TRAIN_ERR_ARG;
    int64_t total = 0;
    for (int k = 0; k < nvars; ++k) {
        if (n[k] < 0) return AF_TRAIN_ERR_ARG;
        if (n[k] > INT32_MAX) return AF_TRAIN_ERR_RANGE;
        total += chunks_of(n[k]);
        if (total > INT32_MAX) return AF_TRAIN_ERR_RANGE;
    }
    return (int)total;
}

int af_train_adam(void* stream, int32_t nvars, const af_train_var* vars, float lr_t, float beta1, float beta2, float eps,
                  float l2_coef, float* l2_partials) {
    if (nvars < 1 || nvars > AF_TRAIN_MAX_VARS || !vars || !l2_partials) return AF_TRAIN_ERR_ARG;
    AdamTable T = {};
    int64_t total = 0;
    for (int k = 0; k < nvars; ++k) {
        const af_train_var& a = vars[k];
        // an empty variable owns no chunk, so no workgroup ever reads its pointers: a zero-size buffer's may be null
        if (a.n < 0 || (a.n > 0 && (!a.p || !a.g || !a.m || !a.v))) return AF_TRAIN_ERR_ARG;
        if (a.n > INT32_MAX) return AF_TRAIN_ERR_RANGE;
        T.p[k] = a.p; T.g[k] = a.g; T.m[k] = a.m; T.v[k] = a.v;
        T.n[k] = (int32_t)a.n;
        T.first[k] = (int32_t)total;
        if (a.decay) T.decay[k >> 5] |= 1u << (k & 31);
        total += chunks_of(a.n);
        if (total > INT32_MAX) return AF_TRAIN_ERR_RANGE;
    }
    T.first[nvars] = (int32_t)total;
    T.nvars = nvars;
    if (total == 0) return 0;
    hipLaunchKernelGGL(af_train_adam_kernel, dim3((unsigned)total), dim3(kThreads), 0, static_cast<hipStream_t>(stream), T, lr_t,
                       beta1, beta2, eps, l2_coef, l2_partials);
    TR_HIP_OK(hipGetLastError());
    return (int)total;
}

int af_train_finalize(void* stream, int32_t B, const double* row_terms, int32_t n_partials, const float* l2_partials,
                      float l2_coef, float* terms) {
    if (B < 1 || !row_terms || n_partials < 0 || (n_partials > 0 && !l2_partials) || !terms) return AF_TRAIN_ERR_ARG;
    FinalizeArgs A{row_terms, l2_partials, terms, B, n_partials, l2_coef};
    hipLaunchKernelGGL(af_train_finalize_kernel, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), A);
    TR_HIP_OK(hipGetLastError());
    return AF_TRAIN_OK;
}

const char* af_train_strerror(int code) {
    switch (code) {
        case AF_TRAIN_OK: return "ok";
        case AF_TRAIN_ERR_ARG: return "bad argument";
        case AF_TRAIN_ERR_HIP: return "HIP runtime error";
        case AF_TRAIN_ERR_RANGE: return "size out of range";
        default: return "unknown error";
    }
}

}  // extern "C"
