// libaf_sym.so (include/af_sym.h): the eight board symmetries around an evaluator, on the device — expand / reduce for the
// symmetry-averaged evaluation, apply / restore for one symmetry drawn per leaf.  Plain elementwise kernels: one thread per output
// element, a grid sized by the element count (a plane is at most 1 KB, so a permutation stays inside a few cache lines).
// The numpy statement they are held to bit for bit is alphafive_amd/symmetry.py.  Built with -ffp-contract=off: the sum of
// af_sym_reduce is seven additions and one multiplication as written, no fma.
#include <hip/hip_runtime.h>

#include <new>

#include "af_noise.h"
#include "af_sym.h"

#define SYM_HIP_OK(expr) do { if ((expr) != hipSuccess) return AF_SYM_ERR_HIP; } while (0)

struct af_sym {
    int S = 0, C = 0, max_batch = 0, device = 0;
    uint64_t seed = 0;
    void* state = nullptr;       // the handle's one allocation: the counter, then syms[max_batch]
    uint64_t* counter = nullptr;
    int32_t* syms = nullptr;
};

namespace {

constexpr int THREADS = 256;

// transform(a, s)[c] = a[source_cell(c, s)]: undo the flip, then undo the quarter turns.  Forward maps: one np.rot90 turn sends
// (i, j) -> (S-1-j, i); the flip sends (i, j) -> (S-1-i, j)  (the maps of af_replay_sample_kernel).
__device__ __forceinline__ int source_cell(int c, int s, int S) {
    int i = c / S, j = c - i * S;
    if (s >> 2) i = S - 1 - i;
    for (int t = 0; t < (s & 3); ++t) {
        const int ni = j, nj = S - 1 - i;
        i = ni; j = nj;
    }
    return i * S + j;
}

// inverse(a, s)[c] = a[image_cell(c, s)]: where transform(., s) sends cell c.
__device__ __forceinline__ int image_cell(int c, int s, int S) {
    int i = c / S, j = c - i * S;
    for (int t = 0; t < (s & 3); ++t) {
        const int ni = S - 1 - j, nj = i;
        i = ni; j = nj;
    }
    if (s >> 2) i = S - 1 - i;
    return i * S + j;
}

// planes8[8 b + s][p][c] = planes[b][p][source_cell(c, s)]
__global__ __launch_bounds__(THREADS) void af_sym_expand_kernel(const float* __restrict__ planes, float* __restrict__ planes8,
                                                                int S, int C, int total) {
    const int e = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (e >= total) return;
    const int c = e % C;
    const int rp = e / C;                 // (8 b + s) * 3 + p
    const int p = rp % 3;
    const int row = rp / 3;
    const int s = row & 7;
    const int b = row >> 3;
    planes8[e] = planes[(b * 3 + p) * C + source_cell(c, s, S)];
}

// Elements [0, B*C): policy[b][c] = (q_0 + q_1 + ... + q_7) * 0.125f in the order of s, q_s = policy8[8 b + s][image_cell(c, s)];
// elements [B*C, B*C + B): value[b] likewise over value8[8 b + s].
__global__ __launch_bounds__(THREADS) void af_sym_reduce_kernel(const float* __restrict__ policy8, const float* __restrict__ value8,
                                                                float* __restrict__ policy, float* __restrict__ value,
                                                                int S, int C, int batch) {
    const int e = (int)(blockIdx.x * THREADS + threadIdx.x);
    const int npol = batch * C;
    if (e < npol) {
        const int b = e / C;
        const int c = e - b * C;
        const float* src = policy8 + b * 8 * C;
        float acc = src[c];                                   // s = 0: the identity
        for (int s = 1; s < 8; ++s) acc = acc + src[s * C + image_cell(c, s, S)];
        policy[e] = acc * 0.125f;
    } else if (e < npol + batch) {
        const int b = e - npol;
        float acc = value8[8 * b];
        for (int s = 1; s < 8; ++s) acc = acc + value8[8 * b + s];
        value[b] = acc * 0.125f;
    }
}

// planes_t[b][p][c] = planes[b][p][source_cell(c, s_b)], s_b drawn from (b, the handle's counter, seed); the thread of a row's
// first element stores s_b.  Reads the counter, never writes it.
__global__ __launch_bounds__(THREADS) void af_sym_apply_kernel(const float* __restrict__ planes, float* __restrict__ planes_t,
                                                               const uint64_t* __restrict__ counter, int32_t* __restrict__ syms,
                                                               uint32_t seed_lo, uint32_t seed_hi, int S, int C, int total) {
    const int e = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (e >= total) return;
    const uint64_t ctr = *counter;
    const int c = e % C;
    const int rp = e / C;                 // b * 3 + p
    const int b = rp / 3;
    const af_u32x4 v = af_philox4x32((uint32_t)b, (uint32_t)ctr, (uint32_t)(ctr >> 32), AF_SYM_DRAW_TAG, seed_lo, seed_hi);
    const int s = (int)(v.v[0] >> 29);
    planes_t[e] = planes[rp * C + source_cell(c, s, S)];
    if (e == b * 3 * C) syms[b] = s;
}

// Elements [0, B*C): policy[b][c] = policy_t[b][image_cell(c, syms[b])]; elements [B*C, B*C + B): the value, if it has to move.
// Thread 0 advances the counter: the one write it ever gets outside af_sym_set_counter.
__global__ __launch_bounds__(THREADS) void af_sym_restore_kernel(const float* __restrict__ policy_t, const float* value_t,
                                                                 float* __restrict__ policy, float* value,
                                                                 const int32_t* __restrict__ syms, uint64_t* counter,
                                                                 int S, int C, int batch) {
    const int e = (int)(blockIdx.x * THREADS + threadIdx.x);
    const int npol = batch * C;
    if (e == 0) *counter = *counter + 1;
    if (e < npol) {
        const int b = e / C;
        const int c = e - b * C;
        policy[e] = policy_t[b * C + image_cell(c, syms[b] & 7, S)];
    } else if (e < npol + batch) {
        const int b = e - npol;
        if (value != value_t) value[b] = value_t[b];
    }
}

__global__ void af_sym_set_counter_kernel(uint64_t* counter, uint64_t value) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *counter = value;
}

inline unsigned blocks_for(int n) { return (unsigned)((n + THREADS - 1) / THREADS); }

}  // namespace

extern "C" {

int af_sym_abi_version(void) { return AF_SYM_ABI_VERSION; }

const char* af_sym_strerror(int code) {
    switch (code) {
        case AF_SYM_OK: return "ok";
        case AF_SYM_ERR_ARG: return "bad argument";
        case AF_SYM_ERR_HIP: return "HIP runtime error";
        default: return "unknown error";
    }
}

int af_sym_create(int32_t S, int32_t max_batch, int32_t device, uint64_t seed, af_sym** out) {
    if (!out || S < 3 || S > 16 || max_batch < 1) return AF_SYM_ERR_ARG;
    if ((int64_t)max_batch * 8 * 3 * S * S + THREADS > INT32_MAX) return AF_SYM_ERR_ARG;   // the kernels index elements in 32 bits
    SYM_HIP_OK(hipSetDevice(device));
    af_sym* h = new (std::nothrow) af_sym();
    if (!h) return AF_SYM_ERR_HIP;
    h->S = S; h->C = S * S; h->max_batch = max_batch; h->device = device; h->seed = seed;
    const size_t bytes = sizeof(uint64_t) + (size_t)max_batch * sizeof(int32_t);
    hipError_t e = hipMalloc(&h->state, bytes);
    if (e == hipSuccess) e = hipMemset(h->state, 0, bytes);
    if (e != hipSuccess) { af_sym_destroy(h); return AF_SYM_ERR_HIP; }
    h->counter = static_cast<uint64_t*>(h->state);
    h->syms = reinterpret_cast<int32_t*>(h->counter + 1);
    *out = h;
    return AF_SYM_OK;
}

void af_sym_destroy(af_sym* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->state) (void)hipFree(h->state);
    delete h;
}

// (every refusal that needs no field of the handle comes first: a null pointer, an aliased pair, batch < 1)
int af_sym_expand(af_sym* h, void* stream, const float* planes, float* planes8, int32_t batch) {
    if (!h || !planes || !planes8 || planes == planes8 || batch < 1) return AF_SYM_ERR_ARG;
    if (batch > h->max_batch) return AF_SYM_ERR_ARG;
    const int total = batch * 8 * 3 * h->C;
    af_sym_expand_kernel<<<blocks_for(total), THREADS, 0, static_cast<hipStream_t>(stream)>>>(planes, planes8, h->S, h->C, total);
    SYM_HIP_OK(hipGetLastError());
    return AF_SYM_OK;
}

int af_sym_reduce(af_sym* h, void* stream, const float* policy8, const float* value8, float* policy, float* value, int32_t batch) {
    if (!h || !policy8 || !value8 || !policy || !value || policy8 == policy || value8 == value || batch < 1) return AF_SYM_ERR_ARG;
    if (batch > h->max_batch) return AF_SYM_ERR_ARG;
    const int total = batch * (h->C + 1);
    af_sym_reduce_kernel<<<blocks_for(total), THREADS, 0, static_cast<hipStream_t>(stream)>>>(policy8, value8, policy, value,
                                                                                              h->S, h->C, batch);
    SYM_HIP_OK(hipGetLastError());
    return AF_SYM_OK;
}

int af_sym_apply(af_sym* h, void* stream, const float* planes, float* planes_t, int32_t batch) {
    if (!h || !planes || !planes_t || planes == planes_t || batch < 1) return AF_SYM_ERR_ARG;
    if (batch > h->max_batch) return AF_SYM_ERR_ARG;
    const int total = batch * 3 * h->C;
    af_sym_apply_kernel<<<blocks_for(total), THREADS, 0, static_cast<hipStream_t>(stream)>>>(
        planes, planes_t, h->counter, h->syms, (uint32_t)h->seed, (uint32_t)(h->seed >> 32), h->S, h->C, total);
    SYM_HIP_OK(hipGetLastError());
    return AF_SYM_OK;
}

int af_sym_restore(af_sym* h, void* stream, const float* policy_t, const float* value_t, float* policy, float* value, int32_t batch) {
    if (!h || !policy_t || !value_t || !policy || !value || policy_t == policy || batch < 1) return AF_SYM_ERR_ARG;
    if (batch > h->max_batch) return AF_SYM_ERR_ARG;
    const int total = batch * (h->C + 1);
    af_sym_restore_kernel<<<blocks_for(total), THREADS, 0, static_cast<hipStream_t>(stream)>>>(policy_t, value_t, policy, value,
                                                                                               h->syms, h->counter, h->S, h->C, batch);
    SYM_HIP_OK(hipGetLastError());
    return AF_SYM_OK;
}

int af_sym_set_counter(af_sym* h, void* stream, uint64_t counter) {
    if (!h) return AF_SYM_ERR_ARG;
    af_sym_set_counter_kernel<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(h->counter, counter);
    SYM_HIP_OK(hipGetLastError());
    return AF_SYM_OK;
}

int af_sym_state(af_sym* h, void* stream, uint64_t* counter, int32_t* syms_host, int32_t cap) {
    if (!h || cap < 0) return AF_SYM_ERR_ARG;
    SYM_HIP_OK(hipSetDevice(h->device));
    SYM_HIP_OK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    if (counter) SYM_HIP_OK(hipMemcpy(counter, h->counter, sizeof(uint64_t), hipMemcpyDeviceToHost));
    const int n = cap < h->max_batch ? cap : h->max_batch;
    if (syms_host && n > 0) SYM_HIP_OK(hipMemcpy(syms_host, h->syms, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return AF_SYM_OK;
}

}  // extern "C"
