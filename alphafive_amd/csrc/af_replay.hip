// af_replay.hip — device-resident replay ring + get_data gather/augmentation kernel (C ABI: include/af_replay.h).
// HBM-bound byte/index work: per sample the kernel reads 121 B of board + 484 B of policy and writes 1452 B of
// planes + 484 B of policy (2.5 KB of algorithmic traffic per sample), one 256-thread workgroup per sample.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "af_noise.h"
#include "af_replay.h"

#define RP_HIP_OK(expr)                                      \
    do {                                                     \
        hipError_t err_ = (expr);                            \
        if (err_ != hipSuccess) return AF_REPLAY_ERR_HIP;    \
    } while (0)

struct af_replay {
    int S = 0, C = 0, cap = 0, device = 0;
    int64_t head = 0;            // physical slot of the oldest position
    int count = 0;
    int8_t* boards = nullptr;    // [cap][C]
    float* policies = nullptr;   // [cap][C]
    int32_t* last = nullptr;     // [cap]
    float* values = nullptr;     // [cap]
    float* weights = nullptr;    // [cap]
    int32_t* sel = nullptr;      // [3][sel_cap] device copy of (slot, quarter turns, flip)
    int sel_cap = 0;
    void* pinned = nullptr;      // staging for append / sample arguments
    size_t pinned_bytes = 0;
    float* wtab = nullptr;       // [max_T + 1][max_T] construct_weights rows (af_replay_set_weights)
    int max_T = 0;
    int32_t* err = nullptr;      // device flags: [0] a packed append whose T did not match the buffer, [1] a malformed state string
    char* stage = nullptr;       // contiguous device block an export gathers into / a state-string append uploads its text to
    size_t stage_bytes = 0;
};

struct SampleArgs {
    const int8_t* boards;
    const float* policies;
    const int32_t* last;
    const float* values;
    const float* weights;
    const int32_t* sel;          // [3][num]: physical slot, quarter turns, flip
    float* out_boards;
    float* out_weights;
    float* out_values;
    float* out_policies;
    int S, C, num;
};

// Output cell (oi, oj) of the augmented board comes from source cell (si, sj): undo the flip, then undo k quarter
// turns.  Forward maps (utils.py:133-140): one np.rot90 turn sends (i, j) -> (S-1-j, i); the flip sends (i, j) -> (S-1-i, j).
__device__ __forceinline__ int source_cell(int oi, int oj, int k, int flip, int S) {
    int si = flip ? S - 1 - oi : oi, sj = oj;
    for (int t = 0; t < k; ++t) {
        const int ni = sj, nj = S - 1 - si;
        si = ni; sj = nj;
    }
    return si * S + sj;
}

__global__ __launch_bounds__(256) void af_replay_sample_kernel(SampleArgs A) {
    const int b = blockIdx.x;
    const int slot = A.sel[b], k = A.sel[A.num + b], flip = A.sel[2 * A.num + b];
    const int S = A.S, C = A.C;
    int la = A.last[slot];
    if (la >= 0) {                                     // forward map of the last move
        int i = la / S, j = la - i * S;
        for (int t = 0; t < k; ++t) {
            const int ni = S - 1 - j, nj = i;
            i = ni; j = nj;
        }
        if (flip) i = S - 1 - i;
        la = i * S + j;
    }
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const int oi = c / S, oj = c - oi * S;
        const int src = source_cell(oi, oj, k, flip, S);
        const int v = A.boards[(size_t)slot * C + src];
        float* ob = A.out_boards + (size_t)b * 3 * C;
        ob[c] = v == 1 ? 1.0f : 0.0f;                  // utils.py:256-272 board_to_inputs
        ob[C + c] = v == -1 ? 1.0f : 0.0f;
        ob[2 * C + c] = c == la ? 1.0f : 0.0f;
        A.out_policies[(size_t)b * C + c] = A.policies[(size_t)slot * C + src];
    }
    if (threadIdx.x == 0) {
        A.out_weights[b] = A.weights[slot];
        A.out_values[b] = A.values[slot];
    }
}

// Device-drawn minibatches (include/af_replay.h, af_replay_sample_device; the numpy statement the kernel is held to bit for bit
// is alphafive_amd/replay.py:draw_reference).  Logical position i of minibatch b owns the Philox4x32-10 block
//   v = af_philox4x32(i, b, draw, AF_REPLAY_DRAW_TAG, seed lo, seed hi):  v[0] = its sort word, v[1] >> 30 = quarter turns, v[2] >> 31 = flip,
// and the minibatch is the k positions with the smallest composite v[0] << 32 | i in ascending order.
struct DrawArgs {
    int32_t* sel;                // [3][total]: physical slot, quarter turns, flip (what af_replay_sample_kernel reads)
    int32_t* draws;              // [3][total]: logical index, quarter turns, flip; may be null
    int64_t head;
    uint32_t k0, k1, draw;
    int n, k, cap, total;        // n stored positions, k = samples per minibatch (1 <= k <= n, k <= AF_REPLAY_MAX_DRAW), total = batches * k
};

__device__ __forceinline__ af_u32x4 draw_block(const DrawArgs& A, uint32_t i, uint32_t b) {
    return af_philox4x32(i, b, A.draw, AF_REPLAY_DRAW_TAG, A.k0, A.k1);
}

// One 256-thread workgroup (4 waves) per minibatch; thread t owns positions t, t + 256, ...  Exact selection, nothing stored per
// position: the words are recomputed in every pass (~100 VALU operations each; at n = 12000 that is 47 per thread and pass).
//   1. radix select of the k-th smallest word T, 4 passes of 8 bits: LDS histogram of the digit among the words that match the
//      digits already fixed, then every wave finds the bin by a prefix over the 256 counts (lane l holds bins 4l .. 4l+3);
//   2. compaction of the composites into LDS: every word < T, and of the words == T the `need` lowest indices — all of them
//      when there are exactly `need` (then the order of arrival does not matter), else by rank in index order, 256 positions a round;
//   3. bitonic sort of next_pow2(k) composites, padded with all-ones;
//   4. entry j of the sorted array is sample j: one more Philox of the winner gives its turns and flip.
// Every index formed is bounded: positions by n, LDS slots by k <= AF_REPLAY_MAX_DRAW, bins by 256, outputs by total, slots by cap.
__global__ __launch_bounds__(256) void af_replay_draw_kernel(DrawArgs A) {
    __shared__ unsigned long long comp[AF_REPLAY_MAX_DRAW];      // 32 KB
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wave_hits[4];
    __shared__ uint32_t fill;
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = (uint32_t)A.n, k = (uint32_t)A.k;

    uint32_t T = 0, need = k, ties = 0;          // `need`: rank (from 1) of the wanted word among those matching the fixed digits of T
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t fixed = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
        hist[tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += 256) {
            const uint32_t w = draw_block(A, i, b).v[0];
            if ((w & fixed) == T) atomicAdd(&hist[(w >> shift) & 255u], 1u);
        }
        __syncthreads();
        const uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
        const uint32_t own = c0 + c1 + c2 + c3;
        uint32_t incl = own;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += up;
        }
        const unsigned long long reach = __ballot(incl >= need);         // never empty: at least `need` words match
        const int src = reach ? __ffsll(reach) - 1 : 63;
        uint32_t below = __shfl(incl - own, src), bin = 4u * (uint32_t)src;
        const uint32_t s0 = __shfl(c0, src), s1 = __shfl(c1, src), s2 = __shfl(c2, src), s3 = __shfl(c3, src);
        ties = s0;
        if (below + ties < need) {
            below += ties; ties = s1; ++bin;
            if (below + ties < need) {
                below += ties; ties = s2; ++bin;
                if (below + ties < need) { below += ties; ties = s3; ++bin; }
            }
        }
        T |= bin << shift;
        need -= below;
        __syncthreads();                                                 // the next pass clears the histogram
    }
    // now: k - need words are < T, `ties` words are == T, and need <= ties of those are wanted
    const uint32_t n_less = k - need;
    const bool all_ties = need >= ties;
    if (tid == 0) fill = 0;
    for (uint32_t j = tid; j < AF_REPLAY_MAX_DRAW; j += 256) comp[j] = ~0ull;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 256) {
        const uint32_t w = draw_block(A, i, b).v[0];
        if (w < T || (all_ties && w == T)) {
            const uint32_t pos = atomicAdd(&fill, 1u);
            if (pos < k) comp[pos] = ((unsigned long long)w << 32) | i;
        }
    }
    if (!all_ties) {                             // equal words at the threshold: the lowest indices win (block-uniform branch)
        uint32_t taken = 0;
        for (uint32_t i0 = 0; i0 < n && taken < need; i0 += 256) {
            const uint32_t i = i0 + tid;
            const bool hit = i < n && draw_block(A, i, b).v[0] == T;
            const unsigned long long m = __ballot(hit);
            if (lane == 0) wave_hits[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t rank = taken, round = 0;
            for (uint32_t w = 0; w < 4; ++w) {
                const uint32_t c = wave_hits[w];
                if (w < wave) rank += c;
                round += c;
            }
            rank += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (hit && rank < need) comp[n_less + rank] = ((unsigned long long)T << 32) | i;       // n_less + rank < k
            taken += round;
            __syncthreads();
        }
    }
    __syncthreads();

    uint32_t P = 1;
    while (P < k) P <<= 1;
    for (uint32_t size = 2; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < (P >> 1); t += 256) {
                const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;          // hi < P <= AF_REPLAY_MAX_DRAW
                const unsigned long long x = comp[lo], y = comp[hi];
                if ((x > y) == ((lo & size) == 0)) { comp[lo] = y; comp[hi] = x; }
            }
            __syncthreads();
        }
    }

    for (uint32_t j = tid; j < k; j += 256) {
        uint32_t i = (uint32_t)comp[j];
        if (i >= n) i = n - 1;                   // cannot happen: exactly k composites were placed
        const af_u32x4 v = draw_block(A, i, b);
        const size_t o = (size_t)b * k + j, total = (size_t)A.total;
        const int32_t turns = (int32_t)(v.v[1] >> 30), flip = (int32_t)(v.v[2] >> 31);
        A.sel[o] = (int32_t)((A.head + (int64_t)i) % A.cap);
        A.sel[total + o] = turns;
        A.sel[2 * total + o] = flip;
        if (A.draws) {
            A.draws[o] = (int32_t)i;
            A.draws[total + o] = turns;
            A.draws[2 * total + o] = flip;
        }
    }
}

// One workgroup per ply of episode `ep` of a packed hand-off buffer (layout: include/af_engine.h af_engine_pack_episodes:
// header {episodes, plies, K, C}, meta [max_eps][4] = {game, seq, T, first ply}, final values [max_eps], then per ply
// K u64 key words (mine bitboard, theirs bitboard) | C policy floats | C visit counts | last cell | action).
struct PackedArgs {
    const int32_t* buf;
    int8_t* boards;
    float* policies;
    int32_t* last;
    float* values;
    float* weights;
    const float* wtab;
    int32_t* err;
    int64_t slot0;               // ring slot of ply 0
    int cap, C, max_eps, ep, T, max_T;
};

__global__ __launch_bounds__(256) void af_replay_append_packed_kernel(PackedArgs A) {
    const int32_t* buf = A.buf;
    const int n_eps = buf[0], K = buf[2], Cc = buf[3];
    const int32_t* meta = buf + 4 + 4 * A.ep;
    const int T = meta[2], p0 = meta[3];
    if (A.ep >= n_eps || T != A.T || Cc != A.C) {                 // the host's view of the buffer is stale: append nothing
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicExch(A.err, 1);
        return;
    }
    const int t = blockIdx.x, R = 2 * K + 2 * Cc + 2, KW = K / 2;
    const int32_t* rec = buf + 4 + 5 * A.max_eps + (size_t)(p0 + t) * R;
    const int64_t slot = (A.slot0 + t) % A.cap;
    const uint32_t* key = reinterpret_cast<const uint32_t*>(rec);      // u64 word w = key[2w] | key[2w+1] << 32
    for (int c = threadIdx.x; c < Cc; c += blockDim.x) {
        const int w = c >> 6, b = c & 63;
        const uint32_t mine = key[2 * w + (b >> 5)] >> (b & 31), theirs = key[2 * (KW + w) + (b >> 5)] >> (b & 31);
        A.boards[slot * Cc + c] = (int8_t)((mine & 1u) ? 1 : ((theirs & 1u) ? -1 : 0));
        A.policies[slot * Cc + c] = __int_as_float(rec[2 * K + c]);
    }
    if (threadIdx.x == 0) {
        const float fv = __int_as_float(buf[4 + 4 * A.max_eps + A.ep]);
        float v = (T & 1) ? -fv : fv;                               // player.py:74-76, then the sign alternates ply by ply (:80-81)
        if (t & 1) v = -v;
        A.last[slot] = rec[2 * K + 2 * Cc];
        A.values[slot] = v;
        A.weights[slot] = A.wtab[(size_t)T * A.max_T + t];
    }
}

// One workgroup per exported position: gathers logical position `first + b` out of the five ring arrays into the contiguous
// staging block (the ring's wrap ends here) and writes its state string (utils.py:156-175: per row a run of c empties is
// 'a' + c, '3' mine, '1' theirs, '/' ends the row), NUL-terminated and NUL-padded to `stride` = S*(S+1) + 1 bytes.
struct ExportArgs {
    const int8_t* boards;
    const float* policies;
    const int32_t* last;
    const float* values;
    const float* weights;
    int8_t* out_boards;          // [n][C]
    float* out_policies;         // [n][C]
    int32_t* out_last;           // [n]
    float* out_values;           // [n]
    float* out_weights;          // [n]
    char* out_states;            // [n][stride]
    int64_t slot0;               // ring slot of the first exported position
    int cap, S, C, stride;
};

__global__ __launch_bounds__(256) void af_replay_export_kernel(ExportArgs A) {
    __shared__ int8_t cell[256];
    __shared__ char rowtxt[16][17];                   // a row of S cells is at most S characters + its '/'
    __shared__ int rowlen[16];
    const int b = blockIdx.x, S = A.S, C = A.C, tid = threadIdx.x;
    const int64_t slot = (A.slot0 + b) % A.cap;
    for (int c = tid; c < C; c += blockDim.x) {
        const int8_t v = A.boards[slot * C + c];
        cell[c] = v;
        A.out_boards[(size_t)b * C + c] = v;
        A.out_policies[(size_t)b * C + c] = A.policies[slot * C + c];
    }
    if (tid == 0) {
        A.out_last[b] = A.last[slot];
        A.out_values[b] = A.values[slot];
        A.out_weights[b] = A.weights[slot];
    }
    __syncthreads();
    if (tid < S) {                                    // one thread per row
        char* txt = rowtxt[tid];
        int len = 0, run = 0;
        for (int j = 0; j < S; ++j) {
            const int v = cell[tid * S + j];
            if (v == 0) { ++run; continue; }
            if (run) { txt[len++] = (char)('a' + run); run = 0; }
            txt[len++] = v > 0 ? '3' : '1';
        }
        if (run) txt[len++] = (char)('a' + run);
        txt[len++] = '/';
        rowlen[tid] = len;
    }
    __syncthreads();
    char* out = A.out_states + (size_t)b * A.stride;
    int total = 0, off = 0;
    for (int r = 0; r < S; ++r) {
        if (r == tid) off = total;
        total += rowlen[r];
    }
    if (tid < S)
        for (int i = 0; i < rowlen[tid]; ++i) out[off + i] = rowtxt[tid][i];
    for (int i = total + tid; i < A.stride; i += blockDim.x) out[i] = 0;      // total <= S*(S+1) < stride
}

// One workgroup per appended position: decodes its state string (utils.py:178-196 state_to_board) into the ring's int8 board.
// Everything derived from the text is checked before it indexes anything: a string that is not exactly S rows of exactly S
// cells in the alphabet above, NUL-terminated inside `stride`, raises err[1] and writes nothing.
struct StatesArgs {
    const char* states;          // [n][stride] (device staging)
    int8_t* boards;
    int32_t* err;
    int64_t slot0;               // ring slot of the first appended position
    int cap, S, C, stride;
};

__global__ __launch_bounds__(256) void af_replay_append_states_kernel(StatesArgs A) {
    __shared__ int8_t cell[256];
    __shared__ int good;
    const int b = blockIdx.x, S = A.S, C = A.C, tid = threadIdx.x;
    for (int c = tid; c < C; c += blockDim.x) cell[c] = 0;
    __syncthreads();
    if (tid == 0) {
        const char* s = A.states + (size_t)b * A.stride;
        int i = 0, j = 0, ok = 1, ended = 0;
        for (int p = 0; p < A.stride && ok; ++p) {
            const int ch = (unsigned char)s[p];
            if (ch == 0) { ended = 1; break; }
            if (i >= S) { ok = 0; break; }                        // text after the S-th row
            if (ch == '/') {
                if (j != S) ok = 0;                               // the row stops short of S cells
                ++i; j = 0;
            } else if (ch == '1' || ch == '3') {
                if (j >= S) { ok = 0; break; }
                cell[i * S + j] = (int8_t)(ch == '3' ? 1 : -1);
                ++j;
            } else if (ch > 'a' && ch <= 'a' + S) {
                if (j + (ch - 'a') > S) { ok = 0; break; }        // the run passes the end of the row
                j += ch - 'a';
            } else {
                ok = 0;
            }
        }
        good = ok && ended && i == S && j == 0;
        if (!good) atomicExch(A.err + 1, 1);
    }
    __syncthreads();
    if (!good) return;
    const int64_t slot = (A.slot0 + b) % A.cap;
    for (int c = tid; c < C; c += blockDim.x) A.boards[slot * C + c] = cell[c];
}

static int ensure_err(af_replay* r) {
    if (r->err) return AF_REPLAY_OK;
    RP_HIP_OK(hipMalloc(reinterpret_cast<void**>(&r->err), 8));
    RP_HIP_OK(hipMemset(r->err, 0, 8));
    return AF_REPLAY_OK;
}

static int ensure_stage(af_replay* r, size_t bytes) {
    if (bytes <= r->stage_bytes) return AF_REPLAY_OK;
    if (r->stage) (void)hipFree(r->stage);
    r->stage = nullptr; r->stage_bytes = 0;
    RP_HIP_OK(hipMalloc(reinterpret_cast<void**>(&r->stage), bytes));
    r->stage_bytes = bytes;
    return AF_REPLAY_OK;
}

static int ensure_pinned(af_replay* r, size_t bytes) {
    if (bytes <= r->pinned_bytes) return AF_REPLAY_OK;
    if (r->pinned) (void)hipHostFree(r->pinned);
    r->pinned = nullptr; r->pinned_bytes = 0;
    RP_HIP_OK(hipHostMalloc(&r->pinned, bytes, hipHostMallocDefault));
    r->pinned_bytes = bytes;
    return AF_REPLAY_OK;
}

static int ensure_sel(af_replay* r, int n) {
    if (n <= r->sel_cap) return AF_REPLAY_OK;
    if (r->sel) (void)hipFree(r->sel);
    r->sel = nullptr; r->sel_cap = 0;
    RP_HIP_OK(hipMalloc(reinterpret_cast<void**>(&r->sel), (size_t)3 * n * 4));
    r->sel_cap = n;
    return AF_REPLAY_OK;
}

// af_replay_sample_kernel over the first `num` triples of r->sel
static int launch_sample(af_replay* r, hipStream_t st, int num, float* boards_dev, float* weights_dev, float* values_dev, float* policies_dev) {
    SampleArgs a;
    a.boards = r->boards; a.policies = r->policies; a.last = r->last; a.values = r->values; a.weights = r->weights;
    a.sel = r->sel; a.out_boards = boards_dev; a.out_weights = weights_dev; a.out_values = values_dev; a.out_policies = policies_dev;
    a.S = r->S; a.C = r->C; a.num = num;
    hipLaunchKernelGGL(af_replay_sample_kernel, dim3(num), dim3(256), 0, st, a);
    RP_HIP_OK(hipGetLastError());
    return AF_REPLAY_OK;
}

// n positions into the slots behind the tail (host pointers; `boards` may be null: af_replay_append_states decodes them on the
// device).  The ring wraps: copy in up to two runs.  `count` is the caller's to move.
static int copy_in(af_replay* r, hipStream_t st, int n, const int8_t* boards, const float* policies, const int32_t* last_cell,
                   const float* values, const float* weights) {
    const size_t C = r->C;
    int done = 0;
    while (done < n) {
        const int64_t slot = (r->head + r->count + done) % r->cap;
        const int run = (int)((int64_t)(n - done) < r->cap - slot ? (n - done) : r->cap - slot);
        if (boards) RP_HIP_OK(hipMemcpyAsync(r->boards + slot * C, boards + (size_t)done * C, (size_t)run * C, hipMemcpyHostToDevice, st));
        RP_HIP_OK(hipMemcpyAsync(r->policies + slot * C, policies + (size_t)done * C, (size_t)run * C * 4, hipMemcpyHostToDevice, st));
        RP_HIP_OK(hipMemcpyAsync(r->last + slot, last_cell + done, (size_t)run * 4, hipMemcpyHostToDevice, st));
        RP_HIP_OK(hipMemcpyAsync(r->values + slot, values + done, (size_t)run * 4, hipMemcpyHostToDevice, st));
        RP_HIP_OK(hipMemcpyAsync(r->weights + slot, weights + done, (size_t)run * 4, hipMemcpyHostToDevice, st));
        done += run;
    }
    return AF_REPLAY_OK;
}

extern "C" {

const char* af_replay_strerror(int code) {
    switch (code) {
        case AF_REPLAY_OK: return "ok";
        case AF_REPLAY_ERR_ARG: return "bad argument";
        case AF_REPLAY_ERR_HIP: return "HIP runtime error";
        case AF_REPLAY_ERR_FULL: return "replay ring full";
        case AF_REPLAY_ERR_RANGE: return "index outside the stored positions";
        case AF_REPLAY_ERR_FORMAT: return "malformed state string";
        default: return "unknown error";
    }
}

int af_replay_create(int32_t S, int32_t capacity, int32_t device, af_replay** out) {
    if (!out || S < 3 || S > 16 || capacity < 1) return AF_REPLAY_ERR_ARG;
    RP_HIP_OK(hipSetDevice(device));
    af_replay* r = new af_replay();
    r->S = S; r->C = S * S; r->cap = capacity; r->device = device;
    const size_t n = (size_t)capacity;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&r->boards), n * r->C);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->policies), n * r->C * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->last), n * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->values), n * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->weights), n * 4);
    if (e != hipSuccess) { af_replay_destroy(r); return AF_REPLAY_ERR_HIP; }
    *out = r;
    return AF_REPLAY_OK;
}

void af_replay_destroy(af_replay* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->boards) (void)hipFree(r->boards);
    if (r->policies) (void)hipFree(r->policies);
    if (r->last) (void)hipFree(r->last);
    if (r->values) (void)hipFree(r->values);
    if (r->weights) (void)hipFree(r->weights);
    if (r->sel) (void)hipFree(r->sel);
    if (r->wtab) (void)hipFree(r->wtab);
    if (r->err) (void)hipFree(r->err);
    if (r->stage) (void)hipFree(r->stage);
    if (r->pinned) (void)hipHostFree(r->pinned);
    delete r;
}

int32_t af_replay_size(const af_replay* r) { return r ? r->count : 0; }

int af_replay_drop_front(af_replay* r, int32_t n) {
    if (!r || n < 0) return AF_REPLAY_ERR_ARG;
    if (n > r->count) return AF_REPLAY_ERR_RANGE;
    r->head = (r->head + n) % r->cap;
    r->count -= n;
    return AF_REPLAY_OK;
}

int af_replay_append(af_replay* r, void* stream, int32_t n, const int8_t* boards, const float* policies,
                     const int32_t* last_cell, const float* values, const float* weights) {
    if (!r || n < 0 || (n > 0 && (!boards || !policies || !last_cell || !values || !weights))) return AF_REPLAY_ERR_ARG;
    if (n == 0) return AF_REPLAY_OK;
    if (r->count + n > r->cap) return AF_REPLAY_ERR_FULL;
    RP_HIP_OK(hipSetDevice(r->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = copy_in(r, st, n, boards, policies, last_cell, values, weights);
    if (rc) return rc;
    RP_HIP_OK(hipStreamSynchronize(st));               // pageable host memory: the caller may reuse its arrays on return
    r->count += n;
    return AF_REPLAY_OK;
}

int32_t af_replay_state_stride(const af_replay* r) { return r ? r->S * (r->S + 1) + 1 : 0; }

int af_replay_append_states(af_replay* r, void* stream, int32_t n, const char* states, int32_t state_stride, const float* policies,
                            const int32_t* last_cell, const float* values, const float* weights) {
    if (!r || n < 0 || (n > 0 && (!states || state_stride < 1 || !policies || !last_cell || !values || !weights))) return AF_REPLAY_ERR_ARG;
    if (n == 0) return AF_REPLAY_OK;
    if (r->count + n > r->cap) return AF_REPLAY_ERR_FULL;
    RP_HIP_OK(hipSetDevice(r->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = ensure_err(r);
    if (!rc) rc = ensure_stage(r, (size_t)n * state_stride);
    if (rc) return rc;
    // everything lands in slots behind the tail, which hold nothing until `count` moves: a rejected call leaves the ring as it was
    RP_HIP_OK(hipMemcpyAsync(r->stage, states, (size_t)n * state_stride, hipMemcpyHostToDevice, st));
    rc = copy_in(r, st, n, nullptr, policies, last_cell, values, weights);
    if (rc) return rc;
    StatesArgs a;
    a.states = r->stage; a.boards = r->boards; a.err = r->err; a.slot0 = (r->head + r->count) % r->cap;
    a.cap = r->cap; a.S = r->S; a.C = r->C; a.stride = state_stride;
    hipLaunchKernelGGL(af_replay_append_states_kernel, dim3(n), dim3(256), 0, st, a);
    RP_HIP_OK(hipGetLastError());
    int32_t bad = 0;
    RP_HIP_OK(hipMemcpyAsync(&bad, r->err + 1, 4, hipMemcpyDeviceToHost, st));
    RP_HIP_OK(hipStreamSynchronize(st));               // pageable host memory: the caller may reuse its arrays on return
    if (bad) {
        RP_HIP_OK(hipMemset(r->err + 1, 0, 4));
        return AF_REPLAY_ERR_FORMAT;
    }
    r->count += n;
    return AF_REPLAY_OK;
}

int af_replay_export(af_replay* r, void* stream, int32_t first, int32_t n, char* states, int8_t* boards, float* policies,
                     int32_t* last_cell, float* values, float* weights) {
    if (!r || first < 0 || n < 0 || (n > 0 && (!policies || !last_cell || !values || !weights))) return AF_REPLAY_ERR_ARG;
    if ((int64_t)first + n > r->count) return AF_REPLAY_ERR_RANGE;
    if (n == 0) return AF_REPLAY_OK;
    RP_HIP_OK(hipSetDevice(r->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t C = r->C, N = n, stride = (size_t)af_replay_state_stride(r);
    // staging layout: policies | last | values | weights | boards | states (the 4-byte arrays first, so all stay aligned)
    const int rc = ensure_stage(r, N * (C * 4 + 12 + C + stride));
    if (rc) return rc;
    ExportArgs a;
    a.boards = r->boards; a.policies = r->policies; a.last = r->last; a.values = r->values; a.weights = r->weights;
    a.out_policies = reinterpret_cast<float*>(r->stage);
    a.out_last = reinterpret_cast<int32_t*>(a.out_policies + N * C);
    a.out_values = reinterpret_cast<float*>(a.out_last + N);
    a.out_weights = a.out_values + N;
    a.out_boards = reinterpret_cast<int8_t*>(a.out_weights + N);
    a.out_states = reinterpret_cast<char*>(a.out_boards + N * C);
    a.slot0 = (r->head + first) % r->cap; a.cap = r->cap; a.S = r->S; a.C = r->C; a.stride = (int)stride;
    hipLaunchKernelGGL(af_replay_export_kernel, dim3(n), dim3(256), 0, st, a);
    RP_HIP_OK(hipGetLastError());
    RP_HIP_OK(hipMemcpyAsync(policies, a.out_policies, N * C * 4, hipMemcpyDeviceToHost, st));
    RP_HIP_OK(hipMemcpyAsync(last_cell, a.out_last, N * 4, hipMemcpyDeviceToHost, st));
    RP_HIP_OK(hipMemcpyAsync(values, a.out_values, N * 4, hipMemcpyDeviceToHost, st));
    RP_HIP_OK(hipMemcpyAsync(weights, a.out_weights, N * 4, hipMemcpyDeviceToHost, st));
    if (boards) RP_HIP_OK(hipMemcpyAsync(boards, a.out_boards, N * C, hipMemcpyDeviceToHost, st));
    if (states) RP_HIP_OK(hipMemcpyAsync(states, a.out_states, N * stride, hipMemcpyDeviceToHost, st));
    RP_HIP_OK(hipStreamSynchronize(st));
    return AF_REPLAY_OK;
}

int af_replay_set_weights(af_replay* r, const float* table_host, int32_t max_T) {
    if (!r || !table_host || max_T < 1) return AF_REPLAY_ERR_ARG;
    RP_HIP_OK(hipSetDevice(r->device));
    RP_HIP_OK(hipDeviceSynchronize());                 // no append may still be reading the old table
    if (r->wtab) (void)hipFree(r->wtab);
    r->wtab = nullptr; r->max_T = 0;
    const size_t bytes = (size_t)(max_T + 1) * max_T * 4;
    RP_HIP_OK(hipMalloc(reinterpret_cast<void**>(&r->wtab), bytes));
    RP_HIP_OK(hipMemcpy(r->wtab, table_host, bytes, hipMemcpyHostToDevice));
    const int rc = ensure_err(r);
    if (rc) return rc;
    r->max_T = max_T;
    return AF_REPLAY_OK;
}

int af_replay_append_packed(af_replay* r, void* stream, const int32_t* packed_dev, int32_t max_episodes, int32_t episode, int32_t T) {
    if (!r || !packed_dev || max_episodes < 1 || episode < 0 || episode >= max_episodes || T < 1) return AF_REPLAY_ERR_ARG;
    if (!r->wtab || T > r->max_T) return AF_REPLAY_ERR_ARG;      // af_replay_set_weights first
    if (r->count + T > r->cap) return AF_REPLAY_ERR_FULL;
    RP_HIP_OK(hipSetDevice(r->device));
    PackedArgs a;
    a.buf = packed_dev; a.boards = r->boards; a.policies = r->policies; a.last = r->last; a.values = r->values; a.weights = r->weights;
    a.wtab = r->wtab; a.err = r->err; a.slot0 = (r->head + r->count) % r->cap; a.cap = r->cap; a.C = r->C;
    a.max_eps = max_episodes; a.ep = episode; a.T = T; a.max_T = r->max_T;
    hipLaunchKernelGGL(af_replay_append_packed_kernel, dim3(T), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    RP_HIP_OK(hipGetLastError());
    r->count += T;
    return AF_REPLAY_OK;
}

/* 1 if a packed append found the buffer not to hold what the host said (and appended nothing); clears the flag */
int af_replay_check(af_replay* r, void* stream) {
    if (!r) return AF_REPLAY_ERR_ARG;
    if (!r->err) return 0;
    int32_t h = 0;
    RP_HIP_OK(hipSetDevice(r->device));
    RP_HIP_OK(hipMemcpyAsync(&h, r->err, 4, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    RP_HIP_OK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    if (h) { RP_HIP_OK(hipMemset(r->err, 0, 4)); return AF_REPLAY_ERR_RANGE; }
    return AF_REPLAY_OK;
}

int af_replay_sample(af_replay* r, void* stream, int32_t num, const int32_t* idx, const int32_t* quarter_turns,
                     const int32_t* flip, float* boards_dev, float* weights_dev, float* values_dev, float* policies_dev) {
    if (!r || num < 0 || (num > 0 && (!idx || !quarter_turns || !flip || !boards_dev || !weights_dev || !values_dev || !policies_dev)))
        return AF_REPLAY_ERR_ARG;
    if (num == 0) return AF_REPLAY_OK;
    RP_HIP_OK(hipSetDevice(r->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = ensure_pinned(r, (size_t)3 * num * 4);
    if (rc) return rc;
    rc = ensure_sel(r, num);
    if (rc) return rc;
    RP_HIP_OK(hipStreamSynchronize(st));               // a previous sample's staging copy must have left the pinned buffer
    int32_t* h = static_cast<int32_t*>(r->pinned);
    for (int i = 0; i < num; ++i) {
        if (idx[i] < 0 || idx[i] >= r->count || quarter_turns[i] < 0 || quarter_turns[i] > 3) return AF_REPLAY_ERR_RANGE;
        h[i] = (int32_t)((r->head + idx[i]) % r->cap);
        h[num + i] = quarter_turns[i];
        h[2 * num + i] = flip[i] ? 1 : 0;
    }
    RP_HIP_OK(hipMemcpyAsync(r->sel, h, (size_t)3 * num * 4, hipMemcpyHostToDevice, st));
    return launch_sample(r, st, num, boards_dev, weights_dev, values_dev, policies_dev);
}

int af_replay_sample_device(af_replay* r, void* stream, int32_t num, int32_t batches, uint64_t seed, uint32_t draw,
                            float* boards_dev, float* weights_dev, float* values_dev, float* policies_dev, int32_t* draws_out_dev) {
    if (!r || !boards_dev || !weights_dev || !values_dev || !policies_dev || num < 1 || batches < 1) return AF_REPLAY_ERR_ARG;
    if (num > AF_REPLAY_MAX_DRAW || batches > AF_REPLAY_MAX_BATCHES) return AF_REPLAY_ERR_RANGE;     // (the handle is not read before this)
    if (num > r->count) return AF_REPLAY_ERR_RANGE;
    RP_HIP_OK(hipSetDevice(r->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int total = batches * num;                                    // <= 4096 * 4096
    const int rc = ensure_sel(r, total);
    if (rc) return rc;
    DrawArgs d;
    d.sel = r->sel; d.draws = draws_out_dev; d.head = r->head; d.k0 = (uint32_t)seed; d.k1 = (uint32_t)(seed >> 32); d.draw = draw;
    d.n = r->count; d.k = num; d.cap = r->cap; d.total = total;
    hipLaunchKernelGGL(af_replay_draw_kernel, dim3(batches), dim3(256), 0, st, d);
    RP_HIP_OK(hipGetLastError());
    return launch_sample(r, st, total, boards_dev, weights_dev, values_dev, policies_dev);
}

}  // extern "C"
