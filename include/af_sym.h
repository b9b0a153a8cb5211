/*
 * af_sym.h — C ABI of the board-symmetry kernels around an evaluator (libaf_sym.so): the search evaluates a leaf under all eight
 * symmetries of the board and averages ("mean"), or under one symmetry drawn per leaf ("random", AlphaGo Zero's evaluator).
 * The forward itself is whatever evaluator the caller wraps; this library only permutes its inputs and outputs, on the device.
 *
 * Specification: alphafive_amd/symmetry.py states every call below in numpy, and the kernels equal it bit for bit.
 *
 * Symmetries: s = 0..7, turns = s & 3, flip = s >> 2.  transform(a, s) = np.rot90(a, turns) over the board axes, then np.flip along
 * the row axis if flip — the (quarter turns, flip) pair of af_replay_sample (include/af_replay.h) and of utils.py:127-138.  s = 0 is
 * the identity.  inverse(a, s) undoes transform(a, s).
 *
 *   mean:    planes8[8 b + s] = transform(planes[b], s)                       af_sym_expand
 *            (policy8, value8) = evaluator(planes8)                            the caller's
 *            policy[b] = ((((((((q_0 + q_1) + q_2) + ... ) + q_7)) * 0.125f,   af_sym_reduce
 *                        q_s = inverse(policy8[8 b + s], s); value[b] likewise over value8[8 b + s]:
 *                        seven fp32 additions in the order of s, one multiplication, each rounded once (no fma).
 *   random:  s_b = v[0] >> 29, v = af_philox4x32(b, (uint32_t)counter, (uint32_t)(counter >> 32), AF_SYM_DRAW_TAG,
 *                                               (uint32_t)seed, (uint32_t)(seed >> 32))            (af_noise.h)
 *            planes_t[b] = transform(planes[b], s_b); syms[b] = s_b            af_sym_apply
 *            (policy_t, value_t) = evaluator(planes_t)                         the caller's
 *            policy[b] = inverse(policy_t[b], syms[b]); value[b] = value_t[b]; counter += 1        af_sym_restore
 *
 * The handle owns the random mode's state — syms[max_batch] and the 64-bit counter, in device memory — so that a captured launch
 * sequence (apply, forward, restore) draws afresh on every replay: apply reads the counter and does not write it, restore reads
 * syms and exactly one of its threads advances the counter; stream order does the rest.
 *
 * The four work calls are one launch each on `stream`: no allocation, no copy to the host, no wait — legal under stream capture —
 * and no value that changes between calls travels in kernel arguments.  All tensors are contiguous float32 device memory:
 * planes [batch][3][S][S], policy [batch][S*S], value [batch].  Rows at or beyond `batch` (8 * batch for planes8) are never written.
 *
 * Plain pointers, int return codes (0 ok, <0 error), no exceptions; one handle per consumer.  AF_SYM_ERR_ARG is returned before
 * any HIP call for a null handle or pointer, batch < 1 or batch > max_batch, and an input that aliases an output it is permuted
 * into (planes == planes8, planes == planes_t, policy_t == policy); anything the runtime refuses is AF_SYM_ERR_HIP.
 */
#ifndef AF_SYM_H
#define AF_SYM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct af_sym af_sym;

#define AF_SYM_OK 0
#define AF_SYM_ERR_ARG (-1)
#define AF_SYM_ERR_HIP (-2)

#define AF_SYM_ABI_VERSION 1
#define AF_SYM_DRAW_TAG 0x53594d30u   /* "SYM0": the domain of these Philox blocks (fourth counter word) */

int af_sym_abi_version(void);

/* board_size 3..16, max_batch >= 1 with the 24 * max_batch * S * S elements of planes8 countable in 31 bits (349,000 rows at
 * 16x16).  Makes the handle's only allocation: the counter (starts at 0) and syms[max_batch]. */
int af_sym_create(int32_t board_size, int32_t max_batch, int32_t device, uint64_t seed, af_sym** out);
void af_sym_destroy(af_sym* h);

/* planes [batch][3][S][S] -> planes8 [8 * batch][3][S][S]; every plane, the last-move plane included, is transformed alike. */
int af_sym_expand(af_sym* h, void* stream, const float* planes, float* planes8, int32_t batch);
/* policy8 [8 * batch][C], value8 [8 * batch] -> policy [batch][C], value [batch]: one thread per output element. */
int af_sym_reduce(af_sym* h, void* stream, const float* policy8, const float* value8, float* policy, float* value, int32_t batch);
/* planes [batch][3][S][S] -> planes_t, each row under the symmetry drawn for it at the handle's counter; stores the draws in syms. */
int af_sym_apply(af_sym* h, void* stream, const float* planes, float* planes_t, int32_t batch);
/* policy_t [batch][C] -> policy under the inverse of the stored symmetries; value_t is copied to value if the two pointers
 * differ; advances the counter by one. */
int af_sym_restore(af_sym* h, void* stream, const float* policy_t, const float* value_t, float* policy, float* value, int32_t batch);

/* The counter takes `counter` behind the work queued on `stream` (one launch). */
int af_sym_set_counter(af_sym* h, void* stream, uint64_t counter);
/* For tests: synchronises `stream`, then copies the counter and the first min(cap, max_batch) stored symmetries to the host.
 * Either output may be NULL. */
int af_sym_state(af_sym* h, void* stream, uint64_t* counter, int32_t* syms_host, int32_t cap);

const char* af_sym_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif
