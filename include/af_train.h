/*
 * af_train.h — C ABI of the trainer's fused kernels (libaf_train.so): what alphafive_amd.train.Trainer(fused=True) runs instead
 * of the ~20 elementwise/reduction ops of the loss head, the per-variable L2 sums and their backward passes, and the nine
 * multi-tensor launches of Adam.  The convolutions and dense layers stay with PyTorch autograd: these calls sit on either side
 * of one torch.autograd.grad([logits, value], params, [dlogits, dvalue]).
 *
 *     af_train_loss_head   logits, value, pi, winner, weight -> dlogits, dvalue, per-row loss terms        one launch
 *     af_train_adam        up to AF_TRAIN_MAX_VARS variables (p, g, m, v) updated in place + L2 partials    one launch
 *     af_train_finalize    per-row terms + L2 partials -> (total, cross_entropy, value_loss, entropy)       one launch
 *
 * No handle, no allocation, no synchronisation, no host read-back: every buffer, workspaces included, is a caller-provided
 * DEVICE buffer (fp32, except the per-row terms, which are fp64) and every call is launches on `stream` only.  Plain pointers, int return codes (>= 0 ok, < 0 error);
 * arguments are checked before any HIP call, and a call that returns an error has launched nothing.
 * wave64, gfx950.  No float atomics: every reduction has a fixed order, so the same inputs give the same bits on every run.
 * Built with -ffp-contract=off: Adam's arithmetic is exactly as written below, one fp32 operation per operator, divide and
 * square root correctly rounded (alphafive_amd/train_hip.py:adam_reference states the element in numpy; the kernel equals it
 * bit for bit).  The loss head and the scalar reduction compute in fp64 from their fp32 inputs and round each fp32 result once.
 */
#ifndef AF_TRAIN_H
#define AF_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AF_TRAIN_OK 0
#define AF_TRAIN_ERR_ARG   (-1)   /* null pointer, negative count, variable count outside 1..AF_TRAIN_MAX_VARS */
#define AF_TRAIN_ERR_HIP   (-2)
#define AF_TRAIN_ERR_RANGE (-3)   /* C above AF_TRAIN_MAX_C, or more elements than the chunk index can address */

#define AF_TRAIN_MAX_C 1024       /* most logits per row: 16 per lane, held in registers */
#define AF_TRAIN_ROW_TERMS 5      /* doubles per row of row_terms */
#define AF_TRAIN_MAX_VARS 64      /* most variables of one af_train_adam call (the table travels in the kernel arguments) */
#define AF_TRAIN_ADAM_CHUNK 2048  /* elements of one variable a workgroup updates; one L2 partial per chunk */

/* Loss head of network.py:40-50 and its gradient, one wavefront per row.  Per row b, with z = logits[b], v = value[b]:
 *     logsm_c = (z_c - max(z)) - log(sum_c exp(z_c - max(z)))
 *     xent    = sum_c pi_c * logsm_c            vsq = (v - winner)^2            ent = -sum_c exp(logsm_c) * logsm_c
 *     row_terms[b] = (w * xent, w * vsq, xent, vsq, ent)                        the entropy is the FIFTH slot
 *     dlogits[b][c] = -(w / B) * (pi_c - exp(logsm_c) * sum_c pi_c)             d total / d logits (sum_c pi_c, not 1: pi is data)
 *     dvalue[b]     = ((4 * w) / B) * (v - winner)                              d total / d value
 * All of it in fp64 (the inputs converted as loaded); dlogits and dvalue are rounded to fp32 once, as they are stored.
 * Sums over c: lane l adds its elements c = l, l + 64, ... in that order, then a 6-step butterfly over the 64 lanes.
 * logits, pi, dlogits float32[B][C]; value, winner, weight, dvalue float32[B]; row_terms float64[B][AF_TRAIN_ROW_TERMS]
 * (8-byte aligned).
 * 1 <= B, 1 <= C <= AF_TRAIN_MAX_C (above: AF_TRAIN_ERR_RANGE).  dlogits may not alias logits or pi. */
int af_train_loss_head(void* stream, int32_t B, int32_t C, const float* logits, const float* value, const float* pi,
                       const float* winner, const float* weight, float* dlogits, float* dvalue, double* row_terms);

/* One variable of af_train_adam: n elements at p (parameter), g (gradient of the data terms), m, v (Adam's slots); decay != 0:
 * the variable is under the L2 penalty.  n = 0 is allowed: nothing happens to it, it has no chunk and no partial, and its
 * pointers are never read (they may be null, as a zero-size buffer's usually are). */
typedef struct af_train_var {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    int32_t decay;
    int32_t reserved;      /* 0 */
} af_train_var;

/* tf.train.AdamOptimizer's update of nvars variables (1 <= nvars <= AF_TRAIN_MAX_VARS; a caller with more issues several
 * calls) in ONE launch.  `vars` is a HOST array: the pointers travel by value in the kernel arguments, so the (fresh every step)
 * gradient tensors need no device-side table.  Per element, in this order, each operator one fp32 operation:
 *     g' = decay ? g + l2_coef * p : g
 *     m  = m * beta1 + g' * (1 - beta1)
 *     v  = v * beta2 + (g' * g') * (1 - beta2)
 *     p  = p - (lr_t * m) / (sqrt(v) + eps)          eps outside the root; lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
 * Workgroup w of the launch takes chunk w: the chunks of variable 0 first, then variable 1's, ...; variable k has
 * ceil(n_k / AF_TRAIN_ADAM_CHUNK) of them.  It also writes l2_partials[w] = sum of p * p over its chunk (p BEFORE the update)
 * for a decay variable, 0 otherwise: thread t of 256 adds elements t, t + 256, ... of the chunk in that order, then a butterfly
 * over the 64 lanes, then the four waves in order.
 * l2_partials: float32[sum_k ceil(n_k / AF_TRAIN_ADAM_CHUNK)].  Returns that count (>= 0), or an error. */
int af_train_adam(void* stream, int32_t nvars, const af_train_var* vars, float lr_t, float beta1, float beta2, float eps,
                  float l2_coef, float* l2_partials);
/* The count af_train_adam would return for these sizes (its l2_partials length), without launching: n int64[nvars]. */
int af_train_adam_partials(int32_t nvars, const int64_t* n);

/* One workgroup: terms[4] = (total, cross_entropy, value_loss, entropy) of network.py:50, with S_j = sum_b row_terms[b][j] and
 * L = sum_i l2_partials[i]:
 *     total = -(S_0 / B) + 2 * (S_1 / B) + l2_coef * (L / 2)       cross_entropy = -(S_2 / B)
 *     value_loss = S_3 / B                                         entropy = S_4 / B
 * in fp64, each of the four rounded to fp32 once.
 * Each sum: thread t of 256 adds entries t, t + 256, ... in index order, then the fixed tree of af_train_adam's partials.
 * n_partials may be 0 (l2_partials may then be NULL): L = 0. */
int af_train_finalize(void* stream, int32_t B, const double* row_terms, int32_t n_partials, const float* l2_partials,
                      float l2_coef, float* terms);

const char* af_train_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif
