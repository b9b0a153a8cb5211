/*
 * af_net.h — C ABI of the hand-written gfx950 forward pass of the reference's policy/value
 * network (libaf_net.so).  Replaces, for the self-play path, what genData/network.py:90-97
 * (ResNet.eval -> sess.run([prob, value])) executes: the graph of network.py:52-88,163-165
 *   conv5x5(3->32)+ELU, residual(64), residual(128), value head (residual(32), 1x1->4, fc 64, fc 1,
 *   tanh(x/2)), policy head (residual(64), residual(32), 1x1->16, fc S*S, softmax)
 * in fp32 on the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate).
 *
 * Variables are handed over under their checkpoint names in TF layout (conv kernels HWIO
 * [kh][kw][cin][cout], dense [in][out], flatten order NCHW), exactly as
 * alphafive_amd.tensorbundle reads them from ckpt/alphaFive-*.  Plain pointers, int return
 * codes (0 ok, <0 error), no exceptions; one handle per GPU; not thread-safe per handle.
 */
#ifndef AF_NET_H
#define AF_NET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct af_net af_net;

#define AF_NET_OK 0
#define AF_NET_ERR_ARG   (-1)
#define AF_NET_ERR_HIP   (-2)
#define AF_NET_ERR_NAME  (-3)   /* unknown variable name or wrong element count */
#define AF_NET_ERR_STATE (-4)   /* forward before finalize / missing variables */

/* board_size S (3..16); max_batch = largest batch af_net_forward will be called with.  Allocates everything the handle will ever own
 * — weight, activation and staging buffers of both conv paths, its side stream and events — or frees what it made and returns
 * AF_NET_ERR_HIP; no later call allocates or frees until af_net_destroy. */
int af_net_create(int32_t board_size, int32_t max_batch, int32_t device, af_net** out);
void af_net_destroy(af_net* n);

/* Provide one variable (host pointer, fp32, TF layout) — e.g. "bone/block1_conv1/kernel": copied into the handle's host image of the
 * variables at once.  af_net_forward returns AF_NET_ERR_STATE from here until the next af_net_finalize or af_net_update_device. */
int af_net_set_variable(af_net* n, const char* tf_name, const float* host_data, int64_t count);
/* Call after all 42 variables are set (AF_NET_ERR_STATE otherwise): waits for the device — forwards in flight on any stream still read
 * the packed weights, so the caller need not wait for them itself —, uploads the host image to the handle's staging area in one copy
 * and packs it in place with the kernels of af_net_update_device (k-pair-major streams and split fp16 fragments for the MFMA
 * kernels).  The packing has finished when it returns: a forward on any stream finds the new weights.  A graph captured over the
 * handle before the call does not: the split-operand kernels take their scales by value. */
int af_net_finalize(af_net* n);

/* Weight hand-over without the host: all 42 variables at once, from DEVICE memory (fp32, TF layout, same names / counts as
 * af_net_set_variable), re-packed by kernels IN PLACE into the buffers the handle already owns — nothing is freed, nothing is
 * allocated, no weight is copied to the host.  Every weight-derived buffer of BOTH conv paths is rewritten (af_net_tune(0, .) may
 * switch paths at any time), to the bytes af_net_set_variable + af_net_finalize make of the same values (the same kernels pack).
 *   - the handle must have been finalized once (AF_NET_ERR_STATE otherwise);
 *   - all or nothing: names, counts and "each of the 42 exactly once" are checked before anything is launched — an unknown name or a
 *     wrong count returns AF_NET_ERR_NAME; a null handle / array / entry, nvars != 42 or a name given twice AF_NET_ERR_ARG (null
 *     handle or arrays: before any HIP call);
 *   - stream-ordered on `stream`: after the forwards already queued there, before later ones.  ONE host wait: the split-operand
 *     path's power-of-two scales depend on max|w| per scale group and the forward kernels take them by value, so the call reduces
 *     the maxima on the device, copies 80 bytes to pinned memory, synchronises `stream` once, picks the scales on the host and
 *     launches the pack kernels; everything else is asynchronous.  The source tensors must stay unchanged until the pack kernels have
 *     run (stream order suffices for a producer on the same stream);
 *   - because it synchronises, it must not be called while `stream` is being captured: AF_NET_ERR_STATE, nothing launched;
 *   - afterwards the handle's host copy of the variables is gone: af_net_finalize returns AF_NET_ERR_STATE until all 42 have been
 *     set again with af_net_set_variable. */
int af_net_update_device(af_net* n, void* stream, const char* const* tf_names, const float* const* dev_ptrs, const int64_t* counts,
                         int32_t nvars);

/* planes_dev float32[batch][3][S][S] (utils.py:256 board_to_inputs layout) ->
 * policy_dev float32[batch][S*S] (softmax probabilities), value_dev float32[batch].
 * Asynchronous on `stream` (hipStream_t; NULL = default stream). */
int af_net_forward(af_net* n, void* stream, const float* planes_dev, int32_t batch, float* policy_dev, float* value_dev);

/* Benchmark / A-B knobs (process-global; an unknown key or value returns AF_NET_ERR_ARG):
 *   key 0: conv path — 5 (default) fp16 split-operand implicit GEMM (af_conv_f16s.hip; 11x11 and 15x15 boards: three fp16 MFMA products
 *          per MAC, fp32 accumulate, 22 operand mantissa bits), 1 fp32 MFMA Winograd F(2x2,3x3) (af_net.hip: 24 bits — the path of every
 *          other board size, and bench.py's config2_fp32mfma leg)
 *   key 4: value branch on a side stream (default 1: on the fp32 path only; 2 forces it on path 5 too, for A/B)
 *   key 5: MFMA policy head of the fp32 path (default 1)
 *   key 7: bits of path 5, named by enum F16sBits in csrc/af_conv_f16s.h; f16s_plan (af_conv_f16s.hip) is the one function that chooses launch variants from them.
 *          kF16sProfilingBits 1 / 2 / 4 / 8 / 4096: profiling ablations (results wrong by design: no slab loads after the first position /
 *          no stores / loads from a hot address / stores, loads addressed modulo 128 positions); kF16sValuStem 16: VALU stem;
 *          kF16sOneWgPerCu 32: one workgroup per CU in the 32-channel-input layers.  Launch structures, each bit selecting the launch it
 *          replaced (same results bit for bit): kF16sTwoHalves15 64 two-halves launch on 15x15 (instead of the 4-tile / 3-tile classes +
 *          corner kernel), kF16sWgPerPosition 128 one workgroup per position at batches <= 8 (instead of the pixel-tile split),
 *          kF16sTwoLaunchBlocks 256 two launches per 32-wide block (instead of af_block_f16s), kF16sBranchLaunchesSmall 512 /
 *          kF16sBranchLaunchesBig 1024 the two-branch launch order at batches <= 8 / above (instead of the value branch as a workgroup
 *          class), kF16sLaunchSequence 2048 (r6) nine dependent launches at batches <= 8 (instead of the single launch of dataflow roles)
 *   key 9: path 5 computes the heads itself — 1x1 head convolutions fused into the last conv of each branch, dense layers on
 *          the same split-operand MFMA (default 1); 0 = the fp32 head kernels of path 1 on fp32 planes
 * (removed in r6 with the kernels they selected: conv paths 0 / 2 / 3 / 4, keys 1 / 2 / 3 / 6 / 8) */
int af_net_tune(int32_t key, int32_t value);

/* Tests / debugging of the fp16 split-operand path (conv path 5, 11x11 and 15x15 boards): intermediate activation `which`
 * (0 stem f0, 1/2 block1 conv1 g1 / output o1, 3/4 block2 g2 / o2, 5 block3 conv1 g3, 6/7 block4 g4 / o4, 8 block5 conv1 g5,
 * 9 / 10 the value / policy head's 1x1 convolution output after its ELU: 4 / 16 channels, the dense layers' input) of the first
 * `batch` positions of the last forward, as fp32 [batch][C][S*S] on the host (hi + lo of the stored halves).  Returns the channel
 * count C or <0.  Synchronises the device.  The call copies a buffer; whether the last forward WROTE it depends on its launch form:
 *
 *   which                      written by
 *   0 1 2 3 4 6 7              every form on both board sizes (roles, paired, branches; tile split or whole positions)
 *   5 (g3), 8 (g5)             15x15 always; 11x11 only with af_net_tune(7, 256) or af_net_tune(9, 0) — with fused blocks (the
 *                              11x11 default) the 32-channel intermediate stays in LDS and the buffer keeps what an earlier forward left
 *   9, 10                      key 9 = 1 (default: fused heads); with key 9 = 0 the branches end in fp32 planes instead
 *   o3, o5 (block 3 / 5 out)   never stored: they feed the head convolution from registers
 *
 * Range of the split-operand path: every stored activation f (all of the above) must satisfy |f| < 65504, the fp16 maximum —
 * activations are stored unscaled as fp16 hi + lo, only weights carry a power-of-two scale.  Within the range the split is good to
 * 2^-22 relative, and to 2^-25 absolute below |f| ~ 2^-3 (fp16 subnormal halves are kept).  Beyond it the outputs are UNDEFINED and
 * may well be finite: the overflowed halves are inf / NaN, the next layer's sum is NaN, and the kernels' ELU (a max / min form)
 * maps NaN to -1.0.  Finite policy and value therefore do not show that a weight set is in range; the per-layer maxima of
 * oracle/net_fp64.intermediates do (shipped checkpoint: at most 376).
 *
 * Tests of the fp32 path (af_net.hip), every board size, with or without a split-operand handle: the handle's fp32 planes, i = 0..10
 * in the order f0, g1, o1, g2, o2, g3, o3, g4, o4, g5, o5 (32, 64, 64, 128, 128, 32, 32, 64, 64, 32, 32 channels):
 *   which = 16 + i   the interior of plane i as fp32 [batch][C][S*S]
 *   which = 32 + i   the same buffer exactly as stored, [batch][C][PP], WP = 2 ceil(S/2) + 2, PP = WP*WP rounded up to a multiple of
 *                    16; board pixel (y, x) sits at (y + 1) WP + x + 1, everything else is border or pad, which no kernel writes
 * Both return C; batch may be anything from 1 to max_batch, not only the last forward's (the buffers are sized for max_batch).
 * Written by: conv path 1 (af_net_tune(0, 1), and every board size other than 11x11 / 15x15) all eleven; path 5 with key 9 = 0
 * o3 and o5 only (the planes its branches end in for the fp32 heads); path 5 by default none. */
int af_net_debug_activation(af_net* n, int32_t which, int32_t batch, float* host_out);

/* Tests: weight-derived device buffer `index` copied to host_out (cap_bytes must hold it); returns its size in bytes (also when
 * host_out is NULL), AF_NET_ERR_ARG past the last index.  Synchronises the device.  Order, blocks b = 0..4 (bone/block1, bone/block2,
 * value/block3, policy/block4, policy/block5), layers l = 2b (conv1), 2b+1 (conv2):
 *   fp32 Winograd path, every board size — 0 stem kernel, 1 stem bias, 2+b conv1 bias (padded), 7+b conv2 + res bias (padded),
 *     12+b / 17+b / 22+b Winograd-domain conv1 / conv2 / projection kernels, 27..36 value/conv kernel, bias, value/fc1 kernel, bias,
 *     value/fc2 kernel, bias, policy/conv kernel, bias, policy/fc kernel, bias;
 *   fp16 split-operand path, 11x11 and 15x15 boards only — 37 stem kernel, 38 stem bias, 39 stem A fragments, 40+l layer A fragments,
 *     50 / 51 produced projection of value/block3 / policy/block5, 52+l layer bias (odd l: conv2 + res), 62 / 63 value / policy head
 *     conv fragments, 64 / 65 their padded biases, 66 / 67 value/fc1 / policy/fc fragments, 68 / 69 their biases, 70 value/fc2
 *     kernel, 71 value/fc2 bias. */
int64_t af_net_debug_weights(af_net* n, int32_t index, void* host_out, int64_t cap_bytes);
/* Tests: the inverse weight scales the split-operand forward passes by value — stem, layers 0..9, produced projections by producer
 * layer 0..9 (0 where there is none), value / policy head conv, value/fc1, policy/fc: 25 floats; returns how many there are (0 on a
 * board size without that path), writes min(cap, that) of them. */
int32_t af_net_debug_scales(af_net* n, float* host_out, int32_t cap);

/* Batches of at most 8 positions on 11x11 (what genData/player.py:186-202 asks for: one leaf per simulation) run as ONE launch of
 * dataflow roles + the policy head's dense layer (csrc/af_conv_f16s.hip: af_small_forward_f16s; af_net_tune(7, 2048) = the nine
 * dependent launches, for A/B).  A role's wait for its producers is bounded; this returns 1 if any wait ever gave up (the outputs
 * of that forward are then undefined), 0 if none did, <0 without the split-operand path.  Synchronises the device. */
int af_net_small_forward_error(af_net* n);

/* FLOPs (2*MAC) of one position's forward pass, as executed (direct convolution). */
int64_t af_net_flops_per_position(const af_net* n);
const char* af_net_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif
