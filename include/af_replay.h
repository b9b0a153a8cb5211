/*
 * af_replay.h — C ABI of the device-resident replay buffer (libaf_replay.so): the storage and the
 * sampling/augmentation half of the reference's utils.RandomStack (utils.py:14-146) on the GPU, so that
 * self-play positions stay in HBM for the trainer.
 *
 * Division of labour (drop-in: alphafive_amd/replay.py:DeviceRandomStack keeps RandomStack's call surface):
 *   host  — the scalar bookkeeping of push() (utils.py:65-116: short-game rejection, colour re-balancing
 *           duplicates, FIFO eviction with partial-episode accounting) and every random draw of get_data()
 *           (utils.py:122,129,136: which positions, how many quarter turns, flip or not), taken from the same
 *           global streams in the same order as the reference, so seeded runs stay reproducible against it;
 *   device — the positions (a ring of boards int8[C], policies float32[C], last-move cell, value, weight) and
 *           get_data()'s per-sample work (utils.py:127-145): rot90^k + vertical flip of board and policy,
 *           the last_action remap, board_to_inputs' three planes, gathered into the batch tensors.
 *           It also owns the codec between its int8 boards and the run-length state strings the reference's records carry
 *           (utils.py:156-196), in both directions: af_replay_export is the way out of the ring (positions in logical order,
 *           as state strings and/or boards, for RandomStack's data*.pkl), af_replay_append_states the way back in.
 *   device-drawn path — af_replay_sample_device takes the draws of get_data() off the host as well: which positions, turns and
 *           flips come from a counter-based generator (Philox4x32-10 of af_noise.h, keyed by a seed and a draw counter) in
 *           af_replay_draw_kernel, which writes the (slot, turns, flip) triples the gather kernel above reads: a training step
 *           then touches the host for launches only.  Same distribution as the reference's draws, not the same streams: the path
 *           above stays for whoever needs seeded equality with the reference.
 * Results are bit-identical to the host class (pure gathers of fp32 / small-integer data).
 *
 * Plain pointers, int return codes (0 ok / count, <0 error), no exceptions; one handle per GPU.
 */
#ifndef AF_REPLAY_H
#define AF_REPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct af_replay af_replay;

#define AF_REPLAY_OK 0
#define AF_REPLAY_ERR_ARG   (-1)
#define AF_REPLAY_ERR_HIP   (-2)
#define AF_REPLAY_ERR_FULL  (-3)   /* append beyond capacity: drop from the front first */
#define AF_REPLAY_ERR_RANGE (-4)   /* sample index / drop count / export range outside the stored range */
#define AF_REPLAY_ERR_FORMAT (-5)  /* a state string that is not S rows of S cells in utils.py:156-175's alphabet */

/* capacity = most positions ever resident at once (RandomStack.length + the longest episode pushed twice). */
int af_replay_create(int32_t board_size, int32_t capacity, int32_t device, af_replay** out);
void af_replay_destroy(af_replay* r);

/* Append n positions at the tail (host pointers; copied asynchronously on `stream`, the call returns after the
 * staging copy so the host arrays may be reused): boards int8[n][C] (+1 mine / -1 theirs / 0, utils.py:185),
 * policies float32[n][C], last_cell int32[n] (i*S+j, or -1 for None), values float32[n], weights float32[n]. */
int af_replay_append(af_replay* r, void* stream, int32_t n, const int8_t* boards, const float* policies,
                     const int32_t* last_cell, const float* values, const float* weights);
/* Device-to-device append ("keep episodes on-GPU for the trainer"): episode `episode` of a packed hand-off buffer
 * that af_engine_pack_episodes (include/af_engine.h) wrote into DEVICE memory with the same max_episodes.  One launch on `stream`
 * decodes every ply of it on the device — position key -> board int8 (+1 mine / -1 theirs: utils.py:185 state_to_board of the
 * recorded root), temperature policy, last move, value = the final value with the signs of player.py:74-82, weight = row T of the
 * table below — straight into the ring.  `T` (the episode's length, which the host reads from the buffer's small header for
 * RandomStack.push's bookkeeping anyway) sizes the launch and must equal the length recorded in the buffer (checked on the
 * device: a mismatch appends nothing and raises the flag af_replay_check() reports).  No host copy of the
 * episode, no per-ply host work. */
int af_replay_append_packed(af_replay* r, void* stream, const int32_t* packed_dev, int32_t max_episodes, int32_t episode, int32_t T);
/* The per-ply training weights utils.construct_weights(T, gamma) (utils.py:286-296; numpy float32 arithmetic) for every episode
 * length: table[max_T + 1][max_T] float32, row T holds w[0..T-1].  Computed by the host mirror (the numpy restatement is the
 * spec: pairwise float32 sum), uploaded once per gamma. */
int af_replay_set_weights(af_replay* r, const float* table_host, int32_t max_T);
/* AF_REPLAY_ERR_RANGE if a packed append since the last call found the buffer not to hold the episode the host described (it
 * appended nothing then); synchronises `stream`.  AF_REPLAY_OK otherwise. */
int af_replay_check(af_replay* r, void* stream);

/* Bytes per exported state string: S*(S+1) + 1.  (A row of S cells encodes to at most S characters - stones + runs <= stones +
 * empties - plus its '/'; one NUL.) */
int32_t af_replay_state_stride(const af_replay* r);
/* Read positions first .. first+n-1, counted from the oldest, in order, into HOST arrays shaped as af_replay_append takes them,
 * plus states char[n][af_replay_state_stride] (utils.py:156-175 board_to_state: per row a run of c empties is 'a'+c, '3' mine,
 * '1' theirs, '/' ends the row; NUL-terminated and NUL-padded).  `states` or `boards` may be NULL.  One launch on `stream` gathers
 * the range out of the ring into a contiguous device staging block (the ring's wrap is invisible to the copies) and writes the
 * strings, ordered behind any af_replay_append_packed still queued on `stream`; the call returns after the copies have landed.
 * AF_REPLAY_ERR_RANGE if the range is not stored.  The ring is not modified. */
int af_replay_export(af_replay* r, void* stream, int32_t first, int32_t n, char* states, int8_t* boards, float* policies,
                     int32_t* last_cell, float* values, float* weights);
/* af_replay_append for records that carry state strings (what the reference's data*.pkl holds): states char[n][state_stride],
 * each NUL-terminated inside its stride; one launch decodes them into the ring's int8 boards.  The decoder checks everything it
 * derives from the text (no NUL inside the stride, a character other than 'a'+1 .. 'a'+S, '1', '3', '/', a row that runs past S
 * cells or stops short of them, a row count other than S): any bad string makes the whole call append nothing and return
 * AF_REPLAY_ERR_FORMAT.  Synchronises `stream` like af_replay_append, so it reports directly, not through af_replay_check. */
int af_replay_append_states(af_replay* r, void* stream, int32_t n, const char* states, int32_t state_stride, const float* policies,
                            const int32_t* last_cell, const float* values, const float* weights);

/* Forget the n oldest positions (utils.py:103 `del self.data[:beyond]`). */
int af_replay_drop_front(af_replay* r, int32_t n);
int32_t af_replay_size(const af_replay* r);

/* get_data (utils.py:118-146) for `num` samples: idx int32[num] = positions counted from the oldest,
 * quarter_turns int32[num] in 0..3 (np.rot90 k, counter-clockwise), flip int32[num] (1 = np.flip axis 0 applied
 * after the rotation).  Device outputs: boards float32[num][3][S][S] (board_to_inputs planes of the transformed
 * board with the remapped last action), weights float32[num], values float32[num], policies float32[num][C]. */
int af_replay_sample(af_replay* r, void* stream, int32_t num, const int32_t* idx, const int32_t* quarter_turns,
                     const int32_t* flip, float* boards_dev, float* weights_dev, float* values_dev, float* policies_dev);

/* Device-drawn get_data: `batches` independent minibatches of `num` samples each, drawn and gathered on the device.
 * Specification (alphafive_amd/replay.py:draw_reference states it in numpy; the kernel equals it bit for bit): for minibatch b
 * and logical position i in [0, n), n = af_replay_size, counted from the oldest as in af_replay_sample,
 *     v        = af_philox4x32(ctr = (i, b, draw, AF_REPLAY_DRAW_TAG), key = ((uint32_t)seed, (uint32_t)(seed >> 32)))   (af_noise.h)
 *     key(i)   = (uint64_t)v[0] << 32 | i          distinct for distinct i
 *     turns(i) = v[1] >> 30                        0..3, np.rot90 k
 *     flip(i)  = v[2] >> 31                        1 = flip applied (the reference's `random.choice([1,2]) == 1`)
 * and minibatch b is the `num` positions with the smallest key, sample j the j-th smallest: a uniform subset in uniform order
 * and one of the 8 symmetries uniformly per sample, the distribution of utils.py:120,129,136.  (Equal 32-bit words are ordered by
 * the lower index: a bias of at most n / 2^32 relative.)  The caller advances `draw` from call to call; one call with
 * batches = 4 is four independent draws from the same buffer state (main.py:62-68).
 * Device outputs as af_replay_sample's with a leading [batches]: boards float32[batches][num][3][S][S], weights and values
 * float32[batches][num], policies float32[batches][num][C]; draws_out_dev (optional, may be NULL) int32[3][batches * num] =
 * logical index, quarter turns, flip of every sample.
 * 1 <= num <= AF_REPLAY_MAX_DRAW, num <= af_replay_size (the caller takes the min, as get_data does), 1 <= batches <=
 * AF_REPLAY_MAX_BATCHES.  A null handle or output and num or batches below 1 are AF_REPLAY_ERR_ARG, anything above its range
 * AF_REPLAY_ERR_RANGE, both before any HIP call.
 * Two launches on `stream` and nothing else — af_replay_draw_kernel, one workgroup per minibatch, then af_replay_sample's gather
 * kernel over batches * num triples: no host staging, no pinned copy, no stream synchronisation (the selection buffer is
 * reallocated when a call needs a larger one than any before it).  The ring's head, size and capacity travel by value, as in
 * every call of this header, so a launch is bound to the ring state of the moment it was issued: the call is not meant for
 * stream capture. */
#define AF_REPLAY_DRAW_TAG 0x52504C59u   /* "RPLY": the domain of these Philox blocks (fourth counter word) */
#define AF_REPLAY_MAX_DRAW 4096
#define AF_REPLAY_MAX_BATCHES 4096
int af_replay_sample_device(af_replay* r, void* stream, int32_t num, int32_t batches, uint64_t seed, uint32_t draw,
                            float* boards_dev, float* weights_dev, float* values_dev, float* policies_dev,
                            int32_t* draws_out_dev);

const char* af_replay_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif
