// af_conv_f16s.h — internal interface (inside libaf_net.so) between af_net.hip and af_conv_f16s.hip: the fp16
// split-operand convolution path of the network (11x11 and 15x15 boards).  Not part of the C ABI (include/af_net.h is).
#ifndef AF_CONV_F16S_H
#define AF_CONV_F16S_H

#include <hip/hip_runtime.h>

#include <map>
#include <string>

struct f16s_net;

// board sizes 11 (one pseudo-position per board) and 15 (two half-board pseudo-positions per board); on both the heads are fused (the
// 1x1 head convolutions ride the last conv of each branch, the dense layers run on af_value_fc_f16s / af_policy_fc_f16s<Geo<S>>)
int f16s_supported(int board_size);
// allocates every device buffer of the handle; the weight-derived ones hold nothing until the first f16s_update_pack
int f16s_create(f16s_net** out, int board_size, int max_batch, int device);
void f16s_destroy(f16s_net* n);
// stem + bone/block1 + bone/block2 on stream st
int f16s_trunk(f16s_net* n, hipStream_t st, const float* planes_dev, int batch);
// value/block3 -> o3, policy/block4+5 -> o5: fp32 planes [batch][32][PP], pixel (y,x) at (y+1)*WP + x+1 (the head kernels' input)
// value / policy != nullptr: the branch's last conv also applies the head's 1x1 convolution and the head's dense layers run on the
// same split-operand MFMA (af_value_fc_f16s / af_policy_fc_f16s) -> value [batch] / policy [batch][121]; o3 / o5 are then not written
int f16s_value_branch(f16s_net* n, hipStream_t st, int batch, float* o3_dev, int WP, int PP, float* value);
int f16s_policy_branch(f16s_net* n, hipStream_t st, int batch, float* o5_dev, int WP, int PP, float* policy);
// batches <= 8 on 11x11, heads fused: both branches on one stream ({policy conv1 || value block} in one launch): no side stream
int f16s_small_branches_ok(const f16s_net* n, int batch);          // (abl bit 9 = the two-stream form, for A/B)
int f16s_small_branches(f16s_net* n, hipStream_t st, int batch, float* value, float* policy);
// batches <= 8 on 11x11 (r6): the whole forward up to the policy head's input as ONE launch of dataflow roles + the policy dense layer
int f16s_small_forward_ok(const f16s_net* n, int batch);           // (abl bit 11 = the multi-launch form, for A/B)
int f16s_small_forward(f16s_net* n, hipStream_t st, const float* planes_dev, int batch, float* value, float* policy);
int f16s_small_forward_error(f16s_net* n);                         // 1 if a role ever gave up waiting (synchronises)
void f16s_set_ablation(f16s_net* n, int bits);
int f16s_read_activation(f16s_net* n, int which, int batch, float* host);

// ---- weight packing, from device memory and in place: the one packer of this path (af_net_finalize over the variables it staged,
// af_net_update_device over the caller's tensors) ----
// name -> fp32 TF-layout tensor in DEVICE memory, all 42 variables (af_net.hip has checked names and counts)
typedef std::map<std::string, const float*> f16s_dev_vars;
constexpr int kF16sScaleGroups = 20;       // stem | per block: conv1, conv2 (+ folded projection), produced projection | 2 head convs | value/fc1 | policy/fc
// max|w| of every scale group -> max_dev[kF16sScaleGroups] (device; NaN elements do not count), asynchronous on st
int f16s_update_absmax(f16s_net* n, hipStream_t st, const f16s_dev_vars& D, float* max_dev);
// pack every weight-derived buffer of the split-operand path in place from D, each scale group with the power-of-two scale its
// max_host[group] picks, asynchronous on st, and store the new inverse scales in the handle; max_host = what f16s_update_absmax
// produced, already on the host
int f16s_update_pack(f16s_net* n, hipStream_t st, const f16s_dev_vars& D, const float* max_host);
// weight-derived device buffers in a fixed order (af_net_debug_weights): 0 on success, -1 past the last one
int f16s_weight_buffer(const f16s_net* n, int index, const void** ptr, size_t* bytes);
int f16s_scales(const f16s_net* n, float* out, int cap);           // the 25 inverse scales (af_net_debug_scales); returns how many
// elementwise device copies shared by both paths' packing: dst[i] = i < n_src ? (sum ? a[i] + (b ? b[i] : 0.0f) : a[i]) : 0.0f, i < n_dst
struct UpdCopy { float* dst; const float* a; const float* b; int n_dst, n_src, sum; };
int upd_launch_copies(hipStream_t st, const UpdCopy* d, int count);

#endif
