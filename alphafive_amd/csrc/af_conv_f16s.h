// af_conv_f16s.h — internal interface (inside libaf_net.so) between af_net.hip and af_conv_f16s.hip: the fp16
// split-operand convolution path of the network (11x11 and 15x15 boards), and the table of the network's blocks and variables that
// both read.  Not part of the C ABI (include/af_net.h is).
#ifndef AF_CONV_F16S_H
#define AF_CONV_F16S_H

#include <hip/hip_runtime.h>

// ---- the network's tensors, stated once for both conv paths: five residual blocks and 42 variables ----
#define AF_NET_BLOCKS(X) X("bone/block1", 32, 64) X("bone/block2", 64, 128) X("value/block3", 128, 32) X("policy/block4", 128, 64) X("policy/block5", 64, 32)
struct NetBlock { const char* name; int cin, cout; };
#define AF_BLOCK_ROW(name, cin, cout) {name, cin, cout},
constexpr NetBlock kBlocks[5] = {AF_NET_BLOCKS(AF_BLOCK_ROW)};
// The variables in the order of the staging area (and of every `const float* const* src` of the packers): the stem's two, the ten of
// the heads, six per block: src[var(b, kC1K)] is block b's conv1 kernel.
enum { kVarStemK, kVarStemB, kVarHeads, kVarVcK = kVarHeads, kVarVcB, kVarV1K, kVarV1B, kVarV2K, kVarV2B, kVarPcK, kVarPcB, kVarPfK, kVarPfB,
       kVarBlocks, kVars = kVarBlocks + 6 * 5, kC1K = 0, kC1B, kC2K, kC2B, kResK, kResB };
constexpr int var(int block, int which) { return kVarBlocks + 6 * block + which; }
struct NetVar { const char* name; int c0, c1, c2; };      // TF name; element count = c0 + c1 * HW + c2 * HW * HW (HW = S*S)
#define AF_BLOCK_VARS(name, cin, cout) {name "_conv1/kernel", 9 * cin * cout}, {name "_conv1/bias", cout}, {name "_conv2/kernel", 9 * cout * cout}, \
                                       {name "_conv2/bias", cout}, {name "_res/kernel", cin * cout}, {name "_res/bias", cout},
constexpr NetVar kNetVars[kVars] = {
    {"bone/conv1/kernel", 75 * 32}, {"bone/conv1/bias", 32}, {"value/conv/kernel", 32 * 4}, {"value/conv/bias", 4},
    {"value/fc1/kernel", 0, 4 * 64}, {"value/fc1/bias", 64}, {"value/fc2/kernel", 64}, {"value/fc2/bias", 1},
    {"policy/conv/kernel", 32 * 16}, {"policy/conv/bias", 16}, {"policy/fc/kernel", 0, 0, 16}, {"policy/fc/bias", 0, 1},
    AF_NET_BLOCKS(AF_BLOCK_VARS)};

struct f16s_net;

// board sizes 11 (one pseudo-position per board) and 15 (two half-board pseudo-positions per board); on both the heads are fused (the
// 1x1 head convolutions ride the last conv of each branch, the dense layers run on af_value_fc_f16s / af_policy_fc_f16s<Geo<S>>)
int f16s_supported(int board_size);
// allocates every device buffer of the handle, once (af_net_create); the weight-derived ones hold nothing until the first f16s_update_pack
int f16s_create(f16s_net** out, int board_size, int max_batch, int device);
void f16s_destroy(f16s_net* n);
// zeroes the role counters of kF16sRoles and what f16s_small_forward_error reports (af_net_finalize, behind its device wait)
int f16s_reset_roles(f16s_net* n);
// ---- the launch plan: which launches a forward of `batch` positions is made of ----
// af_net_tune key 7 (include/af_net.h describes the bits by these names).  The profiling bits reach the kernels (F16sArgs::abl) and
// make the results wrong by design; every other bit selects the launch structure the default replaced.
enum F16sBits : int {
    kF16sProfilingBits = 1 | 2 | 4 | 8 | 4096,   // no slab loads after the first position / no stores / loads from a hot address / stores, loads modulo 128 positions
    kF16sValuStem = 16,              // the VALU stem (af_stem_f16s) instead of the MFMA one
    kF16sOneWgPerCu = 32,            // 11x11, the 32-channel-input layers: one workgroup per CU instead of two
    kF16sTwoHalves15 = 64,           // 15x15: the two-halves launch instead of the 4-tile / 3-tile classes + corner kernel
    kF16sWgPerPosition = 128,        // batches <= 8: one workgroup per position instead of the pixel-tile split
    kF16sTwoLaunchBlocks = 256,      // 11x11: two launches per 32-wide block instead of af_block_f16s
    kF16sBranchLaunchesSmall = 512,  // 11x11, batches <= 8: the two-branch launch order instead of the value branch as a workgroup class
    kF16sBranchLaunchesBig = 1024,   // ... and above 8
    kF16sLaunchSequence = 2048,      // 11x11, batches <= 8: nine dependent launches instead of the single launch of dataflow roles
};
enum F16sForm {
    kF16sRoles,      // batches <= 8 on 11x11: the whole forward up to the policy head's input as ONE launch of dataflow roles + the policy dense layer
    kF16sPaired,     // 11x11: trunk, then both branches on one stream ({policy conv1 || value block} in one launch): no side stream
    kF16sBranches,   // trunk, then f16s_value_branch and f16s_policy_branch (the caller picks their streams)
};
// every choice between launch variants, made once per forward by f16s_plan and nowhere else
struct F16sPlan {
    int batch, bits;
    bool heads;             // the path computes the heads itself (af_net_tune key 9)
    F16sForm form;          // kF16sRoles and kF16sPaired need `heads`
    bool valu_stem, two_wg_per_cu, half_classes, tile_split, fused_blocks;
};
F16sPlan f16s_plan(const f16s_net* n, int batch, int bits, bool heads);
// forms kF16sRoles and kF16sPaired: the whole forward on stream st -> value [batch], policy [batch][121]
int f16s_forward(f16s_net* n, const F16sPlan& p, hipStream_t st, const float* planes_dev, float* value, float* policy);
// form kF16sBranches, in three parts.  Stem + bone/block1 + bone/block2 on stream st:
int f16s_trunk(f16s_net* n, const F16sPlan& p, hipStream_t st, const float* planes_dev);
// value/block3, policy/block4+5.  p.heads: the branch's last conv also applies the head's 1x1 convolution and the head's dense layer
// runs on the same split-operand MFMA (af_value_fc_f16s / af_policy_fc_f16s) -> value [batch] / policy [batch][S*S].  Otherwise
// -> o3 / o5: fp32 planes [batch][32][PP], pixel (y,x) at (y+1)*WP + x+1 (the fp32 head kernels' input)
int f16s_value_branch(f16s_net* n, const F16sPlan& p, hipStream_t st, float* o3_dev, int WP, int PP, float* value);
int f16s_policy_branch(f16s_net* n, const F16sPlan& p, hipStream_t st, float* o5_dev, int WP, int PP, float* policy);
int f16s_small_forward_error(f16s_net* n);                         // 1 if a role of kF16sRoles ever gave up waiting (synchronises)
int f16s_read_activation(f16s_net* n, int which, int batch, float* host);

// ---- weight packing, from device memory and in place: the one packer of this path (af_net_finalize over the variables it staged,
// af_net_update_device over the caller's tensors) ----
// src: the 42 variables as fp32 TF-layout tensors in DEVICE memory, in kNetVars' order (af_net.hip has checked names and counts)
constexpr int kF16sScaleGroups = 20;       // stem | per block: conv1, conv2 (+ folded projection), produced projection | 2 head convs | value/fc1 | policy/fc
// max|w| of every scale group -> max_dev[kF16sScaleGroups] (device; NaN elements do not count), asynchronous on st
int f16s_update_absmax(f16s_net* n, hipStream_t st, const float* const* src, float* max_dev);
// pack every weight-derived buffer of the split-operand path in place from src, each scale group with the power-of-two scale its
// max_host[group] picks, asynchronous on st, and store the new inverse scales in the handle; max_host = what f16s_update_absmax
// produced, already on the host
int f16s_update_pack(f16s_net* n, hipStream_t st, const float* const* src, const float* max_host);
// weight-derived device buffers in a fixed order (af_net_debug_weights): 0 on success, -1 past the last one
int f16s_weight_buffer(const f16s_net* n, int index, const void** ptr, size_t* bytes);
int f16s_scales(const f16s_net* n, float* out, int cap);           // the 25 inverse scales (af_net_debug_scales); returns how many
// elementwise device copies shared by both paths' packing: dst[i] = i < n_src ? (sum ? a[i] + (b ? b[i] : 0.0f) : a[i]) : 0.0f, i < n_dst
struct UpdCopy { float* dst; const float* a; const float* b; int n_dst, n_src, sum; };
int upd_launch_copies(hipStream_t st, const UpdCopy* d, int count);

#endif
