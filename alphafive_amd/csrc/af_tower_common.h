// af_tower_common.h — what the translation units of libaf_tower.so share: af_tower_bf16.hip (the bf16 tower, the handle's
// allocation and the host setters) and af_tower_i8.hip (the int8 residual blocks).  The device helpers here are the ones both
// sets of kernels are made of — LDS-DMA, the ELU, the persistent workgroups' first position, the board geometry, the MFMA row
// permutation of the packers — and the handle struct is the one both files' host parts work on.
#ifndef AF_TOWER_COMMON_H
#define AF_TOWER_COMMON_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "af_tower_bf16.h"

#define TW_HIP_OK(expr)                                      \
    do {                                                     \
        hipError_t err_ = (expr);                            \
        if (err_ != hipSuccess) return AF_TOWER_ERR_HIP;     \
    } while (0)

// LDS-DMA: 16 bytes per lane from global memory into LDS at (wave-uniform lds_dst) + lane*16; counted on vmcnt.
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// ELU as max(x, min(exp(x), 1) - 1): x > 0 ? x : exp(x) - 1 with one v_max_f32 instead of compare + select and the clamp riding on
// v_exp_f32 (r3_44).  exp(x) - 1 > x for x < 0 and the clamped exponential is exactly 1 for x >= 0; only for -3e-4 < x < 0 can the
// rounding of v_exp_f32 put exp(x) - 1 below x, and the max then returns x, within 5e-8 of the true value (see af_conv_f16s.hip)
__device__ __forceinline__ float elu1(float x) {
    const float e = __builtin_amdgcn_exp2f(x * 1.44269504088896341f);
    return fmaxf(x, fminf(fmaxf(e, 0.0f), 1.0f) - 1.0f);
}

// First position of a persistent workgroup (r4, as in af_conv_f16s.hip): consecutive workgroup ids sit on consecutive XCDs, so with
// pos = blockIdx.x the 32 workgroups of XCD k would walk the positions = k (mod 8) only; XCD k takes the contiguous positions
// 32k..32k+31 (+ gridDim.x per pass) instead.  A position's result does not depend on the workgroup that computes it.
__device__ __forceinline__ int first_position() {
    if ((gridDim.x & 7) == 0) return (int)(blockIdx.x >> 3) + (int)(gridDim.x >> 3) * (int)(blockIdx.x & 7);
    return (int)blockIdx.x;
}

// Board geometry: every size below is a compile-time member of Geo<S> (as in af_conv_f16s.hip); the host forks once, in with_geo.
//   11x11: a position is one unit of work.  Its plane is 13 rows x 11 pixels (+1) = 144 units per channel octet, pixel n at unit
//          n + 11, and goes to LDS as it lies in memory: 9 LDS-DMA rounds of 256 lanes x 16 B.
//   15x15: 225 pixels are 8 pixel tiles and a 64-KB plane — neither the four accumulator sets nor three planes in LDS hold a whole
//          position — so the convolution runs every board as HALVES = 2 pseudo-positions: half 0 computes board rows 0..7 (120
//          pixels), half 1 rows 8..14 (105).  A half stages its rows plus one above and one below: 10 rows = 150 units per octet
//          from unit 120 * half of the 256-unit plane (half 1: the 135 units up to the plane's last row, the bottom zero row), gathered
//          by the per-lane addresses of the LDS-DMA into one contiguous half-plane of LPIX = 160 units per octet (a kg stride that
//          is a multiple of 128 B, as 144 is): 10 rounds.  Inside a half-plane pixel n of the half sits at unit n + 15, exactly as
//          pixel n sits at unit n + 11 above, so the tap addresses are the same expressions.
//          Stem, heads and dense layers work on whole positions: 8 pixel / output tiles.
constexpr uint32_t kLds0 = 256u;                                        // planes start here: unit -1 of a plane stays inside LDS
template <int S_> struct Geo;
template <> struct Geo<11> {
    static constexpr int S = 11, NPIX = 121, HALVES = 1;
    static constexpr int PIX = 144, LPIX = 144;                         // units per channel octet: in memory, in LDS
    static constexpr int HPIX0 = 121, HPIX1 = 121, HOFF = 0;            // pixels of half 0 / 1; plane unit where half 1 starts
    static constexpr int LIVE0 = 144, LIVE1 = 144;                      // units per octet a half stages
    static constexpr uint32_t kZeroB = 33024u;                          // all-zero LDS region the edge lanes read instead of a wrapped neighbour
    static constexpr int NT = 4;                                        // 32-pixel tiles of a whole position (= 32-output tiles of the policy)
    static constexpr int KP = 121, KV = 31, KVPAD = 496;                // k-steps of the policy / value-fc1 dense layers
};
template <> struct Geo<15> {
    static constexpr int S = 15, NPIX = 225, HALVES = 2;
    static constexpr int PIX = 256, LPIX = 160;
    static constexpr int HPIX0 = 120, HPIX1 = 105, HOFF = 120;
    static constexpr int LIVE0 = 150, LIVE1 = 135;
    static constexpr uint32_t kZeroB = (14u * 160u + 2u * 15u + 2u) * 16u + 272u;    // 36,624: the largest tap offset + a lane's bank offset + one unit
    static constexpr int NT = 8;
    static constexpr int KP = 225, KV = 57, KVPAD = 912;
};

__device__ __forceinline__ int pack_perm(int m) { return 16 * ((m >> 2) & 1) + 8 * (m >> 4) + 4 * ((m >> 3) & 1) + (m & 3); }   // MFMA row -> output: a lane's 16 accumulator rows are 16 consecutive outputs

// ------------------------------------------------------------------ host ------------------------------------------------------------------
// What the host needs of a geometry, as plain numbers: filled once, in af_tower_create, from Geo<S> (dims_of).
struct Dims {
    int S, npix, pix;               // board side, pixels, units per channel octet of the C8 layout
    int halves;                     // pseudo-positions per board of a convolution launch
    int rows_wp, rows_wv, pb_words; // the dense regions of the ends packer
    int ends_threads;
};

struct af_tower {
    int S = 0, width = 0, blocks = 0, device = 0;
    Dims d = {};
    int ncu = 0;                    // compute units of `device`: the persistent grid of a convolution launch
    char* arena = nullptr;          // the one allocation: every buffer of the table, the staging area and dump, at 256-byte offsets
    std::vector<char*> buf;         // 4 * blocks + 12 buffers; their addresses never change
    std::vector<char> set;          // per group: its host setter has run
    float* stage = nullptr;         // where a host setter's fp32 arrays wait for the packers
    char* dump = nullptr;
    // the int8 path (af_tower_i8.hip; 11x11 handles only): its buffers are part of the one allocation, empty until af_tower_i8_enable
    bool i8 = false;                // enabled: the pack paths run the int8 packers too
    std::vector<char*> qbuf;        // 4 per block: w1q, w2q, mb1, mb2 (af_tower_i8.hip)
    float* act = nullptr;           // [2][2 * blocks]: the activation scales a, then their reciprocals r
    float* keep = nullptr;          // every block's six fp32 source tensors as last packed: what a change of scales re-packs from
    mutable std::vector<char> qset; // per block: the int8 packers have run over it since the first enable (and the keep holds its sources)
    uint32_t* cal = nullptr;        // device calibration: 2 * blocks absmax words (bf16 magnitude bits), then status and count (int32)
    template <class T> T* block(int b, int k) const { return reinterpret_cast<T*>(buf[4 * b + k]); }
    template <class T> T* end(int k) const { return reinterpret_cast<T*>(buf[4 * blocks + k]); }
};

// ---- af_tower_i8.hip's part in the handle's life, called by af_tower_bf16.hip ----
// bytes of the int8 buffers inside the one allocation (0 on a handle the int8 path does not take) ...
size_t af_tower_i8_arena_bytes(const af_tower* t);
// ... their addresses, from p on; raises the kernels' LDS limit
int af_tower_i8_carve(af_tower* t, char* p);
// the int8 packers over blocks b0 .. b0 + nb - 1 from src (six device tensors per block, af_tower_update_device's order): called
// behind the bf16 packers on the same stream wherever those run, when the handle is enabled.  Launches only.
void af_tower_i8_pack(const af_tower* t, hipStream_t st, int b0, int nb, const float* const* src);

// ---- af_tower_bf16.hip's part in the device calibration, called by af_tower_i8.hip ----
// one bf16 layer of block b as af_tower_forward launches it (the persistent kernels under the tune keys, the same bits as every
// other form): second = 0 is x -> g, second = 1 is (g, x) -> x.  Launches only.  AF_TOWER_ERR_STATE while block b has no weights.
int af_tower_launch_layer(af_tower* t, hipStream_t st, int b, bool second, void* x_dev, void* g_dev, int batch);

// tune key 1 of af_tower_tune (persistent workgroups; 0 = one per CU), which the int8 convolutions honour too
int af_tower_grid_override();

#endif
