// Grouped convolution (ConvLayer(..., groups=g): the C maps and the K filters are cut into g groups, filter k reads the
// C/g maps of group k / (K/g) alone; W (K, C/g, f, f) in tn_conv2d_*'s orientation, b (K)) -- what the two families share:
// gconv.hip (fp32 NCHW, tn_gconv_*) and gconv_c8.hip (the 16-bit conv stack, tn_c8_gconv_*).
//
// One launch a product for the whole layer: the group is a grid dimension, a block works inside ONE group, so no product is
// ever issued on the zero blocks of the block-diagonal dense form.
//
// Forward and input gradient are the same kernel (MODE 0 forward; 1 input gradient of a stride-1 layer: the forward with
// the roles of C/g and K/g swapped, the taps unflipped and the padding f - 1 - pad; 2 input gradient of a strided layer: a
// gather over the windows that cover a pixel, none for a pixel no window touches).  A block owns a TH x TW tile of one
// image's output plane and stages the SOURCE tile its windows read -- the group's reduced maps, f - 1 halo included, +0
// outside the map -- in LDS once; every tap is then an address offset into that tile.  gc_src0 / gc_src_dim say where the
// staged tile starts and how long it is along an axis; the tile shrinks until it fits GC_LDS_MAX (two blocks a CU out of
// gfx950's 160 KB), and a geometry whose smallest tile does not fit reads the source straight from HBM (`direct`).
#pragma once
#include "common.h"

#define GC_LDS_MAX (64 << 10)

__host__ __device__ __forceinline__ int gc_ceil_div(int a, int s) { return a >= 0 ? (a + s - 1) / s : -((-a) / s); }

// first source coordinate of the tile whose first output coordinate is o0 (off0: source coordinate of the tap with offset 0
// at output 0: -pad forward, pad - (f - 1) input gradient)
__host__ __device__ __forceinline__ int gc_src0(int mode, int o0, int off0, int s) {
    return mode == 2 ? gc_ceil_div(o0 + off0, s) : o0 * (mode == 0 ? s : 1) + off0;
}
// source coordinates a tile of T outputs reads along one axis
static inline int gc_src_dim(int mode, int T, int f, int s) {
    return mode == 2 ? (T + f - 2) / s + 1 : (T - 1) * (mode == 0 ? s : 1) + f;
}

// consistent geometry along one axis (tn_c8_convg_supported's rule): So windows fit and no more, no more padding than a
// 'same' layer's
static inline bool gc_axis_ok(int S, int f, int stride, int pad, int So) {
    if (S < 1 || So < 1 || f < 1 || stride < 1 || pad < 0 || f >= (1 << 15) || stride >= (1 << 15)) return false;
    const long long hi = (long long)(So - 1) * stride + f - pad - S;
    return pad <= f / 2 && hi <= pad && hi > -(long long)stride;
}

static inline bool gc_groups_ok(int C, int K, int g) { return g >= 1 && C >= 1 && K >= 1 && C % g == 0 && K % g == 0; }

// Narrow groups on the 16-bit stack (gconv_c8_narrow.hip): 2 or 4 maps a group in and out, whole cells of 8 in all -- an
// output cell reads the input cell with the same index alone
static inline bool gc_narrow(int C, int K, int g) {
    return gc_groups_ok(C, K, g) && C == K && C % 8 == 0 && (C / g == 2 || C / g == 4);
}
// what they ask beyond the family's rule, and the narrow branches of tn_c8_gconv_* (c8b_: the bf16 unit's)
bool gc8n_ok(int C, int S, int P, int f, int stride, int pad, int So, int Po);
#define GC8N_DECLARE(pre)                                                                                                          \
    int pre##gc8n_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P, int g,     \
                      int f, int stride, int pad, int So, int Po, int act, float prm);                                            \
    int pre##gc8n_dgrad(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int g, int f,          \
                        int stride, int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm);                   \
    int pre##gc8n_wgrad(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P, int g,      \
                        int f, int stride, int pad, int So, int Po);
GC8N_DECLARE()
GC8N_DECLARE(c8b_)

// Slabs of a weight gradient whose grid has `cols` blocks a slab over `nt` pixel tiles: `target` blocks in all (a constant,
// no CU count: the order of additions is the geometry's alone), at most one slab a tile.
static inline unsigned gc_slabs(long long nt, long long cols, long long target) {
    const long long want = (target + cols - 1) / cols;
    return (unsigned)(want < 1 ? 1 : (want > nt ? nt : want));
}
