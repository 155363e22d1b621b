// DTYPE 'float16' / 'bfloat16': ConvLayer(..., depthwise=True) on the 16-bit-resident c8 tensors of the conv stack
// ([N][ceil(C/8)][P][P][8] 16-bit values; x / dx: S x S maps at pitch P, y / dz: So x So maps at pitch Po): tn_c8_dwconv_fwd
// / _dgrad / _wgrad, the kernels of dwconv.h with the 16-byte cell -- 8 channels of one pixel -- as the unit: a depthwise
// product never leaves the cell, so there is no cross-lane traffic and no operand arrangement, and an f x f sliding window
// over cells is the whole computation.  The arguments are tn_c8_convg_*'s without K; f is 3 or 5.
// Arithmetic: the stack's -- x and dz as stored, W rounded to the element type (nearest even) when a block stages it,
// exact products (two 16-bit values: at most 22 significant bits), fp32 accumulation, bias / activation on the fp32
// sums, one rounding when a cell is stored; dz and dx carry the gradient scale, the fp32 epilogue of the weight
// gradient removes it and sums db from the stored dz.  Every cell of y / dx is written by the op: pad cells at a pitch
// above the side, channels past C in a ragged last octet and input pixels no strided window touches as exact +0.
// Index range: fewer than 2^32 cells per tensor, at most 65535 octets, stride <= 16 (dwconv.h: a one-lane tile fits LDS).
#include "c8_elem.h"
#include "dwconv.h"

template <typename E>
struct DwC8 {
    typedef uint4 cell;
    static constexpr int L = 8;
    static __device__ __forceinline__ void load(const uint4& c, float (&x)[8]) {
        const typename E::v8 v = __builtin_bit_cast(typename E::v8, c);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = (float)v[e];
    }
    static __device__ __forceinline__ uint4 pack(const float (&v)[8]) {
        typename E::v8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (typename E::T)v[e];
        return __builtin_bit_cast(uint4, r);
    }
    static __device__ __forceinline__ float wround(float w) { return (float)(typename E::T)w; }
    static __device__ __forceinline__ uint4 zero() { return make_uint4(0u, 0u, 0u, 0u); }
};

// cells of a c8 tensor of N x C maps of S pixels a side at pitch P (tn_c8_pool_supported's rule), or -1
static long long dw8_cells(int N, int C, int S, int P) {
    if (N <= 0 || C <= 0 || S <= 0 || P < S || (P != S && (P & (P - 1)))) return -1;
    const long long cells = (long long)N * ((C + 7) / 8) * P * P;
    return cells < (1ll << 32) ? cells : -1;
}

static bool dw8_ok(int N, int C, int S, int P, int f, int stride, int pad, int So, int Po) {
    if ((f != 3 && f != 5) || stride < 1 || stride > DW_STRIDE_MAX || (C + 7) / 8 > 65535) return false;
    return dw8_cells(N, C, S, P) >= 0 && dw8_cells(N, C, So, Po) >= 0 && dw_axis_ok(S, f, stride, pad, So);
}

#define DW8_ARGS_FMT "(N %d, %d maps of %d pixels at pitch %d -> %d pixels at pitch %d, filter %d stride %d pad_lo %d)"
#define DW8_ARGS N, C, S, P, So, Po, f, stride, pad

extern "C" {

#ifndef C8_BF16_TU
// the bf16 entry points (dwconv_c8_bf16.hip)
int c8b_tn_c8_dwconv_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P, int f,
                         int stride, int pad, int So, int Po, int act, float prm);
int c8b_tn_c8_dwconv_dgrad(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int f, int stride,
                           int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm);
int c8b_tn_c8_dwconv_wgrad(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P, int f,
                           int stride, int pad, int So, int Po);

// 1 if the depthwise c8 kernels take a layer of this geometry (forward, both gradients; either element type)
int tn_c8_dwconv_supported(int N, int C, int S, int P, int f, int stride, int pad, int So, int Po) {
    return dw8_ok(N, C, S, P, f, stride, pad, So, Po) ? 1 : 0;
}
#endif

// y = act(dwconv(x, W) + b)
int C8_API(tn_c8_dwconv_fwd)(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P,
                             int f, int stride, int pad, int So, int Po, int act, float prm) {
    C8_TO_BF16(tn_c8_dwconv_fwd, ctx, x, W, b, y, N, C, S, P, f, stride, pad, So, Po, act, prm);
    TN_REQUIRE(x && W && b && y && dw8_ok(N, C, S, P, f, stride, pad, So, Po), "tn_c8_dwconv_fwd: bad arguments " DW8_ARGS_FMT,
               DW8_ARGS);
    DwGeom g{};
    g.src = x; g.out = y; g.W = W; g.bias = b; g.act = act; g.prm = prm;
    g.CP = (unsigned)((C + 7) / 8); g.planes = (unsigned)N * g.CP; g.C = C;
    g.Hs = g.Ws = S; g.Ps = P; g.PPs = (unsigned)P * P;
    g.Ho = g.Wo = So; g.OH = g.OW = Po; g.PPo = (unsigned)Po * Po;
    g.stride = stride; g.pad = pad;
    return dw_run<DwC8<C8E>>(ctx, g, f, 0);
}

// dx = (transposed dwconv of dz with W) * act'(prev_a) (prev_a NULL: none)
int C8_API(tn_c8_dwconv_dgrad)(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int f,
                               int stride, int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm) {
    C8_TO_BF16(tn_c8_dwconv_dgrad, ctx, dz, W, dx, N, C, S, P, f, stride, pad, So, Po, prev_a, prev_act, prev_prm);
    TN_REQUIRE(dz && W && dx && dw8_ok(N, C, S, P, f, stride, pad, So, Po), "tn_c8_dwconv_dgrad: bad arguments " DW8_ARGS_FMT,
               DW8_ARGS);
    DwGeom g{};
    g.src = dz; g.out = dx; g.W = W; g.prev_a = prev_a; g.act = prev_act; g.prm = prev_prm;
    g.CP = (unsigned)((C + 7) / 8); g.planes = (unsigned)N * g.CP; g.C = C;
    g.Hs = g.Ws = So; g.Ps = Po; g.PPs = (unsigned)Po * Po;
    g.Ho = g.Wo = S; g.OH = g.OW = P; g.PPo = (unsigned)P * P;
    g.stride = stride; g.pad = stride == 1 ? f - 1 - pad : pad;
    return dw_run<DwC8<C8E>>(ctx, g, f, 1);
}

// dW (C, 1, f, f), db (C) from x and dz; dz carries the gradient scale, the results do not.  OVERWRITE
int C8_API(tn_c8_dwconv_wgrad)(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P,
                               int f, int stride, int pad, int So, int Po) {
    C8_TO_BF16(tn_c8_dwconv_wgrad, ctx, x, dz, dW, db, N, C, S, P, f, stride, pad, So, Po);
    TN_REQUIRE(x && dz && dW && db && dw8_ok(N, C, S, P, f, stride, pad, So, Po),
               "tn_c8_dwconv_wgrad: bad arguments " DW8_ARGS_FMT, DW8_ARGS);
    DwWGeom g{};
    g.x = x; g.dz = dz; g.CP = (unsigned)((C + 7) / 8); g.C = C;
    g.Hs = g.Ws = S; g.Ps = P; g.PPs = (unsigned)P * P;
    g.Ho = g.Wo = So; g.OW = Po; g.PPo = (unsigned)Po * Po;
    g.stride = stride; g.pad = pad; g.oscale = 1.f / ctx->grad_scale;
    return dw_run_wgrad<DwC8<C8E>>(ctx, g, f, N, dW, db);
}

}  // extern "C"
