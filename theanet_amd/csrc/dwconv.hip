// ConvLayer(..., depthwise=True) on fp32 NCHW tensors: tn_dwconv_fwd / _dgrad / _wgrad, the kernels of dwconv.h on scalar
// planes -- one (image, channel) plane a lane group, T::L = 1.  The arguments are tn_conv2d_*'s without K (the layer has
// C maps in and out, W (C, 1, f, f), b (C)); f is 3 or 5.  The ops are fp32 whatever the net's CONV param says: CONV
// 'bfloat16' rounds the operands of a MATRIX product, and a depthwise layer has none -- it runs these kernels unchanged.
// Like tn_conv2d_* they refuse to run while a 16-bit DTYPE is in force (its entry points are tn_c8_dwconv_*).
#include "dwconv.h"

struct DwF32 {
    typedef float cell;
    static constexpr int L = 1;
    static __device__ __forceinline__ void load(const float& c, float (&x)[1]) { x[0] = c; }
    static __device__ __forceinline__ float pack(const float (&v)[1]) { return v[0]; }
    static __device__ __forceinline__ float wround(float w) { return w; }
    static __device__ __forceinline__ float zero() { return 0.f; }
};

static bool dwf_ok(int N, int C, int H, int Wd, int f, int stride, int pad, int Ho, int Wo) {
    if (N < 1 || C < 1 || C > 65535 || (f != 3 && f != 5) || stride < 1 || stride > DW_STRIDE_MAX) return false;
    if (H > 65535 || Wd > 65535) return false;               // (the tile grid: rows in y, columns in z)
    if (!dw_axis_ok(H, f, stride, pad, Ho) || !dw_axis_ok(Wd, f, stride, pad, Wo)) return false;
    const long long planes = (long long)N * C;
    return planes * H * Wd < (1ll << 32) && planes * Ho * Wo < (1ll << 32);
}

#define DWF_ARGS_FMT "(N %d, %d maps of %d x %d -> %d x %d, filter %d stride %d pad_lo %d)"
#define DWF_ARGS N, C, H, Wd, Ho, Wo, f, stride, pad

extern "C" {

int tn_dwconv_supported(int N, int C, int H, int Wd, int f, int stride, int pad, int Ho, int Wo) {
    return dwf_ok(N, C, H, Wd, f, stride, pad, Ho, Wo) ? 1 : 0;
}

int tn_dwconv_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int N, int C, int H, int Wd, int f,
                  int stride, int pad, int Ho, int Wo, int act, float prm) {
    TN_REQUIRE(x && W && b && a && dwf_ok(N, C, H, Wd, f, stride, pad, Ho, Wo), "tn_dwconv_fwd: bad arguments " DWF_ARGS_FMT,
               DWF_ARGS);
    TN_FP32_ONLY(ctx, "tn_dwconv_fwd");
    DwGeom g{};
    g.src = x; g.out = a; g.W = W; g.bias = b; g.act = act; g.prm = prm;
    g.planes = (unsigned)N * C; g.CP = (unsigned)C; g.C = C;
    g.Hs = H; g.Ws = Wd; g.Ps = Wd; g.PPs = (unsigned)H * Wd;
    g.Ho = g.OH = Ho; g.Wo = g.OW = Wo; g.PPo = (unsigned)Ho * Wo;
    g.stride = stride; g.pad = pad;
    return dw_run<DwF32>(ctx, g, f, 0);
}

int tn_dwconv_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int N, int C, int H, int Wd, int f, int stride,
                    int pad, int Ho, int Wo, const float* prev_a, int prev_act, float prev_prm) {
    TN_REQUIRE(dz && W && dx && dwf_ok(N, C, H, Wd, f, stride, pad, Ho, Wo), "tn_dwconv_dgrad: bad arguments " DWF_ARGS_FMT,
               DWF_ARGS);
    TN_FP32_ONLY(ctx, "tn_dwconv_dgrad");
    DwGeom g{};
    g.src = dz; g.out = dx; g.W = W; g.prev_a = prev_a; g.act = prev_act; g.prm = prev_prm;
    g.planes = (unsigned)N * C; g.CP = (unsigned)C; g.C = C;
    g.Hs = Ho; g.Ws = Wo; g.Ps = Wo; g.PPs = (unsigned)Ho * Wo;
    g.Ho = g.OH = H; g.Wo = g.OW = Wd; g.PPo = (unsigned)H * Wd;
    g.stride = stride; g.pad = stride == 1 ? f - 1 - pad : pad;
    return dw_run<DwF32>(ctx, g, f, 1);
}

int tn_dwconv_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int N, int C, int H, int Wd, int f,
                    int stride, int pad, int Ho, int Wo) {
    TN_REQUIRE(x && dz && dW && db && dwf_ok(N, C, H, Wd, f, stride, pad, Ho, Wo),
               "tn_dwconv_wgrad: bad arguments " DWF_ARGS_FMT, DWF_ARGS);
    TN_FP32_ONLY(ctx, "tn_dwconv_wgrad");
    DwWGeom g{};
    g.x = x; g.dz = dz; g.CP = (unsigned)C; g.C = C;
    g.Hs = H; g.Ws = Wd; g.Ps = Wd; g.PPs = (unsigned)H * Wd;
    g.Ho = Ho; g.Wo = g.OW = Wo; g.PPo = (unsigned)Ho * Wo;
    g.stride = stride; g.pad = pad; g.oscale = 1.f;
    return dw_run_wgrad<DwF32>(ctx, g, f, N, dW, db);
}

}  // extern "C"
