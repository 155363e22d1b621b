// CONV 'bfloat16' (opt-in, training param; default off): the three products of a ConvLayer (theanet/layer/convpool.py:54-72
// and their gradients) at bf16 precision for EVERY geometry tn_conv2d_* takes -- any N, C, K, any square filter, 'valid' and
// 'same', any stride, any map size.  The counterpart of MATMUL 'bfloat16' (gemm_bf16.hip) for the conv layers.
//
// Tensors in HBM stay fp32 NCHW (activations, dz, master weights, dW, db).  Both operands of every product are rounded to
// bf16 (nearest even, the (__bf16) conversion gemm_bf16.hip uses) while their tile is staged into LDS; products are exact
// and accumulate in fp32 on v_mfma_f32_32x32x16_bf16; bias, activation and act' run on the fp32 sums in the epilogue.  db is
// the fp32 sum of the UNROUNDED dz (it is no product).  A reduced-precision mode: results differ from the fp32 path's by
// ~2^-9 of the operands' magnitude per product term.  No gradient scale: bf16 has fp32's exponent range.
//
// Implicit GEMM, no im2col buffer: the pixel operand is gathered from the NCHW tensor while it is staged.
//   forward : out[k][m] = act(b[k] + sum_kk W[k][kk] . G[kk][m]),  kk = (c, u', v') in W's native order,
//             G[kk][m] = x[n, c, i*s - pad + f-1-u', j*s - pad + f-1-v'] (the flip of the true convolution on the gather side)
//   dgrad   : the same kernel: rows = the C input maps, kk = (k, u', v'), weight element W[k][c][u'][v'], gathered element
//             dz[n, k, (y + pad - (f-1) + u') / s, (x + pad - (f-1) + v') / s] where the stride divides (otherwise zero)
//   wgrad   : dW[k][kk] = sum_m dz[k][m] . G[kk][m] over the N*Ho*Wo pixels, split over pixel slabs that meet in context
//             scratch and are summed in slab order by the context's reduction (tn_red_wgrad): no atomics.
// Both operands sit in LDS reduction-contiguous, rows of 32 bf16 + 16 bytes (80 bytes: the 16-byte slots of 16 consecutive
// rows fall into distinct banks), read with ds_read_b128 straight into MFMA operands; lanes <-> pixels in the forward /
// dgrad epilogue (coalesced NCHW stores), lanes <-> kk in the weight gradient.  Two LDS stages: tile t+1 is fetched into
// registers before the matrix work on tile t and written to the other buffer after it -- one barrier per tile.
// Whatever lies outside an operand -- a ragged reduction tail, rows / pixels past the end, taps outside the image, taps the
// stride does not divide -- is staged as zero from a clamped (valid) address; ragged output tails are not stored.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

#define CB_BK 32            // reduction depth of a tile: two 16-deep MFMA steps
#define CB_ROW 80           // bytes of an LDS row (32 bf16 + 16)
#define CB_PIX 128          // pixels of a forward / dgrad block (32 per wave)

struct CbArgs {
    const float* src;       // gathered tensor (N, Cs, Hs, Ws): x (forward) or dz (dgrad)
    const float* W;         // (K, C, f, f) master weights
    float* out;             // (N, R, Hd, Wd)
    const float* bias;      // forward
    const float* prev_a;    // dgrad: act'(prev_a) in the epilogue, or NULL
    int N, Cs, Hs, Ws;
    int R;                  // maps of the output = weight-side rows of the product
    int Hd, Wd;             // size of an output map
    int f, stride;
    int off0;               // source coordinate of tap offset 0 at output pixel 0: -pad (forward), pad - (f-1) (dgrad)
    int Kd;                 // Cs * f * f
    int M;                  // N * Hd * Wd
    int w_row, w_grp;       // weight element of (row, kk): W[row * w_row + (kk / ff) * w_grp + kk % ff]
    int act;
    float prm;
};

__device__ __forceinline__ bf16x8 cb_round8(const float* v) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (__bf16)v[j];
    return r;
}

// NM: 32-row tiles of maps per block (1: 32 maps, 2: 64 maps); every wave owns 32 pixels and all NM map tiles
template <bool DGRAD, int NM>
__global__ __launch_bounds__(256) void conv_bf16_kernel(CbArgs g) {
    constexpr int WROWS = 32 * NM;
    constexpr int PPL = CB_PIX * CB_ROW, STAGE = PPL + WROWS * CB_ROW;
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];          // 25 / 30 KB
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const int m0 = blockIdx.x * CB_PIX, r0 = blockIdx.y * WROWS;
    const int ff = g.f * g.f, HWs = g.Hs * g.Ws, HWd = g.Hd * g.Wd;

    // ---- pixel operand: thread = (pixel t & 127, 16 consecutive kk of the tile: half t >> 7, wave-uniform) ----
    const int pp = t & 127, ph = t >> 7;
    const bool mok = m0 + pp < g.M;
    int by, bx;
    const float* sbase;
    {
        const int mm = min(m0 + pp, g.M - 1);
        const int n = mm / HWd, r = mm - n * HWd, i = r / g.Wd, j = r - i * g.Wd;
        by = (DGRAD ? i : i * g.stride) + g.off0;
        bx = (DGRAD ? j : j * g.stride) + g.off0;
        sbase = g.src + (size_t)n * g.Cs * HWs;
    }
    // ---- weight operand: thread = (row t >> 3 of each 32-row tile, 4 consecutive kk) ----
    const int wrow = t >> 3, wk = (t & 7) * 4;

    float rp[16], rw[NM][4];
    auto gload = [&](int ks) __attribute__((always_inline)) {
        {
            const int kk = ks + 16 * ph;
            int c = kk / ff;
            const int r = kk - c * ff;
            int u = r / g.f, v = r - u * g.f;
            bool ok[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                int sy = by + (DGRAD ? u : g.f - 1 - u), sx = bx + (DGRAD ? v : g.f - 1 - v);
                bool o = mok && c < g.Cs;
                if (DGRAD && g.stride > 1) {          // only the taps the stride divides contribute
                    o = o && sy >= 0 && sx >= 0;
                    const int qy = sy / g.stride, qx = sx / g.stride;
                    o = o && qy * g.stride == sy && qx * g.stride == sx;
                    sy = qy; sx = qx;
                }
                o = o && (unsigned)sy < (unsigned)g.Hs && (unsigned)sx < (unsigned)g.Ws;
                ok[j] = o;
                rp[j] = sbase[o ? c * HWs + sy * g.Ws + sx : 0];
                if (++v == g.f) { v = 0; if (++u == g.f) { u = 0; ++c; } }
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) rp[j] = ok[j] ? rp[j] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < NM; ++q) {
            const int row = r0 + wrow + 32 * q;
            const int kk = ks + wk;
            int c = kk / ff, r = kk - c * ff;
            bool ok[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ok[e] = row < g.R && c < g.Cs;
                rw[q][e] = g.W[ok[e] ? (size_t)row * g.w_row + (size_t)c * g.w_grp + r : 0];
                if (++r == ff) { r = 0; ++c; }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) rw[q][e] = ok[e] ? rw[q][e] : 0.f;
        }
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
        char* sp = lds + buf * STAGE;
        char* sw = sp + PPL;
        *reinterpret_cast<bf16x8*>(sp + pp * CB_ROW + ph * 32) = cb_round8(rp);
        *reinterpret_cast<bf16x8*>(sp + pp * CB_ROW + ph * 32 + 16) = cb_round8(rp + 8);
#pragma unroll
        for (int q = 0; q < NM; ++q) {
            bf16x4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = (__bf16)rw[q][e];
            *reinterpret_cast<bf16x4*>(sw + (wrow + 32 * q) * CB_ROW + wk * 2) = w;
        }
    };

    f32x16 acc[NM];
#pragma unroll
    for (int q = 0; q < NM; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    const int p_rd = (wave * 32 + l31) * CB_ROW + hi * 16, w_rd = PPL + l31 * CB_ROW + hi * 16;
    gload(0);
    lstore(0);
    __syncthreads();
    int buf = 0;
    for (int ks = 0; ks < g.Kd; ks += CB_BK) {
        const bool more = ks + CB_BK < g.Kd;            // (block-uniform)
        if (more) gload(ks + CB_BK);
        __builtin_amdgcn_sched_barrier(0);              // (the loads stay above the matrix work that hides them)
        const char* st = lds + buf * STAGE;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(st + p_rd + s * 32);
#pragma unroll
            for (int q = 0; q < NM; ++q) {
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(st + w_rd + q * 32 * CB_ROW + s * 32);
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[q], 0, 0, 0);
            }
        }
        if (more) lstore(buf ^ 1);                      // the other buffer was last read before the previous barrier
        __syncthreads();
        buf ^= 1;
    }

    // ---- epilogue: lane = pixel (32 consecutive per half-wave: coalesced along a map), registers = maps ----
    const int m = m0 + wave * 32 + l31;
    if (m >= g.M) return;
    const int n = m / HWd, p = m - n * HWd;
#pragma unroll
    for (int q = 0; q < NM; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + 32 * q + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (row >= g.R) continue;
            const size_t o = ((size_t)n * g.R + row) * HWd + p;
            float v = acc[q][r];
            if (DGRAD) {
                if (g.prev_a) v *= tn_act_grad_from_out(g.prev_a[o], g.act, g.prm);
            } else {
                v = tn_act_fwd(v + g.bias[row], g.act, g.prm);
            }
            g.out[o] = v;
        }
}

// ---- weight gradient: rows = filters k (operand dz), columns = kk = (c, u', v') (operand gathered from x), reduction over
// the pixels of slab blockIdx.z.  Block 64 x 64, four waves of 32 x 32; thread = (row t >> 2, 8 consecutive pixels): the
// filter row and the kk row of a thread walk the SAME pixels. ----
struct CwArgs {
    const float* x;         // (N, C, H, Wd)
    const float* dz;        // (N, K, Ho, Wo)
    float* out;             // [S][K][Kd] slabs (or dW itself when S == 1)
    float* dbout;           // [S][K] (or db)
    int N, C, H, Wd, K, f, stride, pad, Ho, Wo;
    int Kd, M, mchunk;      // C * f * f, N * Ho * Wo, pixels of a slab (a multiple of 32)
};

__global__ __launch_bounds__(256) void conv_bf16_wgrad_kernel(CwArgs g) {
    constexpr int PL = 64 * CB_ROW, STAGE = 2 * PL;
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];          // 20 KB
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const int c0 = blockIdx.x * 64, k0 = blockIdx.y * 64, z = blockIdx.z;
    const int mbeg = z * g.mchunk, mend = min(g.M, mbeg + g.mchunk);
    const int ff = g.f * g.f, HW = g.H * g.Wd, HoWo = g.Ho * g.Wo;
    const int row = t >> 2, mo = (t & 3) * 8;
    const bool aok = k0 + row < g.K, kok = c0 + row < g.Kd;
    const int arow = min(k0 + row, g.K - 1);
    int xc, du, dv;
    {
        const int kk = min(c0 + row, g.Kd - 1);
        xc = kk / ff;
        const int r = kk - xc * ff;
        du = g.f - 1 - r / g.f - g.pad;
        dv = g.f - 1 - r % g.f - g.pad;
    }

    float ra[8], rb[8], asum = 0.f;
    auto gload = [&](int ms) __attribute__((always_inline)) {
        const int mm = min(ms + mo, g.M - 1);
        int n = mm / HoWo;
        const int r = mm - n * HoWo;
        int i = r / g.Wo, j = r - i * g.Wo;
        bool oa[8], ob[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool in = ms + mo + e < mend;
            oa[e] = in && aok;
            ra[e] = g.dz[oa[e] ? ((size_t)n * g.K + arow) * HoWo + i * g.Wo + j : 0];
            const int sy = i * g.stride + du, sx = j * g.stride + dv;
            ob[e] = in && kok && (unsigned)sy < (unsigned)g.H && (unsigned)sx < (unsigned)g.Wd;
            rb[e] = g.x[ob[e] ? ((size_t)n * g.C + xc) * HW + sy * g.Wd + sx : 0];
            if (++j == g.Wo) { j = 0; if (++i == g.Ho) { i = 0; ++n; } }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            ra[e] = oa[e] ? ra[e] : 0.f;
            rb[e] = ob[e] ? rb[e] : 0.f;
        }
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
        char* sa = lds + buf * STAGE;
        *reinterpret_cast<bf16x8*>(sa + row * CB_ROW + mo * 2) = cb_round8(ra);
        *reinterpret_cast<bf16x8*>(sa + PL + row * CB_ROW + mo * 2) = cb_round8(rb);
#pragma unroll
        for (int e = 0; e < 8; ++e) asum += ra[e];           // bias gradient: the unrounded dz, in pixel order
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int wm = wave & 1, wn = wave >> 1;
    const int a_rd = (wm * 32 + l31) * CB_ROW + hi * 16, b_rd = PL + (wn * 32 + l31) * CB_ROW + hi * 16;

    gload(mbeg);
    lstore(0);
    __syncthreads();
    int buf = 0;
    for (int ms = mbeg; ms < mend; ms += CB_BK) {
        const bool more = ms + CB_BK < mend;
        if (more) gload(ms + CB_BK);
        __builtin_amdgcn_sched_barrier(0);
        const char* st = lds + buf * STAGE;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(st + a_rd + s * 32);
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(st + b_rd + s * 32);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // bias gradient of the slab: the four lanes of a filter row, added in a fixed order
    if (blockIdx.x == 0) {
        asum += __shfl_xor(asum, 1, 64);
        asum += __shfl_xor(asum, 2, 64);
        if ((t & 3) == 0 && aok) g.dbout[(size_t)z * g.K + k0 + row] = asum;
    }
    // lane = kk (contiguous in dW), registers = filters
    const int col = c0 + wn * 32 + l31;
    if (col >= g.Kd) return;
    float* out = g.out + (size_t)z * g.K * g.Kd;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = k0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (k < g.K) out[(size_t)k * g.Kd + col] = acc[r];
    }
}

// ---- launchers (tn_conv2d_* dispatch here, before any of their own branches, while tn_set_conv_matmul(ctx, 2) holds) ----
#define CB_SHAPE_OK(name)                                                                                                   \
    TN_REQUIRE(!ctx->mm_f16, name " (CONV 'bfloat16'): a 16-bit DTYPE is set (its conv stack already runs 16-bit products)"); \
    TN_REQUIRE(N > 0 && C > 0 && H > 0 && Wd > 0 && K > 0 && f > 0 && stride > 0 && pad >= 0 && Ho > 0 && Wo > 0,             \
               name " (CONV 'bfloat16'): bad shape (N %d C %d H %d W %d K %d f %d stride %d pad_lo %d Ho %d Wo %d)", N, C, H,  \
               Wd, K, f, stride, pad, Ho, Wo);                                                                              \
    TN_REQUIRE((long long)N * C * H * Wd < (1ll << 31) && (long long)N * K * Ho * Wo < (1ll << 31) &&                         \
                   (long long)K * C * f * f < (1ll << 31) && (long long)f * f < (1ll << 31) &&                                \
                   (long long)(Ho > H ? Ho : H) * stride + f + pad < (1ll << 31) && K <= 65535 * 32 && C <= 65535 * 32,        \
               name " (CONV 'bfloat16'): shape too large for 32-bit index arithmetic (N %d C %d H %d W %d K %d f %d stride "  \
                    "%d Ho %d Wo %d)", N, C, H, Wd, K, f, stride, Ho, Wo)

template <bool DGRAD>
static int cb_launch(tn_ctx* ctx, const CbArgs& g) {
    if (g.R > 32)
        conv_bf16_kernel<DGRAD, 2><<<dim3(cdiv(g.M, CB_PIX), cdiv(g.R, 64)), 256, 0, ctx->stream>>>(g);
    else
        conv_bf16_kernel<DGRAD, 1><<<dim3(cdiv(g.M, CB_PIX), 1), 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_cb_conv_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int N, int C, int H, int Wd, int K,
                   int f, int stride, int pad, int Ho, int Wo, int act, float prm) {
    TN_REQUIRE(x && W && b && a, "tn_conv2d_fwd (CONV 'bfloat16'): NULL tensor");
    CB_SHAPE_OK("tn_conv2d_fwd");
    CbArgs g{};
    g.src = x; g.W = W; g.out = a; g.bias = b;
    g.N = N; g.Cs = C; g.Hs = H; g.Ws = Wd; g.R = K; g.Hd = Ho; g.Wd = Wo; g.f = f; g.stride = stride; g.off0 = -pad;
    g.Kd = C * f * f; g.M = N * Ho * Wo; g.w_row = g.Kd; g.w_grp = f * f; g.act = act; g.prm = prm;
    return cb_launch<false>(ctx, g);
}

int tn_cb_conv_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int N, int C, int H, int Wd, int K, int f,
                     int stride, int pad, int Ho, int Wo, const float* prev_a, int act, float prm) {
    TN_REQUIRE(dz && W && dx, "tn_conv2d_dgrad (CONV 'bfloat16'): NULL tensor");
    CB_SHAPE_OK("tn_conv2d_dgrad");
    CbArgs g{};
    g.src = dz; g.W = W; g.out = dx; g.prev_a = prev_a;
    g.N = N; g.Cs = K; g.Hs = Ho; g.Ws = Wo; g.R = C; g.Hd = H; g.Wd = Wd; g.f = f; g.stride = stride; g.off0 = pad - (f - 1);
    g.Kd = K * f * f; g.M = N * H * Wd; g.w_row = f * f; g.w_grp = C * f * f; g.act = act; g.prm = prm;
    return cb_launch<true>(ctx, g);
}

int tn_cb_conv_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int N, int C, int H, int Wd, int K,
                     int f, int stride, int pad, int Ho, int Wo) {
    TN_REQUIRE(x && dz && dW && db, "tn_conv2d_wgrad (CONV 'bfloat16'): NULL tensor");
    CB_SHAPE_OK("tn_conv2d_wgrad");
    CwArgs g{};
    g.x = x; g.dz = dz; g.N = N; g.C = C; g.H = H; g.Wd = Wd; g.K = K; g.f = f; g.stride = stride; g.pad = pad; g.Ho = Ho;
    g.Wo = Wo; g.Kd = C * f * f; g.M = N * Ho * Wo;
    // pixel slabs: enough blocks for two per CU, at least 512 pixels (16 tiles) each
    const long long tiles = (long long)cdiv(g.Kd, 64) * cdiv(K, 64);
    long long S = (2ll * ctx->num_cus + tiles - 1) / tiles;
    if (S > g.M / 512) S = g.M / 512;
    if (S > 256) S = 256;
    if (S < 1) S = 1;
    g.mchunk = cdiv(cdiv(g.M, S), CB_BK) * CB_BK;
    const int Sx = cdiv(g.M, g.mchunk);
    const size_t n = (size_t)K * g.Kd;
    const dim3 grid(cdiv(g.Kd, 64), cdiv(K, 64), Sx);
    if (Sx == 1) {
        g.out = dW; g.dbout = db;
        conv_bf16_wgrad_kernel<<<grid, 256, 0, ctx->stream>>>(g);
        TN_LAUNCH_CHECK();
        return TN_OK;
    }
    float* ws;
    int rc = tn_scratch_get(ctx, (size_t)Sx * (n + K) * sizeof(float), &ws);
    if (rc) return rc;
    g.out = ws; g.dbout = ws + (size_t)Sx * n;
    conv_bf16_wgrad_kernel<<<grid, 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return tn_red_wgrad(ctx, g.out, dW, (uint32_t)n, (uint32_t)Sx, (uint32_t)n, g.dbout, db, (uint32_t)K, (uint32_t)Sx,
                        (uint32_t)K);
}
