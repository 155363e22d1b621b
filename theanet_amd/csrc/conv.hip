// Direct (VALU) NCHW convolution kernels for small channel counts (C*f*f below the MFMA
// break-even, SURVEY.md section 7 "hard parts"): thread = one output pixel, KT output maps per
// thread, weights fetched with wave-uniform (scalar) loads.  HBM/L2-bound by design: x is
// read once from HBM (the f*f re-reads hit L1), a is written once.
//
// Semantics: theanet/layer/convpool.py:54-72 (true convolution, W is flipped).
#include "common.h"

// ------------------------------------------------------------------------------------
// forward: a = act(conv(x, W) + b)
// ------------------------------------------------------------------------------------
template <int F, int KT>
__global__ __launch_bounds__(256) void conv_fwd_direct(
    const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ b,
    float* __restrict__ a, int N, int C, int H, int Wd, int K, int f_rt, int stride, int pad,
    int Ho, int Wo, int act, float prm) {
    const int f = F ? F : f_rt;
    const int HoWo = Ho * Wo;
    const long long M = (long long)N * HoWo;
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    const int k0 = blockIdx.y * KT;
    if (m >= M) return;
    const int n = (int)(m / HoWo);
    const int p = (int)(m - (long long)n * HoWo);
    const int i = p / Wo, j = p - i * Wo;
    const int y0 = i * stride - pad, x0 = j * stride - pad;

    float acc[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) acc[kk] = (k0 + kk < K) ? b[k0 + kk] : 0.f;

    const int ff = f * f;
    for (int c = 0; c < C; ++c) {
        const float* xc = x + ((size_t)n * C + c) * H * Wd;
        const float* wc = W + ((size_t)k0 * C + c) * ff;
#pragma unroll
        for (int u = 0; u < f; ++u) {
            const int yy = y0 + u;
            const bool yok = (yy >= 0) && (yy < H);
#pragma unroll
            for (int v = 0; v < f; ++v) {
                const int xx = x0 + v;
                float xv = 0.f;
                if (yok && xx >= 0 && xx < Wd) xv = xc[yy * Wd + xx];
                const int widx = (f - 1 - u) * f + (f - 1 - v);
#pragma unroll
                for (int kk = 0; kk < KT; ++kk) {
                    // wave-uniform address -> s_load
                    const float wv = (k0 + kk < K) ? wc[(size_t)kk * C * ff + widx] : 0.f;
                    acc[kk] = fmaf(xv, wv, acc[kk]);
                }
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
        if (k0 + kk < K)
            a[((size_t)n * K + k0 + kk) * HoWo + p] = tn_act_fwd(acc[kk], act, prm);
    }
}

// ------------------------------------------------------------------------------------
// wgrad: partial[blk][k][c][u][v] (correlation order), db partial; second kernel reduces
// over blocks deterministically and writes the flipped dW.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int F, int KT, int CT>
__global__ __launch_bounds__(256) void conv_wgrad_direct(
    const float* __restrict__ x, const float* __restrict__ dz, float* __restrict__ partial,
    float* __restrict__ dbpartial, int N, int C, int H, int Wd, int K, int stride, int pad,
    int Ho, int Wo) {
    constexpr int FF = F * F;
    __shared__ float red[4][KT * CT * FF + KT];
    const int HoWo = Ho * Wo;
    const long long M = (long long)N * HoWo;
    const int k0 = blockIdx.y * KT, c0 = blockIdx.z * CT;

    float acc[KT][CT][FF];
    float accb[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
        accb[kk] = 0.f;
#pragma unroll
        for (int cc = 0; cc < CT; ++cc)
#pragma unroll
            for (int t = 0; t < FF; ++t) acc[kk][cc][t] = 0.f;
    }

    for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < M;
         m += (long long)gridDim.x * 256) {
        const int n = (int)(m / HoWo);
        const int p = (int)(m - (long long)n * HoWo);
        const int i = p / Wo, j = p - i * Wo;
        const int y0 = i * stride - pad, x0 = j * stride - pad;
        float dzv[KT];
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
            dzv[kk] = (k0 + kk < K) ? dz[((size_t)n * K + k0 + kk) * HoWo + p] : 0.f;
            accb[kk] += dzv[kk];
        }
#pragma unroll
        for (int cc = 0; cc < CT; ++cc) {
            if (c0 + cc < C) {
                const float* xc = x + ((size_t)n * C + c0 + cc) * H * Wd;
#pragma unroll
                for (int u = 0; u < F; ++u) {
                    const int yy = y0 + u;
                    const bool yok = (yy >= 0) && (yy < H);
#pragma unroll
                    for (int v = 0; v < F; ++v) {
                        const int xx = x0 + v;
                        float xv = 0.f;
                        if (yok && xx >= 0 && xx < Wd) xv = xc[yy * Wd + xx];
#pragma unroll
                        for (int kk = 0; kk < KT; ++kk)
                            acc[kk][cc][u * F + v] = fmaf(dzv[kk], xv, acc[kk][cc][u * F + v]);
                    }
                }
            }
        }
    }

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
#pragma unroll
        for (int cc = 0; cc < CT; ++cc)
#pragma unroll
            for (int t = 0; t < FF; ++t) {
                float s = wave_sum_f(acc[kk][cc][t]);
                if (lane == 0) red[wave][(kk * CT + cc) * FF + t] = s;
            }
        float sb = wave_sum_f(accb[kk]);
        if (lane == 0) red[wave][KT * CT * FF + kk] = sb;
    }
    __syncthreads();
    const int KCFF = K * C * FF;
    for (int t = threadIdx.x; t < KT * CT * FF + KT; t += 256) {
        const float s = red[0][t] + red[1][t] + red[2][t] + red[3][t];
        if (t < KT * CT * FF) {
            const int kk = t / (CT * FF), r = t - kk * CT * FF, cc = r / FF, uv = r - cc * FF;
            if (k0 + kk < K && c0 + cc < C)
                partial[(size_t)blockIdx.x * KCFF + ((size_t)(k0 + kk) * C + c0 + cc) * FF + uv] = s;
        } else if (blockIdx.z == 0) {
            const int kk = t - KT * CT * FF;
            if (k0 + kk < K) dbpartial[(size_t)blockIdx.x * K + k0 + kk] = s;
        }
    }
}

// generic fallback (any f): one block per (k, c, u, v), threads stride over pixels
__global__ __launch_bounds__(256) void conv_wgrad_generic(
    const float* __restrict__ x, const float* __restrict__ dz, float* __restrict__ dW,
    int N, int C, int H, int Wd, int K, int f, int stride, int pad, int Ho, int Wo) {
    __shared__ float red[4];
    const int ff = f * f;
    int t = blockIdx.x;
    const int uv = t % ff;
    t /= ff;
    const int c = t % C, k = t / C;
    const int u = uv / f, v = uv % f;
    const int HoWo = Ho * Wo;
    const long long M = (long long)N * HoWo;
    float acc = 0.f;
    for (long long m = threadIdx.x; m < M; m += 256) {
        const int n = (int)(m / HoWo);
        const int p = (int)(m - (long long)n * HoWo);
        const int i = p / Wo, j = p - i * Wo;
        const int yy = i * stride - pad + u, xx = j * stride - pad + v;
        if (yy >= 0 && yy < H && xx >= 0 && xx < Wd)
            acc = fmaf(dz[((size_t)n * K + k) * HoWo + p],
                       x[(((size_t)n * C + c) * H + yy) * Wd + xx], acc);
    }
    acc = wave_sum_f(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        dW[((size_t)k * C + c) * ff + (f - 1 - u) * f + (f - 1 - v)] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void conv_bgrad_generic(const float* __restrict__ dz,
                                                         float* __restrict__ db, int N, int K, int HoWo) {
    __shared__ float red[4];
    const int k = blockIdx.x;
    const long long M = (long long)N * HoWo;
    float acc = 0.f;
    for (long long m = threadIdx.x; m < M; m += 256) {
        const int n = (int)(m / HoWo);
        const int p = (int)(m - (long long)n * HoWo);
        acc += dz[((size_t)n * K + k) * HoWo + p];
    }
    acc = wave_sum_f(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) db[k] = red[0] + red[1] + red[2] + red[3];
}


// ------------------------------------------------------------------------------------
// dgrad: dx[n,c,y,x] = sum_{k,u,v} dz[n,k,(y+pad-u)/s,(x+pad-v)/s] * W[k,c,f-1-u,f-1-v]
// optional fused activation gradient of the layer below (its output prev_a has dx's shape)
// ------------------------------------------------------------------------------------
template <int F, int CT>
__global__ __launch_bounds__(256) void conv_dgrad_direct(
    const float* __restrict__ dz, const float* __restrict__ W, float* __restrict__ dx, int N, int C,
    int H, int Wd, int K, int f_rt, int stride, int pad, int Ho, int Wo,
    const float* __restrict__ prev_a, int prev_act, float prev_prm) {
    const int f = F ? F : f_rt;
    const int ff = f * f;
    const int HW = H * Wd, HoWo = Ho * Wo;
    const long long M = (long long)N * HW;
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c0 = blockIdx.y * CT;
    if (m >= M) return;
    const int n = (int)(m / HW);
    const int p = (int)(m - (long long)n * HW);
    const int y = p / Wd, xq = p - y * Wd;

    float acc[CT];
#pragma unroll
    for (int cc = 0; cc < CT; ++cc) acc[cc] = 0.f;

    if (F > 0 && stride == 1) {
        // stride-1 fast path: branch-free, fully unrolled taps (independent loads in flight)
        for (int k = 0; k < K; ++k) {
            const float* dzk = dz + ((size_t)n * K + k) * HoWo;
            const float* wk = W + ((size_t)k * C + c0) * ff;
#pragma unroll
            for (int u = 0; u < f; ++u) {
                const int i = y + pad - u;
                const bool iok = (unsigned)i < (unsigned)Ho;
                const int ic = min(max(i, 0), Ho - 1);
#pragma unroll
                for (int v = 0; v < f; ++v) {
                    const int j = xq + pad - v;
                    const bool ok = iok && ((unsigned)j < (unsigned)Wo);
                    const int jc = min(max(j, 0), Wo - 1);
                    const float t = dzk[ic * Wo + jc];
                    const float g = ok ? t : 0.f;
                    const int widx = (f - 1 - u) * f + (f - 1 - v);
#pragma unroll
                    for (int cc = 0; cc < CT; ++cc) {
                        const float wv = (c0 + cc < C) ? wk[(size_t)cc * ff + widx] : 0.f;
                        acc[cc] = fmaf(g, wv, acc[cc]);
                    }
                }
            }
        }
    } else {
        for (int k = 0; k < K; ++k) {
            const float* dzk = dz + ((size_t)n * K + k) * HoWo;
            const float* wk = W + ((size_t)k * C + c0) * ff;
            for (int u = 0; u < f; ++u) {
                const int ty = y + pad - u;
                if (ty < 0) continue;
                const int i = ty / stride;
                if (i * stride != ty || i >= Ho) continue;
                for (int v = 0; v < f; ++v) {
                    const int tx = xq + pad - v;
                    if (tx < 0) continue;
                    const int j = tx / stride;
                    if (j * stride != tx || j >= Wo) continue;
                    const float g = dzk[i * Wo + j];
                    const int widx = (f - 1 - u) * f + (f - 1 - v);
#pragma unroll
                    for (int cc = 0; cc < CT; ++cc) {
                        const float wv = (c0 + cc < C) ? wk[(size_t)cc * ff + widx] : 0.f;
                        acc[cc] = fmaf(g, wv, acc[cc]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int cc = 0; cc < CT; ++cc) {
        if (c0 + cc < C) {
            const size_t o = ((size_t)n * C + c0 + cc) * HW + p;
            float r = acc[cc];
            if (prev_a) r *= tn_act_grad_from_out(prev_a[o], prev_act, prev_prm);
            dx[o] = r;
        }
    }
}

// LDS-staged dgrad (stride 1).  A block stages dz of G whole images in LDS with a ZERO HALO of
// f-1 pixels around every map, plus the weights as one float4 (4 input channels) per (k, tap).
// Then thread = one input pixel: every tap is an unconditional LDS read (no bounds selects, so
// the reads pipeline), the weights are wave-broadcast b128 reads, 4 FMAs per tap.
//   dx[n,c,y,x] = sum_{k,u',v'} dzh[n,k,y+pad+u',x+pad+v'] * W[k,c,u',v']      (dzh = haloed dz)
template <int F>
__global__ __launch_bounds__(256) void conv_dgrad_lds(
    const float* __restrict__ dz, const float* __restrict__ W, float* __restrict__ dx, int N, int C,
    int H, int Wd, int K, int pad, int Ho, int Wo, int G, const float* __restrict__ prev_a,
    int prev_act, float prev_prm) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int FF = F * F;
    const int Hh = Ho + 2 * (F - 1), Wh = Wo + 2 * (F - 1);
    const int plane = Hh * Wh, HoWo = Ho * Wo, HW = H * Wd;
    float4* sW = reinterpret_cast<float4*>(sm);                  // [K][FF]
    float* sdz = sm + (size_t)K * FF * 4;                        // [G][K][Hh][Wh]
    const int n0 = blockIdx.x * G;
    const int gcnt = min(G, N - n0);
    const int c0 = blockIdx.y * 4;
    for (int t = threadIdx.x; t < K * FF; t += 256) {
        const int k = t / FF, uv = t - k * FF;
        float4 w;
        w.x = (c0 + 0 < C) ? W[((size_t)k * C + c0 + 0) * FF + uv] : 0.f;
        w.y = (c0 + 1 < C) ? W[((size_t)k * C + c0 + 1) * FF + uv] : 0.f;
        w.z = (c0 + 2 < C) ? W[((size_t)k * C + c0 + 2) * FF + uv] : 0.f;
        w.w = (c0 + 3 < C) ? W[((size_t)k * C + c0 + 3) * FF + uv] : 0.f;
        sW[t] = w;
    }
    const float* src = dz + (size_t)n0 * K * HoWo;
    for (int t = threadIdx.x; t < gcnt * K * plane; t += 256) {
        const int gk = t / plane, r = t - gk * plane;
        const int ii = r / Wh - (F - 1), jj = r % Wh - (F - 1);
        const bool in = ((unsigned)ii < (unsigned)Ho) && ((unsigned)jj < (unsigned)Wo);
        const float v = src[(size_t)gk * HoWo + min(max(ii, 0), Ho - 1) * Wo + min(max(jj, 0), Wo - 1)];
        sdz[t] = in ? v : 0.f;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < gcnt * HW; t += 256) {
        const int gi = t / HW;
        const int p = t - gi * HW;
        const int y = p / Wd, xq = p - y * Wd;
        const float* base = sdz + (size_t)gi * K * plane + (y + pad) * Wh + xq + pad;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < K; ++k) {
            const float* bk = base + k * plane;
            const float4* wk = sW + k * FF;
#pragma unroll
            for (int u = 0; u < F; ++u)
#pragma unroll
                for (int v = 0; v < F; ++v) {
                    const float gv = bk[u * Wh + v];
                    const float4 w = wk[u * F + v];
                    acc.x = fmaf(gv, w.x, acc.x);
                    acc.y = fmaf(gv, w.y, acc.y);
                    acc.z = fmaf(gv, w.z, acc.z);
                    acc.w = fmaf(gv, w.w, acc.w);
                }
        }
        const float r4[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            if (c0 + cc < C) {
                const size_t o = ((size_t)(n0 + gi) * C + c0 + cc) * HW + p;
                float r = r4[cc];
                if (prev_a) r *= tn_act_grad_from_out(prev_a[o], prev_act, prev_prm);
                dx[o] = r;
            }
        }
    }
}

// ------------------------------------------------------------------------------------

int tn_conv_wgrad_finish(tn_ctx* ctx, const float* partial, const float* dbpartial, float* dW,
                         float* db, int nblk, int K, int C, int f) {
    // slabs are in correlation layout: the sum flips every f x f block back (reduce.hip)
    return tn_red_wgrad(ctx, partial, dW, (uint32_t)(K * C * f * f), (uint32_t)nblk, (uint32_t)(K * C * f * f), dbpartial,
                        db, (uint32_t)K, (uint32_t)nblk, (uint32_t)K, (uint32_t)(f * f));
}

// ---- which kernel a product of tn_conv2d_* gets: the whole ladder, in the order it is asked (ConvRoute: common.h) ---------

// images per block of conv_dgrad_lds (0: the filters and one haloed dz image do not fit its 60 KiB of LDS)
static int dgrad_lds_group(int K, int Ho, int Wo, size_t* lds) {
    const size_t per = (size_t)K * (Ho + 4) * (Wo + 4) * sizeof(float);
    const size_t wbytes = (size_t)K * 9 * 16;
    if (per + wbytes > 60 * 1024) return 0;
    int G = (int)((60 * 1024 - wbytes) / per);
    if (G > 4) G = 4;
    *lds = wbytes + (size_t)G * per;
    return G;
}

// unal: the operands whose 16-byte alignment tn_conv_tile_*ok look at -- forward x, weight gradient x and dz, input
// gradient dz -- are not all aligned.  The geometry is the LAYER's in every product.
static ConvRoute conv_route(int conv_bf16, int num_cus, ConvProduct prod, unsigned unal, int N, int C, int H, int Wd,
                            int K, int f, int stride, int pad, int Ho, int Wo) {
    if (conv_bf16) return CONV_BF16;           // the mode, not the shape: asked before the entry points' shape checks,
    if (N <= 0 || C <= 0 || K <= 0 || f <= 0 || stride <= 0 || (prod == CONV_FWD && (Ho <= 0 || Wo <= 0)))
        return CONV_DIRECT;                    // which refuse these: nothing to ask the geometry functions
    size_t lds;
    switch (prod) {
        case CONV_FWD:
            if (tn_conv_mfma_supported(C, K, f, stride))
                return tn_conv_tile_ok(unal, N, C, H, Wd, K, f, pad, Ho, Wo) ? CONV_TILE : CONV_MFMA;
            // few input channels (first layers): still worth the matrix core when the LDS-tile kernel applies
            if (stride == 1 && K >= 16 && tn_conv_tile_ok(unal, N, C, H, Wd, K, f, pad, Ho, Wo)) return CONV_TILE;
            return CONV_DIRECT;
        case CONV_WGRAD:
            // (tn_conv_tile_wgrad_ok cuts its slabs for the context's CU count, the fused block's
            // tn_convpool_tile_supported for 256 CUs whatever the chip: possibly unintended, kept as it is)
            if (tn_conv_mfma_supported(C, K, f, stride))
                return tn_conv_tile_wgrad_ok(num_cus, unal, N, C, H, Wd, K, f, pad, Ho, Wo) ? CONV_TILE : CONV_MFMA;
            if (stride == 1 && tn_conv_tile_smallc_ok(unal, N, C, H, Wd, K, f, pad, Ho, Wo)) return CONV_TILE_SMALLC;
            return (f == 3 || f == 5 || f == 1 || f == 2) ? CONV_DIRECT : CONV_GENERIC;
        default:
            // dx = conv_fwd(dz, Wt) with padding f-1-pad: the roles swap -- reduction K*f*f, rows = C input maps,
            // gathered tensor = dz (N,K,Ho,Wo)
            if (tn_conv_mfma_supported(K, C, f, stride))
                return tn_conv_tile_ok(unal, N, K, Ho, Wo, C, f, f - 1 - pad, H, Wd) ? CONV_TILE : CONV_MFMA;
            if (f == 3 && stride == 1 && dgrad_lds_group(K, Ho, Wo, &lds)) return CONV_LDS_DGRAD;
            return CONV_DIRECT;
    }
}

// What the kernels of this file launch for a product that conv_route sent here (CONV_DIRECT, CONV_LDS_DGRAD,
// CONV_GENERIC): template arguments and grid.  v[] per kernel: include/theanet_hip.h (tn_conv_plan).
static ConvPlan conv_direct_plan(ConvRoute route, ConvProduct prod, unsigned al, int N, int C, int H, int Wd, int K, int f,
                                 int Ho, int Wo) {
    ConvPlan p{};
    p.route = route;
    const int prev = prod == CONV_DGRAD && !(al & CONV_BARE);
    if (route == CONV_GENERIC) {
        p.kernel = CVK_WGRAD_GENERIC;
        p.v[0] = K * C * f * f;
    } else if (route == CONV_LDS_DGRAD) {
        size_t lds = 0;
        const int G = dgrad_lds_group(K, Ho, Wo, &lds);
        p.kernel = CVK_DGRAD_LDS;
        p.t[0] = 3;
        p.v[0] = G; p.v[1] = cdiv(N, G); p.v[2] = cdiv(C, 4); p.v[3] = (int)lds; p.v[4] = prev;
    } else if (prod == CONV_FWD) {
        p.kernel = CVK_FWD_DIRECT;
        p.t[0] = (f == 3 || f == 5) ? f : 0;
        p.t[1] = ((K % 8 == 0) || K > 32) ? 8 : 4;
        p.v[0] = cdiv((long long)N * Ho * Wo, 256); p.v[1] = cdiv(K, p.t[1]);
    } else if (prod == CONV_WGRAD) {
        p.kernel = CVK_WGRAD_DIRECT;
        p.t[0] = f;
        if (f == 3) { p.t[1] = 4; p.t[2] = C >= 4 ? 4 : C >= 2 ? 2 : 1; }
        else if (f == 5) { p.t[1] = C >= 2 ? 2 : 4; p.t[2] = C >= 2 ? 2 : 1; }
        else if (f == 2) { p.t[1] = 4; p.t[2] = C >= 4 ? 4 : 1; }
        else { p.t[0] = 1; p.t[1] = 8; p.t[2] = C >= 4 ? 4 : 1; }
        int nblk = cdiv((long long)N * Ho * Wo, 256 * 16);
        if (nblk > 1024) nblk = 1024;
        if (nblk < 1) nblk = 1;
        p.v[0] = nblk; p.v[1] = cdiv(K, p.t[1]); p.v[2] = cdiv(C, p.t[2]);
    } else {
        p.kernel = CVK_DGRAD_DIRECT;
        p.t[0] = f == 3 ? 3 : 0;
        p.t[1] = C >= 8 ? 8 : 4;
        p.v[0] = cdiv((long long)N * H * Wd, 256); p.v[1] = cdiv(C, p.t[1]); p.v[2] = prev;
    }
    return p;
}

extern "C" {

// What a tn_conv2d_* call of this shape launches in CONV mode 0: conv_route, then the plan function of the route's
// launcher -- the functions the entry points below and their launchers run.  Layout and flags: include/theanet_hip.h.
int tn_conv_plan(int prod_, int N, int C, int H, int Wd, int K, int f, int stride, int pad_lo, int Ho, int Wo, int num_cus,
                 unsigned flags, int* out, int nout) {
    if (prod_ < 0 || prod_ > 2 || num_cus < 0 || (nout > 0 && !out)) return TN_E_ARG;
    if (N <= 0 || C <= 0 || K <= 0 || f <= 0 || stride <= 0 || (prod_ == CONV_FWD && (Ho <= 0 || Wo <= 0))) return TN_E_ARG;
    if (H <= 0 || Wd <= 0 || Ho <= 0 || Wo <= 0) return TN_E_ARG;     // (nothing to launch: the entry points do not ask)
    if (num_cus == 0) num_cus = tn_current_cus();
    const ConvProduct prod = (ConvProduct)prod_;
    const unsigned unal = flags & CONV_UNAL_GATHER;
    const ConvRoute route = conv_route(0, num_cus, prod, unal, N, C, H, Wd, K, f, stride, pad_lo, Ho, Wo);
    ConvPlan p{};
    int ok = 1;
    switch (route) {
        case CONV_TILE:
            ok = prod == CONV_WGRAD ? tn_conv_tile_wgrad_plan(num_cus, N, C, H, Wd, K, &p)
                                    : tn_conv_tile_plan(prod, flags, N, C, H, Wd, K, pad_lo, Ho, Wo, &p);
            break;
        case CONV_TILE_SMALLC: ok = tn_conv_tile_smallc_plan(num_cus, N, C, H, Wd, K, &p); break;
        case CONV_MFMA: ok = tn_conv_mfma_plan(prod, num_cus, flags, N, C, H, Wd, K, f, pad_lo, Ho, Wo, &p); break;
        default: p = conv_direct_plan(route, prod, flags, N, C, H, Wd, K, f, Ho, Wo); break;
    }
    if (!ok) return TN_E_ARG;
    const int* v = &p.route;
    static_assert(sizeof(ConvPlan) == CONV_PLAN_INTS * sizeof(int), "ConvPlan is CONV_PLAN_INTS ints");
    for (int k = 0; k < CONV_PLAN_INTS && k < nout; ++k) out[k] = v[k];
    return CONV_PLAN_INTS;
}

int tn_conv2d_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int N,
                  int C, int H, int Wd, int K, int f, int stride, int pad_lo, int Ho, int Wo,
                  int act, float act_param) {
    const ConvRoute route = conv_route(ctx->conv_bf16, ctx->num_cus, CONV_FWD, conv_unal(x), N, C, H, Wd, K, f, stride, pad_lo, Ho, Wo);
    if (route == CONV_BF16) return tn_cb_conv_fwd(ctx, x, W, b, a, N, C, H, Wd, K, f, stride, pad_lo, Ho, Wo, act, act_param);
    TN_REQUIRE(N > 0 && C > 0 && K > 0 && f > 0 && stride > 0 && Ho > 0 && Wo > 0, "tn_conv2d_fwd: bad shape");
    TN_FP32_ONLY(ctx, "tn_conv2d_fwd");
    switch (route) {
        case CONV_TILE: return tn_conv_tile_fwd(ctx, x, W, b, a, N, C, H, Wd, K, pad_lo, Ho, Wo, act, act_param);
        case CONV_MFMA: return tn_conv_mfma_fwd(ctx, x, W, b, a, N, C, H, Wd, K, f, pad_lo, Ho, Wo, act, act_param);
        default: break;      // CONV_DIRECT
    }
    const ConvPlan p = conv_direct_plan(route, CONV_FWD, 0, N, C, H, Wd, K, f, Ho, Wo);
#define LAUNCH_FWD(F_, KT_)                                                                     \
    case F_ * 16 + KT_:                                                                         \
        conv_fwd_direct<F_, KT_><<<dim3(p.v[0], p.v[1]), 256, 0, ctx->stream>>>(                 \
            x, W, b, a, N, C, H, Wd, K, f, stride, pad_lo, Ho, Wo, act, act_param);             \
        break
    switch (p.t[0] * 16 + p.t[1]) {
        LAUNCH_FWD(3, 8); LAUNCH_FWD(3, 4); LAUNCH_FWD(5, 8); LAUNCH_FWD(5, 4); LAUNCH_FWD(0, 8); LAUNCH_FWD(0, 4);
        default: return tn_fail(ctx, TN_E_ARG, "tn_conv2d_fwd: no conv_fwd_direct<%d,%d>", p.t[0], p.t[1]);
    }
#undef LAUNCH_FWD
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_conv2d_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int N, int C,
                    int H, int Wd, int K, int f, int stride, int pad_lo, int Ho, int Wo) {
    const ConvRoute route = conv_route(ctx->conv_bf16, ctx->num_cus, CONV_WGRAD, conv_unal(x, dz), N, C, H, Wd, K, f, stride, pad_lo, Ho, Wo);
    if (route == CONV_BF16) return tn_cb_conv_wgrad(ctx, x, dz, dW, db, N, C, H, Wd, K, f, stride, pad_lo, Ho, Wo);
    TN_REQUIRE(N > 0 && C > 0 && K > 0 && f > 0 && stride > 0, "tn_conv2d_wgrad: bad shape");
    TN_FP32_ONLY(ctx, "tn_conv2d_wgrad");
    switch (route) {
        case CONV_TILE: return tn_conv_tile_wgrad(ctx, x, dz, dW, db, N, C, H, Wd, K);
        case CONV_MFMA: return tn_conv_mfma_wgrad(ctx, x, dz, dW, db, N, C, H, Wd, K, f, pad_lo, Ho, Wo);
        case CONV_TILE_SMALLC: return tn_conv_tile_smallc_wgrad(ctx, x, dz, dW, db, N, C, H, Wd, K);
        default: break;      // CONV_GENERIC, CONV_DIRECT
    }
    const ConvPlan p = conv_direct_plan(route, CONV_WGRAD, 0, N, C, H, Wd, K, f, Ho, Wo);
    if (p.kernel == CVK_WGRAD_GENERIC) {
        conv_wgrad_generic<<<p.v[0], 256, 0, ctx->stream>>>(x, dz, dW, N, C, H, Wd, K, f, stride, pad_lo, Ho, Wo);
        TN_LAUNCH_CHECK();
        conv_bgrad_generic<<<K, 256, 0, ctx->stream>>>(dz, db, N, K, Ho * Wo);
        TN_LAUNCH_CHECK();
        return TN_OK;
    }
    const int nblk = p.v[0];
    float *partial, *dbpartial;
    int rc = conv_slabs(ctx, nblk, (size_t)K * C * f * f, K, &partial, &dbpartial);
    if (rc) return rc;
#define LAUNCH_WG(F_, KT_, CT_)                                                                  \
    case F_ * 256 + KT_ * 16 + CT_:                                                              \
        conv_wgrad_direct<F_, KT_, CT_><<<dim3(nblk, p.v[1], p.v[2]), 256, 0, ctx->stream>>>(     \
            x, dz, partial, dbpartial, N, C, H, Wd, K, stride, pad_lo, Ho, Wo);                  \
        break
    switch (p.t[0] * 256 + p.t[1] * 16 + p.t[2]) {
        LAUNCH_WG(3, 4, 4); LAUNCH_WG(3, 4, 2); LAUNCH_WG(3, 4, 1);
        LAUNCH_WG(5, 2, 2); LAUNCH_WG(5, 4, 1);
        LAUNCH_WG(2, 4, 4); LAUNCH_WG(2, 4, 1);
        LAUNCH_WG(1, 8, 4); LAUNCH_WG(1, 8, 1);
        default: return tn_fail(ctx, TN_E_ARG, "tn_conv2d_wgrad: no conv_wgrad_direct<%d,%d,%d>", p.t[0], p.t[1], p.t[2]);
    }
#undef LAUNCH_WG
    TN_LAUNCH_CHECK();
    return tn_conv_wgrad_finish(ctx, partial, dbpartial, dW, db, nblk, K, C, f);
}

int tn_conv2d_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int N, int C, int H,
                    int Wd, int K, int f, int stride, int pad_lo, int Ho, int Wo, const float* prev_a,
                    int prev_act, float prev_act_param) {
    const ConvRoute route = conv_route(ctx->conv_bf16, ctx->num_cus, CONV_DGRAD, conv_unal(dz), N, C, H, Wd, K, f, stride, pad_lo, Ho, Wo);
    if (route == CONV_BF16)
        return tn_cb_conv_dgrad(ctx, dz, W, dx, N, C, H, Wd, K, f, stride, pad_lo, Ho, Wo, prev_a, prev_act, prev_act_param);
    TN_REQUIRE(N > 0 && C > 0 && K > 0 && f > 0 && stride > 0, "tn_conv2d_dgrad: bad shape");
    TN_FP32_ONLY(ctx, "tn_conv2d_dgrad");
    switch (route) {
        case CONV_TILE: return tn_conv_tile_dgrad(ctx, dz, W, dx, N, C, H, Wd, K, pad_lo, Ho, Wo, prev_a, prev_act, prev_act_param);
        case CONV_MFMA: return tn_conv_mfma_dgrad(ctx, dz, W, dx, N, C, H, Wd, K, f, pad_lo, Ho, Wo, prev_a, prev_act, prev_act_param);
        default: break;      // CONV_LDS_DGRAD, CONV_DIRECT
    }
    const ConvPlan p = conv_direct_plan(route, CONV_DGRAD, 0, N, C, H, Wd, K, f, Ho, Wo);
    if (p.kernel == CVK_DGRAD_LDS) {
        conv_dgrad_lds<3><<<dim3(p.v[1], p.v[2]), 256, (size_t)p.v[3], ctx->stream>>>(
            dz, W, dx, N, C, H, Wd, K, pad_lo, Ho, Wo, p.v[0], prev_a, prev_act, prev_act_param);
        TN_LAUNCH_CHECK();
        return TN_OK;
    }
#define LAUNCH_DG(F_, CT_)                                                                       \
    case F_ * 16 + CT_:                                                                          \
        conv_dgrad_direct<F_, CT_><<<dim3(p.v[0], p.v[1]), 256, 0, ctx->stream>>>(                \
            dz, W, dx, N, C, H, Wd, K, f, stride, pad_lo, Ho, Wo, prev_a, prev_act, prev_act_param); \
        break
    switch (p.t[0] * 16 + p.t[1]) {
        LAUNCH_DG(3, 8); LAUNCH_DG(3, 4); LAUNCH_DG(0, 8); LAUNCH_DG(0, 4);
        default: return tn_fail(ctx, TN_E_ARG, "tn_conv2d_dgrad: no conv_dgrad_direct<%d,%d>", p.t[0], p.t[1]);
    }
#undef LAUNCH_DG
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
