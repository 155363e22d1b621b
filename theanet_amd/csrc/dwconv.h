// Depthwise convolution (ConvLayer(..., depthwise=True): every map convolved with its own f x f filter, nothing summed
// across maps; W (C, 1, f, f) in tn_conv2d_*'s orientation, b (C)) -- the kernels both tensor types share.  dwconv.hip
// runs them on the scalar planes of fp32 NCHW tensors, dwconv_c8.hip on the 16-byte cells of the 16-bit conv stack (8
// channels of a pixel: a depthwise product never leaves the cell).  There is no matrix product here: the ops are bound
// by memory, the kernels are an LDS halo tile and a register sliding window.
//
// A tensor is a run of PLANES (fp32: one per (image, channel); c8: one per (image, channel octet)) of `cell`s; T says
// what a cell is: T::L channels, T::load to fp32, T::pack from fp32 (the one rounding of a 16-bit store), T::wround
// (the weight as the arithmetic uses it: rounded to the element type on the stack, itself in fp32).
//
// dw_kernel<T, F, MODE> -- MODE 0 forward, 1 input gradient -- one 256-lane block per tile of the STORED output plane
// (rows x pitch: pad cells of a c8 plane included, they are written as +0):
//   tile     TW columns (a power of two <= 32) x SPP strips of DW_R rows x TP planes, lane = (plane, strip, column):
//            consecutive lanes store consecutive cells.  A plane smaller than the block is taken whole and the block
//            takes TP of them (dw_tile: 8 x 8 maps -> 8 planes a block).
//   staging  the source rows and columns the tile's windows read, f - 1 halo included, as cells [plane][IH][IWp] in LDS
//            (row stride IWp odd: lanes of a wave that sit in different strips start in different banks); cells outside
//            the map are staged as zeros, so the inner loops have no bounds tests.  The planes' f f L weights (rounded
//            once, flipped for the forward) and biases sit beside them as fp32: block-uniform broadcast reads, no VGPRs.
//   stride 1 (both modes: the input gradient of a stride-1 layer is the forward with the filter unflipped and the
//            padding f - 1 - pad): per filter COLUMN v the lane holds the column's f weights in registers and slides
//            down its strip: DW_R + f - 1 cells read once each, every one feeding the (up to f) outputs whose window
//            holds it -- f (DW_R + f - 1) LDS reads for DW_R outputs instead of f f DW_R.  DW_R x L fp32 accumulators.
//   stride s the forward walks the same strip with the tap row found at run time (weights from LDS); the input gradient
//            is a GATHER: output (y, x) sums dz[i, j] W[f-1-u, f-1-v] over the windows i = ceil((y + pad - f + 1) / s)
//            .. floor((y + pad) / s) that cover it (u = y + pad - i s), columns likewise, in row-major window order --
//            at most ceil(f / s)^2 terms, none for a pixel no window touches (+0).  No atomics.
//   epilogue forward: act(sum + b); input gradient: sum * act'(prev_a) (NULL: none); T::pack, one store per cell.  Pad
//            cells and channels past C are stored as +0.
// dw_wgrad_kernel<T, F, TR>: dW[c, f-1-u, f-1-v] = sum over (n, i, j) of dz[n, c, i, j] xpad[n, c, i s + u, j s + v],
//   db[c] = sum dz.  A block owns (channel group, slab); the output pixels of the whole batch are cut into tiles of 256,
//   slab k takes tiles k, k + nslab, ...  (nslab from the geometry alone: dw_slabs).  A lane keeps TR f x L partials (TR
//   tap rows a pass: 3 x 3 in one pass, 5 x 5 row by row -- 40 accumulators instead of 200), reads its dz cell once a
//   pass and the x cells of the taps through the vector cache; the wave adds up by cross-lane moves, the four waves'
//   sums are added in wave order and the block writes ONE partial per slab (scale removed) in dW's layout into context
//   scratch; the context's reduction (tn_red_wgrad) finishes dW and db in slab order: the same bits every run.
#pragma once
#include "common.h"

#define DW_R 4                 // output rows of a lane's strip
#define DW_LDS_MAX (48 << 10)  // a block's tile (three blocks a CU)
#define DW_STRIDE_MAX 16

struct DwGeom {
    const void* src;           // x (forward), dz (input gradient)
    void* out;                 // y / dx
    const float* W;
    const float* bias;         // forward
    const void* prev_a;        // input gradient: output of the layer below (NULL: none)
    unsigned planes, CP;       // N CP planes, CP channel groups an image
    int C;
    int Hs, Ws, Ps;            // source maps: rows, columns, row pitch
    unsigned PPs;              // cells of a source plane
    int Ho, Wo;                // output maps
    int OH, OW;                // ... as stored: rows, row pitch (c8: the pitch both ways)
    unsigned PPo;
    int stride, pad;           // stride 1: the padding of THIS product (input gradient: f - 1 - pad_lo); else the layer's
    int TW, lgTW, SPP, lgSPP, TP, IH, IW, IWp;      // dw_tile
    int act;
    float prm;
};

struct DwTile {
    int TW, lgTW, SPP, lgSPP, TP, IH, IW, IWp;
    size_t wbytes, lds;
    dim3 grid;
};

static inline int dw_lg(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// The tile of a product whose stored output planes have OH rows at pitch OW.  gather: the strided input gradient.
static inline DwTile dw_tile(int F, int L, size_t cell_bytes, long long planes, int OH, int OW, int stride, bool gather) {
    DwTile d;
    d.lgTW = dw_lg(OW < 32 ? OW : 32);
    const int ns = (OH + DW_R - 1) / DW_R;
    d.lgSPP = dw_lg(ns);
    if (d.lgSPP > 8 - d.lgTW) d.lgSPP = 8 - d.lgTW;
    int lgTP = 8 - d.lgTW - d.lgSPP;
    while (lgTP > 0 && (1ll << (lgTP - 1)) >= planes) --lgTP;
    for (;;) {
        d.TW = 1 << d.lgTW; d.SPP = 1 << d.lgSPP; d.TP = 1 << lgTP;
        const int TH = d.SPP * DW_R;
        d.IH = gather ? (TH + F - 2) / stride + 1 : (TH - 1) * stride + F;
        d.IW = gather ? (d.TW + F - 2) / stride + 1 : (d.TW - 1) * stride + F;
        d.IWp = d.IW | 1;
        d.wbytes = ((size_t)d.TP * (F * F + 1) * L * sizeof(float) + 15) & ~(size_t)15;
        d.lds = d.wbytes + (size_t)d.TP * d.IH * d.IWp * cell_bytes;
        if (d.lds <= DW_LDS_MAX) break;
        if (lgTP > 0) --lgTP;                    // fewer lanes at work, never a larger tile
        else if (d.lgSPP > 0) --d.lgSPP;
        else --d.lgTW;                           // (stride <= DW_STRIDE_MAX: a one-lane tile fits)
    }
    d.grid = dim3((unsigned)((planes + d.TP - 1) / d.TP), (unsigned)((OH + d.SPP * DW_R - 1) / (d.SPP * DW_R)),
                  (unsigned)((OW + d.TW - 1) / d.TW));
    return d;
}

__device__ __forceinline__ int dw_ceil_div(int a, int s) { return a >= 0 ? (a + s - 1) / s : -((-a) / s); }

template <typename T, int F, int MODE>
__global__ __launch_bounds__(256) void dw_kernel(DwGeom g) {
    typedef typename T::cell cell;
    constexpr int L = T::L, FF = F * F, WL = (FF + 1) * L;
    extern __shared__ __attribute__((aligned(16))) char dw_smem[];
    float* const wl = reinterpret_cast<float*>(dw_smem);                 // [TP][FF taps, then the bias][L]
    cell* const tile = reinterpret_cast<cell*>(dw_smem + (((size_t)g.TP * WL * sizeof(float) + 15) & ~(size_t)15));
    const cell* const src = static_cast<const cell*>(g.src);
    const int t = threadIdx.x, s = g.stride;
    const bool gather = MODE == 1 && s > 1;
    const int y0 = blockIdx.y * (g.SPP * DW_R), x0 = blockIdx.z * g.TW;   // the tile's first output row / column
    // source coordinate of the staged tile's first row / column
    const int sy0 = gather ? dw_ceil_div(y0 + g.pad - (F - 1), s) : y0 * s - g.pad;
    const int sx0 = gather ? dw_ceil_div(x0 + g.pad - (F - 1), s) : x0 * s - g.pad;
    const unsigned plane0 = blockIdx.x * (unsigned)g.TP;

    for (int i = t; i < g.TP * WL; i += 256) {
        const int pl = i / WL, r = i - pl * WL, tap = r / L, e = r - tap * L;
        const unsigned plane = plane0 + pl;
        const int c = (int)(plane % g.CP) * L + e;
        float w = 0.f;
        if (plane < g.planes && c < g.C) {
            if (tap < FF) w = T::wround(g.W[(size_t)c * FF + (MODE == 0 ? FF - 1 - tap : tap)]);
            else if (MODE == 0) w = g.bias[c];
        }
        wl[i] = w;
    }
    const int per = g.IH * g.IW;
    for (int i = t; i < g.TP * per; i += 256) {
        const int pl = i / per, rem = i - pl * per, r = rem / g.IW, c = rem - r * g.IW;
        const int gy = sy0 + r, gx = sx0 + c;
        const unsigned plane = plane0 + pl;
        cell v = T::zero();
        if (plane < g.planes && gy >= 0 && gy < g.Hs && gx >= 0 && gx < g.Ws)
            v = src[(size_t)plane * g.PPs + (unsigned)gy * g.Ps + (unsigned)gx];
        tile[(pl * g.IH + r) * g.IWp + c] = v;
    }
    __syncthreads();

    const int col = t & (g.TW - 1), q = t >> g.lgTW, strip = q & (g.SPP - 1), pl = q >> g.lgSPP;
    const unsigned plane = plane0 + pl;
    const int oy = y0 + strip * DW_R, ox = x0 + col;
    if (pl >= g.TP || plane >= g.planes || oy >= g.OH || ox >= g.OW) return;
    const cell* const tl = tile + pl * g.IH * g.IWp;
    const float* const wp = wl + pl * WL;
    float acc[DW_R][L];
#pragma unroll
    for (int o = 0; o < DW_R; ++o)
#pragma unroll
        for (int e = 0; e < L; ++e) acc[o][e] = 0.f;

    if (oy < g.Ho && ox < g.Wo) {
        if (s == 1) {
            const cell* const b = tl + strip * DW_R * g.IWp + col;
#pragma unroll
            for (int v = 0; v < F; ++v) {
                float w[F][L];
#pragma unroll
                for (int u = 0; u < F; ++u)
#pragma unroll
                    for (int e = 0; e < L; ++e) w[u][e] = wp[(u * F + v) * L + e];
#pragma unroll
                for (int r = 0; r < DW_R + F - 1; ++r) {
                    float x[L];
                    T::load(b[r * g.IWp + v], x);
#pragma unroll
                    for (int o = 0; o < DW_R; ++o) {
                        const int u = r - o;
                        if (u >= 0 && u < F) {
#pragma unroll
                            for (int e = 0; e < L; ++e) acc[o][e] = fmaf(x[e], w[u][e], acc[o][e]);
                        }
                    }
                }
            }
        } else if (MODE == 0) {
            const cell* const b = tl + strip * DW_R * s * g.IWp + col * s;
            const int nr = (DW_R - 1) * s + F;
#pragma unroll
            for (int v = 0; v < F; ++v)
                for (int r = 0; r < nr; ++r) {
                    float x[L];
                    T::load(b[r * g.IWp + v], x);
#pragma unroll
                    for (int o = 0; o < DW_R; ++o) {
                        const int u = r - o * s;
                        if (u >= 0 && u < F) {
                            const float* const w = wp + (u * F + v) * L;
#pragma unroll
                            for (int e = 0; e < L; ++e) acc[o][e] = fmaf(x[e], w[e], acc[o][e]);
                        }
                    }
                }
        } else {
            const int jlo = dw_ceil_div(ox + g.pad - (F - 1), s), jhi = (ox + g.pad) / s;
#pragma unroll
            for (int o = 0; o < DW_R; ++o) {
                const int y = oy + o;
                const int ilo = dw_ceil_div(y + g.pad - (F - 1), s), ihi = (y + g.pad) / s;
                for (int i = ilo; i <= ihi; ++i)
                    for (int j = jlo; j <= jhi; ++j) {
                        const int up = F - 1 - (y + g.pad - i * s), vp = F - 1 - (ox + g.pad - j * s);
                        float x[L];
                        T::load(tl[(i - sy0) * g.IWp + (j - sx0)], x);
                        const float* const w = wp + (up * F + vp) * L;
#pragma unroll
                        for (int e = 0; e < L; ++e) acc[o][e] = fmaf(x[e], w[e], acc[o][e]);
                    }
            }
        }
    }

    const int nv = g.C - (int)(plane % g.CP) * L;          // channels of this plane inside C
    const bool lk = g.act == TN_ACT_LEAKY;
    const float prm = g.prm, tie = prm > 0.f ? 1.f + prm : 0.f;
    cell* const out = static_cast<cell*>(g.out) + (size_t)plane * g.PPo;
    const cell* const pa = MODE == 1 && g.prev_a ? static_cast<const cell*>(g.prev_a) + (size_t)plane * g.PPo : nullptr;
#pragma unroll
    for (int o = 0; o < DW_R; ++o) {
        const int y = oy + o;
        if (y >= g.OH) break;
        const bool in = y < g.Ho && ox < g.Wo;
        const unsigned at = (unsigned)y * g.OW + (unsigned)ox;
        float a[L], v[L];
        if (MODE == 1 && pa && in) T::load(pa[at], a);
#pragma unroll
        for (int e = 0; e < L; ++e) {
            float z = acc[o][e];
            if (MODE == 0) {
                z += wp[FF * L + e];
                z = lk ? fmaxf(0.f, z) + fminf(0.f, z) * prm : tn_act_fwd(z, g.act, prm);
            } else if (pa && in) {
                z *= lk ? (a[e] > 0.f ? 1.f : (a[e] < 0.f ? prm : tie)) : tn_act_grad_from_out(a[e], g.act, prm);
            }
            v[e] = (in && e < nv) ? z : 0.f;
        }
        out[at] = T::pack(v);
    }
}

struct DwWGeom {
    const void* x;
    const void* dz;
    float* ws;                 // [slab][C][f][f] partial dW (scale removed)
    float* dbws;               // [slab][C]
    unsigned CP;
    int C, Hs, Ws, Ps;
    unsigned PPs;
    int Ho, Wo, OW;            // dz maps and their row pitch
    unsigned PPo, HoWo;
    int stride, pad;
    unsigned long long npix;   // N Ho Wo
    unsigned ntiles, nslab;
    float oscale;
};

// Slabs of the weight gradient: 1024 blocks over all channel groups (four a CU of a 256-CU device, but a constant: the
// order of additions is the geometry's alone), at most one per tile of 256 output pixels.
static inline void dw_slabs(long long npix, int CP, unsigned* ntiles, unsigned* nslab) {
    const long long nt = (npix + 255) / 256, want = (1024 + CP - 1) / CP;
    *ntiles = (unsigned)nt;
    *nslab = (unsigned)(want < nt ? want : nt);
}

// grid (slabs, channel groups)
template <typename T, int F, int TR>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(DwWGeom g) {
    typedef typename T::cell cell;
    constexpr int L = T::L, FF = F * F, NA = TR * F;
    __shared__ float red[4][NA + 1][L];
    const cell* const xs = static_cast<const cell*>(g.x);
    const cell* const ds = static_cast<const cell*>(g.dz);
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, slab = blockIdx.x, grp = blockIdx.y;
    const int s = g.stride;
    for (int u0 = 0; u0 < F; u0 += TR) {
        float acc[NA + 1][L];                   // the pass's taps, then db (first pass)
#pragma unroll
        for (int k = 0; k <= NA; ++k)
#pragma unroll
            for (int e = 0; e < L; ++e) acc[k][e] = 0.f;
        for (unsigned tile_ = slab; tile_ < g.ntiles; tile_ += g.nslab) {
            const unsigned long long gi = (unsigned long long)tile_ * 256 + t;
            if (gi >= g.npix) continue;
            const unsigned n = (unsigned)(gi / g.HoWo), qq = (unsigned)(gi - (unsigned long long)n * g.HoWo);
            const int oh = (int)(qq / (unsigned)g.Wo), ow = (int)qq - oh * g.Wo;
            const size_t plane = (size_t)n * g.CP + grp;
            float d[L];
            T::load(ds[plane * g.PPo + (unsigned)oh * g.OW + (unsigned)ow], d);
            if (u0 == 0) {
#pragma unroll
                for (int e = 0; e < L; ++e) acc[NA][e] += d[e];
            }
            const cell* const xp = xs + plane * g.PPs;
#pragma unroll
            for (int ur = 0; ur < TR; ++ur) {
                const int sy = oh * s + u0 + ur - g.pad;
#pragma unroll
                for (int v = 0; v < F; ++v) {
                    const int sx = ow * s + v - g.pad;
                    if (sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws) {
                        float x[L];
                        T::load(xp[(unsigned)sy * g.Ps + (unsigned)sx], x);
#pragma unroll
                        for (int e = 0; e < L; ++e) acc[ur * F + v][e] = fmaf(d[e], x[e], acc[ur * F + v][e]);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k <= NA; ++k)
#pragma unroll
            for (int e = 0; e < L; ++e) {
                float v = acc[k][e];
#pragma unroll
                for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
                if (lane == 0) red[wave][k][e] = v;
            }
        __syncthreads();
        if (t < (NA + 1) * L) {
            const int k = t / L, e = t - k * L, c = (int)grp * L + e;
            const float v = (((red[0][k][e] + red[1][k][e]) + red[2][k][e]) + red[3][k][e]) * g.oscale;
            if (c < g.C) {
                // tap (u, v) of the correlation is W's (f-1-u, f-1-v)
                if (k < NA) g.ws[((size_t)slab * g.C + c) * FF + (FF - 1 - (u0 * F + k))] = v;
                else if (u0 == 0) g.dbws[(size_t)slab * g.C + c] = v;
            }
        }
        __syncthreads();
    }
}

// consistent geometry along one axis: So windows fit and no more, no more padding than a 'same' layer's
static inline bool dw_axis_ok(int S, int f, int stride, int pad, int So) {
    if (S < 1 || So < 1) return false;
    const long long hi = (long long)(So - 1) * stride + f - pad - S;
    return pad >= 0 && pad <= f / 2 && hi <= pad && hi > -(long long)stride;
}

// The launches of the three ops on tensors described by (planes, CP, C; source rows / columns / pitch / plane cells;
// output rows / columns, stored rows / pitch / plane cells).  g arrives with the tensors and the geometry filled in.
template <typename T, int F>
static int dw_launch(tn_ctx* ctx, DwGeom& g, int mode) {
    const bool gather = mode == 1 && g.stride > 1;
    const DwTile d = dw_tile(F, T::L, sizeof(typename T::cell), g.planes, g.OH, g.OW, g.stride, gather);
    g.TW = d.TW; g.lgTW = d.lgTW; g.SPP = d.SPP; g.lgSPP = d.lgSPP; g.TP = d.TP; g.IH = d.IH; g.IW = d.IW; g.IWp = d.IWp;
    if (mode == 0) dw_kernel<T, F, 0><<<d.grid, 256, d.lds, ctx->stream>>>(g);
    else dw_kernel<T, F, 1><<<d.grid, 256, d.lds, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

template <typename T>
static int dw_run(tn_ctx* ctx, DwGeom& g, int f, int mode) {
    return f == 3 ? dw_launch<T, 3>(ctx, g, mode) : dw_launch<T, 5>(ctx, g, mode);
}

template <typename T>
static int dw_run_wgrad(tn_ctx* ctx, DwWGeom& g, int f, int N, float* dW, float* db) {
    g.HoWo = (unsigned)g.Ho * g.Wo;
    g.npix = (unsigned long long)N * g.HoWo;
    dw_slabs((long long)g.npix, (int)g.CP, &g.ntiles, &g.nslab);
    const size_t n = (size_t)g.C * f * f;
    int rc = tn_scratch_get(ctx, (size_t)g.nslab * (n + g.C) * sizeof(float), &g.ws);
    if (rc) return rc;
    g.dbws = g.ws + (size_t)g.nslab * n;
    const dim3 grid(g.nslab, g.CP);
    if (f == 3) dw_wgrad_kernel<T, 3, 3><<<grid, 256, 0, ctx->stream>>>(g);
    else dw_wgrad_kernel<T, 5, 1><<<grid, 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return tn_red_wgrad(ctx, g.ws, dW, (uint32_t)n, g.nslab, (uint32_t)n, g.dbws, db, (uint32_t)g.C, g.nslab, (uint32_t)g.C);
}
