// ConvLayer(..., dilation=d) on fp32 NCHW tensors: tn_dilconv_fwd / _dgrad / _wgrad.  The arguments are tn_conv2d_*'s with d
// behind K; W (K, C, f, f), b (K).  Products and accumulation in fp32, under every CONV mode: CONV 'bfloat16' rounds the
// operands of the dense family's matrix product, a dilated layer stays on these kernels unchanged.  Like tn_conv2d_* they
// refuse to run while a 16-bit DTYPE is in force (its entry points are tn_c8_dilconv_*).  dilconv.h has the polyphase split.
//
// Forward / input gradient, K >= 16 and C >= 4 (dcf_mfma_kernel): dilconv_c8.hip's design on scalar planes and
// v_mfma_f32_16x16x4_f32 -- grid (images x tiles of a phase plane, phases, groups of row tiles); the 16 rows are 16 outputs,
// the 16 columns 16 pixels of the phase's tile, the 4-deep reduction FOUR items rc = tap * RCH + map of the chunk, one a
// quarter wave.  The phase's source tile ([map][IH][IWp] floats, odd pitch) is staged by row spans: the lanes of a block
// walk the CONTIGUOUS source row span the tile's columns lie in (coalesced 4-byte loads) and each keeps the element it
// loaded if it lies on the phase's lattice -- no lane issues a load of its own at a stride of d.  A table of the items' LDS
// offsets stands beside the tile; a step's B operand is one ds_read, read once for all the row tiles a wave accumulates;
// the weights are arranged as A operands once per call (dcf_wt_kernel).  The maps go through LDS in chunks where the
// smallest tile of all of them outgrows GC_LDS_MAX.
// Narrower layers (dcf_kernel): grid (images x tiles of a phase plane, phases, chunks of DCF_KT outputs), one output pixel
// of the phase a lane and DCF_KT accumulators; the reduced maps go through LDS in chunks of planes of the phase's source
// tile (staged by row spans as above); a staged value feeds DCF_KT fmafs, the weights come through the scalar cache.
// Weight gradient: gconv.hip's two forms with the tap offsets multiplied by d (dilconv.h says why no phases): slabs of
// pixel tiles, one partial a slab in dW's layout, tn_red_wgrad finishes dW and db in slab order -- the same bits every run.
// d = 1 with a stride above 1 is the dense layer and is handed to tn_conv2d_*.
// Index range: fewer than 2^32 elements a tensor, at most 65535 maps, rows and columns, f <= 32, d <= 255, K C f f < 2^28.
#include "dilconv.h"

#define DCF_KT 8

typedef float dcf_f32x4 __attribute__((ext_vector_type(4)));

struct DCF {
    const float* src;
    const float* W;
    const float* wt;           // matrix-core form: the arranged weights
    float* out;
    const float* bias;
    const float* prev_a;
    int R, O;                  // reduced / output maps
    int Hs, Ws, Ho, Wo;        // source and output planes of this product
    int wso, wsr;              // W's stride of an output / a reduced map, in elements
    int f, d, dPy, dPx, off0;
    int lgTW, lgTH, lgWU, npr, TH, IH, IW, IWp, span, RCH, NCH, R4c, MT, OCH, tilesX, tiles;
    unsigned tabbytes;
    int act;
    float prm;
};

// One chunk of the phase's source tile: planes r0 .. r0 + RCH - 1 (+0 past R) of rows sy0 + d r, the columns sx0 + d c out
// of the contiguous span sx0 .. sx0 + span - 1
__device__ __forceinline__ void dcf_stage(const DCF& g, const float* srcn, float* tile, int r0, int sy0, int sx0, int t) {
    const int per = g.IH * g.span;
    for (int i = t; i < g.RCH * per; i += 256) {
        const int pl = i / per, rem = i - pl * per, r = rem / g.span, j = rem - r * g.span;
        const int gy = sy0 + g.d * r, gx = sx0 + j;
        float v = 0.f;
        if (r0 + pl < g.R && gy >= 0 && gy < g.Hs && gx >= 0 && gx < g.Ws) v = srcn[((size_t)(r0 + pl) * g.Hs + gy) * g.Ws + gx];
        const int c = j / g.d;
        if (c * g.d == j) tile[(pl * g.IH + r) * g.IWp + c] = v;
    }
}

__device__ __forceinline__ float dcf_epilogue(const DCF& g, int mode, float z, float bv, size_t at) {
    const bool lk = g.act == TN_ACT_LEAKY;
    const float prm = g.prm;
    if (mode == 0) {
        z += bv;
        return lk ? fmaxf(0.f, z) + fminf(0.f, z) * prm : tn_act_fwd(z, g.act, prm);
    }
    if (g.prev_a) {
        const float a = g.prev_a[at], tie = prm > 0.f ? 1.f + prm : 0.f;
        z *= lk ? (a > 0.f ? 1.f : (a < 0.f ? prm : tie)) : tn_act_grad_from_out(a, g.act, prm);
    }
    return z;
}

// wt[(((mt NCH + ch) R4c + step) 64 + lane] = W(row 16 mt + lane % 16, item 4 step + lane / 16 of chunk ch: tap rc / RCH,
// reduced map ch RCH + rc % RCH); forward: row = filter, reduced = channel; dgrad: swapped.  Zero past the ends.
__global__ __launch_bounds__(256) void dcf_wt_kernel(const float* __restrict__ W, float* __restrict__ wt, int K, int C, int T,
                                                    int RCH, int NCH, int R4c, int dgrad, unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int l = idx & 63u;
    const unsigned rest = idx >> 6;
    const int step = rest % (unsigned)R4c;
    const unsigned r2 = rest / (unsigned)R4c;
    const int ch = r2 % (unsigned)NCH, mt = r2 / (unsigned)NCH;
    const int row = 16 * mt + (l & 15), rc = 4 * step + (l >> 4);
    const int tap = rc / RCH, red = ch * RCH + rc - tap * RCH;
    const int k = dgrad ? red : row, c = dgrad ? row : red;
    wt[idx] = (tap < T && k < K && c < C) ? W[((size_t)k * C + c) * T + tap] : 0.f;
}

template <int MODE>
__global__ __launch_bounds__(256) void dcf_mfma_kernel(DCF g) {
    extern __shared__ __attribute__((aligned(16))) char dcf_smem[];
    int* const tab = reinterpret_cast<int*>(dcf_smem);        // [4 R4c] LDS offset of the item, -1 past the end
    float* const tile = reinterpret_cast<float*>(dcf_smem + g.tabbytes);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, px = lane & 15;
    const unsigned n = blockIdx.x / (unsigned)g.tiles, tl = blockIdx.x - n * (unsigned)g.tiles;
    const int pyh = (int)blockIdx.y / g.dPx, pxh = (int)blockIdx.y - pyh * g.dPx;
    const int ty = (int)tl / g.tilesX, tx = (int)tl - ty * g.tilesX;
    const int TW = 1 << g.lgTW, d = g.d, f = g.f, y0 = ty * g.TH, x0 = tx * TW;
    if (y0 >= dc_count(g.Ho, pyh, d) || x0 >= dc_count(g.Wo, pxh, d)) return;      // a ragged phase: no such tile
    const int sy0 = pyh + g.off0 + d * y0, sx0 = pxh + g.off0 + d * x0;
    const float* const srcn = g.src + (size_t)n * g.R * g.Hs * g.Ws;

    for (int i = t; i < 4 * g.R4c; i += 256) {
        int e = -1;
        if (i < f * f * g.RCH) {
            const int tap = i / g.RCH, c = i - tap * g.RCH, u = tap / f, v = tap - u * f;
            const int du = MODE == 0 ? f - 1 - u : u, dv = MODE == 0 ? f - 1 - v : v;
            e = (c * g.IH + du) * g.IWp + dv;
        }
        tab[i] = e;
    }
    const int wu = wave & ((1 << g.lgWU) - 1), wm = wave >> g.lgWU, WM = 4 >> g.lgWU;
    const int col = px & (TW - 1), rsub = px >> g.lgTW, ox = pxh + d * (x0 + col);
    int oy[4], base[4];
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rl = ((wu * g.npr + i) << (4 - g.lgTW)) + rsub;
        oy[i] = pyh + d * (y0 + rl);
        base[i] = rl * g.IWp + col;
        live[i] = i < g.npr && oy[i] < g.Ho && ox < g.Wo;
    }
    const int mt0 = (int)blockIdx.z * DC_MTB * WM + wm;
    dcf_f32x4 acc[DC_MTB][4];
#pragma unroll
    for (int m = 0; m < DC_MTB; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[m][i] = dcf_f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < g.NCH; ++ch) {
        if (ch) __syncthreads();
        dcf_stage(g, srcn, tile, ch * g.RCH, sy0, sx0, t);
        __syncthreads();
        for (int step = 0; step < g.R4c; ++step) {
            const int e = tab[4 * step + q];
            float b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = (e >= 0 && live[i]) ? tile[base[i] + e] : 0.f;
#pragma unroll
            for (int m = 0; m < DC_MTB; ++m) {
                const int mt = mt0 + m * WM;
                if (mt >= g.MT) break;
                const float a = g.wt[(((size_t)mt * g.NCH + ch) * g.R4c + step) * 64 + lane];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < g.npr) acc[m][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[i], acc[m][i], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < DC_MTB; ++m) {
        const int mt = mt0 + m * WM;
        if (mt >= g.MT) break;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = 16 * mt + 4 * q + e;
            if (o >= g.O) break;
            const float bv = MODE == 0 ? g.bias[o] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!live[i]) continue;
                const size_t at = (((size_t)n * g.O + o) * g.Ho + oy[i]) * g.Wo + ox;
                g.out[at] = dcf_epilogue(g, MODE, acc[m][i][e], bv, at);
            }
        }
    }
}

// the register-tiled form: lane (ly, lx) owns pixel (y0 + ly, x0 + lx) of the phase plane and DCF_KT outputs
template <int MODE>
__global__ __launch_bounds__(256) void dcf_kernel(DCF g) {
    extern __shared__ __attribute__((aligned(16))) float dcf_tile[];      // [RCH][IH][IWp]
    const int t = threadIdx.x, f = g.f, d = g.d;
    const unsigned n = blockIdx.x / (unsigned)g.tiles, tl = blockIdx.x - n * (unsigned)g.tiles;
    const int pyh = (int)blockIdx.y / g.dPx, pxh = (int)blockIdx.y - pyh * g.dPx, o0 = (int)blockIdx.z * DCF_KT;
    const int ty = (int)tl / g.tilesX, tx = (int)tl - ty * g.tilesX;
    const int TW = 1 << g.lgTW, TH = 1 << g.lgTH, y0 = ty * TH, x0 = tx * TW;
    if (y0 >= dc_count(g.Ho, pyh, d) || x0 >= dc_count(g.Wo, pxh, d)) return;
    const int sy0 = pyh + g.off0 + d * y0, sx0 = pxh + g.off0 + d * x0;
    const int lx = t & (TW - 1), ly = t >> g.lgTW, oy = pyh + d * (y0 + ly), ox = pxh + d * (x0 + lx);
    const bool live = ly < TH && oy < g.Ho && ox < g.Wo;
    const float* const srcn = g.src + (size_t)n * g.R * g.Hs * g.Ws;
    float acc[DCF_KT];
#pragma unroll
    for (int j = 0; j < DCF_KT; ++j) acc[j] = 0.f;

    for (int r0 = 0; r0 < g.R; r0 += g.RCH) {
        const int nr = g.R - r0 < g.RCH ? g.R - r0 : g.RCH;
        __syncthreads();
        dcf_stage(g, srcn, dcf_tile, r0, sy0, sx0, t);
        __syncthreads();
        for (int rr = 0; rr < nr; ++rr) {
            const float* const tp = dcf_tile + rr * g.IH * g.IWp;
            const float* const wr = g.W + (size_t)(r0 + rr) * g.wsr;
            for (int u = 0; u < f; ++u)
                for (int v = 0; v < f; ++v) {
                    // W[.., u, v] meets the phase's source at offset f-1-u (forward: the flip), u (input gradient)
                    const int du = MODE == 0 ? f - 1 - u : u, dv = MODE == 0 ? f - 1 - v : v;
                    const float xv = live ? tp[(ly + du) * g.IWp + lx + dv] : 0.f;
                    const float* const wt = wr + u * f + v;
#pragma unroll
                    for (int j = 0; j < DCF_KT; ++j) {
                        const float w = o0 + j < g.O ? wt[(size_t)(o0 + j) * g.wso] : 0.f;
                        acc[j] = fmaf(xv, w, acc[j]);
                    }
                }
        }
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < DCF_KT; ++j) {
        const int o = o0 + j;
        if (o >= g.O) break;
        const size_t at = (((size_t)n * g.O + o) * g.Ho + oy) * g.Wo + ox;
        g.out[at] = dcf_epilogue(g, MODE, acc[j], MODE == 0 ? g.bias[o] : 0.f, at);
    }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------
struct DCFW {
    const float* x;
    const float* dz;
    float* ws;                 // [slab][K][C][f][f]
    float* dbws;               // [slab][K]
    int C, K, KT, H, Wd, Ho, Wo, f, d, pad, NCOL;
    unsigned HoWo, ntiles, nslab;
    unsigned long long npix;
};

// grid (slabs, filters, chunks of 8 channels): gconv.hip's gcf_wgrad_kernel with dilated tap shifts
__global__ __launch_bounds__(256) void dcf_wgrad_kernel(DCFW g) {
    __shared__ float red[4][9];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, slab = blockIdx.x;
    const int k = blockIdx.y, c0 = 8 * blockIdx.z, T = g.f * g.f;
    const size_t HW = (size_t)g.H * g.Wd;
    for (int tap = 0; tap < T; ++tap) {
        const int u = tap / g.f, v = tap - u * g.f;
        const int dy = (g.f - 1 - u) * g.d - g.pad, dx = (g.f - 1 - v) * g.d - g.pad;
        float acc[9];                           // 8 channels, then db (tap 0)
#pragma unroll
        for (int j = 0; j < 9; ++j) acc[j] = 0.f;
        for (unsigned tile = slab; tile < g.ntiles; tile += g.nslab) {
            const unsigned long long gi = (unsigned long long)tile * 256 + t;
            if (gi >= g.npix) continue;
            const unsigned n = (unsigned)(gi / g.HoWo), q = (unsigned)(gi - (unsigned long long)n * g.HoWo);
            const int oh = (int)(q / (unsigned)g.Wo), ow = (int)q - oh * g.Wo;
            const float dv = g.dz[((size_t)n * g.K + k) * g.HoWo + q];
            if (tap == 0) acc[8] += dv;
            const int sy = oh + dy, sx = ow + dx;
            if (sy < 0 || sy >= g.H || sx < 0 || sx >= g.Wd) continue;
            const float* const xp = g.x + ((size_t)n * g.C + c0) * HW + (size_t)sy * g.Wd + sx;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + j < g.C) acc[j] = fmaf(dv, xp[j * HW], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            float s = acc[j];
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
            if (lane == 0) red[wave][j] = s;
        }
        __syncthreads();
        if (t < 9) {
            const float s = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
            if (t < 8) {
                if (c0 + (int)t < g.C) g.ws[(((size_t)slab * g.K + k) * g.C + c0 + t) * T + tap] = s;
            } else if (tap == 0 && blockIdx.z == 0) {
                g.dbws[(size_t)slab * g.K + k] = s;
            }
        }
        __syncthreads();
    }
}

// On the matrix core (K >= 16, C >= 4; gconv.hip's gcf_wgrad_mfma_kernel with dilated tap shifts): the 16 rows are 16
// filters, the 16 columns 16 consecutive (channel, tap) columns of dW's own layout, the 4-deep reduction four output
// pixels.  grid (slabs, chunks of 32 column tiles, 16-filter tiles).  A block walks its slab's tiles of 64 output pixels:
// the 16 filters' dz values and the pixels' (image, row, column) are staged in LDS once a tile; a wave owns up to 8 column
// tiles and keeps their sums in registers, the B operand is the x value at the tap's dilated shift through the vector
// cache (+0 outside the map).  Waves own disjoint columns.  db from the staged dz.
__global__ __launch_bounds__(256) void dcf_wgrad_mfma_kernel(DCFW g) {
    __shared__ float sd[16][64];
    __shared__ int spix[3][64];                  // image, output row / column; row -(1 << 20): no pixel
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, q = lane >> 4, slab = blockIdx.x;
    const int k0 = (int)blockIdx.z * 16, T = g.f * g.f;
    const size_t HW = (size_t)g.H * g.Wd;
    long long xoff[8];
    int dy[8], dx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int colj = ((int)blockIdx.y * 32 + (int)wave + 4 * j) * 16 + (int)(lane & 15u);
        const int c = colj / T, tap = colj - c * T, u = tap / g.f, v = tap - u * g.f;
        const bool valid = colj < g.NCOL;
        dy[j] = valid ? (g.f - 1 - u) * g.d - g.pad : 1 << 20;
        dx[j] = (g.f - 1 - v) * g.d - g.pad;
        xoff[j] = valid ? (long long)c * (long long)HW : 0;
    }
    dcf_f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = dcf_f32x4{0.f, 0.f, 0.f, 0.f};
    float dbs[4] = {0.f, 0.f, 0.f, 0.f};
    const int ntw = ((g.NCOL + 15) / 16 - (int)blockIdx.y * 32 - (int)wave + 3) / 4;      // this wave's column tiles

    for (unsigned tile = slab; tile < g.ntiles; tile += g.nslab) {
        const unsigned long long gi = (unsigned long long)tile * 64 + lane;
        const bool valid = gi < g.npix;
        const unsigned n = valid ? (unsigned)(gi / g.HoWo) : 0u, qq = valid ? (unsigned)(gi - (unsigned long long)n * g.HoWo) : 0u;
        __syncthreads();
        if (wave == 0) {
            const int oh = (int)(qq / (unsigned)g.Wo), ow = (int)qq - oh * g.Wo;
            spix[0][lane] = (int)n;
            spix[1][lane] = valid ? oh : -(1 << 20);
            spix[2][lane] = ow;
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int kl = k0 + (int)wave + 4 * jj;
            const float dv = (valid && kl < g.K) ? g.dz[((size_t)n * g.K + kl) * g.HoWo + qq] : 0.f;
            sd[wave + 4 * jj][lane] = dv;
            dbs[jj] += dv;
        }
        __syncthreads();
        for (int step = 0; step < 16; ++step) {
            const int p = 4 * step + (int)q;
            const float a = sd[lane & 15u][p];
            const int pn = spix[0][p], py = spix[1][p], pxx = spix[2][p];
            const float* const xn = g.x + (size_t)pn * g.C * HW;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (j >= ntw) break;
                const int sy = py + dy[j], sx = pxx + dx[j];
                float b = 0.f;
                if (sy >= 0 && sy < g.H && sx >= 0 && sx < g.Wd) b = xn[xoff[j] + (long long)sy * g.Wd + sx];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[j], 0, 0, 0);
            }
        }
    }
    float* const ws = g.ws + (size_t)slab * g.K * g.NCOL;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int colj = ((int)blockIdx.y * 32 + (int)wave + 4 * j) * 16 + (int)(lane & 15u);
        if (colj >= g.NCOL) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kl = k0 + 4 * (int)q + e;
            if (kl < g.K) ws[(size_t)kl * g.NCOL + colj] = acc[j][e];
        }
    }
    if (blockIdx.y == 0) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            float s = dbs[jj];
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
            const int kl = k0 + (int)wave + 4 * jj;
            if (lane == 0 && kl < g.K) g.dbws[(size_t)slab * g.K + kl] = s;
        }
    }
}

static bool dcf_ok(int N, int C, int H, int Wd, int K, int d, int f, int stride, int pad, int Ho, int Wo) {
    if (N < 1 || C < 1 || K < 1 || K > 65535 || C > 65535 || H > 65535 || Wd > 65535) return false;
    if (!dc_axis_ok(H, f, d, stride, pad, Ho) || !dc_axis_ok(Wd, f, d, stride, pad, Wo)) return false;
    if ((long long)N * C * H * Wd >= (1ll << 32) || (long long)N * K * Ho * Wo >= (1ll << 32)) return false;
    return (long long)K * C * f * f < (1ll << 28);
}

#define DCF_ARGS_FMT "(N %d, %d maps of %d x %d -> %d maps of %d x %d, dilation %d, filter %d stride %d pad_lo %d)"
#define DCF_ARGS N, C, H, Wd, K, Ho, Wo, d, f, stride, pad

static int dcf_lg(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// q arrives with the tensors, the maps and the planes of the product filled in; K and C are the layer's
static int dcf_run(tn_ctx* ctx, DCF& q, int mode, int N, int K, int C) {
    const int T = q.f * q.f, cy = dc_count(q.Ho, 0, q.d), cx = dc_count(q.Wo, 0, q.d);     // the largest phase plane
    q.dPy = q.d < q.Ho ? q.d : q.Ho;
    q.dPx = q.d < q.Wo ? q.d : q.Wo;
    const unsigned phases = (unsigned)(q.dPy * q.dPx);
    if (K >= 16 && C >= 4) {
        q.lgTW = cx <= 4 ? 2 : (cx <= 8 ? 3 : 4);
        const int TW = 1 << q.lgTW, RU = 16 >> q.lgTW, WU = dc_waves_over_pixels(cy, RU), WM = 4 / WU;
        q.lgWU = WU == 4 ? 2 : (WU == 2 ? 1 : 0);
        q.MT = (q.O + 15) / 16;
        q.npr = 4;
        while (q.npr > 1 && WU * (q.npr / 2) * RU >= cy) q.npr /= 2;
        q.IW = TW + q.f - 1;
        q.IWp = q.IW | 1;
        q.span = (q.IW - 1) * q.d + 1;
        q.RCH = q.R;
        size_t lds;
        for (;;) {                                              // shrink the tile, then chunk the maps, until LDS holds it
            q.TH = WU * q.npr * RU;
            q.IH = (q.TH < cy ? q.TH : cy) + q.f - 1;
            q.R4c = (T * q.RCH + 3) / 4;
            q.tabbytes = (4u * q.R4c * (unsigned)sizeof(int) + 15u) & ~15u;
            lds = q.tabbytes + (size_t)q.RCH * q.IH * q.IWp * sizeof(float);
            if (lds <= GC_LDS_MAX) break;
            if (q.npr > 1) q.npr /= 2;
            else q.RCH = (q.RCH + 1) / 2;
        }
        q.NCH = (q.R + q.RCH - 1) / q.RCH;
        q.tilesX = (cx + TW - 1) / TW;
        q.tiles = q.tilesX * ((cy + q.TH - 1) / q.TH);
        const size_t total = (size_t)q.MT * q.NCH * q.R4c * 64;
        const unsigned long long blocks = (unsigned long long)N * q.tiles;
        const int ZB = (q.MT + DC_MTB * WM - 1) / (DC_MTB * WM);
        TN_REQUIRE(total < (1ull << 31) && blocks < (1ull << 31), "dilconv: %d images of %d tiles: too large", N, q.tiles);
        float* wt;
        int rc = tn_scratch_get(ctx, total * sizeof(float), &wt);
        if (rc) return rc;
        dcf_wt_kernel<<<cdiv((long long)total, 256), 256, 0, ctx->stream>>>(q.W, wt, K, C, T, q.RCH, q.NCH, q.R4c, mode, (unsigned)total);
        TN_LAUNCH_CHECK();
        q.wt = wt;
        const dim3 grid((unsigned)blocks, phases, (unsigned)ZB);
        rc = mode == 0 ? tn_launch_lds<dcf_mfma_kernel<0>>(ctx, grid, dim3(256), lds, q)
                       : tn_launch_lds<dcf_mfma_kernel<1>>(ctx, grid, dim3(256), lds, q);
        if (rc) return rc;
        TN_LAUNCH_CHECK();
        return TN_OK;
    }
    q.OCH = (q.O + DCF_KT - 1) / DCF_KT;
    q.lgTW = dcf_lg(cx < 16 ? cx : 16);
    q.lgTH = dcf_lg(cy < 16 ? cy : 16);
    if (q.lgTH > 8 - q.lgTW) q.lgTH = 8 - q.lgTW;
    q.IH = (1 << q.lgTH) + q.f - 1;                             // (f <= 32: a plane of the 16 x 16 tile is 47 x 47 floats)
    q.IW = (1 << q.lgTW) + q.f - 1;
    q.IWp = q.IW | 1;
    q.span = (q.IW - 1) * q.d + 1;
    const size_t plane = (size_t)q.IH * q.IWp * sizeof(float);
    q.RCH = (int)(GC_LDS_MAX / plane);
    if (q.RCH > q.R) q.RCH = q.R;
    q.tilesX = (cx + (1 << q.lgTW) - 1) >> q.lgTW;
    q.tiles = q.tilesX * ((cy + (1 << q.lgTH) - 1) >> q.lgTH);
    const unsigned long long blocks = (unsigned long long)N * q.tiles;
    TN_REQUIRE(blocks < (1ull << 31), "dilconv: %d images of %d tiles: too large", N, q.tiles);
    const dim3 grid((unsigned)blocks, phases, (unsigned)q.OCH);
    const size_t lds = (size_t)q.RCH * plane;
    const int rc = mode == 0 ? tn_launch_lds<dcf_kernel<0>>(ctx, grid, dim3(256), lds, q)
                             : tn_launch_lds<dcf_kernel<1>>(ctx, grid, dim3(256), lds, q);
    if (rc) return rc;
    TN_LAUNCH_CHECK();
    return TN_OK;
}

extern "C" {

int tn_dilconv_supported(int N, int C, int H, int Wd, int K, int d, int f, int stride, int pad, int Ho, int Wo) {
    return dcf_ok(N, C, H, Wd, K, d, f, stride, pad, Ho, Wo) ? 1 : 0;
}

int tn_dilconv_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int N, int C, int H, int Wd, int K, int d,
                   int f, int stride, int pad, int Ho, int Wo, int act, float prm) {
    TN_REQUIRE(x && W && b && a && dcf_ok(N, C, H, Wd, K, d, f, stride, pad, Ho, Wo), "tn_dilconv_fwd: bad arguments " DCF_ARGS_FMT,
               DCF_ARGS);
    TN_FP32_ONLY(ctx, "tn_dilconv_fwd");
    if (stride != 1) return tn_conv2d_fwd(ctx, x, W, b, a, N, C, H, Wd, K, f, stride, pad, Ho, Wo, act, prm);
    DCF q{};
    q.src = x; q.W = W; q.out = a; q.bias = b; q.act = act; q.prm = prm;
    q.R = C; q.O = K;
    q.Hs = H; q.Ws = Wd; q.Ho = Ho; q.Wo = Wo;
    q.wso = C * f * f; q.wsr = f * f;
    q.f = f; q.d = d; q.off0 = -pad;
    return dcf_run(ctx, q, 0, N, K, C);
}

int tn_dilconv_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int N, int C, int H, int Wd, int K, int d, int f,
                     int stride, int pad, int Ho, int Wo, const float* prev_a, int prev_act, float prev_prm) {
    TN_REQUIRE(dz && W && dx && dcf_ok(N, C, H, Wd, K, d, f, stride, pad, Ho, Wo), "tn_dilconv_dgrad: bad arguments " DCF_ARGS_FMT,
               DCF_ARGS);
    TN_FP32_ONLY(ctx, "tn_dilconv_dgrad");
    if (stride != 1) return tn_conv2d_dgrad(ctx, dz, W, dx, N, C, H, Wd, K, f, stride, pad, Ho, Wo, prev_a, prev_act, prev_prm);
    DCF q{};
    q.src = dz; q.W = W; q.out = dx; q.prev_a = prev_a; q.act = prev_act; q.prm = prev_prm;
    q.R = K; q.O = C;
    q.Hs = Ho; q.Ws = Wo; q.Ho = H; q.Wo = Wd;
    q.wso = f * f; q.wsr = C * f * f;
    q.f = f; q.d = d; q.off0 = pad - (f - 1) * d;
    return dcf_run(ctx, q, 1, N, K, C);
}

int tn_dilconv_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int N, int C, int H, int Wd, int K, int d,
                     int f, int stride, int pad, int Ho, int Wo) {
    TN_REQUIRE(x && dz && dW && db && dcf_ok(N, C, H, Wd, K, d, f, stride, pad, Ho, Wo),
               "tn_dilconv_wgrad: bad arguments " DCF_ARGS_FMT, DCF_ARGS);
    TN_FP32_ONLY(ctx, "tn_dilconv_wgrad");
    if (stride != 1) return tn_conv2d_wgrad(ctx, x, dz, dW, db, N, C, H, Wd, K, f, stride, pad, Ho, Wo);
    DCFW m{};
    m.x = x; m.dz = dz; m.C = C; m.K = K; m.KT = (K + 15) / 16;
    m.H = H; m.Wd = Wd; m.Ho = Ho; m.Wo = Wo; m.f = f; m.d = d; m.pad = pad; m.NCOL = C * f * f;
    m.HoWo = (unsigned)Ho * Wo;
    m.npix = (unsigned long long)N * m.HoWo;
    const size_t n = (size_t)K * m.NCOL;
    const bool mfma = K >= 16 && C >= 4;
    const int CH = mfma ? cdiv(cdiv(m.NCOL, 16), 32) : (C + 7) / 8;
    const long long nt = (long long)((m.npix + (mfma ? 63 : 255)) / (mfma ? 64 : 256));
    TN_REQUIRE(CH <= 65535, "tn_dilconv_wgrad: %d x %d x %d x %d weights: too large", K, C, f, f);
    m.ntiles = (unsigned)nt; m.nslab = gc_slabs(nt, (long long)CH * (mfma ? m.KT : K), 1024);
    int rc = tn_scratch_get(ctx, (size_t)m.nslab * (n + K) * sizeof(float), &m.ws);
    if (rc) return rc;
    m.dbws = m.ws + (size_t)m.nslab * n;
    if (mfma) dcf_wgrad_mfma_kernel<<<dim3(m.nslab, (unsigned)CH, (unsigned)m.KT), 256, 0, ctx->stream>>>(m);
    else dcf_wgrad_kernel<<<dim3(m.nslab, (unsigned)K, (unsigned)CH), 256, 0, ctx->stream>>>(m);
    TN_LAUNCH_CHECK();
    return tn_red_wgrad(ctx, m.ws, dW, (uint32_t)n, m.nslab, (uint32_t)n, m.dbws, db, (uint32_t)K, m.nslab, (uint32_t)K);
}

}  // extern "C"
