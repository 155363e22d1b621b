// ConvLayer(..., groups=g) on fp32 NCHW tensors: tn_gconv_fwd / _dgrad / _wgrad.  The arguments are tn_conv2d_*'s with g
// behind K; W (K, C/g, f, f), b (K).  Products and accumulation in fp32 (fmaf), under every CONV mode: CONV 'bfloat16'
// rounds the operands of the dense family's matrix product, a grouped layer stays on these kernels unchanged.  Like
// tn_conv2d_* they refuse to run while a 16-bit DTYPE is in force (its entry points are tn_c8_gconv_*).
//
// A layer with K/g >= 16 and C/g >= 4 runs on the fp32 matrix core (v_mfma_f32_16x16x4_f32: gcf_mfma_kernel,
// gcf_wgrad_mfma_kernel, described where they stand); narrower groups, and a product whose source tile outgrows LDS, take
// the plain forms:
// Forward / input gradient (gcf_kernel, gconv.h for the modes and the tile): grid (images x tiles of the output plane,
// groups x chunks of GCF_KT outputs), 256 lanes, one output pixel a lane and GCF_KT accumulators -- GCF_KT outputs of ONE
// group (filters forward, channels input gradient).  The group's reduced maps go through LDS in chunks of RCH planes of the
// tile's source rows and columns (halo included, +0 outside the map, odd row stride); a staged value feeds GCF_KT fmafs.
// The weights are read at block-uniform addresses (scalar loads, the scalar cache).  The tile is 16 x 16 (smaller planes:
// the power of two above the side) and halves until one plane of it fits GC_LDS_MAX.
// Weight gradient (gcf_wgrad_kernel): grid (slabs, filters, chunks of 8 channels of the filter's group).  The output pixels
// of the batch are cut into tiles of 256, slab k takes tiles k, k + nslab, ...; tap by tap a lane multiplies its dz value
// with the tap-shifted x of 8 channels, the wave adds up by cross-lane moves, the four waves' sums are added in wave
// order and the block writes one partial per slab in dW's layout; tn_red_wgrad finishes dW and db in slab order: no
// atomics, the same bits every run.
// Index range: fewer than 2^32 elements a tensor, at most 65535 rows / columns, f <= 64, K C/g f f < 2^28.
#include "gconv.h"

#define GCF_KT 8

struct GCF {
    const float* src;
    const float* W;
    float* out;
    const float* bias;
    const float* prev_a;
    int R, O, Rg, Og, OCH;     // reduced / output maps of the tensor and of a group, output chunks a group
    int Hs, Ws, Ho, Wo;        // source and output planes of this product
    int wso, wsr;              // W's stride of an output / a reduced map of the group, in elements
    int KgCgT;                 // weights of a group
    int f, stride, off0;
    int lgTW, lgTH, IH, IW, IWp, RCH, tilesX, tiles;
    const float* wt;           // matrix-core form: the arranged weights
    int RC, R4, MT, npr, TH;   // ... reduction items f f Rg, steps of four, 16-row tiles, pixel units a wave, tile rows
    unsigned tabbytes;
    int act;
    float prm;
};

template <int MODE>
__global__ __launch_bounds__(256) void gcf_kernel(GCF g) {
    extern __shared__ __attribute__((aligned(16))) float gcf_tile[];      // [RCH][IH][IWp]
    const int t = threadIdx.x, f = g.f, s = g.stride, se = MODE == 0 ? s : 1;
    const unsigned n = blockIdx.x / (unsigned)g.tiles, tl = blockIdx.x - n * (unsigned)g.tiles;
    const int grp = blockIdx.y / g.OCH, o0 = (blockIdx.y - grp * g.OCH) * GCF_KT;
    const int ty = (int)tl / g.tilesX, tx = (int)tl - ty * g.tilesX;
    const int TW = 1 << g.lgTW, TH = 1 << g.lgTH;
    const int y0 = ty * TH, x0 = tx * TW;
    const int sy0 = gc_src0(MODE, y0, g.off0, s), sx0 = gc_src0(MODE, x0, g.off0, s);
    const int lx = t & (TW - 1), ly = t >> g.lgTW, oy = y0 + ly, ox = x0 + lx;
    const bool live = ly < TH && oy < g.Ho && ox < g.Wo;
    const float* const srcn = g.src + ((size_t)n * g.R + (size_t)grp * g.Rg) * g.Hs * g.Ws;
    const float* const Wg = g.W + (size_t)grp * g.KgCgT;
    float acc[GCF_KT];
#pragma unroll
    for (int j = 0; j < GCF_KT; ++j) acc[j] = 0.f;

    const int per = g.IH * g.IW;
    for (int r0 = 0; r0 < g.Rg; r0 += g.RCH) {
        const int nr = g.Rg - r0 < g.RCH ? g.Rg - r0 : g.RCH;
        __syncthreads();
        for (int i = t; i < nr * per; i += 256) {
            const int pl = i / per, rem = i - pl * per, r = rem / g.IW, c = rem - r * g.IW;
            const int gy = sy0 + r, gx = sx0 + c;
            float v = 0.f;
            if (gy >= 0 && gy < g.Hs && gx >= 0 && gx < g.Ws) v = srcn[((size_t)(r0 + pl) * g.Hs + gy) * g.Ws + gx];
            gcf_tile[(pl * g.IH + r) * g.IWp + c] = v;
        }
        __syncthreads();
        for (int rr = 0; rr < nr; ++rr) {
            const float* const tp = gcf_tile + rr * g.IH * g.IWp;
            const float* const wr = Wg + (size_t)(r0 + rr) * g.wsr;
            for (int u = 0; u < f; ++u)
                for (int v = 0; v < f; ++v) {
                    // W[.., u, v] meets the source at offset f-1-u (forward: the flip), u (input gradient)
                    const int du = MODE == 0 ? f - 1 - u : u, dv = MODE == 0 ? f - 1 - v : v;
                    float xv = 0.f;
                    if (live) {
                        if (MODE != 2) {
                            xv = tp[(ly * se + du) * g.IWp + lx * se + dv];
                        } else {
                            const int sy = oy + g.off0 + du, sx = ox + g.off0 + dv, qy = sy / s, qx = sx / s;
                            if (sy >= 0 && sx >= 0 && qy * s == sy && qx * s == sx) xv = tp[(qy - sy0) * g.IWp + qx - sx0];
                        }
                    }
                    const float* const wt = wr + u * f + v;
#pragma unroll
                    for (int j = 0; j < GCF_KT; ++j) {
                        const float w = o0 + j < g.Og ? wt[(size_t)(o0 + j) * g.wso] : 0.f;
                        acc[j] = fmaf(xv, w, acc[j]);
                    }
                }
        }
    }
    if (!live) return;
    const bool lk = g.act == TN_ACT_LEAKY;
    const float prm = g.prm, tie = prm > 0.f ? 1.f + prm : 0.f;
#pragma unroll
    for (int j = 0; j < GCF_KT; ++j) {
        if (o0 + j >= g.Og) break;
        const int o = grp * g.Og + o0 + j;
        const size_t at = (((size_t)n * g.O + o) * g.Ho + oy) * g.Wo + ox;
        float z = acc[j];
        if (MODE == 0) {
            z += g.bias[o];
            z = lk ? fmaxf(0.f, z) + fminf(0.f, z) * prm : tn_act_fwd(z, g.act, prm);
        } else if (g.prev_a) {
            const float a = g.prev_a[at];
            z *= lk ? (a > 0.f ? 1.f : (a < 0.f ? prm : tie)) : tn_act_grad_from_out(a, g.act, prm);
        }
        g.out[at] = z;
    }
}

struct GCFW {
    const float* x;
    const float* dz;
    float* ws;                 // [slab][K][C/g][f][f]
    float* dbws;               // [slab][K]
    int C, K, Cg, Kg, H, Wd, Ho, Wo, f, stride, pad;
    unsigned HoWo, ntiles, nslab;
    unsigned long long npix;
};

// grid (slabs, filters, chunks of 8 channels of the filter's group)
__global__ __launch_bounds__(256) void gcf_wgrad_kernel(GCFW g) {
    __shared__ float red[4][9];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, slab = blockIdx.x;
    const int k = blockIdx.y, c0 = 8 * blockIdx.z, grp = k / g.Kg, T = g.f * g.f;
    const size_t HW = (size_t)g.H * g.Wd;
    for (int tap = 0; tap < T; ++tap) {
        const int u = tap / g.f, v = tap - u * g.f;
        const int dy = g.f - 1 - u - g.pad, dx = g.f - 1 - v - g.pad;
        float acc[9];                           // 8 channels, then db (tap 0)
#pragma unroll
        for (int j = 0; j < 9; ++j) acc[j] = 0.f;
        for (unsigned tile = slab; tile < g.ntiles; tile += g.nslab) {
            const unsigned long long gi = (unsigned long long)tile * 256 + t;
            if (gi >= g.npix) continue;
            const unsigned n = (unsigned)(gi / g.HoWo), q = (unsigned)(gi - (unsigned long long)n * g.HoWo);
            const int oh = (int)(q / (unsigned)g.Wo), ow = (int)q - oh * g.Wo;
            const float d = g.dz[((size_t)n * g.K + k) * g.HoWo + q];
            if (tap == 0) acc[8] += d;
            const int sy = oh * g.stride + dy, sx = ow * g.stride + dx;
            if (sy < 0 || sy >= g.H || sx < 0 || sx >= g.Wd) continue;
            const float* const xp = g.x + ((size_t)n * g.C + (size_t)grp * g.Cg + c0) * HW + (size_t)sy * g.Wd + sx;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + j < g.Cg) acc[j] = fmaf(d, xp[j * HW], acc[j]);
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
                if (c0 + (int)t < g.Cg) g.ws[(((size_t)slab * g.K + k) * g.Cg + c0 + t) * T + tap] = s;
            } else if (tap == 0 && blockIdx.z == 0) {
                g.dbws[(size_t)slab * g.K + k] = s;
            }
        }
        __syncthreads();
    }
}


// ---- the matrix-core form (a layer with K/g >= 16 and C/g >= 4): v_mfma_f32_16x16x4_f32 ---------------------------------
// gconv_c8.hip's design on scalar planes.  The 16 rows are 16 outputs of one group, the 16 columns 16 pixels of the tile,
// the 4-deep reduction FOUR reduction items rc = tap * Rg + map, one a quarter wave: lane l holds pixel l % 16 of item
// 4 step + l / 16.  A block stages all Rg source planes of its tile, halo included, +0 outside the map, in LDS
// ([map][IH][IWp] floats) with a table of the items' LDS offsets (plane + tap shift): a step's B operand is one ds_read at
// pixel base + table[item].  The weights are arranged as A operands once per call (gcf_wt_kernel, context scratch); a wave
// loads a step's operand once and uses it for its up to four pixel units.  Tile: TW = 16 columns (8 / 4 on narrow planes)
// by 4 waves x npr units.  A lane's accumulators are outputs 4 (l / 16) .. + 3 of its pixel.  A tile that does not fit
// GC_LDS_MAX at npr = 1 leaves the product to gcf_kernel.
typedef float gcf_f32x4 __attribute__((ext_vector_type(4)));
#define GCF_ITEMS_MAX 4096

// wt[((grp MT + mt) R4 + step) 64 + lane] = W(row 16 mt + lane % 16 of the group, item 4 step + lane / 16: tap rc / Rg,
// reduced map rc % Rg); forward: row = filter, reduced = channel; dgrad: swapped.  Zero past the ends.
__global__ __launch_bounds__(256) void gcf_wt_kernel(const float* __restrict__ W, float* __restrict__ wt, int Kg, int Cg, int T,
                                                    int Rg, int R4, int MT, int dgrad, unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int l = idx & 63u;
    const unsigned rest = idx >> 6;
    const int step = rest % (unsigned)R4;
    const unsigned r2 = rest / (unsigned)R4;
    const int mt = r2 % (unsigned)MT, grp = r2 / (unsigned)MT;
    const int row = 16 * mt + (l & 15), rc = 4 * step + (l >> 4);
    const int tap = rc / Rg, red = rc - tap * Rg;
    const int kl = dgrad ? red : row, cl = dgrad ? row : red;
    wt[idx] = (tap < T && kl < Kg && cl < Cg) ? W[(((size_t)grp * Kg + kl) * Cg + cl) * T + tap] : 0.f;
}

// grid (images x tiles, groups)
template <int MODE>
__global__ __launch_bounds__(256) void gcf_mfma_kernel(GCF g) {
    extern __shared__ __attribute__((aligned(16))) char gcf_smem[];
    int2* const tab = reinterpret_cast<int2*>(gcf_smem);      // [4 R4] x: LDS offset of the item, y: (map, du, dv); -1 past the end
    float* const tile = reinterpret_cast<float*>(gcf_smem + g.tabbytes);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, px = lane & 15;
    const unsigned n = blockIdx.x / (unsigned)g.tiles, tl = blockIdx.x - n * (unsigned)g.tiles;
    const int grp = blockIdx.y, f = g.f, s = g.stride, se = MODE == 0 ? s : 1;
    const int ty = (int)tl / g.tilesX, tx = (int)tl - ty * g.tilesX;
    const int TW = 1 << g.lgTW, y0 = ty * g.TH, x0 = tx * TW;
    const int sy0 = gc_src0(MODE, y0, g.off0, s), sx0 = gc_src0(MODE, x0, g.off0, s);
    const float* const srcn = g.src + ((size_t)n * g.R + (size_t)grp * g.Rg) * g.Hs * g.Ws;

    for (int i = t; i < 4 * g.R4; i += 256) {
        int2 e = make_int2(-1, -1);
        if (i < g.RC) {
            const int tap = i / g.Rg, c = i - tap * g.Rg, u = tap / f, v = tap - u * f;
            const int du = MODE == 0 ? f - 1 - u : u, dv = MODE == 0 ? f - 1 - v : v;
            e = make_int2((c * g.IH + du) * g.IWp + dv, (c << 16) | (du << 8) | dv);
        }
        tab[i] = e;
    }
    const int per = g.IH * g.IW;
    for (int i = t; i < g.Rg * per; i += 256) {
        const int pl = i / per, rem = i - pl * per, r = rem / g.IW, c = rem - r * g.IW;
        const int gy = sy0 + r, gx = sx0 + c;
        float v = 0.f;
        if (gy >= 0 && gy < g.Hs && gx >= 0 && gx < g.Ws) v = srcn[((size_t)pl * g.Hs + gy) * g.Ws + gx];
        tile[(pl * g.IH + r) * g.IWp + c] = v;
    }
    __syncthreads();

    const int col = px & (TW - 1), rsub = px >> g.lgTW, ox = x0 + col;
    int oy[4], base[4];
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rl = ((wave * g.npr + i) << (4 - g.lgTW)) + rsub;
        oy[i] = y0 + rl;
        base[i] = rl * se * g.IWp + col * se;
        live[i] = i < g.npr && oy[i] < g.Ho && ox < g.Wo;
    }
    auto operand = [&](int i, int2 e) __attribute__((always_inline)) {
        float val = 0.f;
        if (e.x >= 0 && live[i]) {
            if (MODE != 2) {
                val = tile[base[i] + e.x];
            } else {
                const int sy = oy[i] + g.off0 + ((e.y >> 8) & 255), sx = ox + g.off0 + (e.y & 255), qy = sy / s, qx = sx / s;
                if (sy >= 0 && sx >= 0 && qy * s == sy && qx * s == sx)
                    val = tile[((e.y >> 16) * g.IH + (qy - sy0)) * g.IWp + (qx - sx0)];
            }
        }
        return val;
    };

    const bool lk = g.act == TN_ACT_LEAKY;
    const float prm = g.prm, tie = prm > 0.f ? 1.f + prm : 0.f;
    for (int mt = 0; mt < g.MT; ++mt) {
        gcf_f32x4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = gcf_f32x4{0.f, 0.f, 0.f, 0.f};
        const float* const wp = g.wt + ((size_t)grp * g.MT + mt) * g.R4 * 64 + lane;
        for (int step = 0; step < g.R4; ++step) {
            const float a = wp[(size_t)step * 64];
            const int2 e = tab[4 * step + q];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < g.npr) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, operand(i, e), acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ol = 16 * mt + 4 * q + e;
            if (ol >= g.Og) break;
            const int o = grp * g.Og + ol;
            const float bv = MODE == 0 ? g.bias[o] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!live[i]) continue;
                const size_t at = (((size_t)n * g.O + o) * g.Ho + oy[i]) * g.Wo + ox;
                float z = acc[i][e];
                if (MODE == 0) {
                    z += bv;
                    z = lk ? fmaxf(0.f, z) + fminf(0.f, z) * prm : tn_act_fwd(z, g.act, prm);
                } else if (g.prev_a) {
                    const float a_ = g.prev_a[at];
                    z *= lk ? (a_ > 0.f ? 1.f : (a_ < 0.f ? prm : tie)) : tn_act_grad_from_out(a_, g.act, prm);
                }
                g.out[at] = z;
            }
        }
    }
}

// Weight gradient on the matrix core: dW[k][c, tap] = sum over output pixels of dz[k][pixel] x[c][pixel shifted by tap] -- the 16
// rows are 16 filters of one group, the 16 columns 16 consecutive (channel, tap) columns of dW's own layout, the 4-deep
// reduction four output pixels.  grid (slabs, chunks of 32 column tiles, groups x 16-filter tiles).  A block walks its slab's
// tiles of 64 output pixels: it stages the 16 filters' dz values and the pixels' (image, row, column) in LDS ONCE a tile;
// a wave owns up to 8 column tiles (tiles wave, wave + 4, ...) and keeps their sums in registers, the A operand of a step
// is an LDS read shared by all of them, the B operand the tap-shifted x value through the vector cache (+0 outside the
// map).  Waves own disjoint columns: nothing to add across them.  db from the staged dz.  One partial a slab in dW's
// layout; tn_red_wgrad finishes.
struct GCFM {
    const float* x;
    const float* dz;
    float* ws;
    float* dbws;
    int C, K, Cg, Kg, KT, H, Wd, Ho, Wo, f, stride, pad, NCOL;
    unsigned HoWo, ntiles, nslab;
    unsigned long long npix;
};

__global__ __launch_bounds__(256) void gcf_wgrad_mfma_kernel(GCFM g) {
    __shared__ float sd[16][64];
    __shared__ int spix[3][64];                  // image, source row / column of tap offset 0; row -(1 << 20): no pixel
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, q = lane >> 4, slab = blockIdx.x;
    const int grp = blockIdx.z / g.KT, k0 = (blockIdx.z - grp * g.KT) * 16, T = g.f * g.f;
    const size_t HW = (size_t)g.H * g.Wd;
    long long xoff[8];
    int dy[8], dx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int colj = ((int)blockIdx.y * 32 + (int)wave + 4 * j) * 16 + (int)(lane & 15u);
        const int c = colj / T, tap = colj - c * T, u = tap / g.f, v = tap - u * g.f;
        const bool valid = colj < g.NCOL;
        dy[j] = valid ? g.f - 1 - u - g.pad : 1 << 20;
        dx[j] = g.f - 1 - v - g.pad;
        xoff[j] = valid ? (long long)((size_t)grp * g.Cg + c) * (long long)HW : 0;
    }
    gcf_f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = gcf_f32x4{0.f, 0.f, 0.f, 0.f};
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
            spix[1][lane] = valid ? oh * g.stride : -(1 << 20);
            spix[2][lane] = ow * g.stride;
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int kl = k0 + (int)wave + 4 * jj;
            const float d = (valid && kl < g.Kg) ? g.dz[((size_t)n * g.K + (size_t)grp * g.Kg + kl) * g.HoWo + qq] : 0.f;
            sd[wave + 4 * jj][lane] = d;
            dbs[jj] += d;
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
            if (kl < g.Kg) ws[((size_t)grp * g.Kg + kl) * g.NCOL + colj] = acc[j][e];
        }
    }
    if (blockIdx.y == 0) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            float s = dbs[jj];
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
            const int kl = k0 + (int)wave + 4 * jj;
            if (lane == 0 && kl < g.Kg) g.dbws[(size_t)slab * g.K + grp * g.Kg + kl] = s;
        }
    }
}

static bool gcf_ok(int N, int C, int H, int Wd, int K, int g, int f, int stride, int pad, int Ho, int Wo) {
    if (N < 1 || !gc_groups_ok(C, K, g) || K > 65535 || C > 65535 || f > 64 || H > 65535 || Wd > 65535) return false;
    if (!gc_axis_ok(H, f, stride, pad, Ho) || !gc_axis_ok(Wd, f, stride, pad, Wo)) return false;
    if ((long long)N * C * H * Wd >= (1ll << 32) || (long long)N * K * Ho * Wo >= (1ll << 32)) return false;
    return (long long)K * (C / g) * f * f < (1ll << 28);
}

#define GCF_ARGS_FMT "(N %d, %d maps of %d x %d -> %d maps of %d x %d, %d groups, filter %d stride %d pad_lo %d)"
#define GCF_ARGS N, C, H, Wd, K, Ho, Wo, g, f, stride, pad

static int gcf_lg(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// q arrives with the tensors, the maps and the planes of the product filled in
// The matrix-core form of a product: 0 where it does not apply (narrow groups, a source tile that outgrows LDS)
static int gcf_run_mfma(tn_ctx* ctx, GCF& q, int mode, int N, int groups, int Kg, int Cg, bool* done) {
    *done = false;
    q.RC = q.f * q.f * q.Rg;
    if (Kg < 16 || Cg < 4 || q.RC > GCF_ITEMS_MAX || q.f > 255) return TN_OK;
    q.R4 = (q.RC + 3) / 4; q.MT = (q.Og + 15) / 16;
    q.tabbytes = (4u * q.R4 * (unsigned)sizeof(int2) + 15u) & ~15u;
    q.lgTW = q.Wo <= 4 ? 2 : (q.Wo <= 8 ? 3 : 4);
    const int TW = 1 << q.lgTW, RU = 16 >> q.lgTW;
    q.npr = 4;
    while (q.npr > 1 && 4 * (q.npr / 2) * RU >= q.Ho) q.npr /= 2;
    q.IW = gc_src_dim(mode, TW, q.f, q.stride);
    q.IWp = q.IW | 1;
    size_t lds;
    for (;;) {
        q.TH = 4 * q.npr * RU;
        q.IH = gc_src_dim(mode, q.TH, q.f, q.stride);
        lds = q.tabbytes + (size_t)q.Rg * q.IH * q.IWp * sizeof(float);
        if (lds <= GC_LDS_MAX) break;
        if (q.npr == 1) return TN_OK;
        q.npr /= 2;
    }
    q.tilesX = (q.Wo + TW - 1) / TW;
    q.tiles = q.tilesX * ((q.Ho + q.TH - 1) / q.TH);
    const size_t total = (size_t)groups * q.MT * q.R4 * 64;
    const unsigned long long blocks = (unsigned long long)N * q.tiles;
    TN_REQUIRE(total < (1ull << 31) && blocks < (1ull << 31) && groups <= 65535, "gconv: %d images of %d tiles, %d groups: too large",
               N, q.tiles, groups);
    float* wt;
    int rc = tn_scratch_get(ctx, total * sizeof(float), &wt);
    if (rc) return rc;
    gcf_wt_kernel<<<cdiv((long long)total, 256), 256, 0, ctx->stream>>>(q.W, wt, Kg, Cg, q.f * q.f, q.Rg, q.R4, q.MT, mode != 0,
                                                                       (unsigned)total);
    TN_LAUNCH_CHECK();
    q.wt = wt;
    const dim3 grid((unsigned)blocks, (unsigned)groups);
    rc = mode == 0 ? tn_launch_lds<gcf_mfma_kernel<0>>(ctx, grid, dim3(256), lds, q)
       : mode == 1 ? tn_launch_lds<gcf_mfma_kernel<1>>(ctx, grid, dim3(256), lds, q)
                   : tn_launch_lds<gcf_mfma_kernel<2>>(ctx, grid, dim3(256), lds, q);
    if (rc) return rc;
    TN_LAUNCH_CHECK();
    *done = true;
    return TN_OK;
}

static int gcf_run(tn_ctx* ctx, GCF& q, int mode, int N, int groups) {
    bool done;
    int rc = gcf_run_mfma(ctx, q, mode, N, groups, mode == 0 ? q.Og : q.Rg, mode == 0 ? q.Rg : q.Og, &done);
    if (rc || done) return rc;
    q.OCH = (q.Og + GCF_KT - 1) / GCF_KT;
    q.lgTW = gcf_lg(q.Wo < 16 ? q.Wo : 16);
    q.lgTH = gcf_lg(q.Ho < 16 ? q.Ho : 16);
    if (q.lgTH > 8 - q.lgTW) q.lgTH = 8 - q.lgTW;
    for (;;) {
        q.IH = gc_src_dim(mode, 1 << q.lgTH, q.f, q.stride);
        q.IW = gc_src_dim(mode, 1 << q.lgTW, q.f, q.stride);
        q.IWp = q.IW | 1;
        if ((size_t)q.IH * q.IWp * sizeof(float) <= GC_LDS_MAX) break;
        if (q.lgTH >= q.lgTW && q.lgTH > 0) --q.lgTH;           // (f <= 64: a one-pixel tile fits)
        else --q.lgTW;
    }
    const size_t plane = (size_t)q.IH * q.IWp * sizeof(float);
    q.RCH = (int)(GC_LDS_MAX / plane);
    if (q.RCH > q.Rg) q.RCH = q.Rg;
    q.tilesX = (q.Wo + (1 << q.lgTW) - 1) >> q.lgTW;
    q.tiles = q.tilesX * ((q.Ho + (1 << q.lgTH) - 1) >> q.lgTH);
    const unsigned long long blocks = (unsigned long long)N * q.tiles, gy = (unsigned long long)groups * q.OCH;
    TN_REQUIRE(blocks < (1ull << 31) && gy <= 65535, "gconv: %d images of %d tiles, %d groups: too large", N, q.tiles, groups);
    const dim3 grid((unsigned)blocks, (unsigned)gy);
    const size_t lds = (size_t)q.RCH * plane;
    rc = mode == 0 ? tn_launch_lds<gcf_kernel<0>>(ctx, grid, dim3(256), lds, q)
       : mode == 1 ? tn_launch_lds<gcf_kernel<1>>(ctx, grid, dim3(256), lds, q)
                   : tn_launch_lds<gcf_kernel<2>>(ctx, grid, dim3(256), lds, q);
    if (rc) return rc;
    TN_LAUNCH_CHECK();
    return TN_OK;
}

extern "C" {

int tn_gconv_supported(int N, int C, int H, int Wd, int K, int g, int f, int stride, int pad, int Ho, int Wo) {
    return gcf_ok(N, C, H, Wd, K, g, f, stride, pad, Ho, Wo) ? 1 : 0;
}

int tn_gconv_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int N, int C, int H, int Wd, int K, int g,
                 int f, int stride, int pad, int Ho, int Wo, int act, float prm) {
    TN_REQUIRE(x && W && b && a && gcf_ok(N, C, H, Wd, K, g, f, stride, pad, Ho, Wo), "tn_gconv_fwd: bad arguments " GCF_ARGS_FMT,
               GCF_ARGS);
    TN_FP32_ONLY(ctx, "tn_gconv_fwd");
    GCF q{};
    q.src = x; q.W = W; q.out = a; q.bias = b; q.act = act; q.prm = prm;
    q.R = C; q.O = K; q.Rg = C / g; q.Og = K / g;
    q.Hs = H; q.Ws = Wd; q.Ho = Ho; q.Wo = Wo;
    q.wso = q.Rg * f * f; q.wsr = f * f; q.KgCgT = q.Og * q.Rg * f * f;
    q.f = f; q.stride = stride; q.off0 = -pad;
    return gcf_run(ctx, q, 0, N, g);
}

int tn_gconv_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int N, int C, int H, int Wd, int K, int g, int f,
                   int stride, int pad, int Ho, int Wo, const float* prev_a, int prev_act, float prev_prm) {
    TN_REQUIRE(dz && W && dx && gcf_ok(N, C, H, Wd, K, g, f, stride, pad, Ho, Wo), "tn_gconv_dgrad: bad arguments " GCF_ARGS_FMT,
               GCF_ARGS);
    TN_FP32_ONLY(ctx, "tn_gconv_dgrad");
    GCF q{};
    q.src = dz; q.W = W; q.out = dx; q.prev_a = prev_a; q.act = prev_act; q.prm = prev_prm;
    q.R = K; q.O = C; q.Rg = K / g; q.Og = C / g;
    q.Hs = Ho; q.Ws = Wo; q.Ho = H; q.Wo = Wd;
    q.wso = f * f; q.wsr = q.Og * f * f; q.KgCgT = q.Og * q.Rg * f * f;
    q.f = f; q.stride = stride; q.off0 = pad - (f - 1);
    return gcf_run(ctx, q, stride == 1 ? 1 : 2, N, g);
}

int tn_gconv_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int N, int C, int H, int Wd, int K, int g,
                   int f, int stride, int pad, int Ho, int Wo) {
    TN_REQUIRE(x && dz && dW && db && gcf_ok(N, C, H, Wd, K, g, f, stride, pad, Ho, Wo),
               "tn_gconv_wgrad: bad arguments " GCF_ARGS_FMT, GCF_ARGS);
    TN_FP32_ONLY(ctx, "tn_gconv_wgrad");
    if (K / g >= 16 && C / g >= 4) {
        GCFM m{};
        m.x = x; m.dz = dz; m.C = C; m.K = K; m.Cg = C / g; m.Kg = K / g; m.KT = (m.Kg + 15) / 16;
        m.H = H; m.Wd = Wd; m.Ho = Ho; m.Wo = Wo; m.f = f; m.stride = stride; m.pad = pad; m.NCOL = m.Cg * f * f;
        m.HoWo = (unsigned)Ho * Wo;
        m.npix = (unsigned long long)N * m.HoWo;
        const int CH = cdiv(cdiv(m.NCOL, 16), 32);
        const long long nt = (long long)((m.npix + 63) / 64), gz = (long long)g * m.KT;
        TN_REQUIRE(CH <= 65535 && gz <= 65535, "tn_gconv_wgrad: %d x %d x %d x %d weights: too large", K, C / g, f, f);
        m.ntiles = (unsigned)nt; m.nslab = gc_slabs(nt, (long long)CH * gz, 1024);
        const size_t n = (size_t)K * m.NCOL;
        int rc = tn_scratch_get(ctx, (size_t)m.nslab * (n + K) * sizeof(float), &m.ws);
        if (rc) return rc;
        m.dbws = m.ws + (size_t)m.nslab * n;
        gcf_wgrad_mfma_kernel<<<dim3(m.nslab, (unsigned)CH, (unsigned)gz), 256, 0, ctx->stream>>>(m);
        TN_LAUNCH_CHECK();
        return tn_red_wgrad(ctx, m.ws, dW, (uint32_t)n, m.nslab, (uint32_t)n, m.dbws, db, (uint32_t)K, m.nslab, (uint32_t)K);
    }
    GCFW q{};
    q.x = x; q.dz = dz; q.C = C; q.K = K; q.Cg = C / g; q.Kg = K / g;
    q.H = H; q.Wd = Wd; q.Ho = Ho; q.Wo = Wo; q.f = f; q.stride = stride; q.pad = pad;
    q.HoWo = (unsigned)Ho * Wo;
    q.npix = (unsigned long long)N * q.HoWo;
    const int CCH = (q.Cg + 7) / 8;
    const long long nt = (long long)((q.npix + 255) / 256);
    q.ntiles = (unsigned)nt; q.nslab = gc_slabs(nt, (long long)K * CCH, 1024);
    const size_t n = (size_t)K * q.Cg * f * f;
    int rc = tn_scratch_get(ctx, (size_t)q.nslab * (n + K) * sizeof(float), &q.ws);
    if (rc) return rc;
    q.dbws = q.ws + (size_t)q.nslab * n;
    gcf_wgrad_kernel<<<dim3(q.nslab, (unsigned)K, (unsigned)CCH), 256, 0, ctx->stream>>>(q);
    TN_LAUNCH_CHECK();
    return tn_red_wgrad(ctx, q.ws, dW, (uint32_t)n, q.nslab, (uint32_t)n, q.dbws, db, (uint32_t)K, q.nslab, (uint32_t)K);
}

}  // extern "C"
