// DTYPE 'float16' / 'bfloat16': ConvLayer(..., groups=g) with NARROW groups on the c8 tensors of the conv stack -- C/g == K/g
// == w, w 2 or 4, so C == K, a multiple of 8 (gconv.h: gc_narrow).  The narrow branch of tn_c8_gconv_fwd / _dgrad / _wgrad
// (gconv_c8.hip): layouts, arithmetic and filter orientation are that family's.  An output cell of 8 filters reads the
// input cell with the same index alone: the layer is cell-diagonal, per tap and cell an 8x8 matrix of two 4x4 blocks (w 4:
// a block is a group; w 2: two 2x2 groups on a block's diagonal, zeros off it).
//
// Forward / input gradient (gn_kernel; gconv.h for the modes): grid (images x tiles of the stored output plane, runs of up
// to 8 cells), 256 lanes.
//   product  v_mfma_f32_4x4x4_16b: sixteen independent 4x4x4 products an issue.  Matrix block b = lane / 4 is half-cell b % 2
//            of ONE cell at the pixel quad b / 2 of a unit of 32 pixels: the B operand of lane 8 q + 4 h + j is the 8-byte
//            half-cell h of pixel 4 q + j as it is stored -- one ds_read_b64, a wave reads 512 contiguous bytes of the staged
//            tile at the tap's offset --, the A operand row j of the tap's 4x4 weight block of half-cell h (the same eight
//            rows in every quad), the four fp32 accumulators the half-cell's four outputs at the lane's pixel.  No product
//            lands on the zeros between groups of 4; groups of 2 spend half of a block on them.
//   source   the run's cells of the tile's source rows and columns, halo included, staged once in LDS ([cell][IH][IW]
//            cells, 16-byte loads, +0 outside the map), and a table of the taps' LDS offsets beside it.
//   weights  arranged as A operands once per call (gn_wt_kernel, context scratch): wt[cell][tap][half][row][4], 64 bytes a
//            (cell, tap); a wave loads a tap's operand once and keeps it for the products of all its units.
//   tile     TW = 32 columns (16 / 8 on narrow planes: a unit is then 2 / 4 rows); the four waves are split over the run's
//            cells (WC of them side by side) and over units of rows (WU = 4 / WC), up to 8 units a wave; units, then the
//            run, halve until the plane is not overshot and the source tile fits GC_LDS_MAX.  A geometry whose smallest
//            tile does not fit is refused (tn_c8_gconv_supported).
//   store    a lane holds half a cell of its pixel: one 8-byte store, a wave 512 contiguous bytes.  Every cell of the output
//            is written: pad cells and pixels no window touches as +0.
// Weight gradient (gn_wgrad_kernel): fp32 accumulators on plain FMAs.  grid (slabs, cells, chunks of 3 taps); a wave owns
//   tiles of 64 pixels, a lane one pixel of each: it loads its pixel's dz cell and the x cell under each of the chunk's taps
//   (16-byte loads, the next tile's under the FMAs) and adds the 4x4 (w 2: the two 2x2) products of both half-cells to its
//   own accumulators.  Then lanes (butterfly), waves (0 + 1 + 2 + 3) and slabs (tn_red_wgrad) in fixed order: no atomics,
//   the same bits every run; the off-diagonal quarters of a w 2 block are neither computed nor stored.  db from the same dz.
// Index range: fewer than 2^32 cells a tensor, f <= 255, fewer than 2^31 blocks a launch.
#include "c8_elem.h"
#include "gconv.h"

typedef float gn_f32x4 __attribute__((ext_vector_type(4)));

template <typename E>
__device__ __forceinline__ gn_f32x4 gn_mfma(typename E::v4 a, typename E::v4 b, gn_f32x4 c) {
    if constexpr (E::BF) return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_4x4x4f16(a, b, c, 0, 0, 0);
}

// wt[((cell T + tap) 8 + 4 half + row) 4 + e] = W(output 8 cell + 4 half + row, reduced map 8 cell + 4 half + e, tap), rounded;
// 0 where the two lie in different groups (w 2).  Forward: output = filter, reduced = channel; dgrad: swapped.
template <typename E>
__global__ __launch_bounds__(256) void gn_wt_kernel(const float* __restrict__ W, typename E::T* __restrict__ wt, int w, int T,
                                                   int dgrad, unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int e = idx & 3u, row = (idx >> 2) & 3u;
    const unsigned hc = ((idx >> 5) / (unsigned)T) * 2u + ((idx >> 4) & 1u), tap = (idx >> 5) % (unsigned)T;
    const unsigned o = 4 * hc + row, r = 4 * hc + e, k = dgrad ? r : o, c = dgrad ? o : r;
    wt[idx] = (typename E::T)(o / w == r / w ? W[((size_t)k * w + c % w) * T + tap] : 0.f);
}

struct GN {
    const uint4* src;        // the B operand's tensor: x (forward), dz (input gradient)
    const uint2* wt;
    uint2* out;
    const float* bias;       // forward
    const uint2* prev_a;     // input gradient: stored output of the layer below (NULL: none)
    int Ss, Ps;              // source maps: side, pitch
    unsigned PPs;
    int So, Po;              // output maps of this product: side, pitch
    unsigned PPo;
    unsigned C8, T;          // cells of either tensor, taps
    int f, stride, off0;
    int NC, WC, lgTW, upw, TH, IH, IW, tilesX, tiles;      // cells a run, waves side by side on cells, units a wave
    unsigned tabbytes;
    int act;
    float prm;
};

template <typename E, int MODE>
__global__ __launch_bounds__(256) void gn_kernel(GN g) {
    typedef typename E::v4 v4;
    extern __shared__ __attribute__((aligned(16))) char gn_smem[];
    int2* const tab = reinterpret_cast<int2*>(gn_smem);       // [T] x: LDS offset of the tap, y: (du, dv)
    uint4* const tile = reinterpret_cast<uint4*>(gn_smem + g.tabbytes);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = (lane >> 2) & 1, px = 4 * (lane >> 3) + (lane & 3);
    const unsigned n = blockIdx.x / (unsigned)g.tiles, tl = blockIdx.x - n * (unsigned)g.tiles, cell0 = blockIdx.y * (unsigned)g.NC;
    const int nc = (int)(g.C8 - cell0 < (unsigned)g.NC ? g.C8 - cell0 : (unsigned)g.NC);
    const int ty = (int)tl / g.tilesX, tx = (int)tl - ty * g.tilesX;
    const int TW = 1 << g.lgTW, s = g.stride, se = MODE == 0 ? s : 1, f = g.f;
    const int y0 = ty * g.TH, x0 = tx * TW;
    const int sy0 = gc_src0(MODE, y0, g.off0, s), sx0 = gc_src0(MODE, x0, g.off0, s);
    const int per = g.IH * g.IW;

    for (int i = t; i < (int)g.T; i += 256) {
        const int u = i / f, v = i - u * f;
        const int du = MODE == 0 ? f - 1 - u : u, dv = MODE == 0 ? f - 1 - v : v;
        tab[i] = make_int2(du * g.IW + dv, (du << 8) | dv);
    }
    for (int i = t; i < nc * per; i += 256) {
        const int c = i / per, rem = i - c * per, r = rem / g.IW, cc = rem - r * g.IW;
        const int gy = sy0 + r, gx = sx0 + cc;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (gy >= 0 && gy < g.Ss && gx >= 0 && gx < g.Ss)
            v = g.src[((size_t)n * g.C8 + cell0 + c) * g.PPs + (unsigned)gy * g.Ps + (unsigned)gx];
        tile[i] = v;
    }
    __syncthreads();

    // this lane's pixel of unit i: unit uw upw + i of the tile, 32 >> lgTW rows of TW columns
    const int cw = wave % g.WC, uw = wave / g.WC;
    const int col = px & (TW - 1), rsub = px >> g.lgTW, ox = x0 + col;
    int oy[8], base[8];
    bool live[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int rl = ((uw * g.upw + i) << (5 - g.lgTW)) + rsub;
        oy[i] = y0 + rl;
        base[i] = rl * se * g.IW + col * se;
        live[i] = i < g.upw && oy[i] < g.So && ox < g.So;
    }
    const bool lk = g.act == TN_ACT_LEAKY;
    const float prm = g.prm, tie = prm > 0.f ? 1.f + prm : 0.f;

    for (int c = cw; c < nc; c += g.WC) {
        const uint2* const cells = reinterpret_cast<const uint2*>(tile + c * per);
        auto operand = [&](int i, int2 e) __attribute__((always_inline)) {
            // modes 0 and 1: no test -- a pixel past the map reads cells of the staged tile too, and its sums are not stored
            if (MODE != 2) return __builtin_bit_cast(v4, cells[2 * (base[i] + e.x) + half]);
            uint2 val = make_uint2(0u, 0u);
            if (live[i]) {
                const int sy = oy[i] + g.off0 + ((e.y >> 8) & 255), sx = ox + g.off0 + (e.y & 255);
                const int qy = sy / s, qx = sx / s;
                if (sy >= 0 && sx >= 0 && qy * s == sy && qx * s == sx) val = cells[2 * ((qy - sy0) * g.IW + (qx - sx0)) + half];
            }
            return __builtin_bit_cast(v4, val);
        };
        gn_f32x4 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][r] = 0.f;
        const uint2* const wp = g.wt + (size_t)(cell0 + c) * g.T * 8 + (lane & 7);
        uint2 anext = wp[0];
        for (unsigned tap = 0; tap < g.T; ++tap) {
            const v4 a = __builtin_bit_cast(v4, anext);
            if (tap + 1 < g.T) anext = wp[(size_t)(tap + 1) * 8];     // the next tap's weights travel under the products
            const int2 e = tab[tap];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (i < g.upw) acc[i] = gn_mfma<E>(a, operand(i, e), acc[i]);
        }
        // accumulators 0 .. 3: outputs 4 half .. 4 half + 3 of the cell at this lane's pixel -- half a cell
        float bv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = MODE == 0 ? g.bias[8 * (cell0 + c) + 4 * half + e] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i >= g.upw || oy[i] >= g.Po || ox >= g.Po) continue;
            const size_t at = (((size_t)n * g.C8 + cell0 + c) * g.PPo + (unsigned)oy[i] * g.Po + (unsigned)ox) * 2 + half;
            const bool deriv = MODE >= 1 && g.prev_a != nullptr && live[i];
            v4 pa = __builtin_bit_cast(v4, make_uint2(0u, 0u));
            if (deriv) pa = __builtin_bit_cast(v4, g.prev_a[at]);
            v4 c4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float z = acc[i][e];
                if (MODE == 0) {
                    z += bv[e];
                    z = lk ? fmaxf(0.f, z) + fminf(0.f, z) * prm : tn_act_fwd(z, g.act, prm);
                } else if (deriv) {
                    const float a_ = (float)pa[e];
                    z *= lk ? (a_ > 0.f ? 1.f : (a_ < 0.f ? prm : tie)) : tn_act_grad_from_out(a_, g.act, prm);
                }
                c4[e] = (typename E::T)(live[i] ? z : 0.f);
            }
            g.out[at] = __builtin_bit_cast(uint2, c4);
        }
    }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------
#define GN_TAPS 3            // taps a block (grid z: chunks of them)

struct GNW {
    const uint4* x;
    const uint4* dz;
    float* ws;               // [slab][K][w][f][f] partial dW (scale removed)
    float* dbws;             // [slab][K]
    unsigned S, P, PP, So, SoSo, Po, PPo, C8, K, T, ntiles, nslab;
    int f, stride, pad;
    unsigned long long npix;           // N So So
    float oscale;
};

// WD: maps a group (2, 4).  acc[tap][half][row][m]: filter 4 half + row of the cell on channel 4 half + m (WD 2: + 2 (row / 2))
template <typename E, int WD>
__global__ __launch_bounds__(256) void gn_wgrad_kernel(GNW g) {
    typedef typename E::v8 v8;
    constexpr int NA = GN_TAPS * 8 * WD;
    __shared__ float red[4][NA + 8];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned slab = blockIdx.x, cell = blockIdx.y, tap0 = GN_TAPS * blockIdx.z;
    const bool bias = blockIdx.z == 0;
    int dy[GN_TAPS], dx[GN_TAPS];
    bool tlive[GN_TAPS];
#pragma unroll
    for (int k = 0; k < GN_TAPS; ++k) {
        const unsigned tap = tap0 + k;
        tlive[k] = tap < g.T;
        dy[k] = g.f - 1 - (int)(tap / (unsigned)g.f) - g.pad;
        dx[k] = g.f - 1 - (int)(tap % (unsigned)g.f) - g.pad;
    }
    float acc[GN_TAPS][2][4][WD], dbs[8];
#pragma unroll
    for (int k = 0; k < GN_TAPS; ++k)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int m = 0; m < WD; ++m) acc[k][h][i][m] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) dbs[e] = 0.f;

    uint4 xr[GN_TAPS], dr;
    auto gload = [&](unsigned tile) __attribute__((always_inline)) {
        const unsigned long long gi = (unsigned long long)tile * 64 + lane;
        const bool valid = gi < g.npix;
        const unsigned g_ = valid ? (unsigned)gi : 0u;
        const unsigned n = g_ / g.SoSo, q = g_ - n * g.SoSo;
        const unsigned oh = q / g.So, ow = q - oh * g.So;
        dr = make_uint4(0u, 0u, 0u, 0u);
        if (valid) dr = g.dz[((size_t)n * g.C8 + cell) * g.PPo + oh * g.Po + ow];
#pragma unroll
        for (int k = 0; k < GN_TAPS; ++k) {
            xr[k] = make_uint4(0u, 0u, 0u, 0u);
            const int sy = (int)oh * g.stride + dy[k], sx = (int)ow * g.stride + dx[k];
            if (valid && tlive[k] && sy >= 0 && sx >= 0 && sy < (int)g.S && sx < (int)g.S)
                xr[k] = g.x[((size_t)n * g.C8 + cell) * g.PP + (unsigned)sy * g.P + (unsigned)sx];
        }
    };

    // a wave's tiles: 4 slab + wave, then every 4 nslab-th
    unsigned tile = 4 * slab + wave;
    if (tile < g.ntiles) gload(tile);
    for (; tile < g.ntiles; tile += 4 * g.nslab) {
        const v8 d8 = __builtin_bit_cast(v8, dr);
        v8 x8[GN_TAPS];
#pragma unroll
        for (int k = 0; k < GN_TAPS; ++k) x8[k] = __builtin_bit_cast(v8, xr[k]);
        if (tile + 4 * g.nslab < g.ntiles) gload(tile + 4 * g.nslab);       // the next tile's cells travel under the FMAs
        float d[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            d[e] = (float)d8[e];
            dbs[e] += d[e];
        }
#pragma unroll
        for (int k = 0; k < GN_TAPS; ++k) {
            float xv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[e] = (float)x8[k][e];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int m = 0; m < WD; ++m)
                        acc[k][h][i][m] = fmaf(d[4 * h + i], xv[4 * h + (WD == 2 ? 2 * (i >> 1) : 0) + m], acc[k][h][i][m]);
        }
    }

    // lanes by butterfly (every lane ends with the wave's sum), then the four waves' sums in the order 0 + 1 + 2 + 3
    float* const mine = red[wave];
#pragma unroll
    for (int k = 0; k < GN_TAPS; ++k)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int m = 0; m < WD; ++m) {
                    float s = acc[k][h][i][m];
#pragma unroll
                    for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh);
                    if (lane == 0) mine[((k * 2 + h) * 4 + i) * WD + m] = s;
                }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float s = dbs[e];
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh);
        if (lane == 0) mine[NA + e] = s;
    }
    __syncthreads();
    if (t < (unsigned)NA + 8u) {
        const float s = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        if (t < (unsigned)NA) {
            const unsigned m = t % WD, row = (t / WD) & 7u, tap = tap0 + t / (8 * WD);     // row: 4 half + i, the filter of the cell
            if (tap < g.T) g.ws[(size_t)slab * g.K * WD * g.T + ((size_t)(8 * cell + row) * WD + m) * g.T + tap] = s * g.oscale;
        } else if (bias) {
            g.dbws[(size_t)slab * g.K + 8 * cell + (t - NA)] = s * g.oscale;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The tile of a product: false if the smallest one does not fit GC_LDS_MAX
static bool gn_tile(GN& g, int mode) {
    const int C8 = (int)g.C8;
    g.lgTW = g.Po <= 8 ? 3 : (g.Po <= 16 ? 4 : 5);
    const int TW = 1 << g.lgTW, RU = 32 >> g.lgTW;
    g.tabbytes = (g.T * (unsigned)sizeof(int2) + 15u) & ~15u;
    g.IW = gc_src_dim(mode, TW, g.f, g.stride);
    g.NC = C8 < 8 ? C8 : 8;
    g.upw = 8;
    for (;;) {
        g.WC = g.NC >= 4 ? 4 : (g.NC >= 2 ? 2 : 1);
        const int WU = 4 / g.WC;
        while (g.upw > 1 && WU * (g.upw / 2) * RU >= g.Po) g.upw /= 2;
        g.TH = WU * g.upw * RU;
        g.IH = gc_src_dim(mode, g.TH, g.f, g.stride);
        if (g.tabbytes + (size_t)g.NC * g.IH * g.IW * 16 <= GC_LDS_MAX) break;
        if (g.upw > 1) g.upw /= 2;
        else if (g.NC > 1) g.NC = (g.NC + 1) / 2;
        else return false;
    }
    g.tilesX = (g.Po + TW - 1) / TW;
    g.tiles = g.tilesX * ((g.Po + g.TH - 1) / g.TH);
    return true;
}

static void gn_fwd_args(GN& q, int C, int S, int P, int f, int stride, int pad, int So, int Po) {
    q.C8 = (unsigned)(C / 8); q.T = (unsigned)(f * f);
    q.Ss = S; q.Ps = P; q.PPs = (unsigned)P * P;
    q.So = So; q.Po = Po; q.PPo = (unsigned)Po * Po;
    q.f = f; q.stride = stride; q.off0 = -pad;
}

static void gn_dgrad_args(GN& q, int C, int S, int P, int f, int stride, int pad, int So, int Po) {
    q.C8 = (unsigned)(C / 8); q.T = (unsigned)(f * f);
    q.Ss = So; q.Ps = Po; q.PPs = (unsigned)Po * Po;
    q.So = S; q.Po = P; q.PPo = (unsigned)P * P;
    q.f = f; q.stride = stride; q.off0 = pad - (f - 1);
}

#ifndef C8_BF16_TU
// what the narrow kernels ask beyond the family's rule (gconv_c8.hip, gc8_ok): the smallest tile of either product fits
bool gc8n_ok(int C, int S, int P, int f, int stride, int pad, int So, int Po) {
    GN a{}, b{};
    gn_fwd_args(a, C, S, P, f, stride, pad, So, Po);
    gn_dgrad_args(b, C, S, P, f, stride, pad, So, Po);
    return gn_tile(a, 0) && gn_tile(b, stride == 1 ? 1 : 2);
}
#endif

template <typename E, int MODE>
static int gn_run(tn_ctx* ctx, GN& g, const float* W, int N, int C, int w) {
    TN_REQUIRE(gn_tile(g, MODE), "c8 gconv (narrow groups): the source tile of a %d x %d filter does not fit", g.f, g.f);
    const size_t total = (size_t)g.C8 * g.T * 32;
    const unsigned long long blocks = (unsigned long long)N * g.tiles;
    const int runs = cdiv(g.C8, g.NC);
    TN_REQUIRE(total < (1ull << 31) && blocks < (1ull << 31) && runs <= 65535,
               "c8 gconv (narrow groups): %d maps, %d x %d filters, %d images: too large", C, g.f, g.f, N);
    float* wt;
    int rc = tn_scratch_get(ctx, total * sizeof(typename E::T), &wt);
    if (rc) return rc;
    gn_wt_kernel<E><<<cdiv((long long)total, 256), 256, 0, ctx->stream>>>(W, reinterpret_cast<typename E::T*>(wt), w, (int)g.T,
                                                                        MODE >= 1 ? 1 : 0, (unsigned)total);
    TN_LAUNCH_CHECK();
    g.wt = reinterpret_cast<const uint2*>(wt);
    const size_t lds = g.tabbytes + (size_t)g.NC * g.IH * g.IW * 16;
    rc = tn_launch_lds<gn_kernel<E, MODE>>(ctx, dim3((unsigned)blocks, (unsigned)runs), dim3(256), lds, g);
    if (rc) return rc;
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// The narrow branches of tn_c8_gconv_* (gconv_c8.hip), which has checked the arguments (gc8_ok)
int C8_API(gc8n_fwd)(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P, int g, int f,
                     int stride, int pad, int So, int Po, int act, float prm) {
    GN q{};
    q.src = static_cast<const uint4*>(x); q.out = static_cast<uint2*>(y); q.bias = b; q.act = act; q.prm = prm;
    gn_fwd_args(q, C, S, P, f, stride, pad, So, Po);
    return gn_run<C8E, 0>(ctx, q, W, N, C, C / g);
}

int C8_API(gc8n_dgrad)(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int g, int f, int stride,
                       int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm) {
    GN q{};
    q.src = static_cast<const uint4*>(dz); q.out = static_cast<uint2*>(dx); q.prev_a = static_cast<const uint2*>(prev_a);
    q.act = prev_act; q.prm = prev_prm;
    gn_dgrad_args(q, C, S, P, f, stride, pad, So, Po);
    return stride == 1 ? gn_run<C8E, 1>(ctx, q, W, N, C, C / g) : gn_run<C8E, 2>(ctx, q, W, N, C, C / g);
}

int C8_API(gc8n_wgrad)(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P, int g, int f,
                       int stride, int pad, int So, int Po) {
    const int w = C / g;
    GNW q{};
    q.x = static_cast<const uint4*>(x); q.dz = static_cast<const uint4*>(dz);
    q.S = (unsigned)S; q.P = (unsigned)P; q.PP = (unsigned)P * P;
    q.So = (unsigned)So; q.SoSo = (unsigned)So * So; q.Po = (unsigned)Po; q.PPo = (unsigned)Po * Po;
    q.C8 = (unsigned)(C / 8); q.K = (unsigned)C; q.T = (unsigned)(f * f);
    q.f = f; q.stride = stride; q.pad = pad;
    q.npix = (unsigned long long)N * q.SoSo;
    const int chunks = cdiv(q.T, GN_TAPS);
    const long long nt = (long long)((q.npix + 63) / 64), nt4 = (nt + 3) / 4;       // a block takes four tiles a round
    TN_REQUIRE(q.C8 <= 65535 && chunks <= 65535, "tn_c8_gconv_wgrad: %d x %d x %d x %d weights: too large", C, w, f, f);
    q.ntiles = (unsigned)nt; q.nslab = gc_slabs(nt4, (long long)q.C8 * chunks, 512);
    const size_t n = (size_t)C * w * q.T;
    int rc = tn_scratch_get(ctx, ((size_t)q.nslab * n + (size_t)q.nslab * C) * sizeof(float), &q.ws);
    if (rc) return rc;
    q.dbws = q.ws + (size_t)q.nslab * n;
    q.oscale = 1.f / ctx->grad_scale;
    const dim3 grid(q.nslab, q.C8, (unsigned)chunks);
    if (w == 4) gn_wgrad_kernel<C8E, 4><<<grid, 256, 0, ctx->stream>>>(q);
    else gn_wgrad_kernel<C8E, 2><<<grid, 256, 0, ctx->stream>>>(q);
    TN_LAUNCH_CHECK();
    return tn_red_wgrad(ctx, q.ws, dW, (uint32_t)n, q.nslab, (uint32_t)n, q.dbws, db, (uint32_t)C, q.nslab, (uint32_t)C);
}
