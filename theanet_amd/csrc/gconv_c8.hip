// DTYPE 'float16' / 'bfloat16': ConvLayer(..., groups=g) on the 16-bit-resident c8 tensors of the conv stack
// ([N][C/8][P][P][8] 16-bit values; x / dx: S x S maps at pitch P, y / dz: So x So maps at pitch Po): tn_c8_gconv_fwd / _dgrad /
// _wgrad.  C/g and K/g are multiples of 8: a group is a whole number of 16-byte cells -- or C/g == K/g == 2 or 4 with C a
// multiple of 8: the launchers' narrow branch, gconv_c8_narrow.hip.  Arithmetic: the stack's (convg_c8.hip)
// -- x and dz as stored, W rounded to the element type while it is arranged, exact products, fp32 accumulation on the matrix
// core, bias / activation on the fp32 sums, one rounding on store; the weight gradient's fp32 epilogue removes the gradient
// scale.  Filter orientation: tn_conv2d_*'s.
//
// Forward / input gradient (gc8_kernel, gconv.h for the modes and the tile): grid (images x tiles of the stored output
// plane, groups), 256 lanes.
//   product  v_mfma_f32_16x16x32: the 16 rows are 16 outputs of ONE group (filters forward, channels input gradient), the
//            16 columns 16 pixels of the tile, the 32-deep reduction FOUR reduction cells rc = tap * R8g + octet, one a
//            quarter wave: lane l holds pixel l % 16 of cell 4 step + l / 16 -- a 16-byte cell as it is stored is a lane's
//            B operand.  A group of 8 or 16 outputs fills one tile, 24 a full and a half one (rows past the group are
//            zero weights and are not stored): never a 32-row tile of which three quarters are zeros.  A group of a
//            multiple of 32 outputs on a plane with the rows for it (gc8_rows) takes v_mfma_f32_32x32x16 instead (M = 32):
//            32 rows in convg_c8.hip's row order, 32 pixels a unit, two cells a step, whole 16-byte cells stored.
//   source   the group's R8g octet planes of the tile's source rows and columns, halo included, staged once in LDS
//            ([octet][IH][IW] cells, 16-byte loads, +0 outside the map); a table of the reduction cells' LDS offsets
//            (octet plane + tap shift) beside it, built once a block: a step's operand is ONE ds_read_b128 at
//            pixel base + table[cell].  HBM sees a source cell once a block, not f f times.
//   weights  arranged as A operands once per call (gc8_wt_kernel, context scratch): wt[group][row tile][step][lane][8].
//            A wave loads a step's operand once (16 bytes a lane, coalesced, L2-resident: a group's weights are a few KB)
//            and keeps it in registers for the products of all its pixel units.
//   tile     TW = 16 columns (8 / 4 on narrow planes: a unit of 16 pixels is then 2 / 4 rows), 4 waves x npr units of
//            rows, npr 4 at most; npr halves until the plane is not overshot and the source tile fits GC_LDS_MAX.
//   store    lane l holds rows 4 (l / 16) .. + 3 of its pixel: half a cell, one 8-byte store.  Every cell of the output
//            is written: pad cells and pixels no window touches as +0.
// Weight gradient (gc8_wgrad_kernel): c8_convg_wgrad_kernel's form confined to a group -- a block stages 64 output pixels
//   of up to 8 filter octets of dz and up to 8 column cells (tap x octet of the GROUP's channels, each with its tap's
//   shift) of x in LDS as they are, reads them back with the transposing LDS read into 32x32x16 operands, skips the row /
//   column tile a narrow group leaves empty, adds the four waves' sums in wave order and writes one slab in dW's layout;
//   db from the staged dz.  grid (slabs, column-cell groups, groups x filter-octet groups); tn_red_wgrad finishes.
// Index range: fewer than 2^32 cells a tensor, f <= 255, f f max(C/g, K/g) / 8 <= 4096 reduction cells, at most 65535 groups.
#include <type_traits>

#include "c8_elem.h"
#include "gconv.h"

typedef float gc_f32x4 __attribute__((ext_vector_type(4)));
typedef short gc_short4 __attribute__((ext_vector_type(4)));
typedef short gc_short8 __attribute__((ext_vector_type(8)));

#define GC8_CELLS_MAX 4096

template <typename E>
__device__ __forceinline__ gc_f32x4 gc8_mfma(typename E::v8 a, typename E::v8 b, gc_f32x4 c) {
    if constexpr (E::BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// row of a 32-row operand tile that MFMA row rho stands for (convg_c8.hip, cg_row): a lane's accumulators 8 h .. 8 h + 7 are
// then the whole cell of octet 2 h + lane / 32
__host__ __device__ __forceinline__ int gc8_row32(int rho) {
    const int hi = (rho >> 2) & 1, r = (rho & 3) + 4 * (rho >> 3);
    return 8 * (2 * (r >> 3) + hi) + (r & 7);
}

// wt[(((grp MT + mt) R4 + step) 64 + lane) 8 + e] = W(row M mt + lane % M (M = 32: gc8_row32 of it) of the group, reduction
// cell (64 / M) step + lane / M: tap rc / R8g, reduced map 8 (rc % R8g) + e of the group), rounded; forward: row = filter,
// reduced = channel; dgrad: swapped.
template <typename E>
__global__ __launch_bounds__(256) void gc8_wt_kernel(const float* __restrict__ W, typename E::T* __restrict__ wt, int Kg, int Cg,
                                                    int T, int R8g, int R4, int MT, int M, int dgrad, unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int e = idx & 7u, l = (idx >> 3) & 63u;
    const unsigned rest = idx >> 9;
    const int step = rest % (unsigned)R4;
    const unsigned r2 = rest / (unsigned)R4;
    const int mt = r2 % (unsigned)MT, grp = r2 / (unsigned)MT;
    const int row = M == 32 ? 32 * mt + gc8_row32(l & 31) : 16 * mt + (l & 15);
    const int rc = M == 32 ? 2 * step + (l >> 5) : 4 * step + (l >> 4);
    const int tap = rc / R8g, red = 8 * (rc - tap * R8g) + e;
    const int kl = dgrad ? red : row, cl = dgrad ? row : red;
    wt[idx] = (typename E::T)((tap < T && kl < Kg && cl < Cg) ? W[(((size_t)grp * Kg + kl) * Cg + cl) * T + tap] : 0.f);
}

struct GC8 {
    const uint4* src;        // the B operand's tensor: x (forward), dz (input gradient)
    const uint4* wt;
    uint4* out;
    const float* bias;       // forward
    const uint4* prev_a;     // input gradient: stored output of the layer below (NULL: none)
    int Ss, Ps;              // source maps: side, pitch
    unsigned PPs;
    int So, Po;              // output maps of this product: side, pitch
    unsigned PPo;
    unsigned R8, O8;         // octets of the source / output tensor
    unsigned R8g, O8g, Og;   // a group's reduced octets, output octets, outputs
    unsigned RC, R4, MT;     // reduction cells f f R8g, steps, row tiles
    int f, stride, off0;
    int lgTW, npr, TH, IH, IW, tilesX, tiles, direct;
    unsigned tabbytes;
    int act;
    float prm;
};

// M: rows of the matrix instruction -- 16 (v_mfma_f32_16x16x32: four reduction cells a step, 16 pixels a unit) or 32
// (v_mfma_f32_32x32x16 for groups of a multiple of 32 outputs: two cells a step, 32 pixels a unit, whole cells stored)
template <typename E, int MODE, int M>
__global__ __launch_bounds__(256) void gc8_kernel(GC8 g) {
    typedef typename E::v8 v8;
    typedef typename E::v4 v4;
    typedef typename std::conditional<M == 32, f32x16, gc_f32x4>::type acc_t;
    constexpr int CS = 64 / M, LGM = M == 32 ? 5 : 4;
    extern __shared__ __attribute__((aligned(16))) char gc_smem[];
    int2* const tab = reinterpret_cast<int2*>(gc_smem);       // [CS R4] x: LDS offset of the cell, y: (octet, du, dv); -1 past the end
    uint4* const tile = reinterpret_cast<uint4*>(gc_smem + g.tabbytes);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> LGM, px = lane & (M - 1);
    const unsigned n = blockIdx.x / (unsigned)g.tiles, tl = blockIdx.x - n * (unsigned)g.tiles, grp = blockIdx.y;
    const int ty = (int)tl / g.tilesX, tx = (int)tl - ty * g.tilesX;
    const int TW = 1 << g.lgTW, s = g.stride, se = MODE == 0 ? s : 1, f = g.f;
    const int y0 = ty * g.TH, x0 = tx * TW;
    const int sy0 = gc_src0(MODE, y0, g.off0, s), sx0 = gc_src0(MODE, x0, g.off0, s);
    const size_t plane0 = (size_t)n * g.R8 + (size_t)grp * g.R8g;             // the group's first source plane

    for (int i = t; i < CS * (int)g.R4; i += 256) {
        int2 e = make_int2(-1, -1);
        if (i < (int)g.RC) {
            const int tap = i / (int)g.R8g, oct = i - tap * (int)g.R8g, u = tap / f, v = tap - u * f;
            const int du = MODE == 0 ? f - 1 - u : u, dv = MODE == 0 ? f - 1 - v : v;
            e = make_int2((oct * g.IH + du) * g.IW + dv, (oct << 16) | (du << 8) | dv);
        }
        tab[i] = e;
    }
    if (!g.direct) {
        const int per = g.IH * g.IW, total = (int)g.R8g * per;
        for (int i = t; i < total; i += 256) {
            const int oct = i / per, rem = i - oct * per, r = rem / g.IW, c = rem - r * g.IW;
            const int gy = sy0 + r, gx = sx0 + c;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (gy >= 0 && gy < g.Ss && gx >= 0 && gx < g.Ss) v = g.src[(plane0 + oct) * g.PPs + (unsigned)gy * g.Ps + (unsigned)gx];
            tile[i] = v;
        }
    }
    __syncthreads();

    // this lane's pixel of unit i: unit wave npr + i of the tile, M >> lgTW rows of TW columns
    const int col = px & (TW - 1), rsub = px >> g.lgTW, ox = x0 + col;
    int oy[4], base[4];
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rl = ((wave * g.npr + i) << (LGM - g.lgTW)) + rsub;
        oy[i] = y0 + rl;
        base[i] = rl * se * g.IW + col * se;
        live[i] = i < g.npr && oy[i] < g.So && ox < g.So;
    }
    auto operand = [&](int i, int2 e) __attribute__((always_inline)) {
        uint4 val = make_uint4(0u, 0u, 0u, 0u);
        if (e.x >= 0 && live[i]) {
            if (MODE != 2 && !g.direct) {
                val = tile[base[i] + e.x];
            } else {
                const int oct = e.y >> 16;
                int sy = oy[i] * se + g.off0 + ((e.y >> 8) & 255), sx = ox * se + g.off0 + (e.y & 255);
                bool in = true;
                if (MODE == 2) {
                    const int qy = sy / s, qx = sx / s;
                    in = sy >= 0 && sx >= 0 && qy * s == sy && qx * s == sx;
                    sy = qy; sx = qx;
                }
                if (in) {
                    if (!g.direct) val = tile[(oct * g.IH + (sy - sy0)) * g.IW + (sx - sx0)];
                    else if (sy >= 0 && sy < g.Ss && sx >= 0 && sx < g.Ss)
                        val = g.src[(plane0 + oct) * g.PPs + (unsigned)sy * g.Ps + (unsigned)sx];
                }
            }
        }
        return __builtin_bit_cast(v8, val);
    };

    const bool lk = g.act == TN_ACT_LEAKY;
    const float prm = g.prm, tie = prm > 0.f ? 1.f + prm : 0.f;
    for (unsigned mt = 0; mt < g.MT; ++mt) {
        acc_t acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < (M == 32 ? 16 : 4); ++r) acc[i][r] = 0.f;
        const uint4* const wp = g.wt + ((size_t)grp * g.MT + mt) * g.R4 * 64 + lane;
        for (unsigned step = 0; step < g.R4; ++step) {
            const v8 a = __builtin_bit_cast(v8, wp[(size_t)step * 64]);
            const int2 e = tab[CS * step + q];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < g.npr) {
                    if constexpr (M == 32) acc[i] = E::mfma(a, operand(i, e), acc[i]);
                    else acc[i] = gc8_mfma<E>(a, operand(i, e), acc[i]);
                }
        }
        if constexpr (M == 32) {
            // accumulators 8 h .. 8 h + 7: the cell of octet 4 mt + 2 h + q of the group (gc8_row32)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned o8l = 4 * mt + 2 * h + q, o8 = grp * g.O8g + o8l;
                float bv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) bv[e] = MODE == 0 ? g.bias[grp * g.Og + 8 * o8l + e] : 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i >= g.npr || oy[i] >= g.Po || ox >= g.Po) continue;
                    const size_t at = ((size_t)n * g.O8 + o8) * g.PPo + (unsigned)oy[i] * g.Po + (unsigned)ox;
                    const bool deriv = MODE >= 1 && g.prev_a != nullptr && live[i];
                    v8 pa = __builtin_bit_cast(v8, make_uint4(0u, 0u, 0u, 0u));
                    if (deriv) pa = __builtin_bit_cast(v8, g.prev_a[at]);
                    v8 c8;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float z = acc[i][8 * h + e];
                        if (MODE == 0) {
                            z += bv[e];
                            z = lk ? fmaxf(0.f, z) + fminf(0.f, z) * prm : tn_act_fwd(z, g.act, prm);
                        } else if (deriv) {
                            const float a_ = (float)pa[e];
                            z *= lk ? (a_ > 0.f ? 1.f : (a_ < 0.f ? prm : tie)) : tn_act_grad_from_out(a_, g.act, prm);
                        }
                        c8[e] = (typename E::T)(live[i] ? z : 0.f);
                    }
                    g.out[at] = __builtin_bit_cast(uint4, c8);
                }
            }
            continue;
        }
        // rows 4 q .. 4 q + 3 of the tile: half a cell of this lane's pixel
        const unsigned orow = 16 * mt + 4 * q;
        if (orow >= g.Og) continue;
        const unsigned o8 = grp * g.O8g + (orow >> 3), half = (orow >> 2) & 1u;
        float bv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = MODE == 0 ? g.bias[grp * g.Og + orow + e] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= g.npr || oy[i] >= g.Po || ox >= g.Po) continue;
            const size_t at = (((size_t)n * g.O8 + o8) * g.PPo + (unsigned)oy[i] * g.Po + (unsigned)ox) * 2 + half;
            const bool deriv = MODE >= 1 && g.prev_a != nullptr && live[i];
            v4 pa = __builtin_bit_cast(v4, make_uint2(0u, 0u));
            if (deriv) pa = __builtin_bit_cast(v4, reinterpret_cast<const uint2*>(g.prev_a)[at]);
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
            reinterpret_cast<uint2*>(g.out)[at] = __builtin_bit_cast(uint2, c4);
        }
    }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------
struct GC8W {
    const uint4* x;
    const uint4* dz;
    float* ws;               // [slab][K][C/g][f][f] partial dW (scale removed)
    float* dbws;             // [slab][K]
    unsigned S, P, PP, So, SoSo, Po, PPo, C8, K8, K, Cg, Kg, C8g, K8g, KGg, T, CCg, ntiles, nslab;
    int f, stride, pad;
    unsigned long long npix;           // N So So
    float oscale;
};

// MFMA operand (32 rows x 16 pixels) of row tile `tile` out of cells staged [cell][64 pixels] (convg_c8.hip, cg_tr_operand)
template <typename E>
__device__ __forceinline__ typename E::v8 gc8_tr_operand(const char* s, int tile, int pix0, int lane) {
    const int gl = lane >> 4, i = lane & 15;
    const int oct = 4 * tile + 2 * (gl & 1) + ((i & 3) >> 1), pix = pix0 + 8 * (gl >> 1) + (i >> 2);
    const char* a = s + (oct * 64 + pix) * 16 + 8 * (i & 1);
    const gc_short4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) gc_short4*)a);
    const gc_short4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) gc_short4*)(a + 64));
    const gc_short8 r = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
    return __builtin_bit_cast(typename E::v8, r);
}

// grid (slabs, groups of 8 column cells of a group, channel groups x groups of 8 filter octets of a group)
template <typename E>
__global__ __launch_bounds__(256) void gc8_wgrad_kernel(GC8W g) {
    typedef typename E::v8 v8;
    __shared__ __attribute__((aligned(16))) char smem[16384];     // x cells [8][64], dz cells [8][64]; then the waves' sums
    char* const sx = smem;
    char* const sd = smem + 8192;
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, hi = lane >> 5;
    const unsigned slab = blockIdx.x, cc0 = 8 * blockIdx.y, grp = blockIdx.z / g.KGg, ko0 = 8 * (blockIdx.z - grp * g.KGg);
    const unsigned pl = t & 63u;
    const bool rows2 = g.K8g - ko0 > 4, cols2 = g.CCg - cc0 > 4;     // the second 32-row / 32-column tile holds something
    unsigned xo[2];
    int dy[2], dx[2];
    bool xlive[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const unsigned cc = cc0 + wave + 4 * jj;
        xlive[jj] = cc < g.CCg;
        const unsigned tap = xlive[jj] ? cc / g.C8g : 0u;
        xo[jj] = grp * g.C8g + (xlive[jj] ? cc - tap * g.C8g : 0u);
        dy[jj] = g.f - 1 - (int)(tap / (unsigned)g.f) - g.pad;
        dx[jj] = g.f - 1 - (int)(tap % (unsigned)g.f) - g.pad;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    float dbs[2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 8; ++e) dbs[a][e] = 0.f;

    uint4 xr[2], dr[2];
    auto gload = [&](unsigned tile) __attribute__((always_inline)) {
        const unsigned long long gi = (unsigned long long)tile * 64 + pl;
        const bool valid = gi < g.npix;
        const unsigned g_ = valid ? (unsigned)gi : 0u;
        const unsigned n = g_ / g.SoSo, q = g_ - n * g.SoSo;
        const unsigned oh = q / g.So, ow = q - oh * g.So;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const unsigned ol = wave + 4 * jj;
            xr[jj] = make_uint4(0u, 0u, 0u, 0u);
            dr[jj] = make_uint4(0u, 0u, 0u, 0u);
            const int sy = (int)oh * g.stride + dy[jj], sx_ = (int)ow * g.stride + dx[jj];
            if (valid && xlive[jj] && sy >= 0 && sx_ >= 0 && sy < (int)g.S && sx_ < (int)g.S)
                xr[jj] = g.x[((size_t)n * g.C8 + xo[jj]) * g.PP + (unsigned)sy * g.P + (unsigned)sx_];
            if (valid && ko0 + ol < g.K8g)
                dr[jj] = g.dz[((size_t)n * g.K8 + grp * g.K8g + ko0 + ol) * g.PPo + oh * g.Po + ow];
        }
    };

    unsigned tile = slab;
    if (tile < g.ntiles) gload(tile);
    for (; tile < g.ntiles; tile += g.nslab) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const unsigned ol = wave + 4 * jj;
            *reinterpret_cast<uint4*>(sx + (ol * 64 + pl) * 16) = xr[jj];
            *reinterpret_cast<uint4*>(sd + (ol * 64 + pl) * 16) = dr[jj];
            const v8 d8 = __builtin_bit_cast(v8, dr[jj]);
#pragma unroll
            for (int e = 0; e < 8; ++e) dbs[jj][e] += (float)d8[e];
        }
        __syncthreads();
        if (tile + g.nslab < g.ntiles) gload(tile + g.nslab);       // the next tile's cells travel under the products
        v8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = gc8_tr_operand<E>(sd, i, 16 * (int)wave, (int)lane);
            b[i] = gc8_tr_operand<E>(sx, i, 16 * (int)wave, (int)lane);
        }
        acc[0][0] = E::mfma(a[0], b[0], acc[0][0]);
        if (cols2) acc[0][1] = E::mfma(a[0], b[1], acc[0][1]);
        if (rows2) {
            acc[1][0] = E::mfma(a[1], b[0], acc[1][0]);
            if (cols2) acc[1][1] = E::mfma(a[1], b[1], acc[1][1]);
        }
        __syncthreads();
    }

    // the four waves' sums, added in the order 0 + 1 + 2 + 3
    float* const red = reinterpret_cast<float*>(smem);
    for (unsigned w = 1; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(i * 16 + r) * 64 + lane] = acc[i >> 1][i & 1][r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i >> 1][i & 1][r] += red[(i * 16 + r) * 64 + lane];
        }
    }
    if (wave == 0) {
        float* const ws = g.ws + (size_t)slab * g.K * g.Cg * g.T;
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                // column 32 ct + (lane & 31) of the block: column cell cc of the group, element e of it
                const unsigned col = 32 * ct + (lane & 31u), cc = cc0 + (col >> 3);
                const unsigned tap = cc / g.C8g, c = 8 * (cc - tap * g.C8g) + (col & 7u);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned kl = 8 * ko0 + 32 * ft + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (kl < g.Kg && cc < g.CCg)
                        ws[(((size_t)grp * g.Kg + kl) * g.Cg + c) * g.T + tap] = acc[ft][ct][r] * g.oscale;
                }
            }
    }
    // db: a wave holds octets wave and wave + 4 of the filter group, a lane one pixel column of every tile
    if (blockIdx.y == 0) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float s = dbs[jj][e];
#pragma unroll
                for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
                const unsigned kl = 8 * (ko0 + wave + 4 * jj) + e;
                if (lane == 0 && kl < g.Kg) g.dbws[(size_t)slab * g.K + grp * g.Kg + kl] = s * g.oscale;
            }
    }
}

// cells of a c8 tensor of N x C maps of S pixels a side at pitch P (tn_c8_pool_supported's rule), or -1
static long long gc8_cells(int N, int C, int S, int P) {
    if (N <= 0 || C <= 0 || S <= 0 || P < S || (P != S && (P & (P - 1)))) return -1;
    const long long cells = (long long)N * ((C + 7) / 8) * P * P;
    return cells < (1ll << 32) ? cells : -1;
}

static bool gc8_ok(int N, int C, int S, int P, int K, int g, int f, int stride, int pad, int So, int Po) {
    if (!gc_groups_ok(C, K, g) || f > 255) return false;
    const bool narrow = gc_narrow(C, K, g);        // groups of 2 or 4 maps in and out: gconv_c8_narrow.hip
    if (!narrow && (g > 65535 || (C / g) % 8 || (K / g) % 8)) return false;
    if (!gc_axis_ok(S, f, stride, pad, So) || gc8_cells(N, C, S, P) < 0 || gc8_cells(N, K, So, Po) < 0) return false;
    if (narrow) return (long long)K * (C / g) * f * f < (1ll << 28) && gc8n_ok(C, S, P, f, stride, pad, So, Po);
    const long long r8 = (C / g > K / g ? C / g : K / g) / 8;
    return (long long)f * f * r8 <= GC8_CELLS_MAX && (long long)K * (C / g) * f * f < (1ll << 28);
}

#define GC8_ARGS_FMT \
    "(N %d, %d maps of %d pixels at pitch %d -> %d maps of %d pixels at pitch %d, %d groups, filter %d stride %d pad_lo %d)"
#define GC8_ARGS N, C, S, P, K, So, Po, g, f, stride, pad

// The tile of a product (gconv.h): npr pixel units a wave, the source tile in LDS or -- it does not fit -- none (direct)
static void gc8_tile(GC8& g, int mode, int M) {
    const int TW = 1 << g.lgTW, RU = M >> g.lgTW;
    g.tabbytes = ((64 / M) * g.R4 * (unsigned)sizeof(int2) + 15u) & ~15u;
    g.npr = 4;
    while (g.npr > 1 && 4 * (g.npr / 2) * RU >= g.Po) g.npr /= 2;
    g.IW = gc_src_dim(mode, TW, g.f, g.stride);
    for (;;) {
        g.TH = 4 * g.npr * RU;
        g.IH = gc_src_dim(mode, g.TH, g.f, g.stride);
        g.direct = 0;
        if (g.tabbytes + (size_t)g.R8g * g.IH * g.IW * 16 <= GC_LDS_MAX) break;
        if (g.npr > 1) g.npr /= 2;
        else { g.direct = 1; break; }
    }
    g.tilesX = (g.Po + TW - 1) / TW;
    g.tiles = g.tilesX * ((g.Po + g.TH - 1) / g.TH);
}

// The 32-row instruction where a group's outputs are a multiple of 32 and the plane has the rows for four waves of 32-pixel
// units (below that half the block would idle: the 16-row form covers the plane with whole blocks)
static int gc8_rows(const GC8& g, int Og) { return Og % 32 == 0 && g.Po >= 4 * (32 >> g.lgTW) ? 32 : 16; }

template <typename E, int MODE>
static int gc8_run(tn_ctx* ctx, GC8& g, const float* W, int N, int K, int C, int groups, int f) {
    const int dgrad = MODE >= 1 ? 1 : 0, Kg = K / groups, Cg = C / groups;
    const int Og = dgrad ? Cg : Kg, Rg = dgrad ? Kg : Cg;
    g.Og = (unsigned)Og; g.O8g = (unsigned)(Og / 8); g.R8g = (unsigned)(Rg / 8);
    g.O8 = g.O8g * groups; g.R8 = g.R8g * groups;
    g.lgTW = g.Po <= 4 ? 2 : (g.Po <= 8 ? 3 : 4);
    const int M = gc8_rows(g, Og), CS = 64 / M;
    g.RC = (unsigned)(f * f) * g.R8g; g.R4 = (g.RC + CS - 1) / CS; g.MT = (unsigned)((Og + M - 1) / M);
    gc8_tile(g, MODE, M);
    const size_t total = (size_t)groups * g.MT * g.R4 * 512;
    const unsigned long long blocks = (unsigned long long)N * g.tiles;
    TN_REQUIRE(total < (1ull << 31) && blocks < (1ull << 31), "c8 gconv: %d x %d x %d x %d weights, %d images: too large", K, Cg,
               f, f, N);
    float* wt;
    int rc = tn_scratch_get(ctx, total * sizeof(typename E::T), &wt);
    if (rc) return rc;
    gc8_wt_kernel<E><<<cdiv((long long)total, 256), 256, 0, ctx->stream>>>(W, reinterpret_cast<typename E::T*>(wt), Kg, Cg, f * f,
                                                                         (int)g.R8g, (int)g.R4, (int)g.MT, M, dgrad, (unsigned)total);
    TN_LAUNCH_CHECK();
    g.wt = reinterpret_cast<const uint4*>(wt);
    const size_t lds = g.tabbytes + (g.direct ? 0 : (size_t)g.R8g * g.IH * g.IW * 16);
    const dim3 grid((unsigned)blocks, (unsigned)groups);
    rc = M == 32 ? tn_launch_lds<gc8_kernel<E, MODE, 32>>(ctx, grid, dim3(256), lds, g)
                 : tn_launch_lds<gc8_kernel<E, MODE, 16>>(ctx, grid, dim3(256), lds, g);
    if (rc) return rc;
    TN_LAUNCH_CHECK();
    return TN_OK;
}

extern "C" {

#ifndef C8_BF16_TU
// the bf16 entry points (gconv_c8_bf16.hip)
int c8b_tn_c8_gconv_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P, int K,
                        int g, int f, int stride, int pad, int So, int Po, int act, float prm);
int c8b_tn_c8_gconv_dgrad(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K, int g, int f,
                          int stride, int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm);
int c8b_tn_c8_gconv_wgrad(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P, int K,
                          int g, int f, int stride, int pad, int So, int Po);

// 1 if the grouped c8 kernels take a conv layer of this geometry (forward, both gradients; either element type)
int tn_c8_gconv_supported(int N, int C, int S, int P, int K, int g, int f, int stride, int pad, int So, int Po) {
    return gc8_ok(N, C, S, P, K, g, f, stride, pad, So, Po) ? 1 : 0;
}
#endif

// y = act(gconv(x, W) + b); every cell of y is written (pad cells as +0)
int C8_API(tn_c8_gconv_fwd)(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P,
                            int K, int g, int f, int stride, int pad, int So, int Po, int act, float prm) {
    C8_TO_BF16(tn_c8_gconv_fwd, ctx, x, W, b, y, N, C, S, P, K, g, f, stride, pad, So, Po, act, prm);
    TN_REQUIRE(x && W && b && y && gc8_ok(N, C, S, P, K, g, f, stride, pad, So, Po),
               "tn_c8_gconv_fwd: bad arguments " GC8_ARGS_FMT, GC8_ARGS);
    if (gc_narrow(C, K, g)) return C8_API(gc8n_fwd)(ctx, x, W, b, y, N, C, S, P, g, f, stride, pad, So, Po, act, prm);
    GC8 q{};
    q.src = static_cast<const uint4*>(x); q.out = static_cast<uint4*>(y); q.bias = b; q.act = act; q.prm = prm;
    q.Ss = S; q.Ps = P; q.PPs = (unsigned)P * P;
    q.So = So; q.Po = Po; q.PPo = (unsigned)Po * Po;
    q.f = f; q.stride = stride; q.off0 = -pad;
    return gc8_run<C8E, 0>(ctx, q, W, N, K, C, g, f);
}

// dx = (transposed gconv of dz with W) * act'(prev_a) (prev_a NULL: none); every cell of dx is written (pad cells and input
// pixels no window touches as +0)
int C8_API(tn_c8_gconv_dgrad)(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K, int g,
                              int f, int stride, int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm) {
    C8_TO_BF16(tn_c8_gconv_dgrad, ctx, dz, W, dx, N, C, S, P, K, g, f, stride, pad, So, Po, prev_a, prev_act, prev_prm);
    TN_REQUIRE(dz && W && dx && gc8_ok(N, C, S, P, K, g, f, stride, pad, So, Po),
               "tn_c8_gconv_dgrad: bad arguments " GC8_ARGS_FMT, GC8_ARGS);
    if (gc_narrow(C, K, g))
        return C8_API(gc8n_dgrad)(ctx, dz, W, dx, N, C, S, P, g, f, stride, pad, So, Po, prev_a, prev_act, prev_prm);
    GC8 q{};
    q.src = static_cast<const uint4*>(dz); q.out = static_cast<uint4*>(dx); q.prev_a = static_cast<const uint4*>(prev_a);
    q.act = prev_act; q.prm = prev_prm;
    q.Ss = So; q.Ps = Po; q.PPs = (unsigned)Po * Po;
    q.So = S; q.Po = P; q.PPo = (unsigned)P * P;
    q.f = f; q.stride = stride; q.off0 = pad - (f - 1);
    return stride == 1 ? gc8_run<C8E, 1>(ctx, q, W, N, K, C, g, f) : gc8_run<C8E, 2>(ctx, q, W, N, K, C, g, f);
}

// dW (K, C/g, f, f), db (K) from x and dz; dz carries the gradient scale, the results do not.  OVERWRITE
int C8_API(tn_c8_gconv_wgrad)(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P,
                              int K, int g, int f, int stride, int pad, int So, int Po) {
    C8_TO_BF16(tn_c8_gconv_wgrad, ctx, x, dz, dW, db, N, C, S, P, K, g, f, stride, pad, So, Po);
    TN_REQUIRE(x && dz && dW && db && gc8_ok(N, C, S, P, K, g, f, stride, pad, So, Po),
               "tn_c8_gconv_wgrad: bad arguments " GC8_ARGS_FMT, GC8_ARGS);
    if (gc_narrow(C, K, g)) return C8_API(gc8n_wgrad)(ctx, x, dz, dW, db, N, C, S, P, g, f, stride, pad, So, Po);
    GC8W q{};
    q.x = static_cast<const uint4*>(x); q.dz = static_cast<const uint4*>(dz);
    q.S = (unsigned)S; q.P = (unsigned)P; q.PP = (unsigned)P * P;
    q.So = (unsigned)So; q.SoSo = (unsigned)So * So; q.Po = (unsigned)Po; q.PPo = (unsigned)Po * Po;
    q.C8 = (unsigned)(C / 8); q.K8 = (unsigned)(K / 8); q.K = (unsigned)K;
    q.Cg = (unsigned)(C / g); q.Kg = (unsigned)(K / g); q.C8g = q.Cg / 8; q.K8g = q.Kg / 8;
    q.T = (unsigned)(f * f); q.CCg = q.T * q.C8g; q.KGg = (unsigned)cdiv(q.K8g, 8);
    q.f = f; q.stride = stride; q.pad = pad;
    q.npix = (unsigned long long)N * q.SoSo;
    const int CG = cdiv(q.CCg, 8);
    const long long nt = (long long)((q.npix + 63) / 64), gz = (long long)g * q.KGg;
    TN_REQUIRE(CG <= 65535 && gz <= 65535, "tn_c8_gconv_wgrad: %d x %d x %d x %d weights: too large", K, C / g, f, f);
    q.ntiles = (unsigned)nt; q.nslab = gc_slabs(nt, (long long)CG * gz, 512);
    const size_t n = (size_t)K * q.Cg * q.T;
    int rc = tn_scratch_get(ctx, ((size_t)q.nslab * n + (size_t)q.nslab * K) * sizeof(float), &q.ws);
    if (rc) return rc;
    q.dbws = q.ws + (size_t)q.nslab * n;
    q.oscale = 1.f / ctx->grad_scale;
    gc8_wgrad_kernel<C8E><<<dim3(q.nslab, (unsigned)CG, (unsigned)gz), 256, 0, ctx->stream>>>(q);
    TN_LAUNCH_CHECK();
    return tn_red_wgrad(ctx, q.ws, dW, (uint32_t)n, q.nslab, (uint32_t)n, q.dbws, db, (uint32_t)K, q.nslab, (uint32_t)K);
}

}  // extern "C"
