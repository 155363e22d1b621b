// DTYPE 'float16' / 'bfloat16': ConvLayer(..., dilation=d) on the 16-bit-resident c8 tensors of the conv stack
// ([N][C/8][P][P][8] 16-bit values; x / dx: S x S maps at pitch P, y / dz: So x So maps at pitch Po): tn_c8_dilconv_fwd /
// _dgrad / _wgrad.  Any C and K (a ragged last octet holds +0 past the maps, as in convg_c8.hip).  Arithmetic: the stack's
// -- x and dz as stored, W rounded to the element type while it is arranged, exact products, fp32 accumulation on the matrix
// core, bias / activation on the fp32 sums, one rounding on store; the weight gradient's fp32 epilogue removes the gradient
// scale.  Filter orientation: tn_conv2d_*'s.  dilconv.h has the polyphase split, the tile and the LDS pitch.
//
// Forward / input gradient (dc8_kernel): grid (images x tiles of a phase plane, phases, groups of row tiles), 256 lanes.
//   product  v_mfma_f32_16x16x32: 16 rows are 16 outputs (filters forward, channels input gradient), 16 columns 16 pixels
//            of the phase's tile, the 32-deep reduction FOUR reduction cells rc = tap * RCH + octet of the chunk, one a
//            quarter wave -- a 16-byte cell as it is stored is a lane's B operand.  A multiple of 32 outputs on a phase
//            plane with the rows for it (gc8_rows's rule on the phase plane) takes v_mfma_f32_32x32x16: 32 rows in
//            convg_c8.hip's row order, 32 pixels a unit, two cells a step, whole 16-byte cells stored.
//   source   the chunk's octet planes of the phase's source tile ([octet][IH][IWp] cells), 16-byte loads at a stride of d
//            cells, +0 outside the map; beside it a table of the reduction cells' LDS offsets (octet plane + tap shift),
//            built once a block: a step's operand is ONE ds_read_b128 at pixel base + table[cell], read once for all the
//            row tiles the wave accumulates.
//   weights  arranged as A operands once per call (dc8_wt_kernel, context scratch): wt[row tile][chunk][step][lane][8];
//            a wave loads a step's operand of each of its row tiles (16 bytes a lane, coalesced, L2-resident).
//   store    16-row form: a lane holds rows 4 (l / 16) .. + 3 of its pixel, half a cell, one 8-byte store; 32-row form:
//            whole cells.  The cells of a phase lie d cells apart.  Every cell of the output is written: pad cells and
//            maps past the last as +0.
// Weight gradient (dc8_wgrad_kernel): gconv_c8.hip's form with the tap offsets multiplied by d -- a block stages 64 output
//   pixels of up to 8 filter octets of dz and up to 8 column cells (tap x channel octet, each with its tap's dilated shift)
//   of x in LDS as they are, reads them back with the transposing LDS read into 32x32x16 operands, adds the four waves'
//   sums in wave order and writes one slab in dW's layout; db from the staged dz.  grid (slabs, column-cell groups,
//   filter-octet groups); tn_red_wgrad finishes.
// d = 1 with a stride above 1 is the general family's layer and is handed to tn_c8_convg_*.
// Index range: fewer than 2^32 cells a tensor, f <= 32, d <= 255, K C f f < 2^28.
#include <type_traits>

#include "c8_elem.h"
#include "dilconv.h"

typedef float dc_f32x4 __attribute__((ext_vector_type(4)));
typedef short dc_short4 __attribute__((ext_vector_type(4)));
typedef short dc_short8 __attribute__((ext_vector_type(8)));

template <typename E>
__device__ __forceinline__ dc_f32x4 dc8_mfma(typename E::v8 a, typename E::v8 b, dc_f32x4 c) {
    if constexpr (E::BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
template <typename E>
__device__ __forceinline__ f32x16 dc8_mfma(typename E::v8 a, typename E::v8 b, f32x16 c) { return E::mfma(a, b, c); }

// row of a 32-row operand tile that MFMA row rho stands for (convg_c8.hip, cg_row): a lane's accumulators 8 h .. 8 h + 7 are
// then the whole cell of octet 2 h + lane / 32
__host__ __device__ __forceinline__ int dc8_row32(int rho) {
    const int hi = (rho >> 2) & 1, r = (rho & 3) + 4 * (rho >> 3);
    return 8 * (2 * (r >> 3) + hi) + (r & 7);
}

// wt[((((mt NCH + ch) R4c + step) 64 + lane) 8 + e] = W(row M mt + lane % M (M = 32: dc8_row32 of it), reduction cell
// (64 / M) step + lane / M of chunk ch: tap rc / RCH, reduced map 8 (ch RCH + rc % RCH) + e), rounded; forward: row = filter,
// reduced = channel; dgrad: swapped.  Zero past the ends.
template <typename E>
__global__ __launch_bounds__(256) void dc8_wt_kernel(const float* __restrict__ W, typename E::T* __restrict__ wt, int K, int C,
                                                    int T, int RCH, int NCH, int R4c, int M, int dgrad, unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int e = idx & 7u, l = (idx >> 3) & 63u;
    const unsigned rest = idx >> 9;
    const int step = rest % (unsigned)R4c;
    const unsigned r2 = rest / (unsigned)R4c;
    const int ch = r2 % (unsigned)NCH, mt = r2 / (unsigned)NCH;
    const int row = M == 32 ? 32 * mt + dc8_row32(l & 31) : 16 * mt + (l & 15);
    const int rc = M == 32 ? 2 * step + (l >> 5) : 4 * step + (l >> 4);
    const int tap = rc / RCH, red = 8 * (ch * RCH + rc - tap * RCH) + e;
    const int k = dgrad ? red : row, c = dgrad ? row : red;
    wt[idx] = (typename E::T)((tap < T && k < K && c < C) ? W[((size_t)k * C + c) * T + tap] : 0.f);
}

struct DC8 {
    const uint4* src;        // the B operand's tensor: x (forward), dz (input gradient)
    const uint4* wt;
    uint4* out;
    const float* bias;       // forward
    const uint4* prev_a;     // input gradient: stored output of the layer below (NULL: none)
    int Ss, Ps;              // source maps: side, pitch
    unsigned PPs;
    int So, Po;              // output maps of this product: side, pitch
    unsigned PPo;
    unsigned R8, O8, O;      // octets of the source / output tensor, output maps
    int RCH, NCH, R4c, MT;   // octets a chunk, chunks, steps a chunk, row tiles
    int f, d, dP, off0;      // dP: phases an axis
    int lgTW, lgWU, npr, TH, IH, IW, IWp, tilesX, tiles;
    unsigned tabbytes;
    int act;
    float prm;
};

// M: rows of the matrix instruction, 16 or 32 (above)
template <typename E, int MODE, int M>
__global__ __launch_bounds__(256) void dc8_kernel(DC8 g) {
    typedef typename E::v8 v8;
    typedef typename E::v4 v4;
    typedef typename std::conditional<M == 32, f32x16, dc_f32x4>::type acc_t;
    constexpr int CS = 64 / M, LGM = M == 32 ? 5 : 4, MB = M == 32 ? DC_MTB / 2 : DC_MTB;
    extern __shared__ __attribute__((aligned(16))) char dc_smem[];
    int* const tab = reinterpret_cast<int*>(dc_smem);         // [CS R4c] LDS offset of the cell, -1 past the end
    uint4* const tile = reinterpret_cast<uint4*>(dc_smem + g.tabbytes);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> LGM, px = lane & (M - 1);
    const unsigned n = blockIdx.x / (unsigned)g.tiles, tl = blockIdx.x - n * (unsigned)g.tiles;
    const int pyh = (int)blockIdx.y / g.dP, pxh = (int)blockIdx.y - pyh * g.dP;
    const int ty = (int)tl / g.tilesX, tx = (int)tl - ty * g.tilesX;
    const int TW = 1 << g.lgTW, d = g.d, f = g.f;
    const int y0 = ty * g.TH, x0 = tx * TW;                   // in the phase's plane
    if (y0 >= dc_count(g.Po, pyh, d) || x0 >= dc_count(g.Po, pxh, d)) return;      // a ragged phase: no such tile
    const bool any = pyh + d * y0 < g.So && pxh + d * x0 < g.So;                   // (else: pad cells alone)
    const int sy0 = pyh + g.off0 + d * y0, sx0 = pxh + g.off0 + d * x0;            // source pixel of the staged tile's corner

    for (int i = t; i < CS * g.R4c; i += 256) {
        int e = -1;
        if (i < f * f * g.RCH) {
            const int tap = i / g.RCH, oct = i - tap * g.RCH, u = tap / f, v = tap - u * f;
            const int du = MODE == 0 ? f - 1 - u : u, dv = MODE == 0 ? f - 1 - v : v;
            e = (oct * g.IH + du) * g.IWp + dv;
        }
        tab[i] = e;
    }

    // this lane's pixel of unit i: unit wu npr + i of the tile, M >> lgTW rows of TW columns of the phase plane
    const int wu = wave & ((1 << g.lgWU) - 1), wm = wave >> g.lgWU, WM = 4 >> g.lgWU;
    const int col = px & (TW - 1), rsub = px >> g.lgTW, ox = pxh + d * (x0 + col);
    int oy[4], base[4];
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rl = ((wu * g.npr + i) << (LGM - g.lgTW)) + rsub;
        oy[i] = pyh + d * (y0 + rl);
        base[i] = rl * g.IWp + col;
        live[i] = i < g.npr && oy[i] < g.So && ox < g.So;
    }
    const int mt0 = (int)blockIdx.z * MB * WM + wm;           // this wave's row tiles: mt0 + m WM
    acc_t acc[MB][4];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < (M == 32 ? 16 : 4); ++r) acc[m][i][r] = 0.f;

    const int per = g.IH * g.IW, nch = any ? g.NCH : 0;
    for (int ch = 0; ch < nch; ++ch) {
        if (ch) __syncthreads();
        for (int i = t; i < g.RCH * per; i += 256) {
            const int ol = i / per, rem = i - ol * per, r = rem / g.IW, c = rem - r * g.IW;
            const int gy = sy0 + d * r, gx = sx0 + d * c;
            const unsigned oct = (unsigned)(ch * g.RCH + ol);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (oct < g.R8 && gy >= 0 && gy < g.Ss && gx >= 0 && gx < g.Ss)
                v = g.src[((size_t)n * g.R8 + oct) * g.PPs + (unsigned)gy * g.Ps + (unsigned)gx];
            tile[(ol * g.IH + r) * g.IWp + c] = v;
        }
        __syncthreads();
        for (int step = 0; step < g.R4c; ++step) {
            const int e = tab[CS * step + q];
            v8 b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint4 val = make_uint4(0u, 0u, 0u, 0u);
                if (e >= 0 && live[i]) val = tile[base[i] + e];
                b[i] = __builtin_bit_cast(v8, val);
            }
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const int mt = mt0 + m * WM;
                if (mt >= g.MT) break;
                const v8 a = __builtin_bit_cast(v8, g.wt[(((size_t)mt * g.NCH + ch) * g.R4c + step) * 64 + lane]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < g.npr) acc[m][i] = dc8_mfma<E>(a, b[i], acc[m][i]);
            }
        }
    }

    const bool lk = g.act == TN_ACT_LEAKY;
    const float prm = g.prm, tie = prm > 0.f ? 1.f + prm : 0.f;
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int mt = mt0 + m * WM;
        if (mt >= g.MT) break;
        if constexpr (M == 32) {
            // accumulators 8 h .. 8 h + 7: the cell of octet 4 mt + 2 h + q (dc8_row32); O is a multiple of 32
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned o8 = 4 * mt + 2 * h + q;
                float bv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) bv[e] = MODE == 0 ? g.bias[8 * o8 + e] : 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i >= g.npr || oy[i] >= g.Po || ox >= g.Po) continue;
                    const size_t at = ((size_t)n * g.O8 + o8) * g.PPo + (unsigned)oy[i] * g.Po + (unsigned)ox;
                    const bool deriv = MODE == 1 && g.prev_a != nullptr && live[i];
                    v8 pa = __builtin_bit_cast(v8, make_uint4(0u, 0u, 0u, 0u));
                    if (deriv) pa = __builtin_bit_cast(v8, g.prev_a[at]);
                    v8 c8;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float z = acc[m][i][8 * h + e];
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
        } else {
            // rows 4 q .. 4 q + 3 of the tile: half a cell of this lane's pixel
            const unsigned orow = 16 * mt + 4 * q;
            if (orow >= 8 * g.O8) continue;
            const unsigned o8 = orow >> 3, half = (orow >> 2) & 1u;
            float bv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[e] = (MODE == 0 && orow + e < g.O) ? g.bias[orow + e] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i >= g.npr || oy[i] >= g.Po || ox >= g.Po) continue;
                const size_t at = (((size_t)n * g.O8 + o8) * g.PPo + (unsigned)oy[i] * g.Po + (unsigned)ox) * 2 + half;
                const bool deriv = MODE == 1 && g.prev_a != nullptr && live[i];
                v4 pa = __builtin_bit_cast(v4, make_uint2(0u, 0u));
                if (deriv) pa = __builtin_bit_cast(v4, reinterpret_cast<const uint2*>(g.prev_a)[at]);
                v4 c4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float z = acc[m][i][e];
                    if (MODE == 0) {
                        z += bv[e];
                        z = lk ? fmaxf(0.f, z) + fminf(0.f, z) * prm : tn_act_fwd(z, g.act, prm);
                    } else if (deriv) {
                        const float a_ = (float)pa[e];
                        z *= lk ? (a_ > 0.f ? 1.f : (a_ < 0.f ? prm : tie)) : tn_act_grad_from_out(a_, g.act, prm);
                    }
                    c4[e] = (typename E::T)((live[i] && orow + e < g.O) ? z : 0.f);
                }
                reinterpret_cast<uint2*>(g.out)[at] = __builtin_bit_cast(uint2, c4);
            }
        }
    }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------
struct DC8W {
    const uint4* x;
    const uint4* dz;
    float* ws;               // [slab][K][C][f][f] partial dW (scale removed)
    float* dbws;             // [slab][K]
    unsigned S, P, PP, So, SoSo, Po, PPo, C8, K8, K, C, T, CC, ntiles, nslab;
    int f, d, pad;
    unsigned long long npix;           // N So So
    float oscale;
};

// MFMA operand (32 rows x 16 pixels) of row tile `tile` out of cells staged [cell][64 pixels] (convg_c8.hip, cg_tr_operand)
template <typename E>
__device__ __forceinline__ typename E::v8 dc8_tr_operand(const char* s, int tile, int pix0, int lane) {
    const int gl = lane >> 4, i = lane & 15;
    const int oct = 4 * tile + 2 * (gl & 1) + ((i & 3) >> 1), pix = pix0 + 8 * (gl >> 1) + (i >> 2);
    const char* a = s + (oct * 64 + pix) * 16 + 8 * (i & 1);
    const dc_short4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) dc_short4*)a);
    const dc_short4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) dc_short4*)(a + 64));
    const dc_short8 r = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
    return __builtin_bit_cast(typename E::v8, r);
}

// grid (slabs, groups of 8 column cells, groups of 8 filter octets)
template <typename E>
__global__ __launch_bounds__(256) void dc8_wgrad_kernel(DC8W g) {
    typedef typename E::v8 v8;
    __shared__ __attribute__((aligned(16))) char smem[16384];     // x cells [8][64], dz cells [8][64]; then the waves' sums
    char* const sx = smem;
    char* const sd = smem + 8192;
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, hi = lane >> 5;
    const unsigned slab = blockIdx.x, cc0 = 8 * blockIdx.y, ko0 = 8 * blockIdx.z;
    const unsigned pl = t & 63u;
    const bool rows2 = g.K8 - ko0 > 4, cols2 = g.CC - cc0 > 4;     // the second 32-row / 32-column tile holds something
    unsigned xo[2];
    int dy[2], dx[2];
    bool xlive[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const unsigned cc = cc0 + wave + 4 * jj;
        xlive[jj] = cc < g.CC;
        const unsigned tap = xlive[jj] ? cc / g.C8 : 0u;
        xo[jj] = xlive[jj] ? cc - tap * g.C8 : 0u;
        dy[jj] = (g.f - 1 - (int)(tap / (unsigned)g.f)) * g.d - g.pad;       // the tap's dilated shift
        dx[jj] = (g.f - 1 - (int)(tap % (unsigned)g.f)) * g.d - g.pad;
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
            const int sy = (int)oh + dy[jj], sx_ = (int)ow + dx[jj];
            if (valid && xlive[jj] && sy >= 0 && sx_ >= 0 && sy < (int)g.S && sx_ < (int)g.S)
                xr[jj] = g.x[((size_t)n * g.C8 + xo[jj]) * g.PP + (unsigned)sy * g.P + (unsigned)sx_];
            if (valid && ko0 + ol < g.K8) dr[jj] = g.dz[((size_t)n * g.K8 + ko0 + ol) * g.PPo + oh * g.Po + ow];
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
            a[i] = dc8_tr_operand<E>(sd, i, 16 * (int)wave, (int)lane);
            b[i] = dc8_tr_operand<E>(sx, i, 16 * (int)wave, (int)lane);
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
        float* const ws = g.ws + (size_t)slab * g.K * g.C * g.T;
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                // column 32 ct + (lane & 31) of the block: column cell cc, element e of it
                const unsigned col = 32 * ct + (lane & 31u), cc = cc0 + (col >> 3);
                const unsigned tap = cc / g.C8, c = 8 * (cc - tap * g.C8) + (col & 7u);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned k = 8 * ko0 + 32 * ft + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (k < g.K && cc < g.CC && c < g.C) ws[((size_t)k * g.C + c) * g.T + tap] = acc[ft][ct][r] * g.oscale;
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
                const unsigned k = 8 * (ko0 + wave + 4 * jj) + e;
                if (lane == 0 && k < g.K) g.dbws[(size_t)slab * g.K + k] = s * g.oscale;
            }
    }
}

// cells of a c8 tensor of N x C maps of S pixels a side at pitch P (tn_c8_pool_supported's rule), or -1
static long long dc8_cells(int N, int C, int S, int P) {
    if (N <= 0 || C <= 0 || S <= 0 || P < S || (P != S && (P & (P - 1)))) return -1;
    const long long cells = (long long)N * ((C + 7) / 8) * P * P;
    return cells < (1ll << 32) ? cells : -1;
}

static bool dc8_ok(int N, int C, int S, int P, int K, int d, int f, int stride, int pad, int So, int Po) {
    if (!dc_axis_ok(S, f, d, stride, pad, So) || dc8_cells(N, C, S, P) < 0 || dc8_cells(N, K, So, Po) < 0) return false;
    return (long long)K * C * f * f < (1ll << 28);
}

#define DC8_ARGS_FMT \
    "(N %d, %d maps of %d pixels at pitch %d -> %d maps of %d pixels at pitch %d, dilation %d, filter %d stride %d pad_lo %d)"
#define DC8_ARGS N, C, S, P, K, So, Po, d, f, stride, pad

template <typename E, int MODE>
static int dc8_run(tn_ctx* ctx, DC8& g, const float* W, int N, int K, int C) {
    const int O = MODE ? C : K, R = MODE ? K : C, T = g.f * g.f;
    g.O = (unsigned)O; g.O8 = (unsigned)((O + 7) / 8); g.R8 = (unsigned)((R + 7) / 8);
    g.dP = g.d < g.Po ? g.d : g.Po;
    const int cnt = dc_count(g.Po, 0, g.d);                    // the largest phase plane's side
    g.lgTW = cnt <= 4 ? 2 : (cnt <= 8 ? 3 : 4);
    const int TW = 1 << g.lgTW;
    const int M = (O % 32 == 0 && cnt >= 4 * (32 >> g.lgTW)) ? 32 : 16, CS = 64 / M, RU = M >> g.lgTW;
    const int WU = dc_waves_over_pixels(cnt, RU), WM = 4 / WU, MB = M == 32 ? DC_MTB / 2 : DC_MTB;
    g.lgWU = WU == 4 ? 2 : (WU == 2 ? 1 : 0);
    g.MT = (O + M - 1) / M;
    g.npr = 4;
    while (g.npr > 1 && WU * (g.npr / 2) * RU >= cnt) g.npr /= 2;
    g.IW = TW + g.f - 1;
    g.IWp = dc_pitch(g.IW, TW);
    g.RCH = (int)g.R8;
    for (;;) {                                                  // shrink the tile, then chunk the maps, until LDS holds it
        g.TH = WU * g.npr * RU;
        g.IH = (g.TH < cnt ? g.TH : cnt) + g.f - 1;
        g.R4c = (T * g.RCH + CS - 1) / CS;
        g.tabbytes = ((unsigned)(CS * g.R4c) * (unsigned)sizeof(int) + 15u) & ~15u;
        if (g.tabbytes + (size_t)g.RCH * g.IH * g.IWp * 16 <= GC_LDS_MAX) break;
        if (g.npr > 1) g.npr /= 2;
        else g.RCH = (g.RCH + 1) / 2;
    }
    g.NCH = ((int)g.R8 + g.RCH - 1) / g.RCH;
    g.tilesX = (cnt + TW - 1) / TW;
    g.tiles = g.tilesX * ((cnt + g.TH - 1) / g.TH);
    const size_t total = (size_t)g.MT * g.NCH * g.R4c * 512;
    const unsigned long long blocks = (unsigned long long)N * g.tiles;
    const int ZB = (g.MT + MB * WM - 1) / (MB * WM);
    TN_REQUIRE(total < (1ull << 31) && blocks < (1ull << 31) && ZB <= 65535, "c8 dilconv: %d x %d x %d x %d weights, %d images: too large",
               K, C, g.f, g.f, N);
    float* wt;
    int rc = tn_scratch_get(ctx, total * sizeof(typename E::T), &wt);
    if (rc) return rc;
    dc8_wt_kernel<E><<<cdiv((long long)total, 256), 256, 0, ctx->stream>>>(W, reinterpret_cast<typename E::T*>(wt), K, C, T, g.RCH,
                                                                         g.NCH, g.R4c, M, MODE, (unsigned)total);
    TN_LAUNCH_CHECK();
    g.wt = reinterpret_cast<const uint4*>(wt);
    const size_t lds = g.tabbytes + (size_t)g.RCH * g.IH * g.IWp * 16;
    const dim3 grid((unsigned)blocks, (unsigned)(g.dP * g.dP), (unsigned)ZB);
    rc = M == 32 ? tn_launch_lds<dc8_kernel<E, MODE, 32>>(ctx, grid, dim3(256), lds, g)
                 : tn_launch_lds<dc8_kernel<E, MODE, 16>>(ctx, grid, dim3(256), lds, g);
    if (rc) return rc;
    TN_LAUNCH_CHECK();
    return TN_OK;
}

extern "C" {

#ifndef C8_BF16_TU
// the bf16 entry points (dilconv_c8_bf16.hip)
int c8b_tn_c8_dilconv_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P, int K,
                          int d, int f, int stride, int pad, int So, int Po, int act, float prm);
int c8b_tn_c8_dilconv_dgrad(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K, int d, int f,
                            int stride, int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm);
int c8b_tn_c8_dilconv_wgrad(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P, int K,
                            int d, int f, int stride, int pad, int So, int Po);

// 1 if the dilated c8 kernels take a conv layer of this geometry (forward, both gradients; either element type)
int tn_c8_dilconv_supported(int N, int C, int S, int P, int K, int d, int f, int stride, int pad, int So, int Po) {
    return dc8_ok(N, C, S, P, K, d, f, stride, pad, So, Po) ? 1 : 0;
}
#else
// the general family's bf16 entry points (convg_c8_bf16.hip): d = 1 with a stride
int c8b_tn_c8_convg_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P, int K,
                        int f, int stride, int pad, int So, int Po, int act, float prm);
int c8b_tn_c8_convg_dgrad(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K, int f,
                          int stride, int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm);
int c8b_tn_c8_convg_wgrad(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P, int K,
                          int f, int stride, int pad, int So, int Po);
#endif

// y = act(dilconv(x, W) + b); every cell of y is written (pad cells and maps past K as +0)
int C8_API(tn_c8_dilconv_fwd)(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P,
                              int K, int d, int f, int stride, int pad, int So, int Po, int act, float prm) {
    C8_TO_BF16(tn_c8_dilconv_fwd, ctx, x, W, b, y, N, C, S, P, K, d, f, stride, pad, So, Po, act, prm);
    TN_REQUIRE(x && W && b && y && dc8_ok(N, C, S, P, K, d, f, stride, pad, So, Po),
               "tn_c8_dilconv_fwd: bad arguments " DC8_ARGS_FMT, DC8_ARGS);
    if (stride != 1) return C8_API(tn_c8_convg_fwd)(ctx, x, W, b, y, N, C, S, P, K, f, stride, pad, So, Po, act, prm);
    DC8 q{};
    q.src = static_cast<const uint4*>(x); q.out = static_cast<uint4*>(y); q.bias = b; q.act = act; q.prm = prm;
    q.Ss = S; q.Ps = P; q.PPs = (unsigned)P * P;
    q.So = So; q.Po = Po; q.PPo = (unsigned)Po * Po;
    q.f = f; q.d = d; q.off0 = -pad;
    return dc8_run<C8E, 0>(ctx, q, W, N, K, C);
}

// dx = (transposed dilconv of dz with W) * act'(prev_a) (prev_a NULL: none); every cell of dx is written (pad cells and
// maps past C as +0)
int C8_API(tn_c8_dilconv_dgrad)(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K, int d,
                                int f, int stride, int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm) {
    C8_TO_BF16(tn_c8_dilconv_dgrad, ctx, dz, W, dx, N, C, S, P, K, d, f, stride, pad, So, Po, prev_a, prev_act, prev_prm);
    TN_REQUIRE(dz && W && dx && dc8_ok(N, C, S, P, K, d, f, stride, pad, So, Po),
               "tn_c8_dilconv_dgrad: bad arguments " DC8_ARGS_FMT, DC8_ARGS);
    if (stride != 1)
        return C8_API(tn_c8_convg_dgrad)(ctx, dz, W, dx, N, C, S, P, K, f, stride, pad, So, Po, prev_a, prev_act, prev_prm);
    DC8 q{};
    q.src = static_cast<const uint4*>(dz); q.out = static_cast<uint4*>(dx); q.prev_a = static_cast<const uint4*>(prev_a);
    q.act = prev_act; q.prm = prev_prm;
    q.Ss = So; q.Ps = Po; q.PPs = (unsigned)Po * Po;
    q.So = S; q.Po = P; q.PPo = (unsigned)P * P;
    q.f = f; q.d = d; q.off0 = pad - (f - 1) * d;
    return dc8_run<C8E, 1>(ctx, q, W, N, K, C);
}

// dW (K, C, f, f), db (K) from x and dz; dz carries the gradient scale, the results do not.  OVERWRITE
int C8_API(tn_c8_dilconv_wgrad)(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P,
                                int K, int d, int f, int stride, int pad, int So, int Po) {
    C8_TO_BF16(tn_c8_dilconv_wgrad, ctx, x, dz, dW, db, N, C, S, P, K, d, f, stride, pad, So, Po);
    TN_REQUIRE(x && dz && dW && db && dc8_ok(N, C, S, P, K, d, f, stride, pad, So, Po),
               "tn_c8_dilconv_wgrad: bad arguments " DC8_ARGS_FMT, DC8_ARGS);
    if (stride != 1) return C8_API(tn_c8_convg_wgrad)(ctx, x, dz, dW, db, N, C, S, P, K, f, stride, pad, So, Po);
    DC8W q{};
    q.x = static_cast<const uint4*>(x); q.dz = static_cast<const uint4*>(dz);
    q.S = (unsigned)S; q.P = (unsigned)P; q.PP = (unsigned)P * P;
    q.So = (unsigned)So; q.SoSo = (unsigned)So * So; q.Po = (unsigned)Po; q.PPo = (unsigned)Po * Po;
    q.C8 = (unsigned)((C + 7) / 8); q.K8 = (unsigned)((K + 7) / 8); q.K = (unsigned)K; q.C = (unsigned)C;
    q.T = (unsigned)(f * f); q.CC = q.T * q.C8;
    q.f = f; q.d = d; q.pad = pad;
    q.npix = (unsigned long long)N * q.SoSo;
    const int CG = cdiv(q.CC, 8), KG = cdiv(q.K8, 8);
    const long long nt = (long long)((q.npix + 63) / 64);
    TN_REQUIRE(CG <= 65535 && KG <= 65535, "tn_c8_dilconv_wgrad: %d x %d x %d x %d weights: too large", K, C, f, f);
    q.ntiles = (unsigned)nt; q.nslab = gc_slabs(nt, (long long)CG * KG, 512);
    const size_t n = (size_t)K * C * q.T;
    int rc = tn_scratch_get(ctx, ((size_t)q.nslab * n + (size_t)q.nslab * K) * sizeof(float), &q.ws);
    if (rc) return rc;
    q.dbws = q.ws + (size_t)q.nslab * n;
    q.oscale = 1.f / ctx->grad_scale;
    dc8_wgrad_kernel<C8E><<<dim3(q.nslab, (unsigned)CG, (unsigned)KG), 256, 0, ctx->stream>>>(q);
    TN_LAUNCH_CHECK();
    return tn_red_wgrad(ctx, q.ws, dW, (uint32_t)n, q.nslab, (uint32_t)n, q.dbws, db, (uint32_t)K, q.nslab, (uint32_t)K);
}

}  // extern "C"
