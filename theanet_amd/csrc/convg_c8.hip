// DTYPE 'float16' / 'bfloat16' with CONV_SHAPES 'any': ConvLayers of ANY filter, mode and stride (theanet/layer/convpool.py:
// 54-72, Theano's conv2d(..., subsample=(stride, stride)) on an input padded by pad_lo / pad_hi) on the 16-bit-resident c8
// tensors of the conv stack ([N][ceil(C/8)][P][P][8] 16-bit values; x / dx: S x S maps at pitch P, y / dz: So x So maps at
// pitch Po).  The general route beside the two tuned families (conv_c8.hip: 3x3 'same'; conv1_c8.hip: 1x1): it takes what
// they refuse, straightforwardly.  Arithmetic: the stack's -- x and dz as stored, W rounded to the element type (nearest
// even) while it is arranged, exact products, fp32 accumulation on v_mfma_f32_32x32x16, bias / activation on the fp32 sums,
// one rounding when a tensor is stored; dz carries the gradient scale, the fp32 epilogue of the weight gradient removes it.
// Filter orientation: tn_conv2d_*'s -- y[n, k, i, j] = sum W[k, c, u, v] x[n, c, i s - pad + f-1-u, j s - pad + f-1-v].
//
// All three products are implicit GEMMs whose 16-byte cell (8 channels of a pixel) is one lane's operand of the 32x32x16
// MFMA, loaded straight from HBM (conv1_c8.hip's form: no halo, no LDS image tile):
//   forward / input gradient (c8_convg_kernel): the reduction runs over CELLS rc = tap * R8 + octet (tap = u f + v; R8: the
//     octets of the reduced maps: channels, forward; filters, input gradient), two cells to an MFMA step (lane half hi
//     takes cell 2 kk + hi).  With a single octet (C <= 8: a first layer) a step therefore holds two TAPS instead of a
//     half of zeros.  A = the weights as operand tiles (c8_convg_wt_kernel: rounded once per call into context scratch),
//     rows permuted as in conv1_c8.hip so that a lane's 16 accumulators are two whole output cells.  A lane owns one pixel
//     of the OUTPUT tensor's pitch x pitch plane, pad cells included (they are stored as +0); its cell of a step is the
//     tap-shifted pixel of the source, +0 where that lies outside the map, between the strides (input gradient) or past
//     the last reduction cell.  A wave owns two 32-pixel tiles and one 32-row tile.
//   weight gradient (c8_convg_wgrad_kernel): dW[k][c][u][v] = sum over output pixels, so both operands are transposed out
//     of the cell layout: a block stages 64 output pixels of up to 8 filter octets of dz and of up to 8 COLUMN cells
//     cc = tap * C8 + octet of x (each with its tap's shift) in LDS as they are and reads them back with the transposing
//     LDS read (ds_read_b64_tr_b16).  A wave takes 16 pixels of the staged tile, the four waves' sums are added in a fixed
//     order, a block writes one slab of partial sums in dW's own layout and the context's slab reduction (reduce.hip)
//     finishes dW and db.  db is summed from the stored dz cells as they are staged.  No atomics: one order of additions.
//     The slab count is a function of the geometry alone (no CU count): the same bits on every device.
// Every cell of y / dx is written by the op: pad cells, channels past K / C and input pixels no window touches as +0.
//
// Geometry: a pitch is the side itself (any size) or a power of two above it; `pad` is the low padding, the high one follows
// from So, hi = (So - 1) stride + f - pad - S (negative: the last window ends before the map does), and is consistent when
// pad <= f / 2 and -stride < hi <= pad: So windows fit and no more, no more padding than a 'same' layer's.
// Index range: every tensor has fewer than 2^32 cells, K C f f < 2^28, f and stride below 2^15.
#include <type_traits>

#include "c8_elem.h"

typedef short cg_short4 __attribute__((ext_vector_type(4)));
typedef short cg_short8 __attribute__((ext_vector_type(8)));

// row of a 32-row operand tile that MFMA row rho stands for (conv1_c8.hip, c81_row)
__host__ __device__ __forceinline__ int cg_row(int rho) {
    const int hi = (rho >> 2) & 1, r = (rho & 3) + 4 * (rho >> 3);
    return 8 * (2 * (r >> 3) + hi) + (r & 7);
}

// the weights as A operands: wt[((mt R16 + kk) 64 + lane) 8 + e] = W(row 32 mt + cg_row(lane & 31), reduction cell
// rc = 2 kk + (lane >> 5): tap rc / R8, reduced map 8 (rc % R8) + e), rounded; forward: row = filter, reduced = channel;
// dgrad: swapped.  Cells past the last one and maps past the last one are zero.
template <typename E>
__global__ __launch_bounds__(256) void c8_convg_wt_kernel(const float* __restrict__ W, typename E::T* __restrict__ wt, int K,
                                                         int C, int T, int R8, int R16, int dgrad, unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int e = idx & 7u, l = (idx >> 3) & 63u;
    const unsigned rest = idx >> 9;
    const int kk = rest % (unsigned)R16, mt = rest / (unsigned)R16;
    const int row = 32 * mt + cg_row(l & 31), rc = 2 * kk + (l >> 5);
    const int tap = rc / R8, red = 8 * (rc - tap * R8) + e;
    const int k = dgrad ? red : row, c = dgrad ? row : red;
    wt[idx] = (typename E::T)((tap < T && k < K && c < C) ? W[((size_t)k * C + c) * T + tap] : 0.f);
}

struct CGG {
    const uint4* src;        // the B operand's tensor: x (forward), dz (input gradient)
    const uint4* wt;         // arranged weights, gridDim.y row tiles
    uint4* out;
    const float* bias;       // forward
    const uint4* prev_a;     // input gradient: stored output of the layer below (NULL: none)
    unsigned Ss, Ps, PPs;    // source maps: side, pitch, pitch^2
    unsigned So, Po, PPo;    // output maps (of this product)
    unsigned long long units;          // N PPo
    unsigned R8, RC, R16;    // octets of the reduced maps, reduction cells (taps x octets), MFMA steps
    unsigned O, O8;          // output maps (filters / channels) and their octets
    int f, stride, off0;     // source coordinate of tap (f-1, f-1) at output pixel 0: -pad (forward), pad - (f-1) (dgrad)
    int act;
    float prm;
};

// MODE 0: forward; 1: input gradient, stride 1; 2: input gradient, any stride
template <typename E, int MODE>
__global__ __launch_bounds__(256) void c8_convg_kernel(CGG g) {
    typedef typename E::v8 v8;
    constexpr bool DGRAD = MODE >= 1;
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, hi = lane >> 5, j = lane & 31u;
    const unsigned mt = blockIdx.y;
    unsigned n[2], p[2];
    int by[2], bx[2];                // source coordinate of the tap with offset 0
    bool ok[2], pad[2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        const unsigned long long gi = (((unsigned long long)blockIdx.x * 4 + wave) * 2 + pt) * 32 + j;
        ok[pt] = gi < g.units;
        const unsigned g_ = ok[pt] ? (unsigned)gi : 0u;
        n[pt] = g_ / g.PPo; p[pt] = g_ - n[pt] * g.PPo;
        const unsigned h = p[pt] / g.Po, w = p[pt] - h * g.Po;
        pad[pt] = h >= g.So || w >= g.So;
        by[pt] = (DGRAD ? (int)h : (int)h * g.stride) + g.off0;
        bx[pt] = (DGRAD ? (int)w : (int)w * g.stride) + g.off0;
    }
    f32x16 acc[2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[pt][r] = 0.f;

    // this half wave's reduction cell rc = 2 kk + hi as (octet, tap row u, tap column v), stepped by two cells
    unsigned rc = hi;
    int u = (int)(rc / g.R8) / g.f, v = (int)(rc / g.R8) % g.f;
    unsigned oct = rc % g.R8;
    const uint4* wp_ = g.wt + (size_t)mt * g.R16 * 64 + lane;
    for (unsigned kk = 0; kk < g.R16; ++kk, rc += 2) {
        // offset of the tap on the gather side: f-1-u (forward: the flip), u (input gradient)
        const int du = DGRAD ? u : g.f - 1 - u, dv = DGRAD ? v : g.f - 1 - v;
        v8 b[2];
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            uint4 val = make_uint4(0u, 0u, 0u, 0u);
            int sy = by[pt] + du, sx = bx[pt] + dv;
            bool in = ok[pt] && !pad[pt] && rc < g.RC && sy >= 0 && sx >= 0;
            if (MODE == 2) {
                const int qy = sy / g.stride, qx = sx / g.stride;
                in = in && qy * g.stride == sy && qx * g.stride == sx;
                sy = qy; sx = qx;
            }
            if (in && sy < (int)g.Ss && sx < (int)g.Ss)
                val = g.src[(n[pt] * g.R8 + oct) * g.PPs + (unsigned)sy * g.Ps + (unsigned)sx];
            b[pt] = __builtin_bit_cast(v8, val);
        }
        const v8 a = __builtin_bit_cast(v8, wp_[(size_t)kk * 64]);
        acc[0] = E::mfma(a, b[0], acc[0]);
        acc[1] = E::mfma(a, b[1], acc[1]);
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (++oct == g.R8) {
                oct = 0;
                if (++v == g.f) { v = 0; ++u; }
            }
    }

    // ---- epilogue: accumulators 8 h .. 8 h + 7 of a lane are octet 4 mt + 2 h + hi of its pixel (conv1_c8.hip)
    auto epilogue = [&](auto LKc) __attribute__((always_inline)) {
        constexpr bool LK = decltype(LKc)::value;
        const float prm = g.prm, tie = prm > 0.f ? 1.f + prm : 0.f;
        auto actf = [&](float z) __attribute__((always_inline)) {
            return LK ? fmaxf(0.f, z) + fminf(0.f, z) * prm : tn_act_fwd(z, g.act, prm);
        };
        auto actg = [&](float a) __attribute__((always_inline)) {
            return LK ? (a > 0.f ? 1.f : (a < 0.f ? prm : tie)) : tn_act_grad_from_out(a, g.act, prm);
        };
        (void)actf; (void)actg; (void)tie;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned o8 = 4 * mt + 2 * h + hi;
            if (o8 >= g.O8) continue;
            const int nv = (int)g.O - 8 * (int)o8;            // maps of this octet inside O
            float bv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) bv[e] = (!DGRAD && e < nv) ? g.bias[8 * o8 + e] : 0.f;
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                if (!ok[pt]) continue;
                const unsigned o = (n[pt] * g.O8 + o8) * g.PPo + p[pt];
                const bool deriv = DGRAD && g.prev_a != nullptr && !pad[pt];
                v8 pa = __builtin_bit_cast(v8, make_uint4(0u, 0u, 0u, 0u));
                if (deriv) pa = __builtin_bit_cast(v8, g.prev_a[o]);
                v8 c8;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float val = acc[pt][8 * h + e];
                    if (DGRAD) {
                        if (deriv) val *= actg((float)pa[e]);
                    } else {
                        val = actf(val + bv[e]);
                    }
                    c8[e] = (typename E::T)((e < nv && !pad[pt]) ? val : 0.f);
                }
                g.out[o] = __builtin_bit_cast(uint4, c8);
            }
        }
    };
    if (g.act == TN_ACT_LEAKY) epilogue(std::true_type{});
    else epilogue(std::false_type{});
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------
struct CGW {
    const uint4* x;
    const uint4* dz;
    float* ws;               // [slab][K][C][f][f] partial dW (scale removed)
    float* dbws;             // [slab][K]
    unsigned S, P, PP, So, SoSo, Po, PPo, C, C8, K, K8, T, CC, ntiles, nslab;
    int f, stride, pad;
    unsigned long long npix;           // N So So
    float oscale;
};

// MFMA operand (32 rows x 16 pixels) of row tile `tile` out of cells staged [cell][64 pixels] (conv1_c8.hip, c81_tr_operand)
template <typename E>
__device__ __forceinline__ typename E::v8 cg_tr_operand(const char* s, int tile, int pix0, int lane) {
    const int gl = lane >> 4, i = lane & 15;
    const int oct = 4 * tile + 2 * (gl & 1) + ((i & 3) >> 1), pix = pix0 + 8 * (gl >> 1) + (i >> 2);
    const char* a = s + (oct * 64 + pix) * 16 + 8 * (i & 1);
    const cg_short4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) cg_short4*)a);
    const cg_short4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) cg_short4*)(a + 64));
    const cg_short8 r = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
    return __builtin_bit_cast(typename E::v8, r);
}

// grid (slabs, groups of 8 column cells, groups of 8 filter octets)
template <typename E>
__global__ __launch_bounds__(256) void c8_convg_wgrad_kernel(CGW g) {
    typedef typename E::v8 v8;
    __shared__ __attribute__((aligned(16))) char smem[16384];     // x cells [8][64], dz cells [8][64]; then the waves' sums
    char* const sx = smem;
    char* const sd = smem + 8192;
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, hi = lane >> 5;
    const unsigned slab = blockIdx.x, cc0 = 8 * blockIdx.y, ko0 = 8 * blockIdx.z;
    const unsigned pl = t & 63u;
    // this wave's two column cells: octet and source offset of the tap
    unsigned xo[2];
    int dy[2], dx[2];
    bool xlive[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const unsigned cc = cc0 + wave + 4 * jj;
        xlive[jj] = cc < g.CC;
        const unsigned tap = xlive[jj] ? cc / g.C8 : 0u;
        xo[jj] = xlive[jj] ? cc - tap * g.C8 : 0u;
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
                xr[jj] = g.x[(n * g.C8 + xo[jj]) * g.PP + (unsigned)sy * g.P + (unsigned)sx_];
            if (valid && ko0 + ol < g.K8) dr[jj] = g.dz[(n * g.K8 + ko0 + ol) * g.PPo + oh * g.Po + ow];
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
            a[i] = cg_tr_operand<E>(sd, i, 16 * (int)wave, (int)lane);
            b[i] = cg_tr_operand<E>(sx, i, 16 * (int)wave, (int)lane);
        }
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ft][ct] = E::mfma(a[ft], b[ct], acc[ft][ct]);
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
static long long cg_cells(int N, int C, int S, int P) {
    if (N <= 0 || C <= 0 || S <= 0 || P < S || (P != S && (P & (P - 1)))) return -1;
    const long long cells = (long long)N * ((C + 7) / 8) * P * P;
    return cells < (1ll << 32) ? cells : -1;
}

static bool cg_ok(int N, int C, int S, int P, int K, int f, int stride, int pad, int So, int Po) {
    if (f < 1 || stride < 1 || pad < 0 || f >= (1 << 15) || stride >= (1 << 15) || So < 1) return false;
    if (cg_cells(N, C, S, P) < 0 || cg_cells(N, K, So, Po) < 0) return false;
    // the high padding follows from So (negative: the last window ends before the map does, another one would not fit);
    // no more padding than a 'same' layer's: low at most f / 2, high at most the low
    const long long hi = (long long)(So - 1) * stride + f - pad - S;
    if (pad > f / 2 || hi > pad || hi <= -(long long)stride) return false;
    return (long long)K * C * f * f < (1ll << 28);
}

// What a call takes: tn_c8_convg_plan reports it.
struct cg_plan {
    int kernel, leaky, r8, steps, ragged_red, rows, blocks, ragged_out;
};

// op 0 forward, 1 input gradient: c8_convg_kernel<E, MODE> on grid (blocks of 256 output pixels, 32-row tiles)
static cg_plan cg_choose(int op, int N, int C, int S, int P, int K, int f, int stride, int So, int Po, int act) {
    cg_plan pl;
    const int O = op ? C : K, R = op ? K : C, R8 = (R + 7) / 8, RC = f * f * R8;
    const long long units = (long long)N * (op ? P : Po) * (op ? P : Po);
    (void)S; (void)So;
    pl.kernel = op ? (stride == 1 ? 1 : 2) : 0;
    pl.leaky = act == TN_ACT_LEAKY;
    pl.r8 = R8;
    pl.steps = (RC + 1) / 2;
    pl.ragged_red = (RC & 1) | ((R & 7) ? 2 : 0);       // bit 0: the last step's second cell is past the end; 1: ragged octet
    pl.rows = cdiv(O, 32);
    pl.blocks = (int)((units + 255) / 256);
    pl.ragged_out = (units % 256 != 0) | ((O % 32) ? 2 : 0);
    return pl;
}

// the weight gradient: c8_convg_wgrad_kernel<E> on grid (slabs, column-cell groups, filter-octet groups).  Slabs: 512
// blocks over all groups (two per CU of a 256-CU device, but a constant: the order of additions is the geometry's alone;
// 2048 blocks made the mnist step 2 % slower), at most one per pixel tile
static cg_plan cg_choose_wgrad(int N, int C, int K, int f, int So, unsigned* ntiles, unsigned* nslab) {
    cg_plan pl;
    const long long npix = (long long)N * So * So;
    const int CC = f * f * ((C + 7) / 8), CG = cdiv(CC, 8), KG = cdiv((K + 7) / 8, 8);
    const long long nt = (npix + 63) / 64, want = cdiv(512, (long long)CG * KG);
    const long long ns = want < 1 ? 1 : (want > nt ? nt : want);
    *ntiles = (unsigned)nt; *nslab = (unsigned)ns;
    pl.kernel = 3; pl.leaky = 0;
    pl.r8 = (C + 7) / 8;
    pl.steps = (int)nt;
    pl.ragged_red = npix % 64 != 0;
    pl.rows = CG * KG;
    pl.blocks = (int)ns;
    pl.ragged_out = (CC % 8 != 0) | ((K % 64) ? 2 : 0);
    return pl;
}

#define CG_ARGS_FMT "(N %d, %d maps of %d pixels at pitch %d -> %d maps of %d pixels at pitch %d, filter %d stride %d pad_lo %d)"
#define CG_ARGS N, C, S, P, K, So, Po, f, stride, pad

template <typename E, int MODE>
static int cg_run(tn_ctx* ctx, CGG& g, const float* W, int K, int C, int f) {
    const int dgrad = MODE >= 1 ? 1 : 0;
    const int O = dgrad ? C : K, R = dgrad ? K : C, MT = cdiv(O, 32);
    g.O = (unsigned)O; g.O8 = (unsigned)((O + 7) / 8); g.R8 = (unsigned)((R + 7) / 8);
    g.RC = (unsigned)(f * f) * g.R8; g.R16 = (g.RC + 1) / 2;
    const size_t total = (size_t)MT * g.R16 * 512;
    TN_REQUIRE(total < (1ull << 31) && MT <= 65535, "c8 convg: %d x %d x %d x %d weights: too large", K, C, f, f);
    float* wt;
    int rc = tn_scratch_get(ctx, total * sizeof(typename E::T), &wt);
    if (rc) return rc;
    c8_convg_wt_kernel<E><<<cdiv((long long)total, 256), 256, 0, ctx->stream>>>(W, reinterpret_cast<typename E::T*>(wt), K, C,
                                                                              f * f, (int)g.R8, (int)g.R16, dgrad,
                                                                              (unsigned)total);
    TN_LAUNCH_CHECK();
    g.wt = reinterpret_cast<const uint4*>(wt);
    const dim3 grid((unsigned)((g.units + 255) / 256), (unsigned)MT);
    c8_convg_kernel<E, MODE><<<grid, 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

extern "C" {

#ifndef C8_BF16_TU
// the bf16 entry points (convg_c8_bf16.hip)
int c8b_tn_c8_convg_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P, int K,
                        int f, int stride, int pad, int So, int Po, int act, float prm);
int c8b_tn_c8_convg_dgrad(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K, int f,
                          int stride, int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm);
int c8b_tn_c8_convg_wgrad(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P, int K,
                          int f, int stride, int pad, int So, int Po);

// 1 if the general c8 kernels take a conv layer of this geometry (forward, both gradients; either element type)
int tn_c8_convg_supported(int N, int C, int S, int P, int K, int f, int stride, int pad, int So, int Po) {
    return cg_ok(N, C, S, P, K, f, stride, pad, So, Po) ? 1 : 0;
}

// op 0: tn_c8_convg_fwd, 1: tn_c8_convg_dgrad, 2: tn_c8_convg_wgrad.  out: kernel (0 forward, 1 input gradient stride 1,
// 2 input gradient strided, 3 weight gradient), leaky-ReLU epilogue, octets of the reduced maps (wgrad: of the channels),
// reduction steps (wgrad: pixel tiles), ragged reduction tail (bit 0: half a step past the last cell, bit 1: a ragged
// octet; wgrad: a partial last pixel tile), row tiles (wgrad: column groups x filter groups), pixel blocks (wgrad: slabs),
// ragged output (bit 0: a partial last pixel block / column group, bit 1: a partial row tile / filter group).  No device.
int tn_c8_convg_plan(int op, int N, int C, int S, int P, int K, int f, int stride, int pad, int So, int Po, int act, float prm,
                     int* out, int nout) {
    (void)prm;
    if (op < 0 || op > 2 || !cg_ok(N, C, S, P, K, f, stride, pad, So, Po) || (nout > 0 && !out)) return TN_E_ARG;
    unsigned nt, ns;
    const cg_plan pl = op == 2 ? cg_choose_wgrad(N, C, K, f, So, &nt, &ns) : cg_choose(op, N, C, S, P, K, f, stride, So, Po, act);
    const int v[8] = {pl.kernel, pl.leaky, pl.r8, pl.steps, pl.ragged_red, pl.rows, pl.blocks, pl.ragged_out};
    for (int k = 0; k < 8 && k < nout; ++k) out[k] = v[k];
    return 8;
}
#endif

// y = act(conv(x, W) + b); every cell of y is written (pad cells and channels past K as +0)
int C8_API(tn_c8_convg_fwd)(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P,
                            int K, int f, int stride, int pad, int So, int Po, int act, float prm) {
    C8_TO_BF16(tn_c8_convg_fwd, ctx, x, W, b, y, N, C, S, P, K, f, stride, pad, So, Po, act, prm);
    TN_REQUIRE(x && W && b && y && cg_ok(N, C, S, P, K, f, stride, pad, So, Po), "tn_c8_convg_fwd: bad arguments " CG_ARGS_FMT,
               CG_ARGS);
    CGG g{};
    g.src = static_cast<const uint4*>(x); g.out = static_cast<uint4*>(y); g.bias = b; g.act = act; g.prm = prm;
    g.Ss = (unsigned)S; g.Ps = (unsigned)P; g.PPs = (unsigned)P * P;
    g.So = (unsigned)So; g.Po = (unsigned)Po; g.PPo = (unsigned)Po * Po;
    g.units = (unsigned long long)N * g.PPo;
    g.f = f; g.stride = stride; g.off0 = -pad;
    return cg_run<C8E, 0>(ctx, g, W, K, C, f);
}

// dx = (transposed conv of dz with W) * act'(prev_a) (prev_a NULL: none); every cell of dx is written (pad cells, channels
// past C and input pixels no window touches as +0)
int C8_API(tn_c8_convg_dgrad)(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K, int f,
                              int stride, int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm) {
    C8_TO_BF16(tn_c8_convg_dgrad, ctx, dz, W, dx, N, C, S, P, K, f, stride, pad, So, Po, prev_a, prev_act, prev_prm);
    TN_REQUIRE(dz && W && dx && cg_ok(N, C, S, P, K, f, stride, pad, So, Po), "tn_c8_convg_dgrad: bad arguments " CG_ARGS_FMT,
               CG_ARGS);
    CGG g{};
    g.src = static_cast<const uint4*>(dz); g.out = static_cast<uint4*>(dx); g.prev_a = static_cast<const uint4*>(prev_a);
    g.act = prev_act; g.prm = prev_prm;
    g.Ss = (unsigned)So; g.Ps = (unsigned)Po; g.PPs = (unsigned)Po * Po;
    g.So = (unsigned)S; g.Po = (unsigned)P; g.PPo = (unsigned)P * P;
    g.units = (unsigned long long)N * g.PPo;
    g.f = f; g.stride = stride; g.off0 = pad - (f - 1);
    return stride == 1 ? cg_run<C8E, 1>(ctx, g, W, K, C, f) : cg_run<C8E, 2>(ctx, g, W, K, C, f);
}

// dW (K, C, f, f), db (K) from x and dz; dz carries the gradient scale, the results do not.  OVERWRITE
int C8_API(tn_c8_convg_wgrad)(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P,
                              int K, int f, int stride, int pad, int So, int Po) {
    C8_TO_BF16(tn_c8_convg_wgrad, ctx, x, dz, dW, db, N, C, S, P, K, f, stride, pad, So, Po);
    TN_REQUIRE(x && dz && dW && db && cg_ok(N, C, S, P, K, f, stride, pad, So, Po),
               "tn_c8_convg_wgrad: bad arguments " CG_ARGS_FMT, CG_ARGS);
    CGW g{};
    g.x = static_cast<const uint4*>(x); g.dz = static_cast<const uint4*>(dz);
    g.S = (unsigned)S; g.P = (unsigned)P; g.PP = (unsigned)P * P;
    g.So = (unsigned)So; g.SoSo = (unsigned)So * So; g.Po = (unsigned)Po; g.PPo = (unsigned)Po * Po;
    g.C = (unsigned)C; g.C8 = (unsigned)((C + 7) / 8); g.K = (unsigned)K; g.K8 = (unsigned)((K + 7) / 8);
    g.T = (unsigned)(f * f); g.CC = g.T * g.C8;
    g.f = f; g.stride = stride; g.pad = pad;
    g.npix = (unsigned long long)N * g.SoSo;
    cg_choose_wgrad(N, C, K, f, So, &g.ntiles, &g.nslab);
    const int CG = cdiv(g.CC, 8), KG = cdiv(g.K8, 8);
    TN_REQUIRE(CG <= 65535 && KG <= 65535, "tn_c8_convg_wgrad: %d x %d x %d x %d weights: too large", K, C, f, f);
    const size_t n = (size_t)K * C * g.T;
    int rc = tn_scratch_get(ctx, ((size_t)g.nslab * n + (size_t)g.nslab * K) * sizeof(float), &g.ws);
    if (rc) return rc;
    g.dbws = g.ws + (size_t)g.nslab * n;
    g.oscale = 1.f / ctx->grad_scale;
    const dim3 grid(g.nslab, (unsigned)CG, (unsigned)KG);
    c8_convg_wgrad_kernel<C8E><<<grid, 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return tn_red_wgrad(ctx, g.ws, dW, (uint32_t)n, g.nslab, (uint32_t)n, g.dbws, db, (uint32_t)K, g.nslab, (uint32_t)K);
}

}  // extern "C"
