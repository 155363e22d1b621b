// DTYPE 'float16' / 'bfloat16': 1x1 stride-1 ConvLayers (theanet/layer/convpool.py:54-72 with filter_sz 1: "mlpconv",
// network-in-network) on the 16-bit-resident c8 tensors of the conv stack ([N][ceil(C/8)][P][P][8] 16-bit values, S x S
// maps at pitch P).  Arithmetic: that of the 3x3 kernels (conv_c8.hip) -- operands rounded to the element type (nearest
// even), exact products, fp32 accumulation on the matrix core, bias / activation / 2x2 max-pool on the fp32 sums, one
// rounding when a tensor is stored; gradients carry the gradient scale, the fp32 epilogue of the weight gradient removes it.
//
// A 1x1 product is a plain matrix product over the channels of one pixel, and the 16-byte cell (8 channels of a pixel) IS
// the per-lane B operand of v_mfma_f32_32x32x16: lane (pixel j, half hi) of step kk loads the cell of octet 2 kk + hi of
// its pixel straight from HBM, 32 consecutive cells per half wave.  No halo, no LDS image tile.
//   forward / input gradient (c8_conv1_kernel): A = the weights as operand tiles (c8_conv1_wt_kernel: rounded once per
//     call into context scratch; rows = filters, forward, or channels, input gradient).  The rows of a 32-row tile are
//     PERMUTED so that the 16 accumulators of a lane -- MFMA rows (r & 3) + 8 (r >> 2) + 4 hi -- are two whole output cells
//     (octets 4 m + hi and 4 m + 2 + hi): the epilogue stores 16-byte cells with no cross-lane exchange.  A wave owns two
//     32-pixel tiles and KT (1 / 2 / 4) row tiles.  Pooled forward: the four pixels of a pooling window sit in four
//     adjacent lanes, the window maximum and the tie bits are two lane exchanges each.  Pooled input gradient: dz is formed
//     from the pooled gradient and the block's mask while loading (bit set ? pooled gradient : 0), never written.
//   weight gradient (c8_conv1_wgrad_kernel): dW[k][c] = sum over pixels, so BOTH operands are transposed out of the cell
//     layout: a block stages 64 pixels of up to 8 octets of x and of dz in LDS as they are and reads them back with the
//     transposing LDS read (ds_read_b64_tr_b16: a 16-lane group receives 16 channels x 4 pixels; tools/probe/tr16.hip).
//     A wave takes 16 pixels of the staged tile, the four waves' sums are added in a fixed order, a block writes one slab
//     of partial sums and the context's slab reduction (reduce.hip) finishes dW and db.  db is summed from the stored dz
//     cells as they are staged.  No atomics: one order of additions, the same bits every run.
// Pad cells (S < P) and channels past K (forward) / C (input gradient) are written as zero by the ops themselves.
#include <type_traits>

#include "c8_elem.h"

typedef short c81_short4 __attribute__((ext_vector_type(4)));
typedef short c81_short8 __attribute__((ext_vector_type(8)));

// row of a 32-row operand tile that MFMA row rho stands for (see above): lane half hi = bit 2 of rho, accumulator
// r = (rho & 3) + 4 (rho >> 3); accumulators 0-7 / 8-15 are octets hi / 2 + hi of the tile
__host__ __device__ __forceinline__ int c81_row(int rho) {
    const int hi = (rho >> 2) & 1, r = (rho & 3) + 4 * (rho >> 3);
    return 8 * (2 * (r >> 3) + hi) + (r & 7);
}

// the weights as A operands: wt[((mt R16 + kk) 64 + lane) 8 + e] = W(row 32 mt + c81_row(lane & 31),
// reduction index 16 kk + 8 (lane >> 5) + e), rounded; forward: row = filter, reduction = channel; dgrad: swapped
template <typename E>
__global__ __launch_bounds__(256) void c8_conv1_wt_kernel(const float* __restrict__ W, typename E::T* __restrict__ wt, int K,
                                                         int C, int R16, int dgrad, unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int e = idx & 7u, l = (idx >> 3) & 63u;
    const unsigned rest = idx >> 9;
    const int kk = rest % (unsigned)R16, mt = rest / (unsigned)R16;
    const int row = 32 * mt + c81_row(l & 31), red = 16 * kk + 8 * (l >> 5) + e;
    const int k = dgrad ? red : row, c = dgrad ? row : red;
    wt[idx] = (typename E::T)((k < K && c < C) ? W[(size_t)k * C + c] : 0.f);
}

// dz cell of a pooled block at window element sh (conv_c8.hip c8_pool_cell): the pooled gradient where bit sh of the
// channel's mask byte is set, zero elsewhere
__device__ __forceinline__ uint4 c81_pool_cell(const uint4 g8, const uint2 m8, int sh) {
    const unsigned b0 = (m8.x >> sh) & 0x01010101u, b1 = (m8.y >> sh) & 0x01010101u;
    const unsigned k0 = __umul24(__builtin_amdgcn_perm(0u, b0, 0x0c010c00u), 0xffffu);
    const unsigned k1 = __umul24(__builtin_amdgcn_perm(0u, b0, 0x0c030c02u), 0xffffu);
    const unsigned k2 = __umul24(__builtin_amdgcn_perm(0u, b1, 0x0c010c00u), 0xffffu);
    const unsigned k3 = __umul24(__builtin_amdgcn_perm(0u, b1, 0x0c030c02u), 0xffffu);
    return make_uint4(g8.x & k0, g8.y & k1, g8.z & k2, g8.w & k3);
}

struct C81G {
    const uint4* x;          // the B operand's tensor: x (forward), dz or the pooled gradient (input gradient)
    const uint4* wt;         // arranged weights, gridDim.y * KT row tiles
    uint4* out;
    const float* bias;       // forward
    const uint4* prev_a;     // input gradient: stored output of the block below (NULL: none)
    uint2* mask_out;         // MODE 1 (may be NULL)
    const uint2* mask_in;    // MODE 3
    unsigned N, S, P, PP, Ph, QQ;      // PP = P P; Ph = P / 2, QQ = Ph Ph (pooled forms)
    unsigned long long units;          // pixels (N PP), MODE 1: pooling windows (N QQ)
    unsigned R8, R16;        // octets / 16-steps of the reduction dimension
    unsigned O, O8;          // output rows (filters / channels) and their octets
    int act;
    float prm;
};

// MODE 0: forward; 1: forward + 2x2 max-pool + mask; 2: input gradient; 3: input gradient of a pooled block
template <typename E, int MODE, int KT>
__global__ __launch_bounds__(256) void c8_conv1_kernel(C81G g) {
    typedef typename E::v8 v8;
    constexpr bool POOL = MODE == 1, DGRAD = MODE >= 2, POOLED = MODE == 3;
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, hi = lane >> 5, j = lane & 31u;
    const unsigned mt0 = blockIdx.y * KT;
    unsigned n[2], p[2], q[2];       // image, pixel of the plane, (pooled forms) cell of the pooled plane
    int sh[2];
    bool ok[2], pad[2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        const unsigned long long T = ((unsigned long long)blockIdx.x * 4 + wave) * 2 + pt;
        if (POOL) {
            const unsigned long long wq = T * 8 + (j >> 2);
            ok[pt] = wq < g.units;
            const unsigned w_ = ok[pt] ? (unsigned)wq : 0u, e = j & 3u;
            n[pt] = w_ / g.QQ; q[pt] = w_ - n[pt] * g.QQ;
            const unsigned hp = q[pt] / g.Ph, wp = q[pt] - hp * g.Ph;
            p[pt] = (2 * hp + (e >> 1)) * g.P + 2 * wp + (e & 1u);
            pad[pt] = 2 * hp >= g.S || 2 * wp >= g.S;
            sh[pt] = (int)e;
        } else {
            const unsigned long long gi = T * 32 + j;
            ok[pt] = gi < g.units;
            const unsigned g_ = ok[pt] ? (unsigned)gi : 0u;
            n[pt] = g_ / g.PP; p[pt] = g_ - n[pt] * g.PP;
            const unsigned h = p[pt] / g.P, w = p[pt] - h * g.P;
            pad[pt] = h >= g.S || w >= g.S;
            q[pt] = (h >> 1) * g.Ph + (w >> 1);
            sh[pt] = (int)(2 * (h & 1u) + (w & 1u));
        }
    }
    f32x16 acc[KT][2];
#pragma unroll
    for (int m = 0; m < KT; ++m)
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][pt][r] = 0.f;

    const uint4* wp_ = g.wt + (size_t)mt0 * g.R16 * 64 + lane;
#pragma unroll 2
    for (unsigned kk = 0; kk < g.R16; ++kk) {
        const unsigned oct = 2 * kk + hi;
        v8 b[2];
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (ok[pt] && oct < g.R8) {
                if (POOLED) {
                    const unsigned i = (n[pt] * g.R8 + oct) * g.QQ + q[pt];
                    v = c81_pool_cell(g.x[i], g.mask_in[i], sh[pt]);
                } else {
                    v = g.x[(n[pt] * g.R8 + oct) * g.PP + p[pt]];
                }
            }
            b[pt] = __builtin_bit_cast(v8, v);
        }
#pragma unroll
        for (int m = 0; m < KT; ++m) {
            const v8 a = __builtin_bit_cast(v8, wp_[((size_t)m * g.R16 + kk) * 64]);
            acc[m][0] = E::mfma(a, b[0], acc[m][0]);
            acc[m][1] = E::mfma(a, b[1], acc[m][1]);
        }
    }

    // ---- epilogue: accumulators 8 h .. 8 h + 7 of a lane are octet 4 (mt0 + m) + 2 h + hi of its pixel.  (LK: the
    // leaky-ReLU family as straight-line code, the same expressions as tn_act_fwd / tn_act_grad_from_out)
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
        for (int m = 0; m < KT; ++m)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned oct = 4 * (mt0 + m) + 2 * h + hi;
                const bool live = oct < g.O8;
                const unsigned octc = live ? oct : 0u;
                const int nv = (int)g.O - 8 * (int)octc;            // rows of this octet inside O
                if (DGRAD) {
#pragma unroll
                    for (int pt = 0; pt < 2; ++pt) {
                        const unsigned o = (n[pt] * g.O8 + octc) * g.PP + p[pt];
                        v8 pa = __builtin_bit_cast(v8, make_uint4(0u, 0u, 0u, 0u));
                        if (g.prev_a && ok[pt] && live) pa = __builtin_bit_cast(v8, g.prev_a[o]);
                        v8 o8;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float v = acc[m][pt][8 * h + e];
                            if (g.prev_a && ok[pt] && live) v *= actg((float)pa[e]);
                            o8[e] = (typename E::T)((e < nv && !pad[pt]) ? v : 0.f);
                        }
                        if (ok[pt] && live) g.out[o] = __builtin_bit_cast(uint4, o8);
                    }
                    continue;
                }
                float bv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) bv[e] = (live && e < nv) ? g.bias[8 * octc + e] : 0.f;
                if (!POOL) {
#pragma unroll
                    for (int pt = 0; pt < 2; ++pt) {
                        v8 o8;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float v = actf(acc[m][pt][8 * h + e] + bv[e]);
                            o8[e] = (typename E::T)((e < nv && !pad[pt]) ? v : 0.f);
                        }
                        if (ok[pt] && live) g.out[(n[pt] * g.O8 + octc) * g.PP + p[pt]] = __builtin_bit_cast(uint4, o8);
                    }
                } else {
                    // the window's four pixels are lanes 4 i .. 4 i + 3 (element 2 di + dj = lane & 3): every lane of the wave
                    // takes part in the exchanges, the window's first lane stores
#pragma unroll
                    for (int pt = 0; pt < 2; ++pt) {
                        v8 o8;
                        unsigned mb[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float a = actf(acc[m][pt][8 * h + e] + bv[e]);
                            float mx = fmaxf(a, __shfl_xor(a, 1));
                            mx = fmaxf(mx, __shfl_xor(mx, 2));
                            unsigned bits = a == mx ? (1u << sh[pt]) : 0u;
                            bits |= (unsigned)__shfl_xor((int)bits, 1);
                            bits |= (unsigned)__shfl_xor((int)bits, 2);
                            bits |= (mx > 0.f ? 16u : 0u) | (mx < 0.f ? 32u : 0u);
                            const bool keep = e < nv && !pad[pt];
                            o8[e] = (typename E::T)(keep ? mx : 0.f);
                            mb[e] = keep ? bits : 0u;
                        }
                        if (ok[pt] && live && sh[pt] == 0) {
                            const unsigned o = (n[pt] * g.O8 + octc) * g.QQ + q[pt];
                            g.out[o] = __builtin_bit_cast(uint4, o8);
                            if (g.mask_out) {
                                uint2 m2;
                                m2.x = mb[0] | (mb[1] << 8) | (mb[2] << 16) | (mb[3] << 24);
                                m2.y = mb[4] | (mb[5] << 8) | (mb[6] << 16) | (mb[7] << 24);
                                g.mask_out[o] = m2;
                            }
                        }
                    }
                }
            }
    };
    if (g.act == TN_ACT_LEAKY) epilogue(std::true_type{});
    else epilogue(std::false_type{});
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------
struct C81W {
    const uint4* x;
    const uint4* dz;         // POOL: the pooled gradient
    const uint2* mask;       // POOL
    float* ws;               // [slab][K][C] partial dW (scale removed)
    float* dbws;             // [slab][K]
    unsigned N, P, PP, Ph, QQ, C, C8, K, K8, ntiles, nslab;
    unsigned long long npix;
    float oscale;
};

// MFMA operand (32 rows x 16 pixels, lane: row lane & 31, pixels 8 (lane >> 5) .. + 7) of row tile `tile` out of cells
// staged [octet][64 pixels]: a 16-lane group points at 4 pixels x 16 channels (two octets) and receives them transposed
template <typename E>
__device__ __forceinline__ typename E::v8 c81_tr_operand(const char* s, int tile, int pix0, int lane) {
    const int gl = lane >> 4, i = lane & 15;
    const int oct = 4 * tile + 2 * (gl & 1) + ((i & 3) >> 1), pix = pix0 + 8 * (gl >> 1) + (i >> 2);
    const char* a = s + (oct * 64 + pix) * 16 + 8 * (i & 1);
    const c81_short4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) c81_short4*)a);
    const c81_short4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) c81_short4*)(a + 64));
    const c81_short8 r = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
    return __builtin_bit_cast(typename E::v8, r);
}

// grid (slabs, 64-channel groups, 64-filter groups)
template <typename E, bool POOL>
__global__ __launch_bounds__(256) void c8_conv1_wgrad_kernel(C81W g) {
    typedef typename E::v8 v8;
    __shared__ __attribute__((aligned(16))) char smem[16384];     // x cells [8][64], dz cells [8][64]; then the waves' sums
    char* const sx = smem;
    char* const sd = smem + 8192;
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, hi = lane >> 5;
    const unsigned slab = blockIdx.x, co0 = 8 * blockIdx.y, ko0 = 8 * blockIdx.z;
    const unsigned pl = t & 63u;
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
    uint2 mr[2];
    int shr = 0;
    auto gload = [&](unsigned tile) __attribute__((always_inline)) {
        const unsigned long long gi = (unsigned long long)tile * 64 + pl;
        const bool valid = gi < g.npix;
        const unsigned g_ = valid ? (unsigned)gi : 0u;
        const unsigned n = g_ / g.PP, p = g_ - n * g.PP;
        unsigned q = 0;
        if (POOL) {
            const unsigned h = p / g.P, w = p - h * g.P;
            q = (h >> 1) * g.Ph + (w >> 1);
            shr = (int)(2 * (h & 1u) + (w & 1u));
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const unsigned ol = wave + 4 * jj;
            xr[jj] = make_uint4(0u, 0u, 0u, 0u);
            dr[jj] = make_uint4(0u, 0u, 0u, 0u);
            mr[jj] = make_uint2(0u, 0u);
            if (valid && co0 + ol < g.C8) xr[jj] = g.x[(n * g.C8 + co0 + ol) * g.PP + p];
            if (valid && ko0 + ol < g.K8) {
                if (POOL) {
                    const unsigned i = (n * g.K8 + ko0 + ol) * g.QQ + q;
                    dr[jj] = g.dz[i];
                    mr[jj] = g.mask[i];
                } else {
                    dr[jj] = g.dz[(n * g.K8 + ko0 + ol) * g.PP + p];
                }
            }
        }
    };

    unsigned tile = slab;
    if (tile < g.ntiles) gload(tile);
    for (; tile < g.ntiles; tile += g.nslab) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const unsigned ol = wave + 4 * jj;
            const uint4 d4 = POOL ? c81_pool_cell(dr[jj], mr[jj], shr) : dr[jj];
            *reinterpret_cast<uint4*>(sx + (ol * 64 + pl) * 16) = xr[jj];
            *reinterpret_cast<uint4*>(sd + (ol * 64 + pl) * 16) = d4;
            const v8 d8 = __builtin_bit_cast(v8, d4);
#pragma unroll
            for (int e = 0; e < 8; ++e) dbs[jj][e] += (float)d8[e];
        }
        __syncthreads();
        if (tile + g.nslab < g.ntiles) gload(tile + g.nslab);       // the next tile's cells travel under the products
        v8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = c81_tr_operand<E>(sd, i, 16 * (int)wave, (int)lane);
            b[i] = c81_tr_operand<E>(sx, i, 16 * (int)wave, (int)lane);
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
        float* const ws = g.ws + (size_t)slab * g.K * g.C;
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const unsigned c = 8 * co0 + 32 * ct + (lane & 31u);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned k = 8 * ko0 + 32 * ft + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (k < g.K && c < g.C) ws[(size_t)k * g.C + c] = acc[ft][ct][r] * g.oscale;
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

// cells of a c8 tensor of N x C maps of S pixels a side at pitch P, or -1: bad geometry / 2^32 cells or more
static long long c81_cells(int N, int C, int S, int P) {
    if (N <= 0 || C <= 0 || S <= 0 || P < S || (P != S && (P & (P - 1)))) return -1;
    const long long cells = (long long)N * ((C + 7) / 8) * P * P;
    return cells < (1ll << 32) ? cells : -1;
}

template <typename E, int MODE>
static int c81_run(tn_ctx* ctx, C81G& g, const float* W, int K, int C) {
    const int dgrad = MODE >= 2 ? 1 : 0;
    const int O = dgrad ? C : K, R = dgrad ? K : C;
    // row tiles per wave: 4 from 128 rows on (the plain forward stays at 2: with 4 its epilogue spilled registers)
    const int MT = cdiv(O, 32), KT = (MT >= 4 && MODE != 0) ? 4 : (MT >= 2 ? 2 : 1), GY = cdiv(MT, KT);
    g.O = (unsigned)O; g.O8 = (unsigned)((O + 7) / 8); g.R8 = (unsigned)((R + 7) / 8); g.R16 = (unsigned)cdiv(R, 16);
    const size_t total = (size_t)GY * KT * g.R16 * 512;
    TN_REQUIRE(total < (1ull << 31), "c8 conv1: %d x %d weights: too large", K, C);
    float* wt;
    int rc = tn_scratch_get(ctx, total * sizeof(typename E::T), &wt);
    if (rc) return rc;
    c8_conv1_wt_kernel<E><<<cdiv((long long)total, 256), 256, 0, ctx->stream>>>(W, reinterpret_cast<typename E::T*>(wt), K, C,
                                                                              (int)g.R16, dgrad, (unsigned)total);
    TN_LAUNCH_CHECK();
    g.wt = reinterpret_cast<const uint4*>(wt);
    const unsigned long long per_block = MODE == 1 ? 64 : 256;          // windows / pixels of a block's 8 lane tiles
    const dim3 grid((unsigned)((g.units + per_block - 1) / per_block), (unsigned)GY);
    if (KT == 1) c8_conv1_kernel<E, MODE, 1><<<grid, 256, 0, ctx->stream>>>(g);
    else if (KT == 2) c8_conv1_kernel<E, MODE, 2><<<grid, 256, 0, ctx->stream>>>(g);
    else if constexpr (MODE != 0) c8_conv1_kernel<E, MODE, 4><<<grid, 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

static void c81_geom(C81G& g, int N, int S, int P, bool windows) {
    g.N = (unsigned)N; g.S = (unsigned)S; g.P = (unsigned)P; g.PP = (unsigned)P * P;
    g.Ph = (unsigned)P / 2; g.QQ = g.Ph * g.Ph;
    g.units = (unsigned long long)N * (windows ? g.QQ : g.PP);
}

extern "C" {

#ifndef C8_BF16_TU
// the bf16 entry points (conv1_c8_bf16.hip)
int c8b_tn_c8_conv1_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, uint8_t* mask, int N, int C,
                        int S, int P, int K, int act, float prm, int pool);
int c8b_tn_c8_conv1_dgrad(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K,
                          const void* prev_a, int prev_act, float prev_prm, int pooled, const uint8_t* mask);
int c8b_tn_c8_conv1_wgrad(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P,
                          int K, int pooled, const uint8_t* mask);

// 1 if the c8 kernels take a 1x1 stride-1 layer of this shape (forward, both gradients; either element type)
int tn_c8_conv1_supported(int N, int C, int S, int P, int K) {
    return c81_cells(N, C, S, P) > 0 && c81_cells(N, K, S, P) > 0 && (long long)K * C < (1ll << 28) ? 1 : 0;
}
#endif

// y = act(W . x + b) [pool != 0: followed by a 2x2 max-pool, y at pitch P / 2; mask (may be NULL) as tn_c8_conv_fwd's]
int C8_API(tn_c8_conv1_fwd)(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, uint8_t* mask, int N, int C,
                            int S, int P, int K, int act, float prm, int pool) {
    C8_TO_BF16(tn_c8_conv1_fwd, ctx, x, W, b, y, mask, N, C, S, P, K, act, prm, pool);
    TN_REQUIRE(x && W && b && y && c81_cells(N, C, S, P) > 0 && c81_cells(N, K, S, P) > 0 && (long long)K * C < (1ll << 28) &&
                   (!pool || (S & 1) == 0),
               "tn_c8_conv1_fwd: bad arguments (N %d, %d -> %d maps of %d pixels at pitch %d, pool %d)", N, C, K, S, P, pool);
    C81G g{};
    g.x = static_cast<const uint4*>(x); g.out = static_cast<uint4*>(y); g.bias = b;
    g.mask_out = reinterpret_cast<uint2*>(mask); g.act = act; g.prm = prm;
    c81_geom(g, N, S, P, pool != 0);
    return pool ? c81_run<C8E, 1>(ctx, g, W, K, C) : c81_run<C8E, 0>(ctx, g, W, K, C);
}

// dx = W^T . dz * act'(prev_a) (prev_a NULL: none); pooled != 0: dz is the pooled gradient (N, K, S/2, S/2) at pitch P / 2
// and dz = (bit of the window element in the block's mask) ? pooled gradient : 0 is formed while loading
int C8_API(tn_c8_conv1_dgrad)(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K,
                              const void* prev_a, int prev_act, float prev_prm, int pooled, const uint8_t* mask) {
    C8_TO_BF16(tn_c8_conv1_dgrad, ctx, dz, W, dx, N, C, S, P, K, prev_a, prev_act, prev_prm, pooled, mask);
    TN_REQUIRE(dz && W && dx && c81_cells(N, C, S, P) > 0 && c81_cells(N, K, S, P) > 0 && (long long)K * C < (1ll << 28) &&
                   (!pooled || ((S & 1) == 0 && mask != nullptr)),
               "tn_c8_conv1_dgrad: bad arguments (N %d, %d -> %d maps of %d pixels at pitch %d, pooled %d)", N, C, K, S, P,
               pooled);
    C81G g{};
    g.x = static_cast<const uint4*>(dz); g.out = static_cast<uint4*>(dx); g.prev_a = static_cast<const uint4*>(prev_a);
    g.mask_in = reinterpret_cast<const uint2*>(mask); g.act = prev_act; g.prm = prev_prm;
    c81_geom(g, N, S, P, false);
    return pooled ? c81_run<C8E, 3>(ctx, g, W, K, C) : c81_run<C8E, 2>(ctx, g, W, K, C);
}

// dW (K, C), db (K) from x and dz (pooled != 0: dz formed as in tn_c8_conv1_dgrad); dz carries the gradient scale, the
// results do not.  OVERWRITE
int C8_API(tn_c8_conv1_wgrad)(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P,
                              int K, int pooled, const uint8_t* mask) {
    C8_TO_BF16(tn_c8_conv1_wgrad, ctx, x, dz, dW, db, N, C, S, P, K, pooled, mask);
    TN_REQUIRE(x && dz && dW && db && c81_cells(N, C, S, P) > 0 && c81_cells(N, K, S, P) > 0 &&
                   (long long)K * C < (1ll << 28) && (!pooled || ((S & 1) == 0 && mask != nullptr)),
               "tn_c8_conv1_wgrad: bad arguments (N %d, %d -> %d maps of %d pixels at pitch %d, pooled %d)", N, C, K, S, P,
               pooled);
    C81W g{};
    g.x = static_cast<const uint4*>(x); g.dz = static_cast<const uint4*>(dz); g.mask = reinterpret_cast<const uint2*>(mask);
    g.N = (unsigned)N; g.P = (unsigned)P; g.PP = (unsigned)P * P; g.Ph = (unsigned)P / 2; g.QQ = g.Ph * g.Ph;
    g.C = (unsigned)C; g.C8 = (unsigned)((C + 7) / 8); g.K = (unsigned)K; g.K8 = (unsigned)((K + 7) / 8);
    g.npix = (unsigned long long)N * g.PP;
    g.ntiles = (unsigned)((g.npix + 63) / 64);
    const int CG = cdiv(C, 64), KG = cdiv(K, 64);
    TN_REQUIRE(CG <= 65535 && KG <= 65535, "tn_c8_conv1_wgrad: %d x %d weights: too large", K, C);
    // slabs: two blocks per CU over all (channel group, filter group) pairs, at most one per tile
    const long long want = cdiv(2ll * ctx->num_cus, (long long)CG * KG);
    g.nslab = (unsigned)(want < 1 ? 1 : (want > (long long)g.ntiles ? (long long)g.ntiles : want));
    const size_t n = (size_t)K * C;
    int rc = tn_scratch_get(ctx, ((size_t)g.nslab * n + (size_t)g.nslab * K) * sizeof(float), &g.ws);
    if (rc) return rc;
    g.dbws = g.ws + (size_t)g.nslab * n;
    g.oscale = 1.f / ctx->grad_scale;
    const dim3 grid(g.nslab, (unsigned)CG, (unsigned)KG);
    if (pooled) c8_conv1_wgrad_kernel<C8E, true><<<grid, 256, 0, ctx->stream>>>(g);
    else c8_conv1_wgrad_kernel<C8E, false><<<grid, 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return tn_red_wgrad(ctx, g.ws, dW, (uint32_t)n, g.nslab, (uint32_t)n, g.dbws, db, (uint32_t)K, g.nslab, (uint32_t)K);
}

}  // extern "C"
