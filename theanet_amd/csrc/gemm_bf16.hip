// MATMUL 'bfloat16' (opt-in, training param; default off): the fully-connected products of theanet/layer/hidden.py:30 and
// their gradients (layer.py:83) at bf16 precision, the arithmetic of the 16-bit conv stack (conv_c8.hip) applied to the
// dense layers.
//
// Both operands of every product are rounded to bf16 (nearest even, v_cvt_pk_bf16_f32) while their tile is staged into
// LDS; products are exact and accumulate in fp32 on v_mfma_f32_32x32x16_bf16; bias, activation, dropout mask, act' run
// on the fp32 sums in the epilogue.  Tensors in HBM stay fp32 (activations, dz, master weights, dW, db), and no gradient
// scale is needed: bf16 has fp32's exponent range.  db is the fp32 column sum of the UNROUNDED dz (it is no product).
// This is a reduced-precision mode (unlike 'bf16x3', gemm_b3.hip, which is fp32-grade): results differ from the fp32
// path's by ~2^-9 of the operands' magnitude per product term.
//
// The OUTPUT HEADS stay fp32 by design: tn_fc_skinny_softmax*, tn_fc_softmax_*, the row kernels of heads.hip never
// dispatch here (their products are skinny and fused with the loss), and the host turns the mode off around the affine
// map of a head that goes through tn_fc_fwd / tn_fc_bwd (Context.fc_head, theanet_amd/device.py).
//
// One kernel for the three products of a layer: C (M x N) = A (M x K) . B (K x N), each operand k-contiguous or
// k-major in global memory, staged in the orientation it is stored in; a k-contiguous operand is read with
// ds_read_b128, a k-major one through gfx950's transposing read (ds_read_b64_tr_b16).  One LDS plane per operand (the
// bf16x3 kernel holds three), so the same LDS holds TWO stages of a 128 x (64 | 128) x 32 tile: stage t+1 is fetched
// into registers before the matrix work on stage t and written to the other buffer after it -- one barrier per K tile.
// Four waves of 64 x (32 | 64).  The narrow tile serves products with few column tiles (it doubles the blocks).
//
// ANY shape runs here (no fp32 fall-back for a HiddenLayer): rows / columns / reduction indices beyond the operand are
// staged as zeros and never stored.  Operands whose rows are 16-byte aligned with extents that are multiples of 4 are
// fetched as float4; every other operand element by element with clamped addresses.
// Split-K slabs for the weight gradient, finished in slab order by the step's reduction (tn_red_wgrad).
#include "common.h"

#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf_short4 __attribute__((ext_vector_type(4)));

#define BF_BM 128
#define BF_BK 32
#define BF_RKC 80           // bytes per row of a k-contiguous tile image (32 bf16 + 16: 16-byte slots of 16 rows all distinct)
#define BF_RA 320           // bytes per k-row of a k-major image of 128 rows / columns (128 bf16 + 64: = 64 mod 256)
#define BF_RB64 192         // ... of 64 columns (64 bf16 + 64)

struct BfArgs {
    const float* A; const float* B; float* C;
    int M, N, K;
    long lda, ldb, ldc;
    int kchunk;              // K range of a slab (multiple of 32); blockIdx.z = slab
    int epi;                 // 0: plain store to C + slab * M * N; 1: bias + act + mask; 2: * act'(prev_a) * mask
    int a_vec, b_vec;        // the operand can be fetched as float4 (alignment, extents: bf_vec_ok)
    const float* bias; const uint8_t* mask; const float* prev_a;
    int act; float prm;
    float* colsum;           // != NULL: column sums of B over the slab's k -> colsum[slab * N + n] (blocks of row tile 0)
};

// 8 floats -> 8 bf16 (nearest even), 16 bytes
__device__ __forceinline__ bf16x8 bf_round8(const float (&v)[8]) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (__bf16)v[j];
    return r;
}

__device__ __forceinline__ bf16x8 bf_tr(const char* p, int rs) {
    const bf_short4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf_short4*)p);
    const bf_short4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf_short4*)(p + 4 * rs));
    typedef short s8 __attribute__((ext_vector_type(8)));
    const s8 r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, r);
}

// NI: 32-column tiles per wave (1: block 128 x 64, 2: block 128 x 128)
template <bool AKC, bool BKC, int NI>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(BfArgs g) {
    constexpr int BN = 64 * NI;
    constexpr int RB = NI == 2 ? BF_RA : BF_RB64;
    constexpr int APL = AKC ? BF_BM * BF_RKC : BF_BK * BF_RA;         // bytes of the A image of a stage
    constexpr int BPL = BKC ? BN * BF_RKC : BF_BK * RB;
    constexpr int STAGE = APL + BPL;
    constexpr int NO = BN / 8;                                         // column octets of a k-major B row
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];       // two stages (30 / 40 KB)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const int m0 = blockIdx.y * BF_BM, n0 = blockIdx.x * BN, slab = blockIdx.z;
    const int kbeg = slab * g.kchunk, kend = min(g.K, kbeg + g.kchunk);
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 32 * NI;

    // ---- staging units of this thread: 8 consecutive elements along the contiguous dimension --------------
    // k-contiguous: unit = (row, k octet): 128 rows x 4 = 512 units (two per thread); B: BN x 4 = NI * 256
    // k-major     : unit = (k, octet of rows): A 32 x 16 = 512; B 32 x NO = NI * 256
    float ra[2][8], rb[NI][8];
    auto aunit = [&](int u, int& row, int& k) __attribute__((always_inline)) {
        const int id = t + 256 * u;
        if (AKC) { row = id >> 2; k = (id & 3) * 8; }
        else { k = id >> 4; row = (id & 15) * 8; }
    };
    auto bunit = [&](int u, int& col, int& k) __attribute__((always_inline)) {
        const int id = t + 256 * u;
        if (BKC) { col = id >> 2; k = (id & 3) * 8; }
        else { k = id / NO; col = (id % NO) * 8; }
    };
    // Branch-free inside a path: every load of a unit always happens, from a clamped address, and what lies outside
    // the operand (or the slab) is zeroed by selects afterwards.  vec: two float4 (a float4 is inside or outside as a
    // whole: extents are multiples of 4); otherwise eight clamped scalar loads.
    auto load8 = [&](const float* base, long ld, bool kc, bool vec, int row, int k, int rmax, float (&v)[8]) __attribute__((always_inline)) {
        if (vec) {
            float4 x, y;
            bool okx, oky;
            if (kc) {      // elements k .. k+7 of row `row`
                const float* p = base + (long)min(row, rmax - 1) * ld;
                x = *reinterpret_cast<const float4*>(p + min(k, g.K - 4));
                y = *reinterpret_cast<const float4*>(p + min(k + 4, g.K - 4));
                okx = k + 4 <= kend && row < rmax; oky = k + 8 <= kend && row < rmax;
            } else {       // rows row .. row+7 at reduction index k
                const float* p = base + (long)min(k, g.K - 1) * ld;
                x = *reinterpret_cast<const float4*>(p + min(row, rmax - 4));
                y = *reinterpret_cast<const float4*>(p + min(row + 4, rmax - 4));
                okx = k < kend && row + 4 <= rmax; oky = k < kend && row + 8 <= rmax;
            }
            v[0] = okx ? x.x : 0.f; v[1] = okx ? x.y : 0.f; v[2] = okx ? x.z : 0.f; v[3] = okx ? x.w : 0.f;
            v[4] = oky ? y.x : 0.f; v[5] = oky ? y.y : 0.f; v[6] = oky ? y.z : 0.f; v[7] = oky ? y.w : 0.f;
        } else if (kc) {
            const float* p = base + (long)min(row, rmax - 1) * ld;
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = p[min(k + j, g.K - 1)];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (k + j < kend && row < rmax) ? x[j] : 0.f;
        } else {
            const float* p = base + (long)min(k, g.K - 1) * ld;
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = p[min(row + j, rmax - 1)];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (k < kend && row + j < rmax) ? x[j] : 0.f;
        }
    };
    auto gload = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            int row, k;
            aunit(u, row, k);
            load8(g.A, g.lda, AKC, g.a_vec != 0, m0 + row, ks + k, g.M, ra[u]);
        }
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            int col, k;
            bunit(u, col, k);
            load8(g.B, g.ldb, BKC, g.b_vec != 0, n0 + col, ks + k, g.N, rb[u]);
        }
    };
    float csum[8];           // k-major B: both units of a thread hold the same column octet (256 % NO == 0)
#pragma unroll
    for (int j = 0; j < 8; ++j) csum[j] = 0.f;
    auto lstore = [&](int buf) __attribute__((always_inline)) {
        char* sa = lds + buf * STAGE;
        char* sb = sa + APL;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            int row, k;
            aunit(u, row, k);
            *reinterpret_cast<bf16x8*>(sa + (AKC ? row * BF_RKC + k * 2 : k * BF_RA + row * 2)) = bf_round8(ra[u]);
        }
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            int col, k;
            bunit(u, col, k);
            *reinterpret_cast<bf16x8*>(sb + (BKC ? col * BF_RKC + k * 2 : k * RB + col * 2)) = bf_round8(rb[u]);
            if (!BKC && g.colsum) {
#pragma unroll
                for (int j = 0; j < 8; ++j) csum[j] += rb[u][j];
            }
        }
    };

    f32x16 acc[2][NI];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < NI; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][n][r] = 0.f;

    // operand read offsets of this lane inside an image (first 16-deep step; + 32 bytes / + 16 k-rows for the second)
    const int grp = lane >> 4, r4 = (lane >> 2) & 3, q4 = lane & 3;
    const int a_rd = AKC ? (wm + l31) * BF_RKC + hi * 16 : (8 * (grp >> 1) + r4) * BF_RA + (wm + 16 * (grp & 1) + 4 * q4) * 2;
    const int b_rd = BKC ? (wn + l31) * BF_RKC + hi * 16 : (8 * (grp >> 1) + r4) * RB + (wn + 16 * (grp & 1) + 4 * q4) * 2;

    gload(kbeg);
    lstore(0);
    __syncthreads();
    int buf = 0;
    for (int ks = kbeg; ks < kend; ks += BF_BK) {
        const bool more = ks + BF_BK < kend;          // (block-uniform)
        if (more) gload(ks + BF_BK);
        __builtin_amdgcn_sched_barrier(0);            // (the loads stay above the matrix work that hides them)
        const char* sa = lds + buf * STAGE;
        const char* sb = sa + APL;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 a[2], b[NI];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (AKC) a[i] = *reinterpret_cast<const bf16x8*>(sa + a_rd + i * 32 * BF_RKC + s * 32);
                else a[i] = bf_tr(sa + a_rd + i * 64 + s * 16 * BF_RA, BF_RA);
            }
#pragma unroll
            for (int n = 0; n < NI; ++n) {
                if (BKC) b[n] = *reinterpret_cast<const bf16x8*>(sb + b_rd + n * 32 * BF_RKC + s * 32);
                else b[n] = bf_tr(sb + b_rd + n * 64 + s * 16 * RB, RB);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int n = 0; n < NI; ++n)
                    acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[n], acc[i][n], 0, 0, 0);
        }
        // the other buffer was last read before the previous barrier
        if (more) lstore(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // ---- column sums of B (the bias gradient of a weight-gradient product): per n, over this slab's k, in k order ----
    if (!BKC && g.colsum && blockIdx.y == 0) {
        constexpr int KR = 256 / NO;                         // k-rows a pass of the 256 threads covers
        float* red = reinterpret_cast<float*>(lds);          // [KR][BN] (8 KB; everybody is past the last stage's reads)
        const int kr = t / NO, col = (t % NO) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) red[kr * BN + col + j] = csum[j];
        __syncthreads();
        if (t < BN) {
            float s = 0.f;
            for (int r = 0; r < KR; ++r) s += red[r * BN + t];
            if (n0 + t < g.N) g.colsum[(size_t)slab * g.N + n0 + t] = s;
        }
    }

    // ---- epilogue: lane = column n (32 consecutive per half-wave), registers = rows ----
    float* C = g.C + (g.epi == 0 ? (size_t)slab * g.M * g.N : 0);
    const float tie = g.prm > 0.f ? 1.f + g.prm : 0.f;
#pragma unroll
    for (int nn = 0; nn < NI; ++nn) {
        const int n = n0 + wn + 32 * nn + l31;
        if (n >= g.N) continue;
        const float bias = (g.epi == 1 && g.bias) ? g.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (m >= g.M) continue;
                const size_t o = (size_t)m * g.ldc + n;
                float v = acc[i][nn][r];
                if (g.epi == 1) {
                    v += bias;
                    v = g.act == TN_ACT_LEAKY ? fmaxf(0.f, v) + fminf(0.f, v) * g.prm : tn_act_fwd(v, g.act, g.prm);
                    if (g.mask) v = g.mask[o] ? v : 0.f;
                } else if (g.epi == 2) {
                    if (g.prev_a) {
                        const float y = g.prev_a[o];
                        v *= g.act == TN_ACT_LEAKY ? (y > 0.f ? 1.f : (y < 0.f ? g.prm : tie)) : tn_act_grad_from_out(y, g.act, g.prm);
                    }
                    if (g.mask) v = g.mask[o] ? v : 0.f;
                }
                C[o] = v;
            }
    }
}

static bool bf_al(const void* p) { return ((uintptr_t)p & 15) == 0; }
// float4 fetches of an operand: 16-byte aligned rows, and the extent along the contiguous dimension a multiple of 4
// (kc: that is the reduction K; k-major: the rows / columns `ext`)
static int bf_vec_ok(const float* p, long ld, int ext) { return bf_al(p) && (ld & 3) == 0 && (ext & 3) == 0 && ext >= 4; }

template <bool AKC, bool BKC>
static int bf_launch(tn_ctx* ctx, BfArgs& g, int S) {
    g.a_vec = bf_vec_ok(g.A, g.lda, AKC ? g.K : g.M);
    g.b_vec = bf_vec_ok(g.B, g.ldb, BKC ? g.K : g.N);
    // wide tiles unless they leave CUs without a block that narrow ones would give one
    const long long wide = (long long)cdiv(g.N, 128) * cdiv(g.M, BF_BM) * S;
    if (g.N > 64 && wide >= ctx->num_cus)
        gemm_bf16_kernel<AKC, BKC, 2><<<dim3(cdiv(g.N, 128), cdiv(g.M, BF_BM), S), 256, 0, ctx->stream>>>(g);
    else
        gemm_bf16_kernel<AKC, BKC, 1><<<dim3(cdiv(g.N, 64), cdiv(g.M, BF_BM), S), 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_bf_fc_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int B, int n_in, int n_out, int act,
                 float prm, const uint8_t* mask) {
    TN_REQUIRE(x && W && b && a && B > 0 && n_in > 0 && n_out > 0, "tn_fc_fwd (MATMUL 'bfloat16'): bad arguments");
    BfArgs g{};
    g.A = x; g.B = W; g.C = a; g.M = B; g.N = n_out; g.K = n_in; g.lda = n_in; g.ldb = n_out; g.ldc = n_out;
    g.kchunk = cdiv(n_in, BF_BK) * BF_BK; g.epi = 1; g.bias = b; g.mask = mask; g.act = act; g.prm = prm;
    return bf_launch<true, false>(ctx, g, 1);
}

int tn_bf_fc_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int B, int n_in, int n_out, const float* prev_a,
                   int act, float prm, const uint8_t* mask) {
    TN_REQUIRE(dz && W && dx && B > 0 && n_in > 0 && n_out > 0, "tn_fc_dgrad (MATMUL 'bfloat16'): bad arguments");
    BfArgs g{};
    g.A = dz; g.B = W; g.C = dx; g.M = B; g.N = n_in; g.K = n_out; g.lda = n_out; g.ldb = n_out; g.ldc = n_in;
    g.kchunk = cdiv(n_out, BF_BK) * BF_BK; g.epi = 2; g.prev_a = prev_a; g.mask = mask; g.act = act; g.prm = prm;
    return bf_launch<true, true>(ctx, g, 1);
}

// dW (n_in, n_out) = x^T . dz, db = column sums of dz; S sample slabs into ws ([S][n_in * n_out] then [S][n_out]),
// recorded for the step's reduction (tn_red_wgrad: slabs are added in slab order) unless one slab covers B
int tn_bf_fc_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int B, int n_in, int n_out, float* ws,
                   int S) {
    TN_REQUIRE(x && dz && dW && db && ws && B > 0 && n_in > 0 && n_out > 0 && S > 0,
               "tn_fc_wgrad (MATMUL 'bfloat16'): bad arguments");
    BfArgs g{};
    g.A = x; g.B = dz; g.M = n_in; g.N = n_out; g.K = B; g.lda = n_in; g.ldb = n_out; g.ldc = n_out;
    g.kchunk = cdiv(cdiv(B, S), BF_BK) * BF_BK;
    const int Sx = cdiv(B, g.kchunk);
    g.epi = 0;
    const size_t MN = (size_t)n_in * n_out;
    if (Sx == 1) {
        g.C = dW; g.colsum = db;
        return bf_launch<false, false>(ctx, g, 1);
    }
    g.C = ws; g.colsum = ws + (size_t)S * MN;
    int rc = bf_launch<false, false>(ctx, g, Sx);
    if (rc) return rc;
    return tn_red_wgrad(ctx, ws, dW, (uint32_t)MN, (uint32_t)Sx, (uint32_t)MN, g.colsum, db, (uint32_t)n_out, (uint32_t)Sx,
                        (uint32_t)n_out);
}
