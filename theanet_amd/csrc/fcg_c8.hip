// DTYPE 'float16' / 'bfloat16', the dense layer on the 16-bit conv stack for ANY layer shape: tn_c8_fcg_*, the general
// family beside the tiled tn_c8_fc_* of fc_c8.hip (which wants the c8 input length a multiple of 64 and n_out a multiple
// of 32 and keeps every shape it takes: HiddenLayer asks tn_c8_fc_supported first).  Same call sites (hidden.py:30 and
// its gradients, layer.py:83), same arguments, same arithmetic -- the oracle's stored-16-bit statement: x as stored (the
// flattened c8 tensor of C maps of HW pixels), W (C*HW, n_out) fp32 in the reference's NCHW-flattened row order
// (neuralnet.py:168-173) walked through the row map k -> (8 o + e) * HW + p and rounded nearest-even to the element type
// while it is staged, dz as E(grad_scale * dz), exact products, fp32 accumulation on v_mfma_f32_32x32x16_f16 / _bf16;
// a, dW and db are fp32 with the gradient scale removed, dx is E(acc * act'(y16)) in c8 order.
//
// One tiling for the three products: block = 256 threads = a 64 x 64 output tile (wave = 32 x 32), the reduction in
// chunks of 64 through LDS.  Both operand tiles are written to LDS AS THEY ARE STORED in global memory (so the global
// loads are coalesced along the stored rows: 16-byte loads of the 16-bit tensors, dword loads of the fp32 ones -- no
// alignment of n_out is assumed anywhere) and read either row-wise (16-byte reads: the reduction index is the stored
// row's) or through gfx950's transposing read (ds_read_b64_tr_b16: the reduction index runs across stored rows):
//   forward : a[m][n]  = sum_k x[m][k] W[row(k)][n]      x rows / W transposed; K slabs [S][B][n_out] in context scratch,
//             summed in slab order by the finishing kernel (bias, activation, dropout mask given or drawn: one thread per
//             output, element elem0 + m n_out + n of tn_dropout_mask's stream whatever n_out's parity)
//   dgrad   : dx[m][k] = sum_n W[row(k)][n] dz16[m][n]   both row-wise; a lane's accumulators are 4 consecutive c8 columns
//             of one sample: 8-byte stores; EVERY c8 cell is written, channels past C as exact +0
//   wgrad   : dW[row(k)][n] = sum_m x[m][k] dz16[m][n]   both transposed; sample slabs [S][C*HW][n_out] (+ [S][n_out] for
//             db, the column sums of dz16 by a product with ones) in context scratch, finished by the context's reduction
// A ragged reduction tail is staged as zeros, a ragged output tail is computed in the padded tile and not stored, and a c8
// column whose channel is past C stages zeros instead of a row of W (nothing is read out of bounds, nothing clamped).
// No atomics: the same call gives the same bits.
//
// Limits (tn_c8_fcg_supported; the ops refuse by name, nothing launched): B, C, HW, n_out >= 1; with
// Kc = ceil(C/8) * HW * 8: B * Kc, B * n_out and C * HW * n_out < 2^31 (element counts: the offsets are 64-bit, the counts
// go to the context's reduction and the launch grids as 32-bit values), (Kc / 8) * HW < 2^32 (the 2^32 / HW + 1 division
// magic of the row map), at most 65535 tiles of 64 samples or of 64 outputs (grid extents).  x, W, b, a, dz, dx, dW, db
// must not be NULL (mask, y16: NULL = none).
#include "c8_elem.h"

typedef unsigned fcg_u4 __attribute__((ext_vector_type(4)));
typedef unsigned fcg_u2 __attribute__((ext_vector_type(2)));
typedef short fcg_short4 __attribute__((ext_vector_type(4)));

#define FCG_RS 144          // row stride of a tile read row-wise (64 elements + 16 bytes: 9 x 16 B)
#define FCG_TS 192          // row stride of a tile read through the transposing read (64 elements + 64 bytes)

struct FCG {
    const void* x;          // (M, Kc) elements, Kc = ceil(C/8) * HW * 8
    const float* W;         // (C * HW, N)
    const float* dz;        // (M, N) fp32
    const void* ya;         // dgrad: output of the layer below in x's order (act' is taken from it) or NULL
    void* dx;               // dgrad: (M, Kc) elements, carries the gradient scale
    float* ws;              // forward: K slabs [S][M][N]; wgrad: sample slabs [S][C*HW][N] (S == 1: dW itself)
    float* dbws;            // wgrad: [S][N]
    int M, N, Kc, C, HW, S, krange, act;
    unsigned magic;         // 2^32 / HW + 1 (0: HW == 1)
    float prm, gs, oscale;
};

struct FcgDrop {            // dropout drawn by the finishing kernel (tn_c8_fcg_fwd_dropout): the numbers of tn_dropout_mask
    uint8_t* mask_out;      // NULL: no inline dropout
    float pdrop;
    uint32_t k0, k1, step;
    const uint32_t* d_step;
    uint64_t elem0;
};

// c8 column k -> row of W, (8 o + e) * HW + p with (o, p) = (cell / HW, cell % HW), cell = k >> 3, e = k & 7 (the division
// by the magic: exact while cell * HW < 2^32, checked by the host); -1: k is past the input or its channel is past C
__device__ __forceinline__ int fcg_wrow(const FCG& g, int k) {
    if (k >= g.Kc) return -1;
    const int cell = k >> 3, e = k & 7;
    const int o = g.magic ? (int)__umulhi((unsigned)cell, g.magic) : cell;
    const int p = cell - o * g.HW, ch = o * 8 + e;
    return ch < g.C ? ch * g.HW + p : -1;
}

// the 32 x 16 MFMA operand of reduction step ks from a tile stored [reduction index][64 columns] (row stride FCG_TS):
// `base` is the lane's address for step 0 (fcg_tr_base)
template <typename E>
__device__ __forceinline__ typename E::v8 fcg_tr_read(const char* base, int ks) {
    typedef typename E::v4 v4;
    const v4 a = __builtin_bit_cast(v4, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                     (__attribute__((address_space(3))) fcg_short4*)(base + 16 * ks * FCG_TS)));
    const v4 b = __builtin_bit_cast(v4, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                     (__attribute__((address_space(3))) fcg_short4*)(base + (16 * ks + 4) * FCG_TS)));
    return typename E::v8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
// group of 16 lanes = 4 reduction rows x 16 columns; lane 4 q + p supplies row q, columns 4 p .. 4 p + 3
__device__ __forceinline__ const char* fcg_tr_base(const char* tile, int lane, int col0) {
    const int grp = lane >> 4, r4 = (lane >> 2) & 3, q4 = lane & 3;
    return tile + (8 * (grp >> 1) + r4) * FCG_TS + (col0 + 16 * (grp & 1) + 4 * q4) * 2;
}

// ---------------------------------------------------------------------------------------------------------------
// forward: grid = (n_out / 64, S K-slabs, B / 64)
// ---------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256) void fcg_fwd_kernel(FCG g) {
    typedef typename E::T T;
    typedef typename E::v8 v8;
    __shared__ __attribute__((aligned(16))) char xs[64 * FCG_RS];      // [sample][k]
    __shared__ __attribute__((aligned(16))) char wsm[64 * FCG_TS];     // [k][output]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const int n0 = blockIdx.x * 64, m0 = blockIdx.z * 64;
    const int kbeg = blockIdx.y * g.krange, kend = min(g.Kc, kbeg + g.krange);
    const int wm = wave >> 1, wn = wave & 1;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // staging roles: x row t >> 2, 16 elements from 16 (t & 3); W output t & 63, k rows (t >> 6) + 4 i
    const int xm = m0 + (t >> 2), xk = 16 * (t & 3), wn_ = n0 + (t & 63), wk = t >> 6;
    const T* const xrow = static_cast<const T*>(g.x) + (size_t)min(xm, g.M - 1) * g.Kc;
    fcg_u4 xr[2];
    float wr[16];
    auto gload = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = kc + xk + 8 * i;
            xr[i] = fcg_u4{0u, 0u, 0u, 0u};
            if (xm < g.M && k < kend) xr[i] = *reinterpret_cast<const fcg_u4*>(xrow + k);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int k = kc + wk + 4 * i;
            const int row = fcg_wrow(g, k < kend ? k : g.Kc);
            wr[i] = 0.f;
            if (row >= 0 && wn_ < g.N) wr[i] = g.W[(size_t)row * g.N + wn_];
        }
    };
    const char* const ard = xs + (wm * 32 + l31) * FCG_RS + 16 * hi;
    const char* const brd = fcg_tr_base(wsm, lane, wn * 32);
    gload(kbeg);
    for (int kc = kbeg; kc < kend; kc += 64) {
        __syncthreads();                       // the previous chunk's reads are done
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<fcg_u4*>(xs + (t >> 2) * FCG_RS + (xk + 8 * i) * 2) = xr[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) *reinterpret_cast<T*>(wsm + (wk + 4 * i) * FCG_TS + (t & 63) * 2) = (T)(wr[i]);
        if (kc + 64 < kend) gload(kc + 64);    // the next chunk travels during this chunk's products
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const v8 a = *reinterpret_cast<const v8*>(ard + 32 * ks);
            const v8 b = fcg_tr_read<E>(brd, ks);
            acc = E::mfma(a, b, acc);
        }
    }
    float* const wz = g.ws + (size_t)blockIdx.y * g.M * g.N;
    const int n = n0 + wn * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (m < g.M && n < g.N) wz[(size_t)m * g.N + n] = acc[r];
    }
}

// out = act(sum of the K slabs + bias) (* mask), slabs added in order; thread = one output.  Element e = elem0 + i of the
// dropout stream uses word (e & 3) of philox(e >> 2): per element, so rows of any length and any elem0 draw
// tn_dropout_mask's bits.  (E is unused: one symbol per translation unit.)
template <typename E>
__global__ __launch_bounds__(256) void fcg_fwd_finish_kernel(const float* __restrict__ ws, int S, size_t MN, int N,
                                                             const float* __restrict__ bias, const uint8_t* __restrict__ mask,
                                                             float* __restrict__ out, int act, float prm, FcgDrop dr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    float v = 0.f;
    for (int z = 0; z < S; ++z) v += ws[(size_t)z * MN + i];
    v += bias[(uint32_t)i % (uint32_t)N];          // (MN < 2^31: tn_c8_fcg_supported)
    v = act == TN_ACT_LEAKY ? fmaxf(0.f, v) + fminf(0.f, v) * prm : tn_act_fwd(v, act, prm);
    if (dr.mask_out) {
        const uint64_t e = dr.elem0 + i, cq = e >> 2;
        const u32x4 r = philox4x32((uint32_t)cq, (uint32_t)(cq >> 32), dr.step + (dr.d_step ? *dr.d_step : 0u),
                                   TN_STREAM_DROPOUT, dr.k0, dr.k1);
        const uint32_t w = ((e & 3) == 0) ? r.x : ((e & 3) == 1) ? r.y : ((e & 3) == 2) ? r.z : r.w;
        const bool keep = tn_u01(w) >= dr.pdrop;
        dr.mask_out[i] = keep ? 1 : 0;
        v = keep ? v : 0.f;
    } else if (mask) {
        v = mask[i] ? v : 0.f;
    }
    out[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------
// dgrad: grid = (Kc / 64, B / 64); C = W_tile . dz16^T: rows = c8 columns, columns = samples
// ---------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256) void fcg_dgrad_kernel(FCG g) {
    typedef typename E::T T;
    typedef typename E::v8 v8;
    typedef typename E::v4 v4;
    __shared__ __attribute__((aligned(16))) char wl[64 * FCG_RS];      // [c8 column][output]
    __shared__ __attribute__((aligned(16))) char dl[64 * FCG_RS];      // [sample][output]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const int kb0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    const int wk = wave & 1, wm = wave >> 1;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // staging roles: output t & 63 of the chunk; W rows / dz rows (t >> 6) + 4 i
    const int cn = t & 63, r0 = t >> 6;
    int wrow[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) wrow[i] = fcg_wrow(g, kb0 + r0 + 4 * i);
    float wr[16], dr[16];
    auto gload = [&](int nc) __attribute__((always_inline)) {
        const int n = nc + cn;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            wr[i] = 0.f;
            if (wrow[i] >= 0 && n < g.N) wr[i] = g.W[(size_t)wrow[i] * g.N + n];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = m0 + r0 + 4 * i;
            dr[i] = 0.f;
            if (m < g.M && n < g.N) dr[i] = g.dz[(size_t)m * g.N + n] * g.gs;
        }
    };
    const char* const ard = wl + (wk * 32 + l31) * FCG_RS + 16 * hi;
    const char* const brd = dl + (wm * 32 + l31) * FCG_RS + 16 * hi;
    gload(0);
    for (int nc = 0; nc < g.N; nc += 64) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) *reinterpret_cast<T*>(wl + (r0 + 4 * i) * FCG_RS + cn * 2) = (T)(wr[i]);
#pragma unroll
        for (int i = 0; i < 16; ++i) *reinterpret_cast<T*>(dl + (r0 + 4 * i) * FCG_RS + cn * 2) = (T)(dr[i]);
        if (nc + 64 < g.N) gload(nc + 64);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const v8 a = *reinterpret_cast<const v8*>(ard + 32 * ks);
            const v8 b = *reinterpret_cast<const v8*>(brd + 32 * ks);
            acc = E::mfma(a, b, acc);
        }
    }
    // lane = sample l31; registers 4 q .. 4 q + 3 are the c8 columns 8 q + 4 hi .. + 3 of the wave's 32 (half a cell)
    const int m = m0 + wm * 32 + l31;
    if (m >= g.M) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = kb0 + wk * 32 + 8 * q + 4 * hi;
        if (k >= g.Kc) continue;               // (Kc is a multiple of 8: the four columns are in or out together)
        const size_t o = (size_t)m * g.Kc + k;
        v4 y4;
        if (g.ya) y4 = *reinterpret_cast<const v4*>(static_cast<const T*>(g.ya) + o);
        v4 o4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = acc[4 * q + e];
            if (g.ya) v *= tn_act_grad_from_out((float)(y4[e]), g.act, g.prm);
            o4[e] = fcg_wrow(g, k + e) >= 0 ? (T)(v) : (T)(0.f);       // channels past C: exact +0
        }
        *reinterpret_cast<v4*>(static_cast<T*>(g.dx) + o) = o4;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// wgrad: grid = (Kc / 64, n_out / 64, S sample slabs)
// ---------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256) void fcg_wgrad_kernel(FCG g) {
    typedef typename E::T T;
    typedef typename E::v8 v8;
    __shared__ __attribute__((aligned(16))) char xl[64 * FCG_TS];      // [sample][c8 column]
    __shared__ __attribute__((aligned(16))) char dl[64 * FCG_TS];      // [sample][output]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const int k0 = blockIdx.x * 64, n0 = blockIdx.y * 64, z = blockIdx.z;
    const int mbeg = z * g.krange, mend = min(g.M, mbeg + g.krange);
    const int wk = wave & 1, wn = wave >> 1;
    f32x16 acc, accb;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.f; accb[r] = 0.f; }
    const bool want_db = blockIdx.x == 0 && wk == 0;
    const v8 ones = {(T)(1.f), (T)(1.f), (T)(1.f), (T)(1.f), (T)(1.f), (T)(1.f), (T)(1.f), (T)(1.f)};
    // staging roles: x sample row t >> 2, 16 columns from 16 (t & 3); dz output t & 63, sample rows (t >> 6) + 4 i
    const int xr_ = t >> 2, xk = k0 + 16 * (t & 3), dn = n0 + (t & 63), dr0 = t >> 6;
    fcg_u4 xr[2];
    float dr[16];
    auto gload = [&](int mc) __attribute__((always_inline)) {
        const int m = mc + xr_;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            xr[i] = fcg_u4{0u, 0u, 0u, 0u};
            if (m < mend && xk + 8 * i < g.Kc)
                xr[i] = *reinterpret_cast<const fcg_u4*>(static_cast<const T*>(g.x) + (size_t)m * g.Kc + xk + 8 * i);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int mm = mc + dr0 + 4 * i;
            dr[i] = 0.f;
            if (mm < mend && dn < g.N) dr[i] = g.dz[(size_t)mm * g.N + dn] * g.gs;
        }
    };
    const char* const ard = fcg_tr_base(xl, lane, wk * 32);
    const char* const brd = fcg_tr_base(dl, lane, wn * 32);
    gload(mbeg);
    for (int mc = mbeg; mc < mend; mc += 64) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<fcg_u4*>(xl + xr_ * FCG_TS + (16 * (t & 3) + 8 * i) * 2) = xr[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) *reinterpret_cast<T*>(dl + (dr0 + 4 * i) * FCG_TS + (t & 63) * 2) = (T)(dr[i]);
        if (mc + 64 < mend) gload(mc + 64);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const v8 a = fcg_tr_read<E>(ard, ks);
            const v8 b = fcg_tr_read<E>(brd, ks);
            acc = E::mfma(a, b, acc);
            if (want_db) accb = E::mfma(ones, b, accb);
        }
    }
    float* const wz = g.ws + (size_t)z * g.C * g.HW * g.N;
    const int n = n0 + wn * 32 + l31;
    if (n >= g.N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = fcg_wrow(g, k0 + wk * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi);
        if (row >= 0) wz[(size_t)row * g.N + n] = acc[r] * g.oscale;
    }
    // row 0 of the product with ones (every row is the column sum)
    if (want_db && hi == 0) g.dbws[(size_t)z * g.N + n] = accb[0] * g.oscale;
}

static unsigned fcg_magic(int HW) { return HW == 1 ? 0u : (unsigned)((1ull << 32) / (unsigned)HW + 1u); }

static bool fcg_shape_ok(int B, int C, int HW, int n_out) {
    if (B <= 0 || C <= 0 || HW <= 0 || n_out <= 0) return false;
    const uint64_t lim = 1ull << 31;
    const uint64_t cells = (uint64_t)((C + 7) / 8) * (uint64_t)HW;      // < 2^59
    if (cells * 8 >= lim) return false;
    const uint64_t Kc = cells * 8;
    return (uint64_t)B * Kc < lim && (uint64_t)B * (uint64_t)n_out < lim && (uint64_t)C * HW * (uint64_t)n_out < lim &&
           cells * (uint64_t)HW < (1ull << 32) && (B + 63) / 64 <= 65535 && (n_out + 63) / 64 <= 65535;
}

static int fcg_check(tn_ctx* ctx, int B, int C, int HW, int n_out, const char* what) {
    TN_REQUIRE(B > 0 && C > 0 && HW > 0 && n_out > 0, "%s: bad shape (%d samples, %d maps of %d pixels, %d outputs)", what, B, C,
               HW, n_out);
    TN_REQUIRE(fcg_shape_ok(B, C, HW, n_out), "%s: %d samples x %d maps of %d pixels -> %d outputs: too large (tn_c8_fcg_supported)",
               what, B, C, HW, n_out);
    return TN_OK;
}

extern "C" {

#ifndef C8_BF16_TU
// the bf16 entry points (fcg_c8_bf16.hip)
int c8b_tn_c8_fcg_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, float* a, int B, int C, int HW, int n_out,
                      int act, float act_param, const uint8_t* mask);
int c8b_tn_c8_fcg_fwd_dropout(tn_ctx* ctx, const void* x, const float* W, const float* b, float* a, int B, int C, int HW,
                              int n_out, int act, float act_param, uint8_t* mask_out, float pdrop, uint64_t seed,
                              uint32_t step, const uint32_t* d_step, uint64_t elem0);
int c8b_tn_c8_fcg_dgrad(tn_ctx* ctx, const float* dz, const float* W, void* dx, int B, int C, int HW, int n_out,
                        const void* y, int act, float act_param);
int c8b_tn_c8_fcg_wgrad(tn_ctx* ctx, const void* x, const float* dz, float* dW, float* db, int B, int C, int HW, int n_out);
#endif

// 1 if the general 16-bit-resident FC products take this layer: every shape within the limits of the header comment
int C8_API(tn_c8_fcg_supported)(int B, int C, int HW, int n_out) { return fcg_shape_ok(B, C, HW, n_out) ? 1 : 0; }

static int fcg_fwd_run(tn_ctx* ctx, const void* x, const float* W, const float* b, float* a, int B, int C, int HW, int n_out,
                       int act, float act_param, const uint8_t* mask, const FcgDrop& dr, const char* what) {
    int rc = fcg_check(ctx, B, C, HW, n_out, what);
    if (rc) return rc;
    TN_REQUIRE(x && W && b && a, "%s: NULL tensor", what);
    FCG g{};
    g.x = x; g.W = W; g.M = B; g.N = n_out; g.C = C; g.HW = HW;
    g.Kc = ((C + 7) / 8) * HW * 8;
    g.magic = fcg_magic(HW);
    const int colg = cdiv(n_out, 64), rowg = cdiv(B, 64);
    // K slabs: about one block per CU, at least four chunks of 64 columns per block
    int S = cdiv(ctx->num_cus, (long long)colg * rowg);
    if (S > g.Kc / 256) S = g.Kc / 256;
    if (S < 1) S = 1;
    g.krange = cdiv(cdiv(g.Kc, S), 64) * 64;
    S = cdiv(g.Kc, g.krange);
    g.S = S;
    const size_t MN = (size_t)B * n_out;
    rc = tn_scratch_get(ctx, (size_t)S * MN * sizeof(float), &g.ws);
    if (rc) return rc;
    fcg_fwd_kernel<C8E><<<dim3(colg, S, rowg), 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    fcg_fwd_finish_kernel<C8E><<<cdiv(MN, 256), 256, 0, ctx->stream>>>(g.ws, S, MN, n_out, b, mask, a, act, act_param, dr);
    TN_LAUNCH_CHECK();
    return TN_OK;
}
int C8_API(tn_c8_fcg_fwd)(tn_ctx* ctx, const void* x, const float* W, const float* b, float* a, int B, int C, int HW,
                          int n_out, int act, float act_param, const uint8_t* mask) {
    C8_TO_BF16(tn_c8_fcg_fwd, ctx, x, W, b, a, B, C, HW, n_out, act, act_param, mask);
    return fcg_fwd_run(ctx, x, W, b, a, B, C, HW, n_out, act, act_param, mask, FcgDrop{}, "tn_c8_fcg_fwd");
}
// the same with the dropout mask drawn by the finishing kernel (dropout.py:12: keep = u01 >= pdrop, no rescale) and
// written to mask_out: the numbers of tn_dropout_mask(mask_out, B * n_out, pdrop, seed, step, d_step, elem0)
int C8_API(tn_c8_fcg_fwd_dropout)(tn_ctx* ctx, const void* x, const float* W, const float* b, float* a, int B, int C,
                                  int HW, int n_out, int act, float act_param, uint8_t* mask_out, float pdrop,
                                  uint64_t seed, uint32_t step, const uint32_t* d_step, uint64_t elem0) {
    C8_TO_BF16(tn_c8_fcg_fwd_dropout, ctx, x, W, b, a, B, C, HW, n_out, act, act_param, mask_out, pdrop, seed, step, d_step,
               elem0);
    TN_REQUIRE(mask_out != nullptr, "tn_c8_fcg_fwd_dropout: NULL mask");
    FcgDrop dr{mask_out, pdrop, (uint32_t)seed, (uint32_t)(seed >> 32), step, d_step, elem0};
    return fcg_fwd_run(ctx, x, W, b, a, B, C, HW, n_out, act, act_param, nullptr, dr, "tn_c8_fcg_fwd_dropout");
}

// dx (B, Kc) elements = E(gs * dz . W^T * act'(y16)) in x's order, every cell written, channels past C zero
int C8_API(tn_c8_fcg_dgrad)(tn_ctx* ctx, const float* dz, const float* W, void* dx, int B, int C, int HW, int n_out,
                            const void* y, int act, float act_param) {
    C8_TO_BF16(tn_c8_fcg_dgrad, ctx, dz, W, dx, B, C, HW, n_out, y, act, act_param);
    int rc = fcg_check(ctx, B, C, HW, n_out, "tn_c8_fcg_dgrad");
    if (rc) return rc;
    TN_REQUIRE(dz && W && dx, "tn_c8_fcg_dgrad: NULL tensor");
    FCG g{};
    g.dz = dz; g.W = W; g.dx = dx; g.ya = y;
    g.M = B; g.N = n_out; g.C = C; g.HW = HW; g.Kc = ((C + 7) / 8) * HW * 8;
    g.act = act; g.prm = act_param; g.gs = ctx->grad_scale;
    g.magic = fcg_magic(HW);
    fcg_dgrad_kernel<C8E><<<dim3(cdiv(g.Kc, 64), cdiv(B, 64)), 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// dW (C*HW, n_out), db (n_out) fp32, OVERWRITE, from x and dz (fp32, rounded as E(gs * dz) while staged)
int C8_API(tn_c8_fcg_wgrad)(tn_ctx* ctx, const void* x, const float* dz, float* dW, float* db, int B, int C, int HW,
                            int n_out) {
    C8_TO_BF16(tn_c8_fcg_wgrad, ctx, x, dz, dW, db, B, C, HW, n_out);
    int rc = fcg_check(ctx, B, C, HW, n_out, "tn_c8_fcg_wgrad");
    if (rc) return rc;
    TN_REQUIRE(x && dz && dW && db, "tn_c8_fcg_wgrad: NULL tensor");
    FCG g{};
    g.x = x; g.dz = dz; g.M = B; g.N = n_out; g.C = C; g.HW = HW;
    g.Kc = ((C + 7) / 8) * HW * 8;
    g.magic = fcg_magic(HW);
    g.gs = ctx->grad_scale; g.oscale = 1.f / ctx->grad_scale;
    const int kb = cdiv(g.Kc, 64), nb = cdiv(n_out, 64);
    // sample slabs: about one block per CU, whole chunks of 64 samples
    int S = cdiv(ctx->num_cus, (long long)kb * nb);
    if (S > cdiv(B, 64)) S = cdiv(B, 64);
    if (S > 65535) S = 65535;
    if (S < 1) S = 1;
    g.krange = cdiv(cdiv(B, S), 64) * 64;
    S = cdiv(B, g.krange);
    g.S = S;
    if (S == 1) {
        g.ws = dW; g.dbws = db;                // (channels beyond C own no row of dW: every row is written)
        fcg_wgrad_kernel<C8E><<<dim3(kb, nb, 1), 256, 0, ctx->stream>>>(g);
        TN_LAUNCH_CHECK();
        return TN_OK;
    }
    const size_t n = (size_t)C * HW * n_out;
    rc = tn_scratch_get(ctx, ((size_t)S * n + (size_t)S * n_out) * sizeof(float), &g.ws);
    if (rc) return rc;
    g.dbws = g.ws + (size_t)S * n;
    fcg_wgrad_kernel<C8E><<<dim3(kb, nb, S), 256, 0, ctx->stream>>>(g);
    TN_LAUNCH_CHECK();
    return tn_red_wgrad(ctx, g.ws, dW, (uint32_t)n, (uint32_t)S, (uint32_t)n, g.dbws, db, (uint32_t)n_out, (uint32_t)S,
                        (uint32_t)n_out);
}

}  // extern "C"
