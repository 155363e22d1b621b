// DTYPE 'float16' / 'bfloat16', an output head on the 16-bit conv stack (STACK_HEAD 'any'): tn_c8_head_fwd and
// tn_c8_head_softmax_nll, the affine map of a head with a handful of outputs (n_out <= 16: the classes) read straight from
// the c8 tensor, each ONE launch -- the counterpart of fc_skinny.hip's "one launch for <= 16 classes" on the stack.  The
// dense families (fc_c8.hip, fcg_c8.hip) cut 64- or 32-wide output tiles, so ten classes are mostly padding there, and they
// need a finishing launch for their K slabs and a third one for the softmax rows.
//
// The arithmetic is tn_c8_fcg_fwd's, argument for argument: x as stored (the flattened c8 tensor of C maps of HW pixels,
// Kc = ceil(C/8) * HW * 8 elements a sample), W (C*HW, n_out) fp32 in the reference's NCHW-flattened row order walked
// through the row map k -> (8 o + e) * HW + p and rounded nearest-even to the element type while it is loaded, exact
// products, fp32 accumulation on v_mfma_f32_16x16x32_f16 / _bf16, bias and activation on the fp32 sum, z fp32.
//
// Tiling: block = 16 samples x 16 outputs, 1 to 16 waves.  A c8 cell (16 bytes: 8 consecutive reduction indices of one
// sample) IS the per-lane A operand of the 16x16x32 MFMA -- lane l holds row l & 15, k = 8 (l >> 4) + j -- so x goes from
// global memory into the operand, no LDS staging; a reduction step is 4 cells.  The B operand follows the same
// enumeration: lane l loads the 8 rows of W of its cell for output l & 15 (W is small and L2-resident) and rounds them.
// The block's waves split the steps into contiguous runs of nearly equal length (wave w of n: steps [w S / n, (w+1) S / n);
// n = ceil(S / HD_U) up to 16 -- a function of the shape alone, so the bits do not depend on the device -- which for the
// heads of the nets puts every load of a block in flight at once), HD_U steps' loads issued before their products, and
// meet in LDS; wave 0 adds the partial sums in wave order.  A row's outputs then sit in the 16 lanes of one DPP row
// of the accumulator layout (column = lane & 15), which is where the softmax / NLL tail reduces them (fc_skinny.hip's tail: tn_softmax_nll's
// statement).  A ragged cell tail (cells % 4), steps past the last one, outputs past n_out and channels past C feed
// zeros: rows of W for channels past C are never read, nothing is read or written past an operand, no alignment of n_out
// is assumed.  No atomics, no scratch: the same call gives the same bits, and the logits of tn_c8_head_softmax_nll are
// tn_c8_head_fwd's linear z bit for bit (the same product code, the same order of the sums).
//
// Traffic: every block of 16 samples walks the whole of W -- 4 n_out bytes of W for 16 x 2 bytes of x per reduction index, at
// cifar_head's shape 80 KB of W for 64 KB of x a block -- as per-lane dword loads at a stride of HW * n_out floats, rounded
// in every block.  W is read from HBM once and from L2 after that (all of it is a few hundred KB at most for n_out <= 16);
// staging the rounded W of a step in LDS once per block, or 32 samples a block, would halve that L2 traffic: not done.
//
// Limits (tn_c8_head_supported; the ops refuse by name, nothing launched): 1 <= n_out <= 16 and tn_c8_fcg_supported's
// index limits; TN_C8_HEAD=0 (knobs.h) switches the family off.
#include "c8_elem.h"

typedef float hd_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned hd_u4 __attribute__((ext_vector_type(4)));

#define HD_U 4              // reduction steps of a wave whose loads are in flight together

__device__ __forceinline__ hd_f32x4 hd_mfma(C8H::v8 a, C8H::v8 b, hd_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ hd_f32x4 hd_mfma(C8B::v8 a, C8B::v8 b, hd_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

struct HD {
    const void* x;          // (B, Kc) elements
    const float* W;         // (C * HW, N)
    const float* b;         // (N)
    float* z;               // (B, N)
    int B, N, Kc, C, HW, cells, steps, waves, act;
    unsigned magic;         // 2^32 / HW + 1 (0: HW == 1)
    float prm;
};

struct HdSoftmax {          // the softmax / NLL tail's outputs (tn_softmax_nll's)
    const int32_t* y;
    int64_t y_row0;
    const int64_t* d_row0;
    float* logprob;
    float* rowloss;
    int32_t* pred;
    float* rowp;
    float* dz;
    float inv_batch;
};

template <int CTRL>
__device__ __forceinline__ float hd_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// all-reduce over the 16 lanes of a DPP row: quad xor 1, quad xor 2, half mirror, mirror
__device__ __forceinline__ float hd_row_max(float v) {
    v = fmaxf(v, hd_dpp<0xB1>(v));
    v = fmaxf(v, hd_dpp<0x4E>(v));
    v = fmaxf(v, hd_dpp<0x141>(v));
    return fmaxf(v, hd_dpp<0x140>(v));
}
__device__ __forceinline__ float hd_row_min(float v) {
    v = fminf(v, hd_dpp<0xB1>(v));
    v = fminf(v, hd_dpp<0x4E>(v));
    v = fminf(v, hd_dpp<0x141>(v));
    return fminf(v, hd_dpp<0x140>(v));
}
__device__ __forceinline__ float hd_row_sum(float v) {
    v += hd_dpp<0xB1>(v);
    v += hd_dpp<0x4E>(v);
    v += hd_dpp<0x141>(v);
    return v + hd_dpp<0x140>(v);
}

#define HD_WAVES 16         // of a block, at most

// grid = ceil(B / 16), block = g.waves waves; SM: the softmax / NLL tail instead of the activation epilogue
template <typename E, bool SM>
__global__ __launch_bounds__(64 * HD_WAVES) void head_kernel(HD g, HdSoftmax sm) {
    typedef typename E::T T;
    typedef typename E::v8 v8;
    extern __shared__ float red_[];                  // [g.waves][256]: the waves' partial sums
    float (*const red)[256] = reinterpret_cast<float (*)[256]>(red_);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lo = lane & 15, qd = lane >> 4;
    const T* const xr = static_cast<const T*>(g.x) + (size_t)min((int)blockIdx.x * 16 + lo, g.B - 1) * g.Kc;
    const bool nlive = lo < g.N;
    const float* const Wc = g.W + min(lo, g.N - 1);
    hd_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // the wave's run of steps
    const int send = (int)(((long long)(w + 1) * g.steps) / g.waves);
    for (int s0 = (int)(((long long)w * g.steps) / g.waves); s0 < send; s0 += HD_U) {
        hd_u4 xv[HD_U];
        float wv[HD_U][8];
#pragma unroll
        for (int i = 0; i < HD_U; ++i) {
            // the lane's cell of step s0 + i; past the run's end or the last cell (a ragged tail): zeros
            const int cell = 4 * (s0 + i) + qd;
            const bool in = s0 + i < send && cell < g.cells;
            xv[i] = hd_u4{0u, 0u, 0u, 0u};
            if (in) xv[i] = *reinterpret_cast<const hd_u4*>(xr + (size_t)cell * 8);
            // (o, p) = (cell / HW, cell % HW): the division by the magic is exact while cell * HW < 2^32 (the host checks)
            const int o = g.magic ? (int)__umulhi((unsigned)cell, g.magic) : cell;
            const int p = cell - o * g.HW;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int ch = 8 * o + e;
                wv[i][e] = 0.f;
                if (in && nlive && ch < g.C) wv[i][e] = Wc[((size_t)ch * g.HW + p) * g.N];
            }
        }
#pragma unroll
        for (int i = 0; i < HD_U; ++i) {
            const v8 bv = {(T)(wv[i][0]), (T)(wv[i][1]), (T)(wv[i][2]), (T)(wv[i][3]),
                           (T)(wv[i][4]), (T)(wv[i][5]), (T)(wv[i][6]), (T)(wv[i][7])};
            acc = hd_mfma(__builtin_bit_cast(v8, xv[i]), bv, acc);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][r * 64 + lane] = acc[r];
    __syncthreads();
    if (w != 0) return;
    const float bias = nlive ? g.b[lo] : 0.f;
    if (!SM) {
        if (!nlive) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = blockIdx.x * 16 + 4 * qd + r;        // accumulator row of register r
            float s = red[0][r * 64 + lane];
            for (int v = 1; v < g.waves; ++v) s += red[v][r * 64 + lane];
            if (row < g.B) g.z[(size_t)row * g.N + lo] = tn_act_fwd(s + bias, g.act, g.prm);
        }
        return;
    }
    // softmax / NLL tail: a row's logits sit in the 16 lanes of one DPP row (lane lo = class)
    const int64_t yoff = sm.y_row0 + (sm.d_row0 ? *sm.d_row0 : 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = blockIdx.x * 16 + 4 * qd + r;
        const int rowc = min(row, g.B - 1);
        float s = red[0][r * 64 + lane];
        for (int v = 1; v < g.waves; ++v) s += red[v][r * 64 + lane];
        const float z = s + bias;
        const float zv = nlive ? z : -INFINITY;
        const float m = hd_row_max(zv);
        // first maximal class (numpy argmax)
        const float am = hd_row_min((nlive && zv == m) ? (float)lo : 1e9f);
        const float se = hd_row_sum(nlive ? expf(zv - m) : 0.f);
        const float lp = zv - m - logf(se);
        const int label = sm.y ? sm.y[yoff + rowc] : -1;
        if (nlive && row < g.B) {
            const size_t o = (size_t)row * g.N + lo;
            g.z[o] = z;
            sm.logprob[o] = lp;
            if (sm.dz) sm.dz[o] = (expf(lp) - (lo == label ? 1.f : 0.f)) * sm.inv_batch;
            if (lo == label) {
                if (sm.rowloss) sm.rowloss[row] = -lp;
                if (sm.rowp) sm.rowp[row] = expf(lp);
            }
            if (lo == 0) sm.pred[row] = (int)am;
        }
    }
}

extern "C" {

#ifndef C8_BF16_TU
// the bf16 entry points (head_c8_bf16.hip)
int c8b_tn_c8_head_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, float* z, int B, int C, int HW, int n_out,
                       int act, float act_param);
int c8b_tn_c8_head_softmax_nll(tn_ctx* ctx, const void* x, const float* W, const float* b, float* logits, int B, int C, int HW,
                               int n_out, const int32_t* y, int64_t y_row0, const int64_t* d_row0, float* logprob,
                               float* rowloss, int32_t* pred, float* rowp, float* dz, float inv_batch);
#endif

// 1 if the head kernels take this layer: at most 16 outputs, within the index limits of the general dense family
// (TN_C8_HEAD 0: never -- heads then take the dense families' forward and the row kernels)
int C8_API(tn_c8_head_supported)(int B, int C, int HW, int n_out) {
    return tn_knob(TN_K_C8_HEAD) && n_out >= 1 && n_out <= 16 && tn_c8_fcg_supported(B, C, HW, n_out) ? 1 : 0;
}

// the waves of a block: one for every HD_U steps (their loads are in flight together), at most HD_WAVES
static int hd_waves(int steps) { return steps >= HD_U * HD_WAVES ? HD_WAVES : cdiv(steps, HD_U); }

static int hd_setup(tn_ctx* ctx, HD& g, const void* x, const float* W, const float* b, float* z, int B, int C, int HW,
                    int n_out, const char* what) {
    TN_REQUIRE(B > 0 && C > 0 && HW > 0 && n_out > 0, "%s: bad shape (%d samples, %d maps of %d pixels, %d outputs)", what, B, C,
               HW, n_out);
    TN_REQUIRE(C8_API(tn_c8_head_supported)(B, C, HW, n_out),
               "%s: %d samples x %d maps of %d pixels -> %d outputs: more than 16 outputs or too large (tn_c8_head_supported)",
               what, B, C, HW, n_out);
    TN_REQUIRE(x && W && b && z, "%s: NULL tensor", what);
    g.x = x; g.W = W; g.b = b; g.z = z;
    g.B = B; g.N = n_out; g.C = C; g.HW = HW;
    g.cells = ((C + 7) / 8) * HW;
    g.Kc = g.cells * 8;
    g.steps = cdiv(g.cells, 4);
    g.waves = hd_waves(g.steps);
    g.magic = HW == 1 ? 0u : (unsigned)((1ull << 32) / (unsigned)HW + 1u);
    return TN_OK;
}

// z (B, n_out) fp32 = act(x . W16 + b)
int C8_API(tn_c8_head_fwd)(tn_ctx* ctx, const void* x, const float* W, const float* b, float* z, int B, int C, int HW,
                           int n_out, int act, float act_param) {
    C8_TO_BF16(tn_c8_head_fwd, ctx, x, W, b, z, B, C, HW, n_out, act, act_param);
    HD g{};
    int rc = hd_setup(ctx, g, x, W, b, z, B, C, HW, n_out, "tn_c8_head_fwd");
    if (rc) return rc;
    g.act = act; g.prm = act_param;
    head_kernel<C8E, false><<<cdiv(B, 16), 64 * g.waves, 1024 * g.waves, ctx->stream>>>(g, HdSoftmax{});
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// logits = x . W16 + b and tn_softmax_nll's statement on them, in the same launch
int C8_API(tn_c8_head_softmax_nll)(tn_ctx* ctx, const void* x, const float* W, const float* b, float* logits, int B, int C,
                                   int HW, int n_out, const int32_t* y, int64_t y_row0, const int64_t* d_row0,
                                   float* logprob, float* rowloss, int32_t* pred, float* rowp, float* dz, float inv_batch) {
    C8_TO_BF16(tn_c8_head_softmax_nll, ctx, x, W, b, logits, B, C, HW, n_out, y, y_row0, d_row0, logprob, rowloss, pred, rowp,
               dz, inv_batch);
    HD g{};
    int rc = hd_setup(ctx, g, x, W, b, logits, B, C, HW, n_out, "tn_c8_head_softmax_nll");
    if (rc) return rc;
    TN_REQUIRE(logprob && pred, "tn_c8_head_softmax_nll: NULL tensor");
    TN_REQUIRE(y != nullptr || (rowloss == nullptr && dz == nullptr && rowp == nullptr),
               "tn_c8_head_softmax_nll: labels required for loss/gradient outputs");
    HdSoftmax sm{y, y_row0, d_row0, logprob, rowloss, pred, rowp, dz, inv_batch};
    head_kernel<C8E, true><<<cdiv(B, 16), 64 * g.waves, 1024 * g.waves, ctx->stream>>>(g, sm);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// what a call launches (no device): op 0 tn_c8_head_fwd / 1 tn_c8_head_softmax_nll -> instantiation (= op: the epilogue),
// row tiles (blocks), reduction steps, waves of a block, steps of the busiest wave, rows of the last tile that are padding,
// cells of the last step that are padding, channels of the last octet that are padding, HW == 1 (no division in the row
// map)
int C8_API(tn_c8_head_plan)(int op, int B, int C, int HW, int n_out, int* out, int nout) {
    if ((op != 0 && op != 1) || !C8_API(tn_c8_head_supported)(B, C, HW, n_out) || (nout > 0 && !out)) return TN_E_ARG;
    const int cells = ((C + 7) / 8) * HW, steps = cdiv(cells, 4), waves = hd_waves(steps);
    const int v[9] = {op, cdiv(B, 16), steps, waves, cdiv(steps, waves), (16 - B % 16) % 16, (4 - cells % 4) % 4,
                      (8 - C % 8) % 8, HW == 1};
    for (int k = 0; k < 9 && k < nout; ++k) out[k] = v[k];
    return 9;
}

}  // extern "C"
