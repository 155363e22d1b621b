// DTYPE 'float16' / 'bfloat16': a PoolLayer whose stride differs from its window (Theano's pool_2d(..., st=), overlapping
// or gapped max-pooling) on the 16-bit-resident conv stack.  Window (i, j) of a p x p, stride st pool covers rows
// i * st .. min(S, i * st + p) - 1 and the same columns: clipped at the map edge, never padded; with st > p some pixels lie
// in no window.  On c8 tensors (pool_c8.hip: S x S maps at pitch P; y: So x So maps at pitch Po):
//   forward   pool_c8.hip's, with the window's origin at (i * st, j * st): the maximum of the STORED values, compared
//             through the ordered integer key, scanned row-major and replaced on strict >; a stored pattern, chosen, never
//             rounded.  Pad cells of y and channels >= C are written as 0; every cell of y is written.  Element-type blind.
//   backward  gin[pos] = the sum of gout[i, j] over every window (i, j) that covers pos and whose maximum equals x[pos] by
//             value (-0 == +0 is a tie; every tied element gets the whole gradient -- Theano's MaxPoolGrad).  The windows
//             that cover row h are i = max(0, ceil((h - p + 1) / st)) .. min(So - 1, h / st), columns likewise; their
//             terms are added in fp32 in row-major window order, the running sum starting from the first term (not from
//             zero: a single term -- stride = window -- is copied bit for bit), and the sum is rounded ONCE, to nearest
//             even, to the element type.  A position with no term (no covering window, no tie, pad cells, channels >= C)
//             gets +0; every cell of gin is written.  The activation derivative of the block below is NOT applied here
//             (PoolLayer.act_info looks through: every contributing window's maximum equals x[pos]).
// The tie test is the forward's key compare; the sum converts 16-bit <-> fp32, which differs for halfs and bf16, so the
// backward is instantiated per element type (plain casts, c8_elem.h) -- both in this unit: it holds no other kernels.
//
// The shape is pool_c8.hip's: one 16-byte cell per lane and access, lane-contiguous stores, plain vector loads and stores,
// no LDS, no atomics -- the backward is a GATHER, a lane per INPUT cell that reads its own x cell and the y and gout cells
// of at most ceil(p / st)^2 covering windows, keeps eight fp32 running sums and writes gin once: one result whatever the
// schedule.  A compile-time (window, stride) -- (3, 2) and (2, 1) -- issues all its loads before the first compare: the
// forward's coordinates past the clipped window are clamped onto its last row / column (pool_c8.hip), the backward's
// candidate windows that do not exist or do not cover the position are clamped into the map and masked out.  Every other
// (p, st) takes run-time loops.
#include "c8_elem.h"
#include "pool_c8.h"

// PW, ST: window and stride as compile-time constants, or 0, 0: p and st at run time.  SH: the OUTPUT pitch is a power of two.
template <int PW, int ST, bool SH>
__global__ __launch_bounds__(256) void c8_pool_st_fwd_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                            unsigned cells, int C, unsigned C8, unsigned S, unsigned P,
                                                            unsigned p_rt, unsigned st_rt, unsigned So, unsigned Po,
                                                            int lgPo) {
    const unsigned cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    const unsigned p = PW ? (unsigned)PW : p_rt, st = PW ? (unsigned)ST : st_rt;
    unsigned pair, i, j;
    c8p_where<SH>(cell, Po, lgPo, pair, i, j);
    uint4 out = make_uint4(0u, 0u, 0u, 0u);
    if (i < So && j < So) {
        const unsigned y0 = i * st, x0 = j * st;                   // (So - 1) * st < S: the window holds (y0, x0)
        const unsigned y1 = min(S, y0 + p), x1 = min(S, x0 + p);
        const uint4* xp = x + (size_t)pair * P * P;
        c8p_cell best, kb;
        if (PW) {
            c8p_cell v[PW ? PW * PW : 1];
#pragma unroll
            for (int dy = 0; dy < PW; ++dy)
#pragma unroll
                for (int dx = 0; dx < PW; ++dx)
                    v[dy * PW + dx] = c8p_load(xp + (min(y0 + dy, y1 - 1u) * P + min(x0 + dx, x1 - 1u)));
            best = v[0];
#pragma unroll
            for (int q = 0; q < 4; ++q) kb.d[q] = c8p_key(best.d[q]);
#pragma unroll
            for (int e = 1; e < PW * PW; ++e) c8p_take(best, kb, v[e]);
        } else {
            best = c8p_load(xp + (y0 * P + x0));
#pragma unroll
            for (int q = 0; q < 4; ++q) kb.d[q] = c8p_key(best.d[q]);
            for (unsigned yy = y0; yy < y1; ++yy) {
                const uint4* xr = xp + yy * P;
                for (unsigned xx = x0; xx < x1; ++xx) c8p_take(best, kb, c8p_load(xr + xx));
            }
        }
        out = c8p_and(c8p_quad(best), c8p_valid(pair, C, C8));
    }
    y[cell] = out;
}

// One window's term of the backward: where x ties with the window's maximum yv, sum <- sum + gout (fp32) and the lane is
// marked in ``have``.  The sums start at -0, so the first term enters as itself (-0 + g == g for every g, -0 included).
template <typename E>
__device__ __forceinline__ void c8ps_add(float (&sum)[8], c8p_cell& have, const c8p_cell& kx, const c8p_cell& yv, uint4 gq,
                                         bool on) {
    union { uint4 q; typename E::v8 v; } g;
    g.q = gq;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        c8p_i16x2 m = c8p_eq(kx.d[q], c8p_key(yv.d[q]));
        if (!on) m = (short)0;
        have.d[q] |= m;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float t = sum[2 * q + e] + (float)g.v[2 * q + e];
            sum[2 * q + e] = m[e] ? t : sum[2 * q + e];
        }
    }
}

// E: the element type.  PW, ST as above.  SH: the INPUT pitch is a power of two.
template <typename E, int PW, int ST, bool SH>
__global__ __launch_bounds__(256) void c8_pool_st_bwd_kernel(const uint4* __restrict__ x, const uint4* __restrict__ y,
                                                            const uint4* __restrict__ gout, uint4* __restrict__ gin,
                                                            unsigned cells, int C, unsigned C8, unsigned S, unsigned P,
                                                            int lgP, unsigned p_rt, unsigned st_rt, unsigned So,
                                                            unsigned Po) {
    constexpr int NW = PW ? (PW + ST - 1) / ST : 1;              // candidate windows along an axis
    const unsigned cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    const int p = PW ? PW : (int)p_rt, st = PW ? ST : (int)st_rt;
    unsigned pair, hu, wu;
    c8p_where<SH>(cell, P, lgP, pair, hu, wu);
    uint4 out = make_uint4(0u, 0u, 0u, 0u);
    if (hu < S && wu < S) {
        const int h = (int)hu, w = (int)wu, last = (int)So - 1;
        const uint4* yp = y + (size_t)pair * Po * Po;
        const uint4* gp = gout + (size_t)pair * Po * Po;
        c8p_cell kx = c8p_load(x + cell), have;
        float sum[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            kx.d[q] = c8p_key(kx.d[q]);
            have.d[q] = (short)0;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) sum[e] = -0.f;
        const int ih = h / st, jh = w / st;                      // the last window that can cover the row / column
        if (PW) {
            // candidates ih - NW + 1 .. ih and jh - NW + 1 .. jh in row-major order: all loads, then the terms
            c8p_cell yv[NW * NW];
            uint4 gv[NW * NW];
            bool on[NW * NW];
#pragma unroll
            for (int a = 0; a < NW; ++a)
#pragma unroll
                for (int b = 0; b < NW; ++b) {
                    const int i = ih - (NW - 1) + a, j = jh - (NW - 1) + b;
                    on[a * NW + b] = i >= 0 && i <= last && i * ST + PW > h && j >= 0 && j <= last && j * ST + PW > w;
                    const unsigned o = (unsigned)min(max(i, 0), last) * Po + (unsigned)min(max(j, 0), last);
                    yv[a * NW + b] = c8p_load(yp + o);
                    gv[a * NW + b] = gp[o];
                }
#pragma unroll
            for (int k = 0; k < NW * NW; ++k) c8ps_add<E>(sum, have, kx, yv[k], gv[k], on[k]);
        } else {
            const int i0 = h >= p ? (h - p + st) / st : 0, i1 = min(last, ih);
            const int j0 = w >= p ? (w - p + st) / st : 0, j1 = min(last, jh);
            for (int i = i0; i <= i1; ++i)
                for (int j = j0; j <= j1; ++j) {
                    const unsigned o = (unsigned)i * Po + (unsigned)j;
                    c8ps_add<E>(sum, have, kx, c8p_load(yp + o), gp[o], true);
                }
        }
        union { uint4 q; typename E::v8 v; } r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r.v[e] = (typename E::T)sum[e];
        out = c8p_and(c8p_and(r.q, c8p_quad(have)), c8p_valid(pair, C, C8));
    }
    gin[cell] = out;
}

// the output side of S pixels under a p x p window at stride st (Theano's Pool.out_shape), -1 where there is none
static int c8ps_side(int S, int p, int st, int ignore_border) {
    if (ignore_border) return S >= p ? (S - p) / st + 1 : -1;
    if (st >= p) return (S - 1) / st + 1;
    const int r = S - 1 - p + st;
    return (r > 0 ? r / st : 0) + 1;
}

// The launchers' whole choice: the (window, stride) instantiation -- (3, 2), (2, 1); (0, 0): run-time loops -- and whether
// the pitch the op's lanes are laid over (forward: Po, backward: P) is a power of two.  tn_c8_pool_st_plan reports it.
struct c8ps_plan {
    int pw, st, sh, lg;
};

static c8ps_plan c8ps_choose(int op, int P, int p, int st, int Po) {
    c8ps_plan pl;
    const bool fixed = (p == 3 && st == 2) || (p == 2 && st == 1);
    pl.pw = fixed ? p : 0;
    pl.st = fixed ? st : 0;
    pl.lg = c8p_lg(op == 0 ? Po : P);
    pl.sh = pl.lg >= 0;
    return pl;
}

extern "C" {

int tn_c8_pool_st_supported(int N, int C, int S, int P, int p, int st, int So, int Po) {
    if (p < 2 || p > 64 || st < 1 || st > 64 || So < 1 || S < 1) return 0;
    if (So != c8ps_side(S, p, st, 1) && So != c8ps_side(S, p, st, 0)) return 0;
    return c8p_cells(N, C, S, P) > 0 && c8p_cells(N, C, So, Po) > 0;
}

#define C8PS_ARGS_FMT "(N %d C %d, maps of %d pixels at pitch %d, window %d stride %d, output %d pixels at pitch %d)"

#define C8PS_DISPATCH(GO)                                                       \
    do {                                                                        \
        if (pl.pw == 3) { if (pl.sh) GO(3, 2, true); else GO(3, 2, false); }     \
        else if (pl.pw == 2) { if (pl.sh) GO(2, 1, true); else GO(2, 1, false); } \
        else { if (pl.sh) GO(0, 0, true); else GO(0, 0, false); }                \
    } while (0)

int tn_c8_pool_st_fwd(tn_ctx* ctx, const void* x, void* y, int N, int C, int S, int P, int p, int st, int So, int Po) {
    TN_REQUIRE(x && y && tn_c8_pool_st_supported(N, C, S, P, p, st, So, Po), "tn_c8_pool_st_fwd: bad arguments " C8PS_ARGS_FMT,
               N, C, S, P, p, st, So, Po);
    const long long cells = c8p_cells(N, C, So, Po);
    const c8ps_plan pl = c8ps_choose(0, P, p, st, Po);
    const unsigned grid = (unsigned)cdiv(cells, 256);
#define C8PS_FWD_GO(PW, ST, SH)                                                                                          \
    c8_pool_st_fwd_kernel<PW, ST, SH><<<grid, 256, 0, ctx->stream>>>(                                                     \
        static_cast<const uint4*>(x), static_cast<uint4*>(y), (unsigned)cells, C, (unsigned)((C + 7) / 8), (unsigned)S, \
        (unsigned)P, (unsigned)p, (unsigned)st, (unsigned)So, (unsigned)Po, pl.lg)
    C8PS_DISPATCH(C8PS_FWD_GO);
#undef C8PS_FWD_GO
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_c8_pool_st_bwd(tn_ctx* ctx, const void* x, const void* y, const void* gout, void* gin, int N, int C, int S, int P,
                      int p, int st, int So, int Po) {
    TN_REQUIRE(x && y && gout && gin && tn_c8_pool_st_supported(N, C, S, P, p, st, So, Po),
               "tn_c8_pool_st_bwd: bad arguments " C8PS_ARGS_FMT, N, C, S, P, p, st, So, Po);
    const long long cells = c8p_cells(N, C, S, P);
    const c8ps_plan pl = c8ps_choose(1, P, p, st, Po);
    const unsigned grid = (unsigned)cdiv(cells, 256);
#define C8PS_BWD_E(E, PW, ST, SH)                                                                                       \
    c8_pool_st_bwd_kernel<E, PW, ST, SH><<<grid, 256, 0, ctx->stream>>>(                                                 \
        static_cast<const uint4*>(x), static_cast<const uint4*>(y), static_cast<const uint4*>(gout), static_cast<uint4*>(gin), \
        (unsigned)cells, C, (unsigned)((C + 7) / 8), (unsigned)S, (unsigned)P, pl.lg, (unsigned)p, (unsigned)st, (unsigned)So, \
        (unsigned)Po)
#define C8PS_BWD_GO(PW, ST, SH) \
    do { if (tn_c8_bf16(ctx)) C8PS_BWD_E(C8B, PW, ST, SH); else C8PS_BWD_E(C8H, PW, ST, SH); } while (0)
    C8PS_DISPATCH(C8PS_BWD_GO);
#undef C8PS_BWD_GO
#undef C8PS_BWD_E
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// op 0: tn_c8_pool_st_fwd -> c8_pool_st_fwd_kernel<PW, ST, SH>, op 1: tn_c8_pool_st_bwd -> c8_pool_st_bwd_kernel<E, PW,
// ST, SH>; the plan is PW, ST, SH, blocks of 256 lanes.  No device, no context.
int tn_c8_pool_st_plan(int op, int N, int C, int S, int P, int p, int st, int So, int Po, int* out, int nout) {
    if ((op != 0 && op != 1) || !tn_c8_pool_st_supported(N, C, S, P, p, st, So, Po) || (nout > 0 && !out)) return TN_E_ARG;
    const c8ps_plan pl = c8ps_choose(op, P, p, st, Po);
    const long long cells = op == 0 ? c8p_cells(N, C, So, Po) : c8p_cells(N, C, S, P);
    const int v[4] = {pl.pw, pl.st, pl.sh, cdiv(cells, 256)};
    for (int k = 0; k < 4 && k < nout; ++k) out[k] = v[k];
    return 4;
}

}  // extern "C"
