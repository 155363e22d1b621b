// DTYPE 'float16' / 'bfloat16': a stand-alone PoolLayer (theanet/layer/convpool.py:97-127: max-pool, stride = window, the
// last window clipped at the map edge or -- ignore_border -- dropped) on the 16-bit-resident conv stack, for every pool the
// fused conv + pool block does not take: any window 2 <= p <= 64 on any map, above a ConvLayer, a PoolLayer or a
// DropOutLayer.  On c8 tensors ([N][ceil(C/8)][P][P][8] 16-bit values, S x S maps at pitch P; y: So x So maps at pitch Po):
//   forward   y = max over the clipped window of the STORED values: a stored value, chosen, never rounded.  The window is
//             scanned row-major and replaced on strict >, so of equal values the first one's pattern is kept (+0 before
//             -0 gives +0).  Pad cells of y and channels >= C are written as 0; every cell of y is written.
//   backward  gin[pos] = value(x[pos]) == value(y[window(pos)]) ? gout[window(pos)] : +0 -- every tied maximum receives
//             the whole gradient (tn_pool_bwd, Theano's MaxPoolGrad), -0 == +0 is a tie; positions no window covers
//             (the ignore_border remainder, pad cells, channels >= C) get +0; the selected values are copied bit for
//             bit; every cell of gin is written.  The activation derivative of the block below is NOT applied here: the
//             layer looks through (PoolLayer.act_info), so whoever produced gout has applied act'(y) and rounded once --
//             and every element that receives gradient equals its window's maximum, act'(y) == act'(x[pos]).
//   test version: the forward.  Inputs are NaN-free.
//
// Comparison is by VALUE, and halfs and bf16 are both sign-magnitude formats whose order is the order of their patterns:
// key(u) = u < 0x8000 ? u : -(u & 0x7fff) is a signed 16-bit integer that grows with the value and sends
// both zeros to 0, whatever the split between exponent and fraction.  So both ops are element-type blind (like the
// train ops of drop_c8.hip) and exist once; subnormals compare as the values they are.
//
// Both ops are memory streams of 16-byte cells: one uint4 per lane and access, lane-contiguous stores (1 KiB per wave and
// instruction), plain vector loads and stores, no atomics, no LDS -- one result whatever the schedule.  The forward gives
// a lane to each OUTPUT cell (pad cells included: they are written as 0); a compile-time window (p = 2, 3) issues its
// p * p loads before the first compare -- coordinates past the clipped window are clamped onto its last row / column, a
// repeat of an element already seen that strict > never selects -- and any other p takes a run-time loop.  The backward
// gives a lane to each INPUT cell, which reads its own x cell and its window's y and gout cells and writes gin once.
#include "pool_c8.h"

// PW: the window as a compile-time constant (2, 3) or 0: p at run time.  SH: the OUTPUT pitch is a power of two.
template <int PW, bool SH>
__global__ __launch_bounds__(256) void c8_pool_fwd_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, unsigned cells,
                                                         int C, unsigned C8, unsigned S, unsigned P, unsigned p_rt,
                                                         unsigned So, unsigned Po, int lgPo) {
    const unsigned cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    const unsigned p = PW ? (unsigned)PW : p_rt;
    unsigned pair, i, j;
    c8p_where<SH>(cell, Po, lgPo, pair, i, j);
    uint4 out = make_uint4(0u, 0u, 0u, 0u);
    if (i < So && j < So) {
        const unsigned y0 = i * p, x0 = j * p;                     // (So - 1) * p < S: the window holds (y0, x0)
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

// SH: the INPUT pitch is a power of two.
template <int PW, bool SH>
__global__ __launch_bounds__(256) void c8_pool_bwd_kernel(const uint4* __restrict__ x, const uint4* __restrict__ y,
                                                         const uint4* __restrict__ gout, uint4* __restrict__ gin,
                                                         unsigned cells, int C, unsigned C8, unsigned S, unsigned P,
                                                         int lgP, unsigned p_rt, unsigned So, unsigned Po) {
    const unsigned cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    const unsigned p = PW ? (unsigned)PW : p_rt;
    unsigned pair, h, w;
    c8p_where<SH>(cell, P, lgP, pair, h, w);
    uint4 out = make_uint4(0u, 0u, 0u, 0u);
    const unsigned i = h / p, j = w / p;
    if (h < S && w < S && i < So && j < So) {
        const size_t o = ((size_t)pair * Po + i) * Po + j;
        const c8p_cell xv = c8p_load(x + cell), yv = c8p_load(y + o);
        const uint4 gv = gout[o];
        c8p_cell m;
#pragma unroll
        for (int q = 0; q < 4; ++q) m.d[q] = c8p_eq(c8p_key(xv.d[q]), c8p_key(yv.d[q]));
        out = c8p_and(c8p_and(gv, c8p_quad(m)), c8p_valid(pair, C, C8));
    }
    gin[cell] = out;
}

// The launchers' whole choice: the window instantiation (2, 3; 0: run-time loop) and whether the pitch the op's lanes
// are laid over (forward: Po, backward: P) is a power of two.  tn_c8_pool_plan reports it.
struct c8p_plan {
    int pw, sh, lg;
};

static c8p_plan c8p_choose(int op, int P, int p, int Po) {
    c8p_plan pl;
    pl.pw = p == 2 || p == 3 ? p : 0;
    pl.lg = c8p_lg(op == 0 ? Po : P);
    pl.sh = pl.lg >= 0;
    return pl;
}

extern "C" {

int tn_c8_pool_supported(int N, int C, int S, int P, int p, int So, int Po) {
    if (p < 2 || p > 64 || So < 1 || S < 1) return 0;
    if (So != S / p && So != (S + p - 1) / p) return 0;
    return c8p_cells(N, C, S, P) > 0 && c8p_cells(N, C, So, Po) > 0;
}

#define C8P_ARGS_FMT "(N %d C %d, maps of %d pixels at pitch %d, window %d, output %d pixels at pitch %d)"

#define C8P_DISPATCH(GO)                                       \
    do {                                                       \
        if (pl.pw == 2) { if (pl.sh) GO(2, true); else GO(2, false); }      \
        else if (pl.pw == 3) { if (pl.sh) GO(3, true); else GO(3, false); } \
        else { if (pl.sh) GO(0, true); else GO(0, false); }                 \
    } while (0)

int tn_c8_pool_fwd(tn_ctx* ctx, const void* x, void* y, int N, int C, int S, int P, int p, int So, int Po) {
    TN_REQUIRE(x && y && tn_c8_pool_supported(N, C, S, P, p, So, Po), "tn_c8_pool_fwd: bad arguments " C8P_ARGS_FMT, N, C, S,
               P, p, So, Po);
    const long long cells = c8p_cells(N, C, So, Po);
    const c8p_plan pl = c8p_choose(0, P, p, Po);
    const unsigned grid = (unsigned)cdiv(cells, 256);
#define C8P_FWD_GO(PW, SH)                                                                                             \
    c8_pool_fwd_kernel<PW, SH><<<grid, 256, 0, ctx->stream>>>(static_cast<const uint4*>(x), static_cast<uint4*>(y),       \
                                                             (unsigned)cells, C, (unsigned)((C + 7) / 8), (unsigned)S,  \
                                                             (unsigned)P, (unsigned)p, (unsigned)So, (unsigned)Po, pl.lg)
    C8P_DISPATCH(C8P_FWD_GO);
#undef C8P_FWD_GO
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_c8_pool_bwd(tn_ctx* ctx, const void* x, const void* y, const void* gout, void* gin, int N, int C, int S, int P, int p,
                   int So, int Po) {
    TN_REQUIRE(x && y && gout && gin && tn_c8_pool_supported(N, C, S, P, p, So, Po),
               "tn_c8_pool_bwd: bad arguments " C8P_ARGS_FMT, N, C, S, P, p, So, Po);
    const long long cells = c8p_cells(N, C, S, P);
    const c8p_plan pl = c8p_choose(1, P, p, Po);
    const unsigned grid = (unsigned)cdiv(cells, 256);
#define C8P_BWD_GO(PW, SH)                                                                                              \
    c8_pool_bwd_kernel<PW, SH><<<grid, 256, 0, ctx->stream>>>(                                                            \
        static_cast<const uint4*>(x), static_cast<const uint4*>(y), static_cast<const uint4*>(gout), static_cast<uint4*>(gin), \
        (unsigned)cells, C, (unsigned)((C + 7) / 8), (unsigned)S, (unsigned)P, pl.lg, (unsigned)p, (unsigned)So, (unsigned)Po)
    C8P_DISPATCH(C8P_BWD_GO);
#undef C8P_BWD_GO
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// op 0: tn_c8_pool_fwd -> c8_pool_fwd_kernel<PW, SH>, op 1: tn_c8_pool_bwd -> c8_pool_bwd_kernel<PW, SH>; the plan is
// PW, SH, blocks of 256 lanes.  No device, no context.
int tn_c8_pool_plan(int op, int N, int C, int S, int P, int p, int So, int Po, int* out, int nout) {
    if ((op != 0 && op != 1) || !tn_c8_pool_supported(N, C, S, P, p, So, Po) || (nout > 0 && !out)) return TN_E_ARG;
    const c8p_plan pl = c8p_choose(op, P, p, Po);
    const long long cells = op == 0 ? c8p_cells(N, C, So, Po) : c8p_cells(N, C, S, P);
    const int v[3] = {pl.pw, pl.sh, cdiv(cells, 256)};
    for (int k = 0; k < 3 && k < nout; ++k) out[k] = v[k];
    return 3;
}

}  // extern "C"
