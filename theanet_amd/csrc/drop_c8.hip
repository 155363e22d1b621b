// DTYPE 'float16' / 'bfloat16': DropOutLayer (theanet/layer/dropout.py:15-31) between the blocks of the 16-bit-resident
// conv stack.  The reference: mask ~ Bernoulli(1 - pdrop), y = x * mask with NO 1/(1-p) rescale (:21-26); the test
// version is y = (1 - pdrop) * x (:28-31).  On c8 tensors ([N][ceil(C/8)][P][P][8] 16-bit values, S x S maps at pitch P):
//   train forward   y = x (.) m      a stored value or +0: exact, no rounding; pad cells and channels >= C written as 0
//   train backward  gin = gout (.) m exact as well.  The activation derivative of the block below is NOT applied here: the
//                   layer looks through (DropOutLayer.act_info), so whoever produced gout has rounded
//                   grad_scale * g * act' once already, and an all-ones mask leaves the net without the layer bit for bit
//   test forward    y = R((1 - pdrop) * x), the product in fp32, one rounding (nearest even) to the element type
// The mask is the fp32 net's mask: element (n, c, h, w) of the LOGICAL (N, C, S, S) tensor takes the number
// tn_dropout_mask gives element e = elem0 + ((n C + c) S + h) S + w -- word e & 3 of philox4x32(e >> 2, step,
// TN_STREAM_DROPOUT, seed), kept if tn_u01(word) >= pdrop (pool.hip dropout_mask_kernel) -- whatever the element type,
// the pitch or the sharding of the batch.  It is kept packed for the backward pass: one byte per 16-byte cell, bit k =
// channel 8 * octet + k kept; 1/16 of the tensor's bytes.
//
// A cell holds 8 channels of one pixel and their element indices lie S*S apart, so a lane on its own needs 8 Philox
// calls for its 8 elements.  The forward therefore lets the 4 lanes that own 4 horizontally adjacent pixels of an octet
// share: each makes the calls of 2 of the 8 channels (a call covers the 4 pixels when a Philox quad lies inside a map
// row: S % 4 == 0 and elem0 % 4 == 0), turns them into 8 keep bits at once, and two cross-lane ORs inside the lane quad
// leave all 32 bits with all four lanes -- one call per 4 elements, the fp32 kernel's rate, while every lane still loads
// and stores its own 16-byte cell (lane-contiguous, 1 KiB per wave and instruction).  Other S / elem0 take the same
// kernel without the sharing: 8 calls per cell, the same numbers.  The loads are issued before the calls and consumed
// after them, so the ALU work runs under the memory latency.  Plain vector loads and stores, no atomics: one result
// whatever the schedule.
//
// The train ops only select 16-bit patterns, so they are element-type blind and live in the fp16 unit alone; the test
// version converts, and drop_c8_bf16.hip instantiates it for bf16 (c8_elem.h).
#include "c8_elem.h"

#ifndef C8_BF16_TU
// the 16-bit lanes of a cell that byte m keeps, as four 32-bit select masks
__device__ __forceinline__ uint4 c8_drop_apply(uint4 v, uint32_t m) {
    const uint32_t lo = 0x0000ffffu, hi = 0xffff0000u;
    v.x &= ((m & 1u) ? lo : 0u) | ((m & 2u) ? hi : 0u);
    v.y &= ((m & 4u) ? lo : 0u) | ((m & 8u) ? hi : 0u);
    v.z &= ((m & 16u) ? lo : 0u) | ((m & 32u) ? hi : 0u);
    v.w &= ((m & 64u) ? lo : 0u) | ((m & 128u) ? hi : 0u);
    return v;
}

// QUAD: the 4 lanes of an aligned lane quad own pixels w0 .. w0+3 of one row (P % 4 == 0) and share their Philox calls
// (S % 4 == 0 and elem0 % 4 == 0).  Every lane of a wave reaches the cross-lane ORs: no early return.
template <bool QUAD>
__global__ __launch_bounds__(256) void c8_drop_fwd_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                         uint8_t* __restrict__ mask8, unsigned cells, int C, unsigned C8,
                                                         unsigned S, unsigned P, float pdrop, uint32_t k0, uint32_t k1,
                                                         uint32_t step, const uint32_t* __restrict__ d_step,
                                                         unsigned long long elem0, int draw) {
    const unsigned t = threadIdx.x, cell = blockIdx.x * 256u + t;
    const bool live = cell < cells;
    const unsigned row = cell / P, w = cell - row * P, pair = row / P, h = row - pair * P;
    const unsigned n = pair / C8, o = pair - n * C8;
    const bool inside = live && h < S && w < S;
    const int nv = C - 8 * (int)o;                               // channels of this octet inside C
    const uint32_t valid = nv >= 8 ? 0xffu : ((1u << nv) - 1u);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (inside) v = x[cell];
    uint32_t m = 0u;
    if (draw) {
        const uint32_t st = step + (d_step ? *d_step : 0u);
        // element index of (n, channel 8 o, h, w); channel k of the octet: + k S S
        const unsigned long long e0 = elem0 + (((unsigned long long)n * (unsigned)C + 8u * o) * S + h) * S + w;
        const unsigned long long SS = (unsigned long long)S * S;
        if (QUAD) {
            const unsigned l = t & 3u;
            uint32_t bits = 0u;                                  // bit 8 p + k: pixel w0 + p, channel k
            if (inside) {
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const unsigned k = 2u * l + jj;
                    if ((int)k < nv) {
                        const unsigned long long cq = (e0 - l + k * SS) >> 2;
                        const u32x4 r = philox4x32((uint32_t)cq, (uint32_t)(cq >> 32), st, TN_STREAM_DROPOUT, k0, k1);
                        const uint32_t b = (tn_u01(r.x) >= pdrop ? 1u : 0u) | (tn_u01(r.y) >= pdrop ? 0x100u : 0u) |
                                           (tn_u01(r.z) >= pdrop ? 0x10000u : 0u) | (tn_u01(r.w) >= pdrop ? 0x1000000u : 0u);
                        bits |= b << k;
                    }
                }
            }
            bits |= __shfl_xor(bits, 1);
            bits |= __shfl_xor(bits, 2);
            m = (bits >> (8u * l)) & 0xffu;
        } else if (inside) {
#pragma unroll 2
            for (int k = 0; k < 8; ++k) {
                if (k < nv) {
                    const unsigned long long e = e0 + k * SS, cq = e >> 2;
                    const u32x4 r = philox4x32((uint32_t)cq, (uint32_t)(cq >> 32), st, TN_STREAM_DROPOUT, k0, k1);
                    const unsigned i = (unsigned)e & 3u;
                    const uint32_t wd = i == 0 ? r.x : i == 1 ? r.y : i == 2 ? r.z : r.w;
                    m |= (tn_u01(wd) >= pdrop ? 1u : 0u) << k;
                }
            }
        }
        if (live) mask8[cell] = (uint8_t)m;
    } else if (inside) {
        m = mask8[cell] & valid;
    }
    if (live) y[cell] = c8_drop_apply(v, m);
}

__global__ __launch_bounds__(256) void c8_drop_bwd_kernel(const uint4* __restrict__ gout, const uint8_t* __restrict__ mask8,
                                                         uint4* __restrict__ gin, unsigned cells) {
    const unsigned cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    const uint4 v = gout[cell];
    const uint32_t m = mask8[cell];
    gin[cell] = c8_drop_apply(v, m);
}
#endif  // C8_BF16_TU

template <typename E>
__global__ __launch_bounds__(256) void c8_scale_kernel(const typename E::T* __restrict__ x, typename E::T* __restrict__ y,
                                                      unsigned cells, float scale) {
    typedef typename E::v8 v8;
    const unsigned cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    const v8 a = reinterpret_cast<const v8*>(x)[cell];
    v8 o8;
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = (typename E::T)__fmul_rn((float)a[e], scale);
    reinterpret_cast<v8*>(y)[cell] = o8;
}

// cells of a c8 tensor of N x C maps of S pixels a side at pitch P, or -1: bad geometry / 2^32 cells or more
static long long c8_drop_cells(int N, int C, int S, int P) {
    if (N <= 0 || C <= 0 || S <= 0 || P < S || (P != S && (P & (P - 1)))) return -1;
    const long long cells = (long long)N * ((C + 7) / 8) * P * P;
    return cells < (1ll << 32) - 256 ? cells : -1;
}

extern "C" {

#ifndef C8_BF16_TU
int c8b_tn_c8_scale(tn_ctx* ctx, const void* x, void* y, int N, int C, int S, int P, float scale);

// y = x (.) m, m drawn (draw != 0: the numbers of tn_dropout_mask(seed, step, d_step, elem0) on the logical (N, C, S, S)
// tensor) and written packed to mask8 (a byte per cell), or read from mask8 (draw == 0).  y may be x.
int tn_c8_dropout_fwd(tn_ctx* ctx, const void* x, void* y, uint8_t* mask8, int N, int C, int S, int P, float pdrop,
                      uint64_t seed, uint32_t step, const uint32_t* d_step, uint64_t elem0, int draw) {
    const long long cells = c8_drop_cells(N, C, S, P);
    TN_REQUIRE(x && y && mask8 && cells > 0 && pdrop >= 0.f && pdrop <= 1.f,
               "tn_c8_dropout_fwd: bad arguments (N %d C %d, maps of %d pixels at pitch %d, pdrop %g)", N, C, S, P, pdrop);
    const unsigned grid = (unsigned)cdiv(cells, 256);
    const bool quad = (S & 3) == 0 && (P & 3) == 0 && (elem0 & 3) == 0;
#define C8_DROP_GO(Q)                                                                                              \
    c8_drop_fwd_kernel<Q><<<grid, 256, 0, ctx->stream>>>(static_cast<const uint4*>(x), static_cast<uint4*>(y), mask8, \
                                                        (unsigned)cells, C, (unsigned)((C + 7) / 8), (unsigned)S,     \
                                                        (unsigned)P, pdrop, (uint32_t)seed, (uint32_t)(seed >> 32),   \
                                                        step, d_step, (unsigned long long)elem0, draw)
    if (quad) C8_DROP_GO(true); else C8_DROP_GO(false);
#undef C8_DROP_GO
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// gin = gout (.) m, m the packed mask of the forward.  gin may be gout.
int tn_c8_dropout_bwd(tn_ctx* ctx, const void* gout, const uint8_t* mask8, void* gin, int N, int C, int S, int P) {
    const long long cells = c8_drop_cells(N, C, S, P);
    TN_REQUIRE(gout && gin && mask8 && cells > 0, "tn_c8_dropout_bwd: bad arguments (N %d C %d, maps of %d pixels at pitch %d)",
               N, C, S, P);
    c8_drop_bwd_kernel<<<(unsigned)cdiv(cells, 256), 256, 0, ctx->stream>>>(static_cast<const uint4*>(gout), mask8,
                                                                           static_cast<uint4*>(gin), (unsigned)cells);
    TN_LAUNCH_CHECK();
    return TN_OK;
}
#endif  // C8_BF16_TU

// y = R(scale * x) on the context's 16-bit element type (the test version: scale = 1 - pdrop).  y may be x.
int C8_API(tn_c8_scale)(tn_ctx* ctx, const void* x, void* y, int N, int C, int S, int P, float scale) {
    C8_TO_BF16(tn_c8_scale, ctx, x, y, N, C, S, P, scale);
    const long long cells = c8_drop_cells(N, C, S, P);
    TN_REQUIRE(x && y && cells > 0 && scale == scale, "tn_c8_scale: bad arguments (N %d C %d, maps of %d pixels at pitch %d)",
               N, C, S, P);
    c8_scale_kernel<C8E><<<(unsigned)cdiv(cells, 256), 256, 0, ctx->stream>>>(
        static_cast<const typename C8E::T*>(x), static_cast<typename C8E::T*>(y), (unsigned)cells, scale);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
