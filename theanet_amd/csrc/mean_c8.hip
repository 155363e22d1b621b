// DTYPE 'float16' / 'bfloat16': MeanLayer (theanet/layer/convpool.py:129-144, tt.mean(inpt, axis=(2,3)): global
// average pooling) on the 16-bit-resident c8 tensor that ends the conv stack.  The layer's output is the fp32 (N, C)
// input of the dense layers above, so the forward sums the STORED 16-bit values in fp32 and does not round its result;
// the backward writes the c8 gradient the block below consumes, R(grad_scale * dy / (H W) * act'(block output)), with
// the conv kernels' contract (act' from the block's stored output, the gradient scale carried, one rounding on store).
//
// Both ops stream the tensor once, 16-byte cells (the 8 channels of an octet at one pixel) per lane:
//   forward : a group of G lanes per (image, octet) pair (G: 8 .. 64, more for a few large maps), fp32 sums in
//             registers, a reduce-scatter then a butterfly (__shfl_xor) across the group's lanes of a wave, then LDS
//             across its waves (G > 64).  Small maps pack 256 / G pairs into a block (a 4x4 map: four pairs per wave).
//   backward: a lane per cell; the block's (image, octet) pairs take grad_scale * dy / (H W) from dy once, into LDS.
// No atomics: every sum has one order, so both are deterministic (the pipelined and sequential schedules agree bit for
// bit).  (DTYPE 'bfloat16': the same kernels on bf16 cells, element type E = C8B; mean_c8_bf16.hip, c8_elem.h)
#include "c8_elem.h"

// channel of the octet whose sum lane j of a group holds after the three reduce-scatter stages below
__device__ __forceinline__ int c8_mean_chan(int j) { return ((j & 1) << 2) | (j & 2) | ((j >> 2) & 1); }

template <typename E>
__global__ __launch_bounds__(256) void c8_mean_fwd_kernel(const typename E::T* __restrict__ x, float* __restrict__ y,
                                                          int pairs, int C, int C8, int HW, int lg) {
    typedef typename E::v8 v8;
    __shared__ float part[4][8];                     // G > 64: the group's per-wave sums
    const int t = threadIdx.x, G = 1 << lg, j = t & (G - 1);
    const int pair = blockIdx.x * (256 >> lg) + (t >> lg);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    if (pair < pairs) {
        const v8* src = reinterpret_cast<const v8*>(x) + (size_t)pair * HW;
#pragma unroll 4
        for (int p = j; p < HW; p += G) {
            const v8 v = src[p];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
        }
    }
    // Across the group's lanes (every lane of the wave takes part; pairs past the end hold zeros).  Reduce-scatter over
    // lane bits 0-2: at each stage a lane keeps half of its sums and hands the other half to its partner, 4 + 2 + 1
    // shuffles for the 8 channels (a butterfly of all 8 would take 24), lane j ending with channel c8_mean_chan(j);
    // then a butterfly of that one sum over lane bits 3 .. log2(G) - 1 within the wave.
#pragma unroll
    for (int k = 4, m = 1; k > 0; k >>= 1, m <<= 1) {
        const bool up = (t & m) != 0;
#pragma unroll
        for (int i = 0; i < k; ++i) {
            const float give = up ? acc[i] : acc[i + k], keep = up ? acc[i + k] : acc[i];
            acc[i] = keep + __shfl_xor(give, m);
        }
    }
    float sum = acc[0];
    for (int m = 8; m < min(G, 64); m <<= 1) sum += __shfl_xor(sum, m);
    if (G > 64) {
        const int wave = t >> 6;
        if ((t & 63) < 8) part[wave][c8_mean_chan(t & 63)] = sum;
        __syncthreads();
        if (j < 8) {
            const int w0 = wave, e = c8_mean_chan(j);
            sum = part[w0][e];
            for (int w = 1; w < (G >> 6); ++w) sum += part[w0 + w][e];
        }
    }
    const int e = c8_mean_chan(j);
    if (j >= 8 || pair >= pairs) return;
    const int n = pair / C8, c = 8 * (pair - n * C8) + e;
    if (c < C) y[(size_t)n * C + c] = sum / (float)HW;
}

template <typename E>
__global__ __launch_bounds__(256) void c8_mean_bwd_kernel(const float* __restrict__ dy, typename E::T* __restrict__ dx,
                                                          const typename E::T* __restrict__ bout, unsigned cells, int C,
                                                          unsigned C8, unsigned HW, float gs, int act, float prm) {
    typedef typename E::v8 v8;
    __shared__ __attribute__((aligned(16))) float s[256 * 8];      // grad_scale * dy / HW of the block's pairs
    const unsigned t = threadIdx.x, c0 = blockIdx.x * 256u, cell = c0 + t;
    const unsigned p0 = c0 / HW, np = (min(c0 + 255u, cells - 1u)) / HW - p0 + 1u;    // pairs the block touches, <= 256
    const float hw = (float)HW;
    for (unsigned i = t; i < 8u * np; i += 256u) {
        const unsigned pair = p0 + (i >> 3), n = pair / C8;
        const int c = 8 * (int)(pair - n * C8) + (int)(i & 7u);
        s[i] = c < C ? dy[(size_t)n * C + c] * gs / hw : 0.f;
    }
    __syncthreads();
    if (cell >= cells) return;
    const unsigned pair = cell / HW;
    const int nv = C - 8 * (int)(pair % C8);        // channels of this octet inside C
    const float4 a = *reinterpret_cast<const float4*>(s + 8 * (pair - p0));
    const float4 b = *reinterpret_cast<const float4*>(s + 8 * (pair - p0) + 4);
    float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (bout) {
        const v8 y8 = reinterpret_cast<const v8*>(bout)[cell];
        const float tie = prm > 0.f ? 1.f + prm : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float yv = (float)y8[e];
            v[e] *= act == TN_ACT_LEAKY ? (yv > 0.f ? 1.f : (yv < 0.f ? prm : tie)) : tn_act_grad_from_out(yv, act, prm);
        }
    }
    v8 o8;
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = (typename E::T)(e < nv ? v[e] : 0.f);
    reinterpret_cast<v8*>(dx)[cell] = o8;
}

extern "C" {

#ifndef C8_BF16_TU
// the bf16 entry points (mean_c8_bf16.hip)
int c8b_tn_c8_mean_fwd(tn_ctx* ctx, const void* x, float* y, int N, int C, int H, int W);
int c8b_tn_c8_mean_bwd(tn_ctx* ctx, const float* dy, void* dx, int N, int C, int H, int W, const void* b_out, int b_act,
                       float b_prm);
#endif

// y (N, C) fp32 row-major = the mean over H x W of the stored values of the c8 tensor x
int C8_API(tn_c8_mean_fwd)(tn_ctx* ctx, const void* x, float* y, int N, int C, int H, int W) {
    C8_TO_BF16(tn_c8_mean_fwd, ctx, x, y, N, C, H, W);
    TN_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0, "tn_c8_mean_fwd: bad arguments (N %d C %d H %d W %d)", N, C, H, W);
    const int C8 = (C + 7) / 8;
    TN_REQUIRE((long long)H * W <= INT_MAX && (long long)N * C8 <= INT_MAX, "tn_c8_mean_fwd: %d x %d x %d x %d: too large", N, C, H, W);
    const int HW = H * W, pairs = N * C8;
    // G = 2^lg lanes per pair: the largest power of two <= HW, from 8 (the reduce-scatter's three lane bits) to 64 (one
    // wave, several cells per lane); up to 256 (LDS across the waves) while that leaves fewer than 64 K lanes busy
    int lg = 3;
    while (lg < 6 && (2 << lg) <= HW) ++lg;
    while (lg < 8 && (2 << lg) <= HW && (long long)pairs << lg < 65536) ++lg;
    c8_mean_fwd_kernel<C8E><<<cdiv(pairs, 256 >> lg), 256, 0, ctx->stream>>>(
        static_cast<const typename C8E::T*>(x), y, pairs, C, C8, HW, lg);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// dx (c8, N x C x H x W) = R(grad_scale * dy[n, c] / (H W) * act'(b_out)); b_out = the stored output of the block below
// (NULL: linear), channels past C zero
int C8_API(tn_c8_mean_bwd)(tn_ctx* ctx, const float* dy, void* dx, int N, int C, int H, int W, const void* b_out, int b_act,
                           float b_prm) {
    C8_TO_BF16(tn_c8_mean_bwd, ctx, dy, dx, N, C, H, W, b_out, b_act, b_prm);
    TN_REQUIRE(dy && dx && N > 0 && C > 0 && H > 0 && W > 0, "tn_c8_mean_bwd: bad arguments (N %d C %d H %d W %d)", N, C, H, W);
    const int C8 = (C + 7) / 8;
    TN_REQUIRE((long long)H * W <= INT_MAX && (long long)N * C8 <= INT_MAX, "tn_c8_mean_bwd: %d x %d x %d x %d: too large", N, C, H, W);
    const long long cells = (long long)N * C8 * H * W;
    TN_REQUIRE(cells < (1ll << 32) - 256, "tn_c8_mean_bwd: %d x %d x %d x %d: too large (2^32 cells)", N, C, H, W);
    c8_mean_bwd_kernel<C8E><<<cdiv(cells, 256), 256, 0, ctx->stream>>>(
        dy, static_cast<typename C8E::T*>(dx), static_cast<const typename C8E::T*>(b_out), (unsigned)cells, C, C8, H * W,
        ctx->grad_scale, b_act, b_prm);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
