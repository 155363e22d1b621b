// tn_avg_net: the exponential moving average of a net's weights (training param WT_AVG: d, Polyak averaging), every
// averaged tensor in ONE launch.
//
// The contract (include/theanet_hip.h states it the same way): every tensor of a layer with updates has an fp32 average
// a of its own shape, a_0 = the weights the net starts from.  p_t (t >= 1) = the weights the forward pass of step t+1
// reads, after the momentum step and the max-norm projection; every p_t enters the average exactly once, in order:
//     c   = fl(1 - d)                              rounded once, on the host
//     a_t = fma(c, fl(p_t - a_{t-1}), a_{t-1})     __fsub_rn / __fmaf_rn, the way common.h spells tn_vel
// p is never written.  mode 1 exchanges p and a bit for bit instead (an evaluation at the averaged weights brackets its
// work with two of them).  No atomics, every element is touched by one thread: the same bits every run.
//
// Grid: tn_sgd_update_net's shape -- block row = segment (rows beyond the grid's y limit stride over it), grid-stride
// along the segment.  A segment may start at any 4-byte boundary: where p and a sit at the same offset from a 16-byte
// boundary the elements up to that boundary and the last n % 4 behind the 16-byte body go one by one, the body as
// 16-byte accesses; where they differ the whole segment goes one by one.  12 bytes of traffic per weight (mode 1: 16),
// no LDS, no matrix work.
#include "common.h"

static_assert(sizeof(tn_avg_seg) == 32, "tn_avg_seg is 32 bytes");

template <int MODE>
__device__ __forceinline__ void avg_one(float* p, float* a, float c) {
    if (MODE == 0) {
        const float av = *a;
        *a = __fmaf_rn(c, __fsub_rn(*p, av), av);
    } else {                                // a bit copy both ways (no arithmetic: a NaN keeps its payload)
        uint32_t* pu = reinterpret_cast<uint32_t*>(p);
        uint32_t* au = reinterpret_cast<uint32_t*>(a);
        const uint32_t x = *pu, y = *au;
        *pu = y;
        *au = x;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void avg_net_kernel(const tn_avg_seg* __restrict__ segs, int nseg, float c) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (int s = blockIdx.y; s < nseg; s += gridDim.y) {
        float* const p = segs[s].p;
        float* const a = segs[s].a;
        const size_t n = segs[s].n;
        // [0, head) one by one, [head, head + 4 nvec) as 16-byte accesses, [head + 4 nvec, n) one by one
        size_t head = n, nvec = 0;
        if ((((uintptr_t)p ^ (uintptr_t)a) & 15) == 0) {
            head = ((16 - ((uintptr_t)a & 15)) & 15) >> 2;
            if (head > n) head = n;
            nvec = (n - head) >> 2;
        }
        const size_t tail0 = head + 4 * nvec, nscal = head + (n - tail0);
        for (size_t i = tid; i < nscal; i += stride) {
            const size_t e = i < head ? i : tail0 + (i - head);
            avg_one<MODE>(p + e, a + e, c);
        }
        if (MODE == 0) {
            const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + head);
            float4* __restrict__ a4 = reinterpret_cast<float4*>(a + head);
            for (size_t i = tid; i < nvec; i += stride) {
                const float4 pv = p4[i];
                float4 av = a4[i];
                av.x = __fmaf_rn(c, __fsub_rn(pv.x, av.x), av.x);
                av.y = __fmaf_rn(c, __fsub_rn(pv.y, av.y), av.y);
                av.z = __fmaf_rn(c, __fsub_rn(pv.z, av.z), av.z);
                av.w = __fmaf_rn(c, __fsub_rn(pv.w, av.w), av.w);
                a4[i] = av;
            }
        } else {
            uint4* __restrict__ p4 = reinterpret_cast<uint4*>(p + head);
            uint4* __restrict__ a4 = reinterpret_cast<uint4*>(a + head);
            for (size_t i = tid; i < nvec; i += stride) {
                const uint4 x = p4[i], y = a4[i];
                p4[i] = y;
                a4[i] = x;
            }
        }
    }
}

extern "C" int tn_avg_net(tn_ctx* ctx, const tn_avg_seg* d_segs, int nseg, size_t max_n, float c, int mode) {
    TN_REQUIRE(mode == TN_AVG_UPDATE || mode == TN_AVG_EXCHANGE, "tn_avg_net: mode %d", mode);
    TN_REQUIRE(c >= 0.f && c <= 1.f, "tn_avg_net: c = %g is not in [0, 1]", (double)c);        // (a NaN is refused too)
    TN_REQUIRE(nseg >= 0 && (nseg == 0 || d_segs != nullptr), "tn_avg_net: no segment table");
    if (nseg == 0) return TN_OK;
    TN_REQUIRE(max_n > 0, "tn_avg_net: empty segments (max_n == 0)");
    int bx = cdiv((long long)max_n, 1024);
    if (bx > 2048) bx = 2048;
    if (bx < 1) bx = 1;
    const dim3 grid(bx, nseg < 65535 ? nseg : 65535);
    if (mode == TN_AVG_UPDATE)
        avg_net_kernel<0><<<grid, 256, 0, ctx->stream>>>(d_segs, nseg, c);
    else
        avg_net_kernel<1><<<grid, 256, 0, ctx->stream>>>(d_segs, nseg, c);
    TN_LAUNCH_CHECK();
    return TN_OK;
}
