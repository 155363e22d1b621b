// tn_wtcost_net: the cost of a step of a net with weight costs -- the minibatch cost (outlayers.py:50-51) plus
// L1*sum|p| + L2*sum p^2 of every regularised tensor (layer.py:109-117, neuralnet.py:208-210) -- as ONE launch.
//
// Grid: one block per (table row, TN_WTCOST_CHUNK-element chunk), whatever the device: the partition, and with it the
// order of every addition, is a function of the table alone.  A block sums its chunk (thread t takes elements
// 4t .. 4t+3 of every 1024, in ascending order, into one accumulator per term; __shfl_xor inside a wave; the four wave
// sums as (w0 + w1) + (w2 + w3)), stores L1*a + L2*s into partial[block] and draws a ticket.  The block that draws the
// last ticket adds the partials in index order, sums the row losses exactly as the cost rider of the update launch
// does (update_body.h), stores *d_cost and puts the ticket back to zero for the next launch.
//
// Visibility across the eight XCDs (private L2s): a partial is stored write-through (agent-scope relaxed atomic store: a
// vector store with sc1), the storing lane fences (__threadfence) and then adds to the ticket (agent-scope atomic);
// the last block fences again and reads the partials with agent-scope relaxed atomic loads (vector loads that bypass
// this CU's L1).  No floating-point atomics anywhere.
#include "common.h"

#define WC_ROWS 32
struct WcBatch {
    const float* p[WC_ROWS];
    uint32_t first[WC_ROWS + 1];        // first block of row r; first[nrows] = number of chunk blocks
    uint64_t n[WC_ROWS];
    float L1[WC_ROWS], L2[WC_ROWS];
    int nrows;
};

__device__ __forceinline__ float wc_block_sum(float s, float* red4) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __syncthreads();                    // red4 may still be read from the previous use
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

__global__ __launch_bounds__(256) void wtcost_net_kernel(WcBatch b, float* partial, uint32_t* ticket,
                                                         const float* __restrict__ rowloss, int nrow, float cost_scale,
                                                         float* d_cost, int accumulate) {
    __shared__ float red4[4];
    __shared__ float stage[1024];
    __shared__ uint32_t drawn;
    const uint32_t bid = blockIdx.x, nchunk = b.first[b.nrows];
    if (bid < nchunk) {
        int r = 0;
        while (r + 1 < b.nrows && bid >= b.first[r + 1]) ++r;
        const float* __restrict__ p = b.p[r];
        const uint64_t n = b.n[r];
        const uint64_t c0 = (uint64_t)(bid - b.first[r]) * TN_WTCOST_CHUNK;
        const uint64_t ce = c0 + TN_WTCOST_CHUNK < n ? c0 + TN_WTCOST_CHUNK : n;
        const bool vec = ((uintptr_t)p & 15) == 0;      // (chunks start at multiples of 4 elements)
        float a = 0.f, s = 0.f;
#pragma unroll 4
        for (uint64_t i = c0 + 4 * threadIdx.x; i < ce; i += 1024) {
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            if (vec && i + 4 <= ce) {
                const float4 q = *reinterpret_cast<const float4*>(p + i);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i + j < ce) x[j] = p[i + j];   // (past the end: 0 adds nothing to either sum)
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a += fabsf(x[j]);
                s = fmaf(x[j], x[j], s);
            }
        }
        a = wc_block_sum(a, red4);
        s = wc_block_sum(s, red4);
        if (threadIdx.x == 0)
            __hip_atomic_store(partial + bid, fmaf(b.L2[r], s, b.L1[r] * a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) {
        __threadfence();                // the partial is out before the ticket says so
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
    }
    __syncthreads();
    if (drawn != gridDim.x - 1) return;
    // ---- the last block: everything the others stored is visible at agent scope
    float w = 0.f;
    for (uint32_t t0 = 0; t0 < nchunk; t0 += 1024) {
        const uint32_t cnt = nchunk - t0 < 1024u ? nchunk - t0 : 1024u;
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < cnt; k += 256)
            stage[k] = __hip_atomic_load(partial + t0 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t k = 0; k < cnt; ++k) w += stage[k];       // index order
    }
    float c = 0.f;
    if (rowloss) {                      // the rider's order (sgd_update_multi_block, by == nseg)
        float s = 0.f;
        for (int i = threadIdx.x; i < nrow; i += 256) s += rowloss[i];
        c = __fmul_rn(cost_scale, wc_block_sum(s, red4));
    }
    if (threadIdx.x == 0) {
        float out = w;
        if (rowloss) out = nchunk ? __fadd_rn(c, w) : c;
        if (accumulate) out = __fadd_rn(d_cost[0], out);
        d_cost[0] = out;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch
    }
}

// the current stream's partial array (>= need floats) and ticket
static int wc_scratch(tn_ctx* ctx, size_t need, float** partial, uint32_t** ticket) {
    const int k = ctx->stream == ctx->streams[1] ? 1 : 0;
    if (!ctx->wc_part[k] || ctx->wc_cap[k] < need) {
        size_t cap = ctx->wc_cap[k] ? ctx->wc_cap[k] : 4096;
        while (cap < need) cap *= 2;
        if (ctx->wc_part[k]) {          // launches that use the old array may still be in flight on this stream
            TN_HIP(hipStreamSynchronize(ctx->stream));
            TN_HIP(hipFree(ctx->wc_part[k] - 4));
            ctx->wc_part[k] = nullptr;
            ctx->wc_cap[k] = 0;
        }
        float* base = nullptr;
        hipError_t e = hipMalloc((void**)&base, (cap + 4) * sizeof(float));
        if (e != hipSuccess) return tn_fail(ctx, TN_E_NOMEM, "tn_wtcost_net: hipMalloc -> %s", hipGetErrorString(e));
        // the ticket block, zeroed on the stream the launches follow on; every launch leaves it at zero again
        e = hipMemsetAsync(base, 0, 16, ctx->stream);
        if (e != hipSuccess) {
            hipFree(base);
            return tn_fail(ctx, TN_E_HIP, "tn_wtcost_net: hipMemsetAsync -> %s", hipGetErrorString(e));
        }
        ctx->wc_part[k] = base + 4;
        ctx->wc_cap[k] = cap;
    }
    *partial = ctx->wc_part[k];
    *ticket = reinterpret_cast<uint32_t*>(ctx->wc_part[k] - 4);
    return TN_OK;
}

extern "C" int tn_wtcost_net(tn_ctx* ctx, const tn_wc_seg* h_tab, int ntab, const float* rowloss, int nrow, float cost_scale,
                             float* d_cost, int accumulate) {
    TN_REQUIRE(ntab >= 0 && (ntab == 0 || h_tab) && d_cost, "tn_wtcost_net: bad arguments");
    TN_REQUIRE(!rowloss || nrow > 0, "tn_wtcost_net: bad cost arguments");
    int i = 0;
    bool first = true;
    do {
        WcBatch b{};
        uint64_t blocks = 0;
        for (; i < ntab && b.nrows < WC_ROWS; ++i) {
            const tn_wc_seg& t = h_tab[i];
            if (!t.n || (t.L1 == 0.f && t.L2 == 0.f)) continue;
            TN_REQUIRE(t.p != nullptr, "tn_wtcost_net: row %d has no tensor", i);
            const int r = b.nrows++;
            b.p[r] = t.p; b.n[r] = t.n; b.L1[r] = t.L1; b.L2[r] = t.L2;
            b.first[r] = (uint32_t)blocks;
            blocks += (t.n + TN_WTCOST_CHUNK - 1) / TN_WTCOST_CHUNK;
            TN_REQUIRE(blocks < (1ull << 31), "tn_wtcost_net: table too large");
        }
        b.first[b.nrows] = (uint32_t)blocks;
        float* partial;
        uint32_t* ticket;
        int rc = wc_scratch(ctx, (size_t)blocks, &partial, &ticket);
        if (rc) return rc;
        wtcost_net_kernel<<<blocks ? (unsigned)blocks : 1u, 256, 0, ctx->stream>>>(
            b, partial, ticket, first ? rowloss : nullptr, nrow, cost_scale, d_cost, first ? accumulate : 1);
        TN_LAUNCH_CHECK();
        first = false;
    } while (i < ntab);
    return TN_OK;
}
