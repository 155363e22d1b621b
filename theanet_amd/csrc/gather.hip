// tn_gather_batch: the minibatch of a SHUFFLED epoch, staged in one launch (include/theanet_hip.h).
//
// The row order of an epoch lives on the device (theanet_amd/trainfn.py set_order); a step copies rows
// order[row0 .. row0 + nrows) of the images, their labels and (aux nets) their aux rows into per-net staging buffers
// that everything downstream reads at a constant row 0.  Pure data movement: two passes over the minibatch's bytes.
//
// Work is cut into WAVE ITEMS, flattened over all three copies, so that a 512-row shard of 3 KB rows is ~2000
// waves and not 512 blocks looping over dwords:
//   * a copy whose rows hold at least 64 units (a unit = 16 bytes where the row size and both bases allow it, else a
//     dword): one item = 64 consecutive units of ONE row = one wave-instruction's load and store.  The item number is
//     wave-uniform, so the row number and the order entry are too: the entry is read once per wave, through the
//     scalar cache, not per lane per chunk.
//   * a copy of shorter rows (the labels: one dword; aux rows: a few floats): one item = floor(64 / units) whole rows,
//     every lane reads the entry of its own row once.
// Rows that are not a multiple of 16 bytes put every second..fourth row off a 16-byte boundary: the whole copy takes
// the dword form (there is no 16-byte body + dword tail to split: a row is either all chunks or all dwords).
#include "common.h"

namespace {

struct gather_seg {
    const char* src;
    char* dst;
    uint32_t units;      // per row: 16-byte chunks (vec) or dwords
    uint32_t per;        // units >= 64: items per row; else rows per item
    uint32_t items;      // wave items of this copy
    uint32_t vec;
};

struct gather_args {
    gather_seg seg[3];   // images, labels, aux rows (items 0 where absent)
    uint32_t nrows, total;
};

template <typename T>
__device__ __forceinline__ void gather_units(const gather_seg& s, const int32_t* __restrict__ order, uint32_t nrows,
                                            uint32_t item, uint32_t lane) {
    const T* __restrict__ src = reinterpret_cast<const T*>(s.src);
    T* __restrict__ dst = reinterpret_cast<T*>(s.dst);
    if (s.units >= 64) {
        const uint32_t r = __builtin_amdgcn_readfirstlane(item / s.per);     // wave-uniform: ONE scalar load of the entry
        const uint32_t c = (item - r * s.per) * 64 + lane;
        const size_t from = (size_t)__builtin_amdgcn_readfirstlane(order[r]);
        if (c < s.units) dst[(size_t)r * s.units + c] = src[from * s.units + c];
    } else {
        const uint32_t sub = lane / s.units;
        const uint32_t r = item * s.per + sub;
        if (sub < s.per && r < nrows) {
            const uint32_t c = lane - sub * s.units;
            dst[(size_t)r * s.units + c] = src[(size_t)order[r] * s.units + c];
        }
    }
}

__device__ __forceinline__ void gather_item(const gather_seg& s, const int32_t* __restrict__ order, uint32_t nrows,
                                            uint32_t item, uint32_t lane) {
    if (s.vec)
        gather_units<uint4>(s, order, nrows, item, lane);
    else
        gather_units<uint32_t>(s, order, nrows, item, lane);
}

__global__ void __launch_bounds__(256) gather_batch_kernel(const gather_args a, const int32_t* __restrict__ order) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    for (uint32_t w = wave0; w < a.total; w += gridDim.x * 4) {
        uint32_t item = w;
        if (item < a.seg[0].items) {
            gather_item(a.seg[0], order, a.nrows, item, lane);
        } else if ((item -= a.seg[0].items) < a.seg[1].items) {
            gather_item(a.seg[1], order, a.nrows, item, lane);
        } else {
            gather_item(a.seg[2], order, a.nrows, item - a.seg[1].items, lane);      // (w < total)
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One copy as wave items; false when it would not fit the 32-bit item count.
bool make_seg(gather_seg& s, const void* src, void* dst, size_t row_bytes, int nrows, uint64_t& total) {
    s = gather_seg{};
    if (!src || !row_bytes) return true;
    const bool vec = row_bytes % 16 == 0 && aligned16(src) && aligned16(dst);
    const size_t units = row_bytes / (vec ? 16 : 4);
    if (units > 0xffffffffull) return false;
    uint64_t items;
    if (units >= 64) {
        s.per = (uint32_t)((units + 63) / 64);
        items = (uint64_t)nrows * s.per;
    } else {
        s.per = (uint32_t)(64 / units);
        items = ((uint64_t)nrows + s.per - 1) / s.per;
    }
    total += items;
    if (total >= (1ull << 31)) return false;
    s.src = static_cast<const char*>(src);
    s.dst = static_cast<char*>(dst);
    s.units = (uint32_t)units;
    s.items = (uint32_t)items;
    s.vec = vec;
    return true;
}

}  // namespace

extern "C" int tn_gather_batch(tn_ctx* ctx, const int32_t* order, int64_t row0, int nrows, const void* x, void* x_out,
                               size_t x_row_bytes, const int32_t* y, int32_t* y_out, const void* aux, void* aux_out,
                               size_t aux_row_bytes) {
    TN_REQUIRE(order && x && x_out, "tn_gather_batch: order, x and x_out must not be NULL");
    TN_REQUIRE(nrows >= 0 && row0 >= 0, "tn_gather_batch: nrows %d, row0 %lld", nrows, (long long)row0);
    TN_REQUIRE(x_row_bytes % 4 == 0 && aux_row_bytes % 4 == 0,
               "tn_gather_batch: row sizes (%zu, %zu bytes) must be multiples of 4", x_row_bytes, aux_row_bytes);
    TN_REQUIRE((y == nullptr) == (y_out == nullptr) && (aux == nullptr) == (aux_out == nullptr),
               "tn_gather_batch: y / y_out and aux / aux_out are NULL in pairs");
    if (!nrows) return TN_OK;
    gather_args a{};
    uint64_t total = 0;
    const bool fits = make_seg(a.seg[0], x, x_out, x_row_bytes, nrows, total) &&
                      make_seg(a.seg[1], y, y_out, 4, nrows, total) &&
                      make_seg(a.seg[2], aux, aux_out, aux_row_bytes, nrows, total);
    TN_REQUIRE(fits, "tn_gather_batch: %d rows of %zu bytes are more than 2^31 wave items", nrows, x_row_bytes);
    if (!total) return TN_OK;
    a.nrows = (uint32_t)nrows;
    a.total = (uint32_t)total;
    // four wave items per block; past 16384 blocks (eight full rounds of the device) the waves stride
    const uint32_t blocks = (uint32_t)((total + 3) / 4 < 16384 ? (total + 3) / 4 : 16384);
    gather_batch_kernel<<<blocks, 256, 0, ctx->stream>>>(a, order + row0);
    TN_LAUNCH_CHECK();
    return TN_OK;
}
