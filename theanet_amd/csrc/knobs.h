// The library's environment switches (TN_*), one row each: name, default, parse form, whether data-parallel ranks
// must agree on it, what it does.  A switch that fixes a slab count or a kernel form fixes the order in which partial
// sums are added, and replicas must stay bit-identical: tn_knobs (include/theanet_hip.h) exports the resolved values
// of those rows and NeuralNet checks them across ranks.  Debug rows (cycle stamps, ablations) are not agreed; nor is a
// switch whose effect the host sees in a capability query and puts into the ranks' agreement itself (C8_HEAD).
// Plain C++, included by both backends (common.h, theanet_cpu.cpp).
#pragma once
#include <cstdio>
#include <cstdlib>

#include "../../include/theanet_hip.h"

// parse forms: atoi (the default when unset); atoi when positive, else the default; 0 iff the first character is '0';
// 1 iff set at all (even to "0")
enum tn_knob_form { TN_KF_ATOI, TN_KF_POS, TN_KF_NOT0, TN_KF_SET };

#define TN_KNOBS(X)                                                                                                   \
    /* conv_c8.hip: the fp16 / bf16 conv stack */                                                                     \
    X(C8_WTR, 1, ATOI, 1, "0: the eight-wave weight gradient everywhere, not the sixteen-wave one (A/B)")             \
    X(C8_ROLL, 1, ATOI, 1, "0: the halo-tile weight gradient everywhere; 2: the ring also on 16-pixel rows (A/B)")    \
    X(C8_WSLAB_DIV, 2, POS, 1, "weight-gradient sample slabs for num_cus / n CUs (1: every CU)")                      \
    X(C8_EXP, 0, ATOI, 1, "weight-gradient experiments: bit 0 no refills inside the loop, bit 1 no matrix steps")     \
    X(C8_DBG, 0, ATOI, 0, "cycle stamps of the conv and weight-gradient kernels (tools/dbg_c8.py)")                   \
    /* fc_c8.hip: the fp16 / bf16 dense layers */                                                                     \
    X(FC8_XCD, 1, ATOI, 1, "0: plain block decode of the forward (A/B)")                                              \
    X(FC8_FWD_HALF, 0, ATOI, 1, "1: one K slab for a forward whose tiles fill at least half the CUs")                 \
    X(FC8_FIN, 1, ATOI, 1, "0: the finishing launch also for one K slab (A/B)")                                       \
    X(FC8_WSLABS, 2, ATOI, 1, "weight-gradient sample slabs: n half blocks per CU")                                   \
    X(FC8_DZ16, 1, ATOI, 1, "0: rounding dz to 16 bits stays a launch of its own (A/B)")                              \
    /* head_c8.hip: an output head on the fp16 / bf16 conv stack */                                                   \
    X(C8_HEAD, 1, ATOI, 0, "0: no head kernels (tn_c8_head_supported answers 0): heads take the dense families")      \
    /* conv_tile.hip: the fp32 tile conv kernels */                                                                   \
    X(CONV_TILE, 1, NOT0, 1, "0: none of the tile kernels")                                                           \
    X(CONV_TILE_WGRAD, 1, NOT0, 1, "0: no tile weight gradient")                                                      \
    X(CONV_TILE_POOL, 1, NOT0, 1, "0: no conv + pool block on the tile kernels")                                      \
    X(CONV_TILE_SMALLC, 1, NOT0, 1, "0: no small-channel tile weight gradient")                                       \
    X(CT_DBG, 0, SET, 0, "cycle stamps of the tile conv kernel")                                                      \
    /* the fp32 conv blocks and the elastic layer */                                                                  \
    X(CONVPOOL_KS, 0, ATOI, 1, "n > 0: tn_convpool_fwd with n filter slices")                                         \
    X(CB_W44, 1, ATOI, 1, "0: the masked conv block weight gradient without the 4x4x1 broadcast MFMA (A/B)")          \
    X(CB_DBG, 0, ATOI, 0, "conv block backward ablations: bits skip its phases")                                      \
    X(CM_DBG, 0, ATOI, 0, "MFMA conv block backward ablations and stamps")                                            \
    X(ELASTIC_CONV, 1, ATOI, 1, "0: elastic resampling never fused into the first conv block")                        \
    /* gemm.hip, fc_skinny.hip: the fp32 dense layers */                                                              \
    X(FC_SKINNY, 1, ATOI, 1, "0: no skinny dense kernels")                                                            \
    X(GEMM_DEEP, 1, ATOI, 1, "0 off, 1 auto, 4 / 8: the deep GEMM with that many waves everywhere it applies")        \
    X(GEMM_DMA, 1, ATOI, 1, "0: register-staged tiles; 2: the DMA kernel also where 128 x 64 tiles would be taken")   \
    X(GEMM_DMA_PAD, 0, ATOI, 1, "bytes of dynamic LDS per DMA GEMM block (residency experiments)")                    \
    X(GEMM_DMA_NS, 0, ATOI, 1, "nonzero: the DMA GEMM's ring stages (8, 2, else 4)")                                  \
    X(GEMM_DBG, 0, ATOI, 0, "cycle stamps of the DMA GEMM (tools/dbg_gemm.py)")                                       \
    X(FC_WSPLIT, 0, ATOI, 1, "1 / 2 / 4 / 8: the dense weight gradient's K slabs")                                    \
    X(FC_DGRAD_SPLIT, 0, ATOI, 1, "n > 0: the dense input gradient's K slabs")                                        \
    X(SOFTMAX_TRAIN, 1, ATOI, 1, "0: the softmax layer's training step as three ops, not one kernel")                 \
    X(PAIR_DMA, 26, ATOI, 1, "the paired backward GEMM's ring stages * 10 + waves per SIMD (experiments)")            \
    X(PAIR_LDS_PAD, -1, ATOI, 1, "n >= 0: n bytes of LDS pad per paired backward GEMM block (A/B)")

enum tn_knob_id {
#define TN_KNOB_ID(name, def, form, agreed, doc) TN_K_##name,
    TN_KNOBS(TN_KNOB_ID)
#undef TN_KNOB_ID
    TN_K_COUNT
};

// (hidden: each library resolves its own table, also when both are loaded into one process)
#pragma GCC visibility push(hidden)

struct tn_knob_row {
    const char* name;
    int def, form, agreed;
};
inline constexpr tn_knob_row tn_knob_rows[TN_K_COUNT] = {
#define TN_KNOB_ROW(name, def, form, agreed, doc) {"TN_" #name, def, TN_KF_##form, agreed},
    TN_KNOBS(TN_KNOB_ROW)
#undef TN_KNOB_ROW
};

// every row's value, read from the environment once per process on first use (a function-local static: thread-safe)
inline const int* tn_knob_values() {
    static const struct Values {
        int v[TN_K_COUNT];
        Values() {
            for (int k = 0; k < TN_K_COUNT; ++k) {
                const tn_knob_row& r = tn_knob_rows[k];
                const char* e = getenv(r.name);
                if (r.form == TN_KF_SET) v[k] = e != nullptr;
                else if (!e) v[k] = r.def;
                else if (r.form == TN_KF_NOT0) v[k] = e[0] != '0';
                else if (r.form == TN_KF_POS) v[k] = atoi(e) > 0 ? atoi(e) : r.def;
                else v[k] = atoi(e);
            }
        }
    } values;
    return values.v;
}

inline int tn_knob(tn_knob_id k) { return tn_knob_values()[k]; }

// tn_knobs: "TN_<name>=<value>" of every agreed row, space-separated in table order
inline int tn_knobs_format(char* buf, int len) {
    if (!buf || len < 1) return TN_E_ARG;
    buf[0] = 0;
    for (int k = 0, n = 0; k < TN_K_COUNT; ++k) {
        if (!tn_knob_rows[k].agreed) continue;
        const int w = snprintf(buf + n, len - n, "%s%s=%d", n ? " " : "", tn_knob_rows[k].name, tn_knob(tn_knob_id(k)));
        if (w < 0 || w >= len - n) return TN_E_ARG;
        n += w;
    }
    return TN_OK;
}

#pragma GCC visibility pop
