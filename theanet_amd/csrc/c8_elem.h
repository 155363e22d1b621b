// The 16-bit element type of the c8 tensors (conv_c8.hip, fc_c8.hip, elastic.hip): DTYPE 'float16' stores IEEE halfs,
// DTYPE 'bfloat16' stores bf16 (fp32's exponent range, 8 significant bits).  Every c8 kernel takes one of these as its
// element-type parameter; the layout, the tiling and the instruction schedule are the same for both -- on gfx950 the
// 32x32x16 f16 and bf16 MFMAs share their cycles, operand lane maps and C/D layout, and everything that only MOVES 16-bit
// values (LDS-DMA, ds_read_b64_tr_b16, masks, the pooled-gradient expansion) is type-blind.  What differs is here: the
// storage type and the MFMA builtin; the kernels convert with plain casts, (typename E::T)v and (float)h -- fp32 -> bf16
// is v_cvt_pk_bf16_f32 (nearest even, as fp32 -> half), bf16 -> fp32 a shift (exact).  (Plain casts on purpose: with
// the fp16 element type the kernels' source is then the pre-bf16 source token for token, and tools/isa_diff.py checks
// that their instructions are too -- conversion helpers, even always-inlined ones, moved hipcc's inlining and
// scheduling decisions in a few kernels.)
#pragma once
#include "conv_tile_common.h"

struct C8H {                 // IEEE half (DTYPE 'float16', tn_set_matmul_dtype mode 1)
    typedef _Float16 T;
    typedef _Float16 v8 __attribute__((ext_vector_type(8)));
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    static constexpr bool BF = false;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};

struct C8B {                 // bfloat16 (DTYPE 'bfloat16', tn_set_matmul_dtype mode 2)
    typedef __bf16 T;
    typedef __bf16 v8 __attribute__((ext_vector_type(8)));
    typedef __bf16 v4 __attribute__((ext_vector_type(4)));
    static constexpr bool BF = true;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};

// the element type of a context's c8 tensors: halfs unless the context is in mode 2
static inline bool tn_c8_bf16(const tn_ctx* ctx) { return ctx->mm_f16 == 2; }

// ONE element type per translation unit.  conv_c8.hip / fc_c8.hip instantiate their kernels for C8H; conv_c8_bf16.hip /
// fc_c8_bf16.hip include them with C8_BF16_TU defined and instantiate the same templates for C8B.  (In one unit, the
// second instantiation of a kernel changed how hipcc compiled the first -- the shared device-library calls of the
// activations and of the elastic-field rider gained callers, and their inlining moved -- and the fp16 kernels must
// stay exactly as they were: tools/isa_diff.py.)  The C8H unit's entry points forward to the C8B unit's (same
// signature, name prefixed c8b_) when the context is in mode 2.
#ifdef C8_BF16_TU
#define C8E C8B
#define C8_API(name) c8b_##name
#define C8_TO_BF16(name, ...)
#else
#define C8E C8H
#define C8_API(name) name
#define C8_TO_BF16(name, ...) \
    if (tn_c8_bf16(ctx)) return c8b_##name(__VA_ARGS__)
#endif
