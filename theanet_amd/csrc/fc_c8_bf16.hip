// DTYPE 'bfloat16': the kernels of fc_c8.hip instantiated for bf16 cells (C8B), in a translation unit of their own
// (c8_elem.h).  fc_c8.hip's entry points forward here, to c8b_tn_c8_fc_*, when the context is in mode 2.
#define C8_BF16_TU 1
#define fc8_fwd_finish_kernel c8b_fc8_fwd_finish_kernel      // (type-blind: fp32 slabs in, fp32 out)
#include "fc_c8.hip"
