// DTYPE 'bfloat16': the kernels of head_c8.hip instantiated for bf16 cells (C8B), in a translation unit of their own
// (c8_elem.h).  head_c8.hip's entry points forward here, to c8b_tn_c8_head_*, when the context is in mode 2.
#define C8_BF16_TU 1
#include "head_c8.hip"
