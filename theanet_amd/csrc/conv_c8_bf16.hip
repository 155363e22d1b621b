// DTYPE 'bfloat16': the kernels of conv_c8.hip instantiated for bf16 cells (C8B), in a translation unit of their own
// (c8_elem.h).  conv_c8.hip's entry points forward here, to c8b_tn_c8_*, when the context is in mode 2.
#define C8_BF16_TU 1
#define c8_zero_cell_g c8b_zero_cell_g
#include "conv_c8.hip"
