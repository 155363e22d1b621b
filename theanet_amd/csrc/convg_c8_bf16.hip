// DTYPE bfloat16: the general conv kernels of convg_c8.hip on bf16 cells (c8_elem.h)
#define C8_BF16_TU
#include "convg_c8.hip"
