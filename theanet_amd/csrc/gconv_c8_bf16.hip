// DTYPE bfloat16: the grouped conv kernels of gconv_c8.hip on bf16 cells (c8_elem.h)
#define C8_BF16_TU
#include "gconv_c8.hip"
