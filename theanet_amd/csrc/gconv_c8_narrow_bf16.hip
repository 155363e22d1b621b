// DTYPE bfloat16: the narrow-group conv kernels of gconv_c8_narrow.hip on bf16 cells (c8_elem.h)
#define C8_BF16_TU
#include "gconv_c8_narrow.hip"
