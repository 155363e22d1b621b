// DTYPE bfloat16: the dilated conv kernels of dilconv_c8.hip on bf16 cells (c8_elem.h)
#define C8_BF16_TU
#include "dilconv_c8.hip"
