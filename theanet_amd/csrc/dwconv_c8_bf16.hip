// DTYPE bfloat16: the depthwise conv kernels of dwconv_c8.hip on bf16 cells (c8_elem.h)
#define C8_BF16_TU
#include "dwconv_c8.hip"
