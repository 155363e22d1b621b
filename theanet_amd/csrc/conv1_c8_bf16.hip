// DTYPE bfloat16: the 1x1 conv kernels of conv1_c8.hip on bf16 cells (c8_elem.h)
#define C8_BF16_TU
#include "conv1_c8.hip"
