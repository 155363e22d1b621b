// DTYPE 'bfloat16': the test-version kernel of drop_c8.hip (tn_c8_scale) instantiated for bf16 cells (C8B), in a translation
// unit of its own (c8_elem.h).  drop_c8.hip's entry point forwards here, to c8b_tn_c8_scale, when the context is in mode 2;
// the train ops only move 16-bit patterns and exist once.
#define C8_BF16_TU 1
#include "drop_c8.hip"
