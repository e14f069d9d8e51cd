// The GeGLU form of k_dec_norm_gu in a translation unit of its own (see gemm_bf16_geglu.hip).
#define DLT_GEGLU_TU 1
#include "decode.hip"
