// The GeGLU form of k_gemm_fw4's gate/up epilogue in a translation unit of its own (see
// gemm_bf16_geglu.hip).
#define DLT_GEGLU_TU 1
#include "gemm_fw4.hip"
