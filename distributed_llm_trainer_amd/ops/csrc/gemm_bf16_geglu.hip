// The GeGLU forms of k_gemm_bf16's gated epilogues (gate/up forward, down data gradient +
// activation backward), in a translation unit of their own: built without packed-fp32 ops
// (ops/build.py), and the existing instantiations in gemm_bf16.hip stay the code they were.
#define DLT_GEGLU_TU 1
#include "gemm_bf16.hip"
