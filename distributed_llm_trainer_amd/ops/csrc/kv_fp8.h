// The FP8 KV cache (decode_kv8.hip, prefill_kv8.hip): conversions between fp32 and OCP e4m3fn bytes.
//
// A cache element is e4m3fn(clamp(x16, -448, 448)), x16 the value the 16-bit cache would hold (the
// caller rounds to the activation dtype first).  No scales.  gfx950 converts in hardware, round to
// nearest even with subnormals down to 2^-9; the clamp in front makes the conversion saturate (448
// is e4m3fn's largest finite value) and maps NaN to -448, so no byte is ever the NaN pattern 0x7F.
// Every e4m3 value is exact in fp32, bf16 and fp16: reading the cache rounds nothing.
#pragma once
#include "common.h"

typedef float kv8_float2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float kv8_clamp(float x) { return __builtin_fminf(__builtin_fmaxf(x, -448.f), 448.f); }

// four values -> four bytes, a at the lowest address: two v_cvt_pk_fp8_f32
__device__ __forceinline__ uint32_t kv8_pack4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a), kv8_clamp(b), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(c), kv8_clamp(d), w, true);
  return (uint32_t)w;
}
__device__ __forceinline__ uint2 kv8_pack8(const float (&x)[8]) {
  return make_uint2(kv8_pack4(x[0], x[1], x[2], x[3]), kv8_pack4(x[4], x[5], x[6], x[7]));
}
__device__ __forceinline__ uint8_t kv8_byte(float a) {
  return (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a), 0.f, 0, false) & 0xFF);
}

// four bytes -> four values: two v_cvt_pk_f32_fp8
__device__ __forceinline__ void kv8_unpack4(uint32_t w, float* f) {
  const kv8_float2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const kv8_float2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0];
  f[1] = lo[1];
  f[2] = hi[0];
  f[3] = hi[1];
}
__device__ __forceinline__ void kv8_unpack16(const uint4& w, float (&f)[16]) {
  kv8_unpack4(w.x, f);
  kv8_unpack4(w.y, f + 4);
  kv8_unpack4(w.z, f + 8);
  kv8_unpack4(w.w, f + 12);
}
