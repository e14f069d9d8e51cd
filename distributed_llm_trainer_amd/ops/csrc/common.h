// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of this framework.
//
// Conventions
//  * wave = 64 lanes; every block size is a multiple of 64.
//  * bf16 tensors are handled as raw 16-bit words and moved in 16-byte vectors
//    (8 x bf16 per lane) -- hipcc does not vectorise scalar bf16 loads.
//  * f32 -> bf16 uses the compiler cast (v_cvt_pk_bf16_f32, RNE, NaN-preserving).
//  * Dropout randomness: lowbias32 hash of (key ^ pair_index); one hash gives 16
//    bits to each of two neighbouring elements (see ops/rng.py for the contract).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DLT_API extern "C" __attribute__((visibility("default")))

typedef uint16_t bf16_t;
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float floatx4_t __attribute__((ext_vector_type(4)));
typedef float floatx16_t __attribute__((ext_vector_type(16)));
typedef short shortx4_t __attribute__((ext_vector_type(4)));

struct alignas(16) u16x8 { uint16_t v[8]; };
struct alignas(8) u16x4 { uint16_t v[4]; };

__device__ __forceinline__ float bf2f(uint16_t u) { return __uint_as_float(((uint32_t)u) << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(uint16_t, b);
}

// 16-bit activation formats.  HK = 0: bf16 (the default compute dtype); HK = 1: fp16
// (--mixed_precision fp16: the same kernels instantiated for IEEE half, RNE casts).
// Kernels that move activations as raw 16-bit words take HK as a template parameter and
// their launchers an `hk` argument (0 / 1).
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
template <int HK>
__device__ __forceinline__ float h2f(uint16_t u) {
  if constexpr (HK == 0) return __uint_as_float(((uint32_t)u) << 16);
  else return (float)__builtin_bit_cast(_Float16, u);
}
template <int HK>
__device__ __forceinline__ uint16_t f2h(float f) {
  if constexpr (HK == 0) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(uint16_t, b);
  } else {
    return __builtin_bit_cast(uint16_t, (_Float16)f);
  }
}
// launcher helper: run F<0> or F<1> by the runtime format
#define DLT_HK_DISPATCH(hk, ...) \
  do {                           \
    if ((hk) == 1) {             \
      constexpr int HKC = 1;     \
      __VA_ARGS__;               \
    } else {                     \
      constexpr int HKC = 0;     \
      __VA_ARGS__;               \
    }                            \
  } while (0)

__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// 16 random bits for flat element index `idx` under `key`.
__device__ __forceinline__ uint32_t drop_bits(uint32_t key, uint64_t idx) {
  uint32_t h = lowbias32(key ^ (uint32_t)(idx >> 1));
  return (idx & 1) ? (h >> 16) : (h & 0xffffu);
}

// sigmoid with the hardware reciprocal (v_rcp_f32, 1 ulp): the IEEE division hipcc
// emits for `1.f / x` is a ~10-instruction sequence, which dominated the SwiGLU GEMM
// epilogue.  Every SwiGLU kernel uses this one so the fused and unfused paths agree.
__device__ __forceinline__ float dlt_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
// GeGLU (mlp_activation "geglu"): tanh-GELU is exactly g * sigmoid(z(g)) with
// z(g) = 2 sqrt(2/pi) (g + 0.044715 g^3), so every GeGLU kernel is its SwiGLU form with
// phi = dlt_sigmoid(z(g)) in place of dlt_sigmoid(g) and, in the backward, the inner
// derivative z'(g) = 2 sqrt(2/pi) (1 + 0.134145 g^2):
//   act = g phi, act' = phi + g phi (1 - phi) z'(g).
// Every operation is an explicit product or fma (nothing left for the compiler to contract
// differently in two kernels), so fused and unfused forms agree bit for bit.
// z and z' are taken at g clamped to +-16: |z(16)| = 318, where exp(-z) has already
// underflowed to 0 / overflowed to inf and phi is exactly 1 / 0, so the clamp changes no
// result and g^2 cannot overflow (bf16's largest finite g would give z' = inf and 0 * inf).
// e = exp(-z) is returned for the backward: 1 - phi = e / (1 + e) = e phi, a product, never
// the cancelling subtraction; e = inf (phi = 0) takes 1 - phi = 1.  Saturated gates give
// phi (1 - phi) = 0 exactly, so act' = phi exactly and no NaN.
#define DLT_GELU_K 1.5957691216057308f  // 2 sqrt(2 / pi)
__device__ __forceinline__ float dlt_gelu_phi(float g, float& gc, float& e) {
  gc = fminf(fmaxf(g, -16.f), 16.f);
  const float z = (DLT_GELU_K * gc) * __builtin_fmaf(0.044715f, gc * gc, 1.f);
  e = __expf(-z);
  return __builtin_amdgcn_rcpf(1.f + e);  // dlt_sigmoid(z), e kept
}
__device__ __forceinline__ float dlt_gelu_phi(float g) {
  float gc, e;
  return dlt_gelu_phi(g, gc, e);
}
// act'(g) from dlt_gelu_phi's (phi, gc, e)
__device__ __forceinline__ float dlt_gelu_dact(float phi, float gc, float e) {
  const float omp = e < INFINITY ? e * phi : 1.f;
  const float dz = __builtin_fmaf(DLT_GELU_K * 0.134145f, gc * gc, DLT_GELU_K);
  return __builtin_fmaf(gc * (phi * omp), dz, phi);
}
// A GeGLU result on its way to the 16-bit store: opaque to instruction selection, so the fp32
// product is rounded to fp32 and then converted in every kernel.  Left to the compiler, the fp16
// k_gemm_fw4 epilogue got v_fma_mixlo_f16 (product and fp16 conversion in one instruction) where
// k_geglu_fwd has v_mul_f32 + v_cvt_pk_f16_f32, and the two differed in the last fp16 bit.
__device__ __forceinline__ float dlt_glu_pin(float x) {
  asm("" : "+v"(x));
  return x;
}
// The gate's multiplier of a gated MLP, ACT = 0: SwiGLU (sigmoid(g)), 1: GeGLU (phi)
enum { DLT_ACT_SWIGLU = 0, DLT_ACT_GEGLU = 1 };
template <int ACT>
__device__ __forceinline__ float dlt_glu_gate(float g) {
  if constexpr (ACT == DLT_ACT_GEGLU) return dlt_gelu_phi(g);
  else return dlt_sigmoid(g);
}
// tanh(x / cap) of the final-logit soft cap, k2 = 2 log2(e) / cap: with a = exp2(-|x| k2) in [0, 1]
// and r = rcp(1 + a) it is copysign((1 - a) r, x), and 1 - tanh^2 = 4 a r^2 (a and r are returned for
// it).  Nothing overflows; an underflowing a gives exactly +-1 and a derivative of exactly 0.
__device__ __forceinline__ float dlt_cap_tanh(float x, float k2, float& a, float& r) {
  a = __builtin_amdgcn_exp2f(-fabsf(x) * k2);
  r = __builtin_amdgcn_rcpf(1.f + a);
  return copysignf((1.f - a) * r, x);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the N neighbouring lanes (N a power of two, the group aligned to N) that share
// one head vector: an xor butterfly adds the same pairs on every lane, so all N lanes end
// with the same bits
template <int N>
__device__ __forceinline__ float head_sum(float v) {
#pragma unroll
  for (int o = 1; o < N; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

#define DLT_CHECK_LAUNCH() return (int)hipGetLastError()

// Device-side bounds checks, compiled in only for the debug library
// (`python -m distributed_llm_trainer_amd.ops.build --debug` -> _dlt_kernels_debug.so,
// selected at run time with DLT_KERNEL_DEBUG=1): a failed check prints the condition
// and traps the wave, so a bad token id or target stops at the faulting kernel instead
// of silently reading another row (XNACK is off: out-of-range reads inside the
// allocation do not fault).
#ifdef DLT_DEBUG
#define DLT_DASSERT(cond)                                                        \
  do {                                                                           \
    if (!(cond)) {                                                               \
      printf("DLT_DASSERT failed %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      __builtin_trap();                                                          \
    }                                                                            \
  } while (0)
#else
#define DLT_DASSERT(cond) ((void)0)
#endif
