// GeGLU (tanh-GELU gated MLP, mlp_activation "geglu"): the unfused forward / backward, the
// forms of k_swiglu_fwd / k_swiglu_bwd (elementwise.hip) with phi = sigmoid(z(g)) as the
// gate's multiplier (common.h, dlt_gelu_phi).  8 elements (16 B) per lane and access.
//   s  = bf16(act(g) * u),            act(g) = g phi
//   dg = bf16(ds * (u * act'(g))),    act'(g) = phi + g phi (1 - phi) z'(g)
//   du = bf16(ds * act(g))
// in fp32 on the 16-bit g, u, ds, one rounding per output.  act is formed before it meets
// ds or u, so a saturated gate (phi = 0 exactly) gives exact zeros whatever ds and u are.
// The fused epilogues (k_gemm_fw4, k_gemm_bf16, k_dec_norm_gu GeGLU forms) call the same
// helpers in the same order: same bits.
// Every result passes dlt_glu_pin before its conversion (common.h).
#include "common.h"

template <int HK>
__global__ __launch_bounds__(256) void k_geglu_fwd(const bf16_t* __restrict__ gu, bf16_t* __restrict__ a, int M, int I) {
  const int q = I >> 3;
  const size_t total = (size_t)M * q;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i / q;
    const int c = (int)(i % q) * 8;
    const u16x8 g = *reinterpret_cast<const u16x8*>(gu + m * 2 * I + c);
    const u16x8 u = *reinterpret_cast<const u16x8*>(gu + m * 2 * I + I + c);
    u16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gv = h2f<HK>(g.v[e]);
      o.v[e] = f2h<HK>(dlt_glu_pin(gv * dlt_gelu_phi(gv) * h2f<HK>(u.v[e])));
    }
    *reinterpret_cast<u16x8*>(a + m * I + c) = o;
  }
}

// S: also writes s (the forward's bits) to s_out, as k_swiglu_bwd's s_out does
template <int HK, bool S>
__global__ __launch_bounds__(256) void k_geglu_bwd(const bf16_t* __restrict__ gu, const bf16_t* __restrict__ da,
                                                   bf16_t* __restrict__ dgu, bf16_t* __restrict__ s_out, int M,
                                                   int I) {
  const int q = I >> 3;
  const size_t total = (size_t)M * q;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i / q;
    const int c = (int)(i % q) * 8;
    const u16x8 g = *reinterpret_cast<const u16x8*>(gu + m * 2 * I + c);
    const u16x8 u = *reinterpret_cast<const u16x8*>(gu + m * 2 * I + I + c);
    const u16x8 d = *reinterpret_cast<const u16x8*>(da + m * I + c);
    u16x8 og, ou, os;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gv = h2f<HK>(g.v[e]), uv = h2f<HK>(u.v[e]), dv = h2f<HK>(d.v[e]);
      float gc, ex;
      const float phi = dlt_gelu_phi(gv, gc, ex);
      const float act = gv * phi;
      og.v[e] = f2h<HK>(dlt_glu_pin(dv * (uv * dlt_gelu_dact(phi, gc, ex))));
      ou.v[e] = f2h<HK>(dlt_glu_pin(dv * act));
      if constexpr (S) os.v[e] = f2h<HK>(dlt_glu_pin(act * uv));
    }
    *reinterpret_cast<u16x8*>(dgu + m * 2 * I + c) = og;
    *reinterpret_cast<u16x8*>(dgu + m * 2 * I + I + c) = ou;
    if constexpr (S) *reinterpret_cast<u16x8*>(s_out + m * I + c) = os;
  }
}

static inline int geglu_blocks(size_t total) {
  const size_t b = (total + 255) / 256;
  return (int)(b > 16384 ? 16384 : (b == 0 ? 1 : b));
}

DLT_API int dlt_geglu_fwd(const bf16_t* gu, bf16_t* a, int M, int I, int hk, hipStream_t st) {
  if (M <= 0 || I <= 0 || I % 8) return -1;
  DLT_HK_DISPATCH(hk, k_geglu_fwd<HKC><<<geglu_blocks((size_t)M * (I / 8)), 256, 0, st>>>(gu, a, M, I));
  DLT_CHECK_LAUNCH();
}

DLT_API int dlt_geglu_bwd(const bf16_t* gu, const bf16_t* da, bf16_t* dgu, bf16_t* s_out, int M, int I, int hk,
                          hipStream_t st) {
  if (M <= 0 || I <= 0 || I % 8) return -1;
  const int blocks = geglu_blocks((size_t)M * (I / 8));
  if (s_out) DLT_HK_DISPATCH(hk, k_geglu_bwd<HKC, true><<<blocks, 256, 0, st>>>(gu, da, dgu, s_out, M, I));
  else DLT_HK_DISPATCH(hk, k_geglu_bwd<HKC, false><<<blocks, 256, 0, st>>>(gu, da, dgu, s_out, M, I));
  DLT_CHECK_LAUNCH();
}
