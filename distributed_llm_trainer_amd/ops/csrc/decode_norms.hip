// The fused decode step of QK-norm and post-norm models (cfg.qk_norm / cfg.post_norm), in a
// translation unit of its own so that decode.hip's instantiations keep their code:
//
//   dec_norm_qkv_qkn : h -> RMSNorm -> QKV GEMV -> per-head RMSNorm(q, k) -> RoPE -> cache row, q
//   dec_gemv_out     : a = bf16(x . W^T)                 (the raw branch: o_proj / down_proj output)
//   PN forms         : k_dec_norm_qkv / _qkn / _gu / _head with the post-norm prologue
//                      (decode.hip stage_postnorm_normed): h_out = h_in + bf16(RMSNorm(a) * pn_w)
//
// With post-norms the value added to the residual needs the norm of the whole branch row, which
// k_dec_gemv_res (rows spread over workgroups) cannot take.  The step keeps five kernels per
// layer: the producer stores the raw branch (k_dec_gemv_out) and the next kernel -- which norms
// the whole residual row redundantly in every workgroup anyway -- absorbs the post-norm.  The
// residual alternates between two fp32 buffers (h_out never aliases h_in).
#define DLT_NORMS_TU 1
#include "decode.hip"

// QK-norm needs mean(x^2) over the 64 dims of a head, on the bf16-rounded GEMV outputs before
// RoPE; k_dec_norm_qkv's quarter-head workgroups cannot form it.  Here one workgroup owns one
// whole head of the packed q | k | v row: grid (nh + 2 nkv), NT / 64 waves, each 4 rows at a time
// (one load round trip, as everywhere here) in 1024 / NT passes: wave w owns dims 4 (p NW + w) ..+3
// in pass p.  rows_pre issues the first pass's weight loads before the activations are staged.
// Lane 0 of each wave writes its rounded values to outv[B][64]; after one barrier a wave per
// batch row (lane = dim) takes the row's 64-term sum with wave_sum64, forms y = x * rsqrt(mean + eps) * w[d]
// in fp32 (w = q_norm / k_norm), rotates y against lane d ^ 32 (the NeoX partner) and rounds once
// to bf16: eval/decode.py's _qk_norm, _rope and .to(dt).  V heads skip norm and RoPE.
// NT per B (qkn_nt): 16 waves hold a wave to 128 VGPRs, which B <= 2 fits; B = 4 takes 8 waves and
// two passes, B = 8 4 waves and four (no scratch anywhere: profiles/decode_norms.md).
// F8 (decode_kv8.hip only): e4m3 caches, as k_dec_norm_qkv's F8 form.
template <int B, bool PN, int NT, bool F8 = false>
__global__ __launch_bounds__(NT) void k_dec_norm_qkv_qkn(
    const float* __restrict__ h, const void* __restrict__ lnw, int wbf16, float eps, const bf16_t* __restrict__ wqkv,
    const void* __restrict__ qnw, const void* __restrict__ knw, int qkbf16, const float* __restrict__ cosT,
    const float* __restrict__ sinT, const long* __restrict__ posp, bf16_t* __restrict__ qout, bf16_t* __restrict__ kc,
    bf16_t* __restrict__ vc, int H, int nh, int nkv, int maxS, const bf16_t* __restrict__ pa,
    const void* __restrict__ pnw, int pnbf16, float* __restrict__ hout) {
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(dsm);                    // [B][H]
  float* red = reinterpret_cast<float*>(dsm + (size_t)B * H * 2);  // [B][NW] (dec_lds_qkn: room for 16)
  float* outv = red + B * 16;                                      // [B][64]
  constexpr int NW = NT / 64, NP = 1024 / NT;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int hb = blockIdx.x;
  const int blk = hb < nh ? 0 : (hb < nh + nkv ? 1 : 2);
  const int head = hb - (blk == 0 ? 0 : (blk == 1 ? nh : nh + nkv));
  const bf16_t* rows[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rows[r] = wqkv + (size_t)(hb * 64 + 4 * wid + r) * H;
  RowsPre<4, 2> pre;
  rows_pre<4, 2>(rows, H, pre);
  if constexpr (PN)
    stage_postnorm_normed<B, NT>(h, pa, pnw, pnbf16, hout, H, lnw, wbf16, eps, xs, red);
  else
    stage_normed<B, NT>(h, H, lnw, wbf16, eps, xs, red);
#pragma unroll 1
  for (int p = 0; p < NP; ++p) {
    float acc[4][B];
    rows_dot<B, 4, 2>(rows, H, xs, pre, acc);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int b = 0; b < B; ++b)
          outv[b * 64 + 4 * (p * NW + wid) + r] = bf_round(acc[r][b]);  // torch bf16 matmul output
    }
    if (p + 1 < NP) {  // the next pass's rows: 4 NW dims further
#pragma unroll
      for (int r = 0; r < 4; ++r) rows[r] += (size_t)4 * NW * H;
      rows_pre<4, 2>(rows, H, pre);
    }
  }
  __syncthreads();
  const int pos = (int)posp[0];
  DLT_DASSERT(pos >= 0 && pos < maxS);
  if (pos < 0 || pos >= maxS) return;  // never write past the cache (as k_dec_norm_qkv)
  for (int b = wid; b < B; b += NW) {  // a wave per batch row, lane = dim
    const int d = lane;
    float y = outv[b * 64 + d];
    if (blk < 2) {
      const float rstd = rsqrtf(wave_sum64(y * y) / 64.f + eps);
      y = y * rstd * norm_w(blk == 0 ? qnw : knw, qkbf16, d);
      const float o = __shfl_xor(y, 32, 64);  // the NeoX partner d ^ 32
      const float c = cosT[(size_t)pos * 32 + (d & 31)], sn = sinT[(size_t)pos * 32 + (d & 31)];
      y = d < 32 ? y * c - o * sn : y * c + o * sn;
    }
    if (blk == 0)
      qout[(size_t)b * H + head * 64 + d] = f2bf(y);
#ifdef DLT_KV8_TU
    else if constexpr (F8)
      reinterpret_cast<uint8_t*>(blk == 1 ? kc : vc)[(((size_t)b * nkv + head) * maxS + pos) * 64 + d] = kv8_byte(bf_round(y));
#endif
    else
      (blk == 1 ? kc : vc)[(((size_t)b * nkv + head) * maxS + pos) * 64 + d] = f2bf(y);
  }
}

// DLT_KV8_TU: this file as included by decode_kv8.hip, which sees the helpers, k_dec_norm_qkv and
// k_dec_norm_qkv_qkn (for their F8 forms), the two budget functions below and no launcher.
constexpr int qkn_nt(int B) { return B <= 2 ? 1024 : (B == 4 ? 512 : 256); }

// LDS of k_dec_norm_qkv_qkn: the normed rows, 16 partials and one head's outputs per batch row
static size_t dec_lds_qkn(int B, int K) { return (size_t)B * K * 2 + (size_t)B * 16 * 4 + (size_t)B * 64 * 4; }

// The post-norm operands of a PN launch: all of pa, pnw set, hout distinct from h (null for the
// head, which stores no residual).
static bool dec_pn_ok(const float* h, const bf16_t* pa, const void* pnw, const float* hout) {
  return pa && pnw && hout != h;
}

#ifndef DLT_KV8_TU

// a[b][r] = bf16(x[b] . W[r]): k_dec_gemv_res with a store in place of the residual add.
template <int B>
__global__ __launch_bounds__(DEC_NT) void k_dec_gemv_out(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                         bf16_t* __restrict__ a, int R, int K) {
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(dsm);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r0 = blockIdx.x * 16 + wid * 4;
  const bf16_t* rows[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rows[r] = w + (size_t)min(r0 + r, R - 1) * K;
  RowsPre<4, 4> pre;
  rows_pre<4, 4>(rows, K, pre);
  stage_copy<B>(x, K, xs);
  float acc[4][B];
  rows_dot<B, 4, 4>(rows, K, xs, pre, acc);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r0 + r < R) {
#pragma unroll
        for (int b = 0; b < B; ++b) a[(size_t)b * R + r0 + r] = f2bf(acc[r][b]);
      }
  }
}

// ------------------------------------------------------------------------ launchers

// dlt_dec_norm_qkv_gqa (nkv == nh: the multi-head layout) with the post-norm prologue.
DLT_API int dlt_dec_norm_qkv_pn(const float* h, const void* lnw, int wbf16, float eps, const bf16_t* wqkv,
                                const float* cosT, const float* sinT, const long* pos, bf16_t* qout, bf16_t* kc,
                                bf16_t* vc, const bf16_t* pa, const void* pnw, int pnbf16, float* hout, int B, int H,
                                int nh, int nkv, int maxS, hipStream_t st) {
  if (H != nh * 64 || H % 8 || nkv < 1 || nh % nkv || maxS < 1 || dec_lds(B, H) > 160 * 1024) return -1;
  if (!dec_pn_ok(h, pa, pnw, hout) || !hout) return -1;
#define L(BB)                                                                                        \
  k_dec_norm_qkv<BB, true><<<(nh + 2 * nkv) * 4, DEC_NT, dec_lds(BB, H), st>>>(                      \
      h, lnw, wbf16, eps, wqkv, cosT, sinT, pos, qout, kc, vc, H, nh, nkv, maxS, pa, pnw, pnbf16, hout)
  DEC_DISPATCH(B, L)
#undef L
  DLT_CHECK_LAUNCH();
}

// The QK-norm form: qnw / knw [64] (fp32, or bf16 with qkbf16).  pa null: no post-norm prologue.
DLT_API int dlt_dec_norm_qkv_qkn(const float* h, const void* lnw, int wbf16, float eps, const bf16_t* wqkv,
                                 const void* qnw, const void* knw, int qkbf16, const float* cosT, const float* sinT,
                                 const long* pos, bf16_t* qout, bf16_t* kc, bf16_t* vc, const bf16_t* pa,
                                 const void* pnw, int pnbf16, float* hout, int B, int H, int nh, int nkv, int maxS,
                                 hipStream_t st) {
  if (H != nh * 64 || H % 8 || nkv < 1 || nh % nkv || maxS < 1 || dec_lds_qkn(B, H) > 160 * 1024) return -1;
  if (!qnw || !knw) return -1;
  if (pa && (!dec_pn_ok(h, pa, pnw, hout) || !hout)) return -1;
#define L(BB)                                                                                                     \
  if (pa)                                                                                                         \
    k_dec_norm_qkv_qkn<BB, true, qkn_nt(BB)><<<nh + 2 * nkv, qkn_nt(BB), dec_lds_qkn(BB, H), st>>>(                               \
        h, lnw, wbf16, eps, wqkv, qnw, knw, qkbf16, cosT, sinT, pos, qout, kc, vc, H, nh, nkv, maxS, pa, pnw,     \
        pnbf16, hout);                                                                                            \
  else                                                                                                            \
    k_dec_norm_qkv_qkn<BB, false, qkn_nt(BB)><<<nh + 2 * nkv, qkn_nt(BB), dec_lds_qkn(BB, H), st>>>(                              \
        h, lnw, wbf16, eps, wqkv, qnw, knw, qkbf16, cosT, sinT, pos, qout, kc, vc, H, nh, nkv, maxS, nullptr,     \
        nullptr, 0, nullptr)
  DEC_DISPATCH(B, L)
#undef L
  DLT_CHECK_LAUNCH();
}

DLT_API int dlt_dec_gemv_out(const bf16_t* x, const bf16_t* w, bf16_t* a, int B, int R, int K, hipStream_t st) {
  if (R < 1 || K < 8 || K % 8 || (size_t)B * K * 2 > 160 * 1024) return -1;
#define L(BB) k_dec_gemv_out<BB><<<(R + 15) / 16, DEC_NT, (size_t)BB * K * 2, st>>>(x, w, a, R, K)
  DEC_DISPATCH(B, L)
#undef L
  DLT_CHECK_LAUNCH();
}

// dlt_dec_norm_gu / dlt_dec_norm_gu_geglu (geglu != 0) with the post-norm prologue.
DLT_API int dlt_dec_norm_gu_pn(const float* h, const void* lnw, int wbf16, float eps, const bf16_t* wgu, bf16_t* s,
                               const bf16_t* pa, const void* pnw, int pnbf16, float* hout, int geglu, int B, int H,
                               int I, hipStream_t st) {
  if (H <= 0 || I <= 0 || H % 8 || dec_lds(B, H) > 160 * 1024) return -1;
  if (!dec_pn_ok(h, pa, pnw, hout) || !hout) return -1;
#define L(BB)                                                                                              \
  if (geglu)                                                                                               \
    k_dec_norm_gu<BB, DLT_ACT_GEGLU, true><<<(I + 7) / 8, DEC_NT, dec_lds(BB, H), st>>>(                   \
        h, lnw, wbf16, eps, wgu, s, H, I, pa, pnw, pnbf16, hout);                                          \
  else                                                                                                     \
    k_dec_norm_gu<BB, DLT_ACT_SWIGLU, true><<<(I + 7) / 8, DEC_NT, dec_lds(BB, H), st>>>(                  \
        h, lnw, wbf16, eps, wgu, s, H, I, pa, pnw, pnbf16, hout)
  DEC_DISPATCH(B, L)
#undef L
  DLT_CHECK_LAUNCH();
}

// dlt_dec_norm_head (cap == 0) / dlt_dec_norm_head_cap with the post-norm prologue; hout may be
// null: the head stores no residual.
DLT_API int dlt_dec_norm_head_pn(const float* h, const void* lnw, int wbf16, float eps, const bf16_t* emb,
                                 float* logits, const bf16_t* pa, const void* pnw, int pnbf16, float* hout, float cap,
                                 int B, int H, int V, hipStream_t st) {
  if (H <= 0 || V <= 0 || H % 8 || dec_lds(B, H) > 160 * 1024 || !(cap >= 0.f) || cap > 3.0e38f) return -1;
  if (!dec_pn_ok(h, pa, pnw, hout)) return -1;
#define L(BB)                                                                                                  \
  if (cap > 0.f)                                                                                               \
    k_dec_norm_head<BB, true, true><<<(V + 15) / 16, DEC_NT, dec_lds(BB, H), st>>>(                            \
        h, lnw, wbf16, eps, emb, logits, H, V, cap, pa, pnw, pnbf16, hout);                                    \
  else                                                                                                         \
    k_dec_norm_head<BB, false, true><<<(V + 15) / 16, DEC_NT, dec_lds(BB, H), st>>>(                           \
        h, lnw, wbf16, eps, emb, logits, H, V, 0.f, pa, pnw, pnbf16, hout)
  DEC_DISPATCH(B, L)
#undef L
  DLT_CHECK_LAUNCH();
}
#endif  // DLT_KV8_TU
