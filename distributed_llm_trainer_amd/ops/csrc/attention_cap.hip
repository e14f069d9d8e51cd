// The CAP forms of the flash-attention kernels (attention-score soft-capping,
// GPTConfig.attn_softcap): scores = cap * tanh(scale q.k / cap) before the masks and the softmax.
//
// The kernels are attention_fwd_body.h and attention_bwd_body.h with CAP = true: right after the
// S = K.Q^T MFMAs the score accumulator becomes t = tanh(scale s / cap) in place (cap_tanh,
// attention.h) and c_log2 is cap * log2(e), so the running max, the deferred rescale, M_DEAD, the
// sink epilogue and the lse store run unchanged in units of t; keys hidden by a mask go to -inf
// (forward) or p = 0 (backward) after the cap, never to -cap.  The backward tiles rebuild t the
// same way from their own accumulator and multiply dS by 1 - t^2 = 4 a r^2 before the dQ / dK
// products; delta, the sink gradient and dV are the plain kernels'.  Every DROP / HK / D / DOC /
// GQA combination of the plain kernels, the forward also with SINK.  A translation unit of its
// own for attention_sink.hip's reason: attention.hip's kernels must compile to what they were.
#include "attention.h"
#define DLT_ATTN_BWD_SECTION 0
#include "attention_bwd_body.h"

// cap_k is a kernel argument; the compiler may leave its scalar load to the first use, inside
// a tile step's counted LDS wait (lgkm_wait4: an SMEM load in flight there would let the wait
// retire the wrong fragments).  This pins the load, and its wait, to the kernel's start.
#define CAP_PIN(x) asm volatile("" : "+s"(x))

template <bool DROP, int HK, int D, bool DOC, bool GQA, bool SINK>
__global__ __launch_bounds__(NT) ATTN_WAVES(D) void k_attn_fwd_cap(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, bf16_t* __restrict__ o,
    float* __restrict__ lse, const uint32_t* __restrict__ mask, int S, int nh, float c_log2, float dscale, long in_bs,
    int in_hs, int in_rs, int xcd_map, const int* __restrict__ dlo, int G, long kv_bs, int kv_hs, int kv_rs,
    const float* __restrict__ sink, float cap_k) {
  constexpr bool CAP = true;
  CAP_PIN(cap_k);
  CAP_PIN(c_log2);
#include "attention_fwd_body.h"
}

template <bool DROP, int HK, int D, bool DOC>
__global__ __launch_bounds__(NT) ATTN_WAVES(D) void k_attn_bwd_dkdv_cap(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    const uint32_t* __restrict__ maskT, bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int S, int nh, float c_log2,
    float scale, float dscale, long in_bs, int in_hs, int in_rs, long out_bs, int out_hs, int out_rs,
    const float* __restrict__ cosT, const float* __restrict__ sinT, int xcd_map, const int* __restrict__ dhi,
    float cap_k) {
  constexpr bool CAP = true;
  CAP_PIN(cap_k);
  CAP_PIN(c_log2);
#define DLT_ATTN_BWD_SECTION 1
#include "attention_bwd_body.h"
}

template <bool DROP, int HK, int D, bool DOC>
__global__ __launch_bounds__(NT) ATTN_WAVES(D) void k_attn_bwd_dkdv_gqa_cap(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    const uint32_t* __restrict__ maskT, bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int S, int nh, float c_log2,
    float scale, float dscale, long in_bs, int in_hs, int in_rs, long out_bs, int out_hs, int out_rs,
    const float* __restrict__ cosT, const float* __restrict__ sinT, int xcd_map, const int* __restrict__ dhi, int G,
    long kv_bs, int kv_hs, int kv_rs, float cap_k) {
  constexpr bool CAP = true;
  CAP_PIN(cap_k);
  CAP_PIN(c_log2);
#define DLT_ATTN_BWD_SECTION 2
#include "attention_bwd_body.h"
}

template <bool DROP, int HK, int D, bool DOC, bool GQA>
__global__ __launch_bounds__(NT) ATTN_WAVES(D) void k_attn_bwd_dq_cap(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout, const bf16_t* __restrict__ o, const float* __restrict__ lse,
    float* __restrict__ delta, const uint32_t* __restrict__ mask, bf16_t* __restrict__ dq, int S, int nh, float c_log2,
    float scale, float dscale, long in_bs, int in_hs, int in_rs, long out_bs, int out_hs, int out_rs,
    const float* __restrict__ cosT, const float* __restrict__ sinT, int xcd_map, const int* __restrict__ dlo, int G,
    long kv_bs, int kv_hs, int kv_rs, float cap_k) {
  constexpr bool CAP = true;
  CAP_PIN(cap_k);
  CAP_PIN(c_log2);
#define DLT_ATTN_BWD_SECTION 3
#include "attention_bwd_body.h"
}

// a: checked by dlt_attn_fwd (head_dim, strides, nkv, the cap, the keep-bit buffer), keep bits written
int attn_fwd_cap_launch(const dlt_attn_args* a, hipStream_t st) {
  const int nh = a->nh, nkv = a->nkv, S = a->S;
  if (!(a->softcap > 0.f) || !attn_hd_ok(a->hd) || S <= 0 || nkv < 0 || (nkv && nh % nkv)) return -1;
  const dlt_attn_stride sq = a->stride.q, skv = nkv ? a->stride.kv : dlt_attn_stride{0, 0, 0};
  const int G = nkv ? nh / nkv : 1;
  const int nrb = (S + RB - 1) / RB;
  const int xm = xcd_map_enabled();
  const dim3 grid(attn_grid(nrb, a->B * nh, xm));  // work items, see work_item()
  // the accumulator holds t = tanh(scale s / cap): exp2 units per unit of t, and cap_tanh's factor
  const float c_log2 = a->softcap * LOG2E, cap_k = 2.f * LOG2E * a->scale / a->softcap;
  DLT_BOOL_DISPATCH(SINKC, a->sink, DLT_BOOL_DISPATCH(DROPC, a->thr, DLT_BOOL_DISPATCH(GQAC, nkv,
      DLT_BOOL_DISPATCH(DOCC, a->lo, DLT_HD_DISPATCH(a->hd, DLT_HK_DISPATCH(a->hk,
          k_attn_fwd_cap<DROPC, HKC, HDC, DOCC, GQAC, SINKC><<<grid, NT, 0, st>>>(
              a->q, a->k, a->v, a->o, a->lse, DROPC ? a->mask : nullptr, S, nh, c_log2, a->dscale, sq.b, sq.h, sq.r,
              xm, a->lo, G, skv.b, skv.h, skv.r, a->sink, cap_k)))))));
  DLT_CHECK_LAUNCH();
}

// a: checked by dlt_attn_bwd.  dQ (which writes delta) then dK/dV, as there.
int attn_bwd_cap_launch(const dlt_attn_args* a, hipStream_t st) {
  const int nh = a->nh, nkv = a->nkv, S = a->S;
  if (!(a->softcap > 0.f) || !attn_hd_ok(a->hd) || S <= 0 || nkv < 0 || (nkv && nh % nkv)) return -1;
  const dlt_attn_stride sq = a->stride.q, sdq = a->stride.dq;
  const dlt_attn_stride skv = nkv ? a->stride.kv : dlt_attn_stride{0, 0, 0}, sdkv = nkv ? a->stride.dkv : sdq;
  const int G = nkv ? nh / nkv : 1;
  const float scale = a->scale, dscale = a->dscale;
  const float c_log2 = a->softcap * LOG2E, cap_k = 2.f * LOG2E * scale / a->softcap;
  const int nrb = (S + RB - 1) / RB;
  const int xm = xcd_map_enabled();
  const dim3 gk(attn_grid(nrb, a->B * (nkv ? nkv : nh), xm)), gq(attn_grid(nrb, a->B * nh, xm));
  const uint32_t* mask = a->thr ? a->mask : nullptr;
  const uint32_t* maskT = mask ? mask + (size_t)a->B * nh * S * ((S + 31) / 32) : nullptr;
  DLT_BOOL_DISPATCH(DROPC, mask, {
    DLT_BOOL_DISPATCH(GQAC, nkv, DLT_BOOL_DISPATCH(DOCC, a->lo, DLT_HD_DISPATCH(a->hd, DLT_HK_DISPATCH(a->hk,
        k_attn_bwd_dq_cap<DROPC, HKC, HDC, DOCC, GQAC><<<gq, NT, 0, st>>>(
            a->q, a->k, a->v, a->dout, a->o, a->lse, a->delta_ws, mask, a->dq, S, nh, c_log2, scale, dscale, sq.b,
            sq.h, sq.r, sdq.b, sdq.h, sdq.r, a->cosT, a->sinT, xm, a->lo, G, skv.b, skv.h, skv.r, cap_k)))));
    if (nkv)  // grid over the B * nkv KV heads
      DLT_BOOL_DISPATCH(DOCC, a->hi, DLT_HD_DISPATCH(a->hd, DLT_HK_DISPATCH(a->hk,
          k_attn_bwd_dkdv_gqa_cap<DROPC, HKC, HDC, DOCC><<<gk, NT, 0, st>>>(
              a->q, a->k, a->v, a->dout, a->lse, a->delta_ws, maskT, a->dk, a->dv, S, nh, c_log2, scale, dscale, sq.b,
              sq.h, sq.r, sdkv.b, sdkv.h, sdkv.r, a->cosT, a->sinT, xm, a->hi, G, skv.b, skv.h, skv.r, cap_k))));
    else
      DLT_BOOL_DISPATCH(DOCC, a->hi, DLT_HD_DISPATCH(a->hd, DLT_HK_DISPATCH(a->hk,
          k_attn_bwd_dkdv_cap<DROPC, HKC, HDC, DOCC><<<gk, NT, 0, st>>>(
              a->q, a->k, a->v, a->dout, a->lse, a->delta_ws, maskT, a->dk, a->dv, S, nh, c_log2, scale, dscale, sq.b,
              sq.h, sq.r, sdq.b, sdq.h, sdq.r, a->cosT, a->sinT, xm, a->hi, cap_k))));
  });
  DLT_CHECK_LAUNCH();
}
