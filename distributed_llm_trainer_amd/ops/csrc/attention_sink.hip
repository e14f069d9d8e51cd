// The SINK forms of the flash-attention forward (attention sinks, GPTConfig.attention_sinks):
// one more logit per query head in the softmax denominator, with no value row.
//
// The kernel is attention_fwd_body.h with SINK = true -- k_attn_fwd's tile loop unchanged, the
// sink folded into the row sum, the normaliser and lse in the epilogue -- for
// every DROP / HK / D / DOC / GQA combination of the plain forward.  It is a translation unit
// of its own: co-compiled instantiations of one template perturb each other's register
// allocation, and attention.hip's kernels must compile to what they were.  The backward needs
// no new MFMA kernel (dQ and dK/dV rebuild P from the stored lse); the sink gradient is
// k_attn_sink_bwd in attention.hip.
#include "attention.h"

template <bool DROP, int HK, int D, bool DOC, bool GQA>
__global__ __launch_bounds__(NT) ATTN_WAVES(D) void k_attn_fwd_sink(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, bf16_t* __restrict__ o,
    float* __restrict__ lse, const uint32_t* __restrict__ mask, int S, int nh, float c_log2, float dscale, long in_bs,
    int in_hs, int in_rs, int xcd_map, const int* __restrict__ dlo, int G, long kv_bs, int kv_hs, int kv_rs,
    const float* __restrict__ sink) {
  // the fragment reads this kernel's parameters and template arguments by name (its header
  // lists them): they are k_attn_fwd's, in its order, plus `sink`
  constexpr bool SINK = true;
  constexpr bool CAP = false;
  constexpr float cap_k = 0.f;
#include "attention_fwd_body.h"
}

// a: checked by dlt_attn_fwd (head_dim, strides, nkv, the keep-bit buffer), keep bits written
int attn_fwd_sink_launch(const dlt_attn_args* a, hipStream_t st) {
  const int nh = a->nh, nkv = a->nkv, S = a->S;
  if (!a->sink || !attn_hd_ok(a->hd) || S <= 0 || nkv < 0 || (nkv && nh % nkv)) return -1;
  const dlt_attn_stride sq = a->stride.q, skv = nkv ? a->stride.kv : dlt_attn_stride{0, 0, 0};
  const int G = nkv ? nh / nkv : 1;
  const int nrb = (S + RB - 1) / RB;
  const int xm = xcd_map_enabled();
  const dim3 grid(attn_grid(nrb, a->B * nh, xm));  // work items, see work_item()
  const float c_log2 = a->scale * LOG2E;
  DLT_BOOL_DISPATCH(DROPC, a->thr, DLT_BOOL_DISPATCH(GQAC, nkv, DLT_BOOL_DISPATCH(DOCC, a->lo,
      DLT_HD_DISPATCH(a->hd, DLT_HK_DISPATCH(a->hk, k_attn_fwd_sink<DROPC, HKC, HDC, DOCC, GQAC><<<grid, NT, 0, st>>>(
          a->q, a->k, a->v, a->o, a->lse, DROPC ? a->mask : nullptr, S, nh, c_log2, a->dscale, sq.b, sq.h, sq.r, xm,
          a->lo, G, skv.b, skv.h, skv.r, a->sink))))));
  DLT_CHECK_LAUNCH();
}
