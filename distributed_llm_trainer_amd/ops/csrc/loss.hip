// Cross-entropy over the (padded) vocabulary with the gradient written in place.
//
// Reference: F.cross_entropy on shifted [B*(S-1), V] logits, fp32 under autocast
// (gpt.py:449-453; SURVEY §2.5 K11/K12: the fp32 log_softmax alone is 1.65 GB for
// small at B=8).  Here the bf16 logits buffer [M, Vp] from the lm_head GEMM is
// overwritten by
//   dlogits = (softmax(l) - onehot(target)) / n_valid       (0 for padded columns
// and for rows whose target is ignore_index), so no fp32 logits or separate
// softmax-backward kernel ever exist.
//
// k_ce_row: one block per row holds the whole row in registers, so HBM sees exactly
// one read and one write of the logits (the memory-bound minimum).  Default for
// Vp <= 57344: 1024 threads x 7 16-byte chunks, held to 64 VGPRs (8 waves per SIMD,
// two rows per CU in flight): 320 us vs 346 us per 8192 x 50304 call for 512 threads
// x 13 chunks (94 VGPRs, five waves per SIMD), bench step -0.1 to -0.2 ms
// (round-2 harness ab_ce.sh, in git history; DLT_CE_THREADS=512 selects the older shape).  Rows too long for
// registers fall back to k_ce_fwd_bwd (online max/sum pass + gradient pass).
//
// Z forms (ZL = true; launched with a coefficient and z_rows): the auxiliary z-loss
// c * lse^2 of the row.  Its gradient is 2 c lse * softmax, so the row's softmax factor
// becomes zf = 1 + 2 c lse (one fma per row; it may be negative, and is used as it is) and
// the target element (p * zf - 1).  loss_rows keeps the cross-entropy part alone and z_rows
// receives lse^2 (0 on ignored rows); the caller forms c * sum(z_rows) / n_valid.  ZL is
// compile-time: the plain forms never read the two extra arguments and keep the vector
// code, registers, LDS and scratch they had before the Z forms existed (profiles/z_loss.md).
//
// CAP forms (CAP = true; launched with a final-logit soft cap): the row's logits are
// c = cap * tanh(x / cap) of the stored 16-bit x, formed in fp32 per element and never stored.
// With a = exp2(-|x| * k2), k2 = 2 log2(e) / cap, and r = rcp(1 + a):
//   tanh(x / cap) = copysign((1 - a) * r, x)      1 - tanh^2 = 4 a r^2
// a lies in [0, 1], so nothing overflows: a huge |x| / cap underflows a to 0, which gives tanh = +-1
// and a derivative of exactly 0; the derivative is a product, never 1 - t * t.  tanh is monotone,
// so the max pass runs on the raw values and the maximum is capped once.  The sum pass costs an
// exp2 and a rcp more per element, the gradient pass the same plus the derivative's products.
// loss_rows is lse(c) - c_t, z_rows lse(c)^2, and the in-place gradient
// grad_scale * (p zf - [j == t]) * (1 - tanh^2) / n_valid with p = softmax(c).  CAP is compile-time
// like ZL: the other forms never read the cap (profiles/logit_softcap.md).
#include "common.h"
#include <cstdlib>

template <int HK = 0, bool ZL = false, bool CAP = false>
__global__ __launch_bounds__(256) void k_ce_fwd_bwd(bf16_t* __restrict__ logits, const int64_t* __restrict__ targets,
                                                    const int64_t* __restrict__ n_valid, float* __restrict__ loss_rows,
                                                    int M, int Vp, int V, float gscale, float zcoef,
                                                    float* __restrict__ z_rows, float cap) {
  __shared__ float sm_m[4], sm_s[4];
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  bf16_t* lrow = logits + (size_t)row * Vp;
  const int64_t tgt = targets[row];
  DLT_DASSERT(tgt == -100 || (tgt >= 0 && tgt < V));  // ignore_index or a real token
  const bool valid = tgt >= 0 && tgt < V;
  const int nchunk = Vp >> 3;
  const float k2 = CAP ? 2.88539008177792681472f / cap : 0.f;  // 2 log2(e) / cap
  // the logit of the softmax: the stored value, or its capped form
  auto lg = [&](uint16_t h) -> float {
    const float x = h2f<HK>(h);
    if constexpr (CAP) {
      float a, r;
      return cap * dlt_cap_tanh(x, k2, a, r);
    } else {
      return x;
    }
  };
  // pass 1: online max / sum-exp
  float mx = -INFINITY, sm = 0.f;
  for (int c = tid; c < nchunk; c += 256) {
    const u16x8 x = *reinterpret_cast<const u16x8*>(lrow + c * 8);
    float v[8];
    float lm = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] = (c * 8 + e < V) ? lg(x.v[e]) : -INFINITY;
      lm = fmaxf(lm, v[e]);
    }
    if (lm > mx) { sm *= __expf(mx - lm); mx = lm; }
    if (mx != -INFINITY) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sm += __expf(v[e] - mx);
    }
  }
  // wave reduce (max, sum) pairs
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sm, o, 64);
    const float nm = fmaxf(mx, om);
    sm = (mx == -INFINITY ? 0.f : sm * __expf(mx - nm)) + (om == -INFINITY ? 0.f : os * __expf(om - nm));
    mx = nm;
  }
  if (lane == 0) { sm_m[wid] = mx; sm_s[wid] = sm; }
  __syncthreads();
  float gm = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
  float gs = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) gs += (sm_m[w] == -INFINITY) ? 0.f : sm_s[w] * __expf(sm_m[w] - gm);
  const float lse = gm + __logf(gs);
  if (tid == 0) loss_rows[row] = valid ? (lse - lg(lrow[tgt])) : 0.f;
  float zf = 1.f;
  if constexpr (ZL) {
    zf = fmaf(2.f * zcoef, lse, 1.f);
    if (tid == 0) z_rows[row] = valid ? lse * lse : 0.f;
  }
  __syncthreads();  // everyone has read lrow[tgt] before it is overwritten
  const int64_t nv = *n_valid;
  const float inv_n = valid ? gscale / (float)(nv > 0 ? nv : 1) : 0.f;
  const float gmul = ZL ? (valid ? inv_n * zf : 0.f) : inv_n;  // an ignored row stays +0 whatever zf is
  // pass 2: gradient in place
  for (int c = tid; c < nchunk; c += 256) {
    u16x8 x = *reinterpret_cast<const u16x8*>(lrow + c * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = c * 8 + e;
      float g = 0.f;
      if (col < V) {
        float dq = 1.f;  // CAP: a r^2, a quarter of 1 - tanh^2
        if constexpr (CAP) {
          float a, r;
          const float ts = dlt_cap_tanh(h2f<HK>(x.v[e]), k2, a, r);
          g = __expf(cap * ts - lse);
          dq = a * r * r;
        } else {
          g = __expf(h2f<HK>(x.v[e]) - lse);
        }
        if constexpr (ZL) {
          g = (col == tgt) ? (g * zf - 1.f) * inv_n : g * gmul;
        } else {
          if (col == tgt) g -= 1.f;
          g *= inv_n;
        }
        if constexpr (CAP) g *= 4.f * dq;
      }
      x.v[e] = f2h<HK>(g);
    }
    *reinterpret_cast<u16x8*>(lrow + c * 8) = x;
  }
}

// gscale: factor on the gradient only (1 for bf16; the fp16 path stores the gradient
// pre-multiplied by the loss scale so it does not underflow fp16, and the engine divides
// the scale back out where it applies dloss)
template <int CPT, int NTH = 512, bool CE_NT = false, int HK = 0, bool ZL = false, bool CAP = false>
__global__ __launch_bounds__(NTH) __attribute__((amdgpu_waves_per_eu(NTH == 1024 ? 8 : 1, 8))) void k_ce_row(bf16_t* __restrict__ logits, const int64_t* __restrict__ targets,
                                                const int64_t* __restrict__ n_valid, float* __restrict__ loss_rows,
                                                int M, int Vp, int V, float gscale, float zcoef,
                                                float* __restrict__ z_rows, float cap) {
  // Per element only: max, one exp2 for the sum, one exp2 + scale for the gradient.
  // Column bounds are tested per 8-wide chunk (only the last chunk straddles V), and
  // the target column is patched by its owning thread per chunk, not per element.
  __shared__ float red[NTH / 64];
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  bf16_t* lrow = logits + (size_t)row * Vp;
  const int64_t tgt = targets[row];
  DLT_DASSERT(tgt == -100 || (tgt >= 0 && tgt < V));  // ignore_index or a real token
  const bool valid = tgt >= 0 && tgt < V;
  const int tchunk = valid ? (int)(tgt >> 3) : -1;
  const int nchunk = Vp >> 3;
  const float L2E = 1.44269504088896340736f;
  uint4 x[CPT];  // 8 bf16 per chunk as 4 packed words
#pragma unroll
  for (int t = 0; t < CPT; ++t) {
    const int c = tid + NTH * t;
    if (c < nchunk) {
      if (CE_NT) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(lrow + c * 8);
        x[t] = make_uint4(__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1),
                          __builtin_nontemporal_load(q + 2), __builtin_nontemporal_load(q + 3));
      } else {
        x[t] = *reinterpret_cast<const uint4*>(lrow + c * 8);
      }
    }
  }
  auto el = [&](int t, int e) -> float {
    const uint32_t w = e < 2 ? (e == 0 ? x[t].x : x[t].x) : e < 4 ? x[t].y : e < 6 ? x[t].z : x[t].w;
    if constexpr (HK == 0) return __uint_as_float((e & 1) ? (w & 0xffff0000u) : (w << 16));
    else return h2f<1>((uint16_t)((e & 1) ? (w >> 16) : (w & 0xffffu)));
  };
  // Keep only the raw bf16 words live across the passes (52 VGPRs at CPT 13): the
  // empty asm makes the compiler re-convert per pass instead of holding 104 floats.
  auto pin = [&]() {
#pragma unroll
    for (int t = 0; t < CPT; ++t) {
      asm volatile("" : "+v"(x[t].x), "+v"(x[t].y), "+v"(x[t].z), "+v"(x[t].w));
    }
  };
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < CPT; ++t) {
    const int c = tid + NTH * t;
    if (c * 8 + 8 <= V) {
#pragma unroll
      for (int e = 0; e < 8; ++e) mx = fmaxf(mx, el(t, e));
    } else if (c < nchunk) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (c * 8 + e < V) mx = fmaxf(mx, el(t, e));
    }
  }
  pin();
  mx = wave_max(mx);
  if (lane == 0) red[wid] = mx;
  __syncthreads();
  float gm = red[0];
#pragma unroll
  for (int w = 1; w < NTH / 64; ++w) gm = fmaxf(gm, red[w]);
  __syncthreads();
  // CAP: the exponent of an element is tanh * (cap log2(e)) through the same fma, and the
  // maximum is the capped raw maximum (tanh is monotone)
  const float k2 = CAP ? (2.f * L2E) / cap : 0.f;
  const float cl = CAP ? cap * L2E : L2E;
  auto ex = [&](int t, int e) -> float {
    if constexpr (CAP) {
      float a, r;
      return dlt_cap_tanh(el(t, e), k2, a, r);
    } else {
      return el(t, e);
    }
  };
  if constexpr (CAP) {
    float a, r;
    gm = cap * dlt_cap_tanh(gm, k2, a, r);
  }
  const float nm2 = -gm * L2E;
  float sm = 0.f;
#pragma unroll
  for (int t = 0; t < CPT; ++t) {
    const int c = tid + NTH * t;
    if (c * 8 + 8 <= V) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sm += __builtin_amdgcn_exp2f(fmaf(ex(t, e), cl, nm2));
    } else if (c < nchunk) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (c * 8 + e < V) sm += __builtin_amdgcn_exp2f(fmaf(ex(t, e), cl, nm2));
    }
  }
  pin();
  sm = wave_sum(sm);
  if (lane == 0) red[wid] = sm;
  __syncthreads();
  float gs = 0.f;
#pragma unroll
  for (int w = 0; w < NTH / 64; ++w) gs += red[w];
  const float lse = gm + __logf(gs);
  const int64_t nv = *n_valid;
  const float inv_n = valid ? gscale / (float)(nv > 0 ? nv : 1) : 0.f;
  const float nl2 = -lse * L2E;
  // Z form: the row's softmax factor carries zf = 1 + 2 c lse; the plain form multiplies by inv_n alone
  float zf = 1.f;
  if constexpr (ZL) zf = fmaf(2.f * zcoef, lse, 1.f);
  const float gmul = ZL ? (valid ? inv_n * zf : 0.f) : inv_n;  // an ignored row stays +0 whatever zf is
  // one element of the gradient off the target: p * gmul, times 4 a r^2 = 1 - tanh^2 in the CAP form
  auto ge = [&](int t, int e) -> float {
    if constexpr (CAP) {
      float a, r;
      const float ts = dlt_cap_tanh(el(t, e), k2, a, r);
      return __builtin_amdgcn_exp2f(fmaf(ts, cl, nl2)) * (gmul * 4.f) * (a * r * r);
    } else {
      return __builtin_amdgcn_exp2f(fmaf(el(t, e), L2E, nl2)) * gmul;
    }
  };
#pragma unroll
  for (int t = 0; t < CPT; ++t) {
    const int c = tid + NTH * t;
    if (c < nchunk) {
      u16x8 o;
      if (c * 8 + 8 <= V) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o.v[e] = f2h<HK>(ge(t, e));
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          o.v[e] = f2h<HK>(c * 8 + e < V ? ge(t, e) : 0.f);
      }
      if (c == tchunk) {
        const int e = (int)(tgt & 7);
        float l = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) l = (j == e) ? el(t, j) : l;
        float dt = 1.f;  // CAP: 1 - tanh^2 at the target
        if constexpr (CAP) {
          float a, r;
          l = dlt_cap_tanh(l, k2, a, r);
          dt = 4.f * (a * r * r);
          loss_rows[row] = lse - cap * l;
        } else {
          loss_rows[row] = lse - l;
        }
        if constexpr (ZL) z_rows[row] = lse * lse;
        const float pt = __builtin_amdgcn_exp2f(fmaf(l, cl, nl2));
        float gtf = ((ZL ? pt * zf : pt) - 1.f) * inv_n;
        if constexpr (CAP) gtf *= dt;
        const uint16_t gt = f2h<HK>(gtf);
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = (j == e) ? gt : o.v[j];
      }
      if (CE_NT) {
        const uint4 w = __builtin_bit_cast(uint4, o);
        uint32_t* q = reinterpret_cast<uint32_t*>(lrow + c * 8);
        __builtin_nontemporal_store(w.x, q);
        __builtin_nontemporal_store(w.y, q + 1);
        __builtin_nontemporal_store(w.z, q + 2);
        __builtin_nontemporal_store(w.w, q + 3);
      } else {
        *reinterpret_cast<u16x8*>(lrow + c * 8) = o;
      }
    }
  }
  if (!valid && tid == 0) {
    loss_rows[row] = 0.f;
    if constexpr (ZL) z_rows[row] = 0.f;
  }
}

// One launch choice for every form, so a shape takes the same variant with and without the z-loss or the cap.
template <int HK, bool ZL, bool CAP = false>
static void ce_launch(int wide, int nt, int cpt, hipStream_t st, bf16_t* logits, const int64_t* targets,
                      const int64_t* n_valid, float* loss_rows, int M, int Vp, int V, float gscale, float zcoef,
                      float* z_rows, float cap = 0.f) {
#define CE_ARGS logits, targets, n_valid, loss_rows, M, Vp, V, gscale, zcoef, z_rows, cap
#define CE_ROW(CPT, NTH, NT) k_ce_row<CPT, NTH, NT, HK, ZL, CAP><<<M, NTH, 0, st>>>(CE_ARGS)
  if (wide && (Vp / 8 + 1023) / 1024 <= 7) {  // 1024 threads x 7 chunks (Vp <= 57344)
    if (nt) CE_ROW(7, 1024, true);
    else CE_ROW(7, 1024, false);
    return;
  }
  if (cpt <= 1) CE_ROW(1, 512, false);
  else if (cpt <= 2) CE_ROW(2, 512, false);
  else if (cpt <= 4) CE_ROW(4, 512, false);
  else if (cpt <= 8) CE_ROW(8, 512, false);
  else if (cpt <= 13) CE_ROW(13, 512, false);
  else if (cpt <= 16) CE_ROW(16, 512, false);
  else k_ce_fwd_bwd<HK, ZL, CAP><<<M, 256, 0, st>>>(CE_ARGS);
#undef CE_ROW
#undef CE_ARGS
}

// The launch variant of a call: the two statics are read once per process and shared by both entry points.
static void ce_choice(int Vp, int* wide_out, int* nt_out, int* cpt_out) {
  *cpt_out = (Vp / 8 + 511) / 512;
  static int wide = -1;
  if (wide < 0) {
    const char* e = getenv("DLT_CE_THREADS");
    wide = (e && atoi(e) == 512) ? 0 : 1;
  }
  // nontemporal logits loads / gradient stores (the [M, Vp] buffer is far larger than
  // the Infinity Cache): 305 vs 319 us per 8192-row call, step -0.06 / -0.14 ms in two
  // same-box pairs; DLT_CE_NT=0 selects plain accesses
  static int nt = -1;
  if (nt < 0) {
    const char* e = getenv("DLT_CE_NT");
    nt = (e && atoi(e) == 0) ? 0 : 1;
  }
  *wide_out = wide;
  *nt_out = nt;
}

// hk: logits format (0 bf16, 1 fp16); gscale multiplies the in-place gradient
DLT_API int dlt_cross_entropy_fwd_bwd(bf16_t* logits, const int64_t* targets, const int64_t* n_valid,
                                      float* loss_rows, int M, int Vp, int V, float gscale, int hk, hipStream_t st) {
  if (Vp % 8 || V > Vp) return -1;
  int wide, nt, cpt;
  ce_choice(Vp, &wide, &nt, &cpt);
  DLT_HK_DISPATCH(hk, (ce_launch<HKC, false>(wide, nt, cpt, st, logits, targets, n_valid, loss_rows, M, Vp, V, gscale,
                                             0.f, nullptr)));
  DLT_CHECK_LAUNCH();
}

// The Z form: as above plus the z-loss coefficient (its gradient joins the in-place gradient)
// and z_rows [M] fp32, which receives lse^2 per row (0 on ignored rows).
DLT_API int dlt_cross_entropy_z_fwd_bwd(bf16_t* logits, const int64_t* targets, const int64_t* n_valid,
                                        float* loss_rows, int M, int Vp, int V, float gscale, int hk, float zcoef,
                                        float* z_rows, hipStream_t st) {
  if (Vp % 8 || V > Vp || !z_rows) return -1;
  int wide, nt, cpt;
  ce_choice(Vp, &wide, &nt, &cpt);
  DLT_HK_DISPATCH(hk, (ce_launch<HKC, true>(wide, nt, cpt, st, logits, targets, n_valid, loss_rows, M, Vp, V, gscale,
                                            zcoef, z_rows)));
  DLT_CHECK_LAUNCH();
}

// The CAP form: the softmax runs over cap * tanh(logits / cap) (cap finite and > 0), with the z-loss
// when zcoef != 0 (z_rows is then required; it may be null without a coefficient).
DLT_API int dlt_cross_entropy_cap_fwd_bwd(bf16_t* logits, const int64_t* targets, const int64_t* n_valid,
                                          float* loss_rows, int M, int Vp, int V, float gscale, int hk, float zcoef,
                                          float* z_rows, float cap, hipStream_t st) {
  if (Vp % 8 || V > Vp || !(cap > 0.f) || cap > 3.0e38f || (zcoef != 0.f && !z_rows)) return -1;
  int wide, nt, cpt;
  ce_choice(Vp, &wide, &nt, &cpt);
  if (z_rows) {
    DLT_HK_DISPATCH(hk, (ce_launch<HKC, true, true>(wide, nt, cpt, st, logits, targets, n_valid, loss_rows, M, Vp, V,
                                                    gscale, zcoef, z_rows, cap)));
  } else {
    DLT_HK_DISPATCH(hk, (ce_launch<HKC, false, true>(wide, nt, cpt, st, logits, targets, n_valid, loss_rows, M, Vp, V,
                                                     gscale, 0.f, nullptr, cap)));
  }
  DLT_CHECK_LAUNCH();
}
