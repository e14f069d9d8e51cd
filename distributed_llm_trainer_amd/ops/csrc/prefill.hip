// Prefill over the KV cache (eval/decode.py forward_cached): T >= 1 new tokens of every batch row
// are appended at cache positions p0 .. p0 + T - 1 and attend to the cache rows 0 .. p0 + T - 1.
//
//   k_prefill_qkv_cache  QK-norm (optional), RoPE at the absolute position p0 + t, and the scatter
//                        of the packed [B*T, H + 2*KV] QKV GEMM output: q back in place, the k and v
//                        rows into the head-major caches [B, nkv, maxS, hd].
//   k_prefill_attn       flash attention of the T queries against the cache, with the window, sink
//                        and score-cap forms of the model.
//
// The training forward (attention_fwd_body.h) cannot serve this: its query index IS its key index
// (no offset p0), q / k / v share one stride set, and it carries dropout and lse.  What the two
// share is the tile machinery of attention.h: the swizzled LDS tiles, the LDS-DMA, the fragment reads
// and their counted waits, the online softmax with the deferred rescale.  The tile step itself is
// prefill_tile below: fwd_tile with P fed to the P.V product as hi + lo (see there).
//
// Design of k_prefill_attn
//  * Work item: 64 query rows of one query head, a workgroup of 2 waves x 32 rows.  The grid is
//    1-D and ranked longest first (an item's key range ends at its last position, so rank 0 is the
//    last 64-row block); short items fill the slots the long ones leave.
//  * Inside a rank the index runs K/V head fastest: j = g * (B * nkv) + bkv for query head
//    kvh * G + g.  Workgroup ids are dealt round-robin to the 8 XCDs, so when B * nkv is a multiple
//    of 8 every query head of a group, at every rank, lands on XCD bkv % 8 and the group's K/V
//    tiles go through that one L2; for other sizes the map is still a bijection and balanced.
//  * Q fragments go from the packed buffer (row stride H + 2*KV) straight to registers.  K and V
//    arrive as 64-key tiles from the cache rows (row stride hd) in double-buffered swizzled LDS
//    (glds_tile); the row bound of the copy is p0 + T, so no row past the written cache is read.
//  * The tile range is arithmetic on positions, no bound arrays: with first / last the positions of
//    the item's first / last valid query, tiles [ks, kw) straddle some row's window edge, [kw, kd)
//    are visible to every row (the unmasked tile form), [kd, nkt) hold the diagonal.
//  * Every row starts from M_DEAD (a windowed row's leading tiles can be wholly hidden); no dropout,
//    no lse.  SINK joins the denominator in the epilogue by k_attn_fwd_sink's rule; CAP is
//    the in-place tanh with c_log2 = cap * log2(e), as in attention_cap.hip.
#include "attention.h"

// Kernel arguments the tile steps read: their scalar loads, and the waits for them, are pinned to
// the kernel's start (an SMEM load in flight inside a tile step's counted LDS wait would let the
// wait retire the wrong fragments; see attention_cap.hip).
#define PREFILL_PIN(x) asm volatile("" : "+s"(x))

// ============================================================================ norm, rotate, scatter
// A thread holds 8 elements of a head's lower rotation half and their 8 partners (d and d + D/2),
// so the D / 16 lanes of a head are neighbours in one wave: the mean square is a butterfly over
// them (head_sum) and the rotation needs no exchange.  fp32 math on the GEMM's rounded output, one
// rounding -- k_qknorm_rope_inplace / k_rope_qk_inplace at position p0 + t, with the k and v rows
// stored to the cache instead of in place.
// F8 (prefill_kv8.hip only): kc / vc are e4m3 caches, one byte an element.  The k and v values are
// the 16-bit ones (k rounded to the activation dtype first), clamped and packed 8 + 8 to 2 x 8
// bytes (kv_fp8.h kv8_pack8); q is written back in 16 bits as ever.
template <int HK, int D, bool QKN, bool F8 = false>
__global__ __launch_bounds__(256) void k_prefill_qkv_cache(bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                           bf16_t* __restrict__ vc, const float* __restrict__ cosT,
                                                           const float* __restrict__ sinT,
                                                           const float* __restrict__ qw,
                                                           const float* __restrict__ kw, float eps, int M, int T,
                                                           int p0, int nh, int nkv, int maxS) {
  constexpr int HALF = D / 2;
  constexpr int CPR = HALF / 8;  // lanes per head
  const int heads = nh + 2 * nkv;
  const int total = M * heads * CPR;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int j = (i % CPR) * 8;
    const int r = i / CPR;
    const int hh = r % heads;
    const int m = r / heads;
    const int b = m / T, pos = p0 + (m - b * T);
    bf16_t* p = qkv + (size_t)m * (heads * D) + hh * D;
    const u16x8 a = *reinterpret_cast<const u16x8*>(p + j);
    const u16x8 c = *reinterpret_cast<const u16x8*>(p + HALF + j);
    float x1[8], x2[8];
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      x1[e] = h2f<HK>(a.v[e]);
      x2[e] = h2f<HK>(c.v[e]);
      ss += x1[e] * x1[e] + x2[e] * x2[e];
    }
    // the lanes of a head take the same branches below; the butterfly runs before any of them
    const float rstd = QKN ? rsqrtf(head_sum<CPR>(ss) * (1.f / D) + eps) : 1.f;
    if (hh >= nh + nkv) {  // v: the row as it is
#ifdef DLT_KV8_TU
      if constexpr (F8) {
        uint8_t* d8 = reinterpret_cast<uint8_t*>(vc) + (((size_t)b * nkv + (hh - nh - nkv)) * maxS + pos) * D;
        *reinterpret_cast<uint2*>(d8 + j) = kv8_pack8(x1);
        *reinterpret_cast<uint2*>(d8 + HALF + j) = kv8_pack8(x2);
        continue;
      }
#endif
      bf16_t* d = vc + (((size_t)b * nkv + (hh - nh - nkv)) * maxS + pos) * D;
      *reinterpret_cast<u16x8*>(d + j) = a;
      *reinterpret_cast<u16x8*>(d + HALF + j) = c;
      continue;
    }
    if constexpr (QKN) {
      const float* w = hh < nh ? qw : kw;
      const float4 a0 = *reinterpret_cast<const float4*>(w + j), a1 = *reinterpret_cast<const float4*>(w + j + 4);
      const float4 b0 = *reinterpret_cast<const float4*>(w + HALF + j);
      const float4 b1 = *reinterpret_cast<const float4*>(w + HALF + j + 4);
      const float w1[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const float w2[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        x1[e] = x1[e] * rstd * w1[e];
        x2[e] = x2[e] * rstd * w2[e];
      }
    }
    const float* cp = cosT + (size_t)pos * HALF + j;
    const float* sp = sinT + (size_t)pos * HALF + j;
    const float4 c0 = *reinterpret_cast<const float4*>(cp), c1 = *reinterpret_cast<const float4*>(cp + 4);
    const float4 s0 = *reinterpret_cast<const float4*>(sp), s1 = *reinterpret_cast<const float4*>(sp + 4);
    const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    u16x8 o1, o2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o1.v[e] = f2h<HK>(x1[e] * cc[e] - x2[e] * sn[e]);
      o2.v[e] = f2h<HK>(x2[e] * cc[e] + x1[e] * sn[e]);
    }
#ifdef DLT_KV8_TU
    if constexpr (F8) {
      if (hh >= nh) {
        float y1[8], y2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          y1[e] = h2f<HK>(o1.v[e]);
          y2[e] = h2f<HK>(o2.v[e]);
        }
        uint8_t* d8 = reinterpret_cast<uint8_t*>(kc) + (((size_t)b * nkv + (hh - nh)) * maxS + pos) * D;
        *reinterpret_cast<uint2*>(d8 + j) = kv8_pack8(y1);
        *reinterpret_cast<uint2*>(d8 + HALF + j) = kv8_pack8(y2);
        continue;
      }
    }
#endif
    bf16_t* d = hh < nh ? p : kc + (((size_t)b * nkv + (hh - nh)) * maxS + pos) * D;
    *reinterpret_cast<u16x8*>(d + j) = o1;
    *reinterpret_cast<u16x8*>(d + HALF + j) = o2;
  }
}

// DLT_KV8_TU: this file as included by prefill_kv8.hip, which sees k_prefill_qkv_cache (for its F8
// form) and the argument checks, and neither the attention kernel nor an entry point.
#ifndef DLT_KV8_TU
// ============================================================================ attention
// Eight fp32 values as a 16-bit MFMA operand (round to nearest even), and back.
template <int HK>
__device__ __forceinline__ bf16x8_t frag16(const floatx8_t& f) {
  if constexpr (HK == 0) return __builtin_convertvector(f, bf16x8_t);
  else return __builtin_bit_cast(bf16x8_t, __builtin_convertvector(f, f16x8_t));
}
template <int HK>
__device__ __forceinline__ floatx8_t frag32(const bf16x8_t& v) {
  if constexpr (HK == 0) return __builtin_convertvector(v, floatx8_t);
  else return __builtin_convertvector(__builtin_bit_cast(f16x8_t, v), floatx8_t);
}

// One 64-key tile as one online-softmax step: fwd_tile (attention.h) without dropout, the same
// reads, waits, cap, masks and deferred rescale, with ONE difference.  The training forward feeds P
// to the P.V product rounded to 16 bits (8 or 11 significant bits); its backward rebuilds the same
// P, so that is self-consistent there.  Prefill has no backward but has a peer: the decode kernels
// and the dense route keep P in fp32, and the cache rows of the next layer are compared with
// theirs.  Here P goes in as hi + lo, hi = round16(p) and lo = round16(p - hi) (the difference is
// exact in fp32), two MFMAs per V fragment: 16 (bf16) or 22 (fp16) significant bits of P for half
// as many MFMAs again in the tile, and o differs from the fp32-P result by fp32 summation order.
template <bool MASK, int HK, int D, bool WIN, bool CAP>
__device__ __forceinline__ void prefill_tile(FwdState<D>& fs, const bf16_t* Kt, const bf16_t* Vt,
                                             const bf16x8_t (&qf)[D / 16], int k0, int qa, int S, int lane,
                                             float c_log2, int lo, float cap_k) {
  const int h = lane >> 5, ql = lane & 31;
  constexpr int NS = D / 16;  // 16-dim contraction steps of S = K.Q^T
  floatx16_t sacc[2];
  {
    // all K fragments of the tile in flight at once, one counted wait per half
    bf16x8_t kf[2][NS];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < NS; ++s) kf[t][s] = lds_row8_asm<D>(Kt, 32 * t + ql, 16 * s + 8 * h);
    if constexpr (D == 64) {
      lgkm_wait4(kf[0][0], kf[0][1], kf[0][2], kf[0][3]);
    } else {
      lgkm_wait8(kf[0][0], kf[0][1], kf[0][2], kf[0][3]);
      pin4(kf[0][4], kf[0][5], kf[0][6], kf[0][7]);
    }
    sacc[0] = zero16();
#pragma unroll
    for (int s = 0; s < NS; ++s) sacc[0] = mfma<HK>(kf[0][s], qf[s], sacc[0]);
    tr_wait_all(kf[1]);
    sacc[1] = zero16();
#pragma unroll
    for (int s = 0; s < NS; ++s) sacc[1] = mfma<HK>(kf[1][s], qf[s], sacc[1]);
  }
  if constexpr (CAP) {  // s -> tanh(scale s / cap) in place; c_log2 is cap * log2(e)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[t][i] = cap_tanh(sacc[t][i], cap_k);
  }
  if (MASK) {  // after the cap: a hidden key is -inf, never -cap
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ka = k0 + 32 * t + acc_row(i, h);
        sacc[t][i] = (ka > qa || ka >= S || (WIN && ka < lo)) ? -INFINITY : sacc[t][i];
      }
  }
  const float mx = xhalf_max(fmaxf(max16(sacc[0]), max16(sacc[1])));
  if (!__all((mx - fs.m) * c_log2 <= RESCALE_LOG2)) {  // rare: a row's max grew by > 2^8
    const float m_new = fmaxf(fs.m, mx);
    const float alpha = fast_exp2((fs.m - m_new) * c_log2);
    fs.m = m_new;
    fs.l *= alpha;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) fs.o[dt][i] *= alpha;
  }
  const float nmc = -fs.m * c_log2;
  float l0 = 0.f, l1 = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    bf16x8_t vf[2][D / 32];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) vf[kk][dt] = tr_frag_asm<D>(Vt, 2 * t + kk, dt, lane);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float p = fast_exp2(fmaf(sacc[t][i], c_log2, nmc));
      if (i & 1) l1 += p;
      else l0 += p;
      sacc[t][i] = p;
    }
    if constexpr (D == 64) {
      tr_wait(vf[0][0], vf[0][1], vf[1][0], vf[1][1]);
    } else {
      tr_wait(vf[0][0], vf[0][1], vf[0][2], vf[0][3]);
      pin4(vf[1][0], vf[1][1], vf[1][2], vf[1][3]);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const floatx8_t pf = kk ? sacc[t].s89abcdef : sacc[t].s01234567;
      const bf16x8_t ph = frag16<HK>(pf);
      const bf16x8_t pl = frag16<HK>(pf - frag32<HK>(ph));
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) {
        fs.o[dt] = mfma<HK>(vf[kk][dt], ph, fs.o[dt]);
        fs.o[dt] = mfma<HK>(vf[kk][dt], pl, fs.o[dt]);
      }
    }
  }
  fs.l += l0 + l1;
}

template <int HK, int D, bool WIN, bool GQA, bool SINK, bool CAP>
__global__ __launch_bounds__(NT) ATTN_WAVES(D) void k_prefill_attn(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    bf16_t* __restrict__ o, const float* __restrict__ sink, int T, int p0, int nh, int nkv, int G, int maxS, int W,
    float c_log2, float cap_k) {
  PREFILL_PIN(c_log2);
  PREFILL_PIN(cap_k);
  __shared__ __attribute__((aligned(16))) bf16_t lds[2 * 2 * KVB * D];  // [buf][K|V][64][D]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, ql = lane & 31;
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;
  using UNM = std::integral_constant<bool, false>;
  using MSK = std::integral_constant<bool, true>;

  // work item: rank 0 = the last (longest) 64-row block; inside a rank K/V head fastest
  const int nqb = (T + RB - 1) / RB;
  const int BH = gridDim.x / nqb;
  const int rank = blockIdx.x / BH, j = blockIdx.x - rank * BH;
  const int qb = nqb - 1 - rank;
  int b, head, kvh;
  if constexpr (GQA) {
    const int BKV = BH / G, g = j / BKV, bkv = j - g * BKV;
    b = bkv / nkv;
    kvh = bkv - b * nkv;
    head = kvh * G + g;
  } else {
    b = j / nh;
    head = j - b * nh;
    kvh = head;
  }
  const int S = p0 + T;  // rows of the cache that are written
  const int rs = (nh + 2 * nkv) * D;
  const size_t hkv = ((size_t)b * nkv + kvh) * (size_t)maxS * D;
  const bf16_t* kh = kc + hkv;
  const bf16_t* vh = vc + hkv;

  const int row0 = qb * RB + wid * 32;  // this wave's first query row (wave-uniform)
  const int t = row0 + ql;
  const int qa = p0 + t;  // this lane's position
  bf16x8_t qf[D / 16];
  {
    const bf16_t* qrow = qkv + ((size_t)b * T + min(t, T - 1)) * rs + head * D;
#pragma unroll
    for (int s = 0; s < D / 16; ++s) qf[s] = load_row8(qrow + 16 * s + 8 * h, t < T);
  }

  FwdState<D> fs;
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) fs.o[dt] = zero16();
  fs.m = M_DEAD;
  fs.l = 0.f;

  // tile range from the positions of the item's first and last valid query
  const int first = p0 + qb * RB, last = p0 + min(T, qb * RB + RB) - 1;
  const int nkt = last / KVB + 1;      // end: the tile after the one holding `last`
  const int kd = (first + 1) / KVB;    // tiles below kd lie at or below every row's position
  int ks = 0, kw = 0, lo_q = 0, lo_w = 0;
  if constexpr (WIN) {
    ks = max(first - W + 1, 0) / KVB;                   // first tile any row needs
    kw = (max(last - W + 1, 0) + KVB - 1) / KVB;        // first tile at or above every row's lower edge
    lo_q = qa - W + 1;
    lo_w = p0 + row0 - W + 1;                           // the wave's smallest lower edge
  }

  glds_tile<D>(kh, ks * KVB, S, D, lds, wid, lane);
  glds_tile<D>(vh, ks * KVB, S, D, lds + KVB * D, wid, lane);
  tile_barrier();

  auto step = [&](auto bufc, auto maskc, int kb) {
    constexpr int BUF = decltype(bufc)::value;
    constexpr bool MASKED = decltype(maskc)::value;
    if (kb + 1 < nkt) {  // next tile straight into the other buffer (read by nobody since the last barrier)
      bf16_t* Kn = lds + (BUF ^ 1) * 2 * KVB * D;
      glds_tile<D>(kh, (kb + 1) * KVB, S, D, Kn, wid, lane);
      glds_tile<D>(vh, (kb + 1) * KVB, S, D, Kn + KVB * D, wid, lane);
    }
    const bf16_t* Kt = lds + BUF * 2 * KVB * D;
    const bf16_t* Vt = Kt + KVB * D;
    const int k0 = kb * KVB;
    if constexpr (!MASKED) {
      prefill_tile<false, HK, D, false, CAP>(fs, Kt, Vt, qf, k0, qa, S, lane, c_log2, 0, cap_k);
    } else {
      // not wholly above this wave's last row, nor wholly below its window
      if (k0 <= p0 + row0 + 31 && (!WIN || k0 + KVB > lo_w))
        prefill_tile<true, HK, D, WIN, CAP>(fs, Kt, Vt, qf, k0, qa, S, lane, c_log2, lo_q, cap_k);
    }
    tile_barrier();
  };
  // Tile kb sits in buffer (kb - ks) & 1; one body per (buffer, kind), picked by two
  // wave-uniform scalar branches per tile.
  for (int kb = ks; kb < nkt; ++kb) {
    const bool msk = kb < kw || kb >= kd;
    if ((kb - ks) & 1) {
      if (msk) step(B1{}, MSK{}, kb);
      else step(B1{}, UNM{}, kb);
    } else {
      if (msk) step(B0{}, MSK{}, kb);
      else step(B0{}, UNM{}, kb);
    }
  }

  float l_tot = xhalf_sum(fs.l);
  float inv_l;
  if constexpr (SINK) {
    // k_attn_fwd_sink's rule: fs.m is deferred and the sink can lie far above every score, so the
    // max is retaken in log2 units, m' = max(m, sink), l is rescaled by alpha = exp2(m - m')
    // before exp2(sink - m') is added, and o takes alpha through its normaliser.  sink = -inf:
    // alpha = 1 and the added term is 0 -- the plain form's bits.
    const float m2 = fs.m * c_log2, s2 = sink[head] * LOG2E;
    const float mn = fmaxf(m2, s2);
    const float alpha = fast_exp2(m2 - mn);
    l_tot = l_tot * alpha + fast_exp2(s2 - mn);
    inv_l = alpha / l_tot;
  } else {
    inv_l = 1.f / l_tot;
  }
  if (t < T) {
    bf16_t* orow = o + (((size_t)b * T + t) * nh + head) * D;
    uint2 w[D / 32][4];
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        u16x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v.v[e] = f2h<HK>(fs.o[dt][4 * g + e] * inv_l);
        w[dt][g] = __builtin_bit_cast(uint2, v);
      }
    store_row16<D>(orow, w, h);
  }
}

#endif  // DLT_KV8_TU
// ============================================================================ C entry points
// Return codes of the two entry points: 0 = launched; a positive value is the hipError_t of the
// launch; a negative one names the argument check that failed, and nothing was launched:
//   -1 hd not 64 / 128            -2 nh, nkv < 1 or nkv does not divide nh
//   -3 B < 1, T < 1, p0 < 0 or p0 + T > maxS
//   -4 W < 0 (0 = no window)      -5 a pointer is null or not 16-byte aligned
//   -6 an index would overflow (32-bit: a head's cache rows, the packed buffer, the grid)
//   -7 hk not 0 / 1, or softcap negative or not finite (0 = no cap)
static inline bool al16(const void* p) { return p && !((uintptr_t)p & 15); }
static inline int prefill_check(const void* qkv, const void* kc, const void* vc, int B, int T, int p0, int nh, int nkv,
                                int hd, int maxS, int hk) {
  if (!attn_hd_ok(hd)) return -1;
  if (nh < 1 || nkv < 1 || nh % nkv) return -2;
  if (B < 1 || T < 1 || p0 < 0 || maxS < 1 || (long)p0 + T > maxS) return -3;
  if (!al16(qkv) || !al16(kc) || !al16(vc)) return -5;
  if ((long)maxS * hd * 2 >= (1L << 32) || (long)B * T * (nh + 2 * nkv) * hd >= (1L << 31)) return -6;
  if (hk != 0 && hk != 1) return -7;
  return 0;
}

#ifndef DLT_KV8_TU
// qkv [B*T, (nh + 2 nkv) * hd] (q | k | v), kc / vc [B, nkv, maxS, hd], cosT / sinT fp32
// [>= p0 + T, hd / 2]; qw, kw: fp32 [hd], both (QK-norm) or neither
DLT_API int dlt_prefill_qkv_cache(bf16_t* qkv, bf16_t* kc, bf16_t* vc, const float* cosT, const float* sinT,
                                  const float* qw, const float* kw, float eps, int B, int T, int p0, int nh, int nkv,
                                  int hd, int maxS, int hk, hipStream_t st) {
  if (const int rc = prefill_check(qkv, kc, vc, B, T, p0, nh, nkv, hd, maxS, hk)) return rc;
  if (!al16(cosT) || !al16(sinT) || (qw != nullptr) != (kw != nullptr) || (qw && (!al16(qw) || !al16(kw)))) return -5;
  const int M = B * T;
  const size_t total = (size_t)M * (nh + 2 * nkv) * (hd / 16);
  const int blocks = (int)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
  DLT_BOOL_DISPATCH(QKNC, qw, DLT_HD_DISPATCH(hd, DLT_HK_DISPATCH(hk,
      k_prefill_qkv_cache<HKC, HDC, QKNC><<<blocks, 256, 0, st>>>(qkv, kc, vc, cosT, sinT, qw, kw, eps, M, T, p0, nh,
                                                                  nkv, maxS))));
  DLT_CHECK_LAUNCH();
}

// q: the packed buffer k_prefill_qkv_cache left (its q columns); o [B*T, nh * hd]; sink fp32 [nh]
// or null; W = 0: no window, W >= p0 + T is none either; softcap = 0: no cap
DLT_API int dlt_prefill_attn(const bf16_t* qkv, const bf16_t* kc, const bf16_t* vc, bf16_t* o, const float* sink,
                             int B, int T, int p0, int nh, int nkv, int hd, int maxS, int W, float scale,
                             float softcap, int hk, hipStream_t st) {
  if (const int rc = prefill_check(qkv, kc, vc, B, T, p0, nh, nkv, hd, maxS, hk)) return rc;
  if (W < 0) return -4;
  if (!al16(o) || (sink && ((uintptr_t)sink & 3))) return -5;
  if (!(softcap >= 0.f) || softcap > 3.0e38f) return -7;
  const int nqb = (T + RB - 1) / RB;
  if ((long)nqb * B * nh >= (1L << 31)) return -6;
  if (W >= p0 + T) W = 0;
  const int G = nh / nkv;
  const dim3 grid(nqb * B * nh);
  // CAP: the accumulator holds t = tanh(scale s / cap): exp2 units per unit of t, and cap_tanh's factor
  const float c_log2 = (softcap > 0.f ? softcap : scale) * LOG2E;
  const float cap_k = softcap > 0.f ? 2.f * LOG2E * scale / softcap : 0.f;
  DLT_BOOL_DISPATCH(WINC, W, DLT_BOOL_DISPATCH(GQAC, G > 1, DLT_BOOL_DISPATCH(SINKC, sink,
      DLT_BOOL_DISPATCH(CAPC, softcap > 0.f, DLT_HD_DISPATCH(hd, DLT_HK_DISPATCH(hk,
          k_prefill_attn<HKC, HDC, WINC, GQAC, SINKC, CAPC><<<grid, NT, 0, st>>>(
              qkv, kc, vc, o, sink, T, p0, nh, nkv, G, maxS, W, c_log2, cap_k)))))));
  DLT_CHECK_LAUNCH();
}
#endif  // DLT_KV8_TU
