// The backward of the flash-attention kernels, shared by attention.hip (the plain forms) and
// attention_cap.hip (the CAP forms, attention-score soft-capping), the way attention_fwd_body.h
// shares the forward.  One file, four sections picked by DLT_ATTN_BWD_SECTION:
//   0  the tile functions (store_head_row, dkdv_subtile, dq_tile), at file scope, once
//   1  the body of k_attn_bwd_dkdv      -- textual fragments, included INSIDE the kernel
//   2  the body of k_attn_bwd_dkdv_gqa     definitions (see attention_fwd_body.h for why they
//   3  the body of k_attn_bwd_dq           are not __device__ functions)
// The fragments read their kernel's parameters and template arguments by name, and expect
//   constexpr bool CAP;  float cap_k;   // cap_k = 2 log2(e) scale / cap, read only when CAP
// in scope.  CAP false is the code as it was; CAP true turns every score accumulator into
// t = tanh(scale q.k / cap) in place (c_log2 is then cap * log2(e)) and carries 1 - t^2 into dS.
#if DLT_ATTN_BWD_SECTION == 0
#ifndef DLT_ATTENTION_BWD_FUNCS
#define DLT_ATTENTION_BWD_FUNCS

// Store one head row held in accumulators (element 4g+e of acc[dt] is dim
// 32*dt + 8*g + 4*h + e) times `sc`.  With RoPE tables the inverse NeoX rotation of
// position `pos` is applied first: the partner of dim j < 32 is j + 32, i.e. the same
// register of the other dt -- the rotation needs no data exchange.  (Replaces the
// separate repack kernel that read dq/dk back and wrote the packed [M, 3H] gradient.)
template <int HK, int D>
__device__ __forceinline__ void store_head_row(bf16_t* __restrict__ dst, const floatx16_t (&a)[D / 32], float sc, int h,
                                               const float* __restrict__ cosT, const float* __restrict__ sinT,
                                               int pos) {
  // dims of a[dt] element 4g + e: 32 dt + 8 g + 4 h + e; the RoPE partner of dim j < D/2
  // is j + D/2, register 4g + e of a[dt + D/64]
  constexpr int HP = D / 64;
  uint2 w[D / 32][4];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int dt = 0; dt < HP; ++dt) {
      u16x4 w0, w1;
      if (cosT) {
        const int ti = pos * (D / 2) + 32 * dt + 8 * g + 4 * h;
        const float4 c4 = *reinterpret_cast<const float4*>(cosT + ti);
        const float4 s4 = *reinterpret_cast<const float4*>(sinT + ti);
        const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x1 = a[dt][4 * g + e] * sc, x2 = a[dt + HP][4 * g + e] * sc;
          w0.v[e] = f2h<HK>(fmaf(x1, cc[e], x2 * ss[e]));
          w1.v[e] = f2h<HK>(fmaf(x2, cc[e], -x1 * ss[e]));
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          w0.v[e] = f2h<HK>(a[dt][4 * g + e] * sc);
          w1.v[e] = f2h<HK>(a[dt + HP][4 * g + e] * sc);
        }
      }
      w[dt][g] = __builtin_bit_cast(uint2, w0);
      w[dt + HP][g] = __builtin_bit_cast(uint2, w1);
    }
  store_row16<D>(dst, w, h);
}

// Per-wave timestamps for tools/cpp/attn_timing.cpp (only with -DDLT_ATTN_TIMING):
// [workgroup][wave][8] shader-clock stamps written by lane 0 with vector stores.
#ifdef DLT_ATTN_TIMING
extern __device__ unsigned long long* g_attn_tim;  // defined in attention.hip
#define ATTN_STAMP(slot)                                                                           \
  do {                                                                                             \
    const unsigned long long _t = __builtin_amdgcn_s_memtime();                                   \
    if (lane == 0) g_attn_tim[((size_t)blockIdx.x * 2 + wid) * 8 + (slot)] = _t;                   \
  } while (0)
#else
#define ATTN_STAMP(slot) ((void)0)
#endif

// ---------------------------------------------------------------- dK / dV
// One workgroup per 128 keys (32 per wave); sweep query tiles of 64 (two 32-row
// sub-tiles).  Accumulators: S and dP with queries in registers, keys on lanes.
template <bool MASK, bool DROP, int HK, int D, bool DOC = false, bool CAP = false>
__device__ __forceinline__ void dkdv_subtile(floatx16_t (&dka)[D / 32], floatx16_t (&dva)[D / 32], const bf16_t* Qt,
                                             const bf16_t* Dt, const float* rl, const float* rd,
                                             uint32_t mw, const bf16x8_t (&kf)[D / 16], const bf16x8_t (&vf)[D / 16],
                                             int qs, int ka, int S, int lane, float c_log2, float dscale,
                                             int hi = 0, float cap_k = 0.f) {
  const int h = lane >> 5, kl = lane & 31;
  floatx16_t sacc = zero16(), pacc = zero16();
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    sacc = mfma<HK>(lds_row8<D>(Qt, kl, 16 * s + 8 * h), kf[s], sacc);
    pacc = mfma<HK>(lds_row8<D>(Dt, kl, 16 * s + 8 * h), vf[s], pacc);
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 l4 = *reinterpret_cast<const float4*>(rl + 8 * g + 4 * h);
    const float4 d4 = *reinterpret_cast<const float4*>(rd + 8 * g + 4 * h);
    const float lv[4] = {l4.x, l4.y, l4.z, l4.w};
    const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * g + e;
      const int r = 8 * g + 4 * h + e;  // query row within the sub-tile
      float p, dt2 = 0.f;  // CAP: the score becomes t = tanh(x / cap); dt2 = 1 - t^2 goes into dS
      if constexpr (CAP) p = fast_exp2(fmaf(cap_tanh(sacc[i], cap_k, dt2), c_log2, -lv[e]));
      else p = fast_exp2(fmaf(sacc[i], c_log2, -lv[e]));
      if (MASK) {
        const int qa = qs + r;
        p = (ka > qa || qa >= S || ka >= S || (DOC && qa > hi)) ? 0.f : p;
      }
      const float dp = pacc[i];
      if (DROP) {
        // dS = P o (s M o dP - Delta) = s (Pd o dP - P Delta / s) with Pd = M o P: the
        // dropped P that dV needs anyway, so the mask is applied once (4 VALU per
        // element instead of 5); rd holds Delta / s and s = 1/(1-p) is folded into the
        // dK and dV epilogues
        const uint32_t ones = keep_ones(mw, 8 * g + e);  // maskT word >> 4h: query qs + r
        const float pd = keep_and(p, ones);
        sacc[i] = pd;                          // dropped P -> dV
        pacc[i] = fmaf(pd, dp, -(p * dv[e]));  // dS / s   -> dK
      } else {
        sacc[i] = p;
        pacc[i] = p * (dp - dv[e]);
      }
      if constexpr (CAP) pacc[i] *= dt2;  // dx = dS (1 - t^2)
    }
    // CAP: four elements' exp2 / rcp chains at a time (all sixteen interleaved spilled at head_dim 64
    // without dropout; the dropout forms fit as they are and spill with the barrier)
    if constexpr (CAP && !DROP && D == 64) __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x8_t pb = acc_frag<HK>(sacc, s);
    const bf16x8_t sb = acc_frag<HK>(pacc, s);
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) {
      dva[dt] = mfma<HK>(tr_frag<D>(Dt, s, dt, lane), pb, dva[dt]);
      dka[dt] = mfma<HK>(tr_frag<D>(Qt, s, dt, lane), sb, dka[dt]);
    }
  }
}

// ---------------------------------------------------------------------- dQ
template <bool MASK, bool DROP, int HK, int D, bool DOC = false, bool CAP = false>
__device__ __forceinline__ void dq_tile(floatx16_t (&dqa)[D / 32], const bf16_t* Kt, const bf16_t* Vt,
                                        const bf16x8_t (&qf)[D / 16], const bf16x8_t (&df)[D / 16], int k0, int qa,
                                        int S, int lane, float c_log2, float nl2, float dl, float dscale, uint2 mw,
                                        int lo = 0, float cap_k = 0.f) {
  constexpr int NS = D / 16;
  const int h = lane >> 5, ql = lane & 31;
  floatx16_t sacc[2], pacc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    sacc[t] = zero16();
    pacc[t] = zero16();
#if DLT_ATTN_KREAD_ASM
    // the half-tile's K and V fragments in flight at once, one counted wait each
    bf16x8_t kf[NS], vf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) kf[s] = lds_row8_asm<D>(Kt, 32 * t + ql, 16 * s + 8 * h);
#pragma unroll
    for (int s = 0; s < NS; ++s) vf[s] = lds_row8_asm<D>(Vt, 32 * t + ql, 16 * s + 8 * h);
    if constexpr (D == 64) {
      lgkm_wait4(kf[0], kf[1], kf[2], kf[3]);
    } else {
      lgkm_wait8(kf[0], kf[1], kf[2], kf[3]);
      pin4(kf[4], kf[5], kf[6], kf[7]);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) sacc[t] = mfma<HK>(kf[s], qf[s], sacc[t]);
    tr_wait_all(vf);
#pragma unroll
    for (int s = 0; s < NS; ++s) pacc[t] = mfma<HK>(vf[s], df[s], pacc[t]);
#else
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      sacc[t] = mfma<HK>(lds_row8<D>(Kt, 32 * t + ql, 16 * s + 8 * h), qf[s], sacc[t]);
      pacc[t] = mfma<HK>(lds_row8<D>(Vt, 32 * t + ql, 16 * s + 8 * h), df[s], pacc[t]);
    }
#endif
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const uint32_t word = DROP ? ((t ? mw.y : mw.x) >> (4 * h)) : 0u;  // prefetched a tile ahead
    // CAP: the softmax VALU of a half stays between the products (with the K^T fragment reads of
    // the dQ product hoisted into it, the head_dim-64 forms spilled)
    if constexpr (CAP && D == 64) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int kr = acc_row(i, h);
      float p, dt2 = 0.f;  // CAP: as in dkdv_subtile
      if constexpr (CAP) p = fast_exp2(fmaf(cap_tanh(sacc[t][i], cap_k, dt2), c_log2, nl2));
      else p = fast_exp2(fmaf(sacc[t][i], c_log2, nl2));
      if (MASK) {
        const int kA = k0 + 32 * t + kr;
        p = (kA > qa || kA >= S || (DOC && kA < lo)) ? 0.f : p;
      }
      float dp = pacc[t][i];
      if (DROP) {
        dp = keep_and(dp, keep_ones(word, (i & 3) + 8 * (i >> 2)));
        pacc[t][i] = p * fmaf(dp, dscale, -dl);
      } else {
        pacc[t][i] = p * (dp - dl);
      }
      if constexpr (CAP) pacc[t][i] *= dt2;  // dx = dS (1 - t^2)
    }
  }
  if constexpr (CAP && D == 64) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const bf16x8_t sb = acc_frag<HK>(pacc[kk >> 1], kk & 1);
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) dqa[dt] = mfma<HK>(tr_frag<D>(Kt, kk, dt, lane), sb, dqa[dt]);
  }
}
#endif  // DLT_ATTENTION_BWD_FUNCS

#elif DLT_ATTN_BWD_SECTION == 1  // ---- body of k_attn_bwd_dkdv
  // one LDS object (avoids hipcc's extra vmcnt waits with several __shared__ arrays)
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * QSTEP * D * 2 + 2 * 2 * QSTEP * 4];
  bf16_t* lds = reinterpret_cast<bf16_t*>(smem);                              // [buf][Q|dO][64][D]
  float* rowc = reinterpret_cast<float*>(smem + 2 * 2 * QSTEP * D * 2);       // [buf][lse2|delta][64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, kl = lane & 31;
  ATTN_STAMP(0);
  const int nrb = (S + RB - 1) / RB;
  int bh, pair;
  const bool lpt = work_item(nrb, xcd_map, bh, pair);
  const int b = bh / nh, head = bh % nh;
  const size_t hin = (size_t)b * in_bs + (size_t)head * in_hs;     // q / k / v
  const size_t hout = (size_t)b * out_bs + (size_t)head * out_hs;  // dk / dv
  const int rstride = nh * D;
  const int W = (S + 31) >> 5;
  const int nqt = (S + QSTEP - 1) / QSTEP;
  const bf16_t* dob = dout + ((size_t)b * S * nh + head) * D;
  const float inv_dscale = 1.f / dscale;
  using UNM = std::integral_constant<bool, false>;
  using MSK = std::integral_constant<bool, true>;

#pragma unroll 1
  for (int it = 0; it < 2; ++it) {
    const int kblk = (lpt || it == 0) ? pair : nrb - 1 - pair;  // long item (early keys) first
    if (it == 1 && (lpt || kblk <= pair)) break;                 // odd nrb: middle item once
    const int k0 = kblk * RB + wid * 32;  // wave-uniform
    const int ka = k0 + kl;
    // this lane's key column of the transposed keep-bit mask: one word per 32 queries
    const uint32_t* mcol = DROP ? maskT + (size_t)bh * W * S + min(ka, S - 1) : nullptr;  // word j at mcol[j*S]

    bf16x8_t kf[D / 16], vf[D / 16];
    const int kc = min(ka, S - 1);
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      kf[s] = load_row8(k + hin + (size_t)kc * in_rs + 16 * s + 8 * h, ka < S);
      vf[s] = load_row8(v + hin + (size_t)kc * in_rs + 16 * s + 8 * h, ka < S);
    }
    floatx16_t dka[D / 32], dva[D / 32];
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) dka[dt] = dva[dt] = zero16();

    const int qt_begin = kblk;  // the 64-query tile holding this item's diagonal
    // DOC: this lane's bound, the wave's largest (its last key's), and the item's tile
    // range: the loop ends before tile nqe, tiles from t_unm on reach past some key's bound
    int hi_k = 0, hi_w = 0, nqe_doc = 0, t_unm = 0;
    if constexpr (DOC) {
      const int* hrow = dhi + (size_t)b * S;
      hi_k = hrow[kc];
      hi_w = __builtin_amdgcn_readlane(hi_k, 31);
      doc_k_range(hrow, kblk, S, nqt, nqe_doc, t_unm);
    }
    const int nqe = DOC ? nqe_doc : nqt;
    float rl = 0.f, rd = 0.f;
    uint2 mw_cur = make_uint2(0u, 0u), mw_next = make_uint2(0u, 0u);
    auto load_rows = [&](int t, int buf) {  // Q / dO tiles by LDS-DMA, row stats via registers
      glds_tile64<D>(q + hin, t * QSTEP, S, in_rs, lds + buf * 2 * QSTEP * D, wid, lane);
      glds_tile64<D>(dob, t * QSTEP, S, rstride, lds + buf * 2 * QSTEP * D + QSTEP * D, wid, lane);
      if (DROP) {  // this lane's two 32-query keep words of tile t (consumed one tile later)
        const int w0 = (t * QSTEP) >> 5;
        mw_next = make_uint2(mcol[(size_t)w0 * S], (w0 + 1 < W) ? mcol[(size_t)(w0 + 1) * S] : 0u);
      }
      if (tid < QSTEP) {
        const int qq = min(t * QSTEP + tid, S - 1);
        const bool ok = t * QSTEP + tid < S;
        rl = ok ? lse[(size_t)bh * S + qq] * LOG2E : 0.f;
        rd = ok ? delta[(size_t)bh * S + qq] * (DROP ? inv_dscale : 1.f) : 0.f;  // Delta / s (dkdv_subtile)
      }
    };
    auto store_rows = [&](int buf) {
      if (tid < QSTEP) {
        rowc[buf * 2 * QSTEP + tid] = rl;
        rowc[buf * 2 * QSTEP + QSTEP + tid] = rd;
      }
    };
    load_rows(qt_begin, 0);
    store_rows(0);
    mw_cur = mw_next;
    __syncthreads();
    ATTN_STAMP(1);

    // Tile qt_begin holds every diagonal sub-tile of the item (masked kind, fully
    // masked sub-tiles skipped); later full tiles are straight-line unmasked; a ragged
    // last tile (S % 64) is masked again.
    auto step = [&](auto maskc, int t) {
      constexpr bool MASKED = decltype(maskc)::value;
      const int cur = (t - qt_begin) & 1;
      const bool more = t + 1 < nqe;
      const uint32_t mw0 = mw_cur.x, mw1 = mw_cur.y;
      if (more) load_rows(t + 1, cur ^ 1);
      const bf16_t* Qt = lds + cur * 2 * QSTEP * D;
      const bf16_t* Dt = Qt + QSTEP * D;
      const float* rlp = rowc + cur * 2 * QSTEP;
      const float* rdp = rlp + QSTEP;
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int qs = t * QSTEP + 32 * qt;
        const bf16_t* Qs = Qt + 32 * qt * D;
        const bf16_t* Ds = Dt + 32 * qt * D;
        const uint32_t mw = (qt ? mw1 : mw0) >> (4 * h);
        if (!MASKED)
          dkdv_subtile<false, DROP, HK, D, false, CAP>(dka, dva, Qs, Ds, rlp + 32 * qt, rdp + 32 * qt, mw, kf, vf, qs, ka, S,
                                           lane, c_log2, dscale, 0, cap_k);
        else if (qs + 31 >= k0 && (!DOC || qs <= hi_w))  // DOC: not wholly past this wave's documents
          dkdv_subtile<true, DROP, HK, D, DOC, CAP>(dka, dva, Qs, Ds, rlp + 32 * qt, rdp + 32 * qt, mw, kf, vf, qs, ka, S,
                                               lane, c_log2, dscale, hi_k, cap_k);
      }
      if (more) store_rows(cur ^ 1);
      mw_cur = mw_next;
      tile_barrier();
    };
    int t = qt_begin;
    const int t_full = DOC ? t_unm : S / QSTEP;  // DOC: the first tile past the item's smallest hi
    if (t < nqe) step(MSK{}, t++);
    ATTN_STAMP(2);
    for (; t < t_full; ++t) step(UNM{}, t);
    for (; t < nqe; ++t) step(MSK{}, t);
    ATTN_STAMP(3);

    if (ka < S) {
      store_head_row<HK, D>(dk + hout + (size_t)ka * out_rs, dka, DROP ? scale * dscale : scale, h, cosT, sinT, ka);
      store_head_row<HK, D>(dv + hout + (size_t)ka * out_rs, dva, DROP ? dscale : 1.f, h, nullptr, nullptr, 0);
    }
#ifdef DLT_ATTN_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ATTN_STAMP(4);
    if (lane == 0) g_attn_tim[((size_t)blockIdx.x * 2 + wid) * 8 + 5] = (unsigned long long)(nqt - qt_begin);
#endif
  }
#elif DLT_ATTN_BWD_SECTION == 2  // ---- body of k_attn_bwd_dkdv_gqa
  // one LDS object (avoids hipcc's extra vmcnt waits with several __shared__ arrays)
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * QSTEP * D * 2 + 2 * 2 * QSTEP * 4];
  bf16_t* lds = reinterpret_cast<bf16_t*>(smem);                              // [buf][Q|dO][64][D]
  float* rowc = reinterpret_cast<float*>(smem + 2 * 2 * QSTEP * D * 2);       // [buf][lse2|delta][64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, kl = lane & 31;
  ATTN_STAMP(0);
  const int nrb = (S + RB - 1) / RB;
  int bh, pair;
  const bool lpt = work_item(nrb, xcd_map, bh, pair);
  // `head` is the KV head and hq0 the group's first query head (g = 0); the q-side bases
  // below are those of hq0 and move on by one query head per pass
  const int nhk = nh / G;
  const int b = bh / nhk, head = bh % nhk;
  const int hq0 = head * G;
  const int bhq0 = b * nh + hq0;                                   // row of lse / delta / the keep bits
  const size_t hin = (size_t)b * in_bs + (size_t)hq0 * in_hs;      // q
  const size_t hout = (size_t)b * out_bs + (size_t)head * out_hs;  // dk / dv
  const size_t hkv = (size_t)b * kv_bs + (size_t)head * kv_hs;     // k / v
  const int krs = kv_rs;
  const int rstride = nh * D;
  const int W = (S + 31) >> 5;
  const int nqt = (S + QSTEP - 1) / QSTEP;
  const bf16_t* dob0 = dout + ((size_t)b * S * nh + hq0) * D;
  const float inv_dscale = 1.f / dscale;
  using UNM = std::integral_constant<bool, false>;
  using MSK = std::integral_constant<bool, true>;

#pragma unroll 1
  for (int it = 0; it < 2; ++it) {
    const int kblk = (lpt || it == 0) ? pair : nrb - 1 - pair;  // long item (early keys) first
    if (it == 1 && (lpt || kblk <= pair)) break;                 // odd nrb: middle item once
    const int k0 = kblk * RB + wid * 32;  // wave-uniform
    const int ka = k0 + kl;
    // this lane's key column of the transposed keep-bit mask: one word per 32 queries
    const uint32_t* mcol0 = DROP ? maskT + (size_t)bhq0 * W * S + min(ka, S - 1) : nullptr;  // word j at mcol[j*S]

    bf16x8_t kf[D / 16], vf[D / 16];
    const int kc = min(ka, S - 1);
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      kf[s] = load_row8(k + hkv + (size_t)kc * krs + 16 * s + 8 * h, ka < S);
      vf[s] = load_row8(v + hkv + (size_t)kc * krs + 16 * s + 8 * h, ka < S);
    }
    floatx16_t dka[D / 32], dva[D / 32];
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) dka[dt] = dva[dt] = zero16();

    const int qt_begin = kblk;  // the 64-query tile holding this item's diagonal
    // DOC: this lane's bound, the wave's largest (its last key's), and the item's tile
    // range: the loop ends before tile nqe, tiles from t_unm on reach past some key's bound
    int hi_k = 0, hi_w = 0, nqe_doc = 0, t_unm = 0;
    if constexpr (DOC) {
      const int* hrow = dhi + (size_t)b * S;
      hi_k = hrow[kc];
      hi_w = __builtin_amdgcn_readlane(hi_k, 31);
      doc_k_range(hrow, kblk, S, nqt, nqe_doc, t_unm);
    }
    const int nqe = DOC ? nqe_doc : nqt;
    // q-side bases of the head whose tiles are being LOADED (one tile ahead of the compute);
    // par = LDS buffer of the tile being computed
    {
      int bhq = bhq0;
      const bf16_t* qb = q + hin;
      const bf16_t* dob = dob0;
      const uint32_t* mcol = mcol0;
      int par = 0;
      float rl = 0.f, rd = 0.f;
      uint2 mw_cur = make_uint2(0u, 0u), mw_next = make_uint2(0u, 0u);
      auto load_rows = [&](int t, int buf) {  // Q / dO tiles by LDS-DMA, row stats via registers
        glds_tile64<D>(qb, t * QSTEP, S, in_rs, lds + buf * 2 * QSTEP * D, wid, lane);
        glds_tile64<D>(dob, t * QSTEP, S, rstride, lds + buf * 2 * QSTEP * D + QSTEP * D, wid, lane);
        if (DROP) {  // this lane's two 32-query keep words of tile t (consumed one tile later)
          const int w0 = (t * QSTEP) >> 5;
          mw_next = make_uint2(mcol[(size_t)w0 * S], (w0 + 1 < W) ? mcol[(size_t)(w0 + 1) * S] : 0u);
        }
        if (tid < QSTEP) {
          const int qq = min(t * QSTEP + tid, S - 1);
          const bool ok = t * QSTEP + tid < S;
          rl = ok ? lse[(size_t)bhq * S + qq] * LOG2E : 0.f;
          rd = ok ? delta[(size_t)bhq * S + qq] * (DROP ? inv_dscale : 1.f) : 0.f;  // Delta / s (dkdv_subtile)
        }
      };
      auto store_rows = [&](int buf) {
        if (tid < QSTEP) {
          rowc[buf * 2 * QSTEP + tid] = rl;
          rowc[buf * 2 * QSTEP + QSTEP + tid] = rd;
        }
      };
      load_rows(qt_begin, 0);
      store_rows(0);
      mw_cur = mw_next;
      __syncthreads();
      ATTN_STAMP(1);

      // Tile qt_begin holds every diagonal sub-tile of the item (masked kind, fully
      // masked sub-tiles skipped); later full tiles are straight-line unmasked; a ragged
      // last tile (S % 64) is masked again.
      auto step = [&](auto maskc, int t, int g) {
        constexpr bool MASKED = decltype(maskc)::value;
        const int cur = par;
        const bool wrap = t + 1 >= nqe;  // the head's last tile: the next one is the next head's first
        const bool more = !wrap || g + 1 < G;
        const uint32_t mw0 = mw_cur.x, mw1 = mw_cur.y;
        if (more) {
          if (wrap) {
            ++bhq;
            qb += in_hs;
            dob += D;
            if (DROP) mcol += (size_t)W * S;
          }
          load_rows(wrap ? qt_begin : t + 1, cur ^ 1);
        }
        const bf16_t* Qt = lds + cur * 2 * QSTEP * D;
        const bf16_t* Dt = Qt + QSTEP * D;
        const float* rlp = rowc + cur * 2 * QSTEP;
        const float* rdp = rlp + QSTEP;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          const int qs = t * QSTEP + 32 * qt;
          const bf16_t* Qs = Qt + 32 * qt * D;
          const bf16_t* Ds = Dt + 32 * qt * D;
          const uint32_t mw = (qt ? mw1 : mw0) >> (4 * h);
          if (!MASKED)
            dkdv_subtile<false, DROP, HK, D, false, CAP>(dka, dva, Qs, Ds, rlp + 32 * qt, rdp + 32 * qt, mw, kf, vf, qs, ka, S,
                                             lane, c_log2, dscale, 0, cap_k);
          else if (qs + 31 >= k0 && (!DOC || qs <= hi_w))  // DOC: not wholly past this wave's documents
            dkdv_subtile<true, DROP, HK, D, DOC, CAP>(dka, dva, Qs, Ds, rlp + 32 * qt, rdp + 32 * qt, mw, kf, vf, qs, ka, S,
                                                 lane, c_log2, dscale, hi_k, cap_k);
        }
        if (more) store_rows(cur ^ 1);
        mw_cur = mw_next;
        par ^= 1;
        tile_barrier();
      };
      const int t_full = DOC ? t_unm : S / QSTEP;  // DOC: the first tile past the item's smallest hi
#pragma unroll 1
      for (int g = 0; g < G; ++g) {
        int t = qt_begin;
        if (t < nqe) step(MSK{}, t++, g);
        for (; t < t_full; ++t) step(UNM{}, t, g);
        for (; t < nqe; ++t) step(MSK{}, t, g);
      }
      ATTN_STAMP(3);
    }

    if (ka < S) {
      store_head_row<HK, D>(dk + hout + (size_t)ka * out_rs, dka, DROP ? scale * dscale : scale, h, cosT, sinT, ka);
      store_head_row<HK, D>(dv + hout + (size_t)ka * out_rs, dva, DROP ? dscale : 1.f, h, nullptr, nullptr, 0);
    }
#ifdef DLT_ATTN_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ATTN_STAMP(4);
    if (lane == 0) g_attn_tim[((size_t)blockIdx.x * 2 + wid) * 8 + 5] = (unsigned long long)(nqt - qt_begin);
#endif
  }
#elif DLT_ATTN_BWD_SECTION == 3  // ---- body of k_attn_bwd_dq
  __shared__ __attribute__((aligned(16))) bf16_t lds[2 * 2 * KVB * D];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, ql = lane & 31;
  const int nrb = (S + RB - 1) / RB;
  int bh, pair;
  const bool lpt = work_item(nrb, xcd_map, bh, pair);
  const int b = bh / nh, head = bh % nh;
  const size_t hin = (size_t)b * in_bs + (size_t)head * in_hs;     // q / k / v
  const size_t hout = (size_t)b * out_bs + (size_t)head * out_hs;  // dq
  const size_t hkv = GQA ? (size_t)b * kv_bs + (size_t)(head / G) * kv_hs : hin;  // k / v of kv head head / G
  const int krs = GQA ? kv_rs : in_rs;
  const int W = (S + 31) >> 5;
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;
  using UNM = std::integral_constant<bool, false>;
  using MSK = std::integral_constant<bool, true>;

#pragma unroll 1
  for (int it = 0; it < 2; ++it) {
    const int qb = (lpt || it == 0) ? nrb - 1 - pair : pair;  // long item first
    if (it == 1 && (lpt || qb >= nrb - 1 - pair)) break;
    const int q0 = qb * RB + wid * 32;
    const int qa = q0 + ql;
    const bool qok = qa < S;
    const int qc = min(qa, S - 1);
    const uint32_t* mrow = mask ? mask + (size_t)bh * W * S + qc : nullptr;  // word j at mrow[j*S]

    bf16x8_t qf[D / 16], df[D / 16];
    const size_t orow = (((size_t)b * S + qc) * nh + head) * D;
    float dsum = 0.f;  // Delta = rowsum(dO * O), computed here (this kernel runs before dK/dV)
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      qf[s] = load_row8(q + hin + (size_t)qc * in_rs + 16 * s + 8 * h, qok);
      df[s] = load_row8(dout + orow + 16 * s + 8 * h, qok);
      const bf16x8_t of = load_row8(o + orow + 16 * s + 8 * h, qok);
#pragma unroll
      for (int j = 0; j < 8; ++j) dsum += frag_f<HK>(df[s], j) * frag_f<HK>(of, j);
    }
    const float nl2 = qok ? -lse[(size_t)bh * S + qc] * LOG2E : 0.f;
    const float dl = xhalf_sum(dsum);
    if (qok && h == 0) delta[(size_t)bh * S + qa] = dl;
    floatx16_t dqa[D / 32];
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) dqa[dt] = zero16();

    int lo_q = 0, lo_w = 0, ks = 0, kdoc = 0;  // DOC: as in the forward
    if constexpr (DOC) {
      const int* lrow = dlo + (size_t)b * S;
      lo_q = lrow[qc];
      lo_w = __builtin_amdgcn_readfirstlane(lo_q);
      doc_q_range(lrow, qb, S, ks, kdoc);
    }

    const int nkv = (min(S, qb * RB + RB) + KVB - 1) / KVB;
    glds_tile<D>(k + hkv, ks * KVB, S, krs, lds, wid, lane);
    glds_tile<D>(v + hkv, ks * KVB, S, krs, lds + KVB * D, wid, lane);
    __syncthreads();

    // Same loop structure as the forward: straight-line unmasked tiles (static LDS
    // buffers, unrolled by two), then the diagonal tile.
    uint2 mw_cur = make_uint2(0u, 0u), mw_next = make_uint2(0u, 0u);
    if (DROP) {
      if constexpr (DOC) mw_cur = make_uint2(mrow[(size_t)(2 * ks) * S], 2 * ks + 1 < W ? mrow[(size_t)(2 * ks + 1) * S] : 0u);
      else mw_cur = make_uint2(mrow[0], W > 1 ? mrow[S] : 0u);
    }
    auto step = [&](auto bufc, auto maskc, int kb) {
      constexpr int BUF = decltype(bufc)::value;
      constexpr bool MASKED = decltype(maskc)::value;
      const bool more = kb + 1 < nkv;
      if (more) {  // next tile straight into the other buffer (read by nobody since the last barrier)
        bf16_t* Kn = lds + (BUF ^ 1) * 2 * KVB * D;
        glds_tile<D>(k + hkv, (kb + 1) * KVB, S, krs, Kn, wid, lane);
        glds_tile<D>(v + hkv, (kb + 1) * KVB, S, krs, Kn + KVB * D, wid, lane);
        if (DROP) mw_next = make_uint2(mrow[(size_t)(2 * (kb + 1)) * S], 2 * (kb + 1) + 1 < W ? mrow[(size_t)(2 * (kb + 1) + 1) * S] : 0u);
      }
      const bf16_t* Kt = lds + BUF * 2 * KVB * D;
      const bf16_t* Vt = Kt + KVB * D;
      const int k0 = kb * KVB;
      if (!MASKED)
        dq_tile<false, DROP, HK, D, false, CAP>(dqa, Kt, Vt, qf, df, k0, qa, S, lane, c_log2, nl2, dl, dscale, mw_cur, 0, cap_k);
      else if (k0 <= q0 + 31 && (!DOC || k0 + KVB > lo_w))
        dq_tile<true, DROP, HK, D, DOC, CAP>(dqa, Kt, Vt, qf, df, k0, qa, S, lane, c_log2, nl2, dl, dscale, mw_cur, lo_q, cap_k);
      mw_cur = mw_next;
      tile_barrier();
    };
    const int nfull = min(qb, nkv);
    if constexpr (DOC) {  // tile kinds and buffers as in the forward's DOC loop
      for (int kb = ks; kb < nkv; ++kb) {
        const bool msk = kb < kdoc || kb >= nfull;
        if ((kb - ks) & 1) {
          if (msk) step(B1{}, MSK{}, kb);
          else step(B1{}, UNM{}, kb);
        } else {
          if (msk) step(B0{}, MSK{}, kb);
          else step(B0{}, UNM{}, kb);
        }
      }
    } else {
      int kb = 0;
      for (; kb + 1 < nfull; kb += 2) {
        step(B0{}, UNM{}, kb);
        step(B1{}, UNM{}, kb + 1);
      }
      if (kb < nfull) {
        step(B0{}, UNM{}, kb);
        if (kb + 1 < nkv) step(B1{}, MSK{}, kb + 1);
      } else if (kb < nkv) {
        step(B0{}, MSK{}, kb);
      }
    }
    if (qok) store_head_row<HK, D>(dq + hout + (size_t)qa * out_rs, dqa, scale, h, cosT, sinT, qa);
  }
#else
#error "attention_bwd_body.h: set DLT_ATTN_BWD_SECTION to 0 .. 3"
#endif
#undef DLT_ATTN_BWD_SECTION
