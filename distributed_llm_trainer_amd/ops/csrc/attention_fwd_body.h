// The body of the flash-attention forward kernels, included INSIDE the kernel definitions:
// k_attn_fwd (attention.hip: SINK = false) and k_attn_fwd_sink (attention_sink.hip: SINK = true).
// A textual fragment, not a __device__ function: called through a forced-inline function the
// plain kernels no longer compiled to the registers they had (4 of the head_dim-128 forms moved
// by 2 - 4 AGPRs).  Expects the kernel's parameters q, k, v, o, lse, mask, S, nh, c_log2,
// dscale, in_bs, in_hs, in_rs, xcd_map, dlo, G, kv_bs, kv_hs, kv_rs, the template parameters
// DROP, HK, D, DOC, GQA, and in scope
//   constexpr bool SINK;  const float* sink;   // fp32 [nh], read only when SINK
//   constexpr bool CAP;   float cap_k;         // 2 log2(e) scale / cap, read only when CAP
// CAP (attention_cap.hip): scores cap * tanh(scale q.k / cap); fwd_tile turns the accumulator into
// the tanh in place and c_log2 is cap * log2(e), so everything here runs unchanged in those units.
// SINK: one more logit per query head in the softmax denominator (natural-log units, not
// scaled, no value row: p_j = exp(s_j) / (sum_j exp(s_j) + exp(sink))); it enters in the
// epilogue only, see there.
  static_assert(std::is_same<std::remove_const_t<decltype(SINK)>, bool>::value && (D == 64 || D == 128) && (HK == 0 || HK == 1),
                "attention_fwd_body.h: include it inside a kernel template <bool DROP, int HK, int D, bool DOC, bool GQA> "
                "with a compile-time `bool SINK` and `const float* sink` in scope");
  __shared__ __attribute__((aligned(16))) bf16_t lds[2 * 2 * KVB * D];  // [buf][K|V][64][D]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, ql = lane & 31;
  const int nrb = (S + RB - 1) / RB;
  int bh, pair;
  const bool lpt = work_item(nrb, xcd_map, bh, pair);
  const int b = bh / nh, head = bh % nh;
  const size_t hin = (size_t)b * in_bs + (size_t)head * in_hs;  // (b, head) base of q / k / v
  // GQA: k / v base of kv head head / G; everything else stays per query head
  const size_t hkv = GQA ? (size_t)b * kv_bs + (size_t)(head / G) * kv_hs : hin;
  const int krs = GQA ? kv_rs : in_rs;
  const int W = (S + 31) >> 5;
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;
  using UNM = std::integral_constant<bool, false>;
  using MSK = std::integral_constant<bool, true>;
#ifdef DLT_ATTN_FWD_TIMING
  unsigned long long f_comp = 0, f_wait = 0, f_tiles = 0;
  const unsigned long long f_t0 = __builtin_amdgcn_s_memtime();
#endif

#pragma unroll 1
  for (int it = 0; it < 2; ++it) {
    const int qb = (lpt || it == 0) ? nrb - 1 - pair : pair;  // long item first
    if (it == 1 && (lpt || qb >= nrb - 1 - pair)) break;       // odd nrb: middle item once
    const int q0 = qb * RB + wid * 32;  // this wave's first query (wave-uniform)
    const int qa = q0 + ql;
    const uint32_t* mrow = mask ? mask + (size_t)bh * W * S + min(qa, S - 1) : nullptr;  // word j at mrow[j*S]

    bf16x8_t qf[D / 16];
#pragma unroll
    for (int s = 0; s < D / 16; ++s)
      qf[s] = load_row8(q + hin + (size_t)min(qa, S - 1) * in_rs + 16 * s + 8 * h, qa < S);

    FwdState<D> fs;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) fs.o[dt] = zero16();
    fs.m = DOC ? M_DEAD : -INFINITY;
    fs.l = 0.f;

    // DOC: this lane's bound, the wave's smallest (its first query's), and the item's
    // tile range: the loop starts at tile ks, tiles below kdoc straddle some row's bound
    int lo_q = 0, lo_w = 0, ks = 0, kdoc = 0;
    if constexpr (DOC) {
      const int* lrow = dlo + (size_t)b * S;
      lo_q = lrow[min(qa, S - 1)];
      lo_w = __builtin_amdgcn_readfirstlane(lo_q);
      doc_q_range(lrow, qb, S, ks, kdoc);
    }

    const int nkv = (min(S, qb * RB + RB) + KVB - 1) / KVB;  // = qb + 1 except at a ragged end
    glds_tile<D>(k + hkv, ks * KVB, S, krs, lds, wid, lane);
    glds_tile<D>(v + hkv, ks * KVB, S, krs, lds + KVB * D, wid, lane);
    __syncthreads();

    // One K/V tile per step.  BUF is a compile-time LDS buffer index and MASKED a
    // compile-time tile kind: tiles kb < qb lie entirely below every query of the
    // item (straight-line unmasked loop, unrolled by two so every LDS address is
    // lane-base + immediate); tile qb holds the diagonal.
    uint2 mw_cur = make_uint2(0u, 0u), mw_next = make_uint2(0u, 0u);
    if (DROP) {  // words of the first tile
      if constexpr (DOC) mw_cur = make_uint2(mrow[(size_t)(2 * ks) * S], 2 * ks + 1 < W ? mrow[(size_t)(2 * ks + 1) * S] : 0u);
      else mw_cur = make_uint2(mrow[0], W > 1 ? mrow[S] : 0u);
    }
    auto step = [&](auto bufc, auto maskc, int kb) {
      constexpr int BUF = decltype(bufc)::value;
      constexpr bool MASKED = decltype(maskc)::value;
      FWD_T(ta);
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
        fwd_tile<false, DROP, HK, D, false, CAP>(fs, Kt, Vt, qf, k0, qa, S, lane, c_log2, mw_cur, 0, cap_k);
      else if (k0 <= q0 + 31 && (!DOC || k0 + KVB > lo_w))  // DOC: not wholly below this wave's documents
        fwd_tile<true, DROP, HK, D, DOC, CAP>(fs, Kt, Vt, qf, k0, qa, S, lane, c_log2, mw_cur, lo_q, cap_k);
      mw_cur = mw_next;
      FWD_T(tb);
      tile_barrier();
      FWD_T(tc);
      FWD_ACC(tb - ta, tc - tb);
    };
    const int nfull = min(qb, nkv);
    if constexpr (DOC) {
      // Tile kb sits in buffer (kb - ks) & 1.  [ks, kdoc): masked by some row's bound;
      // [kdoc, nfull): unmasked; [nfull, nkv): the diagonal.  One body per (buffer, kind),
      // picked by two wave-uniform scalar branches per tile.
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
      if (kb < nfull) {  // odd count: last unmasked tile in buffer 0, diagonal in buffer 1
        step(B0{}, UNM{}, kb);
        if (kb + 1 < nkv) step(B1{}, MSK{}, kb + 1);
      } else if (kb < nkv) {
        step(B0{}, MSK{}, kb);
      }
    }

    float l_tot = xhalf_sum(fs.l);
    float inv_l, lse_q = 0.f;
    if constexpr (SINK) {
      // The sink joins the row sum here.  fs.m is deferred (up to 2^RESCALE_LOG2 below the
      // true max, M_DEAD for a row without keys) and the sink can lie far above every score,
      // so the max is retaken in log2 units, m' = max(m, sink), l is rescaled by
      // alpha = exp2(m - m') before exp2(sink - m') is added, and o takes alpha through its
      // normaliser (a sink 100 above the scores gives alpha = 0: o = 0, lse = sink).
      // sink = -inf: m' = m, alpha = 1 and the added term is 0 -- the plain kernel's bits.
      const float sk = sink[head];
      const float m2 = fs.m * c_log2, s2 = sk * LOG2E;
      const float mn = fmaxf(m2, s2);
      const float alpha = fast_exp2(m2 - mn);
      l_tot = l_tot * alpha + fast_exp2(s2 - mn);
      inv_l = (DROP ? dscale : 1.f) * alpha / l_tot;
      // the plain expression as the plain kernel writes it (one fma), so that a sink below the
      // running max -- and sink = -inf -- keeps its bits; a sink above it is the max itself
      // (the second logarithm goes through an opaque copy: shared with the first, its product
      // with ln 2 is hoisted out of that fma and the last bit moves)
      const float lse_m = fs.m * (c_log2 / LOG2E) + __logf(l_tot);
      float l_sk = l_tot;
      asm volatile("" : "+v"(l_sk));
      lse_q = s2 > m2 ? sk + __logf(l_sk) : lse_m;
    } else {
      inv_l = (DROP ? dscale : 1.f) / l_tot;
    }
    if (qa < S) {
      if (h == 0) lse[(size_t)bh * S + qa] = SINK ? lse_q : fs.m * (c_log2 / LOG2E) + __logf(l_tot);
      bf16_t* orow = o + (((size_t)b * S + qa) * nh + head) * D;
      uint2 w[D / 32][4];
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          u16x4 t;
#pragma unroll
          for (int e = 0; e < 4; ++e) t.v[e] = f2h<HK>(fs.o[dt][4 * g + e] * inv_l);
          w[dt][g] = __builtin_bit_cast(uint2, t);
        }
      store_row16<D>(orow, w, h);
    }
  }
#ifdef DLT_ATTN_FWD_TIMING
  const unsigned long long f_t1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) {
    unsigned long long* r = g_attn_ftim + ((size_t)blockIdx.x * 2 + wid) * 6;
    r[0] = f_t0; r[1] = f_t1; r[2] = f_comp; r[3] = f_wait; r[4] = f_tiles;
  }
#endif
