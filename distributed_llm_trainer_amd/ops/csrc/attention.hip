// Causal flash attention (head_dim 64 or 128: template parameter D) with in-kernel
// dropout for gfx950 MFMA.
//
// Replaces the reference's naive attention (gpt.py:230-234: Q@K^T, triu mask,
// fp32 softmax, bernoulli dropout, @V -- a [B,nh,S,S] score tensor per layer) and
// the SDPA path (gpt.py:199-206).  SURVEY §2.5 K5/K6.
//
// Design (CDNA4-first, see docs/KERNELS.md):
//  * v_mfma_f32_32x32x16_bf16 everywhere, accumulators in arch VGPRs
//    (-mllvm -amdgpu-mfma-vgpr-form: no v_accvgpr copies around the softmax).
//  * "Swapped" products put the softmax row on the lane: S^T = K.Q^T leaves one
//    query per lane with its keys in 16 accumulator registers, so row max / row sum
//    are in-lane plus one xor-32 swap, and the accumulator IS the B operand of the
//    next product (O^T = V^T.P^T) -- P never touches LDS.
//  * V / dO / Q / K^T operands are read with ds_read_b64_tr_b16 (hardware transpose).
//  * K/V (fwd, dQ) and Q/dO (dK/dV) tiles are register-staged into XOR-swizzled LDS,
//    double buffered: global loads of tile t+1 are issued before the MFMAs of tile t
//    and written to LDS after them (issue-early / write-late), one barrier per tile.
//  * Wave-uniform control: the wave index goes through readfirstlane, and each tile
//    is dispatched to a MASKED (diagonal / ragged) or UNMASKED instantiation, so the
//    hot loop has no exec-mask divergence and no per-element mask selects.
//  * Dropout: a VALU kernel hashes the keep decisions once (one lowbias32 per two
//    keys) into bitmasks in two layouts, row-major [bh][q][S/32] for the kernels
//    whose lanes are queries (fwd, dQ) and transposed [bh][k][S/32] for dK/dV whose
//    lanes are keys -- every MFMA kernel fetches ONE 32-bit word per lane per 32x32
//    sub-tile (2 x 12.6 MB per layer at B8 S1024 nh12).
//  * Backward = 2 kernels: dQ (recomputes S, dP; also emits Delta = rowsum(dO*O)),
//    then dK/dV (accumulated in registers) -- no fp32 atomics anywhere.  Causal
//    tile skipping; workgroups process paired items of equal total length.
//  * Document mask (DOC instantiations, packed training sequences): query q sees key k
//    iff lo[q] <= k <= q, equivalently k <= q <= hi[k] (lo / hi: int32 [B, S], first /
//    last position of the token's document, both non-decreasing).  The K/V loop of an
//    item starts at the tile of its smallest lo, the Q/dO loop of dK/dV ends at the tile
//    of its largest hi, and only tiles that straddle a bound take the masked kind.
//
//  * Grouped-query attention (GQA instantiations): nkv = nh / G K/V heads, query head h
//    uses kv head h / G.  Forward and dQ only move the K/V base (the per-query-head
//    arithmetic is the MHA kernel's); a dK/dV work item is 64 keys of one KV head and
//    runs the Q/dO tile pipeline once per query head of the group, in fixed order, with
//    dK/dV staying in registers -- no atomics, bitwise reproducible.
//
// Layouts: q, k, v, dq, dk, dv: strided views -- head-major [B*nh, S, 64] or the
// packed [B*S, 3, nh, 64] QKV GEMM output (see dlt_attn_stride); o, do: [B, S, nh, 64]
// bf16 (= the [M, H] GEMM layout);  lse, delta: [B*nh, S] fp32 (natural-log lse).
#include "attention.h"

#ifdef DLT_ATTN_FWD_TIMING
__device__ unsigned long long* g_attn_ftim;  // forward diagnostics, see attention.h
#endif

// ============================================================================ dropout bits
// Keep-bit words in two layouts (one hash per element pair, computed once):
//   mask [bh][w][q]  bit j = keep(q, key = 32w + j)   -- lane = query (fwd, dQ)
//   maskT[bh][w][k]  bit j = keep(q = 32w + j, key k) -- lane = key   (dK/dV)
// Word-major: the 32 lanes that write (here) or read (MFMA kernels: lane = row) one
// word index touch 128 contiguous bytes; the row-major [bh][q][w] layout made every
// lane's 4-byte access its own cache line (the store side cost ~3x the hashing).
// Only causal 32x32 tiles (key word <= query band) exist.  One half-wave per tile:
// lane l hashes row q = 32r + l (16 hashes -> its row word), then a 5-stage butterfly
// bit transpose gives lane j the column word of key 32w + j.
// Pure VALU, so the MFMA kernels only test bits instead of hashing at 2 waves/SIMD.
// Instruction budget (S % 32 == 0, the fast path): 11 VALU per hash -- the pair index
// is one xor (the row word's 16 pair indices differ from its first only in their low
// 4 bits), and each keep bit is the carry of (16 random bits in the high half) +
// (65536 - thr) << 16, shifted into the word by v_addc (no compare / select / or per
// bit); the transpose is branch-free (ds_swizzle + alignbit + bfi per stage).  Round 4
// form: ~32 VALU per hash (compare + s_nop + select per bit, divergent transpose).

// word = 2 * word + carry(v + c16): shifts in keep = (high 16 bits of v) >= thr at bit 0
// (c16 = (65536 - thr) << 16; the low half of c16 is zero, so v's low half never carries)
__device__ __forceinline__ uint32_t keep_shift_in(uint32_t word, uint32_t v, uint32_t c16) {
  uint32_t sum;  // discarded: only the carry is used
  asm("v_add_co_u32 %1, vcc, %2, %3\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
      : "+v"(word), "=&v"(sum)
      : "s"(c16), "v"(v)
      : "vcc");
  return word;
}
// (x ^ (x >> 16)) << 16: the low 16 bits of lowbias32's last step, in the high half
__device__ __forceinline__ uint32_t lo16_hi(uint32_t x) {
  uint32_t z;
  asm("v_xor_b32_sdwa %0, %1, %1 dst_sel:WORD_1 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1"
      : "=v"(z)
      : "v"(x));
  return z;
}
// lane l ^ d within 32-lane groups (ds_swizzle bitmask mode: and 0x1f, xor d)
template <int d>
__device__ __forceinline__ uint32_t swz_xor(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1f | (d << 10));
}
template <int d>
__device__ __forceinline__ uint32_t bt_stage(uint32_t col, int l) {
  // lanes with bit d clear keep the m-bits of their word and take the partner's m-bits
  // shifted up by d (rotl d, the wrapped bits land in m and are dropped); lanes with
  // bit d set keep ~m and take the partner's ~m-bits shifted down (rotr d)
  constexpr uint32_t m = d == 16 ? 0x0000FFFFu : d == 8 ? 0x00FF00FFu : d == 4 ? 0x0F0F0F0Fu : d == 2 ? 0x33333333u
                                                                                               : 0x55555555u;
  const uint32_t y = swz_xor<d>(col);
  const bool up = (l & d) == 0;
  const uint32_t r = __builtin_amdgcn_alignbit(y, y, up ? 32 - d : d);
  const uint32_t keep = up ? m : ~m;
  return (col & keep) | (r & ~keep);
}

// BAND (sliding-window layers): only the tiles a window can read.  The MFMA kernels walk
// 64-row items over 64-wide tiles (doc_q_range / doc_k_range with lo[q] = max(0, q - W + 1),
// hi[k] = min(S - 1, k + W - 1)): the item of query block qb starts at K/V tile qb - D, the
// item of key block kb ends at Q tile kb + D, D = ceil((W - 1) / 64).  Both read the bit tile
// (r, w) iff r/2 - w/2 <= D, so band r holds the words r - j, j = 0 .. 2D + 1, less the one
// that falls outside for an even r: a rectangle of 2D + 2 slots per band, tile -> (r, j) by
// one division.  Tiles outside the band are left as they were; same bits, same layout.
// The kernel never read its third argument (B * nh is the grid's y extent): the BAND form
// takes D there, so the full form's arguments, and with them its code, are what they were.
template <bool BAND = false>
__global__ __launch_bounds__(256) void k_dropout_bits(uint32_t* __restrict__ mask, uint32_t* __restrict__ maskT,
                                                      int BH_or_D, int S, uint32_t key, uint32_t thr) {
  const int W = (S + 31) >> 5;  // words per row == number of 32-row bands
  const int bh = blockIdx.y;
  const int lane = threadIdx.x & 63, l = lane & 31;
  const int tile = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + (lane >> 5);  // one tile per half-wave
  bool active;
  int r, w;
  if constexpr (BAND) {
    const int D = BH_or_D, nb = 2 * D + 2;
    r = tile / nb;
    w = r - (tile - r * nb);
    active = r < W && w >= 0 && (r >> 1) - (w >> 1) <= D;
    w = max(w, 0);
  } else {
    const int ntiles = W * (W + 1) / 2;
    active = tile < ntiles;
    // tile -> (band r, word w <= r): band r starts at tile r(r+1)/2; the float root is
    // within one of r for any realistic S, corrected once each way without loops
    r = (int)((sqrtf(8.f * (float)tile + 1.f) - 1.f) * 0.5f);
    r += ((r + 1) * (r + 2) / 2 <= tile) ? 1 : 0;
    r -= (r * (r + 1) / 2 > tile) ? 1 : 0;
    w = tile - r * (r + 1) / 2;
  }
  const int q = r * 32 + l;
  const uint32_t kbh = lowbias32(key + (uint32_t)bh * 0x9E3779B9u);
  uint32_t word = 0;
  if (active && q < S) {
    const uint32_t base = (uint32_t)q * (uint32_t)S + (uint32_t)(w * 32);
    if ((S & 31) == 0) {
      // base % 32 == 0: pair index base/2 + m has m in the 4 low bits, which base/2 lacks
      const uint32_t kx = kbh ^ (base >> 1);
      const uint32_t c16 = (65536u - thr) << 16;
#pragma unroll
      for (int m = 15; m >= 0; --m) {  // bits shift in from the top element down
        uint32_t x = kx ^ (uint32_t)m;
        x ^= x >> 16;
        x *= 0x7feb352du;
        x ^= x >> 15;
        x *= 0x846ca68bu;
        word = keep_shift_in(word, x, c16);            // element 2m + 1: high 16 bits
        word = keep_shift_in(word, lo16_hi(x), c16);  // element 2m: low 16 bits
      }
    } else {
      const int nk = min(32, S - w * 32);
      for (int j = 0; j < nk; ++j) {
        const uint32_t flat = base + (uint32_t)j;
        const uint32_t hsh = lowbias32(kbh ^ (flat >> 1));
        const uint32_t bits = (flat & 1u) ? (hsh >> 16) : (hsh & 0xffffu);
        word |= (uint32_t)(bits >= thr) << j;
      }
    }
    mask[((size_t)bh * W + w) * S + q] = word;  // word-major: the half-wave's 32 rows are contiguous
  }
  // 32x32 bit transpose within each half-wave (lane l holds row l; afterwards lane j
  // holds column j).  Every lane runs it (inactive lanes carry zeros) so the swizzles see
  // a full group.
  uint32_t col = word;
  col = bt_stage<16>(col, l);
  col = bt_stage<8>(col, l);
  col = bt_stage<4>(col, l);
  col = bt_stage<2>(col, l);
  col = bt_stage<1>(col, l);
  const int kk = w * 32 + l;
  if (active && kk < S) maskT[((size_t)bh * W + r) * S + kk] = col;
}

// ============================================================================ forward
// DOC: dlo = lo [B, S] of the document mask (see the header); unused otherwise.
// GQA: k / v have nh / G heads with their own strides (kv_bs, kv_hs, kv_rs); unused otherwise.
// The body is attention_fwd_body.h, shared with the SINK forms of attention_sink.hip.
template <bool DROP, int HK, int D, bool DOC = false, bool GQA = false>
__global__ __launch_bounds__(NT) ATTN_WAVES(D) void k_attn_fwd(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                    const bf16_t* __restrict__ v, bf16_t* __restrict__ o,
                                                    float* __restrict__ lse, const uint32_t* __restrict__ mask,
                                                    int S, int nh, float c_log2, float dscale, long in_bs,
                                                    int in_hs, int in_rs, int xcd_map,
                                                    const int* __restrict__ dlo = nullptr, int G = 1,
                                                    long kv_bs = 0, int kv_hs = 0, int kv_rs = 0) {
  // the fragment reads this kernel's parameters and template arguments by name (its header
  // lists them) plus these two; with SINK false it never reads `sink`
  constexpr bool SINK = false;
  const float* sink = nullptr;
#include "attention_fwd_body.h"
}

// ============================================================================ backward
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
__device__ unsigned long long* g_attn_tim;
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
template <bool MASK, bool DROP, int HK, int D, bool DOC = false>
__device__ __forceinline__ void dkdv_subtile(floatx16_t (&dka)[D / 32], floatx16_t (&dva)[D / 32], const bf16_t* Qt,
                                             const bf16_t* Dt, const float* rl, const float* rd,
                                             uint32_t mw, const bf16x8_t (&kf)[D / 16], const bf16x8_t (&vf)[D / 16],
                                             int qs, int ka, int S, int lane, float c_log2, float dscale,
                                             int hi = 0) {
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
      float p = fast_exp2(fmaf(sacc[i], c_log2, -lv[e]));
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
    }
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

// Work items: 64 keys (2 waves x 32); a workgroup processes the pair of key blocks
// (p, nrb-1-p) -- equal work per workgroup (see the forward).
// DOC: dhi = hi [B, S] of the document mask (lanes are keys here); unused otherwise.
template <bool DROP, int HK, int D, bool DOC = false>
__global__ __launch_bounds__(NT) ATTN_WAVES(D) void k_attn_bwd_dkdv(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                         const bf16_t* __restrict__ v,
                                                         const bf16_t* __restrict__ dout,
                                                         const float* __restrict__ lse,
                                                         const float* __restrict__ delta,
                                                         const uint32_t* __restrict__ maskT, bf16_t* __restrict__ dk,
                                                         bf16_t* __restrict__ dv, int S, int nh, float c_log2,
                                                         float scale, float dscale, long in_bs, int in_hs, int in_rs,
                                                         long out_bs, int out_hs, int out_rs,
                                                         const float* __restrict__ cosT,
                                                         const float* __restrict__ sinT, int xcd_map,
                                                         const int* __restrict__ dhi = nullptr) {
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
          dkdv_subtile<false, DROP, HK, D>(dka, dva, Qs, Ds, rlp + 32 * qt, rdp + 32 * qt, mw, kf, vf, qs, ka, S,
                                           lane, c_log2, dscale);
        else if (qs + 31 >= k0 && (!DOC || qs <= hi_w))  // DOC: not wholly past this wave's documents
          dkdv_subtile<true, DROP, HK, D, DOC>(dka, dva, Qs, Ds, rlp + 32 * qt, rdp + 32 * qt, mw, kf, vf, qs, ka, S,
                                               lane, c_log2, dscale, hi_k);
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
}

// ---------------------------------------------------------------- dK / dV, grouped-query
// The kernel above with a loop over the query heads that share the item's KV head.  It is a
// kernel of its own, not a template flag of k_attn_bwd_dkdv: that kernel sits at the VGPR
// limit, and any edit of its source -- even one that is dead code without GQA -- changed
// hipcc's register allocation of the MHA instantiations.
// The grid runs over the B * nh / G KV heads.  k / v use (kv_bs, kv_hs, kv_rs), dk / dv
// the out strides; q, dO, lse, delta and the keep bits are those of query head kvh * G + g,
// g = 0 .. G-1 in this fixed order, all adding into the same dka / dva registers, stored
// once at the end.  The double-buffered Q/dO pipeline does not drain between heads: the
// last tile step of head g prefetches the first tile of head g + 1 into the other buffer
// (the tile order, and so every sum, is that of G restarted pipelines; with a restart
// inside the loop the D = 64 instantiations spilled 50-90 bytes per lane).
template <bool DROP, int HK, int D, bool DOC = false>
__global__ __launch_bounds__(NT) ATTN_WAVES(D) void k_attn_bwd_dkdv_gqa(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    const uint32_t* __restrict__ maskT, bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int S, int nh, float c_log2,
    float scale, float dscale, long in_bs, int in_hs, int in_rs, long out_bs, int out_hs, int out_rs,
    const float* __restrict__ cosT, const float* __restrict__ sinT, int xcd_map, const int* __restrict__ dhi, int G,
    long kv_bs, int kv_hs, int kv_rs) {
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
            dkdv_subtile<false, DROP, HK, D>(dka, dva, Qs, Ds, rlp + 32 * qt, rdp + 32 * qt, mw, kf, vf, qs, ka, S,
                                             lane, c_log2, dscale);
          else if (qs + 31 >= k0 && (!DOC || qs <= hi_w))  // DOC: not wholly past this wave's documents
            dkdv_subtile<true, DROP, HK, D, DOC>(dka, dva, Qs, Ds, rlp + 32 * qt, rdp + 32 * qt, mw, kf, vf, qs, ka, S,
                                                 lane, c_log2, dscale, hi_k);
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
}

// ---------------------------------------------------------------------- dQ
template <bool MASK, bool DROP, int HK, int D, bool DOC = false>
__device__ __forceinline__ void dq_tile(floatx16_t (&dqa)[D / 32], const bf16_t* Kt, const bf16_t* Vt,
                                        const bf16x8_t (&qf)[D / 16], const bf16x8_t (&df)[D / 16], int k0, int qa,
                                        int S, int lane, float c_log2, float nl2, float dl, float dscale, uint2 mw,
                                        int lo = 0) {
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
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int kr = acc_row(i, h);
      float p = fast_exp2(fmaf(sacc[t][i], c_log2, nl2));
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
    }
  }
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const bf16x8_t sb = acc_frag<HK>(pacc[kk >> 1], kk & 1);
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) dqa[dt] = mfma<HK>(tr_frag<D>(Kt, kk, dt, lane), sb, dqa[dt]);
  }
}

// DOC: dlo = lo [B, S] of the document mask, as in the forward; unused otherwise.
// GQA: k / v strides as in the forward; dq, delta and the keep bits stay per query head.
template <bool DROP, int HK, int D, bool DOC = false, bool GQA = false>
__global__ __launch_bounds__(NT) ATTN_WAVES(D) void k_attn_bwd_dq(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                       const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
                                                       const bf16_t* __restrict__ o,
                                                       const float* __restrict__ lse,
                                                       float* __restrict__ delta,
                                                       const uint32_t* __restrict__ mask, bf16_t* __restrict__ dq,
                                                       int S, int nh, float c_log2, float scale, float dscale,
                                                       long in_bs, int in_hs, int in_rs, long out_bs, int out_hs,
                                                       int out_rs, const float* __restrict__ cosT,
                                                       const float* __restrict__ sinT, int xcd_map,
                                                       const int* __restrict__ dlo = nullptr, int G = 1,
                                                       long kv_bs = 0, int kv_hs = 0, int kv_rs = 0) {
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
        dq_tile<false, DROP, HK, D>(dqa, Kt, Vt, qf, df, k0, qa, S, lane, c_log2, nl2, dl, dscale, mw_cur);
      else if (k0 <= q0 + 31 && (!DOC || k0 + KVB > lo_w))
        dq_tile<true, DROP, HK, D, DOC>(dqa, Kt, Vt, qf, df, k0, qa, S, lane, c_log2, nl2, dl, dscale, mw_cur, lo_q);
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
}

// ============================================================================ sink gradient
// Gradient of the attention sinks (k_attn_fwd_sink, attention_sink.hip): with p_sink = exp(sink[h] - lse[b,h,q])
// the sink column has dP = 0, so dS_sink = -p_sink * delta and
//   dsink[h] += -sum_{b,q} p_sink[b,h,q] * delta[b,h,q],
// delta the raw rowsum(dO * O) that dQ leaves in the workspace (the 1 / dscale of dK/dV is
// not part of it).  One workgroup per head: thread t adds the rows t, t + SB_NT, ... of the
// flattened (b, q) index in that order, then the partials are summed by a wave butterfly
// and the waves in wave order through LDS.  No float atomics: two calls give the same bits,
// and the one += per head makes a second call on the same inputs double the first exactly
// (dsink = 0 before).
#define SB_NT 1024
__global__ __launch_bounds__(SB_NT) void k_attn_sink_bwd(const float* __restrict__ lse,
                                                         const float* __restrict__ delta,
                                                         const float* __restrict__ sink,
                                                         float* __restrict__ dsink, int B, int nh, int S) {
  __shared__ float part[SB_NT / 64];
  const int head = blockIdx.x, tid = threadIdx.x;
  const float sk = sink[head];
  const long n = (long)B * S;
  float acc = 0.f;
  for (long i = tid; i < n; i += SB_NT) {
    const long b = i / S, r = i - b * S;
    const size_t at = ((size_t)b * nh + head) * S + r;
    acc += fast_exp2((sk - lse[at]) * LOG2E) * delta[at];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < SB_NT / 64; ++w) t += part[w];
    dsink[head] -= t;
  }
}

// ============================================================================ launchers
// mask: uint32 [2][B*nh, ceil(S/32), S] keep-bits written by the forward when dropout
// is on -- [0] row layout (lane = query), [1] transposed (lane = key), see
// k_dropout_bits.
// Keep-bit masks only (they depend on the key, not on the data): lets the engine
// produce them on a side stream ahead of the layer's GEMMs.
DLT_API int dlt_attn_dropout_mask(uint32_t* mask, int B, int nh, int S, uint32_t key, uint32_t thr,
                                  hipStream_t st) {
  if (S <= 0 || !mask || !thr) return -1;
  const int W = (S + 31) / 32;
  const int ntiles = W * (W + 1) / 2;  // 8 tiles (2 per wave) per block
  uint32_t* maskT = mask + (size_t)B * nh * S * W;
  k_dropout_bits<><<<dim3((ntiles + 7) / 8, B * nh), 256, 0, st>>>(mask, maskT, B * nh, S, key, thr);
  DLT_CHECK_LAUNCH();
}

// The keep bits a sliding-window layer of `window` keys reads (k_dropout_bits<true>): the same
// buffer and the same bits as dlt_attn_dropout_mask inside the band, nothing written outside
// it.  A band that covers the causal triangle takes the full kernel.
DLT_API int dlt_attn_dropout_mask_band(uint32_t* mask, int B, int nh, int S, uint32_t key, uint32_t thr, int window,
                                       hipStream_t st) {
  if (S <= 0 || !mask || !thr || window < 1) return -1;
  const int W = (S + 31) / 32;
  const int D = (int)(((long)window - 1 + 63) / 64 < (long)W ? ((long)window - 1 + 63) / 64 : (long)W);
  if (2 * D + 2 >= W + 1) return dlt_attn_dropout_mask(mask, B, nh, S, key, thr, st);
  const long ntiles = (long)W * (2 * D + 2);
  uint32_t* maskT = mask + (size_t)B * nh * S * W;
  k_dropout_bits<true><<<dim3((unsigned)((ntiles + 7) / 8), B * nh), 256, 0, st>>>(mask, maskT, D, S, key, thr);
  DLT_CHECK_LAUNCH();
}

DLT_API int dlt_attn_args_size() { return (int)sizeof(dlt_attn_args); }

DLT_API int dlt_attn_fwd(const dlt_attn_args* a, hipStream_t st) {
  const int nh = a->nh, nkv = a->nkv, S = a->S;
  const dlt_attn_stride sq = a->stride.q, skv = nkv ? a->stride.kv : dlt_attn_stride{0, 0, 0};
  if (!attn_hd_ok(a->hd) || S <= 0 || !attn_stride_ok(sq, 8)) return -1;
  if (nkv < 0 || (nkv && (nh % nkv || !attn_stride_ok(skv, 8)))) return -5;
  const int G = nkv ? nh / nkv : 1;
  if (a->thr && !a->mask) return -2;  // dropout needs the keep-bit buffer
  const int nrb = (S + RB - 1) / RB;
  const int xm = xcd_map_enabled();
  const dim3 grid(attn_grid(nrb, a->B * nh, xm));  // work items, see work_item()
  const float c_log2 = a->scale * LOG2E;
  if (a->thr && a->gen_mask) {
    const int rc = dlt_attn_dropout_mask(a->mask, a->B, nh, S, a->key, a->thr, st);
    if (rc) return rc;
  }
  if (a->sink) return attn_fwd_sink_launch(a, st);  // the SINK forms: attention_sink.hip
  DLT_BOOL_DISPATCH(DROPC, a->thr, DLT_BOOL_DISPATCH(GQAC, nkv, DLT_BOOL_DISPATCH(DOCC, a->lo,
      DLT_HD_DISPATCH(a->hd, DLT_HK_DISPATCH(a->hk, k_attn_fwd<DROPC, HKC, HDC, DOCC, GQAC><<<grid, NT, 0, st>>>(
          a->q, a->k, a->v, a->o, a->lse, DROPC ? a->mask : nullptr, S, nh, c_log2, a->dscale, sq.b, sq.h, sq.r, xm,
          a->lo, G, skv.b, skv.h, skv.r))))));
  DLT_CHECK_LAUNCH();
}

DLT_API int dlt_attn_bwd(const dlt_attn_args* a, hipStream_t st) {
  const int nh = a->nh, nkv = a->nkv, S = a->S;
  const dlt_attn_stride sq = a->stride.q, sdq = a->stride.dq;
  const dlt_attn_stride skv = nkv ? a->stride.kv : dlt_attn_stride{0, 0, 0}, sdkv = nkv ? a->stride.dkv : sdq;
  if ((a->lo == nullptr) != (a->hi == nullptr)) return -4;
  if (nkv < 0 || (nkv && (nh % nkv || !attn_stride_ok(skv, 8) || !attn_stride_ok(sdkv, 4)))) return -5;
  const int G = nkv ? nh / nkv : 1;
  if (!attn_hd_ok(a->hd) || S <= 0 || !attn_stride_ok(sq, 8) || !attn_stride_ok(sdq, 4)) return -1;
  if ((a->cosT == nullptr) != (a->sinT == nullptr)) return -3;
  if ((a->sink == nullptr) != (a->dsink == nullptr)) return -6;
  if (a->thr && !a->mask) return -2;
  const float scale = a->scale, dscale = a->dscale, c_log2 = scale * LOG2E;
  const int nrb = (S + RB - 1) / RB;
  const int xm = xcd_map_enabled();
  const dim3 gk(attn_grid(nrb, a->B * (nkv ? nkv : nh), xm)), gq(attn_grid(nrb, a->B * nh, xm));  // work items, see work_item()
  // dK/dV's lanes are keys: it reads the transposed keep bits
  const uint32_t* mask = a->thr ? a->mask : nullptr;
  const uint32_t* maskT = mask ? mask + (size_t)a->B * nh * S * ((S + 31) / 32) : nullptr;
  // dQ first: it also produces Delta = rowsum(dO * O) (no separate kernel), which
  // dK/dV then reads.  DROPC spans the three launches: the device code lists the kernels
  // in the order the launches name them (dQ, dK/dV GQA, dK/dV with dropout, then without).
  DLT_BOOL_DISPATCH(DROPC, mask, {
    DLT_BOOL_DISPATCH(GQAC, nkv, DLT_BOOL_DISPATCH(DOCC, a->lo, DLT_HD_DISPATCH(a->hd, DLT_HK_DISPATCH(a->hk,
        k_attn_bwd_dq<DROPC, HKC, HDC, DOCC, GQAC><<<gq, NT, 0, st>>>(
            a->q, a->k, a->v, a->dout, a->o, a->lse, a->delta_ws, mask, a->dq, S, nh, c_log2, scale, dscale, sq.b,
            sq.h, sq.r, sdq.b, sdq.h, sdq.r, a->cosT, a->sinT, xm, a->lo, G, skv.b, skv.h, skv.r)))));
    if (nkv)  // grid over the B * nkv KV heads
      DLT_BOOL_DISPATCH(DOCC, a->hi, DLT_HD_DISPATCH(a->hd, DLT_HK_DISPATCH(a->hk,
          k_attn_bwd_dkdv_gqa<DROPC, HKC, HDC, DOCC><<<gk, NT, 0, st>>>(
              a->q, a->k, a->v, a->dout, a->lse, a->delta_ws, maskT, a->dk, a->dv, S, nh, c_log2, scale, dscale, sq.b,
              sq.h, sq.r, sdkv.b, sdkv.h, sdkv.r, a->cosT, a->sinT, xm, a->hi, G, skv.b, skv.h, skv.r))));
    else
      DLT_BOOL_DISPATCH(DOCC, a->hi, DLT_HD_DISPATCH(a->hd, DLT_HK_DISPATCH(a->hk,
          k_attn_bwd_dkdv<DROPC, HKC, HDC, DOCC><<<gk, NT, 0, st>>>(
              a->q, a->k, a->v, a->dout, a->lse, a->delta_ws, maskT, a->dk, a->dv, S, nh, c_log2, scale, dscale, sq.b,
              sq.h, sq.r, sdq.b, sdq.h, sdq.r, a->cosT, a->sinT, xm, a->hi))));
  });
  // the sink gradient reads lse and the delta dQ has just written (same stream)
  if (a->sink) k_attn_sink_bwd<<<nh, SB_NT, 0, st>>>(a->lse, a->delta_ws, a->sink, a->dsink, a->B, nh, S);
  DLT_CHECK_LAUNCH();
}
