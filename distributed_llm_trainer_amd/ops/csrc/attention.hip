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
  constexpr bool CAP = false;
  constexpr float cap_k = 0.f;
#include "attention_fwd_body.h"
}

// ============================================================================ backward
// store_head_row, dkdv_subtile and dq_tile, and the bodies of the three kernels below, live in
// attention_bwd_body.h, shared with the CAP forms of attention_cap.hip.
#define DLT_ATTN_BWD_SECTION 0
#include "attention_bwd_body.h"

#ifdef DLT_ATTN_TIMING
__device__ unsigned long long* g_attn_tim;  // see ATTN_STAMP
#endif

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
  // the fragment reads this kernel's parameters and template arguments by name, plus these two
  constexpr bool CAP = false;
  constexpr float cap_k = 0.f;
#define DLT_ATTN_BWD_SECTION 1
#include "attention_bwd_body.h"
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
  // the fragment reads this kernel's parameters and template arguments by name, plus these two
  constexpr bool CAP = false;
  constexpr float cap_k = 0.f;
#define DLT_ATTN_BWD_SECTION 2
#include "attention_bwd_body.h"
}

// ---------------------------------------------------------------------- dQ
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
  // the fragment reads this kernel's parameters and template arguments by name, plus these two
  constexpr bool CAP = false;
  constexpr float cap_k = 0.f;
#define DLT_ATTN_BWD_SECTION 3
#include "attention_bwd_body.h"
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

// dlt_attn_args.softcap: 0 (off) or a finite cap in (0, ATTN_SOFTCAP_MAX].  The CAP kernels'
// exponent constant is cap * log2(e), and the DOC forward multiplies it with M_DEAD = -1e30: the
// bound keeps that product finite in fp32 (ops/attn_routes.py SCORE_SOFTCAP_MAX is the same number).
#define ATTN_SOFTCAP_MAX 65536.f
static inline bool attn_softcap_ok(float c) { return c >= 0.f && c <= ATTN_SOFTCAP_MAX; }  // false for NaN, inf

DLT_API int dlt_attn_args_size() { return (int)sizeof(dlt_attn_args); }

DLT_API int dlt_attn_fwd(const dlt_attn_args* a, hipStream_t st) {
  const int nh = a->nh, nkv = a->nkv, S = a->S;
  const dlt_attn_stride sq = a->stride.q, skv = nkv ? a->stride.kv : dlt_attn_stride{0, 0, 0};
  if (!attn_hd_ok(a->hd) || S <= 0 || !attn_stride_ok(sq, 8)) return -1;
  if (nkv < 0 || (nkv && (nh % nkv || !attn_stride_ok(skv, 8)))) return -5;
  if (!attn_softcap_ok(a->softcap)) return -7;  // negative, NaN, inf or beyond the kernels' range
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
  if (a->softcap > 0.f) return attn_fwd_cap_launch(a, st);  // the CAP forms (with or without a sink): attention_cap.hip
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
  if (!attn_softcap_ok(a->softcap)) return -7;  // negative, NaN, inf or beyond the kernels' range
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
  if (a->softcap > 0.f) {  // the CAP forms of dQ and dK/dV: attention_cap.hip
    const int rc = attn_bwd_cap_launch(a, st);
    if (rc) return rc;
  } else {
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
  }
  // the sink gradient reads lse and the delta dQ has just written (same stream)
  if (a->sink) k_attn_sink_bwd<<<nh, SB_NT, 0, st>>>(a->lse, a->delta_ws, a->sink, a->dsink, a->B, nh, S);
  DLT_CHECK_LAUNCH();
}
