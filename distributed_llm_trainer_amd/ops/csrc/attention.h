// Device code and launch arguments shared by the flash-attention translation units:
// attention.hip (forward, backward, keep bits, the C entry points), attention_sink.hip (the
// SINK forms of the forward) and attention_cap.hip (the CAP forms of the forward and the
// backward: attention-score soft-capping), translation units of their own so that
// attention.hip's kernels compile exactly as they did without them.  The kernel bodies are
// the fragments attention_fwd_body.h and attention_bwd_body.h.  See attention.hip for the design.
#pragma once
#include "common.h"

#ifndef DLT_ATTN_KREAD_ASM
#define DLT_ATTN_KREAD_ASM 1
#endif

#include <type_traits>

#define KVB 64     // keys per staged tile (fwd / dQ)
#define RB 64      // rows (queries for fwd / dQ, keys for dK/dV) per work item: 2 waves x 32
#define QSTEP 64   // queries per staged tile (dK/dV)
#define NT 128     // threads per workgroup
#define LOG2E 1.44269504088896340736f

typedef __attribute__((address_space(3))) shortx4_t lds_shortx4_t;
typedef short shortx8_t __attribute__((ext_vector_type(8)));

// LDS tile: [64 rows][D bf16].  D = 64: 128-B rows, 16-B chunk c of row r stored at
// chunk c ^ ((r >> 1) & 7) -- row pairs fill the 64 banks, so 16 consecutive rows of a
// ds_read_b128 row-fragment read are conflict-free.  D = 128: 256-B rows (every row
// starts at bank 0), chunk c ^ (r & 15) gives 16 consecutive rows 16 distinct chunks.
template <int D>
__device__ __forceinline__ int swz_x(int row) { return D == 64 ? ((row >> 1) & 7) : (row & 15); }
template <int D>
__device__ __forceinline__ int swz_off(int row, int col) {
  return row * D + ((((col >> 3) ^ swz_x<D>(row))) << 3) + (col & 7);
}

template <int D>
__device__ __forceinline__ bf16x8_t lds_row8(const bf16_t* T, int row, int col) {
  return *reinterpret_cast<const bf16x8_t*>(T + swz_off<D>(row, col));
}

template <int D>
__device__ __forceinline__ shortx4_t lds_tr4(const bf16_t* T, int row, int col) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_shortx4_t*)(T + swz_off<D>(row, col)));
}

// A operand A[d][k] (k = rows of T) in the permuted k order that matches accumulator
// registers 8s..8s+7 used as the B operand: element j of lane-half h <-> row
// 16*kk + 8*(j>>2) + 4*h + (j&3)  (cdna_hip_programming.md §3).
template <int D>
__device__ __forceinline__ bf16x8_t tr_frag(const bf16_t* T, int kk, int dt, int lane) {
  const int h = lane >> 5, i = lane & 15;
  const int col = 32 * dt + 16 * ((lane >> 4) & 1) + 4 * (i & 3);
  const int r1 = 16 * kk + 4 * h + (i >> 2);
  const shortx4_t a = lds_tr4<D>(T, r1, col);
  const shortx4_t b = lds_tr4<D>(T, r1 + 8, col);
  shortx8_t c = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8_t, c);
}

// The same fragment read through inline asm.  hipcc conservatively drains vmcnt(0)
// before any ds_read_b64_tr_b16 *intrinsic* while a global_load_lds is in flight
// (it cannot prove the DMA target and the read disjoint), which serialises the next
// tile's LDS-DMA with this tile's compute.  Asm reads are invisible to that alias
// check; the protocol that makes them safe is explicit: every tile step ends with
// `s_waitcnt vmcnt(0)` + barrier (tile_barrier), so a tile is complete before any
// wave reads it, and tr_wait() retires the reads before their registers are used.
template <int D>
__device__ __forceinline__ shortx4_t lds_tr4_asm(const bf16_t* T, int row, int col) {
  shortx4_t r;
  const uint32_t addr = (uint32_t)(uintptr_t)(T + swz_off<D>(row, col));
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}
template <int D>
__device__ __forceinline__ bf16x8_t tr_frag_asm(const bf16_t* T, int kk, int dt, int lane) {
  const int h = lane >> 5, i = lane & 15;
  const int col = 32 * dt + 16 * ((lane >> 4) & 1) + 4 * (i & 3);
  const int r1 = 16 * kk + 4 * h + (i >> 2);
  const shortx4_t a = lds_tr4_asm<D>(T, r1, col);
  const shortx4_t b = lds_tr4_asm<D>(T, r1 + 8, col);
  shortx8_t c = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8_t, c);
}
// Row-fragment read through inline asm (see lds_tr4_asm for the protocol), so several
// reads can be in flight under one counted wait (the intrinsic form drew one
// lgkmcnt(0) per MFMA pair).
template <int D>
__device__ __forceinline__ bf16x8_t lds_row8_asm(const bf16_t* T, int row, int col) {
  bf16x8_t r;
  const uint32_t addr = (uint32_t)(uintptr_t)(T + swz_off<D>(row, col));
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}
// Oldest four of eight outstanding LDS reads retired (LDS returns in order; no SMEM
// load is issued inside a tile step).
__device__ __forceinline__ void lgkm_wait4(bf16x8_t& a, bf16x8_t& b, bf16x8_t& c, bf16x8_t& d) {
  asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}
// D = 128 forms: the oldest eight of sixteen reads retired; pin4 keeps four more
// fragments' consumers below the preceding wait (volatile asm stays in order).
__device__ __forceinline__ void lgkm_wait8(bf16x8_t& a, bf16x8_t& b, bf16x8_t& c, bf16x8_t& d) {
  asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}
__device__ __forceinline__ void pin4(bf16x8_t& a, bf16x8_t& b, bf16x8_t& c, bf16x8_t& d) {
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
// Retire every outstanding LDS read, holding the consumers of all N fragments below it.
template <int N>
__device__ __forceinline__ void tr_wait_all(bf16x8_t (&f)[N]) {
  static_assert(N % 4 == 0, "groups of four");
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3])::"memory");
#pragma unroll
  for (int j = 4; j < N; j += 4) pin4(f[j], f[j + 1], f[j + 2], f[j + 3]);
}
__device__ __forceinline__ float max16(const floatx16_t& a) {
  const float m0 = fmaxf(fmaxf(a[0], a[1]), a[2]), m1 = fmaxf(fmaxf(a[3], a[4]), a[5]);
  const float m2 = fmaxf(fmaxf(a[6], a[7]), a[8]), m3 = fmaxf(fmaxf(a[9], a[10]), a[11]);
  const float m4 = fmaxf(fmaxf(a[12], a[13]), a[14]);
  return fmaxf(fmaxf(fmaxf(m0, m1), m2), fmaxf(fmaxf(m3, m4), a[15]));
}
// Retire outstanding LDS reads; the fragments are in/out operands so no consumer can
// be scheduled above the wait.
__device__ __forceinline__ void tr_wait(bf16x8_t& a, bf16x8_t& b, bf16x8_t& c, bf16x8_t& d) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}
// End of a tile step: this wave's LDS-DMA writes have landed, then the workgroup syncs.
__device__ __forceinline__ void tile_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// Accumulator registers 8s..8s+7 as a bf16 MFMA operand: one v_cvt_pk_bf16_f32 per
// pair (an element-wise cast after a select made hipcc emit one cvt per element plus
// a v_perm per pair).
typedef float floatx8_t __attribute__((ext_vector_type(8)));
// HK = 1 (fp16 activations): the same registers as fp16 (RNE), kept in the bf16x8_t
// container type -- fragments are raw 16-byte operands; only mfma<HK> reads their format.
template <int HK = 0>
__device__ __forceinline__ bf16x8_t acc_frag(const floatx16_t& acc, int s) {
  const floatx8_t f = s ? acc.s89abcdef : acc.s01234567;
  if constexpr (HK == 0) return __builtin_convertvector(f, bf16x8_t);
  else return __builtin_bit_cast(bf16x8_t, __builtin_convertvector(f, f16x8_t));
}
// element j of a 16-bit fragment as float
template <int HK>
__device__ __forceinline__ float frag_f(const bf16x8_t& v, int j) {
  if constexpr (HK == 0) return (float)v[j];
  else return (float)__builtin_bit_cast(f16x8_t, v)[j];
}

// Dropout select on the fp32 bit pattern: all-ones / all-zeros from keep bit `bit` of
// `word` (v_bfe_i32), then one AND -- 2 VALU per element instead of and + cmp +
// cndmask.  A dropped element becomes +0.0f.
__device__ __forceinline__ uint32_t keep_ones(uint32_t word, int bit) {
  uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)word, bit, 1);
  // Empty asm (no instruction, so nothing for the hazard recognizer to miss): hides
  // that m is 0 / ~0, which stops LLVM from rewriting bfe + and as and + cmp + cndmask.
  asm("" : "+v"(m));
  return m;
}
__device__ __forceinline__ float keep_and(float x, uint32_t ones) {
#ifdef DLT_ATTN_NOSEL  // diagnostic upper bound only (tools/ab): drops nothing, wrong numerics
  return x;
#endif
  return __uint_as_float(__float_as_uint(x) & ones);
}

template <int HK = 0>
__device__ __forceinline__ floatx16_t mfma(const bf16x8_t& a, const bf16x8_t& b, const floatx16_t& c) {
  if constexpr (HK == 0) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0,
                                                  0, 0);
}

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Attention-score soft-capping (the CAP kernels, attention_cap.hip): the raw product s = q.k
// becomes t = tanh(scale s / cap), in loss.hip's formulation for the final cap:
//   a = exp2(-|s| cap_k), cap_k = 2 log2(e) scale / cap  (= e^(-2|x|/cap), in (0, 1])
//   r = 1 / (1 + a),  t = copysign((1 - a) r, s),  1 - t^2 = 4 a r^2.
// Nothing overflows: |s| -> inf gives a = 0, t = +-1 and a derivative of exactly 0, and the
// derivative is a product, never 1 - t*t (which cancels where the cap bites).
__device__ __forceinline__ float cap_tanh(float s, float cap_k, float& dt2) {
  const float a = fast_exp2(-fabsf(s) * cap_k);
  const float r = __builtin_amdgcn_rcpf(1.f + a);
  dt2 = 4.f * a * r * r;
  return copysignf((1.f - a) * r, s);
}
__device__ __forceinline__ float cap_tanh(float s, float cap_k) {
  const float a = fast_exp2(-fabsf(s) * cap_k);
  return copysignf((1.f - a) * __builtin_amdgcn_rcpf(1.f + a), s);
}

// row (within a 32x32 tile) of accumulator register i for lane-half h
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

__device__ __forceinline__ floatx16_t zero16() {
  floatx16_t z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// Direct global->LDS tile copy (global_load_lds_dwordx4, no staging registers): one
// wave-instruction writes 1 KiB = 1024 / (2D) rows contiguously (lane l -> row
// l / (D/8), 16-B slot l % (D/8)), so the XOR swizzle is applied on the SOURCE
// address: slot s of row r holds global chunk s ^ swz_x(r), exactly the image
// swz_off() reads.  64 rows = 8 (D = 64) or 16 (D = 128) instructions, split over the
// 2 waves.  Completion is tracked by vmcnt; the __syncthreads() that ends every tile
// step waits for it.
typedef __attribute__((address_space(3))) void* lds_vptr_t;
typedef const __attribute__((address_space(1))) void* gbl_cvptr_t;
template <int D>
__device__ __forceinline__ void glds_tile(const bf16_t* __restrict__ base, int row0, int S, int rstride, bf16_t* T,
                                          int wid, int lane) {
  // 32-bit offsets (a head's rows span < 4 GB) on the wave-uniform base: the DMA takes
  // the saddr form and no 64-bit address arithmetic runs per tile (fwd / dQ).
  constexpr int CPR = D / 8, RPI = 64 / CPR, NI = 32 / RPI;  // chunks / row, rows / instr, instr / wave
  const char* b = reinterpret_cast<const char*>(base);
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int rr = (wid * NI + j) * RPI;  // first row of this 1 KiB piece (wave-uniform)
    const int row = rr + lane / CPR;
    const int c = (lane % CPR) ^ swz_x<D>(row);
    const uint32_t off = (uint32_t)(min(row0 + row, S - 1) * rstride + c * 8) * 2u;
    __builtin_amdgcn_global_load_lds((gbl_cvptr_t)(b + off), (lds_vptr_t)(T + rr * D), 16, 0, 0);
  }
}
// The same copy with 64-bit row addressing: fewer live registers in dK/dV, which stages
// two operands with different row strides and sits at the VGPR limit.
template <int D>
__device__ __forceinline__ void glds_tile64(const bf16_t* __restrict__ base, int row0, int S, int rstride, bf16_t* T,
                                            int wid, int lane) {
  constexpr int CPR = D / 8, RPI = 64 / CPR, NI = 32 / RPI;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int rr = (wid * NI + j) * RPI;
    const int row = rr + lane / CPR;
    const int c = (lane % CPR) ^ swz_x<D>(row);
    const bf16_t* g = base + (size_t)min(row0 + row, S - 1) * rstride + c * 8;
    __builtin_amdgcn_global_load_lds((gbl_cvptr_t)g, (lds_vptr_t)(T + rr * D), 16, 0, 0);
  }
}

__device__ __forceinline__ bf16x8_t load_row8(const bf16_t* __restrict__ p, bool ok) {
  bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(p);
  if (!ok) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.f;
  }
  return v;
}

// ============================================================================ work map
// The MFMA kernels run a 1-D grid of (head, item-pair) work items.  The dispatcher deals
// consecutive workgroup ids round-robin to the 8 XCDs, each with its own 4 MB L2; with
// the natural order (pair fastest) XCD x would get pair x of EVERY head, so no two
// workgroups on an XCD share a K/V (fwd, dQ) or Q/dO (dK/dV) stream and every tile is
// fetched once per pair from the fabric.  The XCD-aware map gives each XCD a contiguous
// range of items instead -- all pairs of a head on one XCD, reading the head's tiles
// through the same L2 (bijective for any grid size, like the GEMM's tile map).
__device__ __forceinline__ bool work_item(int nrb, int sched, int& bh, int& pair) {
  const int bid = blockIdx.x;
  if (sched & 2) {
    // LPT: one 64-row item per workgroup, longest first (block ids ascend in dispatch
    // order), so short items fill the slots the long ones leave -- many more, shorter
    // waves than the pairing.  bid % 8 == bh % 8 when B*nh % 8 == 0: a head stays on
    // one XCD (its K/V or Q/dO tiles through one L2).
    const int BH = gridDim.x / nrb;
    pair = bid / BH;  // rank: 0 = longest item
    bh = bid - pair * BH;
    return true;
  }
  const int npairs = (nrb + 1) / 2;
  int wg = bid;
  if (sched & 1) {
    const int nwg = gridDim.x, xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
    wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  }
  bh = wg / npairs;
  pair = wg - bh * npairs;
  return false;
}

// ============================================================================ forward
// Cross-half (lane i <-> i^32) exchange without LDS: v_permlane32_swap (CDNA4).
__device__ __forceinline__ float xhalf_max(float x) {
  const uint32_t u = __float_as_uint(x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_sum(float x) {
  const uint32_t u = __float_as_uint(x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// 16-byte row stores from the split-lane accumulator layout.  Lane (row, h) holds dims
// 32dt + 8g + 4h + [0, 4) (w[dt][g], 4 bf16 = 2 dwords).  One v_permlane32_swap of the
// (g = 2m, 2m + 1) pair -- own g = 2m stays in the low lanes' vdst, the high lanes' g = 2m
// lands there; own g = 2m + 1 stays in the high lanes' vsrc -- leaves lane h holding
// dims 16m + 8h + [0, 8): 4 dwordx4 stores per row instead of 8 dwordx2 (the epilogue's
// store issue is the tail of every work item).
template <int D>
__device__ __forceinline__ void store_row16(bf16_t* __restrict__ row, const uint2 (&w)[D / 32][4], int h) {
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const auto rx = __builtin_amdgcn_permlane32_swap(w[dt][2 * m].x, w[dt][2 * m + 1].x, false, false);
      const auto ry = __builtin_amdgcn_permlane32_swap(w[dt][2 * m].y, w[dt][2 * m + 1].y, false, false);
      *reinterpret_cast<uint4*>(row + 32 * dt + 16 * m + 8 * h) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
    }
}

// Rescale threshold (log2 units): the running max is only moved when some row's max
// grew by more than 2^RESCALE_LOG2 (P is then bounded by 2^8 = 256 instead of 1,
// exact in fp32 l/O and the same relative bf16 precision for P).  Almost every
// rescale after a row's first tile is skipped.
#define RESCALE_LOG2 8.0f
// Running max of a row that has seen no live key yet.  Causal-only rows meet key 0 in
// their first tile, so -inf never survives it.  Under a document mask the later rows
// of an item can have whole leading tiles masked; with m = -inf such a tile gives
// mx - m = -inf - -inf = NaN (and exp2(-inf * c + inf) = NaN).  The DOC kernels start
// from this finite value instead: a dead tile leaves m alone and adds p = exp2(-inf) = 0
// to l and O, and the first live tile rescales by alpha = exp2(-huge) = 0 exactly as
// from -inf, so trivial bounds reproduce the causal kernel bit for bit.
#define M_DEAD (-1e30f)

template <int D>
struct FwdState {
  floatx16_t o[D / 32];
  float m, l;  // running max (raw score units) and per-lane partial row sum
};

template <bool MASK, bool DROP, int HK, int D, bool DOC = false, bool CAP = false>
__device__ __forceinline__ void fwd_tile(FwdState<D>& fs, const bf16_t* Kt, const bf16_t* Vt,
                                         const bf16x8_t (&qf)[D / 16], int k0, int qa, int S, int lane, float c_log2,
                                         uint2 mw, int lo = 0, float cap_k = 0.f) {
  // One 64-key tile as ONE online-softmax step: S = K.Q^T of both 32-key halves first
  // (two independent MFMA chains), one row max / rescale decision for the tile, then
  // per half exp -> dropout -> P.V; the second half's softmax VALU runs while the
  // first half's P.V MFMAs execute.  The row sum uses two partial sums (the single
  // running sum was a 16-deep dependent add chain per half).
  const int h = lane >> 5, ql = lane & 31;
  // keep-bit words of this tile (prefetched with the previous tile's staging loads,
  // so no vmcnt wait lands inside the tile); this lane-half's 16 bits per half-tile
  // sit at (i&3) + 8(i>>2)
  const uint32_t words[2] = {mw.x >> (4 * h), mw.y >> (4 * h)};
  constexpr int NS = D / 16;  // 16-dim contraction steps of S = K.Q^T
  floatx16_t sacc[2];
  {
    bf16x8_t kf[2][NS];
#if DLT_ATTN_KREAD_ASM
    // all K fragments of the tile in flight at once, one counted wait per half
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
#else
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      kf[0][s] = lds_row8<D>(Kt, ql, 16 * s + 8 * h);
      kf[1][s] = lds_row8<D>(Kt, 32 + ql, 16 * s + 8 * h);
    }
    sacc[0] = zero16();
    sacc[1] = zero16();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      sacc[0] = mfma<HK>(kf[0][s], qf[s], sacc[0]);
      sacc[1] = mfma<HK>(kf[1][s], qf[s], sacc[1]);
    }
#endif
  }
  if constexpr (CAP) {  // s -> t = tanh(scale s / cap) in place; c_log2 is cap * log2(e), so m, l and lse
                        // below are those of the capped scores; masked keys go to -inf after, never -cap
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[t][i] = cap_tanh(sacc[t][i], cap_k);
  }
  if (MASK) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ka = k0 + 32 * t + acc_row(i, h);
        sacc[t][i] = (ka > qa || ka >= S || (DOC && ka < lo)) ? -INFINITY : sacc[t][i];
      }
  }
  // row max as a depth-3 max3 tree per half (a linear fmaxf chain is 9 dependent ops)
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
      if (DROP) sacc[t][i] = keep_and(p, keep_ones(words[t], (i & 3) + 8 * (i >> 2)));  // 1/(1-p) at the end
      else sacc[t][i] = p;
    }
    if constexpr (D == 64) {
      tr_wait(vf[0][0], vf[0][1], vf[1][0], vf[1][1]);
    } else {
      tr_wait(vf[0][0], vf[0][1], vf[0][2], vf[0][3]);
      pin4(vf[1][0], vf[1][1], vf[1][2], vf[1][3]);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const bf16x8_t pb = acc_frag<HK>(sacc[t], kk);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) fs.o[dt] = mfma<HK>(vf[kk][dt], pb, fs.o[dt]);
    }
  }
  fs.l += l0 + l1;
}

// Work decomposition (causal balance): a workgroup = 2 waves = one 64-query item.
// Default schedule (work_item, LPT): one item per workgroup, longest first, so the
// short items fill in behind the long ones.  Alternative (DLT_ATTN_SCHED=pair): each
// workgroup processes the PAIR of items (nrb-1-p, p), equal work per workgroup but
// only ~1.5 long waves per SIMD -- a half-empty last round at 2 waves/SIMD (PMC:
// ~1.1 resident waves per SIMD on average at B16).  Round 1 measured one item per
// workgroup in the NATURAL order 1.8x slower than the pairing (equal-length items
// stacked on a CU); longest-first does not stack them.
// Forward diagnostics (tools/cpp/attn_fwd_timing.cpp, -DDLT_ATTN_FWD_TIMING only): per
// wave, the shader cycles inside the tile compute and inside the per-tile DMA wait +
// barrier, and the tile count, written by lane 0 with vector stores.
#ifdef DLT_ATTN_FWD_TIMING
extern __device__ unsigned long long* g_attn_ftim;  // defined in attention.hip
#define FWD_T(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#define FWD_ACC(c, w) (f_comp += (c), f_wait += (w), ++f_tiles)
#else
#define FWD_T(v) ((void)0)
#define FWD_ACC(c, w) ((void)0)
#endif

// DOC tile range of the 64-query item qb (fwd, dQ).  lo is non-decreasing, so the
// item's smallest / largest bound are those of its first / last valid query: two
// workgroup-uniform loads, no reduction.  ks = first K/V tile any row needs, kdoc =
// first tile at or above every row's bound; both clamped into the causal range
// [0, qb], so the loop stays inside the sequence whatever the arrays hold.
__device__ __forceinline__ void doc_q_range(const int* __restrict__ lrow, int qb, int S, int& ks, int& kdoc) {
  const int lo_min = lrow[qb * RB], lo_max = lrow[min(S, qb * RB + RB) - 1];
  ks = min(max(lo_min, 0) / KVB, qb);
  kdoc = min((max(lo_max, 0) + KVB - 1) / KVB, qb);
}
// The mirror image for the 64-key item kblk of dK/dV: hi of its first / last valid key.
// nqe = end of the query-tile loop (the tile after the one holding the largest hi),
// t_unm = first tile that reaches past the smallest hi; clamped to (kblk, nqt].
__device__ __forceinline__ void doc_k_range(const int* __restrict__ hrow, int kblk, int S, int nqt, int& nqe,
                                            int& t_unm) {
  const int hi_min = hrow[kblk * RB], hi_max = hrow[min(S, kblk * RB + RB) - 1];
  nqe = min(max(hi_max / QSTEP, kblk) + 1, nqt);
  t_unm = min(max(hi_min + 1, 0) / QSTEP, S / QSTEP);
}

// D = 128 doubles the O accumulators and Q / K / V fragments: 256 VGPRs would spill,
// so its instantiation may take the whole 512-register file (one wave per SIMD).
#define ATTN_WAVES(D) __attribute__((amdgpu_waves_per_eu(D == 64 ? 2 : 1, 2)))
// ============================================================================ launch arguments
#include <cstdlib>
// head_dim dispatch: HDC = 64 or 128 inside the body
#define DLT_HD_DISPATCH(hd, ...) \
  do {                           \
    if ((hd) == 128) {           \
      constexpr int HDC = 128;   \
      __VA_ARGS__;               \
    } else {                     \
      constexpr int HDC = 64;    \
      __VA_ARGS__;               \
    }                            \
  } while (0)
static inline bool attn_hd_ok(int hd) { return hd == 64 || hd == 128; }
// boolean dispatch: defines `constexpr bool NAME` = (cond) inside the body
#define DLT_BOOL_DISPATCH(NAME, cond, ...) \
  do {                                     \
    if (cond) {                            \
      constexpr bool NAME = true;          \
      __VA_ARGS__;                         \
    } else {                               \
      constexpr bool NAME = false;         \
      __VA_ARGS__;                         \
    }                                      \
  } while (0)
// XCD-aware work map on by default; DLT_ATTN_XCD=0 restores the natural order (A/B).
static inline int xcd_map_enabled() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("DLT_ATTN_XCD");
    v = (e && atoi(e) == 0) ? 0 : 1;
    // default: one item per workgroup, longest first (see work_item; measured B8 nh12
    // S1024: fwd 63 -> 60 us incl. the keep bits, bwd 108 -> 96 us; B16: 117 -> 105,
    // 218 -> 197); DLT_ATTN_SCHED=pair restores the paired items
    const char* sch = getenv("DLT_ATTN_SCHED");
    if (!(sch && sch[0] == 'p')) v |= 2;
  }
  return v;
}
// grid of the MFMA kernels for a work schedule
static inline int attn_grid(int nrb, int BH, int sched) { return (sched & 2) ? nrb * BH : ((nrb + 1) / 2) * BH; }
// One tensor's layout: element (b, head, row, d) lives at base + b*b + head*h + row*r + d.
// Head-major [B*nh, S, hd]: {nh*S*hd, S*hd, hd}; inside the packed [B*S, 3H] QKV GEMM
// output: {S*3H, hd, 3H} with k, v = q + H, q + 2H.
struct dlt_attn_stride {
  long b;
  int h, r;
};
// Arguments of dlt_attn_fwd and dlt_attn_bwd; the forward ignores the backward's fields.
struct dlt_attn_args {
  const bf16_t *q, *k, *v;
  bf16_t* o;    // [B*S, nh*hd]: written by the forward, read by the backward
  float* lse;   // [B, nh, S], per query head
  // uint32 [2][B*nh, ceil(S/32), S] keep bits, needed when thr != 0 -- [0] row layout
  // (lane = query), [1] transposed (lane = key), see k_dropout_bits; per query head
  uint32_t* mask;
  const bf16_t* dout;
  float* delta_ws;  // [B, nh, S] workspace: rowsum(dO * O), written by dQ for dK/dV
  bf16_t *dq, *dk, *dv;
  // document mask's bounds, int32 [B, S]; null = causal only.  The forward and dQ read lo,
  // dK/dV reads hi: the backward takes both or neither
  const int *lo, *hi;
  // [>= S, 32] fp32, both or neither: the backward applies the inverse RoPE rotation to dq
  // and dk in the store (the gradient w.r.t. the pre-rotation q/k of the packed QKV)
  const float *cosT, *sinT;
  int B, nh;
  // 0: the MHA kernels.  > 0: the GQA kernels (also for nkv == nh) -- k / v, dk / dv hold nkv
  // heads (nkv divides nh; query head h reads kv head h / (nh / nkv)) with the kv / dkv
  // strides, which the MHA kernels do not read (k, v follow q's strides, dk, dv follow dq's)
  int nkv;
  int S, hd, hk;
  float scale, dscale;
  uint32_t key, thr;  // thr != 0: dropout on
  int gen_mask;       // forward; 0: the keep bits are already in `mask` (dlt_attn_dropout_mask)
  // attention-score soft-capping: scores = softcap * tanh(scale q.k / softcap) before the masks
  // (the CAP kernels, attention_cap.hip); 0 = off.  It fills the alignment hole before `stride`
  float softcap;
  struct {
    dlt_attn_stride q, kv, dq, dkv;
  } stride;
  // attention sinks, fp32 [nh] (one logit per query head); null = none.  The forward reads
  // sink (the SINK kernels); the backward takes both or neither and adds into dsink
  // (k_attn_sink_bwd, after dQ has written delta_ws)
  const float* sink;
  float* dsink;
};
// ops/hip.py mirrors the struct field by field: a field added on one side only must not load
static_assert(sizeof(dlt_attn_args) == 248, "dlt_attn_args changed: update _AttnArgs in ops/hip.py");
static inline bool attn_stride_ok(const dlt_attn_stride& s, int m) { return !(s.r % m || s.h % m || s.b % m); }

// attention_cap.hip: launch the CAP forms (a->softcap > 0) after dlt_attn_fwd's / dlt_attn_bwd's
// argument checks and keep-bit generation.  The forward covers a->sink too; the backward leaves
// the sink gradient (k_attn_sink_bwd, unchanged by the cap) to dlt_attn_bwd.
int attn_fwd_cap_launch(const dlt_attn_args* a, hipStream_t st);
int attn_bwd_cap_launch(const dlt_attn_args* a, hipStream_t st);
// attention_sink.hip: launches the SINK form of the forward (a->sink set) after dlt_attn_fwd's
// argument checks and keep-bit generation
int attn_fwd_sink_launch(const dlt_attn_args* a, hipStream_t st);
