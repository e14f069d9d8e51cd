// 64-granular MFMA GEMM (gfx950 / MI355X) for the projection shapes no other hand-written
// kernel tiles: hidden sizes that are an odd multiple of 64 (gpt2_xl: H = 1600 = 25 x 64).
//   TN (forward):        C[M, N]     = A[M, K] . B[N, K]^T       (both operands K-contiguous)
//   NN (data gradient):  dX[M, Nout] = dY[M, Nred] . W[Nred, Nout]   (W read as stored)
// bf16 or IEEE half, fp32 accumulate, one rounding to the operand format.
// Shapes: M % 256 == 0, output columns % 64 == 0, reduction % 64 == 0 and >= 128; contiguous.
//
// Tiles.  256 rows x 128 columns (main form) and 256 x 64 (tail form, compile-time: half the
// B image, half the n-tiles) in ONE launch: a width of 128 a + 64 is covered by a main tiles
// and one tail tile per row tile, so no tile reads or stores past column N.  The main tiles
// come first in the tile list and the half-work tail tiles last (they fill the end of the
// last round).  A workgroup walks tiles b, b + G, ... (grid G <= 256, one workgroup per CU).
// 512 threads = 8 waves as 4 (M) x 2 (N): a wave owns 64 x BN/2 outputs = 4 x NT tiles of
// v_mfma_f32_16x16x32_{bf16,f16} (NT = 4 main, 2 tail).
//
// K loop.  BK = 64, a RING of three LDS stages (A 256 x 64 + B BN x 64 per stage, 48 KB)
// addressed by a running stage index, so an odd number of K-tiles (1600 = 25 x 64) costs no
// padded tile and no tail loop -- nothing in the loop depends on the parity of the count.
// Per K-tile a wave issues 4 (A) + BN/64 (B) global_load_lds_dwordx4 pieces; iteration kt
//   s_waitcnt vmcnt(L)   K-tile kt has landed, K-tile kt + 1 (L pieces) stays in flight
//   s_barrier            everyone's pieces of kt landed; everyone finished reading kt - 1
//   issue K-tile kt + 2 into the stage K-tile kt - 1 was read from
//   read both k-steps' fragments, s_waitcnt lgkmcnt(n1) (k-step 0 there, the n1 reads of
//   k-step 1 in flight), 4 x NT MFMA, s_waitcnt lgkmcnt(0), 4 x NT MFMA
// The last K-tile is peeled behind the loop: only there is nothing left in flight.
//
// LDS images.  K-major operands (A, TN's B): 128-byte rows, 16-byte chunk c of row r stored
// at chunk c ^ ((r >> 1) & 7) (source-side swizzle of the LDS-DMA; conflict-free
// ds_read_b128 of 16 rows x one chunk).  NN's B: reduction-major image (64 reduction rows x
// BN columns, 256- / 128-byte rows) with the chunk swizzle of gemm_common.h, read with
// ds_read_b64_tr_b16 (gw_frag), as k_gemm_wgrad and k_gemm_bf16<BT> read theirs.
//
// Epilogue.  Swapped product D = B_tile . A_tile^T: a lane owns one output row and 4
// consecutive columns per 16 x 16 tile; v_permlane16_swap regroups two neighbouring n-tiles
// into 8 consecutive columns, so every lane stores 16 bytes.
// No split-K and no atomics: one workgroup computes a tile whole, in a fixed order.
#include "common.h"
#include "gemm_common.h"

namespace {

constexpr int R6_BM = 256;
constexpr int R6_BK = 64;
constexpr int R6_BN = 128;    // main column tile
constexpr int R6_TAIL = 64;   // tail column tile
constexpr int R6_STAGES = 3;
constexpr int R6_IMG_A = R6_BM * R6_BK;            // elements
constexpr int R6_STAGE = R6_IMG_A + R6_BN * R6_BK;  // A image + the (main-sized) B image
constexpr int R6_MAX_GRID = 256;                    // one workgroup per CU

// element offset of logical 16-byte chunk `chunk` of row `row` in a K-major image
__device__ __forceinline__ int r6_swz(int row, int chunk) { return row * R6_BK + ((chunk ^ ((row >> 1) & 7)) << 3); }

// One 16-byte-per-lane LDS-DMA piece (64 lanes fill 1 KB at `lds`), issued from inline asm so
// that the K loop's own counted s_waitcnt are the only vmcnt waits on it.
__device__ __forceinline__ void r6_dma(const void* g, const void* lds) {
  const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds);
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(m0) : "memory", "m0");
}

typedef __bf16 r6_bf16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 r6_f16x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t r6_u32x4_t __attribute__((ext_vector_type(4)));
// 4 fp32 -> 4 values of the operand format, round to nearest even
template <int HK>
__device__ __forceinline__ uint2 r6_pack(const floatx4_t& v) {
  if constexpr (HK == 0) return __builtin_bit_cast(uint2, __builtin_convertvector(v, r6_bf16x4_t));
  else return __builtin_bit_cast(uint2, __builtin_convertvector(v, r6_f16x4_t));
}

// NN: the A fragments are read from asm too (row offset in the immediate), so that every LDS
// read of the form is invisible to the compiler and the K loop's counted waits are the only
// lgkmcnt waits (a visible read next to the asm transposed reads made the compiler wait for
// all but its own younger reads, i.e. for most of k-step 1, before k-step 0's MFMAs)
template <int OFF>
__device__ __forceinline__ bf16x8_t r6_lds128(uint32_t addr) {
  bf16x8_t r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}

// s_waitcnt lgkmcnt(CNT) that the k-step's fragments depend on: the transposed reads are asm
// and invisible to the compiler's own counting, so no MFMA may be scheduled above the wait
template <int CNT, int NT>
__device__ __forceinline__ void r6_wait_frags(bf16x8_t (&fa)[4], bf16x8_t (&fb)[NT]) {
  static_assert(NT == 4 || NT == 2, "main or tail form");
  if constexpr (NT == 4)
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(fa[0]), "+v"(fa[1]), "+v"(fa[2]), "+v"(fa[3]), "+v"(fb[0]), "+v"(fb[1]), "+v"(fb[2]), "+v"(fb[3])
                 : "n"(CNT)
                 : "memory");
  else
    asm volatile("s_waitcnt lgkmcnt(%6)"
                 : "+v"(fa[0]), "+v"(fa[1]), "+v"(fa[2]), "+v"(fa[3]), "+v"(fb[0]), "+v"(fb[1])
                 : "n"(CNT)
                 : "memory");
}

template <int L>
__device__ __forceinline__ void r6_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L) : "memory");
}

// One 256 x BN output tile at (m0, n0).  A: [M, K] rows of K; B: TN [N, K], NN [K, N]; C [M, N].
template <int BN, bool NN, int HK>
__device__ __forceinline__ void r6_tile(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                                        bf16_t* __restrict__ C, int N, int K, int m0, int n0, bf16_t* lds) {
  constexpr int NT = BN / 32;       // 16-column n-tiles per wave
  constexpr int NB = BN / 64;       // B pieces per wave and K-tile
  constexpr int L = 4 + NB;         // LDS-DMA pieces per wave and K-tile
  constexpr int ROWB = BN * 2;      // NN: bytes per reduction row of the B image
  constexpr int N1 = 4 + (NN ? 2 * NT : NT);  // LDS reads of one k-step
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wid & 3, wn = wid >> 2;
  const int l16 = lane & 15, lq = lane >> 4;
  const int lda = K, ldb = NN ? N : K;

  const bf16_t* const Ab = A + (size_t)m0 * lda;
  const bf16_t* const Bb = NN ? B + n0 : B + (size_t)n0 * ldb;

  // per-lane source byte offsets of the wave's pieces (relative to the K-tile's first element)
  uint32_t oa[4], ob[NB];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (wid * 4 + j) * 8 + (lane >> 3);
    oa[j] = (uint32_t)(row * lda + (((lane & 7) ^ ((row >> 1) & 7)) << 3)) * 2u;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    if constexpr (NN) {
      // piece element e = 16-byte chunk pc of reduction row t; source chunk lc = pc ^ 2 v(t)
      constexpr int CPR = BN / 8;
      const int e = (wid * NB + j) * 64 + lane;
      const int t = e / CPR;
      const int lc = (e % CPR) ^ (2 * (ROWB == 256 ? gw_v256(t) : gw_v128(t)));
      ob[j] = (uint32_t)(t * ldb + lc * 8) * 2u;
    } else {
      const int row = (wid * NB + j) * 8 + (lane >> 3);
      ob[j] = (uint32_t)(row * ldb + (((lane & 7) ^ ((row >> 1) & 7)) << 3)) * 2u;
    }
  }
  auto issue = [&](int kt, int stage) {
    bf16_t* const sa = lds + stage * R6_STAGE;
    bf16_t* const sb = sa + R6_IMG_A;
    const char* const ga = (const char*)(Ab + (size_t)kt * R6_BK);
    const char* const gb = (const char*)(NN ? Bb + (size_t)kt * R6_BK * ldb : Bb + (size_t)kt * R6_BK);
#pragma unroll
    for (int j = 0; j < 4; ++j) r6_dma(ga + oa[j], sa + (wid * 4 + j) * 512);
#pragma unroll
    for (int j = 0; j < NB; ++j) r6_dma(gb + ob[j], sb + (wid * NB + j) * 512);
  };

  // fragment addresses: row of the lane in the wave's A / B rows; NN: transposed-read bases
  const int arow = wm * 64 + l16;
  // (the swizzle of row arow + 16 mt does not depend on mt: one byte offset per k-step)
  const uint32_t ab[2] = {(uint32_t)r6_swz(arow, lq) * 2u, (uint32_t)r6_swz(arow, 4 + lq) * 2u};
  const int brow = wn * (BN / 2) + l16;
  uint32_t kb[NT];
  if constexpr (NN) {
    GwLane<ROWB> ln;
    ln.init(lane);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) kb[nt] = ln.base + ln.koff(NT * wn + nt);
  }

  floatx4_t acc[NT][4];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = floatx4_t{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int stage) {
    const bf16_t* const sa = lds + stage * R6_STAGE;
    const bf16_t* const sb = sa + R6_IMG_A;
    bf16x8_t fa[2][4], fb[2][NT];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        if constexpr (NN) {
          const uint32_t a = (uint32_t)(uintptr_t)sa + ab[s];
          fa[s][mt] = mt == 0 ? r6_lds128<0>(a) : mt == 1 ? r6_lds128<2048>(a) : mt == 2 ? r6_lds128<4096>(a) : r6_lds128<6144>(a);
        } else {
          fa[s][mt] = *reinterpret_cast<const bf16x8_t*>(sa + r6_swz(arow + mt * 16, s * 4 + lq));
        }
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if constexpr (NN)
          fb[s][nt] = gw_frag<ROWB>((uint32_t)(uintptr_t)sb + kb[nt], s);
        else
          fb[s][nt] = *reinterpret_cast<const bf16x8_t*>(sb + r6_swz(brow + nt * 16, s * 4 + lq));
      }
      __builtin_amdgcn_sched_barrier(0);  // k-step 0's reads are older than k-step 1's
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s == 0) r6_wait_frags<N1, NT>(fa[0], fb[0]);
      else r6_wait_frags<0, NT>(fa[1], fb[1]);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = gw_mfma<HK>(fb[s][nt], fa[s][mt], acc[nt][mt]);
      __builtin_amdgcn_s_setprio(0);
    }
  };

  const int nk = K / R6_BK;  // >= 2, odd or even
  // every wave has finished reading the previous tile's last stage before it is restaged
  __builtin_amdgcn_s_barrier();
  issue(0, 0);
  issue(1, 1);
  int cur = 0;
  for (int kt = 0; kt < nk - 1; ++kt) {
    r6_wait_vm<L>();
    __builtin_amdgcn_s_barrier();
    if (kt + 2 < nk) issue(kt + 2, cur == 0 ? 2 : cur - 1);
    compute(cur);
    cur = cur == R6_STAGES - 1 ? 0 : cur + 1;
  }
  r6_wait_vm<0>();
  __builtin_amdgcn_s_barrier();
  compute(cur);

  // acc[nt][mt] = D[n][m]: the lane owns row wm*64 + mt*16 + l16 and columns (n-tile nt) +
  // lq*4 .. +3.  permlane16_swap over the n-tile pair (2p, 2p + 1): lanes with lq even end
  // up with 8 consecutive columns of n-tile 2p, lq odd of 2p + 1.
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int row = m0 + wm * 64 + mt * 16 + l16;
    bf16_t* const crow = C + (size_t)row * N + n0 + wn * (BN / 2);
    uint2 pk[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) pk[t] = r6_pack<HK>(acc[t][mt]);
#pragma unroll
    for (int p = 0; p < NT / 2; ++p) {
      uint32_t x[2] = {pk[2 * p].x, pk[2 * p].y}, y[2] = {pk[2 * p + 1].x, pk[2 * p + 1].y};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        auto sw = __builtin_amdgcn_permlane16_swap(x[h], y[h], false, false);
        x[h] = sw[0];
        y[h] = sw[1];
      }
      const int col = (2 * p + (lq & 1)) * 16 + (lq >> 1) * 8;
      *reinterpret_cast<r6_u32x4_t*>(crow + col) = r6_u32x4_t{x[0], x[1], y[0], y[1]};
    }
  }
}

}  // namespace

template <bool NN, int HK>
__global__ __launch_bounds__(512) void k_gemm_r64(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                                                  bf16_t* __restrict__ C, int M, int N, int K) {
  __shared__ __attribute__((aligned(1024))) bf16_t lds[R6_STAGES * R6_STAGE];
  const int ntm = M / R6_BM, nmain = N / R6_BN;
  const int main_tiles = ntm * nmain;
  const int ntiles = main_tiles + ((N % R6_BN) ? ntm : 0);
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    if (t < main_tiles)
      r6_tile<R6_BN, NN, HK>(A, B, C, N, K, (t / nmain) * R6_BM, (t % nmain) * R6_BN, lds);
    else
      r6_tile<R6_TAIL, NN, HK>(A, B, C, N, K, (t - main_tiles) * R6_BM, nmain * R6_BN, lds);
  }
}

// N: output columns, K: reduction.  grid: workgroups (0 = one per tile up to one per CU).
template <bool NN>
static int r6_launch(const bf16_t* A, const bf16_t* B, bf16_t* C, int M, int N, int K, int grid, int hk,
                     hipStream_t st) {
  if (M <= 0 || N <= 0 || M % R6_BM || N % 64 || K % R6_BK || K < 2 * R6_BK || (hk != 0 && hk != 1) || grid < 0)
    return -1;
  const int ntiles = (M / R6_BM) * ((N + R6_BN - 1) / R6_BN);
  int g = ntiles < R6_MAX_GRID ? ntiles : R6_MAX_GRID;
  if (grid > 0 && grid < g) g = grid;
  DLT_HK_DISPATCH(hk, k_gemm_r64<NN, HKC><<<g, 512, 0, st>>>(A, B, C, M, N, K));
  DLT_CHECK_LAUNCH();
}

// C[M, N] = A[M, K] . B[N, K]^T (hk: 0 bf16, 1 fp16); -1: the shape is refused
DLT_API int dlt_gemm_r64(const bf16_t* A, const bf16_t* B, bf16_t* C, int M, int N, int K, int grid, int hk,
                         hipStream_t st) {
  return r6_launch<false>(A, B, C, M, N, K, grid, hk, st);
}

// dX[M, Nout] = dY[M, Nred] . W[Nred, Nout], W read as stored
DLT_API int dlt_gemm_r64_nn(const bf16_t* dY, const bf16_t* W, bf16_t* dX, int M, int Nout, int Nred, int grid, int hk,
                            hipStream_t st) {
  return r6_launch<true>(dY, W, dX, M, Nout, Nred, grid, hk, st);
}
