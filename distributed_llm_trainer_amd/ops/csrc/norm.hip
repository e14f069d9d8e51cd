// Fused residual-add + dropout + RMSNorm (forward) and its backward.
//
// Replaces the reference's per-block sequence  x + dropout(f(x))  ->  RMSNorm
// (gpt.py:66, 240, 282, 308, 314: pow/mean/add/rsqrt/mul/mul + bernoulli + add =
// ~9 ATen kernels fwd, more bwd) with ONE memory pass each way:
//
//   fwd: x = resid + keep(delta)/(1-p);  y = bf16(x * rsqrt(mean(x^2)+eps) * w)
//   bwd: dx = dres + rstd*(g - xh*mean(g*xh)),  g = dy*w;  ddelta = keep(dx)/(1-p)
//        dw += sum_rows dy*xh
//
// One wave (64 lanes) owns one row; lane l holds the 4-element chunks l, l+64, ...
// in registers (NCH = ceil(H/256) chunks per lane; H = 768 -> exactly 3, every lane
// busy), so each tensor is touched once.  All loads of a row (dy, x, and the incoming
// residual gradient) are issued before the row reduction so their latencies overlap.
// The residual stream is fp32 (matches the reference DDP/autocast numerics, SURVEY
// §2.4 P9).
#include "common.h"
#include <cstdlib>

struct f4 { float v[4]; };

__device__ __forceinline__ f4 ld_f4(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  return f4{{a.x, a.y, a.z, a.w}};
}
__device__ __forceinline__ void st_f4(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <int HK>
__device__ __forceinline__ void ld_h4(const bf16_t* p, float (&v)[4]) {
  const u16x4 d = *reinterpret_cast<const u16x4*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = h2f<HK>(d.v[e]);
}

// Norm weight: fp32 (flat master, DDP path) or 16-bit in the activation format (the
// gathered FSDP unit) -- read in place, so the FSDP path needs no per-call weight upcast.
template <int HK>
__device__ __forceinline__ f4 ld_w4(const void* w, int w16, int off) {
  if (w16) {
    f4 r;
    ld_h4<HK>(reinterpret_cast<const bf16_t*>(w) + off, r.v);
    return r;
  }
  return ld_f4(reinterpret_cast<const float*>(w) + off);
}

__device__ __forceinline__ void st_f4_nt(float* p, const float (&v)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) __builtin_nontemporal_store(v[e], p + e);
}

template <int NCH, bool XNT = false, int HK = 0>
__global__ __launch_bounds__(256) void k_add_dropout_rmsnorm_fwd(
    const float* __restrict__ resid, const bf16_t* __restrict__ delta, const void* __restrict__ w, int wbf16,
    float* __restrict__ x_out, bf16_t* __restrict__ y_out, float* __restrict__ rstd_out,
    int M, int H, float eps, uint32_t key, uint32_t thr, float dscale) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nc = H >> 2;
  const size_t rbase = (size_t)row * H;
  float xv[NCH][4];
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
#pragma unroll
    for (int e = 0; e < 4; ++e) xv[t][e] = 0.f;
    if (c < nc) {
      const size_t off = rbase + (size_t)c * 4;
      if (resid) {
        const f4 r = ld_f4(resid + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[t][e] = r.v[e];
      }
      if (delta) {
        float d[4];
        ld_h4<HK>(delta + off, d);
        if (thr) {
#pragma unroll
          for (int e = 0; e < 4; e += 2) {
            const uint32_t h = lowbias32(key ^ (uint32_t)((off + e) >> 1));
            xv[t][e] += ((h & 0xffffu) >= thr) ? d[e] * dscale : 0.f;
            xv[t][e + 1] += ((h >> 16) >= thr) ? d[e + 1] * dscale : 0.f;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) xv[t][e] += d[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += xv[t][e] * xv[t][e];
    }
  }
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss / (float)H + eps);
  if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
    if (c < nc) {
      const size_t off = rbase + (size_t)c * 4;
      if (x_out) {  // the fp32 block input is read again only by the backward
        if (XNT) st_f4_nt(x_out + off, xv[t]);
        else st_f4(x_out + off, xv[t]);
      }
      const f4 ww = ld_w4<HK>(w, wbf16, c * 4);
      u16x4 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) y.v[e] = f2h<HK>(xv[t][e] * rstd * ww.v[e]);
      *reinterpret_cast<u16x4*>(y_out + off) = y;
    }
  }
}

template <int NCH, int HK = 0>
__global__ __launch_bounds__(256) void k_rmsnorm_bwd(
    const bf16_t* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ rstd_in,
    const void* __restrict__ w, int wbf16, const float* dres, float* dx_out,
    bf16_t* __restrict__ ddelta, float* __restrict__ dw, float* __restrict__ dw_part,
    const float* __restrict__ dy_scale, float dy_mul, int M, int H, uint32_t key, uint32_t thr, float dscale) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [4][H]
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int nc = H >> 2;
  const float sc = (dy_scale ? *dy_scale : 1.f) * dy_mul;
  const float invH = 1.f / (float)H;
  float dwacc[NCH][4];
  float wv[NCH][4];
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
#pragma unroll
    for (int e = 0; e < 4; ++e) { dwacc[t][e] = 0.f; wv[t][e] = 0.f; }
    if (c < nc) {
      const f4 a = ld_w4<HK>(w, wbf16, c * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) wv[t][e] = a.v[e];
    }
  }
  for (int row = blockIdx.x * 4 + wid; row < M; row += gridDim.x * 4) {
    const size_t rbase = (size_t)row * H;
    const float rstd = rstd_in[row];
    float dv[NCH][4], xx[NCH][4], rr[NCH][4];
    // issue every load of the row first
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
      const int c = lane + 64 * t;
#pragma unroll
      for (int e = 0; e < 4; ++e) { dv[t][e] = 0.f; xx[t][e] = 0.f; rr[t][e] = 0.f; }
      if (c < nc) {
        const size_t off = rbase + (size_t)c * 4;
        ld_h4<HK>(dy + off, dv[t]);
        const f4 a = ld_f4(x + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) xx[t][e] = a.v[e];
        if (dres) {
          const f4 r = ld_f4(dres + off);
#pragma unroll
          for (int e = 0; e < 4; ++e) rr[t][e] = r.v[e];
        }
      }
    }
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < NCH; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = dv[t][e] * sc;
        const float xh = xx[t][e] * rstd;
        dwacc[t][e] += d * xh;
        dv[t][e] = d * wv[t][e];  // g
        xx[t][e] = xh;
        dot += dv[t][e] * xh;
      }
    dot = wave_sum(dot) * invH;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
      const int c = lane + 64 * t;
      if (c < nc) {
        const size_t off = rbase + (size_t)c * 4;
        float dx[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) dx[e] = rstd * (dv[t][e] - xx[t][e] * dot) + rr[t][e];
        st_f4(dx_out + off, dx);
        if (ddelta) {
          u16x4 o;
          if (thr) {
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
              const uint32_t h = lowbias32(key ^ (uint32_t)((off + e) >> 1));
              o.v[e] = f2h<HK>(((h & 0xffffu) >= thr) ? dx[e] * dscale : 0.f);
              o.v[e + 1] = f2h<HK>(((h >> 16) >= thr) ? dx[e + 1] * dscale : 0.f);
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o.v[e] = f2h<HK>(dx[e]);
          }
          *reinterpret_cast<u16x4*>(ddelta + off) = o;
        }
      }
    }
  }
  // block-reduce dw over the 4 waves -> this block's partial row (dw_part) or, without
  // a workspace, one atomic per column per block
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
    if (c < nc) {
#pragma unroll
      for (int e = 0; e < 4; ++e) smem[wid * H + c * 4 + e] = dwacc[t][e];
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < H; j += 256) {
    const float s = smem[j] + smem[H + j] + smem[2 * H + j] + smem[3 * H + j];
    if (dw_part) dw_part[(size_t)blockIdx.x * H + j] = s;
    else unsafeAtomicAdd(dw + j, s);
  }
}

// dw[j] += sum over the partial rows, in a fixed order (bitwise reproducible, no
// float atomics).  One 64*QN-thread block per 4*QN columns: thread (g, q) owns columns
// 4q..4q+3 of the slice (float4 loads, QN threads = one row segment) and rows
// g, g+64, ... with 8 loads in flight (the partials were written by blocks on every XCD,
// so the reads come from the fabric: latency-bound without that parallelism); then the
// 64 row-group sums are added through LDS in two fixed-order levels.
__device__ __forceinline__ void f4add(float4& a, const float4 b) {
  a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
}

template <int QN>
__global__ __launch_bounds__(64 * QN) void k_colsum_acc(const float* __restrict__ part, float* __restrict__ dw, int rows,
                                                       int H) {
  constexpr int C = 4 * QN;  // columns per block
  __shared__ float red[64][C + 1];
  __shared__ float red2[16][C];
  const int q = threadIdx.x % QN, g = threadIdx.x / QN;
  const int c0 = blockIdx.x * C + q * 4;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
  if (c0 < H) {  // H % 4 == 0: the quad is in range
    const float* p = part + c0;
    int r = g;
    for (; r + 448 < rows; r += 512) {
      float4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const float4*>(p + (size_t)(r + 64 * u) * H);
      f4add(a0, x[0]); f4add(a1, x[1]); f4add(a2, x[2]); f4add(a3, x[3]);
      f4add(a0, x[4]); f4add(a1, x[5]); f4add(a2, x[6]); f4add(a3, x[7]);
    }
    for (; r < rows; r += 64) f4add(a0, *reinterpret_cast<const float4*>(p + (size_t)r * H));
  }
  f4add(a0, a1);
  f4add(a2, a3);
  f4add(a0, a2);
  red[g][q * 4 + 0] = a0.x;
  red[g][q * 4 + 1] = a0.y;
  red[g][q * 4 + 2] = a0.z;
  red[g][q * 4 + 3] = a0.w;
  __syncthreads();
  {  // level 2: thread (k, j) adds row groups 4k..4k+3 of column j
    const int j = threadIdx.x % C, k = threadIdx.x / C;
    red2[k][j] = (red[4 * k][j] + red[4 * k + 1][j]) + (red[4 * k + 2][j] + red[4 * k + 3][j]);
  }
  __syncthreads();
  if (threadIdx.x < C) {
    const int j = blockIdx.x * C + threadIdx.x;
    if (j < H) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) s += red2[k][threadIdx.x];
      dw[j] += s;
    }
  }
}

// Backward of the QK-norm of k_qknorm_rope_inplace (elementwise.hip).  dqkv is the packed
// gradient as the attention backward leaves it: its q|k columns hold g = dL/du, u the
// normalised pre-RoPE head.  With x the pre-norm head (raw [M, hq * HD]), rstd recomputed
// from it, xh = x * rstd and dxh = g * w, the q|k columns are overwritten in place with
//   dx = rstd * (dxh - xh * mean(dxh * xh))
// (rounded once); the v columns are not touched.  dw[j] = sum over tokens and heads of g * xh:
// blockIdx.y = 0 handles the q heads (weight qw), 1 the k heads (kw).  A thread owns lane
// c = tid % CPR of slot tid / CPR (the forward's lane layout: 8 elements of each rotation
// half) and walks heads slot, slot + gridDim.x * SLOTS, ... adding g * xh into 16 registers;
// the block then sums its SLOTS slots per column through LDS in slot order and writes row
// (blockIdx.y * gridDim.x + blockIdx.x) of the fp32 workspace -- every block writes its row,
// also one without work.  k_colsum_acc adds the rows into dw in a fixed order: no float
// atomics, two calls give the same bits.
template <int HK, int HD>
__global__ __launch_bounds__(256) void k_qknorm_bwd(bf16_t* __restrict__ dqkv, const bf16_t* __restrict__ raw,
                                                    const float* __restrict__ qw, const float* __restrict__ kw,
                                                    float* __restrict__ ws, float eps, int M, int nh, int nkv) {
  constexpr int HALF = HD / 2;
  constexpr int CPR = HALF / 8;  // lanes per head
  constexpr int SLOTS = 256 / CPR;
  __shared__ float red[SLOTS][HD];
  const int part = blockIdx.y;
  const int heads = part ? nkv : nh;
  const int col0 = part ? nh * HD : 0;  // first column of the part in a dqkv / raw row
  const int rs = (nh + 2 * nkv) * HD, rr = (nh + nkv) * HD;
  const float* w = part ? kw : qw;
  const int j = (threadIdx.x % CPR) * 8, slot = threadIdx.x / CPR;
  float w1[8], w2[8], acc1[8], acc2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    w1[e] = w[j + e];
    w2[e] = w[HALF + j + e];
    acc1[e] = 0.f;
    acc2[e] = 0.f;
  }
  const int items = M * heads;
  for (int r = blockIdx.x * SLOTS + slot; r < items; r += gridDim.x * SLOTS) {
    const int m = r / heads, h = r % heads;
    const bf16_t* xp = raw + (size_t)m * rr + col0 + h * HD;
    bf16_t* gp = dqkv + (size_t)m * rs + col0 + h * HD;
    const u16x8 xa = *reinterpret_cast<const u16x8*>(xp + j);
    const u16x8 xc = *reinterpret_cast<const u16x8*>(xp + HALF + j);
    const u16x8 ga = *reinterpret_cast<const u16x8*>(gp + j);
    const u16x8 gc = *reinterpret_cast<const u16x8*>(gp + HALF + j);
    float x1[8], x2[8];
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      x1[e] = h2f<HK>(xa.v[e]);
      x2[e] = h2f<HK>(xc.v[e]);
      ss += x1[e] * x1[e] + x2[e] * x2[e];
    }
    const float rstd = rsqrtf(head_sum<CPR>(ss) * (1.f / HD) + eps);
    float d1[8], d2[8];
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float g1 = h2f<HK>(ga.v[e]), g2 = h2f<HK>(gc.v[e]);
      x1[e] *= rstd;  // xh
      x2[e] *= rstd;
      d1[e] = g1 * w1[e];  // dxh
      d2[e] = g2 * w2[e];
      dot += d1[e] * x1[e] + d2[e] * x2[e];
      acc1[e] += g1 * x1[e];
      acc2[e] += g2 * x2[e];
    }
    const float mean = head_sum<CPR>(dot) * (1.f / HD);
    u16x8 o1, o2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o1.v[e] = f2h<HK>(rstd * (d1[e] - x1[e] * mean));
      o2.v[e] = f2h<HK>(rstd * (d2[e] - x2[e] * mean));
    }
    *reinterpret_cast<u16x8*>(gp + j) = o1;
    *reinterpret_cast<u16x8*>(gp + HALF + j) = o2;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[slot][j + e] = acc1[e];
    red[slot][HALF + j + e] = acc2[e];
  }
  __syncthreads();
  if (threadIdx.x < HD) {
    float s = 0.f;
    for (int k = 0; k < SLOTS; ++k) s += red[k][threadIdx.x];
    ws[((size_t)part * gridDim.x + blockIdx.x) * HD + threadIdx.x] = s;
  }
}

// blocks per part of k_qknorm_bwd: one head per slot and pass, at most 1024 blocks
static inline int qknorm_bwd_blocks(int M, int nh, int hd) {
  const int slots = 256 / (hd / 16);
  const long b = ((long)M * nh + slots - 1) / slots;
  return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

// floats of the workspace of dlt_qknorm_bwd (2 parts x blocks x hd)
DLT_API long dlt_qknorm_bwd_ws(int M, int nh, int hd) {
  if ((hd != 64 && hd != 128) || M <= 0 || nh <= 0) return -1;
  return 2L * qknorm_bwd_blocks(M, nh, hd) * hd;
}

// dqkv [M, (nh + 2 nkv) * hd] (q|k columns rewritten in place), raw [M, (nh + nkv) * hd], qw / kw
// fp32 [hd], dqw / dkw fp32 [hd] accumulated, ws: dlt_qknorm_bwd_ws floats
DLT_API int dlt_qknorm_bwd(bf16_t* dqkv, const bf16_t* raw, const float* qw, const float* kw, float* dqw, float* dkw,
                           float* ws, float eps, int M, int nh, int nkv, int hd, int hk, hipStream_t stream) {
  if ((hd != 64 && hd != 128) || M <= 0 || nkv <= 0 || nh <= 0 || nh % nkv ||
      (long)M * (nh + 2 * nkv) * hd >= (1L << 31))
    return -1;
  const int blocks = qknorm_bwd_blocks(M, nh, hd);
  const dim3 grid(blocks, 2), block(256);
  if (hd == 64)
    DLT_HK_DISPATCH(hk, k_qknorm_bwd<HKC, 64><<<grid, block, 0, stream>>>(dqkv, raw, qw, kw, ws, eps, M, nh, nkv));
  else
    DLT_HK_DISPATCH(hk, k_qknorm_bwd<HKC, 128><<<grid, block, 0, stream>>>(dqkv, raw, qw, kw, ws, eps, M, nh, nkv));
  k_colsum_acc<4><<<(hd + 15) / 16, 256, 0, stream>>>(ws, dqw, blocks, hd);
  k_colsum_acc<4><<<(hd + 15) / 16, 256, 0, stream>>>(ws + (size_t)blocks * hd, dkw, blocks, hd);
  DLT_CHECK_LAUNCH();
}

// Post-norms (cfg.post_norm, the Gemma-2/3 sandwich block): a second RMSNorm on a branch
// output a (the o_proj / down_proj GEMM output as rounded to the activation format), before the
// hidden dropout and the residual add:  u = round(a * rsqrt(mean(a^2) + eps) * w), fp32 math,
// one rounding.  Same row layout as the kernels above: one wave per row, NCH chunks per lane.
//
// k_postnorm_fwd: a -> u, out of place (the MLP site: u is the next layer's delta).
template <int NCH, int HK = 0>
__global__ __launch_bounds__(256) void k_postnorm_fwd(const bf16_t* __restrict__ a, const void* __restrict__ w,
                                                      int w16, bf16_t* __restrict__ u_out, int M, int H, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nc = H >> 2;
  const size_t rbase = (size_t)row * H;
  float av[NCH][4];
  float sa = 0.f;
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
#pragma unroll
    for (int e = 0; e < 4; ++e) av[t][e] = 0.f;
    if (c < nc) {
      ld_h4<HK>(a + rbase + (size_t)c * 4, av[t]);
#pragma unroll
      for (int e = 0; e < 4; ++e) sa += av[t][e] * av[t][e];
    }
  }
  sa = wave_sum(sa);
  const float rstd = rsqrtf(sa / (float)H + eps);
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
    if (c < nc) {
      const f4 ww = ld_w4<HK>(w, w16, c * 4);
      u16x4 u;
#pragma unroll
      for (int e = 0; e < 4; ++e) u.v[e] = f2h<HK>(av[t][e] * rstd * ww.v[e]);
      *reinterpret_cast<u16x4*>(u_out + rbase + (size_t)c * 4) = u;
    }
  }
}

// The attention site, fused: k_postnorm_fwd followed by k_add_dropout_rmsnorm_fwd in one pass.
// u is formed in registers and rounded to the activation format exactly as k_postnorm_fwd
// stores it, then takes the place of that kernel's delta (same dropout hash, same order of the
// fp32 operations), so x, y and rstd have the bits of the two-kernel sequence; u itself never
// goes to memory.  Two wave reductions per row (mean(a^2), mean(x^2)); every load of the row
// is issued before the first.
template <int NCH, bool XNT = false, int HK = 0>
__global__ __launch_bounds__(256) void k_postnorm_add_dropout_rmsnorm_fwd(
    const float* __restrict__ resid, const bf16_t* __restrict__ a, const void* __restrict__ wp, int wp16,
    const void* __restrict__ w, int w16, float* __restrict__ x_out, bf16_t* __restrict__ y_out,
    float* __restrict__ rstd_out, int M, int H, float eps, uint32_t key, uint32_t thr, float dscale) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nc = H >> 2;
  const size_t rbase = (size_t)row * H;
  float av[NCH][4], xv[NCH][4];
  float sa = 0.f;
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
#pragma unroll
    for (int e = 0; e < 4; ++e) { av[t][e] = 0.f; xv[t][e] = 0.f; }
    if (c < nc) {
      const size_t off = rbase + (size_t)c * 4;
      ld_h4<HK>(a + off, av[t]);
      const f4 r = ld_f4(resid + off);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xv[t][e] = r.v[e];
        sa += av[t][e] * av[t][e];
      }
    }
  }
  sa = wave_sum(sa);
  const float rstd_a = rsqrtf(sa / (float)H + eps);
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
    if (c < nc) {
      const size_t off = rbase + (size_t)c * 4;
      const f4 pw = ld_w4<HK>(wp, wp16, c * 4);
      float d[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = h2f<HK>(f2h<HK>(av[t][e] * rstd_a * pw.v[e]));
      if (thr) {
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const uint32_t h = lowbias32(key ^ (uint32_t)((off + e) >> 1));
          xv[t][e] += ((h & 0xffffu) >= thr) ? d[e] * dscale : 0.f;
          xv[t][e + 1] += ((h >> 16) >= thr) ? d[e + 1] * dscale : 0.f;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[t][e] += d[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += xv[t][e] * xv[t][e];
    }
  }
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss / (float)H + eps);
  if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
    if (c < nc) {
      const size_t off = rbase + (size_t)c * 4;
      if (XNT) st_f4_nt(x_out + off, xv[t]);
      else st_f4(x_out + off, xv[t]);
      const f4 ww = ld_w4<HK>(w, w16, c * 4);
      u16x4 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) y.v[e] = f2h<HK>(xv[t][e] * rstd * ww.v[e]);
      *reinterpret_cast<u16x4*>(y_out + off) = y;
    }
  }
}

// Backward of k_postnorm_fwd, in place: du [M, H] holds dL/du (the ddelta k_rmsnorm_bwd wrote,
// dropout already undone) and is overwritten with
//   da = rstd * (g - xh * mean(g * xh)),  g = du * w,  xh = a * rstd,
// rstd recomputed from the kept raw a (as k_qknorm_bwd does from raw); fp32 math, one rounding.
// dw[j] = sum_rows du * xh: a wave walks rows blockIdx.x * 4 + wid, + gridDim.x * 4, ... and adds
// into registers, the block sums its four waves through LDS in wave order and writes row
// blockIdx.x of the fp32 workspace (every block writes its row); k_colsum_acc adds the rows into
// dw in a fixed order -- no float atomics, two calls give the same bits.
template <int NCH, int HK = 0>
__global__ __launch_bounds__(256) void k_postnorm_bwd(bf16_t* du, const bf16_t* __restrict__ a,
                                                      const void* __restrict__ w, int w16,
                                                      float* __restrict__ dw_part, int M, int H, float eps) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [4][H]
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int nc = H >> 2;
  const float invH = 1.f / (float)H;
  float dwacc[NCH][4];
  float wv[NCH][4];
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
#pragma unroll
    for (int e = 0; e < 4; ++e) { dwacc[t][e] = 0.f; wv[t][e] = 0.f; }
    if (c < nc) {
      const f4 q = ld_w4<HK>(w, w16, c * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) wv[t][e] = q.v[e];
    }
  }
  for (int row = blockIdx.x * 4 + wid; row < M; row += gridDim.x * 4) {
    const size_t rbase = (size_t)row * H;
    float gv[NCH][4], xx[NCH][4];
    float sa = 0.f;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
      const int c = lane + 64 * t;
#pragma unroll
      for (int e = 0; e < 4; ++e) { gv[t][e] = 0.f; xx[t][e] = 0.f; }
      if (c < nc) {
        const size_t off = rbase + (size_t)c * 4;
        ld_h4<HK>(du + off, gv[t]);
        ld_h4<HK>(a + off, xx[t]);
#pragma unroll
        for (int e = 0; e < 4; ++e) sa += xx[t][e] * xx[t][e];
      }
    }
    const float rstd = rsqrtf(wave_sum(sa) * invH + eps);
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < NCH; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = xx[t][e] * rstd;
        dwacc[t][e] += gv[t][e] * xh;
        gv[t][e] *= wv[t][e];  // g
        xx[t][e] = xh;
        dot += gv[t][e] * xh;
      }
    dot = wave_sum(dot) * invH;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
      const int c = lane + 64 * t;
      if (c < nc) {
        u16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o.v[e] = f2h<HK>(rstd * (gv[t][e] - xx[t][e] * dot));
        *reinterpret_cast<u16x4*>(du + rbase + (size_t)c * 4) = o;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int c = lane + 64 * t;
    if (c < nc) {
#pragma unroll
      for (int e = 0; e < 4; ++e) smem[wid * H + c * 4 + e] = dwacc[t][e];
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < H; j += 256)
    dw_part[(size_t)blockIdx.x * H + j] = smem[j] + smem[H + j] + smem[2 * H + j] + smem[3 * H + j];
}

static inline int nch_of(int H) {
  int n = (H / 4 + 63) / 64;
  if (n > 8 && n <= 12) n = 12;
  else if (n > 12) n = 16;
  return n;
}

// H = 768: the fp32 block input goes out with nontemporal stores (it is read again only
// by the backward, ~10 ms later): step -0.03 / -0.08 / -0.06 ms in three same-box pairs;
// DLT_FWD_NT=0 selects plain stores
static int fwd_nt() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("DLT_FWD_NT");
    v = (e && atoi(e) == 0) ? 0 : 1;
  }
  return v;
}

template <int HK>
static void rmsnorm_fwd_launch(int nch, dim3 grid, dim3 block, hipStream_t stream, const float* resid,
                               const bf16_t* delta, const void* w, int wbf16, float* x_out, bf16_t* y_out,
                               float* rstd_out, int M, int H, float eps, uint32_t key, uint32_t thr, float dscale);

// hk: activation format of delta / y_out / a 16-bit weight (0 bf16, 1 fp16)
DLT_API int dlt_add_dropout_rmsnorm_fwd(const float* resid, const bf16_t* delta, const void* w, int wbf16,
                                        float* x_out, bf16_t* y_out, float* rstd_out, int M, int H,
                                        float eps, uint32_t key, uint32_t thr, float dscale, int hk,
                                        hipStream_t stream) {
  if (H % 4 != 0 || H > 4096) return -1;
  const dim3 grid((M + 3) / 4), block(256);
  const int nch = nch_of(H);
  DLT_HK_DISPATCH(hk, rmsnorm_fwd_launch<HKC>(nch, grid, block, stream, resid, delta, w, wbf16, x_out, y_out,
                                              rstd_out, M, H, eps, key, thr, dscale));
  DLT_CHECK_LAUNCH();
}

template <int HK>
static void rmsnorm_fwd_launch(int nch, dim3 grid, dim3 block, hipStream_t stream, const float* resid,
                               const bf16_t* delta, const void* w, int wbf16, float* x_out, bf16_t* y_out,
                               float* rstd_out, int M, int H, float eps, uint32_t key, uint32_t thr, float dscale) {
#define ARGS resid, delta, w, wbf16, x_out, y_out, rstd_out, M, H, eps, key, thr, dscale
  switch (nch) {
    case 1: k_add_dropout_rmsnorm_fwd<1, false, HK><<<grid, block, 0, stream>>>(ARGS); break;
    case 2: k_add_dropout_rmsnorm_fwd<2, false, HK><<<grid, block, 0, stream>>>(ARGS); break;
    case 3:
      if (fwd_nt()) k_add_dropout_rmsnorm_fwd<3, true, HK><<<grid, block, 0, stream>>>(ARGS);
      else k_add_dropout_rmsnorm_fwd<3, false, HK><<<grid, block, 0, stream>>>(ARGS);
      break;
    case 4: k_add_dropout_rmsnorm_fwd<4, false, HK><<<grid, block, 0, stream>>>(ARGS); break;
    case 5: k_add_dropout_rmsnorm_fwd<5, false, HK><<<grid, block, 0, stream>>>(ARGS); break;
    case 6: k_add_dropout_rmsnorm_fwd<6, false, HK><<<grid, block, 0, stream>>>(ARGS); break;
    case 7: k_add_dropout_rmsnorm_fwd<7, false, HK><<<grid, block, 0, stream>>>(ARGS); break;
    case 8: k_add_dropout_rmsnorm_fwd<8, false, HK><<<grid, block, 0, stream>>>(ARGS); break;
    case 12: k_add_dropout_rmsnorm_fwd<12, false, HK><<<grid, block, 0, stream>>>(ARGS); break;
    default: k_add_dropout_rmsnorm_fwd<16, false, HK><<<grid, block, 0, stream>>>(ARGS); break;
  }
#undef ARGS
}

template <int HK>
static void rmsnorm_bwd_launch(int nch, dim3 grid, dim3 block, size_t shm, hipStream_t stream, const bf16_t* dy,
                               const float* x, const float* rstd, const void* w, int wbf16, const float* dres,
                               float* dx_out, bf16_t* ddelta, float* dw, float* dw_ws, const float* dy_scale,
                               float dy_mul, int M, int H, uint32_t key, uint32_t thr, float dscale) {
#define ARGS dy, x, rstd, w, wbf16, dres, dx_out, ddelta, dw, dw_ws, dy_scale, dy_mul, M, H, key, thr, dscale
  switch (nch) {
    case 1: k_rmsnorm_bwd<1, HK><<<grid, block, shm, stream>>>(ARGS); break;
    case 2: k_rmsnorm_bwd<2, HK><<<grid, block, shm, stream>>>(ARGS); break;
    case 3: k_rmsnorm_bwd<3, HK><<<grid, block, shm, stream>>>(ARGS); break;
    case 4: k_rmsnorm_bwd<4, HK><<<grid, block, shm, stream>>>(ARGS); break;
    case 5: k_rmsnorm_bwd<5, HK><<<grid, block, shm, stream>>>(ARGS); break;
    case 6: k_rmsnorm_bwd<6, HK><<<grid, block, shm, stream>>>(ARGS); break;
    case 7: k_rmsnorm_bwd<7, HK><<<grid, block, shm, stream>>>(ARGS); break;
    case 8: k_rmsnorm_bwd<8, HK><<<grid, block, shm, stream>>>(ARGS); break;
    case 12: k_rmsnorm_bwd<12, HK><<<grid, block, shm, stream>>>(ARGS); break;
    default: k_rmsnorm_bwd<16, HK><<<grid, block, shm, stream>>>(ARGS); break;
  }
#undef ARGS
}

// hk: activation format of dy / ddelta / a 16-bit weight (0 bf16, 1 fp16)
DLT_API int dlt_rmsnorm_bwd(const bf16_t* dy, const float* x, const float* rstd, const void* w, int wbf16,
                            const float* dres, float* dx_out, bf16_t* ddelta, float* dw, float* dw_ws,
                            const float* dy_scale, float dy_mul, int M, int H, uint32_t key, uint32_t thr,
                            float dscale, int hk, hipStream_t stream) {
  if (H % 4 != 0 || H > 4096) return -1;
  // enough waves to cover HBM latency (~2 rows per wave at M = 8192), few enough
  // blocks that the per-block dw atomics stay negligible
  int blocks = (M + 3) / 4;
  if (blocks > 1024) blocks = 1024;
  const dim3 grid(blocks), block(256);
  const size_t shm = (size_t)4 * H * sizeof(float);
  const int nch = nch_of(H);
  DLT_HK_DISPATCH(hk, rmsnorm_bwd_launch<HKC>(nch, grid, block, shm, stream, dy, x, rstd, w, wbf16, dres, dx_out,
                                              ddelta, dw, dw_ws, dy_scale, dy_mul, M, H, key, thr, dscale));
  if (dw_ws) {
    // 16-column blocks of 256 threads (48 for H = 768) slot into the CUs that the other
    // micro-step chain's kernels leave free; 64-column blocks of 1024 threads waited for
    // a whole free CU (45 us in the overlapped step vs 6 us alone).  Same summation order
    // either way (DLT_COLSUM_WIDE=1: the 1024-thread form).
    static const bool wide = getenv("DLT_COLSUM_WIDE") && atoi(getenv("DLT_COLSUM_WIDE")) == 1;
    if (wide) k_colsum_acc<16><<<(H + 63) / 64, 1024, 0, stream>>>(dw_ws, dw, blocks, H);
    else k_colsum_acc<4><<<(H + 15) / 16, 256, 0, stream>>>(dw_ws, dw, blocks, H);
  }
  DLT_CHECK_LAUNCH();
}

// ---- post-norm launchers (the limits of the launchers above: H % 4 == 0, H <= 4096) ----
#define DLT_NCH_SWITCH(nch, LAUNCH) \
  switch (nch) {                    \
    case 1: LAUNCH(1); break;       \
    case 2: LAUNCH(2); break;       \
    case 3: LAUNCH(3); break;       \
    case 4: LAUNCH(4); break;       \
    case 5: LAUNCH(5); break;       \
    case 6: LAUNCH(6); break;       \
    case 7: LAUNCH(7); break;       \
    case 8: LAUNCH(8); break;       \
    case 12: LAUNCH(12); break;     \
    default: LAUNCH(16); break;     \
  }

// a, u_out [M, H] in the activation format hk; w fp32 or (w16) that format
DLT_API int dlt_postnorm_fwd(const bf16_t* a, const void* w, int w16, bf16_t* u_out, int M, int H, float eps, int hk,
                             hipStream_t stream) {
  if (H % 4 != 0 || H > 4096 || H <= 0 || M <= 0) return -1;
  const dim3 grid((M + 3) / 4), block(256);
  const int nch = nch_of(H);
#define LAUNCH(N) k_postnorm_fwd<N, HKC><<<grid, block, 0, stream>>>(a, w, w16, u_out, M, H, eps)
  DLT_HK_DISPATCH(hk, DLT_NCH_SWITCH(nch, LAUNCH));
#undef LAUNCH
  DLT_CHECK_LAUNCH();
}

// resid, x_out fp32 [M, H]; a, y_out [M, H] in the activation format hk; wp (the post-norm
// weight) and w (the following pre-norm's) fp32 or 16-bit; rstd_out fp32 [M]
DLT_API int dlt_postnorm_add_dropout_rmsnorm_fwd(const float* resid, const bf16_t* a, const void* wp, int wp16,
                                                 const void* w, int w16, float* x_out, bf16_t* y_out,
                                                 float* rstd_out, int M, int H, float eps, uint32_t key,
                                                 uint32_t thr, float dscale, int hk, hipStream_t stream) {
  if (H % 4 != 0 || H > 4096 || H <= 0 || M <= 0) return -1;
  const dim3 grid((M + 3) / 4), block(256);
  const int nch = nch_of(H);
  const bool nt = nch == 3 && fwd_nt();  // x_out as k_add_dropout_rmsnorm_fwd stores it at H = 768
#define LAUNCH(N)                                                                                              \
  if (N == 3 && nt)                                                                                            \
    k_postnorm_add_dropout_rmsnorm_fwd<3, true, HKC><<<grid, block, 0, stream>>>(                              \
        resid, a, wp, wp16, w, w16, x_out, y_out, rstd_out, M, H, eps, key, thr, dscale);                      \
  else                                                                                                         \
    k_postnorm_add_dropout_rmsnorm_fwd<N, false, HKC><<<grid, block, 0, stream>>>(                             \
        resid, a, wp, wp16, w, w16, x_out, y_out, rstd_out, M, H, eps, key, thr, dscale)
  DLT_HK_DISPATCH(hk, DLT_NCH_SWITCH(nch, LAUNCH));
#undef LAUNCH
  DLT_CHECK_LAUNCH();
}

// workgroups of k_postnorm_bwd (= rows of its workspace): k_rmsnorm_bwd's rule
static inline int postnorm_bwd_blocks(int M) {
  const int b = (M + 3) / 4;
  return b > 1024 ? 1024 : b;
}

// floats of the workspace of dlt_postnorm_bwd (blocks x H)
DLT_API long dlt_postnorm_bwd_ws(int M, int H) {
  if (H % 4 != 0 || H > 4096 || H <= 0 || M <= 0) return -1;
  return (long)postnorm_bwd_blocks(M) * H;
}

// du [M, H] (rewritten in place), a [M, H] in the activation format hk; w fp32 or 16-bit;
// dw fp32 [H] accumulated; ws: dlt_postnorm_bwd_ws floats
DLT_API int dlt_postnorm_bwd(bf16_t* du, const bf16_t* a, const void* w, int w16, float* dw, float* ws, int M, int H,
                             float eps, int hk, hipStream_t stream) {
  if (H % 4 != 0 || H > 4096 || H <= 0 || M <= 0) return -1;
  const int blocks = postnorm_bwd_blocks(M);
  const dim3 grid(blocks), block(256);
  const size_t shm = (size_t)4 * H * sizeof(float);
  const int nch = nch_of(H);
#define LAUNCH(N) k_postnorm_bwd<N, HKC><<<grid, block, shm, stream>>>(du, a, w, w16, ws, M, H, eps)
  DLT_HK_DISPATCH(hk, DLT_NCH_SWITCH(nch, LAUNCH));
#undef LAUNCH
  k_colsum_acc<4><<<(H + 15) / 16, 256, 0, stream>>>(ws, dw, blocks, H);
  DLT_CHECK_LAUNCH();
}
