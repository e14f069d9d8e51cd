// The fused decode step over an FP8 (e4m3) KV cache, in a translation unit of its own so that the
// kernels of decode.hip and decode_norms.hip keep their code (kv_fp8.h has the format):
//
//   k_dec_norm_qkv / k_dec_norm_qkv_qkn, F8 forms : the step's new K/V row is rounded to bf16 as in
//                     the 16-bit forms and stored as e4m3 bytes by the kernel that produced it
//   k_dec_attn_f8     : k_dec_attn over e4m3 caches [B, nh, maxS, 64 bytes]
//   k_dec_attn_gqa_f8 : k_dec_attn_gqa over e4m3 caches; its partials go through decode.hip's
//                       k_dec_attn_combine (dec_attn_combine_launch), unchanged
//
// The attention kernels are bound by reading cache rows, and a head row is now 64 bytes, so the
// key-to-lane mapping of the 16-bit kernels (a lane per key, 8 x 16-byte loads of its 128-byte
// row) would leave a lane 4 loads of a row that neighbouring lanes cannot coalesce with.  Here
//   scores : 4 lanes to a row, lane (slot, qd) = (tid / 4, tid % 4) loads the 16 bytes of dims
//            16 qd .. 16 qd + 15 of key slot: one wave-load covers 16 whole rows (1 KiB, contiguous),
//            the workgroup 64 keys, and 4 such loads per lane are in flight (256 keys a trip).  The
//            bytes become fp32 with v_cvt_pk_f32_fp8 (8 per 16 bytes), the lane's 16 FMAs run
//            against its quarter of q, and two xor-shuffles (1, 2) sum the quarters: all 4 lanes
//            hold the score.  A lane past the last key re-reads the last row (no branch round the
//            loads) and stores nothing.
//   o      : k_dec_attn_f8: lane (js, dc) = (tid / 4, tid % 4), 16-byte V loads, 16 accumulators,
//            the wave's 16 key slots summed by halving xor-shuffles (15 in place of 64).
//            k_dec_attn_gqa_f8 keeps the 16-bit kernel's (tid / 8, tid % 8) map with 8-byte loads:
//            GT x 16 accumulators would not fit the registers a group of 16 heads has left.
// The scores in LDS, the (m, l, o) partials, the LDS budgets (dec_attn_gqa_lds, dec_attn_chunk) and
// every rule about rows past `pos` (never read) are those of decode.hip.
#define DLT_KV8_TU 1
#include "kv_fp8.h"
#include "decode_norms.hip"

// decode.hip: k_dec_attn_combine on `st`
int dec_attn_combine_launch(const float* ws, bf16_t* o, int B, int nh, int NS, const float* sink, hipStream_t st);

namespace {

constexpr int KV8_WS = 66;    // floats per partial: o[64], m, l (decode.hip GQA_WS)
constexpr int KV8_GMAX = 16;  // query heads per workgroup (decode.hip GQA_GMAX)

// decode.hip dec_cap_score
__device__ __forceinline__ float kv8_cap_score(float s, float cap, float cap_k) {
  const float a = __builtin_amdgcn_exp2f(-fabsf(s) * cap_k);
  return copysignf(cap * ((1.f - a) * __builtin_amdgcn_rcpf(1.f + a)), s);
}

__device__ __forceinline__ uint4 ld_kv16(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }

}  // namespace

// grid (B * nh): one (b, head), as k_dec_attn; WIN, sink and CAP as there.
template <bool WIN, bool CAP>
__global__ __launch_bounds__(DEC_NT) void k_dec_attn_f8(const bf16_t* __restrict__ q, const uint8_t* __restrict__ kc,
                                                        const uint8_t* __restrict__ vc, const long* __restrict__ posp,
                                                        bf16_t* __restrict__ o, int H, int nh, int maxS, float scale,
                                                        int win, const float* __restrict__ sink, float cap,
                                                        float cap_k) {
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  float* sc = reinterpret_cast<float*>(dsm);       // [maxS] scores -> probabilities (WIN: [min(win, maxS)])
  float* red = sc + (WIN ? min(win, maxS) : maxS); // [8]
  float* oacc = red + 8;                           // [4][64]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.x / nh, head = blockIdx.x % nh;
  DLT_DASSERT(posp[0] >= 0 && posp[0] < maxS);
  const int end = (int)(posp[0] < 0 ? 1 : (posp[0] < maxS ? posp[0] + 1 : maxS));
  const int kf = WIN ? max(0, end - max(win, 1)) : 0;
  const int len = end - kf;  // >= 1
  const uint8_t* K = kc + (((size_t)b * nh + head) * maxS + kf) * 64;
  const uint8_t* V = vc + (((size_t)b * nh + head) * maxS + kf) * 64;
  const int qd = tid & 3, slot = tid >> 2;
  float qv[16];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const u16x8 t = *reinterpret_cast<const u16x8*>(q + (size_t)b * H + head * 64 + qd * 16 + c * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[c * 8 + e] = bf2f(t.v[e]);
  }
  float mx = -INFINITY;
  for (int j0 = 0; j0 < len; j0 += DEC_NT) {  // (uniform) 4 loads of 64 keys
    uint4 kv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) kv[u] = ld_kv16(K + (size_t)min(j0 + 64 * u + slot, len - 1) * 64 + qd * 16);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float kx[16];
      kv8_unpack16(kv[u], kx);
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) s = fmaf(qv[e], kx[e], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s *= scale;
      if constexpr (CAP) s = kv8_cap_score(s, cap, cap_k);
      const int j = j0 + 64 * u + slot;
      if (j < len) {
        if (qd == 0) sc[j] = s;
        mx = fmaxf(mx, s);
      }
    }
  }
#pragma unroll
  for (int o2 = 32; o2 > 0; o2 >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o2, 64));
  if (lane == 0) red[wid] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float sk = sink ? sink[head] : -INFINITY;
  if (sink) mx = fmaxf(mx, sk);
  float sum = 0.f;
  for (int j = tid; j < len; j += DEC_NT) {
    const float p = __expf(sc[j] - mx);
    sc[j] = p;
    sum += p;
  }
  sum = wave_sum64(sum);
  __syncthreads();  // every red[] max read before it is overwritten; every probability written
  if (lane == 0) red[4 + wid] = sum;
  __syncthreads();
  float den = red[4] + red[5] + red[6] + red[7];
  if (sink) den += __expf(sk - mx);
  const float inv = 1.f / den;
  // o[d] = sum_j p_j v_j[d]: lane (js, dc) loads dims 16dc..16dc+15 of keys js, js + 64, ...
  const int dc = qd, js = slot;
  float acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll 4
  for (int j = js; j < len; j += DEC_NT / 4) {
    const uint4 t = ld_kv16(V + (size_t)j * 64 + dc * 16);
    const float p = sc[j];
    float vx[16];
    kv8_unpack16(t, vx);
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = fmaf(p, vx[e], acc[e]);
  }
  // Sum over the wave's 16 key slots (lane bits 5..2) by halving: at each step a lane keeps one
  // half of its values, hands the other to its partner and adds what it receives.  Lane (k, dc),
  // k = (lane >> 2) & 15, ends with the sum of dim 16 dc + k in acc[0].
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    const int m = 32 >> st, half = 8 >> st;
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float send = up ? acc[i] : acc[i + half];
      const float keep = up ? acc[i + half] : acc[i];
      acc[i] = keep + __shfl_xor(send, m, 64);
    }
  }
  oacc[wid * 64 + dc * 16 + ((lane >> 2) & 15)] = acc[0];
  __syncthreads();
  if (tid < 64) {
    const float r = (oacc[tid] + oacc[64 + tid] + oacc[128 + tid] + oacc[192 + tid]) * inv;
    o[(size_t)b * H + head * 64 + tid] = f2bf(r);
  }
}

// grid (B * nkv * GS * NS): workgroup (b, kv head, sub-group, s), as k_dec_attn_gqa; the chunks, the
// WIN anchoring, the sink rule (NS == 1 here, NS > 1 in the combine) and CAP as there.
template <int GT, bool WIN, bool CAP>
__global__ __launch_bounds__(DEC_NT) void k_dec_attn_gqa_f8(const bf16_t* __restrict__ q, const uint8_t* __restrict__ kc,
                                                            const uint8_t* __restrict__ vc,
                                                            const long* __restrict__ posp, bf16_t* __restrict__ o,
                                                            float* __restrict__ ws, int H, int nh, int nkv, int maxS,
                                                            int NS, int C, float scale, int win,
                                                            const float* __restrict__ sink, float cap, float cap_k) {
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  float* red = reinterpret_cast<float*>(dsm);  // [2][4][GT] per-wave max, sum
  float* oacc = red + 8 * GT;                  // [4][GT][64]
  float* qs = oacc + 4 * GT * 64;              // [GT][64] q in fp32
  float* sc = qs + GT * 64;                    // [GT][C] scores -> probabilities
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int G = nh / nkv, GS = (G + KV8_GMAX - 1) / KV8_GMAX;
  int t = blockIdx.x;
  const int s = t % NS;
  t /= NS;
  const int sub = t % GS;
  t /= GS;
  const int kvh = t % nkv, b = t / nkv;
  const int Gl = min(GT, G - sub * GT);  // GT == KV8_GMAX whenever GS > 1
  const int h0 = kvh * G + sub * GT;     // first query head of this workgroup
  DLT_DASSERT(posp[0] >= 0 && posp[0] < maxS);
  const int len = (int)(posp[0] < 0 ? 1 : (posp[0] < maxS ? posp[0] + 1 : maxS));
  const int kf = WIN ? max(0, len - max(win, 1)) : 0;    // first key of the window
  const int lo = kf + s * C, n = min(lo + C, len) - lo;  // n <= C keys of this chunk (<= 0: none)
  if (n <= 0) {  // (uniform) only with NS > 1: chunk 0 always holds key kf
    if (tid < Gl) {
      float* w = ws + (((size_t)b * nh + h0 + tid) * NS + s) * KV8_WS;
      w[64] = -INFINITY;
      w[65] = 0.f;
    }
    return;
  }
  const uint8_t* K = kc + (((size_t)b * nkv + kvh) * maxS + lo) * 64;
  const uint8_t* V = vc + (((size_t)b * nkv + kvh) * maxS + lo) * 64;
  // The lane's first four K pieces and the group's q are requested together; every later trip
  // requests its successor's piece before its own dot products.  Rows are clamped to n - 1 (a row
  // that exists) so that no load sits behind a branch; a clamped row's score is not stored.
  const int qd = tid & 3, slot = tid >> 2;
  uint4 kv[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) kv[u] = ld_kv16(K + (size_t)min(64 * u + slot, n - 1) * 64 + qd * 16);
  // q in fp32; a padded head (g >= Gl) repeats the last one, so the loops over g have no branch
  if (tid < GT * 8) {  // one 16-byte chunk of q per thread
    const u16x8 w = *reinterpret_cast<const u16x8*>(q + (size_t)b * H + (size_t)(h0 + min(tid >> 3, Gl - 1)) * 64 +
                                                    (tid & 7) * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) qs[tid * 8 + e] = bf2f(w.v[e]);
  }
  __syncthreads();
  float mx[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) mx[g] = -INFINITY;
  for (int j0 = 0; j0 < n; j0 += DEC_NT) {  // (uniform)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float kx[16];
      kv8_unpack16(kv[u], kx);
      kv[u] = ld_kv16(K + (size_t)min(j0 + DEC_NT + 64 * u + slot, n - 1) * 64 + qd * 16);
      // dims outer, heads inner: GT independent fma chains; the 4 lanes of a row read 4 distinct
      // 16-byte pieces of a q row, 64 bytes apart (distinct banks), every row's lanes the same 4
      float a[GT];
#pragma unroll
      for (int g = 0; g < GT; ++g) a[g] = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int g = 0; g < GT; ++g) {
          const float4 qv = *reinterpret_cast<const float4*>(qs + g * 64 + qd * 16 + c * 4);
          a[g] = fmaf(qv.x, kx[c * 4], a[g]);
          a[g] = fmaf(qv.y, kx[c * 4 + 1], a[g]);
          a[g] = fmaf(qv.z, kx[c * 4 + 2], a[g]);
          a[g] = fmaf(qv.w, kx[c * 4 + 3], a[g]);
        }
      const int j = j0 + 64 * u + slot;
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        a[g] += __shfl_xor(a[g], 1, 64);
        a[g] += __shfl_xor(a[g], 2, 64);
        a[g] *= scale;
        if constexpr (CAP) a[g] = kv8_cap_score(a[g], cap, cap_k);
        if (j < n) {
          if ((g & 3) == qd) sc[g * C + j] = a[g];  // the row's 4 lanes share the stores
          mx[g] = fmaxf(mx[g], a[g]);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < GT; ++g) {
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) mx[g] = fmaxf(mx[g], __shfl_xor(mx[g], o2, 64));
    if (lane == 0) red[wid * GT + g] = mx[g];
  }
  __syncthreads();  // every score and every wave's max written
  float sum[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    mx[g] = fmaxf(fmaxf(red[g], red[GT + g]), fmaxf(red[2 * GT + g], red[3 * GT + g]));
    if (sink && NS == 1) mx[g] = fmaxf(mx[g], sink[h0 + min(g, Gl - 1)]);  // a padded head repeats the last
    sum[g] = 0.f;
  }
  for (int j = tid; j < n; j += DEC_NT) {
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      const float p = __expf(sc[g * C + j] - mx[g]);
      sc[g * C + j] = p;
      sum[g] += p;
    }
  }
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    sum[g] = wave_sum64(sum[g]);
    if (lane == 0) red[(4 + wid) * GT + g] = sum[g];
  }
  __syncthreads();  // every probability and every wave's sum written
  // o[g][d] = sum_j p_gj v_j[d]: lane (js, dc) = (tid / 8, tid % 8) loads the 8 bytes of dims
  // 8dc..8dc+7 of keys j = js, js + 32, ... once and uses them for every head of the group
  const int dc = tid & 7, js = tid >> 3;
  float acc[GT * 8];  // [g][e]
#pragma unroll
  for (int i = 0; i < GT * 8; ++i) acc[i] = 0.f;
  // 4 keys per trip, their loads issued together; a key past the chunk re-reads key n - 1
  // (a row that exists) with weight 0, so the trip has no branch either
  for (int j0 = js; j0 < n; j0 += 4 * (DEC_NT / 8)) {
    uint2 vv[4];
    int jc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      jc[u] = min(j0 + u * (DEC_NT / 8), n - 1);
      vv[u] = *reinterpret_cast<const uint2*>(V + (size_t)jc[u] * 64 + dc * 8);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float ok = j0 + u * (DEC_NT / 8) < n ? 1.f : 0.f;
      float vf[8];
      kv8_unpack4(vv[u].x, vf);
      kv8_unpack4(vv[u].y, vf + 4);
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        const float p = sc[g * C + jc[u]] * ok;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g * 8 + e] = fmaf(p, vf[e], acc[g * 8 + e]);
      }
    }
  }
  // the wave's 8 key slots (lane bits 5, 4, 3) summed by halving, as in k_dec_attn_gqa: lane (k, dc),
  // k = (lane >> 3) & 7, ends with the GT sums of the flat indices k GT .. k GT + GT - 1 of [g][e]
#pragma unroll
  for (int st = 0; st < 3; ++st) {
    const int m = 32 >> st, half = (GT * 8) >> (st + 1);
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float send = up ? acc[i] : acc[i + half];
      const float keep = up ? acc[i + half] : acc[i];
      acc[i] = keep + __shfl_xor(send, m, 64);
    }
  }
#pragma unroll
  for (int i = 0; i < GT; ++i) {
    const int v = ((lane >> 3) & 7) * GT + i;  // = g * 8 + e
    oacc[(wid * GT + (v >> 3)) * 64 + dc * 8 + (v & 7)] = acc[i];
  }
  __syncthreads();
  for (int i = tid; i < Gl * 64; i += DEC_NT) {
    const int g = i >> 6;
    const float r = oacc[i] + oacc[GT * 64 + i] + oacc[2 * GT * 64 + i] + oacc[3 * GT * 64 + i];
    if (NS == 1) {
      float den = red[4 * GT + g] + red[5 * GT + g] + red[6 * GT + g] + red[7 * GT + g];
      if (sink) {  // the head's max as the softmax above took it
        const float sk = sink[h0 + g];
        const float m = fmaxf(fmaxf(fmaxf(red[g], red[GT + g]), fmaxf(red[2 * GT + g], red[3 * GT + g])), sk);
        den += __expf(sk - m);
      }
      const float inv = 1.f / den;
      o[(size_t)b * H + h0 * 64 + i] = f2bf(r * inv);
    } else {
      ws[(((size_t)b * nh + h0 + g) * NS + s) * KV8_WS + (i & 63)] = r;
    }
  }
  if (NS > 1 && tid < Gl) {
    float* w = ws + (((size_t)b * nh + h0 + tid) * NS + s) * KV8_WS;
    w[64] = fmaxf(fmaxf(red[tid], red[GT + tid]), fmaxf(red[2 * GT + tid], red[3 * GT + tid]));
    w[65] = red[4 * GT + tid] + red[5 * GT + tid] + red[6 * GT + tid] + red[7 * GT + tid];
  }
}

// ------------------------------------------------------------------------ launchers
// The entry points take what their 16-bit namesakes take, with kc / vc e4m3 bytes [B, nkv, maxS, 64],
// and one entry covers the forms: pa null = no post-norm prologue, window 0 = none, sink null = none,
// cap 0 = none.  -1: an argument check failed and nothing was launched.
static inline bool kv8_al16(const void* p) { return p && !((uintptr_t)p & 15); }

DLT_API int dlt_dec_norm_qkv_kv8(const float* h, const void* lnw, int wbf16, float eps, const bf16_t* wqkv,
                                 const float* cosT, const float* sinT, const long* pos, bf16_t* qout, uint8_t* kc,
                                 uint8_t* vc, const bf16_t* pa, const void* pnw, int pnbf16, float* hout, int B, int H,
                                 int nh, int nkv, int maxS, hipStream_t st) {
  if (H != nh * 64 || H % 8 || nkv < 1 || nh % nkv || maxS < 1 || dec_lds(B, H) > 160 * 1024) return -1;
  if (!kc || !vc || (pa && (!dec_pn_ok(h, pa, pnw, hout) || !hout))) return -1;
  bf16_t* k16 = reinterpret_cast<bf16_t*>(kc);  // the kernel's pointer type; its F8 form stores bytes
  bf16_t* v16 = reinterpret_cast<bf16_t*>(vc);
#define L(BB)                                                                                                \
  if (pa)                                                                                                    \
    k_dec_norm_qkv<BB, true, true><<<(nh + 2 * nkv) * 4, DEC_NT, dec_lds(BB, H), st>>>(                      \
        h, lnw, wbf16, eps, wqkv, cosT, sinT, pos, qout, k16, v16, H, nh, nkv, maxS, pa, pnw, pnbf16, hout); \
  else                                                                                                       \
    k_dec_norm_qkv<BB, false, true><<<(nh + 2 * nkv) * 4, DEC_NT, dec_lds(BB, H), st>>>(                     \
        h, lnw, wbf16, eps, wqkv, cosT, sinT, pos, qout, k16, v16, H, nh, nkv, maxS)
  DEC_DISPATCH(B, L)
#undef L
  DLT_CHECK_LAUNCH();
}

DLT_API int dlt_dec_norm_qkv_qkn_kv8(const float* h, const void* lnw, int wbf16, float eps, const bf16_t* wqkv,
                                     const void* qnw, const void* knw, int qkbf16, const float* cosT,
                                     const float* sinT, const long* pos, bf16_t* qout, uint8_t* kc, uint8_t* vc,
                                     const bf16_t* pa, const void* pnw, int pnbf16, float* hout, int B, int H, int nh,
                                     int nkv, int maxS, hipStream_t st) {
  if (H != nh * 64 || H % 8 || nkv < 1 || nh % nkv || maxS < 1 || dec_lds_qkn(B, H) > 160 * 1024) return -1;
  if (!qnw || !knw || !kc || !vc) return -1;
  if (pa && (!dec_pn_ok(h, pa, pnw, hout) || !hout)) return -1;
  bf16_t* k16 = reinterpret_cast<bf16_t*>(kc);
  bf16_t* v16 = reinterpret_cast<bf16_t*>(vc);
#define L(BB)                                                                                                   \
  if (pa)                                                                                                       \
    k_dec_norm_qkv_qkn<BB, true, qkn_nt(BB), true><<<nh + 2 * nkv, qkn_nt(BB), dec_lds_qkn(BB, H), st>>>(       \
        h, lnw, wbf16, eps, wqkv, qnw, knw, qkbf16, cosT, sinT, pos, qout, k16, v16, H, nh, nkv, maxS, pa, pnw, \
        pnbf16, hout);                                                                                          \
  else                                                                                                          \
    k_dec_norm_qkv_qkn<BB, false, qkn_nt(BB), true><<<nh + 2 * nkv, qkn_nt(BB), dec_lds_qkn(BB, H), st>>>(      \
        h, lnw, wbf16, eps, wqkv, qnw, knw, qkbf16, cosT, sinT, pos, qout, k16, v16, H, nh, nkv, maxS, nullptr, \
        nullptr, 0, nullptr)
  DEC_DISPATCH(B, L)
#undef L
  DLT_CHECK_LAUNCH();
}

DLT_API int dlt_dec_attn_kv8(const bf16_t* q, const uint8_t* kc, const uint8_t* vc, const long* pos, bf16_t* o, int B,
                             int H, int nh, int maxS, float scale, int window, const float* sink, float cap,
                             hipStream_t st) {
  if (window < 0 || maxS < 1 || B < 1 || nh < 1 || !(cap >= 0.f) || __builtin_isinf(cap)) return -1;
  if (!kv8_al16(q) || !kv8_al16(kc) || !kv8_al16(vc) || !o || !pos) return -1;
  const size_t lds = (size_t)(window > 0 && window < maxS ? window : maxS) * 4 + 8 * 4 + 4 * 64 * 4;
  if (H != nh * 64 || lds > 160 * 1024) return -1;
  const float cap_k = cap > 0.f ? 2.f * 1.44269504088896340736f / cap : 0.f;
#define L(WINC, CAPC)                                                                                               \
  k_dec_attn_f8<WINC, CAPC><<<B * nh, DEC_NT, lds, st>>>(q, kc, vc, pos, o, H, nh, maxS, scale, window, sink, cap, \
                                                         cap_k)
  if (cap > 0.f && window > 0) L(true, true);
  else if (cap > 0.f) L(false, true);
  else if (window > 0) L(true, false);
  else L(false, false);
#undef L
  DLT_CHECK_LAUNCH();
}

// NS in {1, 2, 4, 8} key chunks per K/V head; ws: fp32 [B, nh, NS, 66] (NS > 1).  Two launches on
// `st` for NS > 1, one otherwise.
DLT_API int dlt_dec_attn_gqa_kv8(const bf16_t* q, const uint8_t* kc, const uint8_t* vc, const long* pos, bf16_t* o,
                                 float* ws, int B, int H, int nh, int nkv, int maxS, int NS, float scale, int window,
                                 const float* sink, float cap, hipStream_t st) {
  if (B < 1 || nh < 1 || H != nh * 64 || nkv < 1 || nh % nkv || maxS < 1 || window < 0) return -1;
  if (!(cap >= 0.f) || __builtin_isinf(cap)) return -1;
  if (!kv8_al16(q) || !kv8_al16(kc) || !kv8_al16(vc) || !o || !pos) return -1;
  if ((NS != 1 && NS != 2 && NS != 4 && NS != 8) || (NS > 1 && !ws)) return -1;
  const float cap_k = cap > 0.f ? 2.f * 1.44269504088896340736f / cap : 0.f;
  const int G = nh / nkv, Gw = G < KV8_GMAX ? G : KV8_GMAX, GS = (G + KV8_GMAX - 1) / KV8_GMAX;
  const int C = (((window > 0 && window < maxS) ? window : maxS) + NS - 1) / NS;  // decode.hip dec_attn_chunk
  const int gts[8] = {1, 2, 3, 4, 6, 8, 12, 16};
  int GT = 16;
  for (int i = 7; i >= 0; --i)
    if (gts[i] >= Gw) GT = gts[i];
  const size_t lds = (size_t)GT * (C + 8 + 4 * 64 + 64) * 4;  // scores, max / sum, o of 4 waves, q
  if (lds > 160 * 1024) return -1;
  const int grid = B * nkv * GS * NS;
#define K8(GG, WINC, CAPC)                                                                                           \
  k_dec_attn_gqa_f8<GG, WINC, CAPC><<<grid, DEC_NT, lds, st>>>(q, kc, vc, pos, o, ws, H, nh, nkv, maxS, NS, C, scale, \
                                                               window, sink, cap, cap_k)
#define L(GG)                                           \
  case GG:                                              \
    if (cap > 0.f && window > 0) K8(GG, true, true);    \
    else if (cap > 0.f) K8(GG, false, true);            \
    else if (window > 0) K8(GG, true, false);           \
    else K8(GG, false, false);                          \
    break
  switch (GT) {
    L(1);
    L(2);
    L(3);
    L(4);
    L(6);
    L(8);
    L(12);
    L(16);
  }
#undef L
#undef K8
  if (NS > 1) return dec_attn_combine_launch(ws, o, B, nh, NS, sink, st);
  DLT_CHECK_LAUNCH();
}
