// The prefill writer over an FP8 (e4m3) KV cache, in a translation unit of its own so that
// prefill.hip's kernels keep their code (kv_fp8.h has the format):
//
//   k_prefill_qkv_cache, F8 form : prefill.hip's kernel with the k and v rows stored as e4m3 bytes
//
// There is no prefill ATTENTION over an FP8 cache yet: the prompt's queries cannot read one, so
// ops.prefill_attn and eval/decode.py forward_cached refuse it.  A form that stages the byte tiles
// through registers into the 16-bit LDS image was built and measured at 1.20x the bf16 time on a
// 64-token append to 16320 cached rows (profiles/kv_fp8.md); what is wanted is LDS-DMA of the byte
// tiles (64 keys x hd bytes, half the LDS per stage), a byte-granular swizzle and 8-byte fragment
// reads expanded to the MFMA operands, with a transposing byte read for V.
#define DLT_KV8_TU 1
#include "kv_fp8.h"
#include "prefill.hip"

// dlt_prefill_qkv_cache with kc / vc e4m3 bytes [B, nkv, maxS, hd]; the same argument checks and
// return codes.
DLT_API int dlt_prefill_qkv_cache_kv8(bf16_t* qkv, uint8_t* kc, uint8_t* vc, const float* cosT, const float* sinT,
                                      const float* qw, const float* kw, float eps, int B, int T, int p0, int nh,
                                      int nkv, int hd, int maxS, int hk, hipStream_t st) {
  if (const int rc = prefill_check(qkv, kc, vc, B, T, p0, nh, nkv, hd, maxS, hk)) return rc;
  if (!al16(cosT) || !al16(sinT) || (qw != nullptr) != (kw != nullptr) || (qw && (!al16(qw) || !al16(kw)))) return -5;
  const int M = B * T;
  const size_t total = (size_t)M * (nh + 2 * nkv) * (hd / 16);
  const int blocks = (int)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
  bf16_t* k16 = reinterpret_cast<bf16_t*>(kc);  // the kernel's pointer type; its F8 form stores bytes
  bf16_t* v16 = reinterpret_cast<bf16_t*>(vc);
  DLT_BOOL_DISPATCH(QKNC, qw, DLT_HD_DISPATCH(hd, DLT_HK_DISPATCH(hk,
      k_prefill_qkv_cache<HKC, HDC, QKNC, true><<<blocks, 256, 0, st>>>(qkv, k16, v16, cosT, sinT, qw, kw, eps, M, T,
                                                                        p0, nh, nkv, maxS))));
  DLT_CHECK_LAUNCH();
}
