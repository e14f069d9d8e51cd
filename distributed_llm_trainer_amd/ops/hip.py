"""ctypes bindings for the gfx950 kernel library (``ops/_dlt_kernels.so``).

Every wrapper validates shapes/dtypes/contiguity on the host BEFORE launching (a
mis-shaped launch of a hand-written kernel must never reach the GPU), allocates
outputs with the torch caching allocator and launches on the current HIP stream, so
the calls are graph-capturable and ordered with hipBLASLt GEMMs and RCCL.

Import is loud: on a GPU box, a missing or stale library raises instead of silently
falling back to PyTorch ops.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional

import torch

from . import rng
from .reference import check_softcap  # noqa: F401  (one validation for both backends)

_LIB = None
# DLT_KERNEL_DEBUG=1 loads the bounds-checked build (ops/build.py --debug);
# DLT_KERNEL_LIB=<file in ops/> loads another build of the same sources (same-box A/B
# of a kernel change: tools/ab/kernels_ab.sh)
_LIBPATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "_dlt_kernels_debug.so" if os.environ.get("DLT_KERNEL_DEBUG") == "1"
                        else os.path.basename(os.environ.get("DLT_KERNEL_LIB", "_dlt_kernels.so")))

c_void_p, c_int, c_float, c_uint32, c_int64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint32, ctypes.c_int64

_SIGS = {
    "dlt_add_dropout_rmsnorm_fwd": [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                    c_int, c_float, c_uint32, c_uint32, c_float, c_int, c_void_p],
    "dlt_rmsnorm_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                        c_void_p, c_void_p, c_float, c_int, c_int, c_uint32, c_uint32, c_float, c_int, c_void_p],
    "dlt_embedding_fwd": [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p],
    "dlt_embedding_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p],
    "dlt_embedding_bwd_chunk": [],
    "dlt_splitk_acc": [c_void_p, c_void_p, ctypes.c_long, c_int, c_void_p],
    "dlt_splitk_sum_bf16": [c_void_p, c_void_p, ctypes.c_long, c_int, c_int, c_void_p],
    "dlt_rope_qkv_fwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                         c_int, c_void_p],
    "dlt_rope_qkv_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                         c_int, c_int, c_void_p],
    "dlt_swiglu_fwd": [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p],
    "dlt_swiglu_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p],
    "dlt_cross_entropy_fwd_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int,
                                  c_void_p],
    "dlt_cross_entropy_z_fwd_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int,
                                    c_float, c_void_p, c_void_p],
    "dlt_cross_entropy_cap_fwd_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int,
                                      c_float, c_void_p, c_float, c_void_p],
    "dlt_sumsq": [c_void_p, c_int64, c_void_p, c_void_p, c_void_p],
    "dlt_clip_coef": [c_void_p, c_void_p, c_float, c_float, c_float, c_void_p],
    "dlt_adamw": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                  c_float, c_float, c_float, c_void_p, c_void_p],
    "dlt_adamw_ex": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                     c_float, c_float, c_float, c_void_p, c_int, c_void_p],
    "dlt_adamw_f16": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                      c_float, c_float, c_float, c_void_p, c_void_p],
    "dlt_cast_bf16": [c_void_p, c_void_p, c_int64, c_int, c_void_p],
    "dlt_add_bf16_f32": [c_void_p, c_void_p, c_int64, c_int, c_void_p],
    "dlt_gemm_wgrad": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                       c_void_p],
    "dlt_gemm_wgrad_sk": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                          c_int, c_void_p],
    "dlt_gemm_wgrad_grp": [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "dlt_scale_bf16": [c_void_p, c_void_p, ctypes.c_long, c_void_p, c_float, c_int, c_void_p],
    "dlt_gemm_bf16_tn": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                         c_void_p],
    "dlt_gemm_fw4": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                     c_int, c_void_p],
    "dlt_lmhead_loss": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                        c_int, c_int, c_int, c_int, c_void_p],
    "dlt_gemm_bf16_qkv_rope": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                               c_void_p],
    "dlt_gemm_bf16_gu_swiglu": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "dlt_gemm_bf16_nn": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                         c_void_p],
    "dlt_gemm_bf16_down_swiglu_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                      c_int, c_void_p],
    # (const dlt_attn_args*, stream): see _AttnArgs
    "dlt_attn_fwd": [c_void_p, c_void_p],
    "dlt_attn_bwd": [c_void_p, c_void_p],
    "dlt_attn_dropout_mask": [c_void_p, c_int, c_int, c_int, c_uint32, c_uint32, c_void_p],
    "dlt_attn_dropout_mask_band": [c_void_p, c_int, c_int, c_int, c_uint32, c_uint32, c_int, c_void_p],
    "dlt_attn_args_size": [],
    "dlt_rope_qk_inplace": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "dlt_qknorm_rope_inplace": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_int,
                                c_int, c_int, c_int, c_void_p],
    "dlt_qknorm_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int,
                       c_int, c_int, c_int, c_void_p],
    "dlt_postnorm_fwd": [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_float, c_int, c_void_p],
    "dlt_postnorm_add_dropout_rmsnorm_fwd": [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                             c_void_p, c_int, c_int, c_float, c_uint32, c_uint32, c_float, c_int,
                                             c_void_p],
    "dlt_postnorm_bwd": [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_float, c_int,
                         c_void_p],
    "dlt_dec_norm_qkv": [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "dlt_dec_attn": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p],
    "dlt_dec_norm_qkv_gqa": [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "dlt_dec_attn_gqa": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                         c_int, c_float, c_void_p],
    "dlt_dec_attn_win": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int,
                         c_void_p],
    "dlt_dec_attn_gqa_win": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_int, c_int, c_float, c_int, c_void_p],
    "dlt_dec_attn_sink": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int,
                          c_void_p, c_void_p],
    "dlt_dec_attn_gqa_sink": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                              c_int, c_int, c_float, c_int, c_void_p, c_void_p],
    "dlt_dec_attn_cap": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int,
                         c_void_p, c_float, c_void_p],
    "dlt_dec_attn_gqa_cap": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_int, c_int, c_float, c_int, c_void_p, c_float, c_void_p],
    "dlt_dec_gemv_res": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p],
    "dlt_dec_norm_gu": [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p],
    "dlt_dec_norm_head": [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p],
    "dlt_dec_norm_head_cap": [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                              c_void_p],
    "dlt_dec_sample": [c_void_p, c_int, c_int, c_float, c_int, c_uint32, c_void_p, c_void_p, c_void_p, c_int, c_int,
                       c_void_p, c_void_p],
    "dlt_dec_sample_p": [c_void_p, c_int, c_int, c_float, c_int, c_float, c_float, c_uint32, c_void_p, c_void_p, c_void_p,
                         c_int, c_int, c_void_p, c_void_p],
    "dlt_dec_sample_ws_ints": [c_int],
    "dlt_dec_advance": [c_void_p, c_void_p],
}


def library_path() -> str:
    return _LIBPATH


def lib():
    """Load (once) the kernel library; raises with a clear message if it is missing."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIBPATH):
            raise RuntimeError(
                f"MI355X kernel library not built: {_LIBPATH} missing. Run "
                "`python -m distributed_llm_trainer_amd.ops.build` (or __graft_entry__.build()).")
        import torch  # noqa: F401  (load torch's HIP runtime first so the .so binds to it)
        L = ctypes.CDLL(_LIBPATH)
        from . import hip_f32
        for name, argt in {**_SIGS, **hip_f32.SIGS}.items():
            fn = getattr(L, name)
            fn.argtypes = argt
            fn.restype = c_int
        L.dlt_gemm_wgrad_sk_scratch.argtypes = [c_int, c_int, c_int, c_int]
        L.dlt_gemm_wgrad_sk_scratch.restype = ctypes.c_long
        L.dlt_gemm_wgrad_grp_scratch.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p]
        L.dlt_gemm_wgrad_grp_scratch.restype = ctypes.c_long
        L.dlt_lmhead_loss_scratch.argtypes = [c_int, c_int]
        L.dlt_lmhead_loss_scratch.restype = ctypes.c_long
        L.dlt_qknorm_bwd_ws.argtypes = [c_int, c_int, c_int]
        L.dlt_qknorm_bwd_ws.restype = ctypes.c_long
        L.dlt_postnorm_bwd_ws.argtypes = [c_int, c_int]
        L.dlt_postnorm_bwd_ws.restype = ctypes.c_long
        if L.dlt_attn_args_size() != ctypes.sizeof(_AttnArgs):
            raise RuntimeError(f"{_LIBPATH}: dlt_attn_args is {L.dlt_attn_args_size()} bytes, _AttnArgs "
                               f"{ctypes.sizeof(_AttnArgs)}: rebuild the library (ops/build.py)")
        _LIB = L
    return _LIB


# ---------------------------------------------------------------- fused decode step
DECODE_BATCHES = (1, 2, 4, 8)


def _dec_w(t: torch.Tensor, name: str) -> None:
    if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError(f"{name}: expected a contiguous, 16-byte aligned bf16 weight")


def dec_norm_qkv(h, ln, eps, wqkv, cos, sin, pos, q_out, kc, vc, nh):
    """h [B, H] fp32 -> RMSNorm -> QKV GEMV -> RoPE; k/v rows written into the caches
    [B, nh, maxS, 64] at device position ``pos`` (int64 [1]); q (roped, bf16) into q_out."""
    B, H = h.shape
    _req(h, torch.float32, "dec.h", B * H)
    w, wbf16 = _norm_weight(ln, H, "dec.ln1")
    _dec_w(wqkv, "dec.wqkv")
    _req(q_out, torch.bfloat16, "dec.q", B * H)
    _req(pos, torch.int64, "dec.pos", 1)
    maxS = kc.shape[2]
    if kc.shape != (B, nh, maxS, 64) or vc.shape != kc.shape or wqkv.shape != (3 * H, H) or cos.shape[0] < maxS:
        raise ValueError("dec_norm_qkv: shape mismatch")
    _chk(lib().dlt_dec_norm_qkv(_p(h), _p(w), wbf16, float(eps), _p(wqkv), _p(cos), _p(sin), _p(pos), _p(q_out),
                                _p(kc), _p(vc), B, H, nh, maxS, _stream()), "dec_norm_qkv")


def _dec_window(window, name: str) -> int:
    """``window`` of the decode attention wrappers: 0 = none, W >= 1 = keys pos - W + 1 .. pos."""
    if isinstance(window, bool) or not isinstance(window, int) or window < 0 or window > 0x7FFFFFFF:
        raise ValueError(f"{name}: window must be an integer >= 0 (0: no window), got {window!r}")
    return window


def _dec_sink(sink, nh: int, device, name: str) -> torch.Tensor:
    """``sink`` of the decode attention wrappers: the layer's attention-sink logits, one per
    query head, as the kernels read them (fp32 [nh] on the caches' device; a 16-bit tensor is
    upcast).  Under a captured graph pass the fp32 parameter itself, so replays read it."""
    if not isinstance(sink, torch.Tensor) or not sink.is_floating_point() or tuple(sink.shape) != (nh,):
        raise ValueError(f"{name}: sink must be a floating-point [{nh}] tensor (one logit per query head)")
    if sink.device != device:
        raise ValueError(f"{name}: sink must be on {device}, got {sink.device}")
    if sink.dtype != torch.float32:
        sink = sink.float()
    if not sink.is_contiguous() or sink.data_ptr() % 4:
        sink = sink.contiguous().clone()
    return sink


def dec_attn(q, kc, vc, pos, o_out, scale, window=0, sink=None, softcap=None):
    """Decode attention of a multi-head model over keys 0..pos of the caches [B, nh, maxS, 64];
    ``window`` = W > 0: over keys max(0, pos - W + 1)..pos only (a sliding-window layer).
    ``sink`` (fp32 [nh]): attention sinks, one more softmax logit per head with no value row.
    ``softcap`` = CAP (finite, > 0): the scores are CAP * tanh(scale q.k / CAP) (the CAP kernels;
    the sink is not capped).  None: the call is what it was."""
    window = _dec_window(window, "dec_attn")
    B, nh, maxS, hd = kc.shape
    H = nh * hd
    _req(q, torch.bfloat16, "dec.q", B * H)
    _req(o_out, torch.bfloat16, "dec.o", B * H)
    if sink is not None or softcap is not None:
        cap = None if softcap is None else _score_cap(softcap, "dec_attn.softcap")
        if sink is not None:
            sink = _dec_sink(sink, nh, kc.device, "dec_attn")
        if hd != 64 or vc.shape != kc.shape:
            raise ValueError("dec_attn: caches must be [B, nh, maxS, 64]")
        _req(kc, torch.bfloat16, "dec.k_cache")
        _req(vc, torch.bfloat16, "dec.v_cache")
        _req(pos, torch.int64, "dec.pos", 1)
        if cap is not None:  # the CAP kernels: window 0 = none, a null sink = none
            _chk(lib().dlt_dec_attn_cap(_p(q), _p(kc), _p(vc), _p(pos), _p(o_out), B, H, nh, maxS, float(scale),
                                        window, _p(sink), cap, _stream()), "dec_attn_cap")
            return
        _chk(lib().dlt_dec_attn_sink(_p(q), _p(kc), _p(vc), _p(pos), _p(o_out), B, H, nh, maxS, float(scale), window,
                                     _p(sink), _stream()), "dec_attn_sink")
        return
    if window:
        if hd != 64 or vc.shape != kc.shape:
            raise ValueError("dec_attn: caches must be [B, nh, maxS, 64]")
        _req(kc, torch.bfloat16, "dec.k_cache")
        _req(vc, torch.bfloat16, "dec.v_cache")
        _req(pos, torch.int64, "dec.pos", 1)
        _chk(lib().dlt_dec_attn_win(_p(q), _p(kc), _p(vc), _p(pos), _p(o_out), B, H, nh, maxS, float(scale), window,
                                    _stream()), "dec_attn_win")
        return
    _chk(lib().dlt_dec_attn(_p(q), _p(kc), _p(vc), _p(pos), _p(o_out), B, H, nh, maxS, float(scale), _stream()),
         "dec_attn")


def dec_norm_qkv_gqa(h, ln, eps, wqkv, cos, sin, pos, q_out, kc, vc, nh, nkv):
    """:func:`dec_norm_qkv` for a grouped-query model: wqkv [H + 2 * nkv * 64, H] laid out
    q | k | v, caches [B, nkv, maxS, 64]; RoPE on the nh query and nkv key heads."""
    B, H = h.shape
    nkv = _req_nkv(nh, nkv, "dec_norm_qkv_gqa")
    _req(h, torch.float32, "dec.h", B * H)
    w, wbf16 = _norm_weight(ln, H, "dec.ln1")
    _dec_w(wqkv, "dec.wqkv")
    _req(q_out, torch.bfloat16, "dec.q", B * H)
    _req(pos, torch.int64, "dec.pos", 1)
    _req(kc, torch.bfloat16, "dec.k_cache")
    _req(vc, torch.bfloat16, "dec.v_cache")
    maxS = kc.shape[2] if kc.dim() == 4 else -1
    if (H != nh * 64 or kc.shape != (B, nkv, maxS, 64) or vc.shape != kc.shape
            or wqkv.shape != (H + 2 * nkv * 64, H) or cos.shape[0] < maxS or sin.shape[0] < maxS):
        raise ValueError("dec_norm_qkv_gqa: shape mismatch")
    _chk(lib().dlt_dec_norm_qkv_gqa(_p(h), _p(w), wbf16, float(eps), _p(wqkv), _p(cos), _p(sin), _p(pos), _p(q_out),
                                    _p(kc), _p(vc), B, H, nh, nkv, maxS, _stream()), "dec_norm_qkv_gqa")


DEC_ATTN_SPLITS = (1, 2, 4, 8)  # key chunks per K/V head of dec_attn_gqa
DEC_ATTN_GQA_HEADS = 16         # query heads per workgroup (GQA_GMAX in decode.hip)
DEC_ATTN_WS = 66                # fp32 per partial: o[64], m, l


def dec_attn_chunk(maxS: int, splits: int) -> int:
    """Keys per workgroup of :func:`dec_attn_gqa`: chunk s is [s * C, min((s + 1) * C, pos + 1))."""
    if splits not in DEC_ATTN_SPLITS or maxS < 1:
        raise ValueError(f"dec_attn_chunk: splits must be one of {DEC_ATTN_SPLITS} and maxS positive")
    return -(-maxS // splits)


def dec_attn_gqa_lds(G: int, C: int) -> int:
    """Bytes of LDS of a ``k_dec_attn_gqa`` workgroup: the scores of its (at most 16) query
    heads over its C keys, and the reduction, output and q areas (decode.hip dlt_dec_attn_gqa)."""
    gw = min(G, DEC_ATTN_GQA_HEADS)
    gt = next(t for t in (1, 2, 3, 4, 6, 8, 12, 16) if t >= gw)
    return gt * (C + 8 + 4 * 64 + 64) * 4


def dec_attn_gqa_workspace(B: int, nh: int, splits: int, device) -> torch.Tensor:
    """The fp32 partials [B, nh, splits, 66] of :func:`dec_attn_gqa` with ``splits`` > 1."""
    return torch.empty(B * nh * splits * DEC_ATTN_WS, dtype=torch.float32, device=device)


def dec_attn_gqa(q, kc, vc, pos, o_out, scale, nh, splits=1, ws=None, window=0, sink=None, softcap=None):
    """Decode attention of a grouped-query model: q, o_out [B, nh * 64] bf16, caches
    [B, nkv, maxS, 64]; every K/V row is read once for the nh / nkv query heads of its group.
    ``splits`` > 1 divides the keys over that many workgroups per K/V head (chunks of
    :func:`dec_attn_chunk`) and merges their partials, in order, through ``ws``
    (:func:`dec_attn_gqa_workspace`).  ``window`` = W > 0: keys max(0, pos - W + 1)..pos only,
    in chunks of ``dec_attn_chunk(min(W, maxS), splits)`` anchored at the window's first key.
    ``sink`` (fp32 [nh], per query head): attention sinks; with ``splits`` > 1 the merge adds the
    sink once.  ``softcap``: as in :func:`dec_attn`."""
    window = _dec_window(window, "dec_attn_gqa")
    if kc.dim() != 4 or kc.shape[3] != 64 or vc.shape != kc.shape:
        raise ValueError("dec_attn_gqa: caches must be [B, nkv, maxS, 64]")
    B, nkv, maxS, _ = kc.shape
    if isinstance(nh, bool) or not isinstance(nh, int) or nh < 1 or nh % nkv:
        raise ValueError(f"dec_attn_gqa: nkv ({nkv}) must divide nh ({nh})")
    if splits not in DEC_ATTN_SPLITS:
        raise ValueError(f"dec_attn_gqa: splits must be one of {DEC_ATTN_SPLITS}")
    H = nh * 64
    _req(q, torch.bfloat16, "dec.q", B * H)
    _req(o_out, torch.bfloat16, "dec.o", B * H)
    _req(kc, torch.bfloat16, "dec.k_cache")
    _req(vc, torch.bfloat16, "dec.v_cache")
    _req(pos, torch.int64, "dec.pos", 1)
    if splits > 1:
        if ws is None:
            raise ValueError("dec_attn_gqa: splits > 1 needs a workspace (dec_attn_gqa_workspace)")
        _req(ws, torch.float32, "dec.attn_ws", B * nh * splits * DEC_ATTN_WS)
    if sink is not None:
        sink = _dec_sink(sink, nh, kc.device, "dec_attn_gqa")
    if softcap is not None:  # the CAP kernels: window 0 = none, a null sink = none
        cap = _score_cap(softcap, "dec_attn_gqa.softcap")
        _chk(lib().dlt_dec_attn_gqa_cap(_p(q), _p(kc), _p(vc), _p(pos), _p(o_out), _p(ws if splits > 1 else None), B,
                                        H, nh, nkv, maxS, splits, float(scale), window, _p(sink), cap, _stream()),
             "dec_attn_gqa_cap")
        return
    if sink is not None:
        _chk(lib().dlt_dec_attn_gqa_sink(_p(q), _p(kc), _p(vc), _p(pos), _p(o_out), _p(ws if splits > 1 else None), B,
                                         H, nh, nkv, maxS, splits, float(scale), window, _p(sink), _stream()),
             "dec_attn_gqa_sink")
        return
    if window:
        _chk(lib().dlt_dec_attn_gqa_win(_p(q), _p(kc), _p(vc), _p(pos), _p(o_out), _p(ws if splits > 1 else None), B,
                                        H, nh, nkv, maxS, splits, float(scale), window, _stream()),
             "dec_attn_gqa_win")
        return
    _chk(lib().dlt_dec_attn_gqa(_p(q), _p(kc), _p(vc), _p(pos), _p(o_out), _p(ws if splits > 1 else None), B, H, nh,
                                nkv, maxS, splits, float(scale), _stream()), "dec_attn_gqa")


def dec_gemv_res(x, w, h):
    """h += bf16(x @ w^T) (fp32 residual); x [B, K] bf16, w [R, K] bf16, h [B, R] fp32."""
    B, K = x.shape
    R = w.shape[0]
    _req(x, torch.bfloat16, "dec.x", B * K)
    _dec_w(w, "dec.w")
    _req(h, torch.float32, "dec.h", B * R)
    if w.shape[1] != K:
        raise ValueError("dec_gemv_res: shape mismatch")
    _chk(lib().dlt_dec_gemv_res(_p(x), _p(w), _p(h), B, R, K, _stream()), "dec_gemv_res")


def dec_norm_gu(h, ln, eps, wgu, s_out):
    B, H = h.shape
    I = wgu.shape[0] // 2
    _req(h, torch.float32, "dec.h", B * H)
    w, wbf16 = _norm_weight(ln, H, "dec.ln2")
    _dec_w(wgu, "dec.wgu")
    _req(s_out, torch.bfloat16, "dec.s", B * I)
    _chk(lib().dlt_dec_norm_gu(_p(h), _p(w), wbf16, float(eps), _p(wgu), _p(s_out), B, H, I, _stream()),
         "dec_norm_gu")


def dec_norm_head(h, ln, eps, emb, logits, V, softcap: float = 0.0):
    """``softcap`` (0 = off): the model's final-logit cap, logits = cap * tanh(logits / cap) (the CAP kernel)."""
    cap = _cap32(softcap, "dec_norm_head.softcap")
    B, H = h.shape
    _req(h, torch.float32, "dec.h", B * H)
    w, wbf16 = _norm_weight(ln, H, "dec.norm")
    _dec_w(emb, "dec.lm_head")
    _req(logits, torch.float32, "dec.logits", B * V)
    if emb.shape[0] < V or emb.shape[1] != H:
        raise ValueError("dec_norm_head: shape mismatch")
    if cap != 0.0:
        _chk(lib().dlt_dec_norm_head_cap(_p(h), _p(w), wbf16, float(eps), _p(emb), _p(logits), B, H, V, cap,
                                         _stream()), "dec_norm_head_cap")
        return
    _chk(lib().dlt_dec_norm_head(_p(h), _p(w), wbf16, float(eps), _p(emb), _p(logits), B, H, V, _stream()),
         "dec_norm_head")


def dec_sample_workspace(B: int, device) -> torch.Tensor:
    """Scratch of the split (16 workgroups per row) top-k sampler."""
    return torch.empty(int(lib().dlt_dec_sample_ws_ints(B)), dtype=torch.int32, device=device)


def check_top_p_min_p(top_p, min_p):
    """(top_p, min_p) as floats; ValueError unless 0 < top_p <= 1 and 0 <= min_p < 1 (a NaN
    or an infinity fails either comparison)."""
    top_p, min_p = float(top_p), float(min_p)
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p={top_p}: expected 0 < top_p <= 1 (1: no nucleus filter)")
    if not 0.0 <= min_p < 1.0:
        raise ValueError(f"min_p={min_p}: expected 0 <= min_p < 1 (0: no min-p filter)")
    return top_p, min_p


def dec_sample(logits, temperature, top_k, seed, pos, ids, hist, hist_base, ws=None, top_p=1.0, min_p=0.0):
    """One top-k multinomial draw per row of ``logits`` [B, V] (fp32) on the device: the
    id goes to ``ids`` (B int64, the next decode step's input) and to
    ``hist[b, pos + 1 - hist_base]`` (int64 [B, L]) when inside the history.  With ``ws``
    (:func:`dec_sample_workspace`) and 1 <= top_k <= 64 the row is split over 16
    workgroups.  ``top_p`` < 1 (nucleus over what top-k leaves) and ``min_p`` > 0 (keep
    p >= min_p * p_max) raise the threshold further in the kernels' ``NUC`` forms; with both
    off this launches the plain kernels."""
    top_p, min_p = check_top_p_min_p(top_p, min_p)
    B, V = logits.shape
    if ws is not None:
        _req(ws, torch.int32, "dec.sample_ws", int(lib().dlt_dec_sample_ws_ints(B)))
    _req(logits, torch.float32, "dec.logits", B * V)
    _req(pos, torch.int64, "dec.pos", 1)
    _req(ids, torch.int64, "dec.ids", B)
    _req(hist, torch.int64, "dec.hist")
    if hist.dim() != 2 or hist.shape[0] != B:
        raise ValueError("dec_sample: hist must be [B, L]")
    # the kernels take fp32: decide on the rounded values (a top_p that rounds to 1 is off; a
    # min_p that rounds to 1 is the largest fp32 below it)
    top_p, min_p = max(c_float(top_p).value, 2.0 ** -126), min(c_float(min_p).value, 1.0 - 2.0 ** -24)
    if top_p == 1.0 and min_p == 0.0:
        _chk(lib().dlt_dec_sample(_p(logits), B, V, float(temperature), int(top_k), int(seed) & 0xFFFFFFFF, _p(pos),
                                  _p(ids), _p(hist), hist.shape[1], int(hist_base), _p(ws), _stream()), "dec_sample")
        return
    if V >= 1 << 24:
        raise ValueError("dec_sample: top_p / min_p need V < 2^24 (40-bit fixed-point mass sums)")
    _chk(lib().dlt_dec_sample_p(_p(logits), B, V, float(temperature), int(top_k), top_p, min_p,
                                int(seed) & 0xFFFFFFFF, _p(pos), _p(ids), _p(hist), hist.shape[1], int(hist_base),
                                _p(ws), _stream()), "dec_sample")


def dec_advance(pos):
    _req(pos, torch.int64, "dec.pos", 1)
    _chk(lib().dlt_dec_advance(_p(pos), _stream()), "dec_advance")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"{name} failed (code {rc})")


def _req(t: torch.Tensor, dtype, name: str, numel: Optional[int] = None):
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a GPU tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name}: expected {numel} elements, got {t.numel()}")
    if t.data_ptr() % 16:
        raise ValueError(f"{name}: must be 16-byte aligned")


# 16-bit activation formats of the kernels (csrc/common.h HK): bf16 = 0, fp16 = 1
_HK = {torch.bfloat16: 0, torch.float16: 1}


def _hk(t: torch.Tensor, name: str) -> int:
    if t.dtype not in _HK:
        raise TypeError(f"{name}: expected bf16 or fp16 activations, got {t.dtype}")
    return _HK[t.dtype]


def _req_act(t: torch.Tensor, dtype, name: str, numel: Optional[int] = None) -> int:
    """_req for a 16-bit activation tensor of the given format; returns its HK code."""
    if dtype not in _HK:
        raise TypeError(f"{name}: the HIP kernels take bf16 or fp16 activations, not {dtype}")
    _req(t, dtype, name, numel)
    return _HK[dtype]


# ------------------------------------------------------------------ tables
def rope_tables(head_dim: int, seq_len: int, device=None):
    from .reference import rope_tables as rt
    c, s = rt(head_dim, seq_len, device=device)
    return c.contiguous(), s.contiguous()


# ---------------------------------------------------------------- split-K
def splitk_acc(part: torch.Tensor, dw: torch.Tensor) -> None:
    """dw += part.sum(0) in fixed order (deterministic); part [splits, *dw.shape] fp32."""
    _req(dw, torch.float32, "splitk_acc.dw")
    _req(part, torch.float32, "splitk_acc.part")
    n = dw.numel()
    if part.numel() % n or n % 4:
        raise ValueError("splitk_acc: part must hold whole copies of dw and dw.numel() % 4 == 0")
    _chk(lib().dlt_splitk_acc(_p(part), _p(dw), n, part.numel() // n, _stream()), "splitk_acc")


def splitk_sum_bf16(part: torch.Tensor, out: torch.Tensor) -> None:
    """out (bf16 or fp16) = part.sum(0) in fixed order; part [splits, *out.shape] fp32."""
    hk = _req_act(out, out.dtype, "splitk_sum_bf16.out")
    _req(part, torch.float32, "splitk_sum_bf16.part")
    n = out.numel()
    if part.numel() % n or n % 4 or out.data_ptr() % 8:
        raise ValueError("splitk_sum_bf16: part must hold whole copies of out, out.numel() % 4 == 0")
    _chk(lib().dlt_splitk_sum_bf16(_p(part), _p(out), n, part.numel() // n, hk, _stream()), "splitk_sum_bf16")


# ---------------------------------------------------------------- embedding
def embedding_fwd(ids: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    ids = ids.reshape(-1).contiguous()
    if ids.dtype != torch.int64:
        ids = ids.long()
    M = ids.numel()
    V, H = weight.shape
    wdt = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}.get(weight.dtype)
    if wdt is None:
        raise TypeError("embedding weight must be fp32, bf16 or fp16")
    _req(weight, weight.dtype, "embedding.weight")
    out = torch.empty(M, H, dtype=torch.float32, device=weight.device)
    _chk(lib().dlt_embedding_fwd(_p(ids), _p(weight), wdt, _p(out), M, H, V, _stream()), "embedding_fwd")
    return out


def embedding_bwd(ids: torch.Tensor, dout: torch.Tensor, dweight: torch.Tensor) -> None:
    """dweight[ids[m]] += dout[m], deterministically: a stable sort groups equal ids
    (rocPRIM radix sort via torch.sort), the kernels sum each run in position order
    with one writer per row (no float atomics)."""
    ids = ids.reshape(-1)
    M = ids.numel()
    H = dweight.shape[-1]
    _req(dout, torch.float32, "embedding_bwd.dout", M * H)
    _req(dweight, torch.float32, "embedding_bwd.dweight")
    if M == 0:
        return
    if dweight.shape[0] >= 2 ** 31:
        raise ValueError("embedding_bwd: vocabulary too large for int32 ids")
    sids, perm = torch.sort(ids.to(torch.int32), stable=True)  # 32-bit keys: half the radix passes
    ch = lib().dlt_embedding_bwd_chunk()
    ws = torch.empty(2 * (-(-M // ch)) * H, dtype=torch.float32, device=dout.device)
    _chk(lib().dlt_embedding_bwd(_p(sids), _p(perm), _p(dout), _p(dweight), _p(ws), M, H, dweight.shape[0],
                                 _stream()), "embedding_bwd")


# ---------------------------------------------------------------- RMSNorm
def _norm_weight(weight: torch.Tensor, H: int, name: str, act=torch.bfloat16):
    """(tensor, is_16bit): fp32 norm weights, and 16-bit ones in the activation format
    (the gathered FSDP unit), are read in place by the kernels; others are upcast once."""
    if weight.dtype not in (torch.float32, act):
        weight = weight.float()
    align = 8 if weight.dtype != torch.float32 else 16  # u16x4 / float4 loads
    if not weight.is_contiguous() or weight.data_ptr() % align:
        weight = weight.contiguous().clone()
    if not weight.is_cuda or weight.numel() != H:
        raise ValueError(f"{name}: expected a GPU tensor of {H} elements")
    return weight, int(weight.dtype != torch.float32)


def add_dropout_rmsnorm_fwd(resid, delta, weight, eps, p, key, out_dtype=torch.bfloat16, y_out=None):
    if out_dtype == torch.float32:
        from . import hip_f32
        return hip_f32.add_dropout_rmsnorm_fwd(resid, delta, weight, eps, p, key, y_out=y_out)
    src = resid if resid is not None else delta
    M, H = src.shape
    if out_dtype not in _HK:
        raise TypeError("HIP rmsnorm emits bf16 or fp16")
    if resid is not None:
        _req(resid, torch.float32, "rmsnorm.resid", M * H)
    if delta is not None:
        _req_act(delta, out_dtype, "rmsnorm.delta", M * H)
    w, wbf16 = _norm_weight(weight, H, "rmsnorm.weight", out_dtype)
    y = torch.empty(M, H, dtype=out_dtype, device=src.device) if y_out is None else y_out
    hk = _req_act(y, out_dtype, "rmsnorm.y", M * H)
    rstd = torch.empty(M, dtype=torch.float32, device=src.device)
    if delta is None:
        x, xo = resid, None       # x is just the residual: no copy
    else:
        x = torch.empty(M, H, dtype=torch.float32, device=src.device)
        xo = x
    thr = rng.keep_threshold(p)
    dscale = 1.0 / (1.0 - p) if thr else 1.0
    _chk(lib().dlt_add_dropout_rmsnorm_fwd(_p(resid), _p(delta), _p(w), wbf16, _p(xo), _p(y), _p(rstd), M, H,
                                           float(eps),
                                           key & 0xFFFFFFFF, thr, dscale, hk, _stream()), "add_dropout_rmsnorm_fwd")
    return x, y, rstd


def rmsnorm_bwd(dy, x, rstd, weight, dres, dweight, p_prev, key_prev, dy_scale=None, want_ddelta=True,
                ddelta_out=None, dy_mul: float = 1.0):
    if dy.dtype == torch.float32:
        from . import hip_f32
        return hip_f32.rmsnorm_bwd(dy, x, rstd, weight, dres, dweight, p_prev, key_prev, dy_scale, want_ddelta, ddelta_out,
                                   dy_mul)
    M, H = x.shape
    act = dy.dtype
    hk = _req_act(dy, act, "rmsnorm_bwd.dy", M * H)
    _req(x, torch.float32, "rmsnorm_bwd.x", M * H)
    _req(rstd, torch.float32, "rmsnorm_bwd.rstd", M)
    if dres is not None:
        _req(dres, torch.float32, "rmsnorm_bwd.dres", M * H)
    _req(dweight, torch.float32, "rmsnorm_bwd.dweight", H)
    w, wbf16 = _norm_weight(weight, H, "rmsnorm_bwd.weight", act)
    scale_t = None
    if dy_scale is not None:
        scale_t = dy_scale.reshape(1).float().contiguous()
    dx = torch.empty(M, H, dtype=torch.float32, device=x.device)
    dd = None
    if want_ddelta:
        dd = torch.empty(M, H, dtype=act, device=x.device) if ddelta_out is None else ddelta_out
        _req(dd, act, "rmsnorm_bwd.ddelta", M * H)
    thr = rng.keep_threshold(p_prev)
    dscale = 1.0 / (1.0 - p_prev) if thr else 1.0
    # per-block dw partials (two-stage column reduction instead of same-address atomics)
    ws = torch.empty(min((M + 3) // 4, 1024) * H, dtype=torch.float32, device=x.device)
    _chk(lib().dlt_rmsnorm_bwd(_p(dy), _p(x), _p(rstd), _p(w), wbf16, _p(dres), _p(dx), _p(dd), _p(dweight), _p(ws),
                               _p(scale_t), float(dy_mul), M, H, key_prev & 0xFFFFFFFF, thr, dscale, hk, _stream()),
         "rmsnorm_bwd")
    return dx, dd


# ------------------------------------------------------------------- RoPE
def _no_split_gqa(name: str):
    raise NotImplementedError(f"{name}: grouped-query attention runs on the packed QKV layout "
                              "(rope_qk_inplace + attention_fwd_packed / attention_bwd_packed with nkv=)")


def rope_qkv_fwd(qkv, B, S, nh, cos, sin, nkv=None):
    if nkv is not None and nkv != nh:
        _no_split_gqa("rope_qkv_fwd")
    if qkv.dtype == torch.float32:
        from . import hip_f32
        return hip_f32.rope_qkv_fwd(qkv, B, S, nh, cos, sin)
    M, threeH = qkv.shape
    hd = threeH // (3 * nh)
    if M != B * S or hd * 3 * nh != threeH:
        raise ValueError("rope_qkv_fwd: bad shapes")
    hk = _req_act(qkv, qkv.dtype, "rope.qkv")
    if cos.shape[0] < S or cos.shape[1] != hd // 2:
        raise ValueError("rope tables too short")
    q = torch.empty(B, nh, S, hd, dtype=qkv.dtype, device=qkv.device)
    k = torch.empty_like(q)
    v = torch.empty_like(q)
    _chk(lib().dlt_rope_qkv_fwd(_p(qkv), _p(cos), _p(sin), _p(q), _p(k), _p(v), B, S, nh, hd, hk, _stream()),
         "rope_qkv_fwd")
    return q, k, v


def rope_qkv_bwd(dq, dk, dv, cos, sin, out=None):
    if dk.dtype == torch.float32:
        from . import hip_f32
        return hip_f32.rope_qkv_bwd(dq, dk, dv, cos, sin, out=out)
    B, nh, S, hd = dk.shape
    if dq.dim() == 4 and dq.shape[1] != nh:
        _no_split_gqa("rope_qkv_bwd")
    act = dk.dtype
    for t, n in ((dk, "dk"), (dv, "dv")):
        hk = _req_act(t, act, "rope_bwd." + n, B * nh * S * hd)
    dqf = dq if dq.dtype == torch.float32 else None
    dqb = dq if dq.dtype == act else None
    _req(dq, dq.dtype, "rope_bwd.dq", B * nh * S * hd)
    if out is None:
        out = torch.empty(B * S, 3 * nh * hd, dtype=act, device=dk.device)
    _req(out, act, "rope_bwd.out", B * S * 3 * nh * hd)
    _chk(lib().dlt_rope_qkv_bwd(_p(dqb), _p(dqf), _p(dk), _p(dv), _p(cos), _p(sin), _p(out), B, S, nh, hd, hk,
                                _stream()),
         "rope_qkv_bwd")
    return out


def _req_nkv(nh: int, nkv, name: str) -> int:
    """Validated number of K/V heads of a grouped-query call."""
    if isinstance(nkv, bool) or not isinstance(nkv, int):
        raise TypeError(f"{name}: nkv must be an int or None, got {type(nkv).__name__}")
    if nkv < 1 or nh % nkv:
        raise ValueError(f"{name}: nkv ({nkv}) must divide nh ({nh})")
    return nkv


def rope_qk_inplace(qkv, B, S, nh, cos, sin, nkv=None):
    """Rotate the q and k column blocks of the packed [B*S, 3H] QKV in place.  With ``nkv``
    (grouped-query attention) the row is [B*S, H + 2*KV]: nh q heads | nkv k heads | nkv v heads."""
    if nkv is not None:
        nkv = _req_nkv(nh, nkv, "rope_qk_inplace")
    if qkv.dtype == torch.float32:
        return _f32("rope_qk_inplace", qkv.shape[1] // (3 * nh), nkv=nkv).rope_qk_inplace(qkv, B, S, nh, cos, sin)
    M, Wd = qkv.shape
    heads = 3 * nh if nkv is None else nh + 2 * nkv
    hd = Wd // heads
    if M != B * S or hd * heads != Wd or hd % 16:
        raise ValueError("rope_qk_inplace: bad shapes" if nkv is None else
                         "rope_qk_inplace: qkv must be [B*S, (nh + 2*nkv)*hd] with hd % 16 == 0")
    hk = _req_act(qkv, qkv.dtype, "rope_qk.qkv")
    if cos.shape[0] < S or cos.shape[1] != hd // 2 or sin.shape != cos.shape:
        raise ValueError("rope tables too short")
    _req(cos, torch.float32, "rope_qk.cos")
    _req(sin, torch.float32, "rope_qk.sin")
    _chk(lib().dlt_rope_qk_inplace(_p(qkv), _p(cos), _p(sin), M, S, nh, nkv or 0, hd, hk, _stream()),
         "rope_qk_inplace" if nkv is None else "rope_qk_inplace_gqa")
    return qkv


# ---------------------------------------------------------------- QK-norm
def _qknorm_dims(t, B, S, nh, nkv, name: str):
    """(nkv, hd) of a packed [B*S, (nh + 2*nkv)*hd] tensor of a QK-norm call (hd 64 / 128)."""
    nkv = nh if nkv is None else _req_nkv(nh, nkv, name)
    if t.dtype == torch.float32:
        raise NotImplementedError(f"{name}: QK-norm is not implemented for fp32 activations on the GPU")
    if t.dim() != 2 or B < 1 or S < 1 or nh < 1:
        raise ValueError(f"{name}: expected a [B*S, (nh + 2*nkv)*hd] tensor")
    M, Wd = t.shape
    heads = nh + 2 * nkv
    hd = Wd // heads
    if M != B * S or hd * heads != Wd:
        raise ValueError(f"{name}: expected [B*S, (nh + 2*nkv)*hd] = [{B * S}, {heads}*hd], got {list(t.shape)}")
    if hd not in ATTN_HEAD_DIMS:
        raise NotImplementedError(f"{name}: QK-norm needs head_dim in {tuple(ATTN_HEAD_DIMS)} on the GPU, got {hd}")
    if M * Wd >= 2 ** 31:
        raise ValueError(f"{name}: {M} x {Wd} elements overflow the kernel's 32-bit index")
    return nkv, hd


def _qknorm_weight(w: torch.Tensor, hd: int, name: str) -> torch.Tensor:
    """The [hd] norm weight as the kernels read it: fp32, contiguous, 16-byte aligned (the
    flat master is; a gathered 16-bit FSDP unit is upcast, hd elements)."""
    if not isinstance(w, torch.Tensor) or not w.is_cuda or w.numel() != hd:
        raise ValueError(f"{name}: expected a GPU tensor of {hd} elements")
    if w.dtype != torch.float32:
        w = w.float()
    if not w.is_contiguous() or w.data_ptr() % 16:
        w = w.contiguous().clone()
    return w


def qknorm_rope_inplace(qkv, B, S, nh, cos, sin, qw, kw, eps, raw_out, nkv=None):
    """QK-norm + RoPE of the q and k heads of the packed [B*S, (nh + 2*nkv)*hd] QKV in place:
    head vector x -> rope(x * rsqrt(mean(x^2) + eps) * w), w = ``qw`` / ``kw`` ([hd]); fp32
    math, one rounding; v untouched.  ``raw_out`` [B*S, (nh + nkv)*hd] receives the pre-norm
    q|k values (the backward's input)."""
    nkv, hd = _qknorm_dims(qkv, B, S, nh, nkv, "qknorm_rope_inplace")
    M = B * S
    hk = _req_act(qkv, qkv.dtype, "qknorm_rope.qkv")
    _req(raw_out, qkv.dtype, "qknorm_rope.raw_out", M * (nh + nkv) * hd)
    if raw_out.device != qkv.device:
        raise ValueError("qknorm_rope.raw_out: expected the device of qkv")
    if cos.dim() != 2 or cos.shape[0] < S or cos.shape[1] != hd // 2 or sin.shape != cos.shape:
        raise ValueError("qknorm_rope_inplace: rope tables too short")
    _req(cos, torch.float32, "qknorm_rope.cos")
    _req(sin, torch.float32, "qknorm_rope.sin")
    qw = _qknorm_weight(qw, hd, "qknorm_rope.qw")
    kw = _qknorm_weight(kw, hd, "qknorm_rope.kw")
    _chk(lib().dlt_qknorm_rope_inplace(_p(qkv), _p(raw_out), _p(cos), _p(sin), _p(qw), _p(kw), float(eps), M, S, nh,
                                       nkv, hd, hk, _stream()), "qknorm_rope_inplace")
    return qkv


def qknorm_bwd_workspace(M: int, nh: int, hd: int, device) -> torch.Tensor:
    """fp32 workspace of :func:`qknorm_bwd`: the per-workgroup weight-gradient partials."""
    n = lib().dlt_qknorm_bwd_ws(M, nh, hd)
    if n <= 0:
        raise ValueError(f"qknorm_bwd: no kernel for M={M}, nh={nh}, hd={hd}")
    return torch.empty(n, dtype=torch.float32, device=device)


def qknorm_bwd(dqkv, raw, B, S, nh, qw, kw, eps, dqw, dkw, nkv=None, ws=None):
    """Backward of the norm of :func:`qknorm_rope_inplace`.  The q|k columns of the packed
    gradient ``dqkv`` (as ``attention_bwd_packed`` leaves it: dL/du, inverse rotation applied)
    are overwritten in place with dL/dx; v columns untouched.  ``dqw`` / ``dkw`` (fp32 [hd])
    += sum over tokens and heads of g * xh, reduced in a fixed order (no atomics)."""
    nkv, hd = _qknorm_dims(dqkv, B, S, nh, nkv, "qknorm_bwd")
    M = B * S
    hk = _req_act(dqkv, dqkv.dtype, "qknorm_bwd.dqkv")
    _req(raw, dqkv.dtype, "qknorm_bwd.raw", M * (nh + nkv) * hd)
    qw = _qknorm_weight(qw, hd, "qknorm_bwd.qw")
    kw = _qknorm_weight(kw, hd, "qknorm_bwd.kw")
    _req(dqw, torch.float32, "qknorm_bwd.dqw", hd)
    _req(dkw, torch.float32, "qknorm_bwd.dkw", hd)
    if ws is None:
        ws = qknorm_bwd_workspace(M, nh, hd, dqkv.device)
    else:
        _req(ws, torch.float32, "qknorm_bwd.ws", lib().dlt_qknorm_bwd_ws(M, nh, hd))
    for t, n in ((raw, "raw"), (dqw, "dqw"), (dkw, "dkw"), (ws, "ws")):
        if t.device != dqkv.device:
            raise ValueError(f"qknorm_bwd.{n}: expected the device of dqkv")
    _chk(lib().dlt_qknorm_bwd(_p(dqkv), _p(raw), _p(qw), _p(kw), _p(dqw), _p(dkw), _p(ws), float(eps), M, nh, nkv,
                              hd, hk, _stream()), "qknorm_bwd")
    return dqkv


# ---------------------------------------------------------------- post-norms
def _postnorm_dims(a, name: str):
    """(M, H) of a branch output [M, H] of a post-norm call: 16-bit, H % 4 == 0, H <= 4096."""
    if not isinstance(a, torch.Tensor) or a.dim() != 2:
        raise ValueError(f"{name}: expected a [M, H] tensor")
    if a.dtype == torch.float32:
        raise NotImplementedError(f"{name}: post-norms are not implemented for fp32 activations on the GPU")
    if a.dtype not in _HK:
        raise TypeError(f"{name}: expected bf16 or fp16 activations, got {a.dtype}")
    M, H = a.shape
    if M < 1 or H < 4 or H % 4 or H > 4096:
        raise ValueError(f"{name}: needs M >= 1, H % 4 == 0 and H <= 4096, got [{M}, {H}]")
    return M, H


def _postnorm_weight(w, H: int, act, device, name: str):
    """(tensor, is_16bit) of an [H] post-norm weight: validated, then as _norm_weight reads it."""
    if not isinstance(w, torch.Tensor) or not w.is_cuda or w.numel() != H or w.device != device:
        raise ValueError(f"{name}: expected a GPU tensor of {H} elements on the device of the activations")
    return _norm_weight(w, H, name, act)


def postnorm_fwd(a, w, eps, out=None):
    """The post-norm of a branch output: u = round(a * rsqrt(mean(a^2) + eps) * w) over the rows of
    ``a`` [M, H] (bf16 / fp16, as the GEMM rounded it), fp32 math, one rounding; ``w`` [H] fp32 or in
    the activation format.  Out of place: returns ``out`` (or a new tensor)."""
    M, H = _postnorm_dims(a, "postnorm_fwd.a")
    hk = _req_act(a, a.dtype, "postnorm_fwd.a")
    wt, w16 = _postnorm_weight(w, H, a.dtype, a.device, "postnorm_fwd.w")
    u = torch.empty_like(a) if out is None else out
    _req(u, a.dtype, "postnorm_fwd.out", M * H)
    if u.device != a.device:
        raise ValueError("postnorm_fwd.out: expected the device of a")
    if u.data_ptr() == a.data_ptr():
        raise ValueError("postnorm_fwd.out: the kernel is out of place (the backward reads the raw a)")
    _chk(lib().dlt_postnorm_fwd(_p(a), _p(wt), w16, _p(u), M, H, float(eps), hk, _stream()), "postnorm_fwd")
    return u


def postnorm_add_dropout_rmsnorm_fwd(resid, a, w_post, w, eps, p, key, out_dtype=torch.bfloat16, y_out=None):
    """:func:`postnorm_fwd` of ``a`` with ``w_post`` followed by :func:`add_dropout_rmsnorm_fwd`
    (resid, u, w, ...) in one kernel: the same bits for (x, y, rstd), and the normed branch u
    never goes to memory.  ``resid`` fp32 [M, H]; ``a`` [M, H] in ``out_dtype``."""
    if out_dtype == torch.float32:
        raise NotImplementedError("postnorm_add_dropout_rmsnorm_fwd: post-norms are not implemented for fp32 "
                                  "activations on the GPU")
    M, H = _postnorm_dims(a, "postnorm_rmsnorm.a")
    hk = _req_act(a, out_dtype, "postnorm_rmsnorm.a")
    if not isinstance(resid, torch.Tensor):
        raise ValueError("postnorm_rmsnorm.resid: expected the fp32 residual [M, H]")
    _req(resid, torch.float32, "postnorm_rmsnorm.resid", M * H)
    if resid.device != a.device:
        raise ValueError("postnorm_rmsnorm.resid: expected the device of a")
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"postnorm_rmsnorm: dropout p ({p}) must be in [0, 1)")
    wp, wp16 = _postnorm_weight(w_post, H, out_dtype, a.device, "postnorm_rmsnorm.w_post")
    wn, wn16 = _postnorm_weight(w, H, out_dtype, a.device, "postnorm_rmsnorm.w")
    y = torch.empty(M, H, dtype=out_dtype, device=a.device) if y_out is None else y_out
    _req(y, out_dtype, "postnorm_rmsnorm.y", M * H)
    if y.device != a.device:
        raise ValueError("postnorm_rmsnorm.y: expected the device of a")
    x = torch.empty(M, H, dtype=torch.float32, device=a.device)
    rstd = torch.empty(M, dtype=torch.float32, device=a.device)
    thr = rng.keep_threshold(p)
    dscale = 1.0 / (1.0 - p) if thr else 1.0
    _chk(lib().dlt_postnorm_add_dropout_rmsnorm_fwd(_p(resid), _p(a), _p(wp), wp16, _p(wn), wn16, _p(x), _p(y),
                                                    _p(rstd), M, H, float(eps), key & 0xFFFFFFFF, thr, dscale, hk,
                                                    _stream()), "postnorm_add_dropout_rmsnorm_fwd")
    return x, y, rstd


def postnorm_bwd_workspace(M: int, H: int, device) -> torch.Tensor:
    """fp32 workspace of :func:`postnorm_bwd`: the per-workgroup weight-gradient partials."""
    n = lib().dlt_postnorm_bwd_ws(int(M), int(H))
    if n <= 0:
        raise ValueError(f"postnorm_bwd: no kernel for M={M}, H={H}")
    return torch.empty(n, dtype=torch.float32, device=device)


def postnorm_bwd(du, a, w, eps, dw, ws=None):
    """Backward of :func:`postnorm_fwd`, in place: ``du`` [M, H] (dL/du, 16-bit) is overwritten with
    da = rstd * (g - xh * mean(g * xh)), g = du * w, xh = a * rstd, rstd recomputed from the raw
    ``a``; ``dw`` (fp32 [H]) += sum over rows of du * xh, reduced in a fixed order (no atomics)."""
    M, H = _postnorm_dims(du, "postnorm_bwd.du")
    hk = _req_act(du, du.dtype, "postnorm_bwd.du")
    if not isinstance(a, torch.Tensor):
        raise ValueError("postnorm_bwd.a: expected the raw branch output [M, H]")
    _req(a, du.dtype, "postnorm_bwd.a", M * H)
    if tuple(a.shape) != (M, H):
        raise ValueError(f"postnorm_bwd.a: expected [{M}, {H}], got {list(a.shape)}")
    if a.data_ptr() == du.data_ptr():
        raise ValueError("postnorm_bwd.a: must not alias du (du is rewritten in place)")
    wt, w16 = _postnorm_weight(w, H, du.dtype, du.device, "postnorm_bwd.w")
    _req(dw, torch.float32, "postnorm_bwd.dw", H)
    n_ws = lib().dlt_postnorm_bwd_ws(M, H)
    if ws is None:
        ws = torch.empty(n_ws, dtype=torch.float32, device=du.device)
    else:
        _req(ws, torch.float32, "postnorm_bwd.ws", n_ws)
    for t, n in ((a, "a"), (dw, "dw"), (ws, "ws")):
        if t.device != du.device:
            raise ValueError(f"postnorm_bwd.{n}: expected the device of du")
    _chk(lib().dlt_postnorm_bwd(_p(du), _p(a), _p(wt), w16, _p(dw), _p(ws), M, H, float(eps), hk, _stream()),
         "postnorm_bwd")
    return du


def _off(t: torch.Tensor, elems: int):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


# -------------------------------------------------------------- attention
class AttnAux(tuple):
    """(lse [B,nh,S] fp32, keep-bit masks [2, B*nh, ceil(S/32), S] int32 or None:
    [0] = bits by (key word, query), [1] = bits by (query word, key); word-major)."""


# head dims of the 16-bit MFMA attention kernels (template parameter D of attention.hip)
ATTN_HEAD_DIMS = (64, 128)


def _req_window(window, name: str):
    """``window`` of the attention wrappers: None, or W >= 1 keys per query with its own."""
    if window is None:
        return None
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise ValueError(f"{name}: window must be None or an integer >= 1, got {window!r}")
    return min(window, 0x7FFFFFFF)


def attention_dropout_mask(B, nh, S, p, key, device=None, window=None, out=None):
    """Keep-bit masks [2, B*nh, ceil(S/32), S] for attention dropout (None if p == 0).
    Data-independent, so the engine builds them on a side stream ahead of time.  ``window``:
    only the 32x32 bit tiles a sliding-window layer of that many keys reads are hashed and
    written (the same bits, the same layout; the rest of the buffer is left as it is).
    ``out``: write into this buffer instead of a new one."""
    thr = rng.keep_threshold(p)
    if not thr:
        return None
    window = _req_window(window, "attention_dropout_mask")
    if out is None:
        mask = torch.empty(2, B * nh, (S + 31) // 32, S, dtype=torch.int32, device=device)
    else:
        mask = out
        _req(mask, torch.int32, "attn.mask", 2 * B * nh * S * ((S + 31) // 32))
    if window is not None and window < S:
        _chk(lib().dlt_attn_dropout_mask_band(_p(mask), B, nh, S, key & 0xFFFFFFFF, thr, window, _stream()),
             "attn_dropout_mask_band")
    else:
        _chk(lib().dlt_attn_dropout_mask(_p(mask), B, nh, S, key & 0xFFFFFFFF, thr, _stream()), "attn_dropout_mask")
    return mask


def window_bounds(B: int, S: int, W: int, device, doc=None):
    """Bounds (lo, hi), int32 [B, S], of a sliding window of ``W`` keys, merged with the
    document bounds ``doc`` when given -- see ``reference.window_bounds``.  Torch plumbing
    over B*S ints, as :func:`doc_bounds` is."""
    from .reference import window_bounds as wb
    return wb(B, S, W, device, doc=doc)


_WINDOW_BOUNDS = {}  # (B, S, W, device) -> bounds without a document mask: built once


def _window_doc(window, doc, B: int, S: int, device, name: str):
    """(window, doc) of an attention wrapper with ``window=``: the window folded into the
    bounds the DOC kernels take.  A window that covers the sequence is no window."""
    window = _req_window(window, name)
    if window is None or window >= S:
        return None, doc
    from .reference import WindowBounds
    if isinstance(doc, WindowBounds) and doc.window == window:  # folded in by the caller
        return window, doc
    if doc is not None:
        _req_doc(doc, B, S, device, name)
        return window, window_bounds(B, S, window, device, doc=doc)
    k = (B, S, window, str(device))
    if k not in _WINDOW_BOUNDS:
        if len(_WINDOW_BOUNDS) >= 64:
            _WINDOW_BOUNDS.clear()
        _WINDOW_BOUNDS[k] = window_bounds(B, S, window, device)
    return window, _WINDOW_BOUNDS[k]


def doc_bounds(ids: torch.Tensor, sep: int):
    """Document bounds (lo, hi), int32 [B, S], of packed sequences -- see
    ``reference.doc_bounds``.  Torch ops on ``ids``' device: plumbing over B*S ints on the
    current stream, not a kernel of the hot path."""
    from .reference import doc_bounds as db
    return db(ids, sep)


def _req_doc(doc, B: int, S: int, device, name: str):
    """(lo, hi) of :func:`doc_bounds` for a [B, S] batch on ``device``; (None, None) for None."""
    if doc is None:
        return None, None
    if not isinstance(doc, (tuple, list)) or len(doc) != 2:
        raise TypeError(f"{name}: doc must be None or (lo, hi)")
    for t, n in zip(doc, ("lo", "hi")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}.doc.{n}: expected a tensor")
        _req(t, torch.int32, f"{name}.doc.{n}", B * S)
        if tuple(t.shape) != (B, S):
            raise ValueError(f"{name}.doc.{n}: expected shape [{B}, {S}], got {list(t.shape)}")
        if t.device != device:
            raise ValueError(f"{name}.doc.{n}: expected device {device}, got {t.device}")
    return doc[0], doc[1]


def _head_major_nkv(q, k, v, nkv, name: str):
    """Number of K/V heads when the grouped-query kernels run a head-major call (``nkv``
    given, or k / v with fewer heads than q), else None: the MHA entry points."""
    nh = q.shape[1]
    if k.dim() != 4 or k.shape != v.shape:
        raise ValueError(f"{name}: k {list(k.shape)} and v {list(v.shape)} must have the same 4-d shape")
    if nkv is None and k.shape[1] == nh:
        return None
    nkv = _req_nkv(nh, k.shape[1] if nkv is None else nkv, name)
    if tuple(k.shape) != (q.shape[0], nkv, q.shape[2], q.shape[3]):
        raise ValueError(f"{name}: k / v must be [B, nkv, S, hd] = {[q.shape[0], nkv, q.shape[2], q.shape[3]]}, "
                         f"got {list(k.shape)}")
    return nkv


class _Stride(ctypes.Structure):
    """dlt_attn_stride: element strides (batch, head, row) of one tensor."""
    _fields_ = [("b", ctypes.c_long), ("h", c_int), ("r", c_int)]


class _AttnStrides(ctypes.Structure):
    _fields_ = [("q", _Stride), ("kv", _Stride), ("dq", _Stride), ("dkv", _Stride)]


class _AttnArgs(ctypes.Structure):
    """dlt_attn_args of csrc/attention.hip, field by field (lib() compares the sizes)."""
    _fields_ = ([(n, c_void_p) for n in ("q", "k", "v", "o", "lse", "mask", "dout", "delta_ws", "dq", "dk", "dv",
                                         "lo", "hi", "cosT", "sinT")]
                + [(n, c_int) for n in ("B", "nh", "nkv", "S", "hd", "hk")]
                + [("scale", c_float), ("dscale", c_float), ("key", c_uint32), ("thr", c_uint32),
                   ("gen_mask", c_int), ("softcap", c_float), ("stride", _AttnStrides), ("sink", c_void_p),
                   ("dsink", c_void_p)])


def _keep_bits_fwd(p, mask, B, nh, S, device, key=0, window=None):
    """(thr, dscale, mask, gen) of a forward: ``mask`` is the caller's keep bits (gen = 0), a new
    buffer for the launcher to fill (gen = 1), or None without dropout.  With ``window`` the new
    buffer gets the banded bits here (gen = 2: filled, but this call's own)."""
    thr = rng.keep_threshold(p)
    if not thr:
        return 0, 1.0, None, 1
    if mask is not None:
        _req(mask, torch.int32, "attn.mask", 2 * B * nh * S * ((S + 31) // 32))
        return thr, 1.0 / (1.0 - p), mask, 0
    if window is not None:
        return thr, 1.0 / (1.0 - p), attention_dropout_mask(B, nh, S, p, key, device=device, window=window), 2
    # [0] row layout (lane = query), [1] transposed (lane = key) -- see attention.hip;
    # with store_mask=False it only lives for this call (the backward regenerates it)
    mask = torch.empty(2, B * nh, (S + 31) // 32, S, dtype=torch.int32, device=device)
    return thr, 1.0 / (1.0 - p), mask, 1


def _keep_bits_bwd(p, key, mask, B, nh, S, device, window=None):
    """(thr, dscale, mask) of a backward; ``mask``: the forward's keep bits or None."""
    thr = rng.keep_threshold(p)
    if not thr:
        return 0, 1.0, None
    if mask is None:  # forward ran with store_mask=False: regenerate the keep bits only
        mask = attention_dropout_mask(B, nh, S, p, key, device=device, window=window)
    return thr, 1.0 / (1.0 - p), mask


def _head_major(q, k, v):
    """((q, k, v) pointers, q strides, k / v strides) of q [B, nh, S, hd] and k, v [B, nkv, S, hd];
    strides are (batch, head, row) in elements."""
    S, hd = q.shape[2], q.shape[3]
    return (_p(q), _p(k), _p(v)), (q.shape[1] * S * hd, S * hd, hd), (k.shape[1] * S * hd, S * hd, hd)


def _packed_row(qkv, S, H, hd, KV):
    """The same for q | k | v inside the packed [B*S, H + 2*KV] rows."""
    Wd = H + 2 * KV
    return (_p(qkv), _off(qkv, H), _off(qkv, H + KV)), (S * Wd, hd, Wd), (S * Wd, hd, Wd)


def _attn_name(name, nkv, doc):
    return name + ("_gqa" if nkv is not None else "" if doc is None else "_doc")


def _attn_sink(sink, nh: int, device, name: str, grad: bool = False):
    """``sink=`` / ``dsink=`` of the attention wrappers (None passes): the attention-sink
    logits, one per query head, as the kernels read them -- fp32 [nh], contiguous, on the
    activations' device.  A 16-bit ``sink`` (a gathered FSDP unit) is upcast, nh elements;
    ``dsink`` is the fp32 accumulator itself (``grad``) and is never copied."""
    if sink is None:
        return None
    if not isinstance(sink, torch.Tensor) or not sink.is_cuda or not sink.is_floating_point() \
            or tuple(sink.shape) != (nh,):
        raise ValueError(f"{name}: expected a floating-point GPU tensor of shape [{nh}] (one logit per query head)")
    if sink.device != device:
        raise ValueError(f"{name}: expected device {device}, got {sink.device}")
    if grad:
        if sink.dtype != torch.float32 or not sink.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous fp32 tensor")
        return sink
    if sink.dtype != torch.float32:
        sink = sink.float()
    if not sink.is_contiguous():
        sink = sink.contiguous()
    return sink


def _score_cap(softcap, name: str) -> float:
    """An attention-score cap (``softcap=`` not None): finite and > 0, also as the kernels' fp32."""
    cap = _cap32(softcap, name)
    if cap == 0.0:
        raise ValueError(f"{name}: the cap must be finite and > 0 (None turns it off), got {softcap!r}")
    return cap


def _attn_cap(softcap, name: str) -> dict:
    """``softcap=`` of the attention wrappers as the ``softcap`` field of the argument struct:
    nothing for None (the struct is the one built without the keyword: the plain kernels), else
    the cap, finite and > 0 also as the fp32 the CAP kernels receive."""
    if softcap is None:
        return {}
    from . import attn_routes
    cap = _score_cap(softcap, name + ".softcap")
    attn_routes.check_score_softcap_range(cap, name + ".softcap")
    return {"softcap": cap}


def _f32(name: str, hd: int, doc=None, window=None, sink=None, nkv=None, scale=None, softcap=None):
    """``hip_f32``, for an fp32 call to hand over to: the fp32 routes have no document mask, window,
    sinks, grouped K/V or score cap, and their score scale is 1/sqrt(head_dim)."""
    from . import attn_routes, hip_f32
    rt = attn_routes.route(torch.float32, hd)
    if softcap is not None:
        attn_routes.require_score_softcap(rt, name)
    for feature, arg in (("sinks", sink), ("gqa", nkv), ("window", window), ("doc", doc)):
        if arg is not None:
            attn_routes.require(rt, feature, name)
    if scale is not None:
        raise NotImplementedError("fp32 attention: the score scale is 1/sqrt(head_dim)")
    return hip_f32


def _attn_fwd_launch(name, src, o, lse, keep, key, lo, B, nh, nkv, S, hd, hk, scale, sink=None, softcap=None):
    """dlt_attn_fwd on q / k / v of layout ``src`` (:func:`_head_major`, :func:`_packed_row`)
    with ``keep`` of :func:`_keep_bits_fwd`; nkv None: the MHA kernels; ``sink``: the SINK forms;
    ``softcap``: the CAP forms (attention_cap.hip)."""
    (q, k, v), sq, skv = src
    thr, dscale, mask, gen = keep
    a = _AttnArgs(q=q, k=k, v=v, o=_p(o), lse=_p(lse), mask=_p(mask), lo=_p(lo), B=B, nh=nh, nkv=nkv or 0, S=S,
                  hd=hd, hk=hk, scale=scale, dscale=dscale, key=key & 0xFFFFFFFF, thr=thr, gen_mask=int(gen == 1),
                  stride=_AttnStrides(q=sq, kv=skv), sink=_p(sink), **_attn_cap(softcap, name))
    _chk(lib().dlt_attn_fwd(ctypes.byref(a), _stream()), _attn_name(name, nkv, lo))


def _attn_bwd_launch(name, src, dst, o, do, lse, keep, doc, rope, B, nh, nkv, S, hd, hk, scale, sink=None,
                     dsink=None, softcap=None):
    """dlt_attn_bwd: dq / dk / dv into layout ``dst``; ``keep`` of :func:`_keep_bits_bwd`,
    ``doc`` = (lo, hi), ``rope`` = (cos, sin) or (None, None).  With ``sink`` / ``dsink`` the
    launch ends with k_attn_sink_bwd, which reads lse and the delta workspace dQ wrote."""
    (q, k, v), sq, skv = src
    (dq, dk, dv), sdq, sdkv = dst
    thr, dscale, mask = keep
    if (sink is None) != (dsink is None):
        raise ValueError(f"{name}: sink and dsink go together")
    cap = _attn_cap(softcap, name)
    delta = torch.empty(B, nh, S, dtype=torch.float32, device=lse.device)
    a = _AttnArgs(q=q, k=k, v=v, o=_p(o), lse=_p(lse), mask=_p(mask), dout=_p(do), delta_ws=_p(delta), dq=dq, dk=dk,
                  dv=dv, lo=_p(doc[0]), hi=_p(doc[1]), cosT=_p(rope[0]), sinT=_p(rope[1]), B=B, nh=nh, nkv=nkv or 0,
                  S=S, hd=hd, hk=hk, scale=scale, dscale=dscale, thr=thr,
                  stride=_AttnStrides(q=sq, kv=skv, dq=sdq, dkv=sdkv), sink=_p(sink), dsink=_p(dsink), **cap)
    _chk(lib().dlt_attn_bwd(ctypes.byref(a), _stream()), _attn_name(name, nkv, doc[0]))


def attention_fwd(q, k, v, p, key, causal=True, store_mask=True, out=None, mask=None, scale=None, doc=None,
                  nkv=None, window=None, sink=None, softcap=None):
    """Returns (o [B*S, nh*hd] bf16, aux).  With dropout on, the keep bits are written
    to a bitmask consumed by attention_bwd (no re-hashing in the backward); pass
    ``mask`` from ``attention_dropout_mask`` to skip generating it here.  ``scale``:
    the score scale (default 1/sqrt(hd); ops/attn_gemm.py runs zero-padded heads with
    the unpadded head_dim's).  ``doc`` = (lo, hi) from :func:`doc_bounds`: the
    intra-document mask of packed sequences (DOC kernels of attention.hip).  Grouped-query
    attention: k, v [B, nkv, S, hd] with nkv dividing nh (or ``nkv=`` given: the GQA kernels
    also for nkv == nh).  ``window`` = W: sliding-window attention, query q sees the keys
    q - W < k <= q (of its document); it runs on the DOC kernels with the bounds of
    :func:`window_bounds`, and keep bits made here are the banded ones.  ``sink`` (fp32 [nh]):
    attention sinks, one more logit per query head in the softmax denominator (not scaled, no
    value row; the SINK kernels); the returned lse holds it.  ``softcap`` = CAP (finite, > 0):
    attention-score soft-capping, scores CAP * tanh(scale q.k / CAP) before the masks and the
    softmax (the CAP kernels); masked keys stay at -inf, a sink is not capped, and lse is that of
    the capped scores; at most ``attn_routes.SCORE_SOFTCAP_MAX``.  None: the call, its argument
    struct and its kernels are what they were."""
    nkv = _head_major_nkv(q, k, v, nkv, "attn")
    if q.dtype == torch.float32:
        return _f32("attention_fwd", q.shape[3], doc, window, sink, nkv, scale, softcap).attention_fwd(
            q, k, v, p, key, causal, store_mask=store_mask, out=out, mask=mask)
    if not causal:
        raise NotImplementedError("only causal attention is implemented (the model is a causal LM)")
    B, nh, S, hd = q.shape
    for t, n, hh in ((q, "q", nh), (k, "k", nkv or nh), (v, "v", nkv or nh)):
        hk = _req_act(t, q.dtype, "attn." + n, B * hh * S * hd)
    window, doc = _window_doc(window, doc, B, S, q.device, "attn")
    lo, _ = _req_doc(doc, B, S, q.device, "attn")
    if hd not in ATTN_HEAD_DIMS:
        raise NotImplementedError(f"attention kernels take head_dim {ATTN_HEAD_DIMS} (got {hd})")
    o = torch.empty(B * S, nh * hd, dtype=q.dtype, device=q.device) if out is None else out
    _req(o, q.dtype, "attn.o", B * S * nh * hd)
    lse = torch.empty(B, nh, S, dtype=torch.float32, device=q.device)
    keep = _keep_bits_fwd(p, mask, B, nh, S, q.device, key, window)
    sc = 1.0 / math.sqrt(hd) if scale is None else float(scale)
    sink = _attn_sink(sink, nh, q.device, "attn.sink")
    _attn_fwd_launch("attn_fwd", _head_major(q, k, v), o, lse, keep, key, lo, B, nh, nkv, S, hd, hk, sc, sink,
                     softcap)
    return o, AttnAux((lse, keep[2] if (store_mask or not keep[3]) else None))


def _packed_dims(qkv, B, S, nh, nkv=None):
    """(M, H, hd, KV) of the packed QKV with rows [H + 2*KV]; KV = H without ``nkv``."""
    M, Wd = qkv.shape
    nk = nh if nkv is None else _req_nkv(nh, nkv, "packed attention")
    hd = Wd // (nh + 2 * nk)
    if M != B * S or hd * (nh + 2 * nk) != Wd:
        raise ValueError("packed attention: qkv must be [B*S, 3*nh*hd]" if nkv is None else
                         "packed attention: qkv must be [B*S, (nh + 2*nkv)*hd]")
    if hd not in ATTN_HEAD_DIMS:
        raise NotImplementedError(f"attention kernels take head_dim {ATTN_HEAD_DIMS} (got {hd})")
    _req_act(qkv, qkv.dtype, "attn.qkv")
    return M, nh * hd, hd, nk * hd


def attention_fwd_packed(qkv, B, S, nh, p, key, out=None, mask=None, store_mask=True, doc=None, nkv=None,
                         window=None, sink=None, softcap=None):
    """Causal attention reading q/k/v straight from the packed (roped) [B*S, 3H] QKV.
    Returns (o [B*S, H] bf16, aux) like :func:`attention_fwd`.  With ``nkv`` (grouped-query
    attention) the packed row is [H + 2*KV]; lse and the keep bits stay per query head.
    ``window``, ``sink``, ``softcap``: see :func:`attention_fwd`."""
    if qkv.dtype == torch.float32:
        return _f32("attention_fwd_packed", qkv.shape[1] // (3 * nh), doc, window, sink, nkv,
                    softcap=softcap).attention_fwd_packed(
            qkv, B, S, nh, p, key, out=out, mask=mask, store_mask=store_mask)
    M, H, hd, KV = _packed_dims(qkv, B, S, nh, nkv)
    window, doc = _window_doc(window, doc, B, S, qkv.device, "attn")
    lo, _ = _req_doc(doc, B, S, qkv.device, "attn")
    o = torch.empty(M, H, dtype=qkv.dtype, device=qkv.device) if out is None else out
    _req(o, qkv.dtype, "attn.o", M * H)
    lse = torch.empty(B, nh, S, dtype=torch.float32, device=qkv.device)
    keep = _keep_bits_fwd(p, mask, B, nh, S, qkv.device, key, window)
    sink = _attn_sink(sink, nh, qkv.device, "attn.sink")
    _attn_fwd_launch("attn_fwd_packed", _packed_row(qkv, S, H, hd, KV), o, lse, keep, key, lo, B, nh, nkv, S, hd,
                     _HK[qkv.dtype], 1.0 / math.sqrt(hd), sink, softcap)
    return o, AttnAux((lse, keep[2] if (store_mask or not keep[3]) else None))


def attention_bwd_packed(qkv, o, do, aux, p, key, B, S, nh, cos, sin, out=None, doc=None, nkv=None, window=None,
                         sink=None, dsink=None, softcap=None):
    """Backward of :func:`attention_fwd_packed` + the in-place RoPE: returns dqkv
    [B*S, 3H] (gradient w.r.t. the pre-rotation QKV GEMM output); dq/dk/dv are written
    into it by the attention kernels with the inverse rotation in their epilogue.  With
    ``nkv`` qkv and dqkv are [B*S, H + 2*KV]; dk / dv are summed over each group's query
    heads in registers, in a fixed order.  ``window``: the forward's.  ``sink`` / ``dsink`` (fp32
    [nh], both or neither): the forward's sinks and their gradient accumulator,
    ``dsink[h] += -sum_{b,q} exp(sink[h] - lse) * rowsum(dO * O)`` in a fixed order (no atomics);
    dq / dk / dv need only the forward's lse.  ``softcap``: the forward's; dQ and dK/dV rebuild
    t = tanh(scale q.k / CAP) and carry 1 - t^2 into dS (the CAP kernels)."""
    if qkv.dtype == torch.float32:
        return _f32("attention_bwd_packed", qkv.shape[1] // (3 * nh), doc, window, sink, nkv,
                    softcap=softcap).attention_bwd_packed(
            qkv, o, do, aux, p, key, B, S, nh, cos, sin, out=out)
    M, H, hd, KV = _packed_dims(qkv, B, S, nh, nkv)
    Wd = H + 2 * KV
    window, doc = _window_doc(window, doc, B, S, qkv.device, "attn_bwd")
    lo, hi = _req_doc(doc, B, S, qkv.device, "attn_bwd")
    for t, nm in ((o, "o"), (do, "do")):
        _req(t, qkv.dtype, "attn_bwd." + nm, M * H)
    lse, mask = aux if isinstance(aux, tuple) else (aux, None)
    _req(lse, torch.float32, "attn_bwd.lse", B * nh * S)
    if cos.shape[0] < S or cos.shape[1] != hd // 2 or sin.shape != cos.shape:
        raise ValueError("rope tables too short")
    _req(cos, torch.float32, "attn_bwd.cos")
    _req(sin, torch.float32, "attn_bwd.sin")
    keep = _keep_bits_bwd(p, key, mask, B, nh, S, qkv.device, window)
    dqkv = torch.empty(M, Wd, dtype=qkv.dtype, device=qkv.device) if out is None else out
    _req(dqkv, qkv.dtype, "attn_bwd.dqkv", M * Wd)
    sink = _attn_sink(sink, nh, qkv.device, "attn_bwd.sink")
    dsink = _attn_sink(dsink, nh, qkv.device, "attn_bwd.dsink", grad=True)
    _attn_bwd_launch("attn_bwd_packed", _packed_row(qkv, S, H, hd, KV), _packed_row(dqkv, S, H, hd, KV), o, do, lse,
                     keep, (lo, hi), (cos, sin), B, nh, nkv, S, hd, _HK[qkv.dtype], 1.0 / math.sqrt(hd), sink, dsink,
                     softcap)
    return dqkv


def attention_bwd(q, k, v, o, do, aux, p, key, causal=True, scale=None, doc=None, nkv=None, window=None,
                  sink=None, dsink=None, softcap=None):
    """Returns dq [B, nh, S, hd] and dk, dv in k's shape ([B, nkv, S, hd] under grouped-query
    attention, see :func:`attention_fwd`).  ``sink`` / ``dsink``, ``softcap``: see :func:`attention_bwd_packed`."""
    nkv = _head_major_nkv(q, k, v, nkv, "attn_bwd")
    if q.dtype == torch.float32:
        return _f32("attention_bwd", q.shape[3], doc, window, sink, nkv, scale, softcap).attention_bwd(
            q, k, v, o, do, aux, p, key, causal)
    B, nh, S, hd = q.shape
    n = B * nh * S * hd
    nk = B * (nkv or nh) * S * hd
    for t, nm, cnt in ((q, "q", n), (k, "k", nk), (v, "v", nk), (o, "o", n), (do, "do", n)):
        hk = _req_act(t, q.dtype, "attn_bwd." + nm, cnt)
    window, doc = _window_doc(window, doc, B, S, q.device, "attn_bwd")
    lo, hi = _req_doc(doc, B, S, q.device, "attn_bwd")
    lse, mask = aux if isinstance(aux, tuple) else (aux, None)
    _req(lse, torch.float32, "attn_bwd.lse", B * nh * S)
    keep = _keep_bits_bwd(p, key, mask, B, nh, S, q.device, window)
    dq = torch.empty_like(q)
    dk = torch.empty_like(k)
    dv = torch.empty_like(v)
    sc = 1.0 / math.sqrt(hd) if scale is None else float(scale)
    sink = _attn_sink(sink, nh, q.device, "attn_bwd.sink")
    dsink = _attn_sink(dsink, nh, q.device, "attn_bwd.dsink", grad=True)
    _attn_bwd_launch("attn_bwd", _head_major(q, k, v), _head_major(dq, dk, dv), o, do, lse, keep, (lo, hi),
                     (None, None), B, nh, nkv, S, hd, hk, sc, sink, dsink, softcap)
    return dq, dk, dv


# ----------------------------------------------------------------- SwiGLU
def swiglu_fwd(gu, out=None):
    if gu.dtype == torch.float32:
        from . import hip_f32
        return hip_f32.swiglu_fwd(gu, out=out)
    M, twoI = gu.shape
    hk = _req_act(gu, gu.dtype, "swiglu.gu")
    if out is None:
        out = torch.empty(M, twoI // 2, dtype=gu.dtype, device=gu.device)
    _req(out, gu.dtype, "swiglu.out", M * twoI // 2)
    _chk(lib().dlt_swiglu_fwd(_p(gu), _p(out), M, twoI // 2, hk, _stream()), "swiglu_fwd")
    return out


def swiglu_bwd(gu, da, out=None, s_out=None):
    """dgu = SwiGLU backward; ``s_out``: also writes s = silu(g) * u (the forward's bits)."""
    if gu.dtype == torch.float32:
        from . import hip_f32
        return hip_f32.swiglu_bwd(gu, da, out=out, s_out=s_out)
    M, twoI = gu.shape
    hk = _req_act(gu, gu.dtype, "swiglu_bwd.gu")
    _req(da, gu.dtype, "swiglu_bwd.da", M * twoI // 2)
    if out is None:
        out = torch.empty_like(gu)
    _req(out, gu.dtype, "swiglu_bwd.out", M * twoI)
    if s_out is not None:
        _req(s_out, gu.dtype, "swiglu_bwd.s_out", M * twoI // 2)
    _chk(lib().dlt_swiglu_bwd(_p(gu), _p(da), _p(out), _p(s_out) if s_out is not None else None, M, twoI // 2, hk,
                              _stream()), "swiglu_bwd")
    return out


# ------------------------------------------------------------ cross-entropy
def _cap32(softcap, name: str = "ce.softcap") -> float:
    """check_softcap, and the cap must still be finite and > 0 as the fp32 the kernels receive."""
    cap = check_softcap(softcap, name)
    if cap != 0.0 and not 0.0 < ctypes.c_float(cap).value < math.inf:
        raise ValueError(f"{name}: the cap must be finite and > 0 in fp32, got {softcap!r}")
    return cap


def check_z_rows(z_rows, logits, name: str = "ce.z_rows") -> None:
    """``z_rows`` of the z-loss form: fp32 [M], contiguous, on the logits' device."""
    if not isinstance(z_rows, torch.Tensor):
        raise TypeError(f"{name}: the z-loss form needs an fp32 [M] tensor for the rows' lse^2")
    if z_rows.device != logits.device:
        raise ValueError(f"{name}: expected a tensor on {logits.device}, got {z_rows.device}")
    if z_rows.dtype != torch.float32:
        raise TypeError(f"{name}: expected torch.float32, got {z_rows.dtype}")
    if tuple(z_rows.shape) != (logits.shape[0],) or not z_rows.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous [{logits.shape[0]}] tensor, got {tuple(z_rows.shape)}")


def cross_entropy_fwd_bwd(logits, targets, vocab, n_valid, grad_scale: float = 1.0, z_loss: float = 0.0,
                          z_rows=None, softcap: float = 0.0):
    """Per-row loss; the logits buffer (bf16 or fp16) is overwritten by
    grad_scale * (softmax - onehot) / n_valid (fp16: grad_scale = the loss scale, so the
    gradient does not underflow).

    The z-loss form (``z_loss`` != 0 or ``z_rows`` given; ``z_rows`` fp32 [M] is then required):
    the gradient is that of ``(lse - logit[target]) + z_loss * lse^2``, i.e.
    grad_scale * (softmax * (1 + 2 z_loss lse) - onehot) / n_valid; the returned rows stay the
    cross-entropy part and ``z_rows`` receives lse^2 (0 on ignored rows).  Without either
    argument the plain kernels run, as before the form existed.

    The CAP form (``softcap`` != 0, finite and > 0; 16-bit logits only): the softmax, the rows and
    ``z_rows`` are those of ``c = softcap * tanh(logits / softcap)``, and every element of the
    gradient carries ``1 - tanh^2(logits / softcap)``.  With ``softcap`` 0 the call is what it was."""
    cap = _cap32(softcap)
    if logits.dtype == torch.float32:
        if cap != 0.0:
            raise NotImplementedError("ce.softcap: fp32 logits have no CAP kernel on the GPU (logit_softcap)")
        from . import hip_f32
        return hip_f32.cross_entropy_fwd_bwd(logits, targets, vocab, n_valid, grad_scale, z_loss, z_rows)
    M, Vp = logits.shape
    hk = _req_act(logits, logits.dtype, "ce.logits")
    targets = targets.contiguous()
    if targets.dtype != torch.int64 or targets.numel() != M:
        raise ValueError("ce.targets must be int64 [M]")
    nv = n_valid.reshape(1).to(torch.int64).contiguous()
    loss = torch.empty(M, dtype=torch.float32, device=logits.device)
    if cap != 0.0:
        if float(z_loss) != 0.0 or z_rows is not None:
            check_z_rows(z_rows, logits)
        if Vp % 8 or vocab > Vp:
            raise ValueError(f"ce.logits: the padded width {Vp} must be a multiple of 8 and hold the vocabulary {vocab}")
        _chk(lib().dlt_cross_entropy_cap_fwd_bwd(_p(logits), _p(targets), _p(nv), _p(loss), M, Vp, vocab,
                                                 float(grad_scale), hk, float(z_loss), _p(z_rows), cap, _stream()),
             "cross_entropy_cap")
        return loss
    if float(z_loss) == 0.0 and z_rows is None:
        _chk(lib().dlt_cross_entropy_fwd_bwd(_p(logits), _p(targets), _p(nv), _p(loss), M, Vp, vocab,
                                             float(grad_scale), hk, _stream()), "cross_entropy")
        return loss
    check_z_rows(z_rows, logits)
    if Vp % 8 or vocab > Vp:
        raise ValueError(f"ce.logits: the padded width {Vp} must be a multiple of 8 and hold the vocabulary {vocab}")
    _chk(lib().dlt_cross_entropy_z_fwd_bwd(_p(logits), _p(targets), _p(nv), _p(loss), M, Vp, vocab,
                                           float(grad_scale), hk, float(z_loss), _p(z_rows), _stream()),
         "cross_entropy_z")
    return loss


# --------------------------------------------------------------- optimizer
_SUMSQ_PARTS = {}  # device -> 1024-float workspace of the two-stage (deterministic) reduction


def sumsq(x: torch.Tensor, out: torch.Tensor) -> None:
    """out[0] += sum(x**2), bitwise reproducible (fixed-order partials, no atomics)."""
    _req(x, torch.float32, "sumsq.x")
    _req(out, torch.float32, "sumsq.out")
    part = _SUMSQ_PARTS.get(x.device)
    if part is None:
        part = _SUMSQ_PARTS[x.device] = torch.empty(1024, dtype=torch.float32, device=x.device)
    _chk(lib().dlt_sumsq(_p(x), x.numel(), _p(part), _p(out), _stream()), "sumsq")


def clip_coef(sumsq_t: torch.Tensor, out: torch.Tensor, norm_mul: float, max_norm: float, scale_mul: float) -> None:
    _chk(lib().dlt_clip_coef(_p(sumsq_t), _p(out), norm_mul, max_norm, scale_mul, _stream()), "clip_coef")


def adamw_flat(param, grad, exp_avg, exp_avg_sq, shadow, lr, beta1, beta2, eps, wd, step, gscale,
               zero_grad: bool = False):
    """One fused AdamW pass over flat fp32 buffers (+ the 16-bit shadow); ``zero_grad``:
    the gradient is zeroed in the same pass."""
    n = param.numel()
    for t, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _req(t, torch.float32, "adamw." + nm, n)
    if shadow is not None and (shadow.dtype not in (torch.bfloat16, torch.float16) or shadow.numel() != n):
        raise ValueError("adamw.shadow must be bf16 or fp16 of the same numel")
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    f16 = shadow is not None and shadow.dtype == torch.float16
    if zero_grad:
        _chk(lib().dlt_adamw_ex(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(shadow), n, lr, beta1, beta2,
                                eps, wd, lr / bc1, 1.0 / math.sqrt(bc2), _p(gscale), (1 if f16 else 0) | 2,
                                _stream()), "adamw")
        return
    fn = lib().dlt_adamw_f16 if f16 else lib().dlt_adamw
    _chk(fn(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(shadow), n, lr, beta1, beta2, eps, wd,
            lr / bc1, 1.0 / math.sqrt(bc2), _p(gscale), _stream()), "adamw")


def add_bf16_into_f32(dst: torch.Tensor, src: torch.Tensor) -> bool:
    """dst (fp32) += src (bf16 or fp16) in one kernel; False (nothing launched) if the
    shapes or alignment do not fit the 8-wide vector path."""
    n = dst.numel()
    if (src.numel() != n or n % 8 or not dst.is_contiguous() or not src.is_contiguous()
            or dst.dtype != torch.float32 or src.dtype not in _HK or dst.data_ptr() % 16 or src.data_ptr() % 16):
        return False
    _chk(lib().dlt_add_bf16_f32(_p(dst), _p(src), n, _HK[src.dtype], _stream()), "add_bf16_f32")
    return True


def cast_bf16(x: torch.Tensor, y: torch.Tensor) -> None:
    _chk(lib().dlt_cast_bf16(_p(x), _p(y), x.numel(), _HK[y.dtype], _stream()), "cast_bf16")


# ---------------------------------------------------------------- wgrad GEMM
# the 256 x 128 tile forms of the hand GEMMs (hidden sizes 192 does not divide, e.g. the
# medium model's 1024); DLT_GEMM_BN128=0 leaves such shapes to hipBLASLt
_BN128 = os.environ.get("DLT_GEMM_BN128", "1") != "0"


def wgrad_bn(Nc: int) -> int:
    """dW column tile of the weight-gradient kernel: 192, else 128 (e.g. hidden 1024), else 0."""
    return 192 if Nc % 192 == 0 else (128 if _BN128 and Nc % 128 == 0 else 0)


def wgrad_fits(T: int, Nr: int, Nc: int) -> bool:
    """Shapes the 256 x 192 (or 256 x 128) weight-gradient kernel tiles (T in 128-token
    pairs; a last half row tile when Nr % 256 == 128)."""
    return T > 0 and T % 128 == 0 and Nr % 128 == 0 and wgrad_bn(Nc) > 0


def wgrad_splits(T: int, Nr: int, Nc: int, target: int = 256) -> int:
    """Split-K factor that brings tiles x splits closest to `target` workgroups (one per
    CU), capped by the number of 128-token pairs."""
    tiles = ((Nr + 255) // 256) * (Nc // wgrad_bn(Nc))
    return max(1, min(T // 128, (target + tiles // 2) // tiles))


def gemm_wgrad(dw: Optional[torch.Tensor], dy: torch.Tensor, x: torch.Tensor, splits: int = 0,
               part: Optional[torch.Tensor] = None) -> bool:
    """dw[Nr,Nc] (fp32) += dy[T,Nr]^T @ x[T,Nc] with the hand-written MFMA kernel
    (csrc/gemm_wgrad.hip).  splits == 0 picks the CU-filling split; with splits > 1 the
    fp32 partials go to `part` ([splits, Nr, Nc], allocated if None) and are summed into
    dw in fixed split order (deterministic).  dw = None with splits > 1: only the
    partials are written (the caller reduces them, e.g. straight into bf16).  dy / x:
    both bf16 or both fp16.  Returns False (nothing launched) when the shape does not tile."""
    T, Nr = dy.shape
    Nc = x.shape[1]
    if not wgrad_fits(T, Nr, Nc) or dy.stride(1) != 1 or x.stride(1) != 1 or dy.stride(0) % 8 or x.stride(0) % 8:
        return False
    if dw is None:
        if splits <= 1 or part is None or part.dtype != torch.float32 or part.numel() < splits * Nr * Nc \
                or not part.is_contiguous():
            raise ValueError("gemm_wgrad: partials-only mode needs splits > 1 and an fp32 part buffer")
    else:
        _req(dw, torch.float32, "wgrad.dw", Nr * Nc)
    if dy.dtype not in _WG_HK or x.dtype != dy.dtype or x.shape[0] != T:
        raise ValueError("gemm_wgrad: bf16 / fp16 dy[T,Nr] / x[T,Nc] of one dtype expected")
    if splits <= 0:
        splits = wgrad_splits(T, Nr, Nc)
    splits = min(splits, T // 128)
    if splits > 1 and (part is None or part.numel() < splits * Nr * Nc):
        part = torch.empty(splits * Nr * Nc, device=dw.device, dtype=torch.float32)
    _chk(lib().dlt_gemm_wgrad(_p(dy), _p(x), _p(dw) if dw is not None else None, _p(part) if splits > 1 else None,
                              T, Nr, Nc, dy.stride(0), x.stride(0), splits, _WG_HK[dy.dtype], _stream()),
         "gemm_wgrad")
    if splits > 1 and dw is not None:
        _chk(lib().dlt_splitk_acc(_p(part), _p(dw), Nr * Nc, splits, _stream()), "splitk_acc")
    return True


# operand format of the weight-gradient kernels (HK template parameter)
_WG_HK = {torch.bfloat16: 0, torch.float16: 1}

# DLT_WGRAD_SK_SHARES=n: n shares per column tile instead of 256 / column tiles (A/B knob)
_SK_SHARES = int(os.environ.get("DLT_WGRAD_SK_SHARES", "0"))


def gemm_wgrad_sk(dw: torch.Tensor, dy: torch.Tensor, x: torch.Tensor, shares: int = 0) -> bool:
    """dw[Nr,Nc] (fp32) += dy[T,Nr]^T @ x[T,Nc], stream-K form of the hand-written kernel
    (csrc/gemm_wgrad.hip k_gemm_wgrad_sk): one resident workgroup per CU walks an equal
    share of (row tile, token pair) work of one column tile; tiles split between shares
    are summed into dw in fixed share order (bitwise reproducible).  Pays off when a
    share is a sizable part of a tile (gate/up 6144 x 768 and lm_head 50304 x 768 at
    T = 32768: 275 / 2273 us vs 312 / 2422 for the best split-K, profiles/r3_wgrad.md).
    Returns False when the shape does not tile."""
    T, Nr = dy.shape
    Nc = x.shape[1]
    if not wgrad_fits(T, Nr, Nc) or dy.stride(1) != 1 or x.stride(1) != 1 or dy.stride(0) % 8 or x.stride(0) % 8:
        return False
    _req(dw, torch.float32, "wgrad_sk.dw", Nr * Nc)
    if dy.dtype not in _WG_HK or x.dtype != dy.dtype or x.shape[0] != T:
        raise ValueError("gemm_wgrad_sk: bf16 / fp16 dy[T,Nr] / x[T,Nc] of one dtype expected")
    shares = shares or _SK_SHARES
    n = int(lib().dlt_gemm_wgrad_sk_scratch(T, Nr, Nc, shares))
    part = torch.empty(n, device=dw.device, dtype=torch.float32)
    _chk(lib().dlt_gemm_wgrad_sk(_p(dy), _p(x), _p(dw), _p(part), T, Nr, Nc, dy.stride(0), x.stride(0), shares,
                                 _WG_HK[dy.dtype], _stream()), "gemm_wgrad_sk")
    return True


# ---------------------------------------------------------------- grouped wgrad GEMM
WGRAD_GROUP_MAX = 8  # problems per launch (GW_GRP_MAX of csrc/gemm_wgrad.hip)


def wgrad_group_shares(T: int, shapes, grid: int = 256):
    """Shares per column tile of every problem of a grouped weight gradient
    (``shapes``: (Nr, Nc) per problem, one column tile for all), so that ``grid``
    workgroups each get about the same number of (row tile, 128-token pair) iterations:
    problem p's workgroups are shares x column tiles, its work row tiles x column tiles x
    pairs, so equal shares mean shares proportional to row tiles.  Every problem gets at
    least one share (then sum(shares x column tiles) can exceed ``grid`` only when the
    column tiles alone do); workgroups left over by the rounding go, one share at a time,
    to the problem with the longest shares.  Pure arithmetic, no GPU."""
    bn = wgrad_bn(shapes[0][1])
    if T <= 0 or T % 128 or bn == 0 or any(wgrad_bn(nc) != bn or nr % 128 or nr <= 0 for nr, nc in shapes):
        raise ValueError("wgrad_group_shares: the group does not tile")
    npair = T // 128
    ntc = [nc // bn for _, nc in shapes]
    work = [((nr + 255) // 256) * npair for nr, _ in shapes]  # iterations of one column tile
    total = sum(w * c for w, c in zip(work, ntc))
    shares = [max(1, min(w, grid * w // total)) for w in work]

    def used():
        return sum(s * c for s, c in zip(shares, ntc))
    while used() > grid:  # only after the max(1, .) above: take from the shortest shares
        cand = [p for p in range(len(shapes)) if shares[p] > 1]
        if not cand:
            break
        shares[min(cand, key=lambda p: (work[p] / shares[p], p))] -= 1
    while True:
        cand = [p for p in range(len(shapes)) if shares[p] < work[p] and used() + ntc[p] <= grid]
        if not cand:
            break
        shares[max(cand, key=lambda p: (work[p] / shares[p], -p))] += 1
    return shares


# DLT_WGRAD_GROUP_SPREAD=1: deal the shares of a group to the least-loaded XCD instead of
# packing problem after problem (A/B knob)
_GRP_SPREAD = os.environ.get("DLT_WGRAD_GROUP_SPREAD", "0") == "1"


def wgrad_group_table(shapes, shares, spread=None):
    """Workgroup id -> (problem, column tile, share) of a grouped weight gradient, as a list
    with a multiple of 8 entries, ``None`` for padding.  The dispatcher deals ids round-robin
    to the 8 XCDs (id % 8).  The column tiles of one share read the same dY rows, so they
    go to one XCD, on consecutive ids of it.  Shares are placed widest first (most column
    tiles), problem after problem, each on the first XCD that stays within an equal part
    of all workgroups: the shares of one problem read the same X columns, so packing them
    onto few XCDs keeps X in few L2s, and every XCD gets the same number of working
    workgroups whenever the share widths allow it (small preset, 256 workgroups: two
    16-column down shares fill an XCD, the 52 four-column shares fill the other six).  A
    share that fits nowhere -- and every share with ``spread`` -- goes to the XCD with the
    fewest workgroups so far."""
    spread = _GRP_SPREAD if spread is None else spread
    bn = wgrad_bn(shapes[0][1])
    ntc = [nc // bn for _, nc in shapes]
    units = sorted(((p, g) for p in range(len(shapes)) for g in range(shares[p])), key=lambda u: -ntc[u[0]])
    cap = -(-sum(s * c for s, c in zip(shares, ntc)) // 8)
    lists = [[] for _ in range(8)]
    for p, g in units:
        fit = [] if spread else [i for i in range(8) if len(lists[i]) + ntc[p] <= cap]
        x = fit[0] if fit else min(range(8), key=lambda i: (len(lists[i]), i))
        lists[x].extend((p, c, g) for c in range(ntc[p]))
    depth = max(len(li) for li in lists)
    return [lists[i % 8][i // 8] if i // 8 < len(lists[i % 8]) else None for i in range(8 * depth)]


_GRP_CACHE = {}  # (device, stream, T, shapes, shares) -> table / scratch / static arguments


def _grp_state(dev, T, shapes, shares):
    """Device table, scratch and static argument arrays of a group signature, made once
    per (device, stream): launches on one stream are ordered, so they can share scratch."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, T, shapes, shares)
    st = _GRP_CACHE.get(key)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            return None  # a table cannot be uploaded inside a capture: warm the group up first
        n = len(shapes)
        ints = ctypes.c_int * n
        nr, nc, sh = ints(*(s[0] for s in shapes)), ints(*(s[1] for s in shapes)), ints(*shares)
        floats = int(lib().dlt_gemm_wgrad_grp_scratch(n, T, nr, nc, sh))
        if floats < 0:
            _GRP_CACHE[key] = st = False
            return st
        ents = wgrad_group_table(shapes, shares)
        table = torch.tensor([(-1, 0) if e is None else ((e[0] << 24) | e[1], e[2]) for e in ents],
                             dtype=torch.int32, device=dev)
        part = torch.empty(max(floats, 4), dtype=torch.float32, device=dev)
        _GRP_CACHE[key] = st = (table, len(ents), part, nr, nc, sh)
    return st


def gemm_wgrad_group(problems, shares=None, grid: int = 256) -> bool:
    """dw_p[Nr_p, Nc_p] (fp32) += dy_p[T, Nr_p]^T @ x_p[T, Nc_p] for every (dw, dy, x) of
    ``problems`` in one stream-K launch and one fix-up launch (csrc/gemm_wgrad.hip
    k_gemm_wgrad_grp): the weight gradients of a layer are each too small to fill the chip
    well, together they are a whole number of three-quarter-tile shares.  ``shares``: shares
    per column tile for every problem (default ``wgrad_group_shares(T, shapes, grid)``);
    problem p's result equals ``gemm_wgrad_sk(dw_p, dy_p, x_p, shares[p])`` bit for bit.
    Returns False with nothing launched and no dw touched when the group is refused:
    different T, dtypes or column tiles, a shape that does not tile, a dw that is not
    contiguous fp32, more than WGRAD_GROUP_MAX problems (or, inside a stream capture, a
    group signature not run before)."""
    n = len(problems)
    if n < 1 or n > WGRAD_GROUP_MAX:
        return False
    dw0, dy0, x0 = problems[0]
    T, bn = dy0.shape[0], wgrad_bn(x0.shape[1])
    if dy0.dtype not in _WG_HK or bn == 0:
        return False
    for dw, dy, x in problems:
        if (dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != T or x.shape[0] != T or dy.dtype != dy0.dtype
                or x.dtype != dy0.dtype or not wgrad_fits(T, dy.shape[1], x.shape[1]) or wgrad_bn(x.shape[1]) != bn
                or dy.stride(1) != 1 or x.stride(1) != 1 or dy.stride(0) % 8 or x.stride(0) % 8
                or dy.data_ptr() % 16 or x.data_ptr() % 16
                or not dw.is_cuda or dw.dtype != torch.float32 or not dw.is_contiguous()
                or dw.numel() != dy.shape[1] * x.shape[1] or dw.data_ptr() % 16 or dw.device != dy0.device
                or dy.device != dy0.device or x.device != dy0.device):
            return False
    shapes = tuple((dy.shape[1], x.shape[1]) for _, dy, x in problems)
    if shares is None:
        shares = wgrad_group_shares(T, shapes, grid)
    shares = tuple(int(s) for s in shares)
    npair = T // 128
    if len(shares) != n or any(s < 1 or s > ((nr + 255) // 256) * npair for s, (nr, _) in zip(shares, shapes)):
        return False
    st = _grp_state(dy0.device, T, shapes, shares)
    if not st:
        return False
    table, nblocks, part, nr, nc, sh = st
    ptrs, ints = ctypes.c_void_p * n, ctypes.c_int * n
    rc = lib().dlt_gemm_wgrad_grp(n, ptrs(*(p[1].data_ptr() for p in problems)),
                                  ptrs(*(p[2].data_ptr() for p in problems)),
                                  ptrs(*(p[0].data_ptr() for p in problems)), _p(part), _p(table), nblocks, T, nr, nc,
                                  ints(*(p[1].stride(0) for p in problems)), ints(*(p[2].stride(0) for p in problems)),
                                  sh, _WG_HK[dy0.dtype], _stream())
    if rc == -1:
        return False
    _chk(rc, "gemm_wgrad_group")
    return True


# ------------------------------------------------- projection GEMMs (csrc/gemm_bf16.hip)
# launch flags of the hand projection GEMMs; DLT_GEMM_FLAGS bit 256 = bounded persistence
# (each workgroup walks at most (flags >> 24) & 15 tiles, default 1, grid = tiles / that)
# instead of the persistent grid; DLT_GEMM_GRID=n caps the persistent grid at n
# (multiple of 8) workgroups (A/B knobs for overlapped schedules)
# Production flags (round 4): 1024 = LDS-transposed C stores (whole 192-byte row
# segments per store instruction: the plain epilogue's cycles -26 %), 12 = XCD row-band
# tile walk (an XCD keeps its A panels in its L2), 2048 = write-through (sc1) C stores
# (the C lines leave the XCD's L2 instead of evicting the operand panels: lm_head forward
# later K-iterations 6461 -> 4909 cycles); tools/cpp/gemm_stamps.cpp and
# profiles/r4_gemm_forward.md.  DLT_GEMM_FLAGS=n replaces them (bits 256 / 1024 / 2048 / 12).
_GB_DEFAULT_FLAGS = 2048 | 1024 | 12
_GB_FLAG_BITS = 256 | 1024 | 2048 | 4096 | 12 | (0xf << 24)  # (256 + bits 24-27: tiles per workgroup)
_GB_FLAGS = (int(os.environ.get("DLT_GEMM_FLAGS", str(_GB_DEFAULT_FLAGS))) & _GB_FLAG_BITS) | \
    ((min(int(os.environ.get("DLT_GEMM_GRID", "0")), 2040) // 8) << 16)
# launch flags of the FORWARD projection GEMMs only (plain / RoPE / SwiGLU epilogues),
# A/B knob for the two-chain window: DLT_GEMM_FWD_FLAGS=n replaces their flag bits (e.g.
# 256 | 3084: one tile per workgroup, grid = tiles) while the data gradients keep
# DLT_GEMM_FLAGS; the grid cap of gemm_grid_cap applies to both
_GB_FWD_OVERRIDE = os.environ.get("DLT_GEMM_FWD_FLAGS")


def _fwd_flags() -> int:
    if _GB_FWD_OVERRIDE is None:
        return _GB_FLAGS
    return (int(_GB_FWD_OVERRIDE) & _GB_FLAG_BITS) | (_GB_FLAGS & (0xff << 16))


def gemm_grid_cap(n: int) -> int:
    """Cap the persistent grid of the hand projection GEMMs at ``n`` workgroups (a
    multiple of 8; 0 = one per CU) for the launches that follow; returns the previous
    cap.  Each output tile is still computed whole by one workgroup, so results do not
    change.  The ``ffbb`` window sets 192: the other chain's kernels keep 64 CUs."""
    global _GB_FLAGS
    prev = 8 * ((_GB_FLAGS >> 16) & 0xff)
    _GB_FLAGS = (_GB_FLAGS & ~(0xff << 16)) | ((min(max(int(n), 0), 2040) // 8) << 16)
    return prev


def gemm_bf16_fits(M: int, N: int, K: int) -> bool:
    """Shapes the persistent MFMA kernel tiles exactly: 256 x 192 tiles, or 256 x 128 when
    192 does not divide N (plain store / data-gradient forms only)."""
    return M > 0 and M % 256 == 0 and (N % 192 == 0 or (_BN128 and N % 128 == 0)) and K % 128 == 0 and K >= 128


def gemm_bf16_fits192(M: int, N: int, K: int) -> bool:
    """Shapes the fused-epilogue forms (RoPE, SwiGLU, SwiGLU backward) tile: 256 x 192 only."""
    return gemm_bf16_fits(M, N, K) and N % 192 == 0


def gemm_bf16(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """C[M,N] = A[M,K] @ B[N,K]^T (bf16 or fp16 in/out, one format; fp32 accumulate) with
    the hand-written persistent MFMA kernel.  Returns None (nothing launched) when the
    shape does not tile (M % 256, N % 192, K % 128)."""
    M, K = a.shape
    N = b.shape[0]
    if not gemm_bf16_fits(M, N, K) or b.shape[1] != K:
        return None
    dt = a.dtype if a.dtype in _WG_HK else torch.bfloat16
    _req(a, dt, "gemm_bf16.a")
    _req(b, dt, "gemm_bf16.b")
    c = torch.empty(M, N, dtype=dt, device=a.device) if out is None else out
    _req(c, dt, "gemm_bf16.c", M * N)
    _chk(lib().dlt_gemm_bf16_tn(_p(a), _p(b), _p(c), M, N, K, K, K, N, _fwd_flags(), _WG_HK[dt], _stream()),
         "gemm_bf16")
    return c


def gemm_fw4_fits(M: int, N: int, K: int) -> bool:
    """Shapes the 4-wave 256 x 256 forward GEMM (csrc/gemm_fw4.hip) tiles."""
    return M > 0 and N > 0 and K > 0 and M % 256 == 0 and N % 128 == 0 and K % 64 == 0 and K >= 128


# launch flags of k_gemm_fw4 (csrc/gemm_fw4.hip): 1 = write-through (sc1) / 4 = nt C stores, 2 =
# row-major / 2048 = half-band tile order, 16 | 128 = SCHED 5, 4096 = two tiles per workgroup
_FW4_FLAGS = int(os.environ.get("DLT_GEMM_FW4_FLAGS", "148"))


def gemm_fw4(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None,
             flags: Optional[int] = None) -> Optional[torch.Tensor]:
    """C[M,N] = A[M,K] @ B[N,K]^T (bf16 or fp16 in/out, fp32 accumulate) with the 4-wave
    256 x 256 one-tile-per-workgroup MFMA kernel (128 x 128 per wave, AGPR accumulators).
    Returns None (nothing launched) when the shape does not tile (M % 256, N % 128, K % 64,
    K < 128)."""
    M, K = a.shape
    N = b.shape[0]
    if not gemm_fw4_fits(M, N, K) or b.shape[1] != K:
        return None
    hk = _req_act(a, a.dtype, "gemm_fw4.a")
    _req(b, a.dtype, "gemm_fw4.b")
    c = torch.empty(M, N, dtype=a.dtype, device=a.device) if out is None else out
    _req(c, a.dtype, "gemm_fw4.c", M * N)
    fl = _FW4_FLAGS if flags is None else flags
    rc = lib().dlt_gemm_fw4(_p(a), _p(b), _p(c), M, N, K, K, K, N, fl & ~1024, hk, None, 0, _stream())
    if rc == -1:
        return None  # a launch variant the shape does not take (two tiles per workgroup: tiles % 16)
    _chk(rc, "gemm_fw4")
    return c


def lmhead_loss_fits(M: int, Vp: int, K: int) -> bool:
    """Shapes the logits-free lm_head loss (k_gemm_fw4's loss epilogue) tiles."""
    return gemm_fw4_fits(M, Vp, K)


def lmhead_loss(nf: torch.Tensor, w: torch.Tensor, targets: torch.Tensor, V: int, flags: Optional[int] = None):
    """(row_loss [M], lse [M]) fp32 of the lm_head without its logits: with
    l = nf[M, K] @ w[Vp, K]^T rounded to the activation format (bf16 or fp16), lse[m] =
    logsumexp over the columns j < V and row_loss[m] = lse[m] - l[m, targets[m]], 0 where
    the target is ignore_index (-100).  k_gemm_fw4 reduces every 128-column half tile to a
    (max, sum exp) pair per row, k_lse_combine merges them in fixed order (bitwise
    reproducible).  Returns None (nothing launched) when the shape does not tile
    (M % 256, Vp % 128, K % 64, K < 128)."""
    M, K = nf.shape
    Vp = w.shape[0]
    if not lmhead_loss_fits(M, Vp, K) or w.shape[1] != K:
        return None
    if not 0 < V <= Vp:
        raise ValueError(f"lmhead_loss: vocab {V} outside (0, {Vp}]")
    hk = _req_act(nf, nf.dtype, "lmhead_loss.nf")
    _req(w, nf.dtype, "lmhead_loss.w")
    targets = targets.contiguous()
    if not targets.is_cuda or targets.dtype != torch.int64 or targets.numel() != M:
        raise ValueError("lmhead_loss.targets must be a GPU int64 [M]")
    n = int(lib().dlt_lmhead_loss_scratch(M, Vp))
    scratch = torch.empty(n, dtype=torch.float32, device=nf.device)
    out = torch.empty(3, M, dtype=torch.float32, device=nf.device)  # row_loss, lse, target logit
    fl = _FW4_FLAGS if flags is None else flags
    rc = lib().dlt_lmhead_loss(_p(nf), _p(w), _p(targets), _p(out[0]), _p(out[1]), _p(scratch), _p(out[2]), M, Vp,
                               int(V), K, K, K, fl, hk, _stream())
    if rc == -1:
        return None
    _chk(rc, "lmhead_loss")
    return out[0], out[1]


def gemm_fw4_swiglu_fits(M: int, I2: int, K: int) -> bool:
    return gemm_fw4_fits(M, I2, K) and I2 % 256 == 0


def gemm_fw4_swiglu(x: torch.Tensor, wgu: torch.Tensor, gu_out: Optional[torch.Tensor] = None,
                    s_out: Optional[torch.Tensor] = None, flags: Optional[int] = None):
    """(gu[M, 2I], s[M, I]): gu = x @ Wgu^T (gate rows [0, I), up rows [I, 2I)) by the 4-wave
    k_gemm_fw4 with s = silu(gate) * up in its epilogue (csrc/gemm_fw4.hip, flags 1024;
    k_swiglu_fwd's arithmetic, same bits).  None if the shape does not tile (I % 128,
    M % 256, K % 64)."""
    M, K = x.shape
    I2 = wgu.shape[0]
    I = I2 // 2
    if not gemm_fw4_swiglu_fits(M, I2, K) or wgu.shape[1] != K:
        return None
    hk = _req_act(x, x.dtype, "gemm_fw4_swiglu.x")
    _req(wgu, x.dtype, "gemm_fw4_swiglu.w")
    gu = torch.empty(M, I2, dtype=x.dtype, device=x.device) if gu_out is None else gu_out
    s = torch.empty(M, I, dtype=x.dtype, device=x.device) if s_out is None else s_out
    _req(gu, x.dtype, "gemm_fw4_swiglu.gu", M * I2)
    _req(s, x.dtype, "gemm_fw4_swiglu.s", M * I)
    fl = (_FW4_FLAGS if flags is None else flags) & ~(16 | 128)
    if flags is not None and (flags & (16 | 128)) == (16 | 128):
        fl |= 16 | 128  # SCHED 5
    _chk(lib().dlt_gemm_fw4(_p(x), _p(wgu), _p(gu), M, I2, K, K, K, I2, (fl | 1024) & ~4096, hk, _p(s), I, _stream()),
         "gemm_fw4_swiglu")
    return gu, s


def gemm_qkv_rope(x: torch.Tensor, wqkv: torch.Tensor, S: int, cos: torch.Tensor, sin: torch.Tensor,
                  out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """qkv[M, 3H] = x @ Wqkv^T with NeoX RoPE applied to the q and k heads (head_dim 64,
    position of row m = m % S) in the GEMM epilogue -- the packed-QKV projection and
    ``rope_qk_inplace`` in one kernel.  cos/sin: [>= S, 32] fp32.  None if the shape
    does not tile (3H % 192, M % 256, K % 128)."""
    M, K = x.shape
    N = wqkv.shape[0]
    H = N // 3
    if (not gemm_bf16_fits192(M, N, K) or N % 3 or H % 64 or wqkv.shape[1] != K or M % S
            or cos.shape[-1] != 32 or cos.shape[0] < S):
        return None
    _req(x, torch.bfloat16, "gemm_qkv_rope.x")
    _req(wqkv, torch.bfloat16, "gemm_qkv_rope.w")
    _req(cos, torch.float32, "gemm_qkv_rope.cos")
    _req(sin, torch.float32, "gemm_qkv_rope.sin", cos.numel())
    c = torch.empty(M, N, dtype=torch.bfloat16, device=x.device) if out is None else out
    _req(c, torch.bfloat16, "gemm_qkv_rope.out", M * N)
    _chk(lib().dlt_gemm_bf16_qkv_rope(_p(x), _p(wqkv), _p(c), M, H, K, S, _p(cos), _p(sin), _fwd_flags(), _stream()),
         "gemm_qkv_rope")
    return c


def gemm_gu_swiglu(x: torch.Tensor, wgu: torch.Tensor, gu_out: Optional[torch.Tensor] = None,
                   s_out: Optional[torch.Tensor] = None):
    """(gu[M, 2I], s[M, I]) with gu = x @ Wgu^T (gate rows [0, I), up rows [I, 2I)) and
    s = silu(gate) * up computed in the GEMM epilogue.  None if the shape does not tile
    (I % 96, M % 256, K % 128)."""
    M, K = x.shape
    I2 = wgu.shape[0]
    I = I2 // 2
    if not gemm_bf16_fits192(M, I2, K) or I2 % 2 or I % 96 or wgu.shape[1] != K:
        return None
    _req(x, torch.bfloat16, "gemm_gu_swiglu.x")
    _req(wgu, torch.bfloat16, "gemm_gu_swiglu.w")
    gu = torch.empty(M, I2, dtype=torch.bfloat16, device=x.device) if gu_out is None else gu_out
    s = torch.empty(M, I, dtype=torch.bfloat16, device=x.device) if s_out is None else s_out
    _req(gu, torch.bfloat16, "gemm_gu_swiglu.gu", M * I2)
    _req(s, torch.bfloat16, "gemm_gu_swiglu.s", M * I)
    _chk(lib().dlt_gemm_bf16_gu_swiglu(_p(x), _p(wgu), _p(gu), _p(s), M, I, K, _fwd_flags(), _stream()), "gemm_gu_swiglu")
    return gu, s


def gemm_dgrad(dy: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """dX[M, Nout] = dY[M, Nred] @ W[Nred, Nout] with W read as stored (the data gradient
    of a projection y = x @ W^T) by the hand-written persistent MFMA kernel in its
    reduction-major-B form; bf16 or fp16 (all three tensors one dtype).  None (nothing
    launched) when the shape does not tile (M % 256, Nout % 192, Nred % 128)."""
    M, Nred = dy.shape
    Nout = w.shape[1]
    if not gemm_bf16_fits(M, Nout, Nred) or w.shape[0] != Nred:
        return None
    dt = dy.dtype
    if dt not in _WG_HK:
        raise ValueError("gemm_dgrad: bf16 / fp16 operands expected")
    _req(dy, dt, "gemm_dgrad.dy")
    _req(w, dt, "gemm_dgrad.w")
    c = torch.empty(M, Nout, dtype=dt, device=dy.device) if out is None else out
    _req(c, dt, "gemm_dgrad.out", M * Nout)
    _chk(lib().dlt_gemm_bf16_nn(_p(dy), _p(w), _p(c), M, Nout, Nred, Nred, Nout, Nout, _GB_FLAGS, _WG_HK[dt],
                                _stream()), "gemm_dgrad")
    return c


def gemm_down_swiglu_bwd(dd: torch.Tensor, wdown: torch.Tensor, gu: torch.Tensor,
                         out: Optional[torch.Tensor] = None, s_out: Optional[torch.Tensor] = None
                         ) -> Optional[torch.Tensor]:
    """dgu[M, 2I] = SwiGLU backward of ds = dd[M, H] @ Wdown[H, I] (bf16-rounded) against
    the kept gu[M, 2I] -- the down projection's data gradient and ``swiglu_bwd`` in one
    kernel (same math and roundings as the unfused pair).  ``s_out`` [M, I] (optional):
    also writes s = silu(g) * u with the forward's bits (``swiglu_bwd``'s s_out).  None
    if it does not tile."""
    M, H = dd.shape
    I = wdown.shape[1]
    if not gemm_bf16_fits192(M, I, H) or wdown.shape[0] != H or tuple(gu.shape) != (M, 2 * I):
        return None
    dt = dd.dtype if dd.dtype in _WG_HK else torch.bfloat16  # bf16 or fp16, one format for all
    _req(dd, dt, "gemm_down_swiglu_bwd.dd")
    _req(wdown, dt, "gemm_down_swiglu_bwd.w")
    _req(gu, dt, "gemm_down_swiglu_bwd.gu")
    c = torch.empty(M, 2 * I, dtype=dt, device=dd.device) if out is None else out
    _req(c, dt, "gemm_down_swiglu_bwd.out", M * 2 * I)
    if s_out is not None:
        _req(s_out, dt, "gemm_down_swiglu_bwd.s_out", M * I)
    _chk(lib().dlt_gemm_bf16_down_swiglu_bwd(_p(dd), _p(wdown), _p(gu), _p(c), _p(s_out), M, I, H, _GB_FLAGS,
                                             _WG_HK[dt], _stream()), "gemm_down_swiglu_bwd")
    return c


def scale_bf16(x: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None,
               mul: float = 1.0) -> torch.Tensor:
    """y = x * scale * mul with a device scalar (no host sync) and a host factor, x bf16
    or fp16; falls back for odd sizes."""
    if x.dtype == torch.float32:
        from . import hip_f32
        return hip_f32.scale(x, scale, out=out, mul=mul)
    hk = _req_act(x, x.dtype, "scale_bf16.x")
    s = scale.reshape(1).float().contiguous()
    if x.numel() % 8:
        y = (x.float() * s * mul).to(x.dtype)
        return y if out is None else out.copy_(y)
    y = torch.empty_like(x) if out is None else out
    _req(y, x.dtype, "scale_bf16.out", x.numel())
    _chk(lib().dlt_scale_bf16(_p(x), _p(y), x.numel(), _p(s), float(mul), hk, _stream()), "scale_bf16")
    return y
