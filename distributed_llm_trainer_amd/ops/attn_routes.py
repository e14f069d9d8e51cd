"""The attention route a (activation dtype, head_dim) takes on the GPU, and what it can do.

One table for every place that asks "does this model's attention have feature X":

===========================  ======================================  ===  ======  =====  ===  =======  ===
route                        taken when                              doc  window  sinks  gqa  qk_norm  cap
===========================  ======================================  ===  ======  =====  ===  =======  ===
16-bit flash                 bf16 / fp16, head_dim 64 or 128         yes  yes     yes    yes  yes      yes
zero-padded 16-bit flash     bf16 / fp16, other head_dim < 128,      yes  yes     yes    no   no       yes
                             ``DLT_ATTN_PAD`` on
GEMM-formulated              bf16 / fp16, everything else            no   no      no     no   no       no
fp32 (flash, zero-padded     fp32, any head_dim                      no   no      no     no   no       no
flash, GEMM-formulated)
===========================  ======================================  ===  ======  =====  ===  =======  ===

gqa and qk_norm also need the packed QKV layout on the GPU.  cap = attention-score
soft-capping (``attn_softcap``): not one of :data:`FEATURES` (it is a number, not a switch, and
has no config key of the on/off kind); :func:`check_score_softcap` is its check.  The CPU and
the reference ops have every feature.  Pure Python: nothing here loads the HIP library.
"""
from __future__ import annotations

import os
from typing import Any, NamedTuple, Optional

import torch

# feature -> (what it is, the config key that turns it on)
FEATURES = {
    "doc": ("document-masked attention", "doc_sep_token"),
    "window": ("sliding-window attention", "sliding_window"),
    "sinks": ("attention sinks", "attention_sinks"),
    "gqa": ("grouped-query attention", "num_kv_heads < num_heads"),
    "qk_norm": ("QK-norm", "qk_norm"),
}
_NATIVE_ONLY = frozenset(("gqa", "qk_norm"))  # no zero-padded form; packed QKV layout only
_NAMES = {"flash": "flash", "padded": "zero-padded flash", "gemm": "GEMM-formulated"}


class Route(NamedTuple):
    kind: str            # "flash" | "padded" | "gemm"
    name: str            # for messages; the fp32 routes start with "fp32"
    pad: Optional[int]   # "padded": the flash head_dim the heads are zero-padded to
    features: frozenset  # of FEATURES
    head_dim: int
    dtype: Any


def route(dtype, head_dim: int, flash: bool = True) -> Route:
    """The route ``ops.for_device`` gives a model of this activation dtype and head_dim.
    ``flash=False``: the route inside ``ops/attn_gemm.py``, which never runs a head unpadded
    on the flash kernels (its entry points called directly at head_dim 64 pad to 128)."""
    from . import attn_gemm, hip, hip_f32
    fp32 = dtype == torch.float32
    native = flash and head_dim in (hip_f32 if fp32 else hip).ATTN_HEAD_DIMS
    pad = None if native else attn_gemm.pad_dim(dtype, head_dim)
    kind = "flash" if native else "padded" if pad else "gemm"
    if fp32:
        return Route(kind, "fp32 " + _NAMES[kind], pad, frozenset(), head_dim, dtype)
    has = frozenset() if kind == "gemm" else frozenset(FEATURES) - (_NATIVE_ONLY if pad else frozenset())
    return Route(kind, _NAMES[kind].replace("flash", "16-bit flash"), pad, has, head_dim, dtype)


def require(rt: Route, feature: str, where: str) -> None:
    """Raises NotImplementedError unless route ``rt`` has ``feature`` (no silent fallback)."""
    if feature in rt.features:
        return
    what, key = FEATURES[feature]
    raise NotImplementedError(
        f"{where}: the {rt.name} attention route (head_dim {rt.head_dim}, {rt.dtype}) has no {what} ({key}); "
        f"use bf16 or fp16 activations with head_dim "
        f"{'64 or 128' if feature in _NATIVE_ONLY else '<= 128'}")


def check_attention_features(device, head_dim: int, act_dtype, features, packed_qkv: bool = True) -> None:
    """Raises NotImplementedError when the attention route of this model on ``device`` lacks
    one of ``features`` (names of :data:`FEATURES`), or when one of them needs the packed QKV
    layout and ``packed_qkv`` is off.  Called where a model is configured, so the error comes
    before the first step, not inside it.  The CPU and the reference ops have every feature."""
    if torch.device(device).type != "cuda" or os.environ.get("DLT_ALLOW_REFERENCE_ON_GPU") == "1":
        return
    rt = route(act_dtype, head_dim)
    for f in sorted(features, key=list(FEATURES).index):  # a fixed order; an unknown name is a ValueError
        require(rt, f, "this model on the GPU")
        if f in _NATIVE_ONLY and not packed_qkv:
            raise NotImplementedError(f"{FEATURES[f][0]} ({FEATURES[f][1]}) on the GPU runs on the packed QKV layout "
                                      f"(DLT_PACKED_QKV=0 is not supported with it)")


def config_features(cfg) -> frozenset:
    """The features a model config asks of its attention route (the separator is set on the
    model, not in the config: ``set_doc_separator`` checks ``"doc"`` itself)."""
    on = {"gqa": cfg.num_kv_heads != cfg.num_heads, "qk_norm": getattr(cfg, "qk_norm", False),
          "sinks": getattr(cfg, "attention_sinks", False), "window": getattr(cfg, "sliding_window", None) is not None}
    return frozenset(f for f, v in on.items() if v)


# Largest cap the CAP kernels take.  Their exponent constant is cap * log2(e), and the DOC /
# window forward multiplies it with M_DEAD = -1e30 (the running max of a row that has seen no live
# key yet): the product must stay finite in fp32.  2^16 leaves three orders of magnitude, and a
# cap of that size no longer caps anything (Gemma-2 uses 50).
SCORE_SOFTCAP_MAX = 65536.0


def check_score_softcap_range(cap: float, where: str) -> None:
    """Raises ValueError for a cap the CAP kernels of the GPU routes do not take (> SCORE_SOFTCAP_MAX)."""
    if cap > SCORE_SOFTCAP_MAX:
        raise ValueError(f"{where}: the GPU attention kernels take a cap of at most {SCORE_SOFTCAP_MAX:g}, got {cap!r}")


def has_score_softcap(rt: Route) -> bool:
    """Route ``rt`` has the CAP kernels (attention-score soft-capping, ``attn_softcap``): the
    16-bit flash route and its zero-padded form."""
    return rt.kind != "gemm" and rt.dtype != torch.float32


def require_score_softcap(rt: Route, where: str) -> None:
    """Raises NotImplementedError unless route ``rt`` has the CAP kernels (no silent fallback, and
    no silently ignored ``softcap=``)."""
    if not has_score_softcap(rt):
        raise NotImplementedError(
            f"{where}: the {rt.name} attention route (head_dim {rt.head_dim}, {rt.dtype}) has no attention-score "
            f"soft-capping (attn_softcap); use bf16 or fp16 activations with head_dim <= 128")


def check_score_softcap(device, head_dim: int, act_dtype, where: str = "this model on the GPU", cap=None) -> None:
    """Raises NotImplementedError when the attention route of (``act_dtype``, ``head_dim``) on
    ``device`` cannot cap the scores, and ValueError when ``cap`` is given and beyond what its CAP
    kernels take (:data:`SCORE_SOFTCAP_MAX`).  Called where a capped model is configured
    (``enable_engine``), so the error comes before the first step.  The CPU and the reference
    ops cap on every route."""
    if torch.device(device).type != "cuda" or os.environ.get("DLT_ALLOW_REFERENCE_ON_GPU") == "1":
        return
    require_score_softcap(route(act_dtype, head_dim), where)
    if cap is not None:
        check_score_softcap_range(float(cap), where + ": attn_softcap")
