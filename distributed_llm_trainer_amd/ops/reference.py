"""Plain-PyTorch (fp32-accumulating) reference implementations of every fused op.

These define the numerical contract of the HIP kernels in ``ops/csrc`` and are the
CPU execution path of the engine (``models/engine.py``), which lets the hand-written
forward/backward of the whole model be validated against autograd on CPU.

Reference semantics being reproduced (``/root/reference/src/models/gpt.py``):
RMSNorm ``:66-67`` (eps 1e-6, fp32 math), RoPE ``:82-98,116-118,144-147`` (NeoX
half-split), attention ``:199-240`` (causal, scale 1/sqrt(hd), fp32 softmax, dropout on
probabilities), SwiGLU ``:278-282``, shifted cross-entropy ``:449-453``
(ignore_index -100, mean over valid targets).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import rng

IGNORE_INDEX = -100


# ----------------------------------------------------------------- embedding
def embedding_fwd(ids: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    return weight.index_select(0, ids.reshape(-1)).float()


def embedding_bwd(ids: torch.Tensor, dout: torch.Tensor, dweight: torch.Tensor) -> None:
    dweight.index_add_(0, ids.reshape(-1), dout.reshape(-1, dout.shape[-1]).to(dweight.dtype))


# --------------------------------------------------- residual add + dropout + RMSNorm
def dropout_apply(x: torch.Tensor, key: int, p: float) -> torch.Tensor:
    if p <= 0.0:
        return x
    keep = rng.keep_mask(x.shape, key, p, device=x.device)
    return torch.where(keep, x / (1.0 - p), torch.zeros((), dtype=x.dtype, device=x.device))


def add_dropout_rmsnorm_fwd(resid: Optional[torch.Tensor], delta: Optional[torch.Tensor],
                            weight: torch.Tensor, eps: float, p: float, key: int,
                            out_dtype=torch.bfloat16, y_out=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """x = resid + dropout(delta);  y = x * rsqrt(mean(x^2)+eps) * w.

    Returns (x fp32, y out_dtype, rstd fp32[M]).  ``resid``/``delta`` may be None.
    """
    if resid is None:
        x = dropout_apply(delta.float(), key, p)
    elif delta is None:
        x = resid.float()
    else:
        x = resid.float() + dropout_apply(delta.float(), key, p)
    rstd = torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps)
    y = (x * rstd * weight.float()).to(out_dtype)
    if y_out is not None:
        y_out.copy_(y)
        y = y_out
    return x, y, rstd.squeeze(-1)


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, rstd: torch.Tensor, weight: torch.Tensor,
                dres: Optional[torch.Tensor], dweight: torch.Tensor, p_prev: float, key_prev: int,
                dy_scale: Optional[torch.Tensor] = None,
                want_ddelta: bool = True, ddelta_out=None, dy_mul: float = 1.0) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Backward of add_dropout_rmsnorm.

    dx = dres + J_rmsnorm^T dy ; ddelta = dropout_bwd(dx) (grad for the delta that was
    added with dropout key ``key_prev``).  ``dweight`` (fp32) is accumulated in place.
    ``dy_scale`` (0-dim tensor) multiplies ``dy`` first (used for the loss scale).
    """
    out_dt = dy.dtype
    dy = dy.float()
    if dy_scale is not None:
        dy = dy * dy_scale.float()
    if dy_mul != 1.0:
        dy = dy * dy_mul
    r = rstd.float().unsqueeze(-1)
    xh = x.float() * r
    w = weight.float()
    dweight += (dy * xh).sum(dim=0).to(dweight.dtype)
    g = dy * w
    h = x.shape[-1]
    dx = r * (g - xh * (g * xh).sum(dim=-1, keepdim=True) / h)
    if dres is not None:
        dx = dx + dres.float()
    ddelta = None
    if want_ddelta:
        ddelta = dropout_apply(dx, key_prev, p_prev).to(out_dt)
        if ddelta is dx:  # fp32 without dropout: its own tensor, as the kernels' (postnorm_bwd rewrites it in place)
            ddelta = dx.clone()
        if ddelta_out is not None:
            ddelta_out.copy_(ddelta)
            ddelta = ddelta_out
    return dx, ddelta


# ---------------------------------------------------------------- post-norms
def _postnorm_check(a: torch.Tensor, name: str) -> None:
    if a.dim() != 2:
        raise ValueError(f"{name}: expected [M, H], got {list(a.shape)}")


def postnorm_fwd(a: torch.Tensor, w: torch.Tensor, eps: float, out=None) -> torch.Tensor:
    """The post-norm of a branch output (cfg.post_norm): u = a * rsqrt(mean(a^2) + eps) * w over
    the rows of ``a`` [M, H] (the GEMM output as rounded to the activation dtype), fp32 math,
    rounded once to a's dtype.  Out of place."""
    _postnorm_check(a, "postnorm_fwd.a")
    x = a.float()
    u = (x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps) * w.float()).to(a.dtype)
    if out is not None:
        out.copy_(u)
        return out
    return u


def postnorm_add_dropout_rmsnorm_fwd(resid: torch.Tensor, a: torch.Tensor, w_post: torch.Tensor, w: torch.Tensor,
                                     eps: float, p: float, key: int, out_dtype=torch.bfloat16, y_out=None):
    """:func:`postnorm_fwd` of ``a`` then :func:`add_dropout_rmsnorm_fwd` with the rounded u as its
    delta (the HIP kernel fuses the two; the rounding of u is part of the definition)."""
    return add_dropout_rmsnorm_fwd(resid, postnorm_fwd(a, w_post, eps), w, eps, p, key, out_dtype, y_out=y_out)


def postnorm_bwd_workspace(M: int, H: int, device):
    """The HIP kernel's weight-gradient workspace; the reference needs none."""
    return None


def postnorm_bwd(du: torch.Tensor, a: torch.Tensor, w: torch.Tensor, eps: float, dw: torch.Tensor, ws=None):
    """Backward of :func:`postnorm_fwd`, in place: ``du`` (dL/du) is overwritten with
    da = rstd * (g - xh * mean(g * xh)), g = du * w, xh = a * rstd, rstd from the raw ``a``; fp32
    math, rounded once.  ``dw`` += sum over rows of du * xh."""
    _postnorm_check(du, "postnorm_bwd.du")
    if a.shape != du.shape or a.dtype != du.dtype:
        raise ValueError("postnorm_bwd.a: expected the shape and dtype of du")
    x, g0 = a.float(), du.float()
    rstd = torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps)
    xh = x * rstd
    g = g0 * w.float()
    dw += (g0 * xh).sum(dim=0).to(dw.dtype)
    du.copy_((rstd * (g - xh * (g * xh).mean(dim=-1, keepdim=True))).to(du.dtype))
    return du


# ------------------------------------------------------------------- RoPE
def rope_tables(head_dim: int, seq_len: int, base: float = 10000.0, device=None):
    """cos/sin [S, hd/2] fp32 (the reference caches the duplicated [S, hd] form)."""
    inv_freq = 1.0 / (base ** (torch.arange(0, head_dim, 2, device=device).float() / head_dim))
    t = torch.arange(seq_len, device=device).float()
    freqs = torch.outer(t, inv_freq)
    return freqs.cos(), freqs.sin()


def _rot(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def _packed_dims(qkv: torch.Tensor, nh: int, nkv=None):
    """(nkv, hd, H, KV) of a packed [M, H + 2*KV] QKV row: q (nh heads) | k | v (nkv heads each)."""
    nkv = nh if nkv is None else int(nkv)
    if nkv < 1 or nh % nkv:
        raise ValueError(f"nkv ({nkv}) must divide nh ({nh})")
    W = qkv.shape[-1]
    if W % (nh + 2 * nkv):
        raise ValueError(f"packed QKV width {W} is no multiple of nh + 2*nkv = {nh + 2 * nkv}")
    hd = W // (nh + 2 * nkv)
    return nkv, hd, nh * hd, nkv * hd


def _qkv_views(qkv: torch.Tensor, B: int, S: int, nh: int, nkv=None):
    """Views q [B, S, nh, hd], k, v [B, S, nkv, hd] into the packed QKV, and hd."""
    nkv, hd, H, KV = _packed_dims(qkv, nh, nkv)
    t = qkv.view(B, S, H + 2 * KV)
    return (t[..., :H].view(B, S, nh, hd), t[..., H:H + KV].view(B, S, nkv, hd),
            t[..., H + KV:].view(B, S, nkv, hd)), hd


def rope_qkv_fwd(qkv: torch.Tensor, B: int, S: int, nh: int, cos: torch.Tensor, sin: torch.Tensor, nkv=None):
    """qkv [B*S, H + 2*KV] -> q [B, nh, S, hd], k, v [B, nkv, S, hd] (q,k rotated in fp32)."""
    (tq, tk, tv), hd = _qkv_views(qkv, B, S, nh, nkv)
    c = cos[:S].view(1, S, 1, hd // 2)
    s = sin[:S].view(1, S, 1, hd // 2)
    q = _rot(tq.float(), c, s).transpose(1, 2)
    k = _rot(tk.float(), c, s).transpose(1, 2)
    v = tv.float().transpose(1, 2)
    dt = qkv.dtype
    return q.to(dt).contiguous(), k.to(dt).contiguous(), v.to(dt).contiguous()


def rope_qkv_bwd(dq: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor,
                 cos: torch.Tensor, sin: torch.Tensor, out=None) -> torch.Tensor:
    """Inverse rotation; returns dqkv [B*S, H + 2*KV] in dq's dtype (dk, dv: [B, nkv, S, hd])."""
    B, nh, S, hd = dq.shape
    c = cos[:S].view(1, 1, S, hd // 2)
    s = sin[:S].view(1, 1, S, hd // 2)
    gq = _rot(dq.float(), c, -s)
    gk = _rot(dk.float(), c, -s)
    res = torch.cat([t.transpose(1, 2).reshape(B * S, -1) for t in (gq, gk, dv.float())], dim=1).to(dq.dtype)
    if out is not None:
        out.copy_(res)
        return out
    return res


def rope_qk_inplace(qkv: torch.Tensor, B: int, S: int, nh: int, cos: torch.Tensor, sin: torch.Tensor, nkv=None):
    """Rotate the q and k column blocks of the packed [B*S, H + 2*KV] QKV in place."""
    (tq, tk, _), hd = _qkv_views(qkv, B, S, nh, nkv)
    c = cos[:S].view(1, S, 1, hd // 2)
    s = sin[:S].view(1, S, 1, hd // 2)
    for t in (tq, tk):
        t.copy_(_rot(t.float(), c, s).to(qkv.dtype))
    return qkv


def qknorm_rope_inplace(qkv: torch.Tensor, B: int, S: int, nh: int, cos: torch.Tensor, sin: torch.Tensor,
                        qw: torch.Tensor, kw: torch.Tensor, eps: float, raw_out: torch.Tensor, nkv=None):
    """QK-norm + RoPE of the q and k heads of the packed [B*S, H + 2*KV] QKV in place: head
    vector x (the GEMM output as rounded to the activation dtype) -> rope(x * rsqrt(mean(x^2)
    + eps) * w) with ``qw`` / ``kw`` [hd]; norm and rotation in fp32, rounded once.  The
    pre-norm q|k columns go to ``raw_out`` [B*S, H + KV]; v is untouched."""
    (tq, tk, _), hd = _qkv_views(qkv, B, S, nh, nkv)
    _, _, H, KV = _packed_dims(qkv, nh, nkv)
    if tuple(raw_out.shape) != (B * S, H + KV) or raw_out.dtype != qkv.dtype:
        raise ValueError(f"qknorm_rope_inplace: raw_out must be [{B * S}, {H + KV}] {qkv.dtype}")
    raw_out.copy_(qkv[:, :H + KV])
    c = cos[:S].view(1, S, 1, hd // 2)
    s = sin[:S].view(1, S, 1, hd // 2)
    for t, w in ((tq, qw), (tk, kw)):
        x = t.float()
        u = x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps) * w.float()
        t.copy_(_rot(u, c, s).to(qkv.dtype))
    return qkv


def qknorm_bwd(dqkv: torch.Tensor, raw: torch.Tensor, B: int, S: int, nh: int, qw: torch.Tensor, kw: torch.Tensor,
               eps: float, dqw: torch.Tensor, dkw: torch.Tensor, nkv=None, ws=None):
    """Backward of the norm of :func:`qknorm_rope_inplace`.  The q|k columns of ``dqkv`` hold
    g = dL/du (u the normalised pre-RoPE head: ``attention_bwd_packed`` applies the inverse
    rotation) and are overwritten with dx = rstd * (dxh - xh * mean(dxh * xh)), xh = x * rstd,
    dxh = g * w, x from ``raw``; fp32 math, rounded once; v columns untouched.  ``dqw`` /
    ``dkw`` += sum over tokens and heads of g * xh."""
    (gq, gk, _), hd = _qkv_views(dqkv, B, S, nh, nkv)
    nkv, _, H, KV = _packed_dims(dqkv, nh, nkv)
    r = raw.view(B, S, H + KV)
    xq, xk = r[..., :H].view(B, S, nh, hd), r[..., H:].view(B, S, nkv, hd)
    for gt, xt, w, dw in ((gq, xq, qw, dqw), (gk, xk, kw, dkw)):
        x, g = xt.float(), gt.float()
        rstd = torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps)
        xh = x * rstd
        dxh = g * w.float()
        dw += (g * xh).sum(dim=(0, 1, 2)).to(dw.dtype)
        gt.copy_((rstd * (dxh - xh * (dxh * xh).mean(dim=-1, keepdim=True))).to(dqkv.dtype))
    return dqkv


def _split_packed(qkv, B, S, nh, nkv=None):
    views, _ = _qkv_views(qkv, B, S, nh, nkv)
    return tuple(t.transpose(1, 2).contiguous() for t in views)


def attention_fwd_packed(qkv: torch.Tensor, B: int, S: int, nh: int, p: float, key: int, out=None, mask=None,
                         doc=None, nkv=None, window=None, sink=None, softcap=None):
    """Causal attention straight on the (already roped) packed [B*S, H + 2*KV] QKV."""
    q, k, v = _split_packed(qkv, B, S, nh, nkv)
    return attention_fwd(q, k, v, p, key, True, out=out, doc=doc, window=window, sink=sink, softcap=softcap)


def attention_bwd_packed(qkv, o, do, lse, p: float, key: int, B: int, S: int, nh: int,
                         cos: torch.Tensor, sin: torch.Tensor, out=None, doc=None, nkv=None,
                         window=None, sink=None, dsink=None, softcap=None) -> torch.Tensor:
    """Backward of attention_fwd_packed + the in-place RoPE: dqkv [B*S, H + 2*KV] (pre-RoPE)."""
    q, k, v = _split_packed(qkv, B, S, nh, nkv)
    dq, dk, dv = attention_bwd(q, k, v, o, do, lse, p, key, True, doc=doc, window=window, sink=sink, dsink=dsink,
                               softcap=softcap)
    res = rope_qkv_bwd(dq.float(), dk.float(), dv.float(), cos, sin).to(qkv.dtype)
    if out is not None:
        out.copy_(res)
        return out
    return res


# -------------------------------------------------------------- attention
def doc_bounds(ids: torch.Tensor, sep: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Document bounds of packed sequences ``ids`` [B, S]: token ``sep`` ends a document
    and belongs to it.  Returns int32 ``(lo, hi)`` [B, S]: the first and the last position
    of each token's document (``lo[i]`` = 1 + the last separator before i, or 0;
    ``hi[i]`` = the first separator at or after i, or S - 1).  Both are non-decreasing
    along S, and ``lo <= i <= hi``."""
    if ids.dim() != 2:
        raise ValueError("doc_bounds: ids must be [B, S]")
    S = ids.shape[1]
    pos = torch.arange(S, device=ids.device, dtype=torch.int64).expand_as(ids)
    is_sep = ids == sep
    # lo: running max of (separator position + 1), shifted right by one token
    after = torch.where(is_sep, pos + 1, torch.zeros_like(pos))
    lo = torch.zeros_like(pos)
    if S > 1:
        lo[:, 1:] = torch.cummax(after, dim=1).values[:, :-1]
    # hi: running min from the right of the separator positions
    at = torch.where(is_sep, pos, torch.full_like(pos, S - 1))
    hi = torch.cummin(at.flip(1), dim=1).values.flip(1)
    return lo.to(torch.int32).contiguous(), hi.to(torch.int32).contiguous()


class WindowBounds(tuple):
    """``(lo, hi)`` of :func:`window_bounds`, with the window they hold in ``.window``: an
    attention op given these in ``doc=`` together with ``window=`` does not fold it in twice."""

    def __new__(cls, lo, hi, window: int):
        self = super().__new__(cls, (lo, hi))
        self.window = int(window)
        return self


def window_bounds(B: int, S: int, W: int, device, doc=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Bounds of a sliding window of ``W`` >= 1 keys in the form of :func:`doc_bounds`: query q
    sees key k iff q - W < k <= q, i.e. ``lo[q] = max(0, q - W + 1) <= k <= q``, which is the
    same as ``k <= q <= hi[k] = min(S - 1, k + W - 1)``.  With ``doc`` = (lo, hi) the two masks
    are merged (max of the lower, min of the upper bounds): both stay non-decreasing along S
    and keep the lo / hi equivalence, so the DOC attention kernels take them as they are.
    Returns int32 contiguous ``(lo, hi)`` [B, S]."""
    if isinstance(W, bool) or int(W) != W or W < 1:
        raise ValueError(f"window_bounds: W must be an integer >= 1, got {W!r}")
    if isinstance(doc, (tuple, list)) and len(doc) == 2 and isinstance(doc[0], torch.Tensor):
        device = doc[0].device  # "cuda" names the current device, the bounds carry its index
    pos = torch.arange(S, device=device, dtype=torch.int64)
    lo = (pos - (int(W) - 1)).clamp_(min=0).to(torch.int32)
    hi = (pos + (int(W) - 1)).clamp_(max=S - 1).to(torch.int32)
    lo, hi = lo.expand(B, S), hi.expand(B, S)
    if doc is not None:
        dlo, dhi = _req_doc(doc, B, S, device, "window_bounds")
        lo, hi = torch.maximum(lo, dlo), torch.minimum(hi, dhi)
    return WindowBounds(lo.contiguous(), hi.contiguous(), W)


def _fold_window(window, doc, B: int, S: int, device):
    """``window=`` of the attention ops folded into ``doc``; a window >= S is no window."""
    if window is None:
        return doc
    if isinstance(window, bool) or int(window) != window or window < 1:
        raise ValueError(f"attn: window must be None or an integer >= 1, got {window!r}")
    if window >= S or (isinstance(doc, WindowBounds) and doc.window == window):
        return doc
    return window_bounds(B, S, int(window), device, doc=doc)


def _req_doc(doc, B: int, S: int, device, name: str):
    """``doc`` = (lo, hi) of :func:`doc_bounds`: int32, contiguous, [B, S], on ``device``."""
    if not isinstance(doc, (tuple, list)) or len(doc) != 2:
        raise TypeError(f"{name}: doc must be None or (lo, hi)")
    for t, n in zip(doc, ("lo", "hi")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise TypeError(f"{name}.doc.{n}: expected an int32 tensor")
        if tuple(t.shape) != (B, S):
            raise ValueError(f"{name}.doc.{n}: expected shape [{B}, {S}], got {list(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name}.doc.{n}: must be contiguous")
        if t.device != torch.device(device):
            raise ValueError(f"{name}.doc.{n}: expected device {device}, got {t.device}")
    return doc


def _masked_out(S: int, device, causal: bool, doc, B: int, name: str) -> Optional[torch.Tensor]:
    """Dense boolean mask of the scores a query must not see ([S, S], or [B, 1, S, S] with
    a document mask: key k is visible to query q iff lo[q] <= k <= q)."""
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool, device=device), diagonal=1) if causal else None
    if doc is None:
        return mask
    if not causal:
        raise NotImplementedError("the document mask is defined for causal attention")
    lo, _ = _req_doc(doc, B, S, device, name)
    kpos = torch.arange(S, device=device).view(1, 1, 1, S)
    return mask | (kpos < lo.view(B, 1, S, 1))


def _kv_group(q, k, v, name: str) -> int:
    """Group size G = nh // nkv of q [B, nh, S, hd] with k, v [B, nkv, S, hd]."""
    B, nh, S, hd = q.shape
    if k.shape != v.shape or k.dim() != 4:
        raise ValueError(f"{name}: k {list(k.shape)} and v {list(v.shape)} must have the same 4-d shape")
    nkv = k.shape[1]
    if (k.shape[0], k.shape[2], k.shape[3]) != (B, S, hd) or nkv < 1 or nh % nkv:
        raise ValueError(f"{name}: k/v shape {list(k.shape)} does not fit q {list(q.shape)} "
                         f"(expected [B, nkv, S, hd] with nkv dividing nh)")
    return nh // nkv


def _rep_kv(t: torch.Tensor, G: int) -> torch.Tensor:
    return t if G == 1 else t.repeat_interleave(G, dim=1)


def _req_sink(sink, nh: int, device, name: str, grad: bool = False) -> torch.Tensor:
    """``sink`` of the attention ops: one logit per query head, [nh], on ``device``; fp32 (a
    gathered 16-bit FSDP unit is upcast).  ``grad``: the fp32 gradient accumulator, as it is."""
    if not isinstance(sink, torch.Tensor) or not sink.is_floating_point() or tuple(sink.shape) != (nh,):
        raise ValueError(f"{name}: expected a floating-point [{nh}] tensor (one logit per query head)")
    if grad and sink.dtype != torch.float32:
        raise ValueError(f"{name}: expected an fp32 tensor, got {sink.dtype}")
    if sink.device != torch.device(device):
        raise ValueError(f"{name}: expected device {device}, got {sink.device}")
    return sink.float()


def check_score_cap(softcap, name: str = "attn.softcap") -> Optional[float]:
    """``softcap=`` of the attention ops (the attention-score cap): None is off; otherwise a real
    number (no bool), finite and > 0."""
    if softcap is None:
        return None
    cap = check_softcap(softcap, name)
    if cap == 0.0:
        raise ValueError(f"{name}: the cap must be finite and > 0 (None turns it off), got {softcap!r}")
    return cap


def attention_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, p: float, key: int,
                  causal: bool = True, out=None, doc=None, window=None,
                  sink=None, softcap=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """q [B, nh, S, hd], k, v [B, nkv, S, hd] -> o [B*S, nh*hd] (q dtype), lse [B, nh, S] fp32.
    ``doc`` = (lo, hi) from :func:`doc_bounds` adds the intra-document mask.  nkv < nh is
    grouped-query attention: query head h attends with kv head h // (nh // nkv).  ``window`` = W
    is sliding-window attention (:func:`window_bounds`, merged with ``doc``).  ``sink`` (fp32
    [nh]) is one more logit per query head in the softmax denominator, not scaled and with no
    value row: p_j = exp(s_j) / (sum_j exp(s_j) + exp(sink[h])), lse = log of that denominator;
    dropout applies to the p_j only.  ``softcap`` = CAP: attention-score soft-capping, the scaled
    scores become CAP * tanh(s / CAP) before the masks (masked keys stay at -inf; the sink is not
    capped), and lse is that of the capped scores."""
    B, nh, S, hd = q.shape
    cap = check_score_cap(softcap)
    doc = _fold_window(window, doc, B, S, q.device)
    G = _kv_group(q, k, v, "attn")
    scale = 1.0 / math.sqrt(hd)
    k, v = _rep_kv(k.float(), G), _rep_kv(v.float(), G)
    s = torch.matmul(q.float(), k.transpose(-2, -1)) * scale
    if cap is not None:
        s = cap * torch.tanh(s / cap)
    mask = _masked_out(S, q.device, causal, doc, B, "attn")
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    if sink is not None:
        lse = torch.logaddexp(lse, _req_sink(sink, nh, q.device, "attn.sink").view(1, nh, 1).expand_as(lse))
    prob = torch.exp(s - lse.unsqueeze(-1))
    if p > 0.0:
        keep = rng.attn_keep_mask(B * nh, S, S, key, p, device=q.device).view(B, nh, S, S)
        prob = torch.where(keep, prob / (1.0 - p), torch.zeros((), device=q.device))
    o = torch.matmul(prob, v.float())
    o = o.transpose(1, 2).reshape(B * S, nh * hd).to(q.dtype)
    if out is not None:
        out.copy_(o)
        o = out
    return o, lse


def attention_bwd(q, k, v, o, do, lse, p: float, key: int, causal: bool = True, doc=None, window=None,
                  sink=None, dsink=None, softcap=None):
    """Flash-style backward from (o, lse).  do/o are [B*S, H]; returns dq [B,nh,S,hd] and
    dk, dv in k's shape [B,nkv,S,hd] (summed over each kv head's query group in fp32).
    With ``sink`` the forward's ``lse`` already holds the sink, so dq / dk / dv need nothing
    else (the sink column has dP = 0 and delta = rowsum(dO * O) already is sum_j P_j dP_j);
    ``dsink`` (fp32 [nh]) += -sum_{b,q} exp(sink[h] - lse[b,h,q]) * delta[b,h,q].
    ``softcap``: the forward's; with t = tanh(s / CAP), dS carries 1 - t^2 into dq and dk."""
    B, nh, S, hd = q.shape
    cap = check_score_cap(softcap, "attn_bwd.softcap")
    if (sink is None) != (dsink is None):
        raise ValueError("attn_bwd: sink and dsink go together")
    doc = _fold_window(window, doc, B, S, q.device)
    G = _kv_group(q, k, v, "attn_bwd")
    scale = 1.0 / math.sqrt(hd)
    qf, kf, vf = q.float(), _rep_kv(k.float(), G), _rep_kv(v.float(), G)
    of = o.float().view(B, S, nh, hd).transpose(1, 2)
    dof = do.float().view(B, S, nh, hd).transpose(1, 2)
    s = torch.matmul(qf, kf.transpose(-2, -1)) * scale
    dt2 = None
    if cap is not None:
        t = torch.tanh(s / cap)
        s, dt2 = cap * t, 1.0 - t * t
    mask = _masked_out(S, q.device, causal, doc, B, "attn_bwd")
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    prob = torch.exp(s - lse.unsqueeze(-1))
    if p > 0.0:
        keep = rng.attn_keep_mask(B * nh, S, S, key, p, device=q.device).view(B, nh, S, S)
        pd = torch.where(keep, prob / (1.0 - p), torch.zeros((), device=q.device))
    else:
        keep, pd = None, prob
    dv = torch.matmul(pd.transpose(-2, -1), dof)
    dpd = torch.matmul(dof, vf.transpose(-2, -1))
    dp = torch.where(keep, dpd / (1.0 - p), torch.zeros((), device=q.device)) if keep is not None else dpd
    delta = (dof * of).sum(dim=-1, keepdim=True)
    if sink is not None:
        sink = _req_sink(sink, nh, q.device, "attn_bwd.sink")
        _req_sink(dsink, nh, q.device, "attn_bwd.dsink", grad=True)
        p_sink = torch.exp(sink.view(1, nh, 1) - lse)
        dsink += -(p_sink * delta.squeeze(-1)).sum(dim=(0, 2))
    ds = prob * (dp - delta)
    if dt2 is not None:
        ds = ds * dt2
    dq = torch.matmul(ds, kf) * scale
    dk = torch.matmul(ds.transpose(-2, -1), qf) * scale
    if G > 1:
        dk = dk.view(B, nh // G, G, S, hd).sum(dim=2)
        dv = dv.view(B, nh // G, G, S, hd).sum(dim=2)
    dt = q.dtype
    return dq.to(dt), dk.to(dt), dv.to(dt)


# ----------------------------------------------------------------- SwiGLU
def swiglu_fwd(gu: torch.Tensor, out=None) -> torch.Tensor:
    """gu [M, 2I] (gate | up) -> silu(gate) * up [M, I]."""
    i = gu.shape[-1] // 2
    g, u = gu[:, :i].float(), gu[:, i:].float()
    r = (g * torch.sigmoid(g) * u).to(gu.dtype)
    if out is not None:
        out.copy_(r)
        return out
    return r


def swiglu_bwd(gu: torch.Tensor, da: torch.Tensor, out=None, s_out=None) -> torch.Tensor:
    """``s_out``: also writes s = silu(g) * u (as swiglu_fwd)."""
    i = gu.shape[-1] // 2
    if s_out is not None:
        swiglu_fwd(gu, out=s_out)
    g, u = gu[:, :i].float(), gu[:, i:].float()
    d = da.float()
    sg = torch.sigmoid(g)
    silu = g * sg
    dg = d * u * sg * (1.0 + g * (1.0 - sg))
    du = d * silu
    r = torch.cat([dg, du], dim=-1).to(gu.dtype)
    if out is not None:
        out.copy_(r)
        return out
    return r


# ------------------------------------------------------ cross-entropy (fused with grad)
def check_softcap(softcap, name: str = "ce.softcap") -> float:
    """The final-logit soft cap of an op as a float: 0 (or None) is off; otherwise a real number
    (no bool), finite and > 0."""
    if softcap is None:
        return 0.0
    if isinstance(softcap, bool) or not isinstance(softcap, (int, float)):
        raise TypeError(f"{name}: expected a float, got {softcap!r}")
    cap = float(softcap)
    if cap == 0.0:
        return 0.0
    if not math.isfinite(cap) or cap < 0.0:
        raise ValueError(f"{name}: the cap must be finite and > 0 (0 turns it off), got {softcap!r}")
    return cap


def softcap_logits(logits: torch.Tensor, cap: float) -> torch.Tensor:
    """``cap * tanh(logits / cap)`` in fp32 (the model's final-logit soft cap; logits as stored)."""
    return float(cap) * torch.tanh(logits.float() / float(cap))


def cross_entropy_fwd_bwd(logits: torch.Tensor, targets: torch.Tensor, vocab: int,
                          n_valid: torch.Tensor, grad_scale: float = 1.0, z_loss: float = 0.0,
                          z_rows: Optional[torch.Tensor] = None, softcap: float = 0.0) -> torch.Tensor:
    """Per-row loss [M] fp32; ``logits`` [M, Vp] is overwritten with
    grad_scale * dloss_mean/dlogits.

    Columns >= vocab are padding and get zero gradient.  Rows whose target is
    IGNORE_INDEX get zero loss and zero gradient.  ``n_valid`` is a 0-dim tensor.

    The z-loss form (``z_loss`` != 0 or ``z_rows`` given, fp32 [M]): the row's objective is
    ``(lse - logit[target]) + z_loss * lse^2``, so the softmax part of the gradient carries
    the factor ``1 + 2 z_loss lse`` (possibly negative; used as it is).  The returned rows stay
    the cross-entropy part and ``z_rows`` receives lse^2 (0 on ignored rows).

    The CAP form (``softcap`` != 0, finite and > 0): everything above is taken of
    ``c = softcap * tanh(logits / softcap)``, formed in fp32 from the stored logits, and the
    gradient with respect to the stored logits carries ``1 - tanh^2(logits / softcap)``.
    """
    cap = check_softcap(softcap)
    zform = float(z_loss) != 0.0 or z_rows is not None
    if zform:
        if not isinstance(z_rows, torch.Tensor):
            raise TypeError("ce.z_rows: the z-loss form needs an fp32 [M] tensor for the rows' lse^2")
        if z_rows.device != logits.device:
            raise ValueError(f"ce.z_rows: expected a tensor on {logits.device}, got {z_rows.device}")
        if z_rows.dtype != torch.float32:
            raise TypeError(f"ce.z_rows: expected torch.float32, got {z_rows.dtype}")
        if tuple(z_rows.shape) != (logits.shape[0],):
            raise ValueError(f"ce.z_rows: expected [{logits.shape[0]}], got {tuple(z_rows.shape)}")
    lf = logits[:, :vocab].float()
    if cap != 0.0:
        th = torch.tanh(lf / cap)
        lf = cap * th
    lse = torch.logsumexp(lf, dim=-1)
    valid = targets != IGNORE_INDEX
    tgt = torch.where(valid, targets, torch.zeros_like(targets))
    picked = lf.gather(1, tgt.unsqueeze(1)).squeeze(1)
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse))
    grad = torch.exp(lf - lse.unsqueeze(1))
    if zform:
        grad = grad * (1.0 + 2.0 * float(z_loss) * lse).unsqueeze(1)
        z_rows.copy_(torch.where(valid, lse * lse, torch.zeros_like(lse)))
    grad.scatter_add_(1, tgt.unsqueeze(1), -torch.ones_like(picked).unsqueeze(1))
    grad = grad * (valid.float() * grad_scale / n_valid.float().clamp(min=1)).unsqueeze(1)
    if cap != 0.0:
        grad = grad * (1.0 - th * th)
    logits.zero_()
    logits[:, :vocab] = grad.to(logits.dtype)
    return loss


def lmhead_loss_fits(M: int, Vp: int, K: int) -> bool:
    return M > 0 and Vp > 0 and K > 0


def lmhead_loss(nf: torch.Tensor, w: torch.Tensor, targets: torch.Tensor, V: int, block_rows: int = 1024):
    """(row_loss [M], lse [M]) fp32 of the lm_head without keeping its logits: the product
    nf[M, K] @ w[Vp, K]^T in fp32, rounded to the activation dtype (as stored logits are),
    then an fp32 log-sum-exp over the columns < V; row_loss = lse - logit[target], 0 for
    IGNORE_INDEX rows.  Row blocks bound the fp32 temporaries to [block_rows, V]."""
    M = nf.shape[0]
    wf = w[:V].float()
    loss = torch.empty(M, dtype=torch.float32, device=nf.device)
    lse = torch.empty(M, dtype=torch.float32, device=nf.device)
    for a in range(0, M, block_rows):
        b = min(M, a + block_rows)
        lf = (nf[a:b].float() @ wf.t()).to(nf.dtype).float()
        t = targets[a:b]
        valid = t != IGNORE_INDEX
        lse[a:b] = torch.logsumexp(lf, dim=-1)
        picked = lf.gather(1, torch.where(valid, t, torch.zeros_like(t)).unsqueeze(1)).squeeze(1)
        loss[a:b] = torch.where(valid, lse[a:b] - picked, torch.zeros_like(picked))
    return loss, lse


# -------------------------------------------------------------- optimizer
def adamw_step(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
               shadow: Optional[torch.Tensor], lr: float, beta1: float, beta2: float, eps: float,
               weight_decay: float, step: int, grad_scale: torch.Tensor) -> None:
    """torch.optim.AdamW semantics (decoupled wd, bias correction), grad pre-scaled."""
    g = grad.float() * grad_scale.float()
    param.mul_(1.0 - lr * weight_decay)
    exp_avg.lerp_(g, 1.0 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = (exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(eps)
    param.addcdiv_(exp_avg, denom, value=-lr / bc1)
    if shadow is not None:
        shadow.copy_(param.to(shadow.dtype))


def sumsq(x: torch.Tensor, out: torch.Tensor) -> None:
    out += x.float().pow(2).sum()


def scale_bf16(x: torch.Tensor, scale: torch.Tensor, out: torch.Tensor = None, mul: float = 1.0) -> torch.Tensor:
    """y = x * scale * mul (scale: 0-d/1-element device tensor), result in x's dtype."""
    y = (x.float() * scale.reshape(()).float() * mul).to(x.dtype)
    return y if out is None else out.copy_(y)
