"""fp64 references, tolerances and fixed inputs for the grouped-query decode kernels
(``dec_norm_qkv_gqa``, ``dec_attn_gqa`` in ``ops/csrc/decode.hip``), shared by
test_decode_gqa_cpu.py and test_decode_gqa_gpu.py.  Built on tests/decode_ref.py: the same
named tolerance terms, the same input generators, the same convention (the last value of a
kernel is returned before its final bf16 rounding).

Grouped-query layout: the packed projection row is q | k | v with nh query heads and nkv key
and value heads of 64 dims; query head h reads K/V head h // G, G = nh / nkv.  The split
attention kernel divides the keys 0..pos into NS chunks of C = ``dec_attn_chunk(maxS, NS)``
keys, computes (max m, sum l, unnormalised o) per chunk and merges them in the order
s = 0 .. NS - 1, each partial scaled by exp(m_s - M).
"""
from __future__ import annotations

from typing import Optional

import torch

from tests import decode_ref as R

# ------------------------------------------------------------------------------ shapes
HEADS = ((4, 1), (4, 2), (6, 2), (12, 4), (4, 4))  # (nh, nkv) of the attention grid
QKV_HEADS = ((4, 1), (4, 2), (4, 4), (6, 2))       # hidden 256, 256, 256, 384
QKV_POS = R.QKV_POS
QKV_MAXS = R.QKV_MAXS
ATTN_MAXS = 200  # 200 / 4 = 50: the last chunk of NS = 4 is ragged, and so is any rounding of it
ATTN_SPLITS = (1, 2, 4)
ATTN_KINDS = ("randn", "large60", "equal")
ATTN_BATCHES = (1, 8)
ATTN_SCALE = R.ATTN_SCALE


def attn_positions(C: int, maxS: int = ATTN_MAXS):
    """{0, 1, C - 1, C, C + 1, 2C, maxS - 1} inside the cache: both sides of a chunk boundary,
    an empty trailing chunk (pos < C with NS > 1), the full cache."""
    return tuple(sorted({p for p in (0, 1, C - 1, C, C + 1, 2 * C, maxS - 1) if 0 <= p < maxS}))


# ------------------------------------------------------------------------------ QKV
def qkv_gqa_inputs(nh: int, nkv: int, wbf16: bool):
    """(h [8, H] fp32, norm weight, wqkv [H + 2 * nkv * 64, H] bf16)."""
    H = nh * 64
    return R.normed_inputs(700 + H + nkv, H, H + 2 * nkv * 64, wbf16)


def _rope_checked(x, pre, c, s) -> R.Checked:
    """NeoX RoPE of bf16 GEMV outputs x [B, heads, 64] with the pre-rounding error bound
    ``pre``: the terms of ``decode_ref.qkv_ref`` (final rounding, tie flips of x1 / x2 through
    their partial derivatives, the fp32 dot products' own error through the same)."""
    x1, x2, p1, p2 = x[..., :32], x[..., 32:], pre[..., :32], pre[..., 32:]
    ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    flip = torch.cat([R.U8 * ((x1 * c).abs() + (x2 * s).abs()), R.U8 * ((x2 * c).abs() + (x1 * s).abs())], dim=-1)
    prop = torch.cat([c.abs() * p1 + s.abs() * p2, c.abs() * p2 + s.abs() * p1], dim=-1)
    return R.Checked(ref, R.U8 * ref.abs() + flip + prop)


def qkv_gqa_ref(h, lnw, wqkv, cos, sin, pos: int, nh: int, nkv: int, kmask=None, rope_pos: Optional[int] = None,
                rope_v: bool = False, k_from_v: bool = False):
    """dec_norm_qkv_gqa: {"q": [B, nh, 64], "k": [B, nkv, 64], "v": [B, nkv, 64]} of Checked.
    Planted defects: ``rope_pos`` (another position's table row), ``rope_v`` (v rotated like
    k), ``k_from_v`` (the k block computed from the v weight rows)."""
    B, H = h.shape
    KV = nkv * 64
    assert H == nh * 64 and wqkv.shape == (H + 2 * KV, H)
    g = R.gemv(R.normed(h, lnw), wqkv, kmask)
    x = R.bf16_round(g.y)  # the GEMV outputs, bf16 like torch's matmul
    pre = R.gemv_pre_tol(g, H)
    rp = pos if rope_pos is None else rope_pos
    c, s = cos[rp].double().to(x.device), sin[rp].double().to(x.device)
    ks = slice(H + KV, H + 2 * KV) if k_from_v else slice(H, H + KV)
    vs = slice(H + KV, H + 2 * KV)
    out = {"q": _rope_checked(x[:, :H].view(B, nh, 64), pre[:, :H].view(B, nh, 64), c, s),
           "k": _rope_checked(x[:, ks].view(B, nkv, 64), pre[:, ks].view(B, nkv, 64), c, s)}
    if rope_v:
        out["v"] = _rope_checked(x[:, vs].view(B, nkv, 64), pre[:, vs].view(B, nkv, 64), c, s)
    else:
        out["v"] = R.Checked(g.y[:, vs].view(B, nkv, 64), R.gemv_tol(g, H)[:, vs].view(B, nkv, 64))
    return out


# ------------------------------------------------------------------------------ attention
def attn_gqa_inputs(nh: int, nkv: int, maxS: int = ATTN_MAXS, kind: str = "randn"):
    """(q [8, nh * 64], K cache, V cache [8, nkv, maxS, 64]) bf16: ``decode_ref.attn_inputs``
    with nh heads for q and with nkv heads for the caches."""
    q = R.attn_inputs(nh, maxS, kind)[0]
    _, kc, vc = R.attn_inputs(nkv, maxS, kind)
    return q, kc, vc


def kv_head_of(nh: int, nkv: int, head_map: str = "div") -> torch.Tensor:
    hq = torch.arange(nh)
    if head_map == "div":
        return hq // (nh // nkv)
    assert head_map == "mod"
    return hq % nkv


def attn_gqa_ref(q, kc, vc, pos: int, scale: float, nh: int, head_map: str = "div", extra_keys: int = 0,
                 drop_boundary_key: Optional[int] = None, no_rescale: Optional[int] = None) -> R.Checked:
    """dec_attn_gqa: ``decode_ref.attn_ref`` per query head h on K/V head h // G; [B, nh, 64],
    tolerance U8 |o| + 1e-4 sum p |v|.  The reasoning beside ``attn_ref`` carries over; the
    split adds, per partial, one exp(m_s - M) factor (the same 80 * 2^-24 + 2^-22 relative as
    a probability) and one fp32 multiply-add per output element: a few 2^-24 relative, inside
    the 20x margin of the 1e-4 term.
    Planted defects: ``head_map="mod"`` (K/V head h % nkv), ``extra_keys`` (key pos + 1 ...
    included), ``drop_boundary_key=C`` (the last key of chunk 0, key min(C, pos + 1) - 1, left
    out; needs pos >= 1), ``no_rescale=C`` (chunk partials, each relative to its own max,
    summed without the exp(m_s - M) factors)."""
    nkv = kc.shape[1]
    idx = kv_head_of(nh, nkv, head_map).to(kc.device)
    K, V = kc.index_select(1, idx), vc.index_select(1, idx)  # [B, nh, maxS, 64]
    if drop_boundary_key is not None:
        assert pos >= 1
        d = min(drop_boundary_key, pos + 1) - 1
        keep = torch.tensor([j for j in range(K.shape[2]) if j != d], device=K.device)
        return R.attn_ref(q, K.index_select(2, keep), V.index_select(2, keep), pos - 1, scale, extra_keys)
    if no_rescale is not None:
        C, n = no_rescale, pos + 1
        B = K.shape[0]
        s = torch.einsum("bhd,bhjd->bhj", q.double().view(B, nh, 64), K[:, :, :n].double()) * scale
        num = torch.zeros(B, nh, 64, dtype=torch.float64, device=K.device)
        den = torch.zeros(B, nh, 1, dtype=torch.float64, device=K.device)
        for lo in range(0, n, C):
            sl = s[:, :, lo:lo + C]
            p = torch.exp(sl - sl.amax(dim=-1, keepdim=True))
            num += torch.einsum("bhj,bhjd->bhd", p, V[:, :, lo:min(lo + C, n)].double())
            den += p.sum(dim=-1, keepdim=True)
        o = num / den
        return R.Checked(o, torch.zeros_like(o))
    return R.attn_ref(q, K, V, pos, scale, extra_keys)


def attn_gqa_split32(q, kc, vc, pos: int, scale: float, nh: int, NS: int, C: int) -> torch.Tensor:
    """An fp32 torch model of the split kernel: per chunk (m, l, o) in fp32, merged in the
    order s = 0 .. NS - 1 with exp(m_s - M), empty chunks skipped; bf16 [B, nh, 64]."""
    B, nkv = kc.shape[:2]
    idx = kv_head_of(nh, nkv).to(kc.device)
    n = pos + 1
    qf = q.float().view(B, nh, 64)
    parts = []
    for s in range(NS):
        lo, hi = s * C, min((s + 1) * C, n)
        if hi <= lo:
            continue
        K = kc[:, :, lo:hi].float().index_select(1, idx)
        V = vc[:, :, lo:hi].float().index_select(1, idx)
        sc = torch.einsum("bhd,bhjd->bhj", qf, K) * torch.tensor(scale, dtype=torch.float32)
        m = sc.amax(dim=-1, keepdim=True)
        p = torch.exp(sc - m)
        parts.append((m, p.sum(dim=-1, keepdim=True), torch.einsum("bhj,bhjd->bhd", p, V)))
    if NS == 1:
        m, l, o = parts[0]
        return (o * (1.0 / l)).bfloat16()
    M = parts[0][0]
    for m, _, _ in parts[1:]:
        M = torch.maximum(M, m)
    L = torch.zeros_like(M)
    acc = torch.zeros_like(parts[0][2])
    for m, l, o in parts:
        f = torch.exp(m - M)
        L = L + l * f
        acc = acc + o * f
    return (acc / L).bfloat16()
