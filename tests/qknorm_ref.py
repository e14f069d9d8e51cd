"""fp64 references, derived tolerances, fp32 kernel models with planted defects and the fixed
test inputs of the QK-norm kernels (``k_qknorm_rope_inplace`` in ops/csrc/elementwise.hip,
``k_qknorm_bwd`` in ops/csrc/norm.hip), shared by test_qknorm_cpu.py and test_qknorm_gpu.py.

References.  Each takes the 16-bit tensors the kernel takes (and its fp32 weights and RoPE
tables) and computes in fp64.  The value is returned BEFORE the kernel's one rounding to the
activation dtype, so the "final rounding" term below bounds one rounding whichever way a
near-tie falls.

Tolerances: a sum of named terms per output element.
  ua  = half an ulp of the activation dtype relative to the value: 2^-8 (bf16, 8 significant
        bits) or 2^-11 (fp16, 11 bits)
  sub = fp16 only: half the spacing of the subnormals, 2^-25 (an fp16 result under 2^-14 is
        rounded to a multiple of 2^-24, whatever its size); bf16 has the fp32 exponent range
  u23 = 2^-23, the fp32 ulp of a value in [1, 2)
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from distributed_llm_trainer_amd.ops.reference import rope_tables

U23 = 2.0 ** -23
EPS = 1e-6  # the model's RMSNorm eps
B, S = 2, 200  # M = 400 rows: no multiple of the 64 / 32 head slots of a k_qknorm_bwd block
HEADS = [(4, 4), (4, 2), (6, 2), (4, 1)]
ZERO_AT = (3, 1)    # (row, rotated head): an all-zero q head vector
BIG_AT = (7, -1)    # (row, rotated head): the last k head of the row, scaled by 1e4


def ua(dtype) -> float:
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def sub(dtype) -> float:
    return 2.0 ** -25 if dtype == torch.float16 else 0.0


class Checked(NamedTuple):
    ref: torch.Tensor
    tol: torch.Tensor


class Inputs(NamedTuple):
    qkv: torch.Tensor    # [M, (nh + 2 nkv) * hd] activation dtype: the QKV GEMM output
    dqkv: torch.Tensor   # same shape: q|k columns = dL/d(normalised head), v columns = dL/dv
    cos: torch.Tensor    # [S, hd / 2] fp32
    sin: torch.Tensor
    qw: torch.Tensor     # [hd] fp32, with negative and exactly-zero entries
    kw: torch.Tensor
    nh: int
    nkv: int
    hd: int


def make_inputs(nh: int, nkv: int, hd: int, dtype, seed: int = 0) -> Inputs:
    g = torch.Generator().manual_seed(1000 * seed + 100 * nh + 10 * nkv + hd)
    M, W = B * S, (nh + 2 * nkv) * hd
    qkv = torch.randn(M, W, generator=g).clamp_(-5.0, 5.0)
    hv = qkv.view(M, nh + 2 * nkv, hd)
    hv[ZERO_AT[0], ZERO_AT[1]] = 0.0
    hv[BIG_AT[0], nh + nkv + BIG_AT[1]] *= 1e4  # <= 5e4: inside fp16's range
    dqkv = torch.randn(M, W, generator=g)
    ws = []
    for _ in range(2):
        w = 1.0 + 0.5 * torch.randn(hd, generator=g)
        w[0] = -w[0].abs() - 0.25
        w[hd // 2 + 5] = -0.75
        w[3] = 0.0
        w[hd // 2 + 1] = 0.0
        ws.append(w)
    cos, sin = rope_tables(hd, S)
    return Inputs(qkv.to(dtype), dqkv.to(dtype), cos.contiguous(), sin.contiguous(), ws[0], ws[1], nh, nkv, hd)


def _heads(t: torch.Tensor, inp: Inputs):
    """The q|k head vectors [M, nh + nkv, hd] of a packed tensor (a view)."""
    return t.view(t.shape[0], inp.nh + 2 * inp.nkv, inp.hd)[:, :inp.nh + inp.nkv]


def _w(inp: Inputs, dtype=torch.float64) -> torch.Tensor:
    """[nh + nkv, hd]: the q weight for the q heads, the k weight for the k heads."""
    return torch.cat([inp.qw.to(dtype).expand(inp.nh, -1), inp.kw.to(dtype).expand(inp.nkv, -1)])


def _tables(inp: Inputs, M: int, dtype=torch.float64):
    pos = torch.arange(M) % S
    return inp.cos.to(dtype)[pos][:, None, :], inp.sin.to(dtype)[pos][:, None, :]


# ------------------------------------------------------------------------------ forward
def fwd_ref(inp: Inputs, eps: float = EPS) -> Checked:
    """rope(x * rsqrt(mean(x^2) + eps) * w) of every q|k head, [M, nh + nkv, hd] fp64, unrounded."""
    dtype, hd = inp.qkv.dtype, inp.hd
    x = _heads(inp.qkv, inp).double()
    M = x.shape[0]
    rstd = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + float(np.float32(eps)))
    u = x * rstd * _w(inp)
    c, s = _tables(inp, M)
    u1, u2 = u[..., :hd // 2], u[..., hd // 2:]
    ref = torch.cat([u1 * c - u2 * s, u2 * c + u1 * s], dim=-1)
    # |a| + |b| of the rotation pair: the two products whose sum / difference the element is
    pair = torch.cat([(u1 * c).abs() + (u2 * s).abs(), (u2 * c).abs() + (u1 * s).abs()], dim=-1)
    # fp32 accumulation over hd: the sum of squares behind rstd is hd fp32 additions (each
    # rounds to 2^-24 of a partial sum bounded by the total), the hardware rsqrt is good to an
    # ulp, and the four multiplies of an element round once each: hd * 2^-23 relative covers
    # them, carried to the element through both products of its pair
    acc = hd * U23 * pair
    # the one rounding to the activation dtype, of the kernel's value (within acc of ref)
    final = ua(dtype) * (ref.abs() + acc) + sub(dtype)
    return Checked(ref, final + acc)


def fwd_model(inp: Inputs, eps: float = EPS, defect: Optional[str] = None) -> torch.Tensor:
    """fp32 model of k_qknorm_rope_inplace: the whole packed output [M, W] in the activation
    dtype (v columns copied).  ``defect``: norm_after_rope | k_uses_q_weight | mean_over_half |
    eps_dropped | v_normalised."""
    dtype, hd, nh, nkv = inp.qkv.dtype, inp.hd, inp.nh, inp.nkv
    out = inp.qkv.clone()
    x = _heads(inp.qkv, inp).float()
    M = x.shape[0]
    w = _w(inp, torch.float32)
    if defect == "k_uses_q_weight":
        w = inp.qw.float().expand(nh + nkv, -1)
    c, s = _tables(inp, M, torch.float32)

    def norm(t, wt):
        ss = (t * t).sum(dim=-1, keepdim=True)
        mean = ss / (hd // 2 if defect == "mean_over_half" else hd)
        return t * torch.rsqrt(mean + (0.0 if defect == "eps_dropped" else eps)) * wt

    def rot(t):
        t1, t2 = t[..., :hd // 2], t[..., hd // 2:]
        return torch.cat([t1 * c - t2 * s, t2 * c + t1 * s], dim=-1)

    res = norm(rot(x), w) if defect == "norm_after_rope" else rot(norm(x, w))
    _heads(out, inp).copy_(res.to(dtype))
    if defect == "v_normalised":
        v = out.view(M, nh + 2 * nkv, hd)[:, nh + nkv:]
        v.copy_(norm(v.float(), inp.kw.float()).to(dtype))
    return out


# ------------------------------------------------------------------------------ backward
class Bwd(NamedTuple):
    dx: Checked     # [M, nh + nkv, hd]
    dqw: Checked    # [hd]
    dkw: Checked


def bwd_ref(inp: Inputs, eps: float = EPS) -> Bwd:
    """dx = rstd * (dxh - xh * mean(dxh * xh)) with xh = x * rstd, dxh = g * w (fp64, unrounded)
    and dw = sum over tokens and heads of g * xh."""
    dtype, hd, nh = inp.qkv.dtype, inp.hd, inp.nh
    x = _heads(inp.qkv, inp).double()
    g = _heads(inp.dqkv, inp).double()
    rstd = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + float(np.float32(eps)))
    xh = x * rstd
    dxh = g * _w(inp)
    mean = (dxh * xh).mean(dim=-1, keepdim=True)
    a, b = rstd * dxh, rstd * xh * mean
    ref = a - b
    # the forward's accumulation term on the two products of the difference ...
    acc = hd * U23 * (a.abs() + b.abs())
    # ... plus the cancellation inside mean(dxh * xh): its fp32 sum over hd is off by up to
    # hd * 2^-24 of mean |dxh * xh| (not of the possibly much smaller |mean|), times xh * rstd
    cancel = hd * U23 * (rstd * xh).abs() * (dxh * xh).abs().mean(dim=-1, keepdim=True)
    final = ua(dtype) * (ref.abs() + acc + cancel) + sub(dtype)
    dx = Checked(ref, final + acc + cancel)
    t = g * xh
    M = x.shape[0]
    dws = []
    for sl in (slice(0, nh), slice(nh, None)):
        n = M * t[:, sl].shape[1]  # addends per column
        ref_w = t[:, sl].sum(dim=(0, 1))
        # fp32 accumulation over n addends in any order: every addition rounds a partial sum
        # bounded by sum |addend| to 2^-24; each addend carries xh's relative error (hd * 2^-23)
        dws.append(Checked(ref_w, (n + hd) * U23 * t[:, sl].abs().sum(dim=(0, 1))))
    return Bwd(dx, dws[0], dws[1])


def bwd_model(inp: Inputs, eps: float = EPS, defect: Optional[str] = None):
    """fp32 model of k_qknorm_bwd: (the whole packed dqkv [M, W] in the activation dtype, dqw,
    dkw fp32).  ``defect``: mean_term_dropped | neighbour_rstd."""
    dtype, hd, nh = inp.qkv.dtype, inp.hd, inp.nh
    out = inp.dqkv.clone()
    x = _heads(inp.qkv, inp).float()
    g = _heads(inp.dqkv, inp).float()
    rstd = torch.rsqrt((x * x).sum(dim=-1, keepdim=True) / hd + eps)
    if defect == "neighbour_rstd":
        rstd = torch.roll(rstd, 1, dims=1)
    xh = x * rstd
    dxh = g * _w(inp, torch.float32)
    mean = (dxh * xh).sum(dim=-1, keepdim=True) / hd
    if defect == "mean_term_dropped":
        mean = torch.zeros_like(mean)
    _heads(out, inp).copy_((rstd * (dxh - xh * mean)).to(dtype))
    t = g * xh
    return out, t[:, :nh].sum(dim=(0, 1)), t[:, nh:].sum(dim=(0, 1))


# ------------------------------------------------------------------------------ checks
def worst(got: torch.Tensor, chk: Checked) -> float:
    """max over the elements of |got - ref| / tol (inf for a non-finite value; an element
    with zero tolerance must be exact)."""
    got = got.double().cpu()
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got - chk.ref).abs()
    ratio = torch.where(chk.tol > 0, err / chk.tol.clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0))
    return ratio.max().item()
