"""fp64 references, derived tolerances, fp32 kernel models with planted defects and the fixed
test inputs of the post-norm kernels (``k_postnorm_fwd``, ``k_postnorm_add_dropout_rmsnorm_fwd``,
``k_postnorm_bwd`` in ops/csrc/norm.hip), shared by test_postnorm_cpu.py and test_postnorm_gpu.py.

References.  Each takes the 16-bit tensors the kernel takes (and its weights) and computes in
fp64.  The value is returned BEFORE the kernel's one rounding to the activation dtype, so the
"final rounding" term below bounds one rounding whichever way a near-tie falls.

Tolerances: a sum of named terms per output element.
  ua  = half an ulp of the activation dtype relative to the value: 2^-8 (bf16, 8 significant
        bits) or 2^-11 (fp16, 11 bits)
  sub = fp16 only: half the spacing of the subnormals, 2^-25 (an fp16 result under 2^-14 is
        rounded to a multiple of 2^-24, whatever its size); bf16 has the fp32 exponent range
  u23 = 2^-23, the fp32 ulp of a value in [1, 2)
  acc = H * u23 relative: the sum of squares behind rstd is H fp32 additions (each rounds to
        2^-24 of a partial sum bounded by the total), the hardware rsqrt is good to an ulp and
        the multiplies of an element round once each; carried through the products it scales
  cancel = the fp32 sum behind mean(g * xh) is off by up to H * 2^-24 of mean |g * xh| (not of the
        possibly much smaller |mean|), times the xh * rstd it multiplies
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from distributed_llm_trainer_amd.ops import rng

U23 = 2.0 ** -23
EPS = 1e-6   # the model's RMSNorm eps
M = 403      # rows: the last 4-row workgroup is part empty
HS = [64, 768, 1000, 2560]  # fewer chunks than lanes | NCH 3 exact | a part-filled last chunk | the NCH 12 form
ZERO_ROW = 3  # an all-zero branch row
BIG_ROW = 7   # a row scaled by 1e4 (<= 5e4: inside fp16's range)
KEY = 0x9E3779B9
DEFECTS_FWD = ("eps_dropped", "neighbour_row_rstd")
DEFECTS_FUSED = ("dropout_before_norm", "unrounded_branch", "ln2_weight_used")
DEFECTS_BWD = ("mean_term_dropped", "eps_dropped", "neighbour_row_rstd")


def ua(dtype) -> float:
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def sub(dtype) -> float:
    return 2.0 ** -25 if dtype == torch.float16 else 0.0


class Checked(NamedTuple):
    ref: torch.Tensor
    tol: torch.Tensor


class Inputs(NamedTuple):
    a: torch.Tensor      # [M, H] activation dtype: the branch (o_proj / down_proj) GEMM output
    du: torch.Tensor     # [M, H] activation dtype: dL/du, u the normed branch
    resid: torch.Tensor  # [M, H] fp32: the residual stream the fused forward adds to
    w: torch.Tensor      # [H] fp32 post-norm weight, with negative and exactly-zero entries
    w2: torch.Tensor     # [H] fp32: the following pre-norm's weight (the fused forward's ln2)
    H: int


def make_inputs(H: int, dtype, seed: int = 0, rows: int = M) -> Inputs:
    g = torch.Generator().manual_seed(1000 * seed + H)
    a = torch.randn(rows, H, generator=g).clamp_(-5.0, 5.0)
    a[ZERO_ROW] = 0.0
    a[BIG_ROW] *= 1e4
    du = torch.randn(rows, H, generator=g)
    resid = torch.randn(rows, H, generator=g)
    ws = []
    for _ in range(2):
        w = 1.0 + 0.5 * torch.randn(H, generator=g)
        w[0] = -w[0].abs() - 0.25
        w[H // 2 + 5] = -0.75
        w[3] = 0.0
        w[H // 2 + 1] = 0.0
        ws.append(w)
    return Inputs(a.to(dtype), du.to(dtype), resid, ws[0], ws[1], H)


def _eps64(eps: float) -> float:
    return float(np.float32(eps))


# ------------------------------------------------------------------------------ forward
def fwd_ref(inp: Inputs, eps: float = EPS) -> Checked:
    """u = a * rsqrt(mean(a^2) + eps) * w, [M, H] fp64, unrounded."""
    dtype, H = inp.a.dtype, inp.H
    x = inp.a.double()
    rstd = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + _eps64(eps))
    ref = x * rstd * inp.w.double()
    acc = H * U23 * ref.abs()  # one product chain per element
    final = ua(dtype) * (ref.abs() + acc) + sub(dtype)  # the one rounding, of the kernel's value (within acc of ref)
    return Checked(ref, final + acc)


def fwd_model(inp: Inputs, eps: float = EPS, defect: Optional[str] = None) -> torch.Tensor:
    """fp32 model of k_postnorm_fwd: u [M, H] in the activation dtype.
    ``defect``: eps_dropped | neighbour_row_rstd."""
    x = inp.a.float()
    rstd = torch.rsqrt((x * x).sum(dim=-1, keepdim=True) / inp.H + (0.0 if defect == "eps_dropped" else eps))
    if defect == "neighbour_row_rstd":
        rstd = torch.roll(rstd, 1, dims=0)
    return (x * rstd * inp.w.float()).to(inp.a.dtype)


# ------------------------------------------------------------------------------ fused forward
class Fused(NamedTuple):
    x: Checked      # [M, H] fp32 residual stream after the add
    y: Checked      # [M, H] the following norm's output, before its rounding
    rstd: Checked   # [M]


def _drop(t: torch.Tensor, p: float, key: int) -> torch.Tensor:
    if p <= 0.0:
        return t
    keep = rng.keep_mask(t.shape, key, p)
    return torch.where(keep, t / (1.0 - p), torch.zeros((), dtype=t.dtype))


def fused_ref(inp: Inputs, p: float, key: int = KEY, eps: float = EPS) -> Fused:
    """x = resid + dropout(round_act(u)), y = x * rsqrt(mean(x^2) + eps) * w2, in fp64.

    The rounding of u is part of the definition.  Where u - acc and u + acc (the kernel's fp32 u
    lies between them) round to the same activation value, the rounded u is known exactly and x
    carries only the fp32 roundings of the dropout scale and of the add;
    where they straddle a rounding boundary, either neighbour is right and x may differ by their
    distance."""
    dtype, H = inp.a.dtype, inp.H
    u = fwd_ref(inp, eps)
    acc = H * U23 * u.ref.abs()
    ur = u.ref.to(dtype).double()
    lo, hi = (u.ref - acc).to(dtype).double(), (u.ref + acc).to(dtype).double()
    tie = torch.maximum((hi - ur).abs(), (lo - ur).abs())
    x = inp.resid.double() + _drop(ur, p, key)
    # fp32 roundings of x, 2^-24 each: the dropout scale 1 / (1 - p) as an fp32 number, its product
    # with u (both relative to the scaled u) and the add (relative to |x| <= |resid| + |scaled u|)
    tol_x = _drop(tie, p, key) + 0.5 * U23 * (inp.resid.double().abs() + 3.0 * _drop(ur.abs(), p, key))
    rstd = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + _eps64(eps))
    xh = x * rstd
    y = xh * inp.w2.double()
    # d y_i = rstd * w2_i * (dx_i - xh_i * mean(xh * dx)), and |mean(xh * dx)| <= max |dx| as
    # mean |xh| <= rms(xh) <= 1: the error x carries reaches y through both terms
    prop = rstd * inp.w2.double().abs() * (tol_x + xh.abs() * tol_x.amax(dim=-1, keepdim=True))
    acc_y = H * U23 * y.abs()
    tol_y = ua(dtype) * (y.abs() + acc_y + prop) + sub(dtype) + acc_y + prop
    # rstd = (mean(x^2) + eps)^-1/2: relative error half that of the mean, which x moves by at
    # most 2 * max(tol_x / |x|) ~ 2 * rstd * max tol_x in rms terms; plus the fp32 accumulation
    tol_r = rstd * (H * U23 + rstd * tol_x.amax(dim=-1, keepdim=True))
    return Fused(Checked(x, tol_x), Checked(y, tol_y), Checked(rstd.squeeze(-1), tol_r.squeeze(-1)))


def fused_model(inp: Inputs, p: float, key: int = KEY, eps: float = EPS, defect: Optional[str] = None):
    """fp32 model of k_postnorm_add_dropout_rmsnorm_fwd: (x fp32, y activation dtype, rstd fp32).
    ``defect``: dropout_before_norm | unrounded_branch | ln2_weight_used."""
    dtype, H = inp.a.dtype, inp.H
    a = inp.a.float()
    if defect == "dropout_before_norm":
        a = _drop(a, p, key)
    wp = (inp.w2 if defect == "ln2_weight_used" else inp.w).float()
    u = a * torch.rsqrt((a * a).sum(dim=-1, keepdim=True) / H + eps) * wp
    if defect != "unrounded_branch":
        u = u.to(dtype).float()
    x = inp.resid + (u if defect == "dropout_before_norm" else _drop(u, p, key))
    rstd = torch.rsqrt((x * x).sum(dim=-1, keepdim=True) / H + eps)
    return x, (x * rstd * inp.w2.float()).to(dtype), rstd.squeeze(-1)


# ------------------------------------------------------------------------------ backward
class Bwd(NamedTuple):
    da: Checked   # [M, H]
    dw: Checked   # [H]


def bwd_ref(inp: Inputs, eps: float = EPS) -> Bwd:
    """da = rstd * (g - xh * mean(g * xh)) with xh = a * rstd, g = du * w (fp64, unrounded) and
    dw = sum over rows of du * xh."""
    dtype, H = inp.a.dtype, inp.H
    x, g0 = inp.a.double(), inp.du.double()
    rstd = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + _eps64(eps))
    xh = x * rstd
    g = g0 * inp.w.double()
    mean = (g * xh).mean(dim=-1, keepdim=True)
    t1, t2 = rstd * g, rstd * xh * mean
    ref = t1 - t2
    acc = H * U23 * (t1.abs() + t2.abs())  # the accumulation term on the two products of the difference
    cancel = H * U23 * (rstd * xh).abs() * (g * xh).abs().mean(dim=-1, keepdim=True)
    final = ua(dtype) * (ref.abs() + acc + cancel) + sub(dtype)
    t = g0 * xh
    rows = x.shape[0]
    # fp32 accumulation over `rows` addends in any order: every addition rounds a partial sum
    # bounded by sum |addend| to 2^-24; each addend carries xh's relative error (H * 2^-23)
    dw = Checked(t.sum(dim=0), (rows + H) * U23 * t.abs().sum(dim=0))
    return Bwd(Checked(ref, final + acc + cancel), dw)


def bwd_model(inp: Inputs, eps: float = EPS, defect: Optional[str] = None):
    """fp32 model of k_postnorm_bwd: (da [M, H] in the activation dtype, dw fp32 [H]).
    ``defect``: mean_term_dropped | eps_dropped | neighbour_row_rstd."""
    H = inp.H
    x, g0 = inp.a.float(), inp.du.float()
    rstd = torch.rsqrt((x * x).sum(dim=-1, keepdim=True) / H + (0.0 if defect == "eps_dropped" else eps))
    if defect == "neighbour_row_rstd":
        rstd = torch.roll(rstd, 1, dims=0)
    xh = x * rstd
    g = g0 * inp.w.float()
    mean = (g * xh).sum(dim=-1, keepdim=True) / H
    if defect == "mean_term_dropped":
        mean = torch.zeros_like(mean)
    return (rstd * (g - xh * mean)).to(inp.a.dtype), (g0 * xh).sum(dim=0)


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
