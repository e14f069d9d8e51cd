"""fp64 reference and derived tolerances of the z-loss forms of the cross-entropy kernels
(``ops/csrc/loss.hip`` / ``fp32.hip``, ZL = true), built on tests/stream_ref.py and shared by
test_zloss_cpu.py, test_zloss_gpu.py and zloss_ref_child.py.  Nothing here needs a GPU.

For a row with a real target, ``z = lse(logits[:V])`` and coefficient ``c``:
    loss_rows = z - logit[target]                      (the cross-entropy part alone)
    z_rows    = z^2
    grad_j    = (p_j * zf - [j == target]) * grad_scale / max(n_valid, 1),  zf = 1 + 2 c z
and zero everywhere on rows whose target is -100 and on the padding columns.

Tolerances: sums of named terms on top of ``ce_ref``'s (its U23 = one fp32 ulp per rounding).
``ce_ref`` returns the loss tolerance ``lse_err + U23 |loss|`` and the gradient tolerance
``pre + final_rounding``; the two inner bounds are taken back out of them exactly as they went in.
  z_rows:  2 |lse| lse_err (the error of lse through the square) + U23 lse^2 (the product)
  zf:      2 c lse_err (lse through the fma) + U23 (|2 c lse| + |zf|) (the fma's result and the
           fp32 coefficient)
  grad:    ce_ref's pre-rounding bound scaled by |zf| (everything that makes p_j / n wrong)
           + |p_j scale| zf_err (the factor's own error)
           + U23 |p_j zf scale| (one more product: inv_n * zf, or p * zf on the target)
           + on the target 2 U23 scale ("target patch, unscaled": the subtraction of 1 and the
             product with 1 / n round a value of at most |zf| + 1, and ce_ref's patch term scaled
             by |zf| pays for the |zf| part only -- with zf near zero or negative it pays nothing)
           + the final rounding to the logits' format of a value within all that.
None of it is fitted to a kernel's output.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from tests.stream_ref import (BF, CE_BY_NAME, CE_CASES, CE_CASES_512, CE_CASES_PLAIN, CE_NV_MODES, CE_SHAPES,  # noqa: F401
                              CE_VARIANTS, DT_NAME, DTYPES, F32, F64, HF, I64, U23, Checked, Guarded, bits, ce_depth,
                              ce_inputs, ce_n_valid, ce_ref, ce_variant, f32, final_rounding, half_ulp, round_to,
                              sub_floor)

Z_COEFS = (1e-4, 1e-2)
Z_SCALES = (1.0, 4096.0)

Z_DEFECTS = ("no_z_grad", "zf_half", "patch_times_zf", "z_unscaled", "z_norm_M", "ignored_row_z", "lse_over_padding",
             "z_rows_lse", "zf_abs", "zf_clamp")


class ZCE(NamedTuple):
    loss: Checked  # [M]      the cross-entropy part of every row
    z: Checked     # [M]      lse^2
    grad: Checked  # [M, Vp]  before the rounding to the logits' format
    zf: torch.Tensor  # [M] fp64, the rows' factor 1 + 2 c lse (for the tests' own assertions)


def zce_ref(logits: torch.Tensor, targets: torch.Tensor, V: int, n_valid: int, grad_scale: float, c: float,
            defect: Optional[str] = None, wide: bool = True) -> ZCE:
    """The z-loss form at exactly the kernel's inputs (logits as stored: bf16, fp16 or fp32; the
    coefficient as the fp32 the kernel receives).  Defects: see Z_DEFECTS and test_zloss_cpu.py."""
    M, Vp = logits.shape
    dt = logits.dtype
    ce = ce_ref(logits, targets, V, n_valid, grad_scale, wide=wide)
    c = f32(c)
    x = logits.double()
    real = (torch.arange(Vp) < V).unsqueeze(0)
    valid = (targets != -100)
    v1 = valid.unsqueeze(1)
    over = real if defect != "lse_over_padding" else torch.ones_like(real)
    lse = torch.logsumexp(torch.where(over, x, torch.full_like(x, -math.inf)), dim=1, keepdim=True)
    tgt = torch.where(valid, targets, torch.zeros_like(targets)).unsqueeze(1)
    loss = torch.where(v1, lse - x.gather(1, tgt), torch.zeros_like(lse)).squeeze(1)
    zf = 1.0 + 2.0 * c * lse
    if defect == "no_z_grad":
        zf = torch.ones_like(lse)
    elif defect == "zf_half":
        zf = 1.0 + c * lse
    elif defect == "zf_abs":
        zf = zf.abs()
    elif defect == "zf_clamp":
        zf = zf.clamp(min=0.0)
    n = M if defect == "z_norm_M" else max(n_valid, 1)
    scale = grad_scale / max(n_valid, 1)
    rows_on = torch.ones_like(v1) if defect == "ignored_row_z" else v1
    soft = torch.exp(x - lse) * real
    onehot = torch.zeros_like(x).scatter_(1, tgt, 1.0) * v1
    if defect == "patch_times_zf":
        grad = (soft - onehot) * zf * scale * v1
    elif defect == "z_unscaled":      # the z part of the gradient without grad_scale
        grad = ((soft - onehot) * scale + soft * (zf - 1.0) / max(n_valid, 1)) * v1
    elif defect == "z_norm_M":        # the z part normalised by the row count
        grad = ((soft - onehot) * scale + soft * (zf - 1.0) * grad_scale / n) * v1
    elif defect == "ignored_row_z":   # an ignored row given the z part of the gradient
        grad = (soft - onehot) * scale * v1 + soft * (zf - 1.0) * scale
    else:
        grad = (soft * zf - onehot) * scale * v1
    z = (lse if defect == "z_rows_lse" else lse * lse) * rows_on
    z = z.squeeze(1)

    # ---- tolerances (of the unmodified reference)
    lse_err = (ce.loss.tol - U23 * ce.loss.ref.abs()).unsqueeze(1) * v1        # as ce_ref put it in
    z_tol = ((2 * lse.abs() * lse_err + U23 * lse * lse) * v1).squeeze(1)
    zf_true = 1.0 + 2.0 * c * lse
    zf_err = 2 * c * lse_err + U23 * ((2 * c * lse).abs() + zf_true.abs())
    live = (v1 & real) & (scale != 0)
    # ce_ref: tol = pre + half_ulp (|ref| + pre) + sub_floor wherever the row is live
    hu, sf = half_ulp(dt), sub_floor(dt)
    pre_ce = torch.where(live, (ce.grad.tol - hu * ce.grad.ref.abs() - sf) / (1.0 + hu), ce.grad.tol).clamp(min=0.0)
    soft_s = soft * scale * v1
    pre = pre_ce * zf_true.abs() + soft_s * zf_err + U23 * (soft_s * zf_true).abs() + onehot * scale * 2 * U23
    true_grad = (soft * zf_true - onehot) * scale * v1
    g_tol = pre + final_rounding(true_grad, pre, dt) * live
    return ZCE(Checked(loss, ce.loss.tol), Checked(z, z_tol), Checked(grad, g_tol), zf_true.squeeze(1))


def z_cases(cases=CE_CASES):
    """(name, dtype, Vp, V, kind, n_valid mode, grad_scale, c): every case of ``cases`` (shape, format,
    kind and n_valid mode kept) with every coefficient and every grad_scale."""
    return [(f"{name}-c{c:g}-g{g:g}", dt, Vp, V, kind, nv_mode, g, c)
            for name, dt, Vp, V, kind, nv_mode, _ in cases for c in Z_COEFS for g in Z_SCALES]


def overflow_at(dtype) -> float:
    """The magnitude from which a round-to-nearest to ``dtype`` gives infinity."""
    return {BF: 2.0 ** 128 * (1 - 2.0 ** -9), HF: 65520.0, F32: 2.0 ** 128 * (1 - 2.0 ** -25)}[dtype]


def miss(out: torch.Tensor, chk: Checked, dtype) -> torch.Tensor:
    """Elements of a kernel output outside the tolerance.  A finite element must lie within tol of
    the reference.  An infinite one (fp16 at the ceiling of the format times the loss scale and a
    large zf) is right exactly where a value within tol of the reference rounds to that infinity;
    and where every such value does, infinity is the only right answer."""
    ref, tol = chk.ref.to(out.device), chk.tol.to(out.device)
    o = out.double().reshape(ref.shape)
    lim = overflow_at(dtype)
    inf = torch.isinf(o)
    ok_fin = ~inf & ((o - ref).abs() <= tol) & ~(ref.abs() - tol >= lim)
    ok_inf = inf & (ref.abs() + tol >= lim) & (torch.sign(o) == torch.sign(ref))
    return ~(ok_fin | ok_inf)


Z_CASES = z_cases(CE_CASES)
Z_CASES_512 = z_cases(CE_CASES_512)
Z_CASES_PLAIN = z_cases(CE_CASES_PLAIN)
Z_BY_NAME = {c[0]: c for c in Z_CASES + Z_CASES_512 + Z_CASES_PLAIN}
assert len(Z_BY_NAME) == len(Z_CASES + Z_CASES_512 + Z_CASES_PLAIN)

# the children of test_zloss_gpu.py: the knobs (read once per process) and the cases they reach
Z_CHILD_SETS = {
    "threads512": ({"DLT_CE_THREADS": "512", "DLT_CE_NT": "0"}, [c[0] for c in Z_CASES_512]),
    "plain": ({"DLT_CE_NT": "0"}, [c[0] for c in Z_CASES_PLAIN]),
}


def z_variants_reached() -> dict:
    """dtype -> the launch variants the default process and the two children exercise in Z form."""
    out = {}
    for dt in DTYPES:
        seen = {ce_variant(c[2]) for c in Z_CASES if c[1] == dt}
        seen |= {ce_variant(c[2], wide=False, nt=False) for c in Z_CASES_512 if c[1] == dt}
        seen |= {ce_variant(c[2], nt=False) for c in Z_CASES_PLAIN if c[1] == dt}
        out[dt] = seen
    return out


# fp32 kernel: (name, Vp, V) -- the float4 form (Vp % 4 == 0, aligned rows) and the scalar form (odd Vp)
F32_SHAPES = (("vec4", 4096, 4091), ("scalar", 4099, 4091))


def f32_inputs(Vp: int, V: int, kind: str = "base"):
    """The bf16 inputs of the same shape widened to fp32 plus an fp32-only perturbation, so that
    the logits are no 16-bit values."""
    inp = ce_inputs(BF, Vp if Vp % 8 == 0 else Vp + (-Vp) % 8, V, kind)
    g = torch.Generator().manual_seed(77 + Vp)
    x = inp.logits.float()[:, :Vp].contiguous()
    x = x + torch.randn(x.shape, generator=g) * 2.0 ** -12
    x[:, V:] = 40.0
    return inp._replace(logits=x.contiguous())
