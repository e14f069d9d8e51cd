"""fp64 reference and derived tolerances of the CAP forms of the cross-entropy kernels
(``ops/csrc/loss.hip``, CAP = true) and of ``k_dec_norm_head_cap``, built on tests/stream_ref.py
and tests/zloss_ref.py and shared by test_softcap_cpu.py, test_softcap_gpu.py and
softcap_ref_child.py.  Nothing here needs a GPU.

For a row with a real target, the stored 16-bit logits ``x``, ``u = x / cap``, ``t = tanh(u)``:
    c_j       = cap * t_j                       (j < V; the model's logits)
    loss_rows = lse(c) - c_target
    z_rows    = lse(c)^2
    grad_j    = (p_j * zf - [j == target]) * (1 - t_j^2) * grad_scale / max(n_valid, 1)
with p = softmax(c), zf = 1 + 2 z_loss lse(c) (1 without z-loss); zero on rows whose target is
-100 and on the padding columns.  The values come from fp64 arithmetic on ``c`` directly (the
derivative as 1 / cosh^2, which does not cancel).

What the kernel does (common.h dlt_cap_tanh), each rounding one U23 as in stream_ref.py:
    k2 = 2 log2(e) / cap                         the constant and the division: 2 roundings
    a  = exp2(-|x| k2)                           the product, then the hardware exp2 (1 ulp; results
                                                 under 2^-126 are returned as 0)
    r  = rcp(1 + a)                              the sum, the hardware reciprocal (1 ulp)
    t  = copysign((1 - a) r, x)                  the difference, the product
    1 - t^2 = 4 a r^2                            products only
The exponent of an element is fma(t, cap log2(e), -max log2(e)), cap log2(e) a rounded product.

Tolerances: named terms added to those of ``ce_ref`` / ``zce_ref`` evaluated at ``c``:
  a_rel    = U23 (1 + 6 |u|): exp2's ulp, and three roundings (k2's two, the product) of an
             exponent of size 2 |u| log2(e), which is 2 |u| in the natural logarithm
  t_err    = (1 - t^2) / 2 * a_rel     a's error through t = (1 - a) / (1 + a), dt/da = -2 / (1 + a)^2
                                       -- near zero this is U23 / 2 absolute: the cancellation in 1 - a
           + 2 EXP_FLUSH               an a under the normal range returned as zero (saturation: t = +-1)
           + 4 U23 |t|                 1 + a, rcp, 1 - a and their product
  c_err    = cap t_err + 2 U23 |c|     "the tanh term times cap", and the products with cap log2(e) /
                                       with cap (the two-pass kernel and the target form cap * t)
  lse      : sum_j p_j c_err_j         every exponent is off by its c_err; lse moves by their softmax mean
  loss     : + lse term + c_err_target + U23 |c_target|
  z_rows   : + 2 |lse| (lse term)
  zf       : + 2 z_loss (lse term)
  grad     : the base bound times (1 - t^2)                          (what made (p zf - onehot) / n wrong)
           + |p_j zf scale| (c_err_j + lse term) (1 - t^2)           (p_j through its own exponent and lse)
           + |p_j scale| 2 z_loss (lse term) (1 - t^2)               (zf through lse)
           + |grad| (a_rel + 7 U23)    "the derivative factor": a's error through 4 a / (1 + a)^2 is at most
                                       a_rel relative (the factor |t|); r twice (2 roundings each), the two
                                       products a r r, and the product that joins it to the gradient
           + 4 EXP_FLUSH |p_j zf - onehot| scale    "saturation": a flushed to zero makes the factor exactly 0
           + the final rounding to the logits' format of a value within all that.
The base bounds are evaluated at ``c`` rounded to fp32 (the references take a tensor of a format they
know); they are sums of U23-sized terms that vary smoothly with their input, so the U23 |c| by which
that input is off changes them by U23^2-sized amounts.  None of it is fitted to a kernel's output.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from tests.stream_ref import (BF, CE_BY_NAME, CE_CASES, CE_CASES_512, CE_CASES_PLAIN, CE_VARIANTS, DT_NAME, DTYPES,  # noqa: F401
                              EXP_FLUSH, F32, F64, HF, I64, U23, Checked, Guarded, bits, ce_inputs, ce_n_valid, ce_ref,
                              ce_variant, f32, final_rounding, half_ulp, round_to, sub_floor)
from tests.zloss_ref import miss, overflow_at, zce_ref  # noqa: F401

CAPS = (30.0, 15.0)      # Gemma-2's cap; and one at which the +-80 bf16 rows saturate
Z_COEFS = (0.0, 1e-2)

CAP_DEFECTS = ("no_deriv", "deriv_1_minus_t", "lse_uncapped", "target_uncapped", "cap_over_padding", "no_division",
               "z_rows_uncapped", "zf_uncapped", "ignored_row_grad", "nan_at_saturation")
# |x / cap| from which exp(2 x / cap) overflows fp32: where a formulation through that exponential gives inf / inf
SATURATION_U = 128.0 * math.log(2.0) / 2.0


class CapCE(NamedTuple):
    loss: Checked  # [M]      lse(c) - c_target
    z: Checked     # [M]      lse(c)^2
    grad: Checked  # [M, Vp]  before the rounding to the logits' format
    zf: torch.Tensor  # [M] fp64


def cap_tanh_terms(x: torch.Tensor, cap: float):
    """(c, 1 - t^2, c_err, a_rel) of the stored logits ``x`` (fp64) under the fp32 ``cap``."""
    u = x / cap
    t = torch.tanh(u)
    d = torch.cosh(u).pow(-2)  # 1 - t^2 without the cancellation; cosh overflows to inf, d to 0, where t is +-1
    a_rel = U23 * (1.0 + 6.0 * u.abs())
    t_err = 0.5 * d * a_rel + 2 * EXP_FLUSH + 4 * U23 * t.abs()
    c = cap * t
    return c, d, cap * t_err + 2 * U23 * c.abs(), a_rel


def _pre_of(chk: Checked, live: torch.Tensor, dtype) -> torch.Tensor:
    """The bound before the final rounding, taken back out of ``tol = pre + half_ulp (|ref| + pre) +
    sub_floor`` (ce_ref and zce_ref put it in that way wherever the element is live)."""
    hu, sf = half_ulp(dtype), sub_floor(dtype)
    return torch.where(live, (chk.tol - hu * chk.ref.abs() - sf) / (1.0 + hu), chk.tol).clamp(min=0.0)


def cap_ref(logits: torch.Tensor, targets: torch.Tensor, V: int, n_valid: int, grad_scale: float, cap: float,
            zc: float = 0.0, defect: Optional[str] = None, wide: bool = True) -> CapCE:
    """The CAP form at exactly the kernel's inputs (logits as stored, bf16 or fp16; cap and the z-loss
    coefficient as the fp32 the kernel receives).  Defects: see CAP_DEFECTS and test_softcap_cpu.py."""
    M, Vp = logits.shape
    dt = logits.dtype
    cap, zc = f32(cap), f32(zc)
    x = logits.double()
    real = (torch.arange(Vp) < V).unsqueeze(0)
    valid = targets != -100
    v1 = valid.unsqueeze(1)
    tgt = torch.where(valid, targets, torch.zeros_like(targets)).unsqueeze(1)
    c, d, c_err, a_rel = cap_tanh_terms(x, cap)
    ninf = torch.full_like(x, -math.inf)

    def lse_of(vals, over=real):
        return torch.logsumexp(torch.where(over, vals, ninf), dim=1, keepdim=True)

    # ---- values (with the planted defect, if any)
    cv, dv = c, d
    if defect == "no_division":
        cv = cap * torch.tanh(x)
        dv = 1.0 - torch.tanh(x) ** 2
    elif defect == "nan_at_saturation":  # tanh through exp(2u): inf / inf where that overflows fp32
        cv = torch.where(x.abs() / cap > SATURATION_U, torch.full_like(x, math.nan), c)
    elif defect == "no_deriv":
        dv = torch.ones_like(d)
    elif defect == "deriv_1_minus_t":
        dv = 1.0 - torch.tanh(x / cap)
    over = torch.ones_like(real) if defect == "cap_over_padding" else real
    lse = lse_of(x if defect == "lse_uncapped" else cv, over)
    lse_raw = lse_of(x)
    picked = (x if defect == "target_uncapped" else cv).gather(1, tgt)
    loss = torch.where(v1, lse - picked, torch.zeros_like(lse)).squeeze(1)
    zf = 1.0 + 2.0 * zc * (lse_raw if defect == "zf_uncapped" else lse)
    zl = lse_raw if defect == "z_rows_uncapped" else lse
    z = torch.where(v1, zl * zl, torch.zeros_like(lse)).squeeze(1)
    scale = grad_scale / max(n_valid, 1)
    rows_on = torch.ones_like(v1) if defect == "ignored_row_grad" else v1
    soft = torch.exp((x if defect == "lse_uncapped" else cv) - lse) * real
    onehot = torch.zeros_like(x).scatter_(1, tgt, 1.0) * v1
    grad = (soft * zf - onehot) * scale * dv * rows_on

    # ---- tolerances (of the unmodified reference)
    c32 = c.to(F32)
    if zc != 0.0:
        base = zce_ref(c32, targets, V, n_valid, grad_scale, zc, wide=wide)
        base_loss, base_z, base_grad = base.loss, base.z, base.grad
    else:
        ce = ce_ref(c32, targets, V, n_valid, grad_scale, wide=wide)
        base_loss, base_grad = ce.loss, ce.grad
        # z_rows without a coefficient (the entry point takes the array either way): zce_ref's two terms
        lse_err0 = (ce.loss.tol - U23 * ce.loss.ref.abs()).unsqueeze(1) * v1
        lse0 = lse_of(c)
        base_z = Checked(None, ((2 * lse0.abs() * lse_err0 + U23 * lse0 * lse0) * v1).squeeze(1))
    lse_t = lse_of(c)
    p = torch.exp(c - lse_t) * real
    lse_term = (p * c_err).sum(dim=1, keepdim=True)
    c_t, c_err_t = c.gather(1, tgt), c_err.gather(1, tgt)
    loss_tol = base_loss.tol + ((lse_term + c_err_t + U23 * c_t.abs()) * v1).squeeze(1)
    z_tol = base_z.tol + (2 * lse_t.abs() * lse_term * v1).squeeze(1)
    zf_t = 1.0 + 2.0 * zc * lse_t
    live = (v1 & real) & (scale != 0)
    pre_base = _pre_of(base_grad, live, F32)
    p_s = p * scale * v1
    oh = torch.zeros_like(x).scatter_(1, tgt, 1.0) * v1
    g_nod = (p * zf_t - oh) * scale * v1          # the gradient without the derivative factor
    g_true = g_nod * d
    pre = (pre_base * d
           + p_s * zf_t.abs() * (c_err + lse_term) * d
           + p_s * 2 * zc * lse_term * d
           + g_true.abs() * (a_rel + 7 * U23)
           + 4 * EXP_FLUSH * g_nod.abs())
    g_tol = pre + final_rounding(g_true, pre, dt) * live
    return CapCE(Checked(loss, loss_tol), Checked(z, z_tol), Checked(grad, g_tol), zf_t.squeeze(1))


def kernel_model(logits: torch.Tensor, targets: torch.Tensor, V: int, n_valid: int, grad_scale: float, cap: float,
                 zc: float = 0.0):
    """k_ce_row's CAP arithmetic in fp32 torch ops (an fma as the fp64 expression rounded once):
    (loss_rows, z_rows, grad rounded to the logits' format)."""
    M, Vp = logits.shape
    dt = logits.dtype
    T = lambda v: torch.tensor(v, dtype=F32)  # noqa: E731
    L2E = T(1.44269504088896340736)
    capf = T(cap)
    k2, cl = (2.0 * L2E) / capf, capf * L2E
    x = logits.float()
    real = (torch.arange(Vp) < V).unsqueeze(0)

    def tanh_parts(v):
        a = torch.exp2(-v.abs() * k2)
        r = 1.0 / (1.0 + a)
        return torch.copysign((1.0 - a) * r, v), a, r

    def fma(a_, b_, c_):
        return (a_.double() * b_.double() + c_.double()).float()

    ts, a, r = tanh_parts(x)
    gm = capf * tanh_parts(torch.where(real, x, torch.full_like(x, -math.inf)).amax(dim=1, keepdim=True))[0]
    nm2 = -gm * L2E
    sm = (torch.exp2(fma(ts, cl, nm2)) * real).sum(dim=1, keepdim=True)
    lse = gm + torch.log(sm)
    valid = (targets != -100).unsqueeze(1)
    tgt = torch.where(valid.squeeze(1), targets, torch.zeros_like(targets)).unsqueeze(1)
    inv_n = torch.where(valid, T(grad_scale) / T(float(max(n_valid, 1))), T(0.0))
    nl2 = -lse * L2E
    zf = fma(2.0 * T(zc), lse, T(1.0)) if zc != 0.0 else torch.ones_like(lse)
    gmul = torch.where(valid, inv_n * zf, T(0.0))
    pexp = torch.exp2(fma(ts, cl, nl2))
    g = pexp * (gmul * 4.0) * (a * r * r) * real
    gt = ((pexp * zf if zc != 0.0 else pexp) - 1.0) * inv_n * (4.0 * (a * r * r))
    g = torch.where((torch.arange(Vp).unsqueeze(0) == tgt) & valid, gt, g)
    loss = torch.where(valid, lse - capf * ts.gather(1, tgt), T(0.0)).squeeze(1)
    z = torch.where(valid, lse * lse, T(0.0)).squeeze(1)
    return loss, z, g.to(dt)


def cap_cases(cases=CE_CASES):
    """(name, dtype, Vp, V, kind, n_valid mode, grad_scale, cap, z_loss): every case of ``cases`` with
    every cap and with and without the z-loss."""
    return [(f"{name}-cap{cap:g}-z{zc:g}", dt, Vp, V, kind, nv_mode, g, cap, zc)
            for name, dt, Vp, V, kind, nv_mode, g in cases for cap in CAPS for zc in Z_COEFS]


CAP_CASES = cap_cases(CE_CASES)
# the children: one cap and the z-loss on (the forms differ in launch shape only)
CAP_CASES_512 = [c for c in cap_cases(CE_CASES_512) if c[7] == CAPS[0] and c[8] != 0.0]
CAP_CASES_PLAIN = [c for c in cap_cases(CE_CASES_PLAIN) if c[7] == CAPS[0] and c[8] != 0.0]
CAP_BY_NAME = {c[0]: c for c in CAP_CASES + CAP_CASES_512 + CAP_CASES_PLAIN}
assert len(CAP_BY_NAME) == len(CAP_CASES + CAP_CASES_512 + CAP_CASES_PLAIN)

# the children of test_softcap_gpu.py: the knobs (read once per process) and the cases they reach
CAP_CHILD_SETS = {
    "threads512": ({"DLT_CE_THREADS": "512", "DLT_CE_NT": "0"}, [c[0] for c in CAP_CASES_512]),
    "plain": ({"DLT_CE_NT": "0"}, [c[0] for c in CAP_CASES_PLAIN]),
}


# ------------------------------------------------------------------ dec_norm_head(..., softcap=)
DEC_CAPS = (30.0, 2.0)


def dec_head_cap_ref(chk, cap: float):
    """tests/decode_ref.norm_head_ref's Checked under the cap: cap * tanh(y / cap) of the fp64 logits.
    The map is 1-Lipschitz (its derivative 1 - t^2 is at most 1), so the kernel's rounded logit, within
    ``chk.tol`` of y, caps to within ``chk.tol`` of the reference; plus the tanh term c_err."""
    cap = f32(cap)
    c, _, c_err, _ = cap_tanh_terms(chk.ref, cap)
    return type(chk)(c, chk.tol + c_err)
