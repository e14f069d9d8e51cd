"""fp64 references, derived tolerances, fixed inputs and planted defects for attention-score
soft-capping (the CAP kernels of ``ops/csrc/attention_cap.hip`` and ``decode.hip``), shared by
test_attn_softcap_cpu.py and test_attn_softcap_gpu.py.  Nothing here needs a GPU.

The definition: x = scale q.k, s = CAP tanh(x / CAP) on real scores, masked keys at -inf, a sink
neither scaled nor capped; backward dx = dS (1 - t^2), t = tanh(x / CAP).

Tolerances are those of tests/attn_ref.py (a sum of named terms per output element, read from the
kernel code) with the score's own error replaced.  The plain kernels feed the raw MFMA product
into the exponent; the CAP kernels turn it into t first (attention.h ``cap_tanh``):

  raw       the MFMA chain over head_dim exact products: chain(hd) * sum|q||k| (as attn_ref)
  u         u = |raw| * cap_k, cap_k = 2 log2(e) scale / CAP made on the host in fp32 from fp32
            scale and CAP (two products, a quotient: 3 roundings) and one more for the product:
            4 U23 of u, plus cap_k times raw's error
  a         a = exp2(-u), the hardware exp2 ASSUMED good to one ulp (U23) of its result, as
            attn_ref assumes: relative error rel_a = U23 + ln2 * du.  (u a is bounded, so the
            absolute error da = a rel_a stays small however large the score.)  Below the
            normal range the hardware flushes to zero: an absolute EXP_FLUSH
  r         r = rcp(1 + a): the add rounds once (U23 of a value in (1, 2]), rcp ASSUMED good to
            one ulp: rel_r = 2 U23 + da / (1 + a)
  t         t = (1 - a) r: the subtraction rounds once (U23 of 1 - a) and inherits da, the
            product rounds once.  |dt| <= t (U23 + rel_r + U23) + r da <= 4 U23 t + 2 r da.
            Near x = 0 this is ABSOLUTE (a -> 1, da -> U23: dt ~ U23 whatever t), which is why
            the bound on the capped score CAP t is absolute and proportional to CAP:
            eps_s = CAP dt                                                          (``cap_terms``)
  1 - t^2   4 a r r: three products (the 4 is exact), rel_a + 2 rel_r + 3 U23   (``rel_d``)
  dS -> 16  the scaled dS (1 - t^2) is what the 16-bit rounding sees: half an ulp of it

The exponent then is exp2(fma(t, c, -m c)) with c = CAP log2(e) in place of scale log2(e): the
same three roundings of attn_ref, of |CAP t| <= CAP.  Everything downstream (l, rescales, P -> 16
bit, the chains, the final rounding, the sink epilogue of tests/sink_ref.py) is attn_ref's.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import torch

from tests import attn_ref as A
from tests.stream_ref import BF, EXP_FLUSH, F32, F64, HF, U8, U23, Checked, f32, round_to

LN2 = A.LN2
CAP_MAX = 65536.0  # ops/attn_routes.py SCORE_SOFTCAP_MAX, attention.hip ATTN_SOFTCAP_MAX
DEFECTS = ("no_cap", "cap_unscaled", "masked_at_minus_cap", "no_dt2", "one_minus_t", "sink_capped")


class Cap(NamedTuple):
    s: torch.Tensor      # capped score CAP t (natural-log units), fp64
    eps_s: torch.Tensor  # bound on the kernel's |CAP t - s|
    d: torch.Tensor      # 1 - t^2
    rel_d: torch.Tensor  # bound on the relative error of the kernel's 4 a r r


def cap_terms(x: torch.Tensor, x_err: torch.Tensor, cap: float) -> Cap:
    """``x`` = scale q.k in fp64, ``x_err`` the bound on the kernel's scale * raw (the MFMA chain),
    ``cap`` as the kernel receives it.  See the module docstring for every term."""
    t = torch.tanh(x / cap)
    u = 2.0 * x.abs() * A.LOG2E / cap
    a = torch.exp2(-u)
    r = 1.0 / (1.0 + a)
    du = 4 * U23 * u + (2.0 * A.LOG2E / cap) * x_err
    rel_a = U23 + LN2 * du
    da = a * rel_a + EXP_FLUSH
    rel_r = 2 * U23 + da * r
    dt = 4 * U23 * t.abs() + 2 * r * da
    d = 1.0 - t * t
    # 4 a r r underflows to zero with a: absolute, far below anything a 16-bit output can show
    rel_d = rel_a + 2 * rel_r + 3 * U23
    return Cap(cap * t, cap * dt, d, rel_d)


def _scores(q, k, nh, scale, cap, defect=None):
    """(x, capped s, Cap terms, sabs) of the unmodified definition, and the defective s."""
    sc, capf = f32(scale), f32(cap)
    qd, kd = q.double(), A._kv_heads(k, nh)
    raw = torch.matmul(qd, kd.transpose(-1, -2))
    x = raw * sc
    sabs = torch.matmul(qd.abs(), kd.abs().transpose(-1, -2)) * sc
    ct = cap_terms(x, A._chain(q.shape[-1]) * sabs, capf)
    if defect == "no_cap":
        s, d = x, torch.ones_like(x)
    elif defect == "cap_unscaled":  # tanh of the raw product: s = scale CAP tanh(q.k / CAP)
        tr = torch.tanh(raw / capf)
        s, d = sc * capf * tr, 1.0 - tr * tr
    else:
        s, d = ct.s, ct.d
    if defect == "no_dt2":
        d = torch.ones_like(x)
    elif defect == "one_minus_t":
        d = 1.0 - torch.tanh(x / capf)
    return x, s, d, ct, capf


# ============================================================================== forward
def cap_fwd_ref(q, k, v, scale: float, cap: float, doc=None, p: float = 0.0, key: int = 0, sink=None,
                defect: Optional[str] = None) -> A.Fwd:
    """attn_ref.attn_fwd_ref on the capped scores; ``sink`` fp32 [nh] or None (the epilogue of
    sink_ref.sink_fwd_ref).  o [B, S, nh, hd] before its rounding to 16 bits, lse [B, nh, S]."""
    B, nh, S, hd = q.shape
    dt = q.dtype
    vd = A._kv_heads(v, nh)
    lq, _ = A.live_masks(B, S, doc)
    _, s, _, ct, capf = _scores(q, k, nh, scale, cap, defect)
    hidden = torch.tensor(-capf if defect == "masked_at_minus_cap" else -math.inf, dtype=F64)
    sm = torch.where(lq, s, hidden)
    m = sm.amax(-1, keepdim=True)
    Pn = torch.exp(sm - m)
    l = Pn.sum(-1, keepdim=True)
    keep, dscale, _ = A.keep_of(B, nh, S, key, p)
    o = torch.matmul(Pn * keep, vd) * (dscale / l)
    lse = (m + torch.log(l)).squeeze(-1)

    # ---- tolerance (of the unmodified reference): attn_fwd_ref's, eps_p rebuilt
    live = ~torch.isinf(sm)
    pr = Pn / l
    w = pr * keep * dscale
    va = vd.abs()
    nt = -(-S // A.RB)
    Acap = torch.where(lq, ct.s.abs(), torch.zeros_like(s)).amax(-1, keepdim=True)  # <= CAP
    eps_p = ct.eps_s + U23 * (4 * Acap + 2)
    eps_resc = nt * U23 * (2 * Acap + 2)
    eps_l = (pr * eps_p).sum(-1, keepdim=True) + eps_resc + A._chain(32 * nt + 4)
    wv = torch.matmul(w, va)
    o_pre = torch.matmul(w * (A._hu(dt) + eps_p), va) + torch.matmul(live * keep * (A._fl(dt) * dscale) / l, va)
    o_pre = o_pre + (A._chain(S) + eps_resc + eps_l + 3 * U23) * wv
    logl = torch.log(l).abs().squeeze(-1)
    lse_tol = eps_l.squeeze(-1) + U23 * (2 * Acap.squeeze(-1) + 2 * (logl + A.RESCALE_LOG2 * LN2) + 1 + lse.abs())
    o_t, o_pre_t = o.transpose(1, 2), o_pre.transpose(1, 2)
    if sink is None:
        return A.Fwd(Checked(o_t, A._final(o_t, o_pre_t, dt)), Checked(lse, lse_tol))

    # ---- the sink epilogue: sink_ref.sink_fwd_ref on this base, |score| <= Acap
    base_o, base_o_tol = o_t, A._final(o_t, o_pre_t, dt)
    sk = sink.double().view(1, nh, 1).expand(B, nh, S)
    if defect == "sink_capped":
        sk = capf * torch.tanh(sk / capf)
    fin = torch.isfinite(sk)
    lse2 = torch.logaddexp(lse, sk)
    r = torch.exp(lse - lse2)
    rt = r.transpose(1, 2).unsqueeze(-1)
    o2 = base_o * rt
    zero = torch.zeros_like(sk)
    mk = Acap.squeeze(-1) + A.RESCALE_LOG2 * LN2
    ska = torch.where(fin, sk.abs(), zero)
    eps_exp = U23 * (mk + ska + 2 * (mk + ska) + 2)
    eps_lp = torch.where(fin, eps_exp + 2 * U23 + EXP_FLUSH * 2.0 ** A.RESCALE_LOG2, zero)
    eps_o = torch.where(fin, eps_lp + U23, zero).transpose(1, 2).unsqueeze(-1)
    o_tol = rt * base_o_tol + eps_o * (o2.abs() + rt * base_o_tol) * (1 + A._hu(dt)) + A._fl(dt) \
        + torch.where(fin, zero + EXP_FLUSH * dscale, zero).transpose(1, 2).unsqueeze(-1) * base_o.abs()
    big = torch.maximum(mk, ska)
    lse2_tol = r * lse_tol + eps_lp + U23 * (2 * big + 2 * (math.log(S + 1) + A.RESCALE_LOG2 * LN2) + 1 + lse2.abs())
    return A.Fwd(Checked(o2, o_tol), Checked(lse2, torch.where(fin, lse2_tol, lse_tol)))


# ============================================================================= backward
def cap_bwd_ref(q, k, v, o16, do16, lse32, scale: float, cap: float, doc=None, p: float = 0.0, key: int = 0,
                rope=None, defect: Optional[str] = None) -> A.Bwd:
    """attn_ref.attn_bwd_ref on the capped scores, dS carrying 1 - t^2 into dq and dk.  The stored
    lse is the capped forward's (with its sink, if any: dq / dk / dv need nothing else)."""
    B, nh, S, hd = q.shape
    nkv = k.shape[1]
    G = nh // nkv
    dt = q.dtype
    hu, fl = A._hu(dt), A._fl(dt)
    sc = f32(scale)
    qd, kd, vd = q.double(), A._kv_heads(k, nh), A._kv_heads(v, nh)
    O = o16.double().view(B, S, nh, hd).transpose(1, 2)
    dO = do16.double().view(B, S, nh, hd).transpose(1, 2)
    lse = lse32.double().unsqueeze(-1)
    lq, lk = A.live_masks(B, S, doc)
    _, s, d, ct, capf = _scores(q, k, nh, scale, cap, defect)
    P = torch.exp(s - lse)
    Pq, Pk_ = P * lq, P * lk
    if defect == "masked_at_minus_cap":  # the hidden keys keep the weight of a score of -CAP
        Ph = torch.exp(-capf - lse).expand_as(P)
        Pq, Pk_ = torch.where(lq, P, Ph), torch.where(lk, P, Ph)
    keep, dscale, ds_true = A.keep_of(B, nh, S, key, p)
    dP = torch.matmul(dO, vd.transpose(-1, -2))
    prod = dO * O
    delta = prod.sum(-1, keepdim=True)
    inner = keep * dscale * dP - delta
    dq = sc * torch.matmul(Pq * inner * d, kd)
    dk_h = sc * torch.matmul((Pk_ * inner * d).transpose(-1, -2), qd)
    dv_h = dscale * torch.matmul((Pk_ * keep).transpose(-1, -2), dO)
    grp = lambda t: t.view(B, nkv, G, S, hd).sum(2)
    dk, dv = grp(dk_h), grp(dv_h)

    # ---- tolerance (of the unmodified reference): attn_bwd_ref's, eps_p rebuilt, dS scaled
    Pq0, Pk0 = torch.exp(ct.s - lse) * lq, torch.exp(ct.s - lse) * lk
    eps_p = ct.eps_s + U23 * (ct.s.abs() + lse.abs() + (ct.s - lse).abs() + 2)
    dp_err = A._chain(hd) * torch.matmul(dO.abs(), vd.abs().transpose(-1, -2))
    delta_tol = A._chain(hd + 2) * prod.abs().sum(-1, keepdim=True)
    inner_abs = keep * ds_true * dP.abs() + delta.abs()

    def ds_err(Pm):
        dS = Pm * inner
        pre = dS.abs() * (eps_p + U23) + Pm * (keep * ds_true * dp_err + delta_tol + 3 * U23 * inner_abs)
        # times 1 - t^2 = 4 a r r: its own error and the product's rounding, then the scaled dS -> 16 bit
        dx = dS.abs() * ct.d
        pre = pre * ct.d + dx * (ct.rel_d + U23) + dS.abs() * 4 * EXP_FLUSH
        return dx, pre + hu * (dx + pre) + fl * ds_true * (Pm > 0)

    aq, eq = ds_err(Pq0)
    ak, ek = ds_err(Pk0)
    ka, qa, doa = kd.abs(), qd.abs(), dO.abs()
    dq_pre = sc * (torch.matmul(eq, ka) + (A._chain(S) + 2 * U23) * torch.matmul(aq, ka))
    dk_pre = grp(sc * (torch.matmul(ek.transpose(-1, -2), qa)
                       + (A._chain(G * S) + 2 * U23) * torch.matmul(ak.transpose(-1, -2), qa)))
    Pa = Pk0 * keep
    dv_pre = grp(ds_true * (torch.matmul((Pa * (hu + eps_p) + fl * lk * keep).transpose(-1, -2), doa)
                            + (A._chain(G * S) + 2 * U23) * torch.matmul(Pa.transpose(-1, -2), doa)))
    if rope is not None:
        dq, dq_pre = A._unrope(dq, dq_pre, rope[0], rope[1])
        dk, dk_pre = A._unrope(dk, dk_pre, rope[0], rope[1])
    mk = lambda x_, pre: Checked(x_, A._final(x_, pre, dt))
    return A.Bwd(mk(dq, dq_pre), mk(dk, dk_pre), mk(dv, dv_pre), Checked(delta.squeeze(-1), delta_tol.squeeze(-1)))


# ================================================================================ cases
class CapCase(NamedTuple):
    base: A.Case   # shape, dtype, bounds, dropout, layout (family "gauss": unit-variance scores)
    cap: float
    sink: bool     # forward only: the backward takes the forward's lse and nothing else
    sat: bool      # q, k along one dim with |x| / CAP = 128: t = +-1 and 1 - t^2 = 0 exactly

    @property
    def name(self):
        return f"{self.base.name}-cap{self.cap:g}{'-sink' if self.sink else ''}{'-sat' if self.sat else ''}"


def _cc(dt, B, nh, nkv, S, hd, bounds=(), p=0.0, packed=False, cap=2.0, sink=False, sat=False) -> CapCase:
    return CapCase(A._mk(dt, B, nh, nkv, S, hd, "gauss", bounds, p, packed), cap, sink, sat)


def _cases():
    """One family varied at a time around bf16 / B 2 / nh 4 / hd 64 / CAP 2 / no dropout /
    head-major: S (ragged last tile, the diagonal inside a tile, several key tiles), the K/V
    heads, head_dim, the dtype, dropout, the layout, the bounds, the sink, the cap."""
    out = [_cc(BF, 2, 4, 0, S, 64) for S in (65, 129, 200, 320)]
    out += [_cc(BF, 2, 4, nkv, 129, 64, p=0.1 * (nkv == 2)) for nkv in (4, 2, 1)]
    out += [_cc(BF, 2, 4, 0, 200, 128), _cc(HF, 2, 4, 2, 129, 128, p=0.1)]
    out += [_cc(HF, 2, 4, 0, 200, 64), _cc(HF, 2, 4, 0, 65, 64, p=0.1)]
    out += [_cc(BF, 2, 4, 0, 200, 64, p=0.1), _cc(BF, 2, 4, 0, 320, 128, p=0.1)]
    out += [_cc(BF, 2, 4, 0, 129, 64, packed=True), _cc(BF, 2, 4, 2, 200, 64, p=0.1, packed=True),
            _cc(HF, 2, 4, 1, 65, 128, packed=True)]
    out += [_cc(BF, 2, 4, 0, 200, 64, ("doc",)), _cc(BF, 2, 4, 2, 320, 64, ("doc",), p=0.1, packed=True),
            _cc(BF, 2, 4, 0, 200, 64, ("win", 37)), _cc(HF, 2, 4, 1, 320, 128, ("win", 65), p=0.1),
            _cc(BF, 2, 4, 0, 129, 128, ("doc",), p=0.1)]
    out += [_cc(BF, 2, 4, 0, 129, 64, sink=True), _cc(BF, 2, 4, 2, 200, 128, ("win", 37), p=0.1, sink=True),
            _cc(HF, 2, 4, 0, 65, 64, ("doc",), sink=True, packed=True)]
    out += [_cc(BF, 2, 4, 0, 200, 64, cap=50.0), _cc(HF, 2, 4, 2, 129, 128, p=0.1, cap=50.0),
            _cc(BF, 2, 4, 0, 320, 64, ("doc",), cap=50.0, packed=True)]
    out += [_cc(BF, 2, 4, 0, 129, 64, sat=True), _cc(BF, 2, 4, 2, 200, 64, p=0.1, sat=True)]
    # the largest cap the kernels take, on a window whose later rows meet dead leading tiles: the
    # forward's running max of such a row is M_DEAD = -1e30, times cap * log2(e) in the exponent
    out += [_cc(BF, 2, 4, 0, 200, 64, ("win", 37), cap=CAP_MAX), _cc(HF, 2, 4, 2, 200, 128, ("doc",), p=0.1, cap=CAP_MAX)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CASE_SINKS = torch.tensor([-3.0, 2.5, 0.0, 60.0], dtype=F32)  # one far above every capped score (|s| <= CAP)


@functools.lru_cache(maxsize=None)
def cap_inputs(c: CapCase) -> A.Inputs:
    inp = A.attn_inputs(c.base)
    if not c.sat:
        return inp
    # x = scale q0 k0 = +-(1/8) 64 32 = +-256 = 128 CAP: exp2(-u) underflows to zero in fp32, so
    # t = +-1 and 4 a r r = 0 exactly -- dq and dk are zeros; every softmax is over scores of +-CAP
    g = torch.Generator().manual_seed(c.base.key)
    q, k = torch.zeros_like(inp.q), torch.zeros_like(inp.k)
    q[..., 0] = 64.0
    k[..., 0] = (torch.randint(0, 2, k.shape[:-1], generator=g).double() * 2 - 1).to(k.dtype) * 32.0
    assert c.base.hd == 64 and c.cap == 2.0
    return inp._replace(q=q, k=k)


class Refs(NamedTuple):
    inp: A.Inputs
    sink: Optional[torch.Tensor]
    fwd: A.Fwd
    o16: torch.Tensor
    lse32: torch.Tensor
    bwd: A.Bwd


@functools.lru_cache(maxsize=None)
def case_refs(c: CapCase) -> Refs:
    """The backward's o and lse are the forward reference's, rounded to their storage formats."""
    b = c.base
    inp = cap_inputs(c)
    sink = CASE_SINKS if c.sink else None
    fwd = cap_fwd_ref(inp.q, inp.k, inp.v, inp.scale, c.cap, inp.doc, b.p, b.key, sink)
    o16 = round_to(fwd.o.ref, b.dtype).reshape(b.B * b.S, b.nh * b.hd).contiguous()
    lse32 = fwd.lse.ref.to(F32)
    bwd = cap_bwd_ref(inp.q, inp.k, inp.v, o16, inp.do, lse32, inp.scale, c.cap, inp.doc, b.p, b.key, inp.rope)
    return Refs(inp, sink, fwd, o16, lse32, bwd)


def worst(out: torch.Tensor, chk: Checked) -> float:
    """Largest |out - ref| / tol over the elements (inf where the tolerance is zero and missed)."""
    err = (out.double().reshape(chk.ref.shape) - chk.ref).abs()
    return torch.where(chk.tol > 0, err / chk.tol, torch.where(err > 0, torch.full_like(err, math.inf), err)).max().item()


# defect -> (the case of CASES that shows it, the outputs it must push outside the tolerance)
DEFECT_CASES = {
    "no_cap": (CASES[0], ("o", "lse", "dq", "dk", "dv")),
    "cap_unscaled": (CASES[0], ("o", "lse", "dq", "dk", "dv")),
    "masked_at_minus_cap": (CASES[0], ("o", "lse", "dq", "dk", "dv")),
    "no_dt2": (CASES[0], ("dq", "dk")),
    "one_minus_t": (CASES[0], ("dq", "dk")),
    "sink_capped": (next(c for c in CASES if c.sink), ("o", "lse")),
}


# =============================================================================== decode
DEC_POS = (0, 31, 32, 257)
DEC_MAXS = 320
DEC_SCALE = 0.125
DEC_SINKS = (-3.0, 2.5, 0.0, 1.5, -1.0, 4.0, 0.5, -2.0, 3.0, 1.0, -0.5, 2.0)


def dec_inputs(nh: int, nkv: int, maxS: int = DEC_MAXS):
    """(q [8, nh * 64] bf16, K cache, V cache [8, nkv, maxS, 64] bf16); unit-variance scores."""
    g = torch.Generator().manual_seed(900 + nh * 16 + nkv)
    q = torch.randn(8, nh * 64, generator=g)
    kc = torch.randn(8, nkv, maxS, 64, generator=g)
    vc = torch.randn(8, nkv, maxS, 64, generator=g)
    return q.bfloat16(), kc.bfloat16(), vc.bfloat16()


def dec_cap_ref(q, kc, vc, pos: int, scale: float, nh: int, cap: float, W: Optional[int] = None, sink=None,
                defect: Optional[str] = None) -> Checked:
    """dec_attn / dec_attn_gqa with softcap=: softmax over the keys max(0, pos - W + 1)..pos of
    CAP tanh(scale q.k / CAP) (plus the uncapped sink), times V; [B, nh, 64] before the bf16
    rounding.  The tolerance is decode_ref.attn_ref's (U8 of o for the final rounding, 1e-4 per
    probability for the fp32 softmax and sums, argued there) plus the capped score's own error:
    the fp32 score x (64 fmas: chain(64) sum|q||k| scale, and the product with scale), then
    ``cap_terms`` and the product with CAP (U23 of |s|) -- an absolute error of the exponent, so a
    relative one of the probability, taken twice (the probability's own and the normaliser's)."""
    B, nkv, maxS, hd = kc.shape
    G = nh // nkv
    capf = f32(cap)
    kf = max(0, pos + 1 - W) if W else 0
    qd = q.double().view(B, nh, hd)
    K = kc[:, :, kf:pos + 1].double().repeat_interleave(G, 1)
    V = vc[:, :, kf:pos + 1].double().repeat_interleave(G, 1)
    x = torch.einsum("bhd,bhjd->bhj", qd, K) * scale
    xabs = torch.einsum("bhd,bhjd->bhj", qd.abs(), K.abs()) * scale
    ct = cap_terms(x, (A._chain(hd) + U23) * xabs, capf)
    s = x if defect == "no_cap" else ct.s
    eps_s = ct.eps_s + U23 * ct.s.abs()
    if sink is not None:
        sk = sink.double().view(1, nh, 1).expand(B, nh, 1)
        if defect == "sink_capped":
            sk = capf * torch.tanh(sk / capf)
        pr = torch.softmax(torch.cat([s, sk], -1), -1)[..., :-1]
    else:
        pr = torch.softmax(s, -1)
    o = torch.einsum("bhj,bhjd->bhd", pr, V)
    tol = U8 * o.abs() + torch.einsum("bhj,bhjd->bhd", pr * (1e-4 + 2 * eps_s), V.abs())
    return Checked(o, tol)
