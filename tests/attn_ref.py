"""fp64 references, derived tolerances, fixed inputs, planted defects and a model of the
launchers' dispatch for the flash-attention kernels (``ops/csrc/attention.hip``), shared by
test_attn_kernels_cpu.py, test_attn_kernels_gpu.py and attn_ref_child.py.  Nothing here needs a
GPU.  The shared pieces (Checked, Guarded, final_rounding, ...) are those of tests/stream_ref.py.

References.  Each takes exactly what the kernel takes (q / k / v / dO / o as stored in 16 bits,
lse as stored in fp32, the keep bits of ops/rng.py), computes in fp64 and returns every output
BEFORE its final rounding.  ``defect=`` plants one of DEFECTS; the CPU file shows that each of
them falls outside the tolerance at the case the GPU file runs.

Tolerances: a sum of named terms per output element, read from the kernel code.
  products      16-bit x 16-bit is exact in fp32 (8 + 8 or 11 + 11 significant bits)
  chains        an MFMA chain over n terms: n fp32 roundings of partial sums that the sum of
                absolute terms bounds, U23 each (``chain``)
  exponent      p = exp2(fma(s, c, -m c)): c = scale * log2(e), the product -m c (or -lse
                log2(e)) and the fma round once each, half a U23 of |s|, |m| and |s - m|; charged a
                whole U23 each, which also pays for the fp32 rounding of c itself.  The hardware
                exp2 / log2 are ASSUMED good to one ulp (U23) of their result (``eps_p``)
  P -> 16 bit   acc_frag<HK> converts with __builtin_convertvector: round to nearest even, so
                half an ulp (U8 / U10 / 2) of P; fp16 adds half a subnormal step (2^-25) of the
                kernel's own P, which the deferred rescale keeps in [P_true, 2^8 P_true]
  l             summed from the unrounded fp32 p: one U23 per key of a lane, per tile (``eps_l``)
  rescales      alpha = exp2((m_old - m_new) c) and one product, per tile at the most (``eps_resc``)
  final         stream_ref.final_rounding(): one round-to-nearest of the kernel's own value
The backward adds the 16-bit rounding of dS (dQ: of dS, dK: of dS / s with s = 1 / (1 - p) folded
into the epilogue), the fp32 delta and the rotation of the packed store; see attn_bwd_ref.
``bias_ratio`` looks at the sign of the errors, which no element-wise bound can.
"""
from __future__ import annotations

import functools
import math
import zlib
from typing import NamedTuple, Optional

import torch

from distributed_llm_trainer_amd.ops import reference as opsref
from distributed_llm_trainer_amd.ops import rng
from tests.stream_ref import (BF, DT_NAME, F32, F64, HF, U8, U10, U23, Checked, Guarded, bits, f32, final_rounding,
                              half_ulp, round_to, sub_floor)

__all__ = ["Checked", "Guarded", "bits", "round_to", "U8", "U10"]  # re-exported for the test files

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
RB = 64             # rows per work item, keys per staged tile (attention.hip RB, KVB, QSTEP)
RESCALE_LOG2 = 8.0  # attention.hip: the running max moves only when a row's grew by more than 2^8


# ================================================================================ masks
def live_masks(B: int, S: int, doc=None):
    """(live_q, live_k), bool [B, 1, S, S] indexed [b, 0, query, key]: what the kernels whose
    lanes are queries (forward, dQ: lo[q] <= k <= q) and keys (dK/dV: k <= q <= hi[k]) see.
    The two are equal for consistent bounds."""
    qi = torch.arange(S).view(1, 1, S, 1)
    ki = torch.arange(S).view(1, 1, 1, S)
    causal = (ki <= qi).expand(B, 1, S, S)
    if doc is None:
        return causal.clone(), causal.clone()
    lo, hi = doc
    return causal & (ki >= lo.view(B, 1, S, 1).long()), causal & (qi <= hi.view(B, 1, 1, S).long())


DEFECTS = ("drop_diag", "see_next", "drop_last_key", "drop_lo", "drop_hi", "skip_half_tile", "l_not_rescaled",
           "no_threshold", "no_dropout_scale", "keep_transposed", "kv_mod", "delta_3q", "rope_fwd_sign",
           "gqa_drop_head", "p_trunc", "drop_one")


def _defect_masks(defect, at, lq, lk, S, doc):
    """The live masks as a kernel with ``defect`` sees them.  Rows keep at least one key."""
    lq, lk = lq.clone(), lk.clone()
    idx = torch.arange(S)
    many = lq.sum(-1, keepdim=True) >= 2  # rows that stay non-empty after losing a key
    if defect == "drop_diag":  # ">=" for ">" on the diagonal
        d = torch.eye(S, dtype=torch.bool).view(1, 1, S, S) & many
        lq, lk = lq & ~d, lk & ~d
    elif defect == "see_next":  # the diagonal test one key late: key q + 1 leaks
        d = torch.zeros(S, S, dtype=torch.bool)
        d[idx[:-1], idx[1:]] = True
        lq, lk = lq | d, lk | d
    elif defect == "drop_last_key":  # "ka >= S - 1" for "ka >= S": the last key of a ragged S
        lq[..., S - 1], lk[..., S - 1] = False, False
        lq[..., S - 1, S - 1] = lq[..., S - 1, :S - 1].sum(-1) == 0  # a row of its own keeps it
        lk[..., S - 1, S - 1] = lq[..., S - 1, S - 1]
    elif defect == "drop_lo":  # "ka <= lo" for "ka < lo": the first key of a document or window
        lo = doc[0].long()
        d = (idx.view(1, 1, 1, S) == lo.view(-1, 1, S, 1)) & many
        lq, lk = lq & ~d, lk & ~d
    elif defect == "drop_hi":  # dK/dV alone: "qa >= hi" for "qa > hi": the last query of a key
        hi = doc[1].long()
        d = (idx.view(1, 1, S, 1) == hi.view(-1, 1, 1, S)) & (idx.view(1, 1, 1, S) != idx.view(1, 1, S, 1))
        lk = lk & ~d
    elif defect == "skip_half_tile":  # keys 32 .. 63 of the first tile of a row with keys before them
        d = torch.zeros(S, S, dtype=torch.bool)
        d[:, 32:64] = True
        d = d.view(1, 1, S, S) & (lq[..., :32].sum(-1, keepdim=True) > 0)
        lq, lk = lq & ~d, lk & ~d
    elif defect == "drop_one":  # one (query, key) pair
        lq[..., at[0], at[1]], lk[..., at[0], at[1]] = False, False
    return lq, lk


def _kv_heads(t: torch.Tensor, nh: int, defect=None) -> torch.Tensor:
    """k or v [B, nkv, S, hd] as each query head reads it: kv head h // G (defect kv_mod: h % nkv)."""
    nkv = t.shape[1]
    G = nh // nkv
    h = torch.arange(nh)
    return t.double()[:, (h % nkv) if defect == "kv_mod" else (h // G)]


def keep_of(B, nh, S, key, p, defect=None):
    """(keep [B, nh, S, S] as 0 / 1 fp64, the scale 1 / (1 - p) as the kernel receives it)."""
    if not rng.keep_threshold(p):
        return torch.ones(1, 1, 1, 1, dtype=F64), 1.0, 1.0
    keep = rng.attn_keep_mask(B * nh, S, S, key, p).view(B, nh, S, S)
    if defect == "keep_transposed":
        keep = keep.transpose(-1, -2)
    ds = f32(1.0 / (1.0 - p))
    return keep.double(), (1.0 if defect == "no_dropout_scale" else ds), ds


def running_max(s: torch.Tensor, c_log2: float, threshold: bool = True):
    """The running maximum each row uses in each 64-key tile under the deferred rescale (fwd_tile):
    [.., S, ntiles], -inf before a row's first live tile.  A wave (32 queries) rescales all its
    rows when one of them grew by more than 2^8.  ``s`` holds -inf where masked; ``c_log2`` turns
    its units into log2 units."""
    S = s.shape[-1]
    nt = -(-S // RB)
    m = torch.full(s.shape[:-1], -math.inf, dtype=s.dtype)
    out = []
    for t in range(nt):
        mx = s[..., t * RB:(t + 1) * RB].amax(-1)
        grew = ((mx - m) * c_log2 > RESCALE_LOG2) | (torch.isinf(m) & ~torch.isinf(mx))
        if not threshold:
            grew = torch.isinf(m) & ~torch.isinf(mx)  # the first live tile only
        pad = (-S) % 32
        wave = torch.nn.functional.pad(grew, (0, pad)).unflatten(-1, (-1, 32)).any(-1, keepdim=True)
        wave = wave.expand(*wave.shape[:-1], 32).flatten(-2)[..., :S]
        m = torch.where(wave, torch.maximum(m, mx), m)
        out.append(m)
    return torch.stack(out, -1)


def _chain(n: int) -> float:
    return n * U23


def _hu(dt) -> float:
    return half_ulp(dt) if dt in (BF, HF) else 0.0  # fp64 in, fp64 out: the references' own check


def _fl(dt) -> float:
    return sub_floor(dt) if dt in (BF, HF) else 0.0


def _final(x, pre, dt):
    return pre + (final_rounding(x, pre, dt) if dt in (BF, HF) else 0.0)


# ============================================================================== forward
class Fwd(NamedTuple):
    o: Checked    # [B, S, nh, hd] (= the kernel's [B*S, nh*hd]), before the rounding to 16 bits
    lse: Checked  # [B, nh, S]


def attn_fwd_ref(q, k, v, scale: float, doc=None, p: float = 0.0, key: int = 0, defect: Optional[str] = None,
                 at=None) -> Fwd:
    """q [B, nh, S, hd], k / v [B, nkv, S, hd] 16-bit; doc = (lo, hi) int32 [B, S] or None.
    o = sum_k keep softmax(scale q.k)[k] v[k] / (1 - p), lse = logsumexp over the live keys."""
    B, nh, S, hd = q.shape
    dt = q.dtype
    sc = f32(scale)
    qd, kd, vd = q.double(), _kv_heads(k, nh, defect), _kv_heads(v, nh, defect)
    lq0, _ = live_masks(B, S, doc)
    lq, _ = _defect_masks(defect, at, lq0, lq0, S, doc)
    ninf = torch.tensor(-math.inf, dtype=F64)
    s = torch.matmul(qd, kd.transpose(-1, -2)) * sc
    sm = torch.where(lq, s, ninf)
    m = sm.amax(-1, keepdim=True)
    Pn = torch.exp(sm - m)
    l = Pn.sum(-1, keepdim=True)
    if defect == "l_not_rescaled":  # each tile's p summed as it was, relative to the max of its time
        mt = running_max(sm, LOG2E).repeat_interleave(RB, -1)[..., :S]
        l = torch.where(lq, torch.exp(sm - mt) * torch.exp(mt[..., -1:] - m), torch.zeros_like(s)).sum(-1, keepdim=True)
    keep, dscale, _ = keep_of(B, nh, S, key, p, defect)
    Pk = Pn * keep
    if defect == "p_trunc":  # P cut to the 16-bit format instead of rounded
        step = torch.exp2(torch.floor(torch.log2(Pk.clamp_min(1e-300))) - (7 if dt == BF else 10))
        Pk = torch.floor(Pk / step) * step
    if defect == "no_threshold":  # the max of the first live tile kept for good: P overflows fp16
        m0 = running_max(sm, LOG2E, threshold=False)[..., -1:]
        over = torch.exp(sm - m0) * lq > (65504.0 if dt == HF else 3.38e38)
        Pk = torch.where(over, torch.tensor(math.inf, dtype=F64), Pk)
    o = torch.matmul(Pk, vd) * (dscale / l)
    lse = (m + torch.log(l)).squeeze(-1)

    # ---- tolerance (of the unmodified reference)
    pr = Pn / l
    w = pr * keep * dscale
    va = vd.abs()
    nt = -(-S // RB)
    A = torch.where(lq, s.abs(), torch.zeros_like(s)).amax(-1, keepdim=True)  # largest live |score|
    sabs = torch.matmul(qd.abs(), kd.abs().transpose(-1, -2)) * sc
    # exponent: the score's own chain, then |s|, |m| <= A and |s - m| <= 2A, one exp2
    eps_p = _chain(hd) * sabs + U23 * (4 * A + 2)
    # a rescale per tile at the most: the exponent (m_old, m_new <= A), exp2, the product
    eps_resc = nt * U23 * (2 * A + 2)
    # l: every p's error weighted by its share, one add per key of a lane (16 per 32-key half),
    # the two partial sums, the two lane halves
    eps_l = (pr * eps_p).sum(-1, keepdim=True) + eps_resc + _chain(32 * nt + 4)
    wv = torch.matmul(w, va)
    # P -> 16 bit (half an ulp, round to nearest), p's own error, the subnormal floor of the
    # kernel's P (>= the true one) over an l that is >= the true one
    o_pre = torch.matmul(w * (_hu(dt) + eps_p), va) + torch.matmul(lq * keep * (_fl(dt) * dscale) / l, va)
    # the P.V chain over the keys, O's rescales, l, then 1 / l (a division and dscale) and the product
    o_pre = o_pre + (_chain(S) + eps_resc + eps_l + 3 * U23) * wv
    o_t, o_pre_t = o.transpose(1, 2), o_pre.transpose(1, 2)
    # lse = m_k scale + log(l_k): m_k scale through c / log2(e) (three roundings of <= A); the
    # hardware log2 (1 ulp) times ln 2 of |log l_k| <= |log l| + 8 ln 2, U23 absolute near zero;
    # l's own error; the add
    logl = torch.log(l).abs().squeeze(-1)
    lse_tol = (eps_l.squeeze(-1) + U23 * (2 * A.squeeze(-1) + 2 * (logl + RESCALE_LOG2 * LN2) + 1 + lse.abs()))
    return Fwd(Checked(o_t, _final(o_t, o_pre_t, dt)), Checked(lse, lse_tol))


# ============================================================================= backward
class Bwd(NamedTuple):
    dq: Checked     # [B, nh, S, hd]
    dk: Checked     # [B, nkv, S, hd]
    dv: Checked     # [B, nkv, S, hd]
    delta: Checked  # [B, nh, S] fp32 workspace


def _unrope(x, pre, cos, sin, fwd_sign=False):
    """The inverse NeoX rotation of store_head_row on (value, error bound) [.., S, hd]:
    x1' = x1 c + x2 s, x2' = x2 c - x1 s, each an fma of a rounded product."""
    S, hd = x.shape[-2:]
    c, s = cos[:S].double(), sin[:S].double()
    if fwd_sign:
        s = -s
    x1, x2, p1, p2 = x[..., :hd // 2], x[..., hd // 2:], pre[..., :hd // 2], pre[..., hd // 2:]
    y = torch.cat([x1 * c + x2 * s, x2 * c - x1 * s], -1)
    mag = (x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()
    ca, sa = c.abs(), s.abs()
    e = torch.cat([p1 * ca + p2 * sa + 2 * U23 * mag[0], p2 * ca + p1 * sa + 2 * U23 * mag[1]], -1)
    return y, e


def attn_bwd_ref(q, k, v, o16, do16, lse32, scale: float, doc=None, p: float = 0.0, key: int = 0, rope=None,
                 defect: Optional[str] = None, at=None) -> Bwd:
    """dq, dk, dv of the forward from the stored o / lse and dO [B*S, nh*hd]; with rope = (cos, sin)
    [>= S, hd/2] the inverse rotation is applied to dq and dk as the packed store does.
    delta = rowsum(dO * o) from the stored 16-bit o."""
    B, nh, S, hd = q.shape
    nkv = k.shape[1]
    G = nh // nkv
    dt = q.dtype
    hu, fl = _hu(dt), _fl(dt)
    sc = f32(scale)
    qd, kd, vd = q.double(), _kv_heads(k, nh, defect), _kv_heads(v, nh, defect)
    O = o16.double().view(B, S, nh, hd).transpose(1, 2)
    dO = do16.double().view(B, S, nh, hd).transpose(1, 2)
    lse = lse32.double().unsqueeze(-1)
    lq0, lk0 = live_masks(B, S, doc)
    lq, lk = _defect_masks(defect, at, lq0, lk0, S, doc)
    s = torch.matmul(qd, kd.transpose(-1, -2)) * sc
    P = torch.exp(s - lse)
    keep, dscale, ds_true = keep_of(B, nh, S, key, p, defect)
    dP = torch.matmul(dO, vd.transpose(-1, -2))
    prod = dO * O
    nd = hd * 3 // 4 if defect == "delta_3q" else hd
    delta = prod[..., :nd].sum(-1, keepdim=True)
    inner = keep * dscale * dP - delta
    dSq, dSk = P * lq * inner, P * lk * inner
    Pdk = P * lk * keep
    dq = sc * torch.matmul(dSq, kd)
    dk_h = sc * torch.matmul(dSk.transpose(-1, -2), qd)
    dv_h = dscale * torch.matmul(Pdk.transpose(-1, -2), dO)
    heads = G - 1 if (defect == "gqa_drop_head" and G > 1) else G
    grp = lambda t: t.view(B, nkv, G, S, hd)[:, :, :heads].sum(2)
    dk, dv = grp(dk_h), grp(dv_h)

    # ---- tolerance (of the unmodified reference: the clean masks)
    Pq, Pk_ = P * lq0, P * lk0
    sabs = torch.matmul(qd.abs(), kd.abs().transpose(-1, -2)) * sc
    # exponent: the score's chain; s c, -lse log2(e) and the fma round once each; one exp2
    eps_p = _chain(hd) * sabs + U23 * (s.abs() + lse.abs() + (s - lse).abs() + 2)
    dp_err = _chain(hd) * torch.matmul(dO.abs(), vd.abs().transpose(-1, -2))
    # delta: hd exact products added in fp32, the two lane halves; dK/dV reads it back times the
    # rounded 1 / dscale (charged with the three roundings of the bracket below)
    delta_tol = _chain(hd + 2) * prod.abs().sum(-1, keepdim=True)
    inner_abs = keep * ds_true * dP.abs() + delta.abs()

    def ds_err(Pm):
        dS = Pm * inner
        # p's error and the product; dP's chain and delta's; the bracket's roundings (dscale folded
        # by an fma in dQ, p * delta / s and an fma in dK/dV)
        pre = dS.abs() * (eps_p + U23) + Pm * (keep * ds_true * dp_err + delta_tol + 3 * U23 * inner_abs)
        # dS -> 16 bit, round to nearest; fp16: half a subnormal step of dS (dQ) or dS / s (dK/dV)
        return dS.abs(), pre + hu * (dS.abs() + pre) + fl * ds_true * (Pm > 0)

    aq, eq = ds_err(Pq)
    ak, ek = ds_err(Pk_)
    ka, qa, doa = kd.abs(), qd.abs(), dO.abs()
    # dq: the rounded dS times k over the row's keys (a chain of S at the most), the product with scale
    dq_pre = sc * (torch.matmul(eq, ka) + (_chain(S) + 2 * U23) * torch.matmul(aq, ka))
    dk_pre = grp(sc * (torch.matmul(ek.transpose(-1, -2), qa)
                       + (_chain(G * S) + 2 * U23) * torch.matmul(ak.transpose(-1, -2), qa)))
    Pa = Pk_ * keep
    # dv: P -> 16 bit (round to nearest, the fp16 floor where a key is kept), p's error, the chain
    # over the queries of every head of the group, the product with dscale
    dv_pre = grp(ds_true * (torch.matmul((Pa * (hu + eps_p) + fl * lk0 * keep).transpose(-1, -2), doa)
                            + (_chain(G * S) + 2 * U23) * torch.matmul(Pa.transpose(-1, -2), doa)))
    if rope is not None:
        dq, dq_pre = _unrope(dq, dq_pre, rope[0], rope[1], defect == "rope_fwd_sign")
        dk, dk_pre = _unrope(dk, dk_pre, rope[0], rope[1], defect == "rope_fwd_sign")
    mk = lambda x, pre: Checked(x, _final(x, pre, dt))
    return Bwd(mk(dq, dq_pre), mk(dk, dk_pre), mk(dv, dv_pre), Checked(delta.squeeze(-1), delta_tol.squeeze(-1)))


def bias_ratio(out: torch.Tensor, chk: Checked) -> float:
    """Round-to-nearest errors have no preferred sign; a kernel that truncates (P, dS or an output)
    errs towards zero in every element.  Returns |sum_i (out_i - ref_i) sign(ref_i)| over
    6 sqrt(sum_i tol_i^2): for independent errors bounded by tol_i, Hoeffding's inequality puts
    a value above 1 at a probability under 2 exp(-18) = 3e-8, whatever their distribution; the
    fp32-level terms that a row's elements share are 2^-15 of the tolerance."""
    d = (out.double().reshape(chk.ref.shape) - chk.ref) * torch.sign(chk.ref)
    return (d.sum().abs() / (6.0 * chk.tol.pow(2).sum().sqrt()).clamp_min(1e-300)).item()


# ============================================================== emulation of the kernels
def attn_fwd_emul(q, k, v, scale, doc=None, p=0.0, key=0):
    """The forward's arithmetic in fp32 torch: 64-key tiles, the deferred rescale per 32-query wave,
    exp2 of an fma, l from the unrounded p, P rounded to the 16-bit format, O in fp32.
    Returns (o [B, S, nh, hd] 16-bit, lse fp32)."""
    B, nh, S, hd = q.shape
    dt = q.dtype
    c = torch.tensor(f32(scale), dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    G = nh // k.shape[1]
    kf, vf = (t.float().repeat_interleave(G, 1) for t in (k, v))
    lq, _ = live_masks(B, S, doc)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)).masked_fill(~lq, -math.inf)
    keep, dscale, _ = keep_of(B, nh, S, key, p)
    keep = keep.float().expand(B, nh, S, S)
    mt = running_max(s.double() * f32(scale), float(c) / f32(scale)).float() / f32(scale)  # raw-score units
    m = torch.full((B, nh, S), -1e30, dtype=F32)
    l = torch.zeros(B, nh, S, dtype=F32)
    O = torch.zeros(B, nh, S, hd, dtype=F32)
    for t in range(mt.shape[-1]):
        m_new = torch.where(torch.isinf(mt[..., t]), m, mt[..., t])
        alpha = torch.exp2((m - m_new) * c)
        m, l, O = m_new, l * alpha, O * alpha.unsqueeze(-1)
        sl = slice(t * RB, min(S, (t + 1) * RB))
        pt = torch.exp2(torch.addcmul((-m * c).unsqueeze(-1), s[..., sl], c))
        l = l + pt.sum(-1)
        O = O + torch.matmul((pt * keep[..., sl]).to(dt).float(), vf[..., sl, :])
    inv = torch.tensor(dscale, dtype=F32) / l
    o = (O * inv.unsqueeze(-1)).to(dt).transpose(1, 2)
    lse = m * (c / torch.tensor(LOG2E, dtype=F32)) + torch.log(l)
    return o, lse


def attn_bwd_emul(q, k, v, o16, do16, lse32, scale, doc=None, p=0.0, key=0, rope=None):
    """The backward's arithmetic in fp32: P and dS rounded to the 16-bit format before their
    products (dK from dS / s as the kernel, dscale in the epilogue), fp32 delta, the rotation in
    the store.  Returns 16-bit (dq, dk, dv) and fp32 delta."""
    B, nh, S, hd = q.shape
    nkv = k.shape[1]
    G = nh // nkv
    dt = q.dtype
    sc = torch.tensor(f32(scale), dtype=F32)
    c = sc * torch.tensor(LOG2E, dtype=F32)
    qf = q.float()
    kf, vf = (t.float().repeat_interleave(G, 1) for t in (k, v))
    O = o16.float().view(B, S, nh, hd).transpose(1, 2)
    dO = do16.float().view(B, S, nh, hd).transpose(1, 2)
    lq, lk = live_masks(B, S, doc)
    keep, dscale, _ = keep_of(B, nh, S, key, p)
    keep, dsc = keep.float(), torch.tensor(dscale, dtype=F32)
    s = torch.matmul(qf, kf.transpose(-1, -2))
    P = torch.exp2(torch.addcmul((-lse32 * torch.tensor(LOG2E, dtype=F32)).unsqueeze(-1), s, c))
    dP = torch.matmul(dO, vf.transpose(-1, -2))
    delta = (dO * O).sum(-1, keepdim=True)
    dSq = (P * lq) * (keep * dP * dsc - delta)
    dq = torch.matmul(dSq.to(dt).float(), kf) * sc
    Pk = P * lk
    dSk = (Pk * keep) * dP - Pk * (delta * (1.0 / dsc))  # dS / s
    grp = lambda t: t.view(B, nkv, G, S, hd).sum(2)
    dk = grp(torch.matmul(dSk.to(dt).float().transpose(-1, -2), qf)) * (sc * dsc)
    dv = grp(torch.matmul((Pk * keep).to(dt).float().transpose(-1, -2), dO)) * dsc
    if rope is not None:
        cs, sn = rope[0][:S].float(), rope[1][:S].float()
        rot = lambda x: torch.cat([x[..., :hd // 2] * cs + x[..., hd // 2:] * sn,
                                   x[..., hd // 2:] * cs - x[..., :hd // 2] * sn], -1)
        dq, dk = rot(dq), rot(dk)
    return dq.to(dt), dk.to(dt), dv.to(dt), delta.squeeze(-1)


# ================================================================================ inputs
class Case(NamedTuple):
    name: str
    dtype: torch.dtype
    B: int
    nh: int
    nkv: int        # 0: the MHA kernels; > 0: the GQA kernels with that many K/V heads
    S: int
    hd: int
    family: str     # gauss | flat | steep_under | steep_over | big
    bounds: tuple   # () | ("doc",) | ("doc", step) | ("win", W) | ("docwin", W): see doc_seps
    p: float
    packed: bool    # the packed QKV layout, whose backward applies the inverse RoPE

    @property
    def kvh(self):
        return self.nkv or self.nh

    @property
    def key(self):
        return zlib.crc32(self.name.encode()) & 0x7FFFFFFF


def doc_seps(S: int, step: int = 0):
    """Separator positions: documents that start and end inside 64-key tiles, a one-token
    document, and a late document whose rows leave whole leading tiles of their wave dead.
    ``step`` > 0: a separator every ``step`` tokens instead (rows of at most ``step`` keys);
    ``step`` < 0: a short, a long and a short document."""
    if step > 0:
        return list(range(step - 1, S - 1, step))
    if step < 0:  # one long document: tiles of its later items lie above every row's bound
        return [S // 16, (S * 29) // 32]
    c = {S // 16, S // 7 + 1, (S * 15) // 32, (S * 15) // 32 + 1, (S * 29) // 32}
    return sorted(x for x in c if 0 <= x < S - 1)


def case_bounds(c: Case):
    """doc = (lo, hi) int32 [B, S] of the case, or None.  Batch b > 0 shifts the separators by b."""
    if not c.bounds:
        return None
    kind = c.bounds[0]
    doc = None
    if kind in ("doc", "docwin"):
        ids = torch.zeros(c.B, c.S, dtype=torch.int64)
        step = c.bounds[1] if kind == "doc" and len(c.bounds) > 1 else 0
        for b in range(c.B):
            for x in doc_seps(c.S, step):
                ids[b, min(x + b, c.S - 1)] = 1
        doc = opsref.doc_bounds(ids, 1)
    if kind in ("win", "docwin"):
        doc = tuple(opsref.window_bounds(c.B, c.S, c.bounds[1], "cpu", doc=doc))
    return tuple(doc)


class Inputs(NamedTuple):
    q: torch.Tensor    # [B, nh, S, hd]
    k: torch.Tensor    # [B, kvh, S, hd]
    v: torch.Tensor
    do: torch.Tensor   # [B*S, nh*hd]
    doc: Optional[tuple]
    scale: float
    rope: Optional[tuple]  # (cos, sin) fp32 [S, hd/2] for the packed backward


def _signs(g, shape):
    return torch.randint(0, 2, shape, generator=g).double() * 2 - 1


@functools.lru_cache(maxsize=None)
def attn_inputs(c: Case) -> Inputs:
    """gauss: randn.  flat: q lives on the even head dims and k on the odd ones, so that every
    score is exactly zero and each live key weighs 1/n while dq and dk stay non-zero; q, k, v and
    dO are random signs times 1 + position/256 (exact in bf16).  steep_*: the score rises by a
    fixed step per key (k holds the key's tile and offset as small integers, q the step), so the
    running max grows by 7.8 (under the rescale threshold: P reaches 2^7.8) or 8.2 (over it: a
    rescale in every tile) log2 units per 64-key tile.  big: randn scaled so that |score * scale|
    reaches about 60."""
    g = torch.Generator().manual_seed(c.key)
    B, nh, kvh, S, hd = c.B, c.nh, c.kvh, c.S, c.hd
    scale = 1.0 / math.sqrt(hd)
    rn = lambda *sh: torch.randn(*sh, generator=g, dtype=F64)
    pos = (1.0 + torch.arange(S, dtype=F64) / 256.0).view(1, 1, S, 1)
    if c.family == "flat":
        even = (torch.arange(hd) % 2 == 0).double()
        q = _signs(g, (B, nh, S, hd)) * pos * even
        k = _signs(g, (B, kvh, S, hd)) * pos * (1 - even)
        v = _signs(g, (B, kvh, S, hd)) * pos
        do = _signs(g, (B, nh, S, hd)) * pos
    else:
        amp = 3.75 if c.family == "big" else 1.0
        q, k, v, do = rn(B, nh, S, hd) * amp, rn(B, kvh, S, hd) * amp, rn(B, kvh, S, hd), rn(B, nh, S, hd)
        if c.family.startswith("steep"):
            step = (7.8 if c.family == "steep_under" else 8.2) / RB / (scale * LOG2E)  # raw score per key
            q, k = q * 0.1, k * 0.1
            q[..., 0], q[..., 1] = step, step
            j = torch.arange(S, dtype=F64)
            k[..., 0], k[..., 1] = (j // RB) * RB, j % RB
    q, k, v = q.to(F32).to(c.dtype), k.to(F32).to(c.dtype), v.to(F32).to(c.dtype)
    do = do.transpose(1, 2).reshape(B * S, nh * hd).to(F32).to(c.dtype)
    rope = opsref.rope_tables(hd, S) if c.packed else None
    return Inputs(q, k, v, do, case_bounds(c), scale, rope)


def pack_qkv(inp: Inputs) -> torch.Tensor:
    """q | k | v as the packed [B*S, (nh + 2 kvh) hd] rows the packed wrappers read."""
    B, _, S, _ = inp.q.shape
    return torch.cat([t.transpose(1, 2).reshape(B * S, -1) for t in (inp.q, inp.k, inp.v)], 1).contiguous()


@functools.lru_cache(maxsize=None)
def case_refs(c: Case):
    """(inputs, forward reference, the stored o / lse the backward is given, backward reference).
    The backward's o and lse are the forward reference's, rounded to their storage formats."""
    inp = attn_inputs(c)
    fwd = attn_fwd_ref(inp.q, inp.k, inp.v, inp.scale, inp.doc, c.p, c.key)
    o16 = round_to(fwd.o.ref, c.dtype).reshape(c.B * c.S, c.nh * c.hd).contiguous()
    lse32 = fwd.lse.ref.to(F32)
    bwd = attn_bwd_ref(inp.q, inp.k, inp.v, o16, inp.do, lse32, inp.scale, inp.doc, c.p, c.key, inp.rope)
    return inp, fwd, o16, lse32, bwd


# ======================================================================= dispatch model
SCHEDS = ("lpt", "pair-xcd", "pair-natural")


def sched_of(env) -> str:
    """xcd_map_enabled() of attention.hip: DLT_ATTN_SCHED starting with 'p' selects the paired
    items, and only then does DLT_ATTN_XCD (atoi == 0) choose the natural order."""
    if not env.get("DLT_ATTN_SCHED", "").startswith("p"):
        return "lpt"
    x = env.get("DLT_ATTN_XCD")
    if x is None:
        return "pair-xcd"
    digits = x.strip()
    num = ""
    for i, ch in enumerate(digits):
        if ch.isdigit() or (i == 0 and ch in "+-"):
            num += ch
        else:
            break
    val = int(num) if num.strip("+-") else 0
    return "pair-natural" if val == 0 else "pair-xcd"


def _b(x) -> str:
    return "1" if x else "0"


def fwd_variants(drop, hk, hd, doc, gqa, gen_mask=True):
    out = [f"k_attn_fwd<DROP={_b(drop)},HK={hk},D={hd},DOC={_b(doc)},GQA={_b(gqa)}>"]
    return out + (["k_dropout_bits<BAND=0>"] if drop and gen_mask else [])


def bwd_variants(drop, hk, hd, doc, gqa, rope):
    dkdv = "k_attn_bwd_dkdv_gqa" if gqa else "k_attn_bwd_dkdv"
    return [f"k_attn_bwd_dq<DROP={_b(drop)},HK={hk},D={hd},DOC={_b(doc)},GQA={_b(gqa)}>",
            f"{dkdv}<DROP={_b(drop)},HK={hk},D={hd},DOC={_b(doc)}>",
            "bwd-store:rope" if rope else "bwd-store:plain"]


def mask_variant(S: int, window=None) -> str:
    """dlt_attn_dropout_mask / _band: a band that covers the causal triangle takes the full kernel
    (the ops/hip.py wrapper calls the band entry point only for window < S)."""
    W = (S + 31) // 32
    fast = "S%32==0" if S % 32 == 0 else "S%32!=0"
    if window is None or window >= S:
        return f"k_dropout_bits<BAND=0> {fast}"
    D = min((window - 1 + 63) // 64, W)
    return f"k_dropout_bits<BAND={_b(2 * D + 2 < W + 1)}> {fast}"


def case_window(c: Case):
    return c.bounds[1] if c.bounds and c.bounds[0] in ("win", "docwin") else None


def case_variants(c: Case):
    """Every instantiation one forward + backward of the case launches through ops/hip.py."""
    hk, doc, gqa, drop = int(c.dtype == HF), bool(c.bounds), bool(c.nkv), bool(rng.keep_threshold(c.p))
    w = case_window(c)
    # the keep bits: by the forward itself (head-major, no window: gen_mask 1), ahead of it by
    # dlt_attn_dropout_mask (packed) or by dlt_attn_dropout_mask_band (a window); one kernel either way
    out = fwd_variants(drop, hk, c.hd, doc, gqa, gen_mask=False) + bwd_variants(drop, hk, c.hd, doc, gqa, c.packed)
    if drop:
        mv = mask_variant(c.S, w)
        out += [mv.split(" ")[0], "mask:" + mv]
    return out


ALL_VARIANTS = tuple(
    [f"k_attn_fwd<DROP={d},HK={h},D={D},DOC={o},GQA={g}>" for d in "01" for h in (0, 1) for D in (64, 128) for o in "01" for g in "01"]
    + [f"k_attn_bwd_dq<DROP={d},HK={h},D={D},DOC={o},GQA={g}>" for d in "01" for h in (0, 1) for D in (64, 128) for o in "01" for g in "01"]
    + [f"{kn}<DROP={d},HK={h},D={D},DOC={o}>" for kn in ("k_attn_bwd_dkdv", "k_attn_bwd_dkdv_gqa") for d in "01" for h in (0, 1)
       for D in (64, 128) for o in "01"]
    + ["k_dropout_bits<BAND=0>", "k_dropout_bits<BAND=1>", "bwd-store:rope", "bwd-store:plain",
       "mask:k_dropout_bits<BAND=0> S%32==0", "mask:k_dropout_bits<BAND=0> S%32!=0",
       "mask:k_dropout_bits<BAND=1> S%32==0", "mask:k_dropout_bits<BAND=1> S%32!=0"])

PATH_TAGS = ("unm-none", "unm-odd", "unm-even", "ragged-diag", "doc-ks>0", "doc-bound-tile", "doc-kdoc<nfull",
             "doc-wave-skip", "doc-dead-tile", "dkdv-unmasked", "dkdv-ragged-tail", "dkdv-doc-ends-early",
             "dkdv-doc-bound-tile", "dkdv-doc-unmasked", "pair-it1", "pair-middle", "xcd-rem", "xcd-even")


def path_tags(c: Case, sched: str = "lpt") -> set:
    """The in-kernel paths that depend only on shape, bounds and schedule (k_attn_fwd / _bwd_dq's
    tile loops, k_attn_bwd_dkdv's, work_item)."""
    S, tags = c.S, set()
    nrb = -(-S // RB)
    doc = case_bounds(c)
    for qb in range(nrb):
        end = min(S, qb * RB + RB)
        nkv = -(-end // RB)
        nfull = min(qb, nkv)
        if end % RB:
            tags.add("ragged-diag")
        if doc is None:
            tags.add("unm-none" if nfull == 0 else "unm-odd" if nfull % 2 else "unm-even")
            continue
        for b in range(c.B):
            lo = doc[0][b].tolist()
            ks = min(max(lo[qb * RB], 0) // RB, qb)
            kdoc = min((max(lo[end - 1], 0) + RB - 1) // RB, qb)
            if ks > 0:
                tags.add("doc-ks>0")
            if ks < kdoc:
                tags.add("doc-bound-tile")
            if kdoc < nfull:
                tags.add("doc-kdoc<nfull")
            for q0 in (qb * RB, qb * RB + 32):
                if q0 >= S:
                    continue
                rows = lo[q0:min(S, q0 + 32)]
                for kb in range(ks, nkv):
                    if not (kb < kdoc or kb >= nfull) or kb * RB > q0 + 31:
                        continue
                    if kb * RB + RB <= rows[0]:
                        tags.add("doc-wave-skip")  # wholly below this wave's documents
                    elif any(r >= kb * RB + RB for r in rows):
                        tags.add("doc-dead-tile")  # a lane with no live key in a tile it runs: M_DEAD
    nqt = nrb
    for kblk in range(nrb):
        if doc is None:
            nqe, t_full = nqt, S // RB
            if t_full > kblk + 1:
                tags.add("dkdv-unmasked")
            if nqe > max(t_full, kblk + 1):
                tags.add("dkdv-ragged-tail")
            continue
        for b in range(c.B):
            hi = doc[1][b].tolist()
            end = min(S, kblk * RB + RB)
            nqe = min(max(hi[end - 1] // RB, kblk) + 1, nqt)
            t_unm = min(max(hi[kblk * RB] + 1, 0) // RB, S // RB)
            if nqe < nqt:
                tags.add("dkdv-doc-ends-early")
            if t_unm > kblk + 1:
                tags.add("dkdv-doc-unmasked")
            if nqe > max(t_unm, kblk + 1):
                tags.add("dkdv-doc-bound-tile")
    if sched != "lpt":
        if nrb >= 2:
            tags.add("pair-it1")
        if nrb % 2:
            tags.add("pair-middle")
        if sched == "pair-xcd":
            for bh in {c.B * c.nh, c.B * c.kvh}:
                tags.add("xcd-rem" if (((nrb + 1) // 2) * bh) % 8 else "xcd-even")
    return tags


# ================================================================================= cases
def _name(dt, B, nh, nkv, S, hd, fam, bounds, p, packed):
    bn = "-".join(str(x) for x in bounds) if bounds else "causal"
    return f"{DT_NAME[dt]}-B{B}h{nh}kv{nkv}-S{S}-d{hd}-{fam}-{bn}-p{p}-{'packed' if packed else 'hm'}"


def _mk(dt, B, nh, nkv, S, hd, fam, bounds=(), p=0.0, packed=False) -> Case:
    return Case(_name(dt, B, nh, nkv, S, hd, fam, bounds, p, packed), dt, B, nh, nkv, S, hd, fam, tuple(bounds), p, packed)


def _grid_cases():
    """One case per DROP x HK x D x DOC x GQA, the other axes dealt round-robin over them: S,
    B * nh in {3, 8, 9} with nkv in {nh, nh / 2, 1}, the family, the bounds, the layout."""
    Ss = (320, 129, 200, 65, 33, 64, 1)
    heads = ((1, 3), (2, 4), (1, 9), (3, 1), (1, 8), (3, 3))        # (B, nh): B * nh = 3, 8, 9
    gq = {3: (3, 1), 4: (2, 4, 1), 9: (3, 1, 9), 1: (1,), 8: (4, 8, 2, 1)}
    fams = ("gauss", "flat", "steep_under", "big", "steep_over")
    bnds = (("doc",), ("win", 31), ("docwin", 65), ("win", 64), ("win", 1), ("win", 65), ("doc", 29), ("docwin", 31))
    out, i = [], 0
    for drop in (0, 1):
        for hk in (0, 1):
            for hd in (64, 128):
                for doc in (0, 1):
                    for gqa in (0, 1):
                        B, nh = heads[i % len(heads)]
                        S = Ss[i % len(Ss)]
                        nkv = gq[nh][(i // 2) % len(gq[nh])] if gqa else 0
                        b = bnds[(i // 2) % len(bnds)] if doc else ()
                        if b and b[0] != "doc" and b[1] >= S:  # a window that covers S is no window
                            b = ("doc",)
                        out.append(_mk((BF, HF)[hk], B, nh, nkv, S, hd, fams[i % len(fams)], b, 0.1 * drop,
                                       packed=(i % 3 == 1)))
                        i += 1
    return out


# the edge cases: flat rows of at most ROW_CAP keys (short documents, windows), where one key is
# worth 1 / n of a row, plus the steep families at the rescale threshold in fp16
EXTRA_CASES = [
    _mk(BF, 1, 2, 0, 65, 64, "flat", ("doc", 29)),
    _mk(BF, 1, 2, 0, 200, 64, "flat", ("win", 31), 0.1),
    _mk(HF, 1, 2, 1, 129, 64, "flat", ("docwin", 31), 0.0, True),
    _mk(BF, 1, 4, 2, 33, 64, "flat", (), 0.1, True),
    _mk(BF, 1, 4, 1, 33, 128, "flat", ()),
    _mk(HF, 1, 2, 0, 200, 64, "steep_under"),
    _mk(HF, 1, 2, 0, 200, 64, "steep_over"),
    _mk(BF, 1, 2, 0, 200, 128, "steep_over", ("doc",)),
    _mk(BF, 1, 2, 0, 320, 64, "gauss", ("win", 65), 0.1),
    _mk(BF, 1, 2, 0, 256, 64, "gauss", ("win", 31), 0.1),
    _mk(BF, 1, 1, 0, 96, 64, "gauss", ("win", 1), 0.1),
    _mk(BF, 1, 2, 0, 320, 64, "gauss", ("doc", -1), 0.1),
    _mk(BF, 1, 2, 0, 200, 64, "steep_under"),
    _mk(BF, 1, 2, 0, 200, 64, "steep_over"),
    _mk(BF, 1, 2, 0, 129, 64, "flat", ("win", 64)),
]
CASES = _grid_cases() + EXTRA_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# defect -> the case that shows it and the outputs it must push outside the tolerance
DEFECT_CASES = {
    "drop_diag": (EXTRA_CASES[0], ("o", "lse", "dq", "dk", "dv")),
    "see_next": (EXTRA_CASES[0], ("o", "lse", "dq", "dk", "dv")),
    "drop_last_key": (EXTRA_CASES[4], ("o", "lse", "dq", "dk", "dv")),
    "drop_lo": (EXTRA_CASES[0], ("o", "lse", "dq", "dk", "dv")),
    "drop_lo@window": (EXTRA_CASES[1], ("o", "lse", "dq", "dk", "dv")),
    "drop_hi": (EXTRA_CASES[0], ("dk", "dv")),
    "drop_hi@window": (EXTRA_CASES[1], ("dk", "dv")),
    "skip_half_tile": (EXTRA_CASES[4], ("o", "lse", "dq", "dk", "dv")),
    "l_not_rescaled": (EXTRA_CASES[6], ("o", "lse")),
    "no_threshold": (EXTRA_CASES[6], ("o",)),
    "no_dropout_scale": (EXTRA_CASES[3], ("o", "dq", "dk", "dv")),
    "keep_transposed": (EXTRA_CASES[3], ("o", "dq", "dk", "dv")),
    "kv_mod": (EXTRA_CASES[3], ("o", "dq")),
    "delta_3q": (EXTRA_CASES[3], ("dq", "dk", "delta")),
    "rope_fwd_sign": (EXTRA_CASES[3], ("dq", "dk")),
    "gqa_drop_head": (EXTRA_CASES[3], ("dk", "dv")),
}
# Single-key sensitivity on the flat family (test_single_key_sensitivity): in a row of at most
# this many live keys, losing ANY one of them moves some element of the output outside the
# tolerance by 2x.  o and dv scale as 1 / n and were expected to hold to 64 and 32 keys; dv holds
# to 23 (1.84x at 31).  dq and dk do not scale that way: a pair whose dP happens to equal the
# row's delta has dS = 0 whatever the tolerance, so losing it only moves the other keys' P by
# 1 / n^2; measured over every pair of the three sensitivity cases they hold to 15 and 7 keys.
# Short documents start a fresh row of 1, 2, 3, ... keys at every boundary, so the edge cases
# of DEFECT_CASES all contain rows inside every cap.
ROW_CAP = {"o": 64, "dv": 23, "dq": 15, "dk": 7}
SENSITIVITY_CASES = (EXTRA_CASES[0], EXTRA_CASES[2], EXTRA_CASES[-1])

# the non-default schedules: environment, and the cases each child runs (every S, both layouts,
# DOC and GQA, B * nh with a remainder mod 8 and without)
CHILD_CASES = [c.name for c in CASES[:32] if c.S in (320, 129, 200, 65)][:10] + [c.name for c in EXTRA_CASES[:4]]
CHILD_SETS = {
    "pair_xcd": ({"DLT_ATTN_SCHED": "pair"}, CHILD_CASES),
    "pair_natural": ({"DLT_ATTN_SCHED": "pair", "DLT_ATTN_XCD": "0"}, CHILD_CASES),
}
