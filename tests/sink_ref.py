"""fp64 references, derived tolerances, fp32 models with planted defects and fixed inputs for
attention sinks (``GPTConfig.attention_sinks``): the SINK forms of the flash forward
(``ops/csrc/attention_sink.hip``), ``k_attn_sink_bwd`` (``attention.hip``) and the ``sink=`` forms
of the fused decode kernels (``decode.hip``).  Shared by test_sinks_cpu.py and test_sinks_gpu.py;
nothing here needs a GPU.  Built on tests/attn_ref.py and tests/decode_*_ref.py: the same
conventions (a reference takes exactly what the kernel takes, computes in fp64 and returns every
output before its final rounding) and the same named tolerance terms.

A sink is one fp32 logit per QUERY head, in natural-log units, not multiplied by the score scale,
with no value row:  p_j = exp(s_j) / (sum_j exp(s_j) + exp(sink[h])).  With lse0 the plain
log-sum-exp over the live keys and o0 the plain output,
    lse = logaddexp(lse0, sink),   r = exp(lse0 - lse),   o = r o0,   p_sink = exp(sink - lse),
and dropout touches the p_j only.  The backward kernels rebuild P = exp(s - lse) from the stored lse,
so ``attn_ref.attn_bwd_ref`` fed the sink forward's o and lse IS the sink backward's reference;
    dsink[h] = -sum_{b,q} p_sink[b,h,q] delta[b,h,q],   delta = rowsum(dO * o) as dQ stores it.

Forward tolerance = the plain forward's, scaled by r, plus the epilogue's own terms (sink_fwd_ref):
  exponents   m' = max(m c, sink log2(e)) in log2 units: m c and sink log2(e) round once each (a U23
              of |m| and of |sink|), the differences m c - m' and sink log2(e) - m' once each (a U23
              of their size, at most |m| + |sink|), then one exp2 each (one ulp, ``attn_ref``'s
              assumption): the "one eps_p for the sink's exponential" and the "one rescale"
  l'          l alpha + e_sink: one product, one fp32 addition
  normaliser  dscale alpha / l': one more product
  flush       exp2 flushes results under 2^-126 to zero: alpha (a sink far above the scores: o
              becomes exactly 0) and e_sink (far below: the plain result)
A sink of -inf adds exactly nothing: there the tolerance is the plain one.
dsink tolerance (sink_bwd_ref): per addend the exponent (sink - lse, its product with log2(e), the
exp2, the product with delta: a U23 each, the first two of |sink - lse|), then an fp32 chain over
the B * S addends bounded by sum |p_sink delta|, the final subtraction from dsink, and the flush.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import torch

from tests import attn_ref as A
from tests import decode_gqa_ref as G
from tests import decode_ref as R
from tests import decode_win_ref as WN
from tests.stream_ref import BF, EXP_FLUSH, F32, HF, U23, Checked, f32, round_to, sub_floor

LOG2E = A.LOG2E
NINF = float("-inf")
SINK_VALUES = (NINF, -3.0, 0.0, 2.5, 60.0, 100.0)  # one case overflows a naive exp, one adds nothing


def sinks_for(nh: int, shift: int = 0) -> torch.Tensor:
    """fp32 [nh]: SINK_VALUES dealt to the heads, starting at ``shift``."""
    return torch.tensor([SINK_VALUES[(shift + h) % len(SINK_VALUES)] for h in range(nh)], dtype=F32)


# ============================================================================== forward
def _score_bound(q, k, scale, doc):
    """Largest live |score| of every row, [B, nh, S] (natural-log units)."""
    B, nh, S, _ = q.shape
    s = torch.matmul(q.double(), A._kv_heads(k, nh).transpose(-1, -2)) * f32(scale)
    lq, _ = A.live_masks(B, S, doc)
    return torch.where(lq, s.abs(), torch.zeros_like(s)).amax(-1)


def sink_fwd_ref(q, k, v, scale: float, sink: torch.Tensor, doc=None, p: float = 0.0, key: int = 0) -> A.Fwd:
    """The SINK forward: o [B, S, nh, hd] before its rounding to 16 bits, lse [B, nh, S]."""
    B, nh, S, hd = q.shape
    dt = q.dtype
    base = A.attn_fwd_ref(q, k, v, scale, doc, p, key)
    sk = sink.double().view(1, nh, 1).expand(B, nh, S)
    fin = torch.isfinite(sk)
    lse = torch.logaddexp(base.lse.ref, sk)
    r = torch.exp(base.lse.ref - lse)
    rt = r.transpose(1, 2).unsqueeze(-1)  # [B, S, nh, 1]
    o = base.o.ref * rt
    zero = torch.zeros_like(sk)
    # the kernel's running max is deferred: up to 2^8 under the row's largest score
    mk = _score_bound(q, k, scale, doc) + A.RESCALE_LOG2 * A.LN2
    ska = torch.where(fin, sk.abs(), zero)
    eps_exp = U23 * (mk + ska + 2 * (mk + ska) + 2)  # the two products, the two differences, two exp2
    eps_lp = torch.where(fin, eps_exp + 2 * U23 + EXP_FLUSH * 2.0 ** A.RESCALE_LOG2, zero)  # l alpha + e_sink
    eps_o = torch.where(fin, eps_lp + U23, zero).transpose(1, 2).unsqueeze(-1)       # dscale alpha / l'
    _, dscale, _ = A.keep_of(B, nh, S, key, p)
    o_tol = rt * base.o.tol + eps_o * (o.abs() + rt * base.o.tol) * (1 + A._hu(dt)) + A._fl(dt) \
        + torch.where(fin, zero + EXP_FLUSH * dscale, zero).transpose(1, 2).unsqueeze(-1) * base.o.ref.abs()
    # lse = m' / log2(e) + log(l'): the plain terms with max(|m|, |sink|) for A and l' <= S + 1
    big = torch.maximum(mk, ska)
    lse_tol = r * base.lse.tol + eps_lp + U23 * (2 * big + 2 * (math.log(S + 1) + A.RESCALE_LOG2 * A.LN2) + 1 + lse.abs())
    return A.Fwd(Checked(o, o_tol), Checked(lse, torch.where(fin, lse_tol, base.lse.tol)))


FWD_DEFECTS = ("sink_scaled", "sink_kv_head", "sink_next_head", "lse_only", "sink_dropout_scaled")


def _sink_of_head(sink: torch.Tensor, nh: int, nkv: int, scale: float, defect: Optional[str]) -> torch.Tensor:
    h = torch.arange(nh)
    if defect == "sink_kv_head":     # indexed by the K/V head h // G
        return sink[h // (nh // nkv)]
    if defect == "sink_next_head":   # head h + 1's
        return sink[(h + 1) % nh]
    if defect == "sink_scaled":      # multiplied by the score scale
        return sink * torch.tensor(f32(scale), dtype=F32)
    return sink


def sink_fwd_model(q, k, v, scale: float, sink: torch.Tensor, doc=None, p: float = 0.0, key: int = 0,
                   defect: Optional[str] = None):
    """The SINK kernel's arithmetic in fp32 torch (one softmax pass per row, P rounded to the
    16-bit format, the epilogue as attention_fwd_body.h writes it).  Returns (o [B, S, nh, hd]
    16-bit, lse fp32).  ``defect``: one of FWD_DEFECTS."""
    assert defect is None or defect in FWD_DEFECTS
    B, nh, S, hd = q.shape
    dt = q.dtype
    nkv = k.shape[1]
    L2 = torch.tensor(LOG2E, dtype=F32)
    c = torch.tensor(f32(scale), dtype=F32) * L2
    kf, vf = (t.float().repeat_interleave(nh // nkv, 1) for t in (k, v))
    lq, _ = A.live_masks(B, S, doc)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)).masked_fill(~lq, NINF)
    keep, dscale, _ = A.keep_of(B, nh, S, key, p)
    keep, dsc = keep.float(), torch.tensor(dscale, dtype=F32)
    m = s.amax(-1)
    pt = torch.exp2(torch.addcmul((-m * c).unsqueeze(-1), s, c))
    l = pt.sum(-1)
    O = torch.matmul((pt * keep).to(dt).float(), vf)
    sk = _sink_of_head(sink.float(), nh, nkv, scale, defect).view(1, nh, 1).expand(B, nh, S)
    m2, s2 = m * c, sk * L2
    mn = torch.maximum(m2, s2)
    alpha, es = torch.exp2(m2 - mn), torch.exp2(s2 - mn)
    if defect == "sink_dropout_scaled":  # the sink's term takes the dropout factor 1 / (1 - p)
        es = es * dsc
    lp = l * alpha + es
    inv = dsc / l if defect == "lse_only" else dsc * alpha / lp  # lse_only: o keeps the plain normaliser
    o = (O * inv.unsqueeze(-1)).to(dt).transpose(1, 2)
    lse = torch.where(s2 > m2, sk, m * (c / L2)) + torch.log(lp)
    return o, lse


# ============================================================================= dsink
BWD_DEFECTS = ("dsink_sign", "dsink_delta_over_dscale")


def sink_bwd_ref(lse32: torch.Tensor, delta32: torch.Tensor, sink: torch.Tensor) -> Checked:
    """dsink [nh] from the stored fp32 lse and delta [B, nh, S] (what k_attn_sink_bwd reads),
    for an accumulator that was zero."""
    B, nh, S = lse32.shape
    sk = sink.double().view(1, nh, 1)
    fin = torch.isfinite(sk).expand(B, nh, S)
    x = sk - lse32.double()
    t = torch.exp(x) * delta32.double()
    ref = -t.sum(dim=(0, 2))
    zero = torch.zeros_like(t)
    # the difference and its product with log2(e) (a U23 of |sink - lse| each), exp2, the product with delta
    eps_ps = torch.where(fin, U23 * (2 * x.abs() + 2), zero)
    tabs = t.abs()
    tol = (tabs * eps_ps).sum(dim=(0, 2)) + A._chain(B * S) * tabs.sum(dim=(0, 2)) + U23 * ref.abs() \
        + EXP_FLUSH * delta32.double().abs().sum(dim=(0, 2))
    return Checked(ref, tol)


def sink_bwd_model(lse32, delta32, sink, defect: Optional[str] = None, dscale: float = 1.0) -> torch.Tensor:
    """k_attn_sink_bwd in fp32 torch; ``defect``: one of BWD_DEFECTS."""
    assert defect is None or defect in BWD_DEFECTS
    nh = lse32.shape[1]
    d = delta32 / torch.tensor(f32(dscale), dtype=F32) if defect == "dsink_delta_over_dscale" else delta32
    t = (torch.exp2((sink.float().view(1, nh, 1) - lse32) * torch.tensor(LOG2E, dtype=F32)) * d).sum(dim=(0, 2))
    return t if defect == "dsink_sign" else -t


# ================================================================================ cases
HEADS = ((4, 0), (4, 2), (4, 1), (6, 2), (4, 4))   # (nh, nkv): nkv 0 = the MHA kernels, (4, 4) the GQA kernels at G = 1
WINDOWS = (1, 37, 64, 200)


def _cases():
    """One case per DROP x HK x D x DOC x GQA of the SINK forward, the other axes dealt round-robin:
    S 192 / 200, the heads, the layout, and for the DOC forms a document mask (separators inside
    32-query halves: attn_ref.doc_seps) or one of the windows.  B = 2 throughout."""
    out, i, ng, nd = [], 0, 0, 0
    bnds = (("doc",), ("win", 1), ("win", 37), ("win", 64), ("docwin", 37), ("doc",), ("win", 64), ("win", 37))
    gq = ((4, 2), (4, 1), (6, 2), (4, 4))
    for drop in (0, 1):
        for hk in (0, 1):
            for hd in (64, 128):
                for doc in (0, 1):
                    for gqa in (0, 1):
                        nh, nkv = gq[ng % 4] if gqa else (4, 0)
                        b = bnds[nd % len(bnds)] if doc else ()
                        ng, nd = ng + gqa, nd + doc
                        S = (192, 200)[(i + i // 2 + i // 4) % 2]
                        out.append(A._mk((BF, HF)[hk], 2, nh, nkv, S, hd, "gauss", b, 0.1 * drop,
                                         packed=((i + i // 8) % 3 != 0)))
                        i += 1
    # a window that covers the sequence (W = 200 at S = 200 and 192) is no window: the plain SINK forms
    out.append(A._mk(BF, 2, 4, 2, 200, 64, "gauss", ("win", 200), 0.1, packed=True))
    out.append(A._mk(BF, 2, 4, 0, 192, 64, "gauss", ("win", 200), 0.0, packed=False))
    # large scores next to the sinks: |score| reaches about 60
    out.append(A._mk(BF, 2, 6, 2, 200, 64, "big", (), 0.0, packed=True))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the case the planted defects are shown at: grouped heads, dropout on, four different finite sinks
DEFECT_CASE = next(c for c in CASES if (c.nh, c.nkv) == (4, 2) and c.p > 0 and not c.bounds and c.dtype == BF)
DEFECT_SINKS = torch.tensor([-3.0, 2.5, 0.0, 60.0], dtype=F32)


# The cases whose dq / dk / dv bound is attn_ref's plus the flush term: only the "big" family, which
# the issue does not list.  Every listed configuration keeps attn_ref's backward tolerance as it is.
FLUSH_CASES = frozenset(c.name for c in CASES if c.family == "big")


def case_sinks(c: A.Case) -> torch.Tensor:
    """The sinks of a case: every value of SINK_VALUES appears over the cases, -inf and +100 in most."""
    if c.name == DEFECT_CASE.name:
        return DEFECT_SINKS.clone()
    return sinks_for(c.nh, shift=CASES.index(c))


def bwd_flush_terms(c, inp, o16, lse32):
    """What the hardware exp2's flush adds to ``attn_ref.attn_bwd_ref``'s bound: (dq, dk, dv) extras.
    The backward kernels rebuild P = exp2(s c - lse log2(e)); a P under the fp32 normal range comes
    out as exactly 0, an absolute error of at most 2^-126 per (query, key) pair.  It reaches
    dS = P (keep dscale dP - delta) through |keep dscale dP - delta|, dq and dk through |k| and |q|
    times the scale, and dv through keep dscale |dO|.  Without sinks the term cannot matter (a row's
    largest P is at least 1 / S, next to which 2^-126 vanishes) and attn_ref does not carry it; a
    sink far above the scores pushes WHOLE rows under the range, where the kernel's 0 differs from
    a true value of about 1e-38 by more than half a bf16 subnormal.  With rope the rotation mixes
    the two halves of a row: each half is charged both."""
    B, nh, S, hd = inp.q.shape
    nkv = inp.k.shape[1]
    G = nh // nkv
    sc = f32(inp.scale)
    qd, kd, vd = inp.q.double(), A._kv_heads(inp.k, nh), A._kv_heads(inp.v, nh)
    O = o16.double().view(B, S, nh, hd).transpose(1, 2)
    dO = inp.do.double().view(B, S, nh, hd).transpose(1, 2)
    lq, lk = A.live_masks(B, S, inp.doc)
    keep, _, ds_true = A.keep_of(B, nh, S, c.key, c.p)
    inner = (keep * ds_true * torch.matmul(dO, vd.transpose(-1, -2)) - (dO * O).sum(-1, keepdim=True)).abs()
    grp = lambda t: t.view(B, nkv, G, S, hd).sum(2)  # noqa: E731
    dq = EXP_FLUSH * sc * torch.matmul(inner * lq, kd.abs())
    dk = grp(EXP_FLUSH * sc * torch.matmul((inner * lk).transpose(-1, -2), qd.abs()))
    dv = grp(EXP_FLUSH * ds_true * torch.matmul((keep * lk * torch.ones_like(inner)).transpose(-1, -2), dO.abs()))
    if inp.rope is not None:
        mix = lambda e: torch.cat([e[..., :hd // 2] + e[..., hd // 2:]] * 2, -1)  # noqa: E731
        dq, dk = mix(dq), mix(dk)
    return dq, dk, dv


class Refs(NamedTuple):
    inp: A.Inputs
    sink: torch.Tensor
    fwd: A.Fwd
    o16: torch.Tensor     # the forward reference's o / lse in their storage formats: the backward's inputs
    lse32: torch.Tensor
    bwd: A.Bwd
    delta32: torch.Tensor
    dsink: Checked


@functools.lru_cache(maxsize=None)
def case_refs(name: str) -> Refs:
    c = BY_NAME[name]
    inp = A.attn_inputs(c)
    sink = case_sinks(c)
    fwd = sink_fwd_ref(inp.q, inp.k, inp.v, inp.scale, sink, inp.doc, c.p, c.key)
    o16 = round_to(fwd.o.ref, c.dtype).reshape(c.B * c.S, c.nh * c.hd).contiguous()
    lse32 = fwd.lse.ref.to(F32)
    bwd = A.attn_bwd_ref(inp.q, inp.k, inp.v, o16, inp.do, lse32, inp.scale, inp.doc, c.p, c.key, inp.rope)
    if c.name in FLUSH_CASES:  # an extra of this file: attn_ref's bound plus the exp2 flush, see bwd_flush_terms
        ex = bwd_flush_terms(c, inp, o16, lse32)
        bwd = bwd._replace(**{nm: Checked(getattr(bwd, nm).ref, getattr(bwd, nm).tol + e)
                              for nm, e in zip(("dq", "dk", "dv"), ex)})
    delta32 = bwd.delta.ref.to(F32)
    ds = sink_bwd_ref(lse32, delta32, sink)
    # k_attn_sink_bwd reads the delta dQ wrote in the same launch, within bwd.delta.tol (and one
    # fp32 rounding) of the reference's: every addend moves by at most p_sink times that
    p_sink = torch.exp(sink.double().view(1, c.nh, 1) - lse32.double())
    ds = Checked(ds.ref, ds.tol + (p_sink * (bwd.delta.tol + U23 * bwd.delta.ref.abs())).sum(dim=(0, 2)))
    return Refs(inp, sink, fwd, o16, lse32, bwd, delta32, ds)


def worst(out: torch.Tensor, chk: Checked) -> float:
    """max |out - ref| / tol (an error where the tolerance is zero counts as itself)."""
    err = (out.double().reshape(chk.ref.shape) - chk.ref).abs()
    bad = ~(err <= chk.tol)
    if not bad.any():
        return torch.where(chk.tol > 0, err / chk.tol, err).max().item()
    return max(1.0 + 1e-9, torch.where(chk.tol > 0, err / chk.tol, torch.full_like(err, math.inf))[bad].max().item())


# =============================================================================== decode
DEC_MAXS = G.ATTN_MAXS          # a 200-key cache: the last chunk of NS = 4 / 8 is ragged
DEC_SPLITS = (1, 2, 4, 8)
DEC_HEADS = ((4, 1), (4, 2), (6, 2), (12, 4))
DEC_WINDOWS = (None, 50, 7)
DEC_SCALE = R.ATTN_SCALE
DEC_DEFECTS = ("sink_per_chunk", "sink_no_rescale")
# The sink's terms on top of decode_ref.attn_ref's tolerance: one more probability (the 80 * 2^-24
# + 2^-22 relative of its docstring), the max with the sink and the addition into the normaliser
# (2^-23 each); relative to o, whose every element the normaliser scales.  With the sink as the
# maximum every key's probability can lie under the fp32 normal range, where exp flushes to zero
# (2^-126 per key, over a normaliser of at least 1), and o itself under bf16's (half a subnormal).
DEC_SINK_REL = 80 * 2.0 ** -24 + 2.0 ** -22 + 2.0 ** -22


def dec_positions(W: Optional[int], NS: int, maxS: int = DEC_MAXS):
    """Position 0, both sides of every chunk boundary, the last cache row."""
    C = WN.chunk(maxS, W, NS)
    if W:
        return WN.gqa_positions(W, C, NS, maxS)
    ps = {0, maxS - 1}
    for s in range(1, NS):
        ps |= {s * C - 1, s * C, s * C + 1}
    return tuple(sorted(p for p in ps if 0 <= p < maxS))


def dec_sink_ref(q, kc, vc, pos: int, scale: float, nh: int, sink: torch.Tensor, W: Optional[int] = None) -> R.Checked:
    """dec_attn / dec_attn_gqa with ``sink=``: the windowed reference scaled by the keys' share r
    of the softmax mass; tolerance r (U8 |o| + 1e-4 sum p |v|) + DEC_SINK_REL |o| + the flush floor."""
    base = WN.attn_gqa_win_ref(q, kc, vc, pos, scale, nh, W)
    B, nkv = kc.shape[:2]
    kf = WN.first_key(pos, W)
    idx = G.kv_head_of(nh, nkv).to(kc.device)
    K = kc[:, :, kf:pos + 1].double().index_select(1, idx)
    s = torch.einsum("bhd,bhjd->bhj", q.double().view(B, nh, 64), K) * scale
    lse0 = torch.logsumexp(s, dim=-1)
    r = torch.exp(lse0 - torch.logaddexp(lse0, sink.double().to(kc.device).view(1, nh).expand(B, nh))).unsqueeze(-1)
    o = base.ref * r
    V = vc[:, :, kf:pos + 1].double().index_select(1, idx)
    floor = EXP_FLUSH * V.abs().sum(dim=2) + sub_floor(BF)
    return R.Checked(o, r * base.tol + DEC_SINK_REL * o.abs() + floor)


def dec_sink_split32(q, kc, vc, pos: int, scale: float, nh: int, NS: int, W: Optional[int], sink: torch.Tensor,
                     defect: Optional[str] = None) -> torch.Tensor:
    """fp32 model of k_dec_attn_gqa + k_dec_attn_combine with a sink (NS == 1: also k_dec_attn's
    arithmetic): per chunk (m, l, o), merged in the order s = 0 .. NS - 1; the sink joins ONCE,
    M = max(M, sink) before the partials are rescaled, L += exp(sink - M).  bf16 [B, nh, 64].
    ``defect``:
      sink_per_chunk    every chunk workgroup folds the sink into its own max and sum
      sink_no_rescale   the combine adds exp(sink - max(M, sink)) to partials rescaled to the OLD M"""
    assert defect is None or defect in DEC_DEFECTS
    B, nkv, maxS = kc.shape[:3]
    idx = G.kv_head_of(nh, nkv)
    end, kf, C = pos + 1, WN.first_key(pos, W), WN.chunk(maxS, W, NS)
    qf = q.float().view(B, nh, 64)
    sk = sink.float().view(1, nh, 1).expand(B, nh, 1)
    parts = []
    for s in range(NS):
        lo, hi = kf + s * C, min(kf + (s + 1) * C, end)
        if hi <= lo:
            continue
        K = kc[:, :, lo:hi].float().index_select(1, idx)
        V = vc[:, :, lo:hi].float().index_select(1, idx)
        sc = torch.einsum("bhd,bhjd->bhj", qf, K) * torch.tensor(scale, dtype=F32)
        m = sc.amax(dim=-1, keepdim=True)
        if NS == 1 or defect == "sink_per_chunk":
            m = torch.maximum(m, sk)
        p = torch.exp(sc - m)
        l = p.sum(dim=-1, keepdim=True)
        if NS == 1 or defect == "sink_per_chunk":
            l = l + torch.exp(sk - m)
        parts.append((m, l, torch.einsum("bhj,bhjd->bhd", p, V)))
    if NS == 1:
        m, l, o = parts[0]
        return (o * (1.0 / l)).bfloat16()
    M = parts[0][0]
    for m, _, _ in parts[1:]:
        M = torch.maximum(M, m)
    M_parts = M
    if defect != "sink_per_chunk":
        M = torch.maximum(M, sk)
        if defect != "sink_no_rescale":
            M_parts = M
    L = torch.zeros_like(M)
    acc = torch.zeros_like(parts[0][2])
    for m, l, o in parts:
        f = torch.exp(m - M_parts)
        L = L + l * f
        acc = acc + o * f
    if defect != "sink_per_chunk":
        L = L + torch.exp(sk - M)
    return (acc / L).bfloat16()
