"""What tests/attn_ref.py claims, checked without a GPU: the fp64 references agree with autograd
through an eager fp64 attention, a plain fp32 emulation of the kernels' arithmetic stays inside
every tolerance, every planted defect falls outside by 2x at the case the GPU file runs, one
missing key of a short flat row is visible, and the case lists reach every instantiation and
path tag of the dispatch model.  ``pytest -s`` shows the ratios."""
import itertools
import math

import pytest
import torch

from distributed_llm_trainer_amd.ops import reference as opsref
from distributed_llm_trainer_amd.ops import rng
from tests import attn_ref as A

F64 = torch.float64
INF = torch.tensor(math.inf, dtype=F64)
OUTS = ("o", "lse", "dq", "dk", "dv", "delta")


def ratio(out, chk) -> float:
    """Worst err / tol; an element that is NaN, or off where the tolerance is zero, counts as inf."""
    err = (out.double().reshape(chk.ref.shape) - chk.ref).abs()
    r = torch.where(chk.tol > 0, err / chk.tol, torch.where(err > 0, INF, err))
    return torch.where(torch.isnan(r), INF, r).max().item()


def defect_ratios(c, defect, at=None):
    """Per output: how far the reference with ``defect`` lies from the clean one, in tolerances."""
    inp, fwd, o16, lse32, bwd = A.case_refs(c)
    d = defect.split("@")[0]
    f = A.attn_fwd_ref(inp.q, inp.k, inp.v, inp.scale, inp.doc, c.p, c.key, defect=d, at=at)
    b = A.attn_bwd_ref(inp.q, inp.k, inp.v, o16, inp.do, lse32, inp.scale, inp.doc, c.p, c.key, inp.rope, defect=d, at=at)
    got = dict(o=f.o, lse=f.lse, dq=b.dq, dk=b.dk, dv=b.dv, delta=b.delta)
    want = dict(o=fwd.o, lse=fwd.lse, dq=bwd.dq, dk=bwd.dk, dv=bwd.dv, delta=bwd.delta)
    return {k: ratio(got[k].ref, want[k]) for k in OUTS}


# ------------------------------------------------------------------ references vs autograd
def _eager(q, k, v, do, scale, doc, p, key, rope):
    """Eager fp64 attention with masked_fill and the rng keep mask; gradients by autograd.  With
    ``rope`` q and k are the rotation of the leaves, so the leaves' gradients carry its inverse."""
    B, nh, S, hd = q.shape
    G = nh // k.shape[1]
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    if rope is not None:
        c, s = rope[0].double().view(1, 1, S, hd // 2), rope[1].double().view(1, 1, S, hd // 2)
        qr, kr = opsref._rot(ql, c, s), opsref._rot(kl, c, s)
    else:
        qr, kr = ql, kl
    sc = torch.matmul(qr, kr.repeat_interleave(G, 1).transpose(-1, -2)) * A.f32(scale)
    dead = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1).view(1, 1, S, S)
    if doc is not None:
        dead = dead | (torch.arange(S).view(1, 1, 1, S) < doc[0].view(B, 1, S, 1))
    sc = sc.masked_fill(dead, -math.inf)
    lse = torch.logsumexp(sc, -1)
    prob = torch.softmax(sc, -1)
    if rng.keep_threshold(p):
        prob = prob * rng.attn_keep_mask(B * nh, S, S, key, p).view(B, nh, S, S) * A.f32(1.0 / (1.0 - p))
    o = torch.matmul(prob, vl.repeat_interleave(G, 1)).transpose(1, 2)  # [B, S, nh, hd]
    o.backward(do.view(B, S, nh, hd))
    return o.detach(), lse.detach(), ql.grad, kl.grad, vl.grad


@pytest.mark.parametrize("bounds,nkv,p,rope", list(itertools.product(
    ((), ("doc",), ("win", 31), ("docwin", 17)), (0, 4, 2, 1), (0.0, 0.1), (False, True))),
    ids=lambda x: str(x).replace(" ", ""))
def test_references_agree_with_autograd(bounds, nkv, p, rope):
    c = A._mk(A.BF, 2, 4, nkv, 70, 64, "gauss", bounds, p, rope)
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(c.B, h, c.S, c.hd, generator=g, dtype=F64) for h in (c.nh, c.kvh, c.kvh, c.nh))
    do = do.transpose(1, 2).reshape(c.B * c.S, -1).contiguous()
    doc = A.case_bounds(c)
    tabs = opsref.rope_tables(c.hd, c.S) if rope else None
    scale = 1.0 / math.sqrt(c.hd)
    qr, kr = q, k
    if rope:
        cs, sn = tabs[0].double().view(1, 1, c.S, -1), tabs[1].double().view(1, 1, c.S, -1)
        qr, kr = opsref._rot(q, cs, sn), opsref._rot(k, cs, sn)
    o, lse, dq, dk, dv = _eager(q, k, v, do, scale, doc, p, c.key, tabs)
    fwd = A.attn_fwd_ref(qr, kr, v, scale, doc, p, c.key)
    bwd = A.attn_bwd_ref(qr, kr, v, o.reshape(c.B * c.S, -1), do, lse, scale, doc, p, c.key, tabs)
    for name, got, want in (("o", fwd.o.ref, o), ("lse", fwd.lse.ref, lse), ("dq", bwd.dq.ref, dq),
                            ("dk", bwd.dk.ref, dk), ("dv", bwd.dv.ref, dv)):
        rel = ((got - want).abs().max() / want.abs().max()).item()
        assert rel <= 1e-12, f"{name}: {rel:.3e}"
    delta = (do.view(c.B, c.S, c.nh, c.hd) * o).sum(-1).transpose(1, 2)
    assert ((bwd.delta.ref - delta).abs().max() / delta.abs().max()).item() <= 1e-12


# ------------------------------------------------------------ emulation inside tolerances
WORST = {}


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_emulation_inside_every_tolerance(name):
    c = A.BY_NAME[name]
    inp, fwd, o16, lse32, bwd = A.case_refs(c)
    o, lse = A.attn_fwd_emul(inp.q, inp.k, inp.v, inp.scale, inp.doc, c.p, c.key)
    dq, dk, dv, delta = A.attn_bwd_emul(inp.q, inp.k, inp.v, o16, inp.do, lse32, inp.scale, inp.doc, c.p, c.key, inp.rope)
    rs = dict(o=ratio(o, fwd.o), lse=ratio(lse, fwd.lse), dq=ratio(dq, bwd.dq), dk=ratio(dk, bwd.dk),
              dv=ratio(dv, bwd.dv), delta=ratio(delta, bwd.delta))
    print("EMUL " + name + " " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))
    for k, v in rs.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    assert all(v < 1.0 for v in rs.values()), rs
    if name == A.CASES[-1].name:
        print("EMUL worst err/tol per output: " + " ".join(f"{k}={v:.3f}" for k, v in WORST.items()))


def test_emulation_is_not_the_reference():
    """The emulation's 16-bit roundings are there: its error is a visible share of the tolerance."""
    c = A.CASES[0]
    inp, fwd, o16, lse32, bwd = A.case_refs(c)
    o, _ = A.attn_fwd_emul(inp.q, inp.k, inp.v, inp.scale, inp.doc, c.p, c.key)
    assert ratio(o, fwd.o) > 0.2


# --------------------------------------------------------------------------- the defects
@pytest.mark.parametrize("defect", list(A.DEFECT_CASES))
def test_planted_defect_falls_outside(defect):
    c, outs = A.DEFECT_CASES[defect]
    r = defect_ratios(c, defect)
    print(f"DEFECT {defect} on {c.name}: " + " ".join(f"{k}={r[k]:.2f}" for k in outs))
    assert all(r[k] >= 2.0 for k in outs), r


def test_every_defect_has_a_case():
    named = {d.split("@")[0] for d in A.DEFECT_CASES}
    assert named == set(A.DEFECTS) - {"drop_one", "p_trunc"}  # those two: the tests below


def test_p_truncated_cannot_reach_2x():
    """acc_frag rounds P to nearest.  A kernel that truncated it is wrong by at most one ulp of P,
    2 U8 sum_k P |v|, where the tolerance grants U8 (sum_k P |v| + |o|) for the rounding of P and of
    o; the shift is proportional to sum_k P v = o, so it cannot grow while |o| stays small.  The
    defect is therefore bounded by 1x here and is recorded as not detectable per element."""
    r = defect_ratios(A.CASES[0], "p_trunc")
    print(f"DEFECT p_trunc: o={r['o']:.2f}")
    assert 0.3 < r["o"] < 2.0


def test_p_truncated_shows_in_the_bias_check():
    """What the element-wise bound cannot see, the sign of the errors does: bias_ratio() of the
    truncating defect is far above 2, of the round-to-nearest emulation below 1."""
    c = A.CASES[0]
    inp, fwd, o16, lse32, bwd = A.case_refs(c)
    bad = A.attn_fwd_ref(inp.q, inp.k, inp.v, inp.scale, inp.doc, c.p, c.key, defect="p_trunc")
    r = A.bias_ratio(bad.o.ref, fwd.o)
    print(f"DEFECT p_trunc: bias ratio {r:.2f}")
    assert r >= 2.0
    for c in (x for x in A.CASES if x.family == "gauss" and x.S >= 64):
        inp, fwd, o16, lse32, bwd = A.case_refs(c)
        o, _ = A.attn_fwd_emul(inp.q, inp.k, inp.v, inp.scale, inp.doc, c.p, c.key)
        dq, dk, dv, _ = A.attn_bwd_emul(inp.q, inp.k, inp.v, o16, inp.do, lse32, inp.scale, inp.doc, c.p, c.key, inp.rope)
        rs = [A.bias_ratio(x, y) for x, y in ((o, fwd.o), (dq, bwd.dq), (dk, bwd.dk), (dv, bwd.dv))]
        print(f"BIAS {c.name}: " + " ".join(f"{x:.3f}" for x in rs))
        assert max(rs) < 1.0


# ------------------------------------------------------------------ single-key sensitivity
@pytest.mark.parametrize("idx", range(len(A.SENSITIVITY_CASES)))
def test_single_key_sensitivity(idx):
    """Flat rows: losing any one live key of a row of at most ROW_CAP[output] keys moves that
    output outside its tolerance by 2x.  Every pair of the first case; every row and its first,
    middle and last key of the longer two."""
    c = A.SENSITIVITY_CASES[idx]
    lq, _ = A.live_masks(c.B, c.S, A.attn_inputs(c).doc)
    worst = {k: (math.inf, None) for k in A.ROW_CAP}
    seen = {k: 0 for k in A.ROW_CAP}
    for qi in range(c.S):
        ks = lq[0, 0, qi].nonzero().flatten().tolist()
        n = len(ks)
        if n < 2 or n > max(A.ROW_CAP.values()):
            continue
        for kk in (ks if idx == 0 else sorted({ks[0], ks[n // 2], ks[-1]})):
            r = defect_ratios(c, "drop_one", at=(qi, kk))
            for out, cap in A.ROW_CAP.items():
                if n <= cap:
                    seen[out] = max(seen[out], n)
                    if r[out] < worst[out][0]:
                        worst[out] = (r[out], (qi, kk, n))
    print(f"SENSITIVITY {c.name}: " + " ".join(f"{k}={v[0]:.2f}@{v[1]} (rows to {seen[k]})" for k, v in worst.items()))
    assert all(v[0] >= 2.0 for v in worst.values()), worst
    if idx == 2:
        assert seen["o"] == A.ROW_CAP["o"]


# ----------------------------------------------------------------------- dispatch coverage
def test_sched_of_reads_the_environment_as_the_launcher():
    assert A.sched_of({}) == "lpt"
    assert A.sched_of({"DLT_ATTN_XCD": "0"}) == "lpt"  # LPT overrides the XCD bit
    assert A.sched_of({"DLT_ATTN_SCHED": "lpt", "DLT_ATTN_XCD": "0"}) == "lpt"
    assert A.sched_of({"DLT_ATTN_SCHED": "pair"}) == "pair-xcd"
    assert A.sched_of({"DLT_ATTN_SCHED": "p", "DLT_ATTN_XCD": "1"}) == "pair-xcd"
    assert A.sched_of({"DLT_ATTN_SCHED": "pair", "DLT_ATTN_XCD": "0"}) == "pair-natural"
    assert A.sched_of({"DLT_ATTN_SCHED": "pair", "DLT_ATTN_XCD": "off"}) == "pair-natural"  # atoi("off") == 0
    assert {A.sched_of(env) for env, _ in A.CHILD_SETS.values()} == {"pair-xcd", "pair-natural"}


def test_mask_variant_follows_the_band_launcher():
    assert A.mask_variant(320) == "k_dropout_bits<BAND=0> S%32==0"
    assert A.mask_variant(200, 31) == "k_dropout_bits<BAND=1> S%32!=0"
    assert A.mask_variant(320, 65) == "k_dropout_bits<BAND=1> S%32==0"   # D = 1: 4 slots < 11 bands
    assert A.mask_variant(96, 65) == "k_dropout_bits<BAND=0> S%32==0"    # 4 slots >= 3 + 1 bands: the full kernel
    assert A.mask_variant(64, 31) == "k_dropout_bits<BAND=0> S%32==0"
    assert A.mask_variant(96, 1) == "k_dropout_bits<BAND=1> S%32==0"
    assert A.mask_variant(64, 64) == "k_dropout_bits<BAND=0> S%32==0"   # a window that covers S


def test_cases_reach_every_variant():
    """Each instantiation dlt_attn_fwd / dlt_attn_bwd / dlt_attn_dropout_mask{,_band} can emit, by
    name: DROP x HK x D x DOC x GQA of the forward and dQ, DROP x HK x D x DOC of both dK/dV
    kernels, both k_dropout_bits forms on both of their paths, both stores of the backward."""
    assert len(A.ALL_VARIANTS) == 32 + 32 + 16 + 16 + 2 + 2 + 4 and len(set(A.ALL_VARIANTS)) == len(A.ALL_VARIANTS)
    hit = {}
    for c in A.CASES:
        for v in A.case_variants(c):
            assert v in A.ALL_VARIANTS, f"{c.name} launches {v}, which the model does not list"
            hit.setdefault(v, c.name)
    # the forward's own generation (gen_mask = 1) runs in every case with dropout and no window
    for v in A.ALL_VARIANTS:
        print(f"VARIANT {v}: {hit.get(v)}")
    missing = [v for v in A.ALL_VARIANTS if v not in hit]
    assert not missing, missing


def test_variant_model_covers_the_launchers_template_arguments():
    """The names the model emits are built from the template argument lists of attention.hip: a
    template parameter added to a kernel there changes this count and fails here."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed_llm_trainer_amd",
                            "ops", "csrc", "attention.hip")).read()
    want = {"k_attn_fwd": ["DROP", "HK", "D", "DOC", "GQA"], "k_attn_bwd_dq": ["DROP", "HK", "D", "DOC", "GQA"],
            "k_attn_bwd_dkdv": ["DROP", "HK", "D", "DOC"], "k_attn_bwd_dkdv_gqa": ["DROP", "HK", "D", "DOC"],
            "k_dropout_bits": ["BAND"]}
    for kern, params in want.items():
        m = re.search(r"template <([^>]*)>\s*__global__[^;{]*?\b" + kern + r"\(", src)
        assert m, kern
        got = [p.split("=")[0].split()[-1] for p in m.group(1).split(",")]
        assert got == params, (kern, got)
        assert any(v.startswith(kern + "<" + params[0] + "=") for v in A.ALL_VARIANTS)
    assert sorted(set(re.findall(r"\b(k_\w+)<[^<>]*><<<", src))) == sorted(want)


def test_cases_reach_every_path_tag():
    hit = {}
    for c in A.CASES:
        for t in A.path_tags(c, "lpt"):
            hit.setdefault(t, c.name)
    for env, names in A.CHILD_SETS.values():
        for n in names:
            for t in A.path_tags(A.BY_NAME[n], A.sched_of(env)):
                hit.setdefault(t, n)
    for t in A.PATH_TAGS:
        print(f"PATH {t}: {hit.get(t)}")
    assert set(hit) <= set(A.PATH_TAGS), set(hit) - set(A.PATH_TAGS)
    assert not [t for t in A.PATH_TAGS if t not in hit]
    # the paired schedules see odd and even item counts, and B * nh (and B * nkv) with and
    # without a remainder mod 8
    child = [A.BY_NAME[n] for n in A.CHILD_CASES]
    assert {-(-c.S // 64) % 2 for c in child} == {0, 1}
    assert {t for c in child for t in A.path_tags(c, "pair-xcd")} >= {"pair-it1", "pair-middle", "xcd-rem", "xcd-even"}


def test_case_lists_hold_the_shapes_the_issue_names():
    cs = A.CASES
    assert {c.S for c in cs} >= {1, 33, 64, 65, 129, 200, 320} and max(c.S for c in cs) <= 320
    assert {c.B * c.nh for c in cs} >= {3, 8, 9} and max(c.B * c.nh for c in cs) <= 9
    assert {c.hd for c in cs} == {64, 128}
    assert any(c.nkv == c.nh for c in cs) and any(c.nkv and c.nkv * 2 == c.nh for c in cs)
    assert any(c.nkv == 1 and c.nh > 1 for c in cs) and any(c.nkv == 0 for c in cs)
    assert {c.packed for c in cs} == {True, False}
    assert {c.bounds[1] for c in cs if c.bounds and c.bounds[0] == "win"} >= {1, 31, 64, 65}
    assert any(c.bounds and c.bounds[0] == "docwin" for c in cs)
    assert {c.family for c in cs} == {"gauss", "flat", "steep_under", "steep_over", "big"}
    assert {(c.family, c.dtype) for c in cs} >= {(f, d) for f in ("steep_under", "steep_over") for d in (A.BF, A.HF)}


def test_fixed_inputs_are_what_they_say():
    # flat: every score exactly zero; steep: the running max grows by just under / over 2^8 per tile
    c = A.EXTRA_CASES[0]
    inp = A.attn_inputs(c)
    assert not torch.matmul(inp.q.double(), inp.k.double().transpose(-1, -2)).any()
    assert inp.q.double().abs().sum() > 0 and inp.k.double().abs().sum() > 0
    for fam, dt in itertools.product(("steep_under", "steep_over"), (A.BF, A.HF)):
        c = next(x for x in A.CASES if x.family == fam and x.dtype == dt and not x.bounds and x.S >= 129)
        inp = A.attn_inputs(c)
        s = torch.matmul(inp.q.double(), inp.k.double().transpose(-1, -2)) * A.f32(inp.scale) * A.LOG2E
        s = s.masked_fill(~A.live_masks(c.B, c.S)[0], -math.inf)
        tile_max = torch.stack([s[..., c.S - 1, t * 64:(t + 1) * 64].amax(-1) for t in range(-(-c.S // 64))], -1)
        grow = (tile_max[..., 1:-1] - tile_max[..., :-2])
        assert ((grow < 8.0) if fam == "steep_under" else (grow > 8.0)).all() and (grow - 8.0).abs().max() < 0.5, (fam, grow)
    c = next(x for x in A.CASES if x.family == "big" and x.S >= 129)
    inp = A.attn_inputs(c)
    smax = (torch.matmul(inp.q.double(), inp.k.double().transpose(-1, -2)) * inp.scale).abs().max().item()
    assert 40.0 < smax < 90.0, smax
