"""What tests/gemm_ref.py claims, checked without a GPU: every planted defect falls outside the
tolerance at a case the GPU file runs, the clean references stay inside their own tolerances
after the final rounding and against fp32 emulations that sum in other orders, the ``int``
family's exactness bound holds, no case masks an element, and the chosen cases reach every
branch of the dispatch model.  ``pytest -s`` shows the ratios."""
import math

import pytest
import torch

from tests import gemm_ref as R
from tests.stream_ref import BF, DTYPES, F32, F64, HF

INF = torch.tensor(math.inf, dtype=F64)
ALL_GEMM = R.GB_CASES + R.FW4_CASES
ALL_FUSED = R.ROPE_CASES + R.GU_CASES + R.FW4_SW_CASES + R.DOWN_CASES
ALL_WGRAD = R.WG_CASES + R.SK_CASES
RUN_BY_GPU = set(ALL_GEMM) | set(ALL_FUSED) | set(ALL_WGRAD) | set(R.LD_CASES)


def ratio(out, chk, dt) -> float:
    """Worst err / tol against ``chk``; where the tolerance is zero the output must be
    round_to(ref) bit for bit (anything else, and any NaN, counts as inf)."""
    out = out.double().reshape(chk.ref.shape)
    want = torch.where(chk.tol == 0, R.round_to(chk.ref, dt).double(), chk.ref)
    err = (out - want).abs()
    r = torch.where(chk.tol > 0, err / chk.tol, torch.where(err > 0, INF, err))
    return torch.where(torch.isnan(r), INF, r).max().item()


def outputs(c):
    """{output name: (Checked, format)} of a case."""
    if isinstance(c, R.Gemm):
        return {"c": (R.gemm_case(c)[2], c.dt)}
    if isinstance(c, R.Wgrad):
        return {"dw": (R.wgrad_case(c)[3], F32)}
    ref = R.fused_case(c)[1]
    if c.kernel == "qkv_rope":
        return {"qkv": (ref, c.dt)}
    if c.kernel == "down_swiglu_bwd":
        return {"dgu": (ref.dgu, c.dt), "s": (ref.s, c.dt)}
    return {"gu": (ref.gu, c.dt), "s": (ref.s, c.dt)}


def planted(c, defect):
    """{output name: fp64 value} of the reference with ``defect`` planted."""
    if defect == "ld_ignored":
        return {"c": R.ld_defect_ref(c).ref}
    if isinstance(c, R.Gemm):
        P, Q, _ = R.gemm_case(c)
        if c.kernel == "gemm_fw4":
            walk, bn = R.fw4_walk(c.M, c.N, 0), 256
        else:
            bn = R.gb_bn(c.N)
            walk = R.gb_walk(c.M, c.N, R.GB_DEFAULT_FLAGS, c.cap)[1]
        return {"c": R.gemm_ref(P, Q, c.family, defect, walk, bn).ref}
    if isinstance(c, R.Wgrad):
        dy, x, base = R.wgrad_inputs(c)
        pl = R.sk_plan(c.T, c.Nr, c.Nc, c.splits) if c.sk else None
        s = 1 if c.sk else R.wgrad_splits(c.T, c.Nr, c.Nc, c.splits)
        return {"dw": R.wgrad_ref(dy, x, base, c.family, defect=defect, splits=s, plan=pl).ref}
    inp = R.fused_case(c)[0]
    if c.kernel == "qkv_rope":
        return {"qkv": R.qkv_rope_ref(*inp[:2], c.S, *inp[2:], c.family, defect).ref}
    if c.kernel == "down_swiglu_bwd":
        r = R.down_swiglu_bwd_ref(*inp, c.family, defect)
        return {"dgu": r.dgu.ref, "s": r.s.ref}
    r = R.gu_swiglu_ref(*inp, c.family, defect)
    return {"gu": r.gu.ref, "s": r.s.ref}


def test_case_lists_hold_no_duplicates():
    """Every shape runs gauss and int in both formats, once each."""
    for lst in (R.GB_CASES, R.FW4_CASES, R.LD_CASES, R.ROPE_CASES, R.GU_CASES, R.FW4_SW_CASES, R.DOWN_CASES, R.WG_CASES,
                R.SK_CASES):
        assert len(set(lst)) == len(lst) and len({c.name for c in lst}) == len(lst)
    both = lambda cases, key: all({(c.dt, c.family) for c in cases if key(c) == k} >= {(d, f) for d in DTYPES for f in ("gauss", "int")}
                                  for k in {key(c) for c in cases if c.family != "cancel"})
    assert both(R.GB_CASES, lambda c: (c.kernel, c.M, c.N, c.K)) and both(R.FW4_CASES, lambda c: (c.M, c.N, c.K))
    assert both(R.WG_CASES, lambda c: (c.T, c.Nr, c.Nc, c.splits)) and both(R.SK_CASES, lambda c: (c.T, c.Nr, c.Nc, c.splits))
    assert both(R.FW4_SW_CASES, lambda c: (c.M, c.a, c.K)) and both(R.DOWN_CASES, lambda c: (c.M, c.a, c.K))


# ------------------------------------------------------------------------------ defects
def test_every_defect_has_a_case():
    shown = {k.split("@")[0] for k in R.DEFECT_CASES} | {"trunc_final"}
    assert shown == set(R.DEFECTS)
    for name, (c, _) in R.DEFECT_CASES.items():
        assert c in RUN_BY_GPU, f"{name}: {c.name} is not a case the GPU file runs"
    assert all(c in RUN_BY_GPU and c.family == "gauss" for c in R.TRUNC_CASES)


@pytest.mark.parametrize("name", list(R.DEFECT_CASES))
def test_defect_falls_outside(name):
    c, outs = R.DEFECT_CASES[name]
    want = R.ld_case(c)[2] if name.startswith("ld_ignored") else None
    got = planted(c, name.split("@")[0])
    for o in outs:
        chk, dt = ({"c": (want, c.dt)} if want is not None else outputs(c))[o]
        r = ratio(R.round_to(got[o], dt), chk, dt)
        print(f"DEFECT {name} {c.name} {o} {r:.1f}")
        assert r > 2.0, f"{name}: {o} of {c.name} stays within {r:.2f} tolerances"


@pytest.mark.parametrize("c", R.TRUNC_CASES, ids=lambda c: c.name)
def test_truncation_shows_in_the_bias(c):
    """A store that cuts instead of rounding stays inside every element's tolerance (it is off by
    under one ulp) and is caught by the sign of its errors alone."""
    chk = R.gemm_case(c)[2]
    cut, rnd = R.trunc_to(chk.ref, c.dt), R.round_to(chk.ref, c.dt)
    b_cut, b_rnd = R.bias_ratio(cut, chk), R.bias_ratio(rnd, chk)
    print(f"BIAS {c.name} truncated {b_cut:.2f} rounded {b_rnd:.4f}")
    assert b_cut > 2.0 and b_rnd < 0.5


# -------------------------------------------------------------- the clean references
def acc32(P, Q, order: str):
    """P Q^T accumulated in fp32 over chunks of 32 (one MFMA each): ``rev`` adds the chunks last
    to first, ``pair`` adds them pairwise."""
    Pf, Qf = P.float(), Q.float()
    parts = [Pf[:, i:i + 32] @ Qf[:, i:i + 32].t() for i in range(0, P.shape[1], 32)]
    if order == "rev":
        acc = torch.zeros_like(parts[0])
        for p in reversed(parts):
            acc = acc + p
        return acc
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def _emulate(c, order):
    """{output: tensor in its storage format} of a plain fp32 evaluation of the case."""
    if isinstance(c, R.Gemm):
        P, Q, _ = R.gemm_case(c)
        return {"c": acc32(P, Q, order).to(c.dt)}
    if isinstance(c, R.Wgrad):
        dy, x, base, _ = R.wgrad_case(c)
        n = 1 if c.sk else R.wgrad_splits(c.T, c.Nr, c.Nc, c.splits)
        dw = base.clone()
        for p0, p1 in (R.split_pairs(c.T, n) if order == "rev" else reversed(R.split_pairs(c.T, n))):
            dw = dw + acc32(dy[p0 * 128:p1 * 128].t(), x[p0 * 128:p1 * 128].t(), order)
        return {"dw": dw}
    inp = R.fused_case(c)[0]
    dt = c.dt
    if c.kernel == "qkv_rope":
        x, w, cos, sin = inp
        M, N = x.shape[0], w.shape[0]
        y = acc32(x, w, order).to(dt).float().view(M, N // 64, 64)
        nrot = 2 * (N // 3) // 64
        cs, sn = (t[torch.arange(M) % c.S].view(M, 1, 32) for t in (cos, sin))
        x1, x2 = y[:, :nrot, :32].clone(), y[:, :nrot, 32:].clone()
        y[:, :nrot, :32], y[:, :nrot, 32:] = x1 * cs - x2 * sn, x2 * cs + x1 * sn
        return {"qkv": y.view(M, N).to(dt)}
    if c.kernel == "down_swiglu_bwd":
        dd, wd, gu = inp
        d = acc32(dd, wd.t(), order).to(dt).float()
        g, u = gu.float()[:, :c.a], gu.float()[:, c.a:]
        sg = torch.sigmoid(g)
        return {"dgu": torch.cat([d * u * sg * (1 + g * (1 - sg)), d * g * sg], 1).to(dt), "s": (g * sg * u).to(dt)}
    x, w = inp
    gu = acc32(x, w, order).to(dt)
    g, u = gu.float()[:, :c.a], gu.float()[:, c.a:]
    return {"gu": gu, "s": (g * torch.sigmoid(g) * u).to(dt)}


SMALL = [c for c in ALL_GEMM + ALL_FUSED + ALL_WGRAD if not (isinstance(c, R.Gemm) and c.M * c.N > 2 ** 21)]
LARGE = [c for c in ALL_GEMM if c not in SMALL]


@pytest.mark.parametrize("c", SMALL + LARGE[:2], ids=lambda c: c.name)
def test_clean_reference_inside_its_tolerance(c):
    """After round_to, and for two fp32 evaluations in other summation orders: the bound is not too
    tight for a correct kernel.  On ``int`` the zero tolerance makes this a check of exactness."""
    for o, (chk, dt) in outputs(c).items():
        assert torch.isfinite(chk.ref).all() and torch.isfinite(chk.tol).all() and (chk.tol >= 0).all()
        r0 = ratio(R.round_to(chk.ref, dt), chk, dt)
        assert r0 <= 1.0, f"{c.name} {o}: round_to(ref) at {r0:.3f}"
    for order in ("rev", "pair"):
        got = _emulate(c, order)
        for o, (chk, dt) in outputs(c).items():
            r = ratio(got[o], chk, dt)
            print(f"EMUL {c.name} {o} {order} {r:.4f}")
            assert r <= 1.0, f"{c.name} {o}: a correct fp32 evaluation ({order}) at {r:.3f} tolerances"


def test_partials_and_splitk_references():
    c = R.Wgrad(BF, 384, 256, 192, 2, "gauss")
    dy, x, base, chk = R.wgrad_case(c)
    parts = R.wgrad_parts_ref(dy, x, c.family, 2)
    total = R.splitk_ref(parts.ref.float(), base)
    assert ratio(total.ref.float(), chk, F32) <= 1.0
    for dt in DTYPES:
        p = R.tie_partials(dt)
        s = p.double().sum(0)
        up, dn = R.round_to(s + s.abs() * 2.0 ** -20, dt), R.round_to(s - s.abs() * 2.0 ** -20, dt)
        tie = R.bits(up) != R.bits(dn)
        assert tie.sum() >= p.shape[1] // 4  # a third of the columns sit exactly on a tie


# ---------------------------------------------------------------------- int exactness
@pytest.mark.parametrize("c", [c for c in ALL_GEMM + ALL_FUSED + ALL_WGRAD if c.family == "int"], ids=lambda c: c.name)
def test_int_family_is_exact(c):
    """Every partial sum of every route stays below 2^24: the sum of absolute terms bounds them all."""
    if isinstance(c, R.Wgrad):
        dy, x, base = R.wgrad_inputs(c)
        bound = (dy.double().abs().t() @ x.double().abs() + base.double().abs()).max().item()
        red, ops = c.T, (dy, x)
    else:
        inp = R.gemm_case(c)[:2] if isinstance(c, R.Gemm) else R.fused_case(c)[0][:2]
        P, Q = (inp[0], inp[1].t()) if getattr(c, "kernel", "") == "down_swiglu_bwd" else inp
        bound = (P.double().abs() @ Q.double().abs().t()).max().item()
        red, ops = P.shape[1], (P, Q)
    r = R.int_range(red, R.INT_BASE)
    assert bound < R.EXACT and red * r * r + R.INT_BASE < R.EXACT
    for t in ops:
        assert torch.equal(t.double(), t.double().round()) and t.double().abs().max() <= r
    for o, (chk, dt) in outputs(c).items():
        if o in ("c", "dw", "gu"):  # the product alone: zero tolerance everywhere
            assert (chk.tol == 0).all()
            assert torch.equal(chk.ref, chk.ref.round())


def test_nothing_is_masked():
    """No element is left out: every reference is finite and, with its tolerance, inside the
    output format's range (the masked share is zero)."""
    for c in ALL_GEMM + ALL_FUSED + ALL_WGRAD:
        for o, (chk, dt) in outputs(c).items():
            top = (chk.ref.abs() + chk.tol).max().item()
            assert top < {HF: 65504.0, BF: 3.3e38, F32: 3.4e38}[dt], f"{c.name} {o}: {top}"


# --------------------------------------------------------------------- dispatch model
def test_gemm_bf16_walk_reaches_every_branch():
    tags = set()
    for M, N, K, cap in R.GB_SHAPES:
        for fl in R.gb_flag_sets():
            mode, wgs = R.gb_walk(M, N, fl, cap)
            assert R.walk_covers(M, N, wgs, R.gb_bn(N)), (M, N, fl)
            assert len(wgs) == R.gb_launch_grid((M // 256) * (N // R.gb_bn(N)), fl | ((cap // 8) << 16)) and len(wgs) % 8 == 0
            tags |= R.gb_tags(M, N, K, fl, cap)
    assert tags >= set(R.GB_MODES) | set(R.GB_WALK_TAGS) | {"bn192", "bn128"}, tags
    # the cases the issue names
    assert R.gb_tags(256, 192, 128, R.GB_DEFAULT_FLAGS) >= {"idle-workgroup", "one-pass", "row-major"}
    assert [len(w) for w in R.gb_walk(256, 192, R.GB_DEFAULT_FLAGS)[1]] == [1] + [0] * 7
    assert sorted(len(w) for w in R.gb_walk(768, 768, R.GB_DEFAULT_FLAGS, 8)[1]) == [1] * 4 + [2] * 4
    mode, wgs = R.gb_walk(2048, 384, R.GB_DEFAULT_FLAGS, 8)
    assert mode == "xband" and all(len(w) == 2 for w in wgs)
    mode, wgs = R.gb_walk(*R.GB_BIG[:2], R.GB_DEFAULT_FLAGS)
    assert mode == "grouped" and len(wgs) == 256 and sum(len(w) for w in wgs) == 384
    # the fused forms: heads that straddle the 192-column tiles; 96-row tile stride of the SwiGLU forward
    for c in R.ROPE_CASES:
        assert R.walk_covers(c.M, 3 * c.a * 64, R.gb_walk(c.M, 3 * c.a * 64, R.GB_DEFAULT_FLAGS)[1], 192)
    assert {(3 * c.a * 64 // 192) for c in R.ROPE_CASES} == {1, 3, 4} and {c.M // c.S for c in R.ROPE_CASES} == {2, 4}
    assert {c.a // 96 for c in R.GU_CASES} == {1, 2}
    assert {fl & 4096 for fl in R.gb_flag_sets(late=True)} == {0, 4096}


def test_wgrad_plans_reach_every_branch():
    seen = set()
    for T, Nr, Nc, s in R.WG_SHAPES:
        n = R.wgrad_splits(T, Nr, Nc, s)
        pr = R.split_pairs(T, n)
        assert pr[0][0] == 0 and pr[-1][1] == T // 128 and all(a[1] == b[0] for a, b in zip(pr, pr[1:]))
        seen |= {f"bn{R.wgrad_bn(Nc)}", "half-tile-only" if Nr == 128 else "half-tile" if Nr % 256 else "whole-rows",
                 "one-split" if n == 1 else "splits", "clamped" if s > T // 128 else "", "auto" if s == 0 else "",
                 "uneven" if len({b - a for a, b in pr}) > 1 else "", f"ntc{Nc // R.wgrad_bn(Nc)}"}
    assert seen >= {"bn192", "bn128", "half-tile-only", "half-tile", "whole-rows", "one-split", "splits", "clamped",
                    "auto", "uneven", "ntc1", "ntc2"}, seen
    assert R.wgrad_splits(128, 256, 192, 4) == 1 and R.wgrad_splits(640, 256, 192, 0) == 5
    kinds = set()
    for T, Nr, Nc, g in R.SK_SHAPES:
        pl = R.sk_plan(T, Nr, Nc, g)
        segs = R.sk_segments(pl)
        assert sum(p1 - p0 for sh in segs for _, p0, p1, _ in sh) == pl.Wc and all(len(sh) <= pl.maxseg for sh in segs)
        kinds |= R.sk_kinds(pl)
    assert kinds == set(R.SK_KINDS), kinds
    assert {(T, Nr) for T, Nr, _, _ in R.SK_SHAPES} >= {(256, 384), (256, 512), (384, 384), (384, 512)}


def test_fw4_plans_reach_every_branch():
    seen = set()
    for M, N, K in R.FW4_SHAPES:
        tiles = (M // 256) * ((N + 255) // 256)
        for fl in R.FW4_FLAGS + (R.FW4_TWO if tiles % 16 == 0 else ()):
            T, order, ragged, sched = R.fw4_plan(M, N, fl)
            w = R.fw4_walk(M, N, fl)
            assert sorted(t for g in w for t in g) == [(a, b) for a in range(M // 256) for b in range((N + 255) // 256)]
            seen |= {f"T{T}", order, "ragged" if ragged else "whole", f"sched{sched}", "odd-stages" if (K // 64) % 2 else "even-stages"}
        if tiles % 16:
            assert R.fw4_plan(M, N, 4096) is None
    assert seen >= {"T1", "T2", "band", "half-band", "row-major", "ragged", "whole", "sched4", "sched5", "odd-stages", "even-stages"}, seen
    assert R.fw4_plan(256, 128, 16) is None and R.fw4_plan(256, 128, 128) is None and R.fw4_plan(256, 120, 0) is None
