"""Self-checks of tests/stream_ref.py, runnable without a GPU: each reference agrees with an
independent fp64 oracle, the tolerances admit a plain fp32 computation of the same operation,
every planted defect falls outside them at the very inputs the GPU tests use, and the GPU
case lists reach every launch variant according to the model of the launchers' dispatch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_llm_trainer_amd.ops import rng
from tests import stream_ref as R

BF, HF, F32, F64 = R.BF, R.HF, R.F32, R.F64
ALL_CE = R.CE_CASES + R.CE_CASES_512 + R.CE_CASES_PLAIN


def _miss(out, chk):
    """Elements of ``out`` outside the tolerance (a NaN misses)."""
    return ~((out.double() - chk.ref).abs() <= chk.tol)


def _inside(name, out, chk):
    err = (out.double() - chk.ref).abs()
    bad = ~(err <= chk.tol)
    assert not bad.any(), f"{name}: err/tol = {torch.where(chk.tol > 0, err / chk.tol, err).max().item():.3f}"


def _as_kernel(x, dtype):
    """A defective kernel's output: its fp64 value rounded as the kernel rounds it."""
    return R.round_to(x, dtype).double()


def _ce(case, **kw):
    _, dt, Vp, V, kind, nv_mode, gscale = case
    inp = R.ce_inputs(dt, Vp, V, kind)
    return inp, R.ce_ref(inp.logits, inp.targets, V, R.ce_n_valid(inp, nv_mode), gscale, **kw)


# ---------------------------------------------------------------------------- cross-entropy
@pytest.mark.parametrize("case", [c for c in ALL_CE if c[2] <= 8192], ids=lambda c: c[0])
def test_ce_ref_against_autograd(case):
    _, dt, Vp, V, kind, nv_mode, gscale = case
    inp, ref = _ce(case)
    n = max(R.ce_n_valid(inp, nv_mode), 1)
    x = inp.logits.double()[:, :V].clone().requires_grad_(True)
    rows = F.cross_entropy(x, inp.targets, ignore_index=-100, reduction="none")
    (F.cross_entropy(x, inp.targets, ignore_index=-100, reduction="sum") / n * gscale).backward()
    torch.testing.assert_close(ref.loss.ref, rows.detach(), rtol=1e-12, atol=1e-9)
    torch.testing.assert_close(ref.grad.ref[:, :V], x.grad, rtol=1e-9, atol=1e-14 * gscale)  # softmax - 1 cancels at a spike
    assert not ref.grad.ref[:, V:].any() and not ref.grad.ref[inp.targets == -100].any()
    assert not ref.grad.tol[:, V:].any() and not ref.loss.tol[inp.targets == -100].any()


def _ce32(logits16, targets, V, n_valid, gscale):
    """A plain fp32 cross-entropy with the gradient rounded to the logits' format."""
    x = logits16.float()[:, :V]
    lse = torch.logsumexp(x, dim=1, keepdim=True)
    valid = (targets != -100).unsqueeze(1)
    tgt = targets.clamp(min=0).unsqueeze(1)
    loss = torch.where(valid, lse - x.gather(1, tgt), torch.zeros_like(lse)).squeeze(1)
    g = torch.exp(x - lse)
    g.scatter_add_(1, tgt, -torch.ones_like(lse))
    g = g * (valid * np.float32(gscale) / np.float32(max(n_valid, 1)))
    out = torch.zeros_like(logits16)
    out[:, :V] = g.to(logits16.dtype)
    return loss, out


@pytest.mark.parametrize("case", ALL_CE, ids=lambda c: c[0])
def test_ce_tolerance_and_defects(case):
    _, dt, Vp, V, kind, nv_mode, gscale = case
    for wide in (True, False):
        inp, ref = _ce(case, wide=wide)
        loss32, grad32 = _ce32(inp.logits, inp.targets, V, R.ce_n_valid(inp, nv_mode), gscale)
        _inside("fp32 loss", loss32, ref.loss)
        _inside("fp32 grad", grad32, ref.grad)
    inp, ref = _ce(case)
    live = inp.targets != -100

    def bad(defect, **kw):
        b = _ce(case, defect=defect, **kw)[1]
        return _miss(b.loss.ref, ref.loss), _miss(_as_kernel(b.grad.ref, dt), ref.grad)

    # the padding holds +40: a sum that runs over it shows on every row whose maximum is lower (all
    # base rows, the bottom rows of the large case; the +-6e4 rows of the ceiling case cannot show it);
    # a maximum taken over it shows only where it pushes the row's exponentials under the fp32 range
    low = live & (inp.logits.float()[:, :V].amax(dim=1) < 30)
    if V < Vp and kind != "ceil":
        ml, mg = bad("sum_nomask")
        assert low.any() and ml[low].all() and mg[low].any(dim=1).all(), "sum over the padding stays inside"
        if kind == "large":
            assert bad("max_nomask")[0][low].all(), "maximum over the padding stays inside"
    for r, col in enumerate(inp.spikes):  # the chunk of every boundary: the row whose spike it holds
        if live[r]:
            ml, mg = bad("drop_chunk", chunk=col // 8)
            assert ml[r] and mg[r].any(), f"dropped chunk {col // 8} stays inside"
    ml, mg = bad("patch_wrong_elem")
    assert mg[live].any(dim=1).all(), "target patch on the wrong element stays inside"
    assert bad("ignored_row_grad")[1][~live].any(dim=1).all(), "gradient on an ignored row stays inside"
    if nv_mode != "true":
        assert bad("recount_n_valid")[1][live].any(), "recounted n_valid stays inside"
    if gscale != 1.0:
        assert bad("drop_grad_scale")[1][live].any(), "dropped grad_scale stays inside"


def test_ce_cases_show_every_defect_and_variant():
    cases = R.CE_CASES
    assert any(c[4] == "large" and c[3] < c[2] for c in cases)                    # max_nomask
    assert {c[5] for c in cases} == set(R.CE_NV_MODES) and {c[6] for c in cases} == {1.0, 4096.0}
    assert any(c[1] == HF and c[4] == "ceil" for c in cases) and any(c[1] == BF and c[4] == "large" for c in cases)
    assert {(c[2], c[3]) for c in cases if c[4] == "base"} == set(R.CE_SHAPES)
    for dt in R.DTYPES:
        seen = {R.ce_variant(c[2]) for c in R.CE_CASES if c[1] == dt}
        seen |= {R.ce_variant(c[2], wide=False, nt=False) for c in R.CE_CASES_512 if c[1] == dt}
        seen |= {R.ce_variant(c[2], nt=False) for c in R.CE_CASES_PLAIN if c[1] == dt}
        assert seen == set(R.CE_VARIANTS), sorted(set(R.CE_VARIANTS) - seen)
        # the shapes this file exists for: 512 x 16 and the two-pass kernel under the default knobs
        assert {"512x16", "two-pass"} <= {R.ce_variant(c[2]) for c in R.CE_CASES if c[1] == dt}
    assert R.ce_variant(57344) == "1024x7 NT" and R.ce_variant(57352) == "512x16"
    assert R.ce_variant(65536) == "512x16" and R.ce_variant(65544) == "two-pass"
    for c in ALL_CE:
        inp = R.ce_inputs(c[1], c[2], c[3], c[4])
        assert inp.targets[-1] == -100 and (inp.targets == -100).sum() == 2 and len(inp.spikes) <= 64
        t = inp.targets[inp.targets != -100]
        assert (t >= 0).all() and (t < c[3]).all()
        assert (inp.logits[:, c[3]:].float() == 40.0).all()


# --------------------------------------------------------------------------------- RMSNorm
def _fwd(case, **kw):
    _, dt, M, H, which, p, w16 = case
    inp = R.norm_fwd_inputs(dt, M, H, which, p, w16)
    return inp, R.rmsnorm_fwd_ref(inp.resid, inp.delta, inp.w, R.EPS, p, inp.key, out_dtype=dt, **kw)


def _bwd(case, **kw):
    _, dt, M, H, dres, p, w16, scaled, dw_start, want_dd = case
    inp = R.norm_bwd_inputs(dt, M, H, dres, p, w16, scaled, dw_start)
    return inp, R.rmsnorm_bwd_ref(inp.dy, inp.x, inp.rstd, inp.w, inp.dres, inp.dw0, p, inp.key, inp.dy_scale,
                                  inp.dy_mul, **kw)


def _keep(M, H, p, key):
    return rng.keep_mask((M, H), key, p).double() / (1.0 - p) if rng.keep_threshold(p) else torch.ones(M, H, dtype=F64)


@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: c[0])
def test_norm_fwd_reference_tolerance_and_defects(case):
    _, dt, M, H, which, p, w16 = case
    inp, ref = _fwd(case)
    # oracle: torch's own rms_norm in fp64 on the masked add
    x = torch.zeros(M, H, dtype=F64)
    if inp.resid is not None:
        x = x + inp.resid.double()
    if inp.delta is not None:
        x = x + inp.delta.double() * _keep(M, H, p, inp.key)
    torch.testing.assert_close(ref.x.ref, x, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(ref.y.ref, F.rms_norm(x, (H,), inp.w.double(), R.EPS), rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(ref.rstd.ref, 1.0 / torch.sqrt(x.pow(2).mean(dim=1) + R.EPS), rtol=1e-13, atol=0)
    # a plain fp32 computation stays inside
    x32 = torch.zeros(M, H)
    if inp.resid is not None:
        x32 = x32 + inp.resid
    if inp.delta is not None:
        x32 = x32 + inp.delta.float() * _keep(M, H, p, inp.key).float()
    rstd32 = torch.rsqrt(x32.pow(2).mean(dim=1) + np.float32(R.EPS))
    _inside("fp32 x", x32, ref.x)
    _inside("fp32 rstd", rstd32, ref.rstd)
    _inside("fp32 y", (x32 * rstd32.unsqueeze(1) * inp.w.float()).to(dt), ref.y)
    if H % 256 and H > 256:
        b = _fwd(case, defect="drop_last_chunk")[1]  # four columns of 3076 move y by less than a bf16 ulp: rstd shows it
        assert _miss(b.rstd.ref, ref.rstd).all(), "a row sum without its last chunk stays inside"
    if R.nch_of(H) * 256 != H:
        b = _fwd(case, defect="mean_nch256")[1]
        assert _miss(b.rstd.ref, ref.rstd).all(), "a mean over NCH * 256 columns stays inside"


@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: c[0])
def test_norm_bwd_reference_tolerance_and_defects(case):
    _, dt, M, H, dres, p, w16, scaled, dw_start, want_dd = case
    inp, ref = _bwd(case)
    # oracle: autograd through a plain fp64 RMSNorm.  The kernel takes rstd as stored (fp32 of an
    # fp32 row sum), so the oracle's own rstd is swapped for it by a straight-through factor.
    sc = (float(inp.dy_scale) if scaled else 1.0) * R.f32(inp.dy_mul)
    x = inp.x.double().requires_grad_(True)
    w = inp.w.double().requires_grad_(True)
    r_own = torch.rsqrt(x.pow(2).mean(dim=1, keepdim=True) + R.EPS)
    fix = (inp.rstd.double().unsqueeze(1) / r_own).detach()
    y = x * (r_own * fix) * w
    (y * inp.dy.double() * sc).sum().backward()
    # d rstd / d x of the oracle is -x r^3 / H with r its own rstd: the reference uses the stored
    # one throughout, so the two agree to the fp32 rounding of rstd, not to fp64
    dr = inp.dres.double() if dres else 0.0
    torch.testing.assert_close(ref.dx.ref, x.grad + dr, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ref.dw.ref, inp.dw0.double() + w.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref.ddelta.ref, ref.dx.ref * _keep(M, H, p, inp.key), rtol=1e-14, atol=0)
    # a plain fp32 computation stays inside
    d32 = inp.dy.float() * (np.float32(float(inp.dy_scale) if scaled else 1.0) * np.float32(inp.dy_mul))
    xh = inp.x * inp.rstd.unsqueeze(1)
    g = d32 * inp.w.float()
    dx32 = inp.rstd.unsqueeze(1) * (g - xh * ((g * xh).sum(dim=1, keepdim=True) / H))
    if dres:
        dx32 = dx32 + inp.dres
    _inside("fp32 dx", dx32, ref.dx)
    _inside("fp32 ddelta", (dx32 * _keep(M, H, p, inp.key).float()).to(dt), ref.ddelta)
    _inside("fp32 dw", inp.dw0 + (d32 * xh).sum(dim=0), ref.dw)
    if rng.keep_threshold(p):
        b = _bwd(case, defect="no_dropout_scale")[1]
        assert _miss(_as_kernel(b.ddelta.ref, dt), ref.ddelta).any(dim=1).all(), "missing dropout scale stays inside"
    if dres:
        b = _bwd(case, defect="drop_dres")[1]
        assert _miss(b.dx.ref, ref.dx).any(dim=1).all(), "dropped dres stays inside"
    nb = R.norm_blocks(M)
    for blk in sorted({0, nb // 2, nb - 1}):
        b = _bwd(case, defect="drop_block_partial", block=blk)[1]
        assert _miss(b.dw.ref, ref.dw).any(), f"missing partial of block {blk} stays inside"


def test_norm_cases_reach_every_variant():
    assert {R.nch_of(c[3]) for c in R.FWD_CASES} == set(R.NCH_SET)
    assert {R.nch_of(c[3]) for c in R.BWD_CASES if c[2] == 9} == set(R.NCH_SET)
    assert {c[3] for c in R.FWD_CASES} == set(R.FWD_H) == {c[3] for c in R.BWD_CASES if c[2] == 9}
    assert [R.nch_of(h) for h in (4, 256, 260, 2048, 2052, 3072, 3076, 4096)] == [1, 1, 2, 8, 12, 12, 16, 16]
    for dt in R.DTYPES:
        mine = [c for c in R.FWD_CASES if c[1] == dt]
        assert {c[2] for c in mine} == {1, 7} and {c[4] for c in mine} == {"resid", "delta", "both"}
        assert {c[6] for c in mine} == {False, True}
        assert {c[5] for c in mine if c[4] != "resid"} == {0.0, 0.1}
    paths = {c[0]: R.colsum_paths(R.norm_blocks(c[2])) for c in R.BWD_CASES}
    assert paths["bf16-M2800-H260"] == {"unrolled", "tail"} and R.norm_blocks(2800) == 700
    assert R.colsum_paths(448) == {"tail"} and R.colsum_paths(449) == {"unrolled", "tail"}
    assert R.colsum_paths(1023) == {"unrolled", "tail"} and R.colsum_paths(1024) == {"unrolled"}
    assert R.norm_blocks(4101) == 1024 and 4101 % 4  # the grid-stride row loop, a ragged last block
    b = R.BWD_CASES
    assert {c[4] for c in b} == {False, True} and {c[9] for c in b} == {False, True}      # dres, want_ddelta
    assert {c[7] for c in b} == {False, True} and {c[8] for c in b} == {False, True}      # scales, dweight start
    assert {c[5] for c in b} == {0.0, 0.1} and {c[6] for c in b} == {False, True}


# ----------------------------------------------------------------------------------- AdamW
def test_adamw_ref_against_torch():
    n, lr, b1, b2, eps, wd = 257, 1e-3, 0.9, 0.95, 1e-8, 0.1
    g_ = torch.Generator().manual_seed(3)
    p = torch.randn(n, generator=g_, dtype=F64)
    tp = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    m, v = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in (1, 2, 3):
        g = torch.randn(n, generator=g_, dtype=F64)
        r = R.adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, None, round_scalars=False)
        p, m, v = r.p.ref, r.m.ref, r.v.ref
        tp.grad = g.clone()
        opt.step()
        torch.testing.assert_close(p, tp.detach(), rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(m, opt.state[tp]["exp_avg"], rtol=1e-13, atol=1e-18)
        torch.testing.assert_close(v, opt.state[tp]["exp_avg_sq"], rtol=1e-13, atol=1e-18)


def _adam32(inp, wd, step):
    """torch.optim.AdamW's arithmetic in plain fp32 tensor operations."""
    f = np.float32
    g = inp.g * (inp.gscale[1] if inp.gscale is not None else f(1))
    p = inp.p * (f(1) - f(R.LR) * f(wd))
    m = torch.lerp(inp.m, g, float(f(1) - f(R.B1)))
    v = inp.v * f(R.B2) + (f(1) - f(R.B2)) * g * g
    denom = v.sqrt() * f(1.0 / np.sqrt(1.0 - R.B2 ** step)) + f(R.AEPS)
    return p - f(R.LR / (1.0 - R.B1 ** step)) * m / denom, m, v


# the two largest sizes are walked once, at step 5
@pytest.mark.parametrize("n,combo", [(n, k) for n in R.ADAM_N for k in range(len(R.ADAM_COMBOS))
                                     if k == 1 or n < 8 * R.ADAM_S])
def test_adamw_tolerance_and_defects(n, combo):
    step, wd, with_gs = R.ADAM_COMBOS[combo]
    inp = R.adamw_inputs(n, step, with_gs)
    args = (inp.p, inp.g, inp.m, inp.v, R.LR, R.B1, R.B2, R.AEPS, wd, step, inp.gscale)
    ref = R.adamw_ref(*args)
    p32, m32, v32 = _adam32(inp, wd, step)
    _inside("fp32 p", p32, ref.p)
    _inside("fp32 m", m32, ref.m)
    _inside("fp32 v", v32, ref.v)
    assert (ref.g == inp.g.double()).all() and not R.adamw_ref(*args, zero_grad=True).g.any()
    grp = R.adamw_groups(n)
    nz = inp.g != 0
    for defect, code in (("skip_second", 1), ("skip_remainder", 2), ("skip_tail", 3)):
        sel = (grp == code) & nz
        if sel.any():
            b = R.adamw_ref(*args, defect=defect)
            for name, out, chk in (("p", b.p.ref, ref.p), ("m", b.m.ref, ref.m), ("v", b.v.ref, ref.v)):
                # all but the few elements whose update happens to cancel to under an fp32 ulp
                assert _miss(out.float(), chk)[sel].float().mean() > 0.99, f"{defect}: {name} stays inside"
    if ((grp == 1) & nz).any():
        b = R.adamw_ref(*args, zero_grad=True, defect="zg_second_kept")
        assert b.g[(grp == 1) & nz].all() and not b.g[grp != 1].any()
    if n <= 100003:
        b = R.adamw_ref(*args, defect="bc_step_minus_1")
        assert not nz.any() or _miss(b.p.ref.float(), ref.p)[nz].float().mean() > 0.99, "bias correction with step - 1 stays inside"
        if wd:
            b = R.adamw_ref(*args, defect="coupled_wd")
            assert _miss(b.p.ref.float(), ref.p).any(), "coupled weight decay stays inside"
        b = R.adamw_ref(*args, defect="shadow_pre_update")
        for sdt in R.DTYPES:  # the GPU test asks for the bits of the updated parameter's cast
            moved = R.round_to(ref.p.ref, sdt) != R.round_to(inp.p.double(), sdt)
            assert (R.round_to(b.shadow, sdt) != R.round_to(ref.shadow, sdt))[moved].all() and (moved.any() or n < 4)


def test_adamw_cases_reach_every_path():
    S = R.ADAM_S
    paths = {n: R.adamw_paths(n) for n in R.ADAM_N}
    assert paths[1] == paths[3] == {"tail"} and paths[4] == {"remainder"} and paths[5] == {"remainder", "tail"}
    assert paths[100003] == {"remainder", "tail"}           # what the earlier test reaches
    assert paths[4 * S + 4] == {"pair", "remainder"} and paths[8 * S] == {"pair"}
    assert paths[12 * S + 4 * 777 + 3] == {"pair", "remainder", "tail"}
    assert R.adamw_paths(4 * S) == {"remainder"}            # the pair loop needs more than one pass of the capped grid
    grp = R.adamw_groups(12 * S + 4 * 777 + 3)
    assert [(grp == c).sum().item() for c in range(4)] == [4 * (S + 777), 4 * (S + 777), 4 * (S - 777), 3]
    g8 = R.adamw_groups(8 * S)
    assert (g8[:4 * S] == 0).all() and (g8[4 * S:] == 1).all()
    # the model against a literal walk of the kernel's loop at a small grid
    n4, stride = 2 * 256 * 3 + 100, 256 * 3  # not reachable through flat_blocks; the walk itself
    want = torch.full((n4,), -1)
    for t in range(stride):
        i = t
        while i + stride < n4:
            want[i], want[i + stride] = 0, 1
            i += 2 * stride
        if i < n4:
            want[i] = 2
    q = torch.arange(n4)
    cnt = (n4 - q % stride + stride - 1) // stride
    got = torch.where((q // stride) % 2 == 1, 1, torch.where(q // stride + 1 < cnt, 0, 2))
    assert (got == want).all()
    assert {m for m, _ in R.ADAM_VARIANTS} == {"plain", "zg"} and {s for _, s in R.ADAM_VARIANTS} == {BF, HF, None}
    assert {c[0] for c in R.ADAM_COMBOS} == {1, 5} and {c[1] for c in R.ADAM_COMBOS} == {0.0, 0.1}
    assert {c[2] for c in R.ADAM_COMBOS} == {False, True}
    for step in (1, 5):
        inp = R.adamw_inputs(1027, step, True)
        assert ((inp.g == 0) & (inp.v != 0)).any() or step == 1
        assert ((inp.g != 0) & (inp.v == 0)).any() and ((inp.g == 0) & (inp.v == 0) & (inp.m == 0)).any()
        assert (inp.m != 0).any() == (step == 5)


# ------------------------------------------------------------------ sumsq, clip, casts, add
@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_sumsq_tolerance(n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
    out0 = R.sumsq_out0(n)
    ref = R.sumsq_ref(x, out0)
    _inside("fp32 sumsq", (x * x).sum().reshape(1) + np.float32(out0), ref)
    # one element is under the rounding of a sum of two million: there, a block's share of a pass
    lost = x[-1:] if n <= 1025 else x[-1024:]
    assert _miss(ref.ref - (lost.double() ** 2).sum(), ref).all(), "dropped elements stay inside"
    assert _miss(ref.ref - out0, ref).all(), "an overwritten (not accumulated) out stays inside"


def test_clip_and_cast_tables():
    for ss, nm, mx, sm in ((36.0, 0.5, 1.0, 0.25), (0.01, 0.5, 1.0, 0.25), (36.0, 0.5, 0.0, 0.25), (0.0, 0.5, 1.0, 0.25)):
        ref = R.clip_ref(ss, nm, mx, sm)
        norm = np.sqrt(np.float32(ss)) * np.float32(nm)
        coef = min(np.float32(1), np.float32(mx) / (norm + np.float32(1e-6))) if mx > 0 else np.float32(1)
        _inside("fp32 clip", torch.tensor([norm, coef * np.float32(sm)]), ref)
    assert R.clip_ref(36.0, 0.5, 1.0, 0.25).ref[1] < 0.25 and R.clip_ref(0.01, 0.5, 1.0, 0.25).ref[1] == 0.25
    assert R.clip_ref(36.0, 0.5, 0.0, 0.25).ref[1] == 0.25 and R.clip_ref(0.0, 0.5, 1.0, 0.25).ref.tolist() == [0.0, 0.25]
    x = R.cast_specials()
    assert torch.isnan(x[-1]) and not torch.isnan(x[:-1]).any()
    for dt in R.DTYPES:  # the table holds what it claims for each format
        y = x[:-1].to(dt)
        assert torch.isinf(y).sum() > torch.isinf(x[:-1]).sum() or dt == BF and torch.isinf(y).sum() >= 3
        assert ((y.float() != x[:-1]) & (y != 0) & torch.isfinite(y)).any() and ((y == 0) & (x[:-1] != 0)).any()
        sub = {BF: 2.0 ** -126, HF: 2.0 ** -14}[dt]
        assert ((y != 0) & (y.float().abs() < sub)).any()
