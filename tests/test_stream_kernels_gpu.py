"""Every launch variant of the cross-entropy, RMSNorm and optimizer kernels (ops/csrc/loss.hip,
norm.hip, optim.hip) against the fp64 references and derived tolerances of tests/stream_ref.py:
every element of every output, at the smallest shapes that reach each path, with sentinel
guards around every output buffer the caller owns.

Each numerical check prints ``RATIO <name> <worst err / tol>`` (pytest -s shows them).  The
checks are plain functions, registered in CHECKS by name, so that tests/stream_ref_child.py can
run the same ones in a fresh process under other DLT_* knobs (they are read once per process)."""
import os
import subprocess
import sys
import time

import pytest
import torch

from distributed_llm_trainer_amd.ops import hip
from tests import stream_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF, F32, I64 = R.BF, R.HF, R.F32, R.I64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = os.environ.get("DLT_CE_THREADS", "").strip() != "512"  # as loss.hip reads it
SENT = {BF: 3.0, HF: 3.0, F32: -7.5}  # sentinel fill of the guard zones


def check(name, out, chk):
    ref, tol = chk.ref.to(out.device), chk.tol.to(out.device)
    err = (out.double().reshape(ref.shape) - ref).abs()
    ratio = torch.where(tol > 0, err / tol, err).max().item()
    print(f"RATIO {name} {ratio:.4f}")
    bad = ~(err <= tol)
    assert not bad.any(), (f"{name}: {bad.sum().item()} of {bad.numel()} elements outside the tolerance, "
                           f"worst err/tol {ratio:.3f} at {bad.nonzero()[0].tolist()}")
    return ratio


def same_bits(name, a, b):
    assert torch.equal(R.bits(a), R.bits(b)), f"{name}: two calls on equal inputs differ"


def _d(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------------------------- cross-entropy
def check_ce(name):
    _, dt, Vp, V, kind, nv_mode, gscale = R.CE_BY_NAME[name]
    inp = R.ce_inputs(dt, Vp, V, kind)
    nv = R.ce_n_valid(inp, nv_mode)
    ref = R.ce_ref(inp.logits, inp.targets, V, nv, gscale, wide=WIDE)
    tg, nvt = inp.targets.to(DEV), torch.tensor(nv, device=DEV)
    runs = []
    for _ in range(2):
        G = R.Guarded(inp.logits.shape, dt, SENT[dt], DEV, init=inp.logits)
        loss = hip.cross_entropy_fwd_bwd(G.t, tg, V, nvt, gscale)
        torch.cuda.synchronize()
        G.assert_guards()
        runs.append((loss, G.t))
    tag = f"ce[{R.ce_variant(Vp, WIDE)}] {name}"
    check(tag + " loss", runs[0][0], ref.loss)
    check(tag + " grad", runs[0][1], ref.grad)
    same_bits(tag + " loss", runs[0][0], runs[1][0])
    same_bits(tag + " grad", runs[0][1], runs[1][1])


# --------------------------------------------------------------------------------- RMSNorm
def check_norm_fwd(name):
    _, dt, M, H, which, p, w16 = R.FWD_BY_NAME[name]
    inp = R.norm_fwd_inputs(dt, M, H, which, p, w16)
    ref = R.rmsnorm_fwd_ref(inp.resid, inp.delta, inp.w, R.EPS, p, inp.key, out_dtype=dt)
    Y = R.Guarded((M, H), dt, SENT[dt], DEV)
    x, y, rstd = hip.add_dropout_rmsnorm_fwd(_d(inp.resid), _d(inp.delta), _d(inp.w), R.EPS, p, inp.key,
                                             out_dtype=dt, y_out=Y.t)
    torch.cuda.synchronize()
    Y.assert_guards()
    tag = f"norm_fwd[nch {R.nch_of(H)}] {name}"
    if inp.delta is not None:
        check(tag + " x", x, ref.x)
    check(tag + " rstd", rstd, ref.rstd)
    check(tag + " y", y, ref.y)


def check_norm_bwd(name):
    _, dt, M, H, dres, p, w16, scaled, dw_start, want_dd = R.BWD_BY_NAME[name]
    inp = R.norm_bwd_inputs(dt, M, H, dres, p, w16, scaled, dw_start)
    ref = R.rmsnorm_bwd_ref(inp.dy, inp.x, inp.rstd, inp.w, inp.dres, inp.dw0, p, inp.key, inp.dy_scale, inp.dy_mul)
    dev = [_d(t) for t in (inp.dy, inp.x, inp.rstd, inp.w, inp.dres, inp.dy_scale)]
    runs = []
    for _ in range(2):
        DW = R.Guarded((H,), F32, SENT[F32], DEV, init=inp.dw0)
        DD = R.Guarded((M, H), dt, SENT[dt], DEV) if want_dd else None
        dx, dd = hip.rmsnorm_bwd(dev[0], dev[1], dev[2], dev[3], dev[4], DW.t, p, inp.key, dy_scale=dev[5],
                                 want_ddelta=want_dd, ddelta_out=DD.t if want_dd else None, dy_mul=inp.dy_mul)
        torch.cuda.synchronize()
        DW.assert_guards()
        if want_dd:
            DD.assert_guards()
        else:
            assert dd is None
        runs.append((dx, dd, DW.t))
    tag = f"norm_bwd[nch {R.nch_of(H)}, colsum {'+'.join(sorted(R.colsum_paths(R.norm_blocks(M))))}] {name}"
    check(tag + " dx", runs[0][0], ref.dx)
    if want_dd:
        check(tag + " ddelta", runs[0][1], ref.ddelta)
        same_bits(tag + " ddelta", runs[0][1], runs[1][1])
    check(tag + " dw", runs[0][2], ref.dw)
    same_bits(tag + " dx", runs[0][0], runs[1][0])
    same_bits(tag + " dw", runs[0][2], runs[1][2])


# ----------------------------------------------------------------------------------- AdamW
def check_adamw(n, combo):
    step, wd, with_gs = R.ADAM_COMBOS[combo]
    base = R.adamw_inputs(n, step, with_gs, full=False)  # one period of the inputs: reference and state repeat it
    ref = R.adamw_ref(base.p, base.g, base.m, base.v, R.LR, R.B1, R.B2, R.AEPS, wd, step, base.gscale)
    ref = ref._replace(p=_tiled(ref.p, n), m=_tiled(ref.m, n), v=_tiled(ref.v, n))
    inp = base._replace(p=R.tile(_d(base.p), n), g=R.tile(_d(base.g), n), m=R.tile(_d(base.m), n), v=R.tile(_d(base.v), n))
    gs = _d(inp.gscale)
    for mode, sdt in R.ADAM_VARIANTS:
        P, G, M_, V_ = (R.Guarded((n,), F32, SENT[F32], DEV, init=t) for t in (inp.p, inp.g, inp.m, inp.v))
        S = R.Guarded((n,), sdt, SENT[sdt], DEV) if sdt is not None else None
        hip.adamw_flat(P.t, G.t, M_.t, V_.t, S.t if S else None, R.LR, R.B1, R.B2, R.AEPS, wd, step, gs,
                       zero_grad=mode == "zg")
        torch.cuda.synchronize()
        for b in (P, G, M_, V_) + ((S,) if S else ()):
            b.assert_guards()
        tag = f"adamw[{'+'.join(sorted(R.adamw_paths(n))) or 'none'}] n={n} step={step} {mode}-{R.DT_NAME.get(sdt)}"
        check(tag + " p", P.t, ref.p)
        check(tag + " m", M_.t, ref.m)
        check(tag + " v", V_.t, ref.v)
        if mode == "zg":
            assert not R.bits(G.t).any(), f"{tag}: gradient not bitwise zero"
        else:
            assert torch.equal(R.bits(G.t), R.bits(inp.g)), f"{tag}: gradient changed"
        if S:
            assert torch.equal(R.bits(S.t), R.bits(P.t.to(sdt))), f"{tag}: shadow is not the cast of the updated parameter"


def _tiled(chk, n):
    return R.Checked(R.tile(chk.ref.to(DEV), n), R.tile(chk.tol.to(DEV), n))


# ---------------------------------------------------------------- registry, timing, children
CHECKS = {}
CHECKS.update({f"ce:{c[0]}": (check_ce, (c[0],)) for c in R.CE_CASES + R.CE_CASES_512 + R.CE_CASES_PLAIN})
CHECKS.update({f"fwd:{c[0]}": (check_norm_fwd, (c[0],)) for c in R.FWD_CASES})
CHECKS.update({f"bwd:{c[0]}": (check_norm_bwd, (c[0],)) for c in R.BWD_CASES})
CHECKS.update({f"adamw:{n}:{k}": (check_adamw, (n, k)) for n in R.ADAM_N for k in range(len(R.ADAM_COMBOS))})
ADAM_KEYS = [k for k in CHECKS if k.startswith("adamw:")]
CHILD_SETS = {
    "threads512": ({"DLT_CE_THREADS": "512", "DLT_CE_NT": "0", "DLT_ADAMW_NT": "0", "DLT_FWD_NT": "0",
                    "DLT_COLSUM_WIDE": "1"},
                   [f"ce:{c[0]}" for c in R.CE_CASES_512] + ADAM_KEYS + ["fwd:bf16-H768", "fwd:fp16-H768",
                                                                        "bwd:bf16-M2800-H260", "bwd:fp16-M2800-H260"]),
    "plain": ({"DLT_CE_NT": "0", "DLT_ADAMW_OCC": "0"}, [f"ce:{c[0]}" for c in R.CE_CASES_PLAIN] + ADAM_KEYS),
}
TIMES = {}  # check -> seconds of its first run in this process
CHILD_START = 60.0  # interpreter start, torch import, library load, first HIP call of a fresh process


def run_check(key):
    fn, args = CHECKS[key]
    t0 = time.perf_counter()
    fn(*args)
    TIMES.setdefault(key, time.perf_counter() - t0)


def _keys(prefix, cases):
    return [f"{prefix}:{c[0]}" for c in cases]


@pytest.mark.parametrize("key", _keys("ce", R.CE_CASES))
def test_cross_entropy(key):
    run_check(key)


def test_cross_entropy_rejects():
    tg, nv = torch.zeros(2, dtype=I64, device=DEV), torch.tensor(2, device=DEV)
    with pytest.raises(RuntimeError):  # Vp % 8
        hip.cross_entropy_fwd_bwd(torch.zeros(2, 100, dtype=BF, device=DEV), tg, 90, nv)
    with pytest.raises(RuntimeError):  # V > Vp
        hip.cross_entropy_fwd_bwd(torch.zeros(2, 64, dtype=BF, device=DEV), tg, 65, nv)


@pytest.mark.parametrize("key", _keys("fwd", R.FWD_CASES))
def test_rmsnorm_fwd(key):
    run_check(key)


@pytest.mark.parametrize("H", [770, 4100])
def test_rmsnorm_rejects(H):
    x = torch.zeros(4, H, device=DEV)
    w = torch.ones(H, device=DEV)
    with pytest.raises(RuntimeError):
        hip.add_dropout_rmsnorm_fwd(x, None, w, R.EPS, 0.0, 1)
    with pytest.raises(RuntimeError):
        hip.rmsnorm_bwd(torch.zeros(4, H, dtype=BF, device=DEV), x, torch.ones(4, device=DEV), w, None,
                        torch.zeros(H, device=DEV), 0.0, 1)


@pytest.mark.parametrize("key", _keys("bwd", R.BWD_CASES))
def test_rmsnorm_bwd(key):
    run_check(key)


@pytest.mark.parametrize("key", ADAM_KEYS)
def test_adamw(key):
    run_check(key)


def test_adamw_rejects_misaligned():
    n = 64
    buf = [torch.zeros(n + 4, device=DEV) for _ in range(4)]
    al = [b[:n] for b in buf]
    for k in range(4):  # each of p, g, m, v one element off 16-byte alignment
        args = list(al)
        args[k] = buf[k][1:n + 1]
        with pytest.raises((ValueError, RuntimeError)):
            hip.adamw_flat(*args, None, R.LR, R.B1, R.B2, R.AEPS, 0.0, 1, None)
    torch.cuda.synchronize()
    assert all(not b.any() for b in buf)


def test_adamw_three_steps_vs_torch():
    """Steps 1..3 from zero moments against torch.optim.AdamW on fp64 copies, inside the sum of
    the per-step tolerances.  The hyperparameters are exact in fp32, so that both sides take the
    same ones (lr / bc1 and 1 / sqrt(bc2) still round once: inside the U23 per rounding)."""
    n, lr, b1, b2, eps, wd = 1027, 2.0 ** -10, 0.875, 0.9375, 2.0 ** -27, 0.125
    g_ = torch.Generator().manual_seed(77)
    p0 = torch.randn(n, generator=g_)
    tp = p0.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    P, M_, V_ = (R.Guarded((n,), F32, SENT[F32], DEV, init=t) for t in (p0, torch.zeros(n), torch.zeros(n)))
    tol = [torch.zeros(n, dtype=torch.float64) for _ in range(3)]
    for step in (1, 2, 3):
        g = torch.randn(n, generator=g_)
        st = opt.state[tp]
        m_prev = st["exp_avg"].clone() if st else torch.zeros(n, dtype=torch.float64)
        v_prev = st["exp_avg_sq"].clone() if st else torch.zeros(n, dtype=torch.float64)
        one = R.adamw_ref(tp.detach().clone(), g, m_prev, v_prev, lr, b1, b2, eps, wd, step, None)
        tp.grad = g.double()
        opt.step()
        hip.adamw_flat(P.t, _d(g), M_.t, V_.t, None, lr, b1, b2, eps, wd, step, None)
        torch.cuda.synchronize()
        for i, c in enumerate((one.p, one.m, one.v)):
            tol[i] = tol[i] + c.tol
        st = opt.state[tp]
        check(f"adamw vs torch step {step} p", P.t, R.Checked(tp.detach(), tol[0]))
        check(f"adamw vs torch step {step} m", M_.t, R.Checked(st["exp_avg"], tol[1]))
        check(f"adamw vs torch step {step} v", V_.t, R.Checked(st["exp_avg_sq"], tol[2]))
    for b in (P, M_, V_):
        b.assert_guards()


# ------------------------------------------------------------------ sumsq, clip, casts, add
@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_sumsq(n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
    out0 = R.sumsq_out0(n)
    ref = R.sumsq_ref(x, out0)
    xd = x.to(DEV)
    outs = []
    for _ in range(2):
        O = R.Guarded((1,), F32, SENT[F32], DEV, init=torch.tensor([out0]))
        hip.sumsq(xd, O.t)
        torch.cuda.synchronize()
        O.assert_guards()
        outs.append(O.t)
    check(f"sumsq n={n}", outs[0], ref)
    same_bits(f"sumsq n={n}", outs[0], outs[1])


@pytest.mark.parametrize("name,ss,norm_mul,max_norm,scale_mul", [
    ("above", 36.0, 0.5, 1.0, 0.25), ("below", 0.01, 0.5, 1.0, 0.25), ("disabled", 36.0, 0.5, 0.0, 0.25),
    ("negative-max", 36.0, 2.0, -1.0, 0.5), ("zero-sum", 0.0, 0.5, 1.0, 0.25), ("inexact", 3.0, 1.0 / 3.0, 0.7, 1.0 / 7.0)])
def test_clip_coef(name, ss, norm_mul, max_norm, scale_mul):
    O = R.Guarded((2,), F32, SENT[F32], DEV)
    hip.clip_coef(torch.tensor([ss], device=DEV), O.t, norm_mul, max_norm, scale_mul)
    torch.cuda.synchronize()
    O.assert_guards()
    check(f"clip_coef {name}", O.t, R.clip_ref(ss, norm_mul, max_norm, scale_mul))


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.DT_NAME[d])
@pytest.mark.parametrize("n", R.CAST_N)
def test_cast(n, dt):
    g_ = torch.Generator().manual_seed(n % 1000 + 5)
    x = torch.randn(n, generator=g_) * torch.exp2(torch.randint(-30, 18, (n,), generator=g_).float())
    Y = R.Guarded((n,), dt, SENT[dt], DEV)
    hip.cast_bf16(x.to(DEV), Y.t)
    torch.cuda.synchronize()
    Y.assert_guards()
    assert torch.equal(R.bits(Y.t.cpu()), R.bits(x.to(dt))), f"cast to {dt} n={n}: not the round-to-nearest-even cast"


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.DT_NAME[d])
def test_cast_special_values(dt):
    x = R.cast_specials()
    Y = R.Guarded((x.numel(),), dt, SENT[dt], DEV)
    hip.cast_bf16(x.to(DEV), Y.t)
    torch.cuda.synchronize()
    Y.assert_guards()
    got, want = Y.t.cpu(), x.to(dt)
    assert torch.isnan(x[-1]) and torch.isnan(got[-1])
    diff = (R.bits(got[:-1]) != R.bits(want[:-1])).nonzero().flatten().tolist()
    assert not diff, f"cast to {dt}: {[(x[i].item(), got[i].item(), want[i].item()) for i in diff]}"


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.DT_NAME[d])
@pytest.mark.parametrize("n", R.ADD_N)
def test_add_bf16_into_f32(n, dt):
    g_ = torch.Generator().manual_seed(n)
    dst, src = torch.randn(n, generator=g_), (torch.randn(n, generator=g_) * 4).to(dt)
    D = R.Guarded((n,), F32, SENT[F32], DEV, init=dst)
    assert hip.add_bf16_into_f32(D.t, src.to(DEV))
    torch.cuda.synchronize()
    D.assert_guards()
    check(f"add_{R.DT_NAME[dt]}_into_f32 n={n}", D.t, R.add_ref(dst, src))


# -------------------------------------------------------------------- environment builds
@pytest.mark.parametrize("name", list(CHILD_SETS))
def test_knob_builds_in_a_child(name):
    """The same checks under the other DLT_* builds, in a fresh process (the knobs are read once
    per process).  The time limit is what this process took for the same checks, twice over for
    a cold start of the caches and the device, plus a fresh process's start-up."""
    knobs, keys = CHILD_SETS[name]
    for k in keys:
        if k not in TIMES:
            run_check(k)
    limit = CHILD_START + 2.0 * sum(TIMES[k] for k in keys)
    env = dict(os.environ)
    env.update(knobs)
    r = subprocess.run([sys.executable, "-m", "tests.stream_ref_child", name], env=env, cwd=ROOT, timeout=limit,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, f"child '{name}' ended with {r.returncode}:\n{r.stdout[-4000:]}"
