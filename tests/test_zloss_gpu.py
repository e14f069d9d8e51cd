"""The z-loss forms of the cross-entropy kernels (ops/csrc/loss.hip, fp32.hip; ZL = true) against
the fp64 reference and derived tolerances of tests/zloss_ref.py, in every launch variant, and the
engine and the trainer with a coefficient on a tiny model.

Each numerical check prints ``RATIO <name> <worst err / tol>`` (pytest -s shows them).  check_zce is
a plain function so that tests/zloss_ref_child.py can run it in a fresh process under the other
DLT_CE_* knobs (the launcher reads them once per process)."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.models.engine import shift_targets
from distributed_llm_trainer_amd.ops import hip
from tests import zloss_ref as Z

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF, F32, I64 = Z.BF, Z.HF, Z.F32, Z.I64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = os.environ.get("DLT_CE_THREADS", "").strip() != "512"  # as loss.hip reads them
NT = os.environ.get("DLT_CE_NT", "").strip() != "0"
SENT = {BF: 3.0, HF: 3.0, F32: -7.5}
SEEN = set()  # (dtype, launch variant) this process has run in Z form


def check(name, out, chk, dt):
    ref, tol = chk.ref.to(out.device), chk.tol.to(out.device)
    err = (out.double().reshape(ref.shape) - ref).abs().nan_to_num(posinf=0.0)  # infinities: Z.miss judges them
    ratio = torch.where(tol > 0, err / tol, err).max().item()
    print(f"RATIO {name} {ratio:.4f}")
    bad = Z.miss(out, chk, dt)
    assert not bad.any(), (f"{name}: {bad.sum().item()} of {bad.numel()} elements outside the tolerance, "
                           f"worst err/tol {ratio:.3f} at {bad.nonzero()[0].tolist()}")


def _raw_z(G, tg, nvt, V, gscale, c, L, ZR):
    """The Z entry point itself, so that loss_rows too is a buffer with guards."""
    M, Vp = G.t.shape
    rc = hip.lib().dlt_cross_entropy_z_fwd_bwd(hip._p(G.t), hip._p(tg), hip._p(nvt), hip._p(L.t), M, Vp, V, float(gscale),
                                               hip._HK[G.t.dtype], float(c), hip._p(ZR.t), hip._stream())
    assert rc == 0, rc


def check_zce(name):
    _, dt, Vp, V, kind, nv_mode, gscale, c = Z.Z_BY_NAME[name]
    inp = Z.ce_inputs(dt, Vp, V, kind)
    nv = Z.ce_n_valid(inp, nv_mode)
    ref = Z.zce_ref(inp.logits, inp.targets, V, nv, gscale, c, wide=WIDE)
    tg, nvt = inp.targets.to(DEV), torch.tensor(nv, device=DEV)
    M = tg.numel()
    variant = Z.ce_variant(Vp, WIDE, NT)
    tag = f"zce[{variant}] {name}"
    # the plain kernel on the same input
    P = Z.Guarded(inp.logits.shape, dt, SENT[dt], DEV, init=inp.logits)
    loss_plain = hip.cross_entropy_fwd_bwd(P.t, tg, V, nvt, gscale)
    # run 1: the entry point, guards around all three outputs; run 2: the wrapper
    G1 = Z.Guarded(inp.logits.shape, dt, SENT[dt], DEV, init=inp.logits)
    L1, Z1 = Z.Guarded((M,), F32, SENT[F32], DEV), Z.Guarded((M,), F32, SENT[F32], DEV)
    _raw_z(G1, tg, nvt, V, gscale, c, L1, Z1)
    G2 = Z.Guarded(inp.logits.shape, dt, SENT[dt], DEV, init=inp.logits)
    Z2 = Z.Guarded((M,), F32, SENT[F32], DEV)
    loss2 = hip.cross_entropy_fwd_bwd(G2.t, tg, V, nvt, gscale, c, Z2.t)
    # c = 0 through the Z entry point
    G0 = Z.Guarded(inp.logits.shape, dt, SENT[dt], DEV, init=inp.logits)
    Z0 = Z.Guarded((M,), F32, SENT[F32], DEV)
    loss0 = hip.cross_entropy_fwd_bwd(G0.t, tg, V, nvt, gscale, 0.0, Z0.t)
    torch.cuda.synchronize()
    for b in (P, G1, L1, Z1, G2, Z2, G0, Z0):
        b.assert_guards()
    SEEN.add((dt, variant))
    print(f"VARIANT {Z.DT_NAME[dt]} {variant}")
    check(tag + " loss", L1.t, ref.loss, F32)
    check(tag + " z_rows", Z1.t, ref.z, F32)
    check(tag + " grad", G1.t, ref.grad, dt)
    assert torch.equal(Z.bits(L1.t), Z.bits(loss_plain)), f"{tag}: loss_rows differ from the plain kernel's"
    assert torch.equal(Z.bits(loss0), Z.bits(loss_plain)) and torch.equal(Z.bits(G0.t), Z.bits(P.t)), \
        f"{tag}: c = 0 through the Z entry point is not the plain kernel"
    assert torch.equal(Z.bits(Z0.t), Z.bits(Z1.t)), f"{tag}: z_rows depend on the coefficient"
    for a, b, what in ((L1.t, loss2, "loss"), (Z1.t, Z2.t, "z_rows"), (G1.t, G2.t, "grad")):
        assert torch.equal(Z.bits(a), Z.bits(b)), f"{tag} {what}: two calls on equal inputs differ"
    dead = (inp.targets == -100).to(DEV)
    assert dead.sum() == 2 and not Z.bits(Z1.t[dead]).any() and not Z.bits(L1.t[dead]).any(), f"{tag}: ignored rows"
    assert not Z.bits(G1.t[dead]).any(), f"{tag}: gradient on an ignored row"
    assert not Z.bits(G1.t[:, V:]).any(), f"{tag}: gradient on the padding columns"
    if nv > 0 and (ref.zf < 0).any():  # the factor is used as it is: the softmax part changes sign with it
        r = int((ref.zf < 0).nonzero()[0])
        col = [j for j in range(V) if j != int(inp.targets[r])][0]
        assert G1.t[r, col].item() <= 0 and ref.grad.ref[r, col] < 0


@pytest.mark.parametrize("name", [c[0] for c in Z.Z_CASES])
def test_z_form(name):
    check_zce(name)


def test_launch_variants_in_children():
    """The 512-thread x {1, 2, 4, 8, 13} variants and the plain-load 1024-thread variant, in fresh
    processes (the statics are read once per process); with the default process's variants, all nine
    in Z form for both formats.  Ends at the first child that fails."""
    assert WIDE and NT, "this test is the default process: it must not run under the knobs itself"
    for dt in Z.DTYPES:  # one case per default variant that test_z_form has not run in this process
        for want in ("1024x7 NT", "512x16", "two-pass"):
            if (dt, want) not in SEEN:
                check_zce([c[0] for c in Z.Z_CASES if c[1] == dt and Z.ce_variant(c[2]) == want][0])
    seen = {(Z.DT_NAME[dt], v) for dt, v in SEEN}
    for name, (knobs, keys) in Z.Z_CHILD_SETS.items():
        env = dict(os.environ)
        env.update(knobs)
        # a fresh process's start (interpreter, torch, the library, the first HIP call), then a few
        # seconds per check: what a test of this suite may take
        r = subprocess.run([sys.executable, "-m", "tests.zloss_ref_child", name], env=env, cwd=ROOT,
                           timeout=60.0 + 3.0 * len(keys), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout)
        assert r.returncode == 0, f"child '{name}' ended with {r.returncode}:\n{r.stdout[-4000:]}"
        seen |= {tuple(ln.split(" ", 2)[1:]) for ln in r.stdout.splitlines() if ln.startswith("VARIANT ")}
    for dt in Z.DTYPES:
        got = {v for d, v in seen if d == Z.DT_NAME[dt]}
        assert got == set(Z.CE_VARIANTS), (Z.DT_NAME[dt], sorted(set(Z.CE_VARIANTS) - got))


# ------------------------------------------------------------------ the fp32 kernel
@pytest.mark.parametrize("c", Z.Z_COEFS)
@pytest.mark.parametrize("form,Vp,V", Z.F32_SHAPES)
def test_fp32_kernel(form, Vp, V, c):
    inp = Z.f32_inputs(Vp, V)
    nv, gscale = inp.n_true, 4.0
    ref = Z.zce_ref(inp.logits, inp.targets, V, nv, gscale, c)
    tg, nvt = inp.targets.to(DEV), torch.tensor(nv, device=DEV)
    M = tg.numel()
    assert (Vp % 4 == 0) == (form == "vec4")
    runs = []
    for coef in (c, c, 0.0):
        G = Z.Guarded(inp.logits.shape, F32, SENT[F32], DEV, init=inp.logits)
        ZR = Z.Guarded((M,), F32, SENT[F32], DEV)
        loss = hip.cross_entropy_fwd_bwd(G.t, tg, V, nvt, gscale, coef, ZR.t)
        torch.cuda.synchronize()
        G.assert_guards()
        ZR.assert_guards()
        runs.append((loss, ZR.t, G.t))
    P = inp.logits.to(DEV).clone()
    loss_plain = hip.cross_entropy_fwd_bwd(P, tg, V, nvt, gscale)
    tag = f"zce_f32[{form}] c={c:g}"
    check(tag + " loss", runs[0][0], ref.loss, F32)
    check(tag + " z_rows", runs[0][1], ref.z, F32)
    check(tag + " grad", runs[0][2], ref.grad, F32)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(Z.bits(a), Z.bits(b)), f"{tag}: two calls differ"
    assert torch.equal(Z.bits(runs[0][0]), Z.bits(loss_plain)), f"{tag}: loss rows differ from the plain kernel's"
    dead = (inp.targets == -100).to(DEV)
    assert not Z.bits(runs[0][1][dead]).any() and not Z.bits(runs[0][2][dead]).any() and not Z.bits(runs[0][2][:, V:]).any()
    # c = 0 through the Z form: the plain objective
    check(tag + " grad at c = 0", runs[2][2], Z.zce_ref(inp.logits, inp.targets, V, nv, gscale, 0.0).grad, F32)


# ------------------------------------------------------------------ host validation
def test_host_validation():
    M, Vp, V = 4, 64, 60
    tg, nv = torch.zeros(M, dtype=I64, device=DEV), torch.tensor(M, device=DEV)
    for dt in (BF, F32):
        lg = torch.zeros(M, Vp, dtype=dt, device=DEV)
        good = torch.zeros(M, device=DEV)
        hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, good)
        with pytest.raises(TypeError):
            hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4)                                         # none given
        with pytest.raises(TypeError):
            hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, torch.zeros(M, dtype=torch.float64, device=DEV))
        with pytest.raises(TypeError):
            hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, torch.zeros(M, dtype=BF, device=DEV))
        with pytest.raises(ValueError):
            hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, torch.zeros(M + 1, device=DEV))
        with pytest.raises(ValueError):
            hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, torch.zeros(M, 1, device=DEV))
        with pytest.raises(ValueError):
            hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, torch.zeros(2 * M, device=DEV)[::2])
        with pytest.raises(ValueError):
            hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, torch.zeros(M))                         # on the host
        with pytest.raises(ValueError):
            hip.cross_entropy_fwd_bwd(lg, tg, Vp + 1, nv, 1.0, 1e-4, good)                              # V > Vp
    with pytest.raises(ValueError):  # Vp % 8
        hip.cross_entropy_fwd_bwd(torch.zeros(M, 100, dtype=BF, device=DEV), tg, 90, nv, 1.0, 1e-4, torch.zeros(M, device=DEV))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the engine on a tiny model
# Far above PaLM's 1e-4: at a fresh model's near-uniform softmax (lse about ln 300) zf is about 12 and
# the z part is a large share of the lm_head gradient, so that the 16-bit engine tolerances see it
CZ = 1.0


def _cfg(dropout=0.1, **kw):
    d = dict(vocab_size=300, hidden_size=256, num_layers=2, num_heads=4, max_seq_len=192, dropout=dropout,
             attention_dropout=dropout)
    d.update(kw)
    return GPTConfig(**d)


def _model(cfg, seed):
    torch.manual_seed(seed)
    return GPT(cfg).to(DEV)


def _grads(m):
    return {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()


def _ids(cfg, n=2, seed=0):
    return torch.randint(0, cfg.vocab_size, (n, cfg.max_seq_len), device=DEV, generator=torch.Generator(DEV).manual_seed(seed))


def _labels(ids):
    lab = ids.clone()
    for b in range(ids.shape[0]):
        lab[b, 7 * b:7 * b + 5 + 9 * b] = -100  # another count of ignored targets in every row
    return lab


def _engine_close(g1, g2):
    """The engine tolerances of the other GPU suites."""
    for n in g1:
        assert _cos(g1[n], g2[n]) > 0.99, n
        r = g1[n].norm() / g2[n].norm()
        assert 0.95 < r.item() < 1.05, (n, r.item())


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_engine_hip_vs_reference_ops(dropout, recompute):
    cfg = _cfg(dropout)
    assert cfg.vocab_size_padded > cfg.vocab_size
    base = _model(cfg, 0)
    base.set_z_loss(CZ)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    e1 = m1.enable_engine(seed=5)
    e2 = m2.enable_engine(seed=5, ops=ops.CPU_OPS)
    assert e1.ops.backend == "hip" and e1.z_loss == CZ == e2.z_loss
    m1.gradient_checkpointing = m2.gradient_checkpointing = recompute
    ids = _ids(cfg)
    lab = _labels(ids)
    res = []
    for m in (m1, m2):
        _, loss = m(ids, labels=lab)
        (loss / 2).backward()
        ce, zt = m.last_loss_parts
        assert abs((ce + zt).item() - loss.item()) <= 2.0 ** -22 * abs(loss.item())
        res.append((loss.item(), ce.item(), zt.item()))
    for a, b in zip(res[0], res[1]):
        assert abs(a - b) < 2e-2 * abs(b), res
    assert res[0][2] > 0.1 * res[0][1], "the z term is too small to be seen at these tolerances"
    _engine_close(_grads(m1), _grads(m2))
    # and the term is in the gradient: without it the lm_head gradient is another one
    m0 = copy.deepcopy(base)
    m0.set_z_loss(0.0)
    m0.enable_engine(seed=5)
    m0.gradient_checkpointing = recompute
    _, l0 = m0(ids, labels=lab)
    (l0 / 2).backward()
    assert abs(l0.item() - res[0][1]) < 1e-3 * res[0][1]
    g0, g1 = _grads(m0)["embed_tokens.weight"], _grads(m1)["embed_tokens.weight"]
    assert (g0 - g1).norm() > 0.1 * g1.norm()


@pytest.mark.parametrize("recompute", [False, True])
def test_train_window_matches_sequential_bit_for_bit(recompute):
    base = _model(_cfg(0.1), 5)
    base.set_z_loss(CZ)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    e1, e2 = m1.enable_engine(seed=9), m2.enable_engine(seed=9)
    m1.gradient_checkpointing = m2.gradient_checkpointing = recompute
    GA = 4
    data = _ids(base.config, n=GA * 2, seed=5).view(GA, 2, -1)
    seq = []
    for j in range(GA):
        e1.set_accumulation(j, GA, defer=True)
        _, loss = m1(data[j], labels=data[j])
        (loss / GA).backward()
        seq.append((loss.item(), [t.item() for t in m1.last_loss_parts]))
    win = e2.train_window([data[j] for j in range(GA)], [shift_targets(data[j]) for j in range(GA)],
                          torch.full((), 1.0 / GA, device=DEV), recompute=recompute)
    torch.cuda.synchronize()
    for j in range(GA):
        assert seq[j][0] == win[j].item()
        assert seq[j][1] == [t.item() for t in e2.window_loss_parts[j]] and seq[j][1][1] > 0
    g1, g2 = _grads(m1), _grads(m2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), (n, (g1[n] - g2[n]).abs().max().item())


def _trainer(cfg, tc_kw):
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    torch.manual_seed(3)
    tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=4, warmup_steps=1, learning_rate=1e-3,
                        micro_step_fusion=1, **tc_kw)
    return DistributedTrainer(cfg, tc)


def test_training_is_bitwise_reproducible():
    cfg = _cfg(0.1)
    data = _ids(cfg, n=8, seed=3)
    res = []
    for _ in range(2):
        tr = _trainer(cfg, dict(z_loss=CZ))
        assert tr.use_engine and tr.model.engine.z_loss == CZ
        outs = [tr.train_step({"input_ids": data}) for _ in range(3)]
        res.append(([(o["loss"], o["ce_loss"], o["z_loss"]) for o in outs], tr.flat_params().detach().clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]), (res[0][1] - res[1][1]).abs().max().item()
    for loss, ce, z in res[0][0]:
        assert z > 0 and abs(ce + z - loss) < 1e-5 * loss


def test_zero_coefficient_is_the_trainer_without_the_flag():
    cfg = _cfg(0.1)
    data = _ids(cfg, n=8, seed=3)
    res = []
    for kw in ({}, dict(z_loss=0.0)):
        tr = _trainer(cfg, kw)
        if kw:  # set and taken back: nothing may stay behind
            tr.model.set_z_loss(0.3)
            tr.model.set_z_loss(0.0)
        outs = [tr.train_step({"input_ids": data}) for _ in range(3)]
        assert all("z_loss" not in o and "ce_loss" not in o for o in outs)
        res.append(([o["loss"] for o in outs], tr.flat_params().detach().clone()))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1])


def test_fused_micro_steps_vs_separate():
    base = _model(_cfg(0.0), 7)
    base.set_z_loss(CZ)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    m1.enable_engine(seed=3)
    e2 = m2.enable_engine(seed=3)
    ids = _ids(base.config, n=4, seed=7)
    lab = _labels(ids)
    lab[2:4, 40:] = -100  # 78 valid targets in the second segment, 363 in the first: a joint normaliser shows
    parts = []
    for k in range(2):
        _, loss = m1(ids[2 * k:2 * k + 2], labels=lab[2 * k:2 * k + 2])
        (loss / 2).backward()
        parts.append([t.item() for t in m1.last_loss_parts])
    e2.set_loss_segments(2)
    _, fused = m2(ids, labels=lab)
    fused.backward()
    fce, fz = (t.item() for t in m2.last_loss_parts)
    assert abs(fce - (parts[0][0] + parts[1][0]) / 2) < 2e-2 * fce
    assert abs(fz - (parts[0][1] + parts[1][1]) / 2) < 2e-2 * fz and fz > 0
    # the same rows through GEMMs of another shape: the engine tolerances; a segment weighted by the
    # joint count would carry 441 / (2 * 78) = 2.8 times less weight
    _engine_close(_grads(m1), _grads(m2))


def test_chunked_head_vs_default():
    """--memory_first's head (row chunks run inside the forwards) against the window-deferred one."""
    base = _model(_cfg(0.1), 11)
    base.set_z_loss(CZ)
    GA = 2
    data = _ids(base.config, n=GA * 2, seed=11).view(GA, 2, -1)
    labs = [_labels(data[j]) for j in range(GA)]
    res = []
    for chunks in (0, 1, 3):
        m = copy.deepcopy(base)
        eng = m.enable_engine(seed=13)
        eng.head_chunks = chunks
        losses = eng.train_window([data[j] for j in range(GA)], [shift_targets(x) for x in labs],
                                  torch.full((), 1.0 / GA, device=DEV))
        torch.cuda.synchronize()
        res.append(([x.item() for x in losses], [[t.item() for t in p] for p in eng.window_loss_parts], _grads(m)))
    for losses, parts, g in res[1:]:
        for j in range(GA):
            assert abs(losses[j] - res[0][0][j]) < 2e-2 * res[0][0][j]
            assert abs(parts[j][1] - res[0][1][j][1]) < 2e-2 * res[0][1][j][1] and parts[j][1] > 0
        _engine_close(g, res[0][2])


def test_fp16_loss_scale_multiplies_the_z_part():
    """fp16: the cross-entropy gradient stored pre-multiplied by the loss scale (ce_grad_scale) against
    the bf16-style path (stored unscaled, the scale applied behind it), both unscaled afterwards.

    The two differ in one rounding of every dlogits element to fp16: 2^-11 relative, or 2^-25 absolute
    below 2^-14 -- here p zf / n >= 2^-17, so at most 2^-8 relative.  A parameter gradient is a linear
    map of dlogits through the same fp16 GEMM chain, whose own roundings then see inputs that differ
    by that much: 2^-8 charged twice, 2^-7 of the gradient's norm.  c = 1 makes the z part (zf about
    12) more than half of the softmax part's norm, far above that bound if the scale missed it."""
    cfg = _cfg(0.0)
    base = _model(cfg, 17)
    ids = _ids(cfg, seed=17)
    lab = _labels(ids)
    LS = 4096.0

    def run(c, ce_scale):
        m = copy.deepcopy(base)
        m.set_z_loss(c)
        eng = m.enable_engine(seed=19, act_dtype=torch.float16)
        eng.ce_grad_scale = ce_scale
        _, loss = m(ids, labels=lab)
        (loss * LS).backward()
        torch.cuda.synchronize()
        return loss.item(), {n: g / LS for n, g in _grads(m).items()}

    l_scaled, g_scaled = run(1.0, LS)
    l_plain, g_plain = run(1.0, 1.0)
    l_off, g_off = run(0.0, LS)
    assert l_scaled == l_plain and l_scaled > 2 * l_off
    for n in g_scaled:
        assert all(torch.isfinite(g[n]).all() for g in (g_scaled, g_plain))
        err = (g_scaled[n] - g_plain[n]).norm().item()
        assert err <= 2.0 ** -7 * g_plain[n].norm().item(), (n, err / g_plain[n].norm().item())
    n = "embed_tokens.weight"
    assert (g_scaled[n] - g_off[n]).norm() > 10 * 2.0 ** -7 * g_scaled[n].norm()
