"""Final-logit soft-capping on the MI355X: the CAP forms of the cross-entropy kernels (ops/csrc/loss.hip)
against the fp64 reference and derived tolerances of tests/softcap_ref.py in every launch variant,
``dec_norm_head(..., softcap=)``, the engine on a tiny padded-vocabulary model, the fused decode step
and generation.

Each numerical check prints ``RATIO <name> <worst err / tol>`` (pytest -s shows them).  check_cap is a
plain function so that tests/softcap_ref_child.py can run it in a fresh process under the other
DLT_CE_* knobs (the launcher reads them once per process)."""
import copy
import functools
import os
import subprocess
import sys
import types

import pytest
import torch

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.models.engine import shift_targets
from distributed_llm_trainer_amd.ops import hip
from tests import decode_ref as R
from tests import softcap_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF, F32, I64 = S.BF, S.HF, S.F32, S.I64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = os.environ.get("DLT_CE_THREADS", "").strip() != "512"  # as loss.hip reads them
NT = os.environ.get("DLT_CE_NT", "").strip() != "0"
SENT = {BF: 3.0, HF: 3.0, F32: -7.5}
SEEN = set()  # (dtype, launch variant) this process has run in CAP form


def check(name, out, chk, dt):
    ref, tol = chk.ref.to(out.device), chk.tol.to(out.device)
    err = (out.double().reshape(ref.shape) - ref).abs().nan_to_num(posinf=0.0)  # infinities: S.miss judges them
    ratio = torch.where(tol > 0, err / tol, err).max().item()
    print(f"RATIO {name} {ratio:.4f}")
    assert not torch.isnan(out).any(), f"{name}: NaN"
    bad = S.miss(out, chk, dt)
    assert not bad.any(), (f"{name}: {bad.sum().item()} of {bad.numel()} elements outside the tolerance, "
                           f"worst err/tol {ratio:.3f} at {bad.nonzero()[0].tolist()}")


def _raw_cap(G, tg, nvt, V, gscale, zc, cap, L, ZR):
    """The CAP entry point itself, so that loss_rows too is a buffer with guards."""
    M, Vp = G.t.shape
    rc = hip.lib().dlt_cross_entropy_cap_fwd_bwd(hip._p(G.t), hip._p(tg), hip._p(nvt), hip._p(L.t), M, Vp, V,
                                                 float(gscale), hip._HK[G.t.dtype], float(zc),
                                                 hip._p(ZR.t) if ZR is not None else None, float(cap), hip._stream())
    assert rc == 0, rc


def check_cap(name):
    _, dt, Vp, V, kind, nv_mode, gscale, cap, zc = S.CAP_BY_NAME[name]
    inp = S.ce_inputs(dt, Vp, V, kind)
    nv = S.ce_n_valid(inp, nv_mode)
    ref = S.cap_ref(inp.logits, inp.targets, V, nv, gscale, cap, zc, wide=WIDE)
    tg, nvt = inp.targets.to(DEV), torch.tensor(nv, device=DEV)
    M = tg.numel()
    variant = S.ce_variant(Vp, WIDE, NT)
    tag = f"cap[{variant}] {name}"

    def G():
        return S.Guarded(inp.logits.shape, dt, SENT[dt], DEV, init=inp.logits)

    def R1():
        return S.Guarded((M,), F32, SENT[F32], DEV)

    # run 1: the entry point, guards around all three outputs (z_rows is taken with a coefficient of 0 too);
    # run 2: the wrapper
    G1, L1, Z1 = G(), R1(), R1()
    _raw_cap(G1, tg, nvt, V, gscale, zc, cap, L1, Z1)
    G2, Z2 = G(), R1()
    loss2 = hip.cross_entropy_fwd_bwd(G2.t, tg, V, nvt, gscale, zc, Z2.t, softcap=cap)
    bufs = [G1, L1, Z1, G2, Z2]
    if zc == 0.0:  # without z_rows: the form the engine runs without a z-loss
        G3, L3 = G(), R1()
        _raw_cap(G3, tg, nvt, V, gscale, 0.0, cap, L3, None)
        bufs += [G3, L3]
    # softcap = 0 through the wrapper: the plain kernel, and the Z form with a coefficient
    P, G0 = G(), G()
    if zc == 0.0:
        loss_p = hip.cross_entropy_fwd_bwd(P.t, tg, V, nvt, gscale)
        loss_0 = hip.cross_entropy_fwd_bwd(G0.t, tg, V, nvt, gscale, softcap=0.0)
        zp = z0 = None
    else:
        ZP, Z0 = R1(), R1()
        loss_p = hip.cross_entropy_fwd_bwd(P.t, tg, V, nvt, gscale, zc, ZP.t)
        loss_0 = hip.cross_entropy_fwd_bwd(G0.t, tg, V, nvt, gscale, zc, Z0.t, softcap=0.0)
        zp, z0 = ZP.t, Z0.t
        bufs += [ZP, Z0]
    bufs += [P, G0]
    torch.cuda.synchronize()
    for b in bufs:
        b.assert_guards()
    SEEN.add((dt, variant))
    print(f"VARIANT {S.DT_NAME[dt]} {variant}")
    check(tag + " loss", L1.t, ref.loss, F32)
    check(tag + " z_rows", Z1.t, ref.z, F32)
    check(tag + " grad", G1.t, ref.grad, dt)
    for a, b, what in ((L1.t, loss2, "loss"), (Z1.t, Z2.t, "z_rows"), (G1.t, G2.t, "grad")):
        assert torch.equal(S.bits(a), S.bits(b)), f"{tag} {what}: two calls on equal inputs differ"
    if zc == 0.0:
        assert torch.equal(S.bits(L3.t), S.bits(L1.t)) and torch.equal(S.bits(G3.t), S.bits(G1.t)), \
            f"{tag}: the form without z_rows differs"
    assert torch.equal(S.bits(loss_0), S.bits(loss_p)) and torch.equal(S.bits(G0.t), S.bits(P.t)), \
        f"{tag}: softcap = 0 is not the kernel without the argument"
    if zp is not None:
        assert torch.equal(S.bits(z0), S.bits(zp))
    dead = (inp.targets == -100).to(DEV)
    assert dead.sum() == 2 and not S.bits(Z1.t[dead]).any() and not S.bits(L1.t[dead]).any(), f"{tag}: ignored rows"
    assert not S.bits(G1.t[dead]).any(), f"{tag}: gradient on an ignored row"
    assert not S.bits(G1.t[:, V:]).any(), f"{tag}: gradient on the padding columns"
    if kind == "ceil":  # +-6e4 / cap: tanh is +-1 there and the gradient exactly 0
        sat = (inp.logits.float().abs() / cap > 2 * S.SATURATION_U).to(DEV)
        sat[:, V:] = False
        assert sat.any() and not (G1.t[sat] != 0).any(), f"{tag}: a saturated element's gradient is not 0"


@pytest.mark.parametrize("name", [c[0] for c in S.CAP_CASES])
def test_cap_form(name):
    check_cap(name)


def test_launch_variants_in_children():
    """The 512-thread x {1, 2, 4, 8, 13} variants and the plain-load 1024-thread variant, in fresh
    processes (the statics are read once per process); with the default process's variants, all nine
    in CAP form for both formats.  Ends at the first child that fails."""
    assert WIDE and NT, "this test is the default process: it must not run under the knobs itself"
    for dt in S.DTYPES:  # one case per default variant that test_cap_form has not run in this process
        for want in ("1024x7 NT", "512x16", "two-pass"):
            if (dt, want) not in SEEN:
                check_cap([c[0] for c in S.CAP_CASES if c[1] == dt and S.ce_variant(c[2]) == want][0])
    seen = {(S.DT_NAME[dt], v) for dt, v in SEEN}
    for name, (knobs, keys) in S.CAP_CHILD_SETS.items():
        env = dict(os.environ)
        env.update(knobs)
        # a fresh process's start (interpreter, torch, the library, the first HIP call), then a few
        # seconds per check: what a test of this suite may take
        r = subprocess.run([sys.executable, "-m", "tests.softcap_ref_child", name], env=env, cwd=ROOT,
                           timeout=60.0 + 3.0 * len(keys), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout)
        assert r.returncode == 0, f"child '{name}' ended with {r.returncode}:\n{r.stdout[-4000:]}"
        seen |= {tuple(ln.split(" ", 2)[1:]) for ln in r.stdout.splitlines() if ln.startswith("VARIANT ")}
    for dt in S.DTYPES:
        got = {v for d, v in seen if d == S.DT_NAME[dt]}
        assert got == set(S.CE_VARIANTS), (S.DT_NAME[dt], sorted(set(S.CE_VARIANTS) - got))


def test_host_validation():
    M, Vp, V = 4, 64, 60
    tg, nv = torch.zeros(M, dtype=I64, device=DEV), torch.tensor(M, device=DEV)
    lg = torch.zeros(M, Vp, dtype=BF, device=DEV)
    zr = torch.zeros(M, device=DEV)
    hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, softcap=30.0)
    hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, zr, softcap=30)
    for bad in (-1.0, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError):
            hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, softcap=bad)
    for bad in (True, "30", torch.tensor(30.0)):
        with pytest.raises(TypeError):
            hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, softcap=bad)
    with pytest.raises(TypeError):  # a coefficient without z_rows
        hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, softcap=30.0)
    with pytest.raises(TypeError):
        hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, torch.zeros(M, dtype=BF, device=DEV), softcap=30.0)
    with pytest.raises(ValueError):
        hip.cross_entropy_fwd_bwd(lg, tg, V, nv, 1.0, 1e-4, torch.zeros(M + 1, device=DEV), softcap=30.0)
    with pytest.raises(ValueError):
        hip.cross_entropy_fwd_bwd(lg, tg, Vp + 1, nv, 1.0, softcap=30.0)                                   # V > Vp
    with pytest.raises(ValueError):  # Vp % 8
        hip.cross_entropy_fwd_bwd(torch.zeros(M, 100, dtype=BF, device=DEV), tg, 90, nv, 1.0, softcap=30.0)
    with pytest.raises(NotImplementedError):  # fp32 logits have no CAP kernel
        hip.cross_entropy_fwd_bwd(torch.zeros(M, Vp, device=DEV), tg, V, nv, 1.0, softcap=30.0)
    h = torch.zeros(1, 64, device=DEV)
    with pytest.raises(ValueError):
        hip.dec_norm_head(h, torch.ones(64, device=DEV), 1e-5, torch.zeros(16, 64, dtype=BF, device=DEV),
                          torch.zeros(1, 16, device=DEV), 16, softcap=-2.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ dec_norm_head(..., softcap=)
@functools.lru_cache(maxsize=None)
def _head_case(HVR, wbf16):
    h, lnw, w = (t.to(DEV) for t in R.head_inputs(*HVR, wbf16))
    return h, lnw, w, R.norm_head_ref(h, lnw, w, HVR[1])


@pytest.mark.parametrize("B", R.DECODE_BATCHES)
@pytest.mark.parametrize("cap", S.DEC_CAPS)
@pytest.mark.parametrize("HVR", R.HEAD_SHAPES)
def test_dec_norm_head_softcap(HVR, cap, B):
    from tests.test_decode_kernels_gpu import Guarded, check as dcheck
    H, V, rows = HVR  # ragged V = 17 and 1000, and V = 50257
    wbf16 = H != 768
    h, lnw, w, plain = _head_case(HVR, wbf16)
    ref = S.dec_head_cap_ref(plain, cap)
    hin = h[:B].contiguous()
    outs = []
    for _ in range(2):
        lg = Guarded((B, V), F32, 1234.5)
        hip.dec_norm_head(hin, lnw, R.EPS, w, lg.t, V, softcap=cap)
        assert torch.isfinite(lg.t).all()
        lg.assert_guards()
        outs.append(lg.t)
    dcheck(f"dec_norm_head_cap[H={H},V={V},cap={cap:g},B={B}]", outs[0], ref, B)
    assert torch.equal(outs[0], outs[1])
    assert outs[0].abs().max().item() <= cap
    if cap == S.DEC_CAPS[-1]:  # the small cap bends these logits: without it the check above fails
        assert (plain.ref[:B] - ref.ref[:B]).abs().max() > 10 * ref.tol[:B].max()
    # softcap unset / 0: the existing call, bit for bit
    a, b, c = (Guarded((B, V), F32, 1234.5) for _ in range(3))
    hip.dec_norm_head(hin, lnw, R.EPS, w, a.t, V)
    hip.dec_norm_head(hin, lnw, R.EPS, w, b.t, V, softcap=0.0)
    hip.lib().dlt_dec_norm_head(hip._p(hin), hip._p(lnw), int(wbf16), float(R.EPS), hip._p(w), hip._p(c.t), B, H, V,
                                hip._stream())
    assert torch.equal(a.t, b.t) and torch.equal(a.t, c.t)
    dcheck(f"dec_norm_head[H={H},V={V},B={B}] (softcap unset)", a.t, plain, B)


# ------------------------------------------------------------------ the engine on a tiny model
# With initializer_range 0.1 a fresh model's logits have a standard deviation of sqrt(256) * 0.1 = 1.6 (a
# normed row times an embedding row): a cap of 1 bends most of them and takes about 1 off a loss of 7, far
# above the 2 % engine tolerances
CAP, INIT = 1.0, 0.1


def _cfg(dropout=0.1, **kw):
    d = dict(vocab_size=300, hidden_size=256, num_layers=2, num_heads=4, max_seq_len=192, dropout=dropout,
             attention_dropout=dropout, logit_softcap=CAP, initializer_range=INIT)
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


FEATURES = [{}, {"z": 1.0}, {"qk_norm": True}, {"num_kv_heads": 2}]


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("kw", FEATURES, ids=["plain", "z_loss", "qk_norm", "gqa"])
def test_engine_hip_vs_reference_ops(kw, recompute):
    kw = dict(kw)
    z = kw.pop("z", 0.0)
    cfg = _cfg(0.1, **kw)
    assert cfg.vocab_size_padded > cfg.vocab_size
    base = _model(cfg, 0)
    base.set_z_loss(z)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    e1 = m1.enable_engine(seed=5)
    e2 = m2.enable_engine(seed=5, ops=ops.CPU_OPS)
    assert e1.ops.backend == "hip" and e1.softcap == CAP == e2.softcap
    m1.gradient_checkpointing = m2.gradient_checkpointing = recompute
    ids = _ids(cfg)
    lab = _labels(ids)
    res = []
    for m in (m1, m2):
        _, loss = m(ids, labels=lab)
        (loss / 2).backward()
        res.append([loss.item()] + [t.item() for t in m.last_loss_parts])
    for a, b in zip(res[0], res[1]):
        assert abs(a - b) <= 2e-2 * abs(b), res
    _engine_close(_grads(m1), _grads(m2))
    # and the cap is in the loss and the gradient: without it both are other ones
    m0 = GPT(GPTConfig.from_dict({**cfg.to_dict(), "logit_softcap": None})).to(DEV)
    m0.load_state_dict(base.state_dict())
    m0.set_z_loss(z)
    e0 = m0.enable_engine(seed=5)
    assert e0.softcap == 0.0
    m0.gradient_checkpointing = recompute
    _, l0 = m0(ids, labels=lab)
    (l0 / 2).backward()
    assert abs(l0.item() - res[0][0]) > 2 * 2e-2 * res[0][0]  # twice the tolerance above
    g0, g1 = _grads(m0)["embed_tokens.weight"], _grads(m1)["embed_tokens.weight"]
    assert (g0 - g1).norm() > 0.1 * g1.norm()


@pytest.mark.parametrize("recompute", [False, True])
def test_train_window_matches_sequential_bit_for_bit(recompute):
    base = _model(_cfg(0.1), 5)
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
        seq.append(loss.item())
    win = e2.train_window([data[j] for j in range(GA)], [shift_targets(data[j]) for j in range(GA)],
                          torch.full((), 1.0 / GA, device=DEV), recompute=recompute)
    torch.cuda.synchronize()
    for j in range(GA):
        assert seq[j] == win[j].item()
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
        tr = _trainer(cfg, {})
        assert tr.use_engine and tr.model.engine.softcap == CAP
        outs = [tr.train_step({"input_ids": data}) for _ in range(3)]
        res.append(([o["loss"] for o in outs], tr.flat_params().detach().clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]), (res[0][1] - res[1][1]).abs().max().item()


def test_fused_micro_steps_vs_separate():
    base = _model(_cfg(0.0), 7)
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
        parts.append(loss.item())
    e2.set_loss_segments(2)
    _, fused = m2(ids, labels=lab)
    fused.backward()
    assert abs(fused.item() - (parts[0] + parts[1]) / 2) < 2e-2 * fused.item()
    _engine_close(_grads(m1), _grads(m2))


def test_chunked_head_vs_default():
    """--memory_first's head (row chunks run inside the forwards) against the window-deferred one."""
    base = _model(_cfg(0.1), 11)
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
        res.append(([x.item() for x in losses], _grads(m)))
    for losses, g in res[1:]:
        for j in range(GA):
            assert abs(losses[j] - res[0][0][j]) < 2e-2 * res[0][0][j]
        _engine_close(g, res[0][1])


def test_fp16_loss_scale():
    """fp16: the CAP gradient stored pre-multiplied by the loss scale (ce_grad_scale) against the same
    gradient stored unscaled with the scale applied behind it, both unscaled afterwards.  The two differ
    in one rounding of every dlogits element to fp16, 2^-8 relative at most at these magnitudes
    (tests/test_zloss_gpu.py derives it); charged twice through the fp16 GEMM chain: 2^-7 of the norm."""
    cfg = _cfg(0.0)
    base = _model(cfg, 17)
    ids = _ids(cfg, seed=17)
    lab = _labels(ids)
    LS = 4096.0

    def run(ce_scale):
        m = copy.deepcopy(base)
        eng = m.enable_engine(seed=19, act_dtype=torch.float16)
        assert eng.softcap == CAP
        eng.ce_grad_scale = ce_scale
        _, loss = m(ids, labels=lab)
        (loss * LS).backward()
        torch.cuda.synchronize()
        return loss.item(), {n: g / LS for n, g in _grads(m).items()}

    l_scaled, g_scaled = run(LS)
    l_plain, g_plain = run(1.0)
    assert l_scaled == l_plain
    for n in g_scaled:
        assert all(torch.isfinite(g[n]).all() for g in (g_scaled, g_plain))
        err = (g_scaled[n] - g_plain[n]).norm().item()
        assert err <= 2.0 ** -7 * g_plain[n].norm().item(), (n, err / g_plain[n].norm().item())


def test_fp32_route_is_refused_when_the_engine_is_enabled():
    m = _model(_cfg(0.0), 1)
    with pytest.raises(NotImplementedError, match="logit_softcap"):
        m.enable_engine(seed=1, act_dtype=torch.float32)
    m0 = _model(_cfg(0.0, logit_softcap=None), 1)
    m0.enable_engine(seed=1, act_dtype=torch.float32)  # the plain model still takes the route


# ------------------------------------------------------------------ evaluation
EVAL_S = 256


@functools.lru_cache(maxsize=None)
def _eval_model():
    torch.manual_seed(11)
    m = GPT(GPTConfig(vocab_size=50257, hidden_size=128, num_layers=1, num_heads=2, max_seq_len=EVAL_S, dropout=0.0,
                      attention_dropout=0.0, logit_softcap=CAP, initializer_range=INIT)).to(DEV)
    m.enable_engine(seed=2)
    m.eval()
    return m


def test_eval_loss_matches_forward_and_keeps_its_memory_bound():
    """eval_loss of a capped model (row chunks of lm_head GEMM + CAP cross-entropy) against forward with
    labels, whose loss is the same kernel over all rows at once: the two means differ by the fp32
    roundings of the row sums alone (2^-20 relative is generous).  Peak memory: under half a logits
    buffer.  The parameters are bit-identical afterwards, and z_loss does not enter."""
    m = _eval_model()
    B = 8
    ids = torch.randint(0, 50257, (B, EVAL_S), device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    labels = ids.clone()
    labels[1, 100:140] = -100
    before = [p.detach().clone() for p in m.parameters()]
    with torch.no_grad():
        logits, want = m(ids, labels=labels)
    assert logits.abs().max().item() <= CAP and logits.dtype == F32
    got = m.eval_loss(ids, labels).item()
    print(f"eval_loss {got:.6f} forward {want.item():.6f}")
    assert abs(got - want.item()) <= 2.0 ** -20 * abs(want.item())
    # against the eager formula on the returned (capped) logits
    dense = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, 50257), labels[:, 1:].reshape(-1)).item()
    assert abs(got - dense) <= 1e-4 * dense
    m.set_z_loss(0.5)
    assert m.eval_loss(ids, labels).item() == got
    m.set_z_loss(0.0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m.eval_loss(ids, labels)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    full = B * EVAL_S * m.config.vocab_size_padded * 2
    print(f"peak rise across eval_loss: {rise / 1e6:.1f} MB, a logits buffer {full / 1e6:.1f} MB")
    assert rise < full / 2
    for p, q in zip(m.parameters(), before):
        assert torch.equal(p, q)


# ------------------------------------------------------------------ decode and generation
# The model of tests/test_decode_gqa_gpu.py (default initialisation: logits with a standard deviation of about
# 0.3) under a cap of 0.25, which bends most of them.  The cap is 1-Lipschitz, so two steps whose uncapped
# logits agree within that suite's 3e-2 agree within 3e-2 capped.
DEC_CAP = 0.25


def _dec_cfg(nkv):
    return GPTConfig(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=nkv, max_seq_len=256,
                     dropout=0.0, attention_dropout=0.0, logit_softcap=DEC_CAP)


@functools.lru_cache(maxsize=None)
def _dec_model(nkv):
    torch.manual_seed(5 + nkv)
    m = GPT(_dec_cfg(nkv)).to(DEV)
    m.enable_engine()
    m.eval()
    return m


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("nkv", [4, 2])
def test_decode_fused_step_matches_torch_step(nkv, B, monkeypatch):
    """The captured fused step of a capped model == the ATen step == the full forward's last logits;
    two fresh fused graphs agree bit for bit; the kernel choice does not depend on the cap."""
    from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, _fused_kind, forward_cached
    m = _dec_model(nkv)
    cfg = m.config
    monkeypatch.setenv("DLT_DECODE_FUSED", "1")
    plain = types.SimpleNamespace(engine=m.engine, config=GPTConfig.from_dict({**cfg.to_dict(), "logit_softcap": None}))
    assert _fused_kind(m, B) == _fused_kind(plain, B) == ("mha" if nkv == 4 else "gqa")
    g = torch.Generator().manual_seed(50 + B)
    ids = torch.randint(0, 1000, (B, 150), generator=g).to(DEV)
    steps = torch.randint(0, 1000, (B, 3), generator=g).to(DEV)
    caches = [KVCache(cfg, B, DEV, m.engine.act_dtype) for _ in range(3)]
    graphs = []
    with torch.no_grad():
        for c, fused in zip(caches, ("1", "0", "1")):
            forward_cached(m, ids, c)
            monkeypatch.setenv("DLT_DECODE_FUSED", fused)
            graphs.append(DecodeGraph(m, c, c.len))
        assert graphs[0].fused and graphs[2].fused and not graphs[1].fused
        ctx = ids
        for t in range(steps.shape[1]):
            a = graphs[0](steps[:, t:t + 1]).clone()
            b = graphs[1](steps[:, t:t + 1]).clone()
            a2 = graphs[2](steps[:, t:t + 1]).clone()
            ctx = torch.cat([ctx, steps[:, t:t + 1]], dim=1)
            full = m(ctx)[0][:, -1].float()
            assert a.abs().max().item() <= DEC_CAP and b.abs().max().item() <= DEC_CAP
            assert (full.abs() > 0.5 * DEC_CAP).any(), "these logits do not reach the cap's bend"
            assert torch.allclose(a, b, atol=3e-2, rtol=3e-2), (t, (a - b).abs().max().item())
            assert torch.allclose(a, full, atol=3e-2, rtol=3e-2), (t, (a - full).abs().max().item())
            assert torch.equal(a, a2), "two fused graphs on the same inputs, other logits"


@pytest.mark.parametrize("nkv", [4, 2])
def test_generate_matches_the_greedy_re_forward(nkv):
    m = _dec_model(nkv)
    ids = torch.randint(0, 1000, (2, 40), generator=torch.Generator().manual_seed(7)).to(DEV)
    out = m.generate(ids, max_new_tokens=12, top_k=1)
    assert out.shape == (2, 52) and torch.equal(out[:, :40], ids)
    ref = ids
    with torch.no_grad():
        for _ in range(12):
            ref = torch.cat([ref, m(ref)[0][:, -1].argmax(dim=-1, keepdim=True)], dim=1)
    assert (out == ref).float().mean().item() > 0.97  # greedy; rare near-ties may flip
