"""Final-logit soft-capping without a GPU: the fp64 reference and tolerances of tests/softcap_ref.py (an
fp32 model of the kernel lies inside them, every planted defect outside), the reference op, the eager
model, the engine on the reference ops, evaluation, generation, the config, the trainers' and
infer.py's CLIs and one DDP run."""
import copy
import importlib
import math
import os
import pickle

import pytest
import torch
import torch.nn.functional as F

from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.models.engine import shift_targets
from distributed_llm_trainer_amd.ops import reference as ref
from tests import softcap_ref as S
from tests.dist_utils import run_multiprocess
from tests.test_zloss_cpu import _dense_logits, _labels, _randomise

BF, HF, F32, F64 = S.BF, S.HF, S.F32, S.F64
ALL_CASES = S.CAP_CASES + S.CAP_CASES_512 + S.CAP_CASES_PLAIN


# ------------------------------------------------------------------ the reference, a model, defects
def _inside(name, out, chk, dt):
    bad = S.miss(out, chk, dt)
    err = (out.double() - chk.ref).abs()
    assert not bad.any(), f"{name}: err/tol = {torch.where(chk.tol > 0, err / chk.tol, err)[bad].max().item():.3f}"


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c[0])
def test_kernel_model_inside_and_planted_defects_outside(case):
    name, dt, Vp, V, kind, nv_mode, g, cap, zc = case
    inp = S.ce_inputs(dt, Vp, V, kind)
    nv = S.ce_n_valid(inp, nv_mode)
    live = inp.targets != -100
    r = S.cap_ref(inp.logits, inp.targets, V, nv, g, cap, zc)
    loss32, z32, grad32 = S.kernel_model(inp.logits, inp.targets, V, nv, g, cap, zc)
    assert not any(torch.isnan(t).any() for t in (loss32, z32, grad32))
    _inside("fp32 loss", loss32, r.loss, F32)
    _inside("fp32 z_rows", z32, r.z, F32)
    _inside("fp32 grad", grad32, r.grad, dt)
    for chk in (r.z, r.grad):
        assert not chk.ref[~live].any() and not chk.tol[~live].any()
    assert not r.grad.ref[:, V:].any() and not r.grad.tol[:, V:].any()
    assert not torch.isnan(r.grad.ref).any() and not torch.isnan(r.grad.tol).any()

    def bad(defect):
        b = S.cap_ref(inp.logits, inp.targets, V, nv, g, cap, zc, defect=defect)
        return (S.miss(b.loss.ref.float(), r.loss, F32), S.miss(b.z.ref.float(), r.z, F32),
                S.miss(S.round_to(b.grad.ref, dt), r.grad, dt).any(dim=1))

    # a row whose spike is its target has a softmax of 1 there and a gradient near zero everywhere: such a
    # row cannot show a defect of the gradient, so those are asked of some live row, not of each
    for d in ("no_deriv", "deriv_1_minus_t"):
        assert bad(d)[2][live].any(), f"{d} stays inside"
    for d in ("lse_uncapped", "no_division"):
        bl, bz, bg = bad(d)
        assert bl[live].all() and bz[live].all() and bg[live].any(), f"{d} stays inside"
    assert bad("target_uncapped")[0][live].any(), "an uncapped target logit stays inside"
    assert bad("z_rows_uncapped")[1][live].all(), "z_rows from the uncapped lse stay inside"
    if zc != 0.0:
        assert bad("zf_uncapped")[2][live].any(), "zf from the uncapped lse stays inside"
    assert bad("ignored_row_grad")[2][~live].all(), "an ignored row's gradient stays inside"
    if V < Vp and kind != "ceil":  # the padding holds +40; the ceiling rows sit at +-cap themselves
        bl, bz, _ = bad("cap_over_padding")
        assert bl[live].any() and bz[live].any(), "the capped padding inside lse stays inside"
    if kind == "ceil":
        bl, bz, bg = bad("nan_at_saturation")
        assert bl[live].all() and bz[live].all() and bg.all(), "NaN at saturation stays inside"


def test_cases_hold_what_the_gpu_tests_need():
    cs = S.CAP_CASES
    assert {c[0].split("-cap")[0] for c in cs} == {c[0] for c in S.CE_CASES}
    for base in S.CE_CASES:
        got = {(c[7], c[8]) for c in cs if c[0].startswith(base[0] + "-cap")}
        assert got == {(cap, z) for cap in (30.0, 15.0) for z in (0.0, 1e-2)}
    for dt in S.DTYPES:
        seen = {S.ce_variant(c[2]) for c in cs if c[1] == dt}
        seen |= {S.ce_variant(c[2], wide=False, nt=False) for c in S.CAP_CASES_512 if c[1] == dt}
        seen |= {S.ce_variant(c[2], nt=False) for c in S.CAP_CASES_PLAIN if c[1] == dt}
        assert seen == set(S.CE_VARIANTS), (dt, sorted(set(S.CE_VARIANTS) - seen))
    assert all(S.ce_inputs(c[1], c[2], c[3], c[4]).targets.numel() <= 64 for c in cs)
    # cap 15 saturates the +-80 rows (tanh within 1e-4 of +-1), and the fp16 ceiling overflows exp(2 x / cap)
    large = S.ce_inputs(BF, 4096, 4091, "large").logits.float()
    assert (1 - torch.tanh(large.abs().amax() / 15.0)) < 1e-4
    assert 6e4 / 30.0 > S.SATURATION_U


def test_saturation_and_the_tolerance_terms():
    x = torch.tensor([[0.0, 1e-3, 30.0, 88.0, 6e4, -6e4]], dtype=F64)
    c, d, c_err, a_rel = S.cap_tanh_terms(x, 30.0)
    assert c[0, 4] == 30.0 and c[0, 5] == -30.0 and d[0, 4] == 0.0 and d[0, 5] == 0.0
    assert torch.isfinite(c_err).all() and torch.isfinite(a_rel).all()
    # near zero the error is absolute: half an fp32 ulp of 1, times the cap
    assert abs(c_err[0, 0].item() - 30.0 * (0.5 * S.U23 + 2 * S.EXP_FLUSH)) < 1e-12
    torch.testing.assert_close(d, 1 - torch.tanh(x / 30.0) ** 2, rtol=1e-9, atol=1e-15)


# ------------------------------------------------------------------ the reference op
@pytest.mark.parametrize("dt", [F32, BF])
@pytest.mark.parametrize("zc", [0.0, 1e-2])
@pytest.mark.parametrize("cap", [30.0, 2.0])
def test_reference_op_against_fp64_autograd(dt, zc, cap):
    g_ = torch.Generator().manual_seed(11)
    M, Vp, V = 9, 72, 67
    lg = (torch.randn(M, Vp, generator=g_) * 3).to(dt)
    lg[:, V:] = 40.0
    tg = torch.randint(0, V, (M,), generator=g_)
    tg[[2, 8]] = -100
    nv, gs = int((tg != -100).sum()), 8.0
    x = lg.double()[:, :V].clone().requires_grad_(True)
    c = cap * torch.tanh(x / cap)
    z = torch.logsumexp(c, dim=1)
    live = tg != -100
    ce_rows = F.cross_entropy(c, tg, ignore_index=-100, reduction="none")
    ((ce_rows.sum() + zc * (z[live] ** 2).sum()) / nv * gs).backward()
    buf = lg.clone()
    z_rows = torch.full((M,), -7.0) if zc else None
    rows = ref.cross_entropy_fwd_bwd(buf, tg, V, torch.tensor(nv), gs, zc, z_rows, softcap=cap)
    tol = dict(rtol=1e-5, atol=1e-5) if dt == F32 else dict(rtol=2.0 ** -7, atol=1e-6)
    torch.testing.assert_close(rows.double(), ce_rows.detach(), rtol=1e-5, atol=1e-5)
    if zc:
        torch.testing.assert_close(z_rows.double(), torch.where(live, z.detach() ** 2, torch.zeros_like(z)), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(buf.double()[:, :V], x.grad, **tol)
    assert not buf[:, V:].any() and not buf[~live].any()
    # softcap = 0: the op it was, bit for bit
    b0, b1 = lg.clone(), lg.clone()
    r0 = ref.cross_entropy_fwd_bwd(b0, tg, V, torch.tensor(nv), gs)
    r1 = ref.cross_entropy_fwd_bwd(b1, tg, V, torch.tensor(nv), gs, softcap=0.0)
    assert torch.equal(r0, r1) and torch.equal(b0, b1) and not torch.equal(b0, buf)


def test_reference_op_at_the_fp16_ceiling_and_its_validation():
    lg = torch.tensor([[6e4, -6e4, 0.0, 1.0] + [0.0] * 4], dtype=HF)
    tg, nv = torch.tensor([2]), torch.tensor(1)
    rows = ref.cross_entropy_fwd_bwd(lg, tg, 4, nv, 1.0, softcap=30.0)
    assert torch.isfinite(rows).all() and torch.isfinite(lg).all() and lg[0, 0] == 0 and lg[0, 1] == 0
    lg = torch.zeros(4, 16)
    tg, nv = torch.zeros(4, dtype=torch.int64), torch.tensor(4)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ref.cross_entropy_fwd_bwd(lg, tg, 16, nv, 1.0, softcap=bad)
    for bad in (True, "30"):
        with pytest.raises(TypeError):
            ref.cross_entropy_fwd_bwd(lg, tg, 16, nv, 1.0, softcap=bad)
    with pytest.raises(TypeError):
        ref.cross_entropy_fwd_bwd(lg, tg, 16, nv, 1.0, 1e-4, softcap=30.0)  # a coefficient without z_rows


# ------------------------------------------------------------------ the models
TINY = dict(vocab_size=256, hidden_size=64, num_layers=2, num_heads=4, max_seq_len=32, dropout=0.0, attention_dropout=0.0)
FEATURES = {"num_kv_heads": 2, "qk_norm": True, "sliding_window": 5, "sliding_window_pattern": 2, "attention_sinks": True}
# initializer_range 0.2 gives logits of several units: a cap of 2 bends most of them
CAP, INIT = 2.0, 0.2
C = 1e-2


def tiny(**kw):
    d = dict(TINY, initializer_range=INIT, logit_softcap=CAP)
    d.update(kw)
    return GPTConfig(**d)


def _dense_loss(m, ids, labels, zc=0.0, **kw):
    """The capped loss written independently of the model's own lines: (ce, z term, capped logits)."""
    x = _dense_logits(m, ids, **kw)
    cap = m.config.logit_softcap
    e2 = torch.exp(2.0 * x / cap)
    logits = cap * (e2 - 1.0) / (e2 + 1.0)
    tg = shift_targets(labels)
    live = tg != -100
    n = max(int(live.sum()), 1)
    lse = torch.log(torch.exp(logits - logits.amax(-1, keepdim=True)).sum(-1)) + logits.amax(-1)
    picked = logits.gather(1, tg.clamp(min=0).unsqueeze(1)).squeeze(1)
    return ((lse - picked) * live).sum() / n, zc * ((lse * lse) * live).sum() / n, logits


def _close_grads(m1, m2, atol=1e-6, rtol=1e-4):
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=atol, rtol=rtol), (n, (p1.grad - p2.grad).abs().max())


def _uncapped(m):
    m0 = GPT(GPTConfig.from_dict({**m.config.to_dict(), "logit_softcap": None}))
    m0.load_state_dict(m.state_dict())
    return m0


@pytest.mark.parametrize("zc", [0.0, C])
@pytest.mark.parametrize("kw", [{}, FEATURES], ids=["plain", "features"])
def test_eager_model_matches_the_dense_formula(kw, zc):
    torch.manual_seed(0)
    m = _randomise(GPT(tiny(**kw)))
    m2 = copy.deepcopy(m)
    m.set_z_loss(zc)
    ids = torch.randint(0, 256, (3, 32))
    lab = _labels(ids)
    logits, l1 = m(ids, labels=lab)
    l1.backward()
    ce, zt, dense = _dense_loss(m2, ids, lab, zc)
    (ce + zt).backward()
    assert abs(l1.item() - (ce + zt).item()) < 1e-5
    assert logits.dtype == F32 and logits.abs().max() <= CAP
    torch.testing.assert_close(logits.reshape(-1, 256), dense.detach(), rtol=1e-4, atol=1e-5)
    _close_grads(m, m2)
    # the cap is live: these logits reach its bend, and the model without it has another loss and gradient
    m3 = _uncapped(m2)
    raw, l3 = m3(ids, labels=lab)
    l3.backward()
    assert raw.abs().max() > 2 * CAP and abs(l3.item() - l1.item()) > 1e-2
    assert (m3.embed_tokens.weight.grad - m.embed_tokens.weight.grad).abs().max() > 1e-4


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kw,zc", [({}, 0.0), (FEATURES, C)], ids=["plain", "features+z_loss"])
def test_engine_matches_autograd_with_the_same_dropout_masks(kw, zc, p, recompute):
    torch.manual_seed(3)
    m1 = _randomise(GPT(tiny(dropout=p, attention_dropout=p, **kw)))
    m2 = copy.deepcopy(m1)
    ids = torch.randint(1, 256, (3, 32))
    lab = _labels(ids)
    ce, zt, _ = _dense_loss(m1, ids, lab, zc, seed=21, micro=0, p_attn=p, p_hidden=p)
    (ce + zt).backward()
    m2.set_z_loss(zc)
    eng = m2.enable_engine(seed=21)
    assert eng.softcap == CAP
    m2.gradient_checkpointing = recompute
    m2.train()
    _, l2 = m2(ids, labels=lab)
    l2.backward()
    assert abs((ce + zt).item() - l2.item()) < 1e-5
    pce, pz = m2.last_loss_parts
    assert abs(pce.item() - ce.item()) < 1e-5 and abs(pz.item() - zt.item()) < 1e-6
    _close_grads(m1, m2)


def test_engine_gradient_by_finite_differences():
    torch.manual_seed(7)
    m = GPT(tiny())
    m0 = _uncapped(m)  # the same weights without the cap: its share of the slope must be visible
    m.enable_engine()
    m0.enable_engine()
    ids = torch.randint(0, 256, (3, 32))
    lab = _labels(ids)
    m.train()
    _, loss = m(ids, labels=lab)
    loss.backward()
    w = m.embed_tokens.weight
    g = w.grad.clone()
    d = g / g.norm()
    h = 0.05
    ls = []
    for sgn in (1.0, -1.0):
        with torch.no_grad():
            w.add_(sgn * h * d)
            m.store.refresh_shadow()
            ls.append(m(ids, labels=lab)[1].item())
            w.sub_(sgn * h * d)
    fd = (ls[0] - ls[1]) / (2 * h)
    # central difference: O(h^2) truncation (charged 2 % of the slope) + the fp32 loss's own error,
    # a few tens of ulps of a value under 32 (2^-19), over 2h
    tol = 2e-2 * abs(fd) + 40 * 2.0 ** -19 / (2 * h)
    assert abs(fd - g.norm().item()) <= tol, (fd, g.norm().item(), tol)
    m0.train()
    m0(ids, labels=lab)[1].backward()
    assert abs((m0.embed_tokens.weight.grad * d).sum().item() - g.norm().item()) > 2 * tol, "the cap's slope is under the noise"


def test_fused_micro_steps_equal_the_mean_of_separate_ones():
    torch.manual_seed(5)
    Fs = 3
    m1 = GPT(tiny())
    m2 = copy.deepcopy(m1)
    for m in (m1, m2):
        m.set_z_loss(C)
        m.enable_engine(seed=5)
        m.train()
    ids = torch.randint(0, 256, (2 * Fs, 32))
    lab = ids.clone()
    lab[0:2, 5:] = -100     # 2 x 4 valid targets in the first segment
    lab[2:4, 20:] = -100    # 2 x 19 in the second, 2 x 31 in the third
    parts = []
    for k in range(Fs):
        _, loss = m1(ids[2 * k:2 * k + 2], labels=lab[2 * k:2 * k + 2])
        (loss / Fs).backward()
        parts.append(loss.item())
    m2.engine.set_loss_segments(Fs)
    _, fused = m2(ids, labels=lab)
    fused.backward()
    assert abs(fused.item() - sum(parts) / Fs) < 1e-5
    assert max(parts) - min(parts) > 1e-3
    _close_grads(m1, m2)


@pytest.mark.parametrize("segments", [1, 2])
def test_chunked_head_equals_the_single_call(segments):
    torch.manual_seed(9)
    GA = 2
    m1 = GPT(tiny(dropout=0.1, attention_dropout=0.1))
    m2 = copy.deepcopy(m1)
    data = [torch.randint(0, 256, (4, 32)) for _ in range(GA)]
    labs = [_labels(d, seed=j) for j, d in enumerate(data)]
    outs = []
    for m, chunks in ((m1, 0), (m2, 3)):
        eng = m.enable_engine(seed=9)
        eng.head_chunks = chunks
        eng.set_loss_segments(segments)
        m.train()
        outs.append(eng.train_window(data, [shift_targets(x) for x in labs], torch.full((), 1.0 / GA)))
    for j in range(GA):
        assert abs(outs[0][j].item() - outs[1][j].item()) < 1e-5
    _close_grads(m1, m2)
    # against the eager capped model on the first micro-step's loss
    m3 = GPT(m1.config)
    m3.load_state_dict({k: v for k, v in m1.state_dict().items()})
    m3.eval()
    m1.eval()
    assert abs(m1.eval_loss(data[0], labs[0]).item() - m3.eval_loss(data[0], labs[0]).item()) < 1e-5


def test_train_window_matches_sequential_bit_for_bit():
    torch.manual_seed(5)
    GA = 2
    m1 = GPT(tiny(dropout=0.1, attention_dropout=0.1))
    m2 = copy.deepcopy(m1)
    for m in (m1, m2):
        m.enable_engine(seed=5)
        m.train()
    data = [torch.randint(0, 256, (2, 32)) for _ in range(GA)]
    seq = []
    for j in range(GA):
        m1.engine.set_accumulation(j, GA, defer=True)
        _, loss = m1(data[j], labels=data[j])
        (loss / GA).backward()
        seq.append(loss.detach())
    win = m2.engine.train_window(data, [shift_targets(d) for d in data], torch.full((), 1.0 / GA))
    for j in range(GA):
        assert torch.equal(seq[j], win[j])
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p1.grad, p2.grad), n


@pytest.mark.parametrize("rows", [(2, 32), (1, 3)], ids=["64 rows", "3 rows"])
def test_eval_loss_matches_forward_with_labels(rows):
    """The engine's chunked evaluation head, the engine's forward with labels and the eager model agree;
    evaluation is the plain cross-entropy of the capped logits whatever z_loss is."""
    torch.manual_seed(1)
    m = GPT(tiny())
    eager = copy.deepcopy(m)
    eng = m.enable_engine()
    m.eval()
    eager.eval()
    ids = torch.randint(0, 256, rows)
    lab = ids.clone()
    lab[0, 1] = -100
    with torch.no_grad():
        logits, want = m(ids, labels=lab)
        _, want_eager = eager(ids, labels=lab)
    assert logits.abs().max() <= CAP
    got = m.eval_loss(ids, lab)
    assert abs(got.item() - want.item()) < 1e-5 and abs(got.item() - want_eager.item()) < 1e-5
    assert abs(eager.eval_loss(ids, lab).item() - got.item()) < 1e-5
    s0, n0 = m.eval_loss_sum(ids, lab)
    m.set_z_loss(0.5)
    s1, n1 = m.eval_loss_sum(ids, lab)
    assert torch.equal(s0, s1) and torch.equal(n0, n1) and eng.z_loss == 0.5
    assert abs(_uncapped(eager).eval().eval_loss(ids, lab).item() - got.item()) > 1e-2


def test_kv_cached_greedy_generation_matches_the_full_re_forward():
    torch.manual_seed(4)
    m = GPT(tiny())
    m.enable_engine()
    eager = GPT(m.config)
    eager.load_state_dict(m.state_dict())
    ids = torch.randint(0, 256, (2, 6))
    out = m.generate(ids, max_new_tokens=10, top_k=1)
    out_eager = eager.generate(ids, max_new_tokens=10, top_k=1)
    want = ids
    with torch.no_grad():
        for _ in range(10):
            lg = m(want)[0][:, -1]
            assert lg.abs().max() <= CAP
            want = torch.cat([want, lg.argmax(-1, keepdim=True)], dim=1)
    assert torch.equal(out, want) and torch.equal(out_eager, want)
    from distributed_llm_trainer_amd.eval.decode import KVCache, forward_cached
    cache = KVCache(m.config, 2, ids.device, m.engine.act_dtype)
    last = forward_cached(m, ids, cache)
    torch.testing.assert_close(last, m(ids)[0][:, -1].float(), rtol=1e-5, atol=1e-5)
    assert last.abs().max() <= CAP
    # the uncapped model picks other tokens somewhere: the cap reaches generation
    raw = _uncapped(eager)(ids)[0][:, -1]
    assert raw.abs().max() > CAP


@pytest.mark.parametrize("engine", [False, True])
def test_unset_cap_is_the_model_that_never_heard_of_it(engine):
    torch.manual_seed(2)
    kw = dict(TINY, dropout=0.1, attention_dropout=0.1)
    m1 = GPT(GPTConfig(**kw))
    m2 = GPT(GPTConfig(**kw, logit_softcap=None))
    m2.load_state_dict(m1.state_dict())
    del m1.config.__dict__["logit_softcap"]  # a config object from before the field existed
    assert list(m1.state_dict()) == list(m2.state_dict())
    if engine:
        m1.enable_engine(seed=4)
        e2 = m2.enable_engine(seed=4)
        assert e2.softcap == 0.0
    ids = torch.randint(0, 256, (3, 32))
    lab = _labels(ids)
    outs = []
    for m in (m1, m2):
        m.train()
        torch.manual_seed(77)  # the eager model's dropout
        _, loss = m(ids, labels=lab)
        loss.backward()
        m.eval()
        with torch.no_grad():
            outs.append((loss.detach(), m(ids)[0], m.eval_loss(ids, lab)))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert outs[0][1].dtype == outs[1][1].dtype
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p1.grad, p2.grad), n


def test_unset_cap_runs_the_calls_it_ran(monkeypatch):
    """With the field unset the engine hands the ops no softcap argument: the kernels launched are the same."""
    torch.manual_seed(2)
    m = GPT(GPTConfig(**TINY))
    eng = m.enable_engine()
    seen = []
    real = eng.ops.cross_entropy_fwd_bwd

    def spy(*a, **k):
        seen.append((len(a), sorted(k)))
        return real(*a, **k)

    monkeypatch.setattr(eng.ops, "cross_entropy_fwd_bwd", spy)
    ids = torch.randint(0, 256, (2, 32))
    m.train()
    m(ids, labels=ids)[1].backward()
    m.set_z_loss(1e-3)
    m(ids, labels=ids)[1].backward()
    assert seen == [(5, []), (7, [])]


# ------------------------------------------------------------------ configuration
def test_config_validation_to_dict_and_pickles():
    assert GPTConfig().logit_softcap is None
    c = GPTConfig(logit_softcap=30)
    assert c.logit_softcap == 30.0 and isinstance(c.logit_softcap, float)
    for bad in (True, False, 0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "30"):
        with pytest.raises(ValueError):
            GPTConfig(logit_softcap=bad)
    # the key is dropped when None: configs without the cap are what they were
    assert "logit_softcap" not in GPTConfig().to_dict() and c.to_dict()["logit_softcap"] == 30.0
    assert GPTConfig.from_dict(c.to_dict()).logit_softcap == 30.0
    assert GPTConfig.from_dict(GPTConfig().to_dict()).logit_softcap is None
    assert "logit_softcap" not in GPTConfig().__getstate__()
    assert pickle.loads(pickle.dumps(c)).logit_softcap == 30.0
    assert pickle.loads(pickle.dumps(GPTConfig())).logit_softcap is None
    old = GPTConfig.__new__(GPTConfig)  # a pickle from before the field existed
    state = GPTConfig().__getstate__()
    assert "logit_softcap" not in state
    old.__setstate__(state)
    assert old.logit_softcap is None and old.to_dict() == GPTConfig().to_dict()
    assert c.num_parameters() == GPTConfig().num_parameters()
    assert list(GPT(tiny()).state_dict()) == list(GPT(tiny(logit_softcap=None)).state_dict())


def test_checkpoint_round_trip_and_infer(tmp_path):
    from distributed_llm_trainer_amd.eval import infer
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint, model_state_dict_cpu, save_checkpoint

    def save(path, model):
        save_checkpoint(path, {"model": model_state_dict_cpu(model), "model_config": model.config})

    torch.manual_seed(0)
    m = GPT(tiny())
    path = str(tmp_path / "ck.pt")
    save(path, m)
    assert load_checkpoint(path, map_location="cpu")["model_config"].logit_softcap == CAP
    ids = torch.randint(0, 256, (1, 8))
    m.eval()
    loaded = infer.load_model(path)
    assert loaded.config.logit_softcap == CAP
    assert torch.equal(loaded(ids)[0], m(ids)[0])
    # a checkpoint whose config lacks the field: the flag supplies it; and the flag overrides
    m0 = _uncapped(m)
    path0 = str(tmp_path / "ck0.pt")
    save(path0, m0)
    assert infer.load_model(path0).config.logit_softcap is None
    capped = infer.load_model(path0, logit_softcap=CAP)
    assert capped.config.logit_softcap == CAP and torch.equal(capped(ids)[0], m(ids)[0])
    assert infer.load_model(path, logit_softcap=7.0).config.logit_softcap == 7.0
    with pytest.raises(ValueError):
        infer.load_model(path0, logit_softcap=-1.0)


# ------------------------------------------------------------------ CLI, YAML
def _yaml(tmp_path, cap):
    p = tmp_path / "m.yaml"
    extra = f"  logit_softcap: {cap}\n" if cap is not None else ""
    p.write_text("model:\n  hidden_size: 64\n  num_layers: 1\n  num_heads: 4\n  vocab_size: 128\n  max_seq_len: 16\n" + extra
                 + "training:\n  log_interval: 1\n  warmup_steps: 0\n")
    return str(p)


def _main(trainer, tmp_path, argv, cap_yaml=None, steps=1):
    mod = importlib.import_module(f"distributed_llm_trainer_amd.training.{trainer}")
    env_before = os.environ.get("DLT_DUMMY_BATCHES")
    os.environ["DLT_DUMMY_BATCHES"] = "2"
    try:
        return mod.main(["--config", _yaml(tmp_path, cap_yaml), "--batch_size", "1", "--max_steps", str(steps),
                         "--gradient_accumulation_steps", "2", "--no_final_save", "--checkpoint_dir", str(tmp_path / "ck"),
                         *argv])
    finally:
        if env_before is None:
            os.environ.pop("DLT_DUMMY_BATCHES", None)
        else:
            os.environ["DLT_DUMMY_BATCHES"] = env_before


@pytest.mark.parametrize("trainer", ["ddp_trainer", "fsdp_trainer"])
def test_cli_flag_precedence_and_rejected_values(tmp_path, trainer):
    """CLI > YAML > preset, and the value reaches the model and its engine."""
    mod = importlib.import_module(f"distributed_llm_trainer_amd.training.{trainer}")
    assert mod.build_parser().parse_args([]).logit_softcap is None

    def run(argv, cap_yaml=None):
        tr = _main(trainer, tmp_path, argv, cap_yaml)
        cap = tr.model.config.logit_softcap
        assert tr.model.engine is None or tr.model.engine.softcap == (cap or 0.0)
        return cap

    assert run([]) is None                                        # preset
    assert run([], "20.0") == 20.0                                # YAML over the preset
    assert run(["--logit_softcap", "30"], "20.0") == 30.0         # CLI over YAML
    assert run(["--logit_softcap", "30", "--z_loss", "1e-4", "--num_kv_heads", "2", "--qk_norm",
                "--doc_sep_token", "0"]) == 30.0                  # with the other flags
    for bad in ("-1", "0", "nan", "inf"):
        with pytest.raises(ValueError):
            run([f"--logit_softcap={bad}"])
    with pytest.raises(ValueError):
        run([], "-0.5")


def test_one_step_with_the_flag_changes_the_parameters_and_is_saved(tmp_path):
    p = {}
    for cap in (None, "0.05"):
        tr = _main("ddp_trainer", tmp_path, ["--logit_softcap", cap] if cap else [], steps=1)
        p[cap] = tr.flat_params().clone()
        assert tr.global_step == 1
    assert (p[None] - p["0.05"]).abs().max() > 0
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint
    path = str(tmp_path / "saved.pt")
    tr.save_checkpoint(path)
    assert load_checkpoint(path, map_location="cpu")["model_config"].logit_softcap == 0.05


def test_infer_cli_takes_the_flag():
    from distributed_llm_trainer_amd.eval import infer
    import inspect
    assert "logit_softcap" in inspect.signature(infer.load_model).parameters
    src = inspect.getsource(infer.main)
    assert "--logit_softcap" in src


# ------------------------------------------------------------------ distributed
DIST = dict(vocab_size=384, hidden_size=96, num_layers=2, num_heads=6, num_kv_heads=2, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0, initializer_range=0.2)


def _data(step, rank, n=8, seq=32, vocab=384):
    g = torch.Generator().manual_seed(1000 * step + rank)
    return torch.randint(0, vocab, (n, seq), generator=g)


def _ddp_trainer(GA, cap=CAP):
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=GA, warmup_steps=1, max_steps=100,
                        learning_rate=1e-2, bucket_cap_mb=0.05, micro_step_fusion=1)
    return DistributedTrainer(GPTConfig(**DIST, logit_softcap=cap), tc)


def _ddp_worker(rank, world, steps):
    tr = _ddp_trainer(2)
    for s in range(steps):
        out = tr.train_step({"input_ids": _data(s, rank, n=4)})
    return tr.flat_params().clone(), out


def test_ddp_matches_single_process():
    (p0, o0), (p1, _) = run_multiprocess(_ddp_worker, world=2, args=(3,))
    assert torch.equal(p0, p1), "ranks diverged"
    tr = _ddp_trainer(4)
    for s in range(3):
        out = tr.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    assert torch.allclose(p0, tr.flat_params(), atol=2e-5, rtol=1e-4), (p0 - tr.flat_params()).abs().max()
    assert abs(o0["loss_global"] - out["loss"]) < 1e-4
    off = _ddp_trainer(4, cap=None)
    for s in range(3):
        off.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    assert (off.flat_params() - tr.flat_params()).abs().max() > 1e-4, "the cap changed nothing"
