"""QK-norm on the GPU: ``k_qknorm_rope_inplace`` / ``k_qknorm_bwd`` against the fp64
references of tests/qknorm_ref.py (tolerances derived there; the planted defects that fall
outside them are in test_qknorm_cpu.py, at these inputs), bitwise properties (v columns,
raw, repeat calls, guards around every written buffer), and the engine with
``GPTConfig.qk_norm``: HIP ops against the reference ops with identical dropout masks,
recompute, the two-chain window, reproducibility, the refused routes and generation.

Shapes: B = 2, S = 200 (M = 400 rows: no multiple of a backward block's 64 / 32 head slots),
(nh, nkv) multi-head, grouped and multi-query, head_dim 64 / 128, bf16 / fp16; one all-zero
head, one head scaled by 1e4, weights with negative and exactly-zero entries."""
import copy
import functools

import pytest
import torch

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip
from tests import qknorm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
CASES = [(nh, nkv, hd, dt) for nh, nkv in R.HEADS for hd in (64, 128) for dt in DTYPES]
GUARD = 4096  # elements on each side of a guarded buffer
SENT16, SENT32 = 123.0, -7.5  # exact in bf16 / fp16 / fp32


@functools.lru_cache(maxsize=None)
def _case(nh, nkv, hd, dtype):
    """Inputs and fp64 references of a case, computed once and never written."""
    inp = R.make_inputs(nh, nkv, hd, dtype)
    return inp, R.fwd_ref(inp), R.bwd_ref(inp)


def _guarded(src=None, shape=None, dtype=None, sentinel=SENT16):
    """(whole buffer, view of its middle): the view holds ``src`` (or is filled with the
    sentinel too), GUARD sentinel elements lie before and after it."""
    shape = tuple(src.shape) if src is not None else tuple(shape)
    dtype = src.dtype if src is not None else dtype
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    mid = buf[GUARD:GUARD + n].view(shape)
    if src is not None:
        mid.copy_(src)
    return buf, mid


def _guards_intact(buf, sentinel=SENT16):
    return bool((buf[:GUARD] == sentinel).all() and (buf[-GUARD:] == sentinel).all())


def _fwd(inp, qkv_src):
    M, W = qkv_src.shape[0], (inp.nh + inp.nkv) * inp.hd
    qbuf, qkv = _guarded(qkv_src)
    rbuf, raw = _guarded(shape=(M, W), dtype=qkv_src.dtype)
    hip.qknorm_rope_inplace(qkv, R.B, R.S, inp.nh, inp.cos.to(DEV), inp.sin.to(DEV), inp.qw.to(DEV), inp.kw.to(DEV),
                            R.EPS, raw, nkv=inp.nkv)
    torch.cuda.synchronize()
    return qbuf, qkv, rbuf, raw


@pytest.mark.parametrize("nh,nkv,hd,dtype", CASES)
def test_forward(nh, nkv, hd, dtype):
    inp, fref, _ = _case(nh, nkv, hd, dtype)
    W = (nh + nkv) * hd
    qbuf, qkv, rbuf, raw = _fwd(inp, inp.qkv)
    worst = R.worst(R._heads(qkv.cpu(), inp), fref)
    print(f"forward worst |err| / tol = {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(qkv[:, W:].cpu(), inp.qkv[:, W:]), "v columns changed"
    assert torch.equal(raw.cpu(), inp.qkv[:, :W]), "raw is not the pre-norm q|k"
    assert _guards_intact(qbuf) and _guards_intact(rbuf)
    _, qkv2, _, raw2 = _fwd(inp, inp.qkv)
    assert torch.equal(qkv, qkv2) and torch.equal(raw, raw2), "repeat call differs"
    if nkv == nh:  # nkv=None is the multi-head row
        q3 = inp.qkv.to(DEV)
        raw3 = torch.empty_like(raw)
        hip.qknorm_rope_inplace(q3, R.B, R.S, nh, inp.cos.to(DEV), inp.sin.to(DEV), inp.qw.to(DEV), inp.kw.to(DEV),
                                R.EPS, raw3)
        assert torch.equal(q3, qkv)


def _bwd(inp, dqw=None, dkw=None):
    M, W = inp.qkv.shape[0], (inp.nh + inp.nkv) * inp.hd
    gbuf, dqkv = _guarded(inp.dqkv)
    raw = inp.qkv[:, :W].contiguous().to(DEV)
    n_ws = hip.qknorm_bwd_workspace(M, inp.nh, inp.hd, DEV).numel()
    wbuf, ws = _guarded(shape=(n_ws,), dtype=torch.float32, sentinel=SENT32)
    dbuf, dw = _guarded(shape=(2, inp.hd), dtype=torch.float32, sentinel=SENT32)
    if dqw is None:
        dw.zero_()
    else:
        dw[0].copy_(dqw)
        dw[1].copy_(dkw)
    hip.qknorm_bwd(dqkv, raw, R.B, R.S, inp.nh, inp.qw.to(DEV), inp.kw.to(DEV), R.EPS, dw[0], dw[1], nkv=inp.nkv, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(raw.cpu(), inp.qkv[:, :W]), "raw was written"
    assert _guards_intact(gbuf) and _guards_intact(wbuf, SENT32) and _guards_intact(dbuf, SENT32)
    assert bool((ws != SENT32).all()), "a workspace row was left unwritten"
    return dqkv, dw[0].clone(), dw[1].clone()


@pytest.mark.parametrize("nh,nkv,hd,dtype", CASES)
def test_backward(nh, nkv, hd, dtype):
    inp, _, bref = _case(nh, nkv, hd, dtype)
    W = (nh + nkv) * hd
    dx, dqw, dkw = _bwd(inp)
    worst = (R.worst(R._heads(dx.cpu(), inp), bref.dx), R.worst(dqw, bref.dqw), R.worst(dkw, bref.dkw))
    print("backward worst |err| / tol: dx %.3f dqw %.3f dkw %.3f" % worst)
    assert max(worst) <= 1.0
    assert torch.equal(dx[:, W:].cpu(), inp.dqkv[:, W:]), "v columns of dqkv changed"
    # repeat from equal state: the same bits (fixed-order reduction, no atomics)
    dx2, dqw2, dkw2 = _bwd(inp)
    assert torch.equal(dx, dx2) and torch.equal(dqw, dqw2) and torch.equal(dkw, dkw2)
    # dw accumulates: a second call on top of the first adds the same sum again -- twice the
    # first, up to the one fp32 rounding of that addition (half an ulp: 2^-24 relative)
    _, aq, ak = _bwd(inp, dqw, dkw)
    for acc, one in ((aq, dqw), (ak, dkw)):
        assert bool(((acc.double() - 2 * one.double()).abs() <= 2.0 ** -24 * (2 * one.double()).abs()).all())
    # without an explicit workspace the binding allocates it
    g = inp.dqkv.to(DEV)
    d0, d1 = torch.zeros(hd, device=DEV), torch.zeros(hd, device=DEV)
    hip.qknorm_bwd(g, inp.qkv[:, :W].contiguous().to(DEV), R.B, R.S, nh, inp.qw.to(DEV), inp.kw.to(DEV), R.EPS, d0, d1,
                   nkv=nkv)
    assert torch.equal(g, dx) and torch.equal(d0, dqw) and torch.equal(d1, dkw)


def test_sixteen_bit_weights_are_upcast():
    """A gathered FSDP unit hands the norm weights over in the activation dtype."""
    inp, _, _ = _case(4, 2, 64, torch.bfloat16)
    w16 = inp._replace(qw=inp.qw.bfloat16().float(), kw=inp.kw.bfloat16().float())
    _, want, _, _ = _fwd(w16, inp.qkv)
    qkv = inp.qkv.to(DEV)
    raw = torch.empty(400, 6 * 64, dtype=torch.bfloat16, device=DEV)
    hip.qknorm_rope_inplace(qkv, R.B, R.S, 4, inp.cos.to(DEV), inp.sin.to(DEV), inp.qw.to(DEV).bfloat16(),
                            inp.kw.to(DEV).bfloat16(), R.EPS, raw, nkv=2)
    assert torch.equal(qkv, want)


def test_host_validation():
    inp, _, _ = _case(4, 2, 64, torch.bfloat16)
    cos, sin, qw, kw = inp.cos.to(DEV), inp.sin.to(DEV), inp.qw.to(DEV), inp.kw.to(DEV)
    qkv = inp.qkv.to(DEV)
    raw = torch.empty(400, 6 * 64, dtype=torch.bfloat16, device=DEV)
    dw = torch.zeros(2, 64, device=DEV)
    with pytest.raises(ValueError):
        hip.qknorm_rope_inplace(qkv, R.B, R.S, 4, cos, sin, qw, kw, R.EPS, raw[:, :-64].contiguous(), nkv=2)
    with pytest.raises(ValueError):
        hip.qknorm_rope_inplace(qkv, R.B, R.S + 1, 4, cos, sin, qw, kw, R.EPS, raw, nkv=2)
    with pytest.raises(ValueError):
        hip.qknorm_rope_inplace(qkv, R.B, R.S, 4, cos, sin, qw, kw, R.EPS, raw, nkv=3)
    with pytest.raises(ValueError):
        hip.qknorm_rope_inplace(qkv, R.B, R.S, 4, cos[:100], sin[:100], qw, kw, R.EPS, raw, nkv=2)
    with pytest.raises(ValueError):
        hip.qknorm_rope_inplace(qkv, R.B, R.S, 4, cos, sin, qw[:32], kw, R.EPS, raw, nkv=2)
    with pytest.raises(TypeError):
        hip.qknorm_rope_inplace(qkv, R.B, R.S, 4, cos, sin, qw, kw, R.EPS, raw.half(), nkv=2)
    with pytest.raises(NotImplementedError, match="fp32"):
        hip.qknorm_rope_inplace(qkv.float(), R.B, R.S, 4, cos, sin, qw, kw, R.EPS, raw.float(), nkv=2)
    with pytest.raises(NotImplementedError, match="head_dim"):  # the row read as 16 heads of 32
        hip.qknorm_rope_inplace(qkv, R.B, R.S, 8, cos, sin, qw, kw, R.EPS, raw, nkv=4)
    with pytest.raises(ValueError):
        hip.qknorm_bwd(qkv, raw[:, :-64].contiguous(), R.B, R.S, 4, qw, kw, R.EPS, dw[0], dw[1], nkv=2)
    with pytest.raises(TypeError):
        hip.qknorm_bwd(qkv, raw, R.B, R.S, 4, qw, kw, R.EPS, dw[0].double(), dw[1], nkv=2)
    with pytest.raises(ValueError):
        hip.qknorm_bwd(qkv, raw, R.B, R.S, 4, qw, kw, R.EPS, dw[0], dw[1], nkv=2, ws=torch.empty(16, device=DEV))
    assert torch.equal(qkv.cpu(), inp.qkv), "a refused call wrote its input"


# ------------------------------------------------------------------ engine
SEP = 3


def _cfg(dropout=0.1, **kw):
    d = dict(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, max_seq_len=192, dropout=dropout,
             attention_dropout=dropout, qk_norm=True)
    d.update(kw)
    return GPTConfig(**d)


def _model(cfg, seed):
    """A model with non-unit q_norm / k_norm weights (the init is ones)."""
    torch.manual_seed(seed)
    m = GPT(cfg)
    with torch.no_grad():
        for layer in m.layers:
            for n in (layer.attention.q_norm, layer.attention.k_norm):
                n.weight.copy_(1.0 + 0.5 * torch.randn(n.weight.shape))
                n.weight[5] = -0.5
    return m.to(DEV)


def _grads(m):
    return {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()


def _ids(cfg, n=2, seed=0, sep=None):
    ids = torch.randint(4, 1000, (n, cfg.max_seq_len), device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
    if sep is not None:
        ids[0, [0, 1, 70, 150]] = sep
        ids[1:, cfg.max_seq_len // 2] = sep
    return ids


@pytest.mark.parametrize("dropout,nkv,sep", [(0.0, None, None), (0.1, None, None), (0.1, 2, None), (0.1, 2, SEP)])
def test_engine_hip_vs_reference_ops(dropout, nkv, sep):
    """Same 16-bit weights, activations and dropout masks through the HIP ops and through the
    reference ops: loss and every gradient at the engine tolerances of the other GPU suites."""
    cfg = _cfg(dropout, num_kv_heads=nkv)
    base = _model(cfg, 0)
    base.set_doc_separator(sep)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    e1 = m1.enable_engine(seed=5)
    m2.enable_engine(seed=5, ops=ops.CPU_OPS)
    assert e1.qk_norm and e1.ops.backend == "hip" and e1.packed_qkv and e1.gqa == (nkv is not None)
    ids = _ids(cfg, sep=sep)
    _, l1 = m1(ids, labels=ids)
    (l1 / 2).backward()
    _, l2 = m2(ids, labels=ids)
    (l2 / 2).backward()
    assert abs(l1.item() - l2.item()) < 2e-2 * abs(l2.item())
    g1, g2 = _grads(m1), _grads(m2)
    assert g1["layers.0.attention.q_norm.weight"].shape == (64,) and g1["layers.1.attention.k_norm.weight"].abs().max() > 0
    for n in g1:
        assert _cos(g1[n], g2[n]) > 0.99, n
        r = g1[n].norm() / g2[n].norm()
        assert 0.95 < r.item() < 1.05, (n, r.item())


def test_engine_recompute_is_bit_identical():
    """No recompute, recompute with the QKV output and raw kept, and with both regenerated."""
    base = _model(_cfg(0.1, num_kv_heads=2), 2)
    ids = _ids(base.config, seed=2)
    res = []
    for ac, budget in ((False, None), (True, None), (True, 0.0)):
        m = copy.deepcopy(base)
        eng = m.enable_engine(seed=7)
        if budget is not None:
            eng.ac_budget = budget
        m.gradient_checkpointing = ac
        _, loss = m(ids, labels=ids)
        loss.backward()
        res.append((loss.item(), _grads(m)))
    for loss, g in res[1:]:
        assert loss == res[0][0]
        for n in g:
            assert torch.equal(res[0][1][n], g[n]), n


@pytest.mark.parametrize("recompute", [False, True])
def test_train_window_matches_sequential_bit_for_bit(recompute):
    from distributed_llm_trainer_amd.models.engine import shift_targets
    base = _model(_cfg(0.1, num_kv_heads=2), 5)
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
    for a, b in zip(seq, win):
        assert a == b.item(), (seq, [w.item() for w in win])
    g1, g2 = _grads(m1), _grads(m2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), (n, (g1[n] - g2[n]).abs().max().item())


def test_training_is_bitwise_reproducible():
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    cfg = _cfg(0.1, num_kv_heads=2)
    data = _ids(cfg, n=8, seed=3)
    res = []
    for _ in range(2):
        torch.manual_seed(3)
        tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=4, warmup_steps=1, learning_rate=1e-3,
                            micro_step_fusion=1)
        tr = DistributedTrainer(cfg, tc)
        assert tr.use_engine and tr.model.engine.qk_norm
        losses = [tr.train_step({"input_ids": data})["loss"] for _ in range(3)]
        res.append((losses, tr.flat_params().detach().clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]), (res[0][1] - res[1][1]).abs().max().item()
    s = tr.model.store.layout.by_name["layers.0.attention.q_norm.weight"]
    assert not torch.equal(res[0][1][s.offset:s.offset + s.numel].cpu(), torch.ones(64)), "q_norm never trained"


def test_unsupported_routes_refuse_at_enable_engine(monkeypatch):
    m = GPT(_cfg(0.0)).to(DEV)
    with pytest.raises(NotImplementedError, match="fp32"):
        m.enable_engine(act_dtype=torch.float32)
    assert m.engine is None and m.store is None
    m96 = GPT(_cfg(0.0, hidden_size=384)).to(DEV)  # head_dim 96: the zero-padded route
    with pytest.raises(NotImplementedError, match="head_dim"):
        m96.enable_engine()
    with pytest.raises(NotImplementedError):
        ops.check_attention_features(DEV, 192, torch.bfloat16, {"qk_norm"})  # the GEMM-formulated route
    ops.check_attention_features(DEV, 64, torch.float16, {"qk_norm"})
    ops.check_attention_features(DEV, 128, torch.bfloat16, {"qk_norm"})
    monkeypatch.setenv("DLT_PACKED_QKV", "0")
    with pytest.raises(NotImplementedError, match="packed"):
        GPT(_cfg(0.0)).to(DEV).enable_engine()
    GPT(_cfg(0.0, qk_norm=False)).to(DEV).enable_engine()  # without the flag the split layout still runs


def test_generate_runs_on_the_aten_step():
    from distributed_llm_trainer_amd.eval.decode import _fused_kind
    m = _model(_cfg(0.0), 3)
    m.enable_engine()
    assert _fused_kind(m, 1) is None and _fused_kind(m, 4) is None
    ids = _ids(m.config, n=1, seed=4)[:, :17]
    g = m.generate(ids, max_new_tokens=4, top_k=1)
    assert g.shape == (1, 21)
    for t in range(4):  # greedy KV-cached decode == argmax of a full re-forward at each step
        with torch.no_grad():
            lg, _ = m(g[:, :17 + t])
        assert lg[0, -1].argmax().item() == g[0, 17 + t].item() or \
            (lg[0, -1].max() - lg[0, -1][g[0, 17 + t]]).abs().item() < 0.05
