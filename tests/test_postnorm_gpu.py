"""Post-norms on the GPU: ``k_postnorm_fwd`` / ``k_postnorm_bwd`` against the fp64 references of
tests/postnorm_ref.py (tolerances derived there; the planted defects that fall outside them are
in test_postnorm_cpu.py, at these inputs), the fused ``k_postnorm_add_dropout_rmsnorm_fwd``
bit for bit against the two-kernel sequence, bitwise properties of the weight gradient, host
validation, and the engine with ``GPTConfig.post_norm``: HIP ops against the reference ops with
identical dropout masks, recompute, the window, reproducibility, the fp32 refusal and generation.

Shapes: M = 403 rows (the last 4-row workgroup is part empty), H = 64 (fewer chunks than lanes),
768 (NCH 3 exact), 1000 (a part-filled last chunk), 2560 (the NCH 12 form); bf16 / fp16; one
all-zero row, one row scaled by 1e4, weights with negative and exactly-zero entries."""
import copy
import functools

import pytest
import torch

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip
from tests import postnorm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
CASES = [(H, dt) for H in R.HS for dt in DTYPES]
GUARD = 4096  # elements on each side of a guarded buffer
SENT16, SENT32 = 123.0, -7.5  # exact in bf16 / fp16 / fp32


@functools.lru_cache(maxsize=None)
def _case(H, dtype):
    """Inputs and fp64 references of a case, computed once and never written."""
    inp = R.make_inputs(H, dtype)
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


def _w(inp, w16: bool, which="w"):
    """The weight as the DDP store (fp32) or a gathered FSDP unit (activation dtype) hands it over."""
    w = getattr(inp, which).to(DEV)
    return w.to(inp.a.dtype) if w16 else w


def _as16(inp):
    """``inp`` with the weights a 16-bit hand-over carries (rounded to the activation dtype)."""
    return inp._replace(w=inp.w.to(inp.a.dtype).float(), w2=inp.w2.to(inp.a.dtype).float())


@pytest.mark.parametrize("w16", [False, True])
@pytest.mark.parametrize("H,dtype", CASES)
def test_forward(H, dtype, w16):
    inp, fref, _ = _case(H, dtype)
    if w16:
        inp = _as16(inp)
        fref = R.fwd_ref(inp)
    a = inp.a.to(DEV)
    ubuf, u = _guarded(shape=a.shape, dtype=dtype)
    assert hip.postnorm_fwd(a, _w(inp, w16), R.EPS, out=u) is u
    torch.cuda.synchronize()
    worst = R.worst(u.cpu(), fref)
    print(f"postnorm_fwd H={H} {dtype} w16={w16}: worst |err| / tol = {worst:.3f}")
    assert worst <= 1.0
    assert _guards_intact(ubuf) and torch.equal(a.cpu(), inp.a), "the input was written or the output overran"
    u2 = hip.postnorm_fwd(a, _w(inp, w16), R.EPS)
    assert u2.data_ptr() != a.data_ptr() and torch.equal(u2, u), "repeat call differs"


@pytest.mark.parametrize("w16", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H,dtype", CASES)
def test_fused_forward_is_bit_identical_to_the_two_kernel_sequence(H, dtype, p, w16):
    inp, _, _ = _case(H, dtype)
    a, resid = inp.a.to(DEV), inp.resid.to(DEV)
    wp, w2 = _w(inp, w16), _w(inp, w16, "w2")
    u = hip.postnorm_fwd(a, wp, R.EPS)
    x0, y0, r0 = hip.add_dropout_rmsnorm_fwd(resid, u, w2, R.EPS, p, R.KEY, dtype)
    ybuf, y_out = _guarded(shape=a.shape, dtype=dtype)
    x1, y1, r1 = hip.postnorm_add_dropout_rmsnorm_fwd(resid, a, wp, w2, R.EPS, p, R.KEY, dtype, y_out=y_out)
    torch.cuda.synchronize()
    assert y1 is y_out and _guards_intact(ybuf)
    assert torch.equal(x0, x1), (x0 - x1).abs().max().item()
    assert torch.equal(y0, y1) and torch.equal(r0, r1)
    assert torch.equal(a.cpu(), inp.a) and torch.equal(resid.cpu(), inp.resid), "an input was written"
    if p > 0:  # the mask is live, and it is the one of the unfused kernel
        xn = hip.add_dropout_rmsnorm_fwd(resid, u, w2, R.EPS, 0.0, R.KEY, dtype)[0]
        dropped = (x1 == resid) & (xn != resid)
        assert 0.05 < dropped.float().mean().item() < 0.15
    f = R.fused_ref(_as16(inp) if w16 else inp, p)
    worst = (R.worst(x1.cpu(), f.x), R.worst(y1.cpu(), f.y), R.worst(r1.cpu(), f.rstd))
    print("fused forward worst |err| / tol: x %.3f y %.3f rstd %.3f" % worst)
    assert max(worst) <= 1.0


def _bwd(inp, w16=False, dw0=None):
    M, H = inp.a.shape
    gbuf, du = _guarded(inp.du)
    a = inp.a.to(DEV)
    n_ws = hip.postnorm_bwd_workspace(M, H, DEV).numel()
    wbuf, ws = _guarded(shape=(n_ws,), dtype=torch.float32, sentinel=SENT32)
    dbuf, dw = _guarded(shape=(H,), dtype=torch.float32, sentinel=SENT32)
    if dw0 is None:
        dw.zero_()
    else:
        dw.copy_(dw0)
    assert hip.postnorm_bwd(du, a, _w(inp, w16), R.EPS, dw, ws=ws) is du
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), inp.a), "a was written"
    assert _guards_intact(gbuf) and _guards_intact(wbuf, SENT32) and _guards_intact(dbuf, SENT32)
    assert bool((ws != SENT32).all()), "a workspace row was left unwritten"
    return du, dw.clone()


@pytest.mark.parametrize("w16", [False, True])
@pytest.mark.parametrize("H,dtype", CASES)
def test_backward(H, dtype, w16):
    inp, _, bref = _case(H, dtype)
    if w16:
        inp = _as16(inp)
        bref = R.bwd_ref(inp)
    da, dw = _bwd(inp, w16)
    worst = (R.worst(da.cpu(), bref.da), R.worst(dw, bref.dw))
    print("postnorm_bwd H=%d %s w16=%s worst |err| / tol: da %.3f dw %.3f" % (H, dtype, w16, *worst))
    assert max(worst) <= 1.0
    # repeat from equal state: the same bits (fixed-order reduction, no atomics)
    da2, dw2 = _bwd(inp, w16)
    assert torch.equal(da, da2) and torch.equal(dw, dw2)
    # dw accumulates: a second call on top of the first adds the same sum again -- exactly twice
    _, acc = _bwd(inp, w16, dw)
    assert torch.equal(acc, 2 * dw)
    # without an explicit workspace the binding allocates it
    g, d0 = inp.du.to(DEV), torch.zeros(H, device=DEV)
    hip.postnorm_bwd(g, inp.a.to(DEV), _w(inp, w16), R.EPS, d0)
    assert torch.equal(g, da) and torch.equal(d0, dw)


def test_host_validation():
    inp, _, _ = _case(64, torch.bfloat16)
    a, du, resid, w, w2 = inp.a.to(DEV), inp.du.to(DEV), inp.resid.to(DEV), inp.w.to(DEV), inp.w2.to(DEV)
    out, dw = torch.full_like(a, SENT16), torch.full((64,), SENT32, device=DEV)
    y = torch.full_like(a, SENT16)
    bad = [
        (ValueError, lambda: hip.postnorm_fwd(a[:, :62].contiguous(), w[:62], R.EPS)),            # H % 4
        (ValueError, lambda: hip.postnorm_fwd(a.view(-1), w, R.EPS)),                             # not [M, H]
        (ValueError, lambda: hip.postnorm_fwd(a, w[:32], R.EPS, out=out)),                        # weight length
        (ValueError, lambda: hip.postnorm_fwd(a, w.cpu(), R.EPS, out=out)),                       # weight device
        (ValueError, lambda: hip.postnorm_fwd(a, w, R.EPS, out=out[:-1])),                        # out shape
        (ValueError, lambda: hip.postnorm_fwd(a, w, R.EPS, out=a)),                               # in place
        (TypeError, lambda: hip.postnorm_fwd(a, w, R.EPS, out=out.half())),                       # out dtype
        (ValueError, lambda: hip.postnorm_fwd(a.t(), w, R.EPS)),                                  # not contiguous
        (ValueError, lambda: hip.postnorm_fwd(a.cpu(), w, R.EPS)),                                # activations device
        (ValueError, lambda: hip.postnorm_fwd(torch.zeros(4, 4100, dtype=a.dtype, device=DEV),
                                              torch.ones(4100, device=DEV), R.EPS)),              # H > 4096
        (NotImplementedError, lambda: hip.postnorm_fwd(a.float(), w, R.EPS)),                     # fp32 activations
        (TypeError, lambda: hip.postnorm_fwd(a.double(), w, R.EPS)),
        (ValueError, lambda: hip.postnorm_add_dropout_rmsnorm_fwd(resid[:-1], a, w, w2, R.EPS, 0.1, 1, a.dtype, y_out=y)),
        (TypeError, lambda: hip.postnorm_add_dropout_rmsnorm_fwd(resid.half(), a, w, w2, R.EPS, 0.1, 1, a.dtype, y_out=y)),
        (ValueError, lambda: hip.postnorm_add_dropout_rmsnorm_fwd(None, a, w, w2, R.EPS, 0.1, 1, a.dtype, y_out=y)),
        (ValueError, lambda: hip.postnorm_add_dropout_rmsnorm_fwd(resid, a, w[:32], w2, R.EPS, 0.1, 1, a.dtype, y_out=y)),
        (ValueError, lambda: hip.postnorm_add_dropout_rmsnorm_fwd(resid, a, w, w2[:32], R.EPS, 0.1, 1, a.dtype, y_out=y)),
        (ValueError, lambda: hip.postnorm_add_dropout_rmsnorm_fwd(resid, a, w, w2, R.EPS, 1.0, 1, a.dtype, y_out=y)),
        (TypeError, lambda: hip.postnorm_add_dropout_rmsnorm_fwd(resid, a, w, w2, R.EPS, 0.1, 1, torch.float16, y_out=y)),
        (TypeError, lambda: hip.postnorm_add_dropout_rmsnorm_fwd(resid, a, w, w2, R.EPS, 0.1, 1, a.dtype, y_out=y.half())),
        (NotImplementedError, lambda: hip.postnorm_add_dropout_rmsnorm_fwd(resid, a.float(), w, w2, R.EPS, 0.1, 1,
                                                                             torch.float32)),
        (ValueError, lambda: hip.postnorm_bwd(du, a[:-1], w, R.EPS, dw)),                         # a shape
        (TypeError, lambda: hip.postnorm_bwd(du, a.half(), w, R.EPS, dw)),                        # a dtype
        (ValueError, lambda: hip.postnorm_bwd(du, du, w, R.EPS, dw)),                             # aliased
        (ValueError, lambda: hip.postnorm_bwd(du, a, w[:32], R.EPS, dw)),
        (TypeError, lambda: hip.postnorm_bwd(du, a, w, R.EPS, dw.double())),
        (ValueError, lambda: hip.postnorm_bwd(du, a, w, R.EPS, dw[:32])),
        (ValueError, lambda: hip.postnorm_bwd(du, a, w, R.EPS, dw, ws=torch.empty(16, device=DEV))),
        (ValueError, lambda: hip.postnorm_bwd(du, a, w, R.EPS, dw.cpu())),
        (NotImplementedError, lambda: hip.postnorm_bwd(du.float(), a.float(), w, R.EPS, dw)),
        (ValueError, lambda: hip.postnorm_bwd_workspace(4, 62, DEV)),
    ]
    for exc, call in bad:
        with pytest.raises(exc):
            call()
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), inp.a) and torch.equal(du.cpu(), inp.du) and torch.equal(resid.cpu(), inp.resid)
    assert bool((out == SENT16).all()) and bool((y == SENT16).all()) and bool((dw == SENT32).all()), \
        "a refused call wrote an output"
    assert hip.postnorm_bwd_workspace(R.M, 64, DEV).shape == (101 * 64,)
    assert hip.postnorm_bwd_workspace(5000, 64, DEV).shape == (1024 * 64,)


# ------------------------------------------------------------------ engine
SEP = 3
POST = ("attn_post_norm", "mlp_post_norm")


def _cfg(dropout=0.1, **kw):
    d = dict(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, max_seq_len=192, dropout=dropout,
             attention_dropout=dropout, post_norm=True)
    d.update(kw)
    return GPTConfig(**d)


def _model(cfg, seed):
    """A model with non-unit post-norm weights (the init is ones)."""
    torch.manual_seed(seed)
    m = GPT(cfg)
    with torch.no_grad():
        for layer in m.layers:
            for name in POST:
                n = getattr(layer, name)
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


@pytest.mark.parametrize("dropout,kw,sep", [
    (0.0, {}, None), (0.1, {}, None), (0.1, {"num_kv_heads": 2}, None), (0.1, {}, SEP),
    (0.1, {"sliding_window": 64}, None), (0.1, {"qk_norm": True, "attention_sinks": True}, None)])
def test_engine_hip_vs_reference_ops(dropout, kw, sep):
    """Same 16-bit weights, activations and dropout masks through the HIP ops and through the
    reference ops: loss and every gradient at the engine tolerances of the other GPU suites."""
    cfg = _cfg(dropout, **kw)
    base = _model(cfg, 0)
    base.set_doc_separator(sep)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    e1 = m1.enable_engine(seed=5)
    m2.enable_engine(seed=5, ops=ops.CPU_OPS)
    assert e1.post_norm and e1.ops.backend == "hip" and e1.provider.layer(1).pn2.shape == (256,)
    ids = _ids(cfg, sep=sep)
    _, l1 = m1(ids, labels=ids)
    (l1 / 2).backward()
    _, l2 = m2(ids, labels=ids)
    (l2 / 2).backward()
    print(f"loss hip {l1.item():.5f} reference ops {l2.item():.5f}")
    assert abs(l1.item() - l2.item()) < 2e-2 * abs(l2.item())
    g1, g2 = _grads(m1), _grads(m2)
    for i in range(2):
        for n in POST:
            assert g1[f"layers.{i}.{n}.weight"].shape == (256,) and g1[f"layers.{i}.{n}.weight"].abs().max() > 0
    for n in g1:
        assert _cos(g1[n], g2[n]) > 0.99, n
        r = g1[n].norm() / g2[n].norm()
        assert 0.95 < r.item() < 1.05, (n, r.item())


def test_engine_recompute_is_bit_identical():
    """No recompute, selective recompute (a / d_out kept), and with a zero keep budget."""
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
        assert tr.use_engine and tr.model.engine.post_norm
        losses = [tr.train_step({"input_ids": data})["loss"] for _ in range(3)]
        res.append((losses, tr.flat_params().detach().clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]), (res[0][1] - res[1][1]).abs().max().item()
    for n in POST:
        s = tr.model.store.layout.by_name[f"layers.0.{n}.weight"]
        assert not torch.equal(res[0][1][s.offset:s.offset + s.numel].cpu(), torch.ones(256)), f"{n} never trained"


def test_fp32_activations_refuse_at_enable_engine():
    m = GPT(_cfg(0.0)).to(DEV)
    with pytest.raises(NotImplementedError, match="post_norm"):
        m.enable_engine(act_dtype=torch.float32)
    assert m.engine is None and m.store is None
    m.enable_engine(act_dtype=torch.float16)  # the 16-bit formats run
    GPT(_cfg(0.0, post_norm=False)).to(DEV).enable_engine(act_dtype=torch.float32)  # without the flag fp32 still runs


def test_generate_runs_on_the_aten_step():
    from distributed_llm_trainer_amd.eval.decode import _fused_kind
    m = _model(_cfg(0.0), 3)
    m.enable_engine()
    assert _fused_kind(m, 1) is None and _fused_kind(m, 4) is None
    off = GPT(_cfg(0.0, post_norm=False)).to(DEV)
    off.enable_engine()
    assert _fused_kind(off, 1) == "mha"  # the default model keeps its fused step
    ids = _ids(m.config, n=1, seed=4)[:, :17]
    g = m.generate(ids, max_new_tokens=4, top_k=1)
    assert g.shape == (1, 21)
    for t in range(4):  # greedy KV-cached decode == argmax of a full re-forward at each step
        with torch.no_grad():
            lg, _ = m(g[:, :17 + t])
        assert lg[0, -1].argmax().item() == g[0, 17 + t].item() or \
            (lg[0, -1].max() - lg[0, -1][g[0, 17 + t]]).abs().item() < 0.05
