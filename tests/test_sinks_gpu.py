"""Attention sinks on the MI355X: the SINK forms of the flash forward (attention_sink.hip),
``k_attn_sink_bwd`` and the existing backward kernels fed the sink forward's lse, against the fp64
references and derived tolerances of tests/sink_ref.py (the planted defects that fall outside
them are in test_sinks_cpu.py, at these inputs), with sentinel guards around every output; the
engine with ``GPTConfig.attention_sinks``; the ``sink=`` forms of the fused decode kernels, the
captured step and ``generate``.

Each check prints ``RATIO <output> <worst err / tol>`` (``pytest -s`` shows them)."""
import copy
import ctypes
import functools

import pytest
import torch

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip, rng
from distributed_llm_trainer_amd.ops.reference import WindowBounds
from tests import attn_ref as A
from tests import decode_gqa_ref as G
from tests import sink_ref as SR
from tests.test_attn_kernels_gpu import SENT, _args, _d, check
from tests.test_decode_gqa_gpu import Guarded as DGuarded, _bits, _dev, _pos, check as dcheck

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
NINF = float("-inf")


# ------------------------------------------------------------------ 1. the kernels
def _bounds(c, inp):
    window = A.case_window(c)
    if window is not None and window >= c.S:  # a window that covers the sequence is no window
        return None, window
    if inp.doc is None:
        return None, None
    lo, hi = _d(inp.doc[0]), _d(inp.doc[1])
    return (WindowBounds(lo, hi, window) if window is not None else (lo, hi)), window


def _run_direct(c, r, sink, doc, window, dsink0=None, o16=None, lse32=None):
    """Head-major: dlt_attn_fwd / dlt_attn_bwd on a hand-filled _AttnArgs, every output guarded."""
    inp = r.inp
    B, nh, S, hd, dt = c.B, c.nh, c.S, c.hd, c.dtype
    q, k, v, do = _d(inp.q), _d(inp.k), _d(inp.v), _d(inp.do)
    thr = rng.keep_threshold(c.p)
    dscale = 1.0 / (1.0 - c.p) if thr else 1.0
    O = A.Guarded((B * S, nh * hd), dt, SENT[dt], DEV)
    L = A.Guarded((B, nh, S), F32, SENT[F32], DEV)
    M = A.Guarded((2, B * nh, (S + 31) // 32, S), I32, SENT[I32], DEV) if thr else None
    gen = 1
    if thr and window is not None and window < S:
        hip.attention_dropout_mask(B, nh, S, c.p, c.key, window=window, out=M.t)
        gen = 0
    _, sq, skv = hip._head_major(q, k, v)
    st = dict(q=sq, kv=skv, dq=sq, dkv=skv)
    common = dict(q=q, k=k, v=v, lo=doc[0] if doc else None, B=B, nh=nh, nkv=c.nkv, S=S, hd=hd, hk=int(dt == A.HF),
                  scale=inp.scale, dscale=dscale, key=c.key, thr=thr, mask=M.t if M else None, sink=sink)
    L_, stream = hip.lib(), hip._stream()
    assert L_.dlt_attn_fwd(ctypes.byref(_args(o=O.t, lse=L.t, gen_mask=gen, strides=st, **common)), stream) == 0
    DQ = A.Guarded(tuple(inp.q.shape), dt, SENT[dt], DEV)
    DK, DV = (A.Guarded(tuple(inp.k.shape), dt, SENT[dt], DEV) for _ in range(2))
    DL = A.Guarded((B, nh, S), F32, SENT[F32], DEV)
    DS = A.Guarded((nh,), F32, SENT[F32], DEV, init=torch.zeros(nh) if dsink0 is None else dsink0)
    assert L_.dlt_attn_bwd(ctypes.byref(_args(o=_d(r.o16 if o16 is None else o16), lse=_d(r.lse32 if lse32 is None else lse32),
                                              dout=do, delta_ws=DL.t, dq=DQ.t, dk=DK.t, dv=DV.t,
                                              hi=doc[1] if doc else None, dsink=DS.t if sink is not None else None,
                                              strides=st, **common)), stream) == 0
    torch.cuda.synchronize()
    for g in (O, L, DQ, DK, DV, DL):
        g.assert_guards()
    DS.assert_guards(written=None if sink is not None else torch.zeros(nh, dtype=torch.bool, device=DEV))
    return dict(o=O.t, lse=L.t, dq=DQ.t, dk=DK.t, dv=DV.t, delta=DL.t, dsink=DS.t)


def _run_packed(c, r, sink, doc, window, dsink0=None, stored_mask=True):
    """Packed QKV through attention_fwd_packed / attention_bwd_packed with guarded ``out=`` buffers."""
    inp = r.inp
    B, nh, S, hd, dt, kvh = c.B, c.nh, c.S, c.hd, c.dtype, c.kvh
    H, KV = nh * hd, kvh * hd
    qkv = _d(A.pack_qkv(inp))
    thr = rng.keep_threshold(c.p)
    O = A.Guarded((B * S, H), dt, SENT[dt], DEV)
    M = A.Guarded((2, B * nh, (S + 31) // 32, S), I32, SENT[I32], DEV) if thr else None
    if thr:  # made ahead, as the engine does: the forward then runs with gen_mask = 0
        hip.attention_dropout_mask(B, nh, S, c.p, c.key, window=window, out=M.t)
    kw = dict(doc=doc, nkv=c.nkv or None, window=window)
    skw = dict(sink=sink) if sink is not None else {}
    o, aux = hip.attention_fwd_packed(qkv, B, S, nh, c.p, c.key, out=O.t, mask=M.t if M else None, **kw, **skw)
    Gd = A.Guarded((B * S, H + 2 * KV), dt, SENT[dt], DEV)
    DS = A.Guarded((nh,), F32, SENT[F32], DEV, init=torch.zeros(nh) if dsink0 is None else dsink0)
    if sink is not None:
        skw["dsink"] = DS.t
    cos, sin = _d(inp.rope[0]), _d(inp.rope[1])
    hip.attention_bwd_packed(qkv, _d(r.o16), _d(inp.do), hip.AttnAux((_d(r.lse32), M.t if (M and stored_mask) else None)),
                             c.p, c.key, B, S, nh, cos, sin, out=Gd.t, **kw, **skw)
    torch.cuda.synchronize()
    for g in (O, Gd):
        g.assert_guards()
    DS.assert_guards(written=None if sink is not None else torch.zeros(nh, dtype=torch.bool, device=DEV))
    hm = lambda t, h: t.view(B, S, h, hd).transpose(1, 2)  # noqa: E731
    return dict(o=O.t, lse=aux[0], dq=hm(Gd.t[:, :H], nh), dk=hm(Gd.t[:, H:H + KV], kvh), dv=hm(Gd.t[:, H + KV:], kvh),
                dsink=DS.t)


def _same(a, b, tag):
    for nm in a:
        assert torch.equal(A.bits(a[nm].contiguous()), A.bits(b[nm].contiguous())), f"{tag} {nm}: the bits differ"


@pytest.mark.parametrize("name", [c.name for c in SR.CASES])
def test_sink_forward_and_backward(name):
    c, r = SR.BY_NAME[name], SR.case_refs(name)
    doc, window = _bounds(c, r.inp)
    run = _run_packed if c.packed else _run_direct
    sink = _d(r.sink)
    outs = run(c, r, sink, doc, window)
    print(f"SINKS {r.sink.tolist()}")
    assert torch.isfinite(outs["o"].float()).all() and torch.isfinite(outs["lse"]).all()
    check(name + " o", outs["o"], r.fwd.o)
    check(name + " lse", outs["lse"], r.fwd.lse)
    # the existing backward kernels, fed the sink forward's lse, at attn_ref's backward tolerances
    # (the one "big" case, an extra of this file, adds the exp2 flush term: sink_ref.bwd_flush_terms)
    for nm in ("dq", "dk", "dv"):
        check(f"{name} {nm}", outs[nm], getattr(r.bwd, nm))
    if "delta" in outs:
        check(name + " delta", outs["delta"], r.bwd.delta)
    check(name + " dsink", outs["dsink"], r.dsink)
    # two calls on equal inputs: the same bits (fixed-order reduction, no atomics)
    again = run(c, r, sink, doc, window)
    _same(outs, again, name)
    # a second accumulating call gives twice the first
    acc = run(c, r, sink, doc, window, dsink0=outs["dsink"].cpu())
    assert torch.equal(acc["dsink"], 2 * outs["dsink"]), (acc["dsink"], outs["dsink"])
    # a head with sink = +100 over scores of order 1: o near 0, lse near the sink
    if c.family == "gauss":
        for h in (r.sink == 100.0).nonzero().flatten().tolist():
            oh = outs["o"].view(c.B, c.S, c.nh, c.hd)[:, :, h].float()
            assert oh.abs().max().item() < 1e-30 and (outs["lse"][:, h] - 100.0).abs().max().item() < 1e-4
    # all sinks -inf: o and lse are the plain kernels', bit for bit, and dsink stays zero
    none = torch.full((c.nh,), NINF, device=DEV)
    plain = run(c, r, None, doc, window)
    minf = run(c, r, none, doc, window)
    for nm in ("o", "lse"):
        assert torch.equal(A.bits(plain[nm].contiguous()), A.bits(minf[nm].contiguous())), f"{name} {nm}: -inf sinks != plain"
    assert not minf["dsink"].any() and not plain["dsink"].any()


@pytest.mark.parametrize("name", [c.name for c in SR.CASES if c.p > 0 and c.packed][:4])
def test_regenerated_keep_bits_give_the_same_bits(name):
    c, r = SR.BY_NAME[name], SR.case_refs(name)
    doc, window = _bounds(c, r.inp)
    a = _run_packed(c, r, _d(r.sink), doc, window, stored_mask=True)
    b = _run_packed(c, r, _d(r.sink), doc, window, stored_mask=False)
    _same(a, b, name)


def test_head_major_wrappers_and_host_validation():
    c = SR.DEFECT_CASE
    r = SR.case_refs(c.name)
    q, k, v, do = _d(r.inp.q), _d(r.inp.k), _d(r.inp.v), _d(r.inp.do)
    sink = _d(r.sink)
    o, aux = hip.attention_fwd(q, k, v, c.p, c.key, sink=sink)
    check("hm o", o, r.fwd.o)
    check("hm lse", aux[0], r.fwd.lse)
    ds = torch.zeros(c.nh, device=DEV)
    dq, dk, dv = hip.attention_bwd(q, k, v, _d(r.o16), do, hip.AttnAux((_d(r.lse32), aux[1])), c.p, c.key, sink=sink, dsink=ds)
    check("hm dv", dv, r.bwd.dv)  # (the case is a packed one: its dq / dk references carry the inverse RoPE)
    check("hm dsink", ds, r.dsink)
    # a 16-bit sink (a gathered FSDP unit) is upcast
    o16, _ = hip.attention_fwd(q, k, v, c.p, c.key, sink=sink.bfloat16())
    o32, _ = hip.attention_fwd(q, k, v, c.p, c.key, sink=sink.bfloat16().float())
    assert torch.equal(o16, o32)
    for bad in (sink[:3], sink.cpu(), sink.long(), [0.0] * c.nh):
        with pytest.raises((ValueError, TypeError)):
            hip.attention_fwd(q, k, v, c.p, c.key, sink=bad)
    with pytest.raises(ValueError, match="together"):
        hip.attention_bwd(q, k, v, _d(r.o16), do, hip.AttnAux((_d(r.lse32), aux[1])), c.p, c.key, sink=sink)
    with pytest.raises(ValueError):
        hip.attention_bwd(q, k, v, _d(r.o16), do, hip.AttnAux((_d(r.lse32), aux[1])), c.p, c.key, sink=sink,
                          dsink=ds.double())
    with pytest.raises(NotImplementedError, match="fp32"):
        hip.attention_fwd(q.float(), k.float(), v.float(), 0.0, 0, sink=sink)
    assert hip.lib().dlt_attn_args_size() == ctypes.sizeof(hip._AttnArgs) == 248


# ------------------------------------------------------------------ 2. the engine
SEP = 3


def _cfg(dropout=0.1, **kw):
    d = dict(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, max_seq_len=192, dropout=dropout,
             attention_dropout=dropout, attention_sinks=True)
    d.update(kw)
    return GPTConfig(**d)


def _model(cfg, seed):
    """A model with non-zero sinks (the init is zeros), one of them far above the scores."""
    torch.manual_seed(seed)
    m = GPT(cfg)
    with torch.no_grad():
        for layer in m.layers:
            layer.attention.sinks.copy_(1.5 * torch.randn(layer.attention.sinks.shape))
            layer.attention.sinks[1] = 4.0
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


COMBO = dict(num_kv_heads=2, qk_norm=True, sliding_window=64, sliding_window_pattern=2)


@pytest.mark.parametrize("dropout,kw,sep", [(0.0, {}, None), (0.1, {}, None), (0.1, COMBO, SEP),
                                            (0.1, {"hidden_size": 384}, None)])
def test_engine_hip_vs_reference_ops(dropout, kw, sep):
    """Same 16-bit weights, activations and dropout masks through the HIP ops and through the
    reference ops: loss and every gradient at the engine tolerances of the other GPU suites.
    hidden_size 384: head_dim 96, zero-padded onto the flash kernels, which pass the sink through."""
    cfg = _cfg(dropout, **kw)
    base = _model(cfg, 0)
    base.set_doc_separator(sep)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    e1 = m1.enable_engine(seed=5)
    m2.enable_engine(seed=5, ops=ops.CPU_OPS)
    assert e1.sinks and e1.ops.backend == "hip" and e1.provider.layer(0).sk.dtype == torch.float32
    ids = _ids(cfg, sep=sep)
    _, l1 = m1(ids, labels=ids)
    (l1 / 2).backward()
    _, l2 = m2(ids, labels=ids)
    (l2 / 2).backward()
    assert abs(l1.item() - l2.item()) < 2e-2 * abs(l2.item())
    g1, g2 = _grads(m1), _grads(m2)
    assert g1["layers.0.attention.sinks"].shape == (4,) and g1["layers.1.attention.sinks"].abs().min() > 0
    for n in g1:
        assert _cos(g1[n], g2[n]) > 0.99, n
        r = g1[n].norm() / g2[n].norm()
        assert 0.95 < r.item() < 1.05, (n, r.item())


def test_engine_recompute_is_bit_identical():
    base = _model(_cfg(0.1, **COMBO), 2)
    base.set_doc_separator(SEP)
    ids = _ids(base.config, seed=2, sep=SEP)
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


def test_training_is_bitwise_reproducible_and_the_sinks_move():
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
        assert tr.use_engine and tr.model.engine.sinks
        losses = [tr.train_step({"input_ids": data})["loss"] for _ in range(3)]
        res.append((losses, tr.flat_params().detach().clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]), (res[0][1] - res[1][1]).abs().max().item()
    s = tr.model.store.layout.by_name["layers.0.attention.sinks"]
    assert res[0][1][s.offset:s.offset + 4].abs().min().item() > 0, "the sinks never moved from zero"
    assert not res[0][1][s.offset + 4:s.offset + 8].any(), "the padding moved"


def test_unsupported_routes_refuse_at_enable_engine():
    m = GPT(_cfg(0.0)).to(DEV)
    with pytest.raises(NotImplementedError, match="fp32"):
        m.enable_engine(act_dtype=torch.float32)
    assert m.engine is None and m.store is None
    with pytest.raises(NotImplementedError, match="attention sinks"):
        ops.check_attention_features(DEV, 192, torch.bfloat16, {"sinks"})  # the GEMM-formulated route
    m192 = GPT(_cfg(0.0, hidden_size=768)).to(DEV)  # head_dim 192
    with pytest.raises(NotImplementedError, match="attention sinks"):
        m192.enable_engine()
    for hd, dt in ((64, torch.float16), (128, torch.bfloat16), (96, torch.bfloat16), (32, torch.float16)):
        ops.check_attention_features(DEV, hd, dt, {"sinks"})
    ops.check_attention_features("cpu", 192, torch.float32, {"sinks"})


# ------------------------------------------------------------------ 3. decode
@functools.lru_cache(maxsize=None)
def _gqa_case(nh, nkv):
    return _dev(G.attn_gqa_inputs(nh, nkv, SR.DEC_MAXS, "randn"))


def _poison(kc, vc, kf, pos):
    k2, v2 = kc.clone(), vc.clone()
    k2[:, :, pos + 1:], v2[:, :, pos + 1:] = float("nan"), 3e38
    k2[:, :, :kf], v2[:, :, :kf] = float("nan"), 3e38
    return k2, v2


@pytest.mark.parametrize("W", SR.DEC_WINDOWS)
def test_dec_attn_sink(W):
    nh, Bn = 4, 2
    q, kc, vc = (t[:Bn].contiguous() for t in _gqa_case(nh, nh))
    sink = SR.sinks_for(nh, shift=2).to(DEV)
    for pos in SR.dec_positions(W, 4):
        k2, v2 = _poison(kc, vc, SR.WN.first_key(pos, W), pos)
        outs = []
        for _ in range(2):
            o = DGuarded((Bn, nh * 64), BF, -777.0)
            hip.dec_attn(q, k2, v2, _pos(pos), o.t, SR.DEC_SCALE, window=W or 0, sink=sink)
            o.assert_guards()
            outs.append(o.t)
        assert torch.isfinite(outs[0]).all()
        dcheck(f"dec_attn[sink,W={W},pos={pos}]", outs[0], SR.dec_sink_ref(q, kc, vc, pos, SR.DEC_SCALE, nh, sink, W))
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two calls, two results"
        # sink=None is the call without the argument, and -inf sinks add nothing
        a, b, c = (torch.empty(Bn, nh * 64, dtype=BF, device=DEV) for _ in range(3))
        hip.dec_attn(q, k2, v2, _pos(pos), a, SR.DEC_SCALE, window=W or 0)
        hip.dec_attn(q, k2, v2, _pos(pos), b, SR.DEC_SCALE, window=W or 0, sink=None)
        hip.dec_attn(q, k2, v2, _pos(pos), c, SR.DEC_SCALE, window=W or 0, sink=torch.full((nh,), NINF, device=DEV))
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))


@pytest.mark.parametrize("W", SR.DEC_WINDOWS)
@pytest.mark.parametrize("NS", SR.DEC_SPLITS)
@pytest.mark.parametrize("nh,nkv", SR.DEC_HEADS)
def test_dec_attn_gqa_sink(nh, nkv, NS, W):
    Bn = 2
    q, kc, vc = (t[:Bn].contiguous() for t in _gqa_case(nh, nkv))
    sink = SR.sinks_for(nh, shift=2).to(DEV)
    none = torch.full((nh,), NINF, device=DEV)
    for pos in SR.dec_positions(W, NS):
        k2, v2 = _poison(kc, vc, SR.WN.first_key(pos, W), pos)
        outs = []
        for _ in range(2):  # the second call on a fresh workspace full of NaN
            o = DGuarded((Bn, nh * 64), BF, -777.0)
            ws = DGuarded((Bn * nh * NS * hip.DEC_ATTN_WS,), F32, float("nan")) if NS > 1 else None
            hip.dec_attn_gqa(q, k2, v2, _pos(pos), o.t, SR.DEC_SCALE, nh, splits=NS, ws=None if ws is None else ws.t,
                             window=W or 0, sink=sink)
            o.assert_guards()
            if ws is not None:
                ws.assert_guards()
            outs.append(o.t)
        tag = f"dec_attn_gqa[sink,nh={nh},nkv={nkv},W={W},NS={NS},pos={pos}]"
        assert torch.isfinite(outs[0]).all(), tag
        dcheck(tag, outs[0], SR.dec_sink_ref(q, kc, vc, pos, SR.DEC_SCALE, nh, sink, W))
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two calls, two results"
        res = []
        for kw in ({}, {"sink": None}, {"sink": none}):
            o = torch.empty(Bn, nh * 64, dtype=BF, device=DEV)
            ws = hip.dec_attn_gqa_workspace(Bn, nh, NS, DEV) if NS > 1 else None
            hip.dec_attn_gqa(q, k2, v2, _pos(pos), o, SR.DEC_SCALE, nh, splits=NS, ws=ws, window=W or 0, **kw)
            res.append(o)
        assert torch.equal(_bits(res[0]), _bits(res[1])) and torch.equal(_bits(res[0]), _bits(res[2])), tag


def test_dec_sink_host_validation():
    nh, nkv = 4, 2
    q, kc, vc = (t[:1].contiguous() for t in _gqa_case(nh, nkv))
    o = torch.empty(1, nh * 64, dtype=BF, device=DEV)
    good = torch.zeros(nh, device=DEV)
    for bad in (good[:3], good.cpu(), good.long()):
        with pytest.raises(ValueError, match="sink"):
            hip.dec_attn_gqa(q, kc, vc, _pos(0), o, 0.125, nh, sink=bad)
    qm, km, vm = (t[:1].contiguous() for t in _gqa_case(nh, nh))
    with pytest.raises(ValueError, match="sink"):
        hip.dec_attn(qm, km, vm, _pos(0), o, 0.125, sink=good[:2])
    a, b = torch.empty_like(o), torch.empty_like(o)
    hip.dec_attn(qm, km, vm, _pos(9), a, 0.125, sink=good.bfloat16())  # a 16-bit sink is upcast
    hip.dec_attn(qm, km, vm, _pos(9), b, 0.125, sink=good)
    assert torch.equal(_bits(a), _bits(b))


def _dec_cfg(nkv, W):
    return GPTConfig(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=nkv, max_seq_len=256,
                     dropout=0.0, attention_dropout=0.0, sliding_window=W, attention_sinks=True)


@functools.lru_cache(maxsize=None)
def _dec_model(nkv, W):
    m = _model(_dec_cfg(nkv, W), 5 + nkv)
    m.enable_engine()
    m.eval()
    return m


DEC_MODELS = [(4, None), (2, None), (2, 64)]  # multi-head, grouped-query, windowed grouped-query


@pytest.mark.parametrize("nkv,W", DEC_MODELS)
def test_decode_fused_step_matches_torch_step(nkv, W, monkeypatch):
    """The captured fused step of a model with sinks == the ATen step: logits and the K/V rows it
    appends, over a 150-token context and 5 steps; two fused graphs bit for bit; the sinks are live."""
    from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, _fused_kind, forward_cached
    m = _dec_model(nkv, W)
    cfg = m.config
    Bn = 2
    monkeypatch.setenv("DLT_DECODE_FUSED", "1")
    assert _fused_kind(m, Bn) == ("mha" if nkv == 4 else "gqa")
    g = torch.Generator().manual_seed(50 + nkv)
    ids = torch.randint(0, 1000, (Bn, 150), generator=g).to(DEV)
    steps = torch.randint(0, 1000, (Bn, 5), generator=g).to(DEV)
    caches = [KVCache(cfg, Bn, DEV, m.engine.act_dtype) for _ in range(3)]
    graphs = []
    with torch.no_grad():
        for c, fused in zip(caches, ("1", "0", "1")):
            forward_cached(m, ids, c)
            monkeypatch.setenv("DLT_DECODE_FUSED", fused)
            graphs.append(DecodeGraph(m, c, c.len))
        assert graphs[0].fused and graphs[2].fused and not graphs[1].fused
        for t in range(steps.shape[1]):
            a = graphs[0](steps[:, t:t + 1]).clone()
            b = graphs[1](steps[:, t:t + 1]).clone()
            a2 = graphs[2](steps[:, t:t + 1]).clone()
            assert torch.allclose(a, b, atol=3e-2, rtol=3e-2), (t, (a - b).abs().max().item())
            assert torch.equal(a, a2), "two fused graphs on the same inputs, other logits"
        # the sinks are live in the fused step: the same weights without them give other logits
        off = GPT(GPTConfig.from_dict({k: v for k, v in cfg.to_dict().items() if k != "attention_sinks"})).to(DEV)
        off.load_state_dict(m.state_dict(), strict=False)
        off.enable_engine()
        off.eval()
        c0 = KVCache(cfg, Bn, DEV, m.engine.act_dtype)
        forward_cached(off, ids, c0)
        monkeypatch.setenv("DLT_DECODE_FUSED", "1")
        g0 = DecodeGraph(off, c0, c0.len)
        c1 = KVCache(cfg, Bn, DEV, m.engine.act_dtype)
        forward_cached(m, ids, c1)
        g1 = DecodeGraph(m, c1, c1.len)
        assert g0.fused and g1.fused
        assert (g0(steps[:, :1]) - g1(steps[:, :1])).abs().max().item() > 3e-2


@pytest.mark.parametrize("nkv,W", DEC_MODELS)
def test_generate_matches_the_greedy_full_reforward(nkv, W):
    m = _dec_model(nkv, W)
    ids = _ids(m.config, n=1, seed=4)[:, :100]
    g = m.generate(ids, max_new_tokens=6, top_k=1)
    assert g.shape == (1, 106)
    for t in range(6):  # greedy KV-cached decode == argmax of a full re-forward at each step
        with torch.no_grad():
            lg, _ = m(g[:, :100 + t])
        assert lg[0, -1].argmax().item() == g[0, 100 + t].item() or \
            (lg[0, -1].max() - lg[0, -1][g[0, 100 + t]]).abs().item() < 0.05
