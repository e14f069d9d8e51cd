"""Attention-score soft-capping on the GPU: the CAP kernels (ops/csrc/attention_cap.hip, decode.hip)
against the fp64 references and derived tolerances of tests/attn_cap_ref.py -- every element of o,
lse, dq, dk, dv, outputs in guarded buffers -- then dispatch, determinism, the fused decode step
and a tiny capped model on the HIP engine against the same engine on the reference ops.

Each check prints ``RATIO <output> <worst err / tol>``; ``pytest -s`` shows them."""
import copy
import ctypes
import functools

import pytest
import torch

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip, rng
from distributed_llm_trainer_amd.ops.reference import WindowBounds
from tests import attn_cap_ref as C
from tests import attn_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
SENT = {A.BF: 3.0, A.HF: 3.0, F32: -7.5, I32: 0x5A5A5A5A}


def check(name, out, chk):
    ref, tol = chk.ref.to(out.device), chk.tol.to(out.device)
    err = (out.double().reshape(ref.shape) - ref).abs()
    ratio = torch.where(tol > 0, err / tol, err).max().item()
    print(f"RATIO {name} {ratio:.4f}")
    bad = ~(err <= tol)
    assert not bad.any(), (f"{name}: {bad.sum().item()} of {bad.numel()} elements outside the tolerance, "
                           f"worst err/tol {ratio:.3f} at {bad.nonzero()[0].tolist()}")


def _d(t):
    return None if t is None else t.to(DEV)


def _args(**kw):
    strides = kw.pop("strides")
    return hip._AttnArgs(**{k: (hip._p(v) if isinstance(v, torch.Tensor) else v) for k, v in kw.items() if v is not None},
                         stride=hip._AttnStrides(**strides))


def _bounds(b, inp):
    window = A.case_window(b)
    if inp.doc is None:
        return None, None
    lo, hi = _d(inp.doc[0]), _d(inp.doc[1])
    return (WindowBounds(lo, hi, window) if window is not None else (lo, hi)), window


# ------------------------------------------------------------------ 1. the training kernels
def _run_direct(c, r, doc, window, cap):
    """Head-major: dlt_attn_fwd / dlt_attn_bwd on a hand-filled _AttnArgs, every output guarded.
    ``cap`` None leaves the softcap field out (zero): the plain kernels."""
    b, inp = c.base, r.inp
    B, nh, S, hd, dt = b.B, b.nh, b.S, b.hd, b.dtype
    q, k, v, do = _d(inp.q), _d(inp.k), _d(inp.v), _d(inp.do)
    thr = rng.keep_threshold(b.p)
    dscale = 1.0 / (1.0 - b.p) if thr else 1.0
    O = A.Guarded((B * S, nh * hd), dt, SENT[dt], DEV)
    L = A.Guarded((B, nh, S), F32, SENT[F32], DEV)
    M = A.Guarded((2, B * nh, (S + 31) // 32, S), I32, SENT[I32], DEV) if thr else None
    gen = 1
    if thr and window is not None:
        hip.attention_dropout_mask(B, nh, S, b.p, b.key, window=window, out=M.t)
        gen = 0
    sink = _d(r.sink)
    _, sq, skv = hip._head_major(q, k, v)
    st = dict(q=sq, kv=skv, dq=sq, dkv=skv)
    common = dict(q=q, k=k, v=v, lo=doc[0] if doc else None, B=B, nh=nh, nkv=b.nkv, S=S, hd=hd, hk=int(dt == A.HF),
                  scale=inp.scale, dscale=dscale, key=b.key, thr=thr, mask=M.t if M else None, sink=sink, softcap=cap)
    L_, stream = hip.lib(), hip._stream()
    assert L_.dlt_attn_fwd(ctypes.byref(_args(o=O.t, lse=L.t, gen_mask=gen, strides=st, **common)), stream) == 0
    DQ = A.Guarded(tuple(inp.q.shape), dt, SENT[dt], DEV)
    DK, DV = (A.Guarded(tuple(inp.k.shape), dt, SENT[dt], DEV) for _ in range(2))
    DL = A.Guarded((B, nh, S), F32, SENT[F32], DEV)
    DS = A.Guarded((nh,), F32, SENT[F32], DEV, init=torch.zeros(nh))
    assert L_.dlt_attn_bwd(ctypes.byref(_args(o=_d(r.o16), lse=_d(r.lse32), dout=do, delta_ws=DL.t, dq=DQ.t, dk=DK.t,
                                              dv=DV.t, hi=doc[1] if doc else None,
                                              dsink=DS.t if sink is not None else None, strides=st, **common)),
                           stream) == 0
    torch.cuda.synchronize()
    for g in (O, L, DQ, DK, DV, DL):
        g.assert_guards()
    return dict(o=O.t, lse=L.t, dq=DQ.t, dk=DK.t, dv=DV.t, delta=DL.t)


def _run_packed(c, r, doc, window, cap, with_kw=True):
    """Packed QKV through attention_fwd_packed / attention_bwd_packed with guarded ``out=`` buffers.
    ``with_kw`` False: the calls without the softcap keyword at all."""
    b, inp = c.base, r.inp
    B, nh, S, hd, dt, kvh = b.B, b.nh, b.S, b.hd, b.dtype, b.kvh
    H, KV = nh * hd, kvh * hd
    qkv = _d(A.pack_qkv(inp))
    thr = rng.keep_threshold(b.p)
    O = A.Guarded((B * S, H), dt, SENT[dt], DEV)
    M = A.Guarded((2, B * nh, (S + 31) // 32, S), I32, SENT[I32], DEV) if thr else None
    if thr:
        hip.attention_dropout_mask(B, nh, S, b.p, b.key, window=window, out=M.t)
    kw = dict(doc=doc, nkv=b.nkv or None, window=window)
    if with_kw:
        kw["softcap"] = cap
    sink = _d(r.sink)
    skw = dict(sink=sink) if sink is not None else {}
    o, aux = hip.attention_fwd_packed(qkv, B, S, nh, b.p, b.key, out=O.t, mask=M.t if M else None, **kw, **skw)
    Gd = A.Guarded((B * S, H + 2 * KV), dt, SENT[dt], DEV)
    if sink is not None:
        skw["dsink"] = torch.zeros(nh, device=DEV)
    cos, sin = _d(inp.rope[0]), _d(inp.rope[1])
    hip.attention_bwd_packed(qkv, _d(r.o16), _d(inp.do), hip.AttnAux((_d(r.lse32), M.t if M else None)),
                             b.p, b.key, B, S, nh, cos, sin, out=Gd.t, **kw, **skw)
    torch.cuda.synchronize()
    for g in (O, Gd):
        g.assert_guards()
    hm = lambda t, h: t.view(B, S, h, hd).transpose(1, 2)  # noqa: E731
    return dict(o=O.t, lse=aux[0], dq=hm(Gd.t[:, :H], nh), dk=hm(Gd.t[:, H:H + KV], kvh), dv=hm(Gd.t[:, H + KV:], kvh))


def _run(c, r, cap, **kw):
    doc, window = _bounds(c.base, r.inp)
    return (_run_packed if c.base.packed else _run_direct)(c, r, doc, window, cap, **kw)


def _same(a, b, tag):
    for nm in a:
        assert torch.equal(A.bits(a[nm].contiguous()), A.bits(b[nm].contiguous())), f"{tag} {nm}: the bits differ"


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_cap_kernels_against_the_fp64_reference(name):
    c = C.BY_NAME[name]
    r = C.case_refs(c)
    outs = _run(c, r, c.cap)
    for nm, t in outs.items():
        assert torch.isfinite(t.float()).all(), f"{name} {nm}: not finite"
    check(name + " o", outs["o"], r.fwd.o)
    check(name + " lse", outs["lse"], r.fwd.lse)
    for nm in ("dq", "dk", "dv"):
        check(f"{name} {nm}", outs[nm], getattr(r.bwd, nm))
    if "delta" in outs:
        check(name + " delta", outs["delta"], r.bwd.delta)
    if c.sat:  # |x| / CAP = 128: t = +-1 and 1 - t^2 = 0 exactly, so nothing flows through the scores
        assert torch.count_nonzero(outs["dq"]) == 0 and torch.count_nonzero(outs["dk"]) == 0
        assert outs["dv"].float().abs().max().item() > 0
    # determinism: a second call on equal inputs gives the same bits (no atomics)
    _same(outs, _run(c, r, c.cap), name)


@pytest.mark.parametrize("name", [C.CASES[5].name, C.CASES[14].name, C.CASES[17].name, C.CASES[22].name])
def test_softcap_none_is_the_call_without_the_keyword(name):
    """softcap=None: bit-identical outputs to the same call without the keyword (the plain or the
    SINK kernels), forward and backward; and they are not the capped ones."""
    c = C.BY_NAME[name]
    r = C.case_refs(c)
    if c.base.packed:
        a, b = _run(c, r, None, with_kw=True), _run(c, r, None, with_kw=False)
    else:
        a, b = _run(c, r, None), _run(c, r, 0.0)  # the field left out and the field at its zero
    _same(a, b, name)
    capped = _run(c, r, c.cap)
    assert not torch.equal(A.bits(a["o"].contiguous()), A.bits(capped["o"].contiguous()))


def test_head_major_wrappers_and_host_validation():
    c = C.CASES[5]
    b, r = c.base, C.case_refs(c)
    q, k, v = _d(r.inp.q), _d(r.inp.k), _d(r.inp.v)
    o, aux = hip.attention_fwd(q, k, v, b.p, b.key, True, softcap=c.cap)
    check("wrapper o", o.view(b.B, b.S, b.nh, b.hd), r.fwd.o)
    check("wrapper lse", aux[0], r.fwd.lse)
    dq, dk, dv = hip.attention_bwd(q, k, v, _d(r.o16), _d(r.inp.do), hip.AttnAux((_d(r.lse32), aux[1])), b.p, b.key, True,
                                   softcap=c.cap)
    for nm, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        check("wrapper " + nm, t, getattr(r.bwd, nm))
    for bad in (0.0, -2.0, float("inf"), float("nan"), 1e39, 65537.0):
        with pytest.raises(ValueError, match="softcap"):
            hip.attention_fwd(q, k, v, 0.0, 0, True, softcap=bad)
    # the entry points refuse what the wrappers would have caught
    _, sq, skv = hip._head_major(q, k, v)
    o2 = torch.empty_like(o)
    lse = torch.empty(b.B, b.nh, b.S, device=DEV)
    for bad in (-1.0, float("inf"), float("nan"), 65537.0, 1e9):
        a = _args(q=q, k=k, v=v, o=o2, lse=lse, B=b.B, nh=b.nh, nkv=b.nkv, S=b.S, hd=b.hd, hk=0, scale=0.125, dscale=1.0,
                  softcap=bad, strides=dict(q=sq, kv=skv))
        assert hip.lib().dlt_attn_fwd(ctypes.byref(a), hip._stream()) == -7
        assert hip.lib().dlt_attn_bwd(ctypes.byref(a), hip._stream()) != 0
    assert hip.lib().dlt_attn_args_size() == ctypes.sizeof(hip._AttnArgs) == 248


def test_routes_without_the_cap_refuse_the_keyword():
    from distributed_llm_trainer_amd.ops import attn_gemm
    q = torch.randn(1, 2, 64, 192, device=DEV).bfloat16()
    with pytest.raises(NotImplementedError, match="GEMM-formulated attention route .*attn_softcap"):
        attn_gemm.attention_fwd(q, q, q, 0.0, 0, True, softcap=2.0)
    q32 = torch.randn(1, 2, 64, 64, device=DEV)
    with pytest.raises(NotImplementedError, match="fp32 .*attn_softcap"):
        hip.attention_fwd(q32, q32, q32, 0.0, 0, True, softcap=2.0)
    # the zero-padded route passes it on to the flash kernels
    g = torch.Generator().manual_seed(7)
    q96, k96, v96 = (torch.randn(1, 2, 100, 96, generator=g).bfloat16() for _ in range(3))
    o, _ = attn_gemm.attention_fwd(_d(q96), _d(k96), _d(v96), 0.0, 0, True, softcap=2.0)
    want = C.cap_fwd_ref(q96, k96, v96, 1.0 / 96 ** 0.5, 2.0)
    check("padded o", o.view(1, 100, 2, 96), want.o)
    # and its backward: the stored o / lse are the forward reference's, as in the kernel cases
    do = torch.randn(100, 2 * 96, generator=g).bfloat16()
    o16 = C.round_to(want.o.ref, BF).reshape(100, 2 * 96).contiguous()
    lse32 = want.lse.ref.to(F32)
    bw = C.cap_bwd_ref(q96, k96, v96, o16, do, lse32, 1.0 / 96 ** 0.5, 2.0)
    dq, dk, dv = attn_gemm.attention_bwd(_d(q96), _d(k96), _d(v96), _d(o16), _d(do), hip.AttnAux((_d(lse32), None)), 0.0, 0,
                                         True, softcap=2.0)
    for nm, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        check("padded " + nm, t, getattr(bw, nm))
    dq0, _, _ = attn_gemm.attention_bwd(_d(q96), _d(k96), _d(v96), _d(o16), _d(do), hip.AttnAux((_d(lse32), None)), 0.0, 0, True)
    assert not torch.equal(dq0, dq), "the padded backward ignored the cap"


# ------------------------------------------------------------------ 2. the decode kernels
def _pos(p):
    return torch.tensor([p], dtype=I64, device=DEV)


@functools.lru_cache(maxsize=None)
def _dec_case(nh, nkv):
    return tuple(t.to(DEV) for t in C.dec_inputs(nh, nkv))


def _poison(kc, vc, kf, pos):
    k2, v2 = kc.clone(), vc.clone()
    k2[:, :, pos + 1:], v2[:, :, pos + 1:] = float("nan"), 3e38
    k2[:, :, :kf], v2[:, :, :kf] = float("nan"), 3e38
    return k2, v2


@pytest.mark.parametrize("Bn", [1, 8])
@pytest.mark.parametrize("W,sink", [(None, False), (50, False), (None, True), (50, True)])
def test_dec_attn_cap(W, sink, Bn):
    nh, cap = 4, 2.0
    q, kc, vc = (t[:Bn].contiguous() for t in _dec_case(nh, nh))
    sk = torch.tensor(C.DEC_SINKS[:nh], device=DEV) if sink else None
    for pos in C.DEC_POS:
        kf = max(0, pos + 1 - W) if W else 0
        k2, v2 = _poison(kc, vc, kf, pos)
        outs = []
        for _ in range(2):
            o = A.Guarded((Bn, nh * 64), BF, -777.0, DEV)
            hip.dec_attn(q, k2, v2, _pos(pos), o.t, C.DEC_SCALE, window=W or 0, sink=sk, softcap=cap)
            o.assert_guards()
            outs.append(o.t)
        tag = f"dec_attn[cap,W={W},sink={sink},B={Bn},pos={pos}]"
        assert torch.isfinite(outs[0]).all(), tag
        check(tag, outs[0].view(Bn, nh, 64), C.dec_cap_ref(q.cpu(), kc.cpu(), vc.cpu(), pos, C.DEC_SCALE, nh, cap, W,
                                                          None if sk is None else sk.cpu()))
        assert torch.equal(A.bits(outs[0]), A.bits(outs[1])), "two calls, two results"
        a, b = (torch.empty(Bn, nh * 64, dtype=BF, device=DEV) for _ in range(2))
        hip.dec_attn(q, k2, v2, _pos(pos), a, C.DEC_SCALE, window=W or 0, sink=sk)
        hip.dec_attn(q, k2, v2, _pos(pos), b, C.DEC_SCALE, window=W or 0, sink=sk, softcap=None)
        assert torch.equal(A.bits(a), A.bits(b)), "softcap=None is the call without it"


@pytest.mark.parametrize("Bn", [1, 8])
@pytest.mark.parametrize("W,sink", [(None, False), (50, True)])
@pytest.mark.parametrize("NS", [1, 4])
@pytest.mark.parametrize("nh,nkv", [(4, 2), (12, 4)])
def test_dec_attn_gqa_cap(nh, nkv, NS, W, sink, Bn):
    cap = 2.0
    q, kc, vc = (t[:Bn].contiguous() for t in _dec_case(nh, nkv))
    sk = torch.tensor(C.DEC_SINKS[:nh], device=DEV) if sink else None
    for pos in C.DEC_POS:
        kf = max(0, pos + 1 - W) if W else 0
        k2, v2 = _poison(kc, vc, kf, pos)
        outs = []
        for _ in range(2):  # the second call on a fresh workspace full of NaN
            o = A.Guarded((Bn, nh * 64), BF, -777.0, DEV)
            ws = A.Guarded((Bn * nh * NS * hip.DEC_ATTN_WS,), F32, float("nan"), DEV) if NS > 1 else None
            hip.dec_attn_gqa(q, k2, v2, _pos(pos), o.t, C.DEC_SCALE, nh, splits=NS, ws=None if ws is None else ws.t,
                             window=W or 0, sink=sk, softcap=cap)
            o.assert_guards()
            if ws is not None:
                ws.assert_guards()
            outs.append(o.t)
        tag = f"dec_attn_gqa[cap,nh={nh},nkv={nkv},NS={NS},W={W},sink={sink},B={Bn},pos={pos}]"
        assert torch.isfinite(outs[0]).all(), tag
        check(tag, outs[0].view(Bn, nh, 64), C.dec_cap_ref(q.cpu(), kc.cpu(), vc.cpu(), pos, C.DEC_SCALE, nh, cap, W,
                                                          None if sk is None else sk.cpu()))
        assert torch.equal(A.bits(outs[0]), A.bits(outs[1])), "two calls, two results"
        res = []
        for kw in ({}, {"softcap": None}):
            o = torch.empty(Bn, nh * 64, dtype=BF, device=DEV)
            ws = hip.dec_attn_gqa_workspace(Bn, nh, NS, DEV) if NS > 1 else None
            hip.dec_attn_gqa(q, k2, v2, _pos(pos), o, C.DEC_SCALE, nh, splits=NS, ws=ws, window=W or 0, sink=sk, **kw)
            res.append(o)
        assert torch.equal(A.bits(res[0]), A.bits(res[1])), tag


def test_dec_cap_host_validation():
    q, kc, vc = (t[:1].contiguous() for t in _dec_case(4, 2))
    qm, km, vm = (t[:1].contiguous() for t in _dec_case(4, 4))
    o = torch.empty(1, 256, dtype=BF, device=DEV)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="softcap"):
            hip.dec_attn_gqa(q, kc, vc, _pos(0), o, 0.125, 4, softcap=bad)
        with pytest.raises(ValueError, match="softcap"):
            hip.dec_attn(qm, km, vm, _pos(0), o, 0.125, softcap=bad)


# ------------------------------------------------------------------ 3. the model
SEP = 3
COMBO = dict(num_kv_heads=2, qk_norm=True, sliding_window=64, sliding_window_pattern=2, attention_sinks=True)


def _cfg(dropout=0.1, **kw):
    d = dict(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, max_seq_len=128, dropout=dropout,
             attention_dropout=dropout, attn_softcap=2.0)
    d.update(kw)
    return GPTConfig(**d)


def _model(cfg, seed):
    """Scores of a few units (the q / k weights scaled up), so that a cap of 2 bends them; non-zero
    sinks where the model has them."""
    torch.manual_seed(seed)
    m = GPT(cfg)
    with torch.no_grad():
        for layer in m.layers:
            at = layer.attention
            if not cfg.qk_norm:
                at.q_proj.weight.mul_(12.0)
                at.k_proj.weight.mul_(12.0)
            else:
                at.q_norm.weight.mul_(3.0)
            if cfg.attention_sinks:
                at.sinks.copy_(1.5 * torch.randn(at.sinks.shape))
    return m.to(DEV)


def _grads(m):
    return {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()


def _ids(cfg, n=2, seed=0, sep=None):
    ids = torch.randint(4, 1000, (n, cfg.max_seq_len), device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
    if sep is not None:
        ids[0, [0, 1, 70, 100]] = sep
        ids[1:, cfg.max_seq_len // 2] = sep
    return ids


@pytest.mark.parametrize("dropout,kw,sep", [(0.0, {}, None), (0.1, {}, None), (0.1, COMBO, SEP)])
def test_engine_hip_vs_reference_ops(dropout, kw, sep):
    """Same 16-bit weights, activations and dropout masks through the HIP ops and through the
    reference ops: loss and every gradient at the engine tolerances of the other GPU suites."""
    cfg = _cfg(dropout, **kw)
    base = _model(cfg, 0)
    base.set_doc_separator(sep)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    e1 = m1.enable_engine(seed=5)
    m2.enable_engine(seed=5, ops=ops.CPU_OPS)
    assert e1.attn_softcap == 2.0 and e1.ops.backend == "hip"
    ids = _ids(cfg, sep=sep)
    _, l1 = m1(ids, labels=ids)
    (l1 / 2).backward()
    _, l2 = m2(ids, labels=ids)
    (l2 / 2).backward()
    assert abs(l1.item() - l2.item()) < 2e-2 * abs(l2.item())
    g1, g2 = _grads(m1), _grads(m2)
    for n in g1:
        assert _cos(g1[n], g2[n]) > 0.99, n
        r = g1[n].norm() / g2[n].norm()
        assert 0.95 < r.item() < 1.05, (n, r.item())
    # the cap is live: the same weights without it give another loss
    off = GPT(GPTConfig.from_dict({k: v for k, v in cfg.to_dict().items() if k != "attn_softcap"})).to(DEV)
    off.load_state_dict(base.state_dict())
    off.set_doc_separator(sep)
    off.enable_engine(seed=5)
    assert abs(off(ids, labels=ids)[1].item() - l1.item()) > 1e-3


def test_engine_recompute_is_bit_identical():
    base = _model(_cfg(0.1, **COMBO), 2)
    base.set_doc_separator(SEP)
    ids = _ids(base.config, seed=2, sep=SEP)
    res = []
    for ac in (False, True):
        m = copy.deepcopy(base)
        m.enable_engine(seed=7)
        m.gradient_checkpointing = ac
        _, loss = m(ids, labels=ids)
        loss.backward()
        res.append((loss.item(), _grads(m)))
    assert res[1][0] == res[0][0]
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n


def test_a_few_optimizer_steps_reduce_the_loss():
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    cfg = _cfg(0.0, num_kv_heads=2)
    data = _ids(cfg, n=4, seed=3)
    torch.manual_seed(3)
    tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=2, warmup_steps=1, learning_rate=1e-3)
    tr = DistributedTrainer(cfg, tc)
    assert tr.use_engine and tr.model.engine.attn_softcap == 2.0
    losses = [tr.train_step({"input_ids": data})["loss"] for _ in range(6)]
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0] - 0.05, losses


def test_unsupported_routes_refuse_at_enable_engine():
    m = GPT(_cfg(0.0)).to(DEV)
    with pytest.raises(NotImplementedError, match="fp32 .*attn_softcap"):
        m.enable_engine(act_dtype=torch.float32)
    assert m.engine is None
    m192 = GPT(_cfg(0.0, hidden_size=768)).to(DEV)  # head_dim 192
    with pytest.raises(NotImplementedError, match="GEMM-formulated .*head_dim 192.*attn_softcap"):
        m192.enable_engine()
    GPT(_cfg(0.0, hidden_size=384)).to(DEV).enable_engine()  # head_dim 96: zero-padded onto the flash kernels


def _dec_cfg(nkv):
    return GPTConfig(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=nkv, max_seq_len=256,
                     dropout=0.0, attention_dropout=0.0, attn_softcap=2.0)


@functools.lru_cache(maxsize=None)
def _dec_model(nkv):
    m = _model(_dec_cfg(nkv), 5 + nkv)
    m.enable_engine()
    m.eval()
    return m


@pytest.mark.parametrize("Bn", [1, 4])
@pytest.mark.parametrize("nkv", [4, 2])
def test_decode_fused_step_matches_forward_cached(nkv, Bn, monkeypatch):
    """The captured fused step of a capped model against forward_cached (torch ops): logits at
    atol = rtol = 3e-2 and the K/V rows it appends at 2e-2, the tolerances of the other fused-step
    tests; the cap is live in the fused step."""
    from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, _fused_kind, forward_cached
    m = _dec_model(nkv)
    cfg = m.config
    monkeypatch.setenv("DLT_DECODE_FUSED", "1")
    assert _fused_kind(m, Bn) == ("mha" if nkv == 4 else "gqa")
    g = torch.Generator().manual_seed(50 + nkv)
    ids = torch.randint(0, 1000, (Bn, 100), generator=g).to(DEV)
    steps = torch.randint(0, 1000, (Bn, 4), generator=g).to(DEV)
    ca, cb = (KVCache(cfg, Bn, DEV, m.engine.act_dtype) for _ in range(2))
    with torch.no_grad():
        forward_cached(m, ids, ca)
        forward_cached(m, ids, cb)
        graph = DecodeGraph(m, ca, ca.len)
        assert graph.fused
        for t in range(steps.shape[1]):
            a = graph(steps[:, t:t + 1]).clone()
            b = forward_cached(m, steps[:, t:t + 1], cb)
            assert torch.allclose(a, b, atol=3e-2, rtol=3e-2), (t, (a - b).abs().max().item())
            pos = ca.len - 1
            for i in range(cfg.num_layers):
                for x, y in ((ca.k[i], cb.k[i]), (ca.v[i], cb.v[i])):
                    assert torch.allclose(x[:, :, pos].float(), y[:, :, pos].float(), atol=2e-2, rtol=2e-2)
        off = GPT(GPTConfig.from_dict({k: v for k, v in cfg.to_dict().items() if k != "attn_softcap"})).to(DEV)
        off.load_state_dict(m.state_dict())
        off.enable_engine()
        off.eval()
        c0, c1 = (KVCache(cfg, Bn, DEV, m.engine.act_dtype) for _ in range(2))
        forward_cached(off, ids, c0)
        forward_cached(m, ids, c1)
        g0, g1 = DecodeGraph(off, c0, c0.len), DecodeGraph(m, c1, c1.len)
        assert g0.fused and g1.fused
        assert (g0(steps[:, :1]) - g1(steps[:, :1])).abs().max().item() > 3e-2


@pytest.mark.parametrize("nkv", [4, 2])
def test_generate_matches_the_greedy_full_reforward(nkv):
    m = _dec_model(nkv)
    ids = _ids(m.config, n=1, seed=4)[:, :100]
    g = m.generate(ids, max_new_tokens=6, top_k=1)
    assert g.shape == (1, 106)
    for t in range(6):  # greedy KV-cached decode == argmax of a full re-forward, or within the QK-norm test's margin
        with torch.no_grad():
            lg, _ = m(g[:, :100 + t])
        assert lg[0, -1].argmax().item() == g[0, 100 + t].item() or \
            (lg[0, -1].max() - lg[0, -1][g[0, 100 + t]]).abs().item() < 0.05
