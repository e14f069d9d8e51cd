"""Sliding-window attention on the MI355X: the banded keep-bit kernel, the attention kernels
with ``window=`` against the dense reference ops, the engine end to end, the windowed decode
kernels alone against the fp64 references of tests/decode_win_ref.py (sentinel guards around
every output), and the captured fused step and ``generate`` of windowed models.

Each decode check prints ``RATIO <kernel> <worst err / tol>`` (pytest -s shows them)."""
import copy
import ctypes
import functools

import pytest
import torch

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import attn_gemm, hip, reference as ref, rng
from tests import decode_gqa_ref as G
from tests import decode_ref as R
from tests import decode_win_ref as WR
from tests.test_decode_gqa_gpu import BF, F32, Guarded, _bits, _dev, _pos, check
from tests.test_doc_mask_gpu import _close, _cos, _grads

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEP = 3
KEY = rng.site_key(2, 4, 1, rng.SITE_ATTN)
SENTINEL = 0x5A5A5A5A


# ------------------------------------------------------------------ 1. banded keep bits
def _needed(S, W, device):
    """[W32 (row band r), W32 (word w)] bool: the 32x32 bit tiles a window of W keys reads:
    w <= r and r // 2 - w // 2 <= ceil((W - 1) / 64) (64-row items over 64-wide tiles)."""
    n = (S + 31) // 32
    r = torch.arange(n, device=device).view(n, 1)
    w = torch.arange(n, device=device).view(1, n)
    return (w <= r) & (r // 2 - w // 2 <= (W - 1 + 63) // 64)


@pytest.mark.parametrize("W", [1, 64, 65, 130])
@pytest.mark.parametrize("S", [200, 192, 512])
def test_banded_keep_bits(S, W):
    B, nh, p = 1, 3, 0.1
    n = (S + 31) // 32

    def buf():
        return torch.full((2, B * nh, n, S), SENTINEL, dtype=torch.int32, device=DEV)

    full = hip.attention_dropout_mask(B, nh, S, p, KEY, device=DEV, out=buf())
    band = hip.attention_dropout_mask(B, nh, S, p, KEY, device=DEV, window=W, out=buf())
    again = hip.attention_dropout_mask(B, nh, S, p, KEY, device=DEV, window=W, out=buf())
    assert torch.equal(band, again), "a repeat call gives other bits"
    need = _needed(S, W, DEV)
    col = torch.arange(S, device=DEV) // 32
    # [0]: word (w, q) belongs to tile (r = q // 32, w); [1]: word (r, k) to tile (r, w = k // 32)
    inside = torch.stack([need.t()[:, col], need[:, col]]).unsqueeze(1).expand_as(full)
    assert torch.equal(band[inside], full[inside]), "a word inside the band differs from the full kernel's"
    out = ~inside
    assert ((band[out] == SENTINEL) | (band[out] == full[out])).all(), "a word outside the band holds other bits"
    causal = torch.stack([(torch.arange(n, device=DEV).view(n, 1) <= col.view(1, S)),
                          (col.view(1, S) <= torch.arange(n, device=DEV).view(n, 1))]).unsqueeze(1).expand_as(full)
    assert (full[~causal] == SENTINEL).all() and (full[causal & inside] != SENTINEL).any()
    if 2 * ((W + 62) // 64) + 2 < n:  # the band is narrower than the triangle: work was skipped
        assert (band[causal & out] == SENTINEL).any()
    # the attention wrappers' default buffer: the same bits where the window reads them
    assert hip.attention_dropout_mask(B, nh, S, 0.0, KEY, device=DEV, window=W) is None
    with pytest.raises(ValueError):
        hip.attention_dropout_mask(B, nh, S, p, KEY, device=DEV, window=0)
    assert hip.lib().dlt_attn_dropout_mask_band(None, B, nh, S, 1, 1, W, None) == -1
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip.lib().dlt_attn_dropout_mask_band(ctypes.c_void_p(band.data_ptr()), B, nh, S, 1, 1, 0, st) == -1


# ------------------------------------------------------------------ 2. attention
B = 2
HEADS = ((4, 4), (4, 2))
ATTN_CASES = [(S, W, hd, nh, nkv, p) for S in (192, 200) for W in (1, 33, 64, 100, None) for hd in (64, 128)
              for nh, nkv in HEADS for p in (0.0, 0.1)]


@functools.lru_cache(maxsize=None)
def _inputs(S, hd, nh, nkv):
    g = torch.Generator().manual_seed(1000 * S + hd + nkv)
    q = torch.randn(B, nh, S, hd, generator=g).bfloat16().to(DEV)
    k, v = (torch.randn(B, nkv, S, hd, generator=g).bfloat16().to(DEV) for _ in range(2))
    do = torch.randn(B * S, nh * hd, generator=g).bfloat16().to(DEV)
    return q, k, v, do


@functools.lru_cache(maxsize=None)
def _case(S, W, hd, nh, nkv, p):
    """Inputs and the dense reference results of one case, computed once, shared read-only."""
    W = S if W is None else W
    q, k, v, do = _inputs(S, hd, nh, nkv)
    o_ref, lse_ref = ref.attention_fwd(q, k, v, p, KEY, window=W)
    grads_ref = ref.attention_bwd(q, k, v, o_ref, do, lse_ref, p, KEY, window=W)
    return dict(W=W, q=q, k=k, v=v, do=do, o_ref=o_ref, lse_ref=lse_ref, grads_ref=grads_ref)


@pytest.mark.parametrize("S,W,hd,nh,nkv,p", ATTN_CASES)
def test_window_attention_head_major(S, W, hd, nh, nkv, p):
    c = _case(S, W, hd, nh, nkv, p)
    W, q, k, v, do = c["W"], c["q"], c["k"], c["v"], c["do"]
    o, aux = hip.attention_fwd(q, k, v, p, KEY, window=W)
    assert torch.isfinite(o.float()).all() and torch.isfinite(aux[0]).all()
    _close(aux[0], c["lse_ref"], 2e-3, 1e-4, "lse")
    _close(o, c["o_ref"].float(), 2e-2, 2e-2, "o")
    g1 = hip.attention_bwd(q, k, v, c["o_ref"], do, c["lse_ref"], p, KEY, window=W)  # regenerated (banded) bits
    for a, r, n in zip(g1, c["grads_ref"], ("dq", "dk", "dv")):
        assert torch.isfinite(a.float()).all(), n
        scale = r.float().abs().max().item()
        _close(a, r.float(), 2e-2 * max(1.0, scale), 2e-2, n)
    # -- bitwise: window=W is doc=window_bounds(...) with the full keep bits
    doc = hip.window_bounds(B, S, W, DEV)
    full = hip.attention_dropout_mask(B, nh, S, p, KEY, device=DEV)
    kw = {} if full is None else {"mask": full}
    o2, aux2 = hip.attention_fwd(q, k, v, p, KEY, doc=doc if W < S else None, **kw)
    assert torch.equal(o, o2) and torch.equal(aux[0], aux2[0])
    g2 = hip.attention_bwd(q, k, v, c["o_ref"], do, (c["lse_ref"], full), p, KEY, doc=doc if W < S else None)
    g3 = hip.attention_bwd(q, k, v, c["o_ref"], do, (c["lse_ref"], aux[1]), p, KEY, window=W)  # the forward's stored bits
    for a, b2, b3, n in zip(g1, g2, g3, ("dq", "dk", "dv")):
        assert torch.equal(a, b2), f"{n}: banded and full keep bits differ"
        assert torch.equal(a, b3), f"{n}: stored and regenerated keep bits differ"
    if W >= S:  # a window that covers the sequence: the causal kernels, bit for bit
        o0, aux0 = hip.attention_fwd(q, k, v, p, KEY)
        assert torch.equal(o, o0) and torch.equal(aux[0], aux0[0])
        for a, b0, n in zip(g1, hip.attention_bwd(q, k, v, c["o_ref"], do, c["lse_ref"], p, KEY), ("dq", "dk", "dv")):
            assert torch.equal(a, b0), n
    elif p > 0:  # whatever the buffer held outside the band does not reach the result
        res = []
        for fill in (0, -1):
            m = torch.full((2, B * nh, (S + 31) // 32, S), fill, dtype=torch.int32, device=DEV)
            hip.attention_dropout_mask(B, nh, S, p, KEY, device=DEV, window=W, out=m)
            of, _ = hip.attention_fwd(q, k, v, p, KEY, window=W, mask=m)
            res.append((of,) + tuple(hip.attention_bwd(q, k, v, c["o_ref"], do, (c["lse_ref"], m), p, KEY, window=W)))
        for a, b_, g in zip(res[0], res[1], (o,) + tuple(g1)):
            assert torch.equal(a, b_) and torch.equal(a, g), "bits outside the band reached the result"


@pytest.mark.parametrize("S,W,hd,nh,nkv,p", [c for c in ATTN_CASES if c[2] == 64 or c[1] in (33, None)])
def test_window_attention_packed(S, W, hd, nh, nkv, p):
    c = _case(S, W, hd, nh, nkv, p)
    W = c["W"]
    torch.manual_seed(32 + S)
    H, KV = nh * hd, nkv * hd
    gkw = {} if nkv == nh else {"nkv": nkv}
    raw = torch.randn(B * S, H + 2 * KV, device=DEV).bfloat16()
    do = c["do"]
    cos, sin = hip.rope_tables(hd, 1024, device=DEV)
    packed = hip.rope_qk_inplace(raw.clone(), B, S, nh, cos, sin, **gkw)
    o, aux = hip.attention_fwd_packed(packed, B, S, nh, p, KEY, window=W, **gkw)
    o_ref, lse_ref = ref.attention_fwd_packed(packed.float(), B, S, nh, p, KEY, window=W, **gkw)
    _close(aux[0], lse_ref, 2e-3, 1e-4, "lse")
    _close(o, o_ref, 2e-2, 2e-2, "o")
    got = hip.attention_bwd_packed(packed, o, do, aux, p, KEY, B, S, nh, cos, sin, window=W, **gkw)
    want = ref.attention_bwd_packed(packed.float(), o.float(), do.float(), aux[0], p, KEY, B, S, nh, cos, sin,
                                    window=W, **gkw)
    scale = want.abs().max().item()
    _close(got, want, 2e-2 * max(1.0, scale), 2e-2, "dqkv packed vs fp32 ref")
    # the head-major kernels on the same (roped) heads: the same bits
    q4, k4, v4 = (t.to(torch.bfloat16) for t in ref._split_packed(packed, B, S, nh, nkv))
    o1, aux1 = hip.attention_fwd(q4, k4, v4, p, KEY, window=W, **gkw)
    assert torch.equal(o, o1) and torch.equal(aux[0], aux1[0])
    # regenerated (banded) against stored keep bits, and doc= with the bounds folded in already
    got2 = hip.attention_bwd_packed(packed, o, do, aux[0], p, KEY, B, S, nh, cos, sin, window=W, **gkw)
    assert torch.equal(got, got2)
    if W < S:
        wb = hip.window_bounds(B, S, W, DEV)
        o3, _ = hip.attention_fwd_packed(packed, B, S, nh, p, KEY, doc=wb, window=W, **gkw)
        assert torch.equal(o, o3)


def test_window_merges_with_the_document_mask():
    S, W, hd, nh = 200, 33, 64, 4
    q, k, v, do = _inputs(S, hd, nh, nh)
    ids = torch.randint(SEP + 1, 500, (B, S), generator=torch.Generator().manual_seed(S))
    ids[0, [36, 63, 127]] = SEP
    doc = hip.doc_bounds(ids.to(DEV), SEP)
    for p in (0.0, 0.1):
        o, aux = hip.attention_fwd(q, k, v, p, KEY, doc=doc, window=W)
        o_ref, lse_ref = ref.attention_fwd(q, k, v, p, KEY, doc=doc, window=W)
        _close(aux[0], lse_ref, 2e-3, 1e-4, "lse")
        _close(o, o_ref.float(), 2e-2, 2e-2, "o")
        merged = hip.window_bounds(B, S, W, DEV, doc=doc)
        o2, _ = hip.attention_fwd(q, k, v, p, KEY, doc=merged)
        assert torch.equal(o, o2)
        grads = hip.attention_bwd(q, k, v, o_ref, do, lse_ref, p, KEY, doc=doc, window=W)
        for a, r, n in zip(grads, ref.attention_bwd(q, k, v, o_ref, do, lse_ref, p, KEY, doc=doc, window=W), ("dq", "dk", "dv")):
            scale = r.float().abs().max().item()
            _close(a, r.float(), 2e-2 * max(1.0, scale), 2e-2, n)
    # and neither mask alone gives that result
    assert not torch.equal(o, hip.attention_fwd(q, k, v, 0.1, KEY, doc=doc)[0])
    assert not torch.equal(o, hip.attention_fwd(q, k, v, 0.1, KEY, window=W)[0])


def test_padded_head_takes_the_window_and_the_other_routes_refuse():
    S, hd, W, p = 200, 96, 33, 0.1
    g = torch.Generator().manual_seed(96)
    q, k, v = (torch.randn(B, 2, S, hd, generator=g).bfloat16().to(DEV) for _ in range(3))
    o, aux = attn_gemm.attention_fwd(q, k, v, p, KEY, window=W)
    o_ref, lse_ref = ref.attention_fwd(q, k, v, p, KEY, window=W)
    _close(aux[0], lse_ref, 2e-3, 1e-4, "lse")
    _close(o, o_ref.float(), 2e-2, 2e-2, "o")
    q160 = torch.randn(B, 2, 64, 160, device=DEV).bfloat16()
    with pytest.raises(NotImplementedError, match="GEMM-formulated"):
        attn_gemm.attention_fwd(q160, q160, q160, 0.0, KEY, window=8)
    q32 = torch.randn(B, 2, 64, 64, device=DEV)
    with pytest.raises(NotImplementedError, match="fp32"):
        hip.attention_fwd(q32, q32, q32, 0.0, KEY, window=8)
    with pytest.raises(NotImplementedError, match="fp32"):
        hip.attention_fwd_packed(torch.randn(B * 64, 3 * 128, device=DEV), B, 64, 2, 0.0, KEY, window=8)
    q64 = q32.bfloat16()
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            hip.attention_fwd(q64, q64, q64, 0.0, KEY, window=bad)
    # the engine refuses when it is enabled, before any step
    wide = GPT(GPTConfig(vocab_size=512, hidden_size=320, num_layers=1, num_heads=2, max_seq_len=64, sliding_window=8)).to(DEV)
    with pytest.raises(NotImplementedError, match="GEMM-formulated"):
        wide.enable_engine()
    assert wide.engine is None
    f32 = GPT(GPTConfig(vocab_size=512, hidden_size=128, num_layers=1, num_heads=2, max_seq_len=64, sliding_window=8)).to(DEV)
    with pytest.raises(NotImplementedError, match="fp32"):
        f32.enable_engine(act_dtype=torch.float32)


# ------------------------------------------------------------------ 3. engine
def _engine_cfg(**kw):
    d = dict(vocab_size=512, hidden_size=256, num_layers=2, num_heads=4, max_seq_len=256, dropout=0.1,
             attention_dropout=0.1, sliding_window=64)
    d.update(kw)
    return GPTConfig(**d)


def _engine_ids(seed, sep=False):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(SEP + 1, 512, (2, 256), generator=g)
    if sep:
        ids[0, 55] = SEP
        ids[0, 200] = SEP
    return ids.to(DEV)


@functools.lru_cache(maxsize=None)
def _engine_base(kw):
    torch.manual_seed(0)
    m = GPT(_engine_cfg(**dict(kw))).to(DEV)
    if m.config.qk_norm:
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for layer in m.layers:
                for n in (layer.attention.q_norm, layer.attention.k_norm):
                    n.weight.copy_((1.0 + 0.5 * torch.randn(n.weight.shape, generator=g)).to(DEV))
    return m


def _step(kw=(), recompute=False, selective=True, ops_ns=None, sep=None, cfg_over=None):
    m = copy.deepcopy(_engine_base(kw))
    if cfg_over is not None:  # the same weights under another window setting
        m2 = GPT(_engine_cfg(**{**dict(kw), **cfg_over})).to(DEV)
        m2.load_state_dict(m.state_dict())
        m = m2
    m.set_doc_separator(sep)
    eng = m.enable_engine(seed=5, **({"ops": ops_ns} if ops_ns is not None else {}))
    eng.selective_recompute = selective
    m.gradient_checkpointing = recompute
    ids = _engine_ids(1, sep is not None)
    _, loss = m(ids, labels=ids)
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), _grads(m), m


ENGINE_VARIANTS = [((), None), ((("dropout", 0.0), ("attention_dropout", 0.0)), None), ((("num_kv_heads", 2),), None),
                   ((("qk_norm", True),), None), ((), SEP), ((("sliding_window_pattern", 2),), SEP)]


@pytest.mark.parametrize("kw,sep", ENGINE_VARIANTS)
def test_engine_hip_vs_reference_ops(kw, sep):
    l1, g1, m = _step(kw, sep=sep)
    l2, g2, _ = _step(kw, sep=sep, ops_ns=ops.CPU_OPS)  # reference ops on the GPU: same weights, same masks
    assert abs(l1 - l2) < 2e-2 * abs(l2)
    for n in g1:
        assert torch.isfinite(g1[n]).all(), n
        assert _cos(g1[n], g2[n]) > 0.99, n
        r = g1[n].norm() / g2[n].norm()
        assert 0.95 < r.item() < 1.05, (n, r.item())
    l0, _, _ = _step(kw, sep=sep, cfg_over=dict(sliding_window=None, sliding_window_pattern=None))
    assert l0 != l1, "the window must change the loss"
    if dict(kw).get("sliding_window_pattern"):
        la, _, _ = _step(kw, sep=sep, cfg_over=dict(sliding_window_pattern=None))
        assert la != l1, "the global layer must change the loss"


@pytest.mark.parametrize("selective", [True, False])
@pytest.mark.parametrize("kw,sep", [((), None), ((("sliding_window_pattern", 2), ("num_kv_heads", 2)), SEP)])
def test_engine_recompute_is_bitwise(kw, sep, selective):
    l1, g1, _ = _step(kw, sep=sep, recompute=False)
    l2, g2, _ = _step(kw, sep=sep, recompute=True, selective=selective)
    assert l1 == l2
    for n in g1:
        assert torch.equal(g1[n], g2[n]), (n, (g1[n] - g2[n]).abs().max().item())


def test_engine_regenerated_keep_bits_are_bitwise(monkeypatch):
    """DLT_ATTN_MASK_BUDGET_GB=0: no layer keeps its bits, the backward regenerates the band."""
    l1, g1, m1 = _step()
    monkeypatch.setenv("DLT_ATTN_MASK_BUDGET_GB", "0")
    l2, g2, m2 = _step()
    assert m1.engine.attn_mask_budget > 0 and m2.engine.attn_mask_budget == 0
    assert l1 == l2
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


@pytest.mark.parametrize("recompute", [False, True])
def test_engine_train_window_matches_sequential(recompute):
    from distributed_llm_trainer_amd.models.engine import shift_targets
    GA = 2
    kw = (("sliding_window_pattern", 2),)
    m1, m2 = copy.deepcopy(_engine_base(kw)), copy.deepcopy(_engine_base(kw))
    for m in (m1, m2):
        m.set_doc_separator(SEP)
    e1, e2 = m1.enable_engine(seed=9), m2.enable_engine(seed=9)
    m1.gradient_checkpointing = m2.gradient_checkpointing = recompute
    data = [_engine_ids(10 + j, True) for j in range(GA)]
    seq = []
    for j in range(GA):
        e1.set_accumulation(j, GA, defer=True)
        _, loss = m1(data[j], labels=data[j])
        (loss / GA).backward()
        seq.append(loss.item())
    win = e2.train_window(data, [shift_targets(d) for d in data], torch.full((), 1.0 / GA, device=DEV),
                          recompute=recompute)
    torch.cuda.synchronize()
    for a, b in zip(seq, win):
        assert a == b.item(), (seq, [w.item() for w in win])
    g1, g2 = _grads(m1), _grads(m2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), (n, (g1[n] - g2[n]).abs().max().item())


def _trainer(**kw):
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=1, warmup_steps=1, max_steps=100, learning_rate=1e-2)
    return DistributedTrainer(_engine_cfg(**kw), tc)


def _train(steps, **kw):
    tr = _trainer(**kw)
    losses = [float(tr.train_step({"input_ids": _engine_ids(20 + s)})["loss"]) for s in range(steps)]
    return losses, tr.flat_params().clone()


def test_two_runs_are_bit_identical_and_a_covering_window_is_no_window():
    la, pa = _train(3)
    lb, pb = _train(3)
    assert la == lb and torch.equal(pa, pb), "two 3-step runs differ"
    l0, p0 = _train(2, sliding_window=None)
    for W in (256, 5000):  # W >= max_seq_len: the model without the field, bit for bit
        lw, pw = _train(2, sliding_window=W)
        assert lw == l0 and torch.equal(pw, p0), W
    assert la[:2] != l0


# ------------------------------------------------------------------ 4. dec_attn(window=)
@functools.lru_cache(maxsize=None)
def _mha_case(kind):
    return _dev(R.attn_inputs(WR.MHA_NH, WR.MHA_MAXS, kind))


def _poison(kc, vc, kf, pos):
    """NaN in every K row and 3e38 in every V row below kf and beyond pos."""
    k2, v2 = kc.clone(), vc.clone()
    k2[:, :, pos + 1:] = float("nan")
    v2[:, :, pos + 1:] = 3e38
    k2[:, :, :kf] = float("nan")
    v2[:, :, :kf] = 3e38
    return k2, v2


@pytest.mark.parametrize("Bn", [1, 2])
@pytest.mark.parametrize("kind", WR.MHA_KINDS)
@pytest.mark.parametrize("W", WR.MHA_WINDOWS)
def test_dec_attn_window(W, kind, Bn):
    nh, maxS = WR.MHA_NH, WR.MHA_MAXS
    q, kc, vc = (t[:Bn].contiguous() for t in _mha_case(kind))
    q0 = q.clone()
    for pos in WR.mha_positions(W):
        kf = WR.first_key(pos, W)
        k2, v2 = _poison(kc, vc, kf, pos)
        k0, v0 = k2.clone(), v2.clone()
        posd = _pos(pos)
        outs = []
        for _ in range(2):
            o = Guarded((Bn, nh * 64), BF, -777.0)
            hip.dec_attn(q, k2, v2, posd, o.t, R.ATTN_SCALE, window=W)
            o.assert_guards()
            outs.append(o.t)
        assert torch.isfinite(outs[0]).all(), "a cache row outside the window reached the output"
        check(f"dec_attn[W={W},{kind},pos={pos},B={Bn}]", outs[0], WR.attn_win_ref(q, kc, vc, pos, R.ATTN_SCALE, W))
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two calls, two results"
        assert posd.item() == pos and torch.equal(q, q0)
        assert torch.equal(_bits(k2), _bits(k0)) and torch.equal(_bits(v2), _bits(v0))
        if W >= maxS:  # the kernel without a window on the same rows: the same bits
            o1 = torch.empty(Bn, nh * 64, dtype=BF, device=DEV)
            hip.dec_attn(q, k2, v2, posd, o1, R.ATTN_SCALE)
            assert torch.equal(_bits(o1), _bits(outs[0]))


def test_dec_attn_window_host_validation_and_refusals():
    q, kc, vc = (t[:1].contiguous() for t in _mha_case("randn"))
    o = Guarded((1, WR.MHA_NH * 64), BF, -777.0)
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError, match="window"):
            hip.dec_attn(q, kc, vc, _pos(0), o.t, 0.125, window=bad)
    with pytest.raises(TypeError):
        hip.dec_attn(q, kc.float(), vc.float(), _pos(0), o.t, 0.125, window=4)
    with pytest.raises(ValueError):
        hip.dec_attn(q, kc, vc[:, :, :100], _pos(0), o.t, 0.125, window=4)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = hip.lib()
    args = (p(q), p(kc), p(vc), p(_pos(0)), p(o.t))
    assert L.dlt_dec_attn_win(*args, 1, 256, 4, WR.MHA_MAXS, 0.125, 0, st) == -1    # window < 1
    assert L.dlt_dec_attn_win(*args, 1, 256, 3, WR.MHA_MAXS, 0.125, 4, st) == -1    # H != nh * 64
    # min(W, maxS) * 4 + 1056 bytes of LDS: a long cache passes with a window, not without
    big = 50000
    assert L.dlt_dec_attn_win(*args, 1, 256, 4, big, 0.125, big, st) == -1
    assert L.dlt_dec_attn(*args, 1, 256, 4, big, 0.125, st) == -1
    torch.cuda.synchronize()
    o.assert_guards(torch.zeros((1, WR.MHA_NH * 64), dtype=torch.bool, device=DEV))
    kb, vb = (torch.zeros(1, 1, big, 64, dtype=BF, device=DEV) for _ in range(2))
    qb, ob = torch.zeros(1, 64, dtype=BF, device=DEV), torch.ones(1, 64, dtype=BF, device=DEV)
    hip.dec_attn(qb, kb, vb, _pos(big - 1), ob, 0.125, window=1024)
    assert (ob == 0).all()  # V is zero


# ------------------------------------------------------------------ 5. dec_attn_gqa(window=)
@functools.lru_cache(maxsize=None)
def _gqa_case(nh, nkv, kind):
    return _dev(G.attn_gqa_inputs(nh, nkv, WR.GQA_MAXS, kind))


@pytest.mark.parametrize("W,NS", [(50, 1), (50, 2), (50, 4), (50, 8), (7, 8)])
@pytest.mark.parametrize("kind", ["randn", "large60"])
@pytest.mark.parametrize("nh,nkv", WR.GQA_HEADS)
def test_dec_attn_gqa_window(nh, nkv, kind, W, NS):
    maxS, Bn = WR.GQA_MAXS, 2
    C = hip.dec_attn_chunk(min(W, maxS), NS)
    assert C == WR.chunk(maxS, W, NS) and (C == 13 if (W, NS) == (50, 4) else True)
    q, kc, vc = (t[:Bn].contiguous() for t in _gqa_case(nh, nkv, kind))
    q0 = q.clone()
    for pos in WR.gqa_positions(W, C, NS):
        kf = WR.first_key(pos, W)
        k2, v2 = _poison(kc, vc, kf, pos)
        k0, v0 = k2.clone(), v2.clone()
        posd = _pos(pos)
        outs = []
        for _ in range(2):  # the second call on a fresh workspace full of NaN
            o = Guarded((Bn, nh * 64), BF, -777.0)
            ws = Guarded((Bn * nh * NS * hip.DEC_ATTN_WS,), F32, float("nan")) if NS > 1 else None
            hip.dec_attn_gqa(q, k2, v2, posd, o.t, G.ATTN_SCALE, nh, splits=NS, ws=None if ws is None else ws.t,
                             window=W)
            o.assert_guards()
            if ws is not None:
                ws.assert_guards()
            outs.append(o.t)
        tag = f"dec_attn_gqa[nh={nh},nkv={nkv},{kind},W={W},NS={NS},pos={pos}]"
        assert torch.isfinite(outs[0]).all(), "a cache row outside the window reached the output"
        check(tag, outs[0], WR.attn_gqa_win_ref(q, kc, vc, pos, G.ATTN_SCALE, nh, W))
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two calls, two results"
        if NS > 1:  # the chunks are the window-anchored ones: which are empty, and their (m, l)
            model = WR.attn_gqa_win_split32(q, kc, vc, pos, G.ATTN_SCALE, nh, NS, W)
            assert WR.partials_match(WR.workspace_partials(ws.t, Bn, nh, NS), model), tag
        assert posd.item() == pos and torch.equal(q, q0)
        assert torch.equal(_bits(k2), _bits(k0)) and torch.equal(_bits(v2), _bits(v0))


@pytest.mark.parametrize("NS", [1, 4])
def test_dec_attn_gqa_covering_window_is_no_window(NS):
    nh, nkv, maxS = 6, 2, WR.GQA_MAXS
    q, kc, vc = _gqa_case(nh, nkv, "randn")
    for W in (maxS, maxS + 1, 100000):
        for pos in (0, 49, maxS - 1):
            res = []
            for w in (0, W):
                o = torch.empty(8, nh * 64, dtype=BF, device=DEV)
                ws = hip.dec_attn_gqa_workspace(8, nh, NS, DEV) if NS > 1 else None
                hip.dec_attn_gqa(q, kc, vc, _pos(pos), o, G.ATTN_SCALE, nh, splits=NS, ws=ws, window=w)
                res.append(o)
            assert torch.equal(_bits(res[0]), _bits(res[1])), (W, pos)


def test_dec_attn_gqa_window_host_validation_and_refusals():
    nh, nkv = 4, 2
    q, kc, vc = (t[:1].contiguous() for t in _gqa_case(nh, nkv, "randn"))
    o = Guarded((1, nh * 64), BF, -777.0)
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError, match="window"):
            hip.dec_attn_gqa(q, kc, vc, _pos(0), o.t, 0.125, nh, window=bad)
    with pytest.raises(ValueError, match="workspace"):
        hip.dec_attn_gqa(q, kc, vc, _pos(0), o.t, 0.125, nh, splits=2, window=8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = hip.lib()
    args = (p(q), p(kc), p(vc), p(_pos(0)), p(o.t), None)
    assert L.dlt_dec_attn_gqa_win(*args, 1, 256, 4, 2, WR.GQA_MAXS, 1, 0.125, 0, st) == -1   # window < 1
    assert L.dlt_dec_attn_gqa_win(*args, 1, 256, 4, 3, WR.GQA_MAXS, 1, 0.125, 8, st) == -1   # nh % nkv
    assert L.dlt_dec_attn_gqa_win(*args, 1, 256, 4, 2, WR.GQA_MAXS, 2, 0.125, 8, st) == -1   # NS > 1, no workspace
    assert L.dlt_dec_attn_gqa_win(*args, 1, 256, 4, 2, WR.GQA_MAXS, 3, 0.125, 8, st) == -1   # NS not in {1, 2, 4, 8}
    torch.cuda.synchronize()
    o.assert_guards(torch.zeros((1, nh * 64), dtype=torch.bool, device=DEV))
    # G * C * 4 bytes of scores: 16 heads over 4096 keys do not fit one CU, over a window of 2048 they do
    q16 = torch.zeros(1, 16 * 64, dtype=BF, device=DEV)
    k1, v1 = (torch.zeros(1, 1, 4096, 64, dtype=BF, device=DEV) for _ in range(2))
    o16 = torch.ones(1, 16 * 64, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="dec_attn_gqa"):
        hip.dec_attn_gqa(q16, k1, v1, _pos(4095), o16, 0.125, 16, splits=1)
    hip.dec_attn_gqa(q16, k1, v1, _pos(4095), o16, 0.125, 16, splits=1, window=2048)
    assert (o16 == 0).all()  # V is zero


# ------------------------------------------------------------------ 6. the step and generation
def _dec_cfg(nkv, N):
    return GPTConfig(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=nkv, max_seq_len=256,
                     dropout=0.0, attention_dropout=0.0, sliding_window=64, sliding_window_pattern=N)


@functools.lru_cache(maxsize=None)
def _dec_model(nkv, N):
    torch.manual_seed(5 + nkv)
    m = GPT(_dec_cfg(nkv, N)).to(DEV)
    m.enable_engine()
    m.eval()
    return m


@pytest.mark.parametrize("N", [None, 2])
@pytest.mark.parametrize("nkv", [4, 2])
def test_decode_fused_window_step_matches_torch_step(nkv, N, monkeypatch):
    """The captured fused step of a windowed model == the ATen step: logits and the K/V rows
    it appends, over a 150-token context (beyond W) and 5 steps; two fused graphs bit for bit."""
    from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, _fused_kind, forward_cached
    m = _dec_model(nkv, N)
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
            pos = caches[0].len - 1
            for i in range(cfg.num_layers):
                for x, y in ((caches[0].k[i], caches[1].k[i]), (caches[0].v[i], caches[1].v[i])):
                    assert torch.allclose(x[:, :, pos].float(), y[:, :, pos].float(), atol=2e-2, rtol=2e-2)
        # the window is live in both steps: the model without it gives other logits
        off = GPT(GPTConfig.from_dict({k: v for k, v in cfg.to_dict().items() if not k.startswith("sliding")})).to(DEV)
        off.load_state_dict(m.state_dict())
        off.enable_engine()
        off.eval()
        c0 = KVCache(cfg, Bn, DEV, m.engine.act_dtype)
        forward_cached(off, ids, c0)
        monkeypatch.setenv("DLT_DECODE_FUSED", "1")
        g0 = DecodeGraph(off, c0, c0.len)
        c1 = KVCache(cfg, Bn, DEV, m.engine.act_dtype)
        forward_cached(m, ids, c1)
        g1 = DecodeGraph(m, c1, c1.len)
        assert (g0(steps[:, :1]) - g1(steps[:, :1])).abs().max().item() > 3e-2


@pytest.mark.parametrize("N", [None, 2])
@pytest.mark.parametrize("nkv", [4, 2])
def test_generate_device_loop_matches_host_loop_window(nkv, N, monkeypatch):
    m = _dec_model(nkv, N)
    ids = torch.randint(0, 1000, (2, 240), generator=torch.Generator().manual_seed(7)).to(DEV)
    monkeypatch.setenv("DLT_DECODE_DEVICE_LOOP", "1")
    a = m.generate(ids, max_new_tokens=24, top_k=1)
    monkeypatch.setenv("DLT_DECODE_DEVICE_LOOP", "0")
    b = m.generate(ids, max_new_tokens=24, top_k=1)
    assert a.shape == b.shape == (2, 264)
    assert (a == b).float().mean().item() > 0.97  # greedy; rare near-ties may flip
