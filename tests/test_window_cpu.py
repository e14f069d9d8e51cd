"""Sliding-window attention (``GPTConfig.sliding_window`` / ``sliding_window_pattern``) on the
CPU: config, ``window_bounds``, the reference ops against an independent dense softmax, the
eager model, the engine on the reference ops, checkpoints, the CLI flags, KV-cached generation
and the planted defects of the windowed decode kernels' fp32 model (tests/decode_win_ref.py)."""
import copy
import math
import os
import pickle
import types

import pytest
import torch
import torch.nn.functional as F

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.models.engine import shift_targets
from distributed_llm_trainer_amd.ops import reference as ref, rng
from tests import decode_gqa_ref as G
from tests import decode_win_ref as WR

SEP = 7
TINY = dict(vocab_size=256, hidden_size=64, num_layers=2, num_heads=4, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0, sliding_window=5)


def tiny(**kw):
    d = dict(TINY)
    d.update(kw)
    return GPTConfig(**d)


# ------------------------------------------------------------------ config
@pytest.mark.parametrize("kw", [dict(sliding_window=0), dict(sliding_window=-3), dict(sliding_window=2.5),
                                dict(sliding_window=True), dict(sliding_window=4, sliding_window_pattern=1),
                                dict(sliding_window=4, sliding_window_pattern=0), dict(sliding_window_pattern=2),
                                dict(sliding_window=4, sliding_window_pattern=2.5)])
def test_invalid_values_raise(kw):
    with pytest.raises(ValueError):
        GPTConfig(**kw)


def test_unset_fields_leave_the_serialised_config_what_it_was():
    cfg = GPTConfig()
    assert cfg.sliding_window is None and cfg.sliding_window_pattern is None
    assert "sliding_window" not in cfg.to_dict() and "sliding_window_pattern" not in cfg.to_dict()
    assert "sliding_window" not in cfg.__getstate__() and "sliding_window_pattern" not in cfg.__getstate__()
    names = [f.name for f in __import__("dataclasses").fields(GPTConfig)]
    assert names[-2:] == ["sliding_window", "sliding_window_pattern"]
    on = GPTConfig(sliding_window=128, sliding_window_pattern=3)
    d = on.to_dict()
    assert list(d)[-2:] == ["sliding_window", "sliding_window_pattern"] and d["sliding_window"] == 128
    assert GPTConfig.from_dict(d) == on and pickle.loads(pickle.dumps(on)) == on
    only_w = GPTConfig(sliding_window=128)
    assert "sliding_window_pattern" not in only_w.to_dict() and pickle.loads(pickle.dumps(only_w)) == only_w
    assert pickle.loads(pickle.dumps(cfg)).sliding_window is None
    # no parameters, no state-dict keys
    assert on.num_parameters() == cfg.num_parameters()
    assert list(GPT(tiny()).state_dict()) == list(GPT(tiny(sliding_window=None)).state_dict())


def test_an_old_pickle_loads_without_the_fields():
    state = {k: v for k, v in GPTConfig.gpt2_small().__dict__.items()
             if k not in ("sliding_window", "sliding_window_pattern", "qk_norm", "num_kv_heads")}
    old = GPTConfig.__new__(GPTConfig)
    old.__setstate__(state)
    assert old.sliding_window is None and old.sliding_window_pattern is None and old == GPTConfig.gpt2_small()
    assert old.layer_window(0) is None


def test_layer_window_follows_the_pattern():
    assert [GPTConfig(num_layers=6).layer_window(i) for i in range(6)] == [None] * 6
    assert [GPTConfig(num_layers=6, sliding_window=9).layer_window(i) for i in range(6)] == [9] * 6
    two = GPTConfig(num_layers=6, sliding_window=9, sliding_window_pattern=2)
    assert [two.layer_window(i) for i in range(6)] == [9, None, 9, None, 9, None]
    three = GPTConfig(num_layers=7, sliding_window=9, sliding_window_pattern=3)
    assert [three.layer_window(i) for i in range(7)] == [9, 9, None, 9, 9, None, 9]
    m = GPT(tiny(num_layers=4, sliding_window_pattern=2))
    assert [layer.attention.window for layer in m.layers] == [5, None, 5, None]


@pytest.mark.parametrize("S,W,N", [(16, 1, None), (16, 5, None), (16, 16, None), (16, 40, None), (16, 5, 2), (33, 7, 3)])
def test_flops_per_token_counts_the_window(S, W, N):
    base = dict(vocab_size=100, hidden_size=32, num_layers=6, num_heads=2, max_seq_len=S)
    plain = GPTConfig(**base)
    cfg = GPTConfig(**base, sliding_window=W, sliding_window_pattern=N)
    h, L = 32, 6
    attn = 0.0
    for i in range(L):
        if cfg.layer_window(i) is None:
            keys = S / 2.0  # the plain count, as flops_per_token has it for a causal layer
        else:
            keys = sum(len([k for k in range(S) if q - W < k <= q]) for q in range(S)) / S  # brute force
        attn += 2 * 2 * h * keys
    dense = plain.flops_per_token(S) / 3.0 - 2 * 2 * S * h * L * 0.5
    assert cfg.flops_per_token(S) == pytest.approx(3.0 * (dense + attn), rel=1e-12)
    assert cfg.flops_per_token(S, recompute=True) == pytest.approx(4.0 * (dense + attn), rel=1e-12)
    assert plain.flops_per_token(S) == 3.0 * (dense + 2 * 2 * S * h * L * 0.5)  # unset: unchanged
    if W < S:
        assert cfg.flops_per_token(S) < plain.flops_per_token(S)


# ------------------------------------------------------------------ window_bounds
def _ids_with_seps(B, S, seps_per_row, sep=SEP):
    ids = torch.randint(sep + 1, 200, (B, S))
    for b, seps in enumerate(seps_per_row):
        for j in seps:
            ids[b, j] = sep
    return ids


def _check_bounds(lo, hi, allowed):
    """Monotone, lo <= i <= hi, and both forms of the mask are ``allowed`` [B, S(q), S(k)]."""
    B, S = lo.shape
    pos = torch.arange(S, dtype=torch.int32)
    assert lo.dtype == hi.dtype == torch.int32 and lo.is_contiguous() and hi.is_contiguous()
    assert (lo[:, 1:] >= lo[:, :-1]).all() and (hi[:, 1:] >= hi[:, :-1]).all(), "bounds must be monotone"
    assert (lo <= pos).all() and (pos <= hi).all()
    q, k = pos.view(1, S, 1), pos.view(1, 1, S)
    by_lo = (lo.unsqueeze(2) <= k) & (k <= q)
    by_hi = (k <= q) & (q <= hi.unsqueeze(1))
    assert torch.equal(by_lo, allowed) and torch.equal(by_hi, allowed)


@pytest.mark.parametrize("W", [1, 2, 5, 6, 7, 100])
def test_window_bounds(W):
    B, S = 2, 6
    lo, hi = ref.window_bounds(B, S, W, "cpu")
    pos = torch.arange(S)
    win = ((pos.view(1, 1, S) <= pos.view(1, S, 1)) & (pos.view(1, 1, S) > pos.view(1, S, 1) - W)).expand(B, S, S)
    _check_bounds(lo, hi, win)
    # merged with the document bounds, on the layouts of tests/test_doc_mask_cpu.py
    for row in ([SEP, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, SEP], [1, 2, SEP, SEP, 3, 4], [1, 2, 3, 4, 5, 6],
                [SEP, SEP, SEP, 1, SEP, 2]):
        ids = torch.tensor([row, list(reversed(row))])
        dlo, dhi = ref.doc_bounds(ids, SEP)
        mlo, mhi = ref.window_bounds(B, S, W, "cpu", doc=(dlo, dhi))
        doc = (dlo.unsqueeze(2) <= pos.view(1, 1, S)) & (pos.view(1, 1, S) <= pos.view(1, S, 1))
        _check_bounds(mlo, mhi, win & doc)
    for ns in (ops.CPU_OPS, __import__("distributed_llm_trainer_amd.ops.hip", fromlist=["x"])):
        a, b = ns.window_bounds(B, S, W, "cpu")
        assert torch.equal(a, lo) and torch.equal(b, hi)
    with pytest.raises(ValueError):
        ref.window_bounds(B, S, 0, "cpu")


# ------------------------------------------------ reference ops vs a dense windowed softmax
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("W", [1, 31, 64, 65, 200, 500])
def test_reference_ops_match_a_dense_windowed_softmax(W, p):
    torch.manual_seed(W)
    B, nh, nkv, S, hd = 2, 4, 2, 200, 8
    q = torch.randn(B, nh, S, hd, requires_grad=True)
    k, v = (torch.randn(B, nkv, S, hd, requires_grad=True) for _ in range(2))
    key = rng.site_key(3, 1, 0, rng.SITE_ATTN)
    pos = torch.arange(S)
    allowed = (pos.view(1, S) <= pos.view(S, 1)) & (pos.view(1, S) > pos.view(S, 1) - W)
    s = (q @ k.repeat_interleave(2, dim=1).transpose(-2, -1)) / math.sqrt(hd)
    prob = torch.softmax(s.masked_fill(~allowed, float("-inf")), dim=-1)
    if p > 0:
        prob = prob * rng.attn_keep_mask(B * nh, S, S, key, p).view(B, nh, S, S) / (1.0 - p)
    want = prob @ v.repeat_interleave(2, dim=1)
    do = torch.randn(B, nh, S, hd)
    gq, gk, gv = torch.autograd.grad(want, (q, k, v), do)
    qd, kd, vd = q.detach(), k.detach(), v.detach()
    o, lse = ref.attention_fwd(qd, kd, vd, p, key, window=W)
    assert torch.allclose(o.view(B, S, nh, hd).transpose(1, 2), want, atol=1e-5, rtol=1e-4)
    assert torch.allclose(lse, torch.logsumexp(s.detach().masked_fill(~allowed, float("-inf")), -1), atol=1e-5)
    do_rows = do.transpose(1, 2).reshape(B * S, nh * hd)
    for a, b, n in zip(ref.attention_bwd(qd, kd, vd, o, do_rows, lse, p, key, window=W), (gq, gk, gv), ("dq", "dk", "dv")):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-4), n
    # window= is doc=window_bounds(...), and a window that covers the sequence is no window
    o2, lse2 = ref.attention_fwd(qd, kd, vd, p, key, doc=ref.window_bounds(B, S, W, "cpu"))
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    o0, lse0 = ref.attention_fwd(qd, kd, vd, p, key)
    assert (torch.equal(o, o0) and torch.equal(lse, lse0)) == (W >= S)


def test_reference_packed_ops_take_the_window_and_merge_it_with_doc():
    torch.manual_seed(1)
    B, S, nh, hd, W = 2, 24, 2, 8, 5
    qkv = torch.randn(B * S, 3 * nh * hd)
    ids = _ids_with_seps(B, S, [[3, 11], []])
    doc = ref.doc_bounds(ids, SEP)
    key = rng.site_key(1, 0, 0, rng.SITE_ATTN)
    cos, sin = ref.rope_tables(hd, S)
    o1, lse1 = ref.attention_fwd_packed(qkv, B, S, nh, 0.1, key, doc=doc, window=W)
    merged = ref.window_bounds(B, S, W, "cpu", doc=doc)
    o2, lse2 = ref.attention_fwd_packed(qkv, B, S, nh, 0.1, key, doc=merged)
    o3, _ = ref.attention_fwd_packed(qkv, B, S, nh, 0.1, key, doc=merged, window=W)  # folded in once
    assert torch.equal(o1, o2) and torch.equal(lse1, lse2) and torch.equal(o1, o3)
    do = torch.randn(B * S, nh * hd)
    g1 = ref.attention_bwd_packed(qkv, o1, do, lse1, 0.1, key, B, S, nh, cos, sin, doc=doc, window=W)
    g2 = ref.attention_bwd_packed(qkv, o1, do, lse1, 0.1, key, B, S, nh, cos, sin, doc=merged)
    assert torch.equal(g1, g2)
    assert not torch.equal(o1, ref.attention_fwd_packed(qkv, B, S, nh, 0.1, key, doc=doc)[0])
    with pytest.raises(ValueError):
        ref.attention_fwd_packed(qkv, B, S, nh, 0.1, key, window=0)


# ------------------------------------------------------------------ eager model
def _rot(x, cos, sin):
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def _autograd_loss(m, ids, seed=0, micro=0, sep=None, p_attn=0.0, p_hidden=0.0, logits=False):
    """The model as an independent dense formula over ``m``'s parameters (plain autograd): the
    window of each layer from ``config.layer_window``, the dense document mask, QK-norm,
    grouped K/V heads and the engine's counter-hash dropout masks."""
    cfg = m.config
    B, S = ids.shape
    nh, nkv, hd, H = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.hidden_size
    pos = torch.arange(S)
    causal = (pos.view(1, 1, 1, S) <= pos.view(1, 1, S, 1)).expand(B, 1, S, S)
    if sep is not None:
        lo, _ = ref.doc_bounds(ids, sep)
        causal = causal & (pos.view(1, 1, 1, S) >= lo.view(B, 1, S, 1))
    cos, sin = ref.rope_tables(hd, S)
    cos, sin = cos.view(1, 1, S, hd // 2), sin.view(1, 1, S, hd // 2)

    def drop(x, key, p):
        return x * rng.keep_mask(x.shape, key, p) / (1.0 - p) if p > 0 else x

    def norm(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w

    x = m.embed_tokens.weight[ids.reshape(-1)]
    for i, layer in enumerate(m.layers):
        k_attn, k_resid, k_mlp = (rng.site_key(seed, micro, i, s) for s in (rng.SITE_ATTN, rng.SITE_RESID, rng.SITE_MLP))
        W = cfg.layer_window(i)
        allowed = causal if W is None else causal & (pos.view(1, 1, 1, S) > pos.view(1, 1, S, 1) - W)
        at = layer.attention
        n1 = norm(x, layer.input_layernorm.weight)
        q = (n1 @ at.q_proj.weight.t()).view(B, S, nh, hd).transpose(1, 2)
        k = (n1 @ at.k_proj.weight.t()).view(B, S, nkv, hd).transpose(1, 2)
        v = (n1 @ at.v_proj.weight.t()).view(B, S, nkv, hd).transpose(1, 2)
        if cfg.qk_norm:
            q, k = norm(q, at.q_norm.weight), norm(k, at.k_norm.weight)
        q, k = _rot(q, cos, sin), _rot(k, cos, sin)
        idx = torch.arange(nh) // (nh // nkv)
        s = (q @ k[:, idx].transpose(-2, -1)) / math.sqrt(hd)
        pr = torch.softmax(s.masked_fill(~allowed, float("-inf")), dim=-1)
        if p_attn > 0:
            pr = pr * rng.attn_keep_mask(B * nh, S, S, k_attn, p_attn).view(B, nh, S, S) / (1.0 - p_attn)
        a = (pr @ v[:, idx]).transpose(1, 2).reshape(B * S, H) @ at.o_proj.weight.t()
        x = x + drop(a, k_resid, p_hidden)
        n2 = norm(x, layer.post_attention_layernorm.weight)
        mlp = layer.mlp
        d = (F.silu(n2 @ mlp.gate_proj.weight.t()) * (n2 @ mlp.up_proj.weight.t())) @ mlp.down_proj.weight.t()
        x = x + drop(d, k_mlp, p_hidden)
    lg = norm(x, m.norm.weight) @ m.embed_tokens.weight.t()
    if logits:
        return lg.view(B, S, -1)
    return F.cross_entropy(lg, shift_targets(ids), ignore_index=-100)


def _randomise_norms(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in m.layers:
            if m.config.qk_norm:
                for n in (layer.attention.q_norm, layer.attention.k_norm):
                    n.weight.copy_(1.0 + 0.5 * torch.randn(n.weight.shape, generator=g))
    return m


def _sep_ids(B=3, S=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(SEP + 1, 256, (B, S), generator=g)
    ids[0, [4, 5, 19]] = SEP
    ids[2, 31] = SEP
    return ids


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("kw,sep", [(dict(), None), (dict(num_kv_heads=2, qk_norm=True), SEP),
                                    (dict(sliding_window_pattern=2), None), (dict(sliding_window=1), SEP)])
def test_eager_model_matches_the_dense_formula(kw, sep, flash):
    torch.manual_seed(0)
    m = _randomise_norms(GPT(tiny(use_flash_attention=flash, **kw)))
    m.set_doc_separator(sep)
    m2 = copy.deepcopy(m)
    ids = _sep_ids()
    _, l1 = m(ids, labels=ids)
    l1.backward()
    l2 = _autograd_loss(m2, ids, sep=sep)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n
    # the window is live: the same weights without it give another loss
    off = GPT(GPTConfig.from_dict({k: v for k, v in m.config.to_dict().items() if not k.startswith("sliding")}))
    off.load_state_dict(m.state_dict())
    off.set_doc_separator(sep)
    assert abs(off(ids, labels=ids)[1].item() - l1.item()) > 1e-4


@pytest.mark.parametrize("flash", [False, True])
def test_receptive_field_of_two_windowed_layers(flash):
    """Token 0 reaches position q through two layers of window W only if q <= 2 (W - 1)."""
    torch.manual_seed(1)
    W = 5
    m = GPT(tiny(sliding_window=W, use_flash_attention=flash)).eval()
    ids = torch.randint(0, 256, (2, 32))
    ids2 = ids.clone()
    ids2[:, 0] = (ids[:, 0] + 1) % 256
    with torch.no_grad():
        a, b = m(ids)[0], m(ids2)[0]
    reach = 2 * (W - 1)
    # rows beyond the reach take no input that changed, and the CPU matmuls compute each row
    # of a batch from that row alone: the same bits
    assert torch.equal(a[:, reach + 1:], b[:, reach + 1:])
    assert (a[:, :reach + 1] != b[:, :reach + 1]).any(dim=-1).all(), "every position inside the reach changes"
    # a pattern model (layer 1 global) and the causal model see token 0 everywhere
    for kw in (dict(sliding_window_pattern=2), dict(sliding_window=None)):
        g = GPT(tiny(**{**dict(sliding_window=W, use_flash_attention=flash), **kw})).eval()
        g.load_state_dict(m.state_dict())
        with torch.no_grad():
            assert (g(ids)[0][:, -1] != g(ids2)[0][:, -1]).any()


def test_pattern_model_differs_from_all_windowed_and_from_causal():
    torch.manual_seed(2)
    base = GPT(tiny(sliding_window=4)).eval()
    ids = torch.randint(0, 256, (2, 32))
    outs = []
    for kw in (dict(sliding_window=4), dict(sliding_window=4, sliding_window_pattern=2), dict(sliding_window=None)):
        m = GPT(tiny(**kw)).eval()
        m.load_state_dict(base.state_dict())
        with torch.no_grad():
            outs.append(m(ids)[0])
    for i in range(3):
        for j in range(i + 1, 3):
            assert (outs[i] - outs[j]).abs().max().item() > 1e-4
        assert torch.equal(outs[i][:, :4], outs[0][:, :4])  # the first W positions see everything anyway


# ------------------------------------------------------------------ engine on the reference ops
@pytest.mark.parametrize("recompute,selective", [(False, True), (True, True), (True, False)])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("kw,sep", [(dict(), None), (dict(num_kv_heads=2, qk_norm=True), SEP),
                                    (dict(sliding_window_pattern=2), SEP)])
def test_engine_matches_autograd_with_the_same_dropout_masks(recompute, selective, packed, kw, sep):
    torch.manual_seed(3)
    m1 = _randomise_norms(GPT(tiny(dropout=0.1, attention_dropout=0.1, **kw)))
    m2 = copy.deepcopy(m1)
    ids = _sep_ids(seed=3)
    l1 = _autograd_loss(m1, ids, seed=21, micro=0, sep=sep, p_attn=0.1, p_hidden=0.1)
    l1.backward()
    m2.set_doc_separator(sep)
    eng = m2.enable_engine(seed=21)
    eng.packed_qkv = packed and eng.packed_qkv
    eng.selective_recompute = selective
    m2.gradient_checkpointing = recompute
    m2.train()
    _, l2 = m2(ids, labels=ids)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n


def test_engine_chain_state_and_cached_bounds():
    m = GPT(tiny(sliding_window_pattern=2))
    eng = m.enable_engine()
    ids = _sep_ids()
    st = types.SimpleNamespace(B=3, S=32, doc=None)
    w1 = eng._window_bounds(st, ids.device)
    assert w1 is eng._window_bounds(st, ids.device), "without a separator the bounds are built once"
    st.win = w1
    assert eng._attn_kw(st, 0, None) == {"doc": w1, "window": 5} and eng._attn_kw(st, 1, None) == {}
    st.doc = ref.doc_bounds(ids, SEP)
    st.win = eng._window_bounds(st, ids.device)
    assert torch.equal(st.win[0], torch.maximum(w1[0], st.doc[0])) and torch.equal(st.win[1], torch.minimum(w1[1], st.doc[1]))
    assert eng._attn_kw(st, 1, None) == {"doc": st.doc}
    st.S = 5  # the window covers the batch: the plain path
    assert eng._window_bounds(st, ids.device) is None


@pytest.mark.parametrize("W", [32, 33, 1000])
def test_a_window_that_covers_the_batch_is_the_model_without_one(W):
    torch.manual_seed(4)
    base = GPT(tiny(sliding_window=None, dropout=0.1, attention_dropout=0.1))
    ids = torch.randint(0, 256, (2, 32))
    res = []
    for w in (None, W):
        m = GPT(tiny(sliding_window=w, dropout=0.1, attention_dropout=0.1))
        m.load_state_dict(base.state_dict())
        with torch.no_grad():
            eager = m.eval()(ids)[0]
        m.train()
        m.enable_engine(seed=11)
        _, loss = m(ids, labels=ids)
        loss.backward()
        res.append((eager, loss.item(), [p.grad.clone() for p in m.parameters()]))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    for a, b in zip(res[0][2], res[1][2]):
        assert torch.equal(a, b)


def test_eval_loss_applies_the_window():
    torch.manual_seed(6)
    m = GPT(tiny())
    off = GPT(tiny(sliding_window=None))
    off.load_state_dict(m.state_dict())
    ids = torch.randint(0, 256, (2, 32))
    want = _autograd_loss(m, ids).item()
    m.enable_engine()
    off.enable_engine()
    assert abs(m.eval_loss(ids).item() - want) < 1e-5
    assert abs(off.eval_loss(ids).item() - want) > 1e-4


def test_routes_that_refuse_the_window():
    ops.check_attention_features("cpu", 160, torch.float32, {"window"})  # the CPU ops mask densely
    ops.check_attention_features("cuda", 64, torch.bfloat16, {"window"})
    ops.check_attention_features("cuda", 96, torch.float16, {"window"})   # zero-padded onto the flash kernels
    with pytest.raises(NotImplementedError, match="GEMM-formulated"):
        ops.check_attention_features("cuda", 160, torch.bfloat16, {"window"})
    with pytest.raises(NotImplementedError, match="fp32"):
        ops.check_attention_features("cuda", 64, torch.float32, {"window"})
    with pytest.raises(NotImplementedError, match="sliding"):
        ops.check_attention_features("cuda", 96, torch.float32, {"window"})


# ------------------------------------------------------------------ checkpoints and the CLI
DIST = dict(vocab_size=384, hidden_size=64, num_layers=2, num_heads=4, max_seq_len=16, dropout=0.0,
            attention_dropout=0.0, sliding_window=6, sliding_window_pattern=2)


def _ddp_trainer():
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=1, warmup_steps=1, max_steps=100, learning_rate=1e-2)
    return DistributedTrainer(GPTConfig(**DIST), tc)


def test_full_checkpoint_round_trip_and_generate(tmp_path):
    from distributed_llm_trainer_amd.eval.infer import load_model
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    tr = _ddp_trainer()
    g = torch.Generator().manual_seed(0)
    for _ in range(2):
        tr.train_step({"input_ids": torch.randint(0, 384, (2, 16), generator=g)})
    path = str(tmp_path / "win.pt")
    tr.save_checkpoint(path)
    tr2 = _ddp_trainer()
    tr2.load_checkpoint(path)
    assert torch.equal(tr2.flat_params(), tr.flat_params())
    back = load_model(path)
    assert back.config.sliding_window == 6 and back.config.sliding_window_pattern == 2
    assert back.config == tr.model.config and [l.attention.window for l in back.layers] == [6, None]
    ids = torch.randint(0, 384, (1, 5))
    assert back.generate(ids, max_new_tokens=4, top_k=1).shape == (1, 9)
    # the flags override a stored config that does not carry the fields
    ck = load_checkpoint(path, map_location="cpu")
    ck["model_config"] = GPTConfig.from_dict({k: v for k, v in DIST.items() if not k.startswith("sliding")})
    save_checkpoint(path, ck)
    assert load_model(path).config.sliding_window is None
    over = load_model(path, sliding_window=3, sliding_window_pattern=2).config
    assert over.sliding_window == 3 and over.sliding_window_pattern == 2


def _yaml(tmp_path, w, n=None):
    p = tmp_path / "m.yaml"
    extra = (f"  sliding_window: {w}\n" if w is not None else "") + (f"  sliding_window_pattern: {n}\n" if n is not None else "")
    p.write_text("model:\n  hidden_size: 64\n  num_layers: 2\n  num_heads: 4\n  vocab_size: 128\n"
                 "  max_seq_len: 16\n" + extra)
    return str(p)


@pytest.mark.parametrize("trainer", ["ddp_trainer", "fsdp_trainer"])
def test_cli_flag_precedence(tmp_path, trainer):
    """CLI > YAML > preset, in both trainers."""
    import importlib
    mod = importlib.import_module(f"distributed_llm_trainer_amd.training.{trainer}")
    from distributed_llm_trainer_amd.training.common import apply_model_args
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.utils.config_loader import load_yaml_config
    parser = mod.build_parser()
    assert parser.parse_args([]).sliding_window is None and parser.parse_args([]).sliding_window_pattern is None

    def resolve(argv, yaml_w="absent", yaml_n=None):
        args = parser.parse_args(argv)
        cfg = GPTConfig.from_preset("small")
        if yaml_w != "absent":
            cfg = load_yaml_config(_yaml(tmp_path, yaml_w, yaml_n), cfg, TrainingConfig(), None)[0]
        apply_model_args(args, cfg)
        return cfg.sliding_window, cfg.sliding_window_pattern

    assert resolve([]) == (None, None)                                             # preset
    assert resolve(["--sliding_window", "64"]) == (64, None)                       # CLI over the preset
    assert resolve([], None) == (None, None)                                       # YAML without the keys
    assert resolve([], 8, 2) == (8, 2)                                             # YAML over the preset
    assert resolve(["--sliding_window", "4"], 8, 2) == (4, 2)                      # CLI over YAML, key by key
    assert resolve(["--sliding_window_pattern", "3"], 8, 2) == (8, 3)
    assert resolve(["--sliding_window", "4", "--sliding_window_pattern", "3"], 8) == (4, 3)
    with pytest.raises(ValueError):
        resolve(["--sliding_window_pattern", "2"])                                 # needs a window
    with pytest.raises(ValueError):
        resolve(["--sliding_window", "0"])


def test_cli_trains_and_infers_a_windowed_model(tmp_path, capsys):
    """--sliding_window reaches the trainer's model and its checkpoint; infer.py reads it back,
    together with --num_kv_heads, --qk_norm and --doc_sep_token."""
    from distributed_llm_trainer_amd.eval import infer
    from distributed_llm_trainer_amd.training import ddp_trainer
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint
    env_before = os.environ.get("DLT_DUMMY_BATCHES")
    os.environ["DLT_DUMMY_BATCHES"] = "2"
    try:
        ddp_trainer.main(["--config", _yaml(tmp_path, 8), "--sliding_window", "4", "--sliding_window_pattern", "2",
                          "--num_kv_heads", "2", "--qk_norm", "--doc_sep_token", "5", "--batch_size", "1",
                          "--max_steps", "1", "--gradient_accumulation_steps", "1", "--checkpoint_dir",
                          str(tmp_path / "ck")])
    finally:
        if env_before is None:
            os.environ.pop("DLT_DUMMY_BATCHES", None)
        else:
            os.environ["DLT_DUMMY_BATCHES"] = env_before
    path = str(tmp_path / "ck" / "final.pt")
    cfg = load_checkpoint(path, map_location="cpu")["model_config"]
    assert (cfg.sliding_window, cfg.sliding_window_pattern, cfg.num_kv_heads, cfg.qk_norm) == (4, 2, 2, True)
    m = infer.load_model(path)
    assert [l.attention.window for l in m.layers] == [4, None]
    infer.main(["--checkpoint", path, "--tokenizer", "byte", "--prompt", "ab", "--max_new_tokens", "3", "--device", "cpu"])
    assert infer.load_model(path, sliding_window=2).config.sliding_window == 2          # the infer.py flag wins


# ------------------------------------------------------------------ generation
@pytest.mark.parametrize("kw", [dict(), dict(num_kv_heads=2), dict(sliding_window_pattern=2), dict(qk_norm=True)])
def test_kv_cached_generate_matches_greedy_full_forward(kw):
    """A prompt longer than W and a generation that crosses W more than once."""
    torch.manual_seed(5)
    m1 = _randomise_norms(GPT(tiny(**kw)))
    m2 = copy.deepcopy(m1)
    m2.enable_engine()
    ids = torch.randint(0, 256, (2, 9))
    o1 = m1.generate(ids, max_new_tokens=14, temperature=1.0, top_k=1)  # greedy full re-forward
    o2 = m2.generate(ids, max_new_tokens=14, temperature=1.0, top_k=1)
    assert o1.shape == (2, 23) and torch.equal(o1, o2)
    # the window is live in the cached path: the last-position logits differ from the causal model's
    from distributed_llm_trainer_amd.eval.decode import KVCache, forward_cached
    off = GPT(tiny(**{**kw, "sliding_window": None, "sliding_window_pattern": None}))
    off.load_state_dict(m1.state_dict())
    off.enable_engine()
    lg = forward_cached(m2, ids, KVCache(m2.config, 2, "cpu", m2.engine.act_dtype))
    lg0 = forward_cached(off, ids, KVCache(off.config, 2, "cpu", off.engine.act_dtype))
    assert (lg - lg0).abs().max().item() > 1e-4
    # one token at a time through the cache == the prefill of the whole prompt
    c = KVCache(m2.config, 2, "cpu", m2.engine.act_dtype)
    for t in range(ids.shape[1]):
        step = forward_cached(m2, ids[:, t:t + 1], c)
    assert torch.allclose(step, lg, atol=1e-5, rtol=1e-5)


def _stub(nh, nkv, maxS, **fields):
    o = types.SimpleNamespace(backend="hip", dec_norm_qkv=lambda *a: None, DECODE_BATCHES=(1, 2, 4, 8),
                              dec_attn_gqa=lambda *a: None)
    cfg = types.SimpleNamespace(num_heads=nh, num_kv_heads=nkv, head_dim=64, hidden_size=nh * 64, max_seq_len=maxS,
                                **fields)
    return types.SimpleNamespace(engine=types.SimpleNamespace(ops=o), config=cfg)


def test_fused_kind_uses_the_largest_need_over_the_layers(monkeypatch):
    from distributed_llm_trainer_amd.eval.decode import _attn_keys, _fused_kind
    monkeypatch.delenv("DLT_DECODE_KV_SPLITS", raising=False)
    monkeypatch.delenv("DLT_DECODE_FUSED", raising=False)
    # stubs without the fields behave as before: k_dec_attn holds maxS * 4 + 1056 bytes
    assert _fused_kind(_stub(12, 12, 40000), 1) == "mha" and _fused_kind(_stub(12, 12, 41000), 1) is None
    # every layer windowed: min(W, maxS) keys
    assert _fused_kind(_stub(12, 12, 65536, sliding_window=1024, sliding_window_pattern=None, num_layers=4), 1) == "mha"
    assert _fused_kind(_stub(12, 12, 65536, sliding_window=50000, sliding_window_pattern=None, num_layers=4), 1) is None
    assert _fused_kind(_stub(12, 12, 1024, sliding_window=50000, sliding_window_pattern=None, num_layers=4), 1) == "mha"
    # a pattern model has global layers, which need what they need today ...
    pat = dict(sliding_window=1024, sliding_window_pattern=2, num_layers=4)
    assert _fused_kind(_stub(12, 12, 65536, **pat), 1) is None and _fused_kind(_stub(12, 12, 4096, **pat), 1) == "mha"
    # ... unless the pattern never comes round within the layers
    assert _attn_keys(_stub(12, 12, 65536, sliding_window=1024, sliding_window_pattern=5, num_layers=4).config) == 1024
    # grouped-query: 16 heads over maxS / 8 = 8192 keys do not fit, over 1024 / 8 they do
    assert _fused_kind(_stub(16, 1, 65536), 1) is None
    assert _fused_kind(_stub(16, 1, 65536, sliding_window=1024, sliding_window_pattern=None, num_layers=2), 1) == "gqa"
    assert _fused_kind(_stub(16, 1, 65536, sliding_window=1024, sliding_window_pattern=2, num_layers=2), 1) is None
    # real configs
    m = GPT(GPTConfig(vocab_size=64, hidden_size=128, num_layers=2, num_heads=2, max_seq_len=64, sliding_window=8))
    assert _attn_keys(m.config) == 8
    assert _attn_keys(GPTConfig(num_layers=2, sliding_window=8, sliding_window_pattern=2)) == 1024


# ------------------------------------------------------------------ planted defects
def _inside(out, chk):
    return bool(((out.double().reshape(chk.ref.shape) - chk.ref).abs() <= chk.tol).all())


@pytest.mark.parametrize("nh,nkv", WR.GQA_HEADS)
@pytest.mark.parametrize("W,NS", [(50, 1), (50, 2), (50, 4), (50, 8), (7, 8), (7, 4)])
def test_fp32_model_is_inside_the_tolerance_and_every_defect_outside(nh, nkv, W, NS):
    """At the GPU tests' inputs: the window-anchored fp32 model passes the check the kernel
    has to pass (the output against the fp64 reference at its tolerance, the chunk partials
    against the model's), and each planted defect fails it at some position the GPU test
    visits."""
    maxS = WR.GQA_MAXS
    C = WR.chunk(maxS, W, NS)
    assert (W, NS, C) != (50, 4, 0) and (C == 13 if (W, NS) == (50, 4) else True) and (C == 1 if (W, NS) == (7, 8) else True)
    caught = {d: False for d in WR.DEFECTS}
    for kind in ("randn", "large60"):
        q, kc, vc = G.attn_gqa_inputs(nh, nkv, maxS, kind)
        for pos in WR.gqa_positions(W, C, NS):
            chk = WR.attn_gqa_win_ref(q, kc, vc, pos, G.ATTN_SCALE, nh, W)
            good = WR.attn_gqa_win_split32(q, kc, vc, pos, G.ATTN_SCALE, nh, NS, W)
            assert _inside(good.o, chk), (kind, pos)
            for d in WR.DEFECTS:
                bad = WR.attn_gqa_win_split32(q, kc, vc, pos, G.ATTN_SCALE, nh, NS, W, defect=d)
                if not _inside(bad.o, chk) or not WR.partials_match(bad, good):
                    caught[d] = True
    if NS == 1:  # one chunk: how the chunks are cut cannot matter
        caught["chunks_anchored_at_0"] = caught["chunk_from_maxS"] = True
    assert all(caught.values()), caught


@pytest.mark.parametrize("kind", ["randn", "large60"])
def test_a_window_on_a_global_layer_is_outside_the_tolerance(kind):
    """The fifth defect: a pattern model's global layer run with the window (or a windowed one
    without).  Both directions are outside the fp64 tolerance once pos >= W."""
    nh, nkv, W, maxS = 4, 2, 50, WR.GQA_MAXS
    q, kc, vc = G.attn_gqa_inputs(nh, nkv, maxS, kind)
    for pos in (W, maxS - 1):
        glob = WR.attn_gqa_win_ref(q, kc, vc, pos, G.ATTN_SCALE, nh, None)
        win = WR.attn_gqa_win_ref(q, kc, vc, pos, G.ATTN_SCALE, nh, W)
        assert _inside(WR.attn_gqa_win_split32(q, kc, vc, pos, G.ATTN_SCALE, nh, 4, None).o, glob)
        assert not _inside(WR.attn_gqa_win_split32(q, kc, vc, pos, G.ATTN_SCALE, nh, 4, W).o, glob)
        assert not _inside(WR.attn_gqa_win_split32(q, kc, vc, pos, G.ATTN_SCALE, nh, 4, None).o, win)
    # below W the two are the same layer
    a = WR.attn_gqa_win_split32(q, kc, vc, W - 1, G.ATTN_SCALE, nh, 4, W)
    b = WR.attn_gqa_win_split32(q, kc, vc, W - 1, G.ATTN_SCALE, nh, 4, maxS)
    assert torch.equal(a.o, b.o)


@pytest.mark.parametrize("W", WR.MHA_WINDOWS)
def test_mha_window_reference_and_off_by_one_defects(W):
    """dec_attn(window=W): the fp64 reference on the slice; one key too many or too few is
    outside its tolerance wherever the window is full and does not cover the cache."""
    from tests import decode_ref as R
    q, kc, vc = R.attn_inputs(WR.MHA_NH, WR.MHA_MAXS, "randn")  # every key carries weight
    q, kc, vc = q[:2], kc[:2], vc[:2]
    for pos in WR.mha_positions(W):
        chk = WR.attn_win_ref(q, kc, vc, pos, R.ATTN_SCALE, W)
        kf = WR.first_key(pos, W)
        assert kf == max(0, pos - W + 1) and pos - kf + 1 == min(W, pos + 1)
        same = R.attn_ref(q, kc[:, :, kf:], vc[:, :, kf:], pos - kf, R.ATTN_SCALE)
        assert torch.equal(chk.ref, same.ref)
        if kf > 0:
            more = R.attn_ref(q, kc[:, :, kf - 1:], vc[:, :, kf - 1:], pos - kf + 1, R.ATTN_SCALE).ref
            assert not ((more - chk.ref).abs() <= chk.tol).all(), ("key pos - W included", pos)
            if W > 1:
                less = R.attn_ref(q, kc[:, :, kf + 1:], vc[:, :, kf + 1:], pos - kf - 1, R.ATTN_SCALE).ref
                assert not ((less - chk.ref).abs() <= chk.tol).all(), ("key pos - W + 1 dropped", pos)
