"""Attention sinks (``GPTConfig.attention_sinks``: one learned softmax logit per query head, no
value row) on the CPU: the kernels' fp64 references, fp32 models and planted defects
(tests/sink_ref.py), config, eager model, the reference ops, the engine on the reference ops, the
flat layout and optimizer groups, DDP / FSDP over gloo, checkpoints, the CLI flag and KV-cached
generation."""
import copy
import math
import os
import pickle

import pytest
import torch
import torch.nn.functional as F

from distributed_llm_trainer_amd.models import GPT, GPTConfig, count_parameters
from distributed_llm_trainer_amd.models.engine import shift_targets
from distributed_llm_trainer_amd.ops import reference as ref, rng
from tests import attn_ref as A
from tests import sink_ref as SR
from tests.dist_utils import run_multiprocess

SEP = 0
TINY = dict(vocab_size=256, hidden_size=64, num_layers=2, num_heads=4, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0, attention_sinks=True)


def tiny(**kw):
    d = dict(TINY)
    d.update(kw)
    return GPTConfig(**d)


def _randomise_sinks(m, seed=0):
    """Non-zero sinks (the init is zeros, which hides a swapped head or a scaled sink)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in m.layers:
            layer.attention.sinks.copy_(1.5 * torch.randn(layer.attention.sinks.shape, generator=g))
    return m


# ------------------------------------------------------------------ kernels: references, models, defects
SHOWN = [SR.DEFECT_CASE.name] + [c.name for c in SR.CASES if c.family == "big" or c.bounds == ("win", 1)][:2]


def test_case_list_holds_what_the_issue_names():
    cs = SR.CASES
    assert {c.B for c in cs} == {2} and {c.S for c in cs} == {192, 200}
    assert {(c.nh, c.nkv) for c in cs} == set(SR.HEADS)
    assert {c.hd for c in cs} == {64, 128} and {c.dtype for c in cs} == {A.BF, A.HF}
    assert {c.p for c in cs} == {0.0, 0.1} and {c.packed for c in cs} == {True, False}
    assert {c.bounds[1] for c in cs if c.bounds and c.bounds[0] == "win"} == set(SR.WINDOWS)
    assert any(c.bounds == ("doc",) for c in cs)
    # every DROP x HK x D x DOC x GQA form of the SINK forward
    forms = {(c.p > 0, c.dtype, c.hd, bool(c.bounds) and A.case_window(c) != 200, bool(c.nkv)) for c in cs}
    assert len(forms) == 32
    # a document boundary inside a 32-query half
    assert any(x % 32 not in (0, 31) for x in A.doc_seps(200))
    seen = set()
    for c in cs:
        seen |= set(SR.case_sinks(c).tolist())
    assert seen == set(SR.SINK_VALUES)


@pytest.mark.parametrize("name", SHOWN)
def test_fp32_models_of_the_kernels_are_inside_the_tolerance(name):
    c, r = SR.BY_NAME[name], SR.case_refs(name)
    o, lse = SR.sink_fwd_model(r.inp.q, r.inp.k, r.inp.v, r.inp.scale, r.sink, r.inp.doc, c.p, c.key)
    ws = (SR.worst(o, r.fwd.o), SR.worst(lse, r.fwd.lse), SR.worst(SR.sink_bwd_model(r.lse32, r.delta32, r.sink), r.dsink))
    print("worst err / tol: o %.3f lse %.3f dsink %.3f" % ws)
    assert max(ws) <= 1.0
    # dq, dk, dv: the existing backward's arithmetic, fed the sink forward's o and lse
    dq, dk, dv, delta = A.attn_bwd_emul(r.inp.q, r.inp.k, r.inp.v, r.o16, r.inp.do, r.lse32, r.inp.scale, r.inp.doc, c.p,
                                        c.key, r.inp.rope)
    for nm, t in (("dq", dq), ("dk", dk), ("dv", dv), ("delta", delta)):
        assert SR.worst(t, getattr(r.bwd, nm)) <= 1.0, nm


def test_a_sink_of_minus_infinity_is_the_plain_forward():
    c = SR.DEFECT_CASE
    inp = A.attn_inputs(c)
    none = torch.full((c.nh,), float("-inf"))
    got = SR.sink_fwd_ref(inp.q, inp.k, inp.v, inp.scale, none, inp.doc, c.p, c.key)
    want = A.attn_fwd_ref(inp.q, inp.k, inp.v, inp.scale, inp.doc, c.p, c.key)
    assert torch.equal(got.o.ref, want.o.ref) and torch.equal(got.lse.ref, want.lse.ref)
    assert torch.equal(got.lse.tol, want.lse.tol)
    o, lse = SR.sink_fwd_model(inp.q, inp.k, inp.v, inp.scale, none, inp.doc, c.p, c.key)
    assert SR.worst(o, want.o) <= 1.0 and SR.worst(lse, want.lse) <= 1.0
    d = SR.sink_bwd_ref(lse, torch.ones_like(lse), none)
    assert not d.ref.any() and SR.worst(SR.sink_bwd_model(lse, torch.ones_like(lse), none), d) <= 1.0


def test_a_sink_far_above_the_scores_gives_zero_output_and_lse_equal_to_the_sink():
    c = SR.DEFECT_CASE
    inp = A.attn_inputs(c)
    big = torch.full((c.nh,), 100.0)
    f = SR.sink_fwd_ref(inp.q, inp.k, inp.v, inp.scale, big, inp.doc, c.p, c.key)
    assert f.o.ref.abs().max() < 1e-30 and (f.lse.ref - 100.0).abs().max() < 1e-30
    o, lse = SR.sink_fwd_model(inp.q, inp.k, inp.v, inp.scale, big, inp.doc, c.p, c.key)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert SR.worst(o, f.o) <= 1.0 and SR.worst(lse, f.lse) <= 1.0


@pytest.mark.parametrize("defect", SR.FWD_DEFECTS)
def test_planted_forward_defects_are_outside_the_tolerance(defect):
    c, r = SR.DEFECT_CASE, SR.case_refs(SR.DEFECT_CASE.name)
    assert c.p > 0 and c.nkv == 2 and torch.equal(r.sink, SR.DEFECT_SINKS)
    o, lse = SR.sink_fwd_model(r.inp.q, r.inp.k, r.inp.v, r.inp.scale, r.sink, r.inp.doc, c.p, c.key, defect=defect)
    assert SR.worst(o, r.fwd.o) > 1.0
    if defect == "lse_only":  # lse is right: only o's normaliser misses the sink
        assert SR.worst(lse, r.fwd.lse) <= 1.0
    else:
        assert SR.worst(lse, r.fwd.lse) > 1.0


@pytest.mark.parametrize("defect", SR.BWD_DEFECTS)
def test_planted_dsink_defects_are_outside_the_tolerance(defect):
    c, r = SR.DEFECT_CASE, SR.case_refs(SR.DEFECT_CASE.name)
    got = SR.sink_bwd_model(r.lse32, r.delta32, r.sink, defect, dscale=1.0 / (1.0 - c.p))
    assert SR.worst(got, r.dsink) > 1.0


DEC_SHOWN = [(nh, nkv, NS, W) for nh, nkv in ((4, 2), (12, 4)) for NS in SR.DEC_SPLITS for W in (None, 50)]


@pytest.mark.parametrize("nh,nkv,NS,W", DEC_SHOWN)
def test_split_decode_model_and_its_planted_defects(nh, nkv, NS, W):
    q, kc, vc = SR.G.attn_gqa_inputs(nh, nkv, SR.DEC_MAXS, "randn")
    q, kc, vc = q[:2], kc[:2], vc[:2]
    sink = SR.sinks_for(nh, shift=2)  # 0, 2.5, 60, 100 (and the rest at nh = 12)
    assert {0.0, 60.0} <= set(sink.tolist())
    for pos in SR.dec_positions(W, NS):
        want = SR.dec_sink_ref(q, kc, vc, pos, SR.DEC_SCALE, nh, sink, W)
        got = SR.dec_sink_split32(q, kc, vc, pos, SR.DEC_SCALE, nh, NS, W, sink)
        assert torch.isfinite(got.float()).all()
        assert SR.worst(got, want) <= 1.0, pos
        C = SR.WN.chunk(SR.DEC_MAXS, W, NS)
        if NS > 1 and pos - SR.WN.first_key(pos, W) >= C:  # more than one chunk holds keys
            for d in SR.DEC_DEFECTS:
                bad = SR.dec_sink_split32(q, kc, vc, pos, SR.DEC_SCALE, nh, NS, W, sink, defect=d)
                assert SR.worst(bad, want) > 1.0, (d, pos)
    none = torch.full((nh,), float("-inf"))
    plain = SR.WN.attn_gqa_win_split32(q, kc, vc, 150, SR.DEC_SCALE, nh, NS, W).o
    assert torch.equal(SR.dec_sink_split32(q, kc, vc, 150, SR.DEC_SCALE, nh, NS, W, none), plain)


# ------------------------------------------------------------------ config
OLD_FIELDS = ["vocab_size", "hidden_size", "num_layers", "num_heads", "intermediate_size", "max_seq_len", "dropout",
              "attention_dropout", "initializer_range", "activation", "use_flash_attention", "gradient_checkpointing"]
# the keys of a pickled default config's state: the field names of before the feature, no more
PARENT_PICKLE_FIELDS = OLD_FIELDS


def test_config_without_the_flag_serialises_as_before():
    cfg = GPTConfig.gpt2_small()
    assert cfg.attention_sinks is False
    assert list(cfg.to_dict()) == OLD_FIELDS and list(cfg.__getstate__()) == PARENT_PICKLE_FIELDS
    assert pickle.dumps(cfg) == pickle.dumps(GPTConfig(attention_sinks=False))
    # the bytes are those of an object that never had the field
    bare = GPTConfig.__new__(GPTConfig)
    bare.__dict__.update({k: v for k, v in cfg.__dict__.items() if k != "attention_sinks"})
    assert pickle.dumps(cfg) == pickle.dumps(bare)
    assert GPTConfig.from_dict(cfg.to_dict()) == cfg
    on = tiny()
    assert on.to_dict()["attention_sinks"] is True and GPTConfig.from_dict(on.to_dict()) == on
    assert pickle.loads(pickle.dumps(on)).attention_sinks is True
    assert pickle.loads(pickle.dumps(cfg)).attention_sinks is False
    both = tiny(num_kv_heads=2, qk_norm=True, sliding_window=8)
    assert list(both.to_dict())[-4:] == ["num_kv_heads", "qk_norm", "attention_sinks", "sliding_window"]


def test_config_validation_and_old_pickles():
    with pytest.raises(ValueError, match="attention_sinks"):
        GPTConfig(attention_sinks="yes")
    with pytest.raises(ValueError, match="attention_sinks"):
        GPTConfig(attention_sinks=2)
    assert GPTConfig(attention_sinks=1).attention_sinks is True
    state = {k: v for k, v in GPTConfig.gpt2_small().__dict__.items() if k not in ("attention_sinks", "qk_norm", "num_kv_heads")}
    old = GPTConfig.__new__(GPTConfig)
    old.__setstate__(state)
    assert old.attention_sinks is False and old == GPTConfig.gpt2_small()


@pytest.mark.parametrize("nkv", [None, 2])
def test_num_parameters_counts_the_sinks(nkv):
    cfg = tiny(num_kv_heads=nkv)
    assert cfg.num_parameters() == count_parameters(GPT(cfg))
    assert cfg.num_parameters() - tiny(num_kv_heads=nkv, attention_sinks=False).num_parameters() == 2 * 4


def test_state_dict_keys_init_and_dtype():
    off, on = GPT(tiny(attention_sinks=False)).state_dict(), GPT(tiny()).state_dict()
    new = [k for k in on if k not in off]
    assert new == [f"layers.{i}.attention.sinks" for i in range(2)]
    assert [k for k in on if k in off] == list(off)
    for k in new:
        assert on[k].shape == (4,) and on[k].dtype == torch.float32 and not on[k].any()
    assert list(off) == list(GPT(GPTConfig(**{k: v for k, v in TINY.items() if k != "attention_sinks"})).state_dict())
    assert not hasattr(GPT(tiny(attention_sinks=False)).layers[0].attention, "sinks")


# ------------------------------------------------------------------ eager model
def _rot(x, cos, sin):
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def _autograd_loss(m, ids, seed=0, micro=0, sep=None, p_attn=0.0, p_hidden=0.0):
    """The sink model as an independent dense formula over ``m``'s parameters (plain autograd): a
    softmax over S + 1 columns, the sink column dropped before dropout, with the engine's
    counter-hash dropout masks, the dense document mask and the layers' windows."""
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
        at = layer.attention
        n1 = norm(x, layer.input_layernorm.weight)
        q = (n1 @ at.q_proj.weight.t()).view(B, S, nh, hd).transpose(1, 2)
        k = (n1 @ at.k_proj.weight.t()).view(B, S, nkv, hd).transpose(1, 2)
        v = (n1 @ at.v_proj.weight.t()).view(B, S, nkv, hd).transpose(1, 2)
        if cfg.qk_norm:
            q, k = norm(q, at.q_norm.weight), norm(k, at.k_norm.weight)
        q, k = _rot(q, cos, sin), _rot(k, cos, sin)
        idx = torch.arange(nh) // (nh // nkv)
        allowed = causal
        W = cfg.layer_window(i)
        if W is not None:
            allowed = allowed & (pos.view(1, 1, 1, S) > pos.view(1, 1, S, 1) - W)
        s = ((q @ k[:, idx].transpose(-2, -1)) / math.sqrt(hd)).masked_fill(~allowed, float("-inf"))
        # one more column per query head: not scaled, indexed by the QUERY head, no value row
        col = at.sinks.view(1, nh, 1, 1).expand(B, nh, S, 1)
        pr = torch.softmax(torch.cat([s, col], dim=-1), dim=-1)[..., :S]
        if p_attn > 0:
            pr = pr * rng.attn_keep_mask(B * nh, S, S, k_attn, p_attn).view(B, nh, S, S) / (1.0 - p_attn)
        a = (pr @ v[:, idx]).transpose(1, 2).reshape(B * S, H) @ at.o_proj.weight.t()
        x = x + drop(a, k_resid, p_hidden)
        n2 = norm(x, layer.post_attention_layernorm.weight)
        mlp = layer.mlp
        d = (F.silu(n2 @ mlp.gate_proj.weight.t()) * (n2 @ mlp.up_proj.weight.t())) @ mlp.down_proj.weight.t()
        x = x + drop(d, k_mlp, p_hidden)
    logits = norm(x, m.norm.weight) @ m.embed_tokens.weight.t()
    return F.cross_entropy(logits, shift_targets(ids), ignore_index=-100)


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("kw", [{}, {"num_kv_heads": 2}, {"num_kv_heads": 1, "qk_norm": True, "sliding_window": 5,
                                                           "sliding_window_pattern": 2}])
def test_eager_model_matches_the_dense_formula(kw, flash):
    torch.manual_seed(0)
    m = _randomise_sinks(GPT(tiny(use_flash_attention=flash, **kw)))
    m2 = copy.deepcopy(m)
    ids = torch.randint(0, 256, (3, 32))
    _, l1 = m(ids, labels=ids)
    l1.backward()
    l2 = _autograd_loss(m2, ids)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n
    assert m.layers[0].attention.sinks.grad.abs().max() > 0
    # the sink is live: the same weights without it give another loss
    off = GPT(tiny(use_flash_attention=flash, attention_sinks=False, **kw))
    off.load_state_dict(m.state_dict(), strict=False)
    assert abs(off(ids, labels=ids)[1].item() - l1.item()) > 1e-3


# ------------------------------------------------------------------ reference ops
def _dense_sink_attention(q, k, v, sink, keep, p, doc, window):
    """fp64 autograd formula: softmax over S + 1 columns, the sink's dropped, dropout on the rest."""
    B, nh, S, hd = q.shape
    G = nh // k.shape[1]
    pos = torch.arange(S)
    allowed = (pos.view(1, 1, 1, S) <= pos.view(1, 1, S, 1)).expand(B, 1, S, S)
    if doc is not None:
        allowed = allowed & (pos.view(1, 1, 1, S) >= doc[0].view(B, 1, S, 1))
    if window is not None:
        allowed = allowed & (pos.view(1, 1, 1, S) > pos.view(1, 1, S, 1) - window)
    s = (q @ k.repeat_interleave(G, 1).transpose(-1, -2)) / math.sqrt(hd)
    s = s.masked_fill(~allowed, float("-inf"))
    col = sink.view(1, nh, 1, 1).expand(B, nh, S, 1)
    full = torch.softmax(torch.cat([s, col], -1), -1)
    pr = full[..., :S]
    if p > 0:
        pr = pr * keep / (1.0 - p)
    o = (pr @ v.repeat_interleave(G, 1)).transpose(1, 2).reshape(B * S, nh * hd)
    return o, torch.logsumexp(torch.cat([s, col], -1), -1)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mask", ["plain", "w1", "w37", "w200", "doc"])
@pytest.mark.parametrize("nkv", [4, 2, 1])
def test_reference_ops_match_fp64_autograd(nkv, mask, p):
    B, S, nh, hd, key = 2, 200, 4, 16, 77
    g = torch.Generator().manual_seed(nkv * 10 + len(mask))
    q, k, v = (torch.randn(B, h, S, hd, generator=g, dtype=torch.float64) for h in (nh, nkv, nkv))
    do = torch.randn(B * S, nh * hd, generator=g, dtype=torch.float64)
    sink = torch.tensor([-1.0, 0.5, 3.0, float("-inf")])
    window = int(mask[1:]) if mask[0] == "w" else None
    doc = None
    if mask == "doc":
        ids = torch.ones(B, S, dtype=torch.long)
        ids[0, [12, 29, 90, 91, 181]] = SEP
        ids[1, 150] = SEP
        doc = ref.doc_bounds(ids, SEP)
    keep = rng.attn_keep_mask(B * nh, S, S, key, p).view(B, nh, S, S).double() if p > 0 else None
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    sa = sink.double().clone().requires_grad_(True)
    o_want, lse_want = _dense_sink_attention(qa, ka, va, sa, keep, p, doc, window)
    (o_want * do).sum().backward()

    o, lse = ref.attention_fwd(q.float(), k.float(), v.float(), p, key, True, doc=doc, window=window, sink=sink)
    assert lse.dtype == torch.float32
    assert torch.allclose(o.double(), o_want, atol=2e-5, rtol=1e-4) and torch.allclose(lse.double(), lse_want, atol=2e-5)
    dsink = torch.zeros(nh)
    dq, dk, dv = ref.attention_bwd(q.float(), k.float(), v.float(), o, do.float(), lse, p, key, True, doc=doc,
                                   window=window, sink=sink, dsink=dsink)
    for got, want in ((dq, qa.grad), (dk, ka.grad), (dv, va.grad)):
        assert torch.allclose(got.double(), want, atol=5e-5, rtol=1e-3)
    assert torch.allclose(dsink.double(), sa.grad, atol=5e-5, rtol=1e-3) and dsink[3] == 0 and dsink[:3].abs().min() > 0
    # += : a second call on top of the first adds the same sum again
    ref.attention_bwd(q.float(), k.float(), v.float(), o, do.float(), lse, p, key, True, doc=doc, window=window,
                      sink=sink, dsink=dsink)
    assert torch.allclose(dsink.double(), 2 * sa.grad, atol=1e-4, rtol=1e-3)
    # the packed forms are the same ops on q | k | v rows
    qkv = torch.cat([t.float().transpose(1, 2).reshape(B * S, -1) for t in (q, k, v)], 1).contiguous()
    o2, lse2 = ref.attention_fwd_packed(qkv, B, S, nh, p, key, doc=doc, nkv=nkv, window=window, sink=sink)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    cos, sin = ref.rope_tables(hd, S)
    d2 = torch.zeros(nh)
    g2 = ref.attention_bwd_packed(qkv, o, do.float(), lse, p, key, B, S, nh, cos, sin, doc=doc, nkv=nkv, window=window,
                                  sink=sink, dsink=d2)
    assert g2.shape == qkv.shape and torch.allclose(d2.double(), sa.grad, atol=5e-5, rtol=1e-3)


def test_reference_ops_validate_the_sink():
    q = torch.randn(1, 4, 8, 16)
    with pytest.raises(ValueError, match="sink"):
        ref.attention_fwd(q, q, q, 0.0, 0, True, sink=torch.zeros(3))
    o, lse = ref.attention_fwd(q, q, q, 0.0, 0, True, sink=torch.zeros(4))
    with pytest.raises(ValueError, match="together"):
        ref.attention_bwd(q, q, q, o, o, lse, 0.0, 0, True, sink=torch.zeros(4))
    with pytest.raises(ValueError, match="fp32"):
        ref.attention_bwd(q, q, q, o, o, lse, 0.0, 0, True, sink=torch.zeros(4), dsink=torch.zeros(4, dtype=torch.float64))
    # without the argument the ops are what they were
    o0, lse0 = ref.attention_fwd(q, q, q, 0.0, 0, True)
    o1, lse1 = ref.attention_fwd(q, q, q, 0.0, 0, True, sink=torch.full((4,), float("-inf")))
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)


# ------------------------------------------------------------------ engine on the reference ops
COMBOS = [({}, None), ({"num_kv_heads": 2}, None),
          ({"num_kv_heads": 2, "qk_norm": True, "sliding_window": 5, "sliding_window_pattern": 2}, SEP)]


@pytest.mark.parametrize("recompute,selective", [(False, True), (True, True), (True, False)])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("kw,sep", COMBOS)
def test_engine_matches_autograd_with_the_same_dropout_masks(recompute, selective, packed, kw, sep):
    torch.manual_seed(3)
    m1 = _randomise_sinks(GPT(tiny(dropout=0.1, attention_dropout=0.1, **kw)))
    m2 = copy.deepcopy(m1)
    ids = torch.randint(1, 256, (3, 32))
    if sep is not None:
        ids[0, [4, 5, 19]] = sep
        ids[2, 31] = sep
    l1 = _autograd_loss(m1, ids, seed=21, micro=0, sep=sep, p_attn=0.1, p_hidden=0.1)
    l1.backward()
    m2.set_doc_separator(sep)
    eng = m2.enable_engine(seed=21)
    assert eng.sinks and eng.provider.layer(0).sk.shape == (4,) and eng.provider.layer_grads(1).sk.dtype == torch.float32
    eng.packed_qkv = packed and eng.packed_qkv
    eng.selective_recompute = selective
    m2.gradient_checkpointing = recompute
    m2.train()
    _, l2 = m2(ids, labels=ids)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n
    assert m2.layers[1].attention.sinks.grad.abs().min() > 0


@pytest.mark.parametrize("recompute", [False, True])
def test_train_window_matches_sequential_bit_for_bit(recompute):
    torch.manual_seed(5)
    GA = 2
    m1 = _randomise_sinks(GPT(tiny(num_kv_heads=2, dropout=0.1, attention_dropout=0.1)))
    m2 = copy.deepcopy(m1)
    e1, e2 = m1.enable_engine(seed=5), m2.enable_engine(seed=5)
    m1.gradient_checkpointing = m2.gradient_checkpointing = recompute
    m1.train()
    m2.train()
    data = [torch.randint(0, 256, (2, 32)) for _ in range(GA)]
    seq = []
    for j in range(GA):
        e1.set_accumulation(j, GA, defer=True)
        _, loss = m1(data[j], labels=data[j])
        (loss / GA).backward()
        seq.append(loss.detach())
    win = e2.train_window(data, [shift_targets(d) for d in data], torch.full((), 1.0 / GA), recompute=recompute)
    for a, b in zip(seq, win):
        assert torch.equal(a, b)
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p1.grad, p2.grad), n


def test_engine_sink_gradient_by_finite_differences():
    torch.manual_seed(7)
    # weights ten times the default range: scores and values of order 1, so that the sinks carry a
    # gradient well above the fp32 loss's noise
    m = _randomise_sinks(GPT(tiny(num_kv_heads=2, initializer_range=0.2)))
    m.enable_engine()
    ids = torch.randint(0, 256, (3, 32))
    m.train()
    _, loss = m(ids, labels=ids)
    loss.backward()
    for i in range(2):
        w = m.layers[i].attention.sinks
        g = w.grad.clone()
        d = g / g.norm()  # along the gradient: the largest signal
        h = 0.2
        ls = []
        for sgn in (1.0, -1.0):
            with torch.no_grad():
                w.add_(sgn * h * d)
                ls.append(m.eval_loss(ids).item())
                w.sub_(sgn * h * d)
        fd = (ls[0] - ls[1]) / (2 * h)
        # central difference: O(h^2) truncation (h^2 / 6 of the slope for a third derivative of
        # its size: under 1 %, charged 2 %) + the fp32 loss's own error, a few tens of ulps of a
        # value under 16 (2^-20), over 2h
        tol = 2e-2 * abs(fd) + 40 * 2.0 ** -20 / (2 * h)
        assert abs(fd - g.norm().item()) <= tol, (i, fd, g.norm().item(), tol)
        assert g.norm().item() > 10 * 40 * 2.0 ** -20 / (2 * h), "signal under the noise floor"


# ------------------------------------------------------------------ flat layout, optimizer groups
def test_flat_layout_keeps_every_later_segment_aligned():
    from distributed_llm_trainer_amd.parallel.flat import FlatLayout, sinks_alloc
    cfg = GPTConfig(vocab_size=256, hidden_size=25 * 8, num_layers=3, num_heads=25, max_seq_len=16, attention_sinks=True,
                    qk_norm=True)
    lay = FlatLayout(cfg)
    assert sinks_alloc(25) == 32 and sinks_alloc(12) == 16 and sinks_alloc(8) == 8
    names = [s.name for s in lay.segments]
    for i in range(3):
        at = names.index(f"layers.{i}.attention.sinks")
        assert names[at - 3:at] == [f"layers.{i}.post_attention_layernorm.weight", f"layers.{i}.attention.q_norm.weight",
                                    f"layers.{i}.attention.k_norm.weight"]
        s = lay.by_name[names[at]]
        assert s.numel == 25 and s.shape == (25,) and lay.segments[at + 1].offset == s.offset + 32
    first = lay.by_name["layers.0.attention.sinks"].offset
    for s in lay.segments:
        if s.offset > first:
            assert s.offset % 4 == 0, s.name  # 16 bytes in the fp32 buffers ...
            assert s.offset % 8 == 0, s.name  # ... and in the bf16 shadow
    off = FlatLayout(GPTConfig(vocab_size=256, hidden_size=200, num_layers=3, num_heads=25, max_seq_len=16, qk_norm=True))
    assert lay.total == off.total + 3 * 32 and lay.decay_end == off.decay_end
    assert [s.name for s in off.segments] == [n for n in names if not n.endswith("sinks")]


def test_sinks_are_in_the_no_decay_group_and_their_padding_stays_zero():
    from distributed_llm_trainer_amd.training.optim import flat_store_optimizer
    cfg = GPTConfig(vocab_size=256, hidden_size=48, num_layers=2, num_heads=6, max_seq_len=16, dropout=0.0,
                    attention_dropout=0.0, attention_sinks=True)
    m = GPT(cfg)
    m.enable_engine()
    opt = flat_store_optimizer(m.store, 1e-2, (0.9, 0.95), 1e-8, 0.1)
    lay = m.store.layout
    (a0, b0, wd0), (a1, b1, wd1) = opt.regions
    assert wd0 == 0.1 and wd1 == 0.0 and b1 == lay.total
    for i in range(2):
        s = lay.by_name[f"layers.{i}.attention.sinks"]
        assert a1 <= s.offset and s.offset + 8 <= b1
    nd_names = [n for n, *_ in opt.param_map[1]]
    assert "layers.1.attention.sinks" in nd_names and not any("sinks" in n for n, *_ in opt.param_map[0])
    # the lazy optimizer's units cover the buffer exactly once, the sinks and their padding in their layer's unit
    spans = sorted(r for u in m.store.unit_ranges().values() for r in u)
    assert spans[0][0] == 0 and spans[-1][1] == lay.total
    assert all(spans[j][1] == spans[j + 1][0] for j in range(len(spans) - 1))
    s1 = lay.by_name["layers.1.attention.sinks"]
    assert m.store.unit_ranges()[1][1][1] == s1.offset + 8
    ids = torch.randint(0, 256, (2, 16))
    m.train()
    for _ in range(3):
        _, loss = m(ids, labels=ids)
        loss.backward()
        opt.step()
        opt.zero_grad()
    m.store.flush_pending()
    for i in range(2):
        s = lay.by_name[f"layers.{i}.attention.sinks"]
        assert m.store.flat[s.offset:s.offset + 6].abs().min() > 0, "the sinks did not move from zero"
        assert not m.store.flat[s.offset + 6:s.offset + 8].any(), "the padding moved"
        assert torch.equal(m.layers[i].attention.sinks.data, m.store.flat[s.offset:s.offset + 6])


# ------------------------------------------------------------------ distributed
DIST = dict(vocab_size=384, hidden_size=96, num_layers=2, num_heads=6, num_kv_heads=2, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0, attention_sinks=True)


def _data(step, rank, n=8, seq=32, vocab=384):
    g = torch.Generator().manual_seed(1000 * step + rank)
    return torch.randint(0, vocab, (n, seq), generator=g)


def _ddp_trainer(GA):
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=GA, warmup_steps=1, max_steps=100,
                        learning_rate=1e-2, bucket_cap_mb=0.05, micro_step_fusion=1)
    return DistributedTrainer(GPTConfig(**DIST), tc)


def _ddp_worker(rank, world, steps):
    tr = _ddp_trainer(2)
    for s in range(steps):
        tr.train_step({"input_ids": _data(s, rank, n=4)})
    lay = tr.model.store.layout
    head = [b for b in tr.ddp.buckets if b[0] == lay.embed_offset][0]
    return tr.flat_params().clone(), head, lay.total


def test_ddp_matches_single_process():
    (p0, head, total), (p1, _, _) = run_multiprocess(_ddp_worker, world=2, args=(3,))
    assert torch.equal(p0, p1), "ranks diverged"
    assert head[1] == total  # the bucket of the embedding and the norm weights carries the sinks
    tr = _ddp_trainer(4)
    for s in range(3):
        tr.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    ref_p = tr.flat_params()
    cfg = GPTConfig(**DIST)
    assert p0.numel() == cfg.num_parameters() + (cfg.vocab_size_padded - 384) * 96 + 2 * 2  # + the sinks' padding
    assert torch.allclose(p0, ref_p, atol=2e-5, rtol=1e-4), (p0 - ref_p).abs().max()
    s = tr.model.store.layout.by_name["layers.0.attention.sinks"]
    assert p0[s.offset:s.offset + 6].abs().min() > 0, "the sinks never trained"
    assert not p0[s.offset + 6:s.offset + 8].any()


def _fsdp_trainer(GA, ac, reduce_dtype="fp32"):
    from distributed_llm_trainer_amd.training.configs import FSDPConfig, FSDPTrainingConfig
    from distributed_llm_trainer_amd.training.fsdp_trainer import FSDPTrainer
    tc = FSDPTrainingConfig(batch_size=2, gradient_accumulation_steps=GA, warmup_steps=1, max_steps=100,
                            learning_rate=1e-2, micro_step_fusion=1)
    fc = FSDPConfig(sharding_strategy="FULL_SHARD", activation_checkpointing=ac, reduce_dtype=reduce_dtype)
    return FSDPTrainer(GPTConfig(**DIST), tc, fc)


def _fsdp_worker(rank, world, steps):
    tr = _fsdp_trainer(2, True)
    for s in range(steps):
        tr.train_step({"input_ids": _data(s, rank, n=4)})
    return {k: v for k, v in tr._full_state().items() if "rotary" not in k}


def test_fsdp_full_shard_matches_single_process():
    outs = run_multiprocess(_fsdp_worker, world=2, args=(3,))
    tr = _fsdp_trainer(4, False)
    for s in range(3):
        tr.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    ref_sd = {k: v for k, v in tr._full_state().items() if "rotary" not in k}
    assert ref_sd["layers.1.attention.sinks"].shape == (6,) and ref_sd["layers.1.attention.sinks"].abs().min() > 0
    u = tr.runtime.units[0]
    assert u.segs[-1].name == "layers.0.attention.sinks" and u.numel == u.segs[-1].offset + 8
    for k in ref_sd:
        assert torch.equal(outs[0][k], outs[1][k]), f"{k}: ranks diverged"
        assert torch.allclose(outs[0][k], ref_sd[k], atol=3e-5, rtol=1e-4), (k, (outs[0][k] - ref_sd[k]).abs().max())


# ------------------------------------------------------------------ checkpoints
def test_full_checkpoint_round_trip_and_generate(tmp_path):
    from distributed_llm_trainer_amd.eval.infer import load_model
    tr = _ddp_trainer(1)
    for s in range(2):  # the first step is the warm-up step: its learning rate is 0
        tr.train_step({"input_ids": _data(s, 0, n=2)})
    path = str(tmp_path / "sk.pt")
    tr.save_checkpoint(path)
    want = tr.flat_params().clone()
    tr2 = _ddp_trainer(1)
    tr2.load_checkpoint(path)
    assert torch.equal(tr2.flat_params(), want)
    back = load_model(path)
    assert back.config.attention_sinks and back.config == tr.model.config
    sd = tr.model.state_dict()
    assert sd["layers.0.attention.sinks"].abs().min() > 0
    for k, v in back.state_dict().items():
        assert torch.equal(v, sd[k].cpu()), k
    ids = torch.randint(0, 384, (1, 5))
    assert back.generate(ids, max_new_tokens=4, top_k=1).shape == (1, 9)
    # the flag overrides a stored config that does not carry it
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    ck = load_checkpoint(path, map_location="cpu")
    ck["model_config"] = GPTConfig.from_dict({**tr.model.config.to_dict(), "attention_sinks": False})
    save_checkpoint(path, ck)
    assert load_model(path, attention_sinks=True).config.attention_sinks


def test_sharded_checkpoint_round_trip(tmp_path):
    from distributed_llm_trainer_amd.utils.checkpoint import consolidate_sharded
    tr = _fsdp_trainer(1, False)
    for s in range(2):  # the first step is the warm-up step: its learning rate is 0
        tr.train_step({"input_ids": _data(s, 0, n=2)})
    want = {k: v.clone() for k, v in tr._full_state().items()}
    d = str(tmp_path / "sharded")
    tr.save_sharded_checkpoint(d)
    tr2 = _fsdp_trainer(1, False)
    tr2.load_checkpoint(d)
    got = tr2._full_state()
    assert want["layers.0.attention.sinks"].abs().min() > 0
    for k in want:
        assert torch.equal(got[k], want[k]), k
    full = consolidate_sharded(d)
    mc = full["model_config"]
    assert (mc["attention_sinks"] if isinstance(mc, dict) else mc.attention_sinks) is True
    for k in ("layers.0.attention.sinks", "layers.1.attention.sinks"):
        assert full["model"][k].shape == (6,) and torch.equal(full["model"][k], want[k]), k


# ------------------------------------------------------------------ CLI
def _yaml(tmp_path, val):
    p = tmp_path / "m.yaml"
    extra = f"  attention_sinks: {val}\n" if val is not None else ""
    p.write_text("model:\n  hidden_size: 64\n  num_layers: 1\n  num_heads: 4\n  vocab_size: 128\n"
                 "  max_seq_len: 16\n" + extra)
    return str(p)


@pytest.mark.parametrize("trainer", ["ddp_trainer", "fsdp_trainer"])
def test_cli_flag_precedence(tmp_path, trainer):
    """CLI > YAML > preset."""
    import importlib
    mod = importlib.import_module(f"distributed_llm_trainer_amd.training.{trainer}")
    from distributed_llm_trainer_amd.training.common import apply_model_args
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.utils.config_loader import load_yaml_config
    parser = mod.build_parser()
    assert parser.parse_args([]).attention_sinks is None

    def resolve(argv, yaml_val="absent"):
        args = parser.parse_args(argv)
        cfg = GPTConfig.from_preset("small")
        if yaml_val != "absent":
            cfg = load_yaml_config(_yaml(tmp_path, yaml_val), cfg, TrainingConfig(), None)[0]
        apply_model_args(args, cfg)
        return cfg

    assert resolve([]).attention_sinks is False                              # preset
    assert resolve(["--attention_sinks"]).attention_sinks is True            # CLI over the preset
    assert resolve([], None).attention_sinks is False                        # YAML without the key
    assert resolve([], "true").attention_sinks is True                       # YAML over the preset
    assert resolve(["--attention_sinks"], "false").attention_sinks is True   # CLI over YAML
    assert resolve(["--attention_sinks"], "false").num_parameters() == resolve([], "false").num_parameters() + 4
    both = resolve(["--attention_sinks", "--num_kv_heads", "2", "--qk_norm", "--sliding_window", "8"])
    assert both.attention_sinks and both.num_kv_heads == 2 and both.qk_norm and both.sliding_window == 8


def test_cli_trains_and_infers_a_model_with_sinks(tmp_path):
    """--attention_sinks reaches the trainer's model and its checkpoint, and infer.py reads it back."""
    from distributed_llm_trainer_amd.eval.infer import load_model
    from distributed_llm_trainer_amd.training import ddp_trainer
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint
    env_before = os.environ.get("DLT_DUMMY_BATCHES")
    os.environ["DLT_DUMMY_BATCHES"] = "2"
    try:
        ddp_trainer.main(["--config", _yaml(tmp_path, None), "--attention_sinks", "--doc_sep_token", "3", "--batch_size",
                          "1", "--max_steps", "1", "--gradient_accumulation_steps", "1", "--checkpoint_dir",
                          str(tmp_path / "ck")])
    finally:
        if env_before is None:
            os.environ.pop("DLT_DUMMY_BATCHES", None)
        else:
            os.environ["DLT_DUMMY_BATCHES"] = env_before
    ck = load_checkpoint(str(tmp_path / "ck" / "final.pt"), map_location="cpu")
    assert ck["model_config"].attention_sinks is True
    assert any(k.endswith("layers.0.attention.sinks") for k in ck["model"])
    m = load_model(str(tmp_path / "ck" / "final.pt"))
    assert m.config.attention_sinks and m.layers[0].attention.sinks.shape == (4,)


# ------------------------------------------------------------------ generation
@pytest.mark.parametrize("kw", [{}, {"num_kv_heads": 2}, {"num_kv_heads": 2, "sliding_window": 4}])
def test_kv_cached_generate_matches_greedy_full_forward(kw):
    torch.manual_seed(5)
    m1 = _randomise_sinks(GPT(tiny(**kw)))
    m2 = copy.deepcopy(m1)
    m2.enable_engine()
    ids = torch.randint(0, 256, (1, 5))
    o1 = m1.generate(ids, max_new_tokens=8, temperature=1.0, top_k=1)  # greedy full re-forward
    o2 = m2.generate(ids, max_new_tokens=8, temperature=1.0, top_k=1)
    assert o1.shape == (1, 13)
    assert torch.equal(o1, o2)
    # the sink is live in the cached path: without it the logits differ
    from distributed_llm_trainer_amd.eval.decode import KVCache, forward_cached
    lg = forward_cached(m2, ids, KVCache(m2.config, 1, "cpu", m2.engine.act_dtype))
    with torch.no_grad():
        for layer in m2.layers:
            layer.attention.sinks.fill_(float("-inf"))
    lg1 = forward_cached(m2, ids, KVCache(m2.config, 1, "cpu", m2.engine.act_dtype))
    assert (lg - lg1).abs().max().item() > 1e-4
