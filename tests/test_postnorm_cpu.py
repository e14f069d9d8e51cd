"""Post-norms (``GPTConfig.post_norm``: a second RMSNorm on each branch output, the Gemma-2/3
sandwich block) on the CPU: the kernels' fp64 references and planted defects
(tests/postnorm_ref.py), config, eager model, the engine on the reference ops, the flat store,
optimizer groups, DDP / FSDP over gloo, checkpoints, the CLI flag and KV-cached generation."""
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
from tests import postnorm_ref as R
from tests.dist_utils import run_multiprocess

SEP = 0
TINY = dict(vocab_size=256, hidden_size=64, num_layers=2, num_heads=4, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0, post_norm=True)
DTYPES = [torch.bfloat16, torch.float16]
POST = ("attn_post_norm", "mlp_post_norm")


def tiny(**kw):
    d = dict(TINY)
    d.update(kw)
    return GPTConfig(**d)


def _randomise_norms(m, seed=0):
    """Non-unit post-norm weights (the init is ones, which hides a swapped or missing weight), and
    non-unit pre-norm weights so that ln2 and attn_post_norm differ."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in m.layers:
            mods = [layer.input_layernorm, layer.post_attention_layernorm]
            mods += [getattr(layer, n) for n in POST if hasattr(layer, n)]
            at = layer.attention
            mods += [at.q_norm, at.k_norm] if getattr(at, "qk_norm", False) else []
            for n in mods:
                n.weight.copy_(1.0 + 0.5 * torch.randn(n.weight.shape, generator=g))
    return m


# ------------------------------------------------------------------ kernels: references, models, defects
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", R.HS)
def test_fp32_models_of_the_kernels_are_inside_the_tolerance(H, dtype):
    inp = R.make_inputs(H, dtype)
    assert (inp.a[R.ZERO_ROW] == 0).all() and inp.a[R.BIG_ROW].float().abs().max() > 1e3
    assert torch.isfinite(inp.a.float()).all()
    assert (inp.w == 0).sum() == 2 and (inp.w < 0).sum() >= 2
    assert R.worst(R.fwd_model(inp), R.fwd_ref(inp)) <= 1.0
    da, dw = R.bwd_model(inp)
    b = R.bwd_ref(inp)
    assert R.worst(da, b.da) <= 1.0 and R.worst(dw, b.dw) <= 1.0
    for p in (0.0, 0.1):
        x, y, rstd = R.fused_model(inp, p)
        f = R.fused_ref(inp, p)
        assert R.worst(x, f.x) <= 1.0 and R.worst(y, f.y) <= 1.0 and R.worst(rstd, f.rstd) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("defect", R.DEFECTS_FWD)
def test_planted_forward_defects_are_outside_the_tolerance(defect, H, dtype):
    inp = R.make_inputs(H, dtype)
    assert R.worst(R.fwd_model(inp, defect=defect), R.fwd_ref(inp)) > 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("defect", R.DEFECTS_FUSED)
def test_planted_fused_forward_defects_are_outside_the_tolerance(defect, H, dtype):
    inp = R.make_inputs(H, dtype)
    x, y, rstd = R.fused_model(inp, 0.1, defect=defect)
    assert R.worst(x, R.fused_ref(inp, 0.1).x) > 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("defect", R.DEFECTS_BWD)
def test_planted_backward_defects_are_outside_the_tolerance(defect, H, dtype):
    inp = R.make_inputs(H, dtype)
    da, dw = R.bwd_model(inp, defect=defect)
    b = R.bwd_ref(inp)
    assert R.worst(da, b.da) > 1.0
    if defect == "neighbour_row_rstd":  # xh itself is wrong: the weight gradient leaves its bound too
        assert R.worst(dw, b.dw) > 1.0


@pytest.mark.parametrize("dtype", [torch.float32] + DTYPES)
@pytest.mark.parametrize("H", [64, 1000])
def test_reference_ops_are_the_kernels_contract(H, dtype):
    """ops/reference.py rounds where the kernels do: the 16-bit results are inside the fp64
    tolerance and the fused op equals the two-op sequence bit for bit; in fp32 they match autograd."""
    act = torch.bfloat16 if dtype == torch.float32 else dtype
    inp = R.make_inputs(H, act)
    a, du = inp.a.to(dtype), inp.du.to(dtype)
    u = ref.postnorm_fwd(a, inp.w, R.EPS)
    assert u.dtype == dtype and u.data_ptr() != a.data_ptr()
    out = torch.empty_like(a)
    assert ref.postnorm_fwd(a, inp.w, R.EPS, out=out) is out and torch.equal(out, u)
    dw = torch.zeros(H)
    g = du.clone()
    assert ref.postnorm_bwd(g, a, inp.w, R.EPS, dw) is g
    for p in (0.0, 0.1):
        got = ref.postnorm_add_dropout_rmsnorm_fwd(inp.resid, a, inp.w, inp.w2, R.EPS, p, R.KEY, dtype)
        want = ref.add_dropout_rmsnorm_fwd(inp.resid, u, inp.w2, R.EPS, p, R.KEY, dtype)
        for x, y in zip(got, want):
            assert torch.equal(x, y)
        if dtype != torch.float32:
            f = R.fused_ref(inp, p)
            assert R.worst(got[0], f.x) <= 1.0 and R.worst(got[1], f.y) <= 1.0 and R.worst(got[2], f.rstd) <= 1.0
    if dtype != torch.float32:
        b = R.bwd_ref(inp)
        assert R.worst(u, R.fwd_ref(inp)) <= 1.0
        assert R.worst(g, b.da) <= 1.0 and R.worst(dw, b.dw) <= 1.0
        dw2 = dw.clone()
        ref.postnorm_bwd(du.clone(), a, inp.w, R.EPS, dw2)
        assert torch.equal(dw2, 2 * dw)
        return
    x = a.clone().requires_grad_(True)
    w = inp.w.clone().requires_grad_(True)
    (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + R.EPS) * w).backward(du)
    keep = torch.ones(a.shape[0], dtype=torch.bool)
    keep[R.BIG_ROW] = False  # its fp32 sums of squares lose bits autograd loses elsewhere
    assert torch.allclose(g[keep], x.grad[keep], atol=1e-4, rtol=1e-4)
    assert torch.allclose(dw, w.grad, atol=1e-3, rtol=1e-4)


# ------------------------------------------------------------------ config
OLD_FIELDS = ["vocab_size", "hidden_size", "num_layers", "num_heads", "intermediate_size", "max_seq_len", "dropout",
              "attention_dropout", "initializer_range", "activation", "use_flash_attention", "gradient_checkpointing"]


def test_config_without_the_flag_serialises_as_before():
    cfg = GPTConfig.gpt2_small()
    assert cfg.post_norm is False
    assert list(cfg.to_dict()) == OLD_FIELDS and list(cfg.__getstate__()) == OLD_FIELDS
    assert cfg.to_dict() == GPTConfig(post_norm=False).to_dict()
    assert pickle.dumps(cfg) == pickle.dumps(GPTConfig(post_norm=False))
    assert GPTConfig.from_dict(cfg.to_dict()) == cfg
    on = tiny()
    assert on.to_dict()["post_norm"] is True and GPTConfig.from_dict(on.to_dict()) == on
    assert list(on.to_dict()) == OLD_FIELDS + ["post_norm"]
    assert pickle.loads(pickle.dumps(on)).post_norm is True and pickle.loads(pickle.dumps(cfg)).post_norm is False
    assert pickle.loads(pickle.dumps(on)) == on


def test_config_validation():
    with pytest.raises(ValueError, match="post_norm"):
        GPTConfig(post_norm="yes")
    with pytest.raises(ValueError, match="post_norm"):
        GPTConfig(post_norm=2)
    assert GPTConfig(post_norm=1).post_norm is True and GPTConfig(post_norm=0).post_norm is False


def test_an_old_pickle_loads_without_post_norm():
    state = {k: v for k, v in GPTConfig.gpt2_small().__dict__.items()
             if k not in ("post_norm", "attention_sinks", "qk_norm", "num_kv_heads")}
    old = GPTConfig.__new__(GPTConfig)
    old.__setstate__(state)
    assert old.post_norm is False and old == GPTConfig.gpt2_small()
    assert "post_norm" not in " ".join(GPT(tiny(post_norm=False)).state_dict())


@pytest.mark.parametrize("kw", [{}, {"num_kv_heads": 2, "qk_norm": True, "attention_sinks": True}])
def test_num_parameters_counts_the_two_vectors(kw):
    cfg = tiny(**kw)
    assert cfg.num_parameters() == count_parameters(GPT(cfg))
    assert cfg.num_parameters() - tiny(post_norm=False, **kw).num_parameters() == 2 * 2 * 64


def test_state_dict_keys_and_init():
    off, on = GPT(tiny(post_norm=False)).state_dict(), GPT(tiny()).state_dict()
    new = [k for k in on if k not in off]
    assert new == [f"layers.{i}.{n}.weight" for i in range(2) for n in POST]
    assert [k for k in on if k in off] == list(off)
    for k in new:
        assert on[k].shape == (64,) and torch.equal(on[k], torch.ones(64))
    blk = GPT(tiny()).layers[0]
    assert blk.attn_post_norm.eps == blk.mlp_post_norm.eps == blk.post_attention_layernorm.eps == GPT(tiny()).norm.eps


def test_flag_off_keeps_the_key_list_and_flat_layout():
    from distributed_llm_trainer_amd.parallel.flat import FlatLayout
    cfg = tiny(post_norm=False)
    assert list(GPT(cfg).state_dict()) == list(GPT(GPTConfig(**{k: v for k, v in TINY.items() if k != "post_norm"})).state_dict())
    assert not hasattr(GPT(cfg).layers[0], "attn_post_norm")
    names = [s.name for s in FlatLayout(cfg).segments]
    H, I, L = 64, 256, 2
    want = []
    for i in range(L):
        want += [f"layers.{i}.attention.{n}_proj.weight" for n in "qkvo"]
        want += [f"layers.{i}.mlp.{n}_proj.weight" for n in ("gate", "up", "down")]
    want += ["embed_tokens.weight"]
    for i in range(L):
        want += [f"layers.{i}.input_layernorm.weight", f"layers.{i}.post_attention_layernorm.weight"]
    want += ["norm.weight"]
    assert names == want
    lay = FlatLayout(cfg)
    assert lay.total == L * (4 * H * H + 3 * H * I) + 256 * H + (2 * L + 1) * H


@pytest.mark.parametrize("nh", [4, 5])
def test_flat_layout_offsets_and_alignment(nh):
    """The two vectors are the tail of the layer's no-decay segment, after ln1 | ln2 | q_norm | k_norm |
    sinks + padding; no earlier offset moves and every later segment stays 16-byte aligned."""
    from distributed_llm_trainer_amd.parallel.flat import FlatLayout, sinks_alloc
    kw = dict(hidden_size=16 * nh, num_heads=nh, num_layers=3, qk_norm=True, attention_sinks=True)
    on, off = FlatLayout(tiny(**kw)), FlatLayout(tiny(post_norm=False, **kw))
    H = 16 * nh
    assert on.total == off.total + 3 * 2 * H and on.decay_end == off.decay_end
    for i in range(3):
        sk = on.by_name[f"layers.{i}.attention.sinks"]
        p1, p2 = on.by_name[f"layers.{i}.attn_post_norm.weight"], on.by_name[f"layers.{i}.mlp_post_norm.weight"]
        assert p1.offset == sk.offset + sinks_alloc(nh) and p2.offset == p1.offset + H and p1.offset >= on.decay_end
        for s in off.segments:  # the layer's earlier segments keep their place relative to its first norm weight
            if s.name.startswith(f"layers.{i}.") and s.offset >= off.decay_end:
                base_on = on.by_name[f"layers.{i}.input_layernorm.weight"].offset
                base_off = off.by_name[f"layers.{i}.input_layernorm.weight"].offset
                assert on.by_name[s.name].offset - base_on == s.offset - base_off
    for s in off.segments:
        if s.offset < off.decay_end:
            assert on.by_name[s.name].offset == s.offset
    for s in on.segments:
        if s.offset >= on.decay_end:
            assert s.offset % 8 == 0, s.name  # 16 bytes in the bf16 shadow, 32 in the fp32 buffers


# ------------------------------------------------------------------ eager model
def _rot(x, cos, sin):
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def _autograd_loss(m, ids, seed=0, micro=0, sep=None, p_attn=0.0, p_hidden=0.0, dtype=torch.float32):
    """The post-norm model as an independent dense formula over ``m``'s parameters (plain
    autograd, in ``dtype``), with the engine's counter-hash dropout masks and the dense document mask."""
    cfg = m.config
    B, S = ids.shape
    nh, nkv, hd, H = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.hidden_size
    pos = torch.arange(S)
    allowed = (pos.view(1, 1, 1, S) <= pos.view(1, 1, S, 1)).expand(B, 1, S, S)
    if sep is not None:
        lo, _ = ref.doc_bounds(ids, sep)
        allowed = allowed & (pos.view(1, 1, 1, S) >= lo.view(B, 1, S, 1))
    if cfg.sliding_window is not None:
        allowed = allowed & (pos.view(1, 1, 1, S) > pos.view(1, 1, S, 1) - cfg.sliding_window)
    cos, sin = ref.rope_tables(hd, S)
    cos, sin = cos.view(1, 1, S, hd // 2).to(dtype), sin.view(1, 1, S, hd // 2).to(dtype)

    def P(t):
        return t.to(dtype)

    def drop(x, key, p):
        return x * rng.keep_mask(x.shape, key, p) / (1.0 - p) if p > 0 else x

    def norm(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * P(w)

    x = P(m.embed_tokens.weight)[ids.reshape(-1)]
    for i, layer in enumerate(m.layers):
        k_attn, k_resid, k_mlp = (rng.site_key(seed, micro, i, s) for s in (rng.SITE_ATTN, rng.SITE_RESID, rng.SITE_MLP))
        at = layer.attention
        n1 = norm(x, layer.input_layernorm.weight)
        q = (n1 @ P(at.q_proj.weight).t()).view(B, S, nh, hd).transpose(1, 2)
        k = (n1 @ P(at.k_proj.weight).t()).view(B, S, nkv, hd).transpose(1, 2)
        v = (n1 @ P(at.v_proj.weight).t()).view(B, S, nkv, hd).transpose(1, 2)
        if cfg.qk_norm:
            q, k = norm(q, at.q_norm.weight), norm(k, at.k_norm.weight)
        q, k = _rot(q, cos, sin), _rot(k, cos, sin)
        idx = torch.arange(nh) // (nh // nkv)
        s = (q @ k[:, idx].transpose(-2, -1)) / math.sqrt(hd)
        s = s.masked_fill(~allowed, float("-inf"))
        if cfg.attention_sinks:
            sink = P(at.sinks).view(1, nh, 1, 1).expand(B, -1, S, 1)
            pr = torch.softmax(torch.cat([s, sink], dim=-1), dim=-1)[..., :S]
        else:
            pr = torch.softmax(s, dim=-1)
        if p_attn > 0:
            pr = pr * rng.attn_keep_mask(B * nh, S, S, k_attn, p_attn).view(B, nh, S, S) / (1.0 - p_attn)
        a = (pr @ v[:, idx]).transpose(1, 2).reshape(B * S, H) @ P(at.o_proj.weight).t()
        x = x + drop(norm(a, layer.attn_post_norm.weight), k_resid, p_hidden)  # norm, then dropout, then the add
        n2 = norm(x, layer.post_attention_layernorm.weight)
        mlp = layer.mlp
        d = (F.silu(n2 @ P(mlp.gate_proj.weight).t()) * (n2 @ P(mlp.up_proj.weight).t())) @ P(mlp.down_proj.weight).t()
        x = x + drop(norm(d, layer.mlp_post_norm.weight), k_mlp, p_hidden)
    logits = norm(x, m.norm.weight) @ P(m.embed_tokens.weight).t()
    return F.cross_entropy(logits, shift_targets(ids), ignore_index=-100)


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("kw", [{}, {"num_kv_heads": 2, "qk_norm": True, "attention_sinks": True}])
def test_eager_model_matches_fp64_autograd(kw, flash):
    torch.manual_seed(0)
    m = _randomise_norms(GPT(tiny(use_flash_attention=flash, **kw)))
    m2 = copy.deepcopy(m)
    ids = torch.randint(0, 256, (3, 32))
    _, l1 = m(ids, labels=ids)
    l1.backward()
    l2 = _autograd_loss(m2, ids, dtype=torch.float64)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n
    assert m.layers[0].attn_post_norm.weight.grad.abs().max() > 0 and m.layers[1].mlp_post_norm.weight.grad.abs().max() > 0
    # the norms are live: the same weights without them give another loss
    off = GPT(tiny(use_flash_attention=flash, post_norm=False, **kw))
    off.load_state_dict(m.state_dict(), strict=False)
    assert abs(off(ids, labels=ids)[1].item() - l1.item()) > 1e-3


def test_eager_dropout_follows_the_norm_and_the_default_rng_use_is_unchanged():
    """Post-norm model: dropout(norm(branch)).  Default model: the same random numbers as before."""
    torch.manual_seed(1)
    m = _randomise_norms(GPT(tiny(dropout=0.5)))
    m.train()
    blk = m.layers[0]
    x = torch.randn(2, 8, 64)
    torch.manual_seed(7)
    got = blk.mlp(x, post_norm=blk.mlp_post_norm)
    torch.manual_seed(7)
    want = F.dropout(blk.mlp_post_norm(blk.mlp.down_proj(F.silu(blk.mlp.gate_proj(x)) * blk.mlp.up_proj(x))), 0.5, True)
    assert torch.equal(got, want)
    off = GPT(tiny(dropout=0.5, post_norm=False))
    off.train()
    ids = torch.randint(0, 256, (2, 16))
    torch.manual_seed(3)
    l1 = off(ids, labels=ids)[1]
    s1 = torch.get_rng_state()
    torch.manual_seed(3)
    h = off.embed_tokens(ids)
    for layer in off.layers:  # the block as it was written before the flag existed
        h = h + layer.attention(layer.input_layernorm(h), None, None)
        h = h + layer.mlp(layer.post_attention_layernorm(h))
    l2 = F.cross_entropy(off.lm_head(off.norm(h))[:, :-1].reshape(-1, 256), ids[:, 1:].reshape(-1))
    assert torch.equal(l1, l2) and torch.equal(s1, torch.get_rng_state())


# ------------------------------------------------------------------ engine on the reference ops
FEATURES = [({}, None), ({"num_kv_heads": 2}, None), ({"num_kv_heads": 2, "qk_norm": True, "attention_sinks": True}, SEP),
            ({"sliding_window": 5}, None)]


@pytest.mark.parametrize("recompute,selective", [(False, True), (True, True), (True, False)])
@pytest.mark.parametrize("kw,sep", FEATURES)
def test_engine_matches_autograd_with_the_same_dropout_masks(recompute, selective, kw, sep):
    torch.manual_seed(3)
    m1 = _randomise_norms(GPT(tiny(dropout=0.1, attention_dropout=0.1, **kw)))
    m2 = copy.deepcopy(m1)
    ids = torch.randint(1, 256, (3, 32))
    if sep is not None:
        ids[0, [4, 5, 19]] = sep
        ids[2, 31] = sep
    l1 = _autograd_loss(m1, ids, seed=21, micro=0, sep=sep, p_attn=0.1, p_hidden=0.1)
    l1.backward()
    m2.set_doc_separator(sep)
    eng = m2.enable_engine(seed=21)
    assert eng.post_norm and eng.provider.layer(0).pn1.shape == (64,) and eng.provider.layer_grads(1).pn2.shape == (64,)
    eng.selective_recompute = selective
    m2.gradient_checkpointing = recompute
    m2.train()
    _, l2 = m2(ids, labels=ids)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n
    assert m2.layers[1].mlp_post_norm.weight.grad.abs().max() > 0


def test_engine_with_z_loss_matches_the_eager_model():
    torch.manual_seed(4)
    m1 = _randomise_norms(GPT(tiny()))
    m2 = copy.deepcopy(m1)
    for m in (m1, m2):
        m.set_z_loss(1e-2)
    m2.enable_engine()
    ids = torch.randint(0, 256, (2, 32))
    m1.train()
    m2.train()
    l1, l2 = m1(ids, labels=ids)[1], m2(ids, labels=ids)[1]
    l1.backward()
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n


def test_engine_recompute_modes_are_bit_identical_and_keep_the_raw_branches():
    """Recompute off, selective (a / d_out kept), whole-block (regenerated): same bits."""
    torch.manual_seed(2)
    base = _randomise_norms(GPT(tiny(num_kv_heads=2, dropout=0.1, attention_dropout=0.1)))
    ids = torch.randint(0, 256, (2, 32))
    res = []
    for ac, selective, budget in ((False, True, None), (True, True, None), (True, True, 0.0), (True, False, None)):
        m = copy.deepcopy(base)
        eng = m.enable_engine(seed=11)
        eng.selective_recompute = selective
        if budget is not None:
            eng.ac_budget = budget
        m.gradient_checkpointing = ac
        m.train()
        loss, _, st = eng.forward(ids, shift_targets(ids), train=True, recompute=ac, need_backward=True)
        c = st.caches[0]
        if ac and not selective:
            assert c.a is None and c.dr is None and c.o is None
        else:  # kept always, like o: [M, H] each in the activation dtype
            assert c.a.shape == c.dr.shape == (64, 64) and c.a.dtype == eng.act_dtype
        eng.backward(st, torch.ones(()))
        res.append((loss.item(), [p.grad.clone() for p in m.parameters()]))
    for loss, grads in res[1:]:
        assert loss == res[0][0]
        for a, b in zip(res[0][1], grads):
            assert torch.equal(a, b)


@pytest.mark.parametrize("recompute", [False, True])
def test_train_window_matches_sequential_bit_for_bit(recompute):
    torch.manual_seed(5)
    GA = 2
    m1 = _randomise_norms(GPT(tiny(num_kv_heads=2, dropout=0.1, attention_dropout=0.1)))
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
    assert m2.layers[0].attn_post_norm.weight.grad.abs().max() > 0


# ------------------------------------------------------------------ optimizer groups
def test_post_norm_weights_are_in_the_no_decay_group():
    from distributed_llm_trainer_amd.training.optim import flat_store_optimizer
    m = GPT(tiny(qk_norm=True, attention_sinks=True))
    m.enable_engine()
    opt = flat_store_optimizer(m.store, 1e-3, (0.9, 0.95), 1e-8, 0.1)
    lay = m.store.layout
    (a0, b0, wd0), (a1, b1, wd1) = opt.regions
    assert wd0 == 0.1 and wd1 == 0.0 and b1 == lay.total
    for i in range(2):
        for n in POST:
            s = lay.by_name[f"layers.{i}.{n}.weight"]
            assert a1 <= s.offset and s.offset + s.numel <= b1
    nd_names = [n for n, *_ in opt.param_map[1]]
    assert "layers.1.mlp_post_norm.weight" in nd_names and "layers.0.attn_post_norm.weight" in nd_names
    assert not any("post_norm" in n for n, *_ in opt.param_map[0])
    # the lazy optimizer's units cover the buffer exactly once, the new vectors in their layer's unit
    spans = sorted(r for u in m.store.unit_ranges().values() for r in u)
    assert spans[0][0] == 0 and spans[-1][1] == lay.total
    assert all(spans[j][1] == spans[j + 1][0] for j in range(len(spans) - 1))
    p2 = lay.by_name["layers.1.mlp_post_norm.weight"]
    assert m.store.unit_ranges()[1][1][1] == p2.offset + p2.numel


# ------------------------------------------------------------------ distributed
DIST = dict(vocab_size=384, hidden_size=64, num_layers=2, num_heads=4, num_kv_heads=2, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0, post_norm=True)


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
    assert head[1] == total  # the bucket of the embedding and the norm weights carries the post-norm weights
    tr = _ddp_trainer(4)
    for s in range(3):
        tr.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    ref_p = tr.flat_params()
    assert p0.numel() == GPTConfig(**DIST).num_parameters() + (GPTConfig(**DIST).vocab_size_padded - 384) * 64
    assert torch.allclose(p0, ref_p, atol=2e-5, rtol=1e-4), (p0 - ref_p).abs().max()
    for n in POST:
        s = tr.model.store.layout.by_name[f"layers.0.{n}.weight"]
        assert not torch.equal(p0[s.offset:s.offset + s.numel], torch.ones(64)), f"{n} never trained"


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
    for n in POST:
        assert ref_sd[f"layers.1.{n}.weight"].shape == (64,)
        assert not torch.equal(ref_sd[f"layers.1.{n}.weight"], torch.ones(64))
    assert [s.name for s in tr.runtime.units[0].segs][-2:] == [f"layers.0.{n}.weight" for n in POST]
    for k in ref_sd:
        assert torch.equal(outs[0][k], outs[1][k]), f"{k}: ranks diverged"
        assert torch.allclose(outs[0][k], ref_sd[k], atol=3e-5, rtol=1e-4), (k, (outs[0][k] - ref_sd[k]).abs().max())


def test_fsdp_side_buffer_holds_the_post_norm_gradients():
    """bf16-gradient mode: the two vectors' gradients accumulate in the fp32 norm_grad side buffer,
    after ln1 | ln2 (| q_norm | k_norm | sinks + padding), 16-byte aligned."""
    import types

    from distributed_llm_trainer_amd.parallel.fsdp import FSDPRuntime
    for kw, want in (({}, 4 * 64), ({"qk_norm": True, "attention_sinks": True, "num_heads": 4}, 4 * 64 + 32 + 8)):
        rt = types.SimpleNamespace(cfg=tiny(**kw))
        n = FSDPRuntime._side_numel(rt)
        assert n == want
        d = FSDPRuntime._qk_side(rt, torch.arange(n, dtype=torch.float32))
        assert list(d)[-2:] == ["pn1", "pn2"]
        assert d["pn1"][0].item() == n - 128 and d["pn2"][0].item() == n - 64 and d["pn2"].numel() == 64
        assert (n - 128) % 4 == 0
    off = types.SimpleNamespace(cfg=tiny(post_norm=False, attention_sinks=True, num_heads=4))
    assert FSDPRuntime._side_numel(off) == 2 * 64 + 4  # without the flag: what it was


# ------------------------------------------------------------------ checkpoints
def test_full_checkpoint_round_trip_and_generate(tmp_path):
    from distributed_llm_trainer_amd.eval.infer import load_model
    tr = _ddp_trainer(1)
    for s in range(2):  # the first step is the warm-up step: its learning rate is 0
        tr.train_step({"input_ids": _data(s, 0, n=2)})
    path = str(tmp_path / "pn.pt")
    tr.save_checkpoint(path)
    want = tr.flat_params().clone()
    tr2 = _ddp_trainer(1)
    tr2.load_checkpoint(path)
    assert torch.equal(tr2.flat_params(), want)
    back = load_model(path)
    assert back.config.post_norm and back.config == tr.model.config
    sd = tr.model.state_dict()
    assert not torch.equal(sd["layers.0.attn_post_norm.weight"].cpu(), torch.ones(64))
    for k, v in back.state_dict().items():
        assert torch.equal(v, sd[k].cpu()), k
    ids = torch.randint(0, 384, (1, 5))
    assert back.generate(ids, max_new_tokens=4, top_k=1).shape == (1, 9)
    # the flag overrides a stored config that does not carry it
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    ck = load_checkpoint(path, map_location="cpu")
    ck["model_config"] = GPTConfig.from_dict({**tr.model.config.to_dict(), "post_norm": False})
    save_checkpoint(path, ck)
    assert load_model(path, post_norm=True).config.post_norm


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
    assert not torch.equal(want["layers.0.mlp_post_norm.weight"], torch.ones(64))
    for k in want:
        assert torch.equal(got[k], want[k]), k
    full = consolidate_sharded(d)
    mc = full["model_config"]
    assert (mc["post_norm"] if isinstance(mc, dict) else mc.post_norm) is True
    for k in ("layers.0.attn_post_norm.weight", "layers.1.mlp_post_norm.weight"):
        assert torch.equal(full["model"][k], want[k]), k


# ------------------------------------------------------------------ CLI
def _yaml(tmp_path, val):
    p = tmp_path / "m.yaml"
    extra = f"  post_norm: {val}\n" if val is not None else ""
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
    assert parser.parse_args([]).post_norm is None

    def resolve(argv, yaml_val="absent"):
        args = parser.parse_args(argv)
        cfg = GPTConfig.from_preset("small")
        if yaml_val != "absent":
            cfg = load_yaml_config(_yaml(tmp_path, yaml_val), cfg, TrainingConfig(), None)[0]
        apply_model_args(args, cfg)
        return cfg

    assert resolve([]).post_norm is False                       # preset
    assert resolve(["--post_norm"]).post_norm is True           # CLI over the preset
    assert resolve([], None).post_norm is False                 # YAML without the key
    assert resolve([], "true").post_norm is True                # YAML over the preset
    assert resolve(["--post_norm"], "false").post_norm is True  # CLI over YAML
    assert resolve(["--post_norm"], "false").num_parameters() == resolve([], "false").num_parameters() + 2 * 64
    both = resolve(["--post_norm", "--num_kv_heads", "2", "--qk_norm", "--attention_sinks", "--attn_softcap", "50"])
    assert both.post_norm and both.num_kv_heads == 2 and both.qk_norm and both.attention_sinks and both.attn_softcap == 50.0


def test_cli_trains_and_infers_a_post_norm_model(tmp_path, capsys):
    """--post_norm (with --z_loss and --doc_sep_token) reaches the trainer's model and its
    checkpoint, and infer.py reads it back."""
    from distributed_llm_trainer_amd.eval import infer
    from distributed_llm_trainer_amd.training import ddp_trainer
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint
    env_before = os.environ.get("DLT_DUMMY_BATCHES")
    os.environ["DLT_DUMMY_BATCHES"] = "2"
    try:
        ddp_trainer.main(["--config", _yaml(tmp_path, None), "--post_norm", "--z_loss", "1e-4", "--doc_sep_token", "3",
                          "--batch_size", "1", "--max_steps", "1", "--gradient_accumulation_steps", "1",
                          "--checkpoint_dir", str(tmp_path / "ck")])
    finally:
        if env_before is None:
            os.environ.pop("DLT_DUMMY_BATCHES", None)
        else:
            os.environ["DLT_DUMMY_BATCHES"] = env_before
    ck = load_checkpoint(str(tmp_path / "ck" / "final.pt"), map_location="cpu")
    assert ck["model_config"].post_norm is True
    assert any(k.endswith("layers.0.attn_post_norm.weight") for k in ck["model"])
    m = infer.load_model(str(tmp_path / "ck" / "final.pt"))
    assert m.config.post_norm and m.layers[0].mlp_post_norm.weight.shape == (64,)
    # infer.py's own flag, for a checkpoint whose config lacks the field
    with pytest.raises(SystemExit):
        infer.main(["--post_norm", "--help"])
    assert "--post_norm" in capsys.readouterr().out


# ------------------------------------------------------------------ generation
@pytest.mark.parametrize("kw", [{}, {"num_kv_heads": 2, "qk_norm": True}])
def test_kv_cached_generate_matches_greedy_full_forward(kw):
    from distributed_llm_trainer_amd.eval.decode import KVCache, _fused_kind, forward_cached
    torch.manual_seed(5)
    m1 = _randomise_norms(GPT(tiny(**kw)))
    m2 = copy.deepcopy(m1)
    m2.enable_engine()
    assert _fused_kind(m2, 1) is None
    ids = torch.randint(0, 256, (1, 5))
    o1 = m1.generate(ids, max_new_tokens=8, temperature=1.0, top_k=1)  # greedy full re-forward
    o2 = m2.generate(ids, max_new_tokens=8, temperature=1.0, top_k=1)
    assert o1.shape == (1, 13)
    assert torch.equal(o1, o2)
    # forward_cached agrees with the full forward, and the norms are live in it
    lg = forward_cached(m2, ids, KVCache(m2.config, 1, "cpu", m2.engine.act_dtype))
    m1.eval()
    with torch.no_grad():
        full = m1(ids)[0][:, -1]
    assert torch.allclose(lg, full, atol=1e-4, rtol=1e-4)
    with torch.no_grad():
        for layer in m2.layers:
            layer.attn_post_norm.weight.fill_(1.0)
            layer.mlp_post_norm.weight.fill_(1.0)
    lg1 = forward_cached(m2, ids, KVCache(m2.config, 1, "cpu", m2.engine.act_dtype))
    assert (lg - lg1).abs().max().item() > 1e-4


def test_fused_decode_is_refused_for_a_post_norm_model_only():
    """_fused_kind: None for a post-norm model whatever the ops offer; the default model's answer is untouched."""
    import types

    from distributed_llm_trainer_amd.eval import decode
    ops = types.SimpleNamespace(dec_norm_qkv=None, DECODE_BATCHES=(1, 2, 4, 8))
    cfg = dict(vocab_size=256, hidden_size=256, num_layers=2, num_heads=4, max_seq_len=64)
    for on in (False, True):
        model = types.SimpleNamespace(config=GPTConfig(post_norm=on, **cfg),
                                      engine=types.SimpleNamespace(ops=ops, act_dtype=torch.bfloat16))
        assert decode._fused_kind(model, 1) == (None if on else "mha")
