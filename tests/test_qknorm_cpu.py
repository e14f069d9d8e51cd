"""QK-norm (``GPTConfig.qk_norm``: per-head RMSNorm on q and k before RoPE) on the CPU: the
kernels' fp64 references and planted defects (tests/qknorm_ref.py), config, eager model, the
engine on the reference ops, optimizer groups, DDP / FSDP over gloo, checkpoints, the CLI flag
and KV-cached generation."""
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
from tests import qknorm_ref as R
from tests.dist_utils import run_multiprocess

SEP = 0
TINY = dict(vocab_size=256, hidden_size=64, num_layers=2, num_heads=4, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0, qk_norm=True)
DTYPES = [torch.bfloat16, torch.float16]


def tiny(**kw):
    d = dict(TINY)
    d.update(kw)
    return GPTConfig(**d)


def _randomise_norms(m, seed=0):
    """Non-unit q_norm / k_norm weights (the init is ones, which hides a swapped or missing weight)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in m.layers:
            for n in (layer.attention.q_norm, layer.attention.k_norm):
                n.weight.copy_(1.0 + 0.5 * torch.randn(n.weight.shape, generator=g))
    return m


# ------------------------------------------------------------------ kernels: references, models, defects
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("nh,nkv", R.HEADS)
def test_fp32_models_of_the_kernels_are_inside_the_tolerance(nh, nkv, hd, dtype):
    inp = R.make_inputs(nh, nkv, hd, dtype)
    hv = R._heads(inp.qkv, inp)
    assert (hv[R.ZERO_AT] == 0).all() and hv[R.BIG_AT[0], nh + nkv + R.BIG_AT[1]].abs().max() > 1e3
    assert (inp.qw == 0).sum() == 2 and (inp.qw < 0).sum() >= 2 and (inp.kw == 0).sum() == 2
    out = R.fwd_model(inp)
    assert R.worst(R._heads(out, inp), R.fwd_ref(inp)) <= 1.0
    assert torch.equal(out[:, (nh + nkv) * hd:], inp.qkv[:, (nh + nkv) * hd:])
    dq, dqw, dkw = R.bwd_model(inp)
    b = R.bwd_ref(inp)
    assert R.worst(R._heads(dq, inp), b.dx) <= 1.0
    assert R.worst(dqw, b.dqw) <= 1.0 and R.worst(dkw, b.dkw) <= 1.0
    assert torch.equal(dq[:, (nh + nkv) * hd:], inp.dqkv[:, (nh + nkv) * hd:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("defect", ["norm_after_rope", "k_uses_q_weight", "mean_over_half", "eps_dropped"])
def test_planted_forward_defects_are_outside_the_tolerance(defect, hd, dtype):
    inp = R.make_inputs(4, 2, hd, dtype)
    assert R.worst(R._heads(R.fwd_model(inp, defect=defect), inp), R.fwd_ref(inp)) > 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_v_normalisation_changes_the_v_columns(dtype):
    inp = R.make_inputs(4, 2, 64, dtype)
    out = R.fwd_model(inp, defect="v_normalised")
    assert R.worst(R._heads(out, inp), R.fwd_ref(inp)) <= 1.0  # q|k are right: only the v check sees it
    assert not torch.equal(out[:, 6 * 64:], inp.qkv[:, 6 * 64:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("defect", ["mean_term_dropped", "neighbour_rstd"])
def test_planted_backward_defects_are_outside_the_tolerance(defect, hd, dtype):
    inp = R.make_inputs(4, 2, hd, dtype)
    dq, dqw, dkw = R.bwd_model(inp, defect=defect)
    b = R.bwd_ref(inp)
    assert R.worst(R._heads(dq, inp), b.dx) > 1.0
    if defect == "neighbour_rstd":  # xh itself is wrong: the weight gradients leave their bound too
        assert R.worst(dqw, b.dqw) > 1.0 and R.worst(dkw, b.dkw) > 1.0


@pytest.mark.parametrize("dtype", [torch.float32] + DTYPES)
@pytest.mark.parametrize("nh,nkv", R.HEADS)
def test_reference_ops_are_the_kernels_contract(nh, nkv, dtype):
    """ops/reference.py rounds where the kernels do: the 16-bit results are inside the fp64
    tolerance, raw is the input q|k, v is untouched; in fp32 they match autograd."""
    hd = 64
    act = torch.bfloat16 if dtype == torch.float32 else dtype
    inp = R.make_inputs(nh, nkv, hd, act)
    qkv, dqkv = inp.qkv.to(dtype), inp.dqkv.to(dtype)
    W = (nh + nkv) * hd
    raw = torch.full((R.B * R.S, W), 7.0, dtype=dtype)
    out = ref.qknorm_rope_inplace(qkv.clone(), R.B, R.S, nh, inp.cos, inp.sin, inp.qw, inp.kw, R.EPS, raw, nkv=nkv)
    assert torch.equal(raw, qkv[:, :W]) and torch.equal(out[:, W:], qkv[:, W:])
    dqw, dkw = torch.zeros(hd), torch.zeros(hd)
    dx = ref.qknorm_bwd(dqkv.clone(), raw, R.B, R.S, nh, inp.qw, inp.kw, R.EPS, dqw, dkw, nkv=nkv)
    assert torch.equal(dx[:, W:], dqkv[:, W:])
    if dtype != torch.float32:
        b = R.bwd_ref(inp)
        assert R.worst(R._heads(out, inp), R.fwd_ref(inp)) <= 1.0
        assert R.worst(R._heads(dx, inp), b.dx) <= 1.0
        assert R.worst(dqw, b.dqw) <= 1.0 and R.worst(dkw, b.dkw) <= 1.0
        return
    x = qkv.clone().requires_grad_(True)
    qw, kw = inp.qw.clone().requires_grad_(True), inp.kw.clone().requires_grad_(True)
    hv = x.view(R.B * R.S, nh + 2 * nkv, hd)
    w = torch.cat([qw.expand(nh, -1), kw.expand(nkv, -1)])
    u = hv[:, :nh + nkv]
    u = u * torch.rsqrt(u.pow(2).mean(-1, keepdim=True) + R.EPS) * w
    u.backward(dqkv.view(R.B * R.S, nh + 2 * nkv, hd)[:, :nh + nkv])
    got, want = R._heads(dx, inp), x.grad.view(R.B * R.S, nh + 2 * nkv, hd)[:, :nh + nkv]
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-4)
    assert torch.allclose(dqw, qw.grad, atol=1e-4, rtol=1e-4) and torch.allclose(dkw, kw.grad, atol=1e-4, rtol=1e-4)
    with pytest.raises(ValueError, match="raw_out"):
        ref.qknorm_rope_inplace(qkv.clone(), R.B, R.S, nh, inp.cos, inp.sin, inp.qw, inp.kw, R.EPS, raw[:, :-1], nkv=nkv)


# ------------------------------------------------------------------ config
OLD_FIELDS = ["vocab_size", "hidden_size", "num_layers", "num_heads", "intermediate_size", "max_seq_len", "dropout",
              "attention_dropout", "initializer_range", "activation", "use_flash_attention", "gradient_checkpointing"]


def test_config_without_the_flag_serialises_as_before():
    cfg = GPTConfig.gpt2_small()
    assert cfg.qk_norm is False
    assert list(cfg.to_dict()) == OLD_FIELDS and list(cfg.__getstate__()) == OLD_FIELDS
    assert cfg.to_dict() == GPTConfig(qk_norm=False).to_dict()
    assert pickle.dumps(cfg) == pickle.dumps(GPTConfig(qk_norm=False))
    assert GPTConfig.from_dict(cfg.to_dict()) == cfg
    on = tiny()
    assert on.to_dict()["qk_norm"] is True and GPTConfig.from_dict(on.to_dict()) == on
    assert pickle.loads(pickle.dumps(on)).qk_norm is True and pickle.loads(pickle.dumps(cfg)).qk_norm is False
    g = GPTConfig(hidden_size=64, num_heads=4, num_kv_heads=2)
    assert list(g.to_dict()) == OLD_FIELDS + ["num_kv_heads"]


def test_an_old_pickle_loads_without_qk_norm():
    state = {k: v for k, v in GPTConfig.gpt2_small().__dict__.items() if k not in ("qk_norm", "num_kv_heads")}
    old = GPTConfig.__new__(GPTConfig)
    old.__setstate__(state)
    assert old.qk_norm is False and old == GPTConfig.gpt2_small()
    assert "attention.q_norm.weight" not in " ".join(GPT(tiny(qk_norm=False)).state_dict())


@pytest.mark.parametrize("nkv", [None, 2])
def test_num_parameters_counts_the_two_vectors(nkv):
    cfg = tiny(num_kv_heads=nkv)
    assert cfg.num_parameters() == count_parameters(GPT(cfg))
    assert cfg.num_parameters() - tiny(num_kv_heads=nkv, qk_norm=False).num_parameters() == 2 * 2 * 16


def test_state_dict_keys_and_init():
    off, on = GPT(tiny(qk_norm=False)).state_dict(), GPT(tiny()).state_dict()
    new = [k for k in on if k not in off]
    assert new == [f"layers.{i}.attention.{n}_norm.weight" for i in range(2) for n in ("q", "k")]
    assert [k for k in on if k in off] == list(off)
    for k in new:
        assert on[k].shape == (16,) and torch.equal(on[k], torch.ones(16))
    at = GPT(tiny()).layers[0].attention
    assert at.q_norm.eps == at.k_norm.eps == GPT(tiny()).norm.eps


def test_flag_off_keeps_the_key_list_and_flat_layout():
    from distributed_llm_trainer_amd.parallel.flat import FlatLayout
    cfg = tiny(qk_norm=False)
    assert list(GPT(cfg).state_dict()) == list(GPT(GPTConfig(**{k: v for k, v in TINY.items() if k != "qk_norm"})).state_dict())
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
    on = FlatLayout(tiny())
    assert on.total == lay.total + L * 2 * 16 and on.decay_end == lay.decay_end
    assert on.by_name["layers.0.attention.q_norm.weight"].offset == on.by_name["layers.0.post_attention_layernorm.weight"].offset + H
    assert on.by_name["layers.0.attention.k_norm.weight"].offset >= on.decay_end


# ------------------------------------------------------------------ eager model
def _rot(x, cos, sin):
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def _autograd_loss(m, ids, seed=0, micro=0, sep=None, p_attn=0.0, p_hidden=0.0):
    """The QK-norm model as an independent dense formula over ``m``'s parameters (plain
    autograd), with the engine's counter-hash dropout masks and the dense document mask."""
    cfg = m.config
    B, S = ids.shape
    nh, nkv, hd, H = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.hidden_size
    pos = torch.arange(S)
    allowed = (pos.view(1, 1, 1, S) <= pos.view(1, 1, S, 1)).expand(B, 1, S, S)
    if sep is not None:
        lo, _ = ref.doc_bounds(ids, sep)
        allowed = allowed & (pos.view(1, 1, 1, S) >= lo.view(B, 1, S, 1))
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
        q = _rot(norm(q, at.q_norm.weight), cos, sin)  # one weight for all heads, norm before RoPE
        k = _rot(norm(k, at.k_norm.weight), cos, sin)
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
    logits = norm(x, m.norm.weight) @ m.embed_tokens.weight.t()
    return F.cross_entropy(logits, shift_targets(ids), ignore_index=-100)


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("nkv", [None, 2])
def test_eager_model_matches_the_dense_formula(nkv, flash):
    torch.manual_seed(0)
    m = _randomise_norms(GPT(tiny(num_kv_heads=nkv, use_flash_attention=flash)))
    m2 = copy.deepcopy(m)
    ids = torch.randint(0, 256, (3, 32))
    _, l1 = m(ids, labels=ids)
    l1.backward()
    l2 = _autograd_loss(m2, ids)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n
    assert m.layers[0].attention.q_norm.weight.grad.abs().max() > 0
    # the norm is live: the same weights without it give another loss
    off = GPT(tiny(num_kv_heads=nkv, use_flash_attention=flash, qk_norm=False))
    off.load_state_dict(m.state_dict(), strict=False)
    assert abs(off(ids, labels=ids)[1].item() - l1.item()) > 1e-3


# ------------------------------------------------------------------ engine on the reference ops
@pytest.mark.parametrize("recompute,selective", [(False, True), (True, True), (True, False)])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("nkv,sep", [(None, None), (2, None), (2, SEP)])
def test_engine_matches_autograd_with_the_same_dropout_masks(recompute, selective, packed, nkv, sep):
    torch.manual_seed(3)
    m1 = _randomise_norms(GPT(tiny(num_kv_heads=nkv, dropout=0.1, attention_dropout=0.1)))
    m2 = copy.deepcopy(m1)
    ids = torch.randint(1, 256, (3, 32))
    if sep is not None:
        ids[0, [4, 5, 19]] = sep
        ids[2, 31] = sep
    l1 = _autograd_loss(m1, ids, seed=21, micro=0, sep=sep, p_attn=0.1, p_hidden=0.1)
    l1.backward()
    m2.set_doc_separator(sep)
    eng = m2.enable_engine(seed=21)
    assert eng.qk_norm and eng.provider.layer(0).qn.shape == (16,)
    eng.packed_qkv = packed and eng.packed_qkv
    eng.selective_recompute = selective
    m2.gradient_checkpointing = recompute
    m2.train()
    _, l2 = m2(ids, labels=ids)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n


def test_engine_recompute_and_budget_are_bit_identical():
    """Recompute off, on with the QKV output and raw kept, on with both regenerated: same bits."""
    torch.manual_seed(2)
    base = _randomise_norms(GPT(tiny(num_kv_heads=2, dropout=0.1, attention_dropout=0.1)))
    ids = torch.randint(0, 256, (2, 32))
    res = []
    for ac, budget in ((False, None), (True, None), (True, 0.0)):
        m = copy.deepcopy(base)
        eng = m.enable_engine(seed=11)
        if budget is not None:
            eng.ac_budget = budget
        m.gradient_checkpointing = ac
        _, loss = m(ids, labels=ids)
        loss.backward()
        res.append((loss.item(), [p.grad.clone() for p in m.parameters()]))
    # raw is counted next to the QKV output: (H + 2 KV) + (H + KV) columns per row
    eng.ac_budget = 1e12
    per = 2 * 2 * 4  # layers x chains x fp32 bytes
    eng.ac_budget = 64 * (64 + 2 * 32 + 64 + 32) * per
    assert eng._ac_keep(64)[0] is True
    eng.ac_budget -= 1
    assert eng._ac_keep(64)[0] is False
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


@pytest.mark.parametrize("which", ["q_norm", "k_norm"])
def test_engine_norm_weight_gradients_by_finite_differences(which):
    torch.manual_seed(7)
    m = _randomise_norms(GPT(tiny(num_kv_heads=2)))
    m.enable_engine()
    ids = torch.randint(0, 256, (3, 32))
    m.train()
    _, loss = m(ids, labels=ids)
    loss.backward()
    for i in range(2):
        w = getattr(m.layers[i].attention, which).weight
        g = w.grad.clone()
        d = g / g.norm()  # along the gradient: the largest signal
        h = 2e-2
        ls = []
        for sgn in (1.0, -1.0):
            with torch.no_grad():
                w.add_(sgn * h * d)
                ls.append(m.eval_loss(ids).item())
                w.sub_(sgn * h * d)
        fd = (ls[0] - ls[1]) / (2 * h)
        # central difference: O(h^2) truncation (1 % of the slope) + the fp32 loss's own
        # error, a few tens of ulps of a value near 5.5 (2^-21), over 2h
        tol = 1e-2 * abs(fd) + 40 * 2.0 ** -21 / (2 * h)
        assert abs(fd - g.norm().item()) <= tol, (i, fd, g.norm().item(), tol)
        assert g.norm().item() > 10 * 40 * 2.0 ** -21 / (2 * h), "signal under the noise floor"


# ------------------------------------------------------------------ optimizer groups
def test_norm_weights_are_in_the_no_decay_group():
    from distributed_llm_trainer_amd.training.optim import flat_store_optimizer
    m = GPT(tiny())
    m.enable_engine()
    opt = flat_store_optimizer(m.store, 1e-3, (0.9, 0.95), 1e-8, 0.1)
    lay = m.store.layout
    (a0, b0, wd0), (a1, b1, wd1) = opt.regions
    assert wd0 == 0.1 and wd1 == 0.0 and b1 == lay.total
    for i in range(2):
        for n in ("q_norm", "k_norm"):
            s = lay.by_name[f"layers.{i}.attention.{n}.weight"]
            assert a1 <= s.offset and s.offset + s.numel <= b1
    nd_names = [n for n, *_ in opt.param_map[1]]
    assert "layers.1.attention.k_norm.weight" in nd_names and "layers.0.attention.q_norm.weight" in nd_names
    assert not any("q_norm" in n or "k_norm" in n for n, *_ in opt.param_map[0])
    # the lazy optimizer's units cover the buffer exactly once, the new vectors in their layer's unit
    spans = sorted(r for u in m.store.unit_ranges().values() for r in u)
    assert spans[0][0] == 0 and spans[-1][1] == lay.total
    assert all(spans[j][1] == spans[j + 1][0] for j in range(len(spans) - 1))
    k1 = lay.by_name["layers.1.attention.k_norm.weight"]
    assert m.store.unit_ranges()[1][1][1] == k1.offset + k1.numel


# ------------------------------------------------------------------ distributed
DIST = dict(vocab_size=384, hidden_size=64, num_layers=2, num_heads=4, num_kv_heads=2, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0, qk_norm=True)


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
    assert head[1] == total  # the bucket of the embedding and the norm weights carries q_norm / k_norm
    tr = _ddp_trainer(4)
    for s in range(3):
        tr.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    ref_p = tr.flat_params()
    assert p0.numel() == GPTConfig(**DIST).num_parameters() + (GPTConfig(**DIST).vocab_size_padded - 384) * 64
    assert torch.allclose(p0, ref_p, atol=2e-5, rtol=1e-4), (p0 - ref_p).abs().max()
    s = tr.model.store.layout.by_name["layers.0.attention.q_norm.weight"]
    assert not torch.equal(p0[s.offset:s.offset + s.numel], torch.ones(16)), "q_norm never trained"


def _fsdp_trainer(GA, ac):
    from distributed_llm_trainer_amd.training.configs import FSDPConfig, FSDPTrainingConfig
    from distributed_llm_trainer_amd.training.fsdp_trainer import FSDPTrainer
    tc = FSDPTrainingConfig(batch_size=2, gradient_accumulation_steps=GA, warmup_steps=1, max_steps=100,
                            learning_rate=1e-2, micro_step_fusion=1)
    fc = FSDPConfig(sharding_strategy="FULL_SHARD", activation_checkpointing=ac, reduce_dtype="fp32")
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
    assert ref_sd["layers.1.attention.k_norm.weight"].shape == (16,)
    assert not torch.equal(ref_sd["layers.1.attention.k_norm.weight"], torch.ones(16))
    assert [s.name for s in tr.runtime.units[0].segs][-2:] == ["layers.0.attention.q_norm.weight",
                                                               "layers.0.attention.k_norm.weight"]
    for k in ref_sd:
        assert torch.equal(outs[0][k], outs[1][k]), f"{k}: ranks diverged"
        assert torch.allclose(outs[0][k], ref_sd[k], atol=3e-5, rtol=1e-4), (k, (outs[0][k] - ref_sd[k]).abs().max())


# ------------------------------------------------------------------ checkpoints
def test_full_checkpoint_round_trip_and_generate(tmp_path):
    from distributed_llm_trainer_amd.eval.infer import load_model
    tr = _ddp_trainer(1)
    for s in range(2):  # the first step is the warm-up step: its learning rate is 0
        tr.train_step({"input_ids": _data(s, 0, n=2)})
    path = str(tmp_path / "qk.pt")
    tr.save_checkpoint(path)
    want = tr.flat_params().clone()
    tr2 = _ddp_trainer(1)
    tr2.load_checkpoint(path)
    assert torch.equal(tr2.flat_params(), want)
    back = load_model(path)
    assert back.config.qk_norm and back.config == tr.model.config
    sd = tr.model.state_dict()
    assert not torch.equal(sd["layers.0.attention.q_norm.weight"].cpu(), torch.ones(16))
    for k, v in back.state_dict().items():
        assert torch.equal(v, sd[k].cpu()), k
    ids = torch.randint(0, 384, (1, 5))
    assert back.generate(ids, max_new_tokens=4, top_k=1).shape == (1, 9)
    # the flag overrides a stored config that does not carry it
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    ck = load_checkpoint(path, map_location="cpu")
    ck["model_config"] = GPTConfig.from_dict({**tr.model.config.to_dict(), "qk_norm": False})
    save_checkpoint(path, ck)
    assert load_model(path, qk_norm=True).config.qk_norm


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
    assert not torch.equal(want["layers.0.attention.k_norm.weight"], torch.ones(16))
    for k in want:
        assert torch.equal(got[k], want[k]), k
    full = consolidate_sharded(d)
    assert full["model_config"]["qk_norm"] is True if isinstance(full["model_config"], dict) else full["model_config"].qk_norm
    for k in ("layers.0.attention.q_norm.weight", "layers.1.attention.k_norm.weight"):
        assert torch.equal(full["model"][k], want[k]), k


# ------------------------------------------------------------------ CLI
def _yaml(tmp_path, qk):
    p = tmp_path / "m.yaml"
    extra = f"  qk_norm: {qk}\n" if qk is not None else ""
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
    assert parser.parse_args([]).qk_norm is None

    def resolve(argv, yaml_qk="absent"):
        args = parser.parse_args(argv)
        cfg = GPTConfig.from_preset("small")
        if yaml_qk != "absent":
            cfg = load_yaml_config(_yaml(tmp_path, yaml_qk), cfg, TrainingConfig(), None)[0]
        apply_model_args(args, cfg)
        return cfg

    assert resolve([]).qk_norm is False                    # preset
    assert resolve(["--qk_norm"]).qk_norm is True          # CLI over the preset
    assert resolve([], None).qk_norm is False              # YAML without the key
    assert resolve([], "true").qk_norm is True             # YAML over the preset
    assert resolve(["--qk_norm"], "false").qk_norm is True  # CLI over YAML
    assert resolve(["--qk_norm"], "false").num_parameters() == resolve([], "false").num_parameters() + 2 * 16


def test_cli_trains_and_infers_a_qk_norm_model(tmp_path, capsys):
    """--qk_norm reaches the trainer's model and its checkpoint, and infer.py reads it back."""
    from distributed_llm_trainer_amd.eval.infer import load_model
    from distributed_llm_trainer_amd.training import ddp_trainer
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint
    env_before = os.environ.get("DLT_DUMMY_BATCHES")
    os.environ["DLT_DUMMY_BATCHES"] = "2"
    try:
        ddp_trainer.main(["--config", _yaml(tmp_path, None), "--qk_norm", "--batch_size", "1", "--max_steps",
                          "1", "--gradient_accumulation_steps", "1", "--checkpoint_dir", str(tmp_path / "ck")])
    finally:
        if env_before is None:
            os.environ.pop("DLT_DUMMY_BATCHES", None)
        else:
            os.environ["DLT_DUMMY_BATCHES"] = env_before
    ck = load_checkpoint(str(tmp_path / "ck" / "final.pt"), map_location="cpu")
    assert ck["model_config"].qk_norm is True
    assert any(k.endswith("layers.0.attention.q_norm.weight") for k in ck["model"])
    m = load_model(str(tmp_path / "ck" / "final.pt"))
    assert m.config.qk_norm and m.layers[0].attention.k_norm.weight.shape == (16,)


# ------------------------------------------------------------------ generation
@pytest.mark.parametrize("nkv", [None, 2])
def test_kv_cached_generate_matches_greedy_full_forward(nkv):
    from distributed_llm_trainer_amd.eval.decode import _fused_kind
    torch.manual_seed(5)
    m1 = _randomise_norms(GPT(tiny(num_kv_heads=nkv)))
    m2 = copy.deepcopy(m1)
    m2.enable_engine()
    assert _fused_kind(m2, 1) is None
    ids = torch.randint(0, 256, (1, 5))
    o1 = m1.generate(ids, max_new_tokens=8, temperature=1.0, top_k=1)  # greedy full re-forward
    o2 = m2.generate(ids, max_new_tokens=8, temperature=1.0, top_k=1)
    assert o1.shape == (1, 13)
    assert torch.equal(o1, o2)
    # the norm is live in the cached path: unit weights decode something else or the logits differ
    from distributed_llm_trainer_amd.eval.decode import KVCache, forward_cached
    lg = forward_cached(m2, ids, KVCache(m2.config, 1, "cpu", m2.engine.act_dtype))
    with torch.no_grad():
        for layer in m2.layers:
            layer.attention.q_norm.weight.fill_(1.0)
            layer.attention.k_norm.weight.fill_(1.0)
    lg1 = forward_cached(m2, ids, KVCache(m2.config, 1, "cpu", m2.engine.act_dtype))
    assert (lg - lg1).abs().max().item() > 1e-4
