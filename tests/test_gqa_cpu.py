"""Grouped-query attention (``GPTConfig.num_kv_heads``) on the CPU: config, eager model,
reference ops, the engine on the reference ops, DDP / FSDP over gloo, checkpoints, the
CLI flag and KV-cached generation."""
import copy
import math
import os

import pytest
import torch

from distributed_llm_trainer_amd.models import GPT, GPTConfig, count_parameters
from distributed_llm_trainer_amd.models.engine import shift_targets
from distributed_llm_trainer_amd.ops import reference as ref
from tests.dist_utils import run_multiprocess

SEP = 0
TINY = dict(vocab_size=256, hidden_size=64, num_layers=2, num_heads=4, num_kv_heads=2, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0)


def tiny(**kw):
    d = dict(TINY)
    d.update(kw)
    return GPTConfig(**d)


def _doc_batch(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 256, (B, S), generator=g)
    ids[0, [0, 1, 2, S - 10]] = SEP
    ids[1:, S // 2] = SEP
    return ids


# ------------------------------------------------------------------ config
def test_config_default_is_num_heads():
    cfg = GPTConfig(hidden_size=64, num_heads=4)
    assert cfg.num_kv_heads == 4 and cfg.kv_size == 64
    assert tiny().num_kv_heads == 2 and tiny().kv_size == 32
    assert GPTConfig(hidden_size=64, num_heads=4, num_kv_heads=1).kv_size == 16


@pytest.mark.parametrize("nkv", [3, 0, 8])
def test_config_rejects_a_non_divisor(nkv):
    with pytest.raises(ValueError, match="num_kv_heads"):
        GPTConfig(hidden_size=64, num_heads=4, num_kv_heads=nkv)


def test_num_parameters_and_flops_count_the_smaller_projections():
    cfg = tiny()
    assert cfg.num_parameters() == count_parameters(GPT(cfg))
    mha = tiny(num_kv_heads=None)
    H, KV, L = 64, 32, 2
    assert mha.num_parameters() - cfg.num_parameters() == L * 2 * (H - KV) * H
    # the projections shrink, the score FLOPs (2 * 2 * s * h per layer) do not
    assert mha.flops_per_token(32) - cfg.flops_per_token(32) == 3.0 * 2 * L * 2 * (H - KV) * H


def test_to_dict_of_an_mha_config_is_unchanged():
    d = GPTConfig.gpt2_small().to_dict()
    assert "num_kv_heads" not in d
    assert list(d) == ["vocab_size", "hidden_size", "num_layers", "num_heads", "intermediate_size", "max_seq_len",
                       "dropout", "attention_dropout", "initializer_range", "activation", "use_flash_attention",
                       "gradient_checkpointing"]
    assert GPTConfig.from_dict(d) == GPTConfig.gpt2_small()
    g = tiny().to_dict()
    assert g["num_kv_heads"] == 2 and GPTConfig.from_dict(g) == tiny()


def test_pickled_mha_config_has_no_new_field():
    import pickle
    cfg = GPTConfig.gpt2_small()
    state = cfg.__getstate__()
    assert "num_kv_heads" not in state
    back = pickle.loads(pickle.dumps(cfg))
    assert back == cfg and back.num_kv_heads == 12
    old = GPTConfig.__new__(GPTConfig)  # a pickle written before the field existed
    old.__setstate__({k: v for k, v in state.items()})
    assert old.num_kv_heads == 12 and old.kv_size == 768
    g = pickle.loads(pickle.dumps(tiny()))
    assert g.num_kv_heads == 2


def test_state_dict_shapes_and_keys():
    sd = GPT(tiny()).state_dict()
    assert list(sd) == list(GPT(tiny(num_kv_heads=None)).state_dict())
    assert sd["layers.0.attention.q_proj.weight"].shape == (64, 64)
    assert sd["layers.0.attention.k_proj.weight"].shape == (32, 64)
    assert sd["layers.1.attention.v_proj.weight"].shape == (32, 64)
    assert sd["layers.0.attention.o_proj.weight"].shape == (64, 64)


# ------------------------------------------------------------------ eager model
def _expanded_mha(gqa: GPT) -> GPT:
    """The MHA model that computes what ``gqa`` computes: its k_proj / v_proj rows are
    the GQA rows repeated per group."""
    cfg = gqa.config
    G, hd = cfg.num_heads // cfg.num_kv_heads, cfg.head_dim
    mha = GPT(GPTConfig.from_dict({**cfg.to_dict(), "num_kv_heads": None}))
    sd = {k: v.clone() for k, v in gqa.state_dict().items()}
    for k in list(sd):
        if k.endswith(("k_proj.weight", "v_proj.weight")):
            w = sd[k].view(cfg.num_kv_heads, hd, cfg.hidden_size)
            sd[k] = w.repeat_interleave(G, dim=0).reshape(cfg.hidden_size, cfg.hidden_size)
    mha.load_state_dict(sd)
    return mha


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("sep", [None, SEP])
def test_eager_gqa_equals_mha_with_repeated_kv_rows(sep, flash):
    torch.manual_seed(0)
    gqa = GPT(tiny(use_flash_attention=flash))
    mha = _expanded_mha(gqa)
    gqa.set_doc_separator(sep)
    mha.set_doc_separator(sep)
    ids = _doc_batch(3, 32)
    lg, loss_g = gqa(ids, labels=ids)
    lm, loss_m = mha(ids, labels=ids)
    assert torch.equal(lg, lm) or (lg - lm).abs().max().item() <= 1e-6
    loss_g.backward()
    loss_m.backward()
    cfg = gqa.config
    G, hd, H = cfg.num_heads // cfg.num_kv_heads, cfg.head_dim, cfg.hidden_size
    for i in range(cfg.num_layers):
        for name in ("k_proj", "v_proj"):
            g = getattr(gqa.layers[i].attention, name).weight.grad
            m = getattr(mha.layers[i].attention, name).weight.grad
            want = m.view(cfg.num_kv_heads, G, hd, H).sum(dim=1).reshape(cfg.kv_size, H)
            assert (g - want).abs().max().item() <= 1e-5 * want.abs().max().item(), (i, name)
        gq, mq = gqa.layers[i].attention.q_proj.weight.grad, mha.layers[i].attention.q_proj.weight.grad
        assert torch.allclose(gq, mq, atol=1e-7, rtol=1e-5)


# ------------------------------------------------------------------ reference ops
def _dense_attention(q, k, v, G, doc=None):
    """Independent dense softmax attention with autograd: q [B, nh, S, hd], k, v
    [B, nkv, S, hd]; query head h uses kv head h // G.  Returns o [B, nh, S, hd], lse."""
    B, nh, S, hd = q.shape
    idx = torch.arange(nh) // G
    kk, vv = k[:, idx], v[:, idx]
    s = torch.einsum("bhqd,bhkd->bhqk", q, kk) / math.sqrt(hd)
    qpos, kpos = torch.arange(S)[:, None], torch.arange(S)[None, :]
    hidden = (kpos > qpos)[None, None]
    if doc is not None:
        hidden = hidden | (kpos[None, None] < doc[0].long()[:, None, :, None])
    s = s.masked_fill(hidden, float("-inf"))
    return torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, dim=-1), vv), torch.logsumexp(s, dim=-1)


@pytest.mark.parametrize("nh,nkv", [(4, 1), (4, 2), (6, 2), (4, 4)])
@pytest.mark.parametrize("with_doc", [False, True])
def test_reference_ops_match_dense_autograd(nh, nkv, with_doc):
    torch.manual_seed(1)
    B, S, hd = 2, 24, 16
    q = torch.randn(B, nh, S, hd, requires_grad=True)
    k = torch.randn(B, nkv, S, hd, requires_grad=True)
    v = torch.randn(B, nkv, S, hd, requires_grad=True)
    doc = ref.doc_bounds(_doc_batch(B, S), SEP) if with_doc else None
    o_d, lse_d = _dense_attention(q, k, v, nh // nkv, doc)
    do = torch.randn(B * S, nh * hd)
    o_d.transpose(1, 2).reshape(B * S, nh * hd).backward(do)
    o, lse = ref.attention_fwd(q.detach(), k.detach(), v.detach(), 0.0, 0, True, doc=doc)
    assert torch.allclose(o, o_d.transpose(1, 2).reshape(B * S, nh * hd).detach(), atol=1e-5, rtol=1e-5)
    assert torch.allclose(lse, lse_d.detach(), atol=1e-5, rtol=1e-5)
    dq, dk, dv = ref.attention_bwd(q.detach(), k.detach(), v.detach(), o, do, lse, 0.0, 0, True, doc=doc)
    assert dk.shape == k.shape and dv.shape == v.shape
    for got, want in ((dq, q.grad), (dk, k.grad), (dv, v.grad)):
        assert torch.allclose(got, want, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("nh,nkv", [(4, 2), (6, 2), (4, 1)])
def test_reference_packed_ops_match_the_head_major_ones(nh, nkv):
    torch.manual_seed(2)
    B, S, hd = 2, 16, 16
    H, KV = nh * hd, nkv * hd
    qkv = torch.randn(B * S, H + 2 * KV)
    cos, sin = ref.rope_tables(hd, S)
    q, k, v = ref.rope_qkv_fwd(qkv, B, S, nh, cos, sin, nkv=nkv)
    assert q.shape == (B, nh, S, hd) and k.shape == v.shape == (B, nkv, S, hd)
    roped = ref.rope_qk_inplace(qkv.clone(), B, S, nh, cos, sin, nkv=nkv)
    assert torch.equal(roped[:, H + KV:], qkv[:, H + KV:])  # v untouched
    assert torch.equal(roped[:, :H].view(B, S, nh, hd).transpose(1, 2), q)
    assert torch.equal(roped[:, H:H + KV].view(B, S, nkv, hd).transpose(1, 2), k)
    p, key = 0.1, 1234
    o, lse = ref.attention_fwd(q, k, v, p, key, True)
    o2, lse2 = ref.attention_fwd_packed(roped, B, S, nh, p, key, nkv=nkv)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    do = torch.randn_like(o)
    dq, dk, dv = ref.attention_bwd(q, k, v, o, do, lse, p, key, True)
    dqkv = ref.attention_bwd_packed(roped, o, do, lse, p, key, B, S, nh, cos, sin, nkv=nkv)
    assert dqkv.shape == (B * S, H + 2 * KV)
    assert torch.equal(dqkv, ref.rope_qkv_bwd(dq, dk, dv, cos, sin))
    with pytest.raises(ValueError, match="nkv"):
        ref.attention_fwd_packed(roped, B, S, nh, p, key, nkv=3)


def test_reference_ops_reject_mismatched_kv():
    q = torch.randn(1, 4, 8, 16)
    with pytest.raises(ValueError, match="nkv"):
        ref.attention_fwd(q, torch.randn(1, 3, 8, 16), torch.randn(1, 3, 8, 16), 0.0, 0)
    with pytest.raises(ValueError, match="same"):
        ref.attention_fwd(q, torch.randn(1, 2, 8, 16), torch.randn(1, 4, 8, 16), 0.0, 0)


# ------------------------------------------------------------------ engine on the CPU ops
def _grads(m):
    return {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("nkv", [2, 1])
def test_engine_matches_eager_autograd(recompute, packed, nkv):
    torch.manual_seed(0)
    m1 = GPT(tiny(num_kv_heads=nkv))
    m2 = copy.deepcopy(m1)
    ids = torch.randint(0, 256, (3, 32))
    _, l1 = m1(ids, labels=ids)
    (l1 * 0.5).backward()
    eng = m2.enable_engine()
    assert eng.gqa and eng.qkv_width == 64 + 2 * nkv * 16
    eng.packed_qkv = packed and eng.packed_qkv
    m2.gradient_checkpointing = recompute
    _, l2 = m2(ids, labels=ids)
    (l2 * 0.5).backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    g1, g2 = _grads(m1), _grads(m2)
    assert g2["layers.0.attention.k_proj.weight"].shape == (nkv * 16, 64)
    for n in g1:
        assert torch.allclose(g1[n], g2[n], atol=1e-6, rtol=1e-4), n


def test_engine_matches_eager_autograd_with_separator():
    torch.manual_seed(1)
    m1 = GPT(tiny())
    m1.set_doc_separator(SEP)
    m2 = copy.deepcopy(m1)
    ids = _doc_batch(3, 32)
    _, l1 = m1(ids, labels=ids)
    l1.backward()
    m2.enable_engine()
    _, l2 = m2(ids, labels=ids)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    g1, g2 = _grads(m1), _grads(m2)
    for n in g1:
        assert torch.allclose(g1[n], g2[n], atol=1e-6, rtol=1e-4), n


def test_dropout_recompute_is_bit_identical():
    """Recompute on and off see the same dropout masks and give the same bits."""
    torch.manual_seed(2)
    base = GPT(tiny(dropout=0.1, attention_dropout=0.1))
    ids = torch.randint(0, 256, (2, 32))
    grads, losses = [], []
    for ac in (False, True):
        m = copy.deepcopy(base)
        m.enable_engine(seed=11)
        m.gradient_checkpointing = ac
        _, loss = m(ids, labels=ids)
        loss.backward()
        losses.append(loss.item())
        grads.append([p.grad.clone() for p in m.parameters()])
    assert losses[0] == losses[1]
    for a, b in zip(*grads):
        assert torch.equal(a, b)


@pytest.mark.parametrize("recompute", [False, True])
def test_train_window_matches_sequential_bit_for_bit(recompute):
    torch.manual_seed(5)
    GA = 2
    m1 = GPT(tiny(dropout=0.1, attention_dropout=0.1))
    m2 = copy.deepcopy(m1)
    e1 = m1.enable_engine(seed=5)
    e2 = m2.enable_engine(seed=5)
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


# ------------------------------------------------------------------ distributed
DIST = dict(vocab_size=384, hidden_size=64, num_layers=2, num_heads=4, num_kv_heads=2, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0)


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
    return tr.flat_params().clone(), len(tr.ddp.buckets)


def test_ddp_matches_single_process():
    (p0, nb), (p1, _) = run_multiprocess(_ddp_worker, world=2, args=(3,))
    assert torch.equal(p0, p1), "ranks diverged"
    assert nb > 2
    tr = _ddp_trainer(4)
    for s in range(3):
        tr.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    ref_p = tr.flat_params()
    assert p0.numel() == GPTConfig(**DIST).num_parameters() + (GPTConfig(**DIST).vocab_size_padded - 384) * 64
    assert torch.allclose(p0, ref_p, atol=2e-5, rtol=1e-4), (p0 - ref_p).abs().max()


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
    assert ref_sd["layers.0.attention.k_proj.weight"].shape == (32, 64)
    for k in ref_sd:
        assert torch.equal(outs[0][k], outs[1][k]), f"{k}: ranks diverged"
        assert torch.allclose(outs[0][k], ref_sd[k], atol=3e-5, rtol=1e-4), (k, (outs[0][k] - ref_sd[k]).abs().max())


# ------------------------------------------------------------------ checkpoint, CLI, generation
def test_checkpoint_round_trip_and_generate(tmp_path):
    from distributed_llm_trainer_amd.eval.infer import load_model
    from distributed_llm_trainer_amd.utils.checkpoint import model_state_dict_cpu
    torch.manual_seed(3)
    m = GPT(tiny())
    path = str(tmp_path / "gqa.pt")
    torch.save({"model": model_state_dict_cpu(m), "model_config": m.config}, path)
    back = load_model(path)
    assert back.config.num_kv_heads == 2 and back.config == m.config
    for (n, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a, b), n
    ids = torch.randint(0, 256, (1, 5))
    m.eval()
    assert torch.equal(m.generate(ids, max_new_tokens=6, top_k=1), back.generate(ids, max_new_tokens=6, top_k=1))
    # --num_kv_heads overrides the stored config
    torch.save({"model": model_state_dict_cpu(m), "model_config": tiny(num_kv_heads=None)}, path)
    assert load_model(path, num_kv_heads=2).config.num_kv_heads == 2


def _yaml(tmp_path, nkv):
    p = tmp_path / "m.yaml"
    extra = f"  num_kv_heads: {nkv}\n" if nkv is not None else ""
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
    assert parser.parse_args([]).num_kv_heads is None

    def resolve(argv, yaml_nkv="absent"):
        args = parser.parse_args(argv)
        cfg = GPTConfig.from_preset("small")
        if yaml_nkv != "absent":
            cfg = load_yaml_config(_yaml(tmp_path, yaml_nkv), cfg, TrainingConfig(), None)[0]
        apply_model_args(args, cfg)
        return cfg

    assert resolve([]).num_kv_heads == 12                       # preset
    assert resolve(["--num_kv_heads", "4"]).num_kv_heads == 4   # CLI over the preset
    assert resolve([], None).num_kv_heads == 4                   # YAML without the key: its num_heads
    assert resolve([], 2).num_kv_heads == 2                      # YAML over the preset
    assert resolve(["--num_kv_heads", "1"], 2).num_kv_heads == 1  # CLI over YAML
    assert resolve(["--num_kv_heads", "1"], 2).kv_size == 16
    with pytest.raises(ValueError, match="num_kv_heads"):
        resolve(["--num_kv_heads", "5"])


def test_cli_trains_a_gqa_model_end_to_end(tmp_path):
    """--num_kv_heads reaches the trainer's model and its checkpoint."""
    from distributed_llm_trainer_amd.training import ddp_trainer
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint
    env_before = os.environ.get("DLT_DUMMY_BATCHES")
    os.environ["DLT_DUMMY_BATCHES"] = "2"
    try:
        ddp_trainer.main(["--config", _yaml(tmp_path, None), "--num_kv_heads", "2", "--batch_size", "1", "--max_steps",
                          "1", "--gradient_accumulation_steps", "1", "--checkpoint_dir", str(tmp_path / "ck")])
    finally:
        if env_before is None:
            os.environ.pop("DLT_DUMMY_BATCHES", None)
        else:
            os.environ["DLT_DUMMY_BATCHES"] = env_before
    ck = load_checkpoint(str(tmp_path / "ck" / "final.pt"), map_location="cpu")
    assert ck["model_config"].num_kv_heads == 2
    sd = ck["model"]
    key = [k for k in sd if k.endswith("layers.0.attention.k_proj.weight")][0]
    assert sd[key].shape == (32, 64)


@pytest.mark.parametrize("nkv", [2, 1])
def test_kv_cached_generate_matches_the_eager_re_forward(nkv):
    from distributed_llm_trainer_amd.eval.decode import KVCache
    torch.manual_seed(5)
    m1 = GPT(tiny(num_kv_heads=nkv))
    m2 = copy.deepcopy(m1)
    eng = m2.enable_engine()
    cache = KVCache(m2.config, 1, "cpu", eng.act_dtype)
    assert cache.k[0].shape == (1, nkv, 32, 16) and cache.v[1].shape == (1, nkv, 32, 16)
    ids = torch.randint(0, 256, (1, 5))
    o1 = m1.generate(ids, max_new_tokens=8, temperature=1.0, top_k=1)  # greedy
    o2 = m2.generate(ids, max_new_tokens=8, temperature=1.0, top_k=1)
    assert o1.shape == (1, 13)
    assert torch.equal(o1, o2)
