"""Attention-score soft-capping (GPTConfig.attn_softcap) without a GPU: the config field and its
round trips, the flags, the eager model, the reference ops and the engine on them against dense
autograd formulas, cached decoding, the route check, the argument struct, and the planted defects
of tests/attn_cap_ref.py at the exact inputs tests/test_attn_softcap_gpu.py runs."""
import copy
import ctypes
import math
import os
import pickle

import pytest
import torch
import torch.nn.functional as F

from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.models.engine import shift_targets
from distributed_llm_trainer_amd.ops import attn_routes, reference as ref, rng
from tests import attn_cap_ref as C
from tests import attn_ref as A

SEP = 0
TINY = dict(vocab_size=256, hidden_size=64, num_layers=2, num_heads=4, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0, attn_softcap=1.5)
ALL_ON = {"num_kv_heads": 2, "qk_norm": True, "sliding_window": 5, "sliding_window_pattern": 2,
          "attention_sinks": True, "logit_softcap": 7.0}


def tiny(**kw):
    d = dict(TINY)
    d.update(kw)
    return GPTConfig(**d)


def _randomise(m, seed=0):
    """Larger q / k weights (scores of a few units, so that a cap of 1.5 bends them) and, where
    the model has sinks, non-zero ones."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in m.layers:
            at = layer.attention
            at.q_proj.weight.mul_(20.0)
            at.k_proj.weight.mul_(20.0)
            if getattr(at, "attention_sinks", False):
                at.sinks.copy_(1.5 * torch.randn(at.sinks.shape, generator=g))
    return m


# ------------------------------------------------------------------ config
OLD_FIELDS = ["vocab_size", "hidden_size", "num_layers", "num_heads", "intermediate_size", "max_seq_len", "dropout",
              "attention_dropout", "initializer_range", "activation", "use_flash_attention", "gradient_checkpointing"]


def test_config_without_the_cap_serialises_as_before():
    cfg = GPTConfig.gpt2_small()
    assert cfg.attn_softcap is None
    assert list(cfg.to_dict()) == OLD_FIELDS and list(cfg.__getstate__()) == OLD_FIELDS
    bare = GPTConfig.__new__(GPTConfig)  # an object that never had the field: the same bytes
    bare.__dict__.update({k: v for k, v in cfg.__dict__.items() if k != "attn_softcap"})
    assert pickle.dumps(cfg) == pickle.dumps(bare)
    assert GPTConfig.from_dict(cfg.to_dict()) == cfg
    on = tiny(attn_softcap=50)
    assert on.attn_softcap == 50.0 and isinstance(on.attn_softcap, float)
    assert on.to_dict()["attn_softcap"] == 50.0 and GPTConfig.from_dict(on.to_dict()) == on
    assert pickle.loads(pickle.dumps(on)).attn_softcap == 50.0
    assert pickle.loads(pickle.dumps(cfg)).attn_softcap is None
    both = tiny(logit_softcap=30.0, sliding_window=8)
    assert list(both.to_dict())[-3:] == ["logit_softcap", "attn_softcap", "sliding_window"]
    assert on.num_parameters() == tiny(attn_softcap=None).num_parameters()  # no parameters


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("nan"), True, "50"])
def test_config_validation(bad):
    with pytest.raises(ValueError, match="attn_softcap"):
        GPTConfig(attn_softcap=bad)


def test_old_pickles_load():
    state = {k: v for k, v in GPTConfig.gpt2_small().__dict__.items()
             if k not in ("attn_softcap", "logit_softcap", "attention_sinks", "qk_norm", "num_kv_heads")}
    old = GPTConfig.__new__(GPTConfig)
    old.__setstate__(state)
    assert old.attn_softcap is None and old == GPTConfig.gpt2_small()


def test_state_dict_and_flat_layout_are_unchanged():
    torch.manual_seed(0)
    a, b = GPT(tiny()), GPT(tiny(attn_softcap=None))
    assert list(a.state_dict()) == list(b.state_dict())
    assert [tuple(p.shape) for p in a.parameters()] == [tuple(p.shape) for p in b.parameters()]


# ------------------------------------------------------------------ dense formula
def _rot(x, cos, sin):
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def _autograd_loss(m, ids, seed=0, micro=0, sep=None, p_attn=0.0, p_hidden=0.0):
    """The model as an independent dense formula over ``m``'s parameters (plain autograd):
    s = CAP tanh(scale q.k / CAP) on every score, THEN the masks write -inf, the sink column (not
    capped) joins the softmax and is dropped before dropout; the engine's counter-hash dropout
    masks, the dense document mask, the layers' windows, the final-logit cap."""
    cfg = m.config
    B, S = ids.shape
    nh, nkv, hd, H = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.hidden_size
    cap = cfg.attn_softcap
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
        s = (q @ k[:, idx].transpose(-2, -1)) / math.sqrt(hd)
        if cap is not None:
            s = cap * torch.tanh(s / cap)
        s = s.masked_fill(~allowed, float("-inf"))
        if cfg.attention_sinks:
            col = at.sinks.view(1, nh, 1, 1).expand(B, nh, S, 1)
            pr = torch.softmax(torch.cat([s, col], dim=-1), dim=-1)[..., :S]
        else:
            pr = torch.softmax(s, dim=-1)
        if p_attn > 0:
            pr = pr * rng.attn_keep_mask(B * nh, S, S, k_attn, p_attn).view(B, nh, S, S) / (1.0 - p_attn)
        a = (pr @ v[:, idx]).transpose(1, 2).reshape(B * S, H) @ at.o_proj.weight.t()
        x = x + drop(a, k_resid, p_hidden)
        n2 = norm(x, layer.post_attention_layernorm.weight)
        mlp = layer.mlp
        d = (F.silu(n2 @ mlp.gate_proj.weight.t()) * (n2 @ mlp.up_proj.weight.t())) @ mlp.down_proj.weight.t()
        x = x + drop(d, k_mlp, p_hidden)
    logits = norm(x, m.norm.weight) @ m.embed_tokens.weight.t()
    if cfg.logit_softcap is not None:
        logits = cfg.logit_softcap * torch.tanh(logits / cfg.logit_softcap)
    return F.cross_entropy(logits, shift_targets(ids), ignore_index=-100)


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("kw", [{}, {"num_kv_heads": 2}, ALL_ON])
def test_eager_model_matches_the_dense_formula(kw, flash):
    torch.manual_seed(0)
    m = _randomise(GPT(tiny(use_flash_attention=flash, **kw)))
    m2 = copy.deepcopy(m)
    ids = torch.randint(0, 256, (3, 32))
    _, l1 = m(ids, labels=ids)
    l1.backward()
    l2 = _autograd_loss(m2, ids)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n
    # the cap is live: the same weights without it give another loss
    off = GPT(tiny(use_flash_attention=flash, **{**kw, "attn_softcap": None}))
    off.load_state_dict(m.state_dict())
    assert abs(off(ids, labels=ids)[1].item() - l1.item()) > 1e-3


# ------------------------------------------------------------------ reference ops
def _dense_attention(q, k, v, cap, sink, keep, p, doc, window):
    B, nh, S, hd = q.shape
    G = nh // k.shape[1]
    pos = torch.arange(S)
    allowed = (pos.view(1, 1, 1, S) <= pos.view(1, 1, S, 1)).expand(B, 1, S, S)
    if doc is not None:
        allowed = allowed & (pos.view(1, 1, 1, S) >= doc[0].view(B, 1, S, 1))
    if window is not None:
        allowed = allowed & (pos.view(1, 1, 1, S) > pos.view(1, 1, S, 1) - window)
    s = (q @ k.repeat_interleave(G, 1).transpose(-1, -2)) / math.sqrt(hd)
    s = (cap * torch.tanh(s / cap)).masked_fill(~allowed, float("-inf"))
    if sink is not None:
        s = torch.cat([s, sink.view(1, nh, 1, 1).expand(B, nh, S, 1)], -1)
    pr = torch.softmax(s, -1)[..., :S]
    if p > 0:
        pr = pr * keep / (1.0 - p)
    o = (pr @ v.repeat_interleave(G, 1)).transpose(1, 2).reshape(B * S, nh * hd)
    return o, torch.logsumexp(s, -1)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mask", ["plain", "w37", "doc", "sink"])
@pytest.mark.parametrize("nkv", [4, 2, 1])
def test_reference_ops_match_fp64_autograd(nkv, mask, p):
    B, S, nh, hd, key, cap = 2, 96, 4, 16, 77, 2.0
    g = torch.Generator().manual_seed(nkv * 10 + len(mask))
    q, k, v = (torch.randn(B, h, S, hd, generator=g, dtype=torch.float64) * (2.0 if h == nh else 1.0)
               for h in (nh, nkv, nkv))
    do = torch.randn(B * S, nh * hd, generator=g, dtype=torch.float64)
    window = 37 if mask == "w37" else None
    sink = torch.tensor([-1.0, 0.5, 3.0, 6.0]) if mask == "sink" else None
    doc = None
    if mask == "doc":
        ids = torch.ones(B, S, dtype=torch.long)
        ids[0, [12, 29, 90]] = SEP
        ids[1, 50] = SEP
        doc = ref.doc_bounds(ids, SEP)
    keep = rng.attn_keep_mask(B * nh, S, S, key, p).view(B, nh, S, S).double() if p > 0 else None
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    sa = sink.double().clone().requires_grad_(True) if sink is not None else None
    o_want, lse_want = _dense_attention(qa, ka, va, cap, sa, keep, p, doc, window)
    (o_want * do).sum().backward()

    kw = dict(doc=doc, window=window, softcap=cap)
    o, lse = ref.attention_fwd(q.float(), k.float(), v.float(), p, key, True, sink=sink, **kw)
    assert torch.allclose(o.double(), o_want, atol=2e-5, rtol=1e-4) and torch.allclose(lse.double(), lse_want, atol=2e-5)
    dsink = torch.zeros(nh) if sink is not None else None
    dq, dk, dv = ref.attention_bwd(q.float(), k.float(), v.float(), o, do.float(), lse, p, key, True, sink=sink,
                                   dsink=dsink, **kw)
    for got, want in ((dq, qa.grad), (dk, ka.grad), (dv, va.grad)):
        assert torch.allclose(got.double(), want, atol=5e-5, rtol=1e-3)
    if sink is not None:
        assert torch.allclose(dsink.double(), sa.grad, atol=5e-5, rtol=1e-3)
    # the cap bends these scores: the uncapped ops give something else
    o0, _ = ref.attention_fwd(q.float(), k.float(), v.float(), p, key, True, sink=sink, doc=doc, window=window)
    assert (o0 - o).abs().max() > 1e-2
    # the packed forms are the same ops on q | k | v rows
    qkv = torch.cat([t.float().transpose(1, 2).reshape(B * S, -1) for t in (q, k, v)], 1).contiguous()
    o2, lse2 = ref.attention_fwd_packed(qkv, B, S, nh, p, key, nkv=nkv, sink=sink, **kw)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    cos, sin = ref.rope_tables(hd, S)
    d2 = torch.zeros(nh) if sink is not None else None
    g2 = ref.attention_bwd_packed(qkv, o, do.float(), lse, p, key, B, S, nh, cos, sin, nkv=nkv, sink=sink, dsink=d2, **kw)
    assert g2.shape == qkv.shape


def test_reference_ops_validate_the_cap():
    q = torch.randn(1, 4, 8, 16)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="softcap"):
            ref.attention_fwd(q, q, q, 0.0, 0, True, softcap=bad)
    with pytest.raises(TypeError, match="softcap"):
        ref.attention_fwd(q, q, q, 0.0, 0, True, softcap="2")
    o0, lse0 = ref.attention_fwd(q, q, q, 0.0, 0, True)
    o1, lse1 = ref.attention_fwd(q, q, q, 0.0, 0, True, softcap=None)
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)


# ------------------------------------------------------------------ engine on the reference ops
@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("kw,sep", [({}, None), (ALL_ON, SEP)])
def test_engine_matches_autograd_with_the_same_dropout_masks(recompute, packed, kw, sep):
    torch.manual_seed(3)
    m1 = _randomise(GPT(tiny(dropout=0.1, attention_dropout=0.1, **kw)))
    m2 = copy.deepcopy(m1)
    ids = torch.randint(1, 256, (3, 32))
    if sep is not None:
        ids[0, [4, 5, 19]] = sep
        ids[2, 31] = sep
    l1 = _autograd_loss(m1, ids, seed=21, micro=0, sep=sep, p_attn=0.1, p_hidden=0.1)
    l1.backward()
    m2.set_doc_separator(sep)
    eng = m2.enable_engine(seed=21)
    assert eng.attn_softcap == 1.5
    eng.packed_qkv = packed and eng.packed_qkv
    m2.gradient_checkpointing = recompute
    m2.train()
    _, l2 = m2(ids, labels=ids)
    l2.backward()
    assert abs(l1.item() - l2.item()) < 1e-5
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-6, rtol=1e-4), n


def test_an_uncapped_engine_passes_no_keyword():
    m = GPT(tiny(attn_softcap=None))
    eng = m.enable_engine()
    assert eng.attn_softcap is None

    class St:
        win, doc = None, None

    assert "softcap" not in eng._attn_kw(St, 0, eng.provider.layer(0))
    capped = GPT(tiny()).enable_engine()
    assert capped._attn_kw(St, 0, capped.provider.layer(0))["softcap"] == 1.5


# ------------------------------------------------------------------ generation
@pytest.mark.parametrize("kw", [{}, {"num_kv_heads": 2}, ALL_ON])
def test_forward_cached_matches_a_full_forward(kw):
    from distributed_llm_trainer_amd.eval.decode import KVCache, forward_cached
    torch.manual_seed(5)
    m1 = _randomise(GPT(tiny(**kw))).eval()
    m2 = copy.deepcopy(m1)
    m2.enable_engine()
    ids = torch.randint(0, 256, (2, 9))
    with torch.no_grad():
        full = m1(ids)[0][:, -1]
    cache = KVCache(m2.config, 2, "cpu", m2.engine.act_dtype)
    forward_cached(m2, ids[:, :5], cache)           # a prefill, then token by token
    for t in range(5, 9):
        lg = forward_cached(m2, ids[:, t:t + 1], cache)
    assert torch.allclose(lg, full.float(), atol=2e-4, rtol=1e-4)
    o1 = m1.generate(ids[:1, :5], max_new_tokens=6, temperature=1.0, top_k=1)
    o2 = m2.generate(ids[:1, :5], max_new_tokens=6, temperature=1.0, top_k=1)
    assert torch.equal(o1, o2)
    # the cap is live in the cached path
    m2.config.attn_softcap = None
    lg0 = forward_cached(m2, ids, KVCache(m2.config, 2, "cpu", m2.engine.act_dtype))
    assert (lg0 - lg).abs().max().item() > 1e-3


def test_fused_kind_does_not_depend_on_the_cap():
    import inspect
    from distributed_llm_trainer_amd.eval import decode
    assert "attn_softcap" not in inspect.getsource(decode._fused_kind)


# ------------------------------------------------------------------ checkpoints and flags
def test_checkpoint_round_trip_and_infer_override(tmp_path):
    from distributed_llm_trainer_amd.eval.infer import load_model
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    torch.manual_seed(1)
    m = GPT(tiny(attn_softcap=3.0))
    path = str(tmp_path / "cap.pt")
    save_checkpoint(path, {"model": m.state_dict(), "model_config": m.config})
    back = load_model(path)
    assert back.config.attn_softcap == 3.0 and back.config == m.config
    assert back.layers[0].attention.attn_softcap == 3.0
    ck = load_checkpoint(path, map_location="cpu")
    ck["model_config"] = GPTConfig.from_dict({**m.config.to_dict(), "attn_softcap": None})
    assert "attn_softcap" not in ck["model_config"].to_dict()
    save_checkpoint(path, ck)
    assert load_model(path).config.attn_softcap is None
    assert load_model(path, attn_softcap=7.5).config.attn_softcap == 7.5
    with pytest.raises(ValueError, match="attn_softcap"):
        load_model(path, attn_softcap=-1.0)


def _yaml(tmp_path, val):
    p = tmp_path / "m.yaml"
    extra = f"  attn_softcap: {val}\n" if val is not None else ""
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
    assert parser.parse_args([]).attn_softcap is None

    def resolve(argv, yaml_val="absent"):
        args = parser.parse_args(argv)
        cfg = GPTConfig.from_preset("small")
        if yaml_val != "absent":
            cfg = load_yaml_config(_yaml(tmp_path, yaml_val), cfg, TrainingConfig(), None)[0]
        apply_model_args(args, cfg)
        return cfg

    assert resolve([]).attn_softcap is None                                   # preset
    assert resolve(["--attn_softcap", "50"]).attn_softcap == 50.0             # CLI over the preset
    assert resolve([], None).attn_softcap is None                             # YAML without the key
    assert resolve([], "20.0").attn_softcap == 20.0                           # YAML over the preset
    assert resolve(["--attn_softcap", "50"], "20.0").attn_softcap == 50.0     # CLI over YAML
    with pytest.raises(ValueError, match="attn_softcap"):
        resolve(["--attn_softcap", "-3"])
    both = resolve(["--attn_softcap", "50", "--logit_softcap", "30", "--num_kv_heads", "2", "--qk_norm",
                    "--sliding_window", "8", "--sliding_window_pattern", "2", "--attention_sinks", "--z_loss", "1e-4"])
    assert (both.attn_softcap, both.logit_softcap, both.num_kv_heads, both.qk_norm, both.sliding_window,
            both.attention_sinks) == (50.0, 30.0, 2, True, 8, True)


def test_cli_trains_and_infers_a_capped_model(tmp_path):
    from distributed_llm_trainer_amd.eval.infer import load_model
    from distributed_llm_trainer_amd.training import ddp_trainer
    from distributed_llm_trainer_amd.utils.checkpoint import load_checkpoint
    env_before = os.environ.get("DLT_DUMMY_BATCHES")
    os.environ["DLT_DUMMY_BATCHES"] = "2"
    try:
        ddp_trainer.main(["--config", _yaml(tmp_path, None), "--attn_softcap", "50", "--doc_sep_token", "3",
                          "--batch_size", "1", "--max_steps", "1", "--gradient_accumulation_steps", "1",
                          "--checkpoint_dir", str(tmp_path / "ck")])
    finally:
        if env_before is None:
            os.environ.pop("DLT_DUMMY_BATCHES", None)
        else:
            os.environ["DLT_DUMMY_BATCHES"] = env_before
    ck = load_checkpoint(str(tmp_path / "ck" / "final.pt"), map_location="cpu")
    assert ck["model_config"].attn_softcap == 50.0
    assert load_model(str(tmp_path / "ck" / "final.pt")).config.attn_softcap == 50.0


# ------------------------------------------------------------------ routes and the argument struct
def test_route_check_refusals_and_messages(monkeypatch):
    monkeypatch.delenv("DLT_ALLOW_REFERENCE_ON_GPU", raising=False)
    bf, hf, f32 = torch.bfloat16, torch.float16, torch.float32
    for dt in (bf, hf):
        for hd in (64, 128, 32, 96):  # flash and zero-padded flash
            attn_routes.check_score_softcap("cuda", hd, dt)
    attn_routes.check_score_softcap("cpu", 192, f32)  # the CPU caps on every route
    with pytest.raises(NotImplementedError) as e:
        attn_routes.check_score_softcap("cuda", 192, bf)
    msg = str(e.value)
    assert "GEMM-formulated attention route" in msg and "head_dim 192" in msg and "torch.bfloat16" in msg
    assert "attn_softcap" in msg and "; use bf16 or fp16 activations with head_dim <= 128" in msg
    for hd in (64, 80, 192):
        with pytest.raises(NotImplementedError, match=r"fp32 .* attention route \(head_dim %d, torch.float32\)" % hd):
            attn_routes.check_score_softcap("cuda", hd, f32)
    # not one of the five features of the table
    assert "cap" not in attn_routes.FEATURES and "softcap" not in attn_routes.FEATURES and len(attn_routes.FEATURES) == 5
    assert attn_routes.config_features(tiny()) == attn_routes.config_features(tiny(attn_softcap=None))
    assert "cap" in attn_routes.__doc__.split("\n")[5]


def test_attn_args_keeps_its_size_and_gains_the_field():
    from distributed_llm_trainer_amd.ops import hip
    assert ctypes.sizeof(hip._AttnArgs) == 248
    assert hip._AttnArgs.softcap.offset == 164 and hip._AttnArgs.gen_mask.offset == 160
    assert hip._AttnArgs.stride.offset == 168
    assert hip._AttnArgs().softcap == 0.0  # None builds the struct of before: the field stays zero
    assert hip._attn_cap(None, "x") == {} and hip._attn_cap(2, "x") == {"softcap": 2.0}
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e39, 65537.0, 1e9):
        with pytest.raises(ValueError, match="softcap"):
            hip._attn_cap(bad, "attn")
    assert hip._attn_cap(65536.0, "attn") == {"softcap": 65536.0}


def test_the_gpu_routes_bound_the_cap(monkeypatch):
    """cap * log2(e) times M_DEAD = -1e30 must stay finite in fp32: the GPU routes take at most 2^16."""
    monkeypatch.delenv("DLT_ALLOW_REFERENCE_ON_GPU", raising=False)
    assert attn_routes.SCORE_SOFTCAP_MAX == C.CAP_MAX == 65536.0
    assert 1e30 * attn_routes.SCORE_SOFTCAP_MAX * 1.4427 < 3.4e38 / 1000
    attn_routes.check_score_softcap("cuda", 64, torch.bfloat16, cap=65536.0)
    with pytest.raises(ValueError, match="at most 65536"):
        attn_routes.check_score_softcap("cuda", 64, torch.bfloat16, cap=1e6)
    attn_routes.check_score_softcap("cpu", 64, torch.bfloat16, cap=1e6)  # the reference ops take any finite cap
    o, _ = ref.attention_fwd(torch.randn(1, 2, 8, 16), torch.randn(1, 2, 8, 16), torch.randn(1, 2, 8, 16), 0.0, 0, True,
                             softcap=1e9)
    assert torch.isfinite(o).all()


def test_forward_cached_builds_no_autograd_graph():
    """forward_cached runs under no_grad whoever calls it: logits without a grad_fn, and cache rows
    that do not require grad."""
    from distributed_llm_trainer_amd.eval.decode import KVCache, forward_cached
    for kw in ({}, {"attn_softcap": None}):
        m = GPT(tiny(**kw))
        m.enable_engine()
        assert any(p.requires_grad for p in m.parameters())
        cache = KVCache(m.config, 1, "cpu", m.engine.act_dtype)
        lg = forward_cached(m, torch.randint(0, 256, (1, 6)), cache)
        assert not lg.requires_grad and lg.grad_fn is None
        assert not cache.k[0].requires_grad and not cache.v[1].requires_grad


# ------------------------------------------------------------------ the tolerance and the planted defects
def test_case_list_holds_what_the_issue_names():
    cs = C.CASES
    assert {c.base.S for c in cs} == {65, 129, 200, 320} and {c.base.B for c in cs} == {2} and {c.base.nh for c in cs} == {4}
    assert {c.base.kvh for c in cs} == {4, 2, 1} and {c.base.hd for c in cs} == {64, 128}
    assert {c.base.dtype for c in cs} == {A.BF, A.HF} and {c.base.p for c in cs} == {0.0, 0.1}
    assert {c.base.packed for c in cs} == {True, False} and {c.cap for c in cs} == {2.0, 50.0, C.CAP_MAX}
    kinds = {c.base.bounds[0] if c.base.bounds else "plain" for c in cs}
    assert kinds == {"plain", "doc", "win"} and any(c.sink for c in cs) and any(c.sat for c in cs)
    assert all(c.base.bounds[1] < c.base.S for c in cs if c.base.bounds and c.base.bounds[0] == "win")
    # every CAP instantiation family is reached: MHA and GQA dK/dV, DOC and not, both head dims
    assert {(bool(c.base.nkv), bool(c.base.bounds), c.base.hd) for c in cs} >= {
        (g, d, h) for g in (False, True) for d in (False, True) for h in (64, 128)}


def test_the_cap_bends_at_2_and_is_nearly_linear_at_50():
    c2 = C.case_refs(C.CASES[0])
    x = torch.matmul(c2.inp.q.double(), c2.inp.k.double().transpose(-1, -2)) * c2.inp.scale
    assert 0.8 < x.std().item() < 1.2                                   # unit-variance scores
    assert (2.0 * torch.tanh(x / 2.0) - x).abs().max().item() > 0.5     # CAP 2: tanh bends
    assert (50.0 * torch.tanh(x / 50.0) - x).abs().max().item() < 0.02  # CAP 50: nearly linear
    # the bound on the capped score is absolute near x = 0 and proportional to CAP
    z = torch.zeros(1, dtype=torch.float64)
    e2, e50 = C.cap_terms(z, z, 2.0).eps_s.item(), C.cap_terms(z, z, 50.0).eps_s.item()
    assert e2 > 0 and abs(e50 / e2 - 25.0) < 1e-9 and e2 < 4 * 2.0 * 2.0 ** -23


def test_saturated_case_has_exactly_zero_score_gradients():
    c = next(c for c in C.CASES if c.sat)
    r = C.case_refs(c)
    x = torch.matmul(r.inp.q.double(), A._kv_heads(r.inp.k, 4).transpose(-1, -2)) * r.inp.scale
    assert (x.abs() / c.cap).min().item() > 10
    assert torch.count_nonzero(r.bwd.dq.ref) == 0 and torch.count_nonzero(r.bwd.dk.ref) == 0
    assert r.bwd.dv.ref.abs().max() > 0 and torch.isfinite(r.fwd.o.ref).all() and torch.isfinite(r.fwd.lse.ref).all()


@pytest.mark.parametrize("name", [c.name for c in (C.CASES[0], C.CASES[8], C.CASES[19], C.CASES[22], C.CASES[-1])])
def test_fp32_ops_are_inside_the_tolerance(name):
    """The reference ops in fp32 (another order of operations, torch's tanh) land inside the
    derived bounds on 16-bit-rounded outputs: the bounds are not vacuous either way."""
    c = C.BY_NAME[name]
    b, r = c.base, C.case_refs(c)
    kw = dict(doc=r.inp.doc, softcap=c.cap)
    o, lse = ref.attention_fwd(r.inp.q, r.inp.k, r.inp.v, b.p, b.key, True, sink=r.sink, **kw)
    assert C.worst(o.view(b.B, b.S, b.nh, b.hd), r.fwd.o) <= 1.0 and C.worst(lse, r.fwd.lse) <= 1.0
    ds = torch.zeros(b.nh) if r.sink is not None else None
    dq, dk, dv = ref.attention_bwd(r.inp.q, r.inp.k, r.inp.v, r.o16, r.inp.do, r.lse32, b.p, b.key, True,
                                   sink=r.sink, dsink=ds, **kw)
    if r.inp.rope is None:
        for nm, t in (("dq", dq), ("dk", dk), ("dv", dv)):
            assert C.worst(t, getattr(r.bwd, nm)) <= 1.0, nm


@pytest.mark.parametrize("defect", C.DEFECTS)
def test_planted_defects_are_outside_the_tolerance(defect):
    c, outs = C.DEFECT_CASES[defect]
    b, r = c.base, C.case_refs(c)
    fwd = C.cap_fwd_ref(r.inp.q, r.inp.k, r.inp.v, r.inp.scale, c.cap, r.inp.doc, b.p, b.key, r.sink, defect=defect)
    bwd = C.cap_bwd_ref(r.inp.q, r.inp.k, r.inp.v, r.o16, r.inp.do, r.lse32, r.inp.scale, c.cap, r.inp.doc, b.p, b.key,
                        r.inp.rope, defect=defect)
    got = {"o": (fwd.o.ref, r.fwd.o), "lse": (fwd.lse.ref, r.fwd.lse), "dq": (bwd.dq.ref, r.bwd.dq),
           "dk": (bwd.dk.ref, r.bwd.dk), "dv": (bwd.dv.ref, r.bwd.dv)}
    for nm in outs:
        w = C.worst(round_(got[nm][0], b.dtype if nm != "lse" else torch.float32), got[nm][1])
        assert w > 2.0, f"{defect} hides inside the tolerance of {nm} ({w:.2f})"


def round_(x, dt):
    return x.to(torch.float32).to(dt)


@pytest.mark.parametrize("defect", ["no_cap", "sink_capped"])
def test_planted_decode_defects_are_outside_the_tolerance(defect):
    q, kc, vc = C.dec_inputs(4, 2)
    sink = torch.tensor(C.DEC_SINKS[:4]) * (3.0 if defect == "sink_capped" else 1.0)
    want = C.dec_cap_ref(q[:2], kc[:2], vc[:2], 257, C.DEC_SCALE, 4, 2.0, None, sink)
    bad = C.dec_cap_ref(q[:2], kc[:2], vc[:2], 257, C.DEC_SCALE, 4, 2.0, None, sink, defect=defect)
    assert C.worst(bad.ref.bfloat16(), want) > 2.0
    assert C.worst(want.ref.bfloat16(), want) <= 1.0
