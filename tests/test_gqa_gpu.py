"""Grouped-query attention on the MI355X (GQA instantiations of attention.hip, the GQA
form of the in-place RoPE): forward and dQ bit for bit against the MHA kernels on repeated
K/V, dK/dV against the fp32 reference and against the sum of the MHA kernel's per-head
results, bitwise properties, the document mask, the engine end to end, the routes that
refuse GQA, and KV-cached generation.

Shapes: B = 2, (nh, nkv) in {(4, 1), (4, 2), (6, 2)}, head_dim 64 / 128, dropout 0 / 0.1;
S = 192 is three 64-row blocks (odd: the "middle item once" path of the paired work map),
S = 200 an even block count with a ragged last tile.  Tolerances are those of
tests/test_kernels_gpu.py / tests/test_doc_mask_gpu.py (same per-element arithmetic).

dK/dV against the MHA kernel: the GQA kernel rounds ONE fp32 sum over the group to bf16,
the comparison sums G bf16-rounded per-head results in fp32.  With unit roundoff 2^-9 on
each side the exact bound is 2^-9 (|sum x| + sum |x_g|); the factor 2 covers the fp32
reassociation between one long accumulation and G short ones:
    |gqa - sum_g mha_g| <= 2^-8 (|gqa| + sum_g |mha_g|)   elementwise."""
import copy
import functools

import pytest
import torch

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip, reference as ref, rng

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 2
HEADS = [(4, 1), (4, 2), (6, 2)]
CASES = [(nh, nkv, hd, p, S) for nh, nkv in HEADS for hd in (64, 128) for p in (0.0, 0.1) for S in (192, 200)]
KEY = rng.site_key(3, 1, 2, rng.SITE_ATTN)
SEP = 3
DOC_SEPS = (0, 1, 2, 150)  # batch row 0 of the S = 200 document-mask case


def _close(a, b, atol, rtol=0.0, what=""):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    bad = (err > lim).sum().item()
    assert bad == 0, f"{what}: {bad} elements out of tolerance, max err {err.max().item():.3e}"


def _grad_close(got, want, what):
    scale = want.float().abs().max().item()
    _close(got, want, 2e-2 * max(1.0, scale), 2e-2, what)


def _rep(t, G):
    return t.repeat_interleave(G, dim=1).contiguous()


def _rows(t):
    """[B, h, S, hd] -> the [B*S, h*hd] column block of a packed row."""
    return t.transpose(1, 2).reshape(t.shape[0] * t.shape[2], -1)


def _doc(S):
    g = torch.Generator().manual_seed(S)
    ids = torch.randint(SEP + 1, 500, (B, S), generator=g)
    for j in DOC_SEPS:
        ids[0, j] = SEP
    return hip.doc_bounds(ids.to(DEV), SEP)


@functools.lru_cache(maxsize=None)
def _case(nh, nkv, hd, p, S, with_doc=False):
    """Inputs, the fp32 reference results and the MHA kernels' results on K/V repeated
    over the group; computed once and shared (read-only) by the tests below."""
    G = nh // nkv
    g = torch.Generator().manual_seed(100000 * nh + 10000 * nkv + 10 * S + hd)
    q = torch.randn(B, nh, S, hd, generator=g).bfloat16().to(DEV)
    k, v = (torch.randn(B, nkv, S, hd, generator=g).bfloat16().to(DEV) for _ in range(2))
    do = torch.randn(B * S, nh * hd, generator=g).bfloat16().to(DEV)
    doc = _doc(S) if with_doc else None
    kw = {"doc": doc} if with_doc else {}
    o_ref, lse_ref = ref.attention_fwd(q.float(), k.float(), v.float(), p, KEY, **kw)
    grads_ref = ref.attention_bwd(q.float(), k.float(), v.float(), o_ref, do.float(), lse_ref, p, KEY, **kw)
    kr, vr = _rep(k, G), _rep(v, G)
    o_m, aux_m = hip.attention_fwd(q, kr, vr, p, KEY, **kw)
    grads_m = hip.attention_bwd(q, kr, vr, o_m, do, aux_m, p, KEY, **kw)
    return dict(q=q, k=k, v=v, do=do, kw=kw, G=G, o_ref=o_ref, lse_ref=lse_ref, grads_ref=grads_ref, kr=kr, vr=vr,
                o_m=o_m, lse_m=aux_m[0], grads_m=grads_m)


def _packed(c):
    """The GQA packed rows [M, H + 2*KV] and the MHA rows [M, 3H] of a case (q | k | v,
    taken as already rotated)."""
    pg = torch.cat([_rows(c["q"]), _rows(c["k"]), _rows(c["v"])], dim=1).contiguous()
    pm = torch.cat([_rows(c["q"]), _rows(c["kr"]), _rows(c["vr"])], dim=1).contiguous()
    return pg, pm


def _check_fwd_dq_bitwise(c, nh, nkv, hd, p, S):
    o, aux = hip.attention_fwd(c["q"], c["k"], c["v"], p, KEY, **c["kw"])
    assert aux[0].shape == (B, nh, S)
    assert torch.equal(o, c["o_m"]), "o (head-major)"
    assert torch.equal(aux[0], c["lse_m"]), "lse (head-major)"
    dq, dk, dv = hip.attention_bwd(c["q"], c["k"], c["v"], o, c["do"], aux, p, KEY, **c["kw"])
    assert dk.shape == c["k"].shape and dv.shape == c["v"].shape
    assert torch.equal(dq, c["grads_m"][0]), "dq (head-major)"
    # packed layout: q columns of the gradient carry the same inverse rotation in both
    H = nh * hd
    pg, pm = _packed(c)
    cos, sin = hip.rope_tables(hd, S, device=DEV)
    og, auxg = hip.attention_fwd_packed(pg, B, S, nh, p, KEY, nkv=nkv, **c["kw"])
    om, auxm = hip.attention_fwd_packed(pm, B, S, nh, p, KEY, **c["kw"])
    assert torch.equal(og, om) and torch.equal(auxg[0], auxm[0]), "o / lse (packed)"
    assert torch.equal(og, o), "packed vs head-major o"
    dg = hip.attention_bwd_packed(pg, og, c["do"], auxg, p, KEY, B, S, nh, cos, sin, nkv=nkv, **c["kw"])
    dm = hip.attention_bwd_packed(pm, om, c["do"], auxm, p, KEY, B, S, nh, cos, sin, **c["kw"])
    assert dg.shape == (B * S, H + 2 * nkv * hd)
    assert torch.equal(dg[:, :H], dm[:, :H]), "dq (packed)"


# ------------------------------------------------------------------ 1. forward and dQ
@pytest.mark.parametrize("nh,nkv,hd,p,S", CASES)
def test_fwd_and_dq_are_bitwise_the_mha_kernels(nh, nkv, hd, p, S):
    """The per-query-head arithmetic is the MHA kernel's: o, lse and dq equal the MHA
    kernel's on K/V repeated over the group, in both layouts."""
    _check_fwd_dq_bitwise(_case(nh, nkv, hd, p, S), nh, nkv, hd, p, S)


@pytest.mark.parametrize("nh,nkv,hd,p,S", CASES)
def test_fwd_against_fp32_reference(nh, nkv, hd, p, S):
    c = _case(nh, nkv, hd, p, S)
    o, aux = hip.attention_fwd(c["q"], c["k"], c["v"], p, KEY)
    _close(aux[0], c["lse_ref"], 2e-3, 1e-4, "lse")
    _close(o, c["o_ref"], 2e-2, 2e-2, "o")


# ------------------------------------------------------------------ 2. dK / dV
def _check_dkdv(c, p):
    G = c["G"]
    o, aux = hip.attention_fwd(c["q"], c["k"], c["v"], p, KEY, **c["kw"])
    dq, dk, dv = hip.attention_bwd(c["q"], c["k"], c["v"], o, c["do"], aux, p, KEY, **c["kw"])
    for got, want, n in zip((dq, dk, dv), c["grads_ref"], ("dq", "dk", "dv")):
        assert torch.isfinite(got.float()).all(), n
        _grad_close(got, want, n)
    for got, m, n in ((dk, c["grads_m"][1], "dk"), (dv, c["grads_m"][2], "dv")):
        mg = m.float().view(B, m.shape[1] // G, G, m.shape[2], m.shape[3])
        err = (got.float() - mg.sum(dim=2)).abs()
        lim = 2.0 ** -8 * (got.float().abs() + mg.abs().sum(dim=2))
        bad = (err > lim).sum().item()
        assert bad == 0, f"{n}: {bad} elements beyond 2^-8 (|gqa| + sum |mha_g|), max err {err.max().item():.3e}"


@pytest.mark.parametrize("nh,nkv,hd,p,S", CASES)
def test_dkdv_against_reference_and_the_mha_group_sum(nh, nkv, hd, p, S):
    _check_dkdv(_case(nh, nkv, hd, p, S), p)


# ------------------------------------------------------------------ 3. bitwise consistency
@pytest.mark.parametrize("nh,nkv,hd,p,S", [c for c in CASES if c[3] > 0.0 or c[4] == 200])
def test_repeat_calls_and_regenerated_keep_bits_are_bitwise_equal(nh, nkv, hd, p, S):
    c = _case(nh, nkv, hd, p, S)
    runs = []
    for store in (True, True, False):  # the last: the backward regenerates the keep bits
        o, aux = hip.attention_fwd(c["q"], c["k"], c["v"], p, KEY, store_mask=store)
        assert (aux[1] is None) == (p == 0.0 or not store)
        runs.append((o, aux[0]) + tuple(hip.attention_bwd(c["q"], c["k"], c["v"], o, c["do"], aux, p, KEY)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    pg, _ = _packed(c)
    cos, sin = hip.rope_tables(hd, S, device=DEV)
    outs = []
    for store in (True, True, False):
        o, aux = hip.attention_fwd_packed(pg, B, S, nh, p, KEY, nkv=nkv, store_mask=store)
        outs.append(hip.attention_bwd_packed(pg, o, c["do"], aux, p, KEY, B, S, nh, cos, sin, nkv=nkv))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("hd,p,S", [(hd, p, S) for hd in (64, 128) for p in (0.0, 0.1) for S in (192, 200)])
def test_nkv_equal_nh_through_the_new_entry_points_is_the_old_result(hd, p, S):
    nh = 4
    c = _case(nh, 2, hd, p, S)
    q, k, v, do = c["q"], c["kr"], c["vr"], c["do"]  # nh K/V heads
    o, aux = hip.attention_fwd(q, k, v, p, KEY, nkv=nh)
    assert torch.equal(o, c["o_m"]) and torch.equal(aux[0], c["lse_m"])
    for a, b, n in zip(hip.attention_bwd(q, k, v, o, do, aux, p, KEY, nkv=nh), c["grads_m"], ("dq", "dk", "dv")):
        assert torch.equal(a, b), n
    _, pm = _packed(c)
    cos, sin = hip.rope_tables(hd, S, device=DEV)
    o1, a1 = hip.attention_fwd_packed(pm, B, S, nh, p, KEY)
    o2, a2 = hip.attention_fwd_packed(pm, B, S, nh, p, KEY, nkv=nh)
    assert torch.equal(o1, o2) and torch.equal(a1[0], a2[0])
    assert torch.equal(hip.attention_bwd_packed(pm, o1, do, a1, p, KEY, B, S, nh, cos, sin),
                       hip.attention_bwd_packed(pm, o2, do, a2, p, KEY, B, S, nh, cos, sin, nkv=nh))


@pytest.mark.parametrize("nh,nkv,hd,p,S", CASES)
def test_packed_and_head_major_layouts_agree(nh, nkv, hd, p, S):
    c = _case(nh, nkv, hd, p, S)
    H, KV = nh * hd, nkv * hd
    o, aux = hip.attention_fwd(c["q"], c["k"], c["v"], p, KEY)
    dq, dk, dv = hip.attention_bwd(c["q"], c["k"], c["v"], o, c["do"], aux, p, KEY)
    pg, _ = _packed(c)
    cos, sin = hip.rope_tables(hd, S, device=DEV)
    og, auxg = hip.attention_fwd_packed(pg, B, S, nh, p, KEY, nkv=nkv)
    assert torch.equal(og, o) and torch.equal(auxg[0], aux[0])
    got = hip.attention_bwd_packed(pg, og, c["do"], auxg, p, KEY, B, S, nh, cos, sin, nkv=nkv)
    assert torch.equal(got[:, H + KV:], _rows(dv)), "dv"
    want = ref.rope_qkv_bwd(dq.float(), dk.float(), dv.float(), cos, sin)
    assert want.shape == got.shape
    scale = want.abs().max().item()
    _close(got, want, 1e-2 * max(1.0, scale), 1e-2, "dqkv packed")


# ------------------------------------------------------------------ 4. RoPE
@pytest.mark.parametrize("nh,nkv", HEADS + [(12, 4)])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_qk_inplace_gqa(nh, nkv, hd):
    torch.manual_seed(31 + nh)
    S = 300
    H, KV = nh * hd, nkv * hd
    qkv = torch.randn(B * S, H + 2 * KV, device=DEV).bfloat16()
    cos, sin = hip.rope_tables(hd, 1024, device=DEV)
    got = hip.rope_qk_inplace(qkv.clone(), B, S, nh, cos, sin, nkv=nkv)
    assert torch.equal(got[:, H + KV:], qkv[:, H + KV:]), "v block must be untouched"
    mha = torch.cat([qkv[:, :H], qkv[:, :H], qkv[:, :H]], dim=1).contiguous()  # the same q data, MHA layout
    assert torch.equal(got[:, :H], hip.rope_qk_inplace(mha, B, S, nh, cos, sin)[:, :H]), "q columns"
    want = ref.rope_qk_inplace(qkv.float().clone(), B, S, nh, cos, sin, nkv=nkv)
    _close(got, want, 2e-2, 1e-2, "rope in place")
    assert torch.equal(hip.rope_qk_inplace(qkv.clone(), B, S, nh, cos, sin, nkv=nkv), got)


# ------------------------------------------------------------------ 5. document mask
@pytest.mark.parametrize("hd,p", [(64, 0.0), (64, 0.1), (128, 0.0), (128, 0.1)])
def test_document_mask(hd, p):
    """(nh, nkv) = (4, 2), S = 200, separators {0, 1, 2, 150} in batch row 0: forward, dQ
    and dK/dV against the dense-mask reference, and check 1 with the DOC kernels."""
    nh, nkv, S = 4, 2, 200
    c = _case(nh, nkv, hd, p, S, True)
    o, aux = hip.attention_fwd(c["q"], c["k"], c["v"], p, KEY, **c["kw"])
    assert torch.isfinite(o.float()).all() and torch.isfinite(aux[0]).all()
    _close(aux[0], c["lse_ref"], 2e-3, 1e-4, "lse")
    _close(o, c["o_ref"], 2e-2, 2e-2, "o")
    plain = _case(nh, nkv, hd, p, S)
    assert not torch.equal(o, plain["o_m"]), "the mask must change the result"
    _check_dkdv(c, p)
    _check_fwd_dq_bitwise(c, nh, nkv, hd, p, S)


# ------------------------------------------------------------------ host-side validation
def test_host_validation():
    q = torch.randn(B, 4, 64, 64, device=DEV).bfloat16()
    k3 = torch.randn(B, 3, 64, 64, device=DEV).bfloat16()
    k2 = torch.randn(B, 2, 64, 64, device=DEV).bfloat16()
    with pytest.raises(ValueError, match="nkv"):
        hip.attention_fwd(q, k3, k3, 0.0, KEY)
    with pytest.raises(ValueError):
        hip.attention_fwd(q, k2, k2[:, :1], 0.0, KEY)
    with pytest.raises(ValueError):
        hip.attention_fwd(q, k2, k2, 0.0, KEY, nkv=4)
    with pytest.raises(TypeError):
        hip.attention_fwd(q, k2, k2.half(), 0.0, KEY)
    with pytest.raises(NotImplementedError):
        hip.attention_fwd(q.float(), k2.float(), k2.float(), 0.0, KEY)
    qkv = torch.randn(B * 64, (4 + 2 * 2) * 64, device=DEV).bfloat16()
    cos, sin = hip.rope_tables(64, 64, device=DEV)
    with pytest.raises(ValueError, match="nkv"):
        hip.attention_fwd_packed(qkv, B, 64, 4, 0.0, KEY, nkv=3)
    with pytest.raises(ValueError):
        hip.attention_fwd_packed(qkv, B, 64, 4, 0.0, KEY, nkv=1)  # the width does not fit
    with pytest.raises(ValueError):
        hip.rope_qk_inplace(qkv, B, 64, 4, cos, sin, nkv=4)
    with pytest.raises(NotImplementedError):
        hip.rope_qkv_fwd(qkv, B, 64, 4, cos, sin, nkv=2)
    with pytest.raises(NotImplementedError):
        hip.attention_fwd_packed(qkv.float(), B, 64, 4, 0.0, KEY, nkv=2)


# ------------------------------------------------------------------ 6. engine
def _cfg(dropout=0.1, **kw):
    d = dict(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=2, max_seq_len=128,
             dropout=dropout, attention_dropout=dropout)
    d.update(kw)
    return GPTConfig(**d)


def _grads(m):
    return {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()


def _hip_vs_reference_engine(cfg, seed):
    torch.manual_seed(seed)
    base = GPT(cfg).to(DEV)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    e1 = m1.enable_engine(seed=5)
    m2.enable_engine(seed=5, ops=ops.CPU_OPS)  # reference ops, same bf16 weights, activations and dropout
    assert e1.gqa and e1.ops.backend == "hip" and e1.packed_qkv
    ids = torch.randint(0, 1000, (2, cfg.max_seq_len), device=DEV)
    _, l1 = m1(ids, labels=ids)
    (l1 / 2).backward()
    _, l2 = m2(ids, labels=ids)
    (l2 / 2).backward()
    assert abs(l1.item() - l2.item()) < 2e-2 * abs(l2.item())
    g1, g2 = _grads(m1), _grads(m2)
    assert g1["layers.0.attention.k_proj.weight"].shape == (cfg.kv_size, cfg.hidden_size)
    for n in g1:
        assert _cos(g1[n], g2[n]) > 0.99, n
        r = g1[n].norm() / g2[n].norm()
        assert 0.95 < r.item() < 1.05, (n, r.item())


def test_engine_hip_vs_reference_ops():
    _hip_vs_reference_engine(_cfg(0.1), 0)


def test_engine_fallback_shapes_vs_reference_ops():
    """hidden 320, 5 heads, 1 kv head (G = 5): the QKV width 448 fits no 128-column hand
    tile, so the GEMMs go through the race's fallback."""
    cfg = _cfg(0.1, hidden_size=320, num_heads=5, num_kv_heads=1)
    assert cfg.hidden_size + 2 * cfg.kv_size == 448
    _hip_vs_reference_engine(cfg, 1)


def test_engine_recompute_is_bit_identical():
    torch.manual_seed(2)
    base = GPT(_cfg(0.1)).to(DEV)
    ids = torch.randint(0, 1000, (2, 128), device=DEV)
    res = []
    for ac in (False, True):
        m = copy.deepcopy(base)
        m.enable_engine(seed=7)
        m.gradient_checkpointing = ac
        _, loss = m(ids, labels=ids)
        loss.backward()
        res.append((loss.item(), _grads(m)))
    assert res[0][0] == res[1][0]
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n


@pytest.mark.parametrize("recompute", [False, True])
def test_train_window_matches_sequential_bit_for_bit(recompute):
    from distributed_llm_trainer_amd.models.engine import shift_targets
    torch.manual_seed(5)
    base = GPT(_cfg(0.1)).to(DEV)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    e1, e2 = m1.enable_engine(seed=9), m2.enable_engine(seed=9)
    m1.gradient_checkpointing = m2.gradient_checkpointing = recompute
    GA = 4
    data = torch.randint(0, 1000, (GA, 2, 128), device=DEV)
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
    data = torch.randint(0, 1000, (8, 128), device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    res = []
    for _ in range(2):
        torch.manual_seed(3)
        tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=4, warmup_steps=1, learning_rate=1e-3,
                            micro_step_fusion=1)
        tr = DistributedTrainer(_cfg(0.1), tc)
        assert tr.use_engine and tr.model.engine.gqa
        losses = [tr.train_step({"input_ids": data})["loss"] for _ in range(3)]
        res.append((losses, tr.flat_params().detach().clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]), (res[0][1] - res[1][1]).abs().max().item()


# ------------------------------------------------------------------ 7. unsupported routes
def test_unsupported_routes_refuse_at_enable_engine():
    m = GPT(_cfg(0.0)).to(DEV)
    with pytest.raises(NotImplementedError, match="fp32"):
        m.enable_engine(act_dtype=torch.float32)
    assert m.engine is None and m.store is None
    m96 = GPT(_cfg(0.0, hidden_size=384)).to(DEV)  # head_dim 96: the zero-padded route
    assert m96.config.head_dim == 96
    with pytest.raises(NotImplementedError, match="head_dim"):
        m96.enable_engine()
    with pytest.raises(NotImplementedError):
        ops.check_attention_features(DEV, 192, torch.bfloat16, {"gqa"})  # the GEMM-formulated route
    ops.check_attention_features(DEV, 64, torch.float16, {"gqa"})
    ops.check_attention_features(DEV, 128, torch.bfloat16, {"gqa"})
    GPT(_cfg(0.0, num_kv_heads=None, hidden_size=384)).to(DEV).enable_engine()  # MHA still takes head_dim 96


# ------------------------------------------------------------------ 8. generation
def test_kv_cached_generate_matches_the_eager_re_forward():
    from distributed_llm_trainer_amd.eval.decode import KVCache, _fused_ok
    torch.manual_seed(3)
    m = GPT(_cfg(0.0)).to(DEV)
    eng = m.enable_engine()
    assert not _fused_ok(m, 1) and not _fused_ok(m, 4)
    cache = KVCache(m.config, 1, DEV, eng.act_dtype)
    assert cache.k[0].shape == (1, 2, 128, 64) and cache.v[0].shape == (1, 2, 128, 64)
    ids = torch.randint(0, 1000, (1, 17), device=DEV)
    g = m.generate(ids, max_new_tokens=4, top_k=1)
    assert g.shape == (1, 21)
    for t in range(4):  # greedy KV-cached decode == argmax of a full re-forward at each step
        with torch.no_grad():
            lg, _ = m(g[:, :17 + t])
        assert lg[0, -1].argmax().item() == g[0, 17 + t].item() or \
            (lg[0, -1].max() - lg[0, -1][g[0, 17 + t]]).abs().item() < 0.05
