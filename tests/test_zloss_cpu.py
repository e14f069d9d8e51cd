"""The auxiliary z-loss without a GPU: the fp64 reference and tolerances of tests/zloss_ref.py (an
fp32 model of the kernel lies inside them, every planted defect outside), the reference op, the
eager model, the engine on the reference ops, the trainers and their CLIs."""
import copy
import importlib
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.models.engine import shift_targets
from distributed_llm_trainer_amd.ops import reference as ref, rng
from tests import zloss_ref as Z
from tests.dist_utils import run_multiprocess

BF, HF, F32, F64 = Z.BF, Z.HF, Z.F32, Z.F64
BASE_CASES = Z.CE_CASES + Z.CE_CASES_512 + Z.CE_CASES_PLAIN


# ------------------------------------------------------------------ the reference, a model, defects
def _zce32(logits, targets, V, n_valid, gscale, c):
    """The kernel in fp32, in its order: lse, zf = fma(2 c, lse, 1), the row factor inv_n * zf, the
    target patched as (p * zf - 1) * inv_n, the gradient rounded to the logits' format."""
    x = logits.float()[:, :V]
    lse = torch.logsumexp(x, dim=1, keepdim=True)
    valid = (targets != -100).unsqueeze(1)
    tgt = targets.clamp(min=0).unsqueeze(1)
    loss = torch.where(valid, lse - x.gather(1, tgt), torch.zeros_like(lse)).squeeze(1)
    c2 = np.float32(2.0) * np.float32(c)
    zf = (float(c2) * lse.double() + 1.0).float()  # one rounding, as the fma
    inv_n = (valid * (np.float32(gscale) / np.float32(max(n_valid, 1)))).float()
    p = torch.exp(x - lse)
    g = p * (inv_n * zf)
    pt = p.gather(1, tgt)
    g.scatter_(1, tgt, torch.where(valid, (pt * zf - 1.0) * inv_n, torch.zeros_like(pt)))
    out = torch.zeros_like(logits)
    out[:, :V] = g.to(logits.dtype)
    z = torch.where(valid, lse * lse, torch.zeros_like(lse)).squeeze(1)
    return loss, z, out


def _inside(name, out, chk, dt):
    bad = Z.miss(out, chk, dt)
    err = (out.double() - chk.ref).abs()
    assert not bad.any(), f"{name}: err/tol = {torch.where(chk.tol > 0, err / chk.tol, err)[bad].max().item():.3f}"


@pytest.mark.parametrize("case", BASE_CASES, ids=lambda c: c[0])
def test_kernel_model_inside_and_planted_defects_outside(case):
    _, dt, Vp, V, kind, nv_mode, _ = case
    inp = Z.ce_inputs(dt, Vp, V, kind)
    nv = Z.ce_n_valid(inp, nv_mode)
    live = inp.targets != -100
    M = inp.targets.numel()
    for c in Z.Z_COEFS:
        for g in Z.Z_SCALES:
            tag = f"c={c:g} g={g:g}"
            for wide in (True, False):
                r = Z.zce_ref(inp.logits, inp.targets, V, nv, g, c, wide=wide)
                loss32, z32, grad32 = _zce32(inp.logits, inp.targets, V, nv, g, c)
                _inside(tag + " fp32 loss", loss32, r.loss, F32)
                _inside(tag + " fp32 z_rows", z32, r.z, F32)
                _inside(tag + " fp32 grad", grad32, r.grad, dt)
            r = Z.zce_ref(inp.logits, inp.targets, V, nv, g, c)
            assert not r.z.ref[~live].any() and not r.z.tol[~live].any()
            assert not r.grad.ref[~live].any() and not r.grad.tol[~live].any()
            assert not r.grad.ref[:, V:].any() and not r.grad.tol[:, V:].any()

            def bad(defect):
                b = Z.zce_ref(inp.logits, inp.targets, V, nv, g, c, defect=defect)
                return (Z.miss(b.z.ref.float(), r.z, F32),
                        Z.miss(Z.round_to(b.grad.ref, dt), r.grad, dt))

            # fp16 at the ceiling of the format with c = 1e-2 and the loss scale: the true gradient is
            # infinite wherever it is not zero, and so is a wrong factor's; such a row shows a defect
            # of the factor at grad_scale 1 only
            fin = live & (r.grad.ref.abs().amax(dim=1) < Z.overflow_at(dt) / 4)
            assert fin.any() or (kind == "ceil" and g != 1.0)
            if fin.any():
                assert bad("no_z_grad")[1][fin].any(), f"{tag}: the z term missing from the gradient stays inside"
                assert bad("zf_half")[1][fin].any(), f"{tag}: 1 + c z stays inside"
                assert bad("patch_times_zf")[1][fin].any(), f"{tag}: the target patched as (p - 1) zf stays inside"
                if g != 1.0:
                    assert bad("z_unscaled")[1][fin].any(), f"{tag}: a z gradient without grad_scale stays inside"
                if max(nv, 1) != M:
                    assert bad("z_norm_M")[1][fin].any(), f"{tag}: the z term normalised by M stays inside"
            bz, bg = bad("ignored_row_z")
            assert bz[~live].all() and bg[~live].any(dim=1).all(), f"{tag}: an ignored row's z term stays inside"
            assert bad("z_rows_lse")[0][live].all(), f"{tag}: z_rows = lse stays inside"
            low = live & (inp.logits.float()[:, :V].amax(dim=1) < 30)
            if V < Vp and kind != "ceil":  # the padding holds +40: it shows on every row whose maximum is lower
                bz, bg = bad("lse_over_padding")
                assert low.any() and bz[low].all() and bg[low].any(dim=1).all(), f"{tag}: lse over the padding stays inside"
            neg = live & (r.zf < 0)
            if neg.any():
                for d in ("zf_abs", "zf_clamp"):
                    assert bad(d)[1][neg].any(dim=1).all(), f"{tag}: {d} stays inside"


def test_cases_hold_what_the_gpu_tests_need():
    cs = Z.Z_CASES
    assert {(c[2], c[3]) for c in cs if c[4] == "base"} == set(Z.CE_SHAPES)
    for dt, kind in ((BF, "base"), (HF, "base"), (BF, "large"), (HF, "ceil")):
        got = {(c[7], c[6]) for c in cs if c[1] == dt and c[4] == kind}
        assert got == {(c, g) for c in Z.Z_COEFS for g in Z.Z_SCALES}, (dt, kind)
    assert {c[5] for c in cs} == set(Z.CE_NV_MODES)
    for dt, seen in Z.z_variants_reached().items():
        assert seen == set(Z.CE_VARIANTS), (dt, sorted(set(Z.CE_VARIANTS) - seen))
    assert all(Z.ce_inputs(c[1], c[2], c[3], c[4]).targets.numel() <= 64 for c in cs)
    # c = 1e-2 drives zf negative on the large rows whose lse is about -64
    name, dt, Vp, V, kind, nv_mode, g, c = [x for x in cs if x[4] == "large" and x[7] == 1e-2][0]
    inp = Z.ce_inputs(dt, Vp, V, kind)
    zf = Z.zce_ref(inp.logits, inp.targets, V, Z.ce_n_valid(inp, nv_mode), g, c).zf
    assert (zf < -0.2).any() and (zf > 2.0).any()


# ------------------------------------------------------------------ the reference op
@pytest.mark.parametrize("dt", [F32, BF])
@pytest.mark.parametrize("c", [1e-4, 1e-2, 0.5])
def test_reference_op_against_fp64_autograd(dt, c):
    g_ = torch.Generator().manual_seed(11)
    M, Vp, V = 9, 72, 67
    lg = (torch.randn(M, Vp, generator=g_) * 3).to(dt)
    lg[:, V:] = 40.0
    tg = torch.randint(0, V, (M,), generator=g_)
    tg[[2, 8]] = -100
    nv, gs = int((tg != -100).sum()), 8.0
    x = lg.double()[:, :V].clone().requires_grad_(True)
    z = torch.logsumexp(x, dim=1)
    live = tg != -100
    ce_rows = F.cross_entropy(x, tg, ignore_index=-100, reduction="none")
    ((ce_rows.sum() + c * (z[live] ** 2).sum()) / nv * gs).backward()
    buf = lg.clone()
    z_rows = torch.full((M,), -7.0)
    rows = ref.cross_entropy_fwd_bwd(buf, tg, V, torch.tensor(nv), gs, c, z_rows)
    tol = dict(rtol=1e-5, atol=1e-5) if dt == F32 else dict(rtol=2.0 ** -7, atol=1e-6)
    torch.testing.assert_close(rows.double(), ce_rows.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(z_rows.double(), torch.where(live, z.detach() ** 2, torch.zeros_like(z)), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(buf.double()[:, :V], x.grad, **tol)
    assert not buf[:, V:].any() and not buf[~live].any() and not z_rows[~live].any()
    # without the two arguments: the op it was, bit for bit; c = 0 with z_rows: the same gradient
    b0, b1 = lg.clone(), lg.clone()
    r0 = ref.cross_entropy_fwd_bwd(b0, tg, V, torch.tensor(nv), gs)
    r1 = ref.cross_entropy_fwd_bwd(b1, tg, V, torch.tensor(nv), gs, 0.0, torch.empty(M))
    assert torch.equal(r0, rows) and torch.equal(r0, r1) and torch.equal(b0, b1)


def test_reference_op_validates_z_rows():
    lg, tg, nv = torch.zeros(4, 16), torch.zeros(4, dtype=torch.int64), torch.tensor(4)
    with pytest.raises(TypeError):
        ref.cross_entropy_fwd_bwd(lg, tg, 16, nv, 1.0, 1e-4)                                   # no z_rows
    with pytest.raises(TypeError):
        ref.cross_entropy_fwd_bwd(lg, tg, 16, nv, 1.0, 1e-4, torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError):
        ref.cross_entropy_fwd_bwd(lg, tg, 16, nv, 1.0, 1e-4, torch.zeros(5))
    with pytest.raises(ValueError):
        ref.cross_entropy_fwd_bwd(lg, tg, 16, nv, 1.0, 1e-4, torch.zeros(4, 1))


# ------------------------------------------------------------------ the models
TINY = dict(vocab_size=256, hidden_size=64, num_layers=2, num_heads=4, max_seq_len=32, dropout=0.0, attention_dropout=0.0)
FEATURES = {"num_kv_heads": 2, "qk_norm": True, "sliding_window": 5, "sliding_window_pattern": 2, "attention_sinks": True}
C = 1e-2


def tiny(**kw):
    d = dict(TINY)
    d.update(kw)
    return GPTConfig(**d)


def _randomise(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in m.layers:
            if m.config.attention_sinks:
                layer.attention.sinks.copy_(1.5 * torch.randn(layer.attention.sinks.shape, generator=g))
    return m


def _labels(ids, seed=1):
    """ids with a few positions ignored, a different count in every row."""
    lab = ids.clone()
    g = torch.Generator().manual_seed(seed)
    for b in range(ids.shape[0]):
        lab[b, torch.randperm(ids.shape[1], generator=g)[:2 + 3 * b]] = -100
    return lab


def _rot(x, cos, sin):
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def _dense_logits(m, ids, seed=0, micro=0, p_attn=0.0, p_hidden=0.0):
    """The model as an independent dense formula over ``m``'s parameters (plain autograd), with
    the engine's counter-hash dropout masks: [B * S, V] logits."""
    cfg = m.config
    B, S = ids.shape
    nh, nkv, hd, H = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.hidden_size
    pos = torch.arange(S)
    causal = (pos.view(1, 1, 1, S) <= pos.view(1, 1, S, 1)).expand(B, 1, S, S)
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
        if cfg.attention_sinks:
            s = torch.cat([s, at.sinks.view(1, nh, 1, 1).expand(B, nh, S, 1)], dim=-1)
        pr = torch.softmax(s, dim=-1)[..., :S]
        if p_attn > 0:
            pr = pr * rng.attn_keep_mask(B * nh, S, S, k_attn, p_attn).view(B, nh, S, S) / (1.0 - p_attn)
        a = (pr @ v[:, idx]).transpose(1, 2).reshape(B * S, H) @ at.o_proj.weight.t()
        x = x + drop(a, k_resid, p_hidden)
        n2 = norm(x, layer.post_attention_layernorm.weight)
        mlp = layer.mlp
        d = (F.silu(n2 @ mlp.gate_proj.weight.t()) * (n2 @ mlp.up_proj.weight.t())) @ mlp.down_proj.weight.t()
        x = x + drop(d, k_mlp, p_hidden)
    return norm(x, m.norm.weight) @ m.embed_tokens.weight.t()


def _dense_loss(m, ids, labels, c, **kw):
    """(ce, z_term): F.cross_entropy and c * mean over the valid targets of logsumexp^2, written
    independently of the model's own lines."""
    logits = _dense_logits(m, ids, **kw)
    tg = shift_targets(labels)
    live = tg != -100
    n = max(int(live.sum()), 1)
    lse = torch.log(torch.exp(logits - logits.amax(-1, keepdim=True)).sum(-1)) + logits.amax(-1)
    picked = logits.gather(1, tg.clamp(min=0).unsqueeze(1)).squeeze(1)
    ce = ((lse - picked) * live).sum() / n
    return ce, c * ((lse * lse) * live).sum() / n


def _close_grads(m1, m2, atol=1e-6, rtol=1e-4):
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=atol, rtol=rtol), (n, (p1.grad - p2.grad).abs().max())


@pytest.mark.parametrize("kw", [{}, FEATURES], ids=["plain", "features"])
def test_eager_model_matches_the_dense_formula(kw):
    torch.manual_seed(0)
    m = _randomise(GPT(tiny(**kw)))
    m2 = copy.deepcopy(m)
    m.set_z_loss(C)
    ids = torch.randint(0, 256, (3, 32))
    lab = _labels(ids)
    _, l1 = m(ids, labels=lab)
    l1.backward()
    ce, zt = _dense_loss(m2, ids, lab, C)
    (ce + zt).backward()
    assert abs(l1.item() - (ce + zt).item()) < 1e-5 and zt.item() > 1e-3 * C
    pce, pz = m.last_loss_parts
    assert not pce.requires_grad and abs(pce.item() - ce.item()) < 1e-5 and abs(pz.item() - zt.item()) < 1e-6
    assert abs((pce + pz).item() - l1.item()) <= 2.0 ** -22 * abs(l1.item())
    _close_grads(m, m2)
    # the term is live: the gradient without it is another one
    m3 = copy.deepcopy(m2)
    m3.zero_grad()
    m3(ids, labels=lab)[1].backward()
    assert (m3.embed_tokens.weight.grad - m.embed_tokens.weight.grad).abs().max() > 1e-6


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kw", [{}, FEATURES], ids=["plain", "features"])
def test_engine_matches_autograd_with_the_same_dropout_masks(kw, p, recompute):
    torch.manual_seed(3)
    m1 = _randomise(GPT(tiny(dropout=p, attention_dropout=p, **kw)))
    m2 = copy.deepcopy(m1)
    ids = torch.randint(1, 256, (3, 32))
    lab = _labels(ids)
    ce, zt = _dense_loss(m1, ids, lab, C, seed=21, micro=0, p_attn=p, p_hidden=p)
    (ce + zt).backward()
    m2.set_z_loss(C)  # before the engine exists: it must reach it
    eng = m2.enable_engine(seed=21)
    assert eng.z_loss == C
    m2.gradient_checkpointing = recompute
    m2.train()
    _, l2 = m2(ids, labels=lab)
    l2.backward()
    assert abs((ce + zt).item() - l2.item()) < 1e-5
    pce, pz = m2.last_loss_parts
    assert abs(pce.item() - ce.item()) < 1e-5 and abs(pz.item() - zt.item()) < 1e-6
    assert abs((pce + pz).item() - l2.item()) <= 2.0 ** -22 * abs(l2.item())
    _close_grads(m1, m2)


def test_engine_gradient_by_finite_differences():
    torch.manual_seed(7)
    c = 0.05
    m = GPT(tiny(initializer_range=0.2))
    m0 = copy.deepcopy(m)  # the same weights without the term: its share of the slope must be visible
    m.set_z_loss(c)
    m.enable_engine()
    m0.enable_engine()
    ids = torch.randint(0, 256, (3, 32))
    lab = _labels(ids)
    m.train()
    _, loss = m(ids, labels=lab)
    loss.backward()
    w = m.embed_tokens.weight
    g = w.grad.clone()
    d = g / g.norm()
    h = 0.05
    ls = []
    for sgn in (1.0, -1.0):
        with torch.no_grad():
            w.add_(sgn * h * d)
            m.store.refresh_shadow()
            ls.append(m(ids, labels=lab)[1].item())
            w.sub_(sgn * h * d)
    fd = (ls[0] - ls[1]) / (2 * h)
    # central difference: O(h^2) truncation (charged 2 % of the slope) + the fp32 loss's own error,
    # a few tens of ulps of a value under 32 (2^-19), over 2h
    tol = 2e-2 * abs(fd) + 40 * 2.0 ** -19 / (2 * h)
    assert abs(fd - g.norm().item()) <= tol, (fd, g.norm().item(), tol)
    m0.train()
    m0(ids, labels=lab)[1].backward()
    assert abs((m0.embed_tokens.weight.grad * d).sum().item() - g.norm().item()) > 2 * tol, "the z term's slope is under the noise"


def test_fused_micro_steps_equal_the_mean_of_separate_ones():
    torch.manual_seed(5)
    Fs = 3
    m1 = GPT(tiny())
    m2 = copy.deepcopy(m1)
    for m in (m1, m2):
        m.set_z_loss(C)
        m.enable_engine(seed=5)
        m.train()
    ids = torch.randint(0, 256, (2 * Fs, 32))
    lab = ids.clone()
    lab[0:2, 5:] = -100     # 2 x 4 valid targets in the first segment
    lab[2:4, 20:] = -100    # 2 x 19 in the second, 2 x 31 in the third
    parts = []
    for k in range(Fs):
        _, loss = m1(ids[2 * k:2 * k + 2], labels=lab[2 * k:2 * k + 2])
        (loss / Fs).backward()
        parts.append(m1.last_loss_parts)
    m2.engine.set_loss_segments(Fs)
    _, fused = m2(ids, labels=lab)
    fused.backward()
    fce, fz = m2.last_loss_parts
    assert abs(fce.item() - sum(p[0].item() for p in parts) / Fs) < 1e-5
    assert abs(fz.item() - sum(p[1].item() for p in parts) / Fs) < 1e-6
    zs = [p[1].item() for p in parts]
    assert max(zs) - min(zs) > 1e-6, "the segments' z terms coincide: the test cannot tell the normalisers apart"
    _close_grads(m1, m2)


@pytest.mark.parametrize("segments", [1, 2])
def test_chunked_head_equals_the_single_call(segments):
    torch.manual_seed(9)
    GA = 2
    m1 = GPT(tiny(dropout=0.1, attention_dropout=0.1))
    m2 = copy.deepcopy(m1)
    data = [torch.randint(0, 256, (4, 32)) for _ in range(GA)]
    labs = [_labels(d, seed=j) for j, d in enumerate(data)]
    outs = []
    for m, chunks in ((m1, 0), (m2, 3)):
        m.set_z_loss(C)
        eng = m.enable_engine(seed=9)
        eng.head_chunks = chunks
        eng.set_loss_segments(segments)
        m.train()
        losses = eng.train_window(data, [shift_targets(x) for x in labs], torch.full((), 1.0 / GA))
        outs.append((losses, eng.window_loss_parts))
        assert len(eng.window_loss_parts) == GA
    for j in range(GA):
        assert abs(outs[0][0][j].item() - outs[1][0][j].item()) < 1e-5
        for a, b in zip(outs[0][1][j], outs[1][1][j]):
            assert abs(a.item() - b.item()) < 1e-5
        ce, zt = outs[1][1][j]
        assert zt.item() > 0 and abs((ce + zt).item() - outs[1][0][j].item()) <= 2.0 ** -22 * outs[1][0][j].item()
    _close_grads(m1, m2)


def test_train_window_matches_sequential_bit_for_bit():
    torch.manual_seed(5)
    GA = 2
    m1 = GPT(tiny(dropout=0.1, attention_dropout=0.1))
    m2 = copy.deepcopy(m1)
    for m in (m1, m2):
        m.set_z_loss(C)
        m.enable_engine(seed=5)
        m.train()
    data = [torch.randint(0, 256, (2, 32)) for _ in range(GA)]
    seq = []
    for j in range(GA):
        m1.engine.set_accumulation(j, GA, defer=True)
        _, loss = m1(data[j], labels=data[j])
        (loss / GA).backward()
        seq.append((loss.detach(), m1.last_loss_parts))
    win = m2.engine.train_window(data, [shift_targets(d) for d in data], torch.full((), 1.0 / GA))
    for j in range(GA):
        assert torch.equal(seq[j][0], win[j])
        assert all(torch.equal(a, b) for a, b in zip(seq[j][1], m2.engine.window_loss_parts[j]))
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p1.grad, p2.grad), n


@pytest.mark.parametrize("engine", [False, True])
def test_evaluation_ignores_the_coefficient(engine):
    torch.manual_seed(1)
    m = GPT(tiny())
    if engine:
        m.enable_engine()
    ids = torch.randint(0, 256, (2, 32))
    s0, n0 = m.eval_loss_sum(ids)
    e0 = m.eval_loss(ids)
    m.set_z_loss(0.5)
    s1, n1 = m.eval_loss_sum(ids)
    assert torch.equal(s0, s1) and torch.equal(n0, n1) and torch.equal(e0, m.eval_loss(ids))
    m.train()
    assert m(ids, labels=ids)[1].item() > e0.item() + 1.0  # while the training objective carries the term


@pytest.mark.parametrize("engine", [False, True])
def test_zero_coefficient_is_the_model_that_never_heard_of_it(engine):
    torch.manual_seed(2)
    m1 = GPT(tiny(dropout=0.1, attention_dropout=0.1))
    m2 = copy.deepcopy(m1)
    m2.set_z_loss(0.3)
    if engine:
        m1.enable_engine(seed=4)
        m2.enable_engine(seed=4)
    m2.set_z_loss(0.0)
    ids = torch.randint(0, 256, (3, 32))
    lab = _labels(ids)
    outs = []
    for m in (m1, m2):
        m.train()
        torch.manual_seed(77)  # the eager model's dropout
        _, loss = m(ids, labels=lab)
        loss.backward()
        outs.append(loss.detach())
    assert torch.equal(outs[0], outs[1])
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p1.grad, p2.grad), n
    ce, zt = m2.last_loss_parts
    assert torch.equal(ce, outs[1]) and zt.item() == 0.0


def test_coefficient_validation_and_the_config_stays_out_of_it():
    m = GPT(tiny())
    for bad in (-1e-4, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            m.set_z_loss(bad)
    assert m.z_loss == 0.0
    eng = m.enable_engine()
    with pytest.raises(ValueError):
        eng.set_z_loss(-1.0)
    m.set_z_loss(1e-4)
    assert eng.z_loss == 1e-4 and "z_loss" not in m.config.to_dict() and not hasattr(m.config, "z_loss")
    from distributed_llm_trainer_amd.training.configs import FSDPTrainingConfig, TrainingConfig
    assert TrainingConfig().z_loss == 0.0 and FSDPTrainingConfig().z_loss == 0.0
    for cls in (TrainingConfig, FSDPTrainingConfig):
        for bad in (-1e-4, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                cls(z_loss=bad)


# ------------------------------------------------------------------ distributed
DIST = dict(vocab_size=384, hidden_size=96, num_layers=2, num_heads=6, num_kv_heads=2, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0)
ZD = 2e-2


def _data(step, rank, n=8, seq=32, vocab=384):
    g = torch.Generator().manual_seed(1000 * step + rank)
    return torch.randint(0, vocab, (n, seq), generator=g)


def _ddp_trainer(GA, z=ZD):
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=GA, warmup_steps=1, max_steps=100,
                        learning_rate=1e-2, bucket_cap_mb=0.05, micro_step_fusion=1, z_loss=z)
    return DistributedTrainer(GPTConfig(**DIST), tc)


def _ddp_worker(rank, world, steps):
    tr = _ddp_trainer(2)
    for s in range(steps):
        out = tr.train_step({"input_ids": _data(s, rank, n=4)})
    return tr.flat_params().clone(), out


def test_ddp_matches_single_process():
    (p0, o0), (p1, _) = run_multiprocess(_ddp_worker, world=2, args=(3,))
    assert torch.equal(p0, p1), "ranks diverged"
    tr = _ddp_trainer(4)
    for s in range(3):
        out = tr.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    assert torch.allclose(p0, tr.flat_params(), atol=2e-5, rtol=1e-4), (p0 - tr.flat_params()).abs().max()
    assert out["z_loss"] > 0 and abs(out["ce_loss"] + out["z_loss"] - out["loss"]) < 1e-5
    assert abs(o0["loss_global"] - out["loss"]) < 1e-4
    off = _ddp_trainer(4, z=0.0)
    for s in range(3):
        out0 = off.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    assert "z_loss" not in out0 and "ce_loss" not in out0
    assert (off.flat_params() - tr.flat_params()).abs().max() > 1e-4, "the coefficient changed nothing"


def _fsdp_trainer(GA, ac, z=ZD):
    from distributed_llm_trainer_amd.training.configs import FSDPConfig, FSDPTrainingConfig
    from distributed_llm_trainer_amd.training.fsdp_trainer import FSDPTrainer
    tc = FSDPTrainingConfig(batch_size=2, gradient_accumulation_steps=GA, warmup_steps=1, max_steps=100,
                            learning_rate=1e-2, micro_step_fusion=1, z_loss=z)
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
        out = tr.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    assert out["z_loss"] > 0 and abs(out["ce_loss"] + out["z_loss"] - out["loss"]) < 1e-5
    ref_sd = {k: v for k, v in tr._full_state().items() if "rotary" not in k}
    for k in ref_sd:
        assert torch.equal(outs[0][k], outs[1][k]), f"{k}: ranks diverged"
        assert torch.allclose(outs[0][k], ref_sd[k], atol=3e-5, rtol=1e-4), (k, (outs[0][k] - ref_sd[k]).abs().max())
    off = _fsdp_trainer(4, False, z=0.0)
    for s in range(3):
        off.train_step({"input_ids": torch.cat([_data(s, r, n=4) for r in range(2)], dim=0)})
    sd0 = off._full_state()
    assert max((sd0[k] - ref_sd[k]).abs().max().item() for k in ref_sd) > 1e-4, "the coefficient changed nothing"


# ------------------------------------------------------------------ CLI, YAML, logs
def _yaml(tmp_path, z):
    p = tmp_path / "m.yaml"
    extra = f"  z_loss: {z}\n" if z is not None else ""
    p.write_text("model:\n  hidden_size: 64\n  num_layers: 1\n  num_heads: 4\n  vocab_size: 128\n  max_seq_len: 16\n"
                 "training:\n  log_interval: 1\n  warmup_steps: 0\n" + extra)
    return str(p)


def _main(trainer, tmp_path, argv, z_yaml=None, steps=1):
    mod = importlib.import_module(f"distributed_llm_trainer_amd.training.{trainer}")
    env_before = os.environ.get("DLT_DUMMY_BATCHES")
    os.environ["DLT_DUMMY_BATCHES"] = "2"
    try:
        return mod.main(["--config", _yaml(tmp_path, z_yaml), "--batch_size", "1", "--max_steps", str(steps),
                         "--gradient_accumulation_steps", "2", "--no_final_save", "--checkpoint_dir", str(tmp_path / "ck"),
                         *argv])
    finally:
        if env_before is None:
            os.environ.pop("DLT_DUMMY_BATCHES", None)
        else:
            os.environ["DLT_DUMMY_BATCHES"] = env_before


@pytest.mark.parametrize("trainer", ["ddp_trainer", "fsdp_trainer"])
def test_cli_flag_precedence_and_rejected_values(tmp_path, trainer):
    """CLI > YAML > default, and the value reaches the model and its engine."""
    mod = importlib.import_module(f"distributed_llm_trainer_amd.training.{trainer}")
    assert mod.build_parser().parse_args([]).z_loss is None

    def run(argv, z_yaml=None):
        tr = _main(trainer, tmp_path, argv, z_yaml)
        assert tr.model.z_loss == tr.training_config.z_loss
        assert tr.model.engine is None or tr.model.engine.z_loss == tr.model.z_loss
        return tr.training_config.z_loss

    assert run([]) == 0.0                               # default
    assert run([], "3e-4") == 3e-4                      # YAML over the default
    assert run(["--z_loss", "1e-4"], "3e-4") == 1e-4    # CLI over YAML
    assert run(["--z_loss", "0"], "3e-4") == 0.0        # ... an explicit 0 too
    for bad in ("-1e-4", "nan", "inf"):
        with pytest.raises(ValueError):
            run([f"--z_loss={bad}"])
    with pytest.raises(ValueError):
        run([], "-0.5")


LINE = {"ddp_trainer": r"^Step +\d+ \| Loss: \d+\.\d{4} \| LR: \d\.\d\de[-+]\d\d \| Tokens/sec: [\d,]+",
        "fsdp_trainer": r"^Step +\d+ \| Loss: \d+\.\d{4} \| LR: \d\.\d\de[-+]\d\d \| Tokens/s: [\d,]+ \| Mem: \d+\.\dGB"}
KEYS = ["step", "loss", "lr", "tokens", "elapsed_s", "tokens_per_sec"]


@pytest.mark.parametrize("trainer", ["ddp_trainer", "fsdp_trainer"])
def test_log_line_and_jsonl_record(tmp_path, capsys, trainer):
    recs, lines = {}, {}
    for name, argv in (("off", []), ("on", ["--z_loss", "1e-3"])):
        path = tmp_path / f"{name}.jsonl"
        _main(trainer, tmp_path, ["--metrics_jsonl", str(path), *argv], steps=2)
        lines[name] = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Step ")]
        recs[name] = [json.loads(ln) for ln in path.read_text().splitlines() if "summary" not in ln]
        assert len(lines[name]) == 2 and len(recs[name]) == 2
    for ln in lines["off"]:
        assert re.match(LINE[trainer] + "$", ln), ln
    for r in recs["off"]:
        assert "ce_loss" not in r and "z_loss" not in r and [k for k in r if k in KEYS] == KEYS
    for ln in lines["on"]:
        assert re.match(LINE[trainer] + r" \| Z loss: \d+\.\d{6}$", ln), ln
    for r in recs["on"]:
        assert r["z_loss"] > 0 and abs(r["ce_loss"] + r["z_loss"] - r["loss"]) < 1e-5
        assert [k for k in r if k not in ("ce_loss", "z_loss")] == list(recs["off"][0])
    # the first step runs on the same weights: its cross-entropy part is the run's without the term
    assert abs(recs["on"][0]["ce_loss"] - recs["off"][0]["loss"]) < 1e-5


def test_one_step_with_the_flag_changes_the_parameters(tmp_path):
    p = {}
    for z in ("0", "1e-3"):
        tr = _main("ddp_trainer", tmp_path, ["--z_loss", z], steps=1)
        p[z] = tr.flat_params().clone()
        assert tr.global_step == 1
    assert (p["0"] - p["1e-3"]).abs().max() > 0
