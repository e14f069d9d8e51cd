"""Self-checks of tests/decode_gqa_ref.py and of the host-side choices of the grouped-query
decode step, runnable without a GPU: at exactly the inputs test_decode_gqa_gpu.py uses, the
tolerances admit an honest fp32 implementation of the split kernel and reject every planted
defect; ``_fused_kind`` on stub configs, ``dec_attn_chunk`` and ``DLT_DECODE_KV_SPLITS``."""
import functools
import types

import pytest
import torch

from distributed_llm_trainer_amd.eval import decode as D
from distributed_llm_trainer_amd.ops import hip
from tests import decode_gqa_ref as G
from tests import decode_ref as R
from tests.test_decode_kernels_cpu import _assert_detected, _assert_inside, _gemv32, _normed32, bf16_out


@functools.lru_cache(maxsize=None)
def _inputs(nh, nkv, kind):
    return G.attn_gqa_inputs(nh, nkv, G.ATTN_MAXS, kind)


@functools.lru_cache(maxsize=None)
def _ref(nh, nkv, kind, pos):
    return G.attn_gqa_ref(*_inputs(nh, nkv, kind), pos, G.ATTN_SCALE, nh)


def _all_positions():
    return sorted({p for NS in G.ATTN_SPLITS for p in G.attn_positions(hip.dec_attn_chunk(G.ATTN_MAXS, NS))})


# ------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("kind", G.ATTN_KINDS)
@pytest.mark.parametrize("NS", G.ATTN_SPLITS)
@pytest.mark.parametrize("nh,nkv", G.HEADS)
def test_fp32_split_model_is_inside_the_tolerance(nh, nkv, NS, kind):
    q, kc, vc = _inputs(nh, nkv, kind)
    C = hip.dec_attn_chunk(G.ATTN_MAXS, NS)
    for pos in G.attn_positions(C):
        out = G.attn_gqa_split32(q, kc, vc, pos, G.ATTN_SCALE, nh, NS, C)
        _assert_inside(f"split32 nh={nh} nkv={nkv} NS={NS} {kind} pos={pos}", out, _ref(nh, nkv, kind, pos))


def test_large60_scores_are_spread_where_the_group_is_one_head():
    """(4, 4): q and the caches come from the same generator call, so the keys lie along +-q
    and the scores reach +-60; key 0 holds the maximum, so every later chunk has a smaller one."""
    q, kc, _ = _inputs(4, 4, "large60")
    s = torch.einsum("bhd,bhjd->bhj", q.double().view(8, 4, 64), kc.double()) * G.ATTN_SCALE
    assert 0.98 * 60 < s.amax().item() < 1.02 * 60 and 0.98 * 60 < -s.amin().item() < 1.02 * 60
    C = hip.dec_attn_chunk(G.ATTN_MAXS, 4)
    assert (s[:, :, :C].amax(-1) > s[:, :, C:2 * C].amax(-1)).all() and (s[:, :, 0] == s.amax(-1)).all()


@pytest.mark.parametrize("nh,nkv", [(4, 2), (6, 2), (12, 4)])
def test_head_map_mod_is_rejected(nh, nkv):
    """Query head h on K/V head h % nkv instead of h // G.  (4, 1) and (4, 4) cannot tell."""
    assert not torch.equal(G.kv_head_of(nh, nkv, "mod"), G.kv_head_of(nh, nkv))
    for pos in _all_positions():
        bad = G.attn_gqa_ref(*_inputs(nh, nkv, "randn"), pos, G.ATTN_SCALE, nh, head_map="mod")
        _assert_detected(f"head_map=mod nh={nh} nkv={nkv} pos={pos}", bf16_out(bad.ref), _ref(nh, nkv, "randn", pos))


@pytest.mark.parametrize("nh,nkv", [(4, 1), (4, 4)])
def test_head_map_mod_is_the_same_map_for_one_group_or_one_head_per_group(nh, nkv):
    assert torch.equal(G.kv_head_of(nh, nkv, "mod"), G.kv_head_of(nh, nkv))


@pytest.mark.parametrize("nh,nkv", G.HEADS)
def test_extra_key_is_rejected(nh, nkv):
    for pos in _all_positions():
        if pos + 1 < G.ATTN_MAXS:
            bad = G.attn_gqa_ref(*_inputs(nh, nkv, "randn"), pos, G.ATTN_SCALE, nh, extra_keys=1)
            _assert_detected(f"key pos+1 nh={nh} nkv={nkv} pos={pos}", bf16_out(bad.ref), _ref(nh, nkv, "randn", pos))


@pytest.mark.parametrize("NS", G.ATTN_SPLITS)
@pytest.mark.parametrize("nh,nkv", G.HEADS)
def test_dropped_boundary_key_is_rejected(nh, nkv, NS):
    C = hip.dec_attn_chunk(G.ATTN_MAXS, NS)
    for pos in G.attn_positions(C):
        if pos >= 1:
            bad = G.attn_gqa_ref(*_inputs(nh, nkv, "randn"), pos, G.ATTN_SCALE, nh, drop_boundary_key=C)
            _assert_detected(f"last key of chunk 0 dropped nh={nh} nkv={nkv} NS={NS} pos={pos}", bf16_out(bad.ref),
                             _ref(nh, nkv, "randn", pos))


@pytest.mark.parametrize("NS", [2, 4])
def test_missing_rescale_is_rejected_on_large60(NS):
    """Chunk partials summed as if every chunk had the same max, at (4, 4) / large60, where
    chunk 0 holds a maximum of 60 and the others smaller ones; every position with a second
    chunk."""
    nh, nkv = 4, 4
    C = hip.dec_attn_chunk(G.ATTN_MAXS, NS)
    hit = 0
    for pos in G.attn_positions(C):
        bad = G.attn_gqa_ref(*_inputs(nh, nkv, "large60"), pos, G.ATTN_SCALE, nh, no_rescale=C)
        if pos < C:  # one chunk: nothing to rescale, the defect is no defect
            _assert_inside(f"no_rescale with one chunk pos={pos}", bf16_out(bad.ref), _ref(nh, nkv, "large60", pos))
        else:
            _assert_detected(f"no_rescale NS={NS} pos={pos}", bf16_out(bad.ref), _ref(nh, nkv, "large60", pos))
            hit += 1
    assert hit >= 3


# ------------------------------------------------------------------------------ QKV
@pytest.mark.parametrize("wbf16", [False, True])
@pytest.mark.parametrize("nh,nkv", G.QKV_HEADS)
def test_qkv_gqa_reference(nh, nkv, wbf16):
    h, lnw, w = G.qkv_gqa_inputs(nh, nkv, wbf16)
    H, KV = nh * 64, nkv * 64
    cos, sin = R.rope_tables(64, G.QKV_MAXS)
    y32 = _gemv32(_normed32(h, lnw), w)
    blocks = {"q": y32[:, :H].view(8, nh, 64), "k": y32[:, H:H + KV].view(8, nkv, 64),
              "v": y32[:, H + KV:].view(8, nkv, 64)}
    for pos in G.QKV_POS:
        ref = G.qkv_gqa_ref(h, lnw, w, cos, sin, pos, nh, nkv)
        assert ref["q"].ref.shape == (8, nh, 64) and ref["k"].ref.shape == ref["v"].ref.shape == (8, nkv, 64)
        c, s = cos[pos], sin[pos]
        for name in "qk":
            x1, x2 = blocks[name][..., :32], blocks[name][..., 32:]
            out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).bfloat16()
            _assert_inside(f"{name} pos={pos}", out, ref[name])
        _assert_inside("v", blocks["v"], ref["v"])
        for dname, km in R.slice_masks(H).items():
            bad = G.qkv_gqa_ref(h, lnw, w, cos, sin, pos, nh, nkv, kmask=km)
            for name in "qkv":
                _assert_detected(f"{dname} {name} pos={pos}", bf16_out(bad[name].ref), ref[name])
        for rp in (pos - 1, pos + 1):
            if 0 <= rp < G.QKV_MAXS:
                bad = G.qkv_gqa_ref(h, lnw, w, cos, sin, pos, nh, nkv, rope_pos=rp)
                for name in "qk":
                    _assert_detected(f"rope pos{rp - pos:+d} {name} pos={pos}", bf16_out(bad[name].ref), ref[name])
        if pos > 0:  # at pos 0 the rotation is the identity
            bad = G.qkv_gqa_ref(h, lnw, w, cos, sin, pos, nh, nkv, rope_v=True)
            _assert_detected(f"RoPE on v pos={pos}", bf16_out(bad["v"].ref), ref["v"])
        bad = G.qkv_gqa_ref(h, lnw, w, cos, sin, pos, nh, nkv, k_from_v=True)
        _assert_detected(f"k from the v rows pos={pos}", bf16_out(bad["k"].ref), ref["k"])


def test_qkv_gqa_reference_is_the_mha_reference_when_nkv_is_nh():
    h, lnw, w = G.qkv_gqa_inputs(4, 4, False)
    cos, sin = R.rope_tables(64, G.QKV_MAXS)
    a, b = G.qkv_gqa_ref(h, lnw, w, cos, sin, 5, 4, 4), R.qkv_ref(h, lnw, w, cos, sin, 5, 4)
    for name in "qkv":
        assert torch.equal(a[name].ref, b[name].ref) and torch.equal(a[name].tol, b[name].tol)


# ------------------------------------------------------------------------------ host side
def test_dec_attn_chunk():
    assert [hip.dec_attn_chunk(200, n) for n in (1, 2, 4, 8)] == [200, 100, 50, 25]
    assert [hip.dec_attn_chunk(1023, n) for n in (1, 2, 4, 8)] == [1023, 512, 256, 128]
    assert hip.dec_attn_chunk(1, 8) == 1
    for maxS in (1, 7, 200, 1023, 16384):
        for n in hip.DEC_ATTN_SPLITS:
            C = hip.dec_attn_chunk(maxS, n)
            assert C * n >= maxS > C * n - n  # the chunks cover the cache, none is spare by a whole key each
    for bad in (0, 3, 16):
        with pytest.raises(ValueError):
            hip.dec_attn_chunk(200, bad)
    assert G.attn_positions(50) == (0, 1, 49, 50, 51, 100, 199)
    assert G.attn_positions(200) == (0, 1, 199)


def test_kv_splits_rule_and_environment(monkeypatch):
    monkeypatch.delenv("DLT_DECODE_KV_SPLITS", raising=False)
    # the measured rule (profiles/gqa_decode.md): 4 chunks, 8 for a cache beyond 4096; B * nkv does not enter
    for B, nkv in ((1, 1), (1, 4), (2, 4), (8, 1), (4, 4), (8, 4), (8, 12), (1, 32)):
        assert D._dec_kv_splits(B, nkv, 256) == D._dec_kv_splits(B, nkv, 1024) == D._dec_kv_splits(B, nkv, 4096) == 4
        assert D._dec_kv_splits(B, nkv, 4097) == D._dec_kv_splits(B, nkv, 16384) == 8
    for n in (1, 2, 4, 8):
        monkeypatch.setenv("DLT_DECODE_KV_SPLITS", str(n))
        assert D._dec_kv_splits(1, 4, 1024) == n and D._dec_kv_splits(8, 12, 16384) == n
    monkeypatch.setenv("DLT_DECODE_KV_SPLITS", " 2 ")
    assert D._dec_kv_splits(8, 4, 1024) == 2
    for bad in ("0", "3", "16", "-1", "two", "2.0"):
        monkeypatch.setenv("DLT_DECODE_KV_SPLITS", bad)
        with pytest.raises(ValueError, match="DLT_DECODE_KV_SPLITS"):
            D._dec_kv_splits(1, 4, 1024)
    monkeypatch.setenv("DLT_DECODE_KV_SPLITS", "")
    assert D._dec_kv_splits(8, 4, 1024) == 4


def _stub(nh, nkv, hidden=None, maxS=1024, gqa_ops=True, dec_ops=True):
    hidden = nh * 64 if hidden is None else hidden
    ops = types.SimpleNamespace(backend="hip")
    if dec_ops:
        ops.dec_norm_qkv, ops.DECODE_BATCHES = (lambda *a: None), (1, 2, 4, 8)
        if gqa_ops:
            ops.dec_attn_gqa = lambda *a: None
    cfg = types.SimpleNamespace(num_heads=nh, num_kv_heads=nkv, head_dim=hidden // nh, hidden_size=hidden,
                                max_seq_len=maxS)
    return types.SimpleNamespace(engine=types.SimpleNamespace(ops=ops), config=cfg)


def test_fused_kind_on_stub_configs(monkeypatch):
    monkeypatch.delenv("DLT_DECODE_KV_SPLITS", raising=False)
    monkeypatch.delenv("DLT_DECODE_FUSED", raising=False)
    mha, gqa, mqa = _stub(12, 12), _stub(12, 4), _stub(12, 1)
    for B in (1, 2, 4, 8):
        assert D._fused_kind(mha, B) == "mha" and D._fused_ok(mha, B)
        assert D._fused_kind(gqa, B) == "gqa" and not D._fused_ok(gqa, B)
        assert D._fused_kind(mqa, B) == "gqa" and not D._fused_ok(mqa, B)
    for m in (mha, gqa):
        assert D._fused_kind(m, 3) is None and D._fused_kind(m, 16) is None  # no such batch instantiation
        assert D._fused_kind(_stub(12, m.config.num_kv_heads, dec_ops=False), 1) is None  # reference ops
    # the MHA conditions are the ones _fused_ok had: k_dec_attn's maxS * 4 + 1056 bytes, the norm rows
    assert D._fused_kind(_stub(4, 4, maxS=40696), 1) == "mha"
    assert D._fused_kind(_stub(4, 4, maxS=40697), 1) is None and not D._fused_ok(_stub(4, 4, maxS=48 * 1024), 1)
    assert D._fused_kind(_stub(4, 4, hidden=512), 1) is None  # head_dim 128
    assert D._fused_kind(_stub(4, 2, hidden=512), 1) is None  # head_dim 128, grouped
    assert D._fused_kind(_stub(192, 192), 8) is None and D._fused_kind(_stub(192, 48), 8) is None  # norm rows: 196 KB
    assert D._fused_kind(_stub(12, 4, gqa_ops=False), 1) is None  # a library without the grouped kernels
    half = _stub(12, 4)
    half.engine.act_dtype = torch.float16  # the grouped kernels are bf16 only: the ATen step as before
    assert D._fused_kind(half, 1) is None
    half.engine.act_dtype = torch.bfloat16
    assert D._fused_kind(half, 1) == "gqa"
    # grouped-query LDS: the scores of a group over one chunk at the chosen NS
    long = _stub(12, 1, maxS=16384)
    assert D._gqa_splits(long.config, 8) == 8 and D._fused_kind(long, 8) == "gqa"  # 12 heads x 2048 keys: 96 KB
    monkeypatch.setenv("DLT_DECODE_KV_SPLITS", "1")  # the environment fixes NS: 786 KB of scores do not fit
    assert D._gqa_splits(long.config, 8) == 1 and D._fused_kind(long, 8) is None
    assert D._fused_kind(gqa, 1) == "gqa"  # 3 heads over 1024 keys: 16 KB
    monkeypatch.delenv("DLT_DECODE_KV_SPLITS")
    assert D._fused_kind(_stub(12, 1, maxS=48 * 1024), 1) is None  # 12 * 6144 * 4 = 295 KB at NS = 8
    assert hip.dec_attn_gqa_lds(12, 2048) <= D.DEC_LDS_MAX < hip.dec_attn_gqa_lds(12, 4096)
    monkeypatch.setenv("DLT_DECODE_FUSED", "0")
    assert D._fused_kind(mha, 1) is None and D._fused_kind(gqa, 1) is None and not D._fused_ok(mha, 1)
