"""The grouped-query decode kernels (dec_norm_qkv_gqa, dec_attn_gqa + its combine) alone
against the fp64 references and derived tolerances of tests/decode_gqa_ref.py, with sentinel
guards around every output buffer; then the captured fused step and ``generate`` of a
grouped-query model against the ATen step.

Each numerical check prints ``RATIO <kernel> <worst err / tol>`` (pytest -s shows them)."""
import ctypes
import functools
import math

import pytest
import torch

from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip
from tests import decode_gqa_ref as G
from tests import decode_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, I64 = torch.bfloat16, torch.float32, torch.int64
PAD = 64  # guard elements on each side of an output (a multiple of 16 bytes for every dtype)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Guarded:
    """A tensor that is a view into a larger sentinel-filled allocation."""

    def __init__(self, shape, dtype, fill, init=None):
        n = math.prod(shape)
        self.buf = torch.full((PAD + n + PAD + (-n) % 8,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n].view(shape)
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(init)
        self.before = self.buf.clone()

    def assert_guards(self, written=None):
        """Bit-identical outside the view, and inside it wherever ``written`` (bool, the
        view's shape; default all of it) is False."""
        want = self.before.clone()
        wv = want[PAD:PAD + self.t.numel()].view(self.t.shape)
        if written is None:
            wv.copy_(self.t)
        else:
            wv[written] = self.t[written]
        diff = (_bits(self.buf) != _bits(want)).nonzero().flatten()
        assert diff.numel() == 0, f"{diff.numel()} elements outside the output changed, first at {diff[0].item() - PAD}"


def check(name, out, chk, B=None):
    ref, tol = (chk.ref, chk.tol) if B is None else (chk.ref[:B], chk.tol[:B])
    out = out.double().reshape(ref.shape)
    err = (out - ref).abs()
    ratio = torch.where(tol > 0, err / tol, err).max().item()
    print(f"RATIO {name} {ratio:.4f}")
    bad = ~(err <= tol)
    assert not bad.any(), (f"{name}: {bad.sum().item()} of {bad.numel()} elements outside the tolerance, "
                           f"worst err/tol {ratio:.3f} at {bad.nonzero()[0].tolist()}")


def _dev(ts):
    return tuple(t.to(DEV) for t in ts)


def _pos(p):
    return torch.tensor([p], dtype=I64, device=DEV)


# ------------------------------------------------------------------------ dec_norm_qkv_gqa
@functools.lru_cache(maxsize=None)
def _qkv_case(nh, nkv, wbf16):
    return _dev(G.qkv_gqa_inputs(nh, nkv, wbf16)) + hip.rope_tables(64, G.QKV_MAXS, device=DEV)


@functools.lru_cache(maxsize=None)
def _qkv_ref(nh, nkv, wbf16, pos):
    h, lnw, w, cos, sin = _qkv_case(nh, nkv, wbf16)
    return G.qkv_gqa_ref(h, lnw, w, cos, sin, pos, nh, nkv)


@pytest.mark.parametrize("B", R.DECODE_BATCHES)
@pytest.mark.parametrize("wbf16", [False, True])
@pytest.mark.parametrize("pos", G.QKV_POS)
@pytest.mark.parametrize("nh,nkv", G.QKV_HEADS)
def test_dec_norm_qkv_gqa(nh, nkv, pos, wbf16, B):
    h, lnw, w, cos, sin = _qkv_case(nh, nkv, wbf16)
    H, maxS = nh * 64, G.QKV_MAXS
    ref = _qkv_ref(nh, nkv, wbf16, pos)
    hin = h[:B].contiguous()
    q = Guarded((B, H), BF, -777.0)
    kc, vc = Guarded((B, nkv, maxS, 64), BF, -555.0), Guarded((B, nkv, maxS, 64), BF, 333.0)
    posd = _pos(pos)
    hip.dec_norm_qkv_gqa(hin, lnw, R.EPS, w, cos, sin, posd, q.t, kc.t, vc.t, nh, nkv)
    tag = f"dec_norm_qkv_gqa[nh={nh},nkv={nkv},pos={pos},wbf16={int(wbf16)},B={B}]"
    check(tag + ".q", q.t, ref["q"], B)
    check(tag + ".k", kc.t[:, :, pos], ref["k"], B)
    check(tag + ".v", vc.t[:, :, pos], ref["v"], B)
    row = torch.zeros((B, nkv, maxS, 64), dtype=torch.bool, device=DEV)
    row[:, :, pos] = True
    q.assert_guards()
    kc.assert_guards(row)
    vc.assert_guards(row)
    assert posd.item() == pos and torch.equal(hin, h[:B])
    if nkv == nh:  # the multi-head entry point on the same inputs: the same bits
        q2 = Guarded((B, H), BF, -777.0)
        k2, v2 = Guarded((B, nh, maxS, 64), BF, -555.0), Guarded((B, nh, maxS, 64), BF, 333.0)
        hip.dec_norm_qkv(hin, lnw, R.EPS, w, cos, sin, posd, q2.t, k2.t, v2.t, nh)
        assert torch.equal(q2.buf, q.buf) and torch.equal(k2.buf, kc.buf) and torch.equal(v2.buf, vc.buf)


def test_dec_norm_qkv_gqa_host_validation():
    nh, nkv, B, maxS = 4, 2, 1, G.QKV_MAXS
    h, lnw, w, cos, sin = _qkv_case(nh, nkv, False)
    hin, posd = h[:B].contiguous(), _pos(0)
    q = torch.empty(B, nh * 64, dtype=BF, device=DEV)
    kc, vc = (torch.zeros(B, nkv, maxS, 64, dtype=BF, device=DEV) for _ in range(2))
    hip.dec_norm_qkv_gqa(hin, lnw, R.EPS, w, cos, sin, posd, q, kc, vc, nh, nkv)
    k4 = torch.zeros(B, 4, maxS, 64, dtype=BF, device=DEV)
    k3 = torch.zeros(B, 3, maxS, 64, dtype=BF, device=DEV)
    with pytest.raises(ValueError):  # the weight is (H + 2 * 2 * 64, H), not (3H, H)
        hip.dec_norm_qkv_gqa(hin, lnw, R.EPS, w, cos, sin, posd, q, k4, k4.clone(), nh, 4)
    with pytest.raises(ValueError):  # caches of another head count
        hip.dec_norm_qkv_gqa(hin, lnw, R.EPS, w, cos, sin, posd, q, k4, k4.clone(), nh, nkv)
    with pytest.raises(ValueError, match="nkv"):  # nh % nkv
        hip.dec_norm_qkv_gqa(hin, lnw, R.EPS, w, cos, sin, posd, q, k3, k3.clone(), nh, 3)
    with pytest.raises(ValueError):
        hip.dec_norm_qkv_gqa(hin, lnw, R.EPS, w[:-64], cos, sin, posd, q, kc, vc, nh, nkv)
    with pytest.raises(ValueError):
        hip.dec_norm_qkv_gqa(hin, lnw, R.EPS, w, cos, sin, posd, q, kc, vc[:, :, :32], nh, nkv)
    with pytest.raises(ValueError):  # RoPE tables shorter than the cache
        hip.dec_norm_qkv_gqa(hin, lnw, R.EPS, w, cos[:32], sin[:32], posd, q, kc, vc, nh, nkv)
    with pytest.raises(TypeError):
        hip.dec_norm_qkv_gqa(hin, lnw, R.EPS, w, cos, sin, posd, q, kc.float(), vc.float(), nh, nkv)
    rc = hip.lib().dlt_dec_norm_qkv_gqa(None, None, 0, 1e-5, None, None, None, None, None, None, None, 1, 256, 4, 3,
                                        64, None)
    assert rc == -1, "the launcher must refuse nh % nkv != 0 before any launch"


# ------------------------------------------------------------------------ dec_attn_gqa
@functools.lru_cache(maxsize=None)
def _attn_case(nh, nkv, kind):
    return _dev(G.attn_gqa_inputs(nh, nkv, G.ATTN_MAXS, kind))


@functools.lru_cache(maxsize=None)
def _attn_ref(nh, nkv, kind, pos):
    """Computed once per (shape, kind, pos) for B = 8 and shared, unchanged, by every NS and B."""
    return G.attn_gqa_ref(*_attn_case(nh, nkv, kind), pos, G.ATTN_SCALE, nh)


@functools.lru_cache(maxsize=16)
def _poisoned(nh, nkv, kind, pos):
    """The caches with NaN in every K row and 3e38 in every V row beyond pos."""
    _, kc, vc = _attn_case(nh, nkv, kind)
    k2, v2 = kc.clone(), vc.clone()
    k2[:, :, pos + 1:] = float("nan")
    v2[:, :, pos + 1:] = 3e38
    return k2, v2


@pytest.mark.parametrize("B", G.ATTN_BATCHES)
@pytest.mark.parametrize("NS", G.ATTN_SPLITS)
@pytest.mark.parametrize("kind", G.ATTN_KINDS)
@pytest.mark.parametrize("nh,nkv", G.HEADS)
def test_dec_attn_gqa(nh, nkv, kind, NS, B):
    maxS = G.ATTN_MAXS
    C = hip.dec_attn_chunk(maxS, NS)
    q = _attn_case(nh, nkv, kind)[0][:B].contiguous()
    q0 = q.clone()
    for pos in G.attn_positions(C):
        kc, vc = (t[:B].contiguous() for t in _poisoned(nh, nkv, kind, pos))
        k0, v0 = kc.clone(), vc.clone()
        posd = _pos(pos)
        outs = []
        for _ in range(2):  # the second call on a fresh workspace full of NaN
            o = Guarded((B, nh * 64), BF, -777.0)
            ws = Guarded((B * nh * NS * hip.DEC_ATTN_WS,), F32, float("nan")) if NS > 1 else None
            hip.dec_attn_gqa(q, kc, vc, posd, o.t, G.ATTN_SCALE, nh, splits=NS, ws=None if ws is None else ws.t)
            o.assert_guards()
            if ws is not None:
                ws.assert_guards()
            outs.append(o.t)
        assert torch.isfinite(outs[0]).all(), "a cache row beyond pos reached the output"
        check(f"dec_attn_gqa[nh={nh},nkv={nkv},{kind},NS={NS},pos={pos},B={B}]", outs[0],
              _attn_ref(nh, nkv, kind, pos), B)
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two calls, two results"
        assert posd.item() == pos and torch.equal(q, q0)
        assert torch.equal(_bits(kc), _bits(k0)) and torch.equal(_bits(vc), _bits(v0))


def test_dec_attn_gqa_splits_8_and_a_group_of_more_than_16_heads():
    """NS = 8 (the largest split), and G = 20 > 16: the group is served by two workgroups
    per chunk (16 + 4 query heads)."""
    for nh, nkv, NS in ((12, 4, 8), (20, 1, 2), (20, 1, 1)):
        C = hip.dec_attn_chunk(G.ATTN_MAXS, NS)
        q, kc, vc = _dev(G.attn_gqa_inputs(nh, nkv, G.ATTN_MAXS, "randn"))
        for pos in (0, C, G.ATTN_MAXS - 1):
            ref = G.attn_gqa_ref(q, kc, vc, pos, G.ATTN_SCALE, nh)
            k2, v2 = kc.clone(), vc.clone()
            k2[:, :, pos + 1:] = float("nan")
            v2[:, :, pos + 1:] = 3e38
            o = Guarded((8, nh * 64), BF, -777.0)
            ws = Guarded((8 * nh * NS * hip.DEC_ATTN_WS,), F32, float("nan"))
            hip.dec_attn_gqa(q, k2, v2, _pos(pos), o.t, G.ATTN_SCALE, nh, splits=NS, ws=ws.t)
            check(f"dec_attn_gqa[nh={nh},nkv={nkv},randn,NS={NS},pos={pos},B=8]", o.t, ref)
            o.assert_guards()
            ws.assert_guards()


def test_dec_attn_gqa_refusals():
    L = hip.lib()
    # G * C * 4 bytes of scores: 16 heads over 4096 keys are 256 KB, over 2 x 2048 they fit
    nh, nkv, maxS = 16, 1, 4096
    q = torch.zeros(1, nh * 64, dtype=BF, device=DEV)
    kc, vc = (torch.zeros(1, nkv, maxS, 64, dtype=BF, device=DEV) for _ in range(2))
    o = Guarded((1, nh * 64), BF, -777.0)
    assert hip.dec_attn_gqa_lds(16, 4096) > 160 * 1024 >= hip.dec_attn_gqa_lds(16, 2048)
    with pytest.raises(RuntimeError, match="dec_attn_gqa"):
        hip.dec_attn_gqa(q, kc, vc, _pos(0), o.t, 0.125, nh, splits=1)
    o.assert_guards(torch.zeros((1, nh * 64), dtype=torch.bool, device=DEV))
    ws = hip.dec_attn_gqa_workspace(1, nh, 2, DEV)
    hip.dec_attn_gqa(q, kc, vc, _pos(0), o.t, 0.125, nh, splits=2, ws=ws)
    assert (o.t == 0).all()  # V is zero
    # nh % nkv: the binding refuses, and so does the launcher itself
    k3 = torch.zeros(1, 3, 64, 64, dtype=BF, device=DEV)
    q4 = torch.zeros(1, 4 * 64, dtype=BF, device=DEV)
    with pytest.raises(ValueError, match="nkv"):
        hip.dec_attn_gqa(q4, k3, k3.clone(), _pos(0), q4.clone(), 0.125, 4)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o4 = Guarded((1, 4 * 64), BF, -777.0)
    args = (p(q4), p(k3), p(k3), p(_pos(0)), p(o4.t), None)
    assert L.dlt_dec_attn_gqa(*args, 1, 256, 4, 3, 64, 1, 0.125, st) == -1
    assert L.dlt_dec_attn_gqa(*args, 1, 256, 4, 1, 64, 3, 0.125, st) == -1  # NS not in {1, 2, 4, 8}
    assert L.dlt_dec_attn_gqa(*args, 1, 256, 4, 1, 64, 2, 0.125, st) == -1  # NS > 1 without a workspace
    torch.cuda.synchronize()
    o4.assert_guards(torch.zeros((1, 4 * 64), dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        hip.dec_attn_gqa(q4, k3[:, :2], k3[:, :2].clone(), _pos(0), q4.clone(), 0.125, 4, splits=3)
    with pytest.raises(ValueError, match="workspace"):
        hip.dec_attn_gqa(q4, k3[:, :2].contiguous(), k3[:, :2].contiguous(), _pos(0), q4.clone(), 0.125, 4, splits=2)
    with pytest.raises(ValueError):  # a workspace of another size
        hip.dec_attn_gqa(q4, k3[:, :2].contiguous(), k3[:, :2].contiguous(), _pos(0), q4.clone(), 0.125, 4, splits=2,
                         ws=hip.dec_attn_gqa_workspace(1, 4, 4, DEV))


# ------------------------------------------------------------------------------- the step
def _cfg(nkv, **kw):
    d = dict(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=nkv, max_seq_len=256,
             dropout=0.0, attention_dropout=0.0)
    d.update(kw)
    return GPTConfig(**d)


@functools.lru_cache(maxsize=None)
def _model(nkv):
    torch.manual_seed(5 + nkv)
    m = GPT(_cfg(nkv)).to(DEV)
    m.enable_engine()
    m.eval()
    return m


@pytest.mark.parametrize("splits", [1, 4])
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("nkv", [1, 2])
def test_decode_fused_gqa_step_matches_torch_step(nkv, B, splits, monkeypatch):
    """The captured fused step of a grouped-query model == the ATen step: logits and the K/V
    cache rows it appends, over a 150-token context; two fresh fused graphs agree bit for bit."""
    from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, _fused_kind, _fused_ok, forward_cached
    m = _model(nkv)
    cfg = m.config
    monkeypatch.setenv("DLT_DECODE_KV_SPLITS", str(splits))
    monkeypatch.setenv("DLT_DECODE_FUSED", "1")
    assert _fused_kind(m, B) == "gqa" and not _fused_ok(m, B)
    g = torch.Generator().manual_seed(50 + B)
    ids = torch.randint(0, 1000, (B, 150), generator=g).to(DEV)
    steps = torch.randint(0, 1000, (B, 5), generator=g).to(DEV)
    caches = [KVCache(cfg, B, DEV, m.engine.act_dtype) for _ in range(3)]
    graphs = []
    with torch.no_grad():
        for c, fused in zip(caches, ("1", "0", "1")):
            forward_cached(m, ids, c)
            monkeypatch.setenv("DLT_DECODE_FUSED", fused)
            graphs.append(DecodeGraph(m, c, c.len))
        assert graphs[0].fused and graphs[0].kind == "gqa" and graphs[0].kv_splits == splits
        assert graphs[2].fused and not graphs[1].fused
        for t in range(steps.shape[1]):
            a = graphs[0](steps[:, t:t + 1]).clone()
            b = graphs[1](steps[:, t:t + 1]).clone()
            a2 = graphs[2](steps[:, t:t + 1]).clone()
            assert torch.allclose(a, b, atol=3e-2, rtol=3e-2), (t, (a - b).abs().max().item())
            assert torch.equal(a, a2), "two fused graphs on the same inputs, other logits"
            pos = caches[0].len - 1
            for i in range(cfg.num_layers):
                assert caches[0].k[i].shape == (B, nkv, 256, 64)
                for x, y in ((caches[0].k[i], caches[1].k[i]), (caches[0].v[i], caches[1].v[i])):
                    assert torch.allclose(x[:, :, pos].float(), y[:, :, pos].float(), atol=2e-2, rtol=2e-2)


# ----------------------------------------------------------------------------- generation
@pytest.mark.parametrize("nkv", [1, 2])
def test_generate_device_loop_matches_host_loop_gqa(nkv, monkeypatch):
    """Greedy generation of a grouped-query model with the on-device loop (fused step +
    sampling in one graph) == the host loop, including the cropped-context tail."""
    m = _model(nkv)
    ids = torch.randint(0, 1000, (2, 240), generator=torch.Generator().manual_seed(7)).to(DEV)
    monkeypatch.setenv("DLT_DECODE_DEVICE_LOOP", "1")
    a = m.generate(ids, max_new_tokens=24, top_k=1)
    monkeypatch.setenv("DLT_DECODE_DEVICE_LOOP", "0")
    b = m.generate(ids, max_new_tokens=24, top_k=1)
    assert a.shape == b.shape == (2, 264)
    assert (a == b).float().mean().item() > 0.97  # greedy; rare near-ties may flip


def test_generate_gqa_from_a_prompt_that_fills_all_but_one_slot(monkeypatch):
    m = _model(2)
    ids = torch.randint(0, 1000, (2, 255), generator=torch.Generator().manual_seed(8)).to(DEV)
    monkeypatch.setenv("DLT_DECODE_DEVICE_LOOP", "1")
    a = m.generate(ids, max_new_tokens=6, top_k=1)
    monkeypatch.setenv("DLT_DECODE_DEVICE_LOOP", "0")
    b = m.generate(ids, max_new_tokens=6, top_k=1)
    assert a.shape == b.shape == (2, 261)
    assert ((a >= 0) & (a < 1000)).all()
    assert (a == b).float().mean().item() > 0.97


def test_generate_gqa_without_the_fused_step_and_with_head_dim_128(monkeypatch):
    from distributed_llm_trainer_amd.eval.decode import _fused_kind
    m = _model(2)
    ids = torch.randint(0, 1000, (1, 16), generator=torch.Generator().manual_seed(9)).to(DEV)
    want = m.generate(ids, max_new_tokens=4, top_k=1)
    monkeypatch.setenv("DLT_DECODE_FUSED", "0")
    assert _fused_kind(m, 1) is None
    got = m.generate(ids, max_new_tokens=4, top_k=1)
    assert got.shape == want.shape == (1, 20) and (got == want).float().mean().item() > 0.9
    monkeypatch.delenv("DLT_DECODE_FUSED")
    torch.manual_seed(11)
    m128 = GPT(_cfg(1, num_heads=2, num_layers=1)).to(DEV)  # head_dim 128, one K/V head
    m128.enable_engine()
    m128.eval()
    assert m128.config.head_dim == 128 and _fused_kind(m128, 1) is None
    out = m128.generate(ids, max_new_tokens=4, top_k=5)
    assert out.shape == (1, 20) and ((out >= 0) & (out < 1000)).all()
