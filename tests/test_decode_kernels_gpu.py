"""Each fused decode kernel (ops/csrc/decode.hip) alone against the fp64 references and the
derived tolerances of tests/decode_ref.py: every element of every output, at the smallest
shapes that reach each code path, with sentinel guards around every output buffer.

Each numerical check prints ``RATIO <kernel> <worst err / tol>`` (pytest -s shows them)."""
import functools
import math

import pytest
import torch

from distributed_llm_trainer_amd.ops import hip
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


# ------------------------------------------------------------------------ GEMV kernels
@functools.lru_cache(maxsize=None)
def _qkv_case(H, wbf16):
    return _dev(R.qkv_inputs(H, wbf16)) + hip.rope_tables(64, R.QKV_MAXS, device=DEV)


@functools.lru_cache(maxsize=None)
def _qkv_ref(H, wbf16, pos):
    h, lnw, w, cos, sin = _qkv_case(H, wbf16)
    return R.qkv_ref(h, lnw, w, cos, sin, pos, H // 64)


@pytest.mark.parametrize("B", R.DECODE_BATCHES)
@pytest.mark.parametrize("wbf16", [False, True])
@pytest.mark.parametrize("pos", R.QKV_POS)
@pytest.mark.parametrize("H", R.QKV_H)
def test_dec_norm_qkv(H, pos, wbf16, B):
    h, lnw, w, cos, sin = _qkv_case(H, wbf16)
    nh, maxS = H // 64, R.QKV_MAXS
    ref = _qkv_ref(H, wbf16, pos)
    hin = h[:B].contiguous()
    q = Guarded((B, H), BF, -777.0)
    kc, vc = Guarded((B, nh, maxS, 64), BF, -555.0), Guarded((B, nh, maxS, 64), BF, 333.0)
    posd = _pos(pos)
    hip.dec_norm_qkv(hin, lnw, R.EPS, w, cos, sin, posd, q.t, kc.t, vc.t, nh)
    tag = f"dec_norm_qkv[H={H},pos={pos},wbf16={int(wbf16)},B={B}]"
    check(tag + ".q", q.t, ref["q"], B)
    check(tag + ".k", kc.t[:, :, pos], ref["k"], B)
    check(tag + ".v", vc.t[:, :, pos], ref["v"], B)
    row = torch.zeros((B, nh, maxS, 64), dtype=torch.bool, device=DEV)
    row[:, :, pos] = True
    q.assert_guards()
    kc.assert_guards(row)
    vc.assert_guards(row)
    assert posd.item() == pos and torch.equal(hin, h[:B])


@functools.lru_cache(maxsize=None)
def _res_case(RK):
    x, w, h = _dev(R.res_inputs(*RK))
    return x, w, h, R.gemv_res_ref(x, w, h)


@pytest.mark.parametrize("B", R.DECODE_BATCHES)
@pytest.mark.parametrize("RK", R.RES_SHAPES)
def test_dec_gemv_res(RK, B):
    x, w, h0, ref = _res_case(RK)
    h = Guarded((B, RK[0]), F32, 1234.5, init=h0[:B])
    hip.dec_gemv_res(x[:B].contiguous(), w, h.t)
    check(f"dec_gemv_res[R={RK[0]},K={RK[1]},B={B}]", h.t, ref, B)
    h.assert_guards()


@functools.lru_cache(maxsize=None)
def _gu_case(HI, wbf16):
    h, lnw, w = _dev(R.gu_inputs(*HI, wbf16))
    return h, lnw, w, R.norm_gu_ref(h, lnw, w)


@pytest.mark.parametrize("B", R.DECODE_BATCHES)
@pytest.mark.parametrize("wbf16", [False, True])
@pytest.mark.parametrize("HI", R.GU_SHAPES)
def test_dec_norm_gu(HI, wbf16, B):
    h, lnw, w, ref = _gu_case(HI, wbf16)
    hin = h[:B].contiguous()
    s = Guarded((B, HI[1]), BF, -777.0)
    hip.dec_norm_gu(hin, lnw, R.EPS, w, s.t)
    check(f"dec_norm_gu[H={HI[0]},I={HI[1]},wbf16={int(wbf16)},B={B}]", s.t, ref, B)
    s.assert_guards()
    assert torch.equal(hin, h[:B])


@functools.lru_cache(maxsize=None)
def _head_case(HVR, wbf16):
    h, lnw, w = _dev(R.head_inputs(*HVR, wbf16))
    return h, lnw, w, R.norm_head_ref(h, lnw, w, HVR[1])


@pytest.mark.parametrize("B", R.DECODE_BATCHES)
@pytest.mark.parametrize("wbf16", [False, True])
@pytest.mark.parametrize("HVR", R.HEAD_SHAPES)
def test_dec_norm_head(HVR, wbf16, B):
    H, V, rows = HVR
    h, lnw, w, ref = _head_case(HVR, wbf16)
    logits = Guarded((B, V), F32, 1234.5)
    hip.dec_norm_head(h[:B].contiguous(), lnw, R.EPS, w, logits.t, V)
    assert torch.isfinite(logits.t).all(), "a NaN weight row >= V reached a logit"
    check(f"dec_norm_head[H={H},V={V},wbf16={int(wbf16)},B={B}]", logits.t, ref, B)
    logits.assert_guards()  # the logits are exactly [B, V]


# --------------------------------------------------------------------------- attention
@functools.lru_cache(maxsize=4)
def _attn_case(nh, maxS, kind):
    return _dev(R.attn_inputs(nh, maxS, kind))


@functools.lru_cache(maxsize=None)
def _attn_ref(nh, maxS, kind, pos):
    q, kc, vc = _attn_case(nh, maxS, kind)
    return R.attn_ref(q, kc, vc, pos, R.ATTN_SCALE)


def _run_attn(nh, maxS, kind, pos, B):
    q, kc, vc = (t[:B].contiguous() for t in _attn_case(nh, maxS, kind))
    posd = _pos(pos)
    o = Guarded((B, nh * 64), BF, -777.0)
    hip.dec_attn(q, kc, vc, posd, o.t, R.ATTN_SCALE)
    check(f"dec_attn[nh={nh},maxS={maxS},{kind},pos={pos},B={B}]", o.t, _attn_ref(nh, maxS, kind, pos), B)
    o.assert_guards()
    assert posd.item() == pos
    if pos + 1 < maxS:  # the cache rows beyond pos must not reach the output
        for fill in (float("nan"), 3e38):
            k2, v2 = kc.clone(), vc.clone()
            k2[:, :, pos + 1:] = fill
            v2[:, :, pos + 1:] = fill
            o2 = Guarded((B, nh * 64), BF, -777.0)
            hip.dec_attn(q, k2, v2, posd, o2.t, R.ATTN_SCALE)
            assert torch.isfinite(o2.t).all() and torch.equal(_bits(o2.t), _bits(o.t)), f"rows > pos = {fill} leak"


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("pos", R.ATTN_POS)
@pytest.mark.parametrize("nh", [3, 12])
def test_dec_attn(nh, pos, B):
    _run_attn(nh, 1024, "randn", pos, B)


def test_dec_attn_long_cache():
    _run_attn(3, 4096, "randn", 4095, 2)


@pytest.mark.parametrize("kind", ["large60", "large100", "equal"])
def test_dec_attn_score_ranges(kind):
    """Scores spread over +-60 and +-100 after scaling (a softmax without the max subtraction
    overflows fp32 at the latter), and all keys equal (uniform probabilities)."""
    _run_attn(3, 1024, kind, 1023, 8)
    _run_attn(3, 1024, kind, 300, 1)


# ----------------------------------------------------------------------------- sampler
def _draw(logits, T, k, seed, n, use_ws, pos0=0):
    """n draws per row at positions pos0 .. pos0 + n - 1 (advanced by dec_advance) -> [B, n]."""
    B = logits.shape[0]
    ids = torch.full((B,), -1, dtype=I64, device=DEV)
    hist = torch.full((B, n), -1, dtype=I64, device=DEV)
    pos = _pos(pos0)
    ws = hip.dec_sample_workspace(B, DEV) if use_ws else None
    for _ in range(n):
        hip.dec_sample(logits, T, k, seed, pos, ids, hist, pos0 + 1, ws=ws)
        hip.dec_advance(pos)
    assert pos.item() == pos0 + n
    assert torch.equal(hist[:, -1], ids)
    return hist.cpu()


def _assert_support(hist, kept):
    V = kept.shape[1]
    assert ((hist >= 0) & (hist < V)).all(), "an id outside [0, V)"
    ok = kept.gather(1, hist)
    assert ok.all(), f"{(~ok).sum().item()} draws outside the kept set, e.g. id {hist[~ok][0].item()}"


def _freq(hist, V):
    f = torch.zeros(hist.shape[0], V, dtype=torch.float64)
    f.scatter_add_(1, hist, torch.ones(hist.shape, dtype=torch.float64))
    return f / hist.shape[1]


def _assert_freq(name, hist, probs, bucket=1):
    """|frequency - p| <= freq_bound per id, or per ``bucket`` consecutive ids where a row keeps
    thousands of ids (the bound is a normal-tail one: it needs n * p of a few draws at least)."""
    n = hist.shape[1]
    if bucket > 1:
        nb = -(-probs.shape[1] // bucket)
        idx = (torch.arange(probs.shape[1]) // bucket).expand(probs.shape[0], -1)
        probs = torch.zeros(probs.shape[0], nb, dtype=torch.float64).scatter_add_(1, idx, probs)
        hist = torch.div(hist, bucket, rounding_mode="floor")
    dev = (_freq(hist, probs.shape[1]) - probs).abs() / R.freq_bound(probs, n)
    print(f"RATIO {name} {dev.max().item():.4f}")
    assert (dev <= 1).all(), f"{name}: worst |freq - p| / bound = {dev.max().item():.3f}"


SCALES = torch.tensor([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0])


def _scaled_logits(V, seed):
    return torch.randn(8, V, generator=torch.Generator().manual_seed(seed)) * SCALES[:, None]


@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("V,k,T", [(50257, 50, 0.8), (3000, 8, 0.7), (100, 8, 1.0), (17, 3, 1.0)])
def test_dec_sample_support_and_frequencies(V, k, T, use_ws):
    """Ids only from the kept set, frequencies of 4000 draws within freq_bound of the fp64
    probabilities.  V = 100 and 17 give the split sampler slices shorter than top_k."""
    logits = _scaled_logits(V, 600 + V)
    kept, probs = R.sample_reference(logits, T, k)
    assert (kept.sum(1) == k).all()
    hist = _draw(logits.to(DEV), T, k, 20240607, 4000, use_ws)
    _assert_support(hist, kept)
    _assert_freq(f"dec_sample.freq[V={V},k={k},ws={int(use_ws)}]", hist, probs)


@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("V,k", [(17, 0), (17, 17), (17, 22), (3000, 0), (3000, 3000), (3000, 3005)])
def test_dec_sample_without_a_filter(V, k, use_ws):
    """top_k = 0 and top_k >= V filter nothing: every id of a flat row is drawn."""
    logits = 0.3 * _scaled_logits(V, 610 + V)[:2]
    kept, probs = R.sample_reference(logits, 1.0, k)
    assert kept.all()
    n = 600 if V == 17 else 3000
    hist = _draw(logits.to(DEV), 1.0, k, 77, n, use_ws)
    _assert_support(hist, kept)
    seen = _freq(hist, V) > 0
    if V == 17:
        assert seen.all()  # p >= 0.03 each: (1 - p)^600 < 1e-8
    else:
        rank = logits.argsort(dim=1, descending=True).argsort(dim=1)
        assert (seen & (rank >= 64)).any(dim=1).all(), "only top-ranked ids drawn: something was filtered"
        _assert_freq(f"dec_sample.freq[V={V},k={k},ws={int(use_ws)}]", hist, probs, bucket=188)


@pytest.mark.parametrize("use_ws", [False, True])
def test_dec_sample_top1_is_argmax(use_ws):
    g = torch.Generator().manual_seed(620)
    for i in range(25):  # 25 x 8 rows
        logits = torch.randn(8, 3000, generator=g) * SCALES[:, None]
        hist = _draw(logits.to(DEV), 0.9, 1, 1000 + i, 1, use_ws, pos0=i)
        assert torch.equal(hist[:, 0], logits.argmax(dim=1))


@pytest.mark.parametrize("V,k", [(5000, 64), (5000, 65), (65536, 50), (65537, 50)])
def test_dec_sample_split_boundaries(V, k):
    """With a workspace: top_k 64 | 65 and V 65536 | 65537 are where the split sampler hands
    over to the one-workgroup sampler."""
    logits = _scaled_logits(V, 630 + V + k)[:4]
    kept, probs = R.sample_reference(logits, 0.8, k)
    hist = _draw(logits.to(DEV), 0.8, k, 4321, 1500, True)
    _assert_support(hist, kept)
    _assert_freq(f"dec_sample.freq[V={V},k={k},ws=1]", hist, probs)


@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("k", [0, 8, 50])
def test_dec_sample_never_draws_minus_inf(k, use_ws):
    g = torch.Generator().manual_seed(640)
    logits = torch.randn(4, 3000, generator=g) * 2
    logits[torch.rand(4, 3000, generator=g) < 0.6] = float("-inf")
    logits[3] = float("-inf")
    logits[3, [5, 700, 1500, 2998, 2999]] = torch.tensor([0.0, 1.0, -1.0, 0.5, 2.0])  # fewer finite than k
    kept, probs = R.sample_reference(logits, 1.0, k)
    hist = _draw(logits.to(DEV), 1.0, k, 99, 1000, use_ws)
    assert torch.isfinite(logits.gather(1, hist)).all(), "a -inf logit was drawn"
    _assert_support(hist, kept)
    _assert_freq(f"dec_sample.freq[-inf,k={k},ws={int(use_ws)}]", hist, probs, bucket=1 if k else 188)


@pytest.mark.parametrize("use_ws", [False, True])
def test_dec_sample_cold_temperature(use_ws):
    """T = 0.05 with logits of +-50 (+-1000 after the division): no NaN, always the argmax set."""
    g = torch.Generator().manual_seed(650)
    logits = torch.full((4, 3000), -50.0)
    for b, m in enumerate((1, 3, 20, 60)):
        logits[b, torch.randperm(2999, generator=g)[:m] + 1] = 50.0
    hist = _draw(logits.to(DEV), 0.05, 8, 5, 1000, use_ws)
    _assert_support(hist, logits == 50.0)
    _assert_freq(f"dec_sample.freq[cold,ws={int(use_ws)}]", hist, R.sample_reference(logits, 0.05, 8)[1])


@pytest.mark.parametrize("use_ws", [False, True])
def test_dec_sample_all_equal_row(use_ws):
    """V = 4096 equal logits, k = 8: every slice overflows its candidate list and the window
    search cannot bracket k, so the radix select runs; like torch it keeps all V."""
    logits = torch.full((2, 4096), 1.25)
    kept, probs = R.sample_reference(logits, 1.0, 8)
    assert kept.all()
    hist = _draw(logits.to(DEV), 1.0, 8, 31337, 4000, use_ws)
    _assert_support(hist, kept)
    _assert_freq(f"dec_sample.freq[equal,ws={int(use_ws)}]", hist, probs, bucket=256)


@pytest.mark.parametrize("use_ws", [False, True])
def test_dec_sample_cliff_row(use_ws):
    """49 values in (max - 1, max], 3000 tied at max - 1.5, the rest far below, k = 50: the
    window search oscillates between 49 and 3049 candidates and the radix select runs; the kept
    set is torch's, with every tie at the threshold."""
    g = torch.Generator().manual_seed(660)
    V = 8192
    logits = torch.empty(4, V)
    for b in range(4):
        perm = torch.randperm(V, generator=g)
        logits[b] = -30.0 - 5 * torch.rand(V, generator=g)
        logits[b, perm[:49]] = 4.0 - 0.999 * torch.rand(49, generator=g)
        logits[b, perm[0]] = 4.0
        logits[b, perm[49:3049]] = 2.5
    kept, probs = R.sample_reference(logits, 1.0, 50)
    assert (kept.sum(1) == 3049).all()
    hist = _draw(logits.to(DEV), 1.0, 50, 2718, 4000, use_ws)
    _assert_support(hist, kept)
    _assert_freq(f"dec_sample.freq[cliff,ws={int(use_ws)}]", hist, probs, bucket=512)
    ties = (logits == 2.5) & (_freq(hist, V) > 0)  # 4000 draws, 96 % of them over the 3000 ties
    assert (ties.sum(1) > 1500).all(), "only a part of the ties at the threshold is ever drawn"


@pytest.mark.parametrize("use_ws", [False, True])
def test_dec_sample_bookkeeping(use_ws):
    """ids always written; hist only for 0 <= pos + 1 - hist_base < L; pos untouched by
    dec_sample and advanced by exactly 1 by dec_advance; the draw is a pure function."""
    B, V, L, base = 4, 3000, 4, 10
    logits = _scaled_logits(V, 670)[:B]
    kept, _ = R.sample_reference(logits, 0.7, 8)
    lg = logits.to(DEV)
    ws = hip.dec_sample_workspace(B, DEV) if use_ws else None
    for p in (0, 8, 9, 12, 13, 1000, 2 ** 40):  # before, first / last slot of, after the window
        pos = Guarded((1,), I64, -3, init=torch.tensor([p]))
        ids = [Guarded((B,), I64, -5) for _ in range(2)]
        hist = Guarded((B, L), I64, -7)
        for i in ids:
            hip.dec_sample(lg, 0.7, 8, 42, pos.t, i.t, hist.t, base, ws=ws)
        assert pos.t.item() == p
        assert torch.equal(ids[0].t, ids[1].t), "same (seed, pos, row), another id"
        _assert_support(ids[0].t.cpu()[:, None], kept)
        written = torch.zeros((B, L), dtype=torch.bool, device=DEV)
        if 0 <= p + 1 - base < L:
            written[:, p + 1 - base] = True
            assert torch.equal(hist.t[:, p + 1 - base], ids[0].t)
        hist.assert_guards(written)
        ids[0].assert_guards()
        hip.dec_advance(pos.t)
        assert pos.t.item() == p + 1
        pos.assert_guards()


@pytest.mark.parametrize("use_ws", [False, True])
def test_dec_sample_uniform_corners(use_ws):
    """The hash values whose top 24 bits are all ones / all zeros (u at the top / bottom of the
    cumulative sum): the id is still one of the kept ones.  k logits tied at the max at ids
    != 0, everything else 20 below, so the partial sums are exact small integers."""
    B, V, k = 4, 3000, 8
    g = torch.Generator().manual_seed(680)
    logits = -20.0 - 5 * torch.rand(B, V, generator=g)
    for b in range(B):
        logits[b, torch.randperm(V - 1, generator=g)[:k] + 1] = 3.0
    kept, _ = R.sample_reference(logits, 1.0, k)
    assert (kept.sum(1) == k).all() and not kept[:, 0].any()
    lg = logits.to(DEV)
    ws = hip.dec_sample_workspace(B, DEV) if use_ws else None
    for p in (0, 7):
        for b in (0, 3):
            for bits in (0xFFFFFF, 0):
                seed = R.seed_for_bits(p, b, bits)
                assert R.draw_hash(seed, p, b) >> 8 == bits
                ids = torch.full((B,), -1, dtype=I64, device=DEV)
                hist = torch.full((B, 1), -1, dtype=I64, device=DEV)
                hip.dec_sample(lg, 1.0, k, seed, _pos(p), ids, hist, 0, ws=ws)
                got = ids.cpu()
                print(f"CORNER ws={int(use_ws)} pos={p} b={b} bits={bits:#x} id={got[b].item()} "
                      f"kept={kept[b].nonzero().flatten().tolist()}")
                assert kept[b, got[b]], f"pos={p} b={b} bits={bits:#x}: id {got[b].item()} is not a kept one"
                _assert_support(got[:, None], kept)
