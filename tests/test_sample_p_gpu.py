"""Nucleus (top-p) and min-p sampling on the device (``dec_sample(..., top_p=, min_p=)``,
ops/csrc/decode.hip) against the fp64 reference of tests/sample_p_ref.py, on the three paths:
the whole-row sampler (top_k = 0), top-k without a workspace, and the split top-k sampler with
its workspace; then ``generate`` end to end on both fused decode steps.

Every input has an EMPTY ``either`` band (asserted where it is built, and again on the CPU in
test_sample_p_cpu.py), so "every id lies in must_keep" is exact."""
import functools
import math

import pytest
import torch

from distributed_llm_trainer_amd.eval.decode import _fused_kind, filter_logits
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip
from tests import decode_ref as R
from tests import sample_p_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
I64 = torch.int64
PAD = 64
N_SUPPORT = 512  # draws of the support check (the issue's n)
N_FREQ = 3000    # draws of the frequency check: 2 launches x 3000 of at most ~0.3 ms, about a second


def _paths(top_k):
    """(use_ws, name): top_k = 0 is the whole-row path whether or not a workspace is passed."""
    return [(False, "whole-row")] if top_k == 0 else [(False, "topk"), (True, "topk-split")]


CASE_PATHS = [(n, ws) for n in P.CASE_NAMES for ws, _ in _paths(P.cases()[n].top_k)]


@functools.lru_cache(maxsize=None)
def _dev_logits(name):
    return P.cases()[name].logits.to(DEV)


def _draw(c, n, use_ws, seeds=(20240607,), pos0=0, **override):
    """n draws per row over positions pos0.. and the given seeds in turn -> [B, n] on the host."""
    lg = _dev_logits(c.name)
    B = lg.shape[0]
    kw = dict(top_p=c.top_p, min_p=c.min_p)
    kw.update(override)
    ids = torch.full((B,), -1, dtype=I64, device=DEV)
    hist = torch.full((B, n), -1, dtype=I64, device=DEV)
    pos = torch.tensor([pos0], dtype=I64, device=DEV)
    ws = hip.dec_sample_workspace(B, DEV) if use_ws else None
    for i in range(n):
        hip.dec_sample(lg, c.T, c.top_k, seeds[i % len(seeds)], pos, ids, hist, pos0 + 1, ws=ws, **kw)
        hip.dec_advance(pos)
    assert pos.item() == pos0 + n
    return hist.cpu()


def _freq(hist, V):
    f = torch.zeros(hist.shape[0], V, dtype=torch.float64)
    f.scatter_add_(1, hist, torch.ones(hist.shape, dtype=torch.float64))
    return f / hist.shape[1]


# ------------------------------------------------------------------------------ support
@pytest.mark.parametrize("name,use_ws", CASE_PATHS)
def test_support(name, use_ws):
    """512 draws over varying pos and seed: every id is in must_keep, and every token of
    must_keep with probability > 20 / n is drawn (it is missed with probability < e^-20)."""
    c = P.cases()[name]
    cl = c.classes
    V = c.logits.shape[1]
    hist = _draw(c, N_SUPPORT, use_ws, seeds=(20240607, 77, 4321))
    assert ((hist >= 0) & (hist < V)).all(), "an id outside [0, V)"
    ok = cl.must_keep.gather(1, hist)
    assert ok.all(), f"{(~ok).sum().item()} draws outside the kept set, e.g. id {hist[~ok][0].item()}"
    likely = cl.must_keep & (cl.probs > 20.0 / N_SUPPORT)
    seen = _freq(hist, V) > 0
    print(f"SUPPORT {name} ws={int(use_ws)} kept/row={cl.must_keep.sum(1).tolist()} likely/row={likely.sum(1).tolist()} "
          f"seen/row={seen.sum(1).tolist()}")
    missed = likely & ~seen
    assert not missed.any(), f"{missed.sum().item()} likely kept tokens never drawn, e.g. {missed.nonzero()[0].tolist()}"


# -------------------------------------------------------------------------- frequencies
@pytest.mark.parametrize("name,use_ws", [(n, ws) for n, ws in CASE_PATHS if n in P.FREQ_CASES])
def test_frequencies(name, use_ws):
    """n = 3000 draws: every token's frequency within decode_ref.freq_bound of the reference
    probability (per 512 consecutive ids where a row keeps thousands, as the plain sampler's
    cliff test buckets them: the bound is a normal-tail one and needs n * p of a few draws)."""
    c = P.cases()[name]
    probs = c.classes.probs
    hist = _draw(c, N_FREQ, use_ws)
    bucket = 512 if c.classes.must_keep.sum(1).max() > 1000 else 1
    if bucket > 1:
        nb = -(-probs.shape[1] // bucket)
        idx = (torch.arange(probs.shape[1]) // bucket).expand(probs.shape[0], -1)
        probs = torch.zeros(probs.shape[0], nb, dtype=torch.float64).scatter_add_(1, idx, probs)
        hist = torch.div(hist, bucket, rounding_mode="floor")
    dev = (_freq(hist, probs.shape[1]) - probs).abs() / R.freq_bound(probs, N_FREQ)
    print(f"RATIO dec_sample_p.freq[{name},ws={int(use_ws)}] {dev.max().item():.4f}")
    assert (dev <= 1).all(), f"worst |freq - p| / bound = {dev.max().item():.3f}"


# ------------------------------------------------------------------------------ bitwise
@pytest.mark.parametrize("name,use_ws", [("zipf-p0.5-m0.05-T2.0-V1000-B8-k0", False), ("nucleus-inside-topk", False),
                                         ("nucleus-inside-topk", True), ("cliff-p0.5", True)])
def test_two_identical_calls_give_identical_ids(name, use_ws):
    c = P.cases()[name]
    a, b = _draw(c, 64, use_ws), _draw(c, 64, use_ws)
    assert torch.equal(a, b)
    assert (a != a[:, :1]).any(), "64 draws, one id: the comparison would show nothing"


@pytest.mark.parametrize("name,use_ws", [("zipf-p0.5-m0.05-T2.0-V1000-B8-k0", False), ("nucleus-inside-topk", False),
                                         ("nucleus-inside-topk", True),
                                         ("zipf-p0.999-m0.5-T2.0-V50257-B8-k50", True)])
def test_explicit_defaults_are_the_plain_sampler(name, use_ws):
    """top_p = 1.0, min_p = 0.0 passed explicitly == the call without them, bit for bit."""
    c = P.cases()[name]
    lg = _dev_logits(name)
    B = lg.shape[0]
    out = []
    for kw in ({}, dict(top_p=1.0, min_p=0.0)):
        ids = torch.full((B,), -1, dtype=I64, device=DEV)
        hist = torch.full((B, 64), -1, dtype=I64, device=DEV)
        pos = torch.tensor([0], dtype=I64, device=DEV)
        ws = hip.dec_sample_workspace(B, DEV) if use_ws else None
        for _ in range(64):
            hip.dec_sample(lg, c.T, c.top_k, 99, pos, ids, hist, 1, ws=ws, **kw)
            hip.dec_advance(pos)
        out.append((ids.cpu(), hist.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    kept = c.classes.must_keep
    assert not kept.gather(1, out[0][1]).all(), "no draw outside the nucleus: the filter was not off"


@pytest.mark.parametrize("kw", [dict(top_p=0.0), dict(top_p=1.0001), dict(top_p=float("nan")), dict(min_p=1.0),
                                dict(min_p=-1e-3), dict(min_p=float("inf"))])
def test_invalid_values_raise_on_the_host(kw):
    c = P.cases()["all-equal-V17"]
    with pytest.raises(ValueError, match="top_p|min_p"):
        _draw(c, 1, False, **kw)


# ------------------------------------------------------------------------- write guards
class Guarded:
    """A tensor that is a view into a larger sentinel-filled allocation."""

    def __init__(self, shape, dtype, fill, init=None):
        n = math.prod(shape)
        self.buf = torch.full((PAD + n + PAD + (-n) % 8,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n].view(shape)
        if init is not None:
            self.t.copy_(init)
        self.before = self.buf.clone()

    def assert_guards(self, written=None):
        want = self.before.clone()
        wv = want[PAD:PAD + self.t.numel()].view(self.t.shape)
        if written is None:
            wv.copy_(self.t)
        else:
            wv[written] = self.t[written]
        diff = (self.buf != want).nonzero().flatten()
        assert diff.numel() == 0, f"{diff.numel()} elements outside the output changed, first at {diff[0].item() - PAD}"


@pytest.mark.parametrize("name,use_ws", [("zipf-p0.5-m0.05-T2.0-V1000-B8-k0", False), ("nucleus-inside-topk", False),
                                         ("nucleus-inside-topk", True), ("all-equal-overflow", True)])
def test_write_guards(name, use_ws):
    """ids always written, hist only at pos + 1 - hist_base, pos and the workspace's
    surroundings untouched."""
    c = P.cases()[name]
    lg = _dev_logits(name)
    B, L, base = lg.shape[0], 4, 10
    kept = c.classes.must_keep
    ws = Guarded((hip.dec_sample_workspace(B, DEV).numel(),), torch.int32, -9) if use_ws else None
    for p in (0, 8, 9, 12, 13, 2 ** 40):  # before, first / last slot of, after the window
        pos = Guarded((1,), I64, -3, init=torch.tensor([p]))
        ids = Guarded((B,), I64, -5)
        hist = Guarded((B, L), I64, -7)
        hip.dec_sample(lg, c.T, c.top_k, 42, pos.t, ids.t, hist.t, base, ws=ws.t if ws else None, top_p=c.top_p,
                       min_p=c.min_p)
        assert pos.t.item() == p
        got = ids.t.cpu()
        assert kept.gather(1, got[:, None]).all()
        written = torch.zeros((B, L), dtype=torch.bool, device=DEV)
        if 0 <= p + 1 - base < L:
            written[:, p + 1 - base] = True
            assert torch.equal(hist.t[:, p + 1 - base], ids.t)
        hist.assert_guards(written)
        ids.assert_guards()
        pos.assert_guards()
        if ws:
            ws.assert_guards()


# --------------------------------------------------------------------------- end to end
def _cfg(nkv):
    return GPTConfig(vocab_size=1000, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=nkv, max_seq_len=256,
                     dropout=0.0, attention_dropout=0.0)


@functools.lru_cache(maxsize=None)
def _model(nkv):
    torch.manual_seed(5 + nkv)
    m = GPT(_cfg(nkv)).to(DEV)
    m.enable_engine()
    m.eval()
    return m


def _generate(m, ids, **kw):
    torch.manual_seed(123)
    return m.generate(ids, max_new_tokens=12, **kw)


@pytest.mark.parametrize("env", [{"DLT_DECODE_DEVICE_LOOP": "1"}, {"DLT_DECODE_DEVICE_LOOP": "0"},
                                 {"DLT_DECODE_GRAPH": "0"}])
@pytest.mark.parametrize("nkv,kind", [(4, "mha"), (2, "gqa")])
def test_generate_with_a_one_token_nucleus_is_greedy(nkv, kind, env, monkeypatch):
    """top_p below every top probability: the ids of top_k = 1 on that same path."""
    m = _model(nkv)
    assert _fused_kind(m, 2) == kind
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ids = torch.randint(0, 1000, (2, 20), generator=torch.Generator().manual_seed(7)).to(DEV)
    greedy = _generate(m, ids, top_k=1)
    assert torch.equal(_generate(m, ids, top_k=50, top_p=1e-6), greedy)
    assert torch.equal(_generate(m, ids, top_k=0, top_p=1e-6, temperature=1.3), greedy)
    assert torch.equal(_generate(m, ids, top_k=0, min_p=1 - 1e-7), greedy)


@pytest.mark.parametrize("nkv", [4, 2])
def test_generate_top_p_ids_lie_in_the_helpers_kept_set(nkv):
    """top_p = 0.9 at T = 0.25 (the tiny model's logits are flat: a cold draw gives a nucleus
    that excludes much of the vocabulary): every generated id is kept by filter_logits on the
    logits of a re-forward -- or its logit is within the near-tie margin (0.05) of the kept
    set's smallest that test_qknorm_gpu.py::test_generate_runs_on_the_aten_step allows the
    argmax, for the same reason: the re-forward is not the decode step's arithmetic."""
    m = _model(nkv)
    n0, T = 20, 0.25
    ids = torch.randint(0, 1000, (2, n0), generator=torch.Generator().manual_seed(8)).to(DEV)
    torch.manual_seed(321)
    out = m.generate(ids, max_new_tokens=12, temperature=T, top_k=0, top_p=0.9)
    assert out.shape == (2, n0 + 12)
    sizes = []
    for t in range(12):
        with torch.no_grad():
            lg = m(out[:, :n0 + t])[0][:, -1].float() / T
        f = filter_logits(lg, 0, 0.9, 0.0)
        kept = torch.isfinite(f)
        sizes.append(kept.sum(1).tolist())
        thr = f.masked_fill(~kept, float("inf")).amin(dim=1)
        got = lg.gather(1, out[:, n0 + t][:, None])[:, 0]
        assert ((got >= thr) | ((thr - got) * T < 0.05)).all(), (t, got.tolist(), thr.tolist())
    print(f"E2E kept sizes {sizes}")
    assert max(max(s) for s in sizes) < 900, "the nucleus excluded next to nothing"
