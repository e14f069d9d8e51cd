"""Nucleus (top-p) and min-p sampling without a GPU: the fp64 reference of
tests/sample_p_ref.py against a brute-force definition, the host helper ``filter_logits`` and
a numpy model of the kernel's select against the reference at every input the GPU tests use,
planted defects that must each be told apart, and the arguments through ``GPT.generate``,
``kv_cached_generate`` and ``infer.py``."""
import copy
import math

import numpy as np
import pytest
import torch

from distributed_llm_trainer_amd.eval import infer
from distributed_llm_trainer_amd.eval.decode import filter_logits, kv_cached_generate
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from tests import sample_p_ref as P


# ----------------------------------------------------------------------- the reference
@pytest.mark.parametrize("top_k,top_p,min_p,T", [(0, 0.5, 0.0, 1.0), (5, 0.9, 0.0, 2.0), (0, 1.0, 0.3, 0.5),
                                                 (7, 0.3, 0.1, 1.0), (3, 0.999, 0.0, 0.05), (0, 0.05, 0.5, 2.0)])
def test_reference_against_the_brute_force_definition(top_k, top_p, min_p, T):
    g = torch.Generator().manual_seed(int(top_k + 100 * top_p + 10 * min_p))
    logits = torch.randn(6, 23, generator=g) * 2
    logits[1, :4] = logits[1, 4]      # ties
    logits[2, 5:15] = float("-inf")
    logits[3] = 0.5                   # everything tied
    logits[4, 3:] = float("-inf")     # 3 finite values
    cl = P.classify(logits, T, top_k, top_p, min_p)
    x = P.scaled(logits, T)
    for b in range(logits.shape[0]):
        want = torch.from_numpy(P.brute_force(x[b], top_k, top_p, min_p))
        decided = ~cl.either[b]
        assert torch.equal(cl.must_keep[b][decided], want[decided]), b
        assert decided.sum() >= 21
    assert cl.must_keep[3].all() and cl.must_keep.any(dim=1).all()
    assert torch.allclose(cl.probs.sum(1), torch.ones(6, dtype=torch.float64))


def test_the_bands_are_the_sum_of_their_terms_and_small():
    x = np.array([0.0, -1.0, -3.0, -50.0, -2000.0])
    inK = np.ones(5, bool)
    dp = P.delta_p(x, inK)
    assert 2 ** -22 < dp < 1e-5
    assert P.delta_p(x * 0, inK) == pytest.approx(2 * 2.0 ** -22 + (2 * 5 + 1) * 2.0 ** -40 / 5 + 2.0 ** -52)
    assert P.delta_m(0.0, 0.5) == pytest.approx(1.01 * math.log(2) * (2.0 ** -22 + 2.0 ** -24))
    assert P.delta_m(1000.0, 0.05) < 1e-4


def test_expected_kept_sets_of_the_constructed_rows():
    """What each constructed row is for, checked on the reference itself."""
    keep = {n: P.cases()[n].classes.must_keep for n in P.CASE_NAMES}
    for n in ("all-equal-V17", "all-equal-V1000", "all-equal-overflow"):
        assert keep[n].all(), n
    assert (keep["cliff-p0.5"].sum(1) == 3049).all()            # the ties at the threshold are in
    assert keep["two-ties-straddle"].sum() == 3 and keep["three-ties-straddle"].sum() == 4
    assert keep["three-ties-straddle-V50257"].sum() == 4
    row = P.cases()["bf16-step-below-boundary"].logits[0]
    v = torch.topk(row, 3).values
    assert keep["bf16-step-below-boundary"].sum() == 2 and v[2].item() == P.bf16_step_below(v[1].item())
    assert (keep["peaked99-p0.9"].sum(1) == 1).all() and (keep["peaked50-p0.9"].sum(1) > 100).all()
    assert (keep["nucleus-inside-topk"].sum(1) < 50).all() and (keep["nucleus-inside-topk"].sum(1) > 1).all()
    c = P.cases()["topk-cuts-nucleus"]  # without top-k the same nucleus is far larger
    assert (keep["topk-cuts-nucleus"].sum(1) == 50).all()
    assert (P.classify(c.logits, c.T, 0, c.top_p, 0.0).must_keep.sum(1) > 1000).all()
    assert keep["minus-inf-k50"][3].sum() <= 5  # the row with fewer finite values than top_k
    for n in ("minus-inf-k0", "minus-inf-k50"):
        assert torch.isfinite(P.cases()[n].logits[keep[n]]).all()
    assert {c.top_p for c in P.cases().values()} >= set(P.TOP_PS)
    grid = [c for c in P.cases().values() if c.name.startswith("zipf")]
    for a, b in (("top_p", "min_p"), ("top_p", "T"), ("min_p", "T")):  # every pair of values occurs
        va, vb = ({getattr(c, f) for c in grid} for f in (a, b))
        assert {(getattr(c, a), getattr(c, b)) for c in grid} == {(p, q) for p in va for q in vb}
    assert {c.min_p for c in grid} == set(P.MIN_PS) and {c.T for c in grid} == set(P.TEMPS)
    assert {(c.logits.shape[1], c.logits.shape[0]) for c in grid} == {(V, B) for V in P.VS for B in P.BS}


# ------------------------------------------------------------- helper and kernel model
@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_filter_logits_keeps_the_reference_set(name):
    c = P.cases()[name]
    cl = c.classes  # asserts that the either band is empty
    lg = torch.from_numpy(P.scaled(c.logits, c.T))
    kept = torch.isfinite(filter_logits(lg, c.top_k, c.top_p, c.min_p))
    assert torch.equal(kept, cl.must_keep)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_kernel_model_keeps_the_reference_set(name):
    """fp32 exponentials, fixed-point masses and the radix descent decide as the reference does."""
    c = P.cases()[name]
    assert torch.equal(P.kernel_model(c.logits, c.T, c.top_k, c.top_p, c.min_p), c.classes.must_keep)


@pytest.mark.parametrize("defect", P.DEFECTS)
def test_planted_defects_are_told_apart(defect):
    """Each defect changes the kept set of at least one input of the GPU tests, so the support
    check there (ids only from must_keep, every likely id of must_keep seen) can tell it.
    (A float-mass defect -- sums in a permuted order giving another threshold -- is not
    planted: no input here has a boundary within an fp32 sum's reordering error, that is what
    the empty either band says.)"""
    hit = []
    for name, c in P.cases().items():
        if c.logits.shape[1] > 1000 and len(hit) > 0:
            continue  # one hit is enough: skip the large rows once found
        if not torch.equal(P.kernel_model(c.logits, c.T, c.top_k, c.top_p, c.min_p, defect), c.classes.must_keep):
            hit.append(name)
    print(f"DEFECT {defect}: {hit}")
    assert hit, f"{defect}: no input of the GPU tests shows it"


def test_filter_logits_defaults_are_the_top_k_code():
    lg = torch.randn(3, 50, generator=torch.Generator().manual_seed(1))
    v, _ = torch.topk(lg, 7)
    want = lg.masked_fill(lg < v[:, [-1]], float("-inf"))
    assert torch.equal(filter_logits(lg, 7), want) and torch.equal(filter_logits(lg, 7, 1.0, 0.0), want)
    assert filter_logits(lg, 0) is lg


# --------------------------------------------------------------------------- generation
TINY = dict(vocab_size=256, hidden_size=64, num_layers=2, num_heads=4, max_seq_len=32, dropout=0.0,
            attention_dropout=0.0)


@pytest.fixture(scope="module")
def models():
    torch.manual_seed(3)
    eager = GPT(GPTConfig(**TINY)).eval()
    eng = copy.deepcopy(eager)
    eng.enable_engine()
    return eager, eng


def _gen(m, ids, seed=11, **kw):
    torch.manual_seed(seed)
    return m.generate(ids, max_new_tokens=8, **kw)


@pytest.mark.parametrize("which", [0, 1])
def test_generate_defaults_change_nothing(models, which):
    m = models[which]
    ids = torch.randint(0, 256, (2, 5), generator=torch.Generator().manual_seed(2))
    want = _gen(m, ids, temperature=0.9, top_k=20)
    assert torch.equal(_gen(m, ids, temperature=0.9, top_k=20, top_p=1.0, min_p=0.0), want)
    if which:
        torch.manual_seed(11)
        assert torch.equal(kv_cached_generate(m, ids, 8, 0.9, 20), want)
        torch.manual_seed(11)
        assert torch.equal(kv_cached_generate(m, ids, 8, 0.9, 20, top_p=1.0, min_p=0.0), want)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("kw", [dict(top_p=1e-6), dict(min_p=1 - 1e-9), dict(top_p=1e-6, min_p=0.5)])
def test_a_one_token_nucleus_is_greedy(models, which, kw):
    """top_p below every top probability / min_p that no runner-up reaches: the top_k = 1 ids."""
    m = models[which]
    ids = torch.randint(0, 256, (2, 5), generator=torch.Generator().manual_seed(4))
    greedy = _gen(m, ids, top_k=1)
    with torch.no_grad():  # the premise: no step has two logits tied at the top
        lg = m(greedy[:, :-1])[0][:, 4:]
    top2 = torch.topk(lg.float(), 2).values
    assert (top2[..., 0] - top2[..., 1]).min() > 1e-6
    assert torch.equal(_gen(m, ids, top_k=0, **kw), greedy)
    assert torch.equal(_gen(m, ids, top_k=20, temperature=1.3, **kw), greedy)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("kw", [dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1), dict(top_p=float("nan")),
                                dict(top_p=float("inf")), dict(min_p=1.0), dict(min_p=-0.1), dict(min_p=float("nan")),
                                dict(min_p=float("inf"))])
def test_invalid_values_raise(models, which, kw):
    ids = torch.zeros(1, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="top_p|min_p"):
        models[which].generate(ids, max_new_tokens=2, **kw)
    with pytest.raises(ValueError, match="top_p|min_p"):
        filter_logits(torch.zeros(1, 4), 0, **kw)
    if which:
        with pytest.raises(ValueError, match="top_p|min_p"):
            kv_cached_generate(models[1], ids, 2, **kw)


# ----------------------------------------------------------------------------- infer.py
def test_infer_passes_the_flags_through(monkeypatch):
    seen = {}

    class Model:
        def generate(self, ids, **kw):
            seen.update(kw)
            return ids

    monkeypatch.setattr(infer, "load_model", lambda *a, **k: Model())
    base = ["--checkpoint", "x.pt", "--tokenizer", "byte", "--device", "cpu", "--prompt", "ab"]
    infer.main(base)
    assert seen["top_p"] == 1.0 and seen["min_p"] == 0.0 and seen["top_k"] == 50
    infer.main(base + ["--top_p", "0.9", "--min_p", "0.05", "--top_k", "0", "--temperature", "0.7"])
    assert seen == dict(max_new_tokens=50, temperature=0.7, top_k=0, top_p=0.9, min_p=0.05)
    with pytest.raises(SystemExit):
        infer.main(base + ["--top_p", "much"])
