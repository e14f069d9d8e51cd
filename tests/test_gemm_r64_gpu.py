"""The 64-granular GEMM (ops/csrc/gemm_r64.hip: 256 x 128 main tiles, a 256 x 64 tail tile, a
ring of 64-wide K-tiles) against gemm_ref's fp64 product and derived tolerance, both operand
forms, every element, with sentinel guards around a NaN-filled output.  On the ``int`` family
the tolerance is zero: the output is round_to(ref) bit for bit."""
import pytest
import torch

from distributed_llm_trainer_amd.ops import gemm, hip
from tests import gemm_ref as R
from tests.gemm_ref import DTYPES, Guarded, gemm_ref, operands

pytestmark = pytest.mark.gpu
DEV = "cuda"
BN = 128  # the kernel's main column tile
# (M, N, K): widths 64 (a tail only), BN + 64, 2 BN + 64 and 2 BN; reductions 128, 192 (an odd
# number of K-tiles) and 320; one and two row tiles
EDGES = ((256, 64, 128), (256, BN + 64, 192), (512, 2 * BN + 64, 320), (512, 2 * BN, 128), (256, 2 * BN + 64, 192),
         (512, 64, 320), (256, BN + 64, 128))
# the gpt2_xl projections at M = 256, (form, output columns, reduction)
XL = (("tn", 1600, 1600), ("tn", 4800, 1600), ("tn", 1600, 6400), ("nn", 1600, 4800), ("nn", 1600, 1600),
      ("nn", 1600, 12800), ("nn", 6400, 1600), ("nn", 1600, 50304))
REFUSED = ((256, 96, 128), (256, 128, 160), (256, 128, 64), (128, 128, 128))


def problem(M, N, K, dt, family):
    P, Q = operands(M * 31 + N * 7 + K, M, N, K, family, dt)
    return P.to(DEV), Q.to(DEV), gemm_ref(P, Q, family)


def run(form, P, Q, **kw):
    """P [M, K], Q [N, K] -> the guarded output of the form's launcher (None where it refuses)."""
    G = Guarded((P.shape[0], Q.shape[0]), P.dtype, 776.0, DEV, init=torch.full((P.shape[0], Q.shape[0]), float("nan")))
    if form == "tn":
        out = hip.gemm_r64(P, Q, out=G.t, **kw)
    else:
        out = hip.gemm_r64_dgrad(P, Q.t().contiguous(), out=G.t, **kw)
    return G, out


def check(name, G, chk, dt):
    G.assert_guards()
    out = G.t.cpu().double()
    want = torch.where(chk.tol == 0, R.round_to(chk.ref, dt).double(), chk.ref)
    bad = ~((out - want).abs() <= chk.tol)  # an unwritten (NaN) element is bad
    print(f"RATIO {name} {torch.where(chk.tol > 0, (out - want).abs() / chk.tol, (out - want).abs()).max().item():.4f}")
    assert not bad.any(), f"{name}: {bad.sum().item()} of {bad.numel()} elements outside the tolerance, first {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("family", ("gauss", "int"))
@pytest.mark.parametrize("dt", DTYPES, ids=("bf16", "fp16"))
@pytest.mark.parametrize("shape", EDGES, ids=lambda s: "x".join(map(str, s)))
def test_tiling_edges(shape, dt, family):
    """Both forms; then a grid of 2 workgroups (more tiles than workgroups wherever there are
    three tiles or more: main and tail tiles in one workgroup's walk) and a second call, bit for bit."""
    P, Q, chk = problem(*shape, dt, family)
    for form in ("tn", "nn"):
        G, out = run(form, P, Q)
        assert out is not None
        check(f"{form} {shape}", G, chk, dt)
        for kw in ({"grid": 2}, {}):
            G2, _ = run(form, P, Q, **kw)
            G2.assert_guards()
            assert torch.equal(R.bits(G2.t), R.bits(G.t)), f"{form} {shape} {kw}: not the first call's bits"


# (the long reduction runs on the exact family only)
@pytest.mark.parametrize("form,N,K,family", [(*c, f) for c in XL for f in ("gauss", "int") if c[2] < 50304 or f == "int"],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("dt", DTYPES, ids=("bf16", "fp16"))
def test_xl_shapes(form, N, K, family, dt):
    P, Q, chk = problem(256, N, K, dt, family)
    G, out = run(form, P, Q)
    assert out is not None
    check(f"{form} 256x{N}x{K}", G, chk, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=("bf16", "fp16"))
def test_same_bits_as_the_persistent_kernel(dt):
    """A shape both kernels tile, exact inputs: the new kernel's bits are the old kernel's."""
    P, Q, _ = problem(256, 384, 256, dt, "int")
    assert torch.equal(run("tn", P, Q)[0].t, hip.gemm_bf16(P, Q))
    assert torch.equal(run("nn", P, Q)[0].t, hip.gemm_dgrad(P, Q.t().contiguous()))


@pytest.mark.parametrize("shape", REFUSED, ids=lambda s: "x".join(map(str, s)))
def test_refused_shapes_launch_nothing(shape):
    M, N, K = shape
    P, Q = (torch.ones(r, K, dtype=torch.bfloat16, device=DEV) for r in (M, N))
    for form in ("tn", "nn"):
        G, out = run(form, P, Q)
        assert out is None
        G.assert_guards(written=torch.zeros(M, N, dtype=torch.bool, device=DEV))
        fn = hip.lib().dlt_gemm_r64 if form == "tn" else hip.lib().dlt_gemm_r64_nn
        assert fn(hip._p(P), hip._p(Q), hip._p(G.t), M, N, K, 0, 0, hip._stream()) == -1


def test_routing(monkeypatch):
    """A planted "r64" / dgrad pick runs the new kernel; shapes another kernel tiles never race it."""
    M, N, K = 256, 320, 192
    x, w, _ = problem(M, N, K, torch.bfloat16, "gauss")
    g = gemm.HipGemm()
    assert g._tn_candidates(M, N, K) == ["r64"] and "r64" not in g._tn_candidates(256, 384, 256)
    assert "r64" not in g._tn_candidates(256, 128, 192)  # fw4 alone fits
    assert g._dgrad_hand(256, 384, 256) is hip.gemm_dgrad

    def no_library(*a, **k):
        raise AssertionError("routed to the library")
    monkeypatch.setattr(g, "_lib_linear", no_library)
    monkeypatch.setattr(g, "_lib_dgrad", no_library)
    monkeypatch.setitem(g._choice, (M, N, K), "r64")
    assert torch.equal(g.linear(x, w), hip.gemm_r64(x, w))
    wt = w.t().contiguous()  # dy [M, K] @ wt [K, N]: Nout = N, Nred = K
    monkeypatch.setitem(g._choice, ("dgrad", M, N, K), True)
    assert torch.equal(g.linear_dgrad(x, wt), hip.gemm_r64_dgrad(x, wt))
    assert g.report_choices()[f"M{M}xN{N}xK{K}"] == "hand-written gemm_r64"
    assert g.report_choices()[f"dgrad M{M}xN{N}xK{K}"] == "hand-written gemm_r64"
