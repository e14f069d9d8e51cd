"""The hand-written GEMM kernels (ops/csrc/gemm_bf16.hip, gemm_fw4.hip, gemm_wgrad.hip and the
split-K sums) against the fp64 references and derived tolerances of tests/gemm_ref.py: every
element of every output, at the smallest shapes that reach each launch path (the dispatch model
of gemm_ref, confirmed in test_gemm_kernels_cpu.py), with sentinel guards around every output,
under every flag set the project ships.  Outputs under different flags, caps, schedules and
routes must also be bit-equal to each other.  On the ``int`` family the tolerance is zero: the
output is round_to(ref) bit for bit.

Each check prints ``RATIO <name> <worst err / tol>`` (and ``BIAS`` on the gauss family of the
plain GEMMs); ``pytest -s`` shows them."""
import contextlib
import ctypes

import pytest
import torch

from distributed_llm_trainer_amd.ops import hip
from tests import gemm_ref as R
from tests.stream_ref import BF, DT_NAME, DTYPES, F32, HF

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = {BF: 776.0, HF: 776.0, F32: -7.5}
ID = lambda c: c.name


def check(name, out, chk, dt, bias=False):
    out = out.detach().cpu().double().reshape(chk.ref.shape)
    want = torch.where(chk.tol == 0, R.round_to(chk.ref, dt).double(), chk.ref)
    err = (out - want).abs()
    bad = ~(err <= chk.tol)
    ratio = torch.where(chk.tol > 0, err / chk.tol, err).max().item()
    exact = " exact" if not (chk.tol > 0).any() and not bad.any() else ""
    print(f"RATIO {name} {ratio:.4f}{exact}")
    assert not bad.any(), (f"{name}: {bad.sum().item()} of {bad.numel()} elements outside the tolerance, "
                           f"worst err/tol {ratio:.3f} at {bad.nonzero()[0].tolist()}")
    if bias:
        b = R.bias_ratio(out, chk)
        print(f"BIAS {name} {b:.4f}")
        assert b < 1.0, f"{name}: the errors lean one way ({b:.2f} of the bound): something truncates"
    return ratio


def guarded(shape, dt, init=None):
    return R.Guarded(tuple(shape), dt, SENT[dt], DEV, init=None if init is None else init.to(DEV))


def untouched(*gs):
    for g in gs:
        g.assert_guards(written=torch.zeros(g.t.shape, dtype=torch.bool, device=DEV))


def same_bits(a, b, what):
    assert torch.equal(R.bits(a), R.bits(b)), f"{what}: outputs differ in {(R.bits(a) != R.bits(b)).sum().item()} elements"


@contextlib.contextmanager
def gb(flags, cap=0):
    """Launch flags and grid cap of the k_gemm_bf16 forms for the calls inside."""
    f0, o0 = hip._GB_FLAGS, hip._GB_FWD_OVERRIDE
    try:
        hip._GB_FWD_OVERRIDE = None
        hip._GB_FLAGS = flags & hip._GB_FLAG_BITS
        hip.gemm_grid_cap(cap)
        yield
    finally:
        hip._GB_FLAGS, hip._GB_FWD_OVERRIDE = f0, o0


def test_flag_sets_are_the_shipped_ones():
    assert R.GB_DEFAULT_FLAGS == hip._GB_DEFAULT_FLAGS
    assert all(f & ~hip._GB_FLAG_BITS == 0 for f in R.gb_flag_sets(late=True))


# ------------------------------------------------------------------- gemm_bf16 / gemm_dgrad
def _run_gb(c, P, Q, out):
    if c.kernel == "gemm_bf16":
        return hip.gemm_bf16(P, Q, out=out)
    return hip.gemm_dgrad(P, Q, out=out)


@pytest.mark.parametrize("c", R.GB_CASES, ids=ID)
def test_gemm_bf16_and_dgrad(c):
    Pc, Qc, chk = R.gemm_case(c)
    P = Pc.to(DEV)
    Q = (Qc if c.kernel == "gemm_bf16" else Qc.t().contiguous()).to(DEV)
    first = None
    for flags, cap in [(f, c.cap) for f in R.gb_flag_sets()] + [(R.GB_DEFAULT_FLAGS, 0), (R.GB_DEFAULT_FLAGS, 16)]:
        G = guarded((c.M, c.N), c.dt)
        with gb(flags, cap):
            assert _run_gb(c, P, Q, G.t) is not None
        G.assert_guards()
        if first is None:
            first = G.t.clone()
            check(c.name, first, chk, c.dt, bias=c.family == "gauss")
        else:
            same_bits(G.t, first, f"{c.name} flags {flags} cap {cap}")


@pytest.mark.parametrize("c", R.LD_CASES, ids=ID)
def test_leading_dimensions(c):
    """lda / ldb / ldc larger than the row length (by c.cap): the C entry points, the output in a
    guarded 2-D buffer whose gap columns must stay as they were."""
    a, b, chk = R.ld_case(c)
    a, b, pad = a.to(DEV), b.to(DEV), c.cap
    fn = hip.lib().dlt_gemm_bf16_tn if c.kernel == "gemm_bf16" else hip.lib().dlt_gemm_bf16_nn
    written = (torch.arange(c.N + pad, device=DEV) < c.N).view(1, -1).expand(c.M, -1)
    for flags in (R.GB_DEFAULT_FLAGS, R.GB_DEFAULT_FLAGS & ~1024):
        G = guarded((c.M, c.N + pad), c.dt)
        rc = fn(hip._p(a), hip._p(b), hip._p(G.t), c.M, c.N, c.K, a.stride(0), b.stride(0), c.N + pad, flags,
                hip._WG_HK[c.dt], hip._stream())
        assert rc == 0
        G.assert_guards(written=written)
        check(f"ld+{pad} {c.name} flags {flags}", G.t[:, :c.N], chk, c.dt)


# ---------------------------------------------------------------------------------- gemm_fw4
@pytest.mark.parametrize("c", R.FW4_CASES, ids=ID)
def test_gemm_fw4(c):
    Pc, Qc, chk = R.gemm_case(c)
    P, Q = Pc.to(DEV), Qc.to(DEV)
    tiles = (c.M // 256) * ((c.N + 255) // 256)
    first = None
    for flags in R.FW4_FLAGS + (R.FW4_TWO if tiles % 16 == 0 else ()):
        assert R.fw4_plan(c.M, c.N, flags) is not None
        G = guarded((c.M, c.N), c.dt)
        assert hip.gemm_fw4(P, Q, out=G.t, flags=flags) is not None
        G.assert_guards()
        if first is None:
            first = G.t.clone()
            check(c.name, first, chk, c.dt, bias=c.family == "gauss")
        else:
            same_bits(G.t, first, f"{c.name} flags {flags}")
    if tiles % 16:
        G = guarded((c.M, c.N), c.dt)
        assert hip.gemm_fw4(P, Q, out=G.t, flags=4096) is None
        untouched(G)


@pytest.mark.parametrize("c", R.FW4_SW_CASES, ids=ID)
def test_gemm_fw4_swiglu(c):
    (xc, wc), ref = R.fused_case(c)
    x, w = xc.to(DEV), wc.to(DEV)
    first = None
    for flags in R.FW4_SWIGLU_FLAGS:
        GU, S = guarded((c.M, 2 * c.a), c.dt), guarded((c.M, c.a), c.dt)
        assert hip.gemm_fw4_swiglu(x, w, gu_out=GU.t, s_out=S.t, flags=flags) is not None
        GU.assert_guards()
        S.assert_guards()
        if first is None:
            first = GU.t.clone(), S.t.clone()
            check(c.name + " gu", first[0], ref.gu, c.dt)
            check(c.name + " s", first[1], ref.s, c.dt)
        else:
            same_bits(GU.t, first[0], f"{c.name} gu flags {flags}")
            same_bits(S.t, first[1], f"{c.name} s flags {flags}")


# ----------------------------------------------------------------------- fused k_gemm_bf16 forms
@pytest.mark.parametrize("c", R.ROPE_CASES, ids=ID)
def test_gemm_qkv_rope(c):
    """S = 128 under 256-row tiles: every tile spans two sequences (position m % S); nh 1 and 3:
    heads that straddle the 192-column tiles; both staging schedules."""
    (xc, wc, cos, sin), ref = R.fused_case(c)
    x, w, cos, sin = (t.to(DEV) for t in (xc, wc, cos, sin))
    first = None
    for flags in R.gb_flag_sets(late=True):
        G = guarded((c.M, 3 * c.a * 64), c.dt)
        with gb(flags):
            assert hip.gemm_qkv_rope(x, w, c.S, cos, sin, out=G.t) is not None
        G.assert_guards()
        if first is None:
            first = G.t.clone()
            check(c.name, first, ref, c.dt)
        else:
            same_bits(G.t, first, f"{c.name} flags {flags}")


@pytest.mark.parametrize("c", R.GU_CASES, ids=ID)
def test_gemm_gu_swiglu(c):
    (xc, wc), ref = R.fused_case(c)
    x, w = xc.to(DEV), wc.to(DEV)
    first = None
    for flags in R.gb_flag_sets():
        GU, S = guarded((c.M, 2 * c.a), c.dt), guarded((c.M, c.a), c.dt)
        with gb(flags):
            assert hip.gemm_gu_swiglu(x, w, gu_out=GU.t, s_out=S.t) is not None
        GU.assert_guards()
        S.assert_guards()
        if first is None:
            first = GU.t.clone(), S.t.clone()
            check(c.name + " gu", first[0], ref.gu, c.dt)
            check(c.name + " s", first[1], ref.s, c.dt)
        else:
            same_bits(GU.t, first[0], f"{c.name} gu flags {flags}")
            same_bits(S.t, first[1], f"{c.name} s flags {flags}")


@pytest.mark.parametrize("c", R.DOWN_CASES, ids=ID)
def test_gemm_down_swiglu_bwd(c):
    (ddc, wdc, guc), ref = R.fused_case(c)
    dd, wd, gu = ddc.to(DEV), wdc.to(DEV), guc.to(DEV)
    first = None
    for flags in R.gb_flag_sets(late=True):
        for with_s in (False, True):
            G, S = guarded((c.M, 2 * c.a), c.dt), guarded((c.M, c.a), c.dt)
            with gb(flags):
                assert hip.gemm_down_swiglu_bwd(dd, wd, gu, out=G.t, s_out=S.t if with_s else None) is not None
            G.assert_guards()
            if with_s:
                S.assert_guards()
                check(f"{c.name} s flags {flags}", S.t, ref.s, c.dt)
            else:
                untouched(S)
            if first is None:
                first = G.t.clone()
                check(c.name + " dgu", first, ref.dgu, c.dt)
            else:
                same_bits(G.t, first, f"{c.name} dgu flags {flags} s_out {with_s}")


# --------------------------------------------------------------------------- weight gradients
def _wide(t, pad=8):
    """``t`` as a column slice of a wider tensor (row stride t.shape[1] + 2 pad)."""
    w = torch.full((t.shape[0], t.shape[1] + 2 * pad), 3.0, dtype=t.dtype, device=t.device)
    w[:, pad:pad + t.shape[1]] = t
    return w[:, pad:pad + t.shape[1]]


@pytest.mark.parametrize("c", R.WG_CASES, ids=ID)
def test_gemm_wgrad(c):
    dyc, xc, base, chk = R.wgrad_case(c)
    dy, x = dyc.to(DEV), xc.to(DEV)
    n = R.wgrad_splits(c.T, c.Nr, c.Nc, c.splits)
    assert c.splits == 0 or n == min(c.splits, c.T // 128)
    DW, PT = guarded((c.Nr, c.Nc), F32, base), guarded((max(n, 2), c.Nr, c.Nc), F32)
    assert hip.gemm_wgrad(DW.t, dy, x, splits=c.splits, part=PT.t)
    DW.assert_guards()
    PT.assert_guards(written=(torch.arange(max(n, 2), device=DEV) < (n if n > 1 else 0)).view(-1, 1, 1).expand(PT.t.shape))
    check(c.name, DW.t, chk, F32)
    # operands as column slices of wider tensors (row stride != row length): the same bits
    DS = guarded((c.Nr, c.Nc), F32, base)
    assert hip.gemm_wgrad(DS.t, _wide(dy), _wide(x, 72), splits=c.splits)
    DS.assert_guards()
    same_bits(DS.t, DW.t, c.name + " strided")
    if n > 1:
        # partials-only mode, each split against its own reference; then splitk_acc on its own
        parts = R.wgrad_parts_ref(dyc, xc, c.family, n)
        P2 = guarded((n, c.Nr, c.Nc), F32)
        assert hip.gemm_wgrad(None, dy, x, splits=n, part=P2.t)
        P2.assert_guards()
        check(c.name + " part", P2.t, parts, F32)
        same_bits(P2.t, PT.t[:n], c.name + " part")
        D2 = guarded((c.Nr, c.Nc), F32, base)
        hip.splitk_acc(P2.t, D2.t)
        D2.assert_guards()
        P2.assert_guards()
        check(c.name + " splitk_acc", D2.t, R.splitk_ref(P2.t.cpu(), base, c.family), F32)
        same_bits(D2.t, DW.t, c.name + " splitk_acc")


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: DT_NAME[d])
def test_splitk_sum_at_ties(dt):
    """Partials whose exact fp32 sum lies half way between two 16-bit values (and one fp32 ulp to
    either side): round to nearest even, bit for bit."""
    part = R.tie_partials(dt)
    ref = part.double().sum(0)
    O = guarded((part.shape[1],), dt)
    hip.splitk_sum_bf16(part.to(DEV), O.t)
    O.assert_guards()
    check(f"splitk_sum-{DT_NAME[dt]}", O.t, R.Checked(ref, torch.zeros_like(ref)), dt)


@pytest.mark.parametrize("c", R.SK_CASES, ids=ID)
def test_gemm_wgrad_stream_k(c):
    dyc, xc, base, chk = R.wgrad_case(c)
    dy, x = dyc.to(DEV), xc.to(DEV)
    pl = R.sk_plan(c.T, c.Nr, c.Nc, c.splits)
    DW = guarded((c.Nr, c.Nc), F32, base)
    assert hip.gemm_wgrad_sk(DW.t, dy, x, shares=c.splits)
    DW.assert_guards()
    check(c.name, DW.t, chk, F32)
    # the C entry point with the scratch in a guarded buffer; strided operands; twice: the same bits
    n = int(hip.lib().dlt_gemm_wgrad_sk_scratch(c.T, c.Nr, c.Nc, c.splits))
    assert n == pl.ntc * pl.Gc * pl.maxseg * 256 * R.wgrad_bn(c.Nc)
    ys, xs = _wide(dy, 72), _wide(x)
    for rep in range(2):
        D2, SC = guarded((c.Nr, c.Nc), F32, base), guarded((n,), F32)
        rc = hip.lib().dlt_gemm_wgrad_sk(hip._p(ys), hip._p(xs), hip._p(D2.t), hip._p(SC.t), c.T, c.Nr, c.Nc,
                                         ys.stride(0), xs.stride(0), c.splits, hip._WG_HK[c.dt], hip._stream())
        assert rc == 0
        D2.assert_guards()
        SC.assert_guards()
        same_bits(D2.t, DW.t, f"{c.name} run {rep}")
    # the grouped launch of this problem alone
    D3 = guarded((c.Nr, c.Nc), F32, base)
    assert hip.gemm_wgrad_group([(D3.t, dy, x)], shares=[pl.Gc])
    D3.assert_guards()
    same_bits(D3.t, DW.t, c.name + " group of one")


# ---------------------------------------------------------------------------------- refusals
def test_refusals_touch_nothing():
    """Every shape or stride the wrappers and C entry points reject: None, False or -1, the
    guarded outputs as they were."""
    L, st = hip.lib(), hip._stream()
    for dt in DTYPES:
        hk = hip._WG_HK[dt]
        a = torch.ones(256, 136, dtype=dt, device=DEV)
        b = torch.ones(192, 136, dtype=dt, device=DEV)
        C, D = guarded((256, 200), dt), guarded((256, 192), F32)
        p = hip._p
        for fn in (L.dlt_gemm_bf16_tn, L.dlt_gemm_bf16_nn):
            for M, N, K, lda, ldb, ldc in ((128, 192, 128, 136, 136, 200), (256, 64, 128, 136, 136, 200),
                                           (256, 192, 64, 136, 136, 200), (256, 192, 192, 136, 136, 200),
                                           (256, 192, 128, 132, 136, 200), (256, 192, 128, 136, 132, 200),
                                           (256, 192, 128, 136, 136, 196), (0, 192, 128, 136, 136, 200)):
                assert fn(p(a), p(b), p(C.t), M, N, K, lda, ldb, ldc, R.GB_DEFAULT_FLAGS, hk, st) == -1
        for M, N, K, lda, ldb, ldc, fl in ((256, 192, 96, 136, 136, 200, 0), (256, 96, 128, 136, 136, 200, 0),
                                           (256, 128, 128, 120, 136, 200, 0), (256, 128, 128, 136, 136, 120, 0),
                                           (256, 128, 128, 136, 136, 200, 16), (256, 128, 128, 136, 136, 200, 128),
                                           (256, 128, 128, 136, 136, 200, 4096), (256, 128, 64, 136, 136, 200, 0)):
            assert L.dlt_gemm_fw4(p(a), p(b), p(C.t), M, N, K, lda, ldb, ldc, fl, hk, None, 0, st) == -1
        dy = torch.ones(256, 256, dtype=dt, device=DEV)
        x = torch.ones(256, 192, dtype=dt, device=DEV)
        for T, Nr, Nc, ldy, ldx, s, part in ((192, 256, 192, 256, 192, 1, None), (256, 192, 192, 256, 192, 1, None),
                                             (256, 256, 96, 256, 192, 1, None), (256, 256, 192, 260, 192, 1, None),
                                             (256, 256, 192, 256, 196, 1, None), (256, 256, 192, 256, 192, 3, C.t),
                                             (256, 256, 192, 256, 192, 2, None), (256, 256, 192, 256, 192, 0, None)):
            assert L.dlt_gemm_wgrad(p(dy), p(x), p(D.t), p(part), T, Nr, Nc, ldy, ldx, s, hk, st) == -1
        assert L.dlt_gemm_wgrad_sk(p(dy), p(x), p(D.t), None, 256, 256, 192, 256, 192, 2, hk, st) == -1
        assert L.dlt_gemm_wgrad_sk(p(dy), p(x), p(D.t), p(C.t), 192, 256, 192, 256, 192, 2, hk, st) == -1
        assert L.dlt_gemm_wgrad_sk_scratch(192, 256, 192, 2) == 0
        # the wrappers
        a2, b2 = a[:, :128].contiguous(), b[:, :128].contiguous()
        O = guarded((256, 192), dt)
        assert hip.gemm_bf16(a2[:, :64].contiguous(), b2[:, :64].contiguous(), out=O.t) is None
        assert hip.gemm_bf16(a2[:128], b2, out=O.t) is None and hip.gemm_bf16(a2, b2[:96], out=O.t) is None
        assert hip.gemm_dgrad(a2, b2[:96].t().contiguous(), out=O.t) is None
        assert hip.gemm_dgrad(a2, torch.ones(64, 192, dtype=dt, device=DEV), out=O.t) is None
        assert hip.gemm_fw4(a2[:, :96].contiguous(), b2[:, :96].contiguous(), out=O.t) is None
        assert hip.gemm_fw4(a2, b2, out=O.t, flags=16) is None and hip.gemm_fw4(a2, b2[:120], out=O.t) is None
        assert hip.gemm_fw4_swiglu(a2, b2[:128], gu_out=O.t, s_out=O.t) is None  # I = 64
        assert hip.gemm_down_swiglu_bwd(a2, torch.ones(128, 96, dtype=dt, device=DEV), torch.ones(256, 192, dtype=dt, device=DEV),
                                        out=O.t) is None
        assert not hip.gemm_wgrad(D.t, dy[:192], x[:192]) and not hip.gemm_wgrad(D.t, dy[:, :64], x)
        assert not hip.gemm_wgrad(D.t, _wide(dy, 2), x) and not hip.gemm_wgrad_sk(D.t, dy, _wide(x, 2))
        assert not hip.gemm_wgrad_sk(D.t, dy[:192], x[:192])
        assert not hip.gemm_wgrad_group([(D.t, dy[:192], x[:192])])
        untouched(C, D, O)
    xb = torch.ones(256, 128, dtype=BF, device=DEV)
    cos, sin = hip.rope_tables(64, 256, device=DEV)
    O = guarded((256, 192), BF)
    w = torch.ones(192, 128, dtype=BF, device=DEV)
    assert hip.gemm_qkv_rope(xb, w, 96, cos, sin, out=O.t) is None                   # M % S
    assert hip.gemm_qkv_rope(xb, w, 512, cos, sin, out=O.t) is None                  # tables shorter than S
    assert hip.gemm_qkv_rope(xb, w[:, :64].contiguous(), 128, cos, sin, out=O.t) is None
    assert hip.gemm_gu_swiglu(xb, torch.ones(128, 128, dtype=BF, device=DEV), gu_out=O.t, s_out=O.t) is None  # I % 96
    assert hip.lib().dlt_gemm_bf16_qkv_rope(hip._p(xb), hip._p(w), hip._p(O.t), 256, 64, 128, 0, hip._p(cos), hip._p(sin),
                                            R.GB_DEFAULT_FLAGS, st) == -1
    untouched(O)
