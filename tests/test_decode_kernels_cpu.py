"""Self-checks of tests/decode_ref.py, runnable without a GPU: the tolerances admit a correct
fp32 implementation, reject every planted defect at the very inputs the GPU tests use, and
the host model of the sampler's uniform stays inside [0, 1)."""
import numpy as np
import pytest
import torch

from tests import decode_ref as R


def _outside(defect: torch.Tensor, chk: R.Checked) -> torch.Tensor:
    """Per batch row: how many elements of the defective output miss the tolerance (a NaN misses)."""
    miss = ~((defect - chk.ref).abs() <= chk.tol)
    return miss.reshape(miss.shape[0], -1).sum(dim=1)


def _assert_detected(name, defect, chk):
    n = _outside(defect, chk)
    assert (n > 0).all(), f"{name}: rows {(n == 0).nonzero().flatten().tolist()} stay inside the tolerance"


def _assert_inside(name, out, chk):
    err = (out.double() - chk.ref).abs()
    assert (err <= chk.tol).all(), f"{name}: err/tol = {(err / chk.tol).max().item():.3f}"


def bf16_out(x):
    """A defective kernel's output: its fp64 value, rounded as the kernel rounds it."""
    return R.bf16_round(x)


# ---- an fp32 model of the kernels' arithmetic (torch ops in fp32, roundings as the kernels)
def _normed32(h, lnw):
    rstd = torch.rsqrt((h * h).mean(dim=1, keepdim=True) + np.float32(R.EPS))
    return (h * rstd * lnw.float()).bfloat16().float()


def _gemv32(x, w):
    return (x @ w.float().T).bfloat16().float()


@pytest.mark.parametrize("wbf16", [False, True])
@pytest.mark.parametrize("H", R.QKV_H)
def test_qkv_reference(H, wbf16):
    h, lnw, w = R.qkv_inputs(H, wbf16)
    nh = H // 64
    cos, sin = R.rope_tables(64, R.QKV_MAXS)
    y32 = _gemv32(_normed32(h, lnw), w).view(8, 3, nh, 64)
    for pos in R.QKV_POS:
        ref = R.qkv_ref(h, lnw, w, cos, sin, pos, nh)
        c, s = cos[pos], sin[pos]
        for i, name in enumerate("qk"):
            x1, x2 = y32[:, i, :, :32], y32[:, i, :, 32:]
            out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).bfloat16()
            _assert_inside(f"{name} pos={pos}", out, ref[name])
        _assert_inside("v", y32[:, 2], ref["v"])
        for dname, km in R.slice_masks(H).items():
            bad = R.qkv_ref(h, lnw, w, cos, sin, pos, nh, kmask=km)
            for name in "qkv":
                _assert_detected(f"{dname} {name} pos={pos}", bf16_out(bad[name].ref), ref[name])
        for rp in (pos - 1, pos + 1):
            if 0 <= rp < R.QKV_MAXS:
                bad = R.qkv_ref(h, lnw, w, cos, sin, pos, nh, rope_pos=rp)
                for name in "qk":
                    _assert_detected(f"rope pos{rp - pos:+d} {name} pos={pos}", bf16_out(bad[name].ref), ref[name])


@pytest.mark.parametrize("RK", R.RES_SHAPES)
def test_gemv_res_reference(RK):
    x, w, h = R.res_inputs(*RK)
    ref = R.gemv_res_ref(x, w, h)
    _assert_inside("gemv_res", h + _gemv32(x.float(), w), ref)
    for dname, km in R.slice_masks(RK[1]).items():
        g = R.gemv(x.double(), w, km)
        _assert_detected(dname, (h.double() + bf16_out(g.y)).float().double(), ref)


@pytest.mark.parametrize("wbf16", [False, True])
@pytest.mark.parametrize("HI", R.GU_SHAPES)
def test_norm_gu_reference(HI, wbf16):
    h, lnw, w = R.gu_inputs(*HI, wbf16)
    I = HI[1]
    ref = R.norm_gu_ref(h, lnw, w)
    y32 = _gemv32(_normed32(h, lnw), w)
    g32, u32 = y32[:, :I], y32[:, I:]
    _assert_inside("norm_gu", (g32 * torch.sigmoid(g32) * u32).bfloat16(), ref)
    _assert_detected("swap gate/up", bf16_out(R.norm_gu_ref(h, lnw, w, swap=True).ref), ref)
    for dname, km in R.slice_masks(HI[0]).items():
        _assert_detected(dname, bf16_out(R.norm_gu_ref(h, lnw, w, kmask=km).ref), ref)


@pytest.mark.parametrize("wbf16", [False, True])
@pytest.mark.parametrize("HVR", R.HEAD_SHAPES)
def test_norm_head_reference(HVR, wbf16):
    H, V, rows = HVR
    h, lnw, w = R.head_inputs(H, V, rows, wbf16)
    assert torch.isnan(w[V:].float()).all() and torch.isfinite(w[:V].float()).all()
    ref = R.norm_head_ref(h, lnw, w, V)
    assert ref.ref.shape == (8, V) and torch.isfinite(ref.ref).all()
    _assert_inside("norm_head", _gemv32(_normed32(h, lnw), w[:V]), ref)
    for dname, km in R.slice_masks(H).items():
        _assert_detected(dname, bf16_out(R.norm_head_ref(h, lnw, w, V, kmask=km).ref), ref)


def _attn32(q, kc, vc, pos, scale):
    B, nh, _, hd = kc.shape
    s = torch.einsum("bhd,bhjd->bhj", q.float().view(B, nh, hd), kc[:, :, :pos + 1].float()) * scale
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = torch.einsum("bhj,bhjd->bhd", p, vc[:, :, :pos + 1].float()) / p.sum(dim=-1, keepdim=True)
    return o.bfloat16()


@pytest.mark.parametrize("nh", [3, 12])
def test_attn_reference(nh):
    q, kc, vc = R.attn_inputs(nh, 1024)
    for pos in R.ATTN_POS:
        ref = R.attn_ref(q, kc, vc, pos, R.ATTN_SCALE)
        _assert_inside(f"attn pos={pos}", _attn32(q, kc, vc, pos, R.ATTN_SCALE), ref)
        if pos + 1 < 1024:
            bad = R.attn_ref(q, kc, vc, pos, R.ATTN_SCALE, extra_keys=1)
            _assert_detected(f"key pos+1 included, pos={pos}", bf16_out(bad.ref), ref)


@pytest.mark.parametrize("kind", ["large60", "large100", "equal"])
def test_attn_reference_score_ranges(kind):
    q, kc, vc = R.attn_inputs(3, 1024, kind)
    s = torch.einsum("bhd,bhjd->bhj", q.double().view(8, 3, 64), kc.double()) * R.ATTN_SCALE
    if kind == "equal":
        assert (s == s[:, :, :1]).all()
    else:
        m = float(kind[5:])
        assert 0.98 * m < s.amax().item() < 1.02 * m and 0.98 * m < -s.amin().item() < 1.02 * m
    ref = R.attn_ref(q, kc, vc, 1023, R.ATTN_SCALE)
    _assert_inside(kind, _attn32(q, kc, vc, 1023, R.ATTN_SCALE), ref)
    no_max = R.attn_ref(q, kc, vc, 1023, R.ATTN_SCALE, no_max=True)
    if kind == "large100":
        # fp32 exp overflows above 88.7: without the max subtraction the output is inf / inf
        _assert_detected("no max subtraction", bf16_out(no_max.ref), ref)
    else:
        # e^60 is finite in fp32: at +-60 this defect is not a numerical defect at all, which is
        # why the +-100 case exists
        _assert_inside("no max subtraction is harmless here", bf16_out(no_max.ref), ref)


def test_sample_reference_keeps_ties_and_never_minus_inf():
    lg = torch.tensor([[0.0, 3.0, 1.0, 3.0, 1.0, float("-inf"), -2.0]])
    kept, p = R.sample_reference(lg, 1.0, 3)
    assert kept[0].tolist() == [False, True, True, True, True, False, False]  # both ties at the 3rd value
    assert abs(p.sum().item() - 1) < 1e-12 and (p[~kept] == 0).all()
    for k in (0, 7, 12):
        kept, p = R.sample_reference(lg, 1.0, k)
        assert kept[0].tolist() == [True] * 5 + [False, True]
    b = R.freq_bound(torch.tensor([0.0, 0.5], dtype=torch.float64), 4000)
    assert b[0].item() == 1 / 4000 and abs(b[1].item() - (5 * 0.5 / 4000 ** 0.5 + 1 / 4000)) < 1e-12


def test_uniform_is_in_unit_interval_for_every_hash():
    bits = np.arange(1 << 24, dtype=np.uint32)
    u = R.uniform_of_bits(bits)
    assert u.dtype == np.float32 and u.min() == 0.0 and u.max() < 1.0
    assert (u.astype(np.float64) * 2.0 ** 24 == bits).all()  # the grid is exact in fp32
    # what the kernels computed before: 16777215 + 0.5f rounds to 16777216, u == total
    assert R.uniform_of_bits_before_fix(bits).max() == 1.0


def test_seed_search_hits_the_hash_corners():
    from distributed_llm_trainer_amd.ops import rng
    for x in (0, 1, 0xDEADBEEF, 0xFFFFFFFF, 15340575):
        assert R.lowbias32_inverse(rng.lowbias32(x)) == x
    assert R.draw_hash(15340575, 0, 0) >> 8 == 0xFFFFFF  # a known seed of the all-ones corner
    for pos in (0, 7):
        for b in (0, 3):
            for bits in (0xFFFFFF, 0):
                seed = R.seed_for_bits(pos, b, bits)
                assert 0 <= seed <= 0xFFFFFFFF and R.draw_hash(seed, pos, b) >> 8 == bits
