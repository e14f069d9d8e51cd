"""The logits-free lm_head loss (k_gemm_fw4's loss epilogue + k_lse_combine) against the
unrounded fp32 product, on the MI355X.

Bound (derived, not tuned).  The kernel rounds every logit to the activation format as the
stored logits are; round-to-nearest moves a logit l by at most 2^-8 |l| in bf16 and
2^-11 |l| in fp16.  The log-sum-exp moves by at most the largest logit move and the target
logit by its own, so with both shares:

    |row_loss - loss_fp32| <= F * max_j |l_fp32[m, j]| + EPS,   F = 2^-7 (bf16), 2^-10 (fp16)

and the same for lse.  EPS covers fp32 accumulation order and the fast exp2 / log: it is
taken from the unfused path this kernel replaces (gemm_fw4 + cross_entropy_fwd_bwd) on the
inputs below -- the largest amount by which that path's error exceeds the rounding term,
doubled (see EPS).  The reference op and the unfused path are held to the same bound on
the same inputs.
"""
import functools

import pytest
import torch

from distributed_llm_trainer_amd.ops import hip, reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

FACTOR = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
# Residual of gemm_fw4 + cross_entropy_fwd_bwd beyond the rounding term over every case of
# CASES on an MI355X, doubled (docs/KERNELS.md, "lm_head loss").  Measured: that path stays
# inside the rounding term on every case -- its largest residual (error minus rounding term,
# worst row) is -5.3e-4 (256 x 128 x 128 fp16, rounding term 2.9e-3), -6.2e-3 the closest in
# bf16 -- so nothing is left over to double and the rounding term alone is the bound.
EPS = 0.0

# (M, K, Vp, V, dtype, logit scale or None)
CASES = [
    (256, 128, 128, 128, torch.bfloat16, None),     # the minimum: one half tile, wave wn = 1 idle
    (256, 192, 384, 331, torch.bfloat16, None),     # ns = 3, ragged last tile, V % 8 != 0, 53 padded columns
    (512, 768, 640, 640, torch.bfloat16, None),     # two row tiles
    (256, 768, 50304, 50257, torch.bfloat16, None),  # the real head width
    (256, 128, 128, 128, torch.float16, None),
    (256, 192, 384, 331, torch.float16, None),
    (512, 768, 640, 640, torch.float16, None),
    (256, 192, 384, 331, torch.bfloat16, 80.0),     # logits reach +-80: the online maximum
]
IDS = ["%dx%dx%d_V%d_%s%s" % (m, k, vp, v, str(dt).split(".")[1], "_big" if sc else "")
       for m, k, vp, v, dt, sc in CASES]


def make_inputs(M, K, Vp, V, dtype, scale, device=DEV):
    g = torch.Generator().manual_seed(1000 * M + Vp + K)
    nf = torch.randn(M, K, generator=g)
    w = torch.randn(Vp, K, generator=g) * 0.05
    if scale is not None:  # bring the largest logit to about +-scale
        peak = (nf.to(dtype).float() @ w[:V].to(dtype).float().t()).abs().max().item()
        nf = nf * (scale / peak)
    w[V:] = 30.0  # padding rows: a missing column mask moves the loss by far more than the bound
    nf, w = nf.to(dtype).to(device), w.to(dtype).to(device)
    l32 = nf.float() @ w[:V].float().t()
    tgt = torch.randint(0, V, (M,), generator=g).to(device)
    n0 = 256 * ((Vp - 1) // 256)  # first column of the last column tile
    cols = [0, V - 1] + [c + 5 for c in (n0, n0 + 128, n0 - 256, n0 - 128) if 0 <= c + 5 < V]
    for i, c in enumerate(cols):
        tgt[i] = c
    tgt[8:16] = l32[8:16].argmax(dim=1)
    tgt[16:24] = -100
    tgt[M - 1] = -100
    return nf, w, tgt, l32


def unfused(nf, w, tgt, V):
    """The path the kernel replaces: stored logits, then the cross-entropy kernel."""
    lg = hip.gemm_fw4(nf, w)
    assert lg is not None
    return hip.cross_entropy_fwd_bwd(lg, tgt, V, (tgt != -100).sum())


@functools.lru_cache(maxsize=None)
def run_case(i):
    M, K, Vp, V, dtype, scale = CASES[i]
    nf, w, tgt, l32 = make_inputs(M, K, Vp, V, dtype, scale)
    valid = tgt != -100
    lse32 = torch.logsumexp(l32, dim=1)
    loss32 = torch.where(valid, lse32 - l32.gather(1, tgt.clamp(min=0).unsqueeze(1)).squeeze(1),
                         torch.zeros_like(lse32))
    out = {"valid": valid, "lse32": lse32, "loss32": loss32, "round": FACTOR[dtype] * l32.abs().max(dim=1).values}
    out["fused"] = hip.lmhead_loss(nf, w, tgt, V)
    out["fused2"] = hip.lmhead_loss(nf, w, tgt, V)
    out["ref"] = ref.lmhead_loss(nf, w, tgt, V)
    out["unfused"] = unfused(nf, w, tgt, V)
    torch.cuda.synchronize()
    return out


def residual(got, want, rounding):
    """Largest amount by which |got - want| exceeds the rounding term (negative: inside it)."""
    return ((got - want).abs() - rounding).max().item()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_lmhead_loss_matches_fp32(i):
    c = run_case(i)
    assert c["fused"] is not None, "the shape tiles: the kernel must run"
    loss, lse = c["fused"]
    res = {
        "unfused loss": residual(c["unfused"], c["loss32"], c["round"]),
        "reference loss": residual(c["ref"][0], c["loss32"], c["round"]),
        "reference lse": residual(c["ref"][1], c["lse32"], c["round"]),
        "fused loss": residual(loss, c["loss32"], c["round"]),
        "fused lse": residual(lse, c["lse32"], c["round"]),
    }
    print(IDS[i], {k: "%.3e" % v for k, v in res.items()}, "rounding term max %.3e" % c["round"].max().item())
    assert torch.isfinite(loss).all() and torch.isfinite(lse).all()
    for name, r in res.items():
        assert r <= EPS, f"{name}: error exceeds the rounding term by {r:.3e} (EPS {EPS:.1e})"
    assert (loss[~c["valid"]] == 0).all(), "ignore_index rows give exactly 0"
    assert (c["ref"][0][~c["valid"]] == 0).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_lmhead_loss_deterministic(i):
    c = run_case(i)
    assert torch.equal(c["fused"][0], c["fused2"][0])
    assert torch.equal(c["fused"][1], c["fused2"][1])


@pytest.mark.parametrize("M,K,Vp", [(128, 128, 128), (256, 128, 192), (256, 96, 128)])
def test_lmhead_loss_untiled_returns_none(M, K, Vp):
    assert not hip.lmhead_loss_fits(M, Vp, K)
    nf = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(Vp, K, dtype=torch.bfloat16, device=DEV)
    tgt = torch.zeros(M, dtype=torch.int64, device=DEV)
    assert hip.lmhead_loss(nf, w, tgt, Vp) is None
