"""GeGLU on the GPU: unfused kernels and decode against fp64, every fused form bit for bit against the unfused pair,
a model through the engine and the captured decode step.  Reference, tolerance and model: tests/test_geglu_cpu.py."""
import pytest
import torch

from distributed_llm_trainer_amd.ops import hip
from tests import decode_ref as D
from tests.test_geglu_cpu import check, check_unfused, engine_and_eager, geglu_fp64, geglu_model

pytestmark = pytest.mark.gpu
DEV, GEGLU, BF, FP = "cuda", {"activation": "geglu"}, torch.bfloat16, torch.float16


@pytest.mark.parametrize("I", [8, 264])
@pytest.mark.parametrize("dtype", [BF, FP])
def test_elementwise_forward_and_backward(dtype, I):
    check_unfused(hip, dtype, I, DEV)


def _rand(n, m, dtype, seed, scale=1.0):
    return (scale * (torch.rand(n, m, generator=torch.Generator().manual_seed(seed)) * 2 - 1)).to(DEV, dtype)


@pytest.mark.parametrize("fw4,M,I,dtype", [(True, 256, 128, BF), (True, 512, 256, BF), (True, 256, 128, FP),
                                           (True, 512, 256, FP), (False, 256, 96, BF), (False, 512, 192, BF)])
def test_gate_up_geglu_epilogues_are_the_unfused_pair(fw4, M, I, dtype):
    x, w = _rand(M, 128, dtype, 1), _rand(2 * I, 128, dtype, 2)
    for flags in ((0, 144) if fw4 else (None,)):  # k_gemm_fw4: SCHED 4 and SCHED 5; else k_gemm_bf16
        gu, s = hip.gemm_fw4_swiglu(x, w, flags=flags, **GEGLU) if fw4 else hip.gemm_gu_swiglu(x, w, **GEGLU)
        assert torch.equal(gu, hip.gemm_fw4(x, w, flags=flags) if fw4 else hip.gemm_bf16(x, w))
        assert torch.equal(s, hip.swiglu_fwd(gu, **GEGLU))


@pytest.mark.parametrize("late", [0, 4096], ids=["stage-in-loop", "epilogue-first"])
@pytest.mark.parametrize("with_s", [False, True])
@pytest.mark.parametrize("M,I", [(256, 192), (512, 384)])
@pytest.mark.parametrize("dtype", [BF, FP])
def test_gemm_down_geglu_bwd_is_the_unfused_pair(dtype, M, I, with_s, late, monkeypatch):
    monkeypatch.setattr(hip, "_GB_FLAGS", (hip._GB_FLAGS & ~4096) | late)
    dd, wt = _rand(M, 128, dtype, 1), _rand(I, 128, dtype, 2)  # wt.t(): Wdown [H, I]
    gu = _rand(M, 2 * I, dtype, 3, 12.0)  # gates from the cancelling point to saturation
    s1, s2 = (torch.full((M, I), 7.0, dtype=dtype, device=DEV) if with_s else None for _ in range(2))
    dgu = hip.gemm_down_swiglu_bwd(dd, wt.t().contiguous(), gu, s_out=s1, **GEGLU)
    assert torch.equal(dgu, hip.swiglu_bwd(gu, hip.gemm_dgrad(dd, wt.t().contiguous()), s_out=s2, **GEGLU))
    assert not with_s or torch.equal(s1, s2)


@pytest.mark.parametrize("B", [D.DECODE_BATCHES[0], D.DECODE_BATCHES[-1]])
def test_dec_norm_gu_geglu(B):
    H, I = 64, 20  # the clamped tail: 20 columns on 8-column workgroups
    h, lnw, w = (t.to(DEV) for t in D.gu_inputs(H, I, False))
    gv = D.gemv(D.normed(h, lnw), w)
    gtol = D.gemv_tol(gv, H).cpu()
    g16, u16 = (D.bf16_round(t).to(BF).cpu() for t in (gv.y[:, :I], gv.y[:, I:]))
    want = geglu_fp64(g16, u16, torch.ones_like(g16))  # ds = 1: its du is act(g)
    # as decode_ref.norm_gu_ref: plus the bf16 GEMV outputs' error times |d gelu_tanh / dg| <= 1.13 and d/du = act(g)
    tol = want["s"][1] + 1.13 * u16.double().abs() * gtol[:, :I] + want["du"][0].abs() * gtol[:, I:]
    buf = torch.full((B * I + 64,), -777.0, dtype=BF, device=DEV)
    hip.dec_norm_gu(h[:B].contiguous(), lnw, D.EPS, w, buf[:B * I].view(B, I), **GEGLU)
    check(f"dec_norm_gu geglu B={B}", buf[:B * I].view(B, I), (want["s"][0][:B], tol[:B]))
    assert (buf[B * I:] == -777.0).all(), "the clamped tail columns were stored"


def test_engine_matches_the_eager_model():
    """At the tolerances of test_postnorm_gpu.py's engine comparison."""
    losses, grads = engine_and_eager(DEV)
    assert abs(losses[0] - losses[1]) < 2e-2 * abs(losses[0]), losses
    for n, a, b in grads:
        assert torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item() > 0.99, n
        assert 0.95 < (b.norm() / a.norm()).item() < 1.05, n


@pytest.mark.parametrize("Bn", [1, 4])
def test_decode_fused_step_matches_forward_cached(Bn, monkeypatch):
    """Several replays of the captured step; atol = rtol = 3e-2 as the other fused-step tests."""
    from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, forward_cached
    m = geglu_model(DEV).eval()
    m.enable_engine()
    monkeypatch.setenv("DLT_DECODE_FUSED", "1")
    ids, steps = (torch.randint(0, 1000, (Bn, n), generator=torch.Generator().manual_seed(n)).to(DEV) for n in (40, 4))
    ca, cb = (KVCache(m.config, Bn, DEV, m.engine.act_dtype) for _ in range(2))
    with torch.no_grad():
        forward_cached(m, ids, ca)
        forward_cached(m, ids, cb)
        graph = DecodeGraph(m, ca, ca.len)
        assert graph.fused
        for t in range(4):
            a, b = graph(steps[:, t:t + 1]).clone(), forward_cached(m, steps[:, t:t + 1], cb)
            assert torch.allclose(a, b, atol=3e-2, rtol=3e-2), (t, (a - b).abs().max().item())
