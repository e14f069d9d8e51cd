"""Host side of the 64-granular GEMM (ops/csrc/gemm_r64.hip): its shape rule, the gpt2_xl
projections it exists for, that HipGemm offers it only where no other hand-written kernel tiles,
and its pin in a plan file.  No GPU."""
import json

import pytest

from distributed_llm_trainer_amd.ops import gemm, hip
from tests import gemm_ref as R

# the gpt2_xl projections that fit no other hand-written kernel: (output columns, reduction)
XL_TN = ((4800, 1600), (1600, 1600), (1600, 6400))
XL_NN = ((1600, 4800), (1600, 1600), (1600, 12800), (6400, 1600), (1600, 50304))


@pytest.mark.parametrize("M,N,K,fits", [
    (256, 64, 128, True), (512, 192, 192, True), (4096, 1600, 1600, True), (256, 64, 64, False), (256, 96, 128, False),
    (256, 128, 160, False), (128, 128, 128, False), (384, 128, 128, False), (0, 64, 128, False), (256, 0, 128, False)])
def test_fits(M, N, K, fits):
    assert hip.gemm_r64_fits(M, N, K) is fits


@pytest.mark.parametrize("M", (256, 4096))
def test_every_xl_role_fits_and_is_routed_here(M):
    for N, K in XL_TN:
        assert hip.gemm_r64_fits(M, N, K) and gemm.HipGemm._tn_candidates(M, N, K) == ["r64"]
    for N, K in XL_NN:
        assert hip.gemm_r64_fits(M, N, K) and gemm.HipGemm._dgrad_hand(M, N, K) is hip.gemm_r64_dgrad


def test_shapes_another_kernel_tiles_are_never_offered():
    for M, N, K in [s[:3] for s in R.GB_SHAPES] + list(R.FW4_SHAPES):
        assert hip.gemm_bf16_fits(M, N, K) or hip.gemm_fw4_fits(M, N, K)
        assert "r64" not in gemm.HipGemm._tn_candidates(M, N, K)
        if hip.gemm_bf16_fits(M, N, K):
            assert gemm.HipGemm._dgrad_hand(M, N, K) is hip.gemm_dgrad


class _Planner:
    """The planner entry points load_plan / export_plan call, with an empty solution table."""
    dlt_gemm_lib_version = staticmethod(lambda: 7)
    dlt_gemm_dump = staticmethod(lambda buf, n: 0)


def test_plan_round_trip_of_an_r64_pin(tmp_path, monkeypatch):
    monkeypatch.setattr(gemm, "lib", lambda: _Planner)
    monkeypatch.setattr(gemm, "_PINNED", {"tn": {}, "splitk": {}, "wgrad_group": {}, "hipblaslt": {}})
    monkeypatch.setattr(gemm, "_RACES", {})
    monkeypatch.setattr(gemm, "_INSTANCES", [])
    path = tmp_path / "plan.json"
    path.write_text(json.dumps({"tn": {"4096x4800x1600": "r64", "4096x1600x6400": "r65"},
                                "fused": {"dgrad:4096x1600x4800": True}}))
    gemm.load_plan(str(path), shipped=True)
    assert gemm._PINNED["tn"][(4096, 4800, 1600)] == "r64" and gemm._PINNED["tn"][(4096, 1600, 6400)] is None
    out = gemm.export_plan()
    assert out["tn"]["4096x4800x1600"] == "r64" and out["fused"]["dgrad:4096x1600x4800"] is True
