"""Prefill over the KV cache without a GPU: when ``forward_cached`` takes the HIP route
(``eval/decode.py::_prefill_fused``) and what the ``hip.prefill_*`` wrappers refuse before any launch."""
import types

import pytest
import torch

from distributed_llm_trainer_amd.eval.decode import _prefill_fused
from distributed_llm_trainer_amd.ops import hip

BF = torch.bfloat16


def _stub(device="cuda", act_dtype=BF, head_dim=64, ops=None):
    """A model as the predicate sees it, the ops namespace stubbed: nothing is loaded."""
    ops = ops or types.SimpleNamespace(backend="hip", prefill_attn=None)
    eng = types.SimpleNamespace(provider=types.SimpleNamespace(device=torch.device(device)), ops=ops, act_dtype=act_dtype)
    return types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(head_dim=head_dim))


def test_prefill_fused_predicate(monkeypatch):
    monkeypatch.delenv("DLT_PREFILL_FUSED", raising=False)
    assert _prefill_fused(_stub(), 2) and _prefill_fused(_stub(act_dtype=torch.float16, head_dim=128), 1024)
    no_kernels = types.SimpleNamespace(backend="reference")  # the CPU ops, or a library without the kernels
    for kw, T in (({}, 1), ({"device": "cpu"}, 2), ({"act_dtype": torch.float32}, 2), ({"head_dim": 96}, 2),
                  ({"ops": no_kernels}, 2)):
        assert not _prefill_fused(_stub(**kw), T), (kw, T)
    monkeypatch.setenv("DLT_PREFILL_FUSED", "0")
    assert not _prefill_fused(_stub(), 2)


@pytest.mark.parametrize("bad,match", [("p0", "must lie in the cache"), ("shape", "one shape"), ("cap", "softcap")])
def test_wrappers_refuse_before_loading_the_library(bad, match, monkeypatch):
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was loaded"))
    nh, nkv, hd, B, T, maxS = 4, 2, 64, 2, 3, 8
    qkv, o = torch.zeros(B * T, (nh + 2 * nkv) * hd, dtype=BF), torch.zeros(B * T, nh * hd, dtype=BF)
    kc = torch.zeros(B, nkv, maxS, hd, dtype=BF)
    vc = torch.zeros(B, nkv, maxS + (bad == "shape"), hd, dtype=BF)
    p0 = maxS - T + (bad == "p0")  # p0 + T == maxS is the last append that fits
    for cap in ((0.0, float("inf"), 1e6) if bad == "cap" else (None,)):
        with pytest.raises(ValueError, match=match):
            hip.prefill_attn(qkv, kc, vc, p0, o, 0.125, nh, softcap=cap)
    if bad != "cap":
        cos = torch.zeros(maxS, hd // 2)
        with pytest.raises(ValueError, match=match):
            hip.prefill_qkv_cache(qkv, kc, vc, cos, cos, p0, nh, nkv)
