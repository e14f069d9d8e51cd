"""``_fused_step`` (eval/decode.py) on stub configs; without norms it answers as ``_fused_kind``."""
import pytest
import torch

from distributed_llm_trainer_amd.eval import decode as D
from tests.test_decode_gqa_cpu import _stub


def _norm_stub(nh, nkv, qk_norm=False, post_norm=False, new_ops=True, dtype=torch.bfloat16, **kw):
    m = _stub(nh, nkv, **kw)
    m.config.qk_norm, m.config.post_norm, m.engine.act_dtype = qk_norm, post_norm, dtype
    if new_ops:
        m.engine.ops.dec_norm_qkv_qkn = m.engine.ops.dec_gemv_out = lambda *a: None
    return m


@pytest.mark.parametrize("nkv,kind", [(12, "mha"), (4, "gqa")])
@pytest.mark.parametrize("qkn,pn", [(True, False), (False, True), (True, True)])
def test_fused_step_of_norm_models(nkv, kind, qkn, pn, monkeypatch):
    monkeypatch.delenv("DLT_DECODE_FUSED", raising=False)
    kw = dict(qk_norm=qkn, post_norm=pn)
    m = _norm_stub(12, nkv, **kw)
    assert D._fused_step(m, 2) == D.FusedStep(kind, qkn, pn)
    assert D._fused_kind(m, 2) is None and not D._fused_ok(m, 2)  # the step without norm forms: as before
    assert D._fused_step(_norm_stub(12, nkv, new_ops=False, **kw), 2) is None  # a library without the norm forms
    assert D._fused_step(_norm_stub(12, nkv, dtype=torch.float16, **kw), 2) is None  # bf16 kernels only
    assert D._fused_step(_norm_stub(4, 4 if kind == "mha" else 2, hidden=512, **kw), 2) is None  # head_dim 128
    assert D._fused_step(m, 3) is None  # not a decode batch
    monkeypatch.setenv("DLT_DECODE_FUSED", "0")
    assert D._fused_step(m, 2) is None


@pytest.mark.parametrize("B", (1, 2, 3, 4, 8))
@pytest.mark.parametrize("kw", [dict(nh=12, nkv=12), dict(nh=12, nkv=4), dict(nh=12, nkv=1, maxS=16384),
                                dict(nh=4, nkv=4, maxS=40697), dict(nh=4, nkv=2, hidden=512), dict(nh=192, nkv=48),
                                dict(nh=12, nkv=4, gqa_ops=False), dict(nh=12, nkv=12, dec_ops=False)])
def test_fused_step_without_norms_is_fused_kind(kw, B, monkeypatch):
    monkeypatch.delenv("DLT_DECODE_FUSED", raising=False)
    m = _norm_stub(new_ops=False, **kw)
    step, kind = D._fused_step(m, B), D._fused_kind(m, B)
    assert (step.kind if step is not None else None) == kind
