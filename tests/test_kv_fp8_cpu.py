"""The FP8 KV cache's host side without a GPU: the cache allocation and the wrappers' dtype check."""
from types import SimpleNamespace

import pytest
import torch

from distributed_llm_trainer_amd.eval import decode as D
from distributed_llm_trainer_amd.ops import hip

FP8, BF = torch.float8_e4m3fn, torch.bfloat16
CFG = SimpleNamespace(num_kv_heads=2, max_seq_len=16, head_dim=64, num_layers=3)


def test_kv_cache_allocates_one_byte_elements_of_the_same_shape():
    a, b = D.KVCache(CFG, 2, "cpu", BF), D.KVCache(CFG, 2, "cpu", BF, kv_dtype=FP8)
    assert [t.dtype for t in a.k + a.v] == [BF] * 6  # "auto": the cache it built
    for x, y in zip(a.k + a.v, b.k + b.v):
        assert y.dtype == FP8 and y.element_size() == 1 and y.shape == x.shape
        assert not y.view(torch.uint8).any()


@pytest.mark.parametrize("call", [
    lambda kc, vc, z: hip.dec_norm_qkv(z, z, 1e-5, z, z, z, z, z, kc, vc, 2),
    lambda kc, vc, z: hip.dec_norm_qkv_gqa(torch.zeros(1, 256), z, 1e-5, z, z, z, z, z, kc, vc, 4, 2),
    lambda kc, vc, z: hip.dec_norm_qkv_qkn(torch.zeros(1, 256), z, 1e-5, z, z, z, z, z, z, z, kc, vc, 4, 2),
    lambda kc, vc, z: hip.dec_attn(z, kc, vc, z, z, 0.125),
    lambda kc, vc, z: hip.dec_attn_gqa(z, kc, vc, z, z, 0.125, 4),
    lambda kc, vc, z: hip.prefill_qkv_cache(torch.zeros(1, 512, dtype=BF), kc, vc, z, z, 0, 4, 2),
    lambda kc, vc, z: hip.prefill_attn(torch.zeros(1, 512, dtype=BF), kc, vc, 0, z, 0.125, 4),
])
def test_wrappers_refuse_mixed_cache_dtypes_before_any_launch(call, monkeypatch):
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("a kernel library call"))
    kc, vc = torch.zeros(1, 2, 16, 64, dtype=BF), torch.zeros(1, 2, 16, 64, dtype=FP8)
    for a, b in ((kc, vc), (vc, kc)):
        with pytest.raises(TypeError, match="k_cache is .* but v_cache is"):
            call(a, b, torch.zeros(1))
