"""The attention route table (``ops/attn_routes.py``) against its four rules, written out
here and not computed from the code under test:

* bf16 / fp16, head_dim 64 or 128: the 16-bit flash route, every feature;
* bf16 / fp16, another head_dim < 128, padding on: zero-padded 16-bit flash -- the document
  mask, the window and the sinks, but no grouped K/V and no QK-norm;
* bf16 / fp16, everything else: the GEMM-formulated route, no feature;
* fp32, any head_dim: no feature.
"""
import types
import warnings

import pytest
import torch

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.ops import attn_gemm, attn_routes

DTYPES = (torch.bfloat16, torch.float16, torch.float32)
HEAD_DIMS = (32, 64, 66, 96, 127, 128, 160, 192, 250)
FEATURES = ("doc", "window", "sinks", "gqa", "qk_norm")
GRID = [(dt, hd, f) for dt in DTYPES for hd in HEAD_DIMS for f in FEATURES]
# substrings today's tests match, per feature and per route
FEATURE_WORDS = {"doc": "doc_sep_token", "window": "sliding", "sinks": "attention sinks",
                 "gqa": "num_kv_heads < num_heads", "qk_norm": "qk_norm"}


def expected(dt, hd, feature, pad=True):
    """(passes, kind) of one cell, from the four rules."""
    if hd in (64, 128):
        kind = "flash"
    elif hd < 128 and pad and (dt != torch.float32 or hd % 2 == 0):  # the fp32 layout copy moves pairs
        kind = "padded"
    else:
        kind = "gemm"
    if dt == torch.float32 or kind == "gemm":
        return False, kind
    return kind == "flash" or feature in ("doc", "window", "sinks"), kind


def check_cell(dt, hd, feature, pad=True):
    ok, kind = expected(dt, hd, feature, pad)
    if ok:
        ops.check_attention_features("cuda", hd, dt, [feature])
        return
    with pytest.raises(NotImplementedError) as e:
        ops.check_attention_features("cuda", hd, dt, [feature])
    msg = str(e.value)
    assert FEATURE_WORDS[feature] in msg and f"head_dim {hd}" in msg and str(dt) in msg and "; use " in msg
    if dt == torch.float32:
        assert "fp32" in msg.replace(str(dt), "")  # the route's name carries it, not only the dtype
    if kind == "gemm":
        assert "GEMM-formulated" in msg
    if kind == "padded":
        assert "zero-padded" in msg


def test_the_grid_has_135_cells_and_the_rows_of_the_table():
    assert len(GRID) == 135
    for dt in (torch.bfloat16, torch.float16):
        for hd in HEAD_DIMS:
            row = [expected(dt, hd, f)[0] for f in FEATURES]
            assert row == ([True] * 5 if hd in (64, 128) else [True] * 3 + [False] * 2 if hd < 128 else [False] * 5)
    assert not any(expected(torch.float32, hd, f)[0] for hd in HEAD_DIMS for f in FEATURES)


@pytest.mark.parametrize("dt,hd,feature", GRID, ids=lambda v: str(v).replace("torch.", ""))
def test_grid(dt, hd, feature):
    check_cell(dt, hd, feature)


def test_padding_off_sends_the_padded_rows_to_the_gemm_route(monkeypatch):
    monkeypatch.setattr(attn_gemm, "PAD_FLASH", False)
    for dt, hd, feature in GRID:
        check_cell(dt, hd, feature, pad=False)
        if dt != torch.float32 and hd in (32, 66, 96, 127):
            assert expected(dt, hd, feature, pad=False) == (False, "gemm")


def test_cpu_and_reference_ops_have_every_feature(monkeypatch):
    for dt, hd, _ in GRID:
        ops.check_attention_features("cpu", hd, dt, FEATURES, packed_qkv=False)
    monkeypatch.setenv("DLT_ALLOW_REFERENCE_ON_GPU", "1")
    for dt, hd, _ in GRID:
        ops.check_attention_features("cuda", hd, dt, FEATURES, packed_qkv=False)


def test_gqa_and_qk_norm_need_the_packed_layout():
    for feature in ("gqa", "qk_norm"):
        with pytest.raises(NotImplementedError, match="packed") as e:
            ops.check_attention_features("cuda", 64, torch.bfloat16, {feature}, packed_qkv=False)
        assert FEATURE_WORDS[feature] in str(e.value)
    ops.check_attention_features("cuda", 64, torch.bfloat16, {"doc", "window", "sinks"}, packed_qkv=False)
    ops.check_attention_features("cuda", 64, torch.bfloat16, FEATURES)
    with pytest.raises(ValueError):
        ops.check_attention_features("cuda", 64, torch.bfloat16, {"alibi"})


def test_config_features():
    cfg = types.SimpleNamespace(num_heads=4, num_kv_heads=4)
    assert attn_routes.config_features(cfg) == frozenset()
    cfg = types.SimpleNamespace(num_heads=4, num_kv_heads=2, qk_norm=True, attention_sinks=True, sliding_window=8)
    assert attn_routes.config_features(cfg) == {"gqa", "qk_norm", "sinks", "window"}


def test_for_device_and_the_check_take_the_route_from_one_function(monkeypatch):
    """``for_device`` (with the library's namespace stubbed: nothing is loaded) and
    ``check_attention_features`` both ask ``attn_routes.route``, get equal values for every
    grid point, and ``for_device`` installs the attn_gemm entry points exactly off the flash
    route."""
    seen = []
    real = attn_routes.route

    def spy(dtype, head_dim, flash=True):
        seen.append(real(dtype, head_dim, flash))
        return seen[-1]

    monkeypatch.setattr(attn_routes, "route", spy)
    monkeypatch.setattr(ops, "hip_ops", lambda: types.SimpleNamespace(backend="hip"))
    for dt in DTYPES:
        for hd in HEAD_DIMS:
            del seen[:]
            kind = expected(dt, hd, "doc")[1]
            ops.check_attention_features("cuda", hd, dt, ())
            if hd % 2 and kind != "flash":
                with pytest.raises(NotImplementedError, match="even head_dim"):
                    ops.for_device("cuda", hd, dt)
            else:
                with warnings.catch_warnings(record=True) as warned:
                    warnings.simplefilter("always")
                    ns = ops.for_device("cuda", hd, dt)
                assert bool(warned) == (kind != "flash")  # the one-time warning names the detour
                assert ns.attn_backend == ("hip" if kind == "flash" else "gemm")
                assert (getattr(ns, "attention_fwd_packed", None) is attn_gemm.attention_fwd_packed) == (kind != "flash")
            assert len(seen) == 2 and seen[0] == seen[1]
            rt = seen[0]
            assert (rt.kind, rt.head_dim, rt.dtype) == (kind, hd, dt)
            assert rt.pad == ((64 if hd < 64 else 128) if kind == "padded" else None)
            assert rt.features == frozenset(f for f in FEATURES if expected(dt, hd, f)[0])
            assert rt.name.startswith("fp32") == (dt == torch.float32)

