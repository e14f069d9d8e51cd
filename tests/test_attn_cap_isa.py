"""Build-time ISA check on the CAP forms of the flash-attention kernels (CPU: hipcc cross-compiles
``ops/csrc/attention_cap.hip`` to assembly).

The CAP kernels keep the plain kernels' counted LDS waits (``lgkm_wait4`` / ``lgkm_wait8``), and
they take one more scalar argument, ``cap_k``, that the tile functions read inside the tile loop:
a scalar load the compiler leaves to the first use would be in flight inside a counted window,
exactly the hazard tests/test_isa_checks.py looks for.  This runs that file's check, unchanged, on
the CAP translation unit."""
import os
import shutil

import pytest

from distributed_llm_trainer_amd.ops import build as kbuild
from tests.test_isa_checks import _counted_lgkm_violations, _device_asm


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_cap_kernels_counted_lds_waits_have_no_smem_in_flight(tmp_path):
    src = os.path.join(kbuild.CSRC, "attention_cap.hip")
    asm = _device_asm(src, tmp_path)
    for kernel in ("k_attn_fwd_cap", "k_attn_bwd_dq_cap", "k_attn_bwd_dkdv_cap", "k_attn_bwd_dkdv_gqa_cap"):
        assert kernel in asm, f"{kernel} is not in attention_cap.hip"
    counted, bad = _counted_lgkm_violations(asm)
    assert asm.count("lgkmcnt(4)") > 0, "the asm K-row reads' counted wait is gone"
    assert counted > 0
    assert not bad, f"SMEM load inside a counted LDS wait window: {bad[:5]}"
