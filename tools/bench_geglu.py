"""GeGLU against SwiGLU on one GPU at the bench.py shapes (profiles/geglu.md sections 2 and 3):
kernel times of every form, A B A B in one session, and what the planner's per-shape race
(HipGemm._fused_pick, pins of the plan removed) picks for each activation.

    python tools/bench_geglu.py
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_llm_trainer_amd import ops  # noqa: E402
from distributed_llm_trainer_amd.ops import gemm  # noqa: E402
from distributed_llm_trainer_amd.ops import hip  # noqa: E402

hip.lib()
DEV = "cuda"
M, H, I = 8192, 768, 3072
torch.manual_seed(0)
x = (torch.randn(M, H, device=DEV)).bfloat16()
wgu = (torch.randn(2 * I, H, device=DEV) * 0.05).bfloat16()
wdown = (torch.randn(H, I, device=DEV) * 0.05).bfloat16()
dd = torch.randn(M, H, device=DEV).bfloat16()
gu = hip.gemm_fw4(x, wgu)
ds = torch.randn(M, I, device=DEV).bfloat16()
s = torch.empty(M, I, dtype=torch.bfloat16, device=DEV)
dgu = torch.empty(M, 2 * I, dtype=torch.bfloat16, device=DEV)
gu_o = torch.empty_like(gu)


def t(fn, n=40, reps=5):
    """Median [min, max] us per launch of ``reps`` groups of ``n`` back-to-back launches."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000 / n)
    return statistics.median(out), min(out), max(out)


forms = {
    "swiglu_fwd": lambda kw: hip.swiglu_fwd(gu, out=s, **kw),
    "swiglu_bwd": lambda kw: hip.swiglu_bwd(gu, ds, out=dgu, **kw),
    "swiglu_bwd+s": lambda kw: hip.swiglu_bwd(gu, ds, out=dgu, s_out=s, **kw),
    "gemm_fw4_swiglu": lambda kw: hip.gemm_fw4_swiglu(x, wgu, gu_out=gu_o, s_out=s, **kw),
    "gemm_gu_swiglu": lambda kw: hip.gemm_gu_swiglu(x, wgu, gu_out=gu_o, s_out=s, **kw),
    "gemm_down_swiglu_bwd": lambda kw: hip.gemm_down_swiglu_bwd(dd, wdown, gu, out=dgu, **kw),
    "gemm_down_swiglu_bwd+s": lambda kw: hip.gemm_down_swiglu_bwd(dd, wdown, gu, out=dgu, s_out=s, **kw),
}
res = {}
for name, f in forms.items():
    for rnd in range(2):  # A B A B
        for act in ("swiglu", "geglu"):
            kw = {} if act == "swiglu" else {"activation": "geglu"}
            res.setdefault(f"{name}/{act}", []).append(t(lambda: f(kw)))
plain = {"gemm_fw4 (gate/up, plain)": lambda: hip.gemm_fw4(x, wgu, out=gu_o),
         "gemm_dgrad (down)": lambda: hip.gemm_dgrad(dd, wdown, out=s)}
for name, f in plain.items():
    res[name] = [t(f), t(f)]
for k, v in res.items():
    print(k, " ".join(f"{m:.1f}us[{lo:.1f}-{hi:.1f}]" for m, lo, hi in v))

# the race itself: fused against unfused as _fused_pick times them, three times per activation
gm, hops = gemm.HipGemm(), ops.for_device(torch.device(DEV), head_dim=64, act_dtype=torch.bfloat16)
keys = [("swiglu4", M, 2 * I, H), ("swiglu", M, 2 * I, H), ("dswiglu", M, I, H)]
print("plan pins:", {k: gm._choice.get(k) for k in keys})
for act in ("swiglu", "geglu", "swiglu", "geglu", "swiglu", "geglu"):
    for k in keys:
        gm._choice.pop(k, None)
    gm.linear_swiglu(x, wgu, hops, s_out=s, activation=act)
    gm.linear_dgrad_swiglu(dd, wdown, gu, hops, out=dgu, activation=act)
    print(f"race {act}:", {k[0]: gm._choice.get(k) for k in keys[1:]})
