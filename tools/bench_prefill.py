"""Prefill over the KV cache: the two HIP kernels alone, ``forward_cached`` on the HIP route against its
ATen route (``DLT_PREFILL_FUSED=0``: the code it ran before the kernels existed), and generation past
``max_seq_len`` (one re-prefill per token).  The two routes alternate inside every repeat.
usage: python tools/bench_prefill.py [model_size] [repeats]

Kernel times are device events around 100 back-to-back launches (per launch, gaps included); call
times are a host clock around calls that end in a device synchronise; peak memory is
``torch.cuda.max_memory_allocated`` over one call minus what was allocated before it."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_llm_trainer_amd.eval.decode import KVCache, forward_cached  # noqa: E402
from distributed_llm_trainer_amd.models import GPT, GPTConfig  # noqa: E402
from distributed_llm_trainer_amd.ops import hip  # noqa: E402

size = sys.argv[1] if len(sys.argv) > 1 else "small"
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
DEV = "cuda"
SHAPES = ((1, 1024, 0), (8, 1024, 0), (1, 64, 960), (8, 64, 960))  # (B, T, p0)


def spread(xs):
    return f"median {sorted(xs)[len(xs) // 2]:.3f} (min {min(xs):.3f}, max {max(xs):.3f})"


def events(fn, n=100):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3  # us


torch.manual_seed(0)
cfg = GPTConfig.from_preset(size)
nh, hd, maxS = cfg.num_heads, cfg.head_dim, cfg.max_seq_len
print(f"# kernels: nh {nh}, hd {hd}, cache {maxS} rows, bf16; us per launch over {REP} repeats")
cos, sin = hip.rope_tables(hd, maxS, device=DEV)
for B, T, p0 in SHAPES:
    qkv = torch.randn(B * T, 3 * nh * hd, device=DEV).bfloat16()
    kc, vc = (torch.randn(B, nh, maxS, hd, device=DEV).bfloat16() for _ in range(2))
    o = torch.empty(B * T, nh * hd, dtype=torch.bfloat16, device=DEV)
    ta = [events(lambda: hip.prefill_attn(qkv, kc, vc, p0, o, hd ** -0.5, nh)) for _ in range(REP)]
    tq = [events(lambda: hip.prefill_qkv_cache(qkv, kc, vc, cos, sin, p0, nh, nh)) for _ in range(REP)]
    flop = 4.0 * B * nh * hd * sum(p0 + t + 1 for t in range(T))
    print(f"B {B} T {T} p0 {p0}: prefill_attn {spread(ta)} us, {flop / min(ta) * 1e-6:.1f} TFLOP/s causal at the min; "
          f"prefill_qkv_cache {spread(tq)} us", flush=True)

m = GPT(cfg).to(DEV)
m.enable_engine()
m.eval()
print(f"# forward_cached, {size} preset: ms per call and peak MB, HIP route | ATen route")
for B, T, p0 in SHAPES:
    ids = torch.randint(0, cfg.vocab_size, (B, p0 + T), device=DEV)
    res = {"1": ([], 0), "0": ([], 0)}
    for r in range(REP + 1):  # the first repeat warms up
        for flag in ("1", "0"):
            os.environ["DLT_PREFILL_FUSED"] = flag
            c = KVCache(cfg, B, DEV, m.engine.act_dtype)
            if p0:
                forward_cached(m, ids[:, :p0], c)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t = time.perf_counter()
            forward_cached(m, ids[:, p0:], c)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) * 1e3
            if r:
                res[flag][0].append(dt)
                res[flag] = (res[flag][0], max(res[flag][1], torch.cuda.max_memory_allocated() - before))
            del c
    print(f"B {B} T {T} p0 {p0}: HIP {spread(res['1'][0])} ms, peak {res['1'][1] / 2 ** 20:.0f} MB | "
          f"ATen {spread(res['0'][0])} ms, peak {res['0'][1] / 2 ** 20:.0f} MB", flush=True)

print("# generation past max_seq_len (B 1, a full-context prompt, 8 new tokens = 7 re-prefills): ms per token")
ids = torch.randint(0, cfg.vocab_size, (1, maxS), device=DEV)
res = {"1": [], "0": []}
for r in range(REP + 1):
    for flag in ("1", "0"):
        os.environ["DLT_PREFILL_FUSED"] = flag
        torch.cuda.synchronize()
        t = time.perf_counter()
        m.generate(ids, max_new_tokens=8)
        torch.cuda.synchronize()
        if r:
            res[flag].append((time.perf_counter() - t) / 8 * 1e3)
print(f"HIP {spread(res['1'])} | ATen {spread(res['0'])}")
