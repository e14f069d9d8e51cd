"""Fused decode step of GPT-2 small with ``attn_softcap`` unset and set, alternating in one process:
multi-head and with ``--kv_heads`` K/V heads (the CAP forms of ``k_dec_attn`` / ``k_dec_attn_gqa``).
The kernel-level comparison of the training kernels is ``tools/bench_attn.py --softcap CAP``, and a
``bench.py``-shaped step with the cap is ``bench.py --model_override attn_softcap=50``."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, forward_cached  # noqa: E402
from distributed_llm_trainer_amd.models import GPT, GPTConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap", type=float, default=50.0)
    ap.add_argument("--kv_heads", type=int, nargs="+", default=[12, 4])
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_softcap: needs a GPU")
    for nkv in a.kv_heads:
        graphs = {}
        for cap in (None, a.cap):
            torch.manual_seed(0)
            cfg = GPTConfig.from_dict({**GPTConfig.gpt2_small().to_dict(), "num_kv_heads": nkv, "dropout": 0.0,
                                       "attention_dropout": 0.0, **({} if cap is None else {"attn_softcap": cap})})
            m = GPT(cfg).cuda()
            m.enable_engine()
            m.eval()
            cache = KVCache(cfg, 1, "cuda", m.engine.act_dtype)
            with torch.no_grad():
                forward_cached(m, torch.randint(0, 50257, (1, a.context), device="cuda"), cache)
                graphs[cap] = (DecodeGraph(m, cache, cache.len), m)
            assert graphs[cap][0].fused
        for rep in range(a.repeats):
            out = []
            for cap, (g, _) in graphs.items():
                for _ in range(10):
                    g.graph.replay()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    g.graph.replay()
                torch.cuda.synchronize()
                out.append(f"attn_softcap {cap}: {(time.perf_counter() - t0) / a.iters * 1e6:7.1f} us")
            print(f"kv_heads {nkv} run {rep} fused decode step ({graphs[None][0].kind}): " + " | ".join(out), flush=True)


if __name__ == "__main__":
    main()
