"""Decode throughput of GPT.generate (KV cache) with and without the HIP-graph step.
usage: python tools/bench_decode.py [model_size] [batch] [new_tokens] [num_kv_heads] [max_seq_len] [window]
("-" leaves an argument at its default)

``num_kv_heads`` (default: the preset's, multi-head) makes the model grouped-query; the
run then also prints which fused step it took (``_fused_kind``) and the key splits (NS,
``DLT_DECODE_KV_SPLITS``) of its attention, and times the captured step once more at the
last cache position (every key read).  ``max_seq_len`` overrides the preset's cache length.
``window`` makes every layer a sliding-window layer of that many keys (``sliding_window``);
the same timings are printed, so a run with and one without it compare the captured step."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_llm_trainer_amd.models import GPT, GPTConfig  # noqa: E402



def _arg(i, default, conv=int):
    return conv(sys.argv[i]) if len(sys.argv) > i and sys.argv[i] != "-" else default


size = _arg(1, "small", str)
B = _arg(2, 1)
N = _arg(3, 200)
NKV = _arg(4, None)
MAXS = _arg(5, None)
WINDOW = _arg(6, None)
torch.manual_seed(0)
cfg = GPTConfig.from_preset(size)
if NKV is not None:
    cfg.num_kv_heads = NKV
if MAXS is not None:
    cfg.max_seq_len = MAXS
if WINDOW is not None:
    cfg.sliding_window = WINDOW
if NKV is not None or MAXS is not None or WINDOW is not None:
    cfg.__post_init__()
m = GPT(cfg).to("cuda")
m.enable_engine()
from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, _fused_kind, _gqa_splits, forward_cached  # noqa: E402
DETAIL = NKV is not None or MAXS is not None or WINDOW is not None
if DETAIL:
    kind = _fused_kind(m, B)
    ns = _gqa_splits(m.config, B) if kind == "gqa" else "-"
    print(f"{size} B={B} nh={m.config.num_heads} nkv={m.config.num_kv_heads} max_seq_len={m.config.max_seq_len} "
          f"window={m.config.sliding_window}: fused kind {kind}, NS {ns}", flush=True)
ids = torch.randint(0, 50257, (B, 32), device="cuda")
for mode, graph, loop in (("eager", "0", "0"), ("graph, host sampling", "1", "0"), ("graph, device loop", "1", "1")):
    os.environ["DLT_DECODE_GRAPH"] = graph
    os.environ["DLT_DECODE_DEVICE_LOOP"] = loop
    m.generate(ids, max_new_tokens=8)
    torch.cuda.synchronize()
    t = time.perf_counter()
    m.generate(ids, max_new_tokens=N)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    print(f"{size} B={B} {mode}: {N / dt:.1f} steps/s, {B * N / dt:.1f} tokens/s ({dt / N * 1e3:.2f} ms/token)",
          flush=True)

# replay-only cost of the captured step (no sampling / Python in the loop)
with torch.no_grad():
    c = KVCache(m.config, B, "cuda", m.engine.act_dtype)
    forward_cached(m, ids, c)
    g = DecodeGraph(m, c, c.len)
    nxt = ids[:, -1:].clone()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(100):
        g.graph.replay()
    torch.cuda.synchronize()
    print(f"graph replay only: {(time.perf_counter() - t) / 100 * 1e3:.3f} ms/step")
    if DETAIL:
        # three windows of 300 replays each, at the prompt's position and over a full cache
        # (the rows beyond the prompt are zero): the spread between windows is the noise
        for name, p in (("prompt position", c.len), ("full cache", m.config.max_seq_len - 1)):
            g.pos.fill_(p)
            ws = []
            for _ in range(4):  # the first window warms up
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(300):
                    g.graph.replay()
                torch.cuda.synchronize()
                ws.append((time.perf_counter() - t) / 300 * 1e3)
            print(f"graph replay only, {name}: min {min(ws[1:]):.4f} ms/step "
                  f"(windows {' '.join(f'{w:.4f}' for w in ws[1:])})", flush=True)
        g.pos.fill_(c.len)
    lg = g(nxt)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(100):
        v, _ = torch.topk(lg, 50)
        l2 = lg.masked_fill(lg < v[:, [-1]], float("-inf"))
        p = torch.softmax(l2, dim=-1)
        s = torch.multinomial(p, 1)
    torch.cuda.synchronize()
    print(f"sampling only: {(time.perf_counter() - t) / 100 * 1e3:.3f} ms/step")
