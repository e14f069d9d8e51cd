"""Micro-benchmark of attention sinks at one shape (default B16 S1024 nh12 hd64, the headline
batch): the flash forward with and without ``sink=`` (``k_attn_fwd_sink`` against
``k_attn_fwd``), the backward with and without ``dsink=`` (the difference is
``k_attn_sink_bwd``), and the fused decode step of GPT-2 small with and without sinks.

Times are device events around ``--iters`` back-to-back calls after a warm-up; the whole table
is measured ``--repeats`` times, the variants interleaved, so the spread between repeats is the
noise of the box."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_llm_trainer_amd.models import GPT, GPTConfig  # noqa: E402
from distributed_llm_trainer_amd.ops import hip  # noqa: E402


def timeit(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def kernels(args, dev, dt):
    B, S, nh, hd = args.B, args.S, args.nh, args.hd
    cos, sin = hip.rope_tables(hd, S, device=dev)
    for nkv in args.kv_heads:
        kw = {} if nkv == nh else {"nkv": nkv}
        qkv = torch.randn(B * S, (nh + 2 * nkv) * hd, device=dev).to(dt)
        do = torch.randn(B * S, nh * hd, device=dev).to(dt)
        sink = torch.randn(nh, device=dev)
        dsink = torch.zeros(nh, device=dev)
        for p in args.dropout:
            mask = hip.attention_dropout_mask(B, nh, S, p, 7, device=dev)
            o0, aux0 = hip.attention_fwd_packed(qkv, B, S, nh, p, 7, mask=mask, **kw)
            o1, aux1 = hip.attention_fwd_packed(qkv, B, S, nh, p, 7, mask=mask, sink=sink, **kw)
            for rep in range(args.repeats):
                f0 = timeit(lambda: hip.attention_fwd_packed(qkv, B, S, nh, p, 7, out=o0, mask=mask, **kw), args.iters)
                f1 = timeit(lambda: hip.attention_fwd_packed(qkv, B, S, nh, p, 7, out=o1, mask=mask, sink=sink, **kw),
                            args.iters)
                b0 = timeit(lambda: hip.attention_bwd_packed(qkv, o0, do, aux0, p, 7, B, S, nh, cos, sin, **kw), args.iters)
                b1 = timeit(lambda: hip.attention_bwd_packed(qkv, o1, do, aux1, p, 7, B, S, nh, cos, sin, sink=sink,
                                                             dsink=dsink, **kw), args.iters)
                print(f"run {rep} nkv {nkv:2d} p {p}: fwd {f0:7.1f} us | fwd sink {f1:7.1f} us | bwd {b0:7.1f} us | "
                      f"bwd + sink_bwd {b1:7.1f} us (k_attn_sink_bwd ~ {b1 - b0:5.1f} us)", flush=True)


def decode(args, dev):
    from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, _fused_kind, forward_cached
    for nkv in args.kv_heads:
        graphs = {}
        for sinks in (False, True):
            torch.manual_seed(0)
            cfg = GPTConfig.from_dict({**GPTConfig.from_preset("small").to_dict(), "num_kv_heads": nkv,
                                       "attention_sinks": sinks})
            m = GPT(cfg).to(dev)
            m.enable_engine()
            m.eval()
            ids = torch.randint(0, 50257, (1, 32), device=dev)
            with torch.no_grad():
                c = KVCache(m.config, 1, dev, m.engine.act_dtype)
                forward_cached(m, ids, c)
                g = DecodeGraph(m, c, c.len)
            graphs[sinks] = (g, _fused_kind(m, 1), m, c)
        for rep in range(args.repeats):
            out = []
            for sinks in (False, True):
                g, kind, m, c = graphs[sinks]
                for name, pos in (("prompt position", 32), ("full cache", m.config.max_seq_len - 1)):
                    g.pos.fill_(pos)
                    out.append(f"{'sinks' if sinks else 'plain'} {name} {timeit(g.graph.replay, 300) / 1e3:.3f} ms")
            print(f"run {rep} decode step, GPT-2 small nkv {nkv} ({graphs[True][1]}): " + " | ".join(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--nh", type=int, default=12)
    ap.add_argument("--hd", type=int, default=64, choices=(64, 128))
    ap.add_argument("--kv_heads", type=int, nargs="+", default=[12, 4])
    ap.add_argument("--dropout", type=float, nargs="+", default=[0.1, 0.0])
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no_decode", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sinks: needs a GPU")
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    print(f"B{args.B} S{args.S} nh{args.nh} hd{args.hd} {args.dtype}, {args.iters} calls per timing")
    kernels(args, "cuda", dt)
    if not args.no_decode:
        decode(args, "cuda")


if __name__ == "__main__":
    main()
