"""Micro-benchmark of the QK-norm kernels next to the plain in-place RoPE at one shape
(default B16 S1024 nh12 hd64, the headline batch): ``k_qknorm_rope_inplace`` and
``k_qknorm_bwd`` (+ its two ``k_colsum_acc`` launches) against ``k_rope_qk_inplace``.

Times are device events around ``--iters`` back-to-back calls after a warm-up; bytes are
what each op has to move, computed from the shape (16-bit elements):
  rope      reads and writes the q|k columns:                2 * M * (H + KV) * 2
  qknorm    the same plus the raw copy:                      3 * M * (H + KV) * 2
  qknorm_bwd reads raw and g, writes dx:                     3 * M * (H + KV) * 2
so GB/s = bytes / time is the achieved rate of the op, not a profiler counter."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--nh", type=int, default=12)
    ap.add_argument("--hd", type=int, default=64, choices=(64, 128))
    ap.add_argument("--kv_heads", type=int, nargs="+", default=[12, 4])
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3, help="the whole table is measured this many times (spread)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qknorm: needs a GPU")
    dev = "cuda"
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    B, S, nh, hd = args.B, args.S, args.nh, args.hd
    M = B * S
    cos, sin = hip.rope_tables(hd, S, device=dev)
    print(f"B{B} S{S} nh{nh} hd{hd} {args.dtype}, {args.iters} calls per timing")
    for rep in range(args.repeats):
        for nkv in args.kv_heads:
            W, QK = (nh + 2 * nkv) * hd, (nh + nkv) * hd
            kw = {} if nkv == nh else {"nkv": nkv}
            qkv = torch.randn(M, W, device=dev).to(dt)
            dqkv = torch.randn(M, W, device=dev).to(dt)
            raw = torch.empty(M, QK, dtype=dt, device=dev)
            qw = 1.0 + 0.1 * torch.randn(hd, device=dev)
            kwt = 1.0 + 0.1 * torch.randn(hd, device=dev)
            dq, dk = torch.zeros(hd, device=dev), torch.zeros(hd, device=dev)
            ws = hip.qknorm_bwd_workspace(M, nh, hd, dev)
            # (the in-place ops rewrite their own output every call: values drift, the traffic does not)
            t_rope = timeit(lambda: hip.rope_qk_inplace(qkv, B, S, nh, cos, sin, **kw), args.iters)
            qkv.normal_()
            t_fwd = timeit(lambda: hip.qknorm_rope_inplace(qkv, B, S, nh, cos, sin, qw, kwt, 1e-6, raw, **kw), args.iters)
            raw.normal_()
            t_bwd = timeit(lambda: hip.qknorm_bwd(dqkv, raw, B, S, nh, qw, kwt, 1e-6, dq, dk, ws=ws, **kw), args.iters)
            by = M * QK * 2
            print(f"run {rep} nkv {nkv:2d}: rope_qk_inplace {t_rope:7.1f} us ({2 * by / t_rope / 1e3:6.0f} GB/s) | "
                  f"qknorm_rope_inplace {t_fwd:7.1f} us ({3 * by / t_fwd / 1e3:6.0f} GB/s) | "
                  f"qknorm_bwd {t_bwd:7.1f} us ({3 * by / t_bwd / 1e3:6.0f} GB/s)", flush=True)


if __name__ == "__main__":
    main()
