"""Micro-benchmark of the post-norm kernels next to the existing fused norm kernels at one
shape (default B16 S1024 H768, the headline batch): ``k_postnorm_fwd``,
``k_postnorm_add_dropout_rmsnorm_fwd`` and ``k_postnorm_bwd`` (+ its ``k_colsum_acc`` launch)
against ``k_add_dropout_rmsnorm_fwd`` and ``k_rmsnorm_bwd``.

Times are device events around ``--iters`` back-to-back calls after a warm-up; bytes are what
each op has to move, computed from the shape (E = M * H elements):
  postnorm_fwd    reads a, writes u (16-bit):                                   2 * E * 2
  postnorm_bwd    reads du and a, writes da (16-bit):                           3 * E * 2
  add_dropout_rmsnorm_fwd  reads resid (fp32) and delta, writes x (fp32), y:    E * (4 + 2 + 4 + 2)
  postnorm_add_dropout_rmsnorm_fwd  the same traffic (a in place of delta)
  rmsnorm_bwd     reads dy, x, dres (fp32), writes dx (fp32), ddelta:           E * (2 + 4 + 4 + 4 + 2)
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
    ap.add_argument("--H", type=int, default=768)
    ap.add_argument("--p", type=float, default=0.1, help="hidden dropout of the fused forward and the norm backward")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3, help="the whole table is measured this many times (spread)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_postnorm: needs a GPU")
    dev = "cuda"
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    M, H, p = args.B * args.S, args.H, args.p
    E = M * H
    a = torch.randn(M, H, device=dev).to(dt)
    du0 = torch.randn(M, H, device=dev).to(dt)
    du = du0.clone()
    u = torch.empty_like(a)
    y = torch.empty_like(a)
    resid = torch.randn(M, H, device=dev)
    dres = torch.randn(M, H, device=dev)
    wp = 1.0 + 0.1 * torch.randn(H, device=dev)
    w2 = 1.0 + 0.1 * torch.randn(H, device=dev)
    dw = torch.zeros(H, device=dev)
    ws = hip.postnorm_bwd_workspace(M, H, dev)
    x, _, rstd = hip.add_dropout_rmsnorm_fwd(resid, a, w2, 1e-6, p, 7, dt)
    print(f"M {M} (B{args.B} S{args.S}) H{H} {args.dtype} p {p}, {args.iters} calls per timing")
    for rep in range(args.repeats):
        t_pf = timeit(lambda: hip.postnorm_fwd(a, wp, 1e-6, out=u), args.iters)
        du.copy_(du0)  # (the in-place backward rewrites its own output every call: values drift, the traffic does not)
        t_pb = timeit(lambda: hip.postnorm_bwd(du, a, wp, 1e-6, dw, ws=ws), args.iters)
        t_nf = timeit(lambda: hip.add_dropout_rmsnorm_fwd(resid, a, w2, 1e-6, p, 7, dt, y_out=y), args.iters)
        t_ff = timeit(lambda: hip.postnorm_add_dropout_rmsnorm_fwd(resid, a, wp, w2, 1e-6, p, 7, dt, y_out=y), args.iters)
        t_nb = timeit(lambda: hip.rmsnorm_bwd(du0, x, rstd, w2, dres, dw, p, 7, ddelta_out=u), args.iters)
        gb = lambda nbytes, t: nbytes / t / 1e3  # noqa: E731
        print(f"run {rep}: postnorm_fwd {t_pf:7.1f} us ({gb(4 * E, t_pf):6.0f} GB/s) | "
              f"postnorm_bwd {t_pb:7.1f} us ({gb(6 * E, t_pb):6.0f} GB/s) | "
              f"add_dropout_rmsnorm_fwd {t_nf:7.1f} us ({gb(12 * E, t_nf):6.0f} GB/s) | "
              f"postnorm_add_dropout_rmsnorm_fwd {t_ff:7.1f} us ({gb(12 * E, t_ff):6.0f} GB/s) | "
              f"rmsnorm_bwd {t_nb:7.1f} us ({gb(16 * E, t_nb):6.0f} GB/s)", flush=True)


if __name__ == "__main__":
    main()
