"""Evaluation head A/B on one GPU: the logits-free lm_head loss (k_gemm_fw4's loss epilogue +
k_lse_combine, ``hip.lmhead_loss``) against the pair it replaces (``hip.gemm_fw4`` into an
[M, Vp] logits buffer + ``hip.cross_entropy_fwd_bwd``), at 8192 x 768 x 50304 in bf16:

* ``head``: the two forms alone -- median of event-timed calls after warm-up, peak memory;
* ``evaluate``: a whole ``DistributedTrainer.evaluate`` of the small preset (8 x 1024 rows
  per batch) with ``DLT_EVAL_HEAD`` fused / unfused -- host clock around the call (it ends
  in a device-to-host copy), peak memory rise.

The two forms alternate, three pairs each.  Every step is a child process under its own
``timeout``; the driver stops at the first step that fails and writes the table.

usage: python tools/bench_eval_head.py [--out profiles/eval_head.md] [--iters 30] [--batches 8]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
M, K, VP, V = 8192, 768, 50304, 50257
PAIRS = 3


def _median_us(fn, iters):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0)
    return statistics.median(ts)


def _peak_rise_mb(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def step_head(args):
    import torch
    from distributed_llm_trainer_amd.ops import hip
    g = torch.Generator("cuda").manual_seed(0)
    nf = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(VP, K, device="cuda", generator=g) * 0.02).bfloat16()
    w[V:] = 0
    tgt = torch.randint(0, V, (M,), device="cuda", generator=g)
    nv = (tgt != -100).sum()
    lg = torch.empty(M, VP, device="cuda", dtype=torch.bfloat16)

    def fused():
        return hip.lmhead_loss(nf, w, tgt, V)[0]

    def unfused():
        hip.gemm_fw4(nf, w, out=lg)
        return hip.cross_entropy_fwd_bwd(lg, tgt, V, nv)

    def unfused_alloc():  # as the engine runs it: the logits buffer allocated per call
        return hip.cross_entropy_fwd_bwd(hip.gemm_fw4(nf, w), tgt, V, nv)

    diff = (fused() - unfused()).abs().max().item()
    out = {"pairs": [], "max_row_diff": diff}
    for _ in range(PAIRS):
        out["pairs"].append({"fused_us": _median_us(fused, args.iters), "unfused_us": _median_us(unfused, args.iters)})
    del lg
    out["fused_peak_mb"] = _peak_rise_mb(fused)
    out["unfused_peak_mb"] = _peak_rise_mb(unfused_alloc)
    print("RESULT " + json.dumps(out), flush=True)


def step_evaluate(args):
    import torch
    from distributed_llm_trainer_amd.models import GPTConfig
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    cfg = GPTConfig.gpt2_small()
    tr = DistributedTrainer(cfg, TrainingConfig(batch_size=8))
    g = torch.Generator("cuda").manual_seed(1)
    held = [torch.randint(0, cfg.vocab_size, (8, cfg.max_seq_len), device="cuda", generator=g)
            for _ in range(args.batches)]

    def run(mode):
        os.environ["DLT_EVAL_HEAD"] = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.evaluate(held, args.batches)
        return (time.perf_counter() - t0) * 1e3, res["val_loss"]

    out = {"pairs": [], "batches": args.batches}
    for mode in ("fused", "unfused"):  # warm-up: GEMM plans of both heads
        run(mode)
    for _ in range(PAIRS):
        f_ms, f_loss = run("fused")
        u_ms, u_loss = run("unfused")
        out["pairs"].append({"fused_ms": f_ms, "unfused_ms": u_ms})
    out["val_loss_fused"], out["val_loss_unfused"] = f_loss, u_loss
    for mode in ("fused", "unfused"):
        os.environ["DLT_EVAL_HEAD"] = mode
        out[mode + "_peak_mb"] = _peak_rise_mb(lambda: tr.evaluate(held, 1))
    print("RESULT " + json.dumps(out), flush=True)


def _child(step, args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
           "--iters", str(args.iters), "--batches", str(args.batches)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"step {step} failed with exit status {r.returncode}: nothing further is started")
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_head.md"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--step", choices=["head", "evaluate"], default=None)
    args = ap.parse_args()
    if args.step:
        return {"head": step_head, "evaluate": step_evaluate}[args.step](args)
    head = _child("head", args, 240)
    ev = _child("evaluate", args, 420)
    med = lambda key, rows: statistics.median(r[key] for r in rows)  # noqa: E731
    hf, hu = med("fused_us", head["pairs"]), med("unfused_us", head["pairs"])
    ef, eu = med("fused_ms", ev["pairs"]), med("unfused_ms", ev["pairs"])
    L = ["# Evaluation head: logits-free lm_head loss vs lm_head GEMM + cross-entropy", "",
         f"`tools/bench_eval_head.py`, one MI355X, bf16, {M} x {K} x {VP} (V = {V}).  The two forms alternate;",
         f"each figure is the median of {args.iters} event-timed calls after 5 warm-up calls.", "",
         "## Head alone", "",
         "| pair | fused: k_gemm_fw4 (loss epilogue) + k_lse_combine, us | unfused: gemm_fw4 + cross_entropy_fwd_bwd, us |",
         "|---|---|---|"]
    L += [f"| {i + 1} | {p['fused_us']:.1f} | {p['unfused_us']:.1f} |" for i, p in enumerate(head["pairs"])]
    L += [f"| median | {hf:.1f} | {hu:.1f} |", "",
          f"Fused / unfused = {hf / hu:.3f}.  Largest row-loss difference between the two: {head['max_row_diff']:.2e}.",
          f"Peak memory rise of one call: fused {head['fused_peak_mb']:.1f} MB, unfused "
          f"{head['unfused_peak_mb']:.1f} MB (its logits buffer is {M * VP * 2 / 1e6:.0f} MB).", "",
          f"## Whole `evaluate`, small preset, {ev['batches']} batches of 8 x 1024", "",
          "| pair | DLT_EVAL_HEAD=fused, ms | DLT_EVAL_HEAD=unfused, ms |", "|---|---|---|"]
    L += [f"| {i + 1} | {p['fused_ms']:.2f} | {p['unfused_ms']:.2f} |" for i, p in enumerate(ev["pairs"])]
    L += [f"| median | {ef:.2f} | {eu:.2f} |", "",
          f"Fused / unfused = {ef / eu:.3f} (host clock around `evaluate`, which ends in a device-to-host copy).",
          f"val_loss: fused {ev['val_loss_fused']:.6f}, unfused {ev['val_loss_unfused']:.6f}.",
          f"Peak memory rise of a one-batch `evaluate`: fused {ev['fused_peak_mb']:.1f} MB, unfused "
          f"{ev['unfused_peak_mb']:.1f} MB.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    main()
