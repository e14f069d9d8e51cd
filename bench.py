#!/usr/bin/env python3
"""Headline benchmark: GPT-2 "124M" (small preset, 151.9M LLaMA-style params),
seq_len 1024, micro-batch 8 x grad-accum 4 per GPU (the reference DDP CLI default,
``ddp_trainer.py:497,523-527``), bf16, DDP over RCCL -- tokens/sec for the WHOLE job.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``; N>1 is
launched by torch.distributed.run (one rank per GPU).  W untimed warmup steps, then
exactly K optimizer steps between barrier+synchronize brackets; the max elapsed time
over ranks is used; rank 0 prints ONE JSON line.

A "step" is one full optimizer step exactly as the trainer runs it: 4 micro-steps of
forward+backward (dropout 0.1 on, like the reference config), gradient all-reduce,
clip-by-global-norm and AdamW -- nothing skipped.  The engine executes the 4
micro-steps of 8 sequences as 2 pipelined chains of 16 (``micro_step_fusion``; the
loss is still normalised per micro-step, so the gradient is the same GA average) --
reported in the JSON ``config``.  Data: synthetic random token ids
(no datasets offline); weights: random init of the real architecture.

A plain run sets up, warms up, times the K steps and prints the JSON line.  Weights,
token ids and dropout streams are seeded, so the same arguments give the same inputs in
every run; ``--dump-outputs DIR`` writes what the last timed step returned as
``DIR/<name>.npy`` (``dump_outputs``), to compare two builds output for output.
``--full`` adds what the headline figure does not need (the GEMM planner's report).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import distributed_llm_trainer_amd  # noqa: E402,F401  (GPU_MAX_HW_QUEUES before the HIP runtime starts)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

BASELINE_TPS = {1: 12500.0, 2: 24100.0, 4: 46800.0}  # BASELINE.md (README.md:191-197 of the reference)
DUMP_PARAM_SAMPLE = 8 * 1024 * 1024  # --dump-outputs: at most this many master weights (32 MB of float32)


def dump_outputs(path, trainer, last):
    """--dump-outputs: what the last timed ``train_step`` handed back to its caller, as
    ``path/<name>.npy``: ``loss`` and ``grad_norm`` (float64 scalars) and ``params``
    (float32), the flat fp32 master weights with that step's AdamW update applied (DDP:
    the whole model; FSDP: this rank's shard).  Past DUMP_PARAM_SAMPLE values ``params``
    is a sample of them: sorted positions drawn from a CPU generator seeded with a
    constant, so two builds dump the same positions."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    flat = trainer.flat_params() if hasattr(trainer, "flat_params") else trainer.runtime.master_flat
    flat = flat.detach().reshape(-1)
    n = flat.numel()
    if n > DUMP_PARAM_SAMPLE:
        g = torch.Generator(device="cpu").manual_seed(20240229)
        idx = torch.randint(0, n, (DUMP_PARAM_SAMPLE,), generator=g).sort().values
        flat = flat[idx.to(flat.device)]
    np.save(os.path.join(path, "params.npy"), flat.float().cpu().numpy())
    np.save(os.path.join(path, "loss.npy"), np.asarray(float(last["loss"]), dtype=np.float64))
    np.save(os.path.join(path, "grad_norm.npy"), np.asarray(float(trainer._last_norm), dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model_size", default="small")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--grad_accum", type=int, default=4)
    ap.add_argument("--seq_len", type=int, default=1024)
    ap.add_argument("--mode", default="ddp", choices=["ddp", "fsdp"])
    ap.add_argument("--sharding", default="FULL_SHARD")
    ap.add_argument("--no_ac", action="store_true", help="FSDP: disable activation checkpointing")
    ap.add_argument("--fsdp_defer_sync", action="store_true",
                    help="FSDP: reduce-scatter once per optimizer step (full-size fp32 unit gradients kept "
                         "across micro-steps, weight gradients deferred) instead of every micro-step")
    ap.add_argument("--cpu_offload", action="store_true",
                    help="FSDP: fp32 master shards + AdamW on the host (pinned), reduced grads staged D2H")
    ap.add_argument("--model_override", default="",
                    help="rehearsal only: comma-separated GPTConfig overrides (e.g. hidden_size=64,num_layers=2); "
                         "the JSON line then names a custom model and vs_baseline is null")
    ap.add_argument("--fusion", type=int, default=0,
                    help="micro_step_fusion: 0 = auto, 1 = run every micro-step on its own")
    ap.add_argument("--memory_lean", action="store_true",
                    help="the trainer's --memory_lean (TrainingConfig.defer_roles='qkv,o'): gate/up, down "
                         "and lm_head weight gradients per chain, lower peak memory")
    ap.add_argument("--memory_first", action="store_true",
                    help="DDP: TrainingConfig.memory_first (lean + unfused micro-steps + SwiGLU output rewritten "
                         "by the backward): the reference's per-GPU memory, lower tok/s")
    ap.add_argument("--no_pipeline", action="store_true",
                    help="DDP: TrainingConfig.pipeline_micro_steps=False (the micro-step chains run one after "
                         "another: only one chain's activations live at a time)")
    ap.add_argument("--defer_roles", default=None,
                    help="DDP: TrainingConfig.defer_roles override ('none' = no weight gradient deferred to the "
                         "window: per-chain weight gradients, no slot buffers)")
    ap.add_argument("--data", default="loader", choices=["loader", "resident"],
                    help="loader (default): every timed step takes a fresh batch from the native C++ loader "
                         "(dummy mode: uniform ids from a counter hash, pinned ring, H2D on a side stream), so "
                         "the input pipeline is inside the timed region as in the reference; resident: 4 "
                         "pre-made device batches reused")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"],
                    help="DDP: TrainingConfig.mixed_precision (the headline is bf16; fp16 = the HIP kernels "
                         "instantiated for IEEE half + dynamic loss scaling, fp32 = the reference/debug mode)")
    ap.add_argument("--dropout", type=float, default=None,
                    help="ablation only: override dropout/attention_dropout (reference config: 0.1)")
    ap.add_argument("--dump-outputs", dest="dump_outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned (loss, gradient norm, "
                         "the fp32 master weights after its update; a fixed seeded sample when they exceed "
                         f"{DUMP_PARAM_SAMPLE:,} values) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the GEMM planner's report (every routed shape, "
                         "its pick and the race timings) on stderr after the result line")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if os.environ.get("DLT_HANG_DUMP"):  # debugging aid: periodic Python stack dumps
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["DLT_HANG_DUMP"]), repeat=True, file=sys.stderr)

    from distributed_llm_trainer_amd.models.config import GPTConfig
    cfg = GPTConfig.from_preset(args.model_size)
    cfg.max_seq_len = args.seq_len
    overrides = {}
    for kv in filter(None, args.model_override.split(",")):
        k, v = kv.split("=", 1)
        if not hasattr(cfg, k):
            raise SystemExit(f"unknown GPTConfig field {k!r}")
        overrides[k] = type(getattr(cfg, k))(v) if getattr(cfg, k) is not None else int(v)
    if overrides:
        if "hidden_size" in overrides and "intermediate_size" not in overrides:
            overrides["intermediate_size"] = 4 * overrides["hidden_size"]
        cfg = GPTConfig(**{**cfg.to_dict(), **overrides})
    if args.dropout is not None:
        cfg.dropout = cfg.attention_dropout = args.dropout
    if args.mode == "ddp":
        from distributed_llm_trainer_amd.training.configs import TrainingConfig
        from distributed_llm_trainer_amd.training.ddp_trainer import LEAN_DEFER_ROLES, DistributedTrainer
        tc = TrainingConfig(batch_size=args.batch_size, gradient_accumulation_steps=args.grad_accum,
                            max_steps=100000, mixed_precision=args.precision, micro_step_fusion=args.fusion,
                            defer_roles=(args.defer_roles if args.defer_roles not in (None, "none") else
                                         LEAN_DEFER_ROLES if args.memory_lean else "all"),
                            defer_wgrad=args.defer_roles != "none", pipeline_micro_steps=not args.no_pipeline,
                            memory_first=args.memory_first)
        trainer = DistributedTrainer(cfg, tc)
    else:
        from distributed_llm_trainer_amd.training.configs import FSDPConfig, FSDPTrainingConfig
        from distributed_llm_trainer_amd.training.fsdp_trainer import FSDPTrainer
        tc = FSDPTrainingConfig(batch_size=args.batch_size, gradient_accumulation_steps=args.grad_accum,
                                max_steps=100000, micro_step_fusion=args.fusion)
        fc = FSDPConfig(sharding_strategy=args.sharding, activation_checkpointing=not args.no_ac,
                        cpu_offload=args.cpu_offload, sync_every_micro_step=not args.fsdp_defer_sync)
        trainer = FSDPTrainer(cfg, tc, fc)
    dev = trainer.device
    world = trainer.world_size
    if world != args.gpus and trainer.is_main_process:
        print(f"[bench] warning: --gpus {args.gpus} but world size {world}", file=sys.stderr)
    g = torch.Generator(device="cpu").manual_seed(1234 + trainer.rank)
    B = args.batch_size * args.grad_accum
    loader = None
    if args.data == "loader":
        from distributed_llm_trainer_amd.runtime.loader import NativeTokenLoader
        loader = NativeTokenLoader(None, args.seq_len, B, vocab_size=cfg.vocab_size, rank=trainer.rank,
                                   world_size=world, seed=1234, device=dev)

        def batch(i):
            return next(loader)
    else:
        batches = [torch.randint(0, cfg.vocab_size, (B, args.seq_len), generator=g).to(dev) for _ in range(4)]

        def batch(i):
            return batches[i % 4]

    for i in range(args.warmup):
        trainer.train_step({"input_ids": batch(i)}, sync_loss=False)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        if trainer.distributed:
            dist.barrier()
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)

    if dev.type == "cuda":
        torch.cuda.reset_peak_memory_stats(dev)
    sync()
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        last = trainer.train_step({"input_ids": batch(args.warmup + i)}, sync_loss=False)
    sync()
    elapsed = time.perf_counter() - t0
    loss = float(last["loss"]) if last is not None else float("nan")
    peak = torch.cuda.max_memory_allocated(dev) / 1e9 if dev.type == "cuda" else 0.0
    t = torch.tensor([elapsed, peak], dtype=torch.float64, device=dev if dev.type == "cuda" else "cpu")
    if trainer.distributed:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed, peak = float(t[0]), float(t[1])
    if args.dump_outputs and trainer.is_main_process:
        dump_outputs(args.dump_outputs, trainer, last)
    tokens = args.steps * B * args.seq_len * world
    tps = tokens / elapsed
    eng = getattr(getattr(trainer, "model", None), "engine", None)
    if trainer.is_main_process:
        base = None if overrides else BASELINE_TPS.get(world)
        out = {
            "metric": "tokens/sec", "value": round(tps, 1), "unit": "tokens/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1000 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": round(tps / base, 3) if base else None, "dtype": args.precision if args.mode == "ddp" else "bf16", "data": "synthetic",
            "input_pipeline": "native loader (fresh batch per step, in the timed loop)" if loader is not None
            else "resident batches",
            "config": {"model": f"GPT-2 124M (gpt2_{args.model_size} preset, {cfg.num_parameters():,} params, "
                                "LLaMA-style as in the reference)" if args.model_size == "small" and not overrides
                                else f"{args.model_size}+{args.model_override}" if overrides else args.model_size,
                       "global_batch": B * world, "seq_len": args.seq_len,
                       "parallelism": f"{args.mode}{world}", "micro_batch": args.batch_size,
                       "grad_accum": args.grad_accum,
                       "micro_step_fusion": trainer.fusion_factor(args.grad_accum, args.batch_size, args.seq_len),
                       **({"memory_lean": True} if args.memory_lean else {}),
                       **({"memory_first": True} if args.memory_first else {}),
                       **({"pipeline_micro_steps": False} if args.no_pipeline else {}),
                       **({"defer_roles": args.defer_roles} if args.defer_roles else {}),
                       **({"cpu_offload": True} if args.cpu_offload else {})},
            "peak_gb_per_gpu": round(peak, 3), "final_loss": round(loss, 4),
            **({"window": eng.last_window, "stream_placement": eng.queue_placement} if eng is not None else {}),
            **({"window_choice": {"decided": eng.window_auto["decided"], "step_ms": eng.window_auto["ms"]}}
               if eng is not None and eng.window_auto is not None else {}),
            "vs_baseline_linear": None if overrides else round(tps / (12500.0 * world), 3),
        }
        print(json.dumps(out), flush=True)
        if (args.full and dev.type == "cuda") or os.environ.get("DLT_GEMM_REPORT"):
            from distributed_llm_trainer_amd.ops import gemm as gemm_mod
            if gemm_mod.available():
                print(gemm_mod.report(), file=sys.stderr)
                print(json.dumps(gemm_mod.race_report(), indent=1), file=sys.stderr)
    if trainer.distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
