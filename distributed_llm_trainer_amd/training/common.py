"""Pieces shared by the DDP and FSDP trainers: process-group bootstrap, device
selection, seeding, LR schedule, memory stats and the YAML/CLI config merge."""
from __future__ import annotations

import datetime
import json
import math
import os
import random
import time
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist


def setup_distributed(require: bool = False, timeout_s: Optional[float] = None):
    """Returns (distributed, rank, world_size, local_rank).

    Backend: "nccl" (= RCCL on ROCm) when a GPU is present, else "gloo" (CPU tests /
    the plumbing config).  ``DLT_PG_TIMEOUT`` (seconds) bounds every collective so a
    dead rank surfaces as an error instead of a hang.
    """
    distributed = dist.is_initialized() or "RANK" in os.environ or require
    if distributed and not dist.is_initialized():
        # RCCL's xGMI defaults, read when the communicator is created (parallel/comm_env.py)
        from ..parallel import comm_env
        comm_env.apply()
        backend = os.environ.get("DLT_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        t = timeout_s or float(os.environ.get("DLT_PG_TIMEOUT", "1800"))
        kw = dict(backend=backend, timeout=datetime.timedelta(seconds=t))
        if backend == "nccl" and torch.cuda.is_available():
            lr = _device_index(int(os.environ.get("LOCAL_RANK", 0)))
            torch.cuda.set_device(lr)
            kw["device_id"] = torch.device(f"cuda:{lr}")
        dist.init_process_group(**kw)
    if distributed:
        return True, dist.get_rank(), dist.get_world_size(), int(os.environ.get("LOCAL_RANK", 0))
    return False, 0, 1, 0


def _device_index(local_rank: int) -> int:
    """GPU of a local rank.  One rank per GPU; ``DLT_SHARE_GPU=1`` folds ranks onto the
    visible GPUs (local_rank mod count) -- only for rehearsing multi-rank code paths
    with the gloo backend on a 1-GPU box (RCCL itself rejects two ranks per GPU)."""
    if os.environ.get("DLT_SHARE_GPU") == "1":
        return local_rank % max(1, torch.cuda.device_count())
    return local_rank


def select_device(local_rank: int) -> torch.device:
    if torch.cuda.is_available() and os.environ.get("DLT_FORCE_CPU") != "1":
        d = torch.device(f"cuda:{_device_index(local_rank)}")
        torch.cuda.set_device(d)
        return d
    return torch.device("cpu")


def seed_all(seed: int) -> None:
    random.seed(seed)
    np.random.seed(seed % (2 ** 32))
    torch.manual_seed(seed)


def cosine_lr(step: int, lr: float, warmup: int, max_steps: int, clamp: bool = True) -> float:
    """Linear warmup then cosine to 0.1*lr (``ddp_trainer.py:262-271``).  The DDP
    reference does not clamp the decay ratio (LR rises again after max_steps, Q6);
    ``clamp=True`` applies the FSDP trainer's clamp (``fsdp_trainer.py:354``)."""
    if step < warmup:
        return lr * (step / warmup)
    denom = max(1, max_steps - warmup)
    ratio = (step - warmup) / denom
    if clamp:
        ratio = min(ratio, 1.0)
    coeff = 0.5 * (1.0 + math.cos(math.pi * ratio))
    min_lr = 0.1 * lr
    return min_lr + coeff * (lr - min_lr)


def memory_stats(device) -> dict:
    """GB (1e9), like ``fsdp_trainer.py:496-505``."""
    if torch.device(device).type != "cuda":
        return {"allocated_gb": 0.0, "reserved_gb": 0.0, "max_allocated_gb": 0.0}
    return {"allocated_gb": torch.cuda.memory_allocated(device) / 1e9,
            "reserved_gb": torch.cuda.memory_reserved(device) / 1e9,
            "max_allocated_gb": torch.cuda.max_memory_allocated(device) / 1e9}


FUSE_TOKENS = 16384  # rows of a fused micro-step chain (GEMM M) the auto rule aims for


def micro_step_fusion(requested: int, GA: int, micro_bs: int, seq_len: int, gpu_engine: bool) -> int:
    """Number of micro-steps executed as one chain (a divisor of GA).

    Measured on one MI355X (small, micro-batch 8 x GA 4, seq 1024): chains of 16
    sequences (F = 2, GEMM M = 16384) run 43.2 ms per optimizer step vs 46.1 ms for
    four 8-sequence chains -- the projection GEMMs reach ~1 PF/s at M >= 16384 (vs
    0.4-0.9 at 8192) and two chains still pipeline (profiles/r2_microbatch_ab.md).
    ``requested`` > 0 forces F (must divide GA); 0 = auto (GPU engine only)."""
    if requested > 0:
        if GA % requested:
            raise ValueError(f"micro_step_fusion={requested} must divide gradient_accumulation_steps={GA}")
        return requested
    if not gpu_engine or GA < 2:
        return 1
    best = 1
    for f in range(1, GA + 1):
        if GA % f == 0 and f * micro_bs * seq_len <= FUSE_TOKENS and GA // f >= 2:
            best = f
    return best


def gemm_plan_hook() -> None:
    """After a step: write the GEMM plan file once if ``DLT_GEMM_PLAN`` asks for one
    (``ops/gemm.py`` ``maybe_save_plan``; a no-op without the planner)."""
    if not (os.environ.get("DLT_GEMM_PLAN") or os.environ.get("DLT_GEMM_PLAN_OUT")):
        return
    from ..ops import gemm
    gemm.maybe_save_plan()


def global_mean_loss(total: torch.Tensor, world: int) -> float:
    """Mean of the ranks' step losses (the reference logs rank 0's local
    loss; that line is kept, the metrics JSONL also gets this).  A collective: every
    rank must call it on the same steps."""
    t = total.detach().reshape(1).float().clone()
    dist.all_reduce(t)
    return float(t.item()) / world


EVAL_SEED_OFFSET = 1_000_003  # the dummy held-out stream's seed is the training seed + this


class HeldOutBatches:
    """The first batches of a held-out loader, the same ones at every evaluation: the
    native loader is rewound (``seek(0)``), any other loader is read once -- with the
    global RNG forked, so a shuffling sampler draws nothing from the training run's
    stream -- and its batches are kept on the host."""

    def __init__(self, loader):
        self.loader = loader
        self._kept = []

    def take(self, n: int):
        if hasattr(self.loader, "seek"):
            self.loader.seek(0)
            it = iter(self.loader)
            for _ in range(n):
                yield unwrap_batch(next(it))
            return
        if len(self._kept) < n:
            with torch.random.fork_rng(devices=[]):
                it = iter(self.loader)
                try:
                    self._kept = [unwrap_batch(next(it)).clone() for _ in range(n)]
                except StopIteration:
                    raise ValueError(f"the held-out loader has fewer than {n} batches") from None
                del it
        yield from self._kept[:n]


@torch.no_grad()
def evaluate_held_out(model, held_out: HeldOutBatches, n_batches: int, device, distributed: bool) -> dict:
    """Token-weighted mean held-out loss over ``n_batches`` batches per rank.  Every rank
    runs the same number of forwards (FSDP gathers are collectives); the loss sum and the
    token count are each all-reduced, then divided.  Reads the model only."""
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)  # eval_s is the evaluation's time, not the queued training work's
    t0 = time.time()
    acc = torch.zeros(2, dtype=torch.float64, device=device)
    for ids in held_out.take(int(n_batches)):
        loss_sum, n = model.eval_loss_sum(ids.to(device, non_blocking=True))
        acc[0] += loss_sum.double()
        acc[1] += n.double()
    if distributed and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(acc)
    loss_sum, tokens = acc.tolist()
    val_loss = loss_sum / max(tokens, 1.0)
    return {"val_loss": val_loss, "val_ppl": math.exp(min(val_loss, 700.0)), "eval_tokens": int(tokens),
            "eval_s": time.time() - t0}


def held_out_of(cache: dict, loader) -> HeldOutBatches:
    """``loader`` as HeldOutBatches, one per loader (so its kept batches survive between calls)."""
    if isinstance(loader, HeldOutBatches):
        return loader
    if id(loader) not in cache:
        cache[id(loader)] = HeldOutBatches(loader)
    return cache[id(loader)]


def log_evaluation(step: int, res: dict, metrics_f=None) -> None:
    """The main process's evaluation output: one log line, one metrics JSONL record."""
    print(f"Step {step:6d} | Val loss: {res['val_loss']:.4f} | Val ppl: {res['val_ppl']:.2f}", flush=True)
    if metrics_f:
        metrics_f.write(json.dumps({"step": step, **res}) + "\n")
        metrics_f.flush()


def add_eval_args(p) -> None:
    p.add_argument("--eval_interval", type=int, default=None,
                   help="evaluate every this many steps (and once after the last) when --eval_batches > 0")
    p.add_argument("--eval_batches", type=int, default=None,
                   help="held-out batches per rank and evaluation; 0 (default) = no evaluation")
    p.add_argument("--eval_data_path", type=str, default=None,
                   help="held-out data for tinystories / openwebtext (same formats as --data_path)")


def add_doc_mask_args(p) -> None:
    p.add_argument("--doc_sep_token", type=int, default=None, metavar="ID",
                   help="intra-document attention masking for packed sequences: token ID ends a document "
                        "(GPT-2: 50256) and a token attends only within its own document; training and "
                        "--eval_batches evaluation both use it (default: plain causal attention)")


class LossParts:
    """The (cross-entropy, weighted z term) parts of an optimizer step's loss, summed on the
    device as the trainers' ``total`` is (no host sync per micro-step).  Inactive without a
    z-loss coefficient: the metrics and the log line are then what they always were."""

    def __init__(self, coef: float, device):
        self.sum = torch.zeros(2, dtype=torch.float32, device=device) if coef > 0.0 else None

    def add(self, pair, chains: int) -> None:
        """``pair``: ``last_loss_parts`` of one micro-step chain; ``chains`` per optimizer step."""
        if self.sum is not None:
            self.sum += torch.stack([pair[0].detach().float(), pair[1].detach().float()]) / chains

    def into(self, out: dict, sync: bool) -> None:
        """``ce_loss`` / ``z_loss`` next to ``loss``: floats when ``sync`` (one copy), else tensors."""
        if self.sum is not None:
            out["ce_loss"], out["z_loss"] = self.sum.tolist() if sync else (self.sum[0], self.sum[1])


def z_loss_suffix(metrics: dict) -> str:
    """`` | Z loss: ...`` for the step line of a run with a z-loss coefficient, else nothing."""
    return f" | Z loss: {float(metrics['z_loss']):.6f}" if "z_loss" in metrics else ""


def z_loss_record(metrics: dict) -> dict:
    """The JSONL record's ``ce_loss`` / ``z_loss`` of a run with a z-loss coefficient, else nothing."""
    return {k: float(metrics[k]) for k in ("ce_loss", "z_loss") if k in metrics}


def add_z_loss_args(p) -> None:
    p.add_argument("--z_loss", type=float, default=None, metavar="COEF",
                   help="auxiliary z-loss: the training loss is ce + COEF * mean(logsumexp(logits)^2) (PaLM: 1e-4); "
                        "validation loss stays plain cross-entropy (default 0: off)")


def add_model_args(p) -> None:
    p.add_argument("--num_kv_heads", type=int, default=None, metavar="N",
                   help="grouped-query attention: N key/value heads shared by groups of num_heads / N query "
                        "heads (N must divide num_heads; 1 = multi-query).  Overrides the YAML's "
                        "model.num_kv_heads and the preset (default: num_heads, plain multi-head attention)")
    p.add_argument("--qk_norm", action="store_true", default=None,
                   help="QK-norm: an RMSNorm over head_dim on every query and key head before RoPE, with one "
                        "q_norm and one k_norm weight per layer.  Overrides the YAML's model.qk_norm and the "
                        "preset (default: off)")
    p.add_argument("--sliding_window", type=int, default=None, metavar="W",
                   help="sliding-window attention: a token attends to the last W tokens, its own included "
                        "(W >= 1).  Overrides the YAML's model.sliding_window and the preset (default: plain "
                        "causal attention)")
    p.add_argument("--sliding_window_pattern", type=int, default=None, metavar="N",
                   help="with --sliding_window: every N-th layer (layers N, 2N, ... counted from 1) stays global "
                        "(plain causal) and the others are windowed (N >= 2).  Overrides the YAML's "
                        "model.sliding_window_pattern (default: every layer is windowed)")
    p.add_argument("--attention_sinks", action="store_true", default=None,
                   help="attention sinks: one learned fp32 logit per query head and layer that takes part in the "
                        "softmax denominator and has no value row (the gpt-oss form).  Overrides the YAML's "
                        "model.attention_sinks and the preset (default: off)")
    p.add_argument("--logit_softcap", type=float, default=None, metavar="CAP",
                   help="final-logit soft-capping: the model's logits are CAP * tanh(logits / CAP) (a finite "
                        "CAP > 0; Gemma-2 and the GPT-2 speed-run recipes use 30), in training, evaluation and "
                        "generation, and saved in checkpoints.  Overrides the YAML's model.logit_softcap and the "
                        "preset (default: off)")
    p.add_argument("--attn_softcap", type=float, default=None, metavar="CAP",
                   help="attention-score soft-capping: every layer's scaled scores are CAP * tanh(scores / CAP) "
                        "before the masks and the softmax (a finite CAP > 0; Gemma-2 uses 50), in training, "
                        "evaluation and generation, and saved in checkpoints.  Overrides the YAML's "
                        "model.attn_softcap and the preset (default: off)")
    p.add_argument("--post_norm", action="store_true", default=None,
                   help="post-norms (the Gemma-2/3 sandwich block): a second RMSNorm on the attention and the MLP "
                        "branch output, before the hidden dropout and the residual add, with an attn_post_norm "
                        "and an mlp_post_norm weight per layer.  Overrides the YAML's model.post_norm and the "
                        "preset (default: off)")


def apply_model_args(args, model_config) -> None:
    """CLI > YAML > preset for the model flags of :func:`add_model_args`."""
    nkv = getattr(args, "num_kv_heads", None)
    if nkv is not None:
        if nkv < 1 or model_config.num_heads % nkv:
            raise ValueError(f"--num_kv_heads {nkv} must divide num_heads ({model_config.num_heads})")
        model_config.num_kv_heads = nkv
    if getattr(args, "qk_norm", None) is not None:
        model_config.qk_norm = bool(args.qk_norm)
    if getattr(args, "attention_sinks", None) is not None:
        model_config.attention_sinks = bool(args.attention_sinks)
    if getattr(args, "post_norm", None) is not None:
        model_config.post_norm = bool(args.post_norm)
    sw, swp = getattr(args, "sliding_window", None), getattr(args, "sliding_window_pattern", None)
    cap = getattr(args, "logit_softcap", None)
    acap = getattr(args, "attn_softcap", None)
    if sw is not None or swp is not None or cap is not None or acap is not None:
        if sw is not None:
            model_config.sliding_window = sw
        if swp is not None:
            model_config.sliding_window_pattern = swp
        if cap is not None:
            model_config.logit_softcap = cap
        if acap is not None:
            model_config.attn_softcap = acap
        model_config.__post_init__()  # the config's own validation (ValueError)


def unwrap_batch(batch):
    if isinstance(batch, dict):
        return batch["input_ids"]
    if isinstance(batch, (list, tuple)):
        return batch[0]
    return batch
