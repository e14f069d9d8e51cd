"""Held-out evaluation on CPU: the reference ``lmhead_loss`` op, ``evaluate`` of both
trainers (single process and 2 gloo ranks) and the evaluation CLI flags."""
import json

import pytest
import torch
import torch.nn.functional as F

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.ops import reference as ref
from tests.dist_utils import run_multiprocess

TINY = dict(vocab_size=384, hidden_size=64, num_layers=2, num_heads=4, max_seq_len=32, dropout=0.1,
            attention_dropout=0.1)


def _data(step, rank, n=4, seq=32, vocab=384):
    g = torch.Generator().manual_seed(1000 * step + rank)
    return torch.randint(0, vocab, (n, seq), generator=g)


def _held_out(rank, n_batches=2):
    return [_data(500 + i, rank, n=2) for i in range(n_batches)]


# ------------------------------------------------------------------ reference op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_reference_lmhead_loss_is_cross_entropy_of_rounded_logits(dtype):
    torch.manual_seed(0)
    M, K, Vp, V = 70, 48, 64, 51
    nf = torch.randn(M, K).to(dtype)
    w = (torch.randn(Vp, K) * 0.3).to(dtype)
    w[V:] = 30.0  # padding rows: must be masked by V, not by their values
    tgt = torch.randint(0, V, (M,))
    tgt[0], tgt[1], tgt[5:9] = 0, V - 1, -100
    loss, lse = ref.lmhead_loss(nf, w, tgt, V, block_rows=32)  # three row blocks, the last ragged
    logits = (nf.float() @ w[:V].float().t()).to(dtype).float()
    want = F.cross_entropy(logits, tgt, reduction="none", ignore_index=-100)
    assert loss.dtype == torch.float32 and lse.dtype == torch.float32
    assert torch.allclose(loss, want, atol=1e-5, rtol=1e-6), (loss - want).abs().max()
    assert torch.allclose(lse, torch.logsumexp(logits, dim=1), atol=1e-5, rtol=1e-6)
    assert (loss[tgt == -100] == 0).all()
    # within the rounding bound of the unrounded product (tests/test_lmhead_loss_gpu.py)
    l32 = nf.float() @ w[:V].float().t()
    want32 = F.cross_entropy(l32, tgt, reduction="none", ignore_index=-100)
    factor = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -23}[dtype]
    assert ((loss - want32).abs() <= factor * l32.abs().max(dim=1).values + 1e-5).all()


def test_lmhead_loss_is_served_by_the_op_tables():
    ns = ops.for_device("cpu")
    assert ns.lmhead_loss is ref.lmhead_loss and ns.lmhead_loss_fits(3, 5, 7)


# ------------------------------------------------------------------ model
def test_gpt_eval_loss_engine_matches_eager():
    from distributed_llm_trainer_amd.models import GPT, GPTConfig
    torch.manual_seed(1)
    model = GPT(GPTConfig(**TINY))
    ids = _data(0, 0)
    labels = ids.clone()
    labels[0, 5:9] = -100
    model.train()  # eval_loss runs without dropout whatever the mode, and leaves the mode alone
    eager = model.eval_loss(ids, labels)
    assert model.training
    model.eval()
    _, want = model(ids, labels=labels)
    assert torch.allclose(eager, want, atol=1e-6)
    model.train()
    eng = model.enable_engine()
    before = eng.micro_counter
    got = model.eval_loss(ids, labels)
    assert eng.micro_counter == before and model.training
    assert torch.allclose(got, want, atol=2e-5), (got, want)


# ------------------------------------------------------------------ DDP trainer, one process
def _ddp_trainer(GA=2):
    from distributed_llm_trainer_amd.models.config import GPTConfig
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=GA, warmup_steps=1, max_steps=100,
                        learning_rate=1e-2)
    return DistributedTrainer(GPTConfig(**TINY), tc)


def _eager_mean_ce(state, batches):
    """Token-weighted mean next-token loss of the eager model over ``batches``."""
    from distributed_llm_trainer_amd.models import GPT, GPTConfig
    model = GPT(GPTConfig(**TINY))
    model.load_state_dict({k: v for k, v in state.items() if "rotary" not in k}, strict=False)
    model.eval()
    total, count = 0.0, 0
    with torch.no_grad():
        for ids in batches:
            logits, _ = model(ids)
            total += F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]).double(), ids[:, 1:].reshape(-1),
                                     reduction="sum").item()
            count += ids[:, 1:].numel()
    return total / count, count


def test_ddp_evaluate_matches_eager_and_rewinds():
    from distributed_llm_trainer_amd.data import create_dummy_dataloader
    from distributed_llm_trainer_amd.utils.checkpoint import model_state_dict_cpu
    tr = _ddp_trainer()
    tr.train_step({"input_ids": _data(0, 0)})  # leaves a recorded (lazy) optimizer step behind
    held = _held_out(0, 3)
    res = tr.evaluate(held, 3)
    want, count = _eager_mean_ce(model_state_dict_cpu(tr.model), held)
    assert res["eval_tokens"] == count and res["eval_s"] >= 0
    assert abs(res["val_loss"] - want) < 2e-5, (res, want)
    assert abs(res["val_ppl"] - torch.tensor(want).exp().item()) < 1e-2
    # a shuffling loader and (when built) the native loader: two evaluations see the same batches
    for native in (False, True):
        loader = create_dummy_dataloader(batch_size=2, seq_len=32, vocab_size=384, num_batches=8, seed=77,
                                         native=native)
        a, b = tr.evaluate(loader, 2), tr.evaluate(loader, 2)
        assert a["val_loss"] == b["val_loss"] and a["eval_tokens"] == 2 * 2 * 31


def test_ddp_evaluation_leaves_training_bit_identical():
    runs = []
    for with_eval in (False, True):
        tr = _ddp_trainer()
        rng0 = torch.random.get_rng_state()
        for s in range(3):
            tr.train_step({"input_ids": _data(s, 0)})
            if with_eval:
                tr.flush_optimizer()  # (the recorded step also zeroes the gradients when it is applied)
                grad = tr.store.grad.clone()
                tr.evaluate(_held_out(0), 2)
                assert torch.equal(tr.store.grad, grad), "evaluation touched the gradient buffer"
        assert torch.equal(torch.random.get_rng_state(), rng0) or not with_eval
        runs.append((tr.flat_params().clone(), tr.model.engine.micro_counter, tr.global_step, tr.tokens_seen))
    (p0, *c0), (p1, *c1) = runs
    assert c0 == c1
    assert torch.equal(p0, p1), (p0 - p1).abs().max()


# ------------------------------------------------------------------ 2 gloo ranks
def _ddp_eval_worker(rank, world):
    from distributed_llm_trainer_amd.utils.checkpoint import model_state_dict_cpu
    tr = _ddp_trainer()
    tr.train_step({"input_ids": _data(0, rank)})
    res = tr.evaluate(_held_out(rank), 2)
    return res, model_state_dict_cpu(tr.model)


def _fsdp_eval_worker(rank, world):
    from distributed_llm_trainer_amd.models.config import GPTConfig
    from distributed_llm_trainer_amd.training.configs import FSDPConfig, FSDPTrainingConfig
    from distributed_llm_trainer_amd.training.fsdp_trainer import FSDPTrainer
    tc = FSDPTrainingConfig(batch_size=2, gradient_accumulation_steps=2, warmup_steps=1, max_steps=100,
                            learning_rate=1e-2)
    tr = FSDPTrainer(GPTConfig(**TINY), tc, FSDPConfig(sharding_strategy="FULL_SHARD", reduce_dtype="fp32"))
    tr.train_step({"input_ids": _data(0, rank)})
    before = tr.runtime.master_flat.clone()
    res = tr.evaluate(_held_out(rank), 2)
    assert torch.equal(tr.runtime.master_flat, before)
    return res, tr._full_state()


@pytest.mark.parametrize("worker", [_ddp_eval_worker, _fsdp_eval_worker], ids=["ddp", "fsdp_full_shard"])
def test_two_ranks_report_the_global_token_weighted_mean(worker):
    (r0, sd0), (r1, _) = run_multiprocess(worker, world=2)
    assert r0["val_loss"] == r1["val_loss"] and r0["eval_tokens"] == r1["eval_tokens"]
    want, count = _eager_mean_ce(sd0, _held_out(0) + _held_out(1))
    assert r0["eval_tokens"] == count
    assert abs(r0["val_loss"] - want) < 2e-5, (r0, want)


# ------------------------------------------------------------------ CLI
YAML = """
model:
  vocab_size: 256
  hidden_size: 64
  num_layers: 2
  num_heads: 2
  max_seq_len: 32
training:
  batch_size: 2
  gradient_accumulation_steps: 2
  learning_rate: 0.001
  warmup_steps: 2
  log_interval: 1
data:
  dataset: dummy
"""


@pytest.mark.parametrize("which", ["ddp", "fsdp"])
def test_cli_eval_flags(which, tmp_path, capsys):
    from distributed_llm_trainer_amd.training import ddp_trainer, fsdp_trainer
    main = ddp_trainer.main if which == "ddp" else fsdp_trainer.main
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(YAML)
    base = ["--config", str(cfg), "--max_steps", "4", "--no_final_save", "--checkpoint_dir", str(tmp_path / "ck")]
    on, off = str(tmp_path / "on.jsonl"), str(tmp_path / "off.jsonl")
    tr_on = main(base + ["--eval_batches", "2", "--eval_interval", "2", "--metrics_jsonl", on])
    out = capsys.readouterr().out
    assert "Step      2 | Val loss: " in out and "Step      4 | Val loss: " in out and "| Val ppl: " in out
    recs = [r for r in map(json.loads, open(on)) if "val_loss" in r]
    assert [r["step"] for r in recs] == [2, 4]
    for r in recs:
        assert r["val_loss"] == r["val_loss"] and abs(r["val_loss"]) < 100 and r["val_ppl"] > 1
        assert r["eval_tokens"] == 2 * 2 * 31 and r["eval_s"] >= 0
    tr_off = main(base + ["--metrics_jsonl", off])
    assert "Val loss" not in capsys.readouterr().out
    assert not [r for r in map(json.loads, open(off)) if "val_loss" in r]
    # the training records are the same with and without evaluation
    strip = lambda path: [(r["step"], r["loss"]) for r in map(json.loads, open(path)) if "loss" in r]  # noqa: E731
    assert strip(on) == strip(off)
    if which == "ddp":
        assert torch.equal(tr_on.flat_params(), tr_off.flat_params())
    else:
        assert torch.equal(tr_on.runtime.master_flat, tr_off.runtime.master_flat)


def test_cli_eval_needs_held_out_data_for_text_datasets():
    from distributed_llm_trainer_amd.training import ddp_trainer
    with pytest.raises(ValueError, match="--eval_data_path"):
        ddp_trainer.main(["--dataset", "tinystories", "--eval_batches", "1", "--max_steps", "1"])
