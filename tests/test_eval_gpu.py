"""The loss-only evaluation forward of the fused engine on the MI355X: value against
``GPT.forward`` with labels, the unfused head (``DLT_EVAL_HEAD=unfused``), peak memory
without a logits buffer, and training left bit-identical by evaluations between steps.

The bound is the per-row bound of tests/test_lmhead_loss_gpu.py applied to the mean: the
mean over the predicted rows of 2^-7 * max_j |l[m, j]| (bf16), plus that file's EPS."""
import pytest
import torch

from distributed_llm_trainer_amd.models import GPT, GPTConfig
from tests.test_lmhead_loss_gpu import EPS, FACTOR

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, S = 4, 512  # 2048 rows: logits would be 2048 x 50304 x 2 B = 206 MB, the loss scratch is 6.5 MB


def _cfg(dropout=0.0):
    return GPTConfig(vocab_size=50257, hidden_size=128, num_layers=1, num_heads=2, max_seq_len=S, dropout=dropout,
                     attention_dropout=dropout)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(11)
    m = GPT(_cfg()).to(DEV)
    m.enable_engine(seed=2)
    m.eval()
    return m


@pytest.fixture(scope="module")
def batch(model):
    ids = torch.randint(0, 50257, (B, S), device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    labels = ids.clone()
    labels[1, 100:140] = -100
    with torch.no_grad():
        logits, loss = model(ids, labels=labels)  # the unfused head, logits returned
    rows = (labels[:, 1:] != -100)
    bound = FACTOR[torch.bfloat16] * logits[:, :-1].float().abs().amax(dim=-1)[rows].mean().item() + EPS
    return ids, labels, loss.item(), bound


def test_eval_loss_matches_forward(model, batch):
    ids, labels, want, bound = batch
    before = model.engine.micro_counter
    got = model.eval_loss(ids, labels).item()
    print(f"eval_loss {got:.6f} forward {want:.6f} diff {abs(got - want):.3e} bound {bound:.3e}")
    assert model.engine.micro_counter == before
    assert abs(got - want) <= bound


def test_eval_loss_unfused_head_matches(model, batch, monkeypatch):
    ids, labels, want, bound = batch
    fused = model.eval_loss(ids, labels).item()
    monkeypatch.setenv("DLT_EVAL_HEAD", "unfused")
    unfused = model.eval_loss(ids, labels).item()
    print(f"fused {fused:.6f} unfused {unfused:.6f} forward {want:.6f} bound {bound:.3e}")
    assert abs(unfused - want) <= bound and abs(unfused - fused) <= bound


def test_eval_loss_keeps_no_logits(model, batch):
    ids, labels, _, _ = batch
    model.eval_loss(ids, labels)  # warm-up: GEMM plans, RoPE tables
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    model.eval_loss(ids, labels)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise across eval_loss: {rise / 1e6:.1f} MB")
    assert rise < 100e6


def test_evaluation_between_steps_leaves_training_bit_identical():
    from distributed_llm_trainer_amd.training.configs import TrainingConfig
    from distributed_llm_trainer_amd.training.ddp_trainer import DistributedTrainer
    g = torch.Generator(DEV).manual_seed(6)
    data = [torch.randint(0, 50257, (4, S), device=DEV, generator=g) for _ in range(3)]
    held = [torch.randint(0, 50257, (B, S), device=DEV, generator=g) for _ in range(2)]
    res = []
    for with_eval in (False, True):
        tc = TrainingConfig(batch_size=2, gradient_accumulation_steps=2, warmup_steps=1, learning_rate=1e-3)
        tr = DistributedTrainer(_cfg(0.1), tc)
        vals = []
        for d in data:
            tr.train_step({"input_ids": d})
            if with_eval:
                vals.append(tr.evaluate(held, 2)["val_loss"])
        res.append((tr.flat_params().detach().clone(), tr.model.engine.micro_counter, tr.global_step,
                    tr.tokens_seen))
        if with_eval:
            assert all(v == v and 0 < v < 30 for v in vals), vals
    assert res[0][1:] == res[1][1:]
    assert torch.equal(res[0][0], res[1][0]), (res[0][0] - res[1][0]).abs().max().item()
