"""Grouped stream-K weight gradient (csrc/gemm_wgrad.hip k_gemm_wgrad_grp + k_wgrad_grp_fix):
several dW_p += dY_p^T . X_p of one T in one launch, each problem with its own share
plan -- against the fp32 reference, against the single-problem stream-K kernel bit for
bit, and through the engine's window backward."""
import copy
import functools

import pytest
import torch

from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (Nr, Nc): one tile; 3 row x 2 column tiles; a last half row tile; 2 x 4 tiles
MIXED = ((256, 192), (768, 384), (384, 192), (512, 768))
# one share (the whole tile goes straight into dW); 2 shares over 3 row tiles (each crosses
# a row tile and runs a whole tile straight into dW; 6 tiles on 4 workgroups); 3 shares over
# the full + half row tile; 5 shares over 2 row tiles
EXPLICIT = (1, 2, 3, 5)


def _close(a, b, atol, rtol=0.0, what=""):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    bad = (err > lim).sum().item()
    assert bad == 0, f"{what}: {bad} elements out of tolerance, max err {err.max().item():.3e}"


@functools.lru_cache(maxsize=None)
def _case(T, shapes=MIXED, dtype=torch.bfloat16, pad=0):
    """Operands, non-zero fp32 bases and fp32 references of a group (made once, never
    modified).  pad > 0: dy / x are column slices of buffers `pad` columns wider."""
    g = torch.Generator(device=DEV).manual_seed(T + pad)
    out = []
    for nr, nc in shapes:
        dy = torch.randn(T, nr + pad, device=DEV, generator=g).to(dtype)[:, pad // 2:pad // 2 + nr]
        x = torch.randn(T, nc + pad, device=DEV, generator=g).to(dtype)[:, pad // 2:pad // 2 + nc]
        base = torch.randn(nr, nc, device=DEV, generator=g)
        out.append((dy, x, base, base + dy.float().t() @ x.float()))
    return tuple(out)


def _run(case, shares=None):
    dws = [base.clone() for _, _, base, _ in case]
    assert hip.gemm_wgrad_group([(dw, dy, x) for dw, (dy, x, _, _) in zip(dws, case)], shares)
    return dws


def _check_ref(dws, case, T, what):
    for p, (dw, (_, _, _, ref)) in enumerate(zip(dws, case)):
        _close(dw, ref, 1e-3 * T ** 0.5, 1e-4, f"{what} problem {p}")


@pytest.mark.parametrize("T", [1024, 2048])
@pytest.mark.parametrize("shares", [None, EXPLICIT])
def test_group_matches_reference(T, shares):
    case = _case(T)
    dws = _run(case, shares)
    _check_ref(dws, case, T, f"group T={T} shares={shares}")
    for a, b in zip(dws, _run(case, shares)):  # bitwise run to run
        assert torch.equal(a, b)


@pytest.mark.parametrize("T", [1024, 2048])
def test_group_equals_per_problem_stream_k(T):
    """Every problem keeps its own share plan: bit-identical to gemm_wgrad_sk with it."""
    case = _case(T)
    dws = _run(case, EXPLICIT)
    for p, (dw, (dy, x, base, _), s) in enumerate(zip(dws, case, EXPLICIT)):
        one = base.clone()
        assert hip.gemm_wgrad_sk(one, dy, x, s)
        assert torch.equal(dw, one), (p, (dw - one).abs().max().item())


def test_group_whole_tiles_only():
    """One share per row tile: every tile goes straight into dW and no fix-up is launched."""
    T = 1024
    case = _case(T)
    shares = (1, 3, 2, 2)
    dws = _run(case, shares)
    _check_ref(dws, case, T, "whole-tile group")
    for dw, (dy, x, base, _), s in zip(dws, case, shares):
        one = base.clone()
        assert hip.gemm_wgrad_sk(one, dy, x, s)
        assert torch.equal(dw, one)


def test_group_default_shares_equal_per_problem_stream_k():
    T = 1024
    case = _case(T)
    shares = hip.wgrad_group_shares(T, MIXED)
    for p, (dw, (dy, x, base, _)) in enumerate(zip(_run(case), case)):
        one = base.clone()
        assert hip.gemm_wgrad_sk(one, dy, x, shares[p])
        assert torch.equal(dw, one), p


def test_group_strided_operands():
    """dy / x are column slices of wider buffers (ldy != Nr, ldx != Nc)."""
    T = 1024
    case = _case(T, pad=64)
    assert all(dy.stride(0) != dy.shape[1] and x.stride(0) != x.shape[1] for dy, x, _, _ in case)
    for shares in (None, EXPLICIT):
        _check_ref(_run(case, shares), case, T, f"strided group shares={shares}")


def test_group_fp16():
    T = 1024
    case = _case(T, dtype=torch.float16)
    _check_ref(_run(case, EXPLICIT), case, T, "fp16 group")
    _check_ref(_run(case), case, T, "fp16 group, default shares")


def test_group_bn128():
    """Nc = 128 and 1024: the 256 x 128 column-tile instance."""
    T = 1024
    shapes = ((256, 128), (384, 1024))
    case = _case(T, shapes=shapes)
    assert all(hip.wgrad_bn(nc) == 128 for _, nc in shapes)
    _check_ref(_run(case), case, T, "BN 128 group")
    dws = _run(case, (3, 2))
    _check_ref(dws, case, T, "BN 128 group, explicit shares")
    for dw, (dy, x, base, _), s in zip(dws, case, (3, 2)):
        one = base.clone()
        assert hip.gemm_wgrad_sk(one, dy, x, s)
        assert torch.equal(dw, one)


def test_group_refusals():
    """Refused groups return False and touch no dw."""
    T = 1024
    (dy0, x0, b0, _), (dy1, x1, b1, _) = _case(T)[:2]
    dy128, x128, b128, _ = _case(T, shapes=((256, 128),))[0]

    def refused(problems):
        before = [dw.clone() for dw, _, _ in problems]
        assert hip.gemm_wgrad_group(problems) is False
        torch.cuda.synchronize()
        for (dw, _, _), b in zip(problems, before):
            assert torch.equal(dw, b)
    refused([(b0.clone(), dy0, x0), (b128.clone(), dy128, x128)])  # column tiles 192 and 128
    refused([(b0.clone(), dy0, x0), (b1[:64].clone(), dy1[:, :64], x1)])  # 64 rows do not tile
    refused([(b0.clone(), dy0, x0), (b1.bfloat16(), dy1, x1)])  # a 16-bit dw


def _grads(m):
    return {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}


def test_engine_window_grouped(monkeypatch):
    """train_window with the layer's four weight gradients grouped against the per-role
    routes: equal losses, gradients within the weight-gradient bound; grouped runs are
    bitwise repeatable."""
    from distributed_llm_trainer_amd.models.engine import shift_targets
    cfg = GPTConfig(vocab_size=1000, hidden_size=384, num_layers=2, num_heads=6, intermediate_size=1536,
                    max_seq_len=256, dropout=0.1, attention_dropout=0.1)
    torch.manual_seed(11)
    base = GPT(cfg).to(DEV)
    GA = 2
    data = torch.randint(0, 1000, (GA, 2, 256), device=DEV)
    T = GA * 2 * 256

    launched = []
    real = hip.gemm_wgrad_group

    def counted(problems, *a, **k):
        launched.append(real(problems, *a, **k) and len(problems))
        return launched[-1] is not False
    monkeypatch.setattr(hip, "gemm_wgrad_group", counted)

    def run(group):
        monkeypatch.setenv("DLT_WGRAD_GROUP", group)
        del launched[:]
        m = copy.deepcopy(base)
        e = m.enable_engine(seed=9)
        win = e.train_window([data[j] for j in range(GA)], [shift_targets(data[j]) for j in range(GA)],
                             torch.full((), 1.0 / GA, device=DEV))
        torch.cuda.synchronize()
        return [w.item() for w in win], _grads(m)
    l_on, g_on = run("1")
    assert launched == [4] * cfg.num_layers  # one launch of all four roles per layer
    l_on2, g_on2 = run("1")
    l_off, g_off = run("0")
    assert launched == []
    assert l_on == l_off and l_on == l_on2
    for n in g_on:
        assert torch.equal(g_on[n], g_on2[n]), n
        _close(g_on[n], g_off[n], 1e-3 * T ** 0.5, 1e-4, n)
