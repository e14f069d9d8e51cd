"""GeGLU without a GPU, and the fp64 reference, inputs and model that test_geglu_gpu.py shares.
Reference (fp64 on the 16-bit g, u, ds): z = K (g + 0.044715 g^3), phi = sigmoid(z), 1 - phi = sigmoid(-z),
z' = K (1 + 0.134145 g^2); s = g phi u, dg = ds u (phi + g phi (1 - phi) z'), du = ds g phi.  Tolerance, derived:
half an ulp of the output format (half a subnormal step below its normal range) for the one rounding, plus the
fp32 evaluation EV * (sum of the magnitudes of the terms): each fp32 operation rounds to 2^-24 and exp(-z) =
exp2(-z log2 e) moves e by 4 |z| 2^-24 of its value; phi inherits that, 1 - phi = e phi twice: EV = (8 |z| + 16)
2^-24 with |z| <= 104 (beyond it phi is exactly 0 / 1 in fp32 and the true phi within 2^-126 of it: TINY).  dg's
terms cancel near g = -0.75, so its bound is on |ds u| (|phi| + |g phi (1 - phi) z'|): an absolute floor there."""
import math
import pickle

import pytest
import torch

from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import reference as ref

K, TINY = 2.0 * math.sqrt(2.0 / math.pi), 2.0 ** -125


def geglu_fp64(g, u, ds):
    """{"s" | "du" | "dg": (fp64 value, tolerance)}."""
    hu = torch.finfo(g.dtype).eps / 2  # half an ulp relative to the value; times tiny: half a subnormal step
    fmt, g, u, ds = g.dtype, g.double(), u.double(), ds.double()
    z = K * (g + 0.044715 * g ** 3)
    phi, dz = torch.sigmoid(z), K * (1.0 + 0.134145 * g * g)
    t2 = g * phi * torch.sigmoid(-z) * dz
    s, dg, du = g * phi * u, ds * u * (phi + t2), ds * g * phi
    ev = (8.0 * z.abs().clamp(max=104.0) + 16.0) * 2.0 ** -24
    tol = lambda r, mag, tiny: hu * (r.abs() + torch.finfo(fmt).tiny) + ev * mag + TINY * tiny  # noqa: E731
    return {"s": (s, tol(s, s.abs(), (g * u).abs())), "du": (du, tol(du, du.abs(), (ds * g).abs())),
            "dg": (dg, tol(dg, (ds * u).abs() * (phi + t2.abs()), (ds * u).abs() * 1000))}


def geglu_inputs(dtype, I, M=3):
    gen = torch.Generator().manual_seed(I)
    g, u, ds = ((sc * torch.randn(M, I, generator=gen)).to(dtype) for sc in (2.0, 1.0, 1.0))
    big = torch.finfo(dtype).max
    # the zero of act', +-30, +-max (u, ds small there), the onset of saturation, the clamp at 16
    sp = [-0.80, -0.76, -0.7518, -0.75, -0.74, -0.70, 30.0, -30.0, big, -big, 10.0, -10.0, 9.5, -9.5, 0.0, 16.5, -16.5]
    g.view(-1)[:len(sp)] = torch.tensor(sp, dtype=torch.float64).to(dtype)
    u[g.abs().float() > 1e4], ds[g.abs().float() > 1e4] = 0.125, -0.25
    return g, u, ds


def check(name, out, ref_tol):
    """Inside the tolerance, no NaN, and an exact zero wherever the fp64 value is one (saturated gates)."""
    out, (r, tol) = out.double().cpu(), ref_tol
    w = ((out - r).abs() / tol).masked_fill(~torch.isfinite(out), float("inf")).max().item()
    print(f"{name}: worst |err| / tol = {w:.3f}")
    assert w <= 1.0 and (out[r == 0] == 0).all(), name


def check_unfused(ops, dtype, I, dev):
    g, u, ds = geglu_inputs(dtype, I)
    gu, s_out = torch.cat([g, u], dim=1).to(dev), torch.full((3, I), 7.0, dtype=dtype, device=dev)
    dgu = ops.swiglu_bwd(gu, ds.to(dev), s_out=s_out, activation="geglu")
    assert torch.equal(ops.swiglu_fwd(gu, activation="geglu"), s_out)
    for (name, want), out in zip(geglu_fp64(g, u, ds).items(), (s_out, dgu[:, I:], dgu[:, :I])):
        check(f"geglu {name} {dtype} I={I}", out, want)


def geglu_model(dev):
    torch.manual_seed(0)
    m = GPT(GPTConfig(vocab_size=1000, hidden_size=128, num_layers=2, num_heads=2, max_seq_len=64, dropout=0.0,
                      attention_dropout=0.0, mlp_activation="geglu")).to(dev)
    for layer in m.layers:  # gates of order 1 (the init leaves them near 0, where gelu and silu agree)
        layer.mlp.gate_proj.weight.data.mul_(8.0)
    return m


def engine_and_eager(dev):
    models = [geglu_model(dev), geglu_model(dev)]
    models[1].enable_engine(seed=5)
    ids = torch.randint(4, 1000, (4, 64), generator=torch.Generator().manual_seed(0)).to(dev)
    losses = [m.train()(ids, labels=ids)[1] for m in models]
    torch.autograd.backward(losses)
    grads = [(n, p.grad.float(), q.grad.float()) for (n, p), (_, q) in zip(*(m.named_parameters() for m in models))]
    return [x.item() for x in losses], grads


def test_reference_ops_and_eager_mlp_match_the_fp64_definition():
    check_unfused(ref, torch.float32, 24, "cpu")
    mlp = geglu_model("cpu").layers[0].mlp.double()
    (x, dy), wd = torch.randn(2, 5, 128, dtype=torch.float64), mlp.down_proj.weight
    (s, _), (du, _), (dg, _) = geglu_fp64(mlp.gate_proj(x).detach(), mlp.up_proj(x).detach(), dy @ wd).values()
    y = mlp(x)
    got = (y, *torch.autograd.grad(y, [mlp.gate_proj.weight, mlp.up_proj.weight], dy))
    for a, b in zip(got, (s @ wd.t(), dg.t() @ x, du.t() @ x)):
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-13)


def test_engine_on_the_reference_ops_matches_autograd():
    """The comparison and tolerance of test_postnorm_cpu.py's engine test."""
    losses, grads = engine_and_eager("cpu")
    assert abs(losses[0] - losses[1]) < 1e-5
    for n, a, b in grads:
        assert torch.allclose(a, b, atol=1e-6, rtol=1e-4), n


def test_config_round_trips():
    on, off = GPTConfig(mlp_activation="geglu"), GPTConfig()
    assert "mlp_activation" not in off.to_dict() and "mlp_activation" not in off.__getstate__()
    assert GPTConfig.from_dict(on.to_dict()).mlp_activation == pickle.loads(pickle.dumps(on)).mlp_activation == "geglu"
    old = GPTConfig.__new__(GPTConfig)  # a pickle from before the field existed
    old.__setstate__({k: v for k, v in off.__dict__.items() if k != "mlp_activation"})
    assert old.mlp_activation == "swiglu" and old.to_dict() == off.to_dict()
    with pytest.raises(ValueError):
        GPTConfig(mlp_activation="gelu")


def test_forward_cached_matches_the_full_forward():
    from distributed_llm_trainer_amd.eval.decode import KVCache, forward_cached
    m, ids = geglu_model("cpu").eval(), torch.randint(0, 1000, (1, 5))
    with torch.no_grad():
        full = m(ids)[0][:, -1]
    m.enable_engine()
    lg = forward_cached(m, ids, KVCache(m.config, 1, "cpu", m.engine.act_dtype))
    assert torch.allclose(lg, full, atol=1e-4, rtol=1e-4)
