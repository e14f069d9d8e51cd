"""Prefill over the KV cache on the GPU (ops/csrc/prefill.hip): ``prefill_attn`` against the fp64
references and derived tolerances of tests/attn_ref.py, sink_ref.py and attn_cap_ref.py (T queries at
cache positions p0 .. p0 + T - 1 are rows p0 .. of the causal reference over L = p0 + T keys),
``prefill_qkv_cache`` against the fp64 norm + rotation, then ``forward_cached`` on the HIP route
against its ATen route, and its peak memory.  Each check prints ``RATIO <name> <worst err / tol>``."""
import functools

import pytest
import torch

from distributed_llm_trainer_amd.eval.decode import KVCache, _prefill_fused, forward_cached
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip
from tests import attn_cap_ref as C
from tests import attn_ref as A
from tests import sink_ref as S

pytestmark = pytest.mark.gpu
DEV, MAXS, POISON, NINF = "cuda", 256, 1e4, float("-inf")
BF, HF = A.BF, A.HF


def check(name, out, ref, tol):
    err = (out.detach().cpu().double().reshape(ref.shape) - ref).abs()
    print(f"RATIO {name} {torch.where(tol > 0, err / tol, err).max().item():.4f}")
    assert (err <= tol).all(), f"{name}: {(~(err <= tol)).sum().item()} of {err.numel()} outside the tolerance"


@functools.lru_cache(maxsize=None)
def _qkv(L, nh, nkv, hd, dt, B, sat):
    g = torch.Generator().manual_seed(1000 * L + 100 * nh + 10 * nkv + hd)
    q, k, v = (torch.randn(B, n, L, hd, generator=g) for n in (nh, nkv, nkv))
    if sat:  # the last query's scores far past any cap: tanh saturates to +-1 exactly
        q[:, 0, L - 1] *= 60.0
    return q.to(dt), k.to(dt), v.to(dt)


@functools.lru_cache(maxsize=None)
def _ref(L, W, nh, nkv, hd, dt, B, sink=None, cap=None):
    """Checked o [B, L, nh, hd] of the causal (windowed) attention over all L positions."""
    q, k, v = _qkv(L, nh, nkv, hd, dt, B, cap is not None)
    doc = None if W is None else hip.window_bounds(B, L, W, "cpu")
    sk = None if sink is None else torch.tensor(sink, dtype=torch.float32)
    if cap is not None:
        return C.cap_fwd_ref(q, k, v, hd ** -0.5, cap, doc, sink=sk).o
    return (A.attn_fwd_ref(q, k, v, hd ** -0.5, doc) if sk is None else S.sink_fwd_ref(q, k, v, hd ** -0.5, sk, doc)).o


def _run(p0, T, W, nh, nkv, hd, dt, B, sink=None, cap=None):
    """prefill_attn on the last T queries: the cache rows >= L and the k | v columns of the packed
    buffer hold a large finite poison, the output sits in a guarded buffer."""
    L = p0 + T
    q, k, v = _qkv(L, nh, nkv, hd, dt, B, cap is not None)
    kc, vc = (torch.full((B, nkv, MAXS, hd), POISON, dtype=dt, device=DEV) for _ in range(2))
    kc[:, :, :L], vc[:, :, :L] = k.to(DEV), v.to(DEV)
    qkv = torch.full((B * T, (nh + 2 * nkv) * hd), POISON, dtype=dt, device=DEV)
    qkv[:, :nh * hd] = q[:, :, p0:].transpose(1, 2).reshape(B * T, nh * hd).to(DEV)
    O = A.Guarded((B * T, nh * hd), dt, 3.0, DEV)
    hip.prefill_attn(qkv, kc, vc, p0, O.t, hd ** -0.5, nh, window=W or 0,
                     sink=None if sink is None else torch.tensor(sink, dtype=torch.float32, device=DEV), softcap=cap)
    torch.cuda.synchronize()
    O.assert_guards()
    return O.t


# (p0, T) x a small set of (W, nh, nkv, hd, dtype, B); every W has a case with p0 > W; "L+" = a window >= L
PLAIN = [(0, 2, None, 3, 3, 64, BF, 2), (0, 2, 1, 4, 2, 128, BF, 1), (0, 2, "L+", 4, 1, 64, BF, 2),
         (0, 64, None, 4, 2, 64, BF, 2), (0, 64, 31, 3, 3, 128, BF, 1), (0, 64, 64, 4, 1, 64, HF, 1),
         (0, 65, None, 4, 1, 128, BF, 1), (0, 65, 65, 3, 3, 64, BF, 2), (0, 65, 1, 4, 2, 64, BF, 1),
         (1, 63, None, 3, 3, 128, BF, 2), (1, 63, 64, 4, 2, 64, BF, 2), (1, 63, 31, 4, 1, 64, BF, 1),
         (63, 2, None, 4, 2, 64, BF, 1), (63, 2, 1, 3, 3, 64, BF, 2), (63, 2, 31, 4, 1, 128, BF, 2),
         (63, 2, "L+", 4, 2, 64, BF, 2), (64, 64, None, 4, 1, 64, BF, 2), (64, 64, 31, 4, 2, 128, BF, 1),
         (64, 64, 64, 3, 3, 64, BF, 2), (64, 64, 65, 4, 2, 64, BF, 1), (100, 130, None, 3, 3, 64, BF, 2),
         (100, 130, 1, 4, 2, 64, BF, 1), (100, 130, 31, 4, 1, 64, BF, 2), (100, 130, 64, 4, 2, 128, BF, 1),
         (100, 130, 65, 3, 3, 64, HF, 2), (0, 200, None, 4, 2, 128, BF, 1), (0, 200, 65, 4, 1, 64, BF, 2),
         (0, 200, 64, 3, 3, 64, BF, 1), (0, 200, 31, 4, 2, 64, BF, 2)]


@pytest.mark.parametrize("p0,T,W,nh,nkv,hd,dt,B", PLAIN, ids=lambda v: str(v).replace("torch.", ""))
def test_prefill_attn(p0, T, W, nh, nkv, hd, dt, B):
    W = p0 + T + 5 if W == "L+" else W
    chk = _ref(p0 + T, W, nh, nkv, hd, dt, B)
    check("o", _run(p0, T, W, nh, nkv, hd, dt, B), chk.ref[:, p0:], chk.tol[:, p0:])


FORMS = [(0, 65, None, 3, 3, 64, "deal", None), (63, 2, 31, 4, 2, 64, "deal", None), (100, 130, 65, 4, 1, 128, "ninf", None),
         (64, 64, None, 4, 2, 64, "high", None), (0, 65, None, 3, 3, 64, None, 2.0), (64, 64, 31, 4, 2, 128, "deal", 2.0),
         (100, 130, None, 4, 1, 64, "ninf", 5.0)]


@pytest.mark.parametrize("p0,T,W,nh,nkv,hd,sink,cap", FORMS)
def test_prefill_attn_sink_and_cap_forms(p0, T, W, nh, nkv, hd, sink, cap):
    """SINK and CAP.  "deal": sink_ref's values over the heads; "ninf": every sink -inf, the bits of
    the form without sinks; "high": 100 above every score (|s| < 10 here), o finite and ~ 0.  The CAP
    cases carry one query whose scores saturate the tanh: finite output."""
    sk = {None: None, "deal": tuple(S.sinks_for(nh, 1).tolist()), "ninf": (NINF,) * nh, "high": (110.0,) * nh}[sink]
    out, chk = _run(p0, T, W, nh, nkv, hd, BF, 2, sk, cap), _ref(p0 + T, W, nh, nkv, hd, BF, 2, sk, cap)
    assert torch.isfinite(out.float()).all()
    check(f"o[{sink},{cap}]", out, chk.ref[:, p0:], chk.tol[:, p0:])
    if sink == "ninf":
        assert torch.equal(A.bits(out), A.bits(_run(p0, T, W, nh, nkv, hd, BF, 2, None, cap)))
    if sink == "high":
        assert out.float().abs().max().item() < 1e-30


@pytest.mark.parametrize("T", [2, 65])
@pytest.mark.parametrize("p0", [0, 5, 63])
@pytest.mark.parametrize("nkv", [4, 2])
@pytest.mark.parametrize("qkn", [False, True])
def test_prefill_qkv_cache(qkn, nkv, p0, T):
    """rope(x * rsqrt(mean(x^2) + eps) * w) at position p0 + t in fp64 (README, QK-norm).  Bound: one
    rounding of the kernel's fp32 value to the activation dtype; before it the rotation is two
    products and an add (3 U23 of |u1 c| + |u2 s|) and, with the norm, an fp32 chain of hd terms for
    the mean square plus eps, 1 / hd, rsqrt and the two products of u (hd + 8 U23)."""
    nh, B, eps = 4, 2, 1e-6
    hd, dt = (128 if p0 == 5 else 64), (HF if p0 == 63 else BF)
    maxS, heads, hf, new = p0 + T + 3, nh + 2 * nkv, hd // 2, slice(p0, p0 + T)
    g = torch.Generator().manual_seed(7 * p0 + T + nkv)
    src = (1.5 * torch.randn(B, T, heads, hd, generator=g)).to(dt)
    qw, kw = (0.5 + torch.rand(hd, generator=g) for _ in range(2))
    cos, sin = hip.rope_tables(hd, maxS, device=DEV)
    qkv = src.to(DEV).view(B * T, heads * hd)
    kc, vc = (torch.randn(B, nkv, maxS, hd, generator=g).to(dt).to(DEV) for _ in range(2))
    kc0, vc0 = kc.clone(), vc.clone()
    hip.prefill_qkv_cache(qkv, kc, vc, cos, sin, p0, nh, nkv, qk_norm=(qw.to(DEV), kw.to(DEV)) if qkn else None, eps=eps)
    torch.cuda.synchronize()
    u, rel = src.double()[:, :, :nh + nkv], 3 * A.U23
    if qkn:
        w = torch.cat([qw.expand(nh, hd), kw.expand(nkv, hd)]).double()
        u, rel = u * torch.rsqrt((u * u).mean(-1, keepdim=True) + A.f32(eps)) * w, rel + (hd + 8) * A.U23
    c, s = (t[new].cpu().double()[None, :, None, :] for t in (cos, sin))
    u1, u2 = u[..., :hf], u[..., hf:]
    ref = torch.cat([u1 * c - u2 * s, u2 * c + u1 * s], -1)
    pre = rel * torch.cat([(u1 * c).abs() + (u2 * s).abs(), (u2 * c).abs() + (u1 * s).abs()], -1)
    tol = pre + A.final_rounding(ref, pre, dt)
    got, v_in = qkv.view(B, T, heads, hd), A.bits(src[:, :, nh + nkv:].to(DEV))
    check("q", got[:, :, :nh], ref[:, :, :nh], tol[:, :, :nh])
    check("k", kc[:, :, new].transpose(1, 2), ref[:, :, nh:], tol[:, :, nh:])
    # v: the rows as they were, in the cache and in the packed buffer; no other cache row moved
    assert torch.equal(A.bits(vc[:, :, new].transpose(1, 2)), v_in) and torch.equal(A.bits(got[:, :, nh + nkv:]), v_in)
    for a, b in ((kc, kc0), (vc, vc0)):
        assert torch.equal(A.bits(a[:, :, :p0]), A.bits(b[:, :, :p0]))
        assert torch.equal(A.bits(a[:, :, p0 + T:]), A.bits(b[:, :, p0 + T:]))


# intermediate_size 2 H: forward_cached's ATen MLP holds 16 I bytes of fp32 temporaries per token; at
# I = 4 H they alone are the nh * T * 4 bytes per token of one score tensor at T 1024, and the
# peak-memory test would measure the MLP
MODELS = {"plain": {}, "full": dict(num_kv_heads=2, qk_norm=True, post_norm=True, sliding_window=64,
                                    sliding_window_pattern=2, attention_sinks=True, attn_softcap=20.0)}


@functools.lru_cache(maxsize=None)
def _model(name, max_seq_len=256):
    torch.manual_seed(21)
    m = GPT(GPTConfig(vocab_size=1000, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4,
                      max_seq_len=max_seq_len, dropout=0.0, attention_dropout=0.0, **MODELS[name])).to(DEV)
    m.enable_engine()
    return m.eval()


@pytest.mark.parametrize("name", MODELS)
def test_forward_cached_hip_route_matches_the_aten_route(name, monkeypatch):
    """A 150-token prefill then a 40-token append (p0 > 0, T > 1): the final logits and every cache
    row written, under the tolerances of the fused-versus-ATen decode tests; two HIP runs agree
    bit for bit.

    Measured on an MI355X, worst |d| / (2e-2 + 2e-2 |y|) over the rows of layer 1: "plain" 0.26, "full"
    0.57 (K rows, QK-normed to rms 1.0: one bf16 step at |y| 0.2); layer 0 differs by 0.0002 at most.
    The kernel feeds P to P.V as hi + lo 16-bit parts; with P rounded once to bf16 the "full" K rows
    missed this bound (10 of 48640 elements, up to 1.36 x)."""
    m = _model(name)
    ids = torch.randint(0, 1000, (2, 190), generator=torch.Generator().manual_seed(60)).to(DEV)

    def run(flag):
        monkeypatch.setenv("DLT_PREFILL_FUSED", flag)
        assert _prefill_fused(m, 40) == (flag == "1")
        c = KVCache(m.config, 2, DEV, m.engine.act_dtype)
        forward_cached(m, ids[:, :150], c)
        return forward_cached(m, ids[:, 150:], c), c

    (a, ca), (b, cb), (a2, ca2) = run("1"), run("0"), run("1")
    assert torch.allclose(a, b, atol=3e-2, rtol=3e-2), (a - b).abs().max().item()
    assert torch.equal(a, a2)
    for x, y, x2 in zip(ca.k + ca.v, cb.k + cb.v, ca2.k + ca2.v):
        assert torch.allclose(x[:, :, :190].float(), y[:, :, :190].float(), atol=2e-2, rtol=2e-2)
        assert torch.equal(x, x2)


def test_forward_cached_peak_memory_is_below_one_dense_score_tensor():
    """B 2, T 1024: the HIP route's peak over the call stays under B * nh * T * T * 4 bytes, one
    fp32 score tensor, of which the ATen route holds at least two."""
    m, B, T = _model("plain", 1024), 2, 1024
    ids = torch.randint(0, 1000, (B, T), generator=torch.Generator().manual_seed(61)).to(DEV)
    c = KVCache(m.config, B, DEV, m.engine.act_dtype)
    assert _prefill_fused(m, T)
    forward_cached(m, ids, c)  # the GEMM library takes its workspace at its first call and keeps it
    c.len = 0
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    forward_cached(m, ids, c)
    peak = torch.cuda.max_memory_allocated() - before
    print(f"PEAK {peak} bound {B * m.config.num_heads * T * T * 4}")
    assert peak < B * m.config.num_heads * T * T * 4
