"""The QK-norm and post-norm decode kernels (ops/csrc/decode_norms.hip) against the fp64 references of
tests/decode_norms_ref.py, and the captured step of such a model against the ATen step."""
import functools

import pytest
import torch

from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip
from tests import decode_norms_ref as N
from tests import decode_ref as R
from tests import softcap_ref as S
from tests.test_decode_kernels_gpu import BF, DEV, F32, Guarded, _dev, _pos, check

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _qkn_case(H, wbf16, nkv):
    return _dev(N.qkn_inputs(H, wbf16, nkv)) + hip.rope_tables(64, R.QKV_MAXS, device=DEV)


def _run_qkv(kind, B, H, nkv, pos, ins, ref, tag, post=None):
    """One launch into guarded q and caches; every element against ``ref()``, evaluated after it."""
    h, lnw, w, qn, kn, cos, sin = ins
    nh, maxS = H // 64, R.QKV_MAXS
    hin = h[:B].contiguous()
    q = Guarded((B, H), BF, -777.0)
    kc, vc = Guarded((B, nkv, maxS, 64), BF, -555.0), Guarded((B, nkv, maxS, 64), BF, 333.0)
    posd = _pos(pos)
    if kind == "qkn":
        hip.dec_norm_qkv_qkn(hin, lnw, R.EPS, w, qn, kn, cos, sin, posd, q.t, kc.t, vc.t, nh, nkv, post=post)
    else:
        hip.dec_norm_qkv(hin, lnw, R.EPS, w, cos, sin, posd, q.t, kc.t, vc.t, nh, post=post)
    ref = ref()
    check(tag + ".q", q.t, ref["q"], B)
    check(tag + ".k", kc.t[:, :, pos], ref["k"], B)
    check(tag + ".v", vc.t[:, :, pos], ref["v"], B)
    row = torch.zeros((B, nkv, maxS, 64), dtype=torch.bool, device=DEV)
    row[:, :, pos] = True
    for g, written in ((q, None), (kc, row), (vc, row)):  # the cache rows other than pos are untouched
        g.assert_guards(written)
    assert posd.item() == pos and torch.equal(hin, h[:B])


@pytest.mark.parametrize("B", R.DECODE_BATCHES)
@pytest.mark.parametrize("wbf16", [False, True])
@pytest.mark.parametrize("pos", R.QKV_POS)
@pytest.mark.parametrize("mqa", [False, True])
@pytest.mark.parametrize("H", R.QKV_H)
def test_dec_norm_qkv_qkn(H, mqa, pos, wbf16, B):
    nkv, ins = (1 if mqa else H // 64), _qkn_case(H, wbf16, 1 if mqa else H // 64)
    _run_qkv("qkn", B, H, nkv, pos, ins, lambda: N.qkn_ref(ins[0][:B], *ins[1:], pos, H // 64, nkv),
             f"dec_norm_qkv_qkn[H={H},nkv={nkv},pos={pos},wbf16={int(wbf16)},B={B}]")


@pytest.mark.parametrize("B", R.DECODE_BATCHES)
@pytest.mark.parametrize("RK", R.RES_SHAPES)
def test_dec_gemv_out(RK, B):
    x, w, _ = _dev(R.res_inputs(*RK))
    a, xin = Guarded((B, RK[0]), BF, -777.0), x[:B].contiguous()
    hip.dec_gemv_out(xin, w, a.t)
    g = R.gemv(xin.double(), w)
    check(f"dec_gemv_out[R={RK[0]},K={RK[1]},B={B}]", a.t, R.Checked(g.y, R.gemv_tol(g, RK[1])))
    a.assert_guards()
    assert torch.equal(xin, x[:B])


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("kernel", ("qkv", "qkn", "gu", "gu_geglu", "head", "head_cap"))
@pytest.mark.parametrize("H", R.QKV_H)
def test_post_norm_forms(H, kernel, B):
    """h_out against post_ref; the outputs against the plain reference at the stored residual."""
    a, pnw = _dev(N.post_inputs(H, wbf16=kernel in ("qkn", "gu_geglu", "head_cap")))
    ain, ho = a[:B].contiguous(), Guarded((B, H), F32, 1234.5)
    tag = f"post[{kernel},H={H},B={B}]"
    if kernel in ("qkv", "qkn"):
        ins = _qkn_case(H, False, H // 64)
        (h, lnw), nh = ins[:2], H // 64
        ref = (lambda: N.qkn_ref(ho.t.double(), *ins[1:], 5, nh, nh)) if kernel == "qkn" else \
            (lambda: R.qkv_ref(ho.t.double(), lnw, ins[2], ins[5], ins[6], 5, nh))
        _run_qkv(kernel, B, H, nh, 5, ins, ref, tag, post=(ain, pnw, ho.t))
    elif kernel.startswith("gu"):
        I = R.GU_SHAPES[0][1]
        h, lnw, w = _dev(R.gu_inputs(H, I, False))
        s = Guarded((B, I), BF, -777.0)
        act = "geglu" if kernel == "gu_geglu" else "swiglu"
        hip.dec_norm_gu(h[:B].contiguous(), lnw, R.EPS, w, s.t, activation=act, post=(ain, pnw, ho.t))
        if act == "swiglu":
            check(tag, s.t, R.norm_gu_ref(ho.t.double(), lnw, w), B)
        else:  # the GeGLU arithmetic has its own tests: here the form is held to the plain kernel at h_out
            s2 = torch.empty_like(s.t)
            hip.dec_norm_gu(ho.t.clone(), lnw, R.EPS, w, s2, activation=act)
            assert torch.equal(s.t, s2)
        s.assert_guards()
    else:
        _, V, rows = R.HEAD_SHAPES[0]
        h, lnw, w = _dev(R.head_inputs(H, V, rows, False))
        cap = 30.0 if kernel == "head_cap" else 0.0
        lg, lg0 = Guarded((B, V), F32, 1234.5), torch.empty(B, V, dtype=F32, device=DEV)
        hip.dec_norm_head(h[:B].contiguous(), lnw, R.EPS, w, lg.t, V, softcap=cap, post=(ain, pnw, ho.t))
        hip.dec_norm_head(h[:B].contiguous(), lnw, R.EPS, w, lg0, V, softcap=cap, post=(ain, pnw, None))
        assert torch.equal(lg.t, lg0), "a null h_out changes the logits"
        ref = R.norm_head_ref(ho.t.double(), lnw, w, V)
        check(tag, lg.t, S.dec_head_cap_ref(ref, cap) if cap else ref, B)
        lg.assert_guards()
    check(tag + ".h_out", ho.t, N.post_ref(h[:B], ain, pnw))
    ho.assert_guards()
    assert torch.equal(ain, a[:B])
    hh = h[:B].contiguous()
    with pytest.raises(ValueError):  # h_out must not alias h
        hip.dec_norm_head(hh, lnw, R.EPS, torch.zeros(16, H, dtype=BF, device=DEV),
                          torch.empty(B, 16, dtype=F32, device=DEV), 16, post=(ain, pnw, hh))


# ------------------------------------------------------------------------------ the model
MODELS = {"qk_norm": dict(qk_norm=True), "post_norm": dict(post_norm=True),
          "full": dict(qk_norm=True, post_norm=True, num_kv_heads=2, sliding_window=64, sliding_window_pattern=2,
                       attention_sinks=True, attn_softcap=20.0, logit_softcap=30.0, mlp_activation="geglu")}


@functools.lru_cache(maxsize=None)
def _model(name, unit_norms=False):
    torch.manual_seed(11)
    m = GPT(GPTConfig(vocab_size=1000, hidden_size=256, num_layers=3, num_heads=4, max_seq_len=256, dropout=0.0,
                      attention_dropout=0.0, **MODELS[name]))
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if any(k in n for k in ("q_norm", "k_norm", "post_norm")):
                p.copy_(torch.ones_like(p) if unit_norms else 0.5 + 2.0 * torch.rand(p.shape, generator=g))
    m = m.to(DEV)
    m.enable_engine()
    return m.eval()


@pytest.mark.parametrize("name", MODELS)
def test_decode_fused_step_matches_torch_step(name, monkeypatch):
    from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, forward_cached
    ids, steps = torch.randint(0, 1000, (2, 155), generator=torch.Generator().manual_seed(50)).to(DEV).split([150, 5], 1)

    def graph(m, fused):
        c = KVCache(m.config, 2, DEV, m.engine.act_dtype)
        forward_cached(m, ids, c)
        monkeypatch.setenv("DLT_DECODE_FUSED", fused)
        return DecodeGraph(m, c, c.len)

    with torch.no_grad():
        m = _model(name)
        g0, g1, g2, unit = graph(m, "1"), graph(m, "0"), graph(m, "1"), graph(_model(name, True), "1")
        assert g0.fused and g2.fused and unit.fused and not g1.fused
        assert (g0.qkn, g0.pn) == (name != "post_norm", name != "qk_norm")
        for t in range(5):
            a, b, a2 = (gr(steps[:, t:t + 1]).clone() for gr in (g0, g1, g2))
            assert torch.allclose(a, b, atol=3e-2, rtol=3e-2), (t, (a - b).abs().max().item())
            assert torch.equal(a, a2), "two fused graphs on the same inputs, other logits"
        # the norms are live: the same weights with unit norm vectors give other logits
        assert (unit(steps[:, :1]) - graph(m, "1")(steps[:, :1])).abs().max().item() > 3e-2
    ids = torch.randint(4, 1000, (1, 100), device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    out = m.generate(ids, max_new_tokens=6, top_k=1)
    for t in range(6):  # greedy KV-cached decode == argmax of a full re-forward at each step
        with torch.no_grad():
            lg = m(out[:, :100 + t])[0][0, -1]
        assert lg.argmax().item() == out[0, 100 + t].item() or (lg.max() - lg[out[0, 100 + t]]).item() < 0.05
