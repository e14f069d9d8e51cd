"""The FP8 (e4m3) KV cache on the GPU; rows a kernel must not read hold the e4m3 NaN byte."""
import functools
import json
import os

import pytest
import torch

from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, forward_cached
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import hip
from tests import attn_cap_ref as C
from tests import attn_ref as A
from tests import decode_win_ref as WN
from tests import sink_ref as S
from tests.kv_fp8_ref import FP8, NAN_BYTE, PLANT, Cache8, planted, quant

pytestmark = pytest.mark.gpu
DEV, BF, HF, SCALE = "cuda", A.BF, A.HF, 0.125


def check(name, out, ref, tol):
    assert torch.isfinite(out.float()).all(), f"{name}: not finite (a row past the written cache was read?)"
    err = (out.detach().cpu().double().reshape(ref.shape) - ref).abs()
    print(f"RATIO {name} {torch.where(tol > 0, err / tol, err).max().item():.4f}")
    assert (err <= tol).all(), f"{name}: {(~(err <= tol)).sum().item()} of {err.numel()} outside the tolerance"


@pytest.mark.parametrize("T,p0", [(1, 0), (3, 5), (65, 63)])
@pytest.mark.parametrize("nkv", [4, 2])
@pytest.mark.parametrize("qkn", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_prefill_writer_bytes(hd, qkn, nkv, T, p0):
    nh, B, maxS, heads = 4, 2, p0 + T + 3, 4 + 2 * nkv
    dt = HF if (hd == 128 and nkv == 2) else BF
    g = torch.Generator().manual_seed(hd + 7 * p0 + nkv)
    src = planted(torch.randn(B, T, heads, hd, generator=g)).to(dt).view(B * T, heads * hd).to(DEV)
    qk = tuple((0.5 + torch.rand(hd, generator=g)).to(DEV) for _ in range(2)) if qkn else None
    cos, sin = hip.rope_tables(hd, maxS, device=DEV)
    q16, k16, v16 = src.clone(), *(torch.zeros(B, nkv, maxS, hd, dtype=dt, device=DEV) for _ in range(2))
    hip.prefill_qkv_cache(q16, k16, v16, cos, sin, p0, nh, nkv, qk_norm=qk)
    q8, k8, v8 = src.clone(), Cache8((B, nkv, maxS, hd), 0x55, DEV), Cache8((B, nkv, maxS, hd), 0xAA, DEV)
    hip.prefill_qkv_cache(q8, k8.t, v8.t, cos, sin, p0, nh, nkv, qk_norm=qk)
    torch.cuda.synchronize()
    new = slice(p0, p0 + T)
    assert torch.equal(k8.u8[:, :, new], quant(k16[:, :, new])) and torch.equal(v8.u8[:, :, new], quant(v16[:, :, new]))
    assert torch.equal(A.bits(q8), A.bits(q16))  # q in place, in 16 bits; the k | v columns as they were
    k8.assert_untouched(new), v8.assert_untouched(new)


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("pos", [0, 15])
@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("kernel", ["mha", "gqa", "qkn"])
def test_decode_writer_bytes(kernel, B, pos, post):
    """Batch row 0 plants PLANT: h = 1 norms to exactly 1.0, weight rows ``value * e_0`` give the value itself
    in the V row, and in the K row at pos 0 (no rotation) without QK-norm; not under the post-norm."""
    nh, nkv, maxS, H = 4, (4 if kernel == "mha" else 2), 16, 256
    g = torch.Generator().manual_seed(B + pos)
    h, ln = torch.randn(B, H, generator=g), torch.ones(H, device=DEV)
    h[0] = 1.0
    h = h.to(DEV)
    prof = torch.tensor([600.0, 1.0, 2.0 ** -8, 30.0])[torch.arange(H + 2 * nkv * 64) % 4, None]
    wqkv = torch.randn(H + 2 * nkv * 64, H, generator=g) / 16 * prof  # saturating .. subnormal rows
    for r0 in (H, H + nkv * 64):
        wqkv[r0:r0 + 8] = 0.0
        wqkv[r0:r0 + 8, 0] = PLANT
    wqkv = wqkv.bfloat16().to(DEV)
    cos, sin = hip.rope_tables(64, maxS, device=DEV)
    posd = torch.tensor([pos], device=DEV)
    a, pnw = torch.randn(B, H, generator=g).bfloat16().to(DEV), (0.5 + torch.rand(H, generator=g)).to(DEV)
    qk = tuple((0.5 + torch.rand(64, generator=g)).to(DEV) for _ in range(2))

    def run(kc, vc):
        q, ho = torch.zeros(B, H, dtype=BF, device=DEV), torch.zeros(B, H, device=DEV)
        kw = {"post": (a, pnw, ho)} if post else {}
        if kernel == "mha":
            hip.dec_norm_qkv(h, ln, 1e-5, wqkv, cos, sin, posd, q, kc, vc, nh, **kw)
        elif kernel == "gqa":
            hip.dec_norm_qkv_gqa(h, ln, 1e-5, wqkv, cos, sin, posd, q, kc, vc, nh, nkv, **kw)
        else:
            hip.dec_norm_qkv_qkn(h, ln, 1e-5, wqkv, *qk, cos, sin, posd, q, kc, vc, nh, nkv, **kw)
        torch.cuda.synchronize()
        return q, ho

    k16, v16 = (torch.zeros(B, nkv, maxS, 64, dtype=BF, device=DEV) for _ in range(2))
    k8, v8 = Cache8((B, nkv, maxS, 64), 0x55, DEV), Cache8((B, nkv, maxS, 64), 0xAA, DEV)
    (q16, h16), (q8, h8) = run(k16, v16), run(k8.t, v8.t)
    row = slice(pos, pos + 1)
    if not post:  # the planted values did reach the 16-bit rows
        assert torch.equal(v16[0, 0, pos, :8].float().cpu(), PLANT)
        assert kernel == "qkn" or pos or torch.equal(k16[0, 0, pos, :8].float().cpu(), PLANT)
    assert torch.equal(k8.u8[:, :, row], quant(k16[:, :, row])) and torch.equal(v8.u8[:, :, row], quant(v16[:, :, row]))
    assert torch.equal(A.bits(q8), A.bits(q16)) and torch.equal(h8, h16)
    k8.assert_untouched(row), v8.assert_untouched(row)


MAXS = 80  # NS = 4: chunks of 20 keys (W = 33: of 9)
POS = (0, 3, 15, 16, 17, 19, 20, 63, 64, 79)  # the edges of a 16-key load, a 64-key trip and a chunk
FORMS = {"plain": {}, "win5": dict(W=5), "win33": dict(W=33), "sink": dict(sink=True), "cap": dict(cap=2.0),
         "all": dict(W=33, sink=True, cap=2.0)}


@functools.lru_cache(maxsize=None)
def _dec_inputs(nh, nkv, B=2):
    g = torch.Generator().manual_seed(10 * nh + nkv)
    q = torch.randn(B, nh * 64, generator=g).bfloat16()
    k8, v8 = (quant(torch.randn(B, nkv, MAXS, 64, generator=g).bfloat16()) for _ in range(2))
    return q, k8, v8, k8.view(FP8).bfloat16(), v8.view(FP8).bfloat16(), torch.tensor(C.DEC_SINKS[:nh])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nh,nkv,NS", [(3, 3, 0), (2, 2, 1), (6, 2, 1), (6, 2, 4), (2, 2, 4)])  # NS 0: dec_attn
def test_dec_attn_fp8_vs_fp64(nh, nkv, NS, form):
    """The 16-bit kernels' references and tolerances (decode_ref / sink_ref / attn_cap_ref), dequantised cache."""
    W, cap = FORMS[form].get("W"), FORMS[form].get("cap")
    q, k8, v8, kd, vd, sinks = _dec_inputs(nh, nkv)
    sink = sinks if FORMS[form].get("sink") else None
    kw = dict(window=W or 0, sink=None if sink is None else sink.to(DEV), softcap=cap)
    ws = hip.dec_attn_gqa_workspace(2, nh, NS, DEV) if NS > 1 else None
    for pos in POS:
        if cap is not None:
            chk = C.dec_cap_ref(q, kd, vd, pos, SCALE, nh, cap, W, sink)
        elif sink is not None:
            chk = S.dec_sink_ref(q, kd, vd, pos, SCALE, nh, sink, W)
        else:
            chk = WN.attn_gqa_win_ref(q, kd, vd, pos, SCALE, nh, W)
        kc, vc = (Cache8((2, nkv, MAXS, 64), 0x33, DEV, init=t.to(DEV)) for t in (k8, v8))
        kc.u8[:, :, pos + 1:], vc.u8[:, :, pos + 1:] = NAN_BYTE, NAN_BYTE
        o = A.Guarded((2, nh * 64), BF, -777.0, DEV)
        posd = torch.tensor([pos], device=DEV)
        if NS == 0:
            hip.dec_attn(q.to(DEV), kc.t, vc.t, posd, o.t, SCALE, **kw)
        else:
            hip.dec_attn_gqa(q.to(DEV), kc.t, vc.t, posd, o.t, SCALE, nh, splits=NS, ws=ws, **kw)
        torch.cuda.synchronize()
        o.assert_guards()
        check(f"o[pos {pos}]", o.t, chk.ref, chk.tol)


MODELS = {"mha": {}, "gqa": dict(num_kv_heads=2), "norms": dict(qk_norm=True, post_norm=True)}


@functools.lru_cache(maxsize=None)
def _model(name):
    torch.manual_seed(21)
    m = GPT(GPTConfig(vocab_size=1000, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4,
                      max_seq_len=128, dropout=0.0, attention_dropout=0.0, **MODELS[name])).to(DEV)
    m.enable_engine()
    return m.eval()


@pytest.mark.parametrize("name", MODELS)
def test_step_on_fp8_cache_matches_the_16_bit_step_on_its_values(name):
    """One captured step on a prompt's quantised cache and on its dequantised 16-bit copy: logits within the
    fused-vs-ATen 3e-2 of test_decode_gqa_gpu.py; layer 0's new rows (same inputs) bit for bit, deeper ones
    (inputs differ by that rounding) within test_prefill_gpu.py's row tolerance plus e4m3's half step 2^-4."""
    m = _model(name)
    ids = torch.randint(0, 1000, (2, 41), generator=torch.Generator().manual_seed(60)).to(DEV)
    c8, c16 = KVCache(m.config, 2, DEV, BF, kv_dtype=FP8), KVCache(m.config, 2, DEV, BF)
    with pytest.raises(NotImplementedError):
        forward_cached(m, ids[:, :40], c8)
    forward_cached(m, ids[:, :40], c16)
    for x8, x16 in zip(c8.k + c8.v, c16.k + c16.v):
        x8.view(torch.uint8).copy_(quant(x16))
        x16.copy_(x8.to(BF))
    c8.len = 40
    g8, g16 = DecodeGraph(m, c8, 40)(ids[:, 40:]).clone(), DecodeGraph(m, c16, 40)(ids[:, 40:]).clone()
    assert torch.allclose(g8, g16, atol=3e-2, rtol=3e-2), (g8 - g16).abs().max().item()
    for i, (x8, x16) in enumerate(zip(c8.k + c8.v, c16.k + c16.v)):
        if i % m.config.num_layers == 0:
            assert torch.equal(x8.view(torch.uint8)[:, :, 40], quant(x16[:, :, 40]))
        assert torch.allclose(x8[:, :, 40].float(), x16[:, :, 40].float(), atol=2e-2, rtol=2e-2 + 2.0 ** -4)
        assert torch.equal(x8[:, :, :40].to(BF), x16[:, :, :40])  # no earlier row moved


@pytest.mark.parametrize("name", MODELS)
def test_generate_gives_the_recorded_ids(name):
    """The default path is untouched: the ids the commit before the FP8 cache gave, recorded on an MI355X."""
    ids = torch.randint(0, 1000, (2, 9), generator=torch.Generator().manual_seed(3)).to(DEV)
    torch.manual_seed(5)
    golden = os.path.join(os.path.dirname(__file__), "golden", "kv_fp8_auto_ids.json")
    assert _model(name).generate(ids, max_new_tokens=12).tolist() == json.load(open(golden))[name]
