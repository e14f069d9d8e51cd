"""Document-masked flash attention on the MI355X (DOC instantiations of attention.hip):
forward, dQ and dK/dV against the dense-mask reference ops, bitwise properties (repeat
calls, stored vs regenerated keep bits, packed vs head-major layout, trivial bounds vs no
mask, isolation between documents), the zero-padded route, the routes that refuse the
mask, and the engine end to end.

Shapes (B = 2, nh = 2; batch row 0 carries the separators, row 1 has none):
  S = 192, separators {36, 63, 127}: a boundary inside a 32-query half, on a tile edge
      minus one, and on a tile edge;
  S = 200, separators {0, 1, 2, 150}: one-token documents (a query sees only itself) and
      a ragged last tile;
  S = 320, separators {69, 250}: in the item of queries 192..255 the queries 251..255
      start a new document, so key tiles 1 and 2 are fully masked for those rows while
      the item still reads them -- the rows whose running max has seen no live key yet.
Tolerances are those of tests/test_kernels_gpu.py (same per-element arithmetic)."""
import copy
import functools

import pytest
import torch

from distributed_llm_trainer_amd import ops
from distributed_llm_trainer_amd.models import GPT, GPTConfig
from distributed_llm_trainer_amd.ops import attn_gemm, hip, reference as ref, rng
from tests.test_lmhead_loss_gpu import EPS, FACTOR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEP = 3
B, NH = 2, 2
SHAPES = {192: (36, 63, 127), 200: (0, 1, 2, 150), 320: (69, 250)}
CASES = [(S, hd, p) for S in SHAPES for hd in (64, 128) for p in (0.0, 0.1)]
KEY = rng.site_key(2, 4, 1, rng.SITE_ATTN)


def _close(a, b, atol, rtol=0.0, what=""):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    bad = (err > lim).sum().item()
    assert bad == 0, f"{what}: {bad} elements out of tolerance, max err {err.max().item():.3e}"


def _ids(S, seps):
    g = torch.Generator().manual_seed(S)
    ids = torch.randint(SEP + 1, 500, (B, S), generator=g)
    for j in seps:
        ids[0, j] = SEP
    return ids.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(S, hd, p):
    """Inputs, bounds and the reference results of one case, computed once and shared
    (read-only) by the tests below."""
    g = torch.Generator().manual_seed(1000 * S + hd)
    q, k, v = (torch.randn(B, NH, S, hd, generator=g).bfloat16().to(DEV) for _ in range(3))
    do = torch.randn(B * S, NH * hd, generator=g).bfloat16().to(DEV)
    doc = hip.doc_bounds(_ids(S, SHAPES[S]), SEP)
    o_ref, lse_ref = ref.attention_fwd(q, k, v, p, KEY, doc=doc)
    grads_ref = ref.attention_bwd(q, k, v, o_ref, do, lse_ref, p, KEY, doc=doc)
    return dict(q=q, k=k, v=v, do=do, doc=doc, o_ref=o_ref, lse_ref=lse_ref, grads_ref=grads_ref)


def test_bounds_on_device_match_the_reference():
    for S, seps in SHAPES.items():
        ids = _ids(S, seps)
        lo, hi = hip.doc_bounds(ids, SEP)
        lo2, hi2 = ref.doc_bounds(ids.cpu(), SEP)
        assert lo.is_cuda and lo.dtype == torch.int32 and lo.is_contiguous()
        assert torch.equal(lo.cpu(), lo2) and torch.equal(hi.cpu(), hi2)


# ------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("S,hd,p", CASES)
def test_doc_attention_fwd(S, hd, p):
    c = _case(S, hd, p)
    o, aux = hip.attention_fwd(c["q"], c["k"], c["v"], p, KEY, doc=c["doc"])
    lse = aux[0]
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    _close(lse, c["lse_ref"], 2e-3, 1e-4, "lse")
    _close(o, c["o_ref"].float(), 2e-2, 2e-2, "o")
    if p > 0:  # the stored keep bits are still the hash, in both layouts
        keep = rng.attn_keep_mask(B * NH, S, S, KEY, p, device=DEV)
        W = (S + 31) // 32
        causal = torch.tril(torch.ones(S, S, dtype=torch.bool, device=DEV))
        idx = torch.arange(S, device=DEV)
        bits = aux[1][0].view(B * NH, W, S).transpose(1, 2)
        got = ((bits[:, :, idx // 32].long() >> (idx % 32)) & 1).bool()
        assert torch.equal(got & causal, keep & causal), "stored dropout bitmask differs from the hash"
        bits_t = aux[1][1].view(B * NH, W, S).transpose(1, 2)
        got_t = ((bits_t[:, :, idx // 32].long() >> (idx % 32)) & 1).bool()
        assert torch.equal(got_t.transpose(1, 2) & causal, keep & causal), "transposed bitmask differs"


# ------------------------------------------------------------------ 2. backward
@pytest.mark.parametrize("S,hd,p", CASES)
def test_doc_attention_bwd(S, hd, p):
    c = _case(S, hd, p)
    q, k, v, do, doc = c["q"], c["k"], c["v"], c["do"], c["doc"]
    o, lse = c["o_ref"], c["lse_ref"]
    g1 = hip.attention_bwd(q, k, v, o, do, lse, p, KEY, doc=doc)  # regenerates the keep bits
    g2 = hip.attention_bwd(q, k, v, o, do, lse, p, KEY, doc=doc)
    _, aux = hip.attention_fwd(q, k, v, p, KEY, doc=doc)
    g3 = hip.attention_bwd(q, k, v, o, do, (lse, aux[1]), p, KEY, doc=doc)  # stored keep bits
    for a, b2, b3, r, n in zip(g1, g2, g3, c["grads_ref"], ("dq", "dk", "dv")):
        assert torch.isfinite(a.float()).all(), n
        assert torch.equal(a, b2), f"{n}: two calls differ"
        assert torch.equal(a, b3), f"{n}: stored-mask and regenerated-mask variants differ"
        scale = r.float().abs().max().item()
        _close(a, r.float(), 2e-2 * max(1.0, scale), 2e-2, n)


# ------------------------------------------------------------------ 3. packed layout
@pytest.mark.parametrize("S,hd,p", CASES)
def test_doc_attention_packed(S, hd, p):
    torch.manual_seed(32 + S)
    H = NH * hd
    raw = torch.randn(B * S, 3 * H, device=DEV).bfloat16()
    do = _case(S, hd, p)["do"]
    doc = _case(S, hd, p)["doc"]
    cos, sin = hip.rope_tables(hd, 1024, device=DEV)
    q, k, v = hip.rope_qkv_fwd(raw, B, S, NH, cos, sin)
    o1, aux1 = hip.attention_fwd(q, k, v, p, KEY, doc=doc)
    packed = hip.rope_qk_inplace(raw.clone(), B, S, NH, cos, sin)
    o2, aux2 = hip.attention_fwd_packed(packed, B, S, NH, p, KEY, doc=doc)
    assert torch.equal(o1, o2) and torch.equal(aux1[0], aux2[0])
    dq, dk, dv = hip.attention_bwd(q, k, v, o1, do, aux1, p, KEY, doc=doc)
    got = hip.attention_bwd_packed(packed, o2, do, aux2, p, KEY, B, S, NH, cos, sin, doc=doc)
    assert torch.equal(dv.transpose(1, 2).reshape(B * S, H), got[:, 2 * H:])
    want = ref.rope_qkv_bwd(dq.float(), dk.float(), dv.float(), cos, sin)
    scale = want.abs().max().item()
    _close(got, want, 1e-2 * max(1.0, scale), 1e-2, "dqkv packed")
    # against the fp32 reference of the whole chain
    want2 = ref.attention_bwd_packed(packed.float(), o2.float(), do.float(), aux2[0], p, KEY, B, S, NH, cos, sin,
                                     doc=doc)
    _close(got, want2, 2e-2 * max(1.0, scale), 2e-2, "dqkv packed vs fp32 ref")


# ------------------------------------------------------------------ 4. trivial bounds
@pytest.mark.parametrize("S,hd,p", CASES)
def test_trivial_bounds_equal_no_mask_bitwise(S, hd, p):
    c = _case(S, hd, p)
    q, k, v, do = c["q"], c["k"], c["v"], c["do"]
    doc = hip.doc_bounds(_ids(S, ()), SEP)  # no separator: lo = 0, hi = S - 1
    assert int(doc[0].max()) == 0 and int(doc[1].min()) == S - 1
    o1, aux1 = hip.attention_fwd(q, k, v, p, KEY, doc=doc)
    o0, aux0 = hip.attention_fwd(q, k, v, p, KEY)
    assert torch.equal(o1, o0) and torch.equal(aux1[0], aux0[0])
    g1 = hip.attention_bwd(q, k, v, o0, do, aux0, p, KEY, doc=doc)
    g0 = hip.attention_bwd(q, k, v, o0, do, aux0, p, KEY)
    for a, b, n in zip(g1, g0, ("dq", "dk", "dv")):
        assert torch.equal(a, b), n


# ------------------------------------------------------------------ 5. isolation
@pytest.mark.parametrize("S,hd,p", CASES)
def test_later_documents_do_not_see_the_first(S, hd, p):
    c = _case(S, hd, p)
    doc = c["doc"]
    first = SHAPES[S][0] + 1  # rows [0, first) of batch row 0 are the first document
    H = NH * hd

    def run(q, k, v, do):
        o, aux = hip.attention_fwd(q, k, v, p, KEY, doc=doc)
        return (o.view(B, S, H), aux[0]) + tuple(hip.attention_bwd(q, k, v, o, do, aux, p, KEY, doc=doc))

    base = run(c["q"], c["k"], c["v"], c["do"])
    g = torch.Generator().manual_seed(7)
    q2, k2, v2 = (t.clone() for t in (c["q"], c["k"], c["v"]))
    do2 = c["do"].clone().view(B, S, H)
    for t in (q2, k2, v2):
        t[0, :, :first] = (3.0 * torch.randn(NH, first, hd, generator=g)).bfloat16().to(DEV)
    do2[0, :first] = torch.randn(first, H, generator=g).bfloat16().to(DEV)
    edit = run(q2, k2, v2, do2.view(B * S, H))
    o_a, lse_a, o_b, lse_b = base[0], base[1], edit[0], edit[1]
    assert torch.equal(o_a[0, first:], o_b[0, first:]) and torch.equal(o_a[1], o_b[1]), "o"
    assert torch.equal(lse_a[0, :, first:], lse_b[0, :, first:]) and torch.equal(lse_a[1], lse_b[1]), "lse"
    assert not torch.equal(o_a[0, :first], o_b[0, :first])
    for a, b, n in zip(base[2:], edit[2:], ("dq", "dk", "dv")):
        assert torch.equal(a[0, :, first:], b[0, :, first:]) and torch.equal(a[1], b[1]), n
    # the same edit without the mask reaches the later rows
    o_c, _ = hip.attention_fwd(c["q"], c["k"], c["v"], p, KEY)
    o_d, _ = hip.attention_fwd(q2, k2, v2, p, KEY)
    assert not torch.equal(o_c.view(B, S, H)[0, first:], o_d.view(B, S, H)[0, first:])


# ------------------------------------------------------------------ 6. other routes
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_padded_head_passes_the_bounds_through(p):
    S, hd = 320, 96
    g = torch.Generator().manual_seed(96)
    q, k, v = (torch.randn(B, NH, S, hd, generator=g).bfloat16().to(DEV) for _ in range(3))
    do = torch.randn(B * S, NH * hd, generator=g).bfloat16().to(DEV)
    doc = hip.doc_bounds(_ids(S, SHAPES[S]), SEP)
    assert attn_gemm.pad_dim(torch.bfloat16, hd) == 128
    o, aux = attn_gemm.attention_fwd(q, k, v, p, KEY, doc=doc)
    o_ref, lse_ref = ref.attention_fwd(q, k, v, p, KEY, doc=doc)
    _close(aux[0], lse_ref, 2e-3, 1e-4, "lse")
    _close(o, o_ref.float(), 2e-2, 2e-2, "o")
    grads = attn_gemm.attention_bwd(q, k, v, o_ref, do, (lse_ref, aux[1]), p, KEY, doc=doc)
    for a, r, n in zip(grads, ref.attention_bwd(q, k, v, o_ref, do, lse_ref, p, KEY, doc=doc), ("dq", "dk", "dv")):
        scale = r.float().abs().max().item()
        _close(a, r.float(), 2e-2 * max(1.0, scale), 2e-2, n)


def test_routes_without_the_mask_raise():
    S = 64
    doc = hip.doc_bounds(_ids(S, (10,)), SEP)
    q160 = torch.randn(B, NH, S, 160, device=DEV).bfloat16()
    o160 = torch.randn(B * S, NH * 160, device=DEV).bfloat16()
    lse = torch.zeros(B, NH, S, device=DEV)
    with pytest.raises(NotImplementedError, match="GEMM-formulated"):
        attn_gemm.attention_fwd(q160, q160, q160, 0.0, KEY, doc=doc)
    with pytest.raises(NotImplementedError, match="GEMM-formulated"):
        attn_gemm.attention_bwd(q160, q160, q160, o160, o160, lse, 0.0, KEY, doc=doc)
    q32 = torch.randn(B, NH, S, 64, device=DEV)
    o32 = torch.randn(B * S, NH * 64, device=DEV)
    with pytest.raises(NotImplementedError, match="fp32"):
        hip.attention_fwd(q32, q32, q32, 0.0, KEY, doc=doc)
    with pytest.raises(NotImplementedError, match="fp32"):
        hip.attention_bwd(q32, q32, q32, o32, o32, lse, 0.0, KEY, doc=doc)
    qkv32 = torch.randn(B * S, 3 * NH * 64, device=DEV)
    with pytest.raises(NotImplementedError, match="fp32"):
        hip.attention_fwd_packed(qkv32, B, S, NH, 0.0, KEY, doc=doc)
    # the engine refuses when the separator is set, before any step
    wide = GPT(GPTConfig(vocab_size=512, hidden_size=320, num_layers=1, num_heads=2, max_seq_len=64)).to(DEV)
    with pytest.warns(UserWarning):
        wide.enable_engine()
    with pytest.raises(NotImplementedError, match="GEMM-formulated"):
        wide.set_doc_separator(SEP)
    assert wide.doc_sep_token is None and wide.engine.doc_sep_token is None
    f32 = GPT(GPTConfig(vocab_size=512, hidden_size=128, num_layers=1, num_heads=2, max_seq_len=64)).to(DEV)
    f32.set_doc_separator(SEP)
    with pytest.raises(NotImplementedError, match="fp32"):
        f32.enable_engine(act_dtype=torch.float32)


def test_doc_argument_is_validated_on_the_host():
    c = _case(192, 64, 0.0)
    q, k, v = c["q"], c["k"], c["v"]
    lo, hi = c["doc"]
    with pytest.raises(TypeError):
        hip.attention_fwd(q, k, v, 0.0, KEY, doc=(lo.long(), hi.long()))
    with pytest.raises(ValueError):
        hip.attention_fwd(q, k, v, 0.0, KEY, doc=(lo[:, :100].contiguous(), hi[:, :100].contiguous()))
    with pytest.raises(ValueError):
        hip.attention_fwd(q, k, v, 0.0, KEY, doc=(lo.cpu(), hi.cpu()))
    with pytest.raises(ValueError):
        hip.attention_fwd(q, k, v, 0.0, KEY, doc=(lo.t().contiguous().t(), hi))  # [B, S] but not contiguous


# ------------------------------------------------------------------ 7. engine
def _engine_cfg():
    return GPTConfig(vocab_size=512, hidden_size=128, num_layers=2, num_heads=2, max_seq_len=256, dropout=0.1,
                     attention_dropout=0.1)


def _engine_ids(seed):
    """B = 2, S = 256; row 0: separators at 55 and 200 (the S = 320 case scaled): in the
    item of queries 192..255 the queries 201..255 have key tiles 1 and 2 fully masked."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(SEP + 1, 512, (2, 256), generator=g)
    ids[0, 55] = SEP
    ids[0, 200] = SEP
    return ids.to(DEV)


def _grads(m):
    return {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()


@functools.lru_cache(maxsize=None)
def _engine_base():
    torch.manual_seed(0)
    return GPT(_engine_cfg()).to(DEV)


def _step(recompute=False, selective=True, ops_ns=None, sep=SEP):
    m = copy.deepcopy(_engine_base())
    m.set_doc_separator(sep)
    eng = m.enable_engine(seed=5, **({"ops": ops_ns} if ops_ns is not None else {}))
    eng.selective_recompute = selective
    m.gradient_checkpointing = recompute
    ids = _engine_ids(1)
    _, loss = m(ids, labels=ids)
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), _grads(m), m


def test_engine_hip_vs_reference_ops_with_separator():
    l1, g1, _ = _step()
    l2, g2, _ = _step(ops_ns=ops.CPU_OPS)  # reference ops on the GPU: same weights, same masks
    assert abs(l1 - l2) < 2e-2 * abs(l2)
    for n in g1:
        assert torch.isfinite(g1[n]).all(), n
        assert _cos(g1[n], g2[n]) > 0.99, n
        r = g1[n].norm() / g2[n].norm()
        assert 0.95 < r.item() < 1.05, (n, r.item())
    l0, _, _ = _step(sep=None)
    assert l0 != l1, "the mask must change the loss"


@pytest.mark.parametrize("selective", [True, False])
def test_engine_recompute_is_bitwise_with_separator(selective):
    l1, g1, _ = _step(recompute=False)
    l2, g2, _ = _step(recompute=True, selective=selective)
    assert l1 == l2
    for n in g1:
        assert torch.equal(g1[n], g2[n]), (n, (g1[n] - g2[n]).abs().max().item())


@pytest.mark.parametrize("recompute", [False, True])
def test_engine_window_matches_sequential_with_separator(recompute):
    from distributed_llm_trainer_amd.models.engine import shift_targets
    GA = 2
    m1, m2 = copy.deepcopy(_engine_base()), copy.deepcopy(_engine_base())
    for m in (m1, m2):
        m.set_doc_separator(SEP)
    e1, e2 = m1.enable_engine(seed=9), m2.enable_engine(seed=9)
    m1.gradient_checkpointing = m2.gradient_checkpointing = recompute
    data = [_engine_ids(10 + j) for j in range(GA)]
    seq = []
    for j in range(GA):
        e1.set_accumulation(j, GA, defer=True)
        _, loss = m1(data[j], labels=data[j])
        (loss / GA).backward()
        seq.append(loss.item())
    win = e2.train_window(data, [shift_targets(d) for d in data], torch.full((), 1.0 / GA, device=DEV),
                          recompute=recompute)
    torch.cuda.synchronize()
    for a, b in zip(seq, win):
        assert a == b.item(), (seq, [w.item() for w in win])
    g1, g2 = _grads(m1), _grads(m2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), (n, (g1[n] - g2[n]).abs().max().item())


def test_engine_eval_loss_matches_forward_with_labels():
    m = copy.deepcopy(_engine_base())
    m.enable_engine(seed=1)
    m.set_doc_separator(SEP)
    ids = _engine_ids(2)
    m.eval()
    with torch.no_grad():
        logits, want = m(ids, labels=ids)  # the unfused head, logits returned
    # both run the same masked layers and differ in the head only: the bound of
    # tests/test_eval_gpu.py (mean over the predicted rows of 2^-7 * max_j |logit|, + EPS)
    bound = FACTOR[torch.bfloat16] * logits[:, :-1].float().abs().amax(dim=-1).mean().item() + EPS
    got = m.eval_loss(ids)
    print(f"eval_loss {got.item():.6f} forward {want.item():.6f} bound {bound:.3e}")
    assert abs(got.item() - want.item()) <= bound
    m.set_doc_separator(None)
    assert m.eval_loss(ids).item() != got.item(), "eval_loss must apply the mask"
