"""Every launch variant of the flash-attention kernels (ops/csrc/attention.hip) against the fp64
references and derived tolerances of tests/attn_ref.py: every element of o, lse, both keep-bit
layouts, dq, dk, dv and the delta workspace, at the smallest shapes that reach each path, with
sentinel guards around every output.

Packed cases go through ops/hip.py's packed wrappers (o and dqkv in guarded ``out=`` buffers);
head-major cases fill ``_AttnArgs`` directly, so that lse, dq, dk, dv and delta sit in guarded
buffers too.  The backward is given the forward REFERENCE's o and lse, rounded to their storage
formats: fixed inputs, the same ones the CPU file uses.

Each check prints ``RATIO <output> <worst err / tol>`` (and ``BIAS`` on the gauss family);
``pytest -s`` shows them.  The checks are plain functions so that tests/attn_ref_child.py can run
them in a fresh process under the other work schedules (read once per process)."""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import pytest
import torch

from distributed_llm_trainer_amd.ops import hip, rng
from distributed_llm_trainer_amd.ops.reference import WindowBounds
from tests import attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, I32 = torch.float32, torch.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = {R.BF: 3.0, R.HF: 3.0, F32: -7.5, I32: 0x5A5A5A5A}
SCHED = R.sched_of(os.environ)


def check(name, out, chk, bias=False):
    ref, tol = chk.ref.to(out.device), chk.tol.to(out.device)
    err = (out.double().reshape(ref.shape) - ref).abs()
    ratio = torch.where(tol > 0, err / tol, err).max().item()
    print(f"RATIO {name} {ratio:.4f}")
    bad = ~(err <= tol)
    assert not bad.any(), (f"{name}: {bad.sum().item()} of {bad.numel()} elements outside the tolerance, "
                           f"worst err/tol {ratio:.3f} at {bad.nonzero()[0].tolist()}")
    if bias:
        b = R.bias_ratio(out.cpu(), chk)
        print(f"BIAS {name} {b:.4f}")
        assert b < 1.0, f"{name}: the errors lean one way ({b:.2f} of the bound): something truncates"
    return ratio


def _d(t):
    return None if t is None else t.to(DEV)


# -------------------------------------------------------------------------------- keep bits
def keep_words(BH, S, key, p):
    """(mask [BH, W, S], maskT [BH, W, S]) as k_dropout_bits defines them: word w of query q holds
    keep(q, 32 w + j) at bit j; word r of key k holds keep(32 r + j, k); zero past S."""
    W = (S + 31) // 32
    keep = rng.attn_keep_mask(BH, S, S, key, p).long()
    pad = W * 32 - S
    wts = (1 << torch.arange(32, dtype=torch.int64))
    kq = torch.nn.functional.pad(keep, (0, pad)).view(BH, S, W, 32)
    mask = (kq * wts).sum(-1).transpose(1, 2)                                  # [BH, W(w), S(q)]
    kk = torch.nn.functional.pad(keep, (0, 0, 0, pad)).view(BH, W, 32, S)
    maskT = (kk * wts.view(32, 1)).sum(2)                                      # [BH, W(r), S(k)]
    wrap = lambda t: torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(I32)
    return wrap(mask), wrap(maskT)


def tiles_written(S, window=None):
    """bool [W(r), W(w)]: the 32x32 bit tiles k_dropout_bits writes (band r = query / 32, word w)."""
    W = (S + 31) // 32
    r, w = torch.arange(W).view(W, 1), torch.arange(W).view(1, W)
    full = w <= r
    if R.mask_variant(S, window).startswith("k_dropout_bits<BAND=0>"):
        return full
    D = min((window - 1 + 63) // 64, W)
    return full & (r - w <= 2 * D + 1) & ((r >> 1) - (w >> 1) <= D)


def check_keep_bits(tag, M, B, nh, S, key, p, window=None):
    """Bit for bit inside the tiles the kernel writes; the sentinel everywhere else and in the guards."""
    BH, W = B * nh, (S + 31) // 32
    want, wantT = keep_words(BH, S, key, p)
    tw = tiles_written(S, window)
    band = torch.arange(S) // 32
    wr = tw[band].t().unsqueeze(0).expand(BH, W, S)       # mask [bh, w, q]: tile (q / 32, w)
    wrT = tw[:, band].unsqueeze(0).expand(BH, W, S)       # maskT [bh, r, k]: tile (r, k / 32)
    written = torch.stack([wr, wrT]).to(DEV)
    M.assert_guards(written=written)
    got = M.t.cpu()
    for nm, g, w_, wm in (("mask", got[0], want, wr), ("maskT", got[1], wantT, wrT)):
        diff = ((g != w_) & wm).nonzero()
        assert diff.numel() == 0, f"{tag} {nm}: {diff.shape[0]} words differ, first at [bh, word, pos] = {diff[0].tolist()}"
    print(f"RATIO {tag} keep-bits[{R.mask_variant(S, window)}] 0.0000")


# ------------------------------------------------------------------------------ one case
OUTPUTS = {}  # case -> {output: CPU tensor} of the first run in this process
TIMES = {}
CHILD_START = 60.0  # interpreter start, torch import, library load, first HIP call of a fresh process


def _args(**kw):
    strides = kw.pop("strides")
    return hip._AttnArgs(**{k: (hip._p(v) if isinstance(v, torch.Tensor) else v) for k, v in kw.items() if v is not None},
                         stride=hip._AttnStrides(**strides))


def _run_direct(c, inp, o16, lse32, doc, window):
    """Head-major: dlt_attn_fwd / dlt_attn_bwd on a hand-filled _AttnArgs, every output guarded."""
    B, nh, S, hd, dt = c.B, c.nh, c.S, c.hd, c.dtype
    q, k, v, do = _d(inp.q), _d(inp.k), _d(inp.v), _d(inp.do)
    thr = rng.keep_threshold(c.p)
    dscale = 1.0 / (1.0 - c.p) if thr else 1.0
    O = R.Guarded((B * S, nh * hd), dt, SENT[dt], DEV)
    L = R.Guarded((B, nh, S), F32, SENT[F32], DEV)
    M = R.Guarded((2, B * nh, (S + 31) // 32, S), I32, SENT[I32], DEV) if thr else None
    gen = 1
    if thr and window is not None:  # the banded bits come from their own entry point
        hip.attention_dropout_mask(B, nh, S, c.p, c.key, window=window, out=M.t)
        gen = 0
    _, sq, skv = hip._head_major(q, k, v)
    st = dict(q=sq, kv=skv, dq=sq, dkv=skv)
    common = dict(q=q, k=k, v=v, lo=doc[0] if doc else None, B=B, nh=nh, nkv=c.nkv, S=S, hd=hd, hk=int(dt == R.HF),
                  scale=inp.scale, dscale=dscale, key=c.key, thr=thr, mask=M.t if M else None)
    L_, stream = hip.lib(), hip._stream()
    assert L_.dlt_attn_fwd(ctypes.byref(_args(o=O.t, lse=L.t, gen_mask=gen, strides=st, **common)), stream) == 0
    DQ = R.Guarded(tuple(inp.q.shape), dt, SENT[dt], DEV)
    DK, DV = (R.Guarded(tuple(inp.k.shape), dt, SENT[dt], DEV) for _ in range(2))
    DL = R.Guarded((B, nh, S), F32, SENT[F32], DEV)
    assert L_.dlt_attn_bwd(ctypes.byref(_args(o=_d(o16), lse=_d(lse32), dout=do, delta_ws=DL.t, dq=DQ.t, dk=DK.t, dv=DV.t,
                                              hi=doc[1] if doc else None, strides=st, **common)), stream) == 0
    torch.cuda.synchronize()
    for g in (O, L, DQ, DK, DV, DL):
        g.assert_guards()
    return dict(o=O.t, lse=L.t, dq=DQ.t, dk=DK.t, dv=DV.t, delta=DL.t), M


def _run_packed(c, inp, o16, lse32, doc, window):
    """Packed QKV through attention_fwd_packed / attention_bwd_packed with guarded ``out=`` buffers."""
    B, nh, S, hd, dt, kvh = c.B, c.nh, c.S, c.hd, c.dtype, c.kvh
    H, KV = nh * hd, kvh * hd
    qkv = _d(R.pack_qkv(inp))
    thr = rng.keep_threshold(c.p)
    O = R.Guarded((B * S, H), dt, SENT[dt], DEV)
    M = R.Guarded((2, B * nh, (S + 31) // 32, S), I32, SENT[I32], DEV) if thr else None
    if thr:  # made ahead, as the engine does: the forward then runs with gen_mask = 0
        hip.attention_dropout_mask(B, nh, S, c.p, c.key, window=window, out=M.t)
    kw = dict(doc=doc, nkv=c.nkv or None, window=window)
    o, aux = hip.attention_fwd_packed(qkv, B, S, nh, c.p, c.key, out=O.t, mask=M.t if M else None, **kw)
    G = R.Guarded((B * S, H + 2 * KV), dt, SENT[dt], DEV)
    cos, sin = _d(inp.rope[0]), _d(inp.rope[1])
    hip.attention_bwd_packed(qkv, _d(o16), _d(inp.do), hip.AttnAux((_d(lse32), M.t if M else None)), c.p, c.key, B, S, nh,
                             cos, sin, out=G.t, **kw)
    torch.cuda.synchronize()
    O.assert_guards()
    G.assert_guards()
    hm = lambda t, h: t.view(B, S, h, hd).transpose(1, 2)
    return dict(o=O.t, lse=aux[0], dq=hm(G.t[:, :H], nh), dk=hm(G.t[:, H:H + KV], kvh), dv=hm(G.t[:, H + KV:], kvh)), M


def check_case(name):
    c = R.BY_NAME[name]
    inp, fwd, o16, lse32, bwd = R.case_refs(c)
    window = R.case_window(c)
    doc = None
    if inp.doc is not None:
        lo, hi = _d(inp.doc[0]), _d(inp.doc[1])
        doc = WindowBounds(lo, hi, window) if window is not None else (lo, hi)
    run = _run_packed if c.packed else _run_direct
    outs, M = run(c, inp, o16, lse32, doc, window)
    tag = f"[{SCHED}] {name}"
    for v in R.case_variants(c):
        print(f"LAUNCH {v}")
    if M is not None:
        check_keep_bits(tag, M, c.B, c.nh, c.S, c.key, c.p, window)
    gauss = c.family == "gauss" and c.S >= 64
    check(tag + " o", outs["o"], fwd.o, bias=gauss)
    check(tag + " lse", outs["lse"], fwd.lse)
    for nm in ("dq", "dk", "dv"):
        check(f"{tag} {nm}", outs[nm], getattr(bwd, nm), bias=gauss)
    if "delta" in outs:
        check(tag + " delta", outs["delta"], bwd.delta)
    again, M2 = run(c, inp, o16, lse32, doc, window)
    for nm, t in outs.items():
        assert torch.equal(R.bits(t.contiguous()), R.bits(again[nm].contiguous())), f"{tag} {nm}: two calls on equal inputs differ"
    if M is not None:
        assert torch.equal(M.t, M2.t), f"{tag}: keep bits of two calls differ"
    OUTPUTS.setdefault(name, {nm: t.detach().contiguous().cpu() for nm, t in outs.items()})


def run_check(name):
    t0 = time.perf_counter()
    check_case(name)
    TIMES.setdefault(name, time.perf_counter() - t0)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_attention_case(name):
    run_check(name)


@pytest.mark.parametrize("name", [c.name for c in R.CASES if rng.keep_threshold(c.p) and not c.packed][:6])
def test_gen_mask_0_and_1_give_the_same_bits(name):
    """The forward's own keep bits (gen_mask = 1) are those of dlt_attn_dropout_mask (gen_mask = 0,
    the full triangle), and o / lse do not depend on who made them."""
    c = R.BY_NAME[name]
    inp = R.attn_inputs(c)
    B, nh, S, hd, dt = c.B, c.nh, c.S, c.hd, c.dtype
    q, k, v = _d(inp.q), _d(inp.k), _d(inp.v)
    lo = _d(inp.doc[0]) if inp.doc else None
    _, sq, skv = hip._head_major(q, k, v)
    res = []
    for gen in (1, 0):
        O = R.Guarded((B * S, nh * hd), dt, SENT[dt], DEV)
        L = R.Guarded((B, nh, S), F32, SENT[F32], DEV)
        M = R.Guarded((2, B * nh, (S + 31) // 32, S), I32, SENT[I32], DEV)
        if gen == 0:
            hip.attention_dropout_mask(B, nh, S, c.p, c.key, out=M.t)
        a = _args(q=q, k=k, v=v, o=O.t, lse=L.t, mask=M.t, lo=lo, B=B, nh=nh, nkv=c.nkv, S=S, hd=hd, hk=int(dt == R.HF),
                  scale=inp.scale, dscale=1.0 / (1.0 - c.p), key=c.key, thr=rng.keep_threshold(c.p), gen_mask=gen,
                  strides=dict(q=sq, kv=skv))
        assert hip.lib().dlt_attn_fwd(ctypes.byref(a), hip._stream()) == 0
        torch.cuda.synchronize()
        check_keep_bits(f"gen_mask={gen} {name}", M, B, nh, S, c.key, c.p)
        O.assert_guards()
        L.assert_guards()
        res.append((M.t, O.t, L.t))
    for x, y in zip(*res):
        assert torch.equal(R.bits(x), R.bits(y))


@pytest.mark.parametrize("S,window", [(320, 65), (200, 31), (96, 1), (96, 65), (129, 64)])
def test_banded_keep_bits_write_nothing_outside_the_band(S, window):
    B, nh, p, key = 1, 3, 0.1, 0x1234567
    M = R.Guarded((2, B * nh, (S + 31) // 32, S), I32, SENT[I32], DEV)
    hip.attention_dropout_mask(B, nh, S, p, key, window=window, out=M.t)
    torch.cuda.synchronize()
    check_keep_bits(f"band S={S} W={window}", M, B, nh, S, key, p, window)


# --------------------------------------------------------------- the other two schedules
def test_this_process_runs_the_default_schedule():
    assert SCHED == "lpt", "DLT_ATTN_SCHED is set: the cases above ran under it, the children compare against it"


def test_other_schedules_in_children():
    """DLT_ATTN_SCHED=pair with the XCD map and with the natural order, each in a fresh process
    (the launchers read the environment once): the same checks, and outputs bitwise equal to the
    default schedule's, since no item's arithmetic depends on which workgroup runs it.  The second
    child starts only if the first ended well."""
    names = R.CHILD_CASES
    for n in names:
        if n not in OUTPUTS:
            run_check(n)
    limit = CHILD_START + 2.0 * sum(TIMES[n] for n in names)
    with tempfile.TemporaryDirectory() as tmp:
        for cset, (knobs, _) in R.CHILD_SETS.items():
            env = dict(os.environ)
            env.update(knobs)
            path = os.path.join(tmp, cset + ".pt")
            r = subprocess.run([sys.executable, "-m", "tests.attn_ref_child", cset, path], env=env, cwd=ROOT, timeout=limit,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            print(r.stdout)
            assert r.returncode == 0, f"child '{cset}' ended with {r.returncode}:\n{r.stdout[-4000:]}"
            theirs = torch.load(path)
            assert sorted(theirs) == sorted(names)
            for n in names:
                for nm, t in OUTPUTS[n].items():
                    assert torch.equal(R.bits(t), R.bits(theirs[n][nm])), f"{cset} {n} {nm}: differs from the default schedule"
            print(f"BITWISE {cset}: {len(names)} cases equal to the default schedule's")
