"""Micro-benchmark of the attention kernels at the headline shape (B8 nh12 S1024 hd64).

``--doc_len N`` also times the document-masked kernels (``doc=``) in the same run: a
separator every N tokens (N >= S: no boundary inside the sequence, i.e. trivial bounds --
the cost of the DOC instantiations themselves), or ``rand:N``: seeded geometric document
lengths with mean N, different in every batch row.  ``--kv_heads N`` times grouped-query
attention: N K/V heads shared by groups of nh / N query heads (the GQA kernels; N == nh
runs them with groups of one, no flag the MHA kernels).  ``--window W`` times sliding-window
attention (``window=W``: the DOC kernels on ``window_bounds`` and the banded keep-bit
kernel) against causal in the same process, the two alternating round by round, and the
banded against the full keep-bit kernel.  ``--softcap CAP`` times attention-score soft-capping
(``softcap=CAP``: the CAP kernels) against the plain kernels the same way.  The backward is one call (dQ then
dK/dV); a kernel trace of this tool (``tools/ab/prof_step.sh`` style: ``rocprofv3
--kernel-trace --stats``) splits it per kernel."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_llm_trainer_amd.ops import hip, rng  # noqa: E402

SEP = 0  # separator id of the synthetic token rows (every other token is 1)


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def doc_ids(spec: str, B: int, S: int, seed: int = 0) -> torch.Tensor:
    """Token rows [B, S] whose separators realise ``spec`` (``N`` or ``rand:N``)."""
    ids = torch.ones(B, S, dtype=torch.int64)
    if spec.startswith("rand:"):
        mean = float(spec[5:])
        g = torch.Generator().manual_seed(seed)
        for b in range(B):
            pos = -1
            while True:  # geometric lengths >= 1 with the given mean
                u = torch.rand((), generator=g).item()
                pos += 1 + (int(math.log1p(-u) / math.log1p(-1.0 / mean)) if mean > 1 else 0)
                if pos >= S:
                    break
                ids[b, pos] = SEP
    else:
        n = int(spec)
        if n < 1:
            raise ValueError("--doc_len must be >= 1")
        ids[:, n - 1::n] = SEP
    return ids


def attended_fraction(doc, S: int) -> float:
    """Scores inside the mask, relative to the causal triangle."""
    lo = doc[0].long()
    q = torch.arange(S, device=lo.device)
    return float((q - lo + 1).sum()) / (lo.shape[0] * S * (S + 1) / 2)


def window_ab(a, q, k, v, key, gkw):
    """causal vs window=W, head-major, alternating: per round fwd (keep bits included), the
    forward kernel alone on given bits, bwd on stored bits, and the keep-bit kernel alone
    (full vs banded).  Prints every round and the medians; the spread of the causal rows
    over the rounds is the noise the ratios have to be read against."""
    W = a.window
    cases = {"causal": dict(gkw), f"window {W}": dict(gkw, window=W)}
    st = {}
    for name, kw in cases.items():
        o, aux = hip.attention_fwd(q, k, v, a.p, key, **kw)
        st[name] = (o, aux, torch.randn_like(o))
    rows = {n: [] for n in cases}
    bits = {"full": [], "banded": []}
    for r in range(a.rounds):
        for name, kw in cases.items():
            o, aux, do = st[name]
            t_f = timeit(lambda: hip.attention_fwd(q, k, v, a.p, key, **kw), a.iters)
            t_k = timeit(lambda: hip.attention_fwd(q, k, v, a.p, key, mask=aux[1], **kw), a.iters) if a.p > 0 else t_f
            t_b = timeit(lambda: hip.attention_bwd(q, k, v, o, do, aux, a.p, key, **kw), a.iters)
            rows[name].append((t_f, t_k, t_b))
            print(f"round {r} [{name}] fwd incl. keep bits {t_f:.1f} us, fwd kernel {t_k:.1f} us, bwd {t_b:.1f} us", flush=True)
        if a.p > 0:
            buf = st["causal"][1][1]
            for name, wkw in (("full", {}), ("banded", {"window": W})):
                bits[name].append(timeit(lambda: hip.attention_dropout_mask(a.B, a.nh, a.S, a.p, key, device="cuda",
                                                                            out=buf, **wkw), a.iters))
            print(f"round {r} keep-bit kernel: full {bits['full'][-1]:.1f} us, banded {bits['banded'][-1]:.1f} us", flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    m = {n: [med([row[i] for row in rows[n]]) for i in range(3)] for n in cases}
    c, w = m["causal"], m[f"window {W}"]
    spread = [(max(row[i] for row in rows["causal"]) - min(row[i] for row in rows["causal"])) / c[i] * 100 for i in range(3)]
    print(f"B{a.B} nh{a.nh} S{a.S} p{a.p} window {W}, medians of {a.rounds} rounds x {a.iters} iterations:")
    for i, nm in enumerate(("fwd incl. keep bits", "fwd kernel", "bwd (dQ + dK/dV)")):
        print(f"  {nm}: causal {c[i]:.1f} us, window {w[i]:.1f} us, ratio {c[i] / w[i]:.2f}x "
              f"(causal spread over the rounds {spread[i]:.1f} %)")
    if a.p > 0:
        print(f"  keep-bit kernel: full {med(bits['full']):.1f} us, banded {med(bits['banded']):.1f} us, "
              f"ratio {med(bits['full']) / med(bits['banded']):.2f}x")


def softcap_ab(a, q, k, v, key, gkw):
    """plain vs softcap=CAP (the CAP kernels), head-major, alternating round by round: the forward
    kernel alone on given keep bits and the backward (dQ + dK/dV) on stored bits.  The causal rows'
    spread over the rounds is the noise the ratios have to be read against; a kernel trace of this
    mode splits the backward per kernel."""
    cases = {"plain": dict(gkw), f"softcap {a.softcap:g}": dict(gkw, softcap=a.softcap)}
    st = {}
    for name, kw in cases.items():
        o, aux = hip.attention_fwd(q, k, v, a.p, key, **kw)
        st[name] = (o, aux, torch.randn_like(o))
    rows = {n: [] for n in cases}
    for r in range(a.rounds):
        for name, kw in cases.items():
            o, aux, do = st[name]
            mkw = {"mask": aux[1]} if a.p > 0 else {}
            t_k = timeit(lambda: hip.attention_fwd(q, k, v, a.p, key, **mkw, **kw), a.iters)
            t_b = timeit(lambda: hip.attention_bwd(q, k, v, o, do, aux, a.p, key, **kw), a.iters)
            rows[name].append((t_k, t_b))
            print(f"round {r} [{name}] fwd kernel {t_k:.1f} us, bwd {t_b:.1f} us", flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    m = {n: [med([row[i] for row in rows[n]]) for i in range(2)] for n in cases}
    c, w = m["plain"], m[f"softcap {a.softcap:g}"]
    spread = [(max(row[i] for row in rows["plain"]) - min(row[i] for row in rows["plain"])) / c[i] * 100 for i in range(2)]
    print(f"B{a.B} nh{a.nh} S{a.S} p{a.p} softcap {a.softcap:g}, medians of {a.rounds} rounds x {a.iters} iterations:")
    for i, nm in enumerate(("fwd kernel", "bwd (dQ + dK/dV)")):
        print(f"  {nm}: plain {c[i]:.1f} us, capped {w[i]:.1f} us, ratio {w[i] / c[i]:.2f}x "
              f"(plain spread over the rounds {spread[i]:.1f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--nh", type=int, default=12)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--packed", action="store_true", help="attention on the packed [B*S, 3H] QKV (engine default)")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    ap.add_argument("--doc_len", default=None, metavar="N|rand:N",
                    help="also time the document-masked kernels: a separator every N tokens, or seeded geometric "
                         "lengths with mean N (rand:N); N >= S gives trivial bounds")
    ap.add_argument("--kv_heads", type=int, default=None, metavar="N",
                    help="grouped-query attention with N K/V heads (must divide --nh); default: the MHA kernels")
    ap.add_argument("--window", type=int, default=None, metavar="W",
                    help="also time sliding-window attention of W keys, alternating with causal (--rounds rounds)")
    ap.add_argument("--softcap", type=float, default=None, metavar="CAP",
                    help="time attention-score soft-capping (the CAP kernels) against the plain kernels, alternating "
                         "(--rounds rounds)")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of the --window / --softcap comparison")
    ap.add_argument("--only", default="both", choices=("both", "off", "doc"),
                    help="which variants to run (a kernel trace of one variant: --only off / --only doc)")
    a = ap.parse_args()
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    torch.manual_seed(0)
    nkv = a.nh if a.kv_heads is None else a.kv_heads
    if nkv < 1 or a.nh % nkv:
        raise ValueError("--kv_heads must divide --nh")
    gkw = {} if a.kv_heads is None else {"nkv": nkv}
    q = torch.randn(a.B, a.nh, a.S, 64, device="cuda").to(dt)
    k, v = (torch.randn(a.B, nkv, a.S, 64, device="cuda").to(dt) for _ in range(2))
    key = rng.site_key(1, 2, 3, rng.SITE_ATTN)
    variants = []
    if a.only != "doc" or a.doc_len is None:
        variants.append(("causal", {}))
    if a.doc_len is not None and a.only != "off":
        doc = hip.doc_bounds(doc_ids(a.doc_len, a.B, a.S).cuda(), SEP)
        variants.append((f"doc_len {a.doc_len} ({100 * attended_fraction(doc, a.S):.1f} % of the causal scores)",
                         {"doc": doc}))
    fl = 4 * a.B * a.nh * a.S * a.S / 2 * 64
    if a.window is not None:
        window_ab(a, q, k, v, key, gkw)
        return
    if a.softcap is not None:
        softcap_ab(a, q, k, v, key, gkw)
        return
    if a.kv_heads is not None:
        nrb = (a.S + 63) // 64
        print(f"kv_heads {nkv} (groups of {a.nh // nkv}): dK/dV runs {a.B * nkv * nrb} work items "
              f"(MHA: {a.B * a.nh * nrb}), each over {a.nh // nkv} query heads")
    for name, kw in variants:
        kw = dict(kw, **gkw)
        tag = f"[{name}] " if a.doc_len is not None else ""  # the plain run prints what it always has
        if a.packed:
            qkv = torch.randn(a.B * a.S, (a.nh + 2 * nkv) * 64, device="cuda").to(dt)
            cos, sin = hip.rope_tables(64, a.S, device="cuda")
            o, aux = hip.attention_fwd_packed(qkv, a.B, a.S, a.nh, a.p, key, **kw)
            do = torch.randn_like(o)
            t_f = timeit(lambda: hip.attention_fwd_packed(qkv, a.B, a.S, a.nh, a.p, key, **kw), a.iters)
            t_b = timeit(lambda: hip.attention_bwd_packed(qkv, o, do, aux, a.p, key, a.B, a.S, a.nh, cos, sin, **kw),
                         a.iters)
            if a.p > 0:  # the forward kernel alone (keep bits already generated) -> bits kernel time
                m = aux[1]
                if m is not None:
                    t_k = timeit(lambda: hip.attention_fwd_packed(qkv, a.B, a.S, a.nh, a.p, key, mask=m, **kw),
                                 a.iters)
                    print(f"{tag}fwd kernel {t_k:.1f} us, keep-bit kernel {t_f - t_k:.1f} us")
        else:
            o, aux = hip.attention_fwd(q, k, v, a.p, key, **kw)
            do = torch.randn_like(o)
            t_f = timeit(lambda: hip.attention_fwd(q, k, v, a.p, key, **kw), a.iters)
            t_b = timeit(lambda: hip.attention_bwd(q, k, v, o, do, aux, a.p, key, **kw), a.iters)
        # TF/s by the causal FLOP count for every variant, so the rows compare as times do
        print(f"{tag}fwd {t_f:.1f} us ({fl / t_f / 1e6:.1f} TF/s)  bwd {t_b:.1f} us ({2.5 * fl / t_b / 1e6:.1f} TF/s)")


if __name__ == "__main__":
    main()
