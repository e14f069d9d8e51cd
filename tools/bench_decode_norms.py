"""Captured decode step of QK-norm / post-norm models: fused HIP step against the ATen step.
usage: python tools/bench_decode_norms.py [steps|kernels|default]

``steps``: GPT-2 small with qk_norm, with post_norm, and with both and 4 K/V heads, at B = 1 and 8:
the fused graph and the ``DLT_DECODE_FUSED=0`` graph of each are replayed in alternating windows
of 200 steps; median and range of the 5 windows of each.  ``kernels``: k_dec_norm_qkv_qkn next
to k_dec_norm_qkv, and the PN forms next to their plain forms (40 launches in a captured graph).
``default``: the default model's captured step (also runs on a tree without the norm forms)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_llm_trainer_amd.eval.decode import DecodeGraph, KVCache, forward_cached  # noqa: E402
from distributed_llm_trainer_amd.models import GPT, GPTConfig  # noqa: E402
from distributed_llm_trainer_amd.ops import hip  # noqa: E402

DEV = "cuda"


def _windows(fns, n=200, reps=5):
    """ms per call of each fn: alternating windows (one warm-up window each), [median, min, max]."""
    ts = [[] for _ in fns]
    for r in range(reps + 1):
        for i, f in enumerate(fns):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(n):
                f()
            torch.cuda.synchronize()
            if r:
                ts[i].append((time.perf_counter() - t) / n * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def _graph(m, B, fused):
    os.environ["DLT_DECODE_FUSED"] = fused
    c = KVCache(m.config, B, DEV, m.engine.act_dtype)
    forward_cached(m, torch.randint(0, 50257, (B, 32), device=DEV), c)
    return DecodeGraph(m, c, c.len)


def _model(**kw):
    torch.manual_seed(0)
    cfg = GPTConfig.from_preset("small")
    for k, v in kw.items():
        setattr(cfg, k, v)
    cfg.__post_init__()
    m = GPT(cfg).to(DEV)
    m.enable_engine()
    return m.eval()


def steps(models):
    for name, kw in models:
        m = _model(**kw)
        for B in (1, 8):
            with torch.no_grad():
                gs = [_graph(m, B, f) for f in (("1", "0") if kw else ("1",))]
            assert gs[0].fused and not (len(gs) > 1 and gs[1].fused)
            res = _windows([g.graph.replay for g in gs])
            line = " | ".join(f"{'fused' if g.fused else 'ATen'} {t[0]:.4f} ms ({t[1]:.4f}-{t[2]:.4f})" for g, t in zip(gs, res))
            print(f"{name} B={B}: {line}" + (f" | ratio {res[1][0] / res[0][0]:.2f}" if len(res) > 1 else ""), flush=True)
        del m


def _captured(fn, n=40):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    return lambda: g.replay(), n


def kernels(H=768, I=3072, V=50257, maxS=1024):
    nh = H // 64
    bf = dict(dtype=torch.bfloat16, device=DEV)
    cos, sin = hip.rope_tables(64, maxS, device=DEV)
    ln, qn, pos = torch.ones(H, device=DEV), torch.ones(64, device=DEV), torch.tensor([100], device=DEV)
    wqkv, wgu, emb = (torch.randn(r, H, **bf) * 0.02 for r in (3 * H, 2 * I, V))
    for B in (1, 8):
        h, h2, a = torch.randn(B, H, device=DEV), torch.empty(B, H, device=DEV), torch.randn(B, H, **bf)
        q, s, lg = torch.empty(B, H, **bf), torch.empty(B, I, **bf), torch.empty(B, V, device=DEV)
        kc, vc = (torch.zeros(B, nh, maxS, 64, **bf) for _ in "kv")
        post = (a, ln, h2)
        cases = {
            "norm_qkv": lambda **k: hip.dec_norm_qkv(h, ln, 1e-5, wqkv, cos, sin, pos, q, kc, vc, nh, **k),
            "norm_qkv_qkn": lambda **k: hip.dec_norm_qkv_qkn(h, ln, 1e-5, wqkv, qn, qn, cos, sin, pos, q, kc, vc, nh, nh, **k),
            "norm_gu": lambda **k: hip.dec_norm_gu(h, ln, 1e-5, wgu, s, **k),
            "norm_head": lambda **k: hip.dec_norm_head(h, ln, 1e-5, emb, lg, V, **k),
        }
        for name, f in cases.items():
            (plain, n), (pn, _) = _captured(f), _captured(lambda: f(post=post))
            r = _windows([plain, pn], n=20)
            print(f"{name} B={B}: plain {r[0][0] / n * 1e3:.2f} us ({r[0][1] / n * 1e3:.2f}-{r[0][2] / n * 1e3:.2f}) | "
                  f"PN {r[1][0] / n * 1e3:.2f} us ({r[1][1] / n * 1e3:.2f}-{r[1][2] / n * 1e3:.2f})", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "steps"
    if what == "steps":
        steps([("small qk_norm", dict(qk_norm=True)), ("small post_norm", dict(post_norm=True)),
               ("small qk_norm post_norm nkv=4", dict(qk_norm=True, post_norm=True, num_kv_heads=4))])
    elif what == "kernels":
        kernels()
    else:
        steps([("small default", {})])
