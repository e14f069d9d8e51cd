"""Is the attention forward / backward waiting on its K/V (Q/dO) tile loads?  Times the
kernels at B16 nh12 S1024 (packed QKV, dropout 0.1) normally and with every (batch,
head) reading head 0's rows (in_bs = in_hs = 0: a one-head working set, L2-resident;
results are garbage, only the time matters)."""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_llm_trainer_amd.ops import hip, rng  # noqa: E402
from distributed_llm_trainer_amd.ops.hip import _attn_bwd_launch, _attn_fwd_launch, _packed_row  # noqa: E402


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
    return s.elapsed_time(e) / iters * 1e3


B, nh, S, hd, p = 16, 12, 1024, 64, 0.1
H = nh * hd
M = B * S
key = rng.site_key(1, 2, 3, rng.SITE_ATTN)
qkv = torch.randn(M, 3 * H, device="cuda").bfloat16()
cos, sin = hip.rope_tables(64, S, device="cuda")
o, aux = hip.attention_fwd_packed(qkv, B, S, nh, p, key)
lse, mask = aux
do = torch.randn_like(o)
keep = (rng.keep_threshold(p), 1.0 / (1.0 - p), mask)
dqkv = torch.empty(M, 3 * H, dtype=torch.bfloat16, device="cuda")
ptrs, st, _ = _packed_row(qkv, S, H, hd, H)
dst = _packed_row(dqkv, S, H, hd, H)
sc = 1.0 / math.sqrt(hd)
for name, bs, hs in (("normal", st[0], st[1]), ("one head (L2)", 0, 0)):
    src = (ptrs, (bs, hs, st[2]), (bs, hs, st[2]))

    def fwd():
        _attn_fwd_launch("attn_fwd_packed", src, o, lse, keep + (0,), key, None, B, nh, None, S, hd, 0, sc)

    def bwd():
        _attn_bwd_launch("attn_bwd_packed", src, dst, o, do, lse, keep, (None, None), (cos, sin), B, nh, None, S, hd,
                         0, sc)
    print(f"{name:14s} fwd {timeit(fwd):6.1f} us  bwd (dQ + dK/dV) {timeit(bwd):6.1f} us", flush=True)
