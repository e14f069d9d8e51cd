"""References for the sliding-window decode kernels (``dec_attn`` / ``dec_attn_gqa`` with
``window=W`` in ``ops/csrc/decode.hip``), shared by test_window_cpu.py and test_window_gpu.py.

A layer with a window of W keys attends, at position ``pos``, to the cache rows
``kf .. pos`` with ``kf = max(0, pos - W + 1)``.  The fp64 reference is therefore the
existing one (``decode_ref.attn_ref`` / ``decode_gqa_ref.attn_gqa_ref``) on the cache
sliced to ``[kf, pos]`` at position ``pos - kf``, with its tolerance unchanged: the kernel's
arithmetic per key is what it was, only the set of keys differs.

``attn_gqa_win_split32`` is an fp32 torch model of the window-anchored split kernel: chunk s
holds the keys ``[kf + s C, min(kf + (s + 1) C, pos + 1))`` with
``C = dec_attn_chunk(min(W, maxS), NS)``.  Its ``defect=`` switch plants the mistakes a
windowed kernel can make; the CPU file shows that the model is inside the tolerance and each
defect outside it at the inputs the GPU tests use.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from tests import decode_gqa_ref as G
from tests import decode_ref as R

# ------------------------------------------------------------------------------ shapes
MHA_NH, MHA_MAXS = 4, 320
MHA_WINDOWS = (1, 5, 64, 256, 257, 320, 1000)
MHA_KINDS = ("randn", "large60", "equal")
GQA_HEADS = ((4, 1), (4, 2), (6, 2), (12, 4))
GQA_SPLITS = (1, 2, 4, 8)
GQA_MAXS = G.ATTN_MAXS  # 200
GQA_WINDOWS = (50, 7)   # 50: C = 13 at NS = 4, a ragged last chunk; 7 with NS = 8: C = 1
DEFECTS = ("include_key_before_window", "drop_first_window_key", "chunks_anchored_at_0", "chunk_from_maxS")


def first_key(pos: int, W: Optional[int]) -> int:
    return 0 if not W else max(0, pos - W + 1)


def chunk(maxS: int, W: Optional[int], NS: int) -> int:
    """``dec_attn_chunk(min(W, maxS), NS)``: keys per workgroup of the windowed split kernel."""
    n = maxS if not W else min(W, maxS)
    return -(-n // NS)


def mha_positions(W: int, maxS: int = MHA_MAXS):
    """0, both sides of the first position whose window is full (W - 1), 255 / 256 (the
    thread count of the kernel), the last cache row."""
    return tuple(sorted({p for p in (0, W - 2, W - 1, W, 255, 256, maxS - 1) if 0 <= p < maxS}))


def gqa_positions(W: int, C: int, NS: int, maxS: int = GQA_MAXS):
    """Both sides of W - 1 and, for a full window ending at maxS - 1 and one in the middle of
    the cache, of every chunk start kf + s C."""
    ps = {0, W - 2, W - 1, W, maxS - 1}
    for s in range(1, NS):
        ps |= {s * C - 1, s * C, s * C + 1}                  # growing window: kf = 0
    mid = maxS // 2
    ps |= {mid, mid + 1}                                     # a full window inside the cache
    return tuple(sorted(p for p in ps if 0 <= p < maxS))


# ------------------------------------------------------------------------------ fp64
def attn_win_ref(q, kc, vc, pos: int, scale: float, W: Optional[int]) -> R.Checked:
    """dec_attn(window=W): ``decode_ref.attn_ref`` on rows kf..pos of the caches."""
    kf = first_key(pos, W)
    return R.attn_ref(q, kc[:, :, kf:pos + 1], vc[:, :, kf:pos + 1], pos - kf, scale)


def attn_gqa_win_ref(q, kc, vc, pos: int, scale: float, nh: int, W: Optional[int]) -> R.Checked:
    """dec_attn_gqa(window=W): ``decode_gqa_ref.attn_gqa_ref`` on rows kf..pos of the caches."""
    kf = first_key(pos, W)
    return G.attn_gqa_ref(q, kc[:, :, kf:pos + 1], vc[:, :, kf:pos + 1], pos - kf, scale, nh)


# ------------------------------------------------------------------------------ fp32 model
class Split(NamedTuple):
    o: torch.Tensor  # [B, nh, 64] bf16, the merged output
    m: torch.Tensor  # [B, nh, NS] fp32 chunk maxima (-inf for an empty chunk)
    l: torch.Tensor  # [B, nh, NS] fp32 chunk sums of exp(score - m) (0 for an empty chunk)


# How far the kernel's partials may be from the model's.  m is the maximum of fp32 scores, each
# 64 fmas on products whose absolute values sum (scaled) to at most 64 at the +-60 scores of
# "large60" (keys along +-q: every product has the sign of the score), + the bf16 keys' own
# spread there: 64 * 2^-24 * 64 = 2.4e-4, 1e-3 is a 4x margin.  l sums exp(s - m) with both s
# and m that uncertain: 2e-3 relative per term, + the fp32 sum over at most 200 keys
# (200 * 2^-24): 5e-3 relative is a 2x margin.  An empty chunk is exact: m = -inf, l = 0.
M_ATOL = 1e-3
L_RTOL = 5e-3


def partials_match(got: Split, want: Split) -> bool:
    """The chunk partials of the kernel (read back from its workspace) against the model's:
    the same chunks empty, m within M_ATOL and l within L_RTOL elsewhere."""
    empty = want.l == 0
    if not torch.equal(got.l == 0, empty) or not torch.equal(torch.isneginf(got.m), empty):
        return False
    live = ~empty
    return bool(((got.m[live] - want.m[live]).abs() <= M_ATOL).all()
                and ((got.l[live] - want.l[live]).abs() <= L_RTOL * want.l[live]).all())


def attn_gqa_win_split32(q, kc, vc, pos: int, scale: float, nh: int, NS: int, W: Optional[int],
                         defect: Optional[str] = None) -> Split:
    """fp32 model of the windowed ``k_dec_attn_gqa`` + ``k_dec_attn_combine``: per chunk
    (m, l, o) in fp32, merged in the order s = 0 .. NS - 1 with exp(m_s - M), empty chunks
    skipped.  ``W`` None / 0: a global layer (the kernel without a window).
    ``defect``:
      include_key_before_window  key pos - W is read too (an off-by-one in kf)
      drop_first_window_key      key pos - W + 1 is left out (the other off-by-one)
      chunks_anchored_at_0       chunk s = [s C, (s + 1) C) cut to the window, as the kernel
                                 without a window anchors them: keys at or beyond NS C are
                                 never read
      chunk_from_maxS            chunks anchored at kf but C = dec_attn_chunk(maxS, NS): the
                                 output is right, the window sits in the first chunk(s) and
                                 the other workgroups idle -- visible in the partials only"""
    assert defect is None or defect in DEFECTS
    B, nkv, maxS = kc.shape[:3]
    idx = G.kv_head_of(nh, nkv).to(kc.device)
    end = pos + 1
    kf = first_key(pos, W)
    C = chunk(maxS, W, NS)
    if defect == "include_key_before_window":
        kf = max(0, kf - 1)
    elif defect == "drop_first_window_key":
        kf = min(kf + 1, pos)
    elif defect == "chunk_from_maxS":
        C = -(-maxS // NS)
    qf = q.float().view(B, nh, 64)
    ms = torch.full((B, nh, NS), float("-inf"), device=kc.device)
    ls = torch.zeros(B, nh, NS, device=kc.device)
    parts = []
    for s in range(NS):
        if defect == "chunks_anchored_at_0":
            lo, hi = max(s * C, kf), min((s + 1) * C, end)
        else:
            lo, hi = kf + s * C, min(kf + (s + 1) * C, end)
        if hi <= lo:
            continue
        K = kc[:, :, lo:hi].float().index_select(1, idx)
        V = vc[:, :, lo:hi].float().index_select(1, idx)
        sc = torch.einsum("bhd,bhjd->bhj", qf, K) * torch.tensor(scale, dtype=torch.float32)
        m = sc.amax(dim=-1, keepdim=True)
        p = torch.exp(sc - m)
        l = p.sum(dim=-1, keepdim=True)
        ms[:, :, s], ls[:, :, s] = m[..., 0], l[..., 0]
        parts.append((m, l, torch.einsum("bhj,bhjd->bhd", p, V)))
    if not parts:  # (a defect only) no chunk holds a key: nothing is summed
        return Split(torch.full((B, nh, 64), float("nan")).bfloat16(), ms, ls)
    if NS == 1:
        m, l, o = parts[0]
        return Split((o * (1.0 / l)).bfloat16(), ms, ls)
    M = parts[0][0]
    for m, _, _ in parts[1:]:
        M = torch.maximum(M, m)
    L = torch.zeros_like(M)
    acc = torch.zeros_like(parts[0][2])
    for m, l, o in parts:
        f = torch.exp(m - M)
        L = L + l * f
        acc = acc + o * f
    return Split((acc / L).bfloat16(), ms, ls)


def workspace_partials(ws: torch.Tensor, B: int, nh: int, NS: int) -> Split:
    """(None, m, l) of the kernel's workspace [B, nh, NS, 66]: o[64], m, l per partial.  The o
    of an empty chunk is not written (nor read by the combine): only m and l are compared."""
    w = ws.view(B, nh, NS, 66)
    return Split(None, w[..., 64].clone(), w[..., 65].clone())
