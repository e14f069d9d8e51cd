"""fp64 references, derived tolerances and fixed test inputs for the fused decode kernels
(``ops/csrc/decode.hip``), shared by test_decode_kernels_cpu.py and test_decode_kernels_gpu.py.

References.  Each takes the bf16 weights and the inputs the kernel takes and computes in
fp64, rounding to bf16 exactly where the kernel header says the kernel does: the normed
activations, every GEMV output that feeds a further step (RoPE, SwiGLU).  The LAST value of
a kernel (the RoPE / SwiGLU result, a plain GEMV output, an attention output) is returned
BEFORE its final bf16 rounding, so that the "final rounding" term below is a bound on one
rounding (of the kernel's value) and holds whichever way a near-tie falls.  Every reference
takes planted defects as options; the CPU file shows that each of them falls
outside the tolerance at the inputs the GPU tests use.

Tolerances: a sum of named terms per output element, each a function below with its reason.
  u8  = 2^-8   bound of half a bf16 ulp relative to the value (8 significant bits: half an
               ulp is 2^-9 of the binade's top, 2^-8 of its bottom)
  u23 = 2^-23  fp32 ulp of a value in [1, 2)
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from distributed_llm_trainer_amd.ops import rng
from distributed_llm_trainer_amd.ops.reference import rope_tables

U8 = 2.0 ** -8
U23 = 2.0 ** -23
EPS = 1e-5
DECODE_BATCHES = (1, 2, 4, 8)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """fp64 -> bf16 (round to nearest even) -> fp64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


# ------------------------------------------------------------------------------ GEMV
class Gemv(NamedTuple):
    y: torch.Tensor      # [B, R] fp64 sum_k w[r, k] x[b, k], not rounded
    sabs: torch.Tensor   # [B, R] sum_k |w x|
    mabs: torch.Tensor   # [B, R] max_k |w x|


def gemv(x: torch.Tensor, w: torch.Tensor, kmask: Optional[torch.Tensor] = None, chunk: int = 4096) -> Gemv:
    """x [B, K] fp64, w [R, K] bf16.  ``kmask`` [K] bool: columns a planted defect skips."""
    x = x.double()
    if kmask is not None:
        x = x * kmask.to(x)
    ys, ss, ms = [], [], []
    for r0 in range(0, w.shape[0], chunk):
        wc = w[r0:r0 + chunk].double()
        ys.append(x @ wc.T)
        ss.append(x.abs() @ wc.abs().T)
        ms.append(torch.stack([(wc.abs() * xb.abs()).amax(dim=1) for xb in x]))
    return Gemv(torch.cat(ys, 1), torch.cat(ss, 1), torch.cat(ms, 1))


def gemv_pre_tol(g: Gemv, K: int) -> torch.Tensor:
    """How far the kernel's fp32 dot product may be from the fp64 one, before any rounding."""
    # fp32 accumulation over K: every one of the K fused multiply-adds (and the shuffle-tree
    # adds) rounds a partial sum bounded by sum|w x| to 2^-24; K * 2^-23 * sum|w x| is the
    # classical (1 + 2^-24)^K - 1 bound with a factor 2 for the tree and the contraction order
    acc = K * U23 * g.sabs
    # a staged activation x_k (bf16 of an fp32 product in the kernel, of an fp64 product here)
    # can fall on the other side of a tie: one bf16 ulp of x_k (<= 2^-7 |x_k|) times w_k
    tie = 2 * U8 * g.mabs
    return acc + tie


def gemv_tol(g: Gemv, K: int) -> torch.Tensor:
    """Tolerance of a bf16-rounded GEMV output against the unrounded fp64 value."""
    final = U8 * g.y.abs()  # the kernel's final bf16 rounding: half an ulp <= 2^-8 |value|
    return final + gemv_pre_tol(g, K)


def slice_masks(K: int):
    """The planted K-range defects: {name: [K] bool mask of the columns still summed}."""
    out = {}
    m = torch.ones(K, dtype=torch.bool)
    m[K - 8:] = False
    out["drop_last_8_columns"] = m
    if K > 512:  # the last (partial, where K % 512) 512-element slice of rows_dot
        m = torch.ones(K, dtype=torch.bool)
        m[512 * ((K - 1) // 512):] = False
        out["drop_last_slice"] = m
    return out


def normed(h: torch.Tensor, lnw: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """bf16(h * rsqrt(mean(h^2) + eps) * w) in fp64 (the staged activations)."""
    h = h.double()
    rstd = torch.rsqrt((h * h).mean(dim=1, keepdim=True) + float(np.float32(eps)))
    return bf16_round(h * rstd * lnw.double())


class Checked(NamedTuple):
    ref: torch.Tensor
    tol: torch.Tensor


def qkv_ref(h, lnw, wqkv, cos, sin, pos: int, nh: int, kmask=None, rope_pos: Optional[int] = None):
    """dec_norm_qkv: {"q": [B, nh, 64], "k": ..., "v": ...} of Checked.  ``rope_pos`` rotates
    with another position's table row (planted defect)."""
    B, H = h.shape
    g = gemv(normed(h, lnw), wqkv, kmask)
    x = bf16_round(g.y).view(B, 3, nh, 64)          # the GEMV outputs, bf16 like torch's matmul
    pre = gemv_pre_tol(g, H).view(B, 3, nh, 64)
    rp = pos if rope_pos is None else rope_pos
    c, s = cos[rp].double().to(x.device), sin[rp].double().to(x.device)  # [32]
    out = {}
    for i, name in enumerate(("q", "k")):
        x1, x2, p1, p2 = x[:, i, :, :32], x[:, i, :, 32:], pre[:, i, :, :32], pre[:, i, :, 32:]
        ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
        # a GEMV output that rounds to the other side of a tie in fp32: one bf16 ulp of x1 / x2
        # times its partial derivative (c or s)
        flip = torch.cat([U8 * ((x1 * c).abs() + (x2 * s).abs()), U8 * ((x2 * c).abs() + (x1 * s).abs())], dim=-1)
        # the fp32 dot products' own error, through the same derivatives
        prop = torch.cat([c.abs() * p1 + s.abs() * p2, c.abs() * p2 + s.abs() * p1], dim=-1)
        out[name] = Checked(ref, U8 * ref.abs() + flip + prop)
    out["v"] = Checked(g.y.view(B, 3, nh, 64)[:, 2], gemv_tol(g, H).view(B, 3, nh, 64)[:, 2])
    return out


def gemv_res_ref(x, w, h, kmask=None) -> Checked:
    """dec_gemv_res: h + bf16(x . w^T), the sum in fp32."""
    K = x.shape[1]
    g = gemv(x.double(), w, kmask)
    # + the fp32 residual add (one rounding of a value of about |h|)
    return Checked(h.double() + g.y, gemv_tol(g, K) + U23 * h.double().abs())


def silu(x):
    return x * torch.sigmoid(x)


def norm_gu_ref(h, lnw, wgu, kmask=None, swap: bool = False) -> Checked:
    """dec_norm_gu: silu(g) * u with g, u the bf16 GEMV outputs.  ``swap``: gate and up rows
    exchanged (planted defect)."""
    H = h.shape[1]
    I = wgu.shape[0] // 2
    g = gemv(normed(h, lnw), wgu, kmask)
    tol = gemv_tol(g, H)
    gate, up, dg, du = bf16_round(g.y[:, :I]), bf16_round(g.y[:, I:]), tol[:, :I], tol[:, I:]
    if swap:
        gate, up, dg, du = up, gate, du, dg
    ref = silu(gate) * up
    # g and u are bf16-rounded intermediates: their error (tie flips included) times the
    # partial derivatives, |d silu / dg| <= 1.0999 and d/du = silu(g)
    return Checked(ref, U8 * ref.abs() + 1.1 * up.abs() * dg + silu(gate).abs() * du)


def norm_head_ref(h, lnw, emb, V: int, kmask=None) -> Checked:
    g = gemv(normed(h, lnw), emb[:V], kmask)
    return Checked(g.y, gemv_tol(g, h.shape[1]))


# -------------------------------------------------------------------------- attention
def attn_ref(q, kc, vc, pos: int, scale: float, extra_keys: int = 0, no_max: bool = False) -> Checked:
    """dec_attn: softmax(q . K[0..pos]^T * scale) . V per (b, head); [B, nh, 64].
    Planted defects: ``extra_keys`` more cache rows, ``no_max`` an fp32 softmax without the
    max subtraction."""
    B, nh, maxS, hd = kc.shape
    n = pos + 1 + extra_keys
    qd = q.double().view(B, nh, hd)
    K, V = kc[:, :, :n].double(), vc[:, :, :n].double()
    s = torch.einsum("bhd,bhjd->bhj", qd, K) * scale
    if no_max:
        e = torch.exp(s.float())
        p = (e / e.sum(dim=-1, keepdim=True)).double()
    else:
        p = torch.softmax(s, dim=-1)
    o = torch.einsum("bhj,bhjd->bhd", p, V)
    # final bf16 rounding + the probabilities' error.  A probability is __expf((s - max))
    # = exp2(fl(x * log2 e)): the argument rounding is |x| * 2^-24 <= 80 * 2^-24 relative in
    # the result for |s - max| <= 80 (beyond it p < 2e-35 and does not matter), exp2 itself
    # and the fp32 score (64 fmas on values of about |s|, a few 2^-24 absolute for scores of
    # order 1) add about 2^-22: 80 * 2^-24 + 2^-22 = 5e-6 relative per probability, in the
    # numerator and (averaged) the normaliser.  1e-4 is a 20x margin over that; the margin
    # also holds the fp32 sums over the keys (the longest sequential chain at maxS = 4096 is
    # 128 fmas per lane slot, 128 * 2^-24 = 8e-6 of sum p|v| in the worst case).
    tol = U8 * o.abs() + 1e-4 * torch.einsum("bhj,bhjd->bhd", p, V.abs())
    return Checked(o, tol)


# ---------------------------------------------------------------------------- inputs
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def column_profile(K: int) -> torch.Tensor:
    """Activation magnitudes per column: outlier channels at the end of K (as LLM residual
    streams have), so the last columns and the last slice carry weight a defect cannot hide
    behind the accumulation term."""
    p = torch.ones(K)
    p[512 * ((K - 1) // 512):] = 3.0
    p[K - 8:] = 8.0
    return p


def norm_weights(K: int, gen, wbf16: bool):
    w = 1.0 + 0.2 * torch.randn(K, generator=gen)
    return w.bfloat16() if wbf16 else w


def normed_inputs(seed: int, H: int, rows: int, wbf16: bool, wscale: float = 1.0):
    """(h [8, H] fp32, norm weight, w [rows, H] bf16); the kernels at B < 8 take h[:B]."""
    g = _gen(seed)
    h = 3.0 * torch.randn(8, H, generator=g) * column_profile(H)
    lnw = norm_weights(H, g, wbf16)
    w = (wscale * torch.randn(rows, H, generator=g) / math.sqrt(H)).bfloat16()
    return h, lnw, w


QKV_H = (192, 768, 1600)
QKV_POS = (0, 5, 63)
QKV_MAXS = 64


def qkv_inputs(H: int, wbf16: bool):
    return normed_inputs(100 + H, H, 3 * H, wbf16)


RES_SHAPES = ((768, 768), (1600, 6400), (100, 520), (20, 8), (768, 3072))


def res_inputs(R: int, K: int):
    """(x [8, K] bf16, w [R, K] bf16, h [8, R] fp32, nonzero)."""
    g = _gen(200 + R + K)
    x = (torch.randn(8, K, generator=g) * column_profile(K)).bfloat16()
    w = (torch.randn(R, K, generator=g) / math.sqrt(K)).bfloat16()
    h = 2.0 * torch.randn(8, R, generator=g)
    return x, w, h


GU_SHAPES = ((192, 1003), (768, 2048), (1600, 1000))


def gu_inputs(H: int, I: int, wbf16: bool):
    return normed_inputs(300 + H + I, H, 2 * I, wbf16, wscale=1.5)


HEAD_SHAPES = ((192, 17, 32), (768, 50257, 50304), (1600, 1000, 1000))


def head_inputs(H: int, V: int, rows: int, wbf16: bool):
    """The weight rows >= V are NaN: the kernel must not read them into any logit."""
    h, lnw, w = normed_inputs(400 + H + V, H, rows, wbf16, wscale=4.0)
    w[V:] = float("nan")
    return h, lnw, w


ATTN_POS = (0, 1, 31, 32, 255, 256, 257, 1023)
ATTN_SCALE = 0.125


def attn_inputs(nh: int, maxS: int, kind: str = "randn"):
    """(q [8, nh * 64] bf16, K cache, V cache [8, nh, maxS, 64] bf16).
    kind: "randn"; "large<m>" scores spread over +-m after scaling; "equal" all keys equal."""
    g = _gen(500 + nh + maxS)
    q = torch.randn(8, nh * 64, generator=g)
    kc = torch.randn(8, nh, maxS, 64, generator=g)
    vc = torch.randn(8, nh, maxS, 64, generator=g)
    if kind.startswith("large"):
        m = float(kind[5:])
        # keys along +-q: q . k * scale = t * |q|^2 / 8 with t uniform in [-1, 1] -> +-m
        qh = q.view(8, nh, 1, 64)
        t = torch.rand(8, nh, maxS, 1, generator=g) * 2 - 1
        t[:, :, 0], t[:, :, 1] = 1.0, -1.0
        kc = t * qh * (m / ATTN_SCALE) / (qh * qh).sum(-1, keepdim=True)
    elif kind == "equal":
        kc = kc[:, :, :1].expand(-1, -1, maxS, -1).contiguous()
    return q.bfloat16(), kc.bfloat16(), vc.bfloat16()


# --------------------------------------------------------------------------- sampler
def sample_reference(logits: torch.Tensor, T: float, top_k: int):
    """(kept [B, V] bool, probs [B, V] fp64): softmax(masked_fill(lg < kth, -inf)) of
    lg = logits / T (fp32 division, as the kernel divides); ties at the k-th value kept."""
    lg = logits.detach().cpu().float() / torch.tensor(T, dtype=torch.float32)
    V = lg.shape[1]
    if 0 < top_k < V:
        kth = torch.topk(lg, top_k, dim=1).values[:, -1:]
        lg = lg.masked_fill(lg < kth, float("-inf"))
    kept = torch.isfinite(lg)
    return kept, torch.softmax(lg.double(), dim=-1)


def freq_bound(p: torch.Tensor, n: int) -> torch.Tensor:
    """5 binomial standard deviations of an empirical frequency over n draws, + one draw."""
    return 5.0 * torch.sqrt(p * (1 - p) / n) + 1.0 / n


# ---- the draw's uniform: host model of draw_uniform() in decode.hip and of the hash
def uniform_of_bits(bits: np.ndarray) -> np.ndarray:
    """fp32 uniform of the hash's top 24 bits, as the kernels form it."""
    return bits.astype(np.float32) * np.float32(2.0 ** -24)


def uniform_of_bits_before_fix(bits: np.ndarray) -> np.ndarray:
    """((h >> 8) + 0.5f) * 2^-24 in fp32: what the kernels computed before."""
    return (bits.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def draw_hash(seed: int, pos: int, b: int) -> int:
    return rng.lowbias32((seed & rng.MASK32) ^ rng.lowbias32((pos * 0x9E3779B9 + b) & rng.MASK32))


def _unxorshift(x: int, s: int) -> int:
    y = x
    for _ in range(32 // s + 1):
        y = x ^ (y >> s)
    return y


def lowbias32_inverse(h: int) -> int:
    x = _unxorshift(h & rng.MASK32, 16)
    x = (x * pow(0x846CA68B, -1, 1 << 32)) & rng.MASK32
    x = _unxorshift(x, 15)
    x = (x * pow(0x7FEB352D, -1, 1 << 32)) & rng.MASK32
    return _unxorshift(x, 16)


def seed_for_bits(pos: int, b: int, bits24: int, low8: int = 0x5A) -> int:
    """A seed whose draw hash at (pos, b) has h >> 8 == bits24 (lowbias32 is a bijection)."""
    return lowbias32_inverse((bits24 << 8) | low8) ^ rng.lowbias32((pos * 0x9E3779B9 + b) & rng.MASK32)
