"""fp64 references, derived tolerances, fixed inputs, planted defects and a model of the
launchers' dispatch for the hand-written GEMM kernels (``ops/csrc/gemm_bf16.hip``,
``gemm_fw4.hip``, ``gemm_wgrad.hip`` and the split-K sums of ``elementwise.hip``), shared by
test_gemm_kernels_cpu.py and test_gemm_kernels_gpu.py.  Nothing here needs a GPU.  The shared
pieces (Checked, Guarded, final_rounding, ...) are those of tests/stream_ref.py.

References.  Each takes exactly what the kernel takes (16-bit operands as stored, the fp32 base
as stored), computes in fp64 and returns every output BEFORE its final rounding.  ``defect=``
plants one of DEFECTS; the CPU file shows that each of them falls outside the tolerance at the
case the GPU file runs.

Tolerances: a sum of named terms per output element, read from the kernel code.
  products      16-bit x 16-bit is exact in fp32 (8 + 8 or 11 + 11 significant bits): zero
  chains        v_mfma_f32_16x16x32 adds 32 products to an fp32 accumulator; a K-tile of 64 is two
                of them per accumulator, K / 32 (T / 32 for a weight gradient) in all.  How the
                instruction rounds inside is not specified: it is ASSUMED to be no worse than
                adding its 32 products to the accumulator one at a time, each partial sum cut or
                rounded to fp32, in some order.  That is n roundings for n terms, each a whole
                U23 of a partial sum that the sum of absolute terms bounds (``chain``)
  partials      split-K: k_splitk_acc adds the partials to dW one after the other (splits
                roundings); stream-K: the fix-up adds the slots of a tile's shares in increasing
                share order (at most Gc); one split or a whole-tile share adds its accumulator to
                dW (one).  Every one is U23 of at most sum |terms| + |base|
  intermediate  a fused epilogue rounds the product to 16 bits first (the pre-rotation qkv, gu,
                ds).  The kernel's product lies within ``pre`` of the reference's, so its rounding
                is some value between round(ref - pre) and round(ref + pre): the farther of the two
                from round(ref) bounds the intermediate's error, zero away from a near-tie
                (``flip``)
  sigmoid       dlt_sigmoid(x) = rcp(1 + exp2(-x log2 e)): the exponent's product (half a U23 of
                |x|), the hardware exp2 and rcp (ASSUMED one ulp each, as tests/attn_ref.py
                assumes of exp2) and the add, relative to sigma: U23 (|x| + 4) (``eps_sig``); an
                exponential under the normal range is flushed to zero (EXP_FLUSH, absolute)
  final         stream_ref.final_rounding(): one round-to-nearest of the kernel's own value
On the ``int`` family every product and every partial sum of every route is an integer below
2^24, so the chain, partial and intermediate terms are exactly zero whatever the order: a
tolerance of zero means "bit-equal to round_to(ref)" (for fp32 outputs, to ref itself).  The
arithmetic of a fused epilogue (rotation, sigmoid) is not exact and keeps its terms there.
``bias_ratio`` looks at the sign of the errors, which no element-wise bound can.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import torch

from distributed_llm_trainer_amd.ops import reference as opsref
from tests.stream_ref import (BF, DT_NAME, DTYPES, EXP_FLUSH, F32, F64, HF, U23, Checked, bits, final_rounding, round_to)
from tests.stream_ref import Guarded  # noqa: F401  (the GPU file takes it from here, with the rest)

MFMA_K = 32    # reduction depth of one v_mfma_f32_16x16x32_{bf16,f16}
BK = 64        # K-tile of every kernel here (GB_BK, GW_BK, F4_BK)
BM = 256       # tile rows
EXACT = 2 ** 24  # integers below it are exact in fp32


def chain(n: int) -> float:
    """Roundings of an fp32 accumulation over n terms (see the header), times U23."""
    return n * U23


def eps_sig(g: torch.Tensor) -> torch.Tensor:
    return U23 * (g.abs() + 4.0)


def sigmoid(g: torch.Tensor) -> torch.Tensor:
    return torch.sigmoid(g)


def flip(ref: torch.Tensor, pre: torch.Tensor, dt) -> torch.Tensor:
    """Bound on |kernel's rounding - round_to(ref)| of an intermediate 16-bit rounding."""
    mid = round_to(ref, dt).double()
    lo, hi = round_to(ref - pre, dt).double(), round_to(ref + pre, dt).double()
    return torch.maximum((hi - mid).abs(), (lo - mid).abs())


def trunc_to(x: torch.Tensor, dt) -> torch.Tensor:
    """fp64 -> ``dt`` towards zero: what a kernel that cuts the significand instead of rounding it
    stores (planted defect ``trunc_final``)."""
    r = round_to(x, dt)
    over = r.double().abs() > x.abs()
    return torch.where(over, bits(r) - 1, bits(r)).view(dt)  # one step down in sign-magnitude


def bias_ratio(out: torch.Tensor, chk: Checked) -> float:
    """|sum_i (out_i - ref_i) sign(ref_i)| over 6 sqrt(sum_i tol_i^2): round-to-nearest errors have
    no preferred sign, a truncating store errs towards zero in every element (Hoeffding: above
    1 with probability under 2 exp(-18) for independent errors bounded by tol_i)."""
    d = (out.double().reshape(chk.ref.shape) - chk.ref) * torch.sign(chk.ref)
    return (d.sum().abs() / (6.0 * chk.tol.pow(2).sum().sqrt()).clamp_min(1e-300)).item()


DEFECTS = ("drop_last_ktile", "drop_ktile1", "second_tile_first_operands", "swap_tile_rc", "skip_half_row_tile",
           "skip_ragged_half", "split_pair_dropped", "split_pair_doubled", "sk_drop_share", "ignore_base",
           "base_twice", "trunc_final", "rope_sign", "rope_pos_m", "rope_on_v", "gu_swapped", "s_unrounded",
           "ld_ignored")

FAMILIES = ("gauss", "int", "cancel")


# ================================================================================ inputs
def int_range(n: int, extra: int = 0) -> int:
    """Largest r <= 3 with n r^2 + extra < 2^24: every partial sum of n products of integers in
    [-r, r] (plus a base of magnitude <= extra) is an integer below 2^24."""
    r = 3
    while r > 1 and n * r * r + extra >= EXACT:
        r -= 1
    assert n * r * r + extra < EXACT
    return r


INT_BASE = 8  # |base| of the int family's weight gradients


@functools.lru_cache(maxsize=None)
def operands(seed: int, m: int, n: int, R: int, family: str, dt, qscale: float = 1.0):
    """(P [m, R], Q [n, R]) 16-bit, the reduction index last.  gauss: randn (Q times qscale).
    int: integers in [-r, r], r = int_range(R).  cancel: the second half of the reduction repeats
    the first with Q negated plus a 2^-6 perturbation, all times 8: the terms are about 64
    and the sum about 1, so only a bound relative to the sum of absolute terms holds."""
    g = torch.Generator().manual_seed(seed)
    if family == "int":
        r = int_range(R, INT_BASE)
        P = torch.randint(-r, r + 1, (m, R), generator=g).double()
        Q = torch.randint(-r, r + 1, (n, R), generator=g).double()
    else:
        P = torch.randn(m, R, generator=g, dtype=F64)
        Q = torch.randn(n, R, generator=g, dtype=F64) * qscale
        if family == "cancel":
            h = R // 2
            P, Q = P * 8, Q * 8
            P[:, h:] = P[:, :h]
            Q[:, h:] = -Q.to(F32).to(dt).double()[:, :h] + torch.randn(n, h, generator=g, dtype=F64) * 2.0 ** -6 * 8
    return P.to(F32).to(dt), Q.to(F32).to(dt)


def _keep(R: int, defect) -> Optional[torch.Tensor]:
    """Reduction indices a kernel with a K-loop defect still visits."""
    idx = torch.arange(R)
    if defect == "drop_last_ktile":
        return idx[idx < R - BK]
    if defect == "drop_ktile1":
        return idx[(idx < BK) | (idx >= 2 * BK)]
    return None


def _prod(P, Q, keep=None):
    Pd, Qd = P.double(), Q.double()
    if keep is not None:
        Pd, Qd = Pd[:, keep], Qd[:, keep]
    return Pd @ Qd.t()


def product_ref(P, Q, family: str, defect: Optional[str] = None):
    """(P Q^T in fp64, the error bound of the kernel's fp32 accumulator)."""
    R = P.shape[1]
    y = _prod(P, Q, _keep(R, defect))
    if family == "int":
        return y, torch.zeros_like(y)
    return y, chain(R) * (P.double().abs() @ Q.double().abs().t())


def _store(y, pre, dt, family):
    if family == "int":
        return Checked(y, torch.zeros_like(y))
    return Checked(y, pre + final_rounding(y, pre, dt))


# ======================================================================== plain GEMMs
def gemm_ref(P, Q, family: str, defect: Optional[str] = None, walk=None, bn: int = 192) -> Checked:
    """C = P Q^T (gemm_bf16: P = A, Q = B; gemm_dgrad: P = dY, Q = W^T; gemm_fw4).  ``walk``:
    the per-workgroup tile lists of gb_walk / fw4_walk for the tile defects."""
    dt = P.dtype
    y, pre = product_ref(P, Q, family, defect)
    blk = lambda t: (slice(t[0] * BM, t[0] * BM + BM), slice(t[1] * bn, min(t[1] * bn + bn, y.shape[1])))
    if defect == "second_tile_first_operands":  # a workgroup's second tile computed from its first tile's panels
        wg = next(w for w in walk if len(w) >= 2)
        y = y.clone()
        src = y[blk(wg[0])]
        dst = y[blk(wg[1])]
        dst.copy_(src[:, :dst.shape[1]])
    if defect == "swap_tile_rc":  # tile (0, 1) computed and stored as (1, 0): (0, 1) keeps the fill
        y = y.clone()
        y[blk((0, 1))] = 0.0
    if defect == "skip_ragged_half":  # fw4: the last 128 columns of a ragged N are never stored
        y = y.clone()
        y[:, -128:] = 0.0
    return _store(y, pre, dt, family)


def strided(t: torch.Tensor, pad: int, seed: int = 0) -> torch.Tensor:
    """``t`` [r, c] as the first c columns of a [r, c + pad] tensor whose other columns hold
    other values of the same family (so that reading them is visible)."""
    g = torch.Generator().manual_seed(977 + seed)
    wide = torch.randint(-3, 4, (t.shape[0], t.shape[1] + pad), generator=g).to(t.dtype)
    wide[:, :t.shape[1]] = t
    return wide


def ld_ignored(wide: torch.Tensor, cols: int) -> torch.Tensor:
    """What a kernel reads that takes the row length for the row stride."""
    return wide.flatten()[:wide.shape[0] * cols].view(wide.shape[0], cols)


# ============================================================================== fused epilogues
def qkv_rope_ref(x, w, S: int, cos, sin, family: str, defect: Optional[str] = None) -> Checked:
    """qkv [M, 3H] = x w^T rounded to bf16, then NeoX RoPE (head_dim 64) on the q and k heads at
    position m % S: x1' = x1 c - x2 s, x2' = x2 c + x1 s."""
    M, N = x.shape[0], w.shape[0]
    H = N // 3
    y, pre = product_ref(x, w, family)
    yb = round_to(y, BF).double()
    e = flip(y, pre, BF) if family != "int" else torch.zeros_like(y)
    pos = torch.arange(M) if defect == "rope_pos_m" else torch.arange(M) % S
    tab = lambda t: t.double()[pos].view(M, 1, 32)
    c, s = tab(cos), tab(sin)
    if defect == "rope_sign":
        s = -s
    heads = N // 64 if defect == "rope_on_v" else 2 * H // 64
    yh, eh = yb.view(M, N // 64, 64), e.view(M, N // 64, 64)
    x1, x2, e1, e2 = yh[:, :heads, :32], yh[:, :heads, 32:], eh[:, :heads, :32], eh[:, :heads, 32:]
    out, tol = yh.clone(), eh.clone()
    out[:, :heads, :32], out[:, :heads, 32:] = x1 * c - x2 * s, x2 * c + x1 * s
    nrot = 2 * H // 64  # the tolerance is the unmodified reference's
    pos = torch.arange(M) % S
    c0, s0 = tab(cos).abs(), tab(sin).abs()
    a1, a2, f1, f2 = yh[:, :nrot, :32].abs(), yh[:, :nrot, 32:].abs(), eh[:, :nrot, :32], eh[:, :nrot, 32:]
    # the intermediate's error through the rotation; a product and an fma (two roundings)
    tol[:, :nrot, :32] = f1 * c0 + f2 * s0 + 2 * U23 * (a1 * c0 + a2 * s0)
    tol[:, :nrot, 32:] = f2 * c0 + f1 * s0 + 2 * U23 * (a2 * c0 + a1 * s0)
    out, tol = out.view(M, N), tol.view(M, N)
    full = tol + final_rounding(out, tol, BF)
    if family == "int":  # the v heads are the product alone: exact
        vcols = torch.arange(N) >= 2 * H
        full = torch.where(vcols.view(1, N), torch.zeros_like(full), full)
    return Checked(out, full)


class GuS(NamedTuple):
    gu: Checked  # [M, 2I]
    s: Checked   # [M, I]


def _s_of(g, u, eg, eu, dt):
    """s = silu(g) u from the rounded g, u (errors eg, eu): |d silu / dg| <= 1.0999 and d / du =
    silu(g); the sigmoid, two products, the flushed exponential; the final rounding."""
    sg = sigmoid(g)
    s = g * sg * u
    pre = 1.1 * eg * (u.abs() + eu) + (g * sg).abs() * eu + s.abs() * (eps_sig(g) + 2 * U23) + EXP_FLUSH * (g * u).abs()
    return Checked(s, pre + final_rounding(s, pre, dt))


def gu_swiglu_ref(x, w, family: str, defect: Optional[str] = None) -> GuS:
    """gu = x w^T (gate rows [0, I), up rows [I, 2I)) and s = silu(g) u from the ROUNDED g, u."""
    dt = x.dtype
    I = w.shape[0] // 2
    y, pre = product_ref(x, w, family)
    gu = _store(y, pre, dt, family)
    e = flip(y, pre, dt) if family != "int" else torch.zeros_like(y)
    yb = y if defect == "s_unrounded" else round_to(y, dt).double()
    g, u, eg, eu = yb[:, :I], yb[:, I:], e[:, :I], e[:, I:]
    if defect == "gu_swapped":
        g, u = u, g
    s = _s_of(g, u, eg, eu, dt)
    if defect is not None:
        clean = gu_swiglu_ref(x, w, family)
        return GuS(gu, Checked(s.ref, clean.s.tol))
    return GuS(gu, s)


class DownBwd(NamedTuple):
    dgu: Checked    # [M, 2I]
    s: Checked      # [M, I]


def down_swiglu_bwd_ref(dd, wdown, gu, family: str, defect: Optional[str] = None) -> DownBwd:
    """ds = dd wdown [M, I] rounded to the activation format, then k_swiglu_bwd's formula on the
    kept gu = [g | u]: dg = ds u sig (1 + g (1 - sig)), du = ds g sig; s_out = g sig u."""
    dt = dd.dtype
    I = wdown.shape[1]
    y, pre = product_ref(dd, wdown.t(), family, defect)
    d = round_to(y, dt).double()
    ed = flip(y, pre, dt) if family != "int" else torch.zeros_like(y)
    g, u = gu.double()[:, :I], gu.double()[:, I:]
    if defect == "gu_swapped":
        g, u = u, g
    sg = sigmoid(g)
    w_ = 1.0 + g * (1.0 - sg)
    dg, du = d * u * sg * w_, d * g * sg
    es = eps_sig(g)
    # ds's error through the factor; 1 - sig (sig's error, the difference), g times it, the add of 1;
    # sig's error on the factor and four products
    dg_pre = ((u * sg * w_).abs() * ed + (d * u * sg).abs() * (g.abs() * (sg * es + 2 * U23) + U23 * w_.abs())
              + dg.abs() * (es + 4 * U23) + EXP_FLUSH * (d * u * g).abs())
    du_pre = (g * sg).abs() * ed + du.abs() * (es + 2 * U23) + EXP_FLUSH * (d * g).abs()
    ref, pr = torch.cat([dg, du], 1), torch.cat([dg_pre, du_pre], 1)
    zero = torch.zeros_like(g)
    return DownBwd(Checked(ref, pr + final_rounding(ref, pr, dt)), _s_of(g, u, zero, zero, dt))


# ============================================================================ weight gradients
def split_pairs(T: int, splits: int):
    """k_gemm_wgrad: the 128-token pair range [p0, p1) of each split."""
    npair = T // 128
    return [((s * npair) // splits, ((s + 1) * npair) // splits) for s in range(splits)]


def wgrad_bn(Nc: int) -> int:
    """gw_bn of gemm_wgrad.hip."""
    return 192 if Nc % 192 == 0 else (128 if Nc % 128 == 0 else 0)


def wgrad_splits(T: int, Nr: int, Nc: int, splits: int = 0, target: int = 256) -> int:
    """The splits gemm_wgrad launches: wgrad_splits() of ops/hip.py for 0, clamped to the pairs."""
    if splits <= 0:
        tiles = ((Nr + 255) // 256) * (Nc // wgrad_bn(Nc))
        splits = max(1, min(T // 128, (target + tiles // 2) // tiles))
    return min(splits, T // 128)


class SkPlan(NamedTuple):
    npair: int
    nrt: int
    Wc: int
    Gc: int
    maxseg: int
    ntc: int


def sk_plan(T: int, Nr: int, Nc: int, shares: int = 0) -> SkPlan:
    """gw_sk_plan of gemm_wgrad.hip."""
    npair, nrt = T // 128, (Nr + 255) // 256
    Wc, ntc = nrt * npair, Nc // wgrad_bn(Nc)
    Gc = shares if shares > 0 else 256 // ntc
    Gc = max(1, min(Gc, Wc))
    share = -(-Wc // Gc)
    return SkPlan(npair, nrt, Wc, Gc, -(-share // npair) + 1, ntc)


def sk_segments(pl: SkPlan):
    """Per share g: its segments (row tile, p0, p1, whole) as gw_sk_share runs them."""
    out = []
    for g in range(pl.Gc):
        i, e, segs = g * pl.Wc // pl.Gc, (g + 1) * pl.Wc // pl.Gc, []
        while i < e:
            rt, p0 = divmod(i, pl.npair)
            p1 = min(pl.npair, p0 + (e - i))
            segs.append((rt, p0, p1, p0 == 0 and p1 == pl.npair))
            i += p1 - p0
        out.append(segs)
    return out


SK_KINDS = ("whole-tiles", "crosses-row-tile", "ends-on-edge", "shares==Wc")


def sk_kinds(pl: SkPlan) -> set:
    """Which of SK_KINDS a plan shows: every share whole tiles; a share with segments in two row
    tiles; a partial share that ends exactly on a tile edge; one iteration per share."""
    segs, k = sk_segments(pl), set()
    if all(s[3] for sh in segs for s in sh):
        k.add("whole-tiles")
    if any(len({s[0] for s in sh}) > 1 and not all(s[3] for s in sh) for sh in segs):
        k.add("crosses-row-tile")
    if any(sh[-1][2] == pl.npair and not sh[-1][3] for sh in segs):
        k.add("ends-on-edge")
    if pl.Gc == pl.Wc:
        k.add("shares==Wc")
    return k


def wgrad_ref(dy, x, base, family: str, parts: int = 1, defect: Optional[str] = None, splits: int = 1,
              plan: Optional[SkPlan] = None) -> Checked:
    """dW = base + dy^T x (dy [T, Nr], x [T, Nc], base fp32 [Nr, Nc]).  ``parts``: additions onto
    dW after the chains (splits, or the shares of stream-K), for the tolerance."""
    T, Nr = dy.shape
    Nc = x.shape[1]
    yd, xd, b = dy.double(), x.double(), base.double()
    acc = yd.t() @ xd
    pair = lambda p: yd[p * 128:(p + 1) * 128].t() @ xd[p * 128:(p + 1) * 128]
    if defect in ("split_pair_dropped", "split_pair_doubled"):  # the pair where split 0 ends
        p1 = split_pairs(T, splits)[0][1]
        acc = acc + pair(p1 - 1) * (-1.0 if defect == "split_pair_dropped" else 1.0)
    if defect == "sk_drop_share":  # the fix-up leaves out the second share of the first split tile (column tile 0)
        segs = sk_segments(plan)
        rt = next(s[0] for sh in segs for s in sh if not s[3])
        part = [s for sh in segs for s in sh if s[0] == rt and not s[3]][1]
        bn = wgrad_bn(Nc)
        lost = sum(pair(p) for p in range(part[1], part[2]))
        acc = acc.clone()
        acc[rt * 256:rt * 256 + 256, :bn] -= lost[rt * 256:rt * 256 + 256, :bn]
    ref = acc + b
    if defect == "ignore_base":
        ref = acc
    if defect == "base_twice":
        ref = acc + 2 * b
    if defect == "skip_half_row_tile":
        ref = ref.clone()
        ref[Nr - 128:] = b[Nr - 128:]
    if family == "int":
        return Checked(ref, torch.zeros_like(ref))
    # the chains over T terms in all, then ``parts`` additions onto dW
    return Checked(ref, (chain(T) + parts * U23) * (yd.abs().t() @ xd.abs() + b.abs()))


def wgrad_parts_ref(dy, x, family: str, splits: int) -> Checked:
    """part [splits, Nr, Nc] of the partials-only mode: split s holds the product over its pairs."""
    outs, tols = [], []
    for p0, p1 in split_pairs(dy.shape[0], splits):
        sl = slice(p0 * 128, p1 * 128)
        c = wgrad_ref(dy[sl], x[sl], torch.zeros(dy.shape[1], x.shape[1]), family, parts=0)
        outs.append(c.ref)
        tols.append(c.tol)
    return Checked(torch.stack(outs), torch.stack(tols))


def splitk_ref(part, base, family: str = "gauss") -> Checked:
    """k_splitk_acc: base + sum_s part[s], added one after the other."""
    p = part.double()
    ref = base.double() + p.sum(0)
    if family == "int":
        return Checked(ref, torch.zeros_like(ref))
    return Checked(ref, part.shape[0] * U23 * (base.double().abs() + p.abs().sum(0)))


@functools.lru_cache(maxsize=None)
def tie_partials(dt, n: int = 1024):
    """fp32 partials [3, n] whose sum is exact in fp32 and lies exactly half way between two
    values of ``dt``, at both parities and both signs, plus the neighbours one fp32 ulp to either
    side: k_splitk_sum_bf16 must round them to nearest even."""
    ulp = 2.0 ** -7 if dt == BF else 2.0 ** -10
    k = torch.arange(n, dtype=F64)
    v = (1.0 + (k % 64) * ulp) * torch.where(k % 2 == 0, 1.0, -1.0)
    nudge = torch.tensor([0.0, 2.0 ** -23, -2.0 ** -23], dtype=F64)[(k.long() // 64) % 3]
    half = torch.sign(v) * (ulp / 2 + nudge)
    part = torch.stack([v, half, torch.zeros_like(v)]).to(F32)
    assert torch.equal(part.double().sum(0).to(F32).double(), part.double().sum(0))
    return part


# ======================================================================= dispatch model
GB_DEFAULT_FLAGS = 2048 | 1024 | 12


def gb_flag_sets(late: bool = False):
    """The flag sets the project ships for k_gemm_bf16 (ops/hip.py): the production default, the
    default without the LDS-transposed stores, without the write-through stores, bounded
    persistence with one and two tiles per workgroup; 4096 (epilogue-first staging) for the two
    LATE forms."""
    d = GB_DEFAULT_FLAGS
    out = [d, d & ~1024, d & ~2048, d | 256 | (1 << 24), d | 256 | (2 << 24)]
    return out + ([d | 4096] if late else [])


def gb_launch_grid(ntiles: int, flags: int) -> int:
    """gb_launch_grid of gemm_bf16.hip (the cap sits in flags bits 16-23, in units of 8)."""
    if flags & 256:
        t = ((flags >> 24) & 15) or 1
        return ((ntiles + t - 1) // t + 7) & ~7
    g = (min(ntiles, 256) + 7) & ~7
    cap = 8 * ((flags >> 16) & 0xff)
    return cap if cap and cap < g else g


def gb_bn(N: int) -> int:
    return 192 if N % 192 == 0 else (128 if N % 128 == 0 else 0)


def gb_walk(M: int, N: int, flags: int, cap: int = 0, bn: Optional[int] = None, ts: Optional[int] = None):
    """(mode, per-workgroup lists of (tile row, tile column)) of k_gemm_bf16's tile walk.
    mode: xband | grouped | row-major.  ``ts``: tile stride in B rows (96 for the SwiGLU forward)."""
    bn = bn or gb_bn(N)
    ntn, ntm = N // (ts or bn), M // BM
    ntiles = ntm * ntn
    fl = flags | ((cap // 8) << 16)
    G = gb_launch_grid(ntiles, fl)
    gx, order = G >> 3, (flags >> 2) & 3
    xband = order == 3 and ntm % 8 == 0 and gx % (ntm >> 3) == 0
    band = (ntm >> 3) * ntn if xband else 0
    gn = 8 if ntn % 8 == 0 else 4 if ntn % 4 == 0 else 2 if ntn % 2 == 0 else 1
    gm = 32 // gn
    grouped = order != 1 and gx == 32 and ntiles % 32 == 0 and ntm % gm == 0
    scols, srows = ntn // gn, ntm // gm

    def coords(L):
        if xband:
            rpx, x = ntm >> 3, L // band
            j = L - x * band
            return x * rpx + j % rpx, j // rpx
        if grouped:
            sidx, i = L >> 5, L & 31
            if order == 2:
                return (sidx // scols) * gm + i // gn, (sidx % scols) * gn + i % gn
            return (sidx % srows) * gm + i // gn, (sidx // srows) * gn + i % gn
        return L // ntn, L % ntn

    wgs = []
    for bid in range(G):
        tend = ((bid & 7) + 1) * band if xband else ntiles
        tiles, r = [], 0
        while True:
            L = (bid & 7) * band + r * gx + (bid >> 3) if xband else r * G + (bid & 7) * gx + (bid >> 3)
            if L >= tend:
                break
            tiles.append(coords(L))
            r += 1
        wgs.append(tiles)
    return ("xband" if xband else "grouped" if grouped else "row-major"), wgs


GB_MODES = ("xband", "grouped", "row-major")
GB_WALK_TAGS = ("idle-workgroup", "one-pass", "two-tiles", "uneven-rounds", "bounded", "capped")


def gb_tags(M: int, N: int, K: int, flags: int, cap: int = 0, ts: Optional[int] = None) -> set:
    mode, wgs = gb_walk(M, N, flags, cap, ts=ts)
    n = [len(w) for w in wgs]
    t = {mode, f"bn{gb_bn(N)}"}
    if 0 in n:
        t.add("idle-workgroup")
    if K == 2 * BK:
        t.add("one-pass")
    if max(n) >= 2:
        t.add("two-tiles")
    if len({x for x in n if x}) > 1:
        t.add("uneven-rounds")
    if flags & 256:
        t.add("bounded")
    elif cap and max(n) >= 2:
        t.add("capped")
    return t


def walk_covers(M: int, N: int, wgs, bn: int) -> bool:
    """Every tile exactly once."""
    seen = sorted(t for w in wgs for t in w)
    return seen == [(a, b) for a in range(M // BM) for b in range(N // bn)]


def fw4_plan(M: int, N: int, flags: int):
    """(tiles per workgroup, tile order, ragged, stages) of dlt_gemm_fw4, or None where it refuses."""
    sb = flags & (16 | 128)
    if M <= 0 or M % 256 or N % 128 or sb in (16, 128):
        return None
    ntm, ntn = M // 256, (N + 255) // 256
    tiles = ntm * ntn
    if flags & 4096 and (tiles % 16 or flags & 1024):
        return None
    order = "half-band" if ntm % 16 == 0 and flags & 2048 else "band" if ntm % 8 == 0 and not flags & 2 else "row-major"
    return (2 if flags & 4096 else 1), order, N % 256 == 128, (5 if sb else 4)


FW4_FLAGS = (1, 0, 4, 2, 2048, 144, 145, 148, 146)  # test_gemm_fw4's list
FW4_TWO = (4096, 4100, 4240, 4244, 6148)            # two tiles per workgroup (tiles % 16 == 0)
FW4_SWIGLU_FLAGS = (0, 4, 1, 144, 150, 2048)


def fw4_walk(M: int, N: int, flags: int):
    """Per-workgroup (tile row, tile column) lists of k_gemm_fw4 (256-column tiles)."""
    T, order, _, _ = fw4_plan(M, N, flags)
    ntm, ntn = M // 256, (N + 255) // 256
    out = []
    for b in range(ntm * ntn // T):
        w = []
        for j in range(T):
            x, jj = b & 7, (b >> 3) * T + j
            if order == "half-band":
                R = ntm >> 4
                per = R * ntn
                band, k = (x, jj) if jj < per else (x + 8, jj - per)
                w.append((band * R + k % R, k // R))
            elif order == "band":
                R = ntm >> 3
                w.append((x * R + jj % R, jj // R))
            else:
                w.append(divmod(b * T + j, ntn))
        out.append(w)
    return out


# ================================================================================= cases
class Gemm(NamedTuple):
    kernel: str      # gemm_bf16 | gemm_dgrad | gemm_fw4
    dt: torch.dtype
    M: int
    N: int
    K: int
    family: str
    cap: int = 0     # gemm_grid_cap for the k_gemm_bf16 forms

    @property
    def name(self):
        return f"{self.kernel}-{DT_NAME[self.dt]}-{self.M}x{self.N}x{self.K}-{self.family}-cap{self.cap}"


# (M, N, K, cap): one tile on a grid of 8 with a single loop pass; the 128-column tile; 12 tiles on
# 8 workgroups; XCD row bands in two rounds; the grouped super-tile walk (ntm 24, 384 tiles on 256
# workgroups); and the 128-column forms of the multi-tile walks
GB_SHAPES = ((256, 192, 128, 0), (256, 128, 256, 0), (768, 768, 256, 8), (2048, 384, 128, 8), (6144, 3072, 128, 0),
             (768, 512, 256, 8), (2048, 256, 128, 8))
GB_BIG = (6144, 3072, 128, 0)


def _gb_cases():
    """Every shape for both kernels, both formats, gauss and int; cancel on one shape per kernel."""
    out = [Gemm(kern, dt, *sh[:3], fam, sh[3]) for sh in GB_SHAPES for kern in ("gemm_bf16", "gemm_dgrad")
           for dt in DTYPES for fam in ("gauss", "int")]
    return out + [Gemm("gemm_bf16", BF, 768, 768, 256, "cancel", 8), Gemm("gemm_dgrad", HF, 768, 768, 256, "cancel", 8)]


GB_CASES = _gb_cases()
# 256 x 128 x 128; a ragged last tile and three stages; two column tiles; 16 tiles (two per workgroup);
# 16 tile rows (the half-height XCD bands of flag 2048)
FW4_SHAPES = ((256, 128, 128), (256, 384, 192), (512, 256, 128), (2048, 512, 128), (4096, 128, 128))
FW4_CASES = [Gemm("gemm_fw4", dt, *sh, fam) for sh in FW4_SHAPES for dt in DTYPES for fam in ("gauss", "int")] + \
    [Gemm("gemm_fw4", BF, 256, 384, 192, "cancel")]
# the leading-dimension cases: (kernel, dtype, M, N, K, pad)
LD_CASES = [Gemm("gemm_bf16", BF, 256, 192, 128, "int", 8), Gemm("gemm_bf16", HF, 512, 128, 256, "gauss", 72),
            Gemm("gemm_dgrad", HF, 256, 192, 128, "int", 72), Gemm("gemm_dgrad", BF, 512, 128, 256, "gauss", 8)]


def _seed(*xs) -> int:
    return sum((i + 1) * 7919 * int(x) for i, x in enumerate(xs)) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def _gemm_problem(M: int, N: int, K: int, dt, family: str):
    P, Q = operands(_seed(M, N, K, DTYPES.index(dt)), M, N, K, family, dt)
    return P, Q, gemm_ref(P, Q, family)


def gemm_case(c: Gemm):
    """(P, Q, Checked): P [M, K], Q [N, K]; the kernels take (a, b) = (P, Q) or (dy, w) = (P, Q^T).
    The kernels of one shape, format and family share the problem and its reference."""
    return _gemm_problem(c.M, c.N, c.K, c.dt, c.family)


class Fused(NamedTuple):
    kernel: str      # qkv_rope | gu_swiglu | fw4_swiglu | down_swiglu_bwd
    dt: torch.dtype
    M: int
    a: int           # qkv_rope: nh; swiglu: I; down: I
    K: int           # reduction (down: H)
    family: str
    S: int = 0       # qkv_rope: sequence length

    @property
    def name(self):
        return f"{self.kernel}-{DT_NAME[self.dt]}-M{self.M}-{self.a}-K{self.K}-S{self.S}-{self.family}"


ROPE_CASES = [Fused("qkv_rope", BF, M, nh, 128, fam, 128) for M, nh in ((256, 1), (512, 3), (256, 4))
              for fam in ("gauss", "int")] + [Fused("qkv_rope", BF, 512, 4, 256, "cancel", 128)]
GU_CASES = [Fused("gu_swiglu", BF, 256, I, 128, fam) for I in (96, 192) for fam in ("gauss", "int")] + \
    [Fused("gu_swiglu", BF, 256, 96, 256, "cancel")]
FW4_SW_CASES = [Fused("fw4_swiglu", dt, M, I, K, fam) for dt in DTYPES for M, I, K in ((256, 128, 128), (256, 256, 192), (512, 128, 128))
                for fam in ("gauss", "int")] + [Fused("fw4_swiglu", HF, 256, 128, 256, "cancel")]
DOWN_CASES = [Fused("down_swiglu_bwd", dt, 256, 192, H, fam) for dt in DTYPES for H in (128, 256)
              for fam in ("gauss", "int")] + [Fused("down_swiglu_bwd", BF, 512, 192, 256, "cancel")]


@functools.lru_cache(maxsize=None)
def fused_case(c: Fused):
    """Inputs and references of a fused-epilogue case.  Weights are scaled by 1 / sqrt(K) on
    gauss so that g and u are of order one; the int family keeps its integers."""
    sd = _seed(c.M, c.a, c.K, DTYPES.index(c.dt), len(c.kernel))
    qs = 1.0 / math.sqrt(c.K)
    if c.kernel == "qkv_rope":
        x, w = operands(sd, c.M, 3 * c.a * 64, c.K, c.family, c.dt, qs)
        cos, sin = opsref.rope_tables(64, c.M)  # longer than S: a kernel that takes position m reads other rows
        return (x, w, cos.contiguous(), sin.contiguous()), qkv_rope_ref(x, w, c.S, cos, sin, c.family)
    if c.kernel in ("gu_swiglu", "fw4_swiglu"):
        x, w = operands(sd, c.M, 2 * c.a, c.K, c.family, c.dt, qs)
        return (x, w), gu_swiglu_ref(x, w, c.family)
    dd, wt = operands(sd, c.M, c.a, c.K, c.family, c.dt, qs)
    g = torch.Generator().manual_seed(sd + 1)
    gu = (torch.randn(c.M, 2 * c.a, generator=g, dtype=F64) * 2).to(F32).to(c.dt)
    wd = wt.t().contiguous()
    return (dd, wd, gu), down_swiglu_bwd_ref(dd, wd, gu, c.family)


class Wgrad(NamedTuple):
    dt: torch.dtype
    T: int
    Nr: int
    Nc: int
    splits: int      # as passed to gemm_wgrad (0: the wrapper's choice); stream-K: the shares
    family: str
    sk: bool = False

    @property
    def name(self):
        return f"{'wgrad_sk' if self.sk else 'wgrad'}-{DT_NAME[self.dt]}-T{self.T}-{self.Nr}x{self.Nc}-s{self.splits}-{self.family}"


# (T, Nr, Nc, splits): one pair (splits clamp to 1); one and two splits; uneven pair ranges;
# the wrapper's choice; the half row tile alone; one and a half row tiles; two; the 128-column tile;
# two column tiles of 192 and of 128
WG_SHAPES = ((128, 256, 192, 4), (256, 256, 192, 1), (256, 256, 192, 2), (384, 256, 192, 2), (640, 256, 192, 0),
             (256, 128, 192, 2), (256, 384, 192, 1), (256, 512, 128, 2), (256, 256, 384, 2), (256, 384, 256, 1))
WG_CASES = [Wgrad(dt, *sh, fam) for sh in WG_SHAPES for dt in DTYPES for fam in ("gauss", "int")] + \
    [Wgrad(BF, 384, 256, 192, 2, "cancel")]
# stream-K (T, Nr, Nc, shares): (a) whole tiles only; (b) a share crossing a row tile; (c) a partial
# share ending on a tile edge; (d) one iteration per share
SK_SHAPES = ((256, 512, 192, 2), (384, 384, 192, 3), (256, 384, 192, 3), (384, 512, 128, 3), (256, 384, 192, 4),
             (384, 384, 384, 5))
SK_CASES = [Wgrad(dt, *sh, fam, True) for sh in SK_SHAPES for dt in DTYPES for fam in ("gauss", "int")] + \
    [Wgrad(HF, 384, 384, 192, 3, "cancel", True)]


@functools.lru_cache(maxsize=None)
def wgrad_inputs(c: Wgrad):
    """(dy [T, Nr], x [T, Nc], base fp32 [Nr, Nc])."""
    sd = _seed(c.T, c.Nr, c.Nc, DTYPES.index(c.dt), int(c.sk))
    P, Q = operands(sd, c.Nr, c.Nc, c.T, c.family, c.dt)
    g = torch.Generator().manual_seed(sd + 2)
    if c.family == "int":
        base = torch.randint(-INT_BASE, INT_BASE + 1, (c.Nr, c.Nc), generator=g).to(F32)
    else:
        base = torch.randn(c.Nr, c.Nc, generator=g, dtype=F32) * 4
    return P.t().contiguous(), Q.t().contiguous(), base


@functools.lru_cache(maxsize=None)
def wgrad_case(c: Wgrad):
    dy, x, base = wgrad_inputs(c)
    if c.sk:
        pl = sk_plan(c.T, c.Nr, c.Nc, c.splits)
        return dy, x, base, wgrad_ref(dy, x, base, c.family, parts=pl.Gc + 1, plan=pl)
    s = wgrad_splits(c.T, c.Nr, c.Nc, c.splits)
    return dy, x, base, wgrad_ref(dy, x, base, c.family, parts=s + 1, splits=s)


@functools.lru_cache(maxsize=None)
def ld_case(c: Gemm):
    """A leading-dimension case (``cap`` holds the padding): the operands as the first columns of
    wider tensors.  gemm_bf16: (A [M, K + pad], B [N, K + pad]); gemm_dgrad: (dY [M, Nred + pad],
    W [Nred, Nout + pad]).  Returns (wide a, wide b, Checked)."""
    P, Q, chk = gemm_case(c._replace(cap=0))
    if c.kernel == "gemm_dgrad":
        return strided(P, c.cap, 1), strided(Q.t().contiguous(), c.cap, 2), chk
    return strided(P, c.cap, 1), strided(Q, c.cap, 2), chk


def ld_defect_ref(c: Gemm) -> Checked:
    """The leading dimension ignored: rows taken at the row length."""
    a, b, _ = ld_case(c)
    if c.kernel == "gemm_dgrad":
        return gemm_ref(ld_ignored(a, c.K), ld_ignored(b, c.N).t(), c.family)
    return gemm_ref(ld_ignored(a, c.K), ld_ignored(b, c.K), c.family)


# defect -> (the case that shows it, the outputs it must push outside the tolerance)
def _find(cases, **kw):
    """The first case of a GPU list with these fields: the defects are shown on the GPU file's own cases."""
    return next(c for c in cases if all(getattr(c, k) == v for k, v in kw.items()))


DEFECT_CASES = {
    "drop_last_ktile": (_find(GB_CASES, kernel="gemm_bf16", N=128, K=256, family="gauss"), ("c",)),
    "drop_ktile1": (_find(GB_CASES, kernel="gemm_dgrad", N=128, K=256, family="gauss"), ("c",)),
    "second_tile_first_operands": (_find(GB_CASES, kernel="gemm_bf16", M=768, N=768, family="int"), ("c",)),
    "swap_tile_rc": (_find(GB_CASES, kernel="gemm_dgrad", M=768, N=768, family="gauss"), ("c",)),
    "skip_half_row_tile": (_find(WG_CASES, Nr=384, Nc=192, family="gauss"), ("dw",)),
    "skip_ragged_half": (_find(FW4_CASES, N=384, family="gauss"), ("c",)),
    "split_pair_dropped": (_find(WG_CASES, T=384, family="gauss"), ("dw",)),
    "split_pair_doubled": (_find(WG_CASES, T=384, family="int"), ("dw",)),
    "sk_drop_share": (_find(SK_CASES, T=384, Nr=384, Nc=192, family="gauss"), ("dw",)),
    "ignore_base": (_find(WG_CASES, T=256, Nr=256, Nc=192, splits=1, family="gauss"), ("dw",)),
    "base_twice": (_find(WG_CASES, T=256, Nr=256, Nc=192, splits=2, family="gauss"), ("dw",)),
    "rope_sign": (_find(ROPE_CASES, a=3, family="gauss"), ("qkv",)),
    "rope_pos_m": (_find(ROPE_CASES, a=1, family="gauss"), ("qkv",)),
    "rope_on_v": (_find(ROPE_CASES, a=4, family="gauss"), ("qkv",)),
    "gu_swapped": (_find(GU_CASES, a=96, family="gauss"), ("s",)),
    "gu_swapped@down": (_find(DOWN_CASES, K=128, family="gauss"), ("dgu", "s")),
    "s_unrounded": (_find(FW4_SW_CASES, a=256, family="gauss"), ("s",)),
    "ld_ignored": (LD_CASES[0], ("c",)),
    "ld_ignored@dgrad": (LD_CASES[3], ("c",)),
}
TRUNC_CASES = (_find(GB_CASES, kernel="gemm_bf16", dt=BF, M=768, N=768, family="gauss"),
               _find(FW4_CASES, dt=HF, M=512, family="gauss"))
