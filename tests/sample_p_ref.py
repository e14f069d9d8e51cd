"""fp64 reference, derived decision bands and fixed inputs for nucleus (top-p) and min-p
sampling (``dec_sample(..., top_p=, min_p=)`` in ``ops/csrc/decode.hip`` and the host helper
``eval.decode.filter_logits``), shared by test_sample_p_cpu.py and test_sample_p_gpu.py.

The definition (one for every path).  x = logits / T in fp32 (the kernel's own division),
then everything in fp64 on those fp32 values.  The kept set is an intersection of
"value >= a threshold" sets:
  top-k  x >= the k-th largest (ties kept; top_k <= 0 or >= V: off);
  top-p  over the top-k set K, with Z = sum_K exp(x - max): v is kept iff
         mass_above(v) / Z < top_p, mass_above(v) the mass of the values of K STRICTLY
         greater than v (the value that crosses top_p is kept, the largest always is, equal
         values stand or fall together; top_p == 1: off);
  min-p  exp(v - max) >= min_p (min_p == 0: off).
top_p and min_p are rounded to fp32 first: that is what the binding hands to the kernel.

Every token is classified ``must_keep``, ``must_drop`` or ``either``; ``either`` holds the
tokens whose decision lies within the kernel's own rounding of a boundary:
  top-p  |mass_above / Z - top_p| <= delta_p        (:func:`delta_p`)
  min-p  |exp(v - max) / min_p - 1| <= delta_m      (:func:`delta_m`)
  top-k  exact (keys are compared as integers): no band.
Every input builder below asserts that its ``either`` set is EMPTY, so the GPU support check
("every id in must_keep") is an exact statement and cannot hide a failure.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np
import torch

U24 = 2.0 ** -24   # half an fp32 ulp, relative
FIX = 2.0 ** -40   # one unit of the kernel's fixed-point mass (exp(0) = 2^40 units)


def f32(v: float) -> float:
    return float(np.float32(v))


def scaled(logits: torch.Tensor, T: float) -> np.ndarray:
    """x = logits / T as the kernel forms it (an fp32 division), [B, V] float32."""
    return (logits.detach().cpu().float() / torch.tensor(T, dtype=torch.float32)).numpy()


# ----------------------------------------------------------------------------- the bands
def exp_rel_err(d: np.ndarray) -> np.ndarray:
    """Relative error bound of the kernel's __expf(x - max) at d = max - x >= 0, named terms:
      arg   the fp32 subtraction x - max rounds to half an ulp, |d| * 2^-24 absolute in the
            argument = relative in the exponential;
      mul   __expf is exp2(fl(a * log2 e)): that product rounds once more, another |d| * 2^-24;
      exp2  the hardware exp2 is good to one fp32 ulp, 2^-23; 2^-22 leaves a factor 2."""
    arg = d * U24
    mul = d * U24
    exp2 = 2.0 ** -22
    return arg + mul + exp2


def delta_p(x: np.ndarray, inK: np.ndarray) -> float:
    """Half-width of the top-p ``either`` band of one row, in units of mass_above / Z.

    The kernel decides A' < ceil(fl64(top_p * Z')) with A', Z' integer sums of
    floor(2^40 * e'_i), e'_i = __expf(x_i - max) = e_i (1 + eps_i):
      exp    |A' - A| and |Z' - Z| are each <= E = sum_K e_i * exp_rel_err(d_i), and
             A/Z moves by at most (|dA| + (A/Z) |dZ|) / Z <= 2 E / Z;
      floor  each floor() loses < 1 unit of 2^-40, at most V of them in A' and in Z':
             the issue's V * 2^-40 / Z, for both sums 2 * V * 2^-40 / Z (a value whose
             exponential underflows in fp32 has e_i < 2^-126 and sits inside this term);
      t_z    top_p * Z' is one fp64 product of (double)Z' (Z' < 2^57 here: one rounding):
             2 * 2^-53 relative, and the ceil moves T by < 1 unit: 2^-40 / Z;
      div    the kernel forms no quotient (the descent compares integer masses): 0.
    top_p itself is the fp32 value on both sides: no term."""
    mx = x[inK].max()
    d = mx - x[inK]
    e = np.exp(-d)
    Z = e.sum()
    exp = 2.0 * float((e * exp_rel_err(d)).sum()) / Z
    floor = 2.0 * x.size * FIX / Z
    t_z = 2.0 ** -52 + FIX / Z
    div = 0.0
    return exp + floor + t_z + div


def delta_m(mx: float, min_p: float) -> float:
    """Half-width of the min-p ``either`` band, in units of exp(v - max) / min_p - 1.

    The kernel keeps v >= c with c = fl(max + logf(min_p)), the real boundary being
    max + ln(min_p); an absolute error dc of c scales the ratio by exp(dc) ~ 1 + dc:
      log   logf is good to an ulp of |ln min_p|; 2^-22 |ln min_p| leaves a factor 2;
      add   the fp32 sum rounds to half an ulp of |c| <= |max| + |ln min_p|;
      x1.01 the second order of exp(dc) - 1 for dc < 0.02.
    The host helper computes the same sum in fp32 with a correctly rounded log: inside it."""
    ln = abs(math.log(min_p))
    log = 2.0 ** -22 * ln
    add = (abs(mx) + ln) * U24
    return 1.01 * (log + add)


# ------------------------------------------------------------------------- the reference
class Classes(NamedTuple):
    must_keep: torch.Tensor  # [B, V] bool
    must_drop: torch.Tensor
    either: torch.Tensor
    probs: torch.Tensor      # [B, V] fp64: softmax of x over must_keep


def mass_above(x: np.ndarray, e: np.ndarray) -> np.ndarray:
    """Per element, the sum of e over the elements with x strictly greater (fp64)."""
    order = np.argsort(-x, kind="stable")
    xs, es = x[order], e[order]
    excl = np.cumsum(es) - es
    first = np.searchsorted(-xs, -xs, side="left")  # the first of each run of equal values
    out = np.empty_like(e)
    out[order] = excl[first]
    return out


def topk_set(x: np.ndarray, top_k: int) -> np.ndarray:
    inK = np.isfinite(x)
    if 0 < top_k < x.size:
        inK &= x >= np.sort(x)[::-1][top_k - 1]
    return inK


def classify(logits: torch.Tensor, T: float, top_k: int, top_p: float, min_p: float) -> Classes:
    xs = scaled(logits, T)
    top_p, min_p = f32(top_p), f32(min_p)
    keep, drop, probs = np.zeros(xs.shape, bool), np.zeros(xs.shape, bool), np.zeros(xs.shape)
    for b, x32 in enumerate(xs):
        x = x32.astype(np.float64)
        inK = topk_set(x, top_k)
        if not inK.any():  # a row without a finite value: nothing to classify
            drop[b] = True
            continue
        mx = x[inK].max()
        with np.errstate(invalid="ignore"):
            e_all = np.where(np.isfinite(x), np.exp(x - mx), 0.0)
        e = np.where(inK, e_all, 0.0)
        k, dr = inK.copy(), ~inK
        if top_p < 1.0:
            r = mass_above(x, e) / e.sum()
            dp = delta_p(x, inK)
            k &= r < top_p - dp
            dr |= r > top_p + dp
        if min_p > 0.0:
            q = e_all / min_p - 1.0
            dm = delta_m(mx, min_p)
            k &= q > dm
            dr |= q < -dm
        keep[b], drop[b] = k, dr
        pk = np.where(k, e, 0.0)
        probs[b] = pk / max(pk.sum(), 1e-300)
    keep_t, drop_t = torch.from_numpy(keep), torch.from_numpy(drop)
    return Classes(keep_t, drop_t, ~(keep_t | drop_t), torch.from_numpy(probs))


def brute_force(x32: np.ndarray, top_k: int, top_p: float, min_p: float) -> np.ndarray:
    """The definition, element by element in O(V^2), no bands: the kept mask of one row."""
    x = [float(v) for v in x32]
    V = len(x)
    top_p, min_p = f32(top_p), f32(min_p)
    fin = [v > -math.inf for v in x]
    inK = list(fin)
    if 0 < top_k < V:
        inK = [fin[i] and sum(1 for j in range(V) if x[j] > x[i]) < top_k for i in range(V)]
    mx = max(v for v, f in zip(x, fin) if f)
    Z = sum(math.exp(x[j] - mx) for j in range(V) if inK[j])
    kept = []
    for i in range(V):
        ok = inK[i]
        if ok and top_p < 1.0:
            ok = sum(math.exp(x[j] - mx) for j in range(V) if inK[j] and x[j] > x[i]) / Z < top_p
        if ok and min_p > 0.0:
            ok = math.exp(x[i] - mx) >= min_p
        kept.append(ok)
    return np.array(kept)


# ------------------------------------------- a numpy model of the kernel's select
def f2key(x32: np.ndarray) -> np.ndarray:
    u = x32.astype(np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def key2f(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k).astype(np.uint32).view(np.float32)


KEY_FINITE = int(f2key(np.array([-np.inf], np.float32))[0]) + 1  # the smallest key of a finite value


def fixed_mass(x32: np.ndarray, mx: np.float32) -> np.ndarray:
    """floor(exp(x - max) * 2^40) as uint64, the exponential in fp32 like the kernel's."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp((x32 - mx).astype(np.float32)).astype(np.float32)
    e = np.where(e > 0, e, np.float32(0))
    return np.floor(e.astype(np.float64) * 2.0 ** 40).astype(np.uint64)


def radix_mass_select(keys: np.ndarray, mass: np.ndarray, lo: int, top_p: float) -> int:
    """mass_key() of decode.hip: integer-mass histograms over the bit fields [31:20], [19:8],
    [7:0], bins walked in descending order for mass_above < T <= mass_above + mass(bin)."""
    sel = keys >= np.uint32(lo)
    keys, mass = keys[sel], mass[sel]
    prefix, pmask, T = 0, 0, None
    for sh, w in ((20, 12), (8, 12), (0, 8)):
        nb = 1 << w
        m = (keys & np.uint32(pmask)) == np.uint32(prefix)
        hist = np.zeros(nb, np.uint64)
        np.add.at(hist, ((keys[m] >> np.uint32(sh)) & np.uint32(nb - 1)).astype(np.int64), mass[m])
        if T is None:
            total = int(hist.sum())
            T = min(max(math.ceil(float(np.float64(np.float32(top_p)) * np.float64(total))), 1), total)
        before, pick = 0, 0
        for bin_ in range(nb - 1, -1, -1):
            c = int(hist[bin_])
            if before < T <= before + c:
                pick, T = bin_, T - before
                break
            before += c
        prefix |= pick << sh
        pmask |= (nb - 1) << sh
    return prefix


DEFECTS = ("crossing_dropped", "nucleus_over_whole_row", "nucleus_before_temperature", "min_p_against_one",
           "min_p_before_temperature", "ties_split", "z_forgotten")


def kernel_model(logits: torch.Tensor, T: float, top_k: int, top_p: float, min_p: float, defect: str = "") -> torch.Tensor:
    """The kept mask [B, V] the kernels compute: fp32 exponentials, 40-bit fixed-point masses,
    the radix descent; thresholds on integer keys.  ``defect``: one of DEFECTS planted."""
    assert defect in ("",) + DEFECTS
    xs = scaled(logits, T)
    raw = logits.detach().cpu().float().numpy()
    top_p, min_p = np.float32(top_p), np.float32(min_p)
    out = np.zeros(xs.shape, bool)
    for b, x in enumerate(xs):
        keys = f2key(x)
        fin = np.isfinite(x)
        if not fin.any():
            continue
        mx = x[fin].max()
        thr = KEY_FINITE
        if 0 < top_k < x.size:
            thr = max(thr, int(np.sort(keys)[::-1][top_k - 1]))
        kept = keys >= np.uint32(thr)
        if top_p < 1:
            src, smx = (raw[b], raw[b][fin].max()) if defect == "nucleus_before_temperature" else (x, mx)
            mass = fixed_mass(src, smx)
            lo = KEY_FINITE if defect == "nucleus_over_whole_row" else thr
            if defect in ("crossing_dropped", "ties_split", "z_forgotten"):
                inn = keys >= np.uint32(lo)
                m = np.where(inn, mass, np.uint64(0)).astype(np.float64)
                Tm = float(top_p) * (2.0 ** 40 if defect == "z_forgotten" else m.sum())
                if defect == "ties_split":  # element-wise exclusive sums, equal values in index order
                    order = np.argsort(-x.astype(np.float64), kind="stable")
                    above = np.empty_like(m)
                    above[order] = np.cumsum(m[order]) - m[order]
                else:
                    above = mass_above(x.astype(np.float64), m)
                if defect == "crossing_dropped":  # the mass of the values >= v instead of > v
                    above = m.sum() - mass_above(-x.astype(np.float64), m)  # all but the mass strictly below
                kept &= inn & (above < Tm)
            else:
                kp = radix_mass_select(keys, mass, lo, float(top_p))
                kept &= keys >= np.uint32(kp)
        if min_p > 0:
            if defect == "min_p_against_one":  # p_i >= min_p instead of p_i >= min_p * p_max
                with np.errstate(invalid="ignore"):
                    e = np.where(fin, np.exp((x - mx).astype(np.float64)), 0.0)
                kept &= e / e.sum() >= float(min_p)
            else:
                src, smx = (raw[b], raw[b][fin].max()) if defect == "min_p_before_temperature" else (x, mx)
                c = np.float32(smx + np.float32(math.log(float(min_p))))
                kept &= f2key(src) >= f2key(np.array([c], np.float32))[0]
        out[b] = kept
    return torch.from_numpy(out)


# --------------------------------------------------------------------------- the inputs
TOP_PS = (0.05, 0.5, 0.9, 0.999)
MIN_PS = (0.0, 0.05, 0.5)
TEMPS = (0.05, 1.0, 2.0)
VS = (17, 1000, 50257)
BS = (1, 4, 8)


class Case(NamedTuple):
    name: str
    logits: torch.Tensor  # [B, V] fp32
    T: float
    top_k: int
    top_p: float
    min_p: float

    @property
    def classes(self) -> Classes:
        return _classes(self.name)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def zipf_rows(B: int, V: int, seed: int, s: float = 1.1) -> torch.Tensor:
    """Zipf-like rows: logit -s * ln(rank) + a little noise, ranks permuted per row."""
    g = _gen(seed)
    out = torch.empty(B, V)
    for b in range(B):
        r = torch.randperm(V, generator=g).float() + 1.0
        out[b] = -s * torch.log(r) + 0.05 * torch.randn(V, generator=g)
    return out


def peaked_rows(B: int, V: int, seed: int, p: float) -> torch.Tensor:
    """One token of mass about p, the rest a gaussian spread sharing 1 - p."""
    g = _gen(seed)
    out = torch.randn(B, V, generator=g)
    for b in range(B):
        i = int(torch.randint(0, V, (1,), generator=g))
        out[b, i] = -30.0
        rest = torch.logsumexp(out[b], 0).item()
        out[b, i] = rest + math.log(p / (1 - p))
    return out


def from_probs(groups, V: int, seed: int, bf16: bool = False) -> torch.Tensor:
    """One row [1, V]: ``groups`` = [(probability, count), ...] placed at permuted ids, the
    remaining ids share what is left equally.  Equal probabilities are exactly equal logits."""
    g = _gen(seed)
    vals = [math.log(p) for p, n in groups for _ in range(n)]
    left = 1.0 - sum(p * n for p, n in groups)
    vals += [math.log(left / (V - len(vals)))] * (V - len(vals))
    row = torch.tensor(vals, dtype=torch.float32)
    if bf16:
        row = row.bfloat16().float()
    return row[torch.randperm(V, generator=g)][None].contiguous()


def bf16_step_below(v: float) -> float:
    """The next bf16 value below the bf16 value v."""
    t = torch.tensor([v], dtype=torch.float32).bfloat16()
    i = t.view(torch.int16)
    return (i + (1 if v < 0 else -1)).view(torch.bfloat16).float().item()


def cliff_rows(B: int, V: int, seed: int) -> torch.Tensor:
    """49 values in (max - 1, max], 3000 tied at max - 1.5, the rest far below (the row that
    makes top-k's window search give up, and whose ties overflow the split path's slices)."""
    g = _gen(seed)
    out = torch.empty(B, V)
    for b in range(B):
        perm = torch.randperm(V, generator=g)
        out[b] = -30.0 - 5 * torch.rand(V, generator=g)
        out[b, perm[:49]] = 4.0 - 0.999 * torch.rand(49, generator=g)
        out[b, perm[0]] = 4.0
        out[b, perm[49:3049]] = 2.5
    return out


def _grid():
    """The 12 (top_p, min_p) pairs, T chosen so that every (top_p, T) and (min_p, T) pair
    occurs too; V, B and top_k cycle through all nine (V, B) pairs, each V with top_k off and on."""
    out = []
    for i, tp in enumerate(TOP_PS):
        for j, mp in enumerate(MIN_PS):
            n = 3 * i + j
            T = TEMPS[(i + j) % 3]
            V, B = VS[n % 3], BS[(n + n // 3) % 3]
            top_k = (50 if V > 50 else 5) if n % 2 else 0  # V = 17: top_k = 50 would be off
            out.append((f"zipf-p{tp}-m{mp}-T{T}-V{V}-B{B}-k{top_k}", zipf_rows(B, V, 900 + n), T, top_k, tp, mp))
    return out


def _specials():
    V = 1000
    out = [
        # ---- peaked rows
        ("peaked99-p0.9", peaked_rows(4, V, 910, 0.99), 1.0, 0, 0.9, 0.0),
        ("peaked99-p0.9-k50", peaked_rows(4, 50257, 911, 0.99), 1.0, 50, 0.9, 0.0),
        ("peaked50-p0.9", peaked_rows(4, V, 912, 0.5), 1.0, 0, 0.9, 0.0),
        ("peaked50-p0.9-k50", peaked_rows(8, 50257, 913, 0.5), 1.0, 50, 0.9, 0.05),
        # ---- top-k paths: a nucleus smaller than k, and one that top-k cuts short
        ("nucleus-inside-topk", zipf_rows(4, 50257, 914, s=1.0), 1.0, 50, 0.5, 0.0),
        ("topk-cuts-nucleus", zipf_rows(4, 50257, 915, s=0.8), 2.0, 50, 0.999, 0.0),
        # ---- everything tied: kept for any top_p (V = 50257, k = 50: every slice of the split
        # path overflows SMP_MAXC, so this is also the sample_row fallback from k_dec_topk_draw)
        ("all-equal-V17", torch.full((1, 17), 1.25), 1.0, 0, 0.05, 0.5),
        ("all-equal-V1000", torch.full((4, V), -0.75), 2.0, 0, 0.5, 0.05),
        ("all-equal-overflow", torch.full((1, 50257), 1.25), 1.0, 50, 0.5, 0.0),
        # ---- the cliff: top-k keeps 3049 values; the 3000 ties hold 96 % of their mass
        ("cliff-p0.5", cliff_rows(4, 50257, 916), 1.0, 50, 0.5, 0.0),
        ("cliff-p0.05-minp", cliff_rows(1, 50257, 917), 1.0, 50, 0.05, 0.5),
        # ---- two / three exactly equal values that straddle the boundary: all kept
        ("two-ties-straddle", from_probs([(0.4, 1), (0.2, 2)], 17, 918), 1.0, 0, 0.5, 0.0),
        ("three-ties-straddle", from_probs([(0.3, 1), (0.15, 3)], V, 919), 1.0, 50, 0.5, 0.0),
        ("three-ties-straddle-V50257", from_probs([(0.3, 1), (0.15, 3)], 50257, 920), 1.0, 50, 0.5, 0.0),
        # ---- rows with -inf entries; row 3 has 5 finite entries, fewer than top_k
        ("minus-inf-k0", _minus_inf(V, 922), 1.0, 0, 0.9, 0.0),
        ("minus-inf-k50", _minus_inf(V, 922), 1.0, 50, 0.9, 0.05),
    ]
    # ---- the boundary value, then a value one bf16 step below it: dropped
    # (masses 0.45 | 0.2 | 0.2- | 0.35 spread: 0.375 of the mass lies above the second value, which
    # crosses 0.5 and is kept; 0.54 lies above the third)
    row = from_probs([(0.45, 1), (0.2, 1)], V, 921, bf16=True)
    second = torch.topk(row[0], 2).values[1].item()
    free = int(row[0].argmin())
    row[0, free] = bf16_step_below(second)
    out.append(("bf16-step-below-boundary", row, 1.0, 0, 0.5, 0.0))
    return out


def _minus_inf(V: int, seed: int) -> torch.Tensor:
    g = _gen(seed)
    lg = torch.randn(4, V, generator=g) * 2
    lg[torch.rand(4, V, generator=g) < 0.6] = float("-inf")
    lg[3] = float("-inf")
    lg[3, [5, 700, 500, V - 2, V - 1]] = torch.tensor([0.0, 1.0, -1.0, 0.5, 2.0])
    return lg


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """{name: Case}: every input of the GPU tests, built once."""
    out = {}
    for name, lg, T, k, tp, mp in _grid() + _specials():
        assert name not in out
        out[name] = Case(name, lg.contiguous(), T, k, tp, mp)
    return out


@functools.lru_cache(maxsize=None)
def _classes(name: str) -> Classes:
    """The classification of a case, computed once and shared; asserts the empty band."""
    c = cases()[name]
    cl = classify(c.logits, c.T, c.top_k, c.top_p, c.min_p)
    n = int(cl.either.sum())
    assert n == 0, f"{name}: {n} tokens inside the either band: pick another seed / value for this input"
    assert cl.must_keep.any(dim=1).all(), f"{name}: a row keeps nothing"
    return cl


CASE_NAMES = tuple(cases())
# frequencies: cases that span the three paths (a top-k case runs without and with the workspace)
FREQ_CASES = (next(n for n in CASE_NAMES if n.startswith("zipf") and "V50257" in n and n.endswith("k0")),
              next(n for n in CASE_NAMES if n.startswith("zipf") and "T2.0-V50257" in n and n.endswith("k50")),
              "peaked50-p0.9", "nucleus-inside-topk", "cliff-p0.5", "topk-cuts-nucleus")
