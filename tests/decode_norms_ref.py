"""fp64 references, derived tolerances and inputs for the QK-norm and post-norm decode kernels
(``ops/csrc/decode_norms.hip``), in the terms of tests/decode_ref.py."""
import numpy as np
import torch

from tests.decode_ref import (EPS, U8, U23, Checked, _gen, bf16_round, column_profile, gemv, gemv_pre_tol,
                              gemv_tol, norm_weights, normed, qkv_inputs)

E32 = float(np.float32(EPS))  # the eps the kernels receive


def _rope(y, dy, c, s):  # NeoX rotation of y [.., 64]; its error bound dy through the partial derivatives
    y1, y2, d1, d2 = y[..., :32], y[..., 32:], dy[..., :32], dy[..., 32:]
    ref = torch.cat([y1 * c - y2 * s, y2 * c + y1 * s], dim=-1)
    return ref, torch.cat([c.abs() * d1 + s.abs() * d2, c.abs() * d2 + s.abs() * d1], dim=-1)


def qkn_ref(h, lnw, wqkv, qn, kn, cos, sin, pos, nh, nkv):
    """dec_norm_qkv_qkn: {"q": [B, nh, 64], "k": [B, nkv, 64], "v": ...} of Checked."""
    B, H = h.shape
    g = gemv(normed(h, lnw), wqkv)
    x, pre = bf16_round(g.y), gemv_pre_tol(g, H)  # the GEMV outputs, bf16 like torch's matmul
    c, s = cos[pos].double().to(x.device), sin[pos].double().to(x.device)
    out, lo = {}, 0
    for name, n, w in (("q", nh, qn), ("k", nkv, kn)):
        xh, ph = x[:, lo:lo + n * 64].view(B, n, 64), pre[:, lo:lo + n * 64].view(B, n, 64)
        lo += n * 64
        ms = (xh * xh).mean(-1, keepdim=True) + E32
        y = xh * torch.rsqrt(ms) * w.double()
        # x_j is off by its dot product's fp32 error and, where that crosses a tie, one bf16 ulp
        # (<= 2^-7 |x_j|).  dy_d/dx_j = rstd w_d [d == j] - y_d x_j / (64 ms): the direct term and
        # the effect of every x_j of the head on the row's rstd.
        # The fp32 norm itself: a 64-term sum (64 * 2^-24 of ms, half of it in rstd), rsqrt (2 ulps),
        # two products and the rotation's three roundings: under 48 * 2^-24 = 24 * U23 of |y|.
        dx = ph + 2 * U8 * xh.abs()
        dy = (torch.rsqrt(ms) * w.double().abs() * dx + y.abs() * (xh.abs() * dx).sum(-1, keepdim=True) / (64 * ms)
              + 24 * U23 * y.abs())
        ref, prop = _rope(y, dy, c, s)
        out[name] = Checked(ref, U8 * ref.abs() + prop)
    out["v"] = Checked(g.y[:, lo:].view(B, nkv, 64), gemv_tol(g, H)[:, lo:].view(B, nkv, 64))
    return out


def qkn_inputs(H, wbf16, nkv):
    """decode_ref.qkv_inputs with the K/V heads cut to ``nkv``, every head of the weight scaled by
    another power of two and each 16-dim quarter of a head by another factor (a sum over the wrong
    64 rows, or over a quarter head, gives another rstd), q_norm != k_norm and both far from 1."""
    nh = H // 64
    h, lnw, w = qkv_inputs(H, wbf16)
    w = torch.cat([w[:H], w[H:H + nkv * 64], w[2 * H:2 * H + nkv * 64]]).float().view(nh + 2 * nkv, 4, 16, H)
    w = w * (2.0 ** (torch.arange(nh + 2 * nkv) % 4 - 2.0)).view(-1, 1, 1, 1) * torch.tensor([1., 3., .5, 2.]).view(1, 4, 1, 1)
    g = _gen(700 + H)
    qn, kn = 0.2 + 0.2 * torch.rand(64, generator=g), 2.0 + 2.0 * torch.rand(64, generator=g)
    if wbf16:
        qn, kn = qn.bfloat16(), kn.bfloat16()
    return h, lnw, w.view(-1, H).bfloat16(), qn, kn


def post_inputs(H, wbf16):
    """(a [8, H] bf16, about 10x the residual's scale; pn_w): a missing or misplaced post-norm shows."""
    g = _gen(800 + H)
    return (30.0 * torch.randn(8, H, generator=g) * column_profile(H).flip(0)).bfloat16(), norm_weights(H, g, wbf16)


def post_ref(h, a, pnw) -> Checked:
    """The residual row of the PN forms: h + bf16(a * rsqrt(mean(a^2) + eps) * pn_w), stored in fp32."""
    u = a.double() * torch.rsqrt((a.double() ** 2).mean(1, keepdim=True) + E32) * pnw.double()
    # u is a bf16-rounded intermediate: one ulp (2^-7 |u|) where the fp32 value falls on the other
    # side of a tie; then one fp32 add
    return Checked(h.double() + bf16_round(u), 2 * U8 * u.abs() + U23 * (h.double().abs() + u.abs()))
