"""KV-cached autoregressive decoding for ``GPT.generate`` on the engine path.

The reference's ``generate`` (``gpt.py:457-484``) re-runs the full forward over the
whole context for every new token (O(T^2) work).  Here the prompt is
prefilled once, per-layer K/V (already RoPE-rotated) are cached in preallocated
``[B, nh, max_seq_len, hd]`` buffers, and each new token costs one token's worth of
GEMV + attention.  Sampling semantics are the reference's: temperature, top-k
filtering (``logits < kth`` -> -inf), softmax, ``torch.multinomial`` -- and, off by default,
nucleus (top-p) and min-p filtering on top of top-k (:func:`filter_logits`); contexts longer
than ``max_seq_len`` are cropped to the last ``max_seq_len`` tokens (the cache is then
re-prefilled on the cropped window so RoPE positions match the reference exactly).

With grouped-query attention (``num_kv_heads < num_heads``) the cache holds the
``num_kv_heads`` K/V heads.  The fused decode step (``ops/csrc/decode.hip``) has a form
for either layout (:func:`_fused_kind`): the grouped-query one reads every cached K/V
row once for all query heads of its group and splits the keys over several workgroups.

Sliding-window layers (``cfg.layer_window``) attend to the last ``W`` cached keys only: the
ATen paths add the lower bound to their masks, the fused step calls the ``window`` forms of
the two attention kernels.  The cache keeps ``max_seq_len`` rows (no ring buffer).

Weights are read from the engine's provider (bf16 shadows on GPU / FSDP gathered
units), so generation works the same for single-GPU, DDP and FSDP-trained models.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from ..ops.hip import check_top_p_min_p


class KVCache:
    def __init__(self, cfg, B: int, device, dtype):
        # grouped-query attention: the cache holds the num_kv_heads K/V heads (not repeated)
        self.k = [torch.zeros(B, cfg.num_kv_heads, cfg.max_seq_len, cfg.head_dim, device=device, dtype=dtype)
                  for _ in range(cfg.num_layers)]
        self.v = [torch.zeros_like(t) for t in self.k]
        self.len = 0


def _rms(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    return xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()


def _branch(a: torch.Tensor, wn, eps: float) -> torch.Tensor:
    """The fp32 value a branch output ``a`` (o_proj / down_proj, activation dtype) adds to the
    residual: with post-norms (cfg.post_norm: ``wn`` = ``w.pn1`` / ``w.pn2`` is set) the RMSNorm of
    ``a`` rounded once to the activation dtype, as the training kernels form it; else ``a``."""
    if wn is None:
        return a.float()
    return _rms(a, wn, eps).to(a.dtype).float()


def _rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    # x [B, T, nh, hd] fp32; cos/sin [T, hd/2]
    half = x.shape[-1] // 2
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def _qk_norm(q: torch.Tensor, k: torch.Tensor, w, eps: float):
    """QK-norm (cfg.qk_norm: ``w.qn`` / ``w.kn`` are set): RMSNorm over head_dim of every
    query / key head, before RoPE -- the cache then holds normalised, rotated keys."""
    if getattr(w, "qn", None) is None:
        return q, k
    return _rms(q, w.qn, eps), _rms(k, w.kn, eps)


def _sink_softmax(s: torch.Tensor, w) -> torch.Tensor:
    """Softmax over the keys of scores ``s`` [B, nh, T, keys] (fp32, masked entries -inf).  With
    attention sinks (cfg.attention_sinks: ``w.sk`` is set) the head's sink logit is one more
    column of the softmax -- it takes part in the denominator and has no value row -- and the
    key columns are returned."""
    sk = getattr(w, "sk", None)
    if sk is None:
        return torch.softmax(s, dim=-1)
    col = sk.float().view(1, -1, 1, 1).expand(s.shape[0], -1, s.shape[2], 1)
    return torch.softmax(torch.cat([s, col], dim=-1), dim=-1)[..., :-1]


def _split_qkv(qkv: torch.Tensor, cfg):
    """Packed projection [B, T, H + 2*KV] fp32 -> q [B, T, nh, hd], k, v [B, T, nkv, hd]."""
    B, T, _ = qkv.shape
    nh, nkv, hd = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim
    if nkv == nh:
        t = qkv.view(B, T, 3, nh, hd)
        return t[:, :, 0], t[:, :, 1], t[:, :, 2]
    H, KV = nh * hd, nkv * hd
    return (qkv[..., :H].view(B, T, nh, hd), qkv[..., H:H + KV].view(B, T, nkv, hd),
            qkv[..., H + KV:].view(B, T, nkv, hd))


def _layer_window(cfg, i: int) -> Optional[int]:
    """Window of layer ``i`` or None (also for configs from before the field existed)."""
    lw = getattr(cfg, "layer_window", None)
    return lw(i) if lw is not None else None


def _attn_keys(cfg) -> int:
    """Keys whose scores the fused attention kernels must hold, the largest need over the
    layers: ``max_seq_len`` for a global layer, ``min(W, max_seq_len)`` for a windowed one."""
    W = getattr(cfg, "sliding_window", None)
    N = getattr(cfg, "sliding_window_pattern", None)
    if W is None or (N is not None and getattr(cfg, "num_layers", N) >= N):  # some layer is global
        return cfg.max_seq_len
    return min(W, cfg.max_seq_len)


def _rep_kv(t: torch.Tensor, cfg) -> torch.Tensor:
    """Cached K or V [B, nkv, S, hd] repeated over each group's query heads."""
    G = cfg.num_heads // cfg.num_kv_heads
    return t if G == 1 else t.repeat_interleave(G, dim=1)


def _softcap(logits: torch.Tensor, cfg) -> torch.Tensor:
    """The model's final-logit soft cap (cfg.logit_softcap) on fp32 logits; unset: the logits themselves."""
    cap = getattr(cfg, "logit_softcap", None)
    return logits if cap is None else cap * torch.tanh(logits / cap)


def _cap_scores(s: torch.Tensor, cfg) -> torch.Tensor:
    """The model's attention-score soft cap (cfg.attn_softcap) on fp32 scaled scores, before any
    mask; unset: the scores themselves."""
    cap = getattr(cfg, "attn_softcap", None)
    return s if cap is None else float(cap) * torch.tanh(s / float(cap))


@torch.no_grad()
def forward_cached(model, ids: torch.Tensor, cache: KVCache) -> torch.Tensor:
    """Append ``ids`` [B, T] at positions cache.len.. ; returns last-position logits [B, V]."""
    eng = model.engine
    cfg = model.config
    prov = eng.provider
    dt = eng.act_dtype
    B, T = ids.shape
    p0 = cache.len
    nh, hd = cfg.num_heads, cfg.head_dim
    cos_t, sin_t = eng.rope(max(cfg.max_seq_len, p0 + T), ids.device)
    cos, sin = cos_t[p0:p0 + T].float(), sin_t[p0:p0 + T].float()
    prov.pre_forward("head")
    hw = prov.head()
    h = hw.embed.index_select(0, ids.reshape(-1)).float().view(B, T, -1)
    scale = 1.0 / math.sqrt(hd)
    for i in range(cfg.num_layers):
        prov.pre_forward(i)
        w = prov.layer(i)
        n1 = _rms(h, w.ln1, eng.eps).to(dt)
        q, k, v = _split_qkv(torch.matmul(n1, w.wqkv.t()).float(), cfg)
        q, k = _qk_norm(q, k, w, eng.eps)
        q = _rope(q, cos, sin)
        k = _rope(k, cos, sin)
        cache.k[i][:, :, p0:p0 + T] = k.transpose(1, 2).to(dt)
        cache.v[i][:, :, p0:p0 + T] = v.transpose(1, 2).to(dt)
        K = _rep_kv(cache.k[i][:, :, :p0 + T].float(), cfg)
        Vv = _rep_kv(cache.v[i][:, :, :p0 + T].float(), cfg)
        qh = q.to(dt).float().transpose(1, 2)  # [B, nh, T, hd]
        s = _cap_scores(torch.matmul(qh, K.transpose(-2, -1)) * scale, cfg)
        W = _layer_window(cfg, i)
        if T > 1 or (W is not None and W < p0 + T):
            qpos = torch.arange(p0, p0 + T, device=ids.device)[:, None]
            kpos = torch.arange(0, p0 + T, device=ids.device)[None, :]
            hidden = kpos > qpos
            if W is not None:  # sliding window: the keys at or below qpos - W are out
                hidden = hidden | (kpos <= qpos - W)
            s = s.masked_fill(hidden, float("-inf"))
        pr = _sink_softmax(s, w)
        o = torch.matmul(pr, Vv).transpose(1, 2).reshape(B, T, nh * hd).to(dt)
        h = h + _branch(torch.matmul(o, w.wo.t()), getattr(w, "pn1", None), eng.eps)
        n2 = _rms(h, w.ln2, eng.eps).to(dt)
        gu = torch.matmul(n2, w.wgu.t()).float()
        I = cfg.intermediate_size
        a = (F.silu(gu[..., :I]) * gu[..., I:]).to(dt)
        h = h + _branch(torch.matmul(a, w.wdown.t()), getattr(w, "pn2", None), eng.eps)
        prov.post_forward(i)
    hw = prov.head()
    nf = _rms(h[:, -1], hw.norm, eng.eps).to(dt)
    logits = _softcap(torch.matmul(nf, hw.lm_head.t())[:, :cfg.vocab_size].float(), cfg)
    prov.post_forward("head")
    cache.len = p0 + T
    return logits


class DecodeGraph:
    """The one-token decode step captured once as a HIP graph and replayed per token.

    Decode is launch-bound (~200 small kernels per token for GPT-2 small); a graph
    replay issues them with one call.  Everything inside has a fixed shape: the token
    ids and the position are device tensors, the new K/V row is written with
    ``index_copy_`` at the position, and attention runs over the whole preallocated
    cache with a ``key_pos > pos`` mask (a few extra MB per layer per token, far cheaper
    than the launches it saves).  Used by ``kv_cached_generate`` on a GPU with a
    single-process parameter store (FSDP gathers are collectives: not captured).
    """

    def __init__(self, model, cache: KVCache, pos: int, sample: Optional[dict] = None):
        """``sample`` (fused step only): dict(temperature, top_k, seed, hist, hist_base and
        optionally top_p, min_p) --
        the graph then also draws the next token (ops ``dec_sample``) into ``self.ids`` and
        ``hist`` and advances the device position, so generation is one replay per token
        with no host round trip."""
        self.model, self.cache = model, cache
        cfg = model.config
        dev = cache.k[0].device
        B = cache.k[0].shape[0]
        self.ids = torch.zeros(B, 1, dtype=torch.long, device=dev)
        self.pos = torch.full((1,), pos, dtype=torch.long, device=dev)
        self.kpos = torch.arange(cfg.max_seq_len, device=dev)
        # fused HIP step (ops/csrc/decode.hip): 5 kernels per layer instead of ~25 ATen ops
        # (a grouped-query model: the _gqa forms of the two attention-side kernels)
        self.kind = _fused_kind(model, B)
        self.fused = self.kind is not None
        if self.kind == "gqa":
            # key chunks per K/V head and the partials they merge through: allocated once,
            # outside the capture
            self.kv_splits = _gqa_splits(cfg, B)
            self.attn_ws = (model.engine.ops.dec_attn_gqa_workspace(B, cfg.num_heads, self.kv_splits, dev)
                            if self.kv_splits > 1 else None)
        if self.fused:
            H, I = cfg.hidden_size, cfg.intermediate_size
            self.h = torch.empty(B, H, dtype=torch.float32, device=dev)
            self.qb = torch.empty(B, H, dtype=torch.bfloat16, device=dev)
            self.ob = torch.empty(B, H, dtype=torch.bfloat16, device=dev)
            self.sb = torch.empty(B, I, dtype=torch.bfloat16, device=dev)
            self.lg = torch.empty(B, cfg.vocab_size, dtype=torch.float32, device=dev)
        self.sample = sample if self.fused else None
        if self.sample is not None:
            self.sample_ws = model.engine.ops.dec_sample_workspace(B, dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # warm up allocations / library plans outside the capture
            for _ in range(2):
                # the sampling step advances the device position: restart every warm-up
                # step at ``pos`` so none writes K/V at pos + 1 (== max_seq_len when the
                # prompt fills all but one slot)
                self.pos.fill_(pos)
                self._step()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.logits = self._step()
        self.pos.fill_(pos)  # the warm-up steps advanced it (sampling graph)

    def _step_fused(self) -> torch.Tensor:
        model, cache = self.model, self.cache
        eng, cfg = model.engine, model.config
        ops, prov = eng.ops, eng.provider
        cos_t, sin_t = eng.rope(cfg.max_seq_len, self.ids.device)
        hw = prov.head()
        self.h.copy_(hw.embed.index_select(0, self.ids.view(-1)))
        scale = 1.0 / math.sqrt(cfg.head_dim)
        for i in range(cfg.num_layers):
            w = prov.layer(i)
            W = _layer_window(cfg, i) or 0
            wkw = {"window": W} if W else {}  # a global layer calls the kernels it always did
            if getattr(w, "sk", None) is not None:  # attention sinks: the kernels' sink= forms
                wkw["sink"] = w.sk
            if getattr(cfg, "attn_softcap", None) is not None:  # a capped model: the CAP kernels
                wkw["softcap"] = cfg.attn_softcap
            if self.kind == "gqa":
                ops.dec_norm_qkv_gqa(self.h, w.ln1, eng.eps, w.wqkv, cos_t, sin_t, self.pos, self.qb, cache.k[i],
                                     cache.v[i], cfg.num_heads, cfg.num_kv_heads)
                ops.dec_attn_gqa(self.qb, cache.k[i], cache.v[i], self.pos, self.ob, scale, cfg.num_heads,
                                 splits=self.kv_splits, ws=self.attn_ws, **wkw)
            else:
                ops.dec_norm_qkv(self.h, w.ln1, eng.eps, w.wqkv, cos_t, sin_t, self.pos, self.qb, cache.k[i],
                                 cache.v[i], cfg.num_heads)
                ops.dec_attn(self.qb, cache.k[i], cache.v[i], self.pos, self.ob, scale, **wkw)
            ops.dec_gemv_res(self.ob, w.wo, self.h)
            ops.dec_norm_gu(self.h, w.ln2, eng.eps, w.wgu, self.sb)
            ops.dec_gemv_res(self.sb, w.wdown, self.h)
        cap = getattr(cfg, "logit_softcap", None)
        if cap is None:
            ops.dec_norm_head(self.h, hw.norm, eng.eps, hw.lm_head, self.lg, cfg.vocab_size)
        else:  # the CAP kernel: the sampler below reads capped logits
            ops.dec_norm_head(self.h, hw.norm, eng.eps, hw.lm_head, self.lg, cfg.vocab_size, softcap=cap)
        if self.sample is not None:
            sm = self.sample
            ops.dec_sample(self.lg, sm["temperature"], sm["top_k"], sm["seed"], self.pos, self.ids, sm["hist"],
                           sm["hist_base"], ws=self.sample_ws, top_p=sm.get("top_p", 1.0), min_p=sm.get("min_p", 0.0))
            ops.dec_advance(self.pos)
        return self.lg

    def _step(self) -> torch.Tensor:
        if self.fused:
            return self._step_fused()
        model, cache = self.model, self.cache
        eng, cfg = model.engine, model.config
        prov, dt = eng.provider, eng.act_dtype
        B = self.ids.shape[0]
        nh, hd = cfg.num_heads, cfg.head_dim
        cos_t, sin_t = eng.rope(cfg.max_seq_len, self.ids.device)
        cos = cos_t.index_select(0, self.pos).float()
        sin = sin_t.index_select(0, self.pos).float()
        hw = prov.head()
        h = hw.embed.index_select(0, self.ids.view(-1)).float().view(B, 1, -1)
        scale = 1.0 / math.sqrt(hd)
        masked_g = (self.kpos > self.pos)[None, None, None, :]
        W = getattr(cfg, "sliding_window", None)
        # the windowed layers' mask: also the keys at or below pos - W (pos stays on the device)
        masked_w = masked_g if W is None else masked_g | (self.kpos <= self.pos - W)[None, None, None, :]
        for i in range(cfg.num_layers):
            w = prov.layer(i)
            masked = masked_g if _layer_window(cfg, i) is None else masked_w
            n1 = _rms(h, w.ln1, eng.eps).to(dt)
            q, k, v = _split_qkv(torch.matmul(n1, w.wqkv.t()).float(), cfg)
            q, k = _qk_norm(q, k, w, eng.eps)
            q = _rope(q, cos, sin)
            k = _rope(k, cos, sin)
            cache.k[i].index_copy_(2, self.pos, k.transpose(1, 2).to(dt))
            cache.v[i].index_copy_(2, self.pos, v.transpose(1, 2).to(dt))
            qh = q.to(dt).transpose(1, 2)  # [B, nh, 1, hd]; bf16 GEMVs straight on the bf16 cache
            s_ = _cap_scores(torch.matmul(qh, _rep_kv(cache.k[i], cfg).transpose(-2, -1)).float() * scale, cfg)
            pr = _sink_softmax(s_.masked_fill(masked, float("-inf")), w)
            o = torch.matmul(pr.to(dt), _rep_kv(cache.v[i], cfg)).transpose(1, 2).reshape(B, 1, nh * hd)
            h = h + _branch(torch.matmul(o, w.wo.t()), getattr(w, "pn1", None), eng.eps)
            n2 = _rms(h, w.ln2, eng.eps).to(dt)
            gu = torch.matmul(n2, w.wgu.t()).float()
            I = cfg.intermediate_size
            h = h + _branch(torch.matmul((F.silu(gu[..., :I]) * gu[..., I:]).to(dt), w.wdown.t()),
                            getattr(w, "pn2", None), eng.eps)
        nf = _rms(h[:, -1], hw.norm, eng.eps).to(dt)
        return _softcap(torch.matmul(nf, hw.lm_head.t())[:, :cfg.vocab_size].float(), cfg)

    def __call__(self, ids: torch.Tensor) -> torch.Tensor:
        """Append ``ids`` [B, 1] at position cache.len; returns logits [B, V] (graph-owned:
        consume before the next call)."""
        self.ids.copy_(ids)
        self.pos.fill_(self.cache.len)
        self.graph.replay()
        self.cache.len += 1
        return self.logits


DEC_LDS_MAX = 160 * 1024  # bytes of LDS per workgroup on gfx950


DEC_KV_SPLITS = (1, 2, 4, 8)
DEC_KV_SPLIT_LONG = 4096  # caches longer than this take 8 key chunks per K/V head, shorter ones 4


def _dec_kv_splits(B: int, nkv: int, maxS: int) -> int:
    """Key chunks per K/V head (NS) of the grouped-query decode attention, fixed when the
    step is captured: 4, and 8 for a cache longer than DEC_KV_SPLIT_LONG.  Measured on GPT-2
    small with 4 and 1 K/V heads at B = 1 and 8 (profiles/gqa_decode.md): over a generation
    that fills the cache this is the fastest NS, or within 2 % of it, in every cell; B * nkv
    (1 to 32 there) did not change the choice, and between the two measured cache lengths
    (1024 and 16384) the threshold is their geometric mean.
    ``DLT_DECODE_KV_SPLITS=n`` (n in 1, 2, 4, 8) overrides the rule for A/B runs."""
    env = os.environ.get("DLT_DECODE_KV_SPLITS", "").strip()
    if env:
        if not env.isdigit() or int(env) not in DEC_KV_SPLITS:
            raise ValueError(f"DLT_DECODE_KV_SPLITS={env!r}: expected one of {DEC_KV_SPLITS}")
        return int(env)
    return 4 if maxS <= DEC_KV_SPLIT_LONG else 8


def _gqa_splits(cfg, B: int) -> int:
    """NS of a model's fused grouped-query step (:func:`_dec_kv_splits`)."""
    return _dec_kv_splits(B, cfg.num_kv_heads, cfg.max_seq_len)


def _fused_kind(model, B: int) -> Optional[str]:
    """Which fused HIP decode step applies: ``"mha"`` (``dec_norm_qkv`` / ``dec_attn``),
    ``"gqa"`` (num_kv_heads < num_heads: ``dec_norm_qkv_gqa`` / ``dec_attn_gqa``) or None,
    for which ``DecodeGraph`` captures the ATen step instead (always for a QK-norm model: the
    fused norm + QKV kernels do not apply q_norm / k_norm).  Both kinds need HIP ops, a
    supported batch, head_dim 64, ``DLT_DECODE_FUSED != 0`` and the LDS of their kernels to
    fit one CU: the norm + GEMV kernels stage one normed bf16 row per batch entry
    (``dec_lds`` in decode.hip); ``k_dec_attn`` keeps all ``max_seq_len`` scores of a
    (batch, head) (maxS * 4 + 1056 B: max_seq_len <= ~40.7k), ``k_dec_attn_gqa`` the scores
    of a group's query heads over one key chunk at the NS of :func:`_gqa_splits`.  Where
    every layer has a sliding window both hold ``min(W, max_seq_len)`` keys instead
    (:func:`_attn_keys`); a model with global layers needs what those need."""
    ops = model.engine.ops
    cfg = model.config
    if getattr(cfg, "qk_norm", False):  # no fused norm + QKV kernel applies q_norm / k_norm: the ATen step does
        return None
    if getattr(cfg, "post_norm", False):  # dec_gemv_res adds the raw branch to the residual: the ATen step norms it
        return None
    norm_lds = B * cfg.hidden_size * 2 + B * 4 * 4 + B * 16 * 4
    if not (hasattr(ops, "dec_norm_qkv") and B in getattr(ops, "DECODE_BATCHES", ())
            and cfg.head_dim == 64 and norm_lds <= DEC_LDS_MAX
            and os.environ.get("DLT_DECODE_FUSED", "1") != "0"):
        return None
    keys = _attn_keys(cfg)
    if cfg.num_kv_heads == cfg.num_heads:
        attn_lds = keys * 4 + 8 * 4 + 4 * 64 * 4
        return "mha" if attn_lds <= DEC_LDS_MAX else None
    # the grouped-query kernels are bf16 only: an fp16 / fp32 engine keeps the ATen step it had
    if not hasattr(ops, "dec_attn_gqa") or getattr(model.engine, "act_dtype", torch.bfloat16) != torch.bfloat16:
        return None
    from ..ops.hip import dec_attn_chunk, dec_attn_gqa_lds
    G = cfg.num_heads // cfg.num_kv_heads
    lds = dec_attn_gqa_lds(G, dec_attn_chunk(keys, _gqa_splits(cfg, B)))
    return "gqa" if lds <= DEC_LDS_MAX else None


def _fused_ok(model, B: int) -> bool:
    """The multi-head fused kernel set applies (:func:`_fused_kind` is ``"mha"``); False
    for every grouped-query model, whose fused step is the ``"gqa"`` kind."""
    return _fused_kind(model, B) == "mha"


def _graph_ok(model, device) -> bool:
    import os
    from ..parallel.flat import FlatParamStore
    return (device.type == "cuda" and os.environ.get("DLT_DECODE_GRAPH", "1") != "0"
            and isinstance(model.engine.provider, FlatParamStore))


def _reset(cache: KVCache) -> KVCache:
    cache.len = 0
    return cache


def filter_logits(lg: torch.Tensor, top_k: int, top_p: float = 1.0, min_p: float = 0.0) -> torch.Tensor:
    """The sampling filters on ``lg`` = logits / temperature [B, V]: what is not kept is -inf.
    Each filter keeps the values >= a threshold of its own, so equal values stand or fall
    together, and the kept set is the intersection (the device sampler, ``dec_sample``, applies
    the same definition):

    * top-k (``top_k`` > 0): the values >= the k-th largest;
    * top-p (``top_p`` < 1), on q = softmax over what top-k left: a value is kept iff the
      q-mass of the values strictly above it is < top_p (the value that crosses top_p is kept,
      the largest always is; the sums are taken in fp64);
    * min-p (``min_p`` > 0): exp(v - max) >= min_p, i.e. p >= min_p * p_max.

    With the defaults this is the top-k code ``generate`` always ran."""
    top_p, min_p = check_top_p_min_p(top_p, min_p)
    x = lg
    if top_k > 0:
        v, _ = torch.topk(lg, min(top_k, lg.size(-1)))
        lg = lg.masked_fill(lg < v[:, [-1]], float("-inf"))
    if top_p < 1.0:
        s, _ = torch.sort(lg, dim=-1, descending=True)
        q = F.softmax(s.double(), dim=-1)
        above = q.cumsum(dim=-1) - q  # exclusive: of equal values the first has the mass strictly above
        thr = s.masked_fill(above >= top_p, float("inf")).amin(dim=-1, keepdim=True)
        lg = lg.masked_fill(lg < thr, float("-inf"))
    if min_p > 0.0:
        thr = x.amax(dim=-1, keepdim=True) + math.log(min_p)
        lg = lg.masked_fill(x < thr, float("-inf"))
    return lg


@torch.no_grad()
def kv_cached_generate(model, input_ids: torch.Tensor, max_new_tokens: int = 100, temperature: float = 1.0,
                       top_k: int = 50, top_p: float = 1.0, min_p: float = 0.0) -> torch.Tensor:
    """KV-cached sampling (``GPT.generate`` on the engine path): temperature, then the top-k,
    top-p and min-p filters of :func:`filter_logits`.  The document mask
    of ``GPT.set_doc_separator`` is not applied here: generation continues one document,
    so the prompt and every cached key are taken to belong to it."""
    top_p, min_p = check_top_p_min_p(top_p, min_p)
    cfg = model.config
    eng = model.engine
    B = input_ids.shape[0]
    cache = KVCache(cfg, B, input_ids.device, eng.act_dtype)
    ctx = input_ids[:, -cfg.max_seq_len:]
    logits = forward_cached(model, ctx, cache)
    out = input_ids
    n_dev = min(max_new_tokens - 1, cfg.max_seq_len - cache.len)
    if (n_dev > 0 and temperature > 0 and _graph_ok(model, input_ids.device)
            and _fused_kind(model, B) is not None and os.environ.get("DLT_DECODE_DEVICE_LOOP", "1") != "0"):
        # first token from the prefill logits (ATen sampling), then one graph replay per
        # token: the fused step samples on the device and feeds itself (no host round trip)
        lg = filter_logits(logits / temperature, top_k, top_p, min_p)
        nxt = torch.multinomial(F.softmax(lg, dim=-1), num_samples=1)
        hist = torch.empty(B, n_dev, dtype=torch.long, device=input_ids.device)
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())  # torch's generator: manual_seed reproducible
        graph = DecodeGraph(model, cache, cache.len,
                            sample=dict(temperature=float(temperature), top_k=int(top_k), seed=seed, hist=hist,
                                        hist_base=cache.len + 1, top_p=top_p, min_p=min_p))
        graph.ids.copy_(nxt)
        for _ in range(n_dev):
            graph.graph.replay()
        cache.len += n_dev
        out = torch.cat([out, nxt, hist], dim=1)
        if n_dev == max_new_tokens - 1:
            return out
        # context window full: continue on the host path (re-prefill cropping)
        logits = forward_cached(model, out[:, -cfg.max_seq_len:], _reset(cache))
        max_new_tokens -= n_dev + 1
    graph = DecodeGraph(model, cache, cache.len) if (_graph_ok(model, input_ids.device)
                                                    and cache.len < cfg.max_seq_len and max_new_tokens > 1) else None
    for step in range(max_new_tokens):
        lg = filter_logits(logits / temperature, top_k, top_p, min_p)
        probs = F.softmax(lg, dim=-1)
        nxt = torch.multinomial(probs, num_samples=1)
        out = torch.cat([out, nxt], dim=1)
        if step == max_new_tokens - 1:
            break
        if cache.len + 1 <= cfg.max_seq_len:
            logits = graph(nxt) if graph is not None else forward_cached(model, nxt, cache)
        else:  # context window full: re-prefill the cropped window (reference cropping semantics)
            cache.len = 0
            logits = forward_cached(model, out[:, -cfg.max_seq_len:], cache)
    return out
