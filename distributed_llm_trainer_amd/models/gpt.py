"""LLaMA-style "GPT-2" model with the reference's module tree and state-dict keys.

Parity target: ``/root/reference/src/models/gpt.py`` -- RMSNorm (``:22-67``), NeoX
RoPE (``:70-147``), causal self-attention with separate bias-free q/k/v/o
(``:150-242``), SwiGLU MLP (``:245-283``), pre-norm block (``:286-316``), tied
``lm_head`` (``:339-342``), N(0, 0.02) init (``:380-385``), shifted CE loss
(``:449-453``), top-k sampling ``generate`` (``:457-484``).

Two execution paths share the same ``nn.Parameter`` objects:

* **eager path** (this file): plain PyTorch modules.  It is the numerics oracle for
  the tests and the CPU "plumbing" path (BASELINE.json configs[0]).
* **engine path** (``enable_engine``): parameters are re-homed into flat fp32
  buffers (``parallel/flat.py``) and forward/backward run through the hand-scheduled
  fused executor (``models/engine.py``) whose hot ops are the HIP/CDNA4 kernels in
  ``ops/csrc``.  On GPU this is the only path the trainers use; the fused loss path
  never materialises the ``[B, S, V]`` logits, so ``forward`` returns
  ``(None, loss)`` when called with labels during training.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from .config import GPTConfig


class RMSNorm(nn.Module):
    def __init__(self, hidden_size: int, eps: float = 1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.eps = eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        rms = torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + self.eps)
        return x * rms * self.weight


class RotaryPositionEmbedding(nn.Module):
    """NeoX-style RoPE.  The cos/sin caches are persistent buffers because the
    reference checkpoint format carries them (``rotary_emb.{inv_freq,cos_cached,sin_cached}``)."""

    def __init__(self, dim: int, max_seq_len: int = 2048, base: int = 10000):
        super().__init__()
        self.dim = dim
        self.max_seq_len = max_seq_len
        self.base = base
        inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2).float() / dim))
        self.register_buffer("inv_freq", inv_freq)
        self._build_cache(max_seq_len)

    def _build_cache(self, seq_len: int) -> None:
        t = torch.arange(seq_len, device=self.inv_freq.device).float()
        freqs = torch.outer(t, self.inv_freq)
        emb = torch.cat((freqs, freqs), dim=-1)
        self.register_buffer("cos_cached", emb.cos())
        self.register_buffer("sin_cached", emb.sin())

    def forward(self, x: torch.Tensor, seq_len: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if seq_len > self.cos_cached.shape[0]:
            # (the reference rebuilds on every long call because it never updates
            # max_seq_len; we rebuild once and keep the larger cache)
            self._build_cache(seq_len)
        return self.cos_cached[:seq_len], self.sin_cached[:seq_len]


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    half = x.shape[-1] // 2
    return torch.cat([-x[..., half:], x[..., :half]], dim=-1)


def apply_rotary_pos_emb(q, k, cos, sin):
    return q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin


class CausalSelfAttention(nn.Module):
    def __init__(self, config: GPTConfig, window: Optional[int] = None):
        super().__init__()
        self.config = config
        # sliding-window attention (config.layer_window of this layer): query q sees the keys
        # q - window < k <= q; None: plain causal
        self.window = window
        self.num_heads = config.num_heads
        self.head_dim = config.hidden_size // config.num_heads
        # grouped-query attention: num_kv_heads K/V heads, each shared by a group of
        # num_heads // num_kv_heads consecutive query heads (num_kv_heads == num_heads: MHA)
        self.num_kv_heads = config.num_kv_heads
        h, kv = config.hidden_size, config.num_kv_heads * self.head_dim
        self.q_proj = nn.Linear(h, h, bias=False)
        self.k_proj = nn.Linear(h, kv, bias=False)
        self.v_proj = nn.Linear(h, kv, bias=False)
        self.o_proj = nn.Linear(h, h, bias=False)
        # QK-norm (config.qk_norm): RMSNorm over head_dim on every query / key head before
        # RoPE, one weight per layer shared by the heads.  Without it the modules (and their
        # state-dict keys) do not exist.
        self.qk_norm = config.qk_norm
        if self.qk_norm:
            self.q_norm = RMSNorm(self.head_dim)
            self.k_norm = RMSNorm(self.head_dim)
        # Attention sinks (config.attention_sinks): one learned fp32 logit per query head in the
        # softmax denominator, no value row.  Without the flag the parameter does not exist.
        self.attention_sinks = config.attention_sinks
        if self.attention_sinks:
            self.sinks = nn.Parameter(torch.zeros(self.num_heads, dtype=torch.float32))
        self.attn_dropout = nn.Dropout(config.attention_dropout)
        self.resid_dropout = nn.Dropout(config.dropout)
        self.rotary_emb = RotaryPositionEmbedding(self.head_dim, config.max_seq_len)
        self.use_flash = config.use_flash_attention
        # Attention-score soft-capping (config.attn_softcap): fp32 scaled scores -> cap * tanh(s / cap)
        # before the masks; SDPA cannot express it, so a capped model takes the explicit formula
        self.attn_softcap = getattr(config, "attn_softcap", None)

    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                doc_hidden: Optional[torch.Tensor] = None, post_norm: Optional[nn.Module] = None):
        """``doc_hidden``: bool [B, 1, S, S], True where a query must not see a key because
        it lies before the query's document (``GPT.set_doc_separator``); applied on top of
        the causal mask in both the naive and the SDPA setting.  ``post_norm``: the block's
        attn_post_norm (config.post_norm), applied to the o_proj output before the dropout."""
        B, S, _ = hidden_states.shape
        q = self.q_proj(hidden_states).view(B, S, self.num_heads, self.head_dim).transpose(1, 2)
        k = self.k_proj(hidden_states).view(B, S, self.num_kv_heads, self.head_dim).transpose(1, 2)
        v = self.v_proj(hidden_states).view(B, S, self.num_kv_heads, self.head_dim).transpose(1, 2)
        if self.qk_norm:
            q, k = self.q_norm(q), self.k_norm(k)
        cos, sin = self.rotary_emb(q, S)
        q, k = apply_rotary_pos_emb(q, k, cos[None, None], sin[None, None])
        if self.num_kv_heads != self.num_heads:  # query head h uses kv head h // G
            G = self.num_heads // self.num_kv_heads
            k = k.repeat_interleave(G, dim=1)
            v = v.repeat_interleave(G, dim=1)
        if self.window is not None and self.window < S:  # keys k <= q - W are out of the window
            pos = torch.arange(S, device=hidden_states.device)
            out_of_window = (pos[None, :] <= pos[:, None] - self.window)[None, None]
            doc_hidden = out_of_window if doc_hidden is None else doc_hidden | out_of_window
        cap = self.attn_softcap
        if self.attention_sinks:  # SDPA cannot express the sink: the explicit formula in either setting
            scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(self.head_dim)
            if cap is not None:  # real scores only: the masks below still write -inf, the sink is not capped
                scores = (cap * torch.tanh(scores.float() / cap)).to(scores.dtype)
            mask = torch.triu(torch.ones(S, S, device=hidden_states.device, dtype=torch.bool), diagonal=1)
            mask = mask[None, None] if doc_hidden is None else mask[None, None] | doc_hidden
            scores = scores.masked_fill(mask, float("-inf"))
            # the sink is one more score column (not scaled, per query head, no value row)
            sink = self.sinks.float().view(1, self.num_heads, 1, 1).expand(B, -1, S, 1)
            probs = F.softmax(torch.cat([scores.float(), sink], dim=-1), dim=-1)[..., :S].to(scores.dtype)
            out = self.attn_dropout(probs) @ v
        elif cap is not None:  # SDPA cannot express the cap either
            scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(self.head_dim)
            scores = cap * torch.tanh(scores.float() / cap)
            mask = torch.triu(torch.ones(S, S, device=hidden_states.device, dtype=torch.bool), diagonal=1)
            mask = mask[None, None] if doc_hidden is None else mask[None, None] | doc_hidden
            scores = scores.masked_fill(mask, float("-inf"))
            probs = F.softmax(scores, dim=-1, dtype=torch.float32).to(q.dtype)
            out = self.attn_dropout(probs) @ v
        elif self.use_flash and doc_hidden is not None:
            causal = torch.tril(torch.ones(S, S, device=hidden_states.device, dtype=torch.bool))
            out = F.scaled_dot_product_attention(
                q, k, v, attn_mask=causal[None, None] & ~doc_hidden,
                dropout_p=self.config.attention_dropout if self.training else 0.0, is_causal=False)
        elif self.use_flash:
            out = F.scaled_dot_product_attention(
                q, k, v, attn_mask=None,
                dropout_p=self.config.attention_dropout if self.training else 0.0, is_causal=True)
        else:
            scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(self.head_dim)
            mask = torch.triu(torch.ones(S, S, device=hidden_states.device, dtype=torch.bool), diagonal=1)
            mask = mask[None, None] if doc_hidden is None else mask[None, None] | doc_hidden
            scores = scores.masked_fill(mask, float("-inf"))
            probs = F.softmax(scores, dim=-1, dtype=torch.float32).to(scores.dtype)
            out = self.attn_dropout(probs) @ v
        out = out.transpose(1, 2).contiguous().view(B, S, -1)
        out = self.o_proj(out)
        if post_norm is not None:
            out = post_norm(out)
        return self.resid_dropout(out)


class MLP(nn.Module):
    def __init__(self, config: GPTConfig):
        super().__init__()
        self.gate_proj = nn.Linear(config.hidden_size, config.intermediate_size, bias=False)
        self.up_proj = nn.Linear(config.hidden_size, config.intermediate_size, bias=False)
        self.down_proj = nn.Linear(config.intermediate_size, config.hidden_size, bias=False)
        self.dropout = nn.Dropout(config.dropout)

    def forward(self, x: torch.Tensor, post_norm: Optional[nn.Module] = None) -> torch.Tensor:
        """``post_norm``: the block's mlp_post_norm (config.post_norm), applied to the down_proj
        output before the dropout."""
        out = self.down_proj(F.silu(self.gate_proj(x)) * self.up_proj(x))
        if post_norm is not None:
            out = post_norm(out)
        return self.dropout(out)


class TransformerBlock(nn.Module):
    """Pre-norm block; the FSDP wrap unit and the activation-checkpoint unit."""

    def __init__(self, config: GPTConfig, layer_idx: int):
        super().__init__()
        self.layer_idx = layer_idx
        self.input_layernorm = RMSNorm(config.hidden_size)
        self.attention = CausalSelfAttention(config, config.layer_window(layer_idx))
        self.post_attention_layernorm = RMSNorm(config.hidden_size)
        self.mlp = MLP(config)
        # Post-norms (config.post_norm): a second RMSNorm on each branch output, before its
        # dropout and the residual add.  Without the flag the modules (and their state-dict
        # keys) do not exist; post_attention_layernorm stays the pre-MLP norm either way.
        self.post_norm = bool(getattr(config, "post_norm", False))
        if self.post_norm:
            self.attn_post_norm = RMSNorm(config.hidden_size)
            self.mlp_post_norm = RMSNorm(config.hidden_size)

    def forward(self, hidden_states, attention_mask=None, doc_hidden=None):
        if self.post_norm:
            h = hidden_states + self.attention(self.input_layernorm(hidden_states), attention_mask, doc_hidden,
                                               post_norm=self.attn_post_norm)
            return h + self.mlp(self.post_attention_layernorm(h), post_norm=self.mlp_post_norm)
        h = hidden_states + self.attention(self.input_layernorm(hidden_states), attention_mask, doc_hidden)
        return h + self.mlp(self.post_attention_layernorm(h))


class GPT(nn.Module):
    def __init__(self, config: GPTConfig):
        super().__init__()
        self.config = config
        self.embed_tokens = nn.Embedding(config.vocab_size, config.hidden_size)
        self.layers = nn.ModuleList([TransformerBlock(config, i) for i in range(config.num_layers)])
        self.norm = RMSNorm(config.hidden_size)
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.lm_head.weight = self.embed_tokens.weight  # tied
        self.gradient_checkpointing = config.gradient_checkpointing
        self.apply(self._init_weights)
        self.engine = None
        self.store = None
        self._anchor = None
        # intra-document attention mask (set_doc_separator); run-time state, not a
        # GPTConfig field: checkpoints and the pickled config are unchanged
        self.doc_sep_token: Optional[int] = None
        # auxiliary z-loss coefficient (set_z_loss): a property of the objective, likewise
        # run-time state; and the (cross-entropy, weighted z term) of the last forward with labels
        self.z_loss: float = 0.0
        self._loss_parts = None

    def set_z_loss(self, coef: float) -> None:
        """Auxiliary z-loss (PaLM): a forward with labels returns ``ce + coef * mean(z^2)``,
        ``z = logsumexp(logits)`` per predicted token, the mean over the tokens whose label
        is not ``ignore_index`` as for the cross-entropy.  It keeps the output logits from
        drifting to magnitudes at which a 16-bit lm_head loses its low bits; PaLM uses 1e-4.
        0 (the default) is plain cross-entropy.  ``last_loss_parts`` has the two parts.
        ``eval_loss`` / ``eval_loss_sum`` always report plain cross-entropy.  Applies to the
        eager path and to the engine (now or when it is enabled later).  Raises ValueError
        for a negative or non-finite coefficient."""
        from .engine import check_z_loss
        coef = check_z_loss(coef)
        if self.engine is not None:
            self.engine.set_z_loss(coef)
        self.z_loss = coef

    @property
    def last_loss_parts(self):
        """``(ce, z_term)`` of the last forward with labels: device scalars (no host sync) with
        ``ce + z_term == loss``; ``z_term`` is the weighted term, zero without a coefficient."""
        if self.engine is not None:
            return self.engine.last_loss_parts
        return self._loss_parts

    def set_doc_separator(self, token_id: Optional[int]) -> None:
        """Intra-document masking for packed training sequences: ``token_id`` (GPT-2:
        50256) ends a document and belongs to it, and every token attends only to the
        tokens of its own document at or before it.  ``None`` (the default) restores plain
        causal attention.  RoPE positions stay absolute and the loss is unchanged.  Applies
        to the eager path and to the engine (now or when it is enabled later); the engine
        raises NotImplementedError if its attention route has no mask."""
        token_id = None if token_id is None else int(token_id)
        if self.engine is not None:
            self.engine.set_doc_separator(token_id)
        self.doc_sep_token = token_id

    def _doc_hidden(self, input_ids: torch.Tensor) -> Optional[torch.Tensor]:
        """Eager path: the dense mask [B, 1, S, S] of keys before each query's document, or
        None when no separator is set or none precedes any token of the batch (the plain
        causal path then runs, bit for bit; one host sync, oracle / CPU path only)."""
        if self.doc_sep_token is None:
            return None
        from ..ops.reference import doc_bounds
        lo, _ = doc_bounds(input_ids, self.doc_sep_token)
        if not bool((lo > 0).any()):
            return None
        S = input_ids.shape[1]
        kpos = torch.arange(S, device=input_ids.device).view(1, 1, 1, S)
        return kpos < lo.view(lo.shape[0], 1, S, 1)

    def _init_weights(self, module):
        if isinstance(module, nn.Linear):
            torch.nn.init.normal_(module.weight, mean=0.0, std=self.config.initializer_range)
            if module.bias is not None:
                torch.nn.init.zeros_(module.bias)
        elif isinstance(module, nn.Embedding):
            torch.nn.init.normal_(module.weight, mean=0.0, std=self.config.initializer_range)

    # ------------------------------------------------------------ engine path
    def enable_engine(self, provider=None, ops=None, act_dtype=None, seed: int = 1234,
                      compute_dtype=None):
        """Switch to the fused executor.  Builds a FlatParamStore unless a provider
        (e.g. the FSDP runtime) is given.  Returns the engine."""
        from ..models.engine import GPTEngine
        from .. import ops as ops_mod
        dev = next(self.parameters()).device
        if act_dtype is None:
            act_dtype = torch.bfloat16 if dev.type == "cuda" else torch.float32
        if compute_dtype is None:
            compute_dtype = act_dtype
        if ops is None or ops.backend == "hip":  # before anything is re-homed
            ops_mod.check_attention_features(dev, self.config.head_dim, act_dtype,
                                             ops_mod.attn_routes.config_features(self.config))
            if getattr(self.config, "post_norm", False) and dev.type == "cuda" and act_dtype == torch.float32:
                raise NotImplementedError("this model on the GPU: fp32 activations have no post-norm kernels "
                                          "(post_norm); use bf16 or fp16 activations")
        if provider is None:
            from ..parallel.flat import FlatParamStore
            provider = FlatParamStore(self, dev, compute_dtype=compute_dtype)
            self.store = provider
        if ops is None:
            # bf16 / fp16 run the 16-bit HIP kernels (csrc/common.h HK), fp32 (the
            # reference / debug mode, --mixed_precision fp32) the fp32 ones (csrc/fp32.hip);
            # GEMMs go through the planner (hipBLASLt fp32 GEMMs in fp32 mode)
            ops = ops_mod.for_device(dev, head_dim=self.config.head_dim, act_dtype=act_dtype)
        gemm = None
        if dev.type == "cuda" and ops.backend == "hip":
            import os
            from ..ops import gemm as gemm_mod
            if os.environ.get("DLT_GEMM", "planner") == "planner" and gemm_mod.available():
                gemm = gemm_mod.HipGemm()
        self.engine = GPTEngine(self.config, provider, ops, act_dtype=act_dtype, seed=seed, gemm=gemm)
        if self.doc_sep_token is not None:
            self.engine.set_doc_separator(self.doc_sep_token)
        self.engine.set_z_loss(self.z_loss)
        self._anchor = torch.zeros((), device=dev, requires_grad=True)
        return self.engine

    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                labels: Optional[torch.Tensor] = None):
        """(logits [B, S, V], loss or None), as the reference (``gpt.py:388-455``).

        Divergence on the engine path: a TRAINING forward with labels (``self.training``
        and grad enabled) returns ``(None, loss)`` -- the fused lm_head + cross-entropy
        turns the logits buffer into dloss/dlogits in place, so full [B, S, V] logits are
        never materialised for the caller.  Eval mode, ``torch.no_grad()`` or a call
        without labels returns the logits as the reference does."""
        if self.engine is not None:
            return self._engine_forward(input_ids, labels)
        h = self.embed_tokens(input_ids)
        doc_hidden = self._doc_hidden(input_ids)
        for layer in self.layers:
            if self.gradient_checkpointing and self.training:
                h = checkpoint(layer, h, attention_mask, doc_hidden, use_reentrant=False)
            else:
                h = layer(h, attention_mask, doc_hidden)
        h = self.norm(h)
        logits = self.lm_head(h)
        cap = getattr(self.config, "logit_softcap", None)
        if cap is not None:  # the model's logits: fp32 from the rounded lm_head output
            logits = cap * torch.tanh(logits.float() / cap)
        loss = None
        if labels is not None:
            shift_logits = logits[..., :-1, :].contiguous()
            shift_labels = labels[..., 1:].contiguous()
            loss = F.cross_entropy(shift_logits.view(-1, self.config.vocab_size), shift_labels.view(-1))
            if self.z_loss != 0.0:
                valid = shift_labels.reshape(-1) != -100
                z = torch.logsumexp(shift_logits.view(-1, self.config.vocab_size).float(), dim=-1)[valid]
                ce, z_term = loss, self.z_loss * (z ** 2).sum() / valid.sum().clamp(min=1)
                loss = ce + z_term.to(ce.dtype)
                self._loss_parts = (ce.detach(), z_term.detach().to(ce.dtype))
            else:
                self._loss_parts = (loss.detach(), torch.zeros_like(loss))
        return logits, loss

    def _engine_forward(self, input_ids, labels):
        from .engine import EngineFunction, shift_targets
        eng = self.engine
        if labels is None:
            _, logits, _ = eng.forward(input_ids, None, train=self.training, need_backward=False)
            return logits, None
        targets = shift_targets(labels)
        recompute = bool(self.gradient_checkpointing)
        if self.training and torch.is_grad_enabled():
            loss = EngineFunction.apply(self._anchor, eng, input_ids, targets, recompute)
            return None, loss
        loss, logits, _ = eng.forward(input_ids, targets, train=self.training, need_backward=False,
                                      return_logits=True)
        return logits, loss

    # ------------------------------------------------------------ evaluation
    @torch.no_grad()
    def eval_loss_sum(self, input_ids: torch.Tensor, labels: Optional[torch.Tensor] = None):
        """(sum of the token losses, number of predicted tokens) of a held-out batch, without
        dropout whatever the module's mode; labels default to the inputs and are shifted as
        in :meth:`forward`.  Engine path: ``GPTEngine.eval_loss`` (no [B, S, V] logits);
        eager path: the same value from :meth:`forward`'s logits."""
        labels = input_ids if labels is None else labels
        if self.engine is not None:
            from .engine import shift_targets
            return self.engine.eval_loss(input_ids, shift_targets(labels))
        was_training = self.training
        self.eval()
        try:
            logits, _ = self(input_ids)
        finally:
            self.train(was_training)
        tgt = labels[..., 1:].reshape(-1)
        loss_sum = F.cross_entropy(logits[..., :-1, :].reshape(-1, self.config.vocab_size).float(), tgt,
                                   reduction="sum")
        return loss_sum, (tgt != -100).sum()

    def eval_loss(self, input_ids: torch.Tensor, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Mean next-token loss of a held-out batch (see :meth:`eval_loss_sum`)."""
        loss_sum, n = self.eval_loss_sum(input_ids, labels)
        return loss_sum / n.clamp(min=1).to(loss_sum.dtype)

    # ------------------------------------------------------------ generation
    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, max_new_tokens: int = 100,
                 temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0,
                 min_p: float = 0.0) -> torch.Tensor:
        """Top-k sampling with the reference's semantics (``gpt.py:457-484``), and on top of
        it nucleus (``top_p`` < 1) and min-p (``min_p`` > 0) filtering as
        ``eval.decode.filter_logits`` defines them; both are off by default.

        With the engine enabled this uses the KV-cached decoder in
        ``eval/decode.py`` (one token per step instead of a full re-forward).  The
        KV-cached decoder does not apply the document mask of ``set_doc_separator``:
        generation continues one document, so every cached key belongs to it."""
        self.eval()
        flush = getattr(getattr(self.engine, "provider", None), "flush_pending", None)
        if flush is not None:  # a recorded (lazy) optimizer step: the decoder reads every unit
            flush()
        from ..eval.decode import filter_logits, kv_cached_generate
        if self.engine is not None:
            return kv_cached_generate(self, input_ids, max_new_tokens, temperature, top_k, top_p, min_p)
        for _ in range(max_new_tokens):
            idx = input_ids if input_ids.size(1) <= self.config.max_seq_len else input_ids[:, -self.config.max_seq_len:]
            logits, _ = self(idx)
            logits = filter_logits(logits[:, -1, :] / temperature, top_k, top_p, min_p)
            probs = F.softmax(logits, dim=-1)
            nxt = torch.multinomial(probs, num_samples=1)
            input_ids = torch.cat([input_ids, nxt], dim=1)
        return input_ids


def count_parameters(model: nn.Module) -> int:
    return sum(p.numel() for p in model.parameters() if p.requires_grad)
