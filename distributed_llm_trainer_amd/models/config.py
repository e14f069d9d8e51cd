"""Model hyper-parameters (``GPTConfig``) and the GPT-2-named presets.

Parity target: ``src/models/config.py:6-102`` of the reference.  Same field names,
defaults and the four ``gpt2_*`` presets, so YAML / pickled configs from the
reference map 1:1 onto this class.

Intentional divergences (documented in SURVEY.md §7.1 / Appendix A):

* ``num_parameters()`` returns the *true* parameter count of the LLaMA-style block
  (RMSNorm + SwiGLU + RoPE + tied head).  The reference formula
  (``config.py:81-102``) assumes a classic GPT-2 layout and under-reports; it is kept
  as ``num_parameters_legacy()`` for comparison (Q4).
* ``activation`` is kept for schema compatibility; as in the reference it is not read
  by the model (the MLP is SwiGLU, ``gpt.py:245-283``).
* ``vocab_size_padded`` is the lm_head GEMM width used internally by the fused MI355X
  path (multiple of 64 so the bf16 weight rows stay 128-B aligned for MFMA tiles);
  the state dict still carries exactly ``vocab_size`` rows.
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass, fields
from typing import Any, Dict, Optional


@dataclass
class GPTConfig:
    """Configuration for the GPT model.  Defaults are the "GPT-2 124M" preset."""

    # Model architecture
    vocab_size: int = 50257
    hidden_size: int = 768
    num_layers: int = 12
    num_heads: int = 12
    intermediate_size: Optional[int] = None  # defaults to 4 * hidden_size
    max_seq_len: int = 1024

    # Regularization
    dropout: float = 0.1
    attention_dropout: float = 0.1

    # Initialization
    initializer_range: float = 0.02

    # Activation (schema-compat only; the block is SwiGLU like the reference)
    activation: str = "gelu"

    # Optimization flags
    use_flash_attention: bool = False
    gradient_checkpointing: bool = False

    # Grouped-query attention: K/V heads (None = num_heads, plain multi-head attention;
    # 1 = multi-query).  Query head h attends with kv head h // (num_heads // num_kv_heads).
    num_kv_heads: Optional[int] = None

    # QK-norm (Qwen3 form): an RMSNorm over head_dim, with one [head_dim] weight per layer for
    # the query heads (q_norm) and one for the key heads (k_norm), applied before RoPE.
    qk_norm: bool = False

    # Attention sinks (gpt-oss form): one learned fp32 logit per query head that takes part in
    # the softmax denominator and has no value row: p_j = exp(s_j) / (sum_j exp(s_j) + exp(sink)).
    attention_sinks: bool = False

    # Post-norms (the Gemma-2/3 "sandwich" block, Grok-1 too): a second RMSNorm over hidden_size on
    # each branch output, before the hidden dropout and the residual add:
    # h + dropout(attn_post_norm(attention(input_layernorm(h)))), likewise mlp_post_norm.
    post_norm: bool = False

    # Final-logit soft-capping (Gemma-2's rule, cap 30 there): the model's logits are
    # cap * tanh(lm_head(norm(h)) / cap), in training, evaluation and generation alike.  None = off.
    logit_softcap: Optional[float] = None

    # Attention-score soft-capping (the other half of Gemma-2's rule, cap 50 there; Grok-1 too):
    # every layer's scaled scores are cap * tanh(scale * q.k / cap) before the masks and the
    # softmax; masked keys stay at -inf and a sink is not capped.  None = off.
    attn_softcap: Optional[float] = None

    # Sliding-window (local) attention: query q sees key k iff q - W < k <= q, W keys with its
    # own (the Mistral / Gemma rule).  With sliding_window_pattern = N, layer i (0-based) is
    # global (plain causal) iff (i + 1) % N == 0 (Gemma-3's rule); unset, every layer is windowed.
    sliding_window: Optional[int] = None
    sliding_window_pattern: Optional[int] = None

    def __post_init__(self) -> None:
        if self.intermediate_size is None:
            self.intermediate_size = 4 * self.hidden_size
        assert self.hidden_size % self.num_heads == 0, (
            f"hidden_size ({self.hidden_size}) must be divisible by num_heads ({self.num_heads})"
        )
        if self.num_kv_heads is None:
            self.num_kv_heads = self.num_heads
        if self.num_kv_heads < 1 or self.num_heads % self.num_kv_heads != 0:
            raise ValueError(
                f"num_kv_heads ({self.num_kv_heads}) must divide num_heads ({self.num_heads})")
        self.qk_norm = bool(self.qk_norm)
        if not isinstance(self.attention_sinks, (bool, int)) or self.attention_sinks not in (0, 1):
            raise ValueError(f"attention_sinks ({self.attention_sinks!r}) must be a bool")
        self.attention_sinks = bool(self.attention_sinks)
        if not isinstance(self.post_norm, (bool, int)) or self.post_norm not in (0, 1):
            raise ValueError(f"post_norm ({self.post_norm!r}) must be a bool")
        self.post_norm = bool(self.post_norm)
        if self.sliding_window is not None:
            if isinstance(self.sliding_window, bool) or int(self.sliding_window) != self.sliding_window \
                    or self.sliding_window < 1:
                raise ValueError(f"sliding_window ({self.sliding_window!r}) must be an integer >= 1")
            self.sliding_window = int(self.sliding_window)
        if self.sliding_window_pattern is not None:
            n = self.sliding_window_pattern
            if self.sliding_window is None:
                raise ValueError("sliding_window_pattern needs sliding_window")
            if isinstance(n, bool) or int(n) != n or n < 2:
                raise ValueError(f"sliding_window_pattern ({n!r}) must be an integer >= 2")
            self.sliding_window_pattern = int(n)
        if self.logit_softcap is not None:
            c = self.logit_softcap
            if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c <= 0:
                raise ValueError(f"logit_softcap ({c!r}) must be a finite float > 0")
            self.logit_softcap = float(c)
        if self.attn_softcap is not None:
            c = self.attn_softcap
            if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c <= 0:
                raise ValueError(f"attn_softcap ({c!r}) must be a finite float > 0")
            self.attn_softcap = float(c)

    # ------------------------------------------------------------------ presets
    @classmethod
    def gpt2_small(cls) -> "GPTConfig":
        """"GPT-2 124M" preset (151,862,784 real parameters)."""
        return cls(vocab_size=50257, hidden_size=768, num_layers=12, num_heads=12)

    @classmethod
    def gpt2_medium(cls) -> "GPTConfig":
        """"GPT-2 355M" preset (454,166,528 real parameters)."""
        return cls(vocab_size=50257, hidden_size=1024, num_layers=24, num_heads=16)

    @classmethod
    def gpt2_large(cls) -> "GPTConfig":
        """"GPT-2 774M" preset (1,008,140,800 real parameters)."""
        return cls(vocab_size=50257, hidden_size=1280, num_layers=36, num_heads=20)

    @classmethod
    def gpt2_xl(cls) -> "GPTConfig":
        """"GPT-2 1.5B" preset (2,046,646,400 real parameters, 25 heads)."""
        return cls(vocab_size=50257, hidden_size=1600, num_layers=48, num_heads=25)

    @classmethod
    def from_preset(cls, name: str) -> "GPTConfig":
        name = name.lower().replace("gpt2-", "").replace("gpt2_", "")
        table = {"small": cls.gpt2_small, "medium": cls.gpt2_medium,
                 "large": cls.gpt2_large, "xl": cls.gpt2_xl}
        if name not in table:
            raise ValueError(f"unknown model preset {name!r}; choose from {sorted(table)}")
        return table[name]()

    # ------------------------------------------------------------- derived
    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads

    @property
    def vocab_size_padded(self) -> int:
        return ((self.vocab_size + 63) // 64) * 64

    @property
    def kv_size(self) -> int:
        """Width of the K (and of the V) projection: num_kv_heads * head_dim."""
        return self.num_kv_heads * self.head_dim

    def layer_window(self, i: int) -> Optional[int]:
        """Window of layer ``i`` (0-based), or None when that layer is global (plain causal).

        The one place that decides which layers are windowed."""
        w = self.__dict__.get("sliding_window")
        if w is None:
            return None
        n = self.__dict__.get("sliding_window_pattern")
        if n is not None and (i + 1) % n == 0:
            return None
        return w

    def num_parameters(self) -> int:
        """True trainable parameter count (tied embedding counted once)."""
        h, i = self.hidden_size, self.intermediate_size
        per_layer = 2 * h * h + 2 * self.kv_size * h + 3 * h * i + 2 * h
        if self.qk_norm:
            per_layer += 2 * self.head_dim  # q_norm, k_norm
        if self.attention_sinks:
            per_layer += self.num_heads  # sinks
        if self.post_norm:
            per_layer += 2 * h  # attn_post_norm, mlp_post_norm
        return self.vocab_size * h + self.num_layers * per_layer + h

    def num_parameters_legacy(self) -> int:
        """The reference's classic-GPT-2 estimate (``config.py:81-102``), kept for parity."""
        embed = self.vocab_size * self.hidden_size
        pos = self.max_seq_len * self.hidden_size
        layer = 4 * self.hidden_size ** 2 + 2 * self.hidden_size * self.intermediate_size + 4 * self.hidden_size
        return embed + pos + self.num_layers * layer + 2 * self.hidden_size

    def flops_per_token(self, seq_len: Optional[int] = None, causal: bool = True,
                        recompute: bool = False) -> float:
        """Training FLOPs per token (fwd + bwd = 3x fwd; +1 fwd with recompute).

        Attention score/value FLOPs are counted for the causal half when ``causal``; a windowed
        layer counts the ``W*(2S-W+1)/(2S)`` keys a query sees on average instead of ``(S+1)/2``.
        """
        s = seq_len or self.max_seq_len
        h, i, L, v = self.hidden_size, self.intermediate_size, self.num_layers, self.vocab_size
        dense = 2 * (2 * h * h + 2 * self.kv_size * h + 3 * h * i) * L + 2 * h * v
        attn = 2 * 2 * s * h * L * (0.5 if causal else 1.0)
        if causal and self.sliding_window is not None:
            attn = 0.0
            for li in range(L):
                w = self.layer_window(li)
                if w is None:  # a global layer of a pattern model: the causal half, as above
                    keys = 0.5 * s
                else:  # sum_q min(q + 1, W) / S
                    w = min(w, s)
                    keys = w * (2 * s - w + 1) / (2.0 * s)
                attn += 2 * 2 * h * keys
        fwd = dense + attn
        return fwd * (4.0 if recompute else 3.0)

    # ------------------------------------------------------------- (de)serialise
    def to_dict(self) -> Dict[str, Any]:
        d = asdict(self)
        if self.num_kv_heads == self.num_heads:  # MHA configs stay what they were
            del d["num_kv_heads"]
        if not self.qk_norm:  # ... and so do configs without QK-norm
            del d["qk_norm"]
        if not self.attention_sinks:  # ... and configs without attention sinks
            del d["attention_sinks"]
        if not self.post_norm:  # ... and configs without post-norms
            del d["post_norm"]
        for k in ("sliding_window", "sliding_window_pattern", "logit_softcap", "attn_softcap"):  # ... and unwindowed / uncapped ones
            if d[k] is None:
                del d[k]
        return d

    # Pickled configs (checkpoints) follow to_dict(): an MHA config carries no num_kv_heads, one
    # without QK-norm no qk_norm, one without sinks no attention_sinks and one without post-norms
    # no post_norm, so their pickles are
    # what they were before the fields existed and older pickles load.
    def __getstate__(self) -> Dict[str, Any]:
        state = dict(self.__dict__)
        if state.get("num_kv_heads") == state.get("num_heads"):
            state.pop("num_kv_heads", None)
        if not state.get("qk_norm"):
            state.pop("qk_norm", None)
        if not state.get("attention_sinks"):
            state.pop("attention_sinks", None)
        if not state.get("post_norm"):
            state.pop("post_norm", None)
        for k in ("sliding_window", "sliding_window_pattern", "logit_softcap", "attn_softcap"):
            if state.get(k) is None:
                state.pop(k, None)
        return state

    def __setstate__(self, state: Dict[str, Any]) -> None:
        self.__dict__.update(state)
        if self.__dict__.get("num_kv_heads") is None:
            self.num_kv_heads = self.num_heads
        self.qk_norm = bool(self.__dict__.get("qk_norm", False))
        self.attention_sinks = bool(self.__dict__.get("attention_sinks", False))
        self.post_norm = bool(self.__dict__.get("post_norm", False))
        self.__dict__.setdefault("sliding_window", None)
        self.__dict__.setdefault("sliding_window_pattern", None)
        self.__dict__.setdefault("logit_softcap", None)
        self.__dict__.setdefault("attn_softcap", None)

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "GPTConfig":
        names = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in d.items() if k in names})
