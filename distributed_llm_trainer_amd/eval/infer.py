"""Text generation from a checkpoint (CLI parity with ``src/eval/infer.py:34-70``).

Differences: checkpoints load with ``weights_only=True`` (config classes are
registered safe globals, including the reference's module paths -- no arbitrary
unpickling, and no placeholder-class hack needed); generation runs the KV-cached
decoder on the fused engine when a GPU is present; the tokenizer resolves offline
(``--tokenizer byte`` works without any downloaded files).
"""
from __future__ import annotations

import argparse

import torch

from ..data.tokenizer import get_tokenizer
from ..models.config import GPTConfig
from ..models.gpt import GPT
from ..utils.checkpoint import load_checkpoint, load_model_state


def pick_device(name: str) -> torch.device:
    if name != "auto":
        return torch.device(name)
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def load_model(path: str, model_size: str = None, device="cpu", num_kv_heads: int = None, qk_norm: bool = None,
               sliding_window: int = None, sliding_window_pattern: int = None, attention_sinks: bool = None,
               logit_softcap: float = None, attn_softcap: float = None, post_norm: bool = None):
    """The model of a checkpoint: built from the checkpoint's own config (which carries
    num_kv_heads for a grouped-query model) unless ``model_size`` names a preset;
    ``num_kv_heads`` overrides either, and so does ``qk_norm`` (the checkpoint's config carries
    it for a QK-norm model), ``sliding_window`` and ``sliding_window_pattern`` (a windowed model's
    config carries them too), ``attention_sinks`` (carried by the config of a model with sinks) and
    ``logit_softcap`` (the final-logit cap, carried by the config of a model trained with one) and
    ``attn_softcap`` (the attention-score cap, carried likewise) and ``post_norm`` (the post-norms,
    carried by the config of a model that has them)."""
    ckpt = load_checkpoint(path, map_location="cpu")
    cfg = ckpt.get("model_config")
    if model_size is not None or not isinstance(cfg, GPTConfig):
        cfg = GPTConfig.from_preset(model_size or "small")
    if num_kv_heads is not None:
        cfg = GPTConfig.from_dict({**cfg.to_dict(), "num_kv_heads": num_kv_heads})
    if qk_norm is not None:
        cfg = GPTConfig.from_dict({**cfg.to_dict(), "qk_norm": bool(qk_norm)})
    if sliding_window is not None:
        cfg = GPTConfig.from_dict({**cfg.to_dict(), "sliding_window": sliding_window})
    if sliding_window_pattern is not None:
        cfg = GPTConfig.from_dict({**cfg.to_dict(), "sliding_window_pattern": sliding_window_pattern})
    if attention_sinks is not None:
        cfg = GPTConfig.from_dict({**cfg.to_dict(), "attention_sinks": bool(attention_sinks)})
    if logit_softcap is not None:
        cfg = GPTConfig.from_dict({**cfg.to_dict(), "logit_softcap": logit_softcap})
    if attn_softcap is not None:
        cfg = GPTConfig.from_dict({**cfg.to_dict(), "attn_softcap": attn_softcap})
    if post_norm is not None:
        cfg = GPTConfig.from_dict({**cfg.to_dict(), "post_norm": bool(post_norm)})
    model = GPT(cfg)
    load_model_state(model, ckpt["model"])
    model = model.to(device)
    if torch.device(device).type == "cuda":
        model.enable_engine()
    model.eval()
    return model


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--checkpoint", required=True)
    p.add_argument("--model_size", default=None, choices=["small", "medium", "large", "xl"])
    p.add_argument("--prompt", default="Once upon a time,")
    p.add_argument("--max_new_tokens", type=int, default=50)
    p.add_argument("--device", default="auto")
    p.add_argument("--temperature", type=float, default=1.0)
    p.add_argument("--top_k", type=int, default=50)
    p.add_argument("--top_p", type=float, default=1.0,
                   help="nucleus sampling: keep the smallest set of top tokens whose probability reaches top_p (1: off)")
    p.add_argument("--min_p", type=float, default=0.0,
                   help="keep the tokens with probability >= min_p * the top token's (0: off)")
    p.add_argument("--tokenizer", default="gpt2")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--num_kv_heads", type=int, default=None, metavar="N",
                   help="key/value heads of a grouped-query checkpoint whose config does not carry them")
    p.add_argument("--qk_norm", action="store_true", default=None,
                   help="the checkpoint is a QK-norm model (q_norm / k_norm weights) whose config does not say so")
    p.add_argument("--sliding_window", type=int, default=None, metavar="W",
                   help="window of a sliding-window checkpoint whose config does not carry it")
    p.add_argument("--sliding_window_pattern", type=int, default=None, metavar="N",
                   help="every N-th layer of that checkpoint is global (plain causal)")
    p.add_argument("--attention_sinks", action="store_true", default=None,
                   help="the checkpoint has attention sinks (a sinks vector per layer) and its config does not say so")
    p.add_argument("--logit_softcap", type=float, default=None, metavar="CAP",
                   help="final-logit soft cap of a checkpoint trained with one whose config does not carry it")
    p.add_argument("--attn_softcap", type=float, default=None, metavar="CAP",
                   help="attention-score soft cap of a checkpoint trained with one whose config does not carry it")
    p.add_argument("--post_norm", action="store_true", default=None,
                   help="the checkpoint has post-norms (attn_post_norm / mlp_post_norm weights) and its config "
                        "does not say so")
    args = p.parse_args(argv)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    dev = pick_device(args.device)
    model = load_model(args.checkpoint, args.model_size, dev, args.num_kv_heads, args.qk_norm, args.sliding_window,
                       args.sliding_window_pattern, args.attention_sinks, args.logit_softcap,
                       args.attn_softcap, args.post_norm)
    tok = get_tokenizer(args.tokenizer)
    ids = torch.tensor([tok.encode(args.prompt)], dtype=torch.long, device=dev)
    out = model.generate(ids, max_new_tokens=args.max_new_tokens, temperature=args.temperature, top_k=args.top_k,
                         top_p=args.top_p, min_p=args.min_p)
    text = tok.decode(out[0].tolist())
    print(text)
    return text


if __name__ == "__main__":
    main()
