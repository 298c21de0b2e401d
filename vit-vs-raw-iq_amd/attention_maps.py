"""Attention maps and attention rollout from the fused forward pass.

The reference's MultiHeadAttention.forward receives every layer's attention matrix and drops it
(V/models/layers/multi_head_attention.py:24,30, "5. visualize attention map").  Here the whole-model plan never forms that
matrix, but an eval forward leaves each layer's packed bf16 q|k|v and fp32 log-sum-exp in the plan's workspace; the native
read-back (iq_model_attention / iq_model_attention_rollout, csrc/attn_maps.hip) rebuilds the probabilities from them with
the same products the forward used.

  attention_maps(model, src, layers=None, query="cls", heads="mean", batch=256)
      query "cls" | "mean" -> (B, L', H', S) fp32 on the model's device;  "all" -> (B, L', H', S, S)
      heads "mean" -> H' = 1, "all" -> H' = n_head;  layers: None (all) or a list of layer indices (L' = len)
  attention_rollout(model, src, alpha=0.5, batch=256)     (B, S), rows sum to 1 (Abnar & Zuidema 2020)
  rollout_to_input(model, roll)   ViT: (B, img_h, img_w); raw IQ: (B, seq_length) -- each token's value over the input
                                  it was embedded from, the CLS entry dropped

`model` is an AMCTransformerViT / AMCTransformerRawIQ or an Encoder*, standing alone or owned by one; the plan its forward
would run is used.  Every chunk of `batch` frames runs one eval-mode forward of that plan (the module's `training` flag is not
touched) and then the read-back on the same stream and workspace.  Like any later forward, it makes a pending backward() of
an earlier forward raise.  There is no CPU path.
"""
from __future__ import annotations

import operator

import torch

from . import _native as N
from .modules import AMCTransformerRawIQ, AMCTransformerViT, EncoderRawIQ, EncoderViT, NativePlan, _parent_of

_QUERY = {"all": 0, "cls": 1, "mean": 2}      # iq_attn_probs `rows`
_HEADS = {"all": 0, "mean": 1}                # iq_attn_probs `heads`


def _resolve(model):
    """-> (encoder, function returning the plan model.forward runs)"""
    if isinstance(model, (AMCTransformerViT, AMCTransformerRawIQ)):
        return model.encoder, model.native_plan
    if isinstance(model, (EncoderViT, EncoderRawIQ)):
        parent = _parent_of(model)
        if parent is not None:
            return model, parent.native_plan

        def own():
            if model._plan is None:
                model._plan = NativePlan(model, model._cfg(), prefix_strip="encoder.")
            return model._plan
        return model, own
    raise TypeError(f"expected an AMCTransformerViT, AMCTransformerRawIQ, EncoderViT or EncoderRawIQ, got {type(model).__name__}")


def _tokens(g):
    """(tokens, has_cls) of an encoder geometry"""
    if g["kind"] == 0:
        return (g["img_h"] // g["patch"]) * (g["img_w"] // g["patch"]), True
    return g["seq_length"] // g["conv_k"], bool(g["use_cls"])


def _batch(batch):
    b = operator.index(batch)
    if b <= 0:
        raise ValueError(f"batch must be positive, got {batch}")
    return b


def _chunks(plan: NativePlan, src: torch.Tensor, batch: int):
    """Yield (first frame, frames) after an eval forward of each chunk in the plan's workspace."""
    for i in range(0, src.shape[0], batch):
        xb = src[i:i + batch]
        plan.forward(xb, False, False, False)
        yield i, xb.shape[0]


def attention_maps(model, src, layers=None, query="cls", heads="mean", batch=256):
    enc, plan_of = _resolve(model)
    g = enc._geom
    n_layers, n_head = g["n_layers"], g["n_head"]
    if query not in _QUERY:
        raise ValueError(f"query must be one of {sorted(_QUERY)}, got {query!r}")
    if heads not in _HEADS:
        raise ValueError(f"heads must be one of {sorted(_HEADS)}, got {heads!r}")
    tok, cls = _tokens(g)
    if query == "cls" and not cls:
        raise ValueError("query='cls' needs a CLS token; this model has none (use query='mean' or 'all')")
    sel = list(range(n_layers)) if layers is None else [operator.index(l) for l in layers]
    for l in sel:
        if not 0 <= l < n_layers:
            raise ValueError(f"layer index {l} out of range for {n_layers} layers")
    batch = _batch(batch)
    src = enc._expect(src)
    plan = plan_of()
    B, S = src.shape[0], plan.S
    rows, hd = _QUERY[query], _HEADS[heads]
    hn = n_head if heads == "all" else 1
    shape = (B, len(sel), hn, S, S) if query == "all" else (B, len(sel), hn, S)
    out = torch.empty(shape, dtype=torch.float32, device=src.device)
    per_layer = hn * S * (S if query == "all" else 1)
    bstride = len(sel) * per_layer
    with torch.no_grad():
        for i, nb in _chunks(plan, src, batch):
            for j, l in enumerate(sel):
                dst = out.data_ptr() + 4 * (i * bstride + j * per_layer)      # out[i:, j], frames bstride apart
                N.check(plan.L.iq_model_attention(plan.h, N.ptr(plan.ws), plan.ws.numel(), nb, l, rows, hd, dst, bstride,
                                                  N.stream_handle()), "iq_model_attention", plan.h)
    return out


def attention_rollout(model, src, alpha=0.5, batch=256):
    enc, plan_of = _resolve(model)
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], got {alpha}")
    batch = _batch(batch)
    src = enc._expect(src)
    plan = plan_of()
    B, S = src.shape[0], plan.S
    out = torch.empty(B, S, dtype=torch.float32, device=src.device)
    with torch.no_grad():
        for i, nb in _chunks(plan, src, batch):
            N.check(plan.L.iq_model_attention_rollout(plan.h, N.ptr(plan.ws), plan.ws.numel(), nb, alpha,
                                                      out.data_ptr() + 4 * i * S, N.stream_handle()),
                    "iq_model_attention_rollout", plan.h)
    return out


def rollout_to_input(model, roll):
    """Token values (B, S) on the input frame: ViT (B, img_h, img_w), every patch's value over its p x p pixels (tokens in
    row-major patch-grid order, as the patch embedding flattens them), 0 outside the grid; raw IQ (B, seq_length), every
    token's value over its segment (conv1d: one sample per token).  The CLS entry is dropped."""
    enc, _ = _resolve(model)
    g = enc._geom
    tok, cls = _tokens(g)
    if not isinstance(roll, torch.Tensor) or roll.dim() != 2 or roll.shape[1] != tok + int(cls):
        raise ValueError(f"expected a (batch, {tok + int(cls)}) tensor, got "
                         f"{tuple(roll.shape) if isinstance(roll, torch.Tensor) else type(roll).__name__}")
    t = roll[:, 1:] if cls else roll
    B = roll.shape[0]
    if g["kind"] == 0:
        p = g["patch"]
        gh, gw = g["img_h"] // p, g["img_w"] // p
        img = roll.new_zeros(B, g["img_h"], g["img_w"])
        img[:, :gh * p, :gw * p] = t.reshape(B, gh, gw).repeat_interleave(p, dim=1).repeat_interleave(p, dim=2)
        return img
    return t.repeat_interleave(g["conv_k"], dim=1)
