"""Class-specific attention relevance: gradient-weighted attention rollout (Chefer, Gur & Wolf, "Transformer Interpretability
Beyond Attention Visualization", ICCV 2021, arXiv 2103.15679, eqs. 5-6).

attention_rollout is the same whichever class is asked about, and input gradients skip the attention structure.  This method
joins the two.  With A_l layer l's softmax probabilities (B, H, S, S) and y_t the logit of the class asked about:

  A'_l = mean_h max(dy_t/dA_l * A_l, 0)          R = I;  for l = 0 .. L-1:  R <- R + A'_l R
  relevance = R[0, :] (CLS token), or the mean of R's rows (the mean-pooled raw-IQ head, as attention_rollout starts)

Each chunk of `batch` frames runs one eval-mode forward of the plan model.forward uses, then one native call
(iq_model_attention_relevance, csrc/model.hip) on the same stream and workspace.  That call carries the one-hot logit gradient
down the data-only backward chain (no parameter gradient).  As each layer's attention-output gradient dO appears, from the
top layer down, it forms the layer's gradient-weighted map and the row step r <- r (I + A'_l) (csrc/attn_maps.hip).  No S x S
matrix and no per-layer dO is kept.

  attention_relevance(model, src, target=None, batch=256)                                          (B, S) fp32
  grad_attention_maps(model, src, target=None, layers=None, query="cls", heads="mean", positive=True, batch=256)
      dy_t/dA_l * A_l read back per layer, in the layout of attention_maps: (B, L', H', S), or (B, L', H', S, S) for
      query="all"; positive=True clamps at 0 per head before the head mean, False gives the signed product

target: None (the class the same forward predicts), an int, or a (B,) integer tensor.  `model` is an AMCTransformerViT or
AMCTransformerRawIQ (a model with logits).  The module's `training` flag and every `p.grad` are left alone.  Like any later
forward, a call makes a pending backward() of an earlier forward raise.  The (B, S) result goes to rollout_to_input unchanged.
There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import operator

import torch

from . import _native as N
from .attention_maps import _HEADS, _QUERY, _tokens
from .saliency import _batch, _classes, _resolve


def _run(model, src, target, batch, sel, query, heads, positive, want_rel):
    """Validate, then per chunk: eval forward -> one-hot dlogits -> iq_model_attention_relevance.  -> (rel, maps)"""
    enc, plan_of, K = _resolve(model)
    g = enc._geom
    n_layers, n_head = g["n_layers"], g["n_head"]
    if query not in _QUERY:
        raise ValueError(f"query must be one of {sorted(_QUERY)}, got {query!r}")
    if heads not in _HEADS:
        raise ValueError(f"heads must be one of {sorted(_HEADS)}, got {heads!r}")
    if not isinstance(positive, bool):
        raise TypeError(f"positive must be a bool, got {type(positive).__name__}")
    if query == "cls" and not _tokens(g)[1]:
        raise ValueError("query='cls' needs a CLS token; this model has none (use query='mean' or 'all')")
    sel = list(range(n_layers)) if sel is None else [operator.index(l) for l in sel]
    for l in sel:
        if not 0 <= l < n_layers:
            raise ValueError(f"layer index {l} out of range for {n_layers} layers")
    if len(set(sel)) != len(sel):
        raise ValueError(f"layer indices must be distinct, got {sel}")
    batch = _batch(batch)
    n = src.shape[0] if isinstance(src, torch.Tensor) and src.dim() > 0 else 0
    tgt = None if target is None else _classes(target, n, K, "target")
    src = enc._expect(src)
    plan = plan_of()
    B, S = src.shape[0], plan.S
    hn = n_head if heads == "all" else 1
    per_layer = hn * S * (S if query == "all" else 1)
    bstride = len(sel) * per_layer
    shape = (B, len(sel), hn, S, S) if query == "all" else (B, len(sel), hn, S)
    maps = torch.empty(shape, dtype=torch.float32, device=src.device) if sel else None
    rel = torch.empty(B, S, dtype=torch.float32, device=src.device) if want_rel else None
    ptrs = (C.c_void_p * max(1, n_layers))()
    with torch.no_grad():
        if tgt is not None:
            tgt = tgt.to(src.device)
        for i in range(0, B, batch):
            xb = src[i:i + batch]
            nb = xb.shape[0]
            logits = plan.forward(xb, False, True, False)[0]
            t = logits.argmax(1) if tgt is None else tgt[i:i + nb]
            dl = torch.nn.functional.one_hot(t, K).float()
            for l in range(n_layers):
                ptrs[l] = None
            for j, l in enumerate(sel):
                ptrs[l] = maps.data_ptr() + 4 * (i * bstride + j * per_layer)     # maps[i:, j], frames bstride apart
            N.check(plan.L.iq_model_attention_relevance(plan.h, N.ptr(dl), nb, N.ptr(plan.ws), plan.ws.numel(),
                                                        None if rel is None else rel.data_ptr() + 4 * i * S, ptrs,
                                                        _QUERY[query], _HEADS[heads], int(positive), bstride,
                                                        N.stream_handle()), "iq_model_attention_relevance", plan.h)
    return rel, maps


def attention_relevance(model, src, target=None, batch=256):
    return _run(model, src, target, batch, [], "all", "mean", True, True)[0]


def grad_attention_maps(model, src, target=None, layers=None, query="cls", heads="mean", positive=True, batch=256):
    if layers is not None and len(layers) == 0:
        raise ValueError("layers must name at least one layer")
    return _run(model, src, target, batch, layers, query, heads, positive, False)[1]
