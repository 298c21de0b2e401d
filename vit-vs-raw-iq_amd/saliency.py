"""Input gradients of the fused model: gradient saliency and integrated gradients.

The reference's AMCTransformer is a plain nn.Module, so `x.requires_grad_()`, `model(x)`, `loss.backward()` fills `x.grad`;
here the same works through the whole-model plan (modules._PlanFn).  The functions below skip autograd altogether: each chunk
of `batch` frames runs one eval-mode forward of the plan model.forward uses, the head gradient is formed on the device, and
iq_model_backward_input carries it down the chain to the input (csrc/model.hip, csrc/embed_dgrad.hip) without forming any
parameter gradient.  The module's `training` flag and every `p.grad` are left alone.  Like any later forward, a call makes a
pending backward() of an earlier forward raise.  There is no CPU path.

  input_gradient(model, src, target=None, batch=256)          d logit[target] / d src; target None = the predicted class
  input_gradient(model, src, labels=y, batch=256)              d CE(logits, y) / d src (per frame: the loss is not averaged)
  integrated_gradients(model, src, target=None, baseline=None, steps=32, batch=256)
      (src - baseline) * mean_k grad(baseline + (k + 1/2)/steps (src - baseline)), k < steps (midpoint Riemann sum);
      baseline None = zeros.  sum(attr) approximates logit[target](src) - logit[target](baseline).

Every result has the shape of `src`, fp32 on its device.  Gradients are with respect to the model's input, which is the
z-scored frame (data.py, iq_frames_preprocess); the z-score is a per-channel affine x = (raw - mean) / std, so
d/d raw = (d/d x) / std channel by channel.
"""
from __future__ import annotations

import operator

import torch

from . import _native as N
from .modules import AMCTransformerRawIQ, AMCTransformerViT, NativePlan


def _resolve(model):
    """-> (encoder, function returning the plan model.forward runs, number of classes)"""
    if isinstance(model, (AMCTransformerViT, AMCTransformerRawIQ)):
        return model.encoder, model.native_plan, model._num_classes
    raise TypeError(f"expected an AMCTransformerViT or AMCTransformerRawIQ (a model with logits), got {type(model).__name__}")


def _batch(batch):
    b = operator.index(batch)
    if b <= 0:
        raise ValueError(f"batch must be positive, got {batch}")
    return b


def _classes(v, B, K, what):
    """An int or an integer tensor of shape (B,) / () with values in [0, K) -> int64 tensor (B,) on the CPU or its device."""
    if isinstance(v, bool):
        raise TypeError(f"{what} must be an int or an integer tensor, got bool")
    if isinstance(v, int):
        if not 0 <= v < K:
            raise ValueError(f"{what} {v} out of range for {K} classes")
        return torch.full((B,), v, dtype=torch.int64)
    t = torch.as_tensor(v)
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise TypeError(f"{what} must hold integers, got {t.dtype}")
    if t.dim() == 0:
        t = t.expand(B)
    if tuple(t.shape) != (B,):
        raise ValueError(f"{what} must have shape ({B},), got {tuple(t.shape)}")
    if B and (int(t.min()) < 0 or int(t.max()) >= K):
        raise ValueError(f"{what} values must be in [0, {K})")
    return t.to(torch.int64)


def _forward(plan: NativePlan, xb):
    """Eval forward of one chunk in the plan's workspace -> logits (B, K) fp32."""
    return plan.forward(xb, False, True, False)[0]


def _ce_grad(plan: NativePlan, logits, labels):
    """d CE(logits, labels) / d logits per frame (smoothing 0, not averaged) on the device."""
    B, K = logits.shape
    dl = torch.empty_like(logits)
    N.check(plan.L.iq_ce_fwd_bwd(N.ptr(logits), N.ptr(labels), B, K, 0.0, 1.0, None, None, N.ptr(dl), N.stream_handle()),
            "iq_ce_fwd_bwd")
    return dl


def _input_grad(plan: NativePlan, xb, dlogits):
    """d(<dlogits, logits>) / d xb of the forward that has just run on xb (no parameter gradient is formed)."""
    dsrc = torch.empty_like(xb)
    plan.backward_input(xb.shape[0], dlogits, None, dsrc)
    return dsrc


def input_gradient(model, src, target=None, labels=None, loss=None, batch=256):
    enc, plan_of, K = _resolve(model)
    if loss is None:
        loss = "ce" if labels is not None else "logit"
    if loss not in ("logit", "ce"):
        raise ValueError(f"loss must be 'logit' or 'ce', got {loss!r}")
    if loss == "ce" and labels is None:
        raise ValueError("loss='ce' needs labels=")
    if loss == "ce" and target is not None:
        raise ValueError("target= selects a logit; with labels= / loss='ce' the gradient is that of the cross entropy")
    if loss == "logit" and labels is not None:
        raise ValueError("labels= gives the cross-entropy gradient: do not combine it with loss='logit'")
    batch = _batch(batch)
    n = src.shape[0] if isinstance(src, torch.Tensor) and src.dim() > 0 else 0
    tgt = None if target is None else _classes(target, n, K, "target")
    lab = None if labels is None else _classes(labels, n, K, "labels")
    src = enc._expect(src)
    plan = plan_of()
    out = torch.empty_like(src)
    with torch.no_grad():
        if tgt is not None:
            tgt = tgt.to(src.device)
        if lab is not None:
            lab = lab.to(src.device)
        for i in range(0, n, batch):
            xb = src[i:i + batch]
            logits = _forward(plan, xb)
            if loss == "ce":
                dl = _ce_grad(plan, logits, lab[i:i + batch].contiguous())
            else:
                t = logits.argmax(1) if tgt is None else tgt[i:i + batch]
                dl = torch.nn.functional.one_hot(t, K).float()
            out[i:i + xb.shape[0]] = _input_grad(plan, xb, dl)
    return out


def integrated_gradients(model, src, target=None, baseline=None, steps=32, batch=256):
    enc, plan_of, K = _resolve(model)
    steps = operator.index(steps)
    if steps <= 0:
        raise ValueError(f"steps must be positive, got {steps}")
    batch = _batch(batch)
    n = src.shape[0] if isinstance(src, torch.Tensor) and src.dim() > 0 else 0
    tgt = None if target is None else _classes(target, n, K, "target")
    if baseline is not None:
        if not isinstance(baseline, torch.Tensor):
            raise TypeError(f"baseline must be a tensor, got {type(baseline).__name__}")
        if isinstance(src, torch.Tensor) and tuple(baseline.shape) not in (tuple(src.shape), tuple(src.shape[1:])):
            raise ValueError(f"baseline must have the shape of src {tuple(src.shape)} or of one frame {tuple(src.shape[1:])}, "
                             f"got {tuple(baseline.shape)}")
    src = enc._expect(src)
    plan = plan_of()
    base = torch.zeros_like(src) if baseline is None else baseline.to(src.device, torch.float32).expand_as(src).contiguous()
    out = torch.empty_like(src)
    alphas = (torch.arange(steps, dtype=torch.float32, device=src.device) + 0.5) / steps
    group = max(1, batch // steps)                      # frames per group: all their interpolation points in one buffer
    with torch.no_grad():
        if tgt is None:
            tgt = torch.empty(n, dtype=torch.int64, device=src.device)
            for i in range(0, n, batch):
                tgt[i:i + batch] = _forward(plan, src[i:i + batch]).argmax(1)
        else:
            tgt = tgt.to(src.device)
        for i in range(0, n, group):
            xs, bs = src[i:i + group], base[i:i + group]
            g = xs.shape[0]
            delta = xs - bs
            pts = (bs[:, None] + alphas.view((1, -1) + (1,) * (src.dim() - 1)) * delta[:, None]).reshape((g * steps,) + src.shape[1:])
            t = tgt[i:i + g].repeat_interleave(steps)
            grads = torch.empty_like(pts)
            for j in range(0, g * steps, batch):
                pb = pts[j:j + batch]
                _forward(plan, pb)
                grads[j:j + pb.shape[0]] = _input_grad(plan, pb, torch.nn.functional.one_hot(t[j:j + batch], K).float())
            out[i:i + g] = delta * grads.view((g, steps) + src.shape[1:]).sum(1) / steps
    return out
