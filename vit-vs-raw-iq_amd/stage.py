"""What the symbol-rate stages share: receiver.Receiver, carrier.Carrier, equaliser.Equaliser, likelihood.LikelihoodClassifier
and cumulants.CumulantClassifier, each one HIP launch per direction on a batch of I/Q frames.

Carrier, Equaliser, LikelihoodClassifier and CumulantClassifier derive from `Stage`: frames of a fixed `length` in one of two layouts, whose names
each class keeps in `LAYOUTS`.  A stage writes what is its own: its arguments and tables, `struct()`, its `__call__` (the side
arguments it takes and the extras it returns), `_forward` / `_backward` (each exactly one C call) and its host fp64 definition.
Here, once: the per-device table cache (`DeviceTables`, which frontend.FrontEnd uses too), the frame check and the CPU refusal,
the coercion of per-frame side arguments (`integers`, `reals`), `pack`, the autograd function of a stage whose estimate the
backward holds fixed (`_HeldFn`: Carrier, Equaliser), `stage_for` (the check of a stage composed behind another object) and the
pieces of the host definitions (`_host`, `_frames`, `_unframes`, `_first_largest`).

Receiver takes frames of any length and has no layout, so it is not a Stage: it uses the cache, the refusal and the helpers.
Its autograd function stays in receiver.py: its output is shorter than its input, it saves the symbols beside the estimate,
and its backward derives the instant from that estimate -- each would be a flag in `_HeldFn`.

Nothing of the package is imported here but _native and _args.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from ._args import MAX_LENGTH, _index


class DeviceTables:
    """The numpy tables an object keeps as attributes, as fp32 tensors per device.  The object sets `self._uploaded = {}`."""

    def table_on(self, device, name="table"):
        """The table `self.<name>` on `device`, uploaded once per device; `name` a tuple of names: the tuple of those tables."""
        t = self._uploaded.get((name, device))               # a call's x.device: found as it is
        if t is None:
            device = torch.device(device)
            if device.type == "cuda" and device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            t = self._uploaded.get((name, device))
            if t is None:
                up = [torch.from_numpy(getattr(self, n)).to(device) for n in ((name,) if isinstance(name, str) else name)]
                t = self._uploaded[name, device] = up[0] if isinstance(name, str) else tuple(up)
        return t


def no_cpu(obj, what="x"):
    """The refusal of a CPU tensor, in the words of every front end and stage: to be raised."""
    return N.IqError(f"{type(obj).__name__} runs on the MI355X only: {what} is a CPU tensor and there is no CPU fallback "
                     f"({obj.reference} is the host definition used by the tests)")


class Stage(DeviceTables):
    """The protocol.  A subclass names its two layouts in `LAYOUTS` (index 0: (B, length, 2), index 1, `planar`: (B, 2, length))
    and its host definition in `reference`."""

    LAYOUTS = None
    reference = None             # the name of the host fp64 definition, for the CPU refusal

    def __init__(self, length, layout):
        self.length = _index(length, "length", 1, MAX_LENGTH)
        if layout not in self.LAYOUTS:
            raise ValueError(f"layout must be one of {self.LAYOUTS}, got {layout!r}")
        self.layout, self.planar = layout, self.LAYOUTS.index(layout)
        self._uploaded = {}      # (table name, device) -> tensor

    def frame_shape(self, B):
        return (B, 2, self.length) if self.planar else (B, self.length, 2)

    def _check_shape(self, x, what="x"):
        """x.shape is read once and no shape is built where x passes: a call costs 12 - 14 us of host time, and the first form
        (frame_shape("B") against tuple(x.shape[1:])) showed in it (profiles/stage_refactor.txt)."""
        s, p = x.shape if isinstance(x, torch.Tensor) else (), self.planar          # the (I, Q) axis is 2 - p, the samples' 1 + p
        if len(s) != 3 or s[2 - p] != 2 or s[1 + p] != self.length:
            raise ValueError(f"{what} must be a {self.frame_shape('B')} tensor (layout {self.layout!r}), got "
                             f"{tuple(x.shape) if hasattr(x, 'shape') else x!r}")

    def _check(self, x, what="x"):
        """The shape, then the device.  A stage with side arguments checks them in between: they are refused on CPU frames too."""
        self._check_shape(x, what)
        if not x.is_cuda:
            raise no_cpu(self)


def _sized(t, what, shape, note, device):
    if tuple(t.shape) != shape:
        raise ValueError(f"{what} must {note[0]}have shape {shape}{note[1]}, got {tuple(t.shape)}")
    return t if device is None else t.to(device=device).contiguous()


def integers(v, what, shape, device=None, note="", wrap=None):
    """A per-frame side argument of integers -> int32 of `shape`, still wherever it was or, with device=, contiguous on it.  A
    tensor is not looked at (that would synchronise); an array goes through `wrap` (its range check; -> numpy int32)."""
    if isinstance(v, torch.Tensor):
        if v.dtype.is_floating_point or v.dtype == torch.bool:
            raise TypeError(f"{what} must hold integers, got dtype {v.dtype}")
        t = v.to(torch.int32)
    else:
        try:
            arr = np.asarray(v)
            if arr.dtype.kind not in "iu":
                raise TypeError
        except (TypeError, ValueError):
            raise TypeError(f"{what} must be a tensor or an array of integers, got {v!r}") from None
        t = torch.from_numpy(arr.astype(np.int32) if wrap is None else wrap(arr))
    return _sized(t, what, shape, ("", note), device)


def reals(v, what, shape, device=None, note="", pairs=False):
    """A per-frame side argument of reals -> fp32 of `shape`, still wherever it was or, with device=, contiguous on it.  pairs:
    `shape` ends in a (re, im) axis, complex values are taken as those pairs and integers refused; otherwise a single number
    stands for every frame."""
    if isinstance(v, torch.Tensor):
        if pairs and v.dtype.is_complex:
            v = torch.view_as_real(v)
        elif pairs and not v.dtype.is_floating_point:
            raise TypeError(f"{what} must hold real or complex numbers, got dtype {v.dtype}")
        elif v.dtype.is_complex or v.dtype == torch.bool:
            raise TypeError(f"{what} must hold real numbers, got dtype {v.dtype}")
        t = v.to(torch.float32)
    else:
        try:
            arr = np.asarray(v)
            if pairs and arr.dtype.kind == "c":
                arr = np.stack([arr.real, arr.imag], axis=-1)
            if arr.dtype.kind not in "fiu":
                raise TypeError
        except (TypeError, ValueError):
            kinds = "a tensor or an array of numbers" if pairs else "a number, an array or a tensor of real numbers"
            raise TypeError(f"{what} must be {kinds}, got {v!r}") from None
        t = torch.from_numpy(np.array(arr, dtype=np.float32, ndmin=int(pairs)))
    if not pairs and t.dim() == 0:
        t = t.expand(shape)
    return _sized(t, what, shape, ("" if pairs else "be a number or ", note), device)


def pack(out, *extras):
    """(out, the extras that are not None) -> a bare tensor where there is none."""
    extras = [t for t in extras if t is not None]
    return (out, *extras) if extras else out


class _HeldFn(torch.autograd.Function):
    """out = stage(x), differentiable with respect to x with the stage's estimate held fixed.  The stage supplies
      _forward(x, *args) -> out, held, extras   the one C call (x contiguous fp32); held: what the backward needs, a tensor
      _backward(dout, dx, held, B)              the one C call dout -> dx with mode 0 and `held`  (B > 0)
    -> (out, held, *extras); everything but out is marked non-differentiable."""

    @staticmethod
    def forward(ctx, x, stage, *args):
        out, held, extras = stage._forward(x.contiguous().float(), *args)
        ctx.stage = stage
        ctx.save_for_backward(held)
        nd = (held,)
        for t in extras:                         # (a loop, not a comprehension: its call showed in the 14 us of a call)
            if t is not None:
                nd += (t,)
        ctx.mark_non_differentiable(*nd)         # all in ONE call: a second call would replace the first's set
        return (out, held, *extras)

    @staticmethod
    def backward(ctx, dout, *_):
        (held,) = ctx.saved_tensors
        dout = dout.contiguous().float()
        dx = torch.empty_like(dout)
        B = dout.shape[0]
        if B > 0:
            ctx.stage._backward(dout, dx, held, B)
        return (dx,) + (None,) * (len(ctx.needs_input_grad) - 1)


def stage_for(stage, cls, what, planar, length, reads, gives, optional=True):
    """The stage composed behind another object: `stage` if it is None (where optional) or a `cls` of the layout `planar` says
    and of `length`.  The refusals are in the caller's words: `reads` opens the layout's, `gives` closes the length's."""
    if stage is None and optional:
        return None
    if not isinstance(stage, cls):
        raise TypeError(f"{what} must be {'an' if cls.__name__[0] in 'AEIOU' else 'a'} {cls.__name__}"
                        f"{' or None' if optional else ''}, got {type(stage).__name__}")
    if bool(stage.planar) != planar:
        raise ValueError(f"{reads}: the {what}'s layout is {stage.layout!r}")
    if stage.length != length:
        raise ValueError(f"the {what} was built for frames of {stage.length} {gives}")
    return stage


# ---- pieces of the host definitions

def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _frames(x, planar):
    """(B, 2, len) (planar) or (B, len, 2) -> complex128 (B, len)."""
    x = _host(x).astype(np.float64)
    if x.ndim != 3 or x.shape[1 if planar else 2] != 2:
        raise ValueError(f"frames must be {'(B, 2, len)' if planar else '(B, len, 2)'}, got {x.shape}")
    return (x[:, 0, :] + 1j * x[:, 1, :]) if planar else (x[:, :, 0] + 1j * x[:, :, 1])


def _unframes(z, planar):
    return np.stack([z.real, z.imag], axis=1 if planar else 2)


def _first_largest(v, axis):
    """Index of the first largest along `axis`; a NaN is never larger nor ever beaten (the kernels' walk)."""
    v = np.moveaxis(v, axis, 0)
    at, best = np.zeros(v.shape[1:], np.int64), v[0].copy()
    for i in range(1, len(v)):
        with np.errstate(invalid="ignore"):
            up = v[i] > best
        at[up], best[up] = i, v[i][up]
    return at, best
