"""What every image front end shares: planar (B, 2, length) I/Q frames on the device -> the (B, channels, height, width) image a
ViT reads, by one HIP launch per direction.

spectrogram.Spectrogram, cyclic.CyclicSpectrum and constellation.Constellation derive from `FrontEnd`.  A front end writes what
is its own: its arguments and tables, `struct()` (the parameter struct of a call), `_forward` / `_backward` (each exactly one C
call, with its tables) and its host fp64 definition.  Everything else is here, once, and no method here knows which subclass
calls it: the refusals of `_check`, the call through one autograd function, the launch routine, `fit` and the checks of the
scaling arguments.  The per-device table cache and the CPU refusal are stage.py's: the symbol-rate stages share them.
`front_end` is the `spectrogram=` argument of the input paths (data.py, synth.py, impairments.py), which read a front end
through `length`, `height` and `width` only.
"""
from __future__ import annotations

import numpy as np
import torch

from ._args import MAX_LENGTH, _index, _number
from .stage import DeviceTables, _host, no_cpu  # noqa: F401  (_host: the front ends' host definitions import it from here)


def _mode(mode, modes):
    if mode not in modes:
        raise ValueError(f"mode must be one of {modes}, got {mode!r}")
    return mode


def _image_geometry(model):
    """The `_geom` of a ViT (an AMCTransformerViT or its encoder), whose image a front end's for_model() is built for."""
    geom = getattr(getattr(model, "encoder", model), "_geom", None)
    if not isinstance(geom, dict) or geom.get("kind") != 0:
        raise TypeError(f"expected a ViT model (image input), got {type(model).__name__}")
    return geom


class FrontEnd(DeviceTables):
    """The protocol.  A subclass sets `height` and `width` (and `channels`, unless 1), names its host definition in `reference`,
    keeps its tables as numpy attributes (stage.DeviceTables' `table_on` uploads them by name) and supplies
      struct()                                 the parameter struct of a call, from the object as it is now
      _forward(x, out, B, par, stream)         the one C call x -> out            (B > 0, x contiguous fp32)
      _backward(x, dout, dx, B, par, stream)   the one C call (x, dout) -> dx     (B > 0, par the struct of the forward call)"""

    channels = 1
    differentiable = True        # False: an input that requires grad is refused
    reference = None             # the name of the host fp64 definition, for the CPU refusal

    def __init__(self, length):
        self.length = _index(length, "length", 1, MAX_LENGTH)
        self._uploaded = {}      # (table name, device) -> tensor

    def image_shape(self, B):
        return (B, self.channels, self.height, self.width)

    def _set_scaling(self, floor, scale, shift):
        self.floor = _number(floor, "floor")                 # of a log or a division: positive after rounding to fp32
        if self.floor <= 0 or float(np.float32(self.floor)) <= 0:
            raise ValueError(f"floor must be positive (in fp32), got {floor!r}")
        self.scale, self.shift = _number(scale, "scale"), _number(shift, "shift")

    def _check(self, x, what="x"):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != 2 or x.shape[2] != self.length:
            raise ValueError(f"{what} must be a (B, 2, {self.length}) tensor, got "
                             f"{tuple(x.shape) if hasattr(x, 'shape') else x!r}")
        if not x.is_cuda:
            raise no_cpu(self)
        if not self.differentiable and x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"this {type(self).__name__} is not differentiable: build it with differentiable=True for "
                               "gradients down to the signal, or pass x.detach()")

    def __call__(self, x):
        """x: device (B, 2, length) fp32 -> image_shape(B) fp32 on the current stream, no host synchronisation; differentiable
        with respect to x."""
        self._check(x)
        return _FrontEndFn.apply(x, self)

    def _launch(self, x):
        """-> (x contiguous fp32, the image, the struct of this call).  image_shape(B) is written out: a call costs 11 us of
        host time, and a method call shows in it (profiles/frontend_refactor.txt)."""
        x = x.contiguous().float()
        B = x.shape[0]
        out = torch.empty((B, self.channels, self.height, self.width), dtype=torch.float32, device=x.device)
        par = self.struct()
        if B > 0:
            self._forward(x, out, B, par, torch.cuda.current_stream(x.device).cuda_stream)
        return x, out, par

    def fit(self, x_subset):
        """Set scale and shift so that the images of `x_subset` (device (B, 2, length)) have zero mean and unit standard
        deviation (unbiased, floored at 1e-8): one call with scale 1 and shift 0, then a device mean / std.  One host
        synchronisation.  -> self."""
        self._check(x_subset, "x_subset")
        if x_subset.shape[0] < 1:
            raise ValueError("x_subset is empty")
        self.scale, self.shift = 1.0, 0.0
        with torch.no_grad():
            std, mean = torch.std_mean(self(x_subset))
        mean, std = float(mean), max(float(std), 1e-8)
        self.scale, self.shift = _number(1.0 / std, "scale"), _number(-mean / std, "shift")
        return self


class _FrontEndFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, front):
        x, out, ctx.par = front._launch(x)       # the scaling of THIS call: fit() may change the object before backward
        ctx.save_for_backward(x)
        ctx.front = front
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        dout = dout.contiguous().float()
        dx = torch.empty_like(x)
        B = x.shape[0]
        if B > 0:
            ctx.front._backward(x, dout, dx, B, ctx.par, torch.cuda.current_stream(x.device).cuda_stream)
        return dx, None


def front_end(front, layout, length):
    """The `spectrogram=` argument of an input path: None, or a FrontEnd for frames of `length` samples, which needs layout 'vit'
    (the launch in front of it then runs with take = len and the image is the front end's image_shape(B))."""
    if front is None:
        return None
    if not isinstance(front, FrontEnd):
        raise TypeError(f"spectrogram must be a Spectrogram or None, got {type(front).__name__}")
    if layout != "vit":
        raise ValueError(f"a spectrogram is an image: layout must be 'vit', got {layout!r}")
    if front.length != length:
        raise ValueError(f"the spectrogram was built for frames of {front.length} samples, these have {length}")
    return front
