"""Spectrogram front end on the device: planar (B, 2, len) I/Q frames -> the (B, 1, n_fft, width) time-frequency image a ViT reads.

The step between the channel (impairments.py) and the ViT.  One HIP kernel (csrc/spectrogram.hip, iq_frames_spectrogram)
computes the short-time Fourier transform of every frame as a sliding complex GEMM on the fp32-input MFMA against a table
built here, with the power / log epilogue fused; iq_frames_spectrogram_bwd is its adjoint (a deterministic gather, no atomics),
so `spec(x)` is differentiable and gradients reach the SIGNAL (x.grad, FGSM / PGD on the frame rather than on the image).
There is no CPU path; `spectrogram_reference` / `spectrogram_reference_bwd` are the host fp64 DEFINITION the tests compare
against.

With z[j] = I[j] + i Q[j], a window w and column t's first sample j0 = t*hop - pad (samples outside [0, len) count as zero):
  X[t, k] = sum_m z[j0 + m] w[m] exp(-2 pi i k m / n_fft)                 m = 0 .. n_fft-1
          = (sum_m I c + Q s) + i (sum_m Q c - I s),   c[m,k] = w[m] cos(2 pi k m / n_fft),  s[m,k] = w[m] sin(2 pi k m / n_fft)
  P = |X|^2 * inv_norm,  inv_norm = 1 / sum w^2
  image[r, t] = P * scale + shift  (mode 'power')   or   log10(P + floor) * scale + shift  (mode 'log')
  row r holds bin k = (r + n_fft/2) mod n_fft: numpy.fft.fftshift order, row 0 is the most negative frequency.
The table (c, s) is computed in fp64 and rounded to fp32 once; the kernel treats it as plain numbers.

  Spectrogram(n_fft, width, length, hop, pad, window, mode, floor, scale, shift)   spec(x) -> image;  .fit(x_subset);  .struct()
  Spectrogram.for_model(model, length, **kw)                                     n_fft, width from the ViT's image geometry
  spectrogram_reference(x, spec), spectrogram_reference_bwd(x, dout, spec)        host fp64
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _native as N
from ._args import _index
from .frontend import FrontEnd, _host, _image_geometry, _mode

WINDOWS = ("hann", "rect")
MODES = ("power", "log")
MIN_FFT, MAX_FFT, FFT_STEP = 32, 256, 32


def _window(name, n_fft):
    """The window in fp64: 'hann' is the periodic Hann window 0.5 - 0.5 cos(2 pi m / n_fft), 'rect' all ones."""
    if name == "hann":
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    return np.ones(n_fft)


def _twiddles(n_fft, w):
    """c[m,k], s[m,k] in fp64; the angle is reduced with integers (k*m mod n_fft) before the cos / sin."""
    m = np.arange(n_fft)
    ang = 2.0 * np.pi * ((m[:, None] * m[None, :]) % n_fft) / n_fft
    return w[:, None] * np.cos(ang), w[:, None] * np.sin(ang)


class Spectrogram(FrontEnd):
    """The geometry and scaling of one front end.  Defaults: hop = max(1, length // width), pad = max(0, ceil(((width-1)*hop +
    n_fft - length) / 2)) (the windows are centred on the frame), inv_norm = 1 / sum w^2.  Arguments are checked here, before
    any device work; the table goes to a device at the first call for that device and stays there."""

    reference = "spectrogram_reference"

    def __init__(self, n_fft, width, length=1024, hop=None, pad=None, window="hann", mode="log", floor=1e-3, scale=1.0,
                 shift=0.0):
        self.n_fft = self.height = _index(n_fft, "n_fft", MIN_FFT, MAX_FFT)
        if self.n_fft % FFT_STEP:
            raise ValueError(f"n_fft must be a multiple of {FFT_STEP}, got {n_fft!r}")
        self.width = _index(width, "width", 1, 2 ** 31 - 1)
        super().__init__(length)
        self.hop = max(1, self.length // self.width) if hop is None else _index(hop, "hop", 1, 2 ** 31 - 1)
        if pad is None:
            pad = max(0, -((self.length - (self.width - 1) * self.hop - self.n_fft) // 2))
        self.pad = _index(pad, "pad", 0, 2 ** 31 - 1)
        if window not in WINDOWS:
            raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
        self.window, self.mode = window, _mode(mode, MODES)
        self._set_scaling(floor, scale, shift)
        w = _window(window, self.n_fft)
        self.inv_norm = 1.0 / float(np.sum(w * w))
        c, s = _twiddles(self.n_fft, w)
        self.table = np.stack([c, s]).astype(np.float32)           # (2, n_fft, n_fft): the kernel's table

    @classmethod
    def for_model(cls, model, length=1024, **kw):
        """A front end whose image is the input of `model` (an AMCTransformerViT or its encoder): n_fft = img_size_h, width =
        img_size_w."""
        geom = _image_geometry(model)
        if geom["in_channels"] != 1:
            raise ValueError(f"a spectrogram has one channel, the model expects {geom['in_channels']}")
        return cls(geom["img_h"], geom["img_w"], length, **kw)

    def struct(self) -> N.Spectrogram:
        """The iq_spectrogram_t of a call."""
        return N.Spectrogram(n_fft=self.n_fft, hop=self.hop, pad=self.pad, width=self.width, mode=MODES.index(self.mode),
                             inv_norm=self.inv_norm, floor=self.floor, scale=self.scale, shift=self.shift)

    def _forward(self, x, out, B, par, stream):
        N.check(N.lib().iq_frames_spectrogram(x.data_ptr(), self.table_on(x.device).data_ptr(), out.data_ptr(), B,
                                              self.length, C.byref(par), stream), "iq_frames_spectrogram")

    def _backward(self, x, dout, dx, B, par, stream):
        N.check(N.lib().iq_frames_spectrogram_bwd(x.data_ptr(), self.table_on(x.device).data_ptr(), dout.data_ptr(),
                                                  dx.data_ptr(), B, self.length, C.byref(par), stream),
                "iq_frames_spectrogram_bwd")

    def __repr__(self):
        return (f"Spectrogram(n_fft={self.n_fft}, width={self.width}, length={self.length}, hop={self.hop}, pad={self.pad}, "
                f"window={self.window!r}, mode={self.mode!r}, floor={self.floor}, scale={self.scale}, shift={self.shift})")


def _columns(spec, length):
    """(width, n_fft) sample index of every window element and the mask of those inside the frame."""
    j = np.arange(spec.width)[:, None] * spec.hop - spec.pad + np.arange(spec.n_fft)[None, :]
    return j, (j >= 0) & (j < length)


def _transform(x, spec):
    if not isinstance(spec, Spectrogram):
        raise TypeError(f"spec must be a Spectrogram, got {type(spec).__name__}")
    x = _host(x).astype(np.float64)
    if x.ndim != 3 or x.shape[1] != 2 or x.shape[2] != spec.length:
        raise ValueError(f"x must be (B, 2, {spec.length}), got {x.shape}")
    c, s = _twiddles(spec.n_fft, _window(spec.window, spec.n_fft))
    E = c - 1j * s                                                     # w[m] exp(-2 pi i k m / n_fft)
    j, inside = _columns(spec, spec.length)
    z = x[:, 0, :] + 1j * x[:, 1, :]
    cols = np.where(inside[None], z[:, np.clip(j, 0, spec.length - 1)], 0.0)      # (B, width, n_fft)
    return cols @ E, E, j, inside                                      # X (B, width, n_fft bins)


def spectrogram_reference(x, spec):
    """The definition in fp64 on the host, from the formula (a matrix product with w[m] exp(-2 pi i k m / n_fft), no FFT).
    x: (B, 2, len) -> float64 (B, 1, n_fft, width)."""
    X, _, _, _ = _transform(x, spec)
    P = (X.real ** 2 + X.imag ** 2) * spec.inv_norm
    v = np.log10(P + spec.floor) if spec.mode == "log" else P
    img = v * spec.scale + spec.shift                                  # (B, width, bins)
    rows = (np.arange(spec.n_fft) + spec.n_fft // 2) % spec.n_fft
    return np.ascontiguousarray(img[:, :, rows].transpose(0, 2, 1))[:, None]


def spectrogram_reference_bwd(x, dout, spec):
    """The analytic adjoint in fp64: the gradient of sum(spectrogram_reference(x) * dout) with respect to x.
    dout: (B, 1, n_fft, width) -> float64 (B, 2, len)."""
    X, E, j, inside = _transform(x, spec)
    d = _host(dout).astype(np.float64)
    B = X.shape[0]
    if d.shape != (B, 1, spec.n_fft, spec.width):
        raise ValueError(f"dout must be {(B, 1, spec.n_fft, spec.width)}, got {d.shape}")
    bins = np.empty(spec.n_fft, np.int64)
    bins[(np.arange(spec.n_fft) + spec.n_fft // 2) % spec.n_fft] = np.arange(spec.n_fft)      # bin k lies in row bins[k]
    dv = d[:, 0].transpose(0, 2, 1)[:, :, bins] * spec.scale           # (B, width, bins)
    if spec.mode == "log":
        P = (X.real ** 2 + X.imag ** 2) * spec.inv_norm
        dv = dv / (math.log(10.0) * (P + spec.floor))
    dX = 2.0 * X * (dv * spec.inv_norm)                                # dRe + i dIm
    dz = dX @ np.conj(E).T                                             # (B, width, n_fft samples of the window)
    out = np.zeros((B, 2, spec.length))
    for t in range(spec.width):
        ok = inside[t]
        out[:, 0, j[t, ok]] += dz[:, t, ok].real                       # the indices of one column are distinct
        out[:, 1, j[t, ok]] += dz[:, t, ok].imag
    return out
