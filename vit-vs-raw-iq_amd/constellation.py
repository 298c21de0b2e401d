"""Constellation front end on the device: planar (B, 2, len) I/Q points -> the (B, 1, height, width) density image a ViT reads.

The constellation diagram as an image: a smoothed 2-D density of the received (I, Q) points.  It is order-free -- it discards
time and keeps the alphabet -- which makes it the complement of the spectrogram (frequency over time) and of the cyclic spectrum
(rates and conjugate lines).  One HIP kernel (csrc/constellation.hip, iq_frames_constellation) computes it on the fp32-input MFMA:
with a separable profile the image of a frame is a Gram matrix over its points, D = A^T B, and a 32 x 32 tile is reached only by
the points within `radius` pixels of it, so the kernel compacts those per tile and runs the chain over them only.
iq_frames_constellation_bwd is its adjoint (a deterministic gather, no atomics), so `con(x)` is differentiable and gradients
reach the points (x.grad, saliency, FGSM / PGD).  There is no CPU path; `constellation_reference` /
`constellation_reference_bwd` are the host fp64 DEFINITION the tests compare against.

With a radial profile p (a table sampled every 1 / n_frac pixel, linear in between, 0 from `radius` pixels on):
  u = I * x_scale + x_off,  v = Q * y_scale + y_off          pixel units; pixel c covers [c, c+1), its centre is c + 0.5
  b[n, c] = p(|u[n] - (c + 0.5)|),   a[n, r] = p(|v[n] - (r + 0.5)|)
  D[r, c] = sum_n a[n, r] b[n, c],   V = D * inv_norm
  image[r, c] = V * scale + shift  (mode 'power')   or   log10(V + floor) * scale + shift  (mode 'log')
  row 0 holds the most negative Q; x_scale = width / (2 extent), x_off = width / 2 (likewise y from height): the image spans
  [-extent, extent) on both axes.  NaN / infinite points and points out of every pixel's reach contribute nothing.
The table is computed in fp64 and rounded to fp32 once; the kernel treats it as plain numbers.  On a non-square grid `sigma`
is in pixels per axis (the blob is round in pixels, not in signal units).

  Constellation(height, width, length, extent, profile, sigma, radius, n_frac, table, mode, floor, scale, shift)
  con(x) -> image;  .fit(x_subset);  .struct();  .table_on(device)
  Constellation.for_model(model, length, **kw)                         height, width from the ViT's image geometry
  constellation_reference(x, con), constellation_reference_bwd(x, dout, con)      host fp64

Symbols: with ReceivedSynth(shaped, receiver) as the synth of a SynthStream the stream's frames ARE the symbols, so
SynthStream(received, stats, "vit", B, spectrogram=Constellation.for_model(model, received.length)) is the whole chain
transmitter -> channel -> receiver -> constellation -> ViT on the device.  Stand-alone, the (B, n_sym, 2) symbols of a Receiver
go in as con(sym.transpose(1, 2)).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _native as N
from ._args import _index, _number
from .frontend import FrontEnd, _host, _image_geometry, _mode

PROFILES = ("gaussian", "triangle")
MODES = ("power", "log")
MIN_SIZE, MAX_SIZE, SIZE_STEP = 32, 256, 32
MAX_RADIUS, MAX_FRAC = 16, 64


def _size(v, name):
    v = _index(v, name, MIN_SIZE, MAX_SIZE)
    if v % SIZE_STEP:
        raise ValueError(f"{name} must be a multiple of {SIZE_STEP}, got {v!r}")
    return v


def profile_table(profile, radius, n_frac, sigma=1.0):
    """The radial profile in fp64 at distances k / n_frac pixels, k = 0 .. radius * n_frac; the last tap is 0.
    'gaussian': exp(-d^2 / (2 sigma^2)); 'triangle': 1 - d / radius (radius 1: bilinear binning, a partition of unity)."""
    d = np.arange(radius * n_frac + 1, dtype=np.float64) / n_frac
    t = np.exp(-0.5 * (d / sigma) ** 2) if profile == "gaussian" else 1.0 - d / radius
    t[-1] = 0.0
    return t


class Constellation(FrontEnd):
    """The geometry, profile and scaling of one front end.  Defaults: 'gaussian' with sigma in pixels and radius =
    ceil(4 sigma), capped at 16; 'triangle' has radius 1; a caller's `table` (radius * n_frac + 1 numbers, radius given or taken
    from its length) replaces both.  inv_norm = 1 / (length * s^2) with s the sum of the profile at the integer pixel distances
    -(radius-1) .. radius-1: the image of one interior point then sums to about 1 / length and that of a frame to about 1.
    floor (log mode) defaults to inv_norm / 10: a tenth of what ONE point leaves in the pixel it sits on (D = 0.1), so a single
    point stands a decade above the empty background.  Arguments are checked here, before any device work; the table goes to a
    device at the first call for that device and stays there."""

    reference = "constellation_reference"

    def __init__(self, height, width, length, extent=3.0, profile="gaussian", sigma=1.0, radius=None, n_frac=8, table=None,
                 mode="log", floor=None, scale=1.0, shift=0.0, inv_norm=None):
        self.height, self.width = _size(height, "height"), _size(width, "width")
        super().__init__(length)
        self.extent = _number(extent, "extent")
        if self.extent <= 0:
            raise ValueError(f"extent must be positive, got {extent!r}")
        self.n_frac = _index(n_frac, "n_frac", 1, MAX_FRAC)
        self.mode = _mode(mode, MODES)
        if table is not None:
            t = np.asarray(table, dtype=np.float64).reshape(-1)
            if radius is None:
                radius = (t.size - 1) // self.n_frac
            self.radius = _index(radius, "radius", 1, MAX_RADIUS)
            if t.size != self.radius * self.n_frac + 1:
                raise ValueError(f"table must hold radius * n_frac + 1 = {self.radius * self.n_frac + 1} numbers, got {t.size}")
            self.profile, self.sigma = "table", None
        else:
            if profile not in PROFILES:
                raise ValueError(f"profile must be one of {PROFILES}, got {profile!r}")
            self.profile = profile
            if profile == "gaussian":
                self.sigma = _number(sigma, "sigma")
                if self.sigma <= 0:
                    raise ValueError(f"sigma must be positive, got {sigma!r}")
                if radius is None:
                    radius = min(MAX_RADIUS, max(1, math.ceil(4.0 * self.sigma)))
            else:
                self.sigma = None
                if radius is None:
                    radius = 1
            self.radius = _index(radius, "radius", 1, MAX_RADIUS)
            t = profile_table(profile, self.radius, self.n_frac, self.sigma)
        self.table = t.astype(np.float32)                            # the kernel's table: rounded once
        if not np.all(np.isfinite(self.table)):
            raise ValueError("the table must be finite (in fp32)")
        self.x_scale, self.x_off = self.width / (2.0 * self.extent), self.width / 2.0
        self.y_scale, self.y_off = self.height / (2.0 * self.extent), self.height / 2.0
        if inv_norm is None:
            taps = self.table.astype(np.float64)[::self.n_frac]      # distances 0, 1, .. radius (the last is the zero tap)
            s = float(taps[0] + 2.0 * taps[1:].sum())
            if not s > 0:
                raise ValueError(f"the profile sums to {s} over the integer pixel distances: pass inv_norm")
            inv_norm = 1.0 / (self.length * s * s)
        self.inv_norm = _number(inv_norm, "inv_norm")
        self._set_scaling(self.inv_norm / 10.0 if floor is None else floor, scale, shift)

    @property
    def n_fft(self):
        """The image height, under the name the other two front ends have for it; nothing in the package reads it."""
        return self.height

    @classmethod
    def for_model(cls, model, length, **kw):
        """A front end whose image is the input of `model` (an AMCTransformerViT or its encoder): height = img_size_h, width =
        img_size_w, both multiples of 32."""
        geom = _image_geometry(model)
        if geom["in_channels"] != 1:
            raise ValueError(f"a constellation image has one channel, the model expects {geom['in_channels']}")
        return cls(geom["img_h"], geom["img_w"], length, **kw)

    def struct(self) -> N.Constellation:
        """The iq_constellation_t of a call."""
        return N.Constellation(height=self.height, width=self.width, radius=self.radius, n_frac=self.n_frac,
                               mode=MODES.index(self.mode), x_scale=self.x_scale, x_off=self.x_off, y_scale=self.y_scale,
                               y_off=self.y_off, inv_norm=self.inv_norm, floor=self.floor, scale=self.scale, shift=self.shift)

    def _forward(self, x, out, B, par, stream):
        N.check(N.lib().iq_frames_constellation(x.data_ptr(), self.table_on(x.device).data_ptr(), out.data_ptr(), B,
                                                self.length, C.byref(par), stream), "iq_frames_constellation")

    def _backward(self, x, dout, dx, B, par, stream):
        N.check(N.lib().iq_frames_constellation_bwd(x.data_ptr(), self.table_on(x.device).data_ptr(), dout.data_ptr(),
                                                    dx.data_ptr(), B, self.length, C.byref(par), stream),
                "iq_frames_constellation_bwd")

    def __repr__(self):
        shape = f"sigma={self.sigma}, " if self.profile == "gaussian" else ""
        return (f"Constellation(height={self.height}, width={self.width}, length={self.length}, extent={self.extent}, "
                f"profile={self.profile!r}, {shape}radius={self.radius}, n_frac={self.n_frac}, mode={self.mode!r}, "
                f"floor={self.floor}, scale={self.scale}, shift={self.shift})")


# ---------------------------------------------------------------------------------------------------------------------------
# the host fp64 definition
# ---------------------------------------------------------------------------------------------------------------------------
def _f32(v):
    return float(np.float32(v))


def _axis_weights(s, scale, off, n_pix, con):
    """s (B, len) fp64 samples of one axis -> (w, d), both (B, len, n_pix): the weight of every pixel and sgn(e) * the slope of
    the table segment it was taken from.  Knots: t = |e| * n_frac falls into segment i = floor(t), so a t exactly on a knot
    takes the segment to its right; t >= radius * n_frac (and a NaN) is out of reach: w = d = 0; sgn(0) = 0."""
    tab = con.table.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = (s * _f32(scale) + _f32(off))[..., None] - (np.arange(n_pix, dtype=np.float64) + 0.5)
        t = np.abs(e) * con.n_frac
        ok = t < con.radius * con.n_frac
    t = np.where(ok, t, 0.0)
    i = np.floor(t).astype(np.int64)
    slope = tab[i + 1] - tab[i]
    w = np.where(ok, (t - i) * slope + tab[i], 0.0)
    d = np.where(ok, np.sign(np.where(ok, e, 0.0)) * slope, 0.0)
    return w, d


def _density(x, con):
    if not isinstance(con, Constellation):
        raise TypeError(f"con must be a Constellation, got {type(con).__name__}")
    x = _host(x).astype(np.float64)
    if x.ndim != 3 or x.shape[1] != 2 or x.shape[2] != con.length:
        raise ValueError(f"x must be (B, 2, {con.length}), got {x.shape}")
    b, db = _axis_weights(x[:, 0], con.x_scale, con.x_off, con.width, con)       # (B, len, width)
    a, da = _axis_weights(x[:, 1], con.y_scale, con.y_off, con.height, con)      # (B, len, height)
    V = (a.transpose(0, 2, 1) @ b) * _f32(con.inv_norm)                          # (B, height, width)
    return V, a, da, b, db


def constellation_reference(x, con):
    """The definition in fp64 on the host, from the fp32-rounded table and parameters.  x: (B, 2, len) -> float64
    (B, 1, height, width)."""
    V = _density(x, con)[0]
    v = np.log10(V + _f32(con.floor)) if con.mode == "log" else V
    return (v * _f32(con.scale) + _f32(con.shift))[:, None]


def constellation_reference_bwd(x, dout, con):
    """The analytic adjoint in fp64: the gradient of sum(constellation_reference(x) * dout) with respect to x (of the piecewise
    linear profile: at a knot the slope of the segment to its right).  dout: (B, 1, height, width) -> float64 (B, 2, len)."""
    V, a, da, b, db = _density(x, con)
    d = _host(dout).astype(np.float64)
    B = V.shape[0]
    if d.shape != (B, 1, con.height, con.width):
        raise ValueError(f"dout must be {(B, 1, con.height, con.width)}, got {d.shape}")
    g = d[:, 0] * _f32(con.scale) * _f32(con.inv_norm)
    if con.mode == "log":
        g = g / (math.log(10.0) * (V + _f32(con.floor)))
    di = _f32(con.x_scale) * con.n_frac * ((a @ g) * db).sum(axis=2)              # (B, len)
    dq = _f32(con.y_scale) * con.n_frac * ((b @ g.transpose(0, 2, 1)) * da).sum(axis=2)
    return np.stack([di, dq], axis=1)
