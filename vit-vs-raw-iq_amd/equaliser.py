"""Blind equaliser on the device: an L-tap complex filter per frame, found by block constant-modulus descent, and the filter.

waveform.ShapedSynth(taps=L) puts a static Rician / Rayleigh channel of up to 8 taps behind the pulse shaping, and the receiver
recovers timing only: what the channel spreads over neighbouring symbols stays in its output.  At sps = 8 that is a blur of the
constellation; at sps = 2 an 8-tap channel spans 3.5 symbols and the points of a QPSK frame fill the plane.  One HIP kernel
(csrc/equaliser.hip, iq_frames_equalise) undoes it blindly, on the symbols of the frame itself: starting from a unit spike, `iters`
steps of gradient descent on the constant-modulus cost J(w) = mean_n (|y[n]|^2 - R)^2, y = w * z, every step over the whole frame
(block CMA), all inside one launch; then out = y.  The definition is written out in include/iqvit.h.  iq_frames_equalise_bwd is
the adjoint with the weights held fixed: the stage is differentiable with respect to its input.  There is no CPU path;
`equaliser_reference` / `equaliser_reference_bwd` are the host fp64 DEFINITIONS the tests compare against.

The limit of the method: J rewards a constant modulus.  PSK has one and gains most ("Blind equaliser": nearest-point
error 0.45 -> 0.11 for QPSK at sps = 2 behind 4 taps).  16QAM has three moduli and only a statistical pull towards R: at 512 or
more symbols it gains modestly (0.30 -> 0.24), and a frame of 128 symbols is too short -- the descent fits the frame's own
symbol pattern and the error doubles (0.096 -> 0.19).  Use it on short frames of non-constant-modulus classes with few steps or
not at all.  What remains after it: one complex gain (CMA is blind to a rotation: the carrier stage behind it takes that out) and a
delay of whole symbols (est[:, 3], the index of the largest weight, shows it).

  Equaliser(length, taps, iters, mu, modulus, layout)              equaliser(x, w=, w0=) -> out [, w, est]
  equaliser_reference(x, taps, iters, mu, ...) -> out, w, est      equaliser_reference_bwd(dout, w, planar) -> dx
  cma_step_reference(z, w, modulus) -> y, g, J                    one step's pieces, for the tests and the sweep

Not here: fractionally spaced equalisation on the raw frame (this one runs at one sample per symbol, behind the receiver),
decision-directed, RLS or multi-modulus variants, choosing `modulus` per frame or per class, and differentiating through the
iterations.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N
from ._args import _flag, _index, _number
from .stage import Stage, _first_largest, _frames, _HeldFn, _host, _unframes, no_cpu, pack, reals

LAYOUTS = ("frames", "planar")               # iq_equaliser_t.planar = 0: (B, length, 2), 1: (B, 2, length)
MAX_TAPS, MAX_ITERS = 32, 4096               # the limits of iq_frames_equalise
# The defaults: chosen on the host definition over mu in {0.005 .. 1.0} x iters in {16 .. 256} on the closed-loop frames of
# tests/equaliser_ref.py ("Blind equaliser", has the sweep)
DEFAULT_TAPS, DEFAULT_ITERS, DEFAULT_MU = 11, 64, 0.2


def _step(mu):
    mu = _number(mu, "mu")
    if mu < 0:
        raise ValueError(f"mu must be >= 0, got {mu!r}")
    return mu


class Equaliser(Stage):
    """Frames of `length` symbols -> the same frames through a blind `taps`-tap equaliser.  iters: the steps of the descent;
    mu: its step size (the gradient is the frame's mean, so mu does not depend on the length); modulus: R = E|a|^4 / E|a|^2 of
    the constellation at unit power (1 for PSK, 1.32 for 16QAM).  The input is expected at unit mean power (Receiver's
    normalise=True).  layout: 'frames' (B, length, 2), what the generators and the receiver write, or 'planar' (B, 2, length),
    what the carrier recovery in front of an image front end reads.  A call runs on the device its x lies on.  Arguments are
    checked here, before any device work."""

    LAYOUTS, reference = LAYOUTS, "equaliser_reference"

    def __init__(self, length, taps: int = DEFAULT_TAPS, iters: int = DEFAULT_ITERS, mu: float = DEFAULT_MU, modulus: float = 1.0,
                 layout: str = "frames"):
        super().__init__(length, layout)
        self.taps = _index(taps, "taps", 1, MAX_TAPS)
        self.iters = _index(iters, "iters", 0, MAX_ITERS)
        self.mu = _step(mu)
        self.modulus = _number(modulus, "modulus")

    def struct(self, w=None, w0=None, mode=1) -> N.Equaliser:
        """The iq_equaliser_t of one call (`w`, `w0`: device addresses)."""
        return N.Equaliser(taps=self.taps, iters=self.iters, planar=self.planar, mode=mode, mu=self.mu, modulus=self.modulus,
                           w=w, w0=w0)

    def __call__(self, x, w=None, w0=None, return_w=False, return_est=False):
        """x: device frames in this equaliser's layout, fp32 -> out of the same shape on the current stream, no host
        synchronisation; differentiable with respect to x (the weights held fixed).  w: (B, taps, 2) weights (or complex
        (B, taps)): nothing is adapted, out = w * x.  w0: the start of the descent in the same form (None: the unit spike at
        taps // 2).  Then, if asked for, w (B, taps, 2) fp32 and est (B, 4) fp32 = {J before (NaN with w=), J after, sum |w|^2,
        index of the largest |w|}."""
        return_w, return_est = _flag(return_w, "return_w"), _flag(return_est, "return_est")
        self._check_shape(x)
        if w is not None and w0 is not None:
            raise ValueError("w= gives the weights and w0= the start of the descent: pass one of them")
        shape, note = (x.shape[0], self.taps, 2), " = (re, im) per frame and tap"
        w = None if w is None else reals(w, "w", shape, x.device, note, pairs=True)
        w0 = None if w0 is None else reals(w0, "w0", shape, x.device, note, pairs=True)
        if not x.is_cuda:
            raise no_cpu(self)
        out, w_out, est = _HeldFn.apply(x, self, w, w0, return_est)
        return pack(out, w_out if return_w else None, est)

    def _forward(self, x, w, w0, want_est):
        B, d = x.shape[0], x.device
        out = torch.empty_like(x)
        w_out = torch.empty(B, self.taps, 2, dtype=torch.float32, device=d)    # the backward's weights, held fixed
        est = torch.empty(B, 4, dtype=torch.float32, device=d) if want_est else None
        if B > 0:
            par = self.struct(N.ptr(w), N.ptr(w0), mode=0 if w is not None else 1)
            N.check(N.lib().iq_frames_equalise(x.data_ptr(), out.data_ptr(), w_out.data_ptr(), N.ptr(est), B, self.length,
                                               C.byref(par), torch.cuda.current_stream(d).cuda_stream), "iq_frames_equalise")
        return out, w_out, (est,)

    def _backward(self, dout, dx, w, B):
        par = self.struct(w=w.data_ptr(), mode=0)
        N.check(N.lib().iq_frames_equalise_bwd(dout.data_ptr(), dx.data_ptr(), B, self.length, C.byref(par),
                                               torch.cuda.current_stream(dout.device).cuda_stream), "iq_frames_equalise_bwd")

    def __repr__(self):
        return (f"Equaliser(length={self.length}, taps={self.taps}, iters={self.iters}, mu={self.mu}, modulus={self.modulus}, "
                f"layout={self.layout!r})")


# ---- the host definition

def _complex_weights(w, B, L, what):
    w = _host(w)
    if not np.iscomplexobj(w):
        w = w.astype(np.float64)
        if w.shape != (B, L, 2):
            raise ValueError(f"{what} must have shape ({B}, {L}, 2), got {w.shape}")
        w = w[:, :, 0] + 1j * w[:, :, 1]
    if w.shape != (B, L):
        raise ValueError(f"{what} must have shape ({B}, {L}), got {w.shape}")
    return w.astype(np.complex128)


def _windows(z, L, adjoint=False):
    """X[b, n, l] = z[b, n + c - l] (adjoint: z[b, n - c + l]), zero outside the frame, c = L // 2."""
    c = L // 2
    if adjoint:
        zp = np.pad(z, ((0, 0), (c, L - 1 - c)))
        return np.lib.stride_tricks.sliding_window_view(zp, L, axis=1)
    zp = np.pad(z, ((0, 0), (L - 1 - c, c)))
    return np.lib.stride_tricks.sliding_window_view(zp, L, axis=1)[:, :, ::-1]


def cma_step_reference(z, w, modulus=1.0):
    """One step's pieces in fp64: z (B, len) complex, w (B, L) complex -> y (B, len), g (B, L), J (B,):
    y = w * z, e = y (|y|^2 - R), g[l] = mean_n conj(z[n + c - l]) e[n], J = mean_n (|y|^2 - R)^2.
    g is the gradient of J / 4 with respect to conj(w): in real terms dJ/dRe w = 4 Re g and dJ/dIm w = 4 Im g."""
    X = _windows(z, w.shape[1])
    with np.errstate(all="ignore"):
        y = np.einsum("bnl,bl->bn", X, w)
        d = y.real ** 2 + y.imag ** 2 - modulus
        g = np.einsum("bnl,bn->bl", np.conj(X), y * d) / z.shape[1]
        return y, g, np.mean(d ** 2, axis=1)


def equaliser_reference(x, taps, iters, mu, modulus=1.0, planar=False, w=None, w0=None):
    """The definition of include/iqvit.h in fp64 on the host.  x: (B, len, 2) or, planar, (B, 2, len).  w: (B, L, 2) or complex
    (B, L): IQ_EQ_GIVEN; w0: the start (None: the unit spike at L // 2).
    -> out (x's shape), w (B, L, 2), est (B, 4) = {J(w0) (NaN when given), J(w), sum |w|^2, argmax |w|}, float64."""
    z = _frames(x, planar)
    B = z.shape[0]
    L = _index(taps, "taps", 1, MAX_TAPS)
    est = np.full((B, 4), np.nan)
    if w is not None:
        wc = _complex_weights(w, B, L, "w")
    else:
        iters = _index(iters, "iters", 0, MAX_ITERS)
        if w0 is None:
            wc = np.zeros((B, L), np.complex128)
            wc[:, L // 2] = 1.0
        else:
            wc = _complex_weights(w0, B, L, "w0")
        for t in range(iters):
            _, g, J = cma_step_reference(z, wc, modulus)
            if t == 0:
                est[:, 0] = J
            wc = wc - mu * g
    y, _, J = cma_step_reference(z, wc, modulus)
    if w is None and iters == 0:
        est[:, 0] = J
    est[:, 1] = J
    p = wc.real ** 2 + wc.imag ** 2
    est[:, 2] = p.sum(axis=1)
    est[:, 3] = _first_largest(p, 1)[0]
    return _unframes(y, planar), np.stack([wc.real, wc.imag], axis=2), est


def equaliser_reference_bwd(dout, w, planar=False):
    """The adjoint in fp64 with the weights held at w ((B, L, 2) or complex (B, L)): the gradient of sum(out * dout) with respect
    to x, out = equaliser_reference(x, ..., w=w)[0]:  dx[m] = sum_l conj(w[l]) dout[m - c + l].  dout in x's layout -> dx
    likewise."""
    dz = _frames(dout, planar)
    w = _host(w)
    L = w.shape[1] if w.ndim >= 2 else 0
    wc = _complex_weights(w, dz.shape[0], L, "w")
    return _unframes(np.einsum("bml,bl->bm", _windows(dz, L, adjoint=True), np.conj(wc)), planar)
