"""Tracking equaliser on the device: the block constant-modulus descent per overlapping segment, and weights that move over time.

equaliser.Equaliser finds ONE filter per frame.  Behind fading.Fading the channel turns within the frame and that filter is the
compromise of all its states ("Fading channel": the hybrid likelihood column falls from 0.594 to 0.219 at a maximum
Doppler of 3e-4 cycles per sample).  Here the frame is cut into segments of `seg` symbols, `hop` apart; every segment runs
`track_iters` steps of the same descent on its own tapered cost J_j(w) = sum_k h[k] (|y[j hop + k]|^2 - R)^2, all from the same
start -- the whole frame's block solution, which the parent class finds with the existing kernel -- so that the segments agree
on the gain, rotation and delay that CMA leaves open; then the frame is filtered with weights interpolated linearly between the
segments' centres.  Every (frame, segment) descent is independent: one wave each, no recursion along the frame (csrc/
equaliser_track.hip, iq_frames_equalise_track; the definition is written out in include/iqvit.h).  iq_frames_equalise_track_bwd is
the adjoint with the (B, S, taps, 2) weights held fixed.  There is no CPU path; `equaliser_track_reference` / `_bwd` are the host
fp64 DEFINITIONS the tests compare against.

The limit is the block equaliser's, sharpened: J rewards a constant modulus, and a segment is a short frame.  PSK gains wherever
the channel moves and loses nothing where it holds still; 16QAM on a segment of 128 symbols fits the segment's own symbol
pattern and loses on a still channel ("Tracking equaliser", has the figures).  Use longer segments or few steps for
classes without a constant modulus.

  TrackingEqualiser(length, taps, iters, mu, modulus, layout, seg, hop, track_iters, track_mu, taper)
      (x, w=, w0=) -> out [, w (B, S, taps, 2), est]
  taper_table(seg, kind) -> fp32 [seg], sum 1          segments(length, seg, hop) -> S
  equaliser_track_reference(x, taps, iters, mu, seg, hop, taper, ...) -> out, w, est
  equaliser_track_reference_bwd(dout, w, seg, hop, planar) -> dx
  segment_step_reference(z, w, seg, hop, taper, modulus) -> y, g, J     one step's pieces of every segment

Not here: phase and amplitude tracking behind the equaliser, decision-directed or RLS updates, fractionally spaced operation on
the raw frame, choosing seg, hop or modulus per frame, and differentiating through the descent.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N
from ._args import _flag, _index
from .equaliser import (DEFAULT_ITERS, DEFAULT_MU, DEFAULT_TAPS, MAX_ITERS, MAX_TAPS, Equaliser, _complex_weights, _step, _windows,
                        cma_step_reference)
from .stage import _frames, _HeldFn, _host, _unframes, no_cpu, pack, reals

MAX_SEG, MAX_SEGMENTS = 512, 256             # the limits of iq_frames_equalise_track
TAPERS = ("hann", "rect")
# The defaults: chosen on the host definition over track_mu in {0.05 .. 0.8} x track_iters in {8 .. 128} on faded QPSK frames
# ("Tracking equaliser", has the sweep)
DEFAULT_SEG, DEFAULT_HOP, DEFAULT_TRACK_ITERS, DEFAULT_TRACK_MU = 128, 64, 32, 0.2


def segments(length, seg, hop):
    """S, the number of segments of a frame of `length` symbols."""
    seg = _index(seg, "seg", 1, MAX_SEG)
    hop = _index(hop, "hop", 1, seg)
    length = _index(length, "length", seg, 2 ** 31 - 1)
    return (length - seg) // hop + 1


def taper_table(seg, kind="hann"):
    """fp32 [seg] with sum 1 (in fp64, before the rounding): 'hann': 0.5 - 0.5 cos(2 pi (k + 1/2) / seg), which has no zero entry
    and is 1.0 at seg = 1; 'rect': 1 / seg each."""
    seg = _index(seg, "seg", 1, MAX_SEG)
    if kind not in TAPERS:
        raise ValueError(f"taper must be one of {TAPERS}, got {kind!r}")
    if kind == "rect":
        return np.full(seg, 1.0 / seg, np.float32)
    h = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(seg) + 0.5) / seg)
    return (h / h.sum()).astype(np.float32)


class TrackingEqualiser(Equaliser):
    """Frames of `length` symbols -> the same frames through a blind `taps`-tap equaliser whose weights follow the channel.
    taps, iters, mu, modulus, layout: those of Equaliser; they find the start w0, one filter for the whole frame.  seg, hop: the
    segments (S = (length - seg) // hop + 1 of them, at most 256); track_iters, track_mu: the steps every segment takes from w0
    on its own cost and their size (the taper sums to 1, so the gradient is a mean and track_mu does not depend on seg);
    taper: 'hann' or 'rect'.  A call runs on the device its x lies on.  Arguments are checked here, before any device work."""

    reference = "equaliser_track_reference"

    def __init__(self, length, taps: int = DEFAULT_TAPS, iters: int = DEFAULT_ITERS, mu: float = DEFAULT_MU, modulus: float = 1.0,
                 layout: str = "frames", seg: int = DEFAULT_SEG, hop: int = DEFAULT_HOP, track_iters: int = DEFAULT_TRACK_ITERS,
                 track_mu: float = DEFAULT_TRACK_MU, taper: str = "hann"):
        super().__init__(length, taps, iters, mu, modulus, layout)
        self.seg = _index(seg, "seg", 1, MAX_SEG)
        self.hop = _index(hop, "hop", 1, self.seg)
        if self.length < self.seg:
            raise ValueError(f"length must be at least seg = {self.seg}, got {self.length}")
        self.segments = segments(self.length, self.seg, self.hop)
        if self.segments > MAX_SEGMENTS:
            raise ValueError(f"length {self.length}, seg {self.seg} and hop {self.hop} give {self.segments} segments: at most "
                             f"{MAX_SEGMENTS} are supported")
        self.track_iters = _index(track_iters, "track_iters", 0, MAX_ITERS)
        self.track_mu = _step(track_mu)
        self.taper = taper
        self.table = taper_table(self.seg, taper)

    def track_struct(self, w=None, w0=None, taper=None, mode=1) -> N.EqualiserTrack:
        """The iq_equaliser_track_t of one call (`w`, `w0`, `taper`: device addresses)."""
        return N.EqualiserTrack(taps=self.taps, iters=self.track_iters, planar=self.planar, mode=mode, seg=self.seg, hop=self.hop,
                                mu=self.track_mu, modulus=self.modulus, w=w, w0=w0, taper=taper)

    def __call__(self, x, w=None, w0=None, return_w=False, return_est=False):
        """x: device frames in this equaliser's layout, fp32 -> out of the same shape on the current stream, no host
        synchronisation; differentiable with respect to x (the weights held fixed).  w: (B, S, taps, 2) weights per segment (or
        complex (B, S, taps)): nothing is adapted.  w0: (B, taps, 2) (or complex (B, taps)), the start of every segment's descent
        (None: the parent's block descent over the whole frame finds it).  Then, if asked for, w (B, S, taps, 2) fp32 and est
        (B, 4) fp32 = {J under w0 alone (NaN with w=), J(out), the largest sum |w_j - w0|^2 (NaN with w=), S}."""
        return_w, return_est = _flag(return_w, "return_w"), _flag(return_est, "return_est")
        self._check_shape(x)
        if w is not None and w0 is not None:
            raise ValueError("w= gives the weights and w0= the start of the descent: pass one of them")
        B = x.shape[0]
        w = None if w is None else reals(w, "w", (B, self.segments, self.taps, 2), x.device, " = (re, im) per frame, segment and tap",
                                         pairs=True)
        w0 = None if w0 is None else reals(w0, "w0", (B, self.taps, 2), x.device, " = (re, im) per frame and tap", pairs=True)
        if not x.is_cuda:
            raise no_cpu(self)
        out, w_out, est = _HeldFn.apply(x, self, w, w0, return_est)
        return pack(out, w_out if return_w else None, est)

    def _forward(self, x, w, w0, want_est):
        B, d = x.shape[0], x.device
        if w is None and w0 is None and B > 0:
            w0 = Equaliser._forward(self, x, None, None, False)[1]           # the whole frame's block solution (the existing kernel)
        out = torch.empty_like(x)
        w_out = torch.empty(B, self.segments, self.taps, 2, dtype=torch.float32, device=d)   # the backward's weights, held fixed
        est = torch.empty(B, 4, dtype=torch.float32, device=d) if want_est else None
        if B > 0:
            par = self.track_struct(N.ptr(w), N.ptr(w0), self.table_on(d).data_ptr(), mode=0 if w is not None else 1)
            N.check(N.lib().iq_frames_equalise_track(x.data_ptr(), out.data_ptr(), w_out.data_ptr(), N.ptr(est), B, self.length,
                                                     C.byref(par), torch.cuda.current_stream(d).cuda_stream),
                    "iq_frames_equalise_track")
        return out, w_out, (est,)

    def _backward(self, dout, dx, w, B):
        par = self.track_struct(w=w.data_ptr(), mode=0)
        N.check(N.lib().iq_frames_equalise_track_bwd(dout.data_ptr(), dx.data_ptr(), B, self.length, C.byref(par),
                                                     torch.cuda.current_stream(dout.device).cuda_stream),
                "iq_frames_equalise_track_bwd")

    def __repr__(self):
        return (f"TrackingEqualiser(length={self.length}, taps={self.taps}, iters={self.iters}, mu={self.mu}, modulus={self.modulus}, "
                f"layout={self.layout!r}, seg={self.seg}, hop={self.hop}, track_iters={self.track_iters}, track_mu={self.track_mu}, "
                f"taper={self.taper!r})")


# ---- the host definition

def _segment_weights(w, B, S, L, what):
    w = _host(w)
    if not np.iscomplexobj(w):
        w = w.astype(np.float64)
        if w.shape != (B, S, L, 2):
            raise ValueError(f"{what} must have shape ({B}, {S}, {L}, 2), got {w.shape}")
        w = w[..., 0] + 1j * w[..., 1]
    if w.shape != (B, S, L):
        raise ValueError(f"{what} must have shape ({B}, {S}, {L}), got {w.shape}")
    return w.astype(np.complex128)


def _taper(taper, seg):
    h = _host(taper).astype(np.float64)
    if h.shape != (seg,):
        raise ValueError(f"taper must have shape ({seg},), got {h.shape}")
    return h


def weights_over_time(w, n, seg, hop):
    """w (B, S, L) complex, n: integer output indices (any) -> w(n) (B, len(n), L): the first segment's weights up to its centre
    seg // 2, the last one's from its centre on, and in between w_j + a (w_{j+1} - w_j), j = t // hop, a = fp32(t % hop) / fp32(hop)
    with t = n - seg // 2."""
    S = w.shape[1]
    t = np.asarray(n, dtype=np.int64) - seg // 2
    inner = (t > 0) & (t < (S - 1) * hop)
    j = np.where(inner, t // hop, np.where(t <= 0, 0, S - 1))
    a = np.where(inner, ((t % hop).astype(np.float32) / np.float32(hop)).astype(np.float64), 0.0)
    wa, wb = w[:, j, :], w[:, np.minimum(j + 1, S - 1), :]
    return np.where(inner[None, :, None], wa + a[None, :, None] * (wb - wa), wa)


def segment_step_reference(z, w, seg, hop, taper, modulus=1.0):
    """One step's pieces of every segment in fp64: z (B, len) complex, w (B, S, L) complex, taper (seg,) ->
    y (B, S, seg): y[b, j, k] = sum_l w[b, j, l] z[b, j hop + k + c - l]; g (B, S, L): g[l] = sum_k h[k] conj(z[j hop + k + c - l]) e[k],
    e = y (|y|^2 - R); J (B, S) = sum_k h[k] (|y|^2 - R)^2.  g is the gradient of J / 4 with respect to conj(w)."""
    B, n = z.shape
    S, L = w.shape[1], w.shape[2]
    h = _taper(taper, seg)
    X = _windows(z, L)                                                        # [b, n, l] = z[b, n + c - l]
    idx = (np.arange(S) * hop)[:, None] + np.arange(seg)[None, :]             # [j, k] -> n
    Xs = X[:, idx, :]                                                         # [b, j, k, l]
    with np.errstate(all="ignore"):
        y = np.einsum("bjkl,bjl->bjk", Xs, w)
        d = y.real ** 2 + y.imag ** 2 - modulus
        g = np.einsum("bjkl,bjk->bjl", np.conj(Xs), y * d * h[None, None, :])
        return y, g, (d ** 2 * h[None, None, :]).sum(axis=2)


def _filter_over_time(z, w, seg, hop, adjoint=False):
    B, n = z.shape
    L = w.shape[2]
    c = L // 2
    with np.errstate(all="ignore"):
        if not adjoint:
            return np.einsum("bnl,bnl->bn", _windows(z, L), weights_over_time(w, np.arange(n), seg, hop))
        # dx[m] = sum_l conj(w(m - c + l)[l]) dout[m - c + l]
        wt = weights_over_time(w, np.arange(-c, n + L - 1 - c), seg, hop)     # [b, n - c .. , l]
        rows = np.arange(n)[:, None] + np.arange(L)[None, :]                  # m - c + l, offset by c
        wml = wt[:, rows, np.arange(L)[None, :]]                              # [b, m, l]
        return np.einsum("bml,bml->bm", _windows(z, L, adjoint=True), np.conj(wml))


def equaliser_track_reference(x, taps, iters, mu, seg, hop, taper, modulus=1.0, planar=False, w=None, w0=None):
    """The definition of include/iqvit.h in fp64 on the host.  x: (B, len, 2) or, planar, (B, 2, len).  taper: (seg,) numbers.
    w: (B, S, L, 2) or complex (B, S, L): IQ_EQT_GIVEN; w0: (B, L, 2) or complex (B, L), the start of every segment (None: the unit
    spike at L // 2).  -> out (x's shape), w (B, S, L, 2), est (B, 4) = {J under w0 alone (NaN when given), J(out), max_j
    sum_l |w_j[l] - w0[l]|^2 (NaN when given), S}, float64."""
    z = _frames(x, planar)
    B, n = z.shape
    L = _index(taps, "taps", 1, MAX_TAPS)
    S = segments(n, seg, hop)
    if S > MAX_SEGMENTS:
        raise ValueError(f"{S} segments: at most {MAX_SEGMENTS} are supported")
    est = np.full((B, 4), np.nan)
    if w is not None:
        ws = _segment_weights(w, B, S, L, "w")
    else:
        iters = _index(iters, "iters", 0, MAX_ITERS)
        if w0 is None:
            wc = np.zeros((B, L), np.complex128)
            wc[:, L // 2] = 1.0
        else:
            wc = _complex_weights(w0, B, L, "w0")
        ws = np.repeat(wc[:, None, :], S, axis=1)
        for _ in range(iters):
            ws = ws - mu * segment_step_reference(z, ws, seg, hop, taper, modulus)[1]
        est[:, 0] = cma_step_reference(z, wc, modulus)[2]
        with np.errstate(all="ignore"):
            D = (np.abs(ws - wc[:, None, :]) ** 2).sum(axis=2)
        best = D[:, 0].copy()
        for j in range(1, S):                                                 # (a NaN is neither larger nor beaten: the kernel's walk)
            up = D[:, j] > best
            best[up] = D[up, j]
        est[:, 2] = best
    y = _filter_over_time(z, ws, seg, hop)
    with np.errstate(all="ignore"):
        est[:, 1] = np.mean((y.real ** 2 + y.imag ** 2 - modulus) ** 2, axis=1)
    est[:, 3] = S
    return _unframes(y, planar), np.stack([ws.real, ws.imag], axis=3), est


def equaliser_track_reference_bwd(dout, w, seg, hop, planar=False):
    """The adjoint in fp64 with the weights held at w ((B, S, L, 2) or complex (B, S, L)): the gradient of sum(out * dout) with
    respect to x, out = equaliser_track_reference(x, ..., w=w)[0]:  dx[m] = sum_l conj(w(n)[l]) dout[n], n = m - c + l.  dout in x's
    layout -> dx likewise."""
    dz = _frames(dout, planar)
    w = _host(w)
    if w.ndim < 3:
        raise ValueError(f"w must be (B, S, L, 2) or complex (B, S, L), got {w.shape}")
    ws = _segment_weights(w, dz.shape[0], segments(dz.shape[1], seg, hop), w.shape[2], "w")
    return _unframes(_filter_over_time(dz, ws, seg, hop, adjoint=True), planar)
