"""Likelihood classifier on the device: the classical baseline of automatic modulation classification.

The ViT and the raw-IQ transformer are learned classifiers; the curve every AMC paper draws above them is the likelihood test
over the candidate constellations.  One HIP kernel (csrc/likelihood.hip, iq_frames_likelihood) computes, for every frame b, every
class c and every carrier rotation r of a table, the log-likelihood of the frame's symbols as independent draws from the class's
constellation in complex Gaussian noise of known variance,

  L[b, c, r] = sum_n ( -q d_min + log( (1 / M_c) sum_k exp(-q (d_k - d_min)) ) ),   d_k = |y'_n - a s_k|^2,  q = 1 / sigma2[b],
  y' = y (cos_r - j sin_r),

then over the rotations their maximum (mode 'max', the GLRT) or the log of their mean (mode 'mean', the ALRT) and the class of the
largest.  The term -len log(pi sigma2) is common to all classes and left out.  The definition with every rounding is written out in
include/iqvit.h.  The work is B R len sum_c M_c evaluations of a distance and an exponential -- 1.4e10 at B = 256, len = 1024,
R = 64 and the 812 points of the 17 table classes -- which torch broadcasting would materialise as a B x R x len x M tensor.
There is no CPU path; `likelihood_reference` is the host fp64 DEFINITION the tests compare against.

  LikelihoodClassifier(length, classes, rotations, mode, layout, differentiable)     clf(x, sigma2= | snr_db=, gain=) -> loglik (B, C)
  clf.predict(...) -> (B,) int64        clf.class_names          noise_for(snr_db, normalised) -> (gain, sigma2)
  clf.input_gradient(x, dloglik, sigma2= | snr_db=, gain=) -> dx       d <dloglik, loglik> / d x, the shape of x

The gradient with respect to the frame (csrc/likelihood_bwd.hip, iq_frames_likelihood_bwd) is the soft symbol decision:
-2 q (y - m) per hypothesis, m the posterior mean of the scaled points, summed over the classes by dloglik and over the rotations by
their shares ('mean') or at the winning rotation alone ('max': the true gradient wherever the maximum is unique).  With
differentiable=True, clf(x, ...) returns loglik on the autograd graph of x, so that Receiver -> Equaliser -> Carrier -> classifier
carries x.grad down to the raw frame; adversarial.fgsm / pgd / robustness_curve take the classifier in place of a model.
  likelihood_reference(x, sigma2, gain, points, classes, angles, mode) -> loglik, per-rotation table, best_rot, pred

The phase grid matters: on 128-symbol frames of the 17 classes at 20 dB the host definition classifies 68 of 68 with 64
rotations and 0.71-0.74 of them with 16 ("Likelihood classifier"), which is why the table is an argument.

Not here: GMSK and OQPSK (not memoryless: no point table) and an unknown noise variance (a grid over sigma2) -- for both see
cumulants.CumulantClassifier, the feature-based baseline -- and gradients with respect to sigma2, gain, the points or the
rotation table.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N
from . import data as D
from ._args import _flag, _index
from .stage import Stage, _first_largest, _frames, _host, no_cpu, pack, reals
from .synth import SHAPED, _points

LAYOUTS = ("frames", "planar")               # iq_likelihood_t.planar = 0: (B, length, 2), 1: (B, 2, length)
MODES = ("max", "mean")                      # IQ_LIK_MAX, IQ_LIK_MEAN
MAX_CLASSES, MAX_ROTATIONS, MAX_POINTS = 64, 256, 2048       # the limits of iq_frames_likelihood
TABLE_CLASSES = tuple(c for c in D.CLASSES if c not in SHAPED)          # the 17 classes data.constellation has a table for


def noise_for(snr_db, normalised=False):
    """(gain, sigma2) of frames at `snr_db`, a number, an array or a tensor (the result is of the same kind).  Two conventions:
    the generators (make_dataset, FrameSynth, ShapedSynth) emit a unit-power signal plus noise: a = 1, sigma2 = 10^(-snr/10).
    Receiver(normalise=True) emits a unit-power FRAME: signal and noise are both divided by sqrt(1 + sigma2), so
    a^2 = 1 / (1 + sigma2) and the variance is sigma2 / (1 + sigma2)."""
    normalised = _flag(normalised, "normalised")
    if isinstance(snr_db, torch.Tensor):
        s2 = torch.pow(10.0, -snr_db.to(torch.float64) / 10.0)
        one = torch.ones_like(s2)
        return (torch.rsqrt(1.0 + s2), s2 / (1.0 + s2)) if normalised else (one, s2)
    s2 = np.power(10.0, -np.asarray(snr_db, dtype=np.float64) / 10.0)
    gain, s2 = (1.0 / np.sqrt(1.0 + s2), s2 / (1.0 + s2)) if normalised else (np.ones_like(s2), s2)
    return (float(gain), float(s2)) if s2.ndim == 0 else (gain, s2)


def _rotation_angles(rotations):
    if isinstance(rotations, (int, np.integer)) and not isinstance(rotations, bool):
        R = _index(rotations, "rotations", 1, MAX_ROTATIONS)
        return 2.0 * np.pi * np.arange(R, dtype=np.float64) / R
    try:
        ang = np.asarray(_host(rotations), dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError(f"rotations must be a count or an array of angles in radians, got {rotations!r}") from None
    if isinstance(rotations, (bool, float)) or ang.ndim != 1:
        raise TypeError(f"rotations must be a count or a one-dimensional array of angles in radians, got {rotations!r}")
    if not 1 <= ang.size <= MAX_ROTATIONS:
        raise ValueError(f"between 1 and {MAX_ROTATIONS} rotations, got {ang.size}")
    if not np.all(np.isfinite(ang)):
        raise ValueError("rotations has a non-finite angle")
    return ang


def rotation_table(angles):
    """(R, 2) fp32 = (cos, sin) of the angles, computed in fp64: what the kernel reads."""
    ang = np.asarray(angles, dtype=np.float64)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)


class _LoglikFn(torch.autograd.Function):
    """loglik = clf(x), differentiable with respect to x with the forward's per-(frame, class) results held fixed.  The classifier
    (LikelihoodClassifier, likelihood_em.HybridLikelihoodClassifier; cumulants.CumulantClassifier, which holds sigma2 alone) supplies
      _forward(x, *args) -> (loglik, *extras), held     the forward's C call (x contiguous fp32); held: what the backward reads,
                                                        tensors or None
      _backward(x, dloglik, *held) -> dx                the one C call
    -> (loglik, *extras); the extras are marked non-differentiable."""

    @staticmethod
    def forward(ctx, x, clf, *args):
        x = x.detach().contiguous().float()
        outs, held = clf._forward(x, *args)
        ctx.clf = clf
        ctx.save_for_backward(x, *held)
        ctx.mark_non_differentiable(*[t for t in outs[1:] if t is not None])      # all in ONE call
        return outs

    @staticmethod
    def backward(ctx, dloglik, *_):
        x, *held = ctx.saved_tensors
        return (ctx.clf._backward(x, dloglik.contiguous().float(), *held),) + (None,) * (len(ctx.needs_input_grad) - 1)


def _dloglik(dloglik, x, n_classes):
    """The (B, C) gradient argument of input_gradient: a tensor, fp32 and contiguous on x's device."""
    if not isinstance(dloglik, torch.Tensor) or dloglik.dtype.is_complex or dloglik.dtype == torch.bool:
        raise TypeError(f"dloglik must be a tensor of real numbers, got {dloglik!r}")
    if tuple(dloglik.shape) != (x.shape[0], n_classes):
        raise ValueError(f"dloglik must have shape {(x.shape[0], n_classes)}: one value per frame and class, got {tuple(dloglik.shape)}")
    return dloglik.detach().to(device=x.device, dtype=torch.float32).contiguous()


class LikelihoodClassifier(Stage):
    """Frames of `length` symbols at one sample per symbol -> the log-likelihood of each of the classes.  classes: names
    data.constellation knows (default: its 17, in data.CLASSES' order), (name, points) pairs or {name: points} for constellations
    of one's own, scaled to unit mean power in fp64 and rounded to the fp32 table as FrameSynth does.  rotations: a count R
    (angles 2 pi r / R, the full circle) or an array of angles in radians.  mode: 'max' or 'mean' over the rotations.  layout:
    'frames' (B, length, 2) or 'planar' (B, 2, length).  differentiable: a call returns loglik on the autograd graph of x (the
    extras are not differentiable); False: x is detached.  A call runs on the device its x lies on.  Arguments are checked here,
    before any device work."""

    LAYOUTS, reference = LAYOUTS, "likelihood_reference"

    def __init__(self, length, classes=None, rotations=64, mode: str = "max", layout: str = "frames", differentiable=False):
        super().__init__(length, layout)
        self.differentiable = _flag(differentiable, "differentiable")
        if classes is None:
            classes = TABLE_CLASSES
        if isinstance(classes, str):
            raise TypeError(f"classes must be a list of names or (name, points) pairs, got {classes!r}")
        items = list(classes.items()) if isinstance(classes, dict) else [c if isinstance(c, tuple) else (c, None) for c in classes]
        if not items:
            raise ValueError("classes is empty")
        if len(items) > MAX_CLASSES:
            raise ValueError(f"at most {MAX_CLASSES} classes, got {len(items)}")
        self.class_names, self.descriptors, tables, off = [], [], [], 0
        for item in items:
            if len(item) != 2 or not isinstance(item[0], str):
                raise TypeError(f"a class is a name or a (name, points) pair, got {item!r}")
            name, pts = item
            if name in self.class_names:
                raise ValueError(f"class {name!r} is listed twice")
            if pts is None:
                if name in SHAPED:
                    raise ValueError(f"class {name!r} is not memoryless: it has no point table and no likelihood here")
                try:
                    pts = D.constellation(name)
                except KeyError:
                    raise ValueError(f"unknown class {name!r}: not a name of data.constellation") from None
            c = _points(name, pts)
            self.class_names.append(name)
            self.descriptors.append((0, off, len(c)))
            tables.append(c)
            off += len(c)
        if off > MAX_POINTS:
            raise ValueError(f"at most {MAX_POINTS} points in all, got {off}")
        pts64 = np.concatenate(tables)
        self.points = np.stack([pts64.real, pts64.imag], axis=1).astype(np.float32)           # (P, 2): the kernel's table
        self.angles = _rotation_angles(rotations)
        self.rot = rotation_table(self.angles)                                                # (R, 2): the kernel's table
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        self.mode = mode
        self._classes_c = (N.SynthClass * len(self.descriptors))(*[N.SynthClass(*d) for d in self.descriptors])

    @property
    def n_classes(self):
        return len(self.descriptors)

    @property
    def n_rotations(self):
        return len(self.angles)

    def tables_on(self, device):
        """(points, rot) as fp32 tensors on `device`, uploaded once per device."""
        return self.table_on(device, ("points", "rot"))

    def struct(self, points=None, rot=None, gain=None) -> N.Likelihood:
        """The iq_likelihood_t of one call (`points`, `rot`, `gain`: device addresses)."""
        return N.Likelihood(points=points, classes=self._classes_c, n_classes=self.n_classes, rot=rot, n_rot=self.n_rotations,
                            planar=self.planar, mode=MODES.index(self.mode), gain=gain)

    def _check(self, x, sigma2=None, snr_db=None, gain=None):
        self._check_shape(x)
        if (sigma2 is None) == (snr_db is None):
            raise ValueError("pass the noise as sigma2= (the variance per frame) or as snr_db= (generator convention): one of them")
        shape, note = (x.shape[0],), ", one value per frame"
        if sigma2 is None:
            sigma2 = noise_for(reals(snr_db, "snr_db", shape, None, note))[1]
        sigma2 = reals(sigma2, "sigma2", shape, x.device, note)
        gain = None if gain is None else reals(gain, "gain", shape, x.device, note)
        if not x.is_cuda:
            raise no_cpu(self)
        return sigma2, gain

    def _run(self, x, sigma2, snr_db, gain, want_rot, want_best, want_pred):
        sigma2, gain = self._check(x, sigma2, snr_db, gain)
        return self._launch(x.detach().contiguous().float(), sigma2, gain, want_rot, want_best, want_pred)

    def _launch(self, x, sigma2, gain, want_rot, want_best, want_pred):
        B, d, Cn, R = x.shape[0], x.device, self.n_classes, self.n_rotations
        loglik = torch.empty(B, Cn, dtype=torch.float32, device=d)
        rot_ll = torch.empty(B, Cn, R, dtype=torch.float32, device=d) if want_rot else None
        best = torch.empty(B, Cn, dtype=torch.int32, device=d) if want_best else None
        pred = torch.empty(B, dtype=torch.int32, device=d) if want_pred else None
        if B > 0:
            points, rot = self.table_on(d, ("points", "rot"))
            par = self.struct(points.data_ptr(), rot.data_ptr(), N.ptr(gain))
            N.check(N.lib().iq_frames_likelihood(x.data_ptr(), sigma2.data_ptr(), loglik.data_ptr(), N.ptr(rot_ll), N.ptr(best),
                                                 N.ptr(pred), B, self.length, C.byref(par),
                                                 torch.cuda.current_stream(d).cuda_stream), "iq_frames_likelihood")
        return loglik, rot_ll, best, pred

    def _forward(self, x, sigma2, gain, want_rot=False, want_best=False):
        """_LoglikFn's forward: the extras asked for, and held = (sigma2, gain, loglik, rot_ll, best_rot), of the last three what
        the mode's backward reads."""
        mean = self.mode == "mean"
        loglik, rot_ll, best, _ = self._launch(x, sigma2, gain, want_rot or mean, want_best or not mean, False)
        return (loglik, rot_ll if want_rot else None, best if want_best else None), \
            (sigma2, gain, loglik if mean else None, rot_ll if mean else None, None if mean else best)

    def _backward(self, x, dloglik, sigma2, gain, loglik, rot_ll, best):
        dx = torch.empty_like(x)
        if x.shape[0] > 0:
            points, rot = self.table_on(x.device, ("points", "rot"))
            par = self.struct(points.data_ptr(), rot.data_ptr(), N.ptr(gain))
            N.check(N.lib().iq_frames_likelihood_bwd(x.data_ptr(), sigma2.data_ptr(), dloglik.data_ptr(), N.ptr(loglik), N.ptr(rot_ll),
                                                     N.ptr(best), dx.data_ptr(), x.shape[0], self.length, C.byref(par),
                                                     torch.cuda.current_stream(x.device).cuda_stream), "iq_frames_likelihood_bwd")
        return dx

    def input_gradient(self, x, dloglik, sigma2=None, snr_db=None, gain=None):
        """d <dloglik, loglik> / d x: x and the noise as in a call, dloglik (B, C) a tensor (a one-hot row: that class's
        gradient; a class with weight 0 costs nothing).  -> dx, the shape of x, fp32.  Two C calls (the forward for what the
        backward reads, then the backward) on the current stream, no autograd and no host synchronisation."""
        self._check_shape(x)
        dloglik = _dloglik(dloglik, x, self.n_classes)
        sigma2, gain = self._check(x, sigma2, snr_db, gain)
        x = x.detach().contiguous().float()
        with torch.no_grad():
            return self._backward(x, dloglik, *self._forward(x, sigma2, gain)[1])

    def __call__(self, x, sigma2=None, snr_db=None, gain=None, return_rot=False, return_best=False):
        """x: device frames in this classifier's layout, fp32; the noise as sigma2 (variance E|w|^2 per frame: a number or B
        values) or as snr_db (generator convention: noise_for(snr_db)); gain: the amplitude of the constellation in the frame
        (None: 1).  -> loglik (B, C) fp32 on the current stream, no host synchronisation; then, if asked for, the per-rotation
        table (B, C, R) fp32 and best_rot (B, C) int32, the first rotation that attains the maximum.  A frame whose sigma2 is
        not a positive finite number gets NaN (best_rot -1)."""
        return_rot, return_best = _flag(return_rot, "return_rot"), _flag(return_best, "return_best")
        if self.differentiable:
            return pack(*_LoglikFn.apply(x, self, *self._check(x, sigma2, snr_db, gain), return_rot, return_best))
        loglik, rot_ll, best, _ = self._run(x, sigma2, snr_db, gain, return_rot, return_best, False)
        return pack(loglik, rot_ll, best)

    def predict(self, x, sigma2=None, snr_db=None, gain=None):
        """-> (B,) int64: the first class with the largest log-likelihood; -1 for a frame whose sigma2 is refused."""
        return self._run(x, sigma2, snr_db, gain, False, False, True)[3].long()

    noise_for = staticmethod(noise_for)

    def __repr__(self):
        return (f"LikelihoodClassifier(length={self.length}, classes={self.class_names!r}, rotations={self.n_rotations}, "
                f"mode={self.mode!r}, layout={self.layout!r}{', differentiable=True' if self.differentiable else ''})")


# ---- the host definition

def likelihood_reference(x, sigma2, gain, points, classes, angles, mode="max", planar=False):
    """The definition of include/iqvit.h in fp64 on the host.  x: (B, len, 2) or, planar, (B, 2, len); sigma2: (B,) or a number;
    gain: (B,), a number or None (1); points: (P, 2) or complex (P,); classes: (offset, count) or (kind, offset, count) per class;
    angles: (R,) in radians, or the (R, 2) table of (cos, sin) itself; mode: 'max' / 'mean' (or IQ_LIK_*).
    -> loglik (B, C), L (B, C, R) float64, best_rot (B, C), pred (B,) int64.  A frame whose sigma2 is not a positive finite
    number has NaN in loglik and L and -1 in best_rot and pred."""
    y = _frames(x, planar)
    B, n = y.shape
    s2 = np.broadcast_to(np.asarray(_host(sigma2), dtype=np.float64), (B,))
    a = np.ones(B) if gain is None else np.broadcast_to(np.asarray(_host(gain), dtype=np.float64), (B,))
    p = _host(points)
    p = p.astype(np.complex128).reshape(-1) if np.iscomplexobj(p) else p.astype(np.float64).reshape(-1, 2) @ np.array([1, 1j])
    rot = np.asarray(_host(angles), dtype=np.float64)
    rot = np.cos(rot) - 1j * np.sin(rot) if rot.ndim == 1 else rot[:, 0] - 1j * rot[:, 1]
    mode = MODES[mode] if isinstance(mode, (int, np.integer)) else mode
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    descs = [tuple(int(v) for v in c) for c in classes]
    descs = [d[1:] if len(d) == 3 else d for d in descs]
    if any(len(d) != 2 or d[0] < 0 or d[1] < 1 or d[0] + d[1] > len(p) for d in descs) or \
            any(len(c) == 3 and int(c[0]) != 0 for c in classes):
        raise ValueError(f"classes must be (offset, count) ranges of the {len(p)} points, of kind 0, got {list(classes)!r}")
    R, Cn = len(rot), len(descs)
    with np.errstate(invalid="ignore"):
        ok = (s2 > 0) & np.isfinite(s2)
    q = np.where(ok, 1.0 / np.where(ok, s2, 1.0), np.nan)
    L = np.empty((B, Cn, R))
    yr = y[:, None, :] * rot[None, :, None]                                  # (B, R, n)
    # the B R n M evaluations in torch's fp64 on the host (its element-wise kernels use every core; numpy's use one)
    yre, yim, qt = torch.from_numpy(yr.real.copy()), torch.from_numpy(yr.imag.copy()), torch.from_numpy(q)
    for c, (off, M) in enumerate(descs):
        step = max(1, (1 << 22) // (R * n * M))
        for b0 in range(0, B, step):
            sl = slice(b0, b0 + step)
            pk = a[sl, None] * p[None, off:off + M]                          # (b, M)
            dr = yre[sl, :, :, None] - torch.from_numpy(pk.real.copy())[:, None, None, :]
            di = yim[sl, :, :, None] - torch.from_numpy(pk.imag.copy())[:, None, None, :]
            d = dr.mul_(dr).add_(di.mul_(di))                                # (b, R, n, M): the difference form
            dmin = d.amin(dim=3)
            qq = qt[sl, None, None]
            ln = -qq * dmin + d.sub_(dmin[..., None]).mul_(-qq[..., None]).exp_().mean(dim=3).log_()
            L[sl, c, :] = ln.sum(dim=2).numpy()
    best_rot, m = _first_largest(L, 2)
    if mode == "max":
        loglik = m
    else:
        with np.errstate(all="ignore"):
            loglik = m + np.log(np.exp(L - m[..., None]).mean(axis=2))
    pred = _first_largest(loglik, 1)[0]
    loglik = np.where(ok[:, None], loglik, np.nan)
    L[~ok] = np.nan
    best_rot[~ok] = -1
    pred[~ok] = -1
    return loglik, L, best_rot, pred
