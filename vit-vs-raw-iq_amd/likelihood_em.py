"""Hybrid likelihood classifier on the device: the likelihood test with the gain, the carrier phase and the noise unknown.

likelihood.LikelihoodClassifier needs the noise variance, the amplitude of the constellation in the frame and a phase grid fine
enough for the densest class -- three things no receiver has.  The hybrid likelihood-ratio test (HLRT) estimates them per frame
and per candidate class: the maximum-likelihood complex gain h (amplitude and phase together, continuous: no grid) and noise
variance v by expectation-maximisation (EM) from a table of starting phases, and compares the classes at their own estimates,

  Lambda[b, c] = max over the starts of  sum_n log( (1 / M_c) sum_k exp(-|y_n - h s_k|^2 / v) ) - len log(pi v)   at the EM's (h, v).

One HIP kernel (csrc/likelihood_em.hip, iq_frames_likelihood_em) runs all starts and all iterations of a (frame, class) inside
one workgroup, one EM chain per wave; the definition with every rounding is written out in include/iqvit.h.  |h|^2 / v of the
winning class is a blind SNR estimate, and (v, |h|) are what LikelihoodClassifier(sigma2=, gain=) and
CumulantClassifier(sigma2=) were missing.  There is no CPU path; `likelihood_em_reference` is the host fp64 DEFINITION the tests
compare against.

  HybridLikelihoodClassifier(length, classes, starts, iters, init_noise, floor, layout, differentiable)     clf(x) -> Lambda (B, C)
  clf.predict(x) -> (B,) int64        clf.estimate(x) -> (pred, snr_db, sigma2, gain)        clf.class_names
  clf.input_gradient(x, dloglik) -> dx       d <dloglik, Lambda> / d x with the estimate (h, v) held fixed, the shape of x

The gradient with respect to the frame (csrc/likelihood_bwd.hip, iq_frames_likelihood_em_bwd) holds the estimate fixed, as the
receiver holds its timing and the equaliser its weights: -(2 / v) (y - m), m the posterior mean of h s_k.  At a converged interior
EM point that is also the total derivative (the estimate maximises the likelihood it is put into).  differentiable=True puts
clf(x) on the autograd graph of x; adversarial.fgsm / pgd / robustness_curve take the classifier in place of a model.
  likelihood_em_reference(x, points, classes, starts, iters, init_noise, floor, h0, v0) -> EmReference

The defaults (16 starts, 32 iterations, a starting noise share of 0.02) are from the host sweep in DESIGN.md, "Hybrid likelihood
classifier": the iteration count and the starting variance matter a great deal, the number of starts beyond 16 does not.

Not here: pruning the starts, a class-dependent start table, a convergence test in place of a fixed `iters`, GMSK and OQPSK (no
point table), a frequency offset inside the model (carrier.Carrier comes first), differentiating through the EM iterations,
gradients with respect to the points.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _native as N
from ._args import _flag, _index, _number
from .likelihood import LAYOUTS, MAX_ROTATIONS, LikelihoodClassifier, _dloglik, _LoglikFn, _rotation_angles, rotation_table
from .stage import Stage, _first_largest, _frames, _host, no_cpu, pack, reals

MAX_STARTS, MAX_ITERS = MAX_ROTATIONS, 4096             # the limits of iq_frames_likelihood_em (its classes: iq_frames_likelihood's)
MODES = ("table", "given")                              # IQ_EM_TABLE, IQ_EM_GIVEN

EmReference = collections.namedtuple("EmReference", "loglik h v best_start start_ll pred snr_db trace")


def _start_angles(starts):
    try:
        return _rotation_angles(starts)
    except (TypeError, ValueError) as e:                 # the same check, in this argument's name
        raise type(e)(str(e).replace("rotations", "starts")) from None


class HybridLikelihoodClassifier(Stage):
    """Frames of `length` symbols at one sample per symbol -> the log-likelihood of each class at its own EM estimate of the
    complex gain and the noise variance.  classes: as LikelihoodClassifier's (whose table and checks these are).  starts: a count
    T (phases 2 pi t / T) or an array of phases in radians.  iters: EM updates per start.  init_noise: the share f0 of the frame's
    power the starting variance takes (the starting amplitude takes the rest).  floor: the variance never falls below floor times
    the frame's power.  layout: 'frames' (B, length, 2) or 'planar' (B, 2, length).  differentiable: a call returns Lambda on the
    autograd graph of x with the estimate held fixed (the extras are not differentiable); False: x is detached.  A call runs on the
    device its x lies on.  Arguments are checked here, before any device work."""

    LAYOUTS, reference = LAYOUTS, "likelihood_em_reference"

    def __init__(self, length, classes=None, starts=16, iters=32, init_noise=0.02, floor=1e-6, layout: str = "frames",
                 differentiable=False):
        super().__init__(length, layout)
        self.differentiable = _flag(differentiable, "differentiable")
        table = LikelihoodClassifier(length, classes, rotations=1, layout=layout)         # the class and point handling: not restated
        self.class_names, self.descriptors, self.points = table.class_names, table.descriptors, table.points
        self._classes_c = table._classes_c
        self.angles = _start_angles(starts)
        self.starts = rotation_table(self.angles)                                         # (T, 2): the kernel's table
        self.iters = _index(iters, "iters", 0, MAX_ITERS)
        self.init_noise, self.floor = _number(init_noise, "init_noise"), _number(floor, "floor")
        if not 0.0 < self.init_noise < 1.0 or not 0.0 < np.float32(self.init_noise) < 1.0:
            raise ValueError(f"init_noise must lie inside (0, 1), got {init_noise!r}")
        if self.floor < 0.0:
            raise ValueError(f"floor must be >= 0, got {floor!r}")

    @property
    def n_classes(self):
        return len(self.descriptors)

    @property
    def n_starts(self):
        return len(self.angles)

    def struct(self, points=None, starts=None, h0=None, v0=None) -> N.LikelihoodEm:
        """The iq_likelihood_em_t of one call (`points`, `starts`, `h0`, `v0`: device addresses; h0 and v0 given: IQ_EM_GIVEN)."""
        return N.LikelihoodEm(points=points, classes=self._classes_c, n_classes=self.n_classes, starts=starts, n_starts=self.n_starts,
                              iters=self.iters, planar=self.planar, mode=int(h0 is not None), f0=self.init_noise, floor=self.floor,
                              h0=h0, v0=v0)

    def _check(self, x, h0=None, v0=None):
        self._check_shape(x)
        if (h0 is None) != (v0 is None):
            raise ValueError("pass both h0 (B, C, 2) and v0 (B, C), the start of every (frame, class), or neither")
        if h0 is not None:
            B, Cn = x.shape[0], self.n_classes
            h0 = reals(h0, "h0", (B, Cn, 2), x.device, ": one (re, im) per frame and class", pairs=True)
            v0 = reals(v0, "v0", (B, Cn), x.device, ", one value per frame and class")
        if not x.is_cuda:
            raise no_cpu(self)
        return h0, v0

    def _run(self, x, h0=None, v0=None, want_starts=False, want_pred=False):
        h0, v0 = self._check(x, h0, v0)
        return self._launch(x.detach().contiguous().float(), h0, v0, want_starts, want_pred)

    def _launch(self, x, h0, v0, want_starts, want_pred):
        B, d, Cn, T = x.shape[0], x.device, self.n_classes, 1 if h0 is not None else self.n_starts
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=d)           # noqa: E731
        loglik, h, v, best = new(B, Cn), new(B, Cn, 2), new(B, Cn), new(B, Cn, dtype=torch.int32)
        start_ll = new(B, Cn, T) if want_starts else None
        pred, snr = (new(B, dtype=torch.int32), new(B)) if want_pred else (None, None)
        if B > 0:
            points, starts = self.table_on(d, ("points", "starts"))
            par = self.struct(points.data_ptr(), starts.data_ptr(), N.ptr(h0), N.ptr(v0))
            N.check(N.lib().iq_frames_likelihood_em(x.data_ptr(), loglik.data_ptr(), h.data_ptr(), v.data_ptr(), best.data_ptr(),
                                                    N.ptr(start_ll), N.ptr(pred), N.ptr(snr), B, self.length, C.byref(par),
                                                    torch.cuda.current_stream(d).cuda_stream), "iq_frames_likelihood_em")
        return loglik, h, v, best, start_ll, pred, snr

    def _forward(self, x, h0=None, v0=None, want_starts=False):
        """_LoglikFn's forward: (Lambda, h, v, best_start, start_ll) and held = (h, v), what the backward reads."""
        loglik, h, v, best, start_ll, _, _ = self._launch(x, h0, v0, want_starts, False)
        return (loglik, h, v, best, start_ll), (h, v)

    def _backward(self, x, dloglik, h, v):
        dx = torch.empty_like(x)
        if x.shape[0] > 0:
            par = self.struct(self.table_on(x.device, "points").data_ptr())
            N.check(N.lib().iq_frames_likelihood_em_bwd(x.data_ptr(), dloglik.data_ptr(), h.data_ptr(), v.data_ptr(), dx.data_ptr(),
                                                        x.shape[0], self.length, C.byref(par),
                                                        torch.cuda.current_stream(x.device).cuda_stream), "iq_frames_likelihood_em_bwd")
        return dx

    def input_gradient(self, x, dloglik, h0=None, v0=None):
        """d <dloglik, Lambda> / d x with the estimate (h, v) of every (frame, class) held fixed: x, h0 and v0 as in a call,
        dloglik (B, C) a tensor (a class with weight 0 costs nothing, and a dead class with weight 0 leaves dx finite).  -> dx, the
        shape of x, fp32.  Two C calls (the forward for (h, v), then the backward) on the current stream, no autograd and no host
        synchronisation."""
        self._check_shape(x)
        dloglik = _dloglik(dloglik, x, self.n_classes)
        h0, v0 = self._check(x, h0, v0)
        x = x.detach().contiguous().float()
        with torch.no_grad():
            return self._backward(x, dloglik, *self._forward(x, h0, v0)[1])

    def __call__(self, x, h0=None, v0=None, return_estimates=False, return_starts=False):
        """x: device frames in this classifier's layout, fp32.  h0 (B, C, 2) (or complex (B, C)) and v0 (B, C): the start of every
        (frame, class), a single one in place of the table (a warm start from the frame before).  -> Lambda (B, C) fp32 on the
        current stream, no host synchronisation; then, with return_estimates, h (B, C, 2), v (B, C) and best_start (B, C) int32;
        then, with return_starts, every start's Lambda (B, C, T).  A (frame, class) whose every start leaves the finite, positive
        states (a class of the origin alone, a NaN sample, an all-zero frame) gets NaN (best_start -1)."""
        return_estimates, return_starts = _flag(return_estimates, "return_estimates"), _flag(return_starts, "return_starts")
        if self.differentiable:
            loglik, h, v, best, start_ll = _LoglikFn.apply(x, self, *self._check(x, h0, v0), return_starts)
        else:
            loglik, h, v, best, start_ll, _, _ = self._run(x, h0, v0, return_starts)
        return pack(loglik, *((h, v, best) if return_estimates else ()), start_ll)

    def predict(self, x):
        """-> (B,) int64: the first class with the largest Lambda, NaN classes passed over; -1 where every class is NaN."""
        return self._run(x, want_pred=True)[5].long()

    def estimate(self, x):
        """-> (pred (B,) int64, snr_db (B,), sigma2 (B,), gain (B,)) of the winning class: snr_db = 10 log10(|h|^2 / v), sigma2 = v,
        gain = |h| -- what LikelihoodClassifier(sigma2=, gain=) and CumulantClassifier(sigma2=) take.  NaN where pred is -1."""
        _, h, v, _, _, pred, snr = self._run(x, want_pred=True)
        pred = pred.long()
        at = pred.clamp(min=0)[:, None]
        nan = torch.full_like(snr, float("nan"))
        sigma2 = torch.where(pred >= 0, v.gather(1, at)[:, 0], nan)
        gain = torch.where(pred >= 0, torch.linalg.vector_norm(h.gather(1, at[..., None].expand(-1, 1, 2))[:, 0], dim=1), nan)
        return pred, snr, sigma2, gain

    def __repr__(self):
        return (f"HybridLikelihoodClassifier(length={self.length}, classes={self.class_names!r}, starts={self.n_starts}, "
                f"iters={self.iters}, init_noise={self.init_noise}, floor={self.floor}, layout={self.layout!r}"
                f"{', differentiable=True' if self.differentiable else ''})")


# ---- the host definition

def _em_pass(yre, yim, sr, si, hr, hi, v):
    """One pass of the definition in torch fp64.  yre, yim (b, n); sr, si (M,); hr, hi, v (b, T).  -> the update sums Ar, Ai, Bq, V
    (b, T) and L (b, T) = sum_n l_n, all at (h, v)."""
    pr = hr[..., None] * sr - hi[..., None] * si                               # (b, T, M)
    pi = hr[..., None] * si + hi[..., None] * sr
    dr = yre[:, None, :, None] - pr[:, :, None, :]                             # (b, T, n, M): the difference form
    di = yim[:, None, :, None] - pi[:, :, None, :]
    d = dr.mul_(dr).add_(di.mul_(di))
    dmin = d.amin(dim=3)
    q = (1.0 / v)[..., None]
    e = torch.exp(-q[..., None] * (d - dmin[..., None]))
    S = e.sum(dim=3)
    gr, gi = (e * sr).sum(dim=3) / S, (e * si).sum(dim=3) / S
    Ar = (yre[:, None] * gr + yim[:, None] * gi).sum(dim=2)
    Ai = (yim[:, None] * gr - yre[:, None] * gi).sum(dim=2)
    Bq = ((e * (sr * sr + si * si)).sum(dim=3) / S).sum(dim=2)
    V = (e.mul_(d).sum(dim=3) / S).sum(dim=2)
    L = (-q * dmin + torch.log(S / len(sr))).sum(dim=2)
    return Ar, Ai, Bq, V, L


def _alive(hr, hi, v):
    return torch.isfinite(hr) & torch.isfinite(hi) & (v >= 2.0 ** -126) & torch.isfinite(v)      # (v a normal fp32 number)


def likelihood_em_reference(x, points, classes, starts, iters=32, init_noise=0.02, floor=1e-6, h0=None, v0=None, planar=False,
                            trace=False):
    """The definition of include/iqvit.h in fp64 on the host.  x: (B, len, 2) or, planar, (B, 2, len); points: (P, 2) or complex
    (P,); classes: (offset, count) or (kind, offset, count) per class; starts: (T,) phases in radians, or the (T, 2) table of
    (cos, sin) itself; init_noise, floor: f0 and floor as the device takes them (fp32 numbers).  h0 (B, C) complex or (B, C, 2) and
    v0 (B, C): the given start, one per (frame, class), in place of the table.
    -> EmReference(loglik (B, C), h (B, C) complex, v (B, C), best_start (B, C), start_ll (B, C, T), pred (B,), snr_db (B,), trace):
    a (frame, class) whose every start dies has NaN and best_start -1, pred passes NaN classes over (-1: all are NaN, snr_db NaN).
    trace: None, or with trace=True (iters + 1, B, C, T): Lambda at the state before every pass, the last of which is start_ll."""
    y = _frames(x, planar)
    B, n = y.shape
    p = _host(points)
    p = p.astype(np.complex128).reshape(-1) if np.iscomplexobj(p) else p.astype(np.float64).reshape(-1, 2) @ np.array([1, 1j])
    descs = [tuple(int(v) for v in c) for c in classes]
    if any(len(c) == 3 and c[0] != 0 for c in descs):
        raise ValueError(f"classes must be of kind 0, got {list(classes)!r}")
    descs = [d[1:] if len(d) == 3 else d for d in descs]
    if any(len(d) != 2 or d[0] < 0 or d[1] < 1 or d[0] + d[1] > len(p) for d in descs):
        raise ValueError(f"classes must be (offset, count) ranges of the {len(p)} points, got {list(classes)!r}")
    iters = _index(iters, "iters", 0, MAX_ITERS)
    f0, floor = float(init_noise), float(floor)
    Cn = len(descs)
    M2 = np.mean(y.real ** 2 + y.imag ** 2, axis=1)                             # (not numpy.abs: its square root rounds)                                        # (B,)
    if (h0 is None) != (v0 is None):
        raise ValueError("pass both h0 and v0 or neither")
    if h0 is None:
        st = np.asarray(_host(starts), dtype=np.float64)
        st = np.cos(st) + 1j * np.sin(st) if st.ndim == 1 else st[:, 0] + 1j * st[:, 1]
        T = len(st)
        with np.errstate(invalid="ignore"):
            H0 = np.broadcast_to((np.sqrt(M2 - f0 * M2)[:, None] * st[None, :])[:, None, :], (B, Cn, T))
        V0 = np.broadcast_to((f0 * M2)[:, None, None], (B, Cn, T))
    else:
        H0 = _host(h0)
        H0 = (H0.astype(np.complex128) if np.iscomplexobj(H0) else H0.astype(np.float64) @ np.array([1, 1j])).reshape(B, Cn, 1)
        V0 = np.asarray(_host(v0), dtype=np.float64).reshape(B, Cn, 1)
        T = 1
    vfloor = torch.from_numpy(floor * M2)
    yre, yim = torch.from_numpy(y.real.copy()), torch.from_numpy(y.imag.copy())
    start_ll, H, Vv = np.empty((B, Cn, T)), np.empty((B, Cn, T), np.complex128), np.empty((B, Cn, T))
    tr = np.empty((iters + 1, B, Cn, T)) if trace else None
    nan = torch.tensor(float("nan"), dtype=torch.float64)
    for c, (off, M) in enumerate(descs):
        sr, si = torch.from_numpy(p[off:off + M].real.copy()), torch.from_numpy(p[off:off + M].imag.copy())
        step = max(1, (1 << 22) // (T * n * M))
        for b0 in range(0, B, step):
            sl = slice(b0, b0 + step)
            hr, hi = torch.from_numpy(H0[sl, c].real.copy()), torch.from_numpy(H0[sl, c].imag.copy())
            v = torch.from_numpy(V0[sl, c].copy())
            for k in range(iters + 1):
                ok = _alive(hr, hi, v)
                hr, hi, v = torch.where(ok, hr, nan), torch.where(ok, hi, nan), torch.where(ok, v, nan)      # dead: NaN from here on
                Ar, Ai, Bq, V, L = _em_pass(yre[sl], yim[sl], sr, si, hr, hi, v)
                lam = L - n * torch.log(np.pi * v)
                if trace:
                    tr[k, sl, c] = lam.numpy()
                if k < iters:
                    t = V / n
                    hr, hi, v = Ar / Bq, Ai / Bq, torch.where(t < vfloor[sl, None], vfloor[sl, None], t)
            start_ll[sl, c], H[sl, c], Vv[sl, c] = lam.numpy(), (hr + 1j * hi).numpy(), v.numpy()
    best, loglik, h, v = _over_starts(start_ll, H, Vv)
    pred, top = _first_valid_largest(loglik, 1)
    at = np.maximum(pred, 0)[:, None]
    with np.errstate(all="ignore"):
        snr = 10.0 * np.log10(np.abs(np.take_along_axis(h, at, 1)[:, 0]) ** 2 / np.take_along_axis(v, at, 1)[:, 0])
    return EmReference(loglik, h, v, best, start_ll, pred, np.where(pred >= 0, snr, np.nan), tr)


def _first_valid_largest(v, axis):
    """Index of the first largest along `axis` with NaNs passed over, and that value; (-1, NaN) where all are NaN."""
    at, best = _first_largest(np.where(np.isnan(v), -np.inf, v), axis)
    none = np.all(np.isnan(v), axis=axis)
    first = np.argmax(~np.isnan(v), axis=axis)                                 # (-inf values tie with the NaNs' stand-in: the first real one)
    at = np.where(np.isneginf(best), first, at)
    return np.where(none, -1, at), np.where(none, np.nan, best)


def _over_starts(start_ll, H, V):
    """The winning start of every (frame, class): best_start, its Lambda, h and v (NaN and -1 where every start is NaN)."""
    best, loglik = _first_valid_largest(start_ll, 2)
    at = np.maximum(best, 0)[..., None]
    h = np.where(best >= 0, np.take_along_axis(H, at, 2)[..., 0], complex(np.nan, np.nan))
    v = np.where(best >= 0, np.take_along_axis(V, at, 2)[..., 0], np.nan)
    return best, loglik, h, v
