"""Cumulant classifier on the device: the feature-based baseline of automatic modulation classification.

Beside the likelihood test (likelihood.py, the upper curve) AMC papers draw a second classical curve: higher-order cumulants in
the style of Swami & Sadler.  One HIP kernel (csrc/cumulants.hip, iq_frames_cumulants) computes, for every frame b, the mean m,
the central moments M_pq = mean(z^(p-q) conj(z)^q) of z = y - m up to order eight, the cumulants C20 C21 C40 C41 C42 C60 C61 C62
C63 C80 of the pair (z, conj z), and ten features

  f = [ |m|^2/P, |C20|/P, |C40|/P^2, |C41|/P^2, C42/P^2, |C60|/P^3, |C61|/P^3, |C62|/P^3, C63/P^3, |C80|/P^4 ],  P = C21 - sigma2,

then score[b, c] = bias[c] - sum_f w[c, f] (f_f - mu[c, f])^2 against a centroid per class, and the class of the largest.  What it
has that the likelihood test lacks: O(len) work per frame; no phase grid (the magnitudes do not see a carrier rotation); no noise
variance (Gaussian noise leaves every cumulant above order two in expectation, so sigma2 = None, the BLIND mode, lets the frame's
own power normalise); and class descriptions that can be FITTED from generated frames, so it covers GMSK and OQPSK and frames that
have been through ShapedSynth -> Receiver (-> Equaliser -> Carrier).  The first feature keeps OOK apart from BPSK, which the mean
removal would otherwise merge.  The definition with every rounding is written out in include/iqvit.h.  There is no CPU path;
`cumulants_reference` and `cumulants_reference_bwd` are the host fp64 DEFINITIONS the tests compare against.

  CumulantClassifier(length, classes, layout, differentiable)     clf(x, sigma2= | snr_db= | neither: blind) -> scores (B, C)
  clf.features(x, ...) -> (B, 10)     clf.predict(x, ...) -> (B,) int64     clf.fit(synth, frames_per_class, ...)
  clf.input_gradient(x, dscore, dfeat, ...) -> dx: d(<dscore, score> + <dfeat, feat>) / dx, one C call without autograd
  clf.indistinguishable() -> the groups of classes whose descriptions are the same numbers (16PSK and 32PSK up to order eight)
  cumulants_reference(x, sigma2, mu, w, bias) -> feat, mom, score, pred      cumulant_features_of(points) -> (10,)
  cumulants_reference_bwd(x, dscore, dfeat, sigma2, mu, w, bias) -> dx

The backward (csrc/cumulants_bwd.hip, iq_frames_cumulants_bwd) is the TRUE gradient with respect to the symbols: sigma2, mu, w and
bias are held fixed and nothing else, so it goes through the mean and through P.  It recomputes the moments from the frame by the
forward's own lines and reads no forward output.  With differentiable=True, clf(x) and clf.features(x) are on the autograd graph
of x, so that Receiver -> Equaliser -> Carrier -> classifier carries x.grad to the raw frame, and adversarial.fgsm / pgd /
robustness_curve / transfer_table take the classifier in a model's place (the eighth-order features are fragile: DESIGN.md,
"Cumulant gradients").

What it costs in accuracy is in DESIGN.md ("Cumulant classifier"): far below the likelihood test on 128-symbol frames, which is
the method's limit (an eighth-order sample cumulant of 128 symbols is mostly estimation noise), not the implementation's.

Not here: cyclic cumulants, orders above eight, decision trees over the features, an estimate of sigma2 itself, gradients with
respect to sigma2, mu, w or bias, differentiating fit().
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N
from . import data as D
from ._args import _flag, _index, _number
from .likelihood import TABLE_CLASSES, _LoglikFn, noise_for
from .stage import Stage, _first_largest, _frames, _host, _unframes, no_cpu, pack, reals
from .synth import SHAPED, FrameSynth, _points

LAYOUTS = ("frames", "planar")               # iq_cumulants_t.planar = 0: (B, length, 2), 1: (B, 2, length)
MAX_CLASSES, F, MOMENTS = 64, 10, 20         # the limit and the row lengths of iq_frames_cumulants
WAVE_ROUTE_MAX = 256                         # frames up to this length run one wave per frame, longer ones one workgroup
FEATURE_NAMES = ("|m|^2/P", "|C20|/P", "|C40|/P^2", "|C41|/P^2", "C42/P^2", "|C60|/P^3", "|C61|/P^3", "|C62|/P^3", "C63/P^3",
                 "|C80|/P^4")
MOMENT_NAMES = ("M20", "M21", "M40", "M41", "M42", "M60", "M61", "M62", "M63", "M80")
REAL_MOMENTS = ("M21", "M42", "M63")
REF = np.array([1, 1, 2, 2, 2, 16, 16, 16, 16, 272], np.float64)     # BPSK's feature magnitudes: the scale of each feature
TINY = 1e-9                                  # a table feature below this is zero (8PSK's |C40|: 1e-17 in fp64)


# ---- the host definition

def central_moments(y):
    """Complex frames (B, len) -> (m (B,), {name: (B,)}) in fp64: the mean and the ten moments of z = y - m."""
    y = np.asarray(y, dtype=np.complex128)
    m = y.mean(axis=1)
    z = y - m[:, None]
    r = (z * z.conj()).real
    z2 = z * z
    z4 = z2 * z2
    M = {"M20": z2, "M21": r, "M40": z4, "M41": z2 * r, "M42": r * r, "M60": z4 * z2, "M61": z4 * r, "M62": z2 * r * r,
         "M63": r * r * r, "M80": z4 * z4}
    return m, {k: v.mean(axis=1) for k, v in M.items()}


def cumulants_of(M):
    """The moments of central_moments -> {name: (B,)}: the cumulants of the pair (z, conj z), as closed forms of the general
    moment-to-cumulant partition formula for a zero-mean variable (tests/cumulants_ref.py has the formula itself)."""
    M20, M21, M40, M41, M42, M60, M61, M62, M63, M80 = (M[k] for k in MOMENT_NAMES)
    n20 = (M20 * M20.conj()).real
    return {
        "C20": M20, "C21": M21,
        "C40": M40 - 3 * M20 ** 2,
        "C41": M41 - 3 * M20 * M21,
        "C42": M42 - n20 - 2 * M21 ** 2,
        "C60": M60 - 15 * M20 * M40 + 30 * M20 ** 3,
        "C61": M61 - 5 * M21 * M40 - 10 * M20 * M41 + 30 * M20 ** 2 * M21,
        "C62": M62 - 6 * M20 * M42 - 8 * M21 * M41 - M20.conj() * M40 + 6 * M20 ** 2 * M20.conj() + 24 * M21 ** 2 * M20,
        "C63": M63 - 9 * M21 * M42 + 12 * M21 ** 3 - 3 * (M20 * M41.conj()).real - 3 * (M20.conj() * M41).real + 18 * n20 * M21,
        "C80": M80 - 28 * M20 * M60 - 35 * M40 ** 2 + 420 * M20 ** 2 * M40 - 630 * M20 ** 4,
    }


def cumulants_reference(x, sigma2=None, mu=None, w=None, bias=None, planar=False):
    """The definition of include/iqvit.h in fp64 on the host.  x: (B, len, 2) or, planar, (B, 2, len); sigma2: (B,), a number or
    None (0: blind); mu, w: (C, 10) or None (features only); bias: (C,) or None (0).
    -> feat (B, 10), mom (B, 20) float64 (m, the ten moments in MOMENT_NAMES' order with the complex ones as (re, im), P), and,
    with mu, score (B, C) and pred (B,) int64 (else None, None).  A frame whose P = C21 - sigma2 is not a positive finite number
    has NaN in feat and score and -1 in pred."""
    y = _frames(x, planar)
    B = y.shape[0]
    m, M = central_moments(y)
    Cu = cumulants_of(M)
    s2 = np.zeros(B) if sigma2 is None else np.broadcast_to(np.asarray(_host(sigma2), dtype=np.float64), (B,))
    P = Cu["C21"].real - s2
    with np.errstate(invalid="ignore"):
        ok = (P > 0) & np.isfinite(P)
    Ps = np.where(ok, P, 1.0)
    with np.errstate(all="ignore"):
        feat = np.stack([np.abs(m) ** 2 / Ps, np.abs(Cu["C20"]) / Ps, np.abs(Cu["C40"]) / Ps ** 2, np.abs(Cu["C41"]) / Ps ** 2,
                         Cu["C42"].real / Ps ** 2, np.abs(Cu["C60"]) / Ps ** 3, np.abs(Cu["C61"]) / Ps ** 3,
                         np.abs(Cu["C62"]) / Ps ** 3, Cu["C63"].real / Ps ** 3, np.abs(Cu["C80"]) / Ps ** 4], axis=1)
    feat[~ok] = np.nan
    cols = [m.real, m.imag]
    for k in MOMENT_NAMES:
        cols += [M[k].real] if k in REAL_MOMENTS else [M[k].real, M[k].imag]
    mom = np.stack(cols + [P], axis=1)
    if mu is None:
        if w is not None or bias is not None:
            raise ValueError("w and bias go with mu")
        return feat, mom, None, None
    mu = np.asarray(_host(mu), dtype=np.float64)
    w = np.asarray(_host(w), dtype=np.float64)
    if mu.ndim != 2 or mu.shape[1] != F or w.shape != mu.shape:
        raise ValueError(f"mu and w must be (C, {F}), got {mu.shape} and {w.shape}")
    b = np.zeros(len(mu)) if bias is None else np.asarray(_host(bias), dtype=np.float64)
    if b.shape != (len(mu),):
        raise ValueError(f"bias must be ({len(mu)},), got {b.shape}")
    with np.errstate(all="ignore"):
        score = b[None, :] - (w[None] * (feat[:, None, :] - mu[None]) ** 2).sum(axis=2)
    pred = _first_largest(score, 1)[0] if len(mu) else np.zeros(B, np.int64)
    pred[~ok] = -1
    return feat, mom, score, pred


_ORDER = np.array([1, 1, 2, 2, 2, 3, 3, 3, 3, 4], np.float64)       # the power of P under each feature
_MAGNITUDES = ((1, "C20"), (2, "C40"), (3, "C41"), (5, "C60"), (6, "C61"), (7, "C62"), (9, "C80"))     # feature f is |C| / P^k


def cumulants_reference_bwd(x, dscore=None, dfeat=None, sigma2=None, mu=None, w=None, bias=None, planar=False):
    """The definition of iq_frames_cumulants_bwd in fp64 on the host: the gradient of
    L = sum_c dscore[b, c] score[b, c] + sum_f dfeat[b, f] feat[b, f] with respect to (Re y_n, Im y_n), with sigma2, mu, w and bias
    held fixed and nothing else (the true gradient, through the mean and through P).  x, sigma2, mu, w, bias, planar as in
    cumulants_reference; dscore (B, C) and dfeat (B, 10), one of them at least.  -> dx float64, the shape of x.  A complex
    gradient is G = dL/dRe + j dL/dIm.  A class whose dscore[b, c] is exactly 0 is skipped before anything of it is read; a
    magnitude |C| that is exactly 0 passes the gradient 0; a frame whose P the forward refuses gets NaN in all of its dx."""
    if dscore is None and dfeat is None:
        raise ValueError("pass dscore, dfeat or both")
    y = _frames(x, planar)
    B, n = y.shape
    feat, mom, _, _ = cumulants_reference(x, sigma2, planar=planar)
    m, M = central_moments(y)
    Cu = cumulants_of(M)
    P = mom[:, -1]
    ok = ~np.isnan(feat[:, 0])
    gf = np.zeros((B, F)) if dfeat is None else np.array(_host(dfeat), dtype=np.float64)
    if gf.shape != (B, F):
        raise ValueError(f"dfeat must be ({B}, {F}), got {gf.shape}")
    if dscore is not None:
        if mu is None or w is None:
            raise ValueError("dscore goes with mu and w")
        ds = np.asarray(_host(dscore), dtype=np.float64)
        mu, w = np.asarray(_host(mu), dtype=np.float64), np.asarray(_host(w), dtype=np.float64)
        if mu.ndim != 2 or mu.shape[1] != F or w.shape != mu.shape or ds.shape != (B, len(mu)):
            raise ValueError(f"mu and w must be (C, {F}) and dscore ({B}, C), got {mu.shape}, {w.shape} and {ds.shape}")
        for c in range(len(mu)):
            asked = ds[:, c] != 0                                  # (a class nobody asked about: not even its NaNs are read)
            with np.errstate(invalid="ignore"):
                gf[asked] += ds[asked, c, None] * (-2.0 * w[c] * (feat[asked] - mu[c]))
    Ps = np.where(ok, P, 1.0)
    with np.errstate(all="ignore"):
        gP = -(_ORDER * feat * gf).sum(axis=1) / Ps
        gm = 2.0 * m * gf[:, 0] / Ps
        g = {"C42": gf[:, 4] / Ps ** 2, "C63": gf[:, 8] / Ps ** 3}
        for f, k in _MAGNITUDES:
            a = np.abs(Cu[k])
            g[k] = np.where(a == 0, 0.0, gf[:, f] * Cu[k] / (np.where(a == 0, 1.0, a) * Ps ** _ORDER[f]))
        M20, M21, M40, M41, M42, M60 = (M[k] for k in ("M20", "M21", "M40", "M41", "M42", "M60"))
        M21, M42 = M21.real, M42.real
        re = lambda u, v: (u.conj() * v).real                      # noqa: E731
        q, n20 = M20 * M20, (M20 * M20.conj()).real
        G = {"M80": g["C80"], "M63": g["C63"], "M62": g["C62"], "M61": g["C61"]}
        G["M60"] = g["C60"] - 28 * M20.conj() * g["C80"]
        G["M42"] = g["C42"] - 6 * re(g["C62"], M20) - 9 * M21 * g["C63"]
        G["M41"] = g["C41"] - 10 * M20.conj() * g["C61"] - 8 * M21 * g["C62"] - 6 * g["C63"] * M20
        G["M40"] = (g["C40"] - 15 * M20.conj() * g["C60"] - 5 * M21 * g["C61"] - M20 * g["C62"]
                    + (420 * q - 70 * M40).conj() * g["C80"])
        G["M21"] = (gP - 3 * re(g["C41"], M20) - 4 * M21 * g["C42"] + re(g["C61"], 30 * q - 5 * M40)
                    + re(g["C62"], 48 * M21 * M20 - 8 * M41) + g["C63"] * (18 * n20 + 36 * M21 ** 2 - 9 * M42))
        G["M20"] = (g["C20"] - 6 * M20.conj() * g["C40"] - 3 * M21 * g["C41"] - 2 * g["C42"] * M20
                    + (90 * q - 15 * M40).conj() * g["C60"] + (60 * M21 * M20 - 10 * M41).conj() * g["C61"]
                    + (24 * M21 ** 2 + 12 * n20 - 6 * M42) * g["C62"] + g["C62"].conj() * (6 * q - M40)
                    + g["C63"] * (36 * M21 * M20 - 6 * M41)
                    + (-2520 * q * M20 + 840 * M20 * M40 - 28 * M60).conj() * g["C80"])
        # moments -> symbols: M = mean(z^p conj(z)^q) gives (G conj(p z^(p-1) conj(z)^q) + conj(G) q z^p conj(z)^(q-1)) / len
        z = y - m[:, None]
        zc = z.conj()
        gn = np.zeros_like(z)
        for k, (p, qq) in zip(MOMENT_NAMES, ((2, 0), (1, 1), (4, 0), (3, 1), (2, 2), (6, 0), (5, 1), (4, 2), (3, 3), (8, 0))):
            Gk = np.asarray(G[k], dtype=np.complex128)[:, None]
            gn += Gk * (p * z ** (p - 1) * zc ** qq).conj()
            if qq:
                gn += Gk.conj() * qq * z ** p * zc ** (qq - 1)
        gn /= n
        dz = gn - gn.mean(axis=1, keepdims=True) + gm[:, None] / n
    dz[~ok] = np.nan + 1j * np.nan
    return _unframes(dz, planar)


def cumulant_features_of(points):
    """The ten features of a constellation's point table (every point equally likely, no noise), exactly, in fp64: the
    centroid of its class.  Magnitudes below 1e-9 are zero."""
    c = _points("points", points)
    f = cumulants_reference(np.stack([c.real, c.imag], axis=1)[None])[0][0]
    f[np.abs(f) < TINY] = 0.0
    return f


def _cotangent(t, what, x, width, per):
    """A gradient argument of input_gradient: a tensor (B, width), fp32 and contiguous on x's device."""
    if not isinstance(t, torch.Tensor) or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError(f"{what} must be a tensor of real numbers, got {t!r}")
    if tuple(t.shape) != (x.shape[0], width):
        raise ValueError(f"{what} must have shape {(x.shape[0], width)}: one value per frame and {per}, got {tuple(t.shape)}")
    return t.detach().to(device=x.device, dtype=torch.float32).contiguous()


class _Features:
    """clf.features as the pair likelihood._LoglikFn asks for: the same two C calls with dfeat in dscore's place."""

    def __init__(self, clf):
        self.clf = clf

    def _forward(self, x, sigma2, want_mom=False):
        feat, mom, _, _ = self.clf._launch(x, sigma2, True, want_mom, False, False)
        return (feat, mom), (sigma2,)

    def _backward(self, x, dfeat, sigma2):
        return self.clf._backward(x, None, sigma2, dfeat)


class CumulantClassifier(Stage):
    """Frames of `length` symbols at one sample per symbol -> the score of each of the classes.  classes: names data.constellation
    knows (default: its 17, in data.CLASSES' order), 'GMSK' and 'OQPSK' (no point table: they need fit()), (name, points) pairs
    or {name: points} for constellations of one's own.  layout: 'frames' (B, length, 2) or 'planar' (B, 2, length).
    differentiable: a call and features() return their result on the autograd graph of x (the extras are not differentiable);
    False: x is detached.  The class descriptions start as the table features (mu = cumulant_features_of(points), rounded to
    fp32; w[c, f] = 1 / REF[f]^2, the same for every class; bias 0) and are replaced by fit().  A call runs on the device its x lies on.  Arguments are checked
    here, before any device work."""

    LAYOUTS, reference = LAYOUTS, "cumulants_reference"

    def __init__(self, length, classes=None, layout: str = "frames", differentiable=False):
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
        self.class_names, rows = [], []
        for item in items:
            if len(item) != 2 or not isinstance(item[0], str):
                raise TypeError(f"a class is a name or a (name, points) pair, got {item!r}")
            name, pts = item
            if name in self.class_names:
                raise ValueError(f"class {name!r} is listed twice")
            if pts is None and name in SHAPED:
                row = np.full(F, np.nan)                      # until fit()
            else:
                if pts is None:
                    try:
                        pts = D.constellation(name)
                    except KeyError:
                        raise ValueError(f"unknown class {name!r}: not a name of data.constellation, 'GMSK' or 'OQPSK'") from None
                row = cumulant_features_of(_points(name, pts))
                if np.isnan(row).any():
                    raise ValueError(f"class {name!r}: the constellation has no variance about its mean, hence no features")
            self.class_names.append(name)
            rows.append(row)
        self.mu = np.stack(rows).astype(np.float32)                                           # (C, 10): the kernel's tables
        self.w = np.broadcast_to((1.0 / REF ** 2).astype(np.float32), self.mu.shape).copy()
        self.bias = np.zeros(len(rows), np.float32)
        self.fitted = None                                    # fit()'s record: dict(frames=(C,), blind, snr_db, floor)

    @property
    def n_classes(self):
        return len(self.class_names)

    def indistinguishable(self):
        """The groups (lists of names, in the classes' order) whose mu, w and bias are the same numbers: their scores tie on
        every frame and the first listed wins."""
        rows = np.concatenate([self.mu, self.w, self.bias[:, None]], axis=1)
        groups = {}
        for name, row in zip(self.class_names, rows):
            groups.setdefault(row.tobytes(), []).append(name)
        return [g for g in groups.values() if len(g) > 1]

    def tables_on(self, device):
        """(mu, w, bias) as fp32 tensors on `device`, uploaded once per device (and again after fit())."""
        return self.table_on(device, ("mu", "w", "bias"))

    def struct(self, sigma2=None, mu=None, w=None, bias=None, n_classes=None) -> N.Cumulants:
        """The iq_cumulants_t of one call (`sigma2`, `mu`, `w`, `bias`: device addresses)."""
        return N.Cumulants(planar=self.planar, sigma2=sigma2, mu=mu, w=w, bias=bias,
                           n_classes=self.n_classes if n_classes is None else n_classes)

    def _check(self, x, sigma2, snr_db, scores=True):
        self._check_shape(x)
        if sigma2 is not None and snr_db is not None:
            raise ValueError("pass the noise as sigma2= (the variance per frame) or as snr_db= (generator convention), or neither "
                             "(blind): not both")
        shape, note = (x.shape[0],), ", one value per frame"
        if snr_db is not None:
            sigma2 = noise_for(reals(snr_db, "snr_db", shape, None, note))[1]
        if sigma2 is not None:
            sigma2 = reals(sigma2, "sigma2", shape, x.device, note)
        if scores and np.isnan(self.mu).any():
            missing = [n for n, r in zip(self.class_names, self.mu) if np.isnan(r).any()]
            raise ValueError(f"classes {missing!r} have no point table: their description comes from fit()")
        if not x.is_cuda:
            raise no_cpu(self)
        return sigma2

    def _run(self, x, sigma2, snr_db, want_feat, want_mom, want_score, want_pred):
        sigma2 = self._check(x, sigma2, snr_db, want_score or want_pred)
        return self._launch(x.detach().contiguous().float(), sigma2, want_feat, want_mom, want_score, want_pred)

    def _launch(self, x, sigma2, want_feat, want_mom, want_score, want_pred):
        scores = want_score or want_pred
        B, d, Cn = x.shape[0], x.device, self.n_classes if scores else 0
        feat = torch.empty(B, F, dtype=torch.float32, device=d) if want_feat else None
        mom = torch.empty(B, MOMENTS, dtype=torch.float32, device=d) if want_mom else None
        score = torch.empty(B, Cn, dtype=torch.float32, device=d) if want_score else None
        pred = torch.empty(B, dtype=torch.int32, device=d) if want_pred else None
        if B > 0:
            mu, w, bias = self.tables_on(d) if scores else (None, None, None)
            par = self.struct(N.ptr(sigma2), N.ptr(mu), N.ptr(w), N.ptr(bias), Cn)
            N.check(N.lib().iq_frames_cumulants(x.data_ptr(), N.ptr(feat), N.ptr(mom), N.ptr(score), N.ptr(pred), B, self.length,
                                                C.byref(par), torch.cuda.current_stream(d).cuda_stream), "iq_frames_cumulants")
        return feat, mom, score, pred

    def _side(self, x, sigma2=None, snr_db=None, **other):
        """The side arguments of an attack on this classifier, checked: -> (sigma2,)."""
        if other:
            raise TypeError(f"CumulantClassifier takes the noise as sigma2= or snr_db=, or neither (blind), not {sorted(other)}: its "
                            f"features are ratios that no gain changes")
        return (self._check(x, sigma2, snr_db),)

    def _forward(self, x, sigma2, want_feat=False, want_mom=False):
        """likelihood._LoglikFn's forward: (score, the extras asked for), and held = (sigma2,): the backward recomputes the rest
        from the frame."""
        feat, mom, score, _ = self._launch(x, sigma2, want_feat, want_mom, True, False)
        return (score, feat, mom), (sigma2,)

    def _backward(self, x, dscore, sigma2, dfeat=None):
        """The one C call: x contiguous fp32, dscore (B, C) and dfeat (B, 10) contiguous fp32 or None (one of them at least)."""
        dx = torch.empty_like(x)
        if x.shape[0] > 0:
            mu, w, bias = self.tables_on(x.device) if dscore is not None else (None, None, None)
            par = self.struct(N.ptr(sigma2), N.ptr(mu), N.ptr(w), N.ptr(bias), self.n_classes if dscore is not None else 0)
            N.check(N.lib().iq_frames_cumulants_bwd(x.data_ptr(), N.ptr(dscore), N.ptr(dfeat), dx.data_ptr(), x.shape[0], self.length,
                                                    C.byref(par), torch.cuda.current_stream(x.device).cuda_stream),
                    "iq_frames_cumulants_bwd")
        return dx

    def input_gradient(self, x, dscore=None, dfeat=None, sigma2=None, snr_db=None):
        """d (<dscore, score> + <dfeat, feat>) / d x, the true gradient (through the mean and through P): x and the noise as in a
        call, dscore (B, C) and dfeat (B, 10) tensors, one of them at least (a class whose dscore is 0 costs nothing and is not
        read).  -> dx, the shape of x, fp32.  ONE C call on the current stream (the backward recomputes the moments from the
        frame), no autograd and no host synchronisation.  A frame whose P is refused gets NaN."""
        self._check_shape(x)
        if dscore is None and dfeat is None:
            raise ValueError("pass dscore (B, C), dfeat (B, 10) or both")
        dscore = None if dscore is None else _cotangent(dscore, "dscore", x, self.n_classes, "class")
        dfeat = None if dfeat is None else _cotangent(dfeat, "dfeat", x, F, "feature")
        sigma2 = self._check(x, sigma2, snr_db, dscore is not None)
        with torch.no_grad():
            return self._backward(x.detach().contiguous().float(), dscore, sigma2, dfeat)

    def __call__(self, x, sigma2=None, snr_db=None, return_features=False, return_moments=False):
        """x: device frames in this classifier's layout, fp32; the noise as sigma2 (variance E|w|^2 per frame: a number or B
        values), as snr_db (generator convention: noise_for(snr_db)) or not at all (blind: P is the frame's own variance).
        -> scores (B, C) fp32 on the current stream, no host synchronisation; then, if asked for, the features (B, 10) and the
        moments (B, 20: m, the ten moments, P).  A frame whose P is not a positive finite number gets NaN.  With
        differentiable=True the scores are on the autograd graph of x; the extras are not."""
        return_features, return_moments = _flag(return_features, "return_features"), _flag(return_moments, "return_moments")
        if self.differentiable:
            return pack(*_LoglikFn.apply(x, self, self._check(x, sigma2, snr_db), return_features, return_moments))
        feat, mom, score, _ = self._run(x, sigma2, snr_db, return_features, return_moments, True, False)
        return pack(score, feat, mom)

    def features(self, x, sigma2=None, snr_db=None, return_moments=False):
        """-> (B, 10) fp32: the features alone (a launch with no classes; works before fit()); then the moments if asked for.
        With differentiable=True the features are on the autograd graph of x."""
        return_moments = _flag(return_moments, "return_moments")
        if self.differentiable:
            return pack(*_LoglikFn.apply(x, _Features(self), self._check(x, sigma2, snr_db, False), return_moments))
        feat, mom, _, _ = self._run(x, sigma2, snr_db, True, return_moments, False, False)
        return pack(feat, mom)

    def predict(self, x, sigma2=None, snr_db=None):
        """-> (B,) int64: the first class with the largest score; -1 for a frame whose P is refused."""
        return self._run(x, sigma2, snr_db, False, False, False, True)[3].long()

    def fit(self, synth, frames_per_class, snr_db=None, blind=True, floor=1e-4, normalised=False, batch=4096, stream=0):
        """The class descriptions from generated frames (Gaussian naive Bayes): mu = the mean of each class's features,
        w = 1 / (2 (var + floor_f)), bias = -0.5 sum_f log(var + floor_f), floor_f = floor * REF[f]^2.  synth: a FrameSynth of
        this classifier's classes, length and layout (a ReceivedSynth, with its equaliser and carrier, is one); frames are made on
        the device and their features taken by the kernel, then accumulated in fp64 on the host (fitting is not a hot path).
        frames_per_class: how many frames of `stream` are generated per class and SNR of the synth.  snr_db: None, or the one SNR
        of the synth's list to fit at (frames with another label are left out).  blind: features without a noise variance;
        False: sigma2 from the frames' SNR labels by noise_for(z, normalised).  A frame with NaN features counts for nothing; a
        class that draws no frame raises.  -> self."""
        if not isinstance(synth, FrameSynth):
            raise TypeError(f"synth must be a FrameSynth, got {type(synth).__name__}")
        if list(synth.class_names) != self.class_names:
            raise ValueError(f"the synth's classes {list(synth.class_names)!r} are not the classifier's {self.class_names!r}")
        if synth.length != self.length:
            raise ValueError(f"the synth's frames have {synth.length} symbols, the classifier was built for {self.length}")
        n_per = _index(frames_per_class, "frames_per_class", 1, 2 ** 24)
        snr = None if snr_db is None else _number(snr_db, "snr_db")
        blind, normalised = _flag(blind, "blind"), _flag(normalised, "normalised")
        floor = _number(floor, "floor")
        if not floor > 0:
            raise ValueError(f"floor must be positive, got {floor!r}")
        batch = _index(batch, "batch", 1, 2 ** 20)
        if not blind and not synth.snrs_db:
            raise ValueError("blind=False needs a synth with SNR labels")
        if snr is not None and not any(abs(s - snr) <= 0.5 for s in synth.snrs_db):
            raise ValueError(f"snr_db={snr!r} is not one of the synth's {synth.snrs_db!r}")
        total = n_per * self.n_classes * max(1, len(synth.snrs_db))
        Cn = self.n_classes
        cnt, s1, s2 = np.zeros(Cn), np.zeros((Cn, F)), np.zeros((Cn, F))
        for base in range(0, total, batch):
            x, y, z = synth.generate(min(batch, total - base), base, stream)[:3]
            sig = None if blind else noise_for(z, normalised)[1]
            f = self.features(x, sigma2=sig).double().cpu().numpy()
            y, z = y.cpu().numpy(), z.cpu().numpy()
            keep = np.isfinite(f).all(axis=1) & (y >= 0) & (y < Cn)
            if snr is not None:
                keep &= np.abs(z - snr) <= 0.5
            f, y = f[keep], y[keep]
            np.add.at(cnt, y, 1.0)
            np.add.at(s1, y, f)
            np.add.at(s2, y, f * f)
        if np.any(cnt == 0):
            raise ValueError(f"classes {[n for n, k in zip(self.class_names, cnt) if k == 0]!r} drew no frame with finite features")
        mean = s1 / cnt[:, None]
        var = np.maximum(s2 / cnt[:, None] - mean * mean, 0.0) + floor * REF ** 2
        self.mu, self.w = mean.astype(np.float32), (1.0 / (2.0 * var)).astype(np.float32)
        self.bias = (-0.5 * np.log(var).sum(axis=1)).astype(np.float32)
        self.fitted = dict(frames=cnt.astype(np.int64), blind=blind, snr_db=snr, floor=floor)
        self._uploaded = {}
        return self

    noise_for = staticmethod(noise_for)

    def __repr__(self):
        return (f"CumulantClassifier(length={self.length}, classes={self.class_names!r}, layout={self.layout!r}, "
                f"fitted={self.fitted is not None}{', differentiable=True' if self.differentiable else ''})")
