"""What tests/test_cumulants_bwd_cpu.py and tests/test_gpu_cumulants_bwd.py share: the header's backward (include/iqvit.h,
iq_frames_cumulants_bwd) written ONCE over an arithmetic `A` and run on the two arithmetics of cumulants_ref.py -- numpy float32
with explicit fused steps (`F32`: the restatement the integer cases are compared with bit for bit) and values that carry an error
bound (`Bnd`) -- a torch fp64 statement of the forward for autograd, and the case generators.  A plain helper module.

THE BOUND is cumulants_ref.py's running error analysis carried on through the backward by the same first-order rules: every
quantity is a pair (v, e), every operation of the header maps pairs to a pair.  Two rules are added:

  mag(g, C, Pk)   where |C| is exactly 0 with e = 0 the device takes the same branch: (0, 0) with e = 0.  Where |C| = 0 but e > 0,
                  or |C| <= e, the division rule gives no bound (inf): the device may be on either side of the kink.  Such a
                  frame fails the condition below and is left out.
  sum g           cumulants_ref's rule for a sum, with the depth of the frame's route.

THE CONDITION.  The bound is only a check where it is small against what it bounds: on every frame the GPU suite compares,
max_n Edx <= 0.05 max_n |dx_ref| (COND).  Above it a missing term could hide.  Frames that fail it are left out, at most
DECISION_SHARE (2 %) of a set; test_cumulants_bwd_cpu.py checks on the host that the sets used stay within that cap.

The integer cases.  On cumulants_ref.exact_case frames every forward sum is exact, so the moments are one division each and the
restatement needs no order for them.  g_n is not an integer (the coefficients are quotients), so `sum g` is restated in the
header's order: the lane's symbols ascending from +0, the butterfly (xor 32 .. 1), then ((w0 + w1) + w2) + w3.
"""
import functools

import numpy as np

import cumulants_ref as R
from cumulants_ref import F32, Bnd, U, SLACK, F

COND = 0.05
ORDER = (1, 1, 2, 2, 2, 3, 3, 3, 3, 4)


# ---- the two arithmetics, with the two rules the backward adds
class F32b(F32):
    @staticmethod
    def col(v):
        return v[:, None]

    @staticmethod
    def zero_where(a, other):
        """other where a != 0, +0 where a == 0"""
        return np.where(a == 0, np.float32(0), other).astype(np.float32)

    @staticmethod
    def total(g, length):
        """The sum along the last axis in the header's order.  g (B, len) float32."""
        B = g.shape[0]
        stride = 64 if length <= R.WAVE_ROUTE_MAX else 256
        lanes = np.zeros((B, stride), np.float32)
        for n0 in range(0, length, stride):
            k = min(stride, length - n0)
            lanes[:, :k] = F32.add(lanes[:, :k], g[:, n0:n0 + k])
        w = lanes.reshape(B, stride // 64, 64)
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            w = F32.add(w, w[:, :, idx ^ o])
        w = w[:, :, 0]
        return w[:, 0] if stride == 64 else F32.add(F32.add(F32.add(w[:, 0], w[:, 1]), w[:, 2]), w[:, 3])


class Bndb(Bnd):
    @staticmethod
    def col(v):
        return Bnd(v.v[:, None], v.e[:, None])

    @staticmethod
    def zero_where(a, other):
        zero = a.v == 0
        return Bnd(np.where(zero, 0.0, other.v), np.where(zero & (a.e == 0), 0.0, np.where(zero, np.inf, other.e)))

    @staticmethod
    def total(g, length):
        return Bnd.total(g, R.depth_of(length))


# ---- the header, once
def cumulants(A, s):
    """The 17 moments -> dict of the moments, q, n and the cumulants, by the forward's operations (cumulants_ref.algebra's; the
    CPU suite asserts that the features formed from these are algebra's bit for bit)."""
    k = lambda c: A.const(c, s[0])                                                        # noqa: E731
    M20, M21, M40, M41, M42 = (s[0], s[1]), s[2], (s[3], s[4]), (s[5], s[6]), s[7]
    M60, M61, M62, M63, M80 = (s[8], s[9]), (s[10], s[11]), (s[12], s[13]), s[14], (s[15], s[16])
    q = R._csq(A, M20)
    n20 = R._norm2(A, M20)
    C40 = R._caxpy(A, k(-3), q, M40)
    C41 = R._caxpy(A, A.neg(A.mul(k(3), M21)), M20, M41)
    C42 = A.fma(A.neg(A.add(M21, M21)), M21, A.sub(M42, n20))
    C60 = R._caxpy(A, k(30), R._cmul(A, q, M20), R._caxpy(A, k(-15), R._cmul(A, M20, M40), M60))
    C61 = R._caxpy(A, A.mul(k(30), M21), q, R._caxpy(A, k(-10), R._cmul(A, M20, M41), R._caxpy(A, A.neg(A.mul(k(5), M21)), M40, M61)))
    e62 = R._caxpy(A, A.neg(A.mul(k(8), M21)), M41, R._caxpy(A, A.neg(A.mul(k(6), M42)), M20, M62))
    v62 = R._cmulc(A, M20, M40)
    g62 = A.fma(A.mul(k(24), M21), M21, A.mul(k(6), n20))
    C62 = R._caxpy(A, g62, M20, (A.sub(e62[0], v62[0]), A.sub(e62[1], v62[1])))
    h63 = A.fma(M20[0], M41[0], A.mul(M20[1], M41[1]))
    C63 = A.fma(A.mul(k(18), n20), M21,
                A.fma(k(-6), h63, A.fma(A.mul(k(12), A.mul(M21, M21)), M21, A.fma(A.neg(A.mul(k(9), M21)), M42, M63))))
    C80 = R._caxpy(A, k(-630), R._csq(A, q), R._caxpy(A, k(420), R._cmul(A, q, M40), R._caxpy(A, k(-35), R._csq(A, M40),
                                                                                       R._caxpy(A, k(-28), R._cmul(A, M20, M60), M80))))
    return dict(M20=M20, M21=M21, M40=M40, M41=M41, M42=M42, M60=M60, q=q, n=n20, C40=C40, C41=C41, C42=C42, C60=C60, C61=C61,
                C62=C62, C63=C63, C80=C80)


def _cadd(A, a, b):
    return A.add(a[0], b[0]), A.add(a[1], b[1])


def _cscale(A, s, a):
    return A.mul(s, a[0]), A.mul(s, a[1])


def _cdivr(A, a, s):
    return A.div(a[0], s), A.div(a[1], s)


def _conj(A, a):
    return a[0], A.neg(a[1])


def _dot(A, a, b):
    return A.fma(a[0], b[0], A.mul(a[1], b[1]))


def _mag(A, g, c, pk):
    a = R._cabs(A, c)
    s = A.div(g, A.mul(a, pk))
    t = _cscale(A, s, c)
    return A.zero_where(a, t[0]), A.zero_where(a, t[1])


def frame_backward(A, m, s, feat, P, gf, flen):
    """m, the 17 moments s, the ten features and P of the forward, gf the ten gfeat, flen (float)len, each one value per frame
    -> (the thirteen coefficients of the header as a dict, gm), by the header's operations in the header's order."""
    k = lambda c: A.const(c, s[0])                                                        # noqa: E731
    ax, mul, neg, fma = (lambda sc, a, b: R._caxpy(A, sc, a, b)), A.mul, A.neg, A.fma       # noqa: E731
    c = cumulants(A, s)
    M20, M21, M40, M41, M42, M60, q, n20 = (c[i] for i in ("M20", "M21", "M40", "M41", "M42", "M60", "q", "n"))
    P2 = mul(P, P)
    P3 = mul(P2, P)
    P4 = mul(P3, P)
    acc = k(0)
    for f in range(F):
        acc = fma(mul(k(ORDER[f]), feat[f]), gf[f], acc)
    gP = neg(A.div(acc, P))
    gm = _cscale(A, A.div(A.add(gf[0], gf[0]), P), m)
    gC20, gC40, gC41 = _mag(A, gf[1], M20, P), _mag(A, gf[2], c["C40"], P2), _mag(A, gf[3], c["C41"], P2)
    gC42 = A.div(gf[4], P2)
    gC60, gC61, gC62 = _mag(A, gf[5], c["C60"], P3), _mag(A, gf[6], c["C61"], P3), _mag(A, gf[7], c["C62"], P3)
    gC63 = A.div(gf[8], P3)
    gC80 = _mag(A, gf[9], c["C80"], P4)

    G60 = ax(k(-28), R._cmulc(A, M20, gC80), gC60)
    G42 = fma(k(-6), _dot(A, gC62, M20), gC42)
    G42 = fma(neg(mul(k(9), M21)), gC63, G42)
    G41 = ax(k(-10), R._cmulc(A, M20, gC61), gC41)
    G41 = ax(neg(mul(k(8), M21)), gC62, G41)
    G41 = ax(mul(k(-6), gC63), M20, G41)
    G40 = ax(k(-15), R._cmulc(A, M20, gC60), gC40)
    G40 = ax(neg(mul(k(5), M21)), gC61, G40)
    G40 = ax(k(-1), R._cmul(A, M20, gC62), G40)
    G40 = _cadd(A, G40, R._cmulc(A, ax(k(420), q, _cscale(A, k(-70), M40)), gC80))
    G21 = fma(k(-3), _dot(A, gC41, M20), gP)
    G21 = fma(neg(mul(k(4), M21)), gC42, G21)
    G21 = A.add(G21, _dot(A, gC61, ax(k(30), q, _cscale(A, k(-5), M40))))
    G21 = A.add(G21, _dot(A, gC62, ax(mul(k(48), M21), M20, _cscale(A, k(-8), M41))))
    G21 = fma(gC63, fma(k(18), n20, fma(mul(k(36), M21), M21, mul(k(-9), M42))), G21)
    G20 = ax(k(-6), R._cmulc(A, M20, gC40), gC20)
    G20 = ax(neg(mul(k(3), M21)), gC41, G20)
    G20 = ax(neg(A.add(gC42, gC42)), M20, G20)
    G20 = _cadd(A, G20, R._cmulc(A, ax(k(90), q, _cscale(A, k(-15), M40)), gC60))
    G20 = _cadd(A, G20, R._cmulc(A, ax(mul(k(60), M21), M20, _cscale(A, k(-10), M41)), gC61))
    G20 = ax(fma(mul(k(24), M21), M21, fma(k(12), n20, mul(k(-6), M42))), gC62, G20)
    G20 = _cadd(A, G20, R._cmulc(A, gC62, ax(k(6), q, (neg(M40[0]), neg(M40[1])))))
    G20 = ax(gC63, ax(mul(k(36), M21), M20, _cscale(A, k(-6), M41)), G20)
    G20 = _cadd(A, G20, R._cmulc(A, ax(k(-2520), R._cmul(A, q, M20), ax(k(840), R._cmul(A, M20, M40), _cscale(A, k(-28), M60))), gC80))

    H41, H62, H61 = _cdivr(A, G41, flen), _cdivr(A, gC62, flen), _cdivr(A, gC61, flen)
    p = dict(A20=_cscale(A, k(2), _cdivr(A, G20, flen)), A21=mul(k(2), A.div(G21, flen)), A40=_cscale(A, k(4), _cdivr(A, G40, flen)),
             A41=_cscale(A, k(3), H41), B41=_conj(A, H41), A42=mul(k(4), A.div(G42, flen)),
             A60=_cscale(A, k(6), _cdivr(A, G60, flen)), A61=_cscale(A, k(5), H61), B61=_conj(A, H61),
             A62=_cscale(A, k(4), H62), B62=_conj(A, _cscale(A, k(2), H62)), A63=mul(k(6), A.div(gC63, flen)),
             A80=_cscale(A, k(8), _cdivr(A, gC80, flen)))
    return p, gm


def symbol_g(A, p, a, b):
    """g_n of the header for the centred symbols (a, b) (B, len); p: frame_backward's coefficients, one value per frame."""
    col = lambda v: tuple(A.col(t) for t in v) if isinstance(v, tuple) else A.col(v)      # noqa: E731
    ax = lambda sc, u, v: R._caxpy(A, sc, u, v)                                           # noqa: E731
    z = (a, b)
    z2 = R._csq(A, z)
    z4 = R._csq(A, z2)
    r = R._norm2(A, z)
    r2 = A.mul(r, r)
    z3 = R._cmul(A, z2, z)
    z5 = R._cmul(A, z4, z)
    z7 = R._cmul(A, z4, z3)
    k1 = ax(r2, col(p["A62"]), ax(r, col(p["A41"]), col(p["A20"])))
    kz = A.fma(r2, col(p["A63"]), A.fma(r, col(p["A42"]), col(p["A21"])))
    k3 = ax(r, col(p["A61"]), col(p["A40"]))
    k3b = ax(r, col(p["B62"]), col(p["B41"]))
    g = R._cmulc(A, z, k1)
    g = ax(kz, z, g)
    g = _cadd(A, g, R._cmulc(A, z3, k3))
    g = _cadd(A, g, R._cmul(A, z3, k3b))
    g = _cadd(A, g, R._cmulc(A, z5, col(p["A60"])))
    g = _cadd(A, g, R._cmul(A, z5, col(p["B61"])))
    g = _cadd(A, g, R._cmulc(A, z7, col(p["A80"])))
    return g


def gfeat(A, feat, dscore, dfeat, mu, w, wrap):
    """gf[0..9] of the header.  feat: ten per-frame values; dscore (B, C) or None and dfeat (B, 10) or None: plain fp32 / fp64
    arrays (inputs: no error); mu, w (C, 10).  A class whose dscore is 0 leaves the frame's gf as it is (nothing of it is read)."""
    like = feat[0]
    gf = [wrap(0.0 if dfeat is None else dfeat[:, f], like) for f in range(F)]
    if dscore is None:
        return gf
    for c in range(dscore.shape[1]):
        asked = dscore[:, c] != 0
        if not asked.any():
            continue
        m2 = A.mul(wrap(-2.0, like), wrap(dscore[:, c], like))
        for f in range(F):
            new = A.fma(A.mul(m2, wrap(w[c, f], like)), A.sub(feat[f], wrap(mu[c, f], like)), gf[f])
            gf[f] = _select(asked, new, gf[f])
    return gf


def _select(mask, x, y):
    if isinstance(x, Bnd):
        return Bnd(np.where(mask, x.v, y.v), np.where(mask, x.e, y.e))
    return np.where(mask, x, y).astype(np.float32)


def _backward(A, x, m, s, sigma2, dscore, dfeat, mu, w, wrap, flen):
    """Everything behind the moments, shared by the two arithmetics -> (dx parts (re, im) (B, len), ok (B,))"""
    n = x.shape[1]
    P, feat = R.algebra(A, m, s, sigma2)
    Pv = P.v if isinstance(P, Bnd) else P
    with np.errstate(invalid="ignore"):
        ok = (Pv > 0) & np.isfinite(Pv)
    with np.errstate(all="ignore"):
        gf = gfeat(A, feat, dscore, dfeat, mu, w, wrap)
        p, gm = frame_backward(A, m, s, feat, P, gf, flen)
        a, b = A.sub(wrap(x[:, :, 0], None), A.col(m[0])), A.sub(wrap(x[:, :, 1], None), A.col(m[1]))
        g = symbol_g(A, p, a, b)
        out = []
        for i in (0, 1):
            c = A.sub(A.div(gm[i], flen), A.div(A.total(g[i], n), flen))
            out.append(A.add(g[i], A.col(c)))
    return out, ok


def restate_bwd_fp32(x, dscore=None, dfeat=None, sigma2=None, mu=None, w=None):
    """The header's backward in numpy float32 on frames whose forward SUMS ARE EXACT (the integer cases; asserted).  x (B, len, 2)
    fp32 -> dx (B, len, 2) float32: what the device must give bit for bit.  NaN in the frames whose P is refused."""
    x = np.asarray(x, np.float32)
    B, n = x.shape[:2]
    flen = np.full(B, n, np.float32)

    def exact_sum(t):
        s = t.astype(np.float64).sum(axis=1)
        assert np.all(np.abs(s) < 2 ** 24) and np.array_equal(s, np.round(s)), "not an exact case"
        return s.astype(np.float32)
    m = (F32.div(exact_sum(x[:, :, 0]), flen), F32.div(exact_sum(x[:, :, 1]), flen))
    a, b = F32.sub(x[:, :, 0], m[0][:, None]), F32.sub(x[:, :, 1], m[1][:, None])
    s = [F32.div(exact_sum(t), flen) for t in R.symbol_terms(F32, a, b)]
    s2 = np.zeros(B, np.float32) if sigma2 is None else np.broadcast_to(np.asarray(sigma2, np.float32), (B,))
    f32 = lambda v: None if v is None else np.asarray(v, np.float32)                      # noqa: E731

    def wrap(v, like):
        return np.asarray(v, np.float32) if like is None else np.broadcast_to(np.asarray(v, np.float32), like.shape)
    (dr, di), ok = _backward(F32b, x, m, s, s2, f32(dscore), f32(dfeat), f32(mu), f32(w), wrap, flen)
    dx = np.stack([dr, di], axis=2).astype(np.float32)
    dx[~ok] = np.nan
    return dx


def reference_and_bound_bwd(x, dscore=None, dfeat=None, sigma2=None, mu=None, w=None):
    """The header's backward in fp64 on the fp32 numbers the device is handed, and the bound.  x (B, len, 2).
    -> dict(dx (B, len, 2) fp64, Edx (B, len, 2), scale (B,) = max_n |dx| per frame (the larger part), usable (B,): P is accepted
    with its bound to spare and max Edx <= COND * scale)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    B, n = x.shape[:2]
    depth = R.depth_of(n)
    flen = Bnd(np.full(B, float(n)))
    m = tuple(Bnd.div(Bnd.total(Bnd(x[:, :, i]), depth), flen) for i in (0, 1))
    a = Bnd.sub(Bnd(x[:, :, 0]), Bndb.col(m[0]))
    b = Bnd.sub(Bnd(x[:, :, 1]), Bndb.col(m[1]))
    s = [Bnd.div(Bnd.total(t, depth), flen) for t in R.symbol_terms(Bnd, a, b)]
    s2 = Bnd(np.zeros(B) if sigma2 is None else np.broadcast_to(np.asarray(sigma2, np.float32).astype(np.float64), (B,)))
    f64 = lambda v: None if v is None else np.asarray(v, np.float32).astype(np.float64)   # noqa: E731

    def wrap(v, like):
        v = np.asarray(v, np.float64)
        return Bnd(v if like is None else np.broadcast_to(v, like.v.shape))
    (dr, di), ok = _backward(Bndb, x, m, s, s2, f64(dscore), f64(dfeat), f64(mu), f64(w), wrap, flen)
    P = R.algebra(Bnd, m, s, s2)[0]
    dx = np.stack([dr.v, di.v], axis=2)
    with np.errstate(invalid="ignore"):
        Edx = SLACK * np.stack([dr.e, di.e], axis=2)
        scale = np.abs(dx).max(axis=(1, 2))
        usable = ok & (P.v - P.e > 0) & (np.nan_to_num(Edx, nan=np.inf).max(axis=(1, 2)) <= COND * scale)
    return dict(dx=dx, Edx=Edx, scale=scale, usable=usable)


# ---- the forward, stated in torch fp64 for autograd
def torch_forward(x, sigma2=None, mu=None, w=None, bias=None):
    """x (B, len, 2) torch fp64 -> (feat (B, 10), score (B, C) or None), the formulas of cumulants.py's docstring in complex
    torch arithmetic; differentiable.  No refusal: the caller keeps to frames whose P is accepted."""
    import torch
    y = torch.complex(x[:, :, 0], x[:, :, 1])
    m = y.mean(dim=1)
    z = y - m[:, None]
    zc = z.conj()
    mom = lambda p, q: (z ** p * zc ** q).mean(dim=1)                                     # noqa: E731
    M20, M21, M40, M41, M42 = mom(2, 0), mom(1, 1).real, mom(4, 0), mom(3, 1), mom(2, 2).real
    M60, M61, M62, M63, M80 = mom(6, 0), mom(5, 1), mom(4, 2), mom(3, 3).real, mom(8, 0)
    n20 = (M20 * M20.conj()).real
    C40 = M40 - 3 * M20 ** 2
    C41 = M41 - 3 * M20 * M21
    C42 = M42 - n20 - 2 * M21 ** 2
    C60 = M60 - 15 * M20 * M40 + 30 * M20 ** 3
    C61 = M61 - 5 * M21 * M40 - 10 * M20 * M41 + 30 * M20 ** 2 * M21
    C62 = M62 - 6 * M20 * M42 - 8 * M21 * M41 - M20.conj() * M40 + 6 * M20 ** 2 * M20.conj() + 24 * M21 ** 2 * M20
    C63 = M63 - 9 * M21 * M42 + 12 * M21 ** 3 - 6 * (M20 * M41.conj()).real + 18 * n20 * M21
    C80 = M80 - 28 * M20 * M60 - 35 * M40 ** 2 + 420 * M20 ** 2 * M40 - 630 * M20 ** 4
    P = M21 - (0.0 if sigma2 is None else torch.as_tensor(sigma2, dtype=torch.float64))
    feat = torch.stack([(m * m.conj()).real / P, M20.abs() / P, C40.abs() / P ** 2, C41.abs() / P ** 2, C42 / P ** 2,
                        C60.abs() / P ** 3, C61.abs() / P ** 3, C62.abs() / P ** 3, C63 / P ** 3, C80.abs() / P ** 4], dim=1)
    if mu is None:
        return feat, None
    mu, w = torch.as_tensor(np.asarray(mu, np.float64)), torch.as_tensor(np.asarray(w, np.float64))
    b = torch.zeros(len(mu), dtype=torch.float64) if bias is None else torch.as_tensor(np.asarray(bias, np.float64))
    return feat, b[None, :] - (w[None] * (feat[:, None, :] - mu[None]) ** 2).sum(dim=2)


# ---- cases
BWD_EXACT_LENGTHS = (2, 63, 64, 65, 255, 256, 257, 1025, 8192)
BWD_EXACT_BATCHES = (1, 3, 5, 65)
EXACT_CLASSES = (0, 1, 17, 64)


def cotangents(B, C, seed, sparse=True):
    """dscore (B, C) (C = 0: None) and dfeat (B, 10), small fp32 numbers; sparse: about half of dscore's entries are exactly 0
    (the skip), and frame 0 asks about one class only."""
    rng = np.random.default_rng(seed)
    dfeat = rng.uniform(-1, 1, (B, F)).astype(np.float32)
    if C == 0:
        return None, dfeat
    ds = rng.uniform(-1, 1, (B, C)).astype(np.float32)
    if sparse:
        ds[rng.random((B, C)) < 0.5] = 0
        ds[0] = 0
        ds[0, C // 2] = 1
    return ds, dfeat


def margin_dscore(score, labels):
    """The margin loss's {-1, +1}: -1 at the label, +1 at the first largest other class.  score (B, C) numpy."""
    s = np.array(score, dtype=np.float64)
    rows = np.arange(len(s))
    s[rows, labels] = -np.inf
    other = R.first_largest(s)
    d = np.zeros(s.shape, np.float32)
    d[rows, labels] = -1
    d[rows, other] = 1
    return d


REAL_CASES = tuple((name, snr, blind) for name, snr in (("QPSK", 20), ("16QAM", 8), ("8PSK", 0)) for blind in (True, False))
REAL_LENGTHS = (200, 700)                  # one on each route, neither a multiple of the stride
REAL_BATCH = 128


@functools.lru_cache(maxsize=None)
def real_case(name, snr_db, blind, length):
    """-> (x (128, len, 2) fp32, sigma2 (128,) fp32 or None, dscore, dfeat, mu, w, bias, ref): real_frames with exact_tables' 5
    classes replaced by the table descriptions of five constellations; ref = reference_and_bound_bwd.  Read-only."""
    from vit_vs_raw_iq_amd import CumulantClassifier
    clf = CumulantClassifier(length, classes=["BPSK", "QPSK", "8PSK", "16QAM", "64QAM"])
    x, s2 = R.real_frames(REAL_BATCH, length, name, snr_db, seed=11 + length)
    s2 = None if blind else s2
    ds, df = cotangents(REAL_BATCH, 5, seed=5, sparse=True)
    ref = reference_and_bound_bwd(x, ds, df, s2, clf.mu, clf.w)
    return x, s2, ds, df, clf.mu, clf.w, clf.bias, ref


# ---- the host FGSM table of the 20 dB decision set (known sigma2, margin loss)
FGSM_EPS = 0.05
FGSM_SNR = 20


def decision_classifier(**kw):
    from vit_vs_raw_iq_amd import CumulantClassifier
    return CumulantClassifier(R.DECISION_LENGTH, classes=R.decision_classes(), **kw)


def host_accuracy(x):
    from vit_vs_raw_iq_amd import cumulants_reference
    clf = decision_classifier()
    _, Y, s2 = R.decision_set(FGSM_SNR)
    return float(np.mean(cumulants_reference(x, s2, clf.mu, clf.w, clf.bias)[3] == Y))


def random_signs(shape, seed=0):
    return np.random.default_rng(seed).choice(np.array([-1.0, 1.0], np.float32), size=shape)


@functools.lru_cache(maxsize=None)
def host_fgsm():
    """One signed step of FGSM_EPS on the margin loss in fp64, and random signs of the same size.  -> dict(g, x_adv, x_rand)."""
    from vit_vs_raw_iq_amd import cumulants_reference, cumulants_reference_bwd
    clf = decision_classifier()
    X, Y, s2 = R.decision_set(FGSM_SNR)
    score = cumulants_reference(X, s2, clf.mu, clf.w, clf.bias)[2]
    g = cumulants_reference_bwd(X, margin_dscore(score, Y), None, s2, clf.mu, clf.w, clf.bias)
    return dict(g=g, x_adv=(X + FGSM_EPS * np.sign(g)).astype(np.float32),
                x_rand=(X + FGSM_EPS * random_signs(X.shape)).astype(np.float32))
