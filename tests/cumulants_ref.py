"""What tests/test_cumulants_cpu.py and tests/test_gpu_cumulants.py share: the general moment-to-cumulant partition formula, the
header's algebra (include/iqvit.h, iq_frames_cumulants) written ONCE over an arithmetic `A` and run on two of them -- numpy
float32 with explicit fused steps (the fp32 restatement, `F32`) and values that carry an error bound (`Bnd`) -- the integer cases
that are exact in fp32, the real cases and the decision sets.  A plain helper module like the other *_ref.py files.

THE BOUND.  u = 2^-24 is the unit roundoff of fp32.  The device follows the header operation by operation; the fp64 definition is
handed the same fp32 numbers (frames, sigma2, mu, w, bias), so only the arithmetic differs.  The bound is a running error
analysis: every quantity is a pair (v, e), v its value in fp64 and e a bound on |device - v|, and every operation of the header
maps pairs to a pair by the first-order rule of that operation plus the rounding of its own result, u |v|:

  x * y           e = |x| e_y + |y| e_x + e_x e_y + u |v|
  x + y, x - y    e = e_x + e_y + u |v|
  fmaf(x, y, z)   e = |x| e_y + |y| e_x + e_x e_y + e_z + u |v|                (one rounding)
  x / y           e = (e_x + |v| e_y) / (|y| - e_y) + u |v|                     (IEEE division)
  |x| of complex  sqrt(fmaf(im, im, re * re)):  e = sqrt(e_re^2 + e_im^2) + 3 u |v|.  The modulus moves by no more than the
                  perturbation's own modulus (the triangle inequality, which holds at |x| = 0 too, where d|x|/dx does not
                  exist); the product and the fmaf put 2 u on the sum of squares, so u on its root, the root's rounding adds u,
                  and the third u covers their second-order terms
  sum of terms    the lane's chain of ceil(len / stride) additions, the 6 of the butterfly and, on the workgroup route, the 3 of
                  the four waves: no partial sum is more than depth = ceil(len / stride) + 6 (+ 3) additions deep, so
                  e = sum_n e_n + depth u sum_n (|v_n| + e_n);   stride 64 for len <= 256, 256 above
The inputs have e = 0.  What comes out is a bound for every entry of mom, feat and score of every frame, evaluated in fp64 on the
data itself (`reference_and_bound`), times 1 + 2^-10 for the second-order terms the rules leave out (each below u times a
first-order one).  The values v follow the header's formulas in fp64, not the definition's complex arithmetic: the two differ by
fp64 rounding, 2^-29 of the bound, which the same factor covers (test_cumulants_cpu.py checks that they agree).
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
F, MOMENTS = 10, 20
WAVE_ROUTE_MAX = 256                       # the route threshold of csrc/cumulants.hip (CUM_WAVE_LEN)


def in_layout(x, planar):
    """(B, len, 2) -> the layout asked for."""
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1))) if planar else x


def to_complex(x):
    x = np.asarray(x, dtype=np.float64)
    return x[:, :, 0] + 1j * x[:, :, 1]


def depth_of(length):
    return -(-length // 64) + 6 if length <= WAVE_ROUTE_MAX else -(-length // 256) + 6 + 3


# ---- the definition of a cumulant
def set_partitions(items):
    """Every partition of the list `items` into non-empty blocks."""
    if not items:
        yield []
        return
    head, rest = items[0], items[1:]
    for part in set_partitions(rest):
        yield [[head]] + part
        for i in range(len(part)):
            yield part[:i] + [[head] + part[i]] + part[i + 1:]


def joint_cumulant(z, p, q, even_blocks_only=False):
    """The cumulant of order p of the sample z (complex (n,)) with q conjugated arguments, cum(z, ..., z, z*, ..., z*), by the
    general moment-to-cumulant formula: the sum over the set partitions pi of the p arguments of
    (-1)^(|pi| - 1) (|pi| - 1)! prod_{block} E[prod of the block's arguments], E the sample mean.  Nothing is assumed of z.
    even_blocks_only: the partitions with a block of odd size are left out, which is the formula for a variable whose moments of
    odd order vanish (one that is symmetric under z -> -z)."""
    z = np.asarray(z, dtype=np.complex128)
    args = [0] * (p - q) + [1] * q                           # 0: z, 1: conj z
    moment = functools.lru_cache(maxsize=None)(lambda a, b: complex(np.mean(z ** a * z.conj() ** b)))
    total = 0.0 + 0.0j
    for part in set_partitions(list(range(p))):
        if even_blocks_only and any(len(block) % 2 for block in part):
            continue
        term = (-1.0) ** (len(part) - 1) * math.factorial(len(part) - 1)
        for block in part:
            b = sum(args[i] for i in block)
            term = term * moment(len(block) - b, b)
        total += term
    return total


CUMULANT_ORDERS = dict(C20=(2, 0), C21=(2, 1), C40=(4, 0), C41=(4, 1), C42=(4, 2), C60=(6, 0), C61=(6, 1), C62=(6, 2), C63=(6, 3),
                       C80=(8, 0))


# ---- two arithmetics
def fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product is exact in fp64, the sum is rounded TO ODD in fp64 (53 >= 2 * 24 + 2
    bits), so the final rounding to fp32 sees what an infinitely precise sum would show it."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                          # TwoSum: p + c = s + err exactly
    with np.errstate(invalid="ignore"):
        even = (np.atleast_1d(s).view(np.int64) & 1) == 0
        fix = (err != 0) & np.isfinite(s) & even.reshape(np.shape(s))
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


class F32:
    """numpy float32, every operation rounded once."""
    @staticmethod
    def const(c, like):
        return np.full(np.shape(like), c, np.float32)

    mul = staticmethod(lambda x, y: np.multiply(x, y, dtype=np.float32))
    add = staticmethod(lambda x, y: np.add(x, y, dtype=np.float32))
    sub = staticmethod(lambda x, y: np.subtract(x, y, dtype=np.float32))
    neg = staticmethod(lambda x: np.negative(x))
    fma = staticmethod(fma32)

    @staticmethod
    def div(x, y):
        with np.errstate(all="ignore"):
            return np.divide(x, y, dtype=np.float32)

    @staticmethod
    def cabs(a):
        with np.errstate(all="ignore"):
            return np.sqrt(fma32(a[1], a[1], np.multiply(a[0], a[0], dtype=np.float32)), dtype=np.float32)


class Bnd:
    """(v, e): a value in fp64 and the bound on the device's distance from it; the rules of the module's docstring."""
    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=np.float64)

    @staticmethod
    def const(c, like):
        return Bnd(np.full(np.shape(like.v), float(c)))

    @staticmethod
    def mul(x, y):
        v = x.v * y.v
        return Bnd(v, np.abs(x.v) * y.e + np.abs(y.v) * x.e + x.e * y.e + U * np.abs(v))

    @staticmethod
    def add(x, y):
        v = x.v + y.v
        return Bnd(v, x.e + y.e + U * np.abs(v))

    @staticmethod
    def sub(x, y):
        v = x.v - y.v
        return Bnd(v, x.e + y.e + U * np.abs(v))

    @staticmethod
    def neg(x):
        return Bnd(-x.v, x.e)

    @staticmethod
    def fma(x, y, z):
        v = x.v * y.v + z.v
        return Bnd(v, np.abs(x.v) * y.e + np.abs(y.v) * x.e + x.e * y.e + z.e + U * np.abs(v))

    @staticmethod
    def div(x, y):
        with np.errstate(all="ignore"):
            v = x.v / y.v
            room = np.abs(y.v) - y.e
            e = np.where(room > 0, (x.e + np.abs(v) * y.e) / np.where(room > 0, room, 1.0), np.inf) + U * np.abs(v)
        return Bnd(v, e)

    @staticmethod
    def cabs(a):
        v = np.hypot(a[0].v, a[1].v)
        return Bnd(v, np.hypot(a[0].e, a[1].e) + 3.0 * U * v)

    @staticmethod
    def total(x, depth):
        """The sum along the last axis in the header's order."""
        return Bnd(x.v.sum(axis=-1), x.e.sum(axis=-1) + depth * U * (np.abs(x.v) + x.e).sum(axis=-1))


# ---- the header's algebra, once
def _cmul(A, a, b):
    return A.fma(a[0], b[0], A.neg(A.mul(a[1], b[1]))), A.fma(a[0], b[1], A.mul(a[1], b[0]))


def _cmulc(A, a, b):
    return A.fma(a[0], b[0], A.mul(a[1], b[1])), A.fma(a[0], b[1], A.neg(A.mul(a[1], b[0])))


def _csq(A, a):
    return A.fma(a[0], a[0], A.neg(A.mul(a[1], a[1]))), A.mul(A.add(a[0], a[0]), a[1])


def _norm2(A, a):
    return A.fma(a[1], a[1], A.mul(a[0], a[0]))


def _cabs(A, a):
    return A.cabs(a)


def _caxpy(A, s, a, b):
    return A.fma(s, a[0], b[0]), A.fma(s, a[1], b[1])


def symbol_terms(A, a, b):
    """The 17 terms of the centred symbols (a, b), in mom's order behind the mean."""
    z = (a, b)
    z2 = _csq(A, z)
    z4 = _csq(A, z2)
    z6 = _cmul(A, z4, z2)
    z8 = _csq(A, z4)
    r = _norm2(A, z)
    r2 = A.mul(r, r)
    return [z2[0], z2[1], r, z4[0], z4[1], A.mul(z2[0], r), A.mul(z2[1], r), r2, z6[0], z6[1], A.mul(z4[0], r), A.mul(z4[1], r),
            A.mul(z2[0], r2), A.mul(z2[1], r2), A.mul(r2, r), z8[0], z8[1]]


def algebra(A, m, s, sigma2):
    """m = (re, im) and the 17 moments s (sums already divided by len), each one value per frame; sigma2 one value per frame
    -> (P, the ten features), by the header's operations in the header's order."""
    k = lambda c: A.const(c, s[0])                                                        # noqa: E731
    M20, M21, M40, M41, M42 = (s[0], s[1]), s[2], (s[3], s[4]), (s[5], s[6]), s[7]
    M60, M61, M62, M63, M80 = (s[8], s[9]), (s[10], s[11]), (s[12], s[13]), s[14], (s[15], s[16])
    q = _csq(A, M20)
    n20 = _norm2(A, M20)
    C40 = _caxpy(A, k(-3), q, M40)
    C41 = _caxpy(A, A.neg(A.mul(k(3), M21)), M20, M41)
    C42 = A.fma(A.neg(A.add(M21, M21)), M21, A.sub(M42, n20))
    C60 = _caxpy(A, k(30), _cmul(A, q, M20), _caxpy(A, k(-15), _cmul(A, M20, M40), M60))
    C61 = _caxpy(A, A.mul(k(30), M21), q, _caxpy(A, k(-10), _cmul(A, M20, M41), _caxpy(A, A.neg(A.mul(k(5), M21)), M40, M61)))
    e62 = _caxpy(A, A.neg(A.mul(k(8), M21)), M41, _caxpy(A, A.neg(A.mul(k(6), M42)), M20, M62))
    v62 = _cmulc(A, M20, M40)
    g62 = A.fma(A.mul(k(24), M21), M21, A.mul(k(6), n20))
    C62 = _caxpy(A, g62, M20, (A.sub(e62[0], v62[0]), A.sub(e62[1], v62[1])))
    h63 = A.fma(M20[0], M41[0], A.mul(M20[1], M41[1]))
    C63 = A.fma(A.mul(k(18), n20), M21,
                A.fma(k(-6), h63, A.fma(A.mul(k(12), A.mul(M21, M21)), M21, A.fma(A.neg(A.mul(k(9), M21)), M42, M63))))
    C80 = _caxpy(A, k(-630), _csq(A, q), _caxpy(A, k(420), _cmul(A, q, M40), _caxpy(A, k(-35), _csq(A, M40),
                                                                                  _caxpy(A, k(-28), _cmul(A, M20, M60), M80))))
    P = A.sub(M21, sigma2)
    P2 = A.mul(P, P)
    P3 = A.mul(P2, P)
    P4 = A.mul(P3, P)
    feat = [A.div(_norm2(A, m), P), A.div(_cabs(A, M20), P), A.div(_cabs(A, C40), P2), A.div(_cabs(A, C41), P2), A.div(C42, P2),
            A.div(_cabs(A, C60), P3), A.div(_cabs(A, C61), P3), A.div(_cabs(A, C62), P3), A.div(C63, P3), A.div(_cabs(A, C80), P4)]
    return P, feat


def scores(A, feat, mu, w, bias, wrap):
    """score[b, c] of the header: feat a list of ten per-frame values, mu / w (C, 10), bias (C,) or None; wrap: number -> A's kind."""
    out = []
    for c in range(len(mu)):
        acc = A.const(0, feat[0])
        for f in range(F):
            d = A.sub(feat[f], wrap(mu[c, f], feat[0]))
            acc = A.fma(A.mul(wrap(w[c, f], feat[0]), d), d, acc)
        out.append(A.sub(wrap(0.0 if bias is None else bias[c], feat[0]), acc))
    return out


def first_largest(score):
    """(B, C) -> (B,): the first largest; a NaN is never larger nor ever beaten."""
    at, best = np.zeros(len(score), np.int64), score[:, 0].copy()
    for c in range(1, score.shape[1]):
        with np.errstate(invalid="ignore"):
            up = score[:, c] > best
        at[up], best[up] = c, score[up, c]
    return at


def _tables(mu, w, bias):
    mu = None if mu is None else np.asarray(mu, np.float32)
    return mu, None if mu is None else np.asarray(w, np.float32), None if bias is None else np.asarray(bias, np.float32)


def restate_fp32(x, sigma2=None, mu=None, w=None, bias=None):
    """The header in numpy float32 on frames whose SUMS ARE EXACT in fp32 (the integer cases: then no order of summation shows;
    asserted).  x (B, len, 2) fp32 -> dict(mom (B, 20), feat (B, 10), score (B, C) or None, pred (B,) or None), float32."""
    x = np.asarray(x, np.float32)
    B, n = x.shape[:2]
    flen = np.full(B, n, np.float32)

    def exact_sum(t):
        s = t.astype(np.float64).sum(axis=1)
        assert np.all(np.abs(s) < 2 ** 24) and np.array_equal(s, np.round(s)), "not an exact case"
        return s.astype(np.float32)
    m = (F32.div(exact_sum(x[:, :, 0]), flen), F32.div(exact_sum(x[:, :, 1]), flen))
    a, b = F32.sub(x[:, :, 0], m[0][:, None]), F32.sub(x[:, :, 1], m[1][:, None])
    s = [F32.div(exact_sum(t), flen) for t in symbol_terms(F32, a, b)]
    s2 = np.zeros(B, np.float32) if sigma2 is None else np.broadcast_to(np.asarray(sigma2, np.float32), (B,))
    P, feat = algebra(F32, m, s, s2)
    with np.errstate(invalid="ignore"):
        ok = (P > 0) & np.isfinite(P)
    feat = np.stack(feat, axis=1)
    feat[~ok] = np.nan
    out = dict(mom=np.stack([m[0], m[1]] + s + [P], axis=1), feat=feat, score=None, pred=None)
    mu, w, bias = _tables(mu, w, bias)
    if mu is not None:
        sc = scores(F32, list(feat.T), mu, w, bias, lambda v, like: np.full(like.shape, v, np.float32))
        out["score"] = np.stack(sc, axis=1) if len(mu) else np.zeros((B, 0), np.float32)
        out["pred"] = np.where(ok, first_largest(out["score"]), -1) if len(mu) else None
    return out


def reference_and_bound(x, sigma2=None, mu=None, w=None, bias=None):
    """The header's formulas in fp64 on the fp32 numbers the device is handed, and the bound derived above.  x (B, len, 2).
    -> dict(mom, feat, score: the values; Emom (B, 20), Efeat (B, 10), Escore (B, C): the bounds; pred; ok (B,): P's bound leaves
    it positive)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    B, n = x.shape[:2]
    depth = depth_of(n)
    flen = Bnd(np.full(B, float(n)))
    m = tuple(Bnd.div(Bnd.total(Bnd(x[:, :, i]), depth), flen) for i in (0, 1))
    a = Bnd.sub(Bnd(x[:, :, 0]), Bnd(m[0].v[:, None], m[0].e[:, None]))
    b = Bnd.sub(Bnd(x[:, :, 1]), Bnd(m[1].v[:, None], m[1].e[:, None]))
    s = [Bnd.div(Bnd.total(t, depth), flen) for t in symbol_terms(Bnd, a, b)]
    s2 = Bnd(np.zeros(B) if sigma2 is None else np.broadcast_to(np.asarray(sigma2, np.float32).astype(np.float64), (B,)))
    P, feat = algebra(Bnd, m, s, s2)
    cols = [m[0], m[1]] + s + [P]
    out = dict(mom=np.stack([c.v for c in cols], axis=1), Emom=SLACK * np.stack([c.e for c in cols], axis=1),
               feat=np.stack([f.v for f in feat], axis=1), Efeat=SLACK * np.stack([f.e for f in feat], axis=1),
               ok=P.v - P.e > 0, score=None, Escore=None, pred=None)
    mu, w, bias = _tables(mu, w, bias)
    if mu is not None and len(mu):
        sc = scores(Bnd, feat, mu.astype(np.float64), w.astype(np.float64), None if bias is None else bias.astype(np.float64),
                    lambda v, like: Bnd(np.full(like.v.shape, float(v))))
        out["score"] = np.stack([c.v for c in sc], axis=1)
        out["Escore"] = SLACK * np.stack([c.e for c in sc], axis=1)
        out["pred"] = first_largest(out["score"])
    return out


def gap(score):
    """Best minus second-best score per frame (inf with one class)."""
    if score.shape[1] < 2:
        return np.full(len(score), np.inf)
    s = np.sort(score, axis=1)
    return s[:, -1] - s[:, -2]


def decided(ref):
    """Frames whose decision the bound settles: the best score less its bound exceeds every other score plus its bound (so the
    device, which is within the bounds, finds the same first largest)."""
    s, e = ref["score"], ref["Escore"]
    if s.shape[1] < 2:
        return np.ones(len(s), bool)
    rows = np.arange(len(s))
    best = first_largest(s)
    hi = s + e
    hi[rows, best] = -np.inf
    return s[rows, best] - e[rows, best] > hi.max(axis=1)


# ---- integer cases, exact in fp32
EXACT_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 8191, 8192)       # (255, 256, 257: also the route threshold - 1, itself and + 1)
EXACT_BATCHES = (1, 3, 5, 65)


def exact_case(n_frames, length, seed, span=1):
    """Frames c + pattern: c one integer constant per frame in [-4, 4]^2, pattern a zero-sum pattern with components in
    {-span, ..., span} (pairs v, -v; an odd length adds the triple 1, -1 + j, -j; length 1 is the constant alone, a frame
    without variance).  The mean is c exactly, every power of z a small integer and every sum below 2^24: the sums are exact in
    fp32 in any order, and each moment is one IEEE division of an integer by len.  span = 1: |z^8| <= 16, any length up to
    8192; but then z^4 and z^8 are real (4 a b (a^2 - b^2) = 0), so three of the 17 sums stay zero.  span = 2 (length <= 2048:
    |z^8| <= 4096) exercises all 17.  -> x (B, len, 2) fp32."""
    assert span == 1 or (span == 2 and length <= 2048)
    rng = np.random.default_rng(seed)
    x = np.zeros((n_frames, length, 2), np.float32)
    for b in range(n_frames):
        pat = np.zeros((length, 2), np.float32)
        k = length // 2 if length % 2 == 0 else (length - 3) // 2
        if length >= 2:
            v = rng.integers(-span, span + 1, size=(max(k, 0), 2)).astype(np.float32)
            parts = [v, -v] + ([np.array([[1, 0], [-1, 1], [0, -1]], np.float32)] if length % 2 else [])
            pat = np.concatenate(parts)[:length]
            if not pat.any():
                pat[0], pat[1] = (1, 1), (-1, -1)                # (a frame of zeros is the isolation test's, not this one's)
            pat = pat[rng.permutation(length)]
        x[b] = pat + rng.integers(-4, 5, size=2).astype(np.float32)
    return x


def exact_tables(C, seed):
    """C classes of arbitrary fp32 numbers (the arithmetic on them is restated, not exact): mu (C, 10), w > 0, bias."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-2, 20, (C, F)).astype(np.float32), rng.uniform(0.01, 2, (C, F)).astype(np.float32),
            rng.uniform(-3, 3, C).astype(np.float32))


# ---- real cases and the decision sets
def real_frames(B, length, name, snr_db, seed):
    """B frames of `length` symbols of data.constellation(name) under one random phase each and AWGN at snr_db.
    -> x (B, len, 2) fp32, sigma2 (B,) fp32."""
    from vit_vs_raw_iq_amd import data as D
    rng = np.random.default_rng(seed)
    pts = D.constellation(name)
    s2 = 10.0 ** (-snr_db / 10.0)
    z = pts[rng.integers(0, len(pts), (B, length))] * np.exp(1j * rng.uniform(0, 2 * np.pi, (B, 1)))
    z = z + np.sqrt(s2 / 2) * (rng.standard_normal((B, length)) + 1j * rng.standard_normal((B, length)))
    return np.stack([z.real, z.imag], axis=2).astype(np.float32), np.full(B, s2, np.float32)


DECISION_LENGTH = 1024
DECISION_SHARE = 0.02                      # at most this share of a set's frames may lie within the margin


def decision_classes():
    """The table classes without 32PSK (which the features cannot tell from 16PSK: an exact tie, tested on its own)."""
    from vit_vs_raw_iq_amd import data as D
    return [c for c in D.CLASSES[:17] if c != "32PSK"]


@functools.lru_cache(maxsize=None)
def decision_set(snr_db):
    """(X (256, 1024, 2) fp32, Y (256,), sigma2 fp32 scalar) of data.make_dataset(256, seed=3, the 16 classes, one SNR, 1024
    symbols): sixteen frames per class, so that the 2 % cap is five frames and not one.  Read-only."""
    from vit_vs_raw_iq_amd import data as D
    X, Y, _ = D.make_dataset(256, seed=3, classes=decision_classes(), snrs_db=(snr_db,), n_symbols=DECISION_LENGTH)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, np.float32(10.0 ** (-snr_db / 10.0))


@functools.lru_cache(maxsize=None)
def decision_reference(snr_db, blind):
    """reference_and_bound of a decision set under CumulantClassifier(1024, the 16 classes)'s table descriptions, once per
    process."""
    from vit_vs_raw_iq_amd import CumulantClassifier
    clf = CumulantClassifier(DECISION_LENGTH, classes=decision_classes())
    X, _, s2 = decision_set(snr_db)
    return reference_and_bound(X, None if blind else s2, clf.mu, clf.w, clf.bias)
