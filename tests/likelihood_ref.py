"""What tests/test_likelihood_cpu.py and tests/test_gpu_likelihood.py share: the likelihood of one frame restated on plain numpy
(numpy.logaddexp), the integer cases that are exact in fp32, the real cases, the 20 dB decision set, and the fp32 error bound of
the device's log-likelihoods.  A plain helper module like the other *_ref.py files.

THE BOUND.  u = 2^-24 is the unit roundoff of fp32.  The device follows include/iqvit.h operation by operation; the fp64
definition is handed the same fp32 numbers (frames, points, gain, sigma2 and the (cos, sin) table), so only the arithmetic differs.
To first order in u, for one frame, class, rotation and symbol:

  scaled point    p = a s, each component one product:                        |dp| <= u a |s|
  rotation        y' = fmaf(c, Re y, s Im y), ...: one product, one fmaf:    |dy'| <= 2 u (|Re y| + |Im y|) <= 2 sqrt(2) u |y|
  difference      Re y' - Re p: the two errors above and its own rounding:    |d(dr)| <= e0 + u |dr|,  e0 = u (2 sqrt(2) |y| + a max|s|)
  distance        d = fmaf(di, di, dr dr):  2 |dr| |d(dr)| + 2 |di| |d(di)| + 2 u d,  |dr| + |di| <= sqrt(2 d):
                                                                              eps(d) = 2 sqrt(2 d) e0 + 4 u d
  minimum         the minimum of perturbed values moves by no more than eps at the minimum (d - eps(d) increases with d)
  q = 1 / sigma2  one division: relative u;   q2 = q LOG2E: the constant, q and the product: relative 3 u
  exponent        t_k = q2 (d_min - d_k): the subtraction and the product 2 u |t_k|, q2 3 u |t_k|, and the two distances, which q
                  AMPLIFIES:  ln2 |dt_k| <= q (eps(d_min) + eps(d_k)) + 5 u q (d_k - d_min)
  exp2            v_exp_f32, stated error 1 ulp = 2 u relative:  term k has relative error r_k = ln2 |dt_k| + 2 u; a term below
                  2^-126 is flushed to zero, which against S >= 1 is below 2^-126 M and is not counted
  S               the sum of M positive terms k ascending: relative sum_k e_k r_k / S + (M - 1) u
  S / M           1 / M and the product: 2 u.   Together rho = sum_k e_k r_k / S + (M + 1) u
  logarithm       v_log_f32, stated error 1 ulp, taken as 2 u max(|log2|, 1) so that a result near 0 is covered; times LN2 (the
                  constant and the product: 2 u):   rho + 4 u max(|ln(S / M)|, 1)
  l_n             fmaf(-q, d_min, .): q eps(d_min) + u q d_min from its operands and u |l_n| from its rounding
  L = sum_n l_n   the lane's chain of ceil(len / 64) additions and the 6 of the butterfly, in the header's fixed order:
                  (ceil(len / 64) + 6) u sum_n |l_n|   (not len additions: no partial sum is more than that many deep)

  E[b, c, r] = sum_n ( q eps(d_min) + u q d_min + rho + 4 u max(|ln(S / M)|, 1) + u |l_n| ) + (ceil(len / 64) + 6) u sum_n |l_n|,
  evaluated in fp64 on the data itself (`reference_and_bound`).  Over the rotations: the maximum of perturbed values moves by at most max_r E; the log of the mean of
  exponentials is 1-Lipschitz in the sup norm, and its own arithmetic adds sum_r e_r (3 u |L_r - m| + 2 u) / T + (R + 1) u +
  4 u max(|ln(T / R)|, 1) and u |loglik| for the last addition.

The bound is multiplied by 1 + 2^-10 for the second-order terms, which are below u times the first-order ones.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
QUARTER_TURNS = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], np.float32)           # (cos, sin) of 0, 90, 180, 270 degrees


def to_complex(x, planar=False):
    x = np.asarray(x, dtype=np.float64)
    return (x[:, 0, :] + 1j * x[:, 1, :]) if planar else (x[:, :, 0] + 1j * x[:, :, 1])


def from_complex(z, planar=False, dtype=np.float32):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=1 if planar else 2), dtype=dtype)


def in_layout(x, planar):
    """(B, len, 2) -> the layout asked for."""
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1))) if planar else x


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- the direct statement
def loglik_plain(y, sigma2, a, pts, theta):
    """sum_n log( (1 / M) sum_k exp(-|y_n e^{-j theta} - a s_k|^2 / sigma2) ) of ONE frame (complex y (n,)), one class (complex
    pts (M,)) and one rotation, with numpy.logaddexp over k and nothing taken out first."""
    yr = np.asarray(y) * np.exp(-1j * theta)
    e = -np.abs(yr[:, None] - a * np.asarray(pts)[None, :]) ** 2 / sigma2
    return float(np.sum(np.logaddexp.reduce(e, axis=1) - np.log(len(pts))))


def logmeanexp_plain(v):
    return float(np.logaddexp.reduce(np.asarray(v, dtype=np.float64)) - np.log(len(v)))


# ---- the fp64 definition with the bound, in one pass
def reference_and_bound(x, sigma2, gain, points, classes, rot, mode, planar=False):
    """The definition on the fp32 numbers the device is handed, in fp64 (torch on the host), and the bound derived above.
    points (P, 2), classes (offset, count), rot the (R, 2) table.  -> dict(loglik (B, C), L (B, C, R), best_rot, pred,
    E (B, C, R): the bound on |L_device - L|, Ell (B, C): the bound on |loglik_device - loglik|)."""
    y = to_complex(x, planar)
    B, n = y.shape
    s2 = np.broadcast_to(np.asarray(sigma2, np.float64), (B,))
    a = np.ones(B) if gain is None else np.broadcast_to(np.asarray(gain, np.float64), (B,))
    p = np.asarray(points, np.float64).reshape(-1, 2)
    rot = np.asarray(rot, np.float64).reshape(-1, 2)
    w = rot[:, 0] - 1j * rot[:, 1]
    R, Cn = len(w), len(classes)
    q = torch.from_numpy(1.0 / s2)
    yr = y[:, None, :] * w[None, :, None]
    yre, yim = torch.from_numpy(yr.real.copy()), torch.from_numpy(yr.imag.copy())
    ymod = torch.from_numpy(np.abs(y))[:, None, :]                                      # (B, 1, n)
    L, E = np.empty((B, Cn, R)), np.empty((B, Cn, R))
    depth = -(-n // 64) + 6
    for c, (off, M) in enumerate(classes):
        pc = p[off:off + M]
        smax = float(np.sqrt((pc ** 2).sum(axis=1)).max())
        step = max(1, (1 << 21) // (R * n * M))
        for b0 in range(0, B, step):
            sl = slice(b0, b0 + step)
            at = torch.from_numpy(a[sl].copy())
            dr = yre[sl, :, :, None] - (at[:, None] * torch.from_numpy(pc[:, 0].copy())[None, :])[:, None, None, :]
            di = yim[sl, :, :, None] - (at[:, None] * torch.from_numpy(pc[:, 1].copy())[None, :])[:, None, None, :]
            d = dr * dr + di * di                                                       # (b, R, n, M)
            dmin = d.amin(dim=3)
            qq = q[sl, None, None]
            e0 = U * (2.0 * np.sqrt(2.0) * ymod[sl] + at[:, None, None].abs() * smax)   # (b, 1, n)
            eps = lambda v, e: 2.0 * torch.sqrt(2.0 * v) * e + 4.0 * U * v              # noqa: E731
            gap = d - dmin[..., None]
            ek = torch.exp(-qq[..., None] * gap)
            S = ek.sum(dim=3)
            rk = qq[..., None] * (eps(dmin, e0)[..., None] + eps(d, e0[..., None])) + 5.0 * U * qq[..., None] * gap + 2.0 * U
            rho = (ek * rk).sum(dim=3) / S + (M + 1) * U
            lg = torch.log(S / M)
            ln = -qq * dmin + lg
            En = qq * eps(dmin, e0) + U * qq * dmin + rho + 4.0 * U * torch.clamp(lg.abs(), min=1.0) + U * ln.abs()
            L[sl, c] = ln.sum(dim=2).numpy()
            E[sl, c] = (En.sum(dim=2) + depth * U * ln.abs().sum(dim=2)).numpy()
    E *= SLACK
    best_rot = np.zeros((B, Cn), np.int64)
    m = L[:, :, 0].copy()
    for r in range(1, R):
        up = L[:, :, r] > m
        best_rot[up], m[up] = r, L[:, :, r][up]
    return dict(L=L, best_rot=best_rot, E=E, **_over_rotations(L, E, mode))


def margin(loglik):
    """Best minus second-best class per frame (inf with one class)."""
    if loglik.shape[1] < 2:
        return np.full(len(loglik), np.inf)
    s = np.sort(loglik, axis=1)
    return s[:, -1] - s[:, -2]


# ---- integer cases, exact in fp32
EXACT_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1025, 8192)
# four classes: one point, 2 copies, 8 copies, one point (the origin: every rotation ties and the first must win)
EXACT_POINTS = np.array([[1, 2]] + [[-2, 1]] * 2 + [[3, -1]] * 8 + [[0, 0]], np.float32)
EXACT_CLASSES = [(0, 1), (1, 2), (3, 8), (11, 1)]


def exact_case(n_frames, length, seed):
    """Integer frames in [-4, 4], sigma2 a power of two in [1/4, 4], gain in {1, 2, 3, 1/2}: every distance is a multiple of
    1/4 below 2 * 13.5^2, every exponential exp2(0) = 1, every S a power of two and S / M = 1, every l_n = -q d_min a multiple of
    1/16 below 2^11, and every partial sum of up to 8192 of them below 2^24 sixteenths: nothing rounds, in fp32 or in fp64."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, size=(n_frames, length, 2)).astype(np.float32)
    sigma2 = (2.0 ** rng.integers(-2, 3, size=n_frames)).astype(np.float32)
    gain = rng.choice(np.array([1.0, 2.0, 3.0, 0.5], np.float32), size=n_frames)
    return x, sigma2, gain


# ---- real cases
def real_frames(B, length, name_or_points, snr_db, seed, gain=1.0):
    """B frames of `length` symbols of a constellation (a data.constellation name or complex points, scaled to unit power) under
    one random phase each and AWGN at snr_db, times `gain`.  -> x (B, len, 2) fp32, sigma2 (B,) fp32 (of the frame as emitted)."""
    from vit_vs_raw_iq_amd import data as D
    rng = np.random.default_rng(seed)
    pts = D.constellation(name_or_points) if isinstance(name_or_points, str) else np.asarray(name_or_points, np.complex128)
    pts = pts / np.sqrt(np.mean(np.abs(pts) ** 2))
    s2 = 10.0 ** (-snr_db / 10.0)
    z = pts[rng.integers(0, len(pts), (B, length))] * np.exp(1j * rng.uniform(0, 2 * np.pi, (B, 1)))
    z = z + np.sqrt(s2 / 2) * (rng.standard_normal((B, length)) + 1j * rng.standard_normal((B, length)))
    return from_complex(gain * z), np.full(B, gain * gain * s2, np.float32)


def random_table(M, seed):
    """M complex points at unit mean power -> (M, 2) fp32."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    c = c / np.sqrt(np.mean(np.abs(c) ** 2)) if M > 1 else c / np.abs(c)
    return np.stack([c.real, c.imag], axis=1).astype(np.float32)


# ---- the decision set: 68 frames of the 17 table classes at 20 dB, 128 symbols
DECISION_SNR_DB = 20.0


@functools.lru_cache(maxsize=None)
def decision_set():
    """(X (68, 128, 2) fp32, Y (68,), sigma2 fp32 scalar) of data.make_dataset(68, seed=3, classes=CLASSES[:17], snrs_db=(20,),
    n_symbols=128).  Read-only."""
    from vit_vs_raw_iq_amd import data as D
    X, Y, Z = D.make_dataset(68, seed=3, classes=D.CLASSES[:17], snrs_db=(DECISION_SNR_DB,), n_symbols=128)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, np.float32(10.0 ** (-DECISION_SNR_DB / 10.0))


@functools.lru_cache(maxsize=None)
def decision_reference(mode):
    """reference_and_bound of the decision set under LikelihoodClassifier(128)'s tables, computed once per process."""
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    clf = LikelihoodClassifier(128, mode=mode)
    X, _, s2 = decision_set()
    if mode == "mean":                                   # L and E do not depend on the mode: one pass serves both
        base = decision_reference("max")
        return {**base, **_over_rotations(base["L"], base["E"], "mean")}
    return reference_and_bound(X, s2, None, clf.points, [d[1:] for d in clf.descriptors], clf.rot, mode)


def _over_rotations(L, E, mode):
    """loglik, its bound Ell and pred of `mode` from a finished table L and its bound E."""
    B, Cn, R = L.shape
    m = L.max(axis=2)
    if mode == "max":
        loglik, Ell = m, E.max(axis=2)
    else:
        er = np.exp(L - m[..., None])
        T = er.sum(axis=2)
        lt = np.log(T / R)
        loglik = m + lt
        own = (er * (3.0 * U * np.abs(L - m[..., None]) + 2.0 * U)).sum(axis=2) / T + (R + 1) * U + 4.0 * U * np.maximum(np.abs(lt), 1.0)
        Ell = E.max(axis=2) + SLACK * (own + U * np.abs(loglik))
    pred = np.zeros(B, np.int64)
    top = loglik[:, 0].copy()
    for c in range(1, Cn):
        up = loglik[:, c] > top
        pred[up], top[up] = c, loglik[up, c]
    return dict(loglik=loglik, Ell=Ell, pred=pred)


def rotation_ties(L, E):
    """ties[b, c, r]: rotation r is within the two bounds of the largest -- the device may take it for the maximum.  A
    constellation with a k-fold symmetry has k equal maxima in exact arithmetic; only rounding orders them."""
    m = L.max(axis=2, keepdims=True)
    at = np.take_along_axis(E, L.argmax(axis=2)[..., None], axis=2)
    return L + E >= m - at
