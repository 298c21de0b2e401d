"""What the tracking equaliser's suites share (tests/test_equaliser_track_cpu.py, tests/test_gpu_equaliser_track.py): the method
restated on plain numpy, the kernels restated operation by operation in fp32, the inputs of the exact cases, the fp32 bound of
one segment step, and the faded closed-loop frames.  A plain helper module; nothing here touches the device.

The method (include/iqvit.h has the definition, vit_vs_raw_iq_amd.equaliser_track the fp64 reference): segment j covers the outputs
j hop .. j hop + seg - 1; from the same start w0 every segment takes `iters` steps w <- w - mu g_j(w), g_j[l] = sum_k h[k]
conj(z[j hop + k + c - l]) e[k], e = y (|y|^2 - R); then out[n] = sum_l w(n)[l] z[n + c - l] with w(n) interpolated linearly between
the segments' centres j hop + seg // 2 and held beyond the first and the last.  `track_plain` is that with numpy.convolve,
numpy.correlate and numpy.interp and nothing else.

THE fp32 RESTATEMENT (restate32).  Every operation of the two forward kernels in their order: the fmaf chains (fma32: the
product of two fp32 numbers is exact in fp64; the fp64 sum is formed with its TwoSum error term and, where it is inexact, moved
to the neighbour with an odd last bit -- rounding to odd -- so that the final rounding to fp32 is fmaf's single rounding, always),
the rounded products of e, lane k % 64 its k ascending, the butterfly xor 32 .. 1 on 64 lanes, thread n % 256 its n ascending for
J, the four wave sums, the fp32 division.  restate32 is therefore what the device must give bit for bit, on any finite input.

THE fp32 BOUND OF ONE SEGMENT STEP (segment_step_bound; u = 2^-24, gamma_k = k u / (1 - k u); inputs exact in fp32).  Steps 1 - 3 are
those of tests/equaliser_ref.py (y, p = |y|^2, d = p - R, e1 = y d with errors dy, dd, de1).  4. e = e1 h (one more rounding, h
exact): de = h de1 + u h (|e1| + de1).  5. G[l] = sum_k conj(z) e: a lane chains 2 ceil(seg / 64) fmaf and the butterfly adds 6
levels: D = 2 ceil(seg / 64) + 6; dG = sum_k (|Re z| + |Im z|) de + gamma_D sum_k (|Re z| + |Im z|)(|e| + de).  6. w' = fmaf(-mu,
G, w): dw = mu dG + u (|w'| + mu dG).  No division: the taper carries the normalisation.
The filter with weights over time (filter_bound_t): a word of w(n) is fl(wa + a fl(wb - wa)), within 3 u max(|wa|, |wb|) of the
definition's; with M the larger of the two neighbours' |Re| + |Im| per tap, dy[n] = gamma_{2 L + 4} sum_l M[l] (|Re z| + |Im z|)[n + c
- l].  J(out) (j_bound): the dJ of tests/equaliser_ref.py with that dy.

SEVERAL STEPS.  As tests/equaliser_ref.py: the device's weights differ from the definition's by the one-step errors and by what the
later steps make of them.  `growth` injects an error of the bound's size into the fp64 iteration at several steps and measures
what is left of it at the end; the allowance is G iters max_t ||dw_t||_2 with G pinned at twice the largest factor measured
(TRACK_GROWTH), which test_equaliser_track_cpu.py asserts on the very frames of the GPU test.
"""
import numpy as np

import equaliser_ref as E

U = E.U
gamma = E.gamma
WAVE, THREADS = 64, 256


# ---- the method on plain numpy

def n_segments(n, seg, hop):
    return (n - seg) // hop + 1


def track_plain(z, L, iters, mu, seg, hop, h, R=1.0, w0=None):
    """One frame -> (y (len,), w (S, L)).  Segment j's gradient: with e zero outside the segment, the lags of numpy.correlate as in
    equaliser_ref.gradient_plain; the weights over time: numpy.interp on each word over the centres (it holds the ends)."""
    n, c = len(z), L // 2
    S = n_segments(n, seg, hop)
    start = E.spike(1, L)[0] if w0 is None else np.array(w0, dtype=np.complex128)
    ws = np.empty((S, L), np.complex128)
    for j in range(S):
        w = start.copy()
        for _ in range(iters):
            y = E.filter_plain(z, w)
            e = np.zeros(n, np.complex128)
            sl = slice(j * hop, j * hop + seg)
            e[sl] = y[sl] * (np.abs(y[sl]) ** 2 - R) * h
            w = w - mu * np.correlate(e, z, "full")[np.arange(L) - c + n - 1]
        ws[j] = w
    centres = np.arange(S) * hop + seg // 2
    t = np.arange(n)
    wt = np.stack([np.interp(t, centres, ws[:, l].real) + 1j * np.interp(t, centres, ws[:, l].imag) for l in range(L)], axis=1)
    zp = np.pad(z, (L - 1 - c, c))
    y = np.array([np.dot(wt[i], zp[i:i + L][::-1]) for i in range(n)])
    return y, ws


# ---- the kernels in fp32

def fma32(a, b, c):
    """fmaf on fp32 arrays, correctly rounded: a b is exact in fp64; s = RN64(a b + c) with its exact error (TwoSum); an inexact s
    with an even last bit moves to its neighbour on the error's side (round to odd), and 53 >= 24 + 2 bits then make the rounding
    to fp32 the rounding of the exact value."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    p, c = np.broadcast_arrays(p, c)
    with np.errstate(all="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = (err != 0) & np.isfinite(s) & ((np.ascontiguousarray(s).view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def mul32(a, b):
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def butterfly(v):
    """(..., 64) float32 -> the wave's sum as every lane holds it after xor 32, 16, 8, 4, 2, 1."""
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(np.float32)
    return v[..., 0]


def _windows32(z, L):
    """complex (B, n) -> float32 Xr, Xi [b, n, l] = z[b, n + c - l]"""
    X = E._windows(z, L)
    return X.real.astype(np.float32), X.imag.astype(np.float32)


def _chain(Xr, Xi, wr, wi):
    """The filter chain over the last axis (l ascending) -> yr, yi float32."""
    yr = np.zeros(Xr.shape[:-1], np.float32)
    yi = np.zeros(Xr.shape[:-1], np.float32)
    for l in range(Xr.shape[-1]):
        yr = fma32(-Xi[..., l], wi[..., l], fma32(Xr[..., l], wr[..., l], yr))
        yi = fma32(Xi[..., l], wr[..., l], fma32(Xr[..., l], wi[..., l], yi))
    return yr, yi


def _j32(yr, yi, R):
    """J of (B, n) outputs in the kernels' order: thread n % 256 ascending, the butterfly, the four wave sums, / (float)len."""
    B, n = yr.shape
    d = (fma32(yi, yi, mul32(yr, yr)) - np.float32(R)).astype(np.float32)
    js = np.zeros((B, THREADS), np.float32)
    for i in range(0, n, THREADS):
        m = min(THREADS, n - i)
        js[:, :m] = fma32(d[:, i:i + m], d[:, i:i + m], js[:, :m])
    s = butterfly(js.reshape(B, 4, WAVE))
    tot = (((s[:, 0] + s[:, 1]).astype(np.float32) + s[:, 2]).astype(np.float32) + s[:, 3]).astype(np.float32)
    return (tot / np.float32(n)).astype(np.float32)


def descent32(z, w0, iters, mu, seg, hop, h, R):
    """track_descent_kernel: z complex (B, n) of fp32 numbers, w0 complex (B, L) -> wr, wi float32 (B, S, L)."""
    B, n = z.shape
    L = w0.shape[1]
    S = n_segments(n, seg, hop)
    Xr, Xi = _windows32(z, L)
    idx = (np.arange(S) * hop)[:, None] + np.arange(seg)[None, :]
    Xr, Xi = Xr[:, idx, :], Xi[:, idx, :]                                     # [b, j, k, l]
    wr = np.repeat(w0.real.astype(np.float32)[:, None, :], S, axis=1)
    wi = np.repeat(w0.imag.astype(np.float32)[:, None, :], S, axis=1)
    h = np.asarray(h, np.float32)
    mu, R = np.float32(mu), np.float32(R)
    for _ in range(iters):
        gr = np.zeros((B, S, WAVE, L), np.float32)
        gi = np.zeros((B, S, WAVE, L), np.float32)
        for k0 in range(0, seg, WAVE):
            m = min(WAVE, seg - k0)
            xr, xi = Xr[:, :, k0:k0 + m, :], Xi[:, :, k0:k0 + m, :]
            yr, yi = _chain(xr, xi, wr[:, :, None, :], wi[:, :, None, :])
            d = (fma32(yi, yi, mul32(yr, yr)) - R).astype(np.float32)
            er, ei = mul32(mul32(yr, d), h[k0:k0 + m]), mul32(mul32(yi, d), h[k0:k0 + m])
            gr[:, :, :m, :] = fma32(xi, ei[..., None], fma32(xr, er[..., None], gr[:, :, :m, :]))
            gi[:, :, :m, :] = fma32(-xi, er[..., None], fma32(xr, ei[..., None], gi[:, :, :m, :]))
        Gr, Gi = butterfly(np.moveaxis(gr, 2, 3)), butterfly(np.moveaxis(gi, 2, 3))
        wr, wi = fma32(-mu, Gr, wr), fma32(-mu, Gi, wi)
    return wr, wi


def _words_over_time32(w, n_idx, seg, hop):
    """w float32 (B, S, L), integer outputs n_idx -> float32 (B, len(n_idx), L): the kernel's segment_of and word_at."""
    S = w.shape[1]
    t = np.asarray(n_idx, np.int64) - seg // 2
    inner = (t > 0) & (t < (S - 1) * hop)
    j = np.where(inner, t // hop, np.where(t <= 0, 0, S - 1))
    a = ((t % hop).astype(np.float32) / np.float32(hop)).astype(np.float32)
    wa, wb = w[:, j, :], w[:, np.minimum(j + 1, S - 1), :]
    mid = fma32(a[None, :, None], (wb - wa).astype(np.float32), wa)
    return np.where(inner[None, :, None], mid, wa)


def filter32(z, wr, wi, seg, hop, R):
    """track_filter_kernel: -> yr, yi float32 (B, n) and J(out) float32 (B,)."""
    B, n = z.shape
    L = wr.shape[2]
    Xr, Xi = _windows32(z, L)
    t = np.arange(n)
    yr, yi = _chain(Xr, Xi, _words_over_time32(wr, t, seg, hop), _words_over_time32(wi, t, seg, hop))
    return yr, yi, _j32(yr, yi, R)


def restate32(x, L, iters, mu, seg, hop, h, R=1.0, w0=None, planar=False):
    """iq_frames_equalise_track under IQ_EQT_CMA -> (out float32 (x's shape), w float32 (B, S, L, 2), est float32 (B, 4))."""
    z = E.to_complex(np.asarray(x, np.float32), planar)
    B = len(z)
    w0c = E.spike(B, L) if w0 is None else (np.asarray(w0, np.float32)[:, :, 0].astype(np.float64) + 1j * np.asarray(w0, np.float32)[:, :, 1])
    wr, wi = descent32(z, w0c, iters, mu, seg, hop, h, R)
    yr, yi, J = filter32(z, wr, wi, seg, hop, R)
    w0r, w0i = w0c.real.astype(np.float32), w0c.imag.astype(np.float32)
    y0r, y0i = _chain(*_windows32(z, L), w0r[:, None, :], w0i[:, None, :])
    J0 = _j32(y0r, y0i, R)
    acc = np.zeros(wr.shape[:2], np.float32)
    for l in range(L):
        dr, di = (wr[:, :, l] - w0r[:, None, l]).astype(np.float32), (wi[:, :, l] - w0i[:, None, l]).astype(np.float32)
        acc = fma32(di, di, fma32(dr, dr, acc))
    best = acc[:, 0].copy()
    for j in range(1, acc.shape[1]):
        up = acc[:, j] > best
        best[up] = acc[up, j]
    est = np.stack([J0, J, best, np.full(B, wr.shape[1], np.float32)], axis=1).astype(np.float32)
    out = E.from_complex(yr.astype(np.float64) + 1j * yi.astype(np.float64), planar)
    return out, np.stack([wr, wi], axis=3), est


# ---- exact cases

def integer_segment_weights(B, S, L, seed, amp=2):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(-amp, amp + 1, (B, S, L)), rng.integers(-amp, amp + 1, (B, S, L))], axis=3).astype(np.float32)


# GIVEN, integer frames in [-3, 3] and integer weights in [-2, 2], hop a power of two: a = r / hop is a dyadic fraction, a word of
# w(n) a multiple of 1 / hop below 2 + 4 in magnitude, a term of y a multiple of 1 / hop below 18, and a sum of 4 * 32 of them stays
# far below 2^24 / hop: every partial sum is an fp32 number in any order.  (len, seg, hop, L): the edges the issue lists.
GIVEN_EXACT = [(64, 64, 64, 11), (128, 128, 32, 3),                           # len = seg: S = 1
               (95, 64, 32, 11), (96, 64, 32, 11), (97, 64, 32, 2),           # len = seg + hop - 1, seg + hop: the S edge
               (40, 8, 1, 3), (200, 8, 1, 1),                                 # hop = 1
               (130, 32, 32, 11), (20, 1, 1, 2), (256, 1, 1, 32),             # hop = seg; seg = 1 (S = len, up to 256)
               (200, 63, 16, 11), (200, 64, 16, 32), (200, 65, 16, 1),        # the lane chain's edges
               (1024, 511, 64, 11), (1025, 512, 128, 2), (1024, 512, 512, 32),
               (300, 128, 64, 11), (8192, 128, 64, 11), (8192, 512, 32, 32)]  # the defaults' shape; the largest frame, 256 segments
GIVEN_ODD_HOP = [(300, 128, 48, 11), (257, 65, 7, 32), (100, 10, 3, 1)]       # a is no dyadic fraction: under filter_bound_t


def dyadic_taper(seg):
    """A taper of small dyadic fractions with sum 1 that is no constant: (1 + (k % 3 == 0)) / 2^q scaled, the rest on entry 0."""
    q = 2.0 ** -int(np.ceil(np.log2(4 * seg)))
    h = np.where(np.arange(seg) % 3 == 0, 2.0, 1.0) * q
    h[0] += 1.0 - h.sum()
    return h.astype(np.float32)


# One and two segment steps on the frames of equaliser_ref.modulus_frames (|z|^2 = R but for `off` samples per frame: a step moves
# w a little, in the segments that hold such a sample), a dyadic taper and a dyadic mu: (len, seg, hop, L, mu, R, off, seeds, steps).  The second step rounds (its squares
# need more than 24 bits); restate32 rounds where the kernel does.
EXACT_CMA = [(64, 64, 64, 3, 0.5, 1, 8, (1, 2), 2), (128, 64, 32, 2, 0.5, 1, 16, (3, 4), 2), (200, 63, 16, 5, 0.25, 2, 24, (5,), 2),
             (200, 65, 16, 3, 0.5, 1, 24, (6, 7), 2), (130, 1, 1, 2, 0.5, 1, 40, (8,), 1), (1024, 511, 64, 11, 0.25, 1, 100, (9, 10), 1),
             (1025, 512, 128, 32, 0.5, 2, 100, (11,), 1), (300, 128, 64, 11, 0.5, 1, 30, (12, 13), 2)]


def exact_cma_case(length, seg, hop, L, mu, R, off, seeds):
    """-> x (B, len, 2) float32, h float32 (seg,)"""
    return np.concatenate([E.modulus_frames(1, length, R, off, s) for s in seeds]), dyadic_taper(seg)


# ---- the bounds

def _segment_windows(z, S, seg, hop, L):
    idx = (np.arange(S) * hop)[:, None] + np.arange(seg)[None, :]
    return E._windows(z, L)[:, idx, :], E._windows(np.abs(z.real) + np.abs(z.imag), L)[:, idx, :]     # [b, j, k, l]


def segment_step_bound(z, w, mu, R, seg, hop, h):
    """-> dw (B, S, L): the bound on either component of every segment's w' = w - mu g after one device step.  z (B, n), w (B, S, L)
    complex, h (seg,).  Steps 1 - 6 of the module docstring at the fp64 values."""
    S, L = w.shape[1], w.shape[2]
    h = np.asarray(h, np.float64)[None, None, :]
    X, Z1 = _segment_windows(z, S, seg, hop, L)
    y = np.einsum("bjkl,bjl->bjk", X, w)
    a = np.abs(w.real) + np.abs(w.imag)
    dy = gamma(2 * L) * np.einsum("bjkl,bjl->bjk", Z1, a)
    p = y.real ** 2 + y.imag ** 2
    dp0 = 2.0 * (np.abs(y.real) + np.abs(y.imag)) * dy + 2.0 * dy ** 2
    dp = dp0 + 2.0 * U * (p + dp0)
    d = p - R
    dd = dp + U * (np.abs(d) + dp)
    ymax = np.maximum(np.abs(y.real), np.abs(y.imag)) + dy
    de1 = ymax * dd + np.abs(d) * dy + U * ymax * (np.abs(d) + dd)
    e1 = np.maximum(np.abs(y.real), np.abs(y.imag)) * np.abs(d)
    de = h * de1 + U * h * (e1 + de1)
    emax = h * e1 + de
    D = 2 * -(-seg // WAVE) + 6
    dG = np.einsum("bjkl,bjk->bjl", Z1, de) + gamma(D) * np.einsum("bjkl,bjk->bjl", Z1, emax)
    G = np.einsum("bjkl,bjk->bjl", np.conj(X), y * d * h)
    w1 = w - mu * G
    return mu * dG + U * (np.maximum(np.abs(w1.real), np.abs(w1.imag)) + mu * dG)


def _neighbour_max(a, n_idx, seg, hop):
    """a (B, S, L) >= 0 -> (B, len(n_idx), L): the larger of the two segments' values between whose centres n lies."""
    S = a.shape[1]
    t = np.asarray(n_idx, np.int64) - seg // 2
    j = np.clip(t // hop, 0, S - 1)
    return np.maximum(a[:, j, :], a[:, np.minimum(j + 1, S - 1), :])


def filter_bound_t(z, w, seg, hop, adjoint=False):
    """|device - definition| of either component of out (adjoint: of dx) under the weights w (B, S, L) complex: (B, n)."""
    n, L = z.shape[1], w.shape[2]
    c = L // 2
    a = np.abs(w.real) + np.abs(w.imag)
    Z1 = E._windows(np.abs(z.real) + np.abs(z.imag), L, adjoint)
    if not adjoint:
        return gamma(2 * L + 4) * np.einsum("bnl,bnl->bn", Z1, _neighbour_max(a, np.arange(n), seg, hop))
    M = _neighbour_max(a, np.arange(-c, n + L - 1 - c), seg, hop)
    rows = np.arange(n)[:, None] + np.arange(L)[None, :]
    return gamma(2 * L + 4) * np.einsum("bml,bml->bm", Z1, M[:, rows, np.arange(L)[None, :]])


def j_bound(y, dy, R):
    """|device - definition| of J = mean (|y|^2 - R)^2 when either component of y carries dy: the dJ of equaliser_ref.one_step_bound."""
    n = y.shape[1]
    p = y.real ** 2 + y.imag ** 2
    dp0 = 2.0 * (np.abs(y.real) + np.abs(y.imag)) * dy + 2.0 * dy ** 2
    dp = dp0 + 2.0 * U * (p + dp0)
    d = p - R
    dd = dp + U * (np.abs(d) + dp)
    Dj = -(-n // THREADS) + 8
    return ((2.0 * np.abs(d) * dd + dd ** 2).sum(axis=1) + gamma(Dj) * ((np.abs(d) + dd) ** 2).sum(axis=1)) / n * (1.0 + U) + U * np.mean(d ** 2, axis=1)


def j_drift_bound_t(z, w, delta, R, seg, hop):
    """sup |J(out') - J(out)| when every segment's weights move by at most delta (B,) in ||.||_2: w'(n) is a convex combination of
    two moved neighbours (and the interpolation's own rounding is in filter_bound_t), so |y'[n] - y[n]| <= ||X[n, :]||_2 delta =: r,
    |d' - d| <= (2 |y| + r) r =: s and |d'^2 - d^2| <= (2 |d| + s) s."""
    from vit_vs_raw_iq_amd.equaliser_track import weights_over_time
    X = E._windows(z, w.shape[2])
    y = np.abs(np.einsum("bnl,bnl->bn", X, weights_over_time(w, np.arange(z.shape[1]), seg, hop)))
    r = np.sqrt((np.abs(X) ** 2).sum(axis=2)) * np.asarray(delta)[:, None]
    s = (2.0 * y + r) * r
    return np.mean((2.0 * np.abs(y ** 2 - R) + s) * s, axis=1)


def trajectory(z, w0, mu, R, iters, seg, hop, h):
    """The fp64 iteration of every segment -> [w^0 .. w^iters], each (B, S, L)."""
    from vit_vs_raw_iq_amd.equaliser_track import segment_step_reference
    S = n_segments(z.shape[1], seg, hop)
    ws = [np.repeat(w0.astype(np.complex128)[:, None, :], S, axis=1)] if w0.ndim == 2 else [w0.astype(np.complex128)]
    for _ in range(iters):
        ws.append(ws[-1] - mu * segment_step_reference(z, ws[-1], seg, hop, h, R)[1])
    return ws


def norm2(dw):
    """||.||_2 over the 2 L words of each segment: complex (B, S, L) differences or per-component bounds -> (B, S)."""
    if np.iscomplexobj(dw):
        return np.sqrt((dw.real ** 2 + dw.imag ** 2).sum(axis=2))
    return np.sqrt(2.0 * (dw ** 2).sum(axis=2))


INJECT_AT = (0, 1, 2, 4, 7, 15, 31)


def growth(z, w0, mu, R, iters, seg, hop, h, seeds=(0, 1)):
    """-> (G (B, S): the largest ||w~^T - w^T||_2 / ||p||_2 over INJECT_AT and `seeds`, w~ the fp64 iteration that leaves w^at + p at
    step `at`, ||p||_2 = step per segment; step (B, S) = max_t ||dw_t||_2 along the definition's own trajectory).  The allowance of
    `iters` device steps is G iters step."""
    ws = trajectory(z, w0, mu, R, iters, seg, hop, h)
    step = np.max([norm2(segment_step_bound(z, w, mu, R, seg, hop, h)) for w in ws[:-1]], axis=0)
    G = np.zeros_like(step)
    for at in (a for a in INJECT_AT if a < iters):
        for seed in seeds:
            rng = np.random.default_rng(seed)
            p = rng.standard_normal(ws[0].shape) + 1j * rng.standard_normal(ws[0].shape)
            p *= (step / norm2(p))[:, :, None]
            end = trajectory(z, ws[at] + p, mu, R, iters - at, seg, hop, h)[-1]
            G = np.maximum(G, norm2(end - ws[-1]) / step)
    return G, step


# The real frames of the bounded GPU tests: equaliser_ref.run_frames; (name, L, planar, seg, hop, taper kind)
BOUNDED = [("qpsk", 11, 0, 128, 64, "hann"), ("8psk", 4, 1, 65, 16, "rect"), ("qpsk_1025", 32, 0, 512, 128, "hann"), ("qpsk", 1, 1, 300, 1, "hann")]
BOUNDED_STEPS, BOUNDED_MU = 8, 0.2
# growth() on those frames from the block solution, 8 steps: the largest factor measured is 1.011 (an error keeps its size or
# shrinks: the start is the whole frame's optimum, inside the basin; 8 steps at mu = 0.2 contract little); pinned at twice that.
TRACK_GROWTH = 2.05


def bounded_start(name, L):
    """The start of the bounded runs: the block solution of the whole frame in fp64, rounded to fp32 -> float32 (B, L, 2)."""
    from vit_vs_raw_iq_amd import equaliser_reference
    return equaliser_reference(E.run_frames(name), L, 64, 0.2)[1].astype(np.float32)


# ---- the moving channel: waveform_reference -> fading_reference -> receiver_reference on the host

FADED = dict(cls="QPSK", sps=2, symbols=512, snr_db=20.0, taps=3, rice_k_db=6.0, decay=0.5, sinusoids=16, frames=16)


def faded_symbols(doppler, B=FADED["frames"], seed=5, cls=FADED["cls"], symbols=FADED["symbols"]):
    """(B, symbols, 2) float32: frames of class `cls` at sps = 2 through the channel of DESIGN.md's fading table (3 taps, Rice 6 dB,
    decay 0.5, 16 sinusoids per tap, Clarke's model drawn with numpy keyed by `seed`) at a maximum Doppler of `doppler` cycles per
    sample, white noise at 20 dB behind the channel, then receiver_reference (timing 'energy'), rounded to fp32."""
    import fading_ref as F
    from vit_vs_raw_iq_amd import Fading, Receiver, ShapedSynth, fading_reference, receiver_reference, waveform_reference
    length = FADED["sps"] * symbols
    ws = ShapedSynth([cls], snrs_db=(FADED["snr_db"],), length=length + 64, seed=seed, sps=FADED["sps"], device="cpu")
    fd = Fading(length + 64, length, taps=FADED["taps"], rice_k_db=FADED["rice_k_db"], decay=FADED["decay"], sinusoids=FADED["sinusoids"])
    rng = np.random.default_rng([seed, 77])                                  # (the same symbols and paths at every Doppler)
    sym = rng.integers(0, ws.descriptors[0][2], (B, ws.n_symbols))
    drawn = np.zeros((B, 8))
    drawn[:, 1] = FADED["snr_db"]
    drawn[:, 2] = rng.uniform(0.0, 2.0 * np.pi, B)
    drawn[:, 4] = rng.integers(0, ws.n_phase, B)
    taps = np.zeros((B, 8, 2))
    taps[:, 0, 0] = ws.los                                                    # the ShapedSynth has no channel of its own
    clean = waveform_reference(sym, drawn, taps, ws)
    paths, amps = F.tables(B)
    paths[:, :fd.taps, :fd.sinusoids + 1, 0] = rng.integers(-2 ** 31, 2 ** 31, size=(B, fd.taps, fd.sinusoids + 1))
    paths[:, :, 0, 0] = 0                                                     # the line of sight starts at phase 0
    angle = rng.random((B, fd.taps, fd.sinusoids + 1))
    paths[:, :fd.taps, :fd.sinusoids + 1, 1] = np.rint(doppler * 2.0 ** 32 * np.cos(2 * np.pi * angle)).astype(np.int64)
    for l in range(fd.taps):
        amps[:, l, 0] = fd.los[l]
        amps[:, l, 1:fd.sinusoids + 1] = np.float32(fd.tap_sigma[l] * np.sqrt(2.0 / fd.sinusoids))
    faded = fading_reference(clean, paths, amps, F.clock_of(fd.start << 32, 0, B), fd)
    sigma = np.sqrt(0.5 * 10.0 ** (-FADED["snr_db"] / 10.0))
    raw = (faded + sigma * rng.standard_normal(faded.shape)).astype(np.float32)
    rx = Receiver.for_synth(ShapedSynth([cls], snrs_db=(FADED["snr_db"],), length=length, seed=seed, sps=FADED["sps"], device="cpu"), timing="energy",
                            device="cpu")
    return receiver_reference(raw, rx.table, rx.sps, rx.timing)[0].astype(np.float32)


def nearest_point_error(out, M=4):
    """Median over frames of the mean distance of the symbols, after the best common gain and rotation of the M-th power, to the
    nearest point of unit-circle M-PSK: what the figure of merit of the host comparison in DESIGN.md is."""
    z = E.to_complex(out)
    z = z / np.sqrt(np.mean(np.abs(z) ** 2, axis=1, keepdims=True))
    rot = np.exp(-1j * (np.angle(np.mean(z ** M, axis=1, keepdims=True)) - np.pi) / M)
    zr = z * rot
    pts = np.exp(1j * (np.pi / M + 2 * np.pi * np.arange(M) / M))
    return float(np.median(np.mean(np.min(np.abs(zr[:, :, None] - pts[None, None, :]), axis=2), axis=1)))
