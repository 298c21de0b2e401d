"""What the equaliser's suites share (tests/test_equaliser_cpu.py, tests/test_gpu_equaliser.py): the method restated on plain
numpy, the inputs of the exact cases with the check that makes them exact, the fp32 bound of one step, and the closed-loop
frames.  A plain helper module; nothing here touches the device.

The method (block constant-modulus descent; include/iqvit.h has the definition, vit_vs_raw_iq_amd.equaliser the fp64 reference):
    y = w * z                       y[n] = sum_l w[l] z[n + c - l], c = L // 2, z zero outside the frame
    e = y (|y|^2 - R)
    g[l] = mean_n conj(z[n + c - l]) e[n]
    w <- w - mu g                   `iters` times from the unit spike at c; then out = y
`cma_plain` below is that, written with numpy.convolve / numpy.correlate and nothing else.

THE fp32 BOUND OF ONE STEP (one_step_bound; u = 2^-24, gamma_k = k u / (1 - k u), inputs z, w, mu, R exact in fp32).
  1. y: each component is an fmaf chain of 2 L terms:  dy[n] = gamma_{2L} Y[n],  Y[n] = sum_l (|Re w_l| + |Im w_l|)
     (|Re z| + |Im z|)[n + c - l]  (an upper bound of either component's sum of |terms|).
  2. p = |y|^2 as fmaf(Im, Im, Re * Re): the operands carry dy, the product and the fmaf round once each:
     dp = 2 (|Re y| + |Im y|) dy + 2 dy^2 + 2 u (p + dp0), dp0 the first two terms.   d = p - R:  dd = dp + u (|d| + dp).
  3. e = y d, the cubic:  de_c = (|y_c| + dy) dd + |d| dy + u (|y_c| + dy)(|d| + dd)  for c = Re, Im.
  4. G[l] = sum_n conj(z) e: per component 2 terms per n; a thread chains 2 ceil(len / 256) fmaf, the butterfly adds 6 levels,
     the wave sums 2 more: depth D = 2 ceil(len / 256) + 8.  dG = sum_n (|Re z| + |Im z|) max(de_re, de_im) [the operands' error]
     + gamma_D sum_n (|Re z| + |Im z|)(max(|e_re|, |e_im|) + max de) [the sum's].
  5. g = G / len (one rounding), w' = fmaf(-mu, g, w) (one rounding):  dg = dG / len + u (|G| + dG) / len,  dw = mu dg + u |w'|.
Nothing is fitted: every term is the standard forward error of the operation it stands for.
J = (sum_n d^2) / len likewise: dJ = [sum_n (2 |d| dd + dd^2) + gamma_{D'} sum_n (|d| + dd)^2] / len (1 + u) + u J, D' = D / 2 + 4.

A WHOLE RUN.  The device's w^T differs from the reference's by the one-step errors delta_t the steps add and by what the later
steps make of them.  If the step map does not expand a perturbation of that size (||.||_2 over the 2 L words; checked on the
host in test_equaliser_cpu.py on the very frames and steps of the GPU test: growth_to_the_end), then ||w_dev^T - w_ref^T||_2 <= sum_t ||delta_t||_2
<= T max_t ||dw_t||_2, dw_t the bound above along the reference's own trajectory: `run_bound`.  Where it does expand (the
closed-loop frames), the same sum holds with every term scaled by G, the largest factor by which the fp64 iteration has grown
an error of that size by the end of the run (`growth`; G is asserted on the host), and J(after) follows the weights through
its gradient: |J(w_dev) - J(w_ref)| <= 4 delta sup ||g||_2 over the ball of radius delta = G T max_t ||dw_t||_2
(`j_drift_bound`), plus the bound of evaluating J once.
"""
import numpy as np

U = 2.0 ** -24
THREADS = 256


def gamma(k):
    return k * U / (1.0 - k * U)


def to_complex(x, planar=False):
    x = np.asarray(x, dtype=np.float64)
    return (x[:, 0, :] + 1j * x[:, 1, :]) if planar else (x[:, :, 0] + 1j * x[:, :, 1])


def from_complex(z, planar=False, dtype=np.float32):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=1 if planar else 2), dtype=dtype)


def weights(w):
    """complex (B, L) -> float32 (B, L, 2)"""
    return np.ascontiguousarray(np.stack([w.real, w.imag], axis=2), dtype=np.float32)


def spike(B, L):
    w = np.zeros((B, L), np.complex128)
    w[:, L // 2] = 1.0
    return w


# ---- the method on plain numpy

def filter_plain(z, w):
    """y[n] = sum_l w[l] z[n + c - l] for one frame, by numpy.convolve: full[k] = sum_l w[l] z[k - l], so y[n] = full[n + c]."""
    c = len(w) // 2
    return np.convolve(z, w)[c:c + len(z)]


def gradient_plain(z, w, R):
    """-> g, J of one frame.  g[l] = mean_n conj(z[n + c - l]) e[n]: numpy.correlate(e, z, 'full')[k] = sum_n e[n + k - (len - 1)]
    conj(z[n]), i.e. lag s = k - (len - 1) holds sum_m e[m] conj(z[m - s]); g[l] is the lag s = l - c."""
    L, n = len(w), len(z)
    y = filter_plain(z, w)
    d = np.abs(y) ** 2 - R
    full = np.correlate(y * d, z, "full")
    return full[np.arange(L) - L // 2 + n - 1] / n, float(np.mean(d ** 2))


def cma_plain(z, L, iters, mu, R=1.0, w0=None):
    """-> y, w, [J(w^0) .. J(w^iters)] of one frame."""
    w = spike(1, L)[0] if w0 is None else np.array(w0, dtype=np.complex128)
    Js = []
    for _ in range(iters):
        g, J = gradient_plain(z, w, R)
        Js.append(J)
        w = w - mu * g
    Js.append(gradient_plain(z, w, R)[1])
    return filter_plain(z, w), w, Js


def residual_isi(w, h):
    """1 - the largest |.|^2 of the combined response w * h over its energy: 0 for a perfect equaliser."""
    p = np.abs(np.convolve(w, h)) ** 2
    return float(1.0 - p.max() / p.sum())


# ---- exact cases

def integer_frames(B, length, seed, amp=3, planar=False):
    rng = np.random.default_rng(seed)
    return from_complex(rng.integers(-amp, amp + 1, (B, length)) + 1j * rng.integers(-amp, amp + 1, (B, length)), planar)


def integer_weights(B, L, seed, amp=2):
    rng = np.random.default_rng(seed)
    return weights(rng.integers(-amp, amp + 1, (B, L)) + 1j * rng.integers(-amp, amp + 1, (B, L)))


def modulus_frames(B, length, R, off, seed):
    """Integer frames on which a step of the descent moves only a little: every sample has |z|^2 = R (R = 1: {1, j, -1, -j};
    R = 2: {+-1 +- j}), so that e = 0 there under the unit spike, but for `off` samples per frame that do not."""
    rng = np.random.default_rng(seed)
    alphabet = np.array([1, 1j, -1, -1j]) if R == 1 else np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j])
    z = alphabet[rng.integers(0, 4, (B, length))]
    other = np.array([0, 1 + 1j, 2, 1 - 1j, -2j]) if R == 1 else np.array([0, 1, 1j, 2, -1])
    for b in range(B):
        pos = rng.choice(length, off, replace=False)
        z[b, pos] = other[rng.integers(0, len(other), off)]
    return from_complex(z)


# (len, L, mu / len, R, off, seeds of modulus_frames (one frame each), steps that are exact): found by search with exact_run_ok
# and `moves`; test_equaliser_cpu.py checks every one again.  The squares and the cubic of a step multiply the number of
# fraction bits of w, which is why two exact steps need mu / len >= 1 / 4 and short filters.
EXACT_CMA = [(8, 2, 0.5, 1, 1, (1, 2, 4), 2), (8, 3, 0.5, 1, 1, (1, 2, 4), 2), (8, 5, 0.5, 1, 1, (7, 16, 17), 2),
             (8, 2, 0.25, 2, 1, (36,), 2), (16, 3, 0.5, 1, 1, (2, 3, 6), 2), (64, 3, 0.5, 1, 2, (1, 25, 35), 2),
             (512, 3, 0.5, 1, 2, (24, 37), 2), (1024, 2, 0.5, 1, 2, (10, 36), 2),
             (1024, 11, 0.25, 2, 3, (2, 4, 9), 1), (1024, 32, 0.5, 1, 3, (2, 5, 9), 1), (2048, 11, 0.5, 2, 2, (0, 1, 4), 1)]


def exact_cma_case(length, L, ratio, R, off, seeds):
    """-> (x (B, len, 2) float32, mu)"""
    return np.concatenate([modulus_frames(1, length, R, off, s) for s in seeds]), ratio * length


def moves(x, L, mu, R, iters):
    """Every step of every frame changes w."""
    ws = trajectory(to_complex(x), spike(len(x), L), mu, float(R), iters)
    return all(bool(np.all(np.any(b != a, axis=1))) for a, b in zip(ws, ws[1:]))


def _quantum(v):
    """The largest power of two that divides every entry of v (fp64 dyadics); 1 when all are zero."""
    v = np.abs(np.asarray(v, dtype=np.float64).ravel())
    v = v[v != 0]
    if v.size == 0:
        return 1.0
    m, e = np.frexp(v)
    k = (m * 2.0 ** 53).astype(np.int64)
    return float(np.min(np.ldexp((k & -k).astype(np.float64), e - 53)))


def _sums_exact(terms, axis):
    """Every partial sum of `terms` along `axis`, in any order, is an fp32 number: the terms are multiples of q and the sum of
    their magnitudes stays below 2^24 q."""
    t = np.concatenate([terms.real, terms.imag], axis=axis) if np.iscomplexobj(terms) else terms
    return bool(np.all(np.abs(t).sum(axis=axis) < 2.0 ** 24 * _quantum(t)))


def _windows(z, L, adjoint=False):
    c = L // 2
    if adjoint:
        return np.lib.stride_tricks.sliding_window_view(np.pad(z, ((0, 0), (c, L - 1 - c))), L, axis=1)   # z[b, n - c + l]
    zp = np.pad(z, ((0, 0), (L - 1 - c, c)))
    return np.lib.stride_tricks.sliding_window_view(zp, L, axis=1)[:, :, ::-1]            # [b, n, l] = z[b, n + c - l]


def exact_run_ok(x, w0, mu, R, iters):
    """_exact_frame_ok of every frame (the grid q of a sum is a frame's own)."""
    return all(_exact_frame_ok(x[b:b + 1], w0[b:b + 1], mu, R, iters) for b in range(len(x)))


def _exact_frame_ok(x, w0, mu, R, iters):
    """True when `iters` steps and the final filter are exact in fp32 on these inputs whatever the order of the sums: every
    product is an fp32 number and every sum passes _sums_exact (then fp64, used here, is exact too).  x (B, len, 2), w0
    complex (B, L); len and mu must be powers of two."""
    z = to_complex(x)
    B, n = z.shape
    L = w0.shape[1]
    if n & (n - 1) or np.frexp(mu)[0] != 0.5:
        return False
    X = _windows(z, L)
    w = w0.astype(np.complex128)
    for t in range(iters + 1):
        parts = np.stack([X.real * w.real[:, None, :], -X.imag * w.imag[:, None, :], X.real * w.imag[:, None, :],
                          X.imag * w.real[:, None, :]], axis=-1).reshape(B, n, -1)
        y = np.einsum("bnl,bl->bn", X, w)
        sq = np.stack([y.real ** 2, y.imag ** 2, np.full(y.shape, -float(R))], axis=-1)
        d = y.real ** 2 + y.imag ** 2 - R
        e = y * d
        ok = _sums_exact(parts, 2) and _sums_exact(sq, 2) and _sums_exact(np.stack([e.real, e.imag]), 0) \
            and _sums_exact((d ** 2)[:, :], 1)
        if not ok:
            return False
        if t == iters:
            break
        gparts = np.stack([X.real * e.real[:, :, None], X.imag * e.imag[:, :, None], X.real * e.imag[:, :, None],
                           -X.imag * e.real[:, :, None]], axis=-1)                         # [b, n, l, 4]
        if not _sums_exact(gparts.transpose(0, 2, 1, 3).reshape(B, L, -1), 2):
            return False
        g = np.einsum("bnl,bn->bl", np.conj(X), e) / n
        step = np.stack([w.real, w.imag, -mu * g.real, -mu * g.imag], axis=-1)             # w - mu g: pairs (w_c, -mu g_c)
        if not (_sums_exact(step[..., [0, 2]], 2) and _sums_exact(step[..., [1, 3]], 2)):
            return False
        w = w - mu * g
    p = np.stack([w.real ** 2, w.imag ** 2], axis=-1).reshape(B, -1)
    return _sums_exact(p, 1)


# ---- the bounds

def filter_bound(z, w, adjoint=False):
    """|device - definition| of either component of y = w * z: gamma_{2L} Y[n]  (step 1 above).  z (B, len), w (B, L) complex.
    adjoint: of dx[m] = sum_l conj(w[l]) dout[m - c + l], the same chain over the other window."""
    L = w.shape[1]
    a = np.abs(w.real) + np.abs(w.imag)
    return gamma(2 * L) * np.einsum("bnl,bl->bn", _windows(np.abs(z.real) + np.abs(z.imag), L, adjoint), a)


def one_step_bound(z, w, mu, R):
    """-> (dw (B, L): the bound on either component of w' = w - mu g after one device step, dJ (B,): on J(w)).  Steps 1 - 5 of
    the module docstring, evaluated at the fp64 values."""
    B, n = z.shape
    L = w.shape[1]
    X = _windows(z, L)
    y = np.einsum("bnl,bl->bn", X, w)
    dy = filter_bound(z, w)
    p = y.real ** 2 + y.imag ** 2
    dp0 = 2.0 * (np.abs(y.real) + np.abs(y.imag)) * dy + 2.0 * dy ** 2
    dp = dp0 + 2.0 * U * (p + dp0)
    d = p - R
    dd = dp + U * (np.abs(d) + dp)
    e = y * d
    ymax = np.maximum(np.abs(y.real), np.abs(y.imag)) + dy
    de = ymax * dd + np.abs(d) * dy + U * ymax * (np.abs(d) + dd)
    emax = np.maximum(np.abs(e.real), np.abs(e.imag)) + de
    D = 2 * -(-n // THREADS) + 8
    Z1 = _windows(np.abs(z.real) + np.abs(z.imag), L)                                       # [b, n, l]
    dG = np.einsum("bnl,bn->bl", Z1, de) + gamma(D) * np.einsum("bnl,bn->bl", Z1, emax)
    G = np.einsum("bnl,bn->bl", np.conj(X), e)
    Gmax = np.maximum(np.abs(G.real), np.abs(G.imag))
    dg = dG / n + U * (Gmax + dG) / n
    w1 = w - mu * G / n
    dw = mu * dg + U * (np.maximum(np.abs(w1.real), np.abs(w1.imag)) + mu * dg)
    Dj = D // 2 + 4
    J = np.mean(d ** 2, axis=1)
    dJ = ((2.0 * np.abs(d) * dd + dd ** 2).sum(axis=1) + gamma(Dj) * ((np.abs(d) + dd) ** 2).sum(axis=1)) / n * (1.0 + U) + U * J
    return dw, dJ


def trajectory(z, w0, mu, R, iters):
    """The fp64 iteration -> [w^0 .. w^iters]."""
    ws = [w0.astype(np.complex128)]
    X = _windows(z, w0.shape[1])
    for _ in range(iters):
        w = ws[-1]
        y = np.einsum("bnl,bl->bn", X, w)
        e = y * (y.real ** 2 + y.imag ** 2 - R)
        ws.append(w - mu * np.einsum("bnl,bn->bl", np.conj(X), e) / z.shape[1])
    return ws


def norm2(dw):
    """||.||_2 over the 2 L words of a complex (B, L) difference, or of a per-component bound (B, L) (both components at it)."""
    if np.iscomplexobj(dw):
        return np.sqrt((dw.real ** 2 + dw.imag ** 2).sum(axis=1))
    return np.sqrt(2.0 * (dw ** 2).sum(axis=1))


def run_bound(z, w0, mu, R, iters):
    """-> (the allowed ||w_dev - w_ref||_2 per frame after `iters` steps: iters * max_t ||dw_t||_2, and max_t ||dw_t||_2)."""
    ws = trajectory(z, w0, mu, R, iters)
    step = np.max([norm2(one_step_bound(z, w, mu, R)[0]) for w in ws[:-1]], axis=0) if iters else np.zeros(len(z))
    return iters * step, step


# ---- the frames of the bounded cases: M-PSK through a mild random channel, 25 dB, unit power, rounded to fp32

RUNS = {"qpsk": (4, 300, 12), "8psk": (8, 300, 12), "qpsk_1025": (4, 1025, 4)}         # name -> (M, len, frames)
INJECT_AT = (0, 1, 2, 4, 8, 16, 32, 48, 63)


def run_frames(name, strength=0.2, snr_db=25.0):
    """(B, len, 2) float32: symbols e^{j (pi / M + 2 pi k / M)} through h = (1, s g1, 0.7 s g2, 0.5 s g3), g complex normal, turned
    by a random phase, plus noise; the spike start then lies in the basin where the step map does not expand (checked, not
    assumed: test_equaliser_cpu.py)."""
    M, n, B = RUNS[name]
    rng = np.random.default_rng([M, n])
    a = np.exp(1j * (np.pi / M + 2 * np.pi / M * rng.integers(0, M, (B, n + 4))))
    h = np.concatenate([np.ones((B, 1)), strength * (rng.standard_normal((B, 3)) + 1j * rng.standard_normal((B, 3))) * [1, 0.7, 0.5]],
                       axis=1)
    z = np.stack([np.convolve(a[b], h[b])[2:2 + n] for b in range(B)]) * np.exp(1j * rng.uniform(0, 2 * np.pi, (B, 1)))
    z = z + np.sqrt(0.5 * 10 ** (-snr_db / 10)) * (rng.standard_normal(z.shape) + 1j * rng.standard_normal(z.shape))
    return from_complex(z / np.sqrt(np.mean(np.abs(z) ** 2, axis=1, keepdims=True)))


def growth_to_the_end(z, w0, mu, R, iters, size, at, seeds=(0, 1, 2)):
    """The largest ||w~^T - w^T||_2 / ||p||_2 per frame over `seeds`, w~ the iteration that leaves w^at + p (||p||_2 = size, a
    random direction) at step `at`: what the run makes, by its end, of an error of that size committed at that step."""
    ws = trajectory(z, w0, mu, R, iters)
    worst = np.zeros(len(z))
    for seed in seeds:
        rng = np.random.default_rng(seed)
        p = rng.standard_normal(w0.shape) + 1j * rng.standard_normal(w0.shape)
        p *= (np.asarray(size) / norm2(p))[:, None]
        end = trajectory(z, ws[at] + p, mu, R, iters - at)[-1]
        worst = np.maximum(worst, norm2(end - ws[-1]) / norm2(p))
    return worst


def growth(z, w0, mu, R, iters):
    """-> (G (B,): max(1, the largest growth_to_the_end over INJECT_AT) for errors of the one-step bound's size, the allowed
    ||w_dev - w_ref||_2 = G * iters * max_t ||dw_t||_2, and max_t ||dw_t||_2).  Where the step map does expand, an error
    committed at step t arrives at the end at most G times as large, and there are `iters` of them."""
    allowed, step = run_bound(z, w0, mu, R, iters)
    G = np.maximum(1.0, np.max([growth_to_the_end(z, w0, mu, R, iters, step, at) for at in INJECT_AT if at < iters], axis=0))
    return G, G * allowed, step


def j_drift_bound(z, w, delta, R):
    """sup |J(w') - J(w)| over ||w' - w||_2 <= delta (B,), per frame: J(w') - J(w) is the line integral of the real gradient,
    whose 2-norm is 4 ||g||_2, so it is at most 4 delta sup ||g||_2.  On the ball |y'[n] - y[n]| <= ||X[n, :]||_2 delta =: r[n]
    (Cauchy-Schwarz), so |y'| lies in [max(|y| - r, 0), |y| + r], ||y'|^2 - R| is largest at an end of that interval, and
    |g'[l]| <= mean_n |z[n + c - l]| |y'|max |d'|max.  Nothing cancels in this bound: it is a worst case over signs."""
    B, n = z.shape
    L = w.shape[1]
    X = _windows(z, L)
    y = np.abs(np.einsum("bnl,bl->bn", X, w))
    r = np.sqrt((np.abs(X) ** 2).sum(axis=2)) * np.asarray(delta)[:, None]
    hi, lo = y + r, np.maximum(y - r, 0.0)
    dmax = np.maximum(np.abs(hi ** 2 - R), np.abs(lo ** 2 - R))
    gsup = np.einsum("bnl,bn->bl", np.abs(X), hi * dmax) / n
    return 4.0 * np.asarray(delta) * np.sqrt((gsup ** 2).sum(axis=1))


# ---- the closed loop: ShapedSynth-like frames made on the host, keyed by (class, seed)

CLOSED = dict(classes=("BPSK", "QPSK", "8PSK"), sps=2, taps=4, snr_db=20.0, length=1024, frames=24)
# On these frames the spike lies outside the basin in which the step map contracts: an error of the one-step bound's size
# committed at an early step arrives at the end of the 64 steps up to 5.57 (BPSK), 4.57 (QPSK), 1.12 (8PSK) times as large (fp64,
# growth()).  The caps asserted for them in test_equaliser_cpu.py, by which test_gpu_equaliser.py scales its allowances:
CLOSED_GROWTH = {"BPSK": 6.0, "QPSK": 5.0, "8PSK": 1.25}


def closed_loop_raw(cls, B=CLOSED["frames"], seed=11):
    """(raw (B, 1024, 2) float32, shaped, receiver): frames of class `cls` as iq_frames_waveform defines them (waveform_reference
    on symbols, carrier phase, timing phase and channel taps drawn here from numpy's generator keyed by the class and `seed`),
    plus white noise at 20 dB; the ShapedSynth they belong to and its receiver (timing 'energy': sps = 2)."""
    from vit_vs_raw_iq_amd import Receiver, ShapedSynth, waveform_reference
    ws = ShapedSynth([cls], snrs_db=(CLOSED["snr_db"],), length=CLOSED["length"], seed=seed, sps=CLOSED["sps"], taps=CLOSED["taps"],
                     device="cpu")
    rng = np.random.default_rng([seed, CLOSED["classes"].index(cls)])
    count = ws.descriptors[0][2]
    sym = rng.integers(0, count, (B, ws.n_symbols))
    drawn = np.zeros((B, 8))
    drawn[:, 1] = CLOSED["snr_db"]
    drawn[:, 2] = rng.uniform(0.0, 2.0 * np.pi, B)
    drawn[:, 4] = rng.integers(0, ws.n_phase, B)
    taps = np.zeros((B, 8, 2))
    taps[:, :ws.taps] = rng.standard_normal((B, ws.taps, 2)) * np.asarray(ws.tap_sigma)[None, :, None]
    taps[:, 0, 0] += ws.los
    clean = waveform_reference(sym, drawn, taps, ws)
    sigma = np.sqrt(0.5 * 10.0 ** (-CLOSED["snr_db"] / 10.0))
    raw = (clean + sigma * rng.standard_normal(clean.shape)).astype(np.float32)
    return raw, ws, Receiver.for_synth(ws, timing="energy", device="cpu")


def closed_loop_symbols(cls, B=CLOSED["frames"], seed=11):
    """The frames of closed_loop_raw through receiver_reference, rounded to fp32: (B, 512, 2), what the equaliser reads."""
    from vit_vs_raw_iq_amd import receiver_reference
    raw, ws, rx = closed_loop_raw(cls, B, seed)
    return receiver_reference(raw, rx.table, rx.sps, rx.timing)[0].astype(np.float32)
