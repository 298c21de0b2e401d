"""What the carrier-recovery suites share (tests/test_carrier_cpu.py, tests/test_gpu_carrier.py): host-made inputs, the derived
fp32 bounds, and the exact-case tables.  Host only, numpy only: everything here can be checked without a GPU.

The bounds (u = 2^-24, tables with |entries| <= 1, w = z^M, L1 = sum_n |w[n]|):

  w       one squaring v <- rot(v, v.re, v.im) errs by at most 2.5 u |v|^2 in modulus (re: u y^2 + u |x^2 - y^2|, im: 3 u |x y|), so
          the relative error obeys e' = 2 e + 3 u: 3 (M - 1) u after log2 M squarings.
  W[k]    stage 1 is a chain of 2 n1 fused terms per component: 2 n1 u sqrt2 T[b], T[b] = sum_a |w[a n2 + b]|; the twiddle passes
          that on times sqrt2 and adds 2 u T[b]: (4 n1 + 2) u T[b]; stage 2 passes it on times sqrt2 and adds 2 n2 u sqrt2 sum_b
          T[b]; the error of w arrives with gain 1.  Per component, with sum_b T[b] = L1:
              dW <= (6 n1 + 3 n2 + 3 M) u L1                                            (5.66 n1 + 2.83 n2 + 2.83 + 3 (M - 1))
  P[k]    P = fmaf(im, im, re * re):  dP <= 2 sqrt2 sqrt(P) dW + 2 dW^2 + 2 u P.
  d       d = 0.5 (a - c) / den, den = a - 2 b + c, each of a, b, c within dlt = dP + 4 u b (the fp32 evaluation of den cancels to
          within 4 u b):  dd <= dlt / |den| + 2 dlt |a - c| / den^2;  F moves by dd 2^32 / (N M), plus 1 for the rounding.
  out     (c, s) = sincospif within 4 u (two ulp of a value below 1, doubled), two roundings per component: 8 u (|I| + |Q|).
  S, TH   S moves with the frequency by at most 2 pi M df sum_n n |w[n]| and with the arithmetic by (len / 256 + 3 M + 16) u L1
          (the partial sums of a thread and of the butterfly, sincospif, the error of w); TH = arg S / (2 pi M) in turns.
A factor 1.01 covers the second-order terms.  None of these figures was fitted to the kernel."""
import numpy as np

EPS = 2.0 ** -24
SLACK = 1.01
TWO32 = 2.0 ** 32

CONSTELLATIONS = {1: np.array([1.0 + 0j]), 2: np.array([1.0, -1.0]) + 0j,
                  4: np.exp(1j * (np.pi / 4 + np.pi / 2 * np.arange(4))), 8: np.exp(1j * np.pi / 4 * np.arange(8))}

# name -> (M, B, len, (n1, n2), snr_db): a tone, BPSK, QPSK and 8PSK under a random frequency offset within +-0.4 / M cycle per
# sample, a random phase and AWGN; N >= 2 len throughout
REAL = {"tone_m1": (1, 6, 500, (32, 32), 10.0), "bpsk_m2": (2, 6, 512, (32, 32), 10.0), "qpsk_m4": (4, 6, 1000, (64, 32), 10.0),
        "8psk_m8": (8, 6, 512, (32, 32), 25.0), "qpsk_m4_8192": (4, 2, 4096, (128, 64), 15.0), "qpsk_m4_96x32": (4, 3, 1500, (96, 32), 12.0)}


def to_planar(z):
    return np.stack([z.real, z.imag], axis=1).astype(np.float32)


def to_complex(x, planar=True):
    x = np.asarray(x, dtype=np.float64)
    return x[:, 0] + 1j * x[:, 1] if planar else x[:, :, 0] + 1j * x[:, :, 1]


def real_case(name):
    """-> planar fp32 frames (B, 2, len) of REAL[name], seeded by the name."""
    M, B, length, _, snr_db = REAL[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    sym = CONSTELLATIONS[M][rng.integers(0, len(CONSTELLATIONS[M]), (B, length))]
    f = rng.uniform(-0.4 / M, 0.4 / M, (B, 1))
    th = rng.uniform(0, 2 * np.pi, (B, 1))
    sigma = np.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
    noise = sigma * (rng.standard_normal((B, length)) + 1j * rng.standard_normal((B, length)))
    return to_planar(sym * np.exp(1j * (2 * np.pi * f * np.arange(length)[None, :] + th)) + noise)


def peak_lead(power, s_hat):
    """Per frame: P[k^] over the largest P outside {k^, k^ +- 1}."""
    B, Nd = power.shape
    lead = np.empty(B)
    for i in range(B):
        k = int(s_hat[i]) % Nd
        rest = np.delete(power[i], [(k - 1) % Nd, k, (k + 1) % Nd])
        lead[i] = power[i, k] / rest.max()
    return lead


def mth_power(z, M):
    w = np.array(z, dtype=np.complex128)
    for _ in range(int(np.log2(M))):
        w = w * w
    return w


def dw_bound(z, M, n1, n2):
    """(B,) the bound on either component of any W[k]."""
    return SLACK * (6 * n1 + 3 * n2 + 3 * M) * EPS * np.abs(mth_power(z, M)).sum(axis=1)


def power_bound(power, dw):
    """(B, N) from the reference's power and dw_bound."""
    dw = dw[:, None]
    return 2 * np.sqrt(2.0) * np.sqrt(power) * dw + 2 * dw ** 2 + 2 * EPS * power


def out_bound(x):
    """Per component of out, x in either layout (the sum runs over the axis of size 2)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    axis = 1 if x.shape[1] == 2 and x.shape[2] != 2 else 2
    return 8 * EPS * np.repeat(x.sum(axis=axis, keepdims=True), 2, axis=axis)


def f_tolerance(power, dP, s_hat, M):
    """(B,) counts of 2^-32 cycle per sample the device's F may differ from the reference's by, the peak bin agreeing."""
    B, Nd = power.shape
    tol = np.empty(B)
    for i in range(B):
        k = int(s_hat[i]) % Nd
        km, kp = (k - 1) % Nd, (k + 1) % Nd
        a, b, c = power[i, km], power[i, k], power[i, kp]
        dlt = max(dP[i, km], dP[i, k], dP[i, kp]) + 4 * EPS * b
        den = a - 2 * b + c
        dd = SLACK * (dlt / abs(den) + 2 * dlt * abs(a - c) / den ** 2)
        tol[i] = dd * TWO32 / (Nd * M) + 1
    return tol


def th_tolerance(z, M, f_ref, f_tol):
    """(B,) counts of 2^-32 turn for TH, compared modulo 2^32 / M: from the reference's S at its own F."""
    w = mth_power(z, M)
    B, length = w.shape
    n = np.arange(length)
    tol = np.empty(B)
    for i in range(B):
        S = abs(np.sum(w[i] * np.exp(-2j * np.pi * M * f_ref[i] / TWO32 * n)))
        aw = np.abs(w[i])
        dS = 2 * np.pi * M * f_tol[i] / TWO32 * np.sum(n * aw) + (length / 256 + 3 * M + 16) * EPS * aw.sum()
        tol[i] = SLACK * np.arcsin(min(1.0, dS / S) if S > 0 else 1.0) / (2 * np.pi * M) * TWO32 + 1
    return tol


def circular(a, b, period):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % period
    return np.minimum(d, period - d)


# ---- exact cases: integer tables and frames
def integer_tables(n1, n2, seed, density=0.15):
    """(t1, t2, tw) with entries in {-1, 0, 1}, about `density` of them non-zero, the corners taking part."""
    rng = np.random.default_rng(seed)

    def draw(shape):
        t = rng.integers(-1, 2, shape) * (rng.random(shape) < density * 1.5)
        return t.astype(np.float32)
    t1, t2, tw = draw((2, n1, n1)), draw((2, n2, n2)), draw((2, n1 * n2))
    for t in (t1, t2):
        t[0, 0, 0] = t[0, -1, -1] = t[1, 0, -1] = t[1, -1, 0] = 1.0
    tw[0, 0] = tw[1, 0] = tw[0, (n1 - 1) * (n2 - 1)] = 1.0
    return t1, t2, tw


def integer_frames(B, length, seed):
    """(B, 2, length) fp32 with entries in {-1, 0, 1}, both ends of every frame non-zero."""
    x = np.random.default_rng(seed).integers(-1, 2, (B, 2, length)).astype(np.float32)
    x[:, 0, 0] = x[:, 1, -1] = 1.0
    return x


def exact_partial_sum_bound(x, tables, M):
    """The largest sum of absolute terms of any component of any W[k] of planar frames x: below 2^12 every fp32 partial sum of
    both stages is an exact integer and so is P = re^2 + im^2 < 2^24."""
    t1, t2, tw = (np.abs(np.asarray(t, dtype=np.float64)).sum(axis=0) for t in tables)
    n1, n2 = t1.shape[0], t2.shape[0]
    w = mth_power(to_complex(x), M)
    wp = np.zeros((w.shape[0], n1 * n2))
    wp[:, :w.shape[1]] = np.abs(w.real) + np.abs(w.imag)
    A = np.einsum("ak,nab->nkb", t1, wp.reshape(-1, n1, n2))
    Bm = A * tw[np.arange(n1)[:, None] * np.arange(n2)[None, :]]
    return float(np.einsum("nkb,bq->nqk", Bm, t2).max())


def permutation_tables(n1, n2):
    """Tables under which W[k1 + n1 k2] = w[k1 n2 + k2]: with M = 1, P is |z|^2 in a known order and any power can be built."""
    eye = lambda n: np.stack([np.eye(n), np.zeros((n, n))]).astype(np.float32)       # noqa: E731
    tw = np.stack([np.ones(n1 * n2), np.zeros(n1 * n2)]).astype(np.float32)
    return eye(n1), eye(n2), tw


def frame_with_power(P, n1, n2):
    """Planar (1, 2, N) frame whose power under permutation_tables is P (squares of integers, natural bin order)."""
    k = np.arange(n1 * n2)
    k1, k2 = k % n1, k // n1
    z = np.zeros(n1 * n2)
    z[k1 * n2 + k2] = np.sqrt(np.asarray(P, dtype=np.float64))
    assert np.array_equal(z, np.rint(z))
    return np.stack([z, np.zeros_like(z)])[None].astype(np.float32)
