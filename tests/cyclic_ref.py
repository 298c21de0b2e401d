"""Host evaluations of the cyclic-spectrum front end (include/iqvit.h, iq_frames_cyclic) the tests share.

  int_case / int_forward   integer frames, (c, s) tables with entries in {-1, 0, 1} and rot entries in {(+-1, 0), (0, +-1)}, and
                           their int64 evaluation.  The cases are sparse enough that X, Y, S, Sc and Sre^2 + Sim^2 -- and every
                           partial sum of absolute terms on the way -- are integers below 2^24 (int_forward asserts it), so
                           every fp32 partial sum of the kernel is exact and the kernel must agree bit for bit
  real_forward             the definition written out in REAL arithmetic (no complex numbers, no FFT) from the fp32 tables of
                           a CyclicSpectrum, in a chosen dtype: float64 restates cyclic_reference another way, float32 measures
                           what fp32 arithmetic costs (E32)
  rect_pulse_frames / check_symbol_rate_line   the sps-8 frames and the assertions on their squared coherence, for the host
                           definition and for the device
  refusal_calls            every ARG / UNSUPPORTED case of the header as a call, for host addresses and for device pointers
"""
import ctypes
import math

import numpy as np

from spectrogram_ref import _re_im, row_bins

LIMIT = 2 ** 24


def phase_index(n_fft, columns, hop, pad):
    """(columns, n_fft) index r = (k * (j0 mod n_fft)) mod n_fft into rot, j0 = t*hop - pad (both mods non-negative)."""
    j0 = np.arange(columns, dtype=np.int64) * hop - pad
    return (np.arange(n_fft, dtype=np.int64)[None, :] * (j0 % n_fft)[:, None]) % n_fft


def _rotate(re, im, rot, r):
    """Y = X (rc - i rs): (B, T, bins)"""
    rc, rs = rot[0][r][None], rot[1][r][None]
    return re * rc + im * rs, im * rc - re * rs


def _grams(yr, yi, kind):
    """[(Re, Im)] of S (kind 0), Sc (kind 1) or both (kind 2), each (B, k, l)"""
    yrt, yit = yr.transpose(0, 2, 1), yi.transpose(0, 2, 1)
    rr, ii, ir, ri = yrt @ yr, yit @ yi, yit @ yr, yrt @ yi           # [k, l] = sum_t a[t, k] b[t, l]
    out = []
    if kind in (0, 2):
        out.append((rr + ii, ir - ri))                                 # Yk conj(Yl)
    if kind in (1, 2):
        out.append((rr - ii, ri + ir))                                 # Yk Yl
    return out


def _image_index(n_fft, conj):
    """(k, l) of image element (rho, kappa): a = (rho + n/2) mod n, k = (kappa + n/2) mod n, l = (k - a) or (a - k) mod n"""
    a = row_bins(n_fft)[:, None]
    k = np.broadcast_to(row_bins(n_fft)[None, :], (n_fft, n_fft))
    return k, ((a - k) if conj else (k - a)) % n_fft


def _conj_flags(kind):
    return ((False,), (True,), (False, True))[kind]


# ---------------------------------------------------------------------------------------------------------------------------
# exact integer cases
# ---------------------------------------------------------------------------------------------------------------------------
def int_case(n_fft, columns, hop, pad, length, n_frames, seed):
    """Integer table (2, n_fft, n_fft) with entries in {-1, 0, 1}, rot (2, n_fft) with columns in {(+-1, 0), (0, +-1)} and frames
    (n_frames, 2, length) with entries in {-1, 0, 1}, as int64.  A table entry and a sample are non-zero with probability p each,
    p^2 = min(1/4, 60 / (n_fft * columns)): E|X|^2 = 4 n_fft p^2, so D[k] = sum_t |Y|^2 is about 240 and |S| stays far below
    2^12 (int_forward asserts the bound, it is not left to chance: the cases are fixed by their seeds)."""
    rng = np.random.default_rng(seed)
    p = math.sqrt(min(0.25, 60.0 / (n_fft * columns)))
    table = rng.integers(-1, 2, (2, n_fft, n_fft)) * (rng.random((2, n_fft, n_fft)) < p)
    x = rng.integers(-1, 2, (n_frames, 2, length)) * (rng.random((n_frames, 2, length)) < p)
    quarter = rng.integers(0, 4, n_fft)
    rot = np.stack([np.array([1, 0, -1, 0])[quarter], np.array([0, 1, 0, -1])[quarter]])
    return table.astype(np.int64), rot.astype(np.int64), x.astype(np.int64)


def int_forward(x, table, rot, geom, kind):
    """mode 'power', inv_norm = scale = 1, shift = 0 in int64 -> (B, C, n_fft, n_fft).  geom = (n_fft, columns, hop, pad).
    Asserts that the sum of the ABSOLUTE values of the terms of every X and of every Gram entry, and Sre^2 + Sim^2, are below
    2^24: every fp32 partial sum of the kernel, in any order, is then an exact integer."""
    n_fft, columns, hop, pad = geom
    re, im, _, _ = _re_im(x, table, geom)
    are, _, _, _ = _re_im(np.abs(x), np.abs(table), geom)            # >= the absolute terms of Re and of Im
    assert are.max(initial=0) < LIMIT
    yr, yi = _rotate(re, im, rot, phase_index(n_fft, columns, hop, pad))
    assert max(np.abs(yr).max(initial=0), np.abs(yi).max(initial=0)) < LIMIT
    ayr, ayi = np.abs(yr), np.abs(yi)
    abound = _grams(ayr, ayi, 0)[0][0]                                 # |Yr||Yr| + |Yi||Yi| summed over t
    assert abound.max(initial=0) < LIMIT and (ayi.transpose(0, 2, 1) @ ayr + ayr.transpose(0, 2, 1) @ ayi).max(initial=0) < LIMIT
    chans = []
    for conj, (gre, gim) in zip(_conj_flags(kind), _grams(yr, yi, kind)):
        P = gre * gre + gim * gim
        assert P.max(initial=0) < LIMIT
        k, l = _image_index(n_fft, conj)
        chans.append(P[:, k, l])
    return np.ascontiguousarray(np.stack(chans, axis=1))


# ---------------------------------------------------------------------------------------------------------------------------
# the definition in real arithmetic of one dtype
# ---------------------------------------------------------------------------------------------------------------------------
def real_forward(x, cs, dtype):
    """(B, 2, len) -> (B, C, n_fft, n_fft) of `dtype`, every operation in `dtype`, from the fp32 tables of `cs`."""
    x = np.asarray(x).astype(dtype)
    table, rot = cs.table.astype(dtype), cs.rot.astype(dtype)
    inv_norm, floor, scale, shift = dtype(cs.inv_norm), dtype(cs.floor), dtype(cs.scale), dtype(cs.shift)
    inv2 = inv_norm * inv_norm
    n = cs.n_fft
    re, im, _, _ = _re_im(x, table, (n, cs.columns, cs.hop, cs.pad))
    yr, yi = _rotate(re, im, rot, phase_index(n, cs.columns, cs.hop, cs.pad))
    D = (yr * yr + yi * yi).sum(axis=1, dtype=dtype)                   # (B, bins)
    kind = ("scf", "conj", "both").index(cs.kind)
    chans = []
    for conj, (gre, gim) in zip(_conj_flags(kind), _grams(yr, yi, kind)):
        k, l = _image_index(n, conj)
        P = (gre * gre + gim * gim)[:, k, l] * inv2
        if cs.mode == "power":
            v = P
        elif cs.mode == "log":
            v = np.log10(P + floor)
        else:
            v = P / (D[:, k] * D[:, l] * inv2 + floor)
        chans.append(v * scale + shift)
    out = np.ascontiguousarray(np.stack(chans, axis=1))
    assert out.dtype == dtype
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the symbol-rate line
# ---------------------------------------------------------------------------------------------------------------------------
def rect_pulse_frames(seed, sps=8, length=1024, snr_db=20.0):
    """Unit-power rectangular-pulse QPSK and BPSK at `sps` samples per symbol with a random symbol timing and carrier phase in
    noise at snr_db, and one frame of unit-power white noise -> (3, 2, length)."""
    rng = np.random.default_rng(seed)
    ns = length // sps + 1
    qpsk = (rng.integers(0, 2, ns) * 2 - 1 + 1j * (rng.integers(0, 2, ns) * 2 - 1)) / np.sqrt(2)
    bpsk = (rng.integers(0, 2, ns) * 2 - 1).astype(complex)
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2)
    out = []
    for sym in (qpsk, bpsk):
        off = rng.integers(0, sps)
        z = np.repeat(sym, sps)[off:off + length] * np.exp(1j * rng.uniform(0, 2 * np.pi))
        out.append(z + sigma * (rng.standard_normal(length) + 1j * rng.standard_normal(length)))
    out.append((rng.standard_normal(length) + 1j * rng.standard_normal(length)) / np.sqrt(2))
    z = np.stack(out)
    return np.stack([z.real, z.imag], axis=1)


def check_symbol_rate_line(img, n_fft=64, sps=8):
    """img (3, 2, Np, Np): the squared coherence of rect_pulse_frames.  A row's figure is its largest element.  On seeds 1, 2, 3
    the fp64 reference gives: rows +-Np/sps 0.963 .. 0.972, their neighbour rows 0.056 .. 0.126, the noise frame's largest row
    off alpha = 0 0.20 .. 0.24; conjugate row 0 0.997 .. 0.998 for BPSK and 0.03 .. 0.22 for QPSK.  The bounds below leave those
    figures a margin of 0.06 at least where they decide (0.9 / 0.3, 0.95 / 0.4) and follow them where they only describe."""
    h, a = n_fft // 2, n_fft // sps
    rows = img.max(axis=3)                                              # (frame, channel, row)
    noise_off_zero = np.delete(rows[2, 0], h).max()
    for f in (0, 1):
        for s in (-1, 1):
            line = rows[f, 0, h + s * a]
            assert line > 0.9
            assert rows[f, 0, h + s * a - 1] < 0.3 and rows[f, 0, h + s * a + 1] < 0.3
            assert line > noise_off_zero + 0.5
    assert noise_off_zero < 0.4
    assert rows[1, 1, h] > 0.95 and rows[0, 1, h] < 0.4                 # conjugate channel, alpha = 0: BPSK yes, QPSK no
    assert rows[2, 1, h] < 0.4
    # Cauchy-Schwarz up to rounding: in fp32 S[k,k] and D[k] are two different chains of 61 terms, each within 61 * 2^-24 = 4e-6
    # of the truth; squared and divided that is 2e-5 at most
    assert img.min() >= 0.0 and img.max() <= 1.0 + 1e-4


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def refusal_calls(L, a):
    """[(description, callable -> status, expected status)]: every ARG / UNSUPPORTED case of the header and the empty calls.  `a` is
    a 16-byte aligned address that is never dereferenced on these paths."""
    from vit_vs_raw_iq_amd import CyclicSpectrum
    ARG, UNSUPPORTED = 1, 2
    base = CyclicSpectrum(32, 64, 8)
    out = []

    def case(expect, x=a, table=a, rot=a, io=a, n=2, length=64, par="ok", **edit):
        def run():
            p = par
            if p == "ok":
                p = base.struct()
                for k, v in edit.items():
                    setattr(p, k, v)
            return L.iq_frames_cyclic(x, table, rot, io, n, length, ctypes.byref(p) if p is not None else None, None)
        what = dict(edit, **{k: v for k, v in (("x", x), ("table", table), ("rot", rot), ("io", io)) if v != a},
                    n=n, length=length, par=None if par is None else "set")
        out.append((repr(what), run, expect))

    for k in ("x", "table", "rot", "io", "par"):
        case(ARG, **{k: None})
    for kw in (dict(length=0), dict(length=-5), dict(hop=0), dict(hop=-1), dict(columns=0), dict(columns=-3), dict(pad=-1),
               dict(kind=3), dict(kind=-1), dict(mode=3), dict(mode=-1)):
        case(ARG, **kw)
    for field in ("inv_norm", "floor", "scale", "shift"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            case(ARG, **{field: bad})
    for mode in (1, 2):
        case(ARG, mode=mode, floor=0.0)
        case(ARG, mode=mode, floor=-1.0)
    case(0, mode=0, floor=0.0, n=0)                                      # the floor is not used in power mode
    for kw in (dict(x=a + 2), dict(table=a + 1), dict(rot=a + 2), dict(io=a + 4), dict(io=a + 8)):
        case(ARG, **kw)
    case(0, x=a + 8, table=a + 4, rot=a + 4, n=0)                        # 4-byte alignment is enough for the operands
    for n_fft in (0, 16, 31, 33, 48, 288, 512, -32):
        case(UNSUPPORTED, n_fft=n_fft)
    case(UNSUPPORTED, length=8193)                                       # 8 bytes per sample above 64 KB of LDS
    case(0, n=0)
    case(0, n=-1)
    for n_fft in range(32, 257, 32):
        case(0, n_fft=n_fft, n=0)
    case(0, length=8192, n=0)
    return out
