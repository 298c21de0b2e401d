"""Host evaluations of the spectrogram front end (include/iqvit.h, iq_frames_spectrogram / _bwd) the tests share.

  int_case / int_forward / int_backward   integer tables and frames and their int64 evaluation: every fp32 partial sum of the
                                          kernel is then an integer below 2^24, so the kernel must agree bit for bit
  real_forward / real_backward            the definition written out in REAL arithmetic (Re, Im, c, s -- no complex numbers, no
                                          FFT) from the fp32 table, in a chosen dtype: float64 restates the product's
                                          spectrogram_reference another way, float32 measures what fp32 arithmetic costs (E32)
"""
import math

import numpy as np


def window_index(n_fft, width, hop, pad, length):
    """(width, n_fft) sample index j = t*hop - pad + m and the mask of those inside [0, length)."""
    j = np.arange(width, dtype=np.int64)[:, None] * hop - pad + np.arange(n_fft, dtype=np.int64)[None, :]
    return j, (j >= 0) & (j < length)


def row_bins(n_fft):
    """bin of image row r: fftshift order"""
    return (np.arange(n_fft) + n_fft // 2) % n_fft


def _columns(x, j, inside):
    """x (B, 2, len) -> I and Q of every window (B, width, n_fft), zero outside the frame"""
    jc = np.clip(j, 0, x.shape[2] - 1)
    zero = np.zeros((), x.dtype)
    return np.where(inside[None], x[:, 0][:, jc], zero), np.where(inside[None], x[:, 1][:, jc], zero)


def _re_im(x, table, geom):
    n_fft, width, hop, pad = geom
    j, inside = window_index(n_fft, width, hop, pad, x.shape[2])
    ci, cq = _columns(x, j, inside)
    c, s = table[0], table[1]
    return ci @ c + cq @ s, cq @ c - ci @ s, j, inside                 # (B, width, bins)


def _overlap_add(gi, gq, j, inside, length):
    B = gi.shape[0]
    out = np.zeros((B, 2, length), gi.dtype)
    for t in range(j.shape[0]):
        ok = inside[t]
        out[:, 0, j[t, ok]] += gi[:, t, ok]
        out[:, 1, j[t, ok]] += gq[:, t, ok]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# exact integer cases
# ---------------------------------------------------------------------------------------------------------------------------
def int_case(n_fft, width, hop, pad, length, n_frames, seed):
    """Integer table (2, n_fft, n_fft), frames (n_frames, 2, length) and dout (n_frames, 1, n_fft, width) as int64.  The
    amplitudes a_t (table) and a_x (frames) satisfy 2 * n_fft * a_t * a_x < 2^11, so |Re|, |Im| < 2^11: P = Re^2 + Im^2 < 2^23 and
    every partial sum on the way are exact in fp32.  dout is in {-1, 0, 1}."""
    rng = np.random.default_rng(seed)
    prod = 2047 // (2 * n_fft)
    a_t = max(1, math.isqrt(prod))
    a_x = prod // a_t
    assert 2 * n_fft * a_t * a_x < 2 ** 11
    table = rng.integers(-a_t, a_t + 1, (2, n_fft, n_fft))
    x = rng.integers(-a_x, a_x + 1, (n_frames, 2, length))
    dout = rng.integers(-1, 2, (n_frames, 1, n_fft, width))
    return table, x, dout


def int_forward(x, table, geom):
    """mode 0, inv_norm = scale = 1, shift = 0 in int64 -> (B, 1, n_fft, width)"""
    re, im, _, _ = _re_im(x, table, geom)
    assert np.abs(re).max(initial=0) < 2 ** 11 and np.abs(im).max(initial=0) < 2 ** 11
    P = re * re + im * im
    return np.ascontiguousarray(P[:, :, row_bins(geom[0])].transpose(0, 2, 1))[:, None]


def int_backward(x, table, dout, geom):
    """-> (dx int64 (B, 2, len), bound): dx of mode 0 with inv_norm = scale = 1, and the largest sum of ABSOLUTE values of the
    terms that make up one dx element: with bound < 2^24 every fp32 partial sum of the kernel, in any order, is an exact integer."""
    n_fft = geom[0]
    re, im, j, inside = _re_im(x, table, geom)
    d = dout[:, 0].transpose(0, 2, 1)                                   # (B, width, rows)
    dbin = np.empty_like(d)
    dbin[:, :, row_bins(n_fft)] = d                                     # (B, width, bins)
    dre, dim = 2 * re * dbin, 2 * im * dbin
    c, s = table[0], table[1]
    gi, gq = dre @ c.T - dim @ s.T, dre @ s.T + dim @ c.T               # (B, width, m)
    bound = np.abs(dre) @ np.abs(c).T + np.abs(dim) @ np.abs(s).T
    bound = np.maximum(bound, np.abs(dre) @ np.abs(s).T + np.abs(dim) @ np.abs(c).T)
    length = x.shape[2]
    return _overlap_add(gi, gq, j, inside, length), int(_overlap_add(bound, bound, j, inside, length).max(initial=0))


# ---------------------------------------------------------------------------------------------------------------------------
# the definition in real arithmetic of one dtype
# ---------------------------------------------------------------------------------------------------------------------------
def _params(spec, dtype):
    return (dtype(spec.inv_norm), dtype(spec.floor), dtype(spec.scale), dtype(spec.shift))


def real_forward(x, spec, dtype):
    """(B, 2, len) -> (B, 1, n_fft, width) of `dtype`, every operation in `dtype`, from the fp32 table of `spec`."""
    x = np.asarray(x).astype(dtype)
    table = spec.table.astype(dtype)
    inv_norm, floor, scale, shift = _params(spec, dtype)
    re, im, _, _ = _re_im(x, table, (spec.n_fft, spec.width, spec.hop, spec.pad))
    P = (re * re + im * im) * inv_norm
    v = np.log10(P + floor) if spec.mode == "log" else P
    img = v * scale + shift
    assert img.dtype == dtype
    return np.ascontiguousarray(img[:, :, row_bins(spec.n_fft)].transpose(0, 2, 1))[:, None]


def real_backward(x, dout, spec, dtype):
    """The adjoint, every operation in `dtype` -> (B, 2, len)."""
    x = np.asarray(x).astype(dtype)
    table = spec.table.astype(dtype)
    inv_norm, floor, scale, _ = _params(spec, dtype)
    re, im, j, inside = _re_im(x, table, (spec.n_fft, spec.width, spec.hop, spec.pad))
    d = np.asarray(dout).astype(dtype)[:, 0].transpose(0, 2, 1)
    dbin = np.empty_like(d)
    dbin[:, :, row_bins(spec.n_fft)] = d
    g = dbin * scale * inv_norm
    if spec.mode == "log":
        P = (re * re + im * im) * inv_norm
        g = g / (dtype(math.log(10.0)) * (P + floor))
    dre, dim = dtype(2) * re * g, dtype(2) * im * g
    c, s = table[0], table[1]
    gi, gq = dre @ c.T - dim @ s.T, dre @ s.T + dim @ c.T
    out = _overlap_add(gi, gq, j, inside, x.shape[2])
    assert out.dtype == dtype
    return out
