"""Host evaluations of the cyclic-spectrum adjoint (include/iqvit.h, iq_frames_cyclic_bwd) the tests share.

  real_backward            the header's formulae written out in REAL arithmetic (no complex numbers, no FFT) from the fp32 tables
                           of a CyclicSpectrum, in a chosen dtype: float64 restates cyclic_reference_bwd another way, float32
                           measures what fp32 arithmetic costs (E32)
  int_dout / int_backward  dout with entries in {-1, 0, 1} for the inputs of cyclic_ref.int_case and the int64 evaluation of the
                           adjoint in mode power with inv_norm = scale = 1.  int_backward asserts that the sum of the ABSOLUTE
                           terms of every partial sum on the way (H, Hc, G_Y, G_X, the per-column products, the overlap-add per
                           sample) is below 2^24: every fp32 partial sum of the kernel, in any order, is then an exact integer
  refusal_calls            every ARG / UNSUPPORTED case of the header as a call, for host addresses and for device pointers
"""
import ctypes
import math

import numpy as np

from cyclic_ref import LIMIT, _conj_flags, _grams, _rotate, phase_index
from spectrogram_ref import _overlap_add, _re_im, row_bins


def pair_index(n_fft, conj):
    """(row, column) of the image element that holds the pair (k, l), each (n_fft, n_fft) indexed [k, l]: row of a = k - l
    (SCF) or k + l (conjugate), column of k, both in fftshift order."""
    k, l = np.meshgrid(np.arange(n_fft), np.arange(n_fft), indexing="ij")
    a = (k + l) % n_fft if conj else (k - l) % n_fft
    h = n_fft // 2
    assert np.array_equal(row_bins(n_fft)[(a + h) % n_fft], a) and np.array_equal(row_bins(n_fft)[(k + h) % n_fft], k)
    return (a + h) % n_fft, (k + h) % n_fft


def _folded(d, n_fft, conj):
    """g[k,l] + g[l,k] of one channel's dout (B, n_fft, n_fft) -> (B, k, l)"""
    row, col = pair_index(n_fft, conj)
    g = d[:, row, col]
    return g + g.transpose(0, 2, 1)


def _gy(yr, yi, hs, kind):
    """G_Y (Re, Im), (B, T, k): sum_l H[k,l] Y[t,l] + Hc[k,l] conj(Y[t,l]); hs = [(Hre, Him)] in the order of cyclic_ref._grams"""
    gyr, gyi = 0, 0
    for conj, (hre, him) in zip(_conj_flags(kind), hs):
        hre, him = hre.transpose(0, 2, 1), him.transpose(0, 2, 1)       # [l, k]
        if conj:
            gyr, gyi = gyr + yr @ hre + yi @ him, gyi + yr @ him - yi @ hre
        else:
            gyr, gyi = gyr + yr @ hre - yi @ him, gyi + yi @ hre + yr @ him
    return gyr, gyi


def _unrotate(gyr, gyi, rot, r):
    """G_X = (rc + i rs) G_Y"""
    rc, rs = rot[0][r][None], rot[1][r][None]
    return gyr * rc - gyi * rs, gyr * rs + gyi * rc


def _to_samples(dre, dim, table, j, inside, length):
    c, s = table[0], table[1]
    return _overlap_add(dre @ c.T - dim @ s.T, dre @ s.T + dim @ c.T, j, inside, length)


# ---------------------------------------------------------------------------------------------------------------------------
# exact integer cases
# ---------------------------------------------------------------------------------------------------------------------------
# (n_fft, columns, hop, pad, len, n_frames): the ten geometries of EXACT in tests/test_gpu_cyclic.py, the smallest that reach each
# route of the kernels (1 / 2 / 3 / 5 / 7 / 8 tiles; 1, 2 and 3 chunks; 31 / 32 / 33 columns; an odd column count and an odd
# length; pad over the front and windows past the end; the forward's two launch shapes and both sides of its 144 KB limit)
EXACT = {
    "one_tile_one_column": (32, 1, 1, 0, 100, 1),
    "two_columns_odd_len": (64, 2, 16, 0, 101, 3),
    "three_columns_wrap": (96, 3, 5, 7, 300, 1),
    "chunk_minus_one": (160, 31, 29, 40, 900, 1),
    "one_chunk": (32, 32, 16, 0, 1024, 1),
    "chunk_plus_one": (224, 33, 29, 100, 1024, 3),
    "eight_tiles_two_chunks": (256, 40, 4, 255, 1024, 1),
    "three_chunks": (64, 70, 5, 9, 333, 3),
    "cache_limit": (256, 3, 97, 0, 1632, 1),
    "past_cache_limit": (256, 3, 97, 0, 1633, 1),
}
DENSITY = 0.75                  # of the non-zero entries of dout at which int_backward's bounds hold for every case above


def int_dout(n_fft, channels, n_frames, seed, density):
    """(n_frames, channels, n_fft, n_fft) int64 with entries in {-1, 0, 1}, non-zero with probability `density`.  The density of a
    case is chosen so that int_backward's bounds hold; its assertions keep it so."""
    rng = np.random.default_rng(seed)
    shape = (n_frames, channels, n_fft, n_fft)
    return (rng.integers(0, 2, shape) * 2 - 1) * (rng.random(shape) < density)


def int_backward(x, table, rot, dout, geom, kind):
    """mode 'power', inv_norm = scale = 1 in int64 -> dx (B, 2, len).  geom = (n_fft, columns, hop, pad).  Asserts the bounds of the
    module docstring (those of Y, S and Sc are cyclic_ref.int_forward's)."""
    n_fft, columns, hop, pad = geom
    length = x.shape[2]
    re, im, j, inside = _re_im(x, table, geom)
    r = phase_index(n_fft, columns, hop, pad)
    yr, yi = _rotate(re, im, rot, r)
    ayr, ayi = np.abs(yr), np.abs(yi)
    hs, ahs = [], []
    for ch, (conj, (gre, gim)) in enumerate(zip(_conj_flags(kind), _grams(yr, yi, kind))):
        w = _folded(dout[:, ch], n_fft, conj)
        hs.append((2 * w * gre, 2 * w * gim))
        ahs.append((np.abs(hs[-1][0]), np.abs(hs[-1][1])))
        assert max(ahs[-1][0].max(initial=0), ahs[-1][1].max(initial=0)) < LIMIT
    gyr, gyi = _gy(yr, yi, hs, kind)
    # absolute terms of Re G_Y and of Im G_Y, both channels in one sum as in the kernel
    agr = sum(ayr @ hre.transpose(0, 2, 1) + ayi @ him.transpose(0, 2, 1) for hre, him in ahs)
    agi = sum(ayi @ hre.transpose(0, 2, 1) + ayr @ him.transpose(0, 2, 1) for hre, him in ahs)
    assert max(agr.max(initial=0), agi.max(initial=0)) < LIMIT
    dre, dim = _unrotate(gyr, gyi, rot, r)
    arot = (np.abs(rot[0]) + np.abs(rot[1]))[r][None]
    assert ((np.abs(gyr) + np.abs(gyi)) * arot).max(initial=0) < LIMIT
    asum = np.abs(dre) + np.abs(dim)
    aprod = asum @ (np.abs(table[0]) + np.abs(table[1])).T             # >= the absolute terms of G_I and of G_Q, over all k
    assert aprod.max(initial=0) < LIMIT
    assert _overlap_add(aprod, aprod, j, inside, length).max(initial=0) < LIMIT
    return _to_samples(dre, dim, table, j, inside, length)


# ---------------------------------------------------------------------------------------------------------------------------
# the formulae in real arithmetic of one dtype
# ---------------------------------------------------------------------------------------------------------------------------
def real_backward(x, dout, cs, dtype):
    """(B, 2, len), (B, C, n_fft, n_fft) -> dx (B, 2, len) of `dtype`, every operation in `dtype`, from the fp32 tables of `cs`."""
    x = np.asarray(x).astype(dtype)
    d = np.asarray(dout).astype(dtype)
    table, rot = cs.table.astype(dtype), cs.rot.astype(dtype)
    inv_norm, floor, scale = dtype(cs.inv_norm), dtype(cs.floor), dtype(cs.scale)
    inv2 = inv_norm * inv_norm
    n = cs.n_fft
    geom = (n, cs.columns, cs.hop, cs.pad)
    re, im, j, inside = _re_im(x, table, geom)
    r = phase_index(*geom)
    yr, yi = _rotate(re, im, rot, r)
    D = (yr * yr + yi * yi).sum(axis=1, dtype=dtype)                   # (B, bins)
    den = D[:, :, None] * D[:, None, :] * inv2 + floor
    kind = ("scf", "conj", "both").index(cs.kind)
    hs, gd = [], np.zeros_like(D)
    for ch, (conj, (gre, gim)) in enumerate(zip(_conj_flags(kind), _grams(yr, yi, kind))):
        w = scale * _folded(d[:, ch], n, conj)
        P = (gre * gre + gim * gim) * inv2
        if cs.mode == "power":
            u = w
        elif cs.mode == "log":
            u = w / (dtype(math.log(10.0)) * (P + floor))
        else:
            u = w / den
            gd += (w * P * D[:, None, :] / (den * den)).sum(axis=2, dtype=dtype)
        h = dtype(2) * inv2 * u
        hs.append((h * gre, h * gim))
    gyr, gyi = _gy(yr, yi, hs, kind)
    if cs.mode == "coherence":
        g2 = dtype(2) * (-inv2 * gd)[:, None, :]
        gyr, gyi = gyr + g2 * yr, gyi + g2 * yi
    dre, dim = _unrotate(gyr, gyi, rot, r)
    out = _to_samples(dre, dim, table, j, inside, x.shape[2])
    assert out.dtype == dtype
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def adjoint_lds_bytes(n_fft, length):
    """The header's LDS rule of iq_frames_cyclic_bwd."""
    return 4 * (2 * ((2 * length + 3) & ~3) + 67 * n_fft + 6688)


def refusal_calls(L, a):
    """[(description, callable -> status, expected status)]: every ARG / UNSUPPORTED case of the header and the empty calls.  `a` is
    a 16-byte aligned address that is never dereferenced on these paths."""
    from vit_vs_raw_iq_amd import CyclicSpectrum
    ARG, UNSUPPORTED = 1, 2
    base = CyclicSpectrum(32, 64, 8)
    out = []

    def case(expect, x=a, table=a, rot=a, dout=a, dx=a, n=2, length=64, par="ok", **edit):
        def run():
            p = par
            if p == "ok":
                p = base.struct()
                for k, v in edit.items():
                    setattr(p, k, v)
            return L.iq_frames_cyclic_bwd(x, table, rot, dout, dx, n, length, ctypes.byref(p) if p is not None else None, None)
        what = dict(edit, **{k: v for k, v in (("x", x), ("table", table), ("rot", rot), ("dout", dout), ("dx", dx)) if v != a},
                    n=n, length=length, par=None if par is None else "set")
        out.append((repr(what), run, expect))

    for k in ("x", "table", "rot", "dout", "dx", "par"):
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
    for kw in (dict(x=a + 2), dict(table=a + 1), dict(rot=a + 2), dict(dout=a + 2), dict(dx=a + 1), dict(dx=a + 3)):
        case(ARG, **kw)
    case(0, x=a + 8, table=a + 4, rot=a + 4, dout=a + 4, dx=a + 12, n=0)  # 4-byte alignment is enough for every operand
    case(ARG, n_fft=48, hop=0)                                           # ARG comes before UNSUPPORTED
    for n_fft in (0, 16, 31, 33, 48, 288, 512, -32):
        case(UNSUPPORTED, n_fft=n_fft)
    case(UNSUPPORTED, length=8193)                                       # 8 bytes per sample above 64 KB of LDS
    # the LDS rule: the frame and its gradient beside the working set; refused even when no frame is given
    assert adjoint_lds_bytes(256, 4280) <= 160 * 1024 < adjoint_lds_bytes(256, 4281)
    assert adjoint_lds_bytes(32, 8032) <= 160 * 1024 < adjoint_lds_bytes(32, 8033)
    case(0, n_fft=256, length=4280, n=0)
    case(UNSUPPORTED, n_fft=256, length=4281, n=0)
    case(UNSUPPORTED, n_fft=256, length=8192)
    case(0, n_fft=32, length=8032, n=0)
    case(UNSUPPORTED, n_fft=32, length=8033)
    case(UNSUPPORTED, n_fft=32, length=8192, n=0)
    case(0, n=0)
    case(0, n=-1)
    for n_fft in range(32, 257, 32):
        case(0, n_fft=n_fft, length=4096, n=0)
    return out
