"""Host evaluations of the constellation front end (include/iqvit.h, iq_frames_constellation / _bwd) the tests share.

  EXACT / int_case / int_forward / int_backward   integer tables and points on a dyadic grid and their int64 evaluation: every
                                          weight is an integer and every fp32 partial sum of the kernel an integer below 2^24
                                          (asserted here, from the sums of ABSOLUTE values), so the kernel must agree bit for bit
  real_forward / real_backward            the definition written out in numpy arithmetic of a chosen dtype from the fp32 table:
                                          float64 restates the product's constellation_reference another way, float32 measures
                                          what fp32 arithmetic costs (E32)
"""
import math

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------------
# exact integer cases
# ---------------------------------------------------------------------------------------------------------------------------
# name -> (height, width, len, radius, n_frac, n_frames, placement, shift).  x_scale = y_scale = 1, offsets 0, inv_norm = scale
# = 1, mode 0: a sample IS its pixel coordinate.  n_frac 1: points at k + 0.5 (t an integer, f = 0); n_frac 2: points at
# multiples of 0.25 and even tables (f in {0, 0.5}, f * slope an integer).  The kernels work in 32 x 32 tiles: forward one
# workgroup per tile row, wave w takes column tiles w, w + 4; backward rounds of four tiles in row-major order.
EXACT = {
    # one point: a list of one survivor, padded to two; one tile.  (Radius 1 needs n_frac 2 for a gradient: at n_frac 1 the
    # points sit on pixel centres, where sgn(e) = 0.)
    "one_point_32x32": (32, 32, 1, 1, 2, 1, "interior", 0),
    # two points, two column tiles (waves 0 and 1), radius 2 with the table [4, 2, 0]
    "two_points_32x64": (32, 64, 2, 2, 1, 1, "interior", 0),
    # 31 points, all within reach of the one tile: an ODD number of survivors; n_frac 2: the interpolation at f = 0.5
    "len31_odd_survivors_nfrac2": (32, 32, 31, 2, 2, 1, "interior", 0),
    # 33 points on and beyond the image border: windows partly and wholly outside; six tiles: a second backward round of two
    "len33_border_96x64": (96, 64, 33, 1, 2, 3, "border", 0),
    # 64 points on tile edges (coordinates 31.5 / 32.5 / 63.5 / 64.5): windows that span two and four tiles
    "len64_tile_edges": (96, 64, 64, 2, 1, 1, "edges", 0),
    # 65 points (a second ballot pass of one point), radius 16: every window spans tiles and most leave the image
    "len65_radius16": (96, 64, 65, 16, 1, 2, "border", 0),
    # 256 x 256: 64 tiles, eight workgroups per frame forward, sixteen full rounds backward; NaN and infinite samples mixed in
    "len1024_nonfinite_256x256_nfrac2": (256, 256, 1024, 2, 2, 2, "nonfinite", 0),
    # every point in ONE pixel next to a tile corner: four tiles whose lists are len = 8192 long (the dense product)
    "len8192_one_pixel": (256, 256, 8192, 2, 1, 1, "one_pixel", 0),
    # all points inside tile (0, 0): the other tiles are empty lists and hold exactly `shift`
    "empty_tiles_hold_shift": (96, 64, 64, 1, 2, 1, "corner", 5),
    # the longest frame over the largest image at the largest radius, n_frac 2
    "len8192_radius16_nfrac2": (256, 256, 8192, 16, 2, 1, "border", 0),
}


def int_table(radius, n_frac, rng):
    """Integer table of radius * n_frac + 1 entries, the last 0; even entries for n_frac 2."""
    if (radius, n_frac) == (2, 1):
        return np.array([4, 2, 0], np.int64)
    t = rng.integers(1, 5, radius * n_frac + 1) * n_frac
    t[-1] = 0
    return t.astype(np.int64)


def int_case(name):
    """-> dict(height, width, radius, n_frac, shift, table int64, x float64 (n, 2, len), dout int64 (n, 1, height, width))."""
    H, W, length, radius, n_frac, n, placement, shift = EXACT[name]
    rng = np.random.default_rng(len(name) + 7 * length + radius)
    step = 1.0 if n_frac == 1 else 0.25
    first = 0.5 if n_frac == 1 else 0.0

    def grid(lo, hi, size):                                   # coordinates on the dyadic grid within [lo, hi)
        return first + step * rng.integers(int(round((lo - first) / step)), int(round((hi - first) / step)), size)
    x = np.empty((n, 2, length))
    if placement in ("interior", "nonfinite"):
        x[:, 0], x[:, 1] = grid(0, W, (n, length)), grid(0, H, (n, length))
    elif placement == "border":
        x[:, 0], x[:, 1] = grid(-radius - 3, W + radius + 3, (n, length)), grid(-radius - 3, H + radius + 3, (n, length))
    elif placement == "edges":
        x[:, 0] = rng.choice([31.5, 32.5, 0.5, W - 0.5], (n, length))
        x[:, 1] = rng.choice([31.5, 32.5, 63.5, 64.5], (n, length))
    elif placement == "one_pixel":
        x[:, 0], x[:, 1] = 64.5, 63.5
    elif placement == "corner":
        x[:, 0], x[:, 1] = grid(2, 30, (n, length)), grid(2, 30, (n, length))
    else:
        raise ValueError(placement)
    if placement == "nonfinite":
        bad = rng.choice([np.nan, np.inf, -np.inf], (n, 2, length))
        x = np.where(rng.random((n, 2, length)) < 0.1, bad, x)
    dout = rng.integers(-1, 2, (n, 1, H, W))
    return dict(height=H, width=W, radius=radius, n_frac=n_frac, shift=shift, table=int_table(radius, n_frac, rng), x=x,
                dout=dout)


def as_constellation(case, mode="power"):
    """The product's Constellation of an exact case: its table, unit scales, zero offsets, inv_norm = scale = 1."""
    from vit_vs_raw_iq_amd import Constellation
    con = Constellation(case["height"], case["width"], case["x"].shape[2], table=case["table"], radius=case["radius"],
                        n_frac=case["n_frac"], mode=mode, floor=1.0, inv_norm=1.0, shift=float(case["shift"]))
    con.x_scale = con.y_scale = 1.0
    con.x_off = con.y_off = 0.0
    return con


def _int_weights(s, n_pix, table, radius, n_frac):
    """s (B, len) pixel coordinates -> (w, d) int64 (B, len, n_pix): the weights and sgn(e) * slope, asserted to be integers."""
    tab = table.astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = s[..., None] - (np.arange(n_pix) + 0.5)
        t = np.abs(e) * n_frac
        ok = t < radius * n_frac
    t = np.where(ok, t, 0.0)
    i = np.floor(t).astype(np.int64)
    slope = tab[i + 1] - tab[i]
    w = np.where(ok, (t - i) * slope + tab[i], 0.0)
    d = np.where(ok, np.sign(np.where(ok, e, 0.0)) * slope, 0.0)
    assert np.array_equal(w, np.rint(w)) and np.array_equal(d, np.rint(d))
    return w.astype(np.int64), d.astype(np.int64)


def _mm(p, q):
    """The matrix product of two int64 arrays through the fp64 BLAS (exact: every sum of absolute terms stays below 2^53, asserted
    by the callers' bounds, which are products of the same kind over the absolute values) -> int64."""
    r = p.astype(np.float64) @ q.astype(np.float64)
    assert np.abs(r).max(initial=0) < 2 ** 53
    return np.rint(r).astype(np.int64)


def int_forward(case):
    """mode 0, inv_norm = scale = 1 in int64 -> ((B, 1, H, W), the largest sum of absolute terms of one pixel, < 2^24)."""
    b, _ = _int_weights(case["x"][:, 0], case["width"], case["table"], case["radius"], case["n_frac"])
    a, _ = _int_weights(case["x"][:, 1], case["height"], case["table"], case["radius"], case["n_frac"])
    D = _mm(a.transpose(0, 2, 1), b)
    bound = int(_mm(np.abs(a).transpose(0, 2, 1), np.abs(b)).max(initial=0)) + abs(case["shift"])
    assert bound < 2 ** 24, bound
    return (D + case["shift"])[:, None], bound


def int_backward(case):
    """-> (dx int64 (B, 2, len), bound): dx of mode 0 with inv_norm = scale = 1, and the largest sum of ABSOLUTE values of the
    terms of one dx element times n_frac: below 2^24 (asserted), so every fp32 partial sum of the kernel is an exact integer."""
    nf = case["n_frac"]
    b, db = _int_weights(case["x"][:, 0], case["width"], case["table"], case["radius"], nf)
    a, da = _int_weights(case["x"][:, 1], case["height"], case["table"], case["radius"], nf)
    g = case["dout"][:, 0]
    di = nf * (_mm(a, g) * db).sum(axis=2)
    dq = nf * (_mm(b, g.transpose(0, 2, 1)) * da).sum(axis=2)
    ag = np.abs(g)
    bound = max(int((nf * (_mm(np.abs(a), ag) * np.abs(db)).sum(axis=2)).max(initial=0)),
                int((nf * (_mm(np.abs(b), ag.transpose(0, 2, 1)) * np.abs(da)).sum(axis=2)).max(initial=0)))
    assert bound < 2 ** 24, bound
    return np.stack([di, dq], axis=1), bound


# ---------------------------------------------------------------------------------------------------------------------------
# the definition in arithmetic of one dtype (the parameters as the kernel gets them: rounded to fp32 first)
# ---------------------------------------------------------------------------------------------------------------------------
def _weights(s, scale, off, n_pix, con, dtype):
    tab = con.table.astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        u = s * dtype(np.float32(scale)) + dtype(np.float32(off))
        e = u[..., None] - (np.arange(n_pix).astype(dtype) + dtype(0.5))
        t = np.abs(e) * dtype(con.n_frac)
        ok = t < dtype(con.radius * con.n_frac)
    t = np.where(ok, t, dtype(0))
    fl = np.floor(t)
    i = fl.astype(np.int64)
    slope = tab[i + 1] - tab[i]
    w = np.where(ok, (t - fl) * slope + tab[i], dtype(0))
    d = np.where(ok, np.sign(np.where(ok, e, dtype(0))) * slope, dtype(0))
    assert w.dtype == dtype and d.dtype == dtype
    return w, d


def _density(x, con, dtype):
    x = np.asarray(x).astype(dtype)
    b, db = _weights(x[:, 0], con.x_scale, con.x_off, con.width, con, dtype)
    a, da = _weights(x[:, 1], con.y_scale, con.y_off, con.height, con, dtype)
    V = (a.transpose(0, 2, 1) @ b) * dtype(np.float32(con.inv_norm))
    return V, a, da, b, db


def real_forward(x, con, dtype):
    """(B, 2, len) -> (B, 1, height, width) of `dtype`, every operation in `dtype`, from the fp32 table of `con`."""
    V = _density(x, con, dtype)[0]
    v = np.log10(V + dtype(np.float32(con.floor))) if con.mode == "log" else V
    img = v * dtype(np.float32(con.scale)) + dtype(np.float32(con.shift))
    assert img.dtype == dtype
    return img[:, None]


def real_backward(x, dout, con, dtype):
    """The adjoint, every operation in `dtype` -> (B, 2, len)."""
    V, a, da, b, db = _density(x, con, dtype)
    g = np.asarray(dout).astype(dtype)[:, 0] * dtype(np.float32(con.scale)) * dtype(np.float32(con.inv_norm))
    if con.mode == "log":
        g = g / (dtype(math.log(10.0)) * (V + dtype(np.float32(con.floor))))
    di = dtype(np.float32(con.x_scale)) * dtype(con.n_frac) * ((a @ g) * db).sum(axis=2)
    dq = dtype(np.float32(con.y_scale)) * dtype(con.n_frac) * ((b @ g.transpose(0, 2, 1)) * da).sum(axis=2)
    out = np.stack([di, dq], axis=1)
    assert out.dtype == dtype
    return out
