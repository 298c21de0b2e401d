"""CPU: the host definition of the constellation front end (vit_vs_raw_iq_amd.constellation) pinned from several sides, and the
argument checks.  The GPU tests (test_gpu_constellation.py) compare the kernels against what is pinned here."""
import math

import numpy as np
import pytest
import torch

import constellation_ref as R


def make(**kw):
    from vit_vs_raw_iq_amd import Constellation
    args = dict(height=32, width=64, length=24)
    args.update(kw)
    return Constellation(**args)


def points(con, n, seed, margin=0.0, clear=1e-3):
    """(n, 2, len) samples whose pixel coordinates cover the image and `margin` pixels around it, none within `clear` of a
    table knot of any pixel (t = |e| * n_frac within `clear` of an integer)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-margin, con.width + margin, (n, con.length))
    v = rng.uniform(-margin, con.height + margin, (n, con.length))
    for p in (u, v):
        frac = (p - 0.5) * con.n_frac
        near = np.abs(frac - np.rint(frac)) < clear
        p[near] += 3 * clear / con.n_frac
    return np.stack([(u - con.x_off) / con.x_scale, (v - con.y_off) / con.y_scale], axis=1)


CONFIGS = {"gaussian_log": dict(profile="gaussian", sigma=1.0, mode="log"),
           "gaussian_power_wide": dict(profile="gaussian", sigma=2.5, n_frac=3, mode="power", scale=2.0, shift=-0.5),
           "triangle_power": dict(profile="triangle", mode="power"),
           "triangle_log": dict(profile="triangle", n_frac=1, mode="log", floor=1e-2)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_reference_equals_a_brute_force_loop_over_points_and_pixels(name):
    from vit_vs_raw_iq_amd import constellation_reference
    con = make(**CONFIGS[name])
    x = points(con, 2, 1, margin=6.0)
    x[0, 0, 3], x[1, 1, 5], x[1, 0, 7] = np.nan, np.inf, -np.inf
    tab = con.table.astype(np.float64)
    f32 = lambda v: float(np.float32(v))     # noqa: E731

    def w(s, scale, off, c):
        e = s * f32(scale) + f32(off) - (c + 0.5)
        t = abs(e) * con.n_frac
        if not t < con.radius * con.n_frac:
            return 0.0
        i = int(math.floor(t))
        return (t - i) * (tab[i + 1] - tab[i]) + tab[i]
    want = np.zeros((2, 1, con.height, con.width))
    for f in range(2):
        for n in range(con.length):
            a = [w(x[f, 1, n], con.y_scale, con.y_off, r) for r in range(con.height)]
            b = [w(x[f, 0, n], con.x_scale, con.x_off, c) for c in range(con.width)]
            want[f, 0] += np.outer(a, b)
    want *= f32(con.inv_norm)
    if con.mode == "log":
        want = np.log10(want + f32(con.floor))
    want = want * f32(con.scale) + f32(con.shift)
    got = constellation_reference(x, con)
    assert got.shape == want.shape and not np.isnan(got).any()
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(R.real_forward(x, con, np.float64), got, rtol=1e-13, atol=1e-15)


def torch_image(x, con):
    """The definition restated in torch fp64, differentiable in x."""
    tab = torch.from_numpy(con.table.astype(np.float64))
    f32 = lambda v: float(np.float32(v))     # noqa: E731

    def weights(s, scale, off, n_pix):
        e = (s * f32(scale) + f32(off))[..., None] - (torch.arange(n_pix, dtype=torch.float64) + 0.5)
        t = e.abs() * con.n_frac
        ok = t < con.radius * con.n_frac
        t = torch.where(ok, t, torch.zeros_like(t))
        i = t.detach().floor().long()
        return torch.where(ok, (t - i) * (tab[i + 1] - tab[i]) + tab[i], torch.zeros_like(t))
    b = weights(x[:, 0], con.x_scale, con.x_off, con.width)
    a = weights(x[:, 1], con.y_scale, con.y_off, con.height)
    V = (a.transpose(1, 2) @ b) * f32(con.inv_norm)
    v = torch.log10(V + f32(con.floor)) if con.mode == "log" else V
    return (v * f32(con.scale) + f32(con.shift))[:, None]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_reference_bwd_equals_autograd_and_central_differences(name):
    from vit_vs_raw_iq_amd import constellation_reference, constellation_reference_bwd
    con = make(**CONFIGS[name])
    x = points(con, 2, 2, margin=3.0)
    dout = np.random.default_rng(3).standard_normal((2, 1, con.height, con.width))
    got = constellation_reference_bwd(x, dout, con)
    xt = torch.from_numpy(x).requires_grad_(True)
    (torch_image(xt, con) * torch.from_numpy(dout)).sum().backward()
    scale = np.abs(got).max()
    assert scale > 0
    np.testing.assert_allclose(got, xt.grad.numpy(), rtol=1e-11, atol=1e-13 * scale)
    np.testing.assert_allclose(R.real_backward(x, dout, con, np.float64), got, rtol=1e-11, atol=1e-13 * scale)
    # central differences of the reference itself: the points stay 1e-3 / n_frac pixels clear of every knot, the step is a
    # tenth of that, so both evaluations lie on the same linear segments and only the log's curvature is left (O(h^2))
    h = 1e-4 / (con.n_frac * max(con.x_scale, con.y_scale))
    rng = np.random.default_rng(4)
    for _ in range(12):
        f, p, n = rng.integers(2), rng.integers(2), rng.integers(con.length)
        xp, xm = x.copy(), x.copy()
        xp[f, p, n] += h
        xm[f, p, n] -= h
        num = ((constellation_reference(xp, con) - constellation_reference(xm, con)) * dout).sum() / (2 * h)
        assert abs(num - got[f, p, n]) <= 1e-6 * scale, (f, p, n, num, got[f, p, n])


def test_triangle_profile_is_bilinear_binning():
    """A partition of unity: the image of an interior point sums to 1 (length 1, power mode) and its first moments over the
    pixel centres are the point's pixel coordinates."""
    from vit_vs_raw_iq_amd import constellation_reference
    con = make(length=1, profile="triangle", mode="power")
    assert con.radius == 1 and con.inv_norm == 1.0
    rng = np.random.default_rng(5)
    for _ in range(20):
        u, v = rng.uniform(0.5, con.width - 0.5), rng.uniform(0.5, con.height - 0.5)
        x = np.array([[[(u - con.x_off) / con.x_scale], [(v - con.y_off) / con.y_scale]]])
        img = constellation_reference(x, con)[0, 0]
        assert (img > 0).sum() <= 4
        np.testing.assert_allclose(img.sum(), 1.0, rtol=1e-12)
        np.testing.assert_allclose((img.sum(axis=0) * (np.arange(con.width) + 0.5)).sum(), u, rtol=1e-6)
        np.testing.assert_allclose((img.sum(axis=1) * (np.arange(con.height) + 0.5)).sum(), v, rtol=1e-6)


def test_a_gaussian_point_sums_to_one_over_length():
    from vit_vs_raw_iq_amd import constellation_reference
    con = make(length=7, mode="power")
    x = np.full((1, 2, 7), np.nan)
    x[0, :, 2] = 0.123, -0.456
    np.testing.assert_allclose(constellation_reference(x, con).sum(), 1.0 / 7, rtol=2e-3)


@pytest.mark.parametrize("name", list(R.EXACT))
def test_int64_evaluation_equals_the_fp64_definition(name):
    from vit_vs_raw_iq_amd import constellation_reference, constellation_reference_bwd
    case = R.int_case(name)
    con = R.as_constellation(case)
    want, bound = R.int_forward(case)
    dx, bound_dx = R.int_backward(case)
    assert 0 < bound < 2 ** 24 and bound_dx < 2 ** 24
    assert np.array_equal(constellation_reference(case["x"], con), want.astype(np.float64))
    assert np.array_equal(constellation_reference_bwd(case["x"], case["dout"], con), dx.astype(np.float64))
    if "nonfinite" in name:
        bad = ~np.isfinite(case["x"]).all(axis=1)
        assert bad.sum() > 10 and np.all(dx.transpose(0, 2, 1)[bad] == 0)


def test_gaussian_table_is_monotone_and_ends_in_zero():
    for sigma, n_frac in ((1.0, 8), (0.5, 1), (3.0, 64), (10.0, 4)):
        con = make(sigma=sigma, n_frac=n_frac)
        assert con.radius == min(16, math.ceil(4 * sigma)) and con.table.dtype == np.float32
        assert con.table.shape == (con.radius * n_frac + 1,) and con.table[0] == 1.0 and con.table[-1] == 0.0
        assert np.all(np.diff(con.table) <= 0) and np.all(con.table[:-1] > 0)
    tri = make(profile="triangle", n_frac=4)
    assert np.array_equal(tri.table, np.array([1, 0.75, 0.5, 0.25, 0], np.float32))


def test_defaults_and_the_struct():
    con = make(height=224, width=224, length=1024)
    assert (con.x_scale, con.x_off, con.y_scale, con.y_off) == (224 / 6.0, 112.0, 224 / 6.0, 112.0)
    assert con.n_fft == 224 and con.mode == "log" and con.radius == 4 and con.n_frac == 8
    taps = con.table.astype(np.float64)[::8]
    s = taps[0] + 2 * taps[1:].sum()
    assert con.inv_norm == 1.0 / (1024 * s * s) and con.floor == con.inv_norm / 10
    p = con.struct()
    assert (p.height, p.width, p.radius, p.n_frac, p.mode) == (224, 224, 4, 8, 1)
    assert p.x_scale == np.float32(224 / 6.0) and p.inv_norm == np.float32(con.inv_norm)
    assert "Constellation(height=224, width=224, length=1024" in repr(con)
    own = make(table=[3.0, 2.0, 1.0, 0.5, 0.0], n_frac=2)
    assert own.radius == 2 and own.profile == "table"


def test_argument_checks():
    from vit_vs_raw_iq_amd import Constellation, IqError, constellation_reference, constellation_reference_bwd
    for bad in (dict(height=48), dict(width=0), dict(height=288), dict(length=0), dict(length=8193), dict(extent=0.0),
                dict(extent=float("nan")), dict(profile="box"), dict(sigma=0.0), dict(radius=0), dict(radius=17),
                dict(n_frac=0), dict(n_frac=65), dict(mode="db"), dict(floor=0.0), dict(floor=-1.0), dict(scale=float("inf")),
                dict(table=[1.0, 0.5, 0.0], n_frac=4), dict(table=[1.0, float("nan"), 0.0], n_frac=1),
                dict(table=[0.0, 0.0], n_frac=1)):
        with pytest.raises(ValueError):
            make(**bad)
    for bad in (dict(height=32.0), dict(n_frac=True), dict(scale="1")):
        with pytest.raises(TypeError):
            make(**bad)
    con = make()
    with pytest.raises(IqError, match="no CPU fallback"):
        con(torch.zeros(2, 2, 24))
    for bad in (torch.zeros(2, 2, 25), torch.zeros(2, 24), torch.zeros(2, 3, 24), np.zeros((2, 2, 24))):
        with pytest.raises(ValueError):
            con(bad)
    with pytest.raises(ValueError):
        constellation_reference(np.zeros((2, 2, 25)), con)
    with pytest.raises(ValueError):
        constellation_reference_bwd(np.zeros((2, 2, 24)), np.zeros((2, 1, 32, 32)), con)
    with pytest.raises(TypeError):
        constellation_reference(np.zeros((2, 2, 24)), object())
    with pytest.raises(TypeError):
        Constellation.for_model(torch.nn.Linear(2, 2), 24)


def test_the_front_end_argument_admits_a_constellation():
    from vit_vs_raw_iq_amd.impairments import _front_end
    con = make()
    assert _front_end(con, "vit", 24) is con and _front_end(None, "rawiq", 24) is None
    with pytest.raises(ValueError):
        _front_end(con, "rawiq", 24)
    with pytest.raises(ValueError):
        _front_end(con, "vit", 25)
    with pytest.raises(TypeError):
        _front_end(object(), "vit", 24)
