"""Host only: the carrier recovery's fp64 definition (vit_vs_raw_iq_amd.carrier.carrier_reference / _bwd), its tables, the ctypes
binding against include/iqvit.h, every refusal of the C entry points that returns before a HIP call, and the argument checks of
Carrier and Synchronised."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(32, 32), (64, 32), (32, 96), (256, 32)]
TWO32 = 2.0 ** 32


def planar(z):
    z = np.atleast_2d(z)
    return np.stack([z.real, z.imag], axis=1)


@pytest.mark.parametrize("n1,n2", GEOMETRIES)
def test_two_stage_dft_is_the_dft(n1, n2):
    from vit_vs_raw_iq_amd.carrier import dft_reference, dft_tables
    rng = np.random.default_rng(n1 + n2)
    w = rng.standard_normal((3, n1 * n2)) + 1j * rng.standard_normal((3, n1 * n2))
    want = np.fft.fft(w)
    err = np.abs(dft_reference(w, dft_tables(n1, n2, np.float64)) - want).max()
    assert err <= 2e-11, err
    # the rounded tables: each of the n1 + n2 + 1 factors of a term carries 2^-24
    t = dft_tables(n1, n2)
    assert all(a.dtype == np.float32 for a in t) and t[0].shape == (2, n1, n1) and t[1].shape == (2, n2, n2) and t[2].shape == (2, n1 * n2)
    err32 = np.abs(dft_reference(w, t) - want).max()
    assert err32 <= 3 * 2.0 ** -24 * np.abs(w).sum(axis=1).max(), err32


def test_tables_are_exact_where_the_angle_is():
    from vit_vs_raw_iq_amd.carrier import dft_tables
    t1, t2, tw = dft_tables(64, 32)
    assert np.array_equal(t1[0, 1, [0, 16, 32, 48]], [1, 0, -1, 0]) and np.array_equal(t1[1, 1, [0, 16, 32, 48]], [0, 1, 0, -1])
    assert np.array_equal(t1[:, 3, 5], t1[:, 5, 3]) and np.array_equal(t1[0, 1, 1:], t1[0, 1, :0:-1])       # cos is even
    assert np.array_equal(tw[:, [0, 512, 1024, 1536]], [[1, 0, -1, 0], [0, 1, 0, -1]])
    for bad, exc in (((31, 32), ValueError), ((32, 288), ValueError), ((0, 32), ValueError), ((32.0, 32), TypeError)):
        with pytest.raises(exc):
            dft_tables(*bad)


def test_tone_on_a_bin_and_between_bins():
    """M = 1, a noiseless tone of len = N samples: on a bin the line is one bin wide, d = 0 and F = k / N exactly; half-way between
    two bins the two neighbours are level and d = +-0.5 from either; a quarter of a bin off, d has the offset's sign."""
    from vit_vs_raw_iq_amd import carrier_reference, dft_tables
    Nd = 1024
    t = dft_tables(32, 32)
    n = np.arange(Nd)
    bins = np.array([10.0, -200.0, 10.5, -37.5, 10.25, 9.75, -512.0])
    phase = np.array([0.3, -2.0, 1.0, 3.0, 0.0, -1.0, 0.5])
    z = np.exp(1j * (2 * np.pi * bins[:, None] * n[None, :] / Nd + phase[:, None]))
    out, est, fth, power = carrier_reference(planar(z), t, 1)
    assert power.shape == (7, Nd) and out.shape == (7, 2, Nd)
    assert np.all(np.abs(est[[0, 1, 6], 2] - bins[[0, 1, 6]]) < 1e-6)
    assert np.array_equal(fth[[0, 1, 6], 0], (bins[[0, 1, 6]] / Nd * TWO32).astype(np.int64))
    assert est[2, 2] == pytest.approx(10.5, abs=1e-6) and est[3, 2] == pytest.approx(-37.5, abs=1e-6)
    d = est[:, 2] - np.rint(est[:, 2])
    assert d[4] > 0.01 and d[5] < -0.01                      # (unpadded: the parabola under-reads a sinc^2, the sign holds)
    # TH: the phase left at n = 0 once F is taken out; exact frequency -> the tone's own phase
    assert np.all(np.abs(np.angle(np.exp(1j * (est[[0, 1, 6], 1] - phase[[0, 1, 6]])))) < 1e-6)
    assert np.allclose(est[:, 0], fth[:, 0] / TWO32) and np.allclose(est[:, 1], fth[:, 1] / TWO32 * 2 * np.pi)
    # the output's line is real and positive, and the lock quality of an exact tone is 1
    o = out[:, 0] + 1j * out[:, 1]
    assert np.all(np.abs(np.angle(o[[0, 1, 6]].sum(axis=1))) < 1e-6) and np.all(np.abs(est[[0, 1, 6], 3] - 1) < 1e-6)
    # M = 4 on a QPSK frame: the M-th-power line of the output sits at bin 0 with angle 0
    rng = np.random.default_rng(0)
    sym = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, 500)))
    zq = sym * np.exp(1j * (2 * np.pi * 0.013 * np.arange(500) + 0.7))
    outq, estq, fq, _ = carrier_reference(planar(zq), t, 4)
    oq = (outq[0, 0] + 1j * outq[0, 1]) ** 4
    assert abs(estq[0, 0] - 0.013) < 1e-4 and abs(np.angle(oq.sum())) < 1e-6 and np.argmax(np.abs(np.fft.fft(oq, 1024))) == 0
    # k_max bounds the search; the neighbours of the refinement still count
    assert carrier_reference(planar(z[:1]), t, 1, k_max=5)[1][0, 2] <= 5.5
    # interleaved layout: the same numbers
    zi = np.stack([z.real, z.imag], axis=2)
    oi, ei, fi, pi = carrier_reference(zi, t, 1, planar=False)
    assert np.array_equal(oi, out.transpose(0, 2, 1)) and np.array_equal(fi, fth) and np.array_equal(pi, power)


def test_zero_and_non_finite_frames_give_zero_estimates():
    from vit_vs_raw_iq_amd import carrier_reference, dft_tables
    t = dft_tables(32, 32)
    x = np.zeros((2, 2, 100))
    x[1, 0, 3] = np.inf
    out, est, fth, power = carrier_reference(x, t, 2)
    assert np.array_equal(fth, np.zeros((2, 2))) and np.array_equal(est[0], [0, 0, -512, 0]) and est[1, 3] == 0
    assert np.array_equal(out[0], x[0])


@pytest.mark.parametrize("is_planar", [True, False])
def test_reference_backward_is_autograd_of_the_given_formula(is_planar):
    from vit_vs_raw_iq_amd import carrier_reference, carrier_reference_bwd
    from vit_vs_raw_iq_amd.carrier import _phasor, _wrap32
    rng = np.random.default_rng(3)
    B, length = 3, 37
    shape = (B, 2, length) if is_planar else (B, length, 2)
    x = rng.standard_normal(shape)
    dout = rng.standard_normal(shape)
    fth = rng.integers(-2 ** 31, 2 ** 31, (B, 2))
    e = _phasor(_wrap32(fth[:, :1] * np.arange(length)[None, :] + fth[:, 1:]))
    xt = torch.tensor(x, requires_grad=True)
    zt = torch.complex(*(xt.unbind(1 if is_planar else 2)))
    ot = zt * torch.tensor(np.conj(e))
    out_t = torch.stack([ot.real, ot.imag], dim=1 if is_planar else 2)
    out, est, f2, power = carrier_reference(x, None, 4, planar=is_planar, fth=fth)
    assert power is None and np.array_equal(f2, fth) and np.all(np.isnan(est[:, 2:]))
    assert np.abs(out - out_t.detach().numpy()).max() < 1e-14
    (dx,) = torch.autograd.grad(out_t, xt, torch.tensor(dout))
    assert np.abs(carrier_reference_bwd(dout, fth, is_planar) - dx.numpy()).max() < 1e-14


def test_binding_struct_matches_the_header():
    import vit_vs_raw_iq_amd._native as N
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iqvit.h")).read(), flags=re.S)
    body = re.search(r"typedef struct iq_carrier \{(.*?)\}", src, flags=re.S).group(1)
    names = [w for d in body.split(";") if d.strip() for w in re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", d.strip())]
    assert names == [f[0] for f in N.Carrier._fields_]
    assert [f[1] for f in N.Carrier._fields_] == [ctypes.c_int] * 7 + [ctypes.c_void_p] * 4
    assert ctypes.sizeof(N.Carrier) == 64
    assert [getattr(N.Carrier, f).offset for f in ("order", "n1", "n2", "k_max", "refine", "planar", "mode", "t1", "t2", "tw", "fth")] \
        == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56]
    enum = re.search(r"enum \{ IQ_CR_GIVEN = (\d), IQ_CR_ESTIMATE = (\d) \}", src)
    assert [int(v) for v in enum.groups()] == [0, 1]
    for name in ("iq_frames_carrier", "iq_frames_carrier_bwd"):
        decl = re.search(r"int " + name + r"\((.*?)\);", src, flags=re.S).group(1)
        assert len(decl.split(",")) == len(N.SIGNATURES[name][1]), name
    assert len(N.SIGNATURES["iq_frames_carrier"][1]) == 9 and len(N.SIGNATURES["iq_frames_carrier_bwd"][1]) == 6


def test_every_refusal_returns_before_a_hip_call():
    """Pointers that are never dereferenced: a refusal looks at their value only."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    ARG, UNSUPPORTED = 1, 2
    A = 0x10000                                            # "an aligned pointer"
    ok = dict(order=4, n1=32, n2=32, k_max=512, refine=1, planar=1, mode=1, t1=A, t2=A, tw=A, fth=A)

    def fwd(x=A, out=A, est=A, fth_out=A, power=A, length=1000, par="ok", **fields):
        p = None if par is None else N.Carrier(**{**ok, **fields})
        return L.iq_frames_carrier(x, out, est, fth_out, power, 1, length, ctypes.byref(p) if p is not None else None, None)

    def bwd(dout=A, dx=A, length=1000, par="ok", **fields):
        p = None if par is None else N.Carrier(**{**ok, **fields})
        return L.iq_frames_carrier_bwd(dout, dx, 1, length, ctypes.byref(p) if p is not None else None, None)
    assert fwd(x=None) == ARG and fwd(out=None) == ARG and fwd(par=None) == ARG
    assert bwd(dout=None) == ARG and bwd(dx=None) == ARG and bwd(par=None) == ARG
    for call in (fwd, bwd):
        for order in (0, 3, 16, -1):
            assert call(order=order) == ARG
        assert call(refine=2) == ARG and call(refine=-1) == ARG and call(planar=2) == ARG and call(planar=-1) == ARG
        assert call(mode=2) == ARG and call(mode=-1) == ARG
        assert call(k_max=-1) == ARG and call(k_max=513) == ARG and call(length=0) == ARG and call(length=-5) == ARG
        assert call(n1=64, n2=64, k_max=2049, length=4096) == ARG
        for field in ("t1", "t2", "tw", "fth"):
            assert call(**{field: A + 2}) == ARG, field
        for n1, n2 in ((0, 32), (31, 32), (32, 48), (288, 32), (32, 16)):
            assert call(n1=n1, n2=n2, k_max=0) == UNSUPPORTED, (n1, n2)
        assert call(length=1025) == UNSUPPORTED                                     # N < len
        assert call(n1=256, n2=64, length=8192) == UNSUPPORTED                      # N > 8192
        assert call(n1=256, n2=64, length=8193) == UNSUPPORTED
    # layouts: planar frames 4-byte, interleaved 8-byte aligned
    assert fwd(x=A + 2) == ARG and fwd(out=A + 2) == ARG and bwd(dout=A + 2) == ARG and bwd(dx=A + 2) == ARG
    assert fwd(x=A + 4, planar=0) == ARG and fwd(out=A + 4, planar=0) == ARG and bwd(dout=A + 4, planar=0) == ARG
    assert fwd(est=A + 2) == ARG and fwd(fth_out=A + 2) == ARG and fwd(power=A + 2) == ARG
    # what a mode needs
    for field in ("t1", "t2", "tw"):
        assert fwd(**{field: None}) == ARG, field
    assert fwd(mode=0, fth=None, power=None) == ARG and fwd(mode=0, power=A) == ARG and bwd(fth=None) == ARG and bwd(mode=1, fth=None) == ARG
    # n_frames <= 0 is success, nothing launched; optional outputs may be NULL; GIVEN and the backward read no table
    for n in (0, -3):
        p = N.Carrier(**ok)
        assert L.iq_frames_carrier(A, A, None, None, None, n, 1000, ctypes.byref(p), None) == 0
        p = N.Carrier(**{**ok, "mode": 0, "t1": None, "t2": None, "tw": None})
        assert L.iq_frames_carrier(A, A, None, None, None, n, 1000, ctypes.byref(p), None) == 0
        assert L.iq_frames_carrier_bwd(A, A, n, 1000, ctypes.byref(p), None) == 0


def test_python_argument_checks():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import Carrier, Constellation, Synchronised, carrier_reference, carrier_reference_bwd
    from vit_vs_raw_iq_amd.carrier import default_n_dft, dft_factors
    assert [default_n_dft(v) for v in (1, 128, 512, 513, 1024, 4096, 4097, 8192)] == [1024, 1024, 1024, 2048, 2048, 8192, 8192, 8192]
    assert dft_factors(1024) == (32, 32) and dft_factors(2048) == (64, 32) and dft_factors(4096) == (64, 64) and dft_factors(8192) == (128, 64)
    assert dft_factors(3072) == (96, 32) and dft_factors(7168) == (224, 32)
    for bad in (1000, 512, 9216, 16384, 0):
        with pytest.raises(ValueError):
            dft_factors(bad)
    for kw, exc in ((dict(length=0), ValueError), (dict(length=8193), ValueError), (dict(length=8.0), TypeError),
                    (dict(length=64, order=3), ValueError), (dict(length=64, order="4"), TypeError), (dict(length=64, n_dft=1000), ValueError),
                    (dict(length=2000, n_dft=1024), ValueError), (dict(length=64, n_dft=(32, 48)), ValueError),
                    (dict(length=64, n_dft=(256, 64)), ValueError), (dict(length=64, n_dft=(32, 32, 32)), ValueError),
                    (dict(length=64, f_max=-0.1), ValueError), (dict(length=64, f_max="x"), TypeError),
                    (dict(length=64, f_max=float("nan")), ValueError), (dict(length=64, refine="yes"), TypeError),
                    (dict(length=64, layout="rawiq"), ValueError), (dict(length=64, tables=(np.zeros((2, 32, 32)),) * 2), TypeError),
                    (dict(length=64, tables=(np.zeros((2, 32, 32)), np.zeros((2, 32, 32)), np.zeros((2, 1000)))), ValueError),
                    (dict(length=64, tables=(np.zeros((2, 32, 32)), np.full((2, 32, 32), np.nan), np.zeros((2, 1024)))), ValueError)):
        with pytest.raises(exc):
            Carrier(**kw)
    cr = Carrier(500, device="cpu")
    assert (cr.order, cr.n1, cr.n2, cr.n_dft, cr.k_max, cr.refine, cr.planar) == (4, 32, 32, 1024, 512, True, 1)
    assert Carrier(500, f_max=0.02, device="cpu").k_max == 81 and Carrier(500, f_max=1.0, device="cpu").k_max == 512
    assert Carrier(500, f_max=0.0, device="cpu").k_max == 0 and Carrier(128, n_dft=(32, 96), order=2, device="cpu").n_dft == 3072
    s = cr.struct((1, 2, 3), 4, mode=0)
    assert (s.order, s.n1, s.n2, s.k_max, s.refine, s.planar, s.mode, s.t1, s.t2, s.tw, s.fth) == (4, 32, 32, 512, 1, 1, 0, 1, 2, 3, 4)
    ci = Carrier(500, layout="interleaved", device="cpu")
    with pytest.raises(ValueError, match="layout 'planar'"):
        cr(torch.zeros(3, 500, 2))
    with pytest.raises(ValueError, match="layout 'interleaved'"):
        ci(torch.zeros(3, 2, 500))
    with pytest.raises(ValueError):
        cr(np.zeros((3, 2, 500)))
    with pytest.raises(ValueError):
        cr(torch.zeros(3, 2, 501))
    with pytest.raises(TypeError, match="return_est"):
        cr(torch.zeros(3, 2, 500), return_est="yes")
    with pytest.raises(TypeError, match="integers"):
        cr(torch.zeros(3, 2, 500), fth=torch.zeros(3, 2))
    with pytest.raises(TypeError, match="integers"):
        cr(torch.zeros(3, 2, 500), fth=[[0.5, 0]] * 3)
    with pytest.raises(ValueError, match="shape"):
        cr(torch.zeros(3, 2, 500), fth=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="range"):
        cr(torch.zeros(3, 2, 500), fth=[[2 ** 32, 0]] * 3)
    with pytest.raises(ValueError, match="return_power"):
        cr(torch.zeros(3, 2, 500), fth=[[0, 0]] * 3, return_power=True)
    for c, x in ((cr, torch.zeros(3, 2, 500)), (ci, torch.zeros(3, 500, 2))):
        with pytest.raises(P.IqError, match="no CPU fallback.*carrier_reference"):
            c(x)
        with pytest.raises(P.IqError, match="carrier_reference"):
            c(x, fth=[[1, -2 ** 31]] * 3)
    # Synchronised
    con = Constellation(32, 32, 500)
    sy = Synchronised(con, cr)
    assert isinstance(sy, P.frontend.FrontEnd) and (sy.height, sy.width, sy.channels, sy.length) == (32, 32, 1, 500)
    assert sy.differentiable == con.differentiable and sy.image_shape(7) == (7, 1, 32, 32)
    assert P.frontend.front_end(sy, "vit", 500) is sy
    with pytest.raises(TypeError):
        Synchronised("con", cr)
    with pytest.raises(TypeError):
        Synchronised(con, con)
    with pytest.raises(ValueError, match="planar"):
        Synchronised(con, ci)
    with pytest.raises(ValueError, match="samples"):
        Synchronised(con, Carrier(499, device="cpu"))
    with pytest.raises(TypeError):
        sy.struct()
    with pytest.raises(P.IqError, match="carrier_reference"):
        sy(torch.zeros(3, 2, 500))
    with pytest.raises(P.IqError, match="carrier_reference"):
        sy.fit(torch.zeros(3, 2, 500))
    with pytest.raises(ValueError):
        sy(torch.zeros(3, 500, 2))
    # the definitions' own checks
    from vit_vs_raw_iq_amd import dft_tables
    t = dft_tables(32, 32)
    with pytest.raises(ValueError):
        carrier_reference(np.zeros((1, 3, 16)), t, 4)
    with pytest.raises(ValueError):
        carrier_reference(np.zeros((1, 2, 16)), t, 3)
    with pytest.raises(ValueError):
        carrier_reference(np.zeros((1, 2, 1025)), t, 4)
    with pytest.raises(ValueError):
        carrier_reference(np.zeros((1, 2, 16)), t, 4, k_max=513)
    with pytest.raises(ValueError):
        carrier_reference(np.zeros((2, 2, 16)), None, 4, fth=[[0, 0]])
    with pytest.raises(ValueError):
        carrier_reference_bwd(np.zeros((2, 16, 2)), [[0, 0]], planar=False)


def test_the_gpu_suites_inputs_are_what_its_bounds_assume():
    """tests/carrier_ref.py on the host: every real-table frame's peak leads the bins outside its neighbourhood by 2 or more, the
    derived power bound stays far below that lead, and the exact cases keep every partial sum an fp32 integer."""
    import carrier_ref as R
    from vit_vs_raw_iq_amd import carrier_reference, dft_tables
    for name, (M, B, length, (n1, n2), _) in R.REAL.items():
        assert n1 * n2 >= 2 * length
        x = R.real_case(name)
        assert x.shape == (B, 2, length) and x.dtype == np.float32
        _, est, _, power = carrier_reference(x, dft_tables(n1, n2), M, refine=False)
        assert np.all(R.peak_lead(power, est[:, 2]) >= 2), name
        dP = R.power_bound(power, R.dw_bound(R.to_complex(x), M, n1, n2))
        assert np.all(dP.max(axis=1) <= 1e-3 * power.max(axis=1)), name
    for n1, n2, length, M in ((32, 32, 1024, 2), (64, 32, 2047, 2), (32, 64, 2000, 1), (256, 32, 8192, 2)):
        tables = R.integer_tables(n1, n2, 7 * n1 + n2 + length)
        assert all(set(np.unique(t)) <= {-1.0, 0.0, 1.0} for t in tables)
        assert R.exact_partial_sum_bound(R.integer_frames(2, length, length + M), tables, M) < 2 ** 12
    P = np.zeros(1024)
    P[[0, 5, 1023]] = [16, 9, 4]
    x = R.frame_with_power(P, 32, 32)
    assert np.array_equal(carrier_reference(x, R.permutation_tables(32, 32), 1)[3][0], P)
