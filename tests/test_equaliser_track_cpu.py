"""Host only: the tracking equaliser's fp64 definition (vit_vs_raw_iq_amd.equaliser_track) against the method restated on plain
numpy (tests/equaliser_track_ref.py), the ctypes binding against include/iqvit.h, every refusal of the C entry points that returns
before a HIP call, the argument checks of TrackingEqualiser, the inputs of the GPU suite against what its exact cases and bounds
assume, and the method's claim on the host chain waveform_reference -> fading_reference -> receiver_reference."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import equaliser_ref as E
import equaliser_track_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_frames(B, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))


def random_taper(seg, seed):
    h = np.random.default_rng(seed).uniform(0.2, 1.0, seg)
    return h / h.sum()


@pytest.mark.parametrize("L,n,seg,hop,iters", [(1, 9, 4, 2, 2), (3, 20, 8, 3, 3), (4, 33, 16, 16, 2), (11, 70, 32, 8, 2), (5, 12, 12, 1, 3),
                                               (2, 15, 1, 1, 2), (32, 80, 40, 17, 1)])
def test_the_definition_is_the_plain_statement(L, n, seg, hop, iters):
    """numpy.correlate on the segment's tapered e, numpy.interp on every word of the weights over the centres.  The only difference
    allowed is rounding: the definition's share a is an fp32 quotient (2^-24 relative)."""
    from vit_vs_raw_iq_amd import equaliser_track_reference
    z = 0.7 * random_frames(2, n, L + n)
    h = random_taper(seg, seg)
    w0 = E.spike(2, L) + 0.1 * random_frames(2, L, L)
    for planar in (False, True):
        out, w, est = equaliser_track_reference(E.from_complex(z, planar, np.float64), L, iters, 0.05, seg, hop, h, 1.2, planar=planar, w0=w0)
        S = T.n_segments(n, seg, hop)
        assert out.shape == ((2, 2, n) if planar else (2, n, 2)) and w.shape == (2, S, L, 2) and np.array_equal(est[:, 3], [S, S])
        for b in range(2):
            y, ws = T.track_plain(z[b], L, iters, 0.05, seg, hop, h, 1.2, w0[b])
            scale = max(1.0, np.abs(ws).max())
            assert np.abs(w[b, :, :, 0] + 1j * w[b, :, :, 1] - ws).max() <= 1e-12 * scale
            assert np.abs(E.to_complex(out, planar)[b] - y).max() <= 4 * 2.0 ** -24 * scale * np.abs(z[b]).sum() / n * L
            assert abs(est[b, 1] - np.mean((np.abs(y) ** 2 - 1.2) ** 2)) <= 1e-5 * max(1.0, est[b, 1])
            assert abs(est[b, 0] - E.gradient_plain(z[b], w0[b], 1.2)[1]) <= 1e-12 * est[b, 0]
            assert abs(est[b, 2] - (np.abs(ws - w0[b]) ** 2).sum(axis=1).max()) <= 1e-12
    # with a power-of-two hop the share is exact and so is the agreement
    if hop & (hop - 1) == 0:
        out, w, _ = equaliser_track_reference(E.from_complex(z, False, np.float64), L, iters, 0.05, seg, hop, h, 1.2, w0=w0)
        y, _ = T.track_plain(z[0], L, iters, 0.05, seg, hop, h, 1.2, w0[0])
        assert np.abs(E.to_complex(out)[0] - y).max() <= 1e-12 * max(1.0, np.abs(y).max())


def test_the_weights_hold_at_both_ends_and_meet_the_segments_at_their_centres():
    from vit_vs_raw_iq_amd.equaliser_track import weights_over_time
    w = random_frames(1, 4 * 3, 1).reshape(1, 4, 3)
    seg, hop = 10, 6                                                          # centres 5, 11, 17, 23
    wt = weights_over_time(w, np.arange(-3, 40), seg, hop)[0]
    at = lambda n: wt[n + 3]                                                  # noqa: E731
    assert all(np.array_equal(at(n), w[0, 0]) for n in (-3, 0, 4, 5)) and all(np.array_equal(at(n), w[0, 3]) for n in (23, 24, 39))
    assert np.array_equal(at(11), w[0, 1]) and np.array_equal(at(17), w[0, 2])
    assert not np.array_equal(at(6), w[0, 0]) and not np.array_equal(at(22), w[0, 3])       # either side of the first and last centre
    assert np.allclose(at(8), 0.5 * (w[0, 0] + w[0, 1])) and np.allclose(at(22), w[0, 2] + 5 / 6 * (w[0, 3] - w[0, 2]), rtol=1e-7)


@pytest.mark.parametrize("L,n,seg,hop,modulus", [(1, 9, 5, 2, 1.0), (4, 30, 8, 8, 1.0), (11, 60, 32, 7, 1.32), (32, 50, 33, 17, 2.0)])
def test_g_is_a_quarter_of_autograds_gradient_of_the_tapered_segment_cost(L, n, seg, hop, modulus):
    """J_j = sum_k h[k] (|y[j hop + k]|^2 - R)^2 is real and w_j complex: torch's gradient is 2 dJ/dconj(w) = 4 g (as for the block
    cost in test_equaliser_cpu.py); every segment has its own weights and its own cost."""
    from vit_vs_raw_iq_amd import segment_step_reference
    S = T.n_segments(n, seg, hop)
    z, w = random_frames(2, n, n), 0.5 * random_frames(2, S * L, L).reshape(2, S, L)
    h = random_taper(seg, L)
    y, g, J = segment_step_reference(z, w, seg, hop, h, modulus)
    wt, zt, ht = torch.tensor(w, requires_grad=True), torch.tensor(z), torch.tensor(h)
    c = L // 2
    zp = torch.nn.functional.pad(zt, (L - 1 - c, c))
    Jt = []
    for j in range(S):
        yt = sum(wt[:, j, l:l + 1] * zp[:, L - 1 - l + j * hop:L - 1 - l + j * hop + seg] for l in range(L))
        assert np.abs(yt.detach().numpy() - y[:, j]).max() <= 1e-12
        Jt.append((ht * (yt.real ** 2 + yt.imag ** 2 - modulus) ** 2).sum(dim=1))
    Jt = torch.stack(Jt, dim=1)
    (grad,) = torch.autograd.grad(Jt.sum(), wt)
    assert np.allclose(Jt.detach().numpy(), J, rtol=1e-12)
    assert np.abs(grad.numpy() - 4.0 * g).max() <= 1e-11 * max(1.0, np.abs(g).max())


@pytest.mark.parametrize("is_planar", [True, False])
@pytest.mark.parametrize("L,n,seg,hop", [(1, 6, 3, 1), (2, 19, 8, 4), (11, 67, 32, 16), (32, 40, 40, 1), (5, 50, 7, 3)])
def test_reference_backward_is_autograd_of_the_given_filter(is_planar, L, n, seg, hop):
    from vit_vs_raw_iq_amd import equaliser_track_reference, equaliser_track_reference_bwd
    from vit_vs_raw_iq_amd.equaliser_track import weights_over_time
    rng = np.random.default_rng(L + n)
    B, S = 2, T.n_segments(n, seg, hop)
    shape = (B, 2, n) if is_planar else (B, n, 2)
    x, dout = rng.standard_normal(shape), rng.standard_normal(shape)
    w = rng.standard_normal((B, S, L, 2))
    xt = torch.tensor(x, requires_grad=True)
    zt = torch.complex(*(xt.unbind(1 if is_planar else 2)))
    wn = torch.tensor(weights_over_time(w[..., 0] + 1j * w[..., 1], np.arange(n), seg, hop))          # (B, n, L), held fixed
    c = L // 2
    zp = torch.nn.functional.pad(zt, (L - 1 - c, c))
    yt = sum(wn[:, :, l] * zp[:, L - 1 - l:L - 1 - l + n] for l in range(L))
    out_t = torch.stack([yt.real, yt.imag], dim=1 if is_planar else 2)
    out = equaliser_track_reference(x, L, 5, 0.1, seg, hop, np.ones(seg), planar=is_planar, w=w)[0]
    assert np.abs(out - out_t.detach().numpy()).max() < 1e-13 * L
    (dx,) = torch.autograd.grad(out_t, xt, torch.tensor(dout))
    assert np.abs(equaliser_track_reference_bwd(dout, w, seg, hop, is_planar) - dx.numpy()).max() < 1e-13 * L


@pytest.mark.parametrize("L,n,iters", [(1, 20, 3), (11, 300, 5), (32, 64, 2)])
def test_one_rectangular_segment_over_the_whole_frame_is_the_block_equaliser(L, n, iters):
    """seg = len, hop anything, h = 1 / len: S = 1, the segment's gradient is the frame's mean and w(n) = w_0 everywhere."""
    from vit_vs_raw_iq_amd import equaliser_reference, equaliser_track_reference
    x = E.from_complex(0.7 * random_frames(3, n, n), False, np.float64)
    for w0 in (None, E.weights(E.spike(3, L) + 0.1 * random_frames(3, L, 1)).astype(np.float64)):
        out, w, est = equaliser_track_reference(x, L, iters, 0.1, n, 1, np.full(n, 1.0 / n), 1.1, w0=w0)
        ob, wb, eb = equaliser_reference(x, L, iters, 0.1, 1.1, w0=w0)
        assert w.shape == (3, 1, L, 2) and np.abs(w[:, 0] - wb).max() <= 1e-14 and np.abs(out - ob).max() <= 1e-13
        assert np.allclose(est[:, 0], eb[:, 0], rtol=1e-13) and np.allclose(est[:, 1], eb[:, 1], rtol=1e-12) and np.all(est[:, 3] == 1)


def test_no_steps_is_the_given_filter():
    from vit_vs_raw_iq_amd import equaliser_reference, equaliser_track_reference, taper_table
    x = E.run_frames("qpsk")
    w0 = E.weights(E.spike(12, 11) + 0.2 * random_frames(12, 11, 3))
    out, w, est = equaliser_track_reference(x, 11, 0, 0.3, 128, 64, taper_table(128), w0=w0)
    ob, _, eb = equaliser_reference(x, 11, 0, 0.0, w=w0)
    assert np.array_equal(out, ob) and np.array_equal(w, np.repeat(w0[:, None].astype(np.float64), 3, axis=1))
    assert np.array_equal(est[:, 0], est[:, 1]) and np.allclose(est[:, 1], eb[:, 1], rtol=1e-14) and not est[:, 2].any()
    given = equaliser_track_reference(x, 11, 7, 0.3, 128, 64, taper_table(128), w=w)
    assert np.array_equal(given[0], out) and np.all(np.isnan(given[2][:, [0, 2]])) and np.array_equal(given[2][:, 1], est[:, 1])


def test_tapers_sum_to_one_and_have_no_zero():
    from vit_vs_raw_iq_amd import taper_table
    for seg in (1, 2, 3, 63, 64, 65, 128, 511, 512):
        for kind in ("hann", "rect"):
            h = taper_table(seg, kind)
            assert h.dtype == np.float32 and h.shape == (seg,) and np.all(h > 0) and abs(h.astype(np.float64).sum() - 1.0) < 1e-6
        assert np.array_equal(taper_table(seg, "hann"), taper_table(seg, "hann")[::-1]) or seg > 2     # symmetric (up to rounding)
    assert taper_table(1)[0] == 1.0 and np.array_equal(taper_table(4, "rect"), np.full(4, 0.25, np.float32))
    h = taper_table(128).astype(np.float64)
    assert np.allclose(h, h[::-1], rtol=1e-6) and h.argmax() in (63, 64) and h[0] < 1e-3 * h[64]


def test_binding_struct_matches_the_header():
    import vit_vs_raw_iq_amd._native as N
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iqvit.h")).read(), flags=re.S)
    body = re.search(r"typedef struct iq_equaliser_track \{(.*?)\}", src, flags=re.S).group(1)
    names = [w for d in body.split(";") if d.strip() for w in re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", d.strip())]
    assert names == [f[0] for f in N.EqualiserTrack._fields_] == ["taps", "iters", "planar", "mode", "seg", "hop", "mu", "modulus", "w", "w0", "taper"]
    assert [f[1] for f in N.EqualiserTrack._fields_] == [ctypes.c_int] * 6 + [ctypes.c_float] * 2 + [ctypes.c_void_p] * 3
    assert ctypes.sizeof(N.EqualiserTrack) == 56
    assert [getattr(N.EqualiserTrack, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48]
    enum = re.search(r"enum \{ IQ_EQT_GIVEN = (\d), IQ_EQT_CMA = (\d) \}", src)
    assert [int(v) for v in enum.groups()] == [0, 1]
    for name in ("iq_frames_equalise_track", "iq_frames_equalise_track_bwd"):
        decl = re.search(r"int " + name + r"\((.*?)\);", src, flags=re.S).group(1)
        assert len(decl.split(",")) == len(N.SIGNATURES[name][1]), name
    assert len(N.SIGNATURES["iq_frames_equalise_track"][1]) == 8 and len(N.SIGNATURES["iq_frames_equalise_track_bwd"][1]) == 6
    # the block equaliser's struct is what it was
    assert ctypes.sizeof(N.Equaliser) == 40 and [f[0] for f in N.Equaliser._fields_] == ["taps", "iters", "planar", "mode", "mu", "modulus", "w", "w0"]


def test_every_refusal_returns_before_a_hip_call():
    """Pointers that are never dereferenced: a refusal looks at their value only."""
    import vit_vs_raw_iq_amd._native as N
    lib = N.lib()
    ARG, UNSUPPORTED = 1, 2
    A = 0x10000                                            # "an aligned pointer"
    ok = dict(taps=11, iters=32, planar=0, mode=1, seg=128, hop=64, mu=0.2, modulus=1.0, w=A, w0=A, taper=A)

    def fwd(x=A, out=A, w_out=A, est=A, length=512, par="ok", **fields):
        p = None if par is None else N.EqualiserTrack(**{**ok, **fields})
        return lib.iq_frames_equalise_track(x, out, w_out, est, 1, length, ctypes.byref(p) if p is not None else None, None)

    def bwd(dout=A, dx=A, length=512, par="ok", **fields):
        p = None if par is None else N.EqualiserTrack(**{**ok, **fields})
        return lib.iq_frames_equalise_track_bwd(dout, dx, 1, length, ctypes.byref(p) if p is not None else None, None)
    assert fwd(x=None) == ARG and fwd(out=None) == ARG and fwd(par=None) == ARG
    assert bwd(dout=None) == ARG and bwd(dx=None) == ARG and bwd(par=None) == ARG
    inf, nan = float("inf"), float("nan")
    for call in (fwd, bwd):
        assert call(taps=0) == ARG and call(taps=-3) == ARG and call(length=0) == ARG and call(length=-5) == ARG and call(iters=-1) == ARG
        assert call(seg=0) == ARG and call(seg=-1) == ARG and call(hop=0) == ARG and call(hop=-2) == ARG and call(hop=129) == ARG
        assert call(length=127) == ARG and call(seg=513, hop=64, length=512) == ARG                    # len < seg
        for bad in (inf, -inf, nan):
            assert call(mu=bad) == ARG and call(modulus=bad) == ARG
        assert call(mu=-0.5) == ARG and call(mu=-1e-30) == ARG
        assert call(planar=2) == ARG and call(planar=-1) == ARG and call(mode=2) == ARG and call(mode=-1) == ARG
        assert call(w=A + 2) == ARG and call(w0=A + 1) == ARG and call(taper=A + 2) == ARG
        assert call(taps=33) == UNSUPPORTED and call(iters=4097) == UNSUPPORTED and call(length=8193) == UNSUPPORTED
        assert call(seg=513, length=1024) == UNSUPPORTED
        assert call(seg=4, hop=1, length=260) == UNSUPPORTED and call(seg=1, hop=1, length=257) == UNSUPPORTED     # 257 segments
        assert call(taps=33, iters=-1) == ARG and call(length=8193, mu=nan) == ARG and call(seg=513, hop=0, length=1024) == ARG   # ARG first
    assert fwd(x=A + 4) == ARG and fwd(out=A + 4) == ARG and bwd(dout=A + 4) == ARG and bwd(dx=A + 4) == ARG
    assert fwd(x=A + 2, planar=1) == ARG and fwd(out=A + 2, planar=1) == ARG and bwd(dout=A + 2, planar=1) == ARG
    assert fwd(w_out=A + 2) == ARG and fwd(est=A + 2) == ARG
    # what a mode needs
    assert fwd(mode=0, w=None) == ARG and bwd(w=None) == ARG and bwd(mode=1, w=None) == ARG
    assert fwd(taper=None) == ARG and fwd(w_out=None) == ARG                                            # CMA: the taper, and w_out
    # n_frames <= 0 is success, nothing launched; the limits themselves are supported; optional pointers may be NULL
    for n in (0, -3):
        for fields, length in ((dict(), 8192), (dict(taps=32, iters=4096, seg=512, hop=512), 8192), (dict(seg=1, hop=1), 256),
                               (dict(seg=4, hop=1), 259), (dict(taps=1, iters=0, mu=0.0, modulus=-1.0, planar=1), 128),
                               (dict(w=None, w0=None), 128), (dict(mode=0, w0=None, taper=None), 128)):
            p = N.EqualiserTrack(**{**ok, **fields})
            assert lib.iq_frames_equalise_track(A, A, A if p.mode else None, None, n, length, ctypes.byref(p), None) == 0, fields
        p = N.EqualiserTrack(**{**ok, "mode": 1, "w0": None, "taper": None})
        assert lib.iq_frames_equalise_track_bwd(A, A, n, 8192, ctypes.byref(p), None) == 0              # the backward needs no taper


def test_python_argument_checks():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import (Carrier, Constellation, Equaliser, ReceivedSynth, Receiver, ShapedSynth, Synchronised, TrackingEqualiser,
                                   equaliser_track_reference, equaliser_track_reference_bwd, taper_table)
    for kw, exc in ((dict(length=0), ValueError), (dict(length=8193), ValueError), (dict(length=127), ValueError),
                    (dict(length=512, seg=0), ValueError), (dict(length=1024, seg=513), ValueError), (dict(length=512, seg=8.0), TypeError),
                    (dict(length=512, hop=0), ValueError), (dict(length=512, hop=129), ValueError), (dict(length=512, hop="1"), TypeError),
                    (dict(length=512, seg=4, hop=1), ValueError),                        # 509 segments
                    (dict(length=512, track_iters=-1), ValueError), (dict(length=512, track_iters=4097), ValueError),
                    (dict(length=512, track_iters=1.5), TypeError), (dict(length=512, track_mu=-0.1), ValueError),
                    (dict(length=512, track_mu=float("nan")), ValueError), (dict(length=512, track_mu="x"), TypeError),
                    (dict(length=512, taper="hamming"), ValueError), (dict(length=512, taper=None), ValueError),
                    (dict(length=512, taps=33), ValueError), (dict(length=512, iters=-1), ValueError), (dict(length=512, layout="interleaved"), ValueError)):
        with pytest.raises(exc):
            TrackingEqualiser(**kw)
    eq = TrackingEqualiser(500)
    assert isinstance(eq, Equaliser) and (eq.taps, eq.iters, eq.mu, eq.modulus, eq.planar) == (11, 64, 0.2, 1.0, 0)
    assert (eq.seg, eq.hop, eq.track_iters, eq.track_mu, eq.taper, eq.segments) == (128, 64, 32, 0.2, "hann", 6)
    assert np.array_equal(eq.table, taper_table(128)) and "TrackingEqualiser(" in repr(eq) and "seg=128" in repr(eq)
    assert TrackingEqualiser(256, seg=1, hop=1).segments == 256 and TrackingEqualiser(8192, seg=512, hop=32).segments == 241
    s = eq.track_struct(7, 9, 11, mode=0)
    assert (s.taps, s.iters, s.planar, s.mode, s.seg, s.hop, s.w, s.w0, s.taper) == (11, 32, 0, 0, 128, 64, 7, 9, 11) and abs(s.mu - 0.2) < 1e-7
    b = eq.struct(7, 9)                                    # the parent's struct is the block descent's
    assert (b.taps, b.iters, b.w, b.w0) == (11, 64, 7, 9)
    x = torch.zeros(3, 500, 2)
    with pytest.raises(ValueError, match="layout 'frames'"):
        eq(torch.zeros(3, 2, 500))
    with pytest.raises(ValueError):
        eq(torch.zeros(3, 501, 2))
    with pytest.raises(TypeError, match="return_w"):
        eq(x, return_w="yes")
    with pytest.raises(ValueError, match="one of them"):
        eq(x, w=torch.zeros(3, 6, 11, 2), w0=torch.zeros(3, 11, 2))
    with pytest.raises(ValueError, match="shape"):
        eq(x, w=torch.zeros(3, 11, 2))                     # the block equaliser's shape is not this one's
    with pytest.raises(ValueError, match="shape"):
        eq(x, w=torch.zeros(3, 5, 11, 2))
    with pytest.raises(ValueError, match="shape"):
        eq(x, w0=torch.zeros(3, 6, 11, 2))
    with pytest.raises(TypeError, match="numbers"):
        eq(x, w=torch.zeros(3, 6, 11, 2, dtype=torch.int32))
    for kw in (dict(), dict(w=torch.zeros(3, 6, 11, 2)), dict(w=np.zeros((3, 6, 11), complex)), dict(w0=torch.zeros(3, 11, 2))):
        with pytest.raises(P.IqError, match="no CPU fallback.*equaliser_track_reference"):
            eq(x, **kw)
    # it goes wherever an Equaliser goes
    con, cr = Constellation(32, 32, 500), Carrier(500, device="cpu")
    ep = TrackingEqualiser(500, layout="planar")
    sy = Synchronised(con, cr, equaliser=ep)
    assert sy.equaliser is ep and "TrackingEqualiser" in repr(sy)
    with pytest.raises(ValueError, match="planar"):
        Synchronised(con, cr, equaliser=eq)
    with pytest.raises(P.IqError, match="equaliser_track_reference"):
        sy(torch.zeros(3, 2, 500))
    ws = ShapedSynth(["BPSK", "QPSK"], snrs_db=(20.0,), length=1024, sps=2, device="cpu")
    rx = Receiver.for_synth(ws, timing="energy", device="cpu")
    e512 = TrackingEqualiser(512)
    rs = ReceivedSynth(ws, rx, equaliser=e512, carrier=Carrier(512, layout="interleaved", device="cpu"))
    assert rs.equaliser is e512 and rs.length == 512 and "TrackingEqualiser" in repr(rs)
    with pytest.raises(ValueError, match="symbols"):
        ReceivedSynth(ws, rx, equaliser=TrackingEqualiser(1024))
    # the definitions' own checks
    h = taper_table(8)
    with pytest.raises(ValueError):
        equaliser_track_reference(np.zeros((1, 16, 3)), 3, 1, 0.1, 8, 4, h)
    with pytest.raises(ValueError):
        equaliser_track_reference(np.zeros((1, 16, 2)), 33, 1, 0.1, 8, 4, h)
    with pytest.raises(ValueError):
        equaliser_track_reference(np.zeros((1, 16, 2)), 3, 1, 0.1, 8, 9, h)        # hop > seg
    with pytest.raises(ValueError):
        equaliser_track_reference(np.zeros((1, 7, 2)), 3, 1, 0.1, 8, 4, h)         # len < seg
    with pytest.raises(ValueError):
        equaliser_track_reference(np.zeros((1, 16, 2)), 3, 1, 0.1, 8, 4, h[:7])
    with pytest.raises(ValueError):
        equaliser_track_reference(np.zeros((1, 16, 2)), 3, 1, 0.1, 8, 4, h, w=np.zeros((1, 2, 3, 2)))     # S = 3
    with pytest.raises(ValueError):
        equaliser_track_reference(np.zeros((1, 300, 2)), 3, 1, 0.1, 1, 1, np.ones(1))                       # 300 segments
    with pytest.raises(ValueError):
        equaliser_track_reference_bwd(np.zeros((2, 16, 2)), np.zeros((2, 3, 2)), 8, 4)


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU suite
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_given_cases_are_exact_in_fp32():
    """Integer frames and weights and a power-of-two hop: every word of w(n) and every term of y is a multiple of 1 / hop and the
    sums of magnitudes stay below 2^24 / hop, so every partial sum in any order is an fp32 number: the fp64 definition IS what the
    device must give, bit for bit, and the fp32 restatement of the filter agrees with it."""
    from vit_vs_raw_iq_amd import equaliser_track_reference, equaliser_track_reference_bwd
    from vit_vs_raw_iq_amd.equaliser_track import weights_over_time
    seen_S = set()
    for n, seg, hop, L in T.GIVEN_EXACT:
        assert hop & (hop - 1) == 0 and 1 <= hop <= seg <= min(n, 512)
        S = T.n_segments(n, seg, hop)
        seen_S.add(S)
        x, w = E.integer_frames(2, n, n + L), T.integer_segment_weights(2, S, L, n)
        wn = weights_over_time(w[..., 0].astype(np.float64) + 1j * w[..., 1], np.arange(n), seg, hop)
        assert np.array_equal(wn * hop, np.rint(wn * hop)) and np.abs(wn.real).max() <= 2 and 4 * L * 6 * 2 * hop < 2 ** 24
        out, w_out, est = equaliser_track_reference(x, L, 0, 0.0, seg, hop, np.ones(seg), w=w)
        assert np.array_equal(out.astype(np.float32).astype(np.float64), out) and np.array_equal(w_out, w)
        yr, yi, J = T.filter32(E.to_complex(x), w[..., 0], w[..., 1], seg, hop, 1.0)
        assert np.array_equal(yr, out[:, :, 0]) and np.array_equal(yi, out[:, :, 1])
        dx = equaliser_track_reference_bwd(x, w, seg, hop)
        assert np.array_equal(dx.astype(np.float32).astype(np.float64), dx)
    assert 1 in seen_S and 2 in seen_S and 256 in seen_S and max(c[0] for c in T.GIVEN_EXACT) == 8192
    assert {c[1] for c in T.GIVEN_EXACT} >= {1, 63, 64, 65, 511, 512} and {c[3] for c in T.GIVEN_EXACT} >= {1, 2, 11, 32}
    assert (95, 64, 32) in {c[:3] for c in T.GIVEN_EXACT} and T.n_segments(95, 64, 32) == 1 and T.n_segments(96, 64, 32) == 2
    for n, seg, hop, L in T.GIVEN_ODD_HOP:
        assert hop & (hop - 1) and T.n_segments(n, seg, hop) >= 3


@pytest.mark.parametrize("case", T.EXACT_CMA, ids=lambda c: f"len{c[0]}_seg{c[1]}_hop{c[2]}_L{c[3]}")
def test_the_restatement_on_the_integer_steps_follows_the_definition(case):
    """The fp32 restatement on the integer step cases of the GPU suite: the first step from the integer spike is exact outright
    (it IS the fp64 definition), every step moves the weights of the segments that hold an off-modulus sample, segments differ, and the restatement stays within the
    derived bound of the fp64 definition (the bound follows the restatement)."""
    from vit_vs_raw_iq_amd import equaliser_track_reference
    n, seg, hop, L, mu, R, off, seeds, steps = case
    x, h = T.exact_cma_case(n, seg, hop, L, mu, R, off, seeds)
    assert abs(h.astype(np.float64).sum() - 1.0) < 1e-6 and np.all(h > 0) and (seg < 4 or len(set(h.tolist())) > 1)
    z = E.to_complex(x)
    prev = None
    for iters in range(1, steps + 1):
        out, w, est = T.restate32(x, L, iters, mu, seg, hop, h, float(R))
        ref_out, ref_w, ref_est = equaliser_track_reference(x, L, iters, mu, seg, hop, h, float(R))
        ws = T.trajectory(z, E.spike(len(x), L), mu, float(R), iters, seg, hop, h)
        dw = sum(T.segment_step_bound(z, wt, mu, float(R), seg, hop, h) for wt in ws[:-1])
        if iters == 1:
            assert np.array_equal(w.astype(np.float64), ref_w)                 # the first step from the integer spike is exact outright
        assert np.all(np.abs(w - ref_w).max(axis=3) <= dw + 1e-300)
        moved = np.any(w != (np.repeat(E.weights(E.spike(len(x), L))[:, None], w.shape[1], axis=1) if prev is None else prev), axis=(2, 3))
        assert np.all(moved.any(axis=1)) and moved.mean() >= 0.2               # (a segment without an off-modulus sample has g = 0)
        prev = w
        assert est[:, 3].tolist() == [float(w.shape[1])] * len(x) and np.all(est[:, 2] > 0)
    if w.shape[1] > 1:
        assert np.any(w[:, 0] != w[:, -1])                                     # the segments went their own ways


@pytest.mark.parametrize("name,L,planar,seg,hop,kind", T.BOUNDED)
def test_the_bounded_runs_follow_the_restatement_and_do_not_grow_an_error(name, L, planar, seg, hop, kind):
    """GPU tests 4 and 5 on real frames: one device step may differ from the definition by segment_step_bound, and 8 steps by
    TRACK_GROWTH * 8 one-step bounds.  Here: the fp32 restatement obeys both, and the growth factor measured by injection into
    the fp64 iteration stays below half the pinned TRACK_GROWTH."""
    from vit_vs_raw_iq_amd import equaliser_track_reference, taper_table
    x = E.run_frames(name)
    z = E.to_complex(x)
    h = taper_table(seg, kind)
    w0 = T.bounded_start(name, L)
    w0c = w0[:, :, 0].astype(np.float64) + 1j * w0[:, :, 1]
    mu = float(np.float32(T.BOUNDED_MU))
    G, step = T.growth(z, w0c, mu, 1.0, T.BOUNDED_STEPS, seg, hop, h)
    print(name, "growth", G.max(), "step bound", step.max())
    assert G.max() <= T.TRACK_GROWTH / 2 and np.all(step > 0) and np.all(step < 1e-4)
    for iters in (1, T.BOUNDED_STEPS):
        _, w, _ = T.restate32(x, L, iters, mu, seg, hop, h, 1.0, w0=w0)
        ref = equaliser_track_reference(x, L, iters, mu, seg, hop, h, w0=w0)[1]
        dw = (w - ref)[..., 0] + 1j * (w - ref)[..., 1]
        if iters == 1:
            bound = T.segment_step_bound(z, np.repeat(w0c[:, None], w.shape[1], axis=1), mu, 1.0, seg, hop, h)
            assert np.all(np.abs(dw.real) <= bound) and np.all(np.abs(dw.imag) <= bound) and np.any(dw != 0)
        else:
            assert np.all(T.norm2(dw) <= T.TRACK_GROWTH * iters * step)


# ---------------------------------------------------------------------------------------------------------------------------
# the method's claim
# ---------------------------------------------------------------------------------------------------------------------------
def test_tracking_lowers_J_where_the_channel_moves_and_costs_nothing_where_it_holds_still():
    """waveform_reference -> fading_reference -> receiver_reference -> equaliser_reference (the defaults) -> equaliser_track_reference
    (the defaults) on 16 QPSK frames of 512 symbols at sps = 2 and 20 dB behind the channel of DESIGN.md's fading table (3 taps, Rice
    6 dB, decay 0.5, 16 sinusoids).  Measured on the fp64 definition:
      Doppler 3e-4 cycles per sample: median J 0.2099 after the block equaliser, 0.0865 after tracking: a gain of 0.1234.
      Doppler 0:                      median J 0.0199 after the block equaliser, 0.0169 after tracking: no loss (-0.0030).
    Asserted: half the measured gain at 3e-4, and at 0 twice the measured loss, which is none: tracking is not above the block
    equaliser's J at all."""
    from vit_vs_raw_iq_amd import TrackingEqualiser, equaliser_reference, equaliser_track_reference
    eq = TrackingEqualiser(T.FADED["symbols"])
    J = {}
    for fd in (0.0, 3e-4):
        sym = T.faded_symbols(fd)
        assert sym.shape == (T.FADED["frames"], T.FADED["symbols"], 2)
        _, w0, eb = equaliser_reference(sym, eq.taps, eq.iters, eq.mu, eq.modulus)
        _, _, et = equaliser_track_reference(sym, eq.taps, eq.track_iters, eq.track_mu, eq.seg, eq.hop, eq.table, eq.modulus, w0=w0)
        assert np.allclose(et[:, 0], eb[:, 1], rtol=1e-12)                     # est[0] is the block equaliser's J(after)
        J[fd] = (float(np.median(eb[:, 1])), float(np.median(et[:, 1])))
        print(f"Doppler {fd:g}: median J {J[fd][0]:.4f} after the block equaliser, {J[fd][1]:.4f} after tracking")
    MEASURED_GAIN, MEASURED_LOSS = 0.1234, 0.0
    assert J[3e-4][0] - J[3e-4][1] >= 0.5 * MEASURED_GAIN
    assert J[0.0][1] - J[0.0][0] <= 2.0 * MEASURED_LOSS
