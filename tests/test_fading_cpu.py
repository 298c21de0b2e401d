"""The fading channel without a GPU: the host definition on hand-checkable frames, the binding against the header, every refusal
that returns before a HIP call, the Python argument checks, the interpolation table, and the inputs of tests/test_gpu_fading.py
(the exact cases are exact in fp32; the bound follows the fp32 restatement; the bound discriminates)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import fading_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEUTRAL = dict(taps=1, rice_k_db=math.inf, sinusoids=0, doppler=0.0, clock_ppm=0.0, start=0, timing=False, K=1, n_frac=1, normalise=False)


def _los_only(B, amp=1.0, inc=0):
    paths, amps = R.tables(B)
    amps[:, 0, 0] = amp
    paths[:, 0, 0, 1] = inc
    return paths, amps


def _tone(f0, t):
    z = np.exp(2j * np.pi * f0 * np.asarray(t, np.float64))
    return np.stack([z.real, z.imag], axis=-1)


def _c(y):
    return y[..., 0] + 1j * y[..., 1]


# ---- fading_reference on frames one can check by hand
def test_a_neutral_setting_is_the_identity():
    from vit_vs_raw_iq_amd import Fading, fading_reference
    x = np.random.default_rng(0).standard_normal((3, 50, 2)).astype(np.float32)
    fd = Fading(50, 50, **NEUTRAL)
    assert (fd.los, fd.tap_sigma, fd.start, fd.drift, fd.margin()) == ((1.0,), (0.0,), 0, (0, 0), 0)
    assert np.array_equal(fd.interp, [[1.0]])
    paths, amps = _los_only(3)
    assert np.array_equal(fading_reference(x, paths, amps, R.clock_of(0, 0, 3), fd), x.astype(np.float64))


def test_a_pure_integer_delay():
    from vit_vs_raw_iq_amd import Fading, fading_reference
    x = np.random.default_rng(1).standard_normal((2, 40, 2)).astype(np.float32)
    fd = Fading(40, 40, **{**NEUTRAL, "delay": (3.0,)})
    y = fading_reference(x, *_los_only(2), R.clock_of(0, 0, 2), fd)
    assert np.array_equal(y[:, 3:], x[:, :-3].astype(np.float64)) and not y[:, :3].any()
    # the same through an odd Kaiser table: phase 0 is the unit spike
    fd9 = Fading(40, 40, **{**NEUTRAL, "delay": (3.0,), "K": 9, "n_frac": 128})
    y9 = fading_reference(x, *_los_only(2), R.clock_of(0, 0, 2), fd9)
    assert np.allclose(y9, y, rtol=0, atol=1e-15)


def test_a_half_sample_delay_of_a_tone_is_the_tone_half_a_sample_earlier():
    """K = 16, beta = 8: the windowed sinc is flat to well below 1e-3 for a tone at 0.05 cycles per sample (its transition band
    starts beyond 0.3); a wrong half sample would be off by 2 pi 0.05 / 2 = 0.157."""
    from vit_vs_raw_iq_amd import Fading, fading_reference
    f0, N = 0.05, 200
    x = _tone(f0, np.arange(N))[None].astype(np.float32)
    fd = Fading(N, N, **{**NEUTRAL, "delay": (0.5,), "K": 16, "n_frac": 256})
    y = _c(fading_reference(x, *_los_only(1), R.clock_of(0, 0), fd))[0]
    want = _c(_tone(f0, np.arange(N) - 0.5))
    err = np.abs(y - want)[16:N - 16]
    print("half-sample delay: worst error", err.max())
    assert err.max() < 1e-3


def test_a_drift_compresses_the_frequency_of_a_tone_by_S_over_2_32():
    from vit_vs_raw_iq_amd import Fading, fading_reference
    f0, N = 0.04, 400
    fd = Fading(N + 20, N, **{**NEUTRAL, "clock_ppm": 10000.0, "K": 16, "n_frac": 256, "start": 8})
    assert fd.drift == (round(0.01 * 2 ** 32),) * 2 and fd.margin() == 410 + 8 + 1 - 400      # the last read: floor(8 + 399 * 1.01) + K - 1 - c
    x = _tone(f0, np.arange(N + 20))[None].astype(np.float32)
    clock = R.clock_of(8 << 32, fd.drift[0])
    y = _c(fading_reference(x, *_los_only(1), clock, fd))[0]
    want = _c(_tone(f0, 8 + np.arange(N) * (clock[0, 1] / 2.0 ** 32)))
    err = np.abs(y - want)
    print("drift: worst error", err.max())
    # the interpolator's own error as in the half-sample test, plus the floor of the position to 1 / n_frac sample: a phase of up to
    # 2 pi f0 / n_frac.  A drift of the wrong size or sign is off by up to 2 pi f0 0.01 N = 1 radian at the end of the frame.
    assert err.max() < 1e-3 + 2 * np.pi * f0 / 256


def test_one_rotating_path_is_a_frequency_shift():
    from vit_vs_raw_iq_amd import Fading, fading_reference
    N, inc = 300, 12345678
    x = np.random.default_rng(2).standard_normal((1, N, 2)).astype(np.float32)
    fd = Fading(N, N, **NEUTRAL)
    y = _c(fading_reference(x, *_los_only(1, amp=0.5, inc=inc), R.clock_of(0, 0), fd))[0]
    want = 0.5 * _c(x.astype(np.float64))[0] * np.exp(2j * np.pi * inc * np.arange(N) / 2.0 ** 32)
    # the phase is converted to fp32 before the cosine: at most 2^-25 of half a turn = pi 2^-25 radians
    assert np.abs(y - want).max() <= np.abs(x).max() * 2 * 0.5 * np.pi * 2.0 ** -25 + 1e-15


def test_positions_in_front_of_and_beyond_the_frame_read_zero():
    from vit_vs_raw_iq_amd import Fading, fading_reference
    x = np.ones((1, 10, 2), np.float32)
    fd = Fading(10, 30, **{**NEUTRAL, "start": -7})
    y = fading_reference(x, *_los_only(1), R.clock_of(-7 << 32, 0), fd)[0]
    assert not y[:7].any() and np.array_equal(y[7:17], np.ones((10, 2))) and not y[17:].any()
    # a negative position with a fraction: the floor, not truncation (-0.5 -> m = -1, f = n_frac / 2)
    m, f = R._positions(np.array([-(1 << 31), 1 << 32]), 3, 0, 256)
    assert m.tolist() == [-1, 0, 1] and f.tolist() == [128, 128, 128]


def test_the_two_host_definitions_agree():
    from vit_vs_raw_iq_amd import Fading, fading_reference
    for name, (kw, x, paths, amps, clock, _) in R.real_cases().items():
        fd = Fading(**kw)
        y, _b = R.definition64(x, paths, amps, clock, fd)
        assert np.abs(_c(fading_reference(x, paths, amps, clock, fd)) - y).max() < 1e-12, name


# ---- the binding and the refusals
def test_binding_struct_matches_the_header():
    import vit_vs_raw_iq_amd._native as N
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iqvit.h")).read(), flags=re.S)
    body = re.search(r"typedef struct iq_fading \{(.*?)\}", src, flags=re.S).group(1)
    names = [w for d in body.split(";") if d.strip() for w in re.findall(r"([A-Za-z_][A-Za-z0-9_]*)(?:\[8\])?\s*(?:,|$)", d.strip())]
    assert names == [f[0] for f in N.Fading._fields_]
    assert ctypes.sizeof(N.Fading) == 208
    assert [getattr(N.Fading, f).offset for f in ("interp", "delay", "los", "tap_sigma", "fd_lo", "d_lo", "start", "stream", "seed",
                                                   "frame_base")] == [32, 72, 104, 136, 168, 176, 184, 188, 192, 200]
    assert [int(v) for v in re.search(r"enum \{ IQ_FADE_GIVEN = (\d), IQ_FADE_DRAWN = (\d) \}", src).groups()] == [0, 1]
    assert re.search(r"#define IQ_SITE_FADE 0xFFFFFFFDu", src)
    decl = re.search(r"int iq_frames_fade\((.*?)\);", src, flags=re.S).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["iq_frames_fade"][1]) == 9


def test_every_refusal_returns_before_a_hip_call():
    """Pointers that are never dereferenced: a refusal looks at their value only."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    ARG, UNSUPPORTED = 1, 2
    A = 0x10000
    ok = dict(mode=1, len_in=512, n_taps=2, n_sin=8, K=9, n_frac=128, normalise=1, timing=1, interp=A, snr_db=A, paths=A, amps=A,
              clock=A, fd_lo=0.0, fd_hi=0.01, d_lo=-5, d_hi=5, start=3, stream=0, seed=1, frame_base=0)
    arrays = dict(delay=[0, 70000], los=[0.9, 0.0], tap_sigma=[0.1, 0.3])

    def call(x=A, y=A, po=A, ao=A, co=A, n=1, length=512, par="ok", **fields):
        if par is None:
            return L.iq_frames_fade(x, y, po, ao, co, n, length, None, None)
        arr = {k: list(fields.pop(k, v)) for k, v in arrays.items()}
        p = N.Fading(**{**ok, **fields}, delay=(ctypes.c_int32 * 8)(*arr["delay"]), los=(ctypes.c_float * 8)(*arr["los"]),
                     tap_sigma=(ctypes.c_float * 8)(*arr["tap_sigma"]))
        return L.iq_frames_fade(x, y, po, ao, co, n, length, ctypes.byref(p), None)
    inf, nan = float("inf"), float("nan")
    assert call(x=None) == ARG and call(y=None) == ARG and call(par=None) == ARG and call(interp=None) == ARG
    assert call(mode=2) == ARG and call(mode=-1) == ARG
    for name in ("paths", "amps", "clock"):
        assert call(mode=0, **{name: None}) == ARG
    assert call(length=0) == ARG and call(length=-4) == ARG and call(len_in=0) == ARG
    assert call(n_taps=0) == ARG and call(K=0) == ARG and call(n_frac=0) == ARG and call(n_sin=-1) == ARG
    assert call(normalise=2) == ARG and call(timing=-1) == ARG
    assert call(delay=[0, -1]) == ARG
    for bad in (inf, nan, -0.5):
        assert call(los=[bad, 0.0]) == ARG and call(tap_sigma=[0.1, bad]) == ARG and call(fd_lo=bad) == ARG
    assert call(fd_hi=inf) == ARG and call(fd_hi=nan) == ARG and call(fd_hi=0.5000001) == ARG and call(fd_lo=0.02) == ARG
    assert call(d_lo=6) == ARG and call(d_lo=-2 ** 31, d_hi=2 ** 31 - 1) == ARG
    for name in ("x", "y", "po", "co"):
        assert call(**{name: A + 4}) == ARG
    assert call(ao=A + 2) == ARG and call(interp=A + 2) == ARG and call(snr_db=A + 1) == ARG
    assert call(paths=A + 4) == ARG and call(amps=A + 2) == ARG and call(clock=A + 4) == ARG
    # a bad value beyond the taps in use is not looked at
    assert call(n=0, delay=[0, 1, -1], los=[1.0, 0.0, nan]) == 0
    assert call(n_taps=9) == UNSUPPORTED and call(n_sin=33) == UNSUPPORTED and call(K=17) == UNSUPPORTED and call(n_frac=257) == UNSUPPORTED
    assert call(length=8193) == UNSUPPORTED and call(len_in=8193) == UNSUPPORTED
    assert call(n_taps=9, n_sin=-1) == ARG and call(length=8193, fd_hi=nan) == ARG           # ARG comes first
    # n_frames <= 0 is success with nothing launched; the limits themselves are supported; optional pointers may be NULL
    for n in (0, -3):
        assert call(n=n) == 0 and call(n=n, po=None, ao=None, co=None, snr_db=None, paths=None, amps=None, clock=None) == 0
        assert call(n=n, length=8192, len_in=8192, n_taps=8, n_sin=32, K=16, n_frac=256, fd_hi=0.5, delay=[0] * 8, los=[0.0] * 8,
                    tap_sigma=[0.0] * 8) == 0
        assert call(n=n, mode=0, n_sin=0, n_taps=1) == 0


def test_python_argument_checks():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import FadedSynth, Fading, ShapedSynth, fading_curve, fading_reference, interp_table
    for kw, exc in ((dict(length_in=0), ValueError), (dict(length_in=8193), ValueError), (dict(length_in=64.0), TypeError),
                    (dict(length_in=64, length_out=0), ValueError), (dict(length_in=64, taps=0), ValueError),
                    (dict(length_in=64, taps=9), ValueError), (dict(length_in=64, sinusoids=-1), ValueError),
                    (dict(length_in=64, sinusoids=33), ValueError), (dict(length_in=64, K=0), ValueError), (dict(length_in=64, K=17), ValueError),
                    (dict(length_in=64, n_frac=257), ValueError), (dict(length_in=64, timing="yes"), TypeError),
                    (dict(length_in=64, normalise=2), TypeError), (dict(length_in=64, decay=0.0), ValueError),
                    (dict(length_in=64, rice_k_db=400.0), ValueError), (dict(length_in=64, rice_k_db="6"), TypeError),
                    (dict(length_in=64, taps=2, delay=(0.0,)), ValueError), (dict(length_in=64, delay=(-1.0,)), ValueError),
                    (dict(length_in=64, delay=1.0), TypeError), (dict(length_in=64, doppler=0.6), ValueError),
                    (dict(length_in=64, doppler=-0.1), ValueError), (dict(length_in=64, doppler=(0.2, 0.1)), ValueError),
                    (dict(length_in=64, doppler=(0.1, 0.2, 0.3)), ValueError), (dict(length_in=64, doppler="fast"), TypeError),
                    (dict(length_in=64, clock_ppm=(5.0, -5.0)), ValueError), (dict(length_in=64, clock_ppm=1e6), ValueError),
                    (dict(length_in=64, clock_ppm=float("nan")), ValueError), (dict(length_in=64, start=1.5), TypeError),
                    (dict(length_in=64, interp=np.ones((3, 3))), ValueError), (dict(length_in=64, interp="table"), TypeError),
                    (dict(length_in=64, K=1, n_frac=1, interp=[[float("inf")]]), ValueError)):
        with pytest.raises(exc):
            Fading(**kw)
    fd = Fading(300, 256, taps=3, doppler=(0.0, 1e-3), clock_ppm=(-50.0, 200.0), timing=True)
    assert (fd.start, fd.drift, fd.delay_q16, fd.margin()) == (6, (-214748, 858993), (0, 65536, 131072), 11)
    assert abs(fd.los[0] ** 2 + 2 * sum(s * s for s in fd.tap_sigma) - 1.0) < 1e-12 and fd.los[1:] == (0.0, 0.0)
    ws = ShapedSynth(["BPSK", "QPSK"], snrs_db=(20.0,), length=1024, sps=2, taps=3, rice_k_db=3.0, decay=0.7, device="cpu")
    same = Fading(64, taps=3, rice_k_db=3.0, decay=0.7)
    assert np.allclose((same.los[0],) + same.tap_sigma, (ws.los,) + ws.tap_sigma, rtol=1e-15)     # a static profile carries over
    s = fd.struct(1, interp=16, seed=9, stream=2, frame_base=5)
    assert (s.mode, s.len_in, s.n_taps, s.n_sin, s.K, s.n_frac, s.normalise, s.timing, s.interp, s.d_lo, s.d_hi, s.start, s.stream, s.seed,
            s.frame_base) == (1, 300, 3, 16, 9, 128, 1, 1, 16, -214748, 858993, 6, 2, 9, 5)
    assert list(s.delay) == [0, 65536, 131072, 0, 0, 0, 0, 0] and s.snr_db is None and s.paths is None
    assert fd.replace(taps=1, doppler=0.01).doppler == (0.01, 0.01)
    with pytest.raises(TypeError, match="unknown"):
        fd.replace(speed=3)
    raw = torch.zeros(4, 300, 2)
    for bad in (torch.zeros(4, 299, 2), torch.zeros(4, 2, 300), np.zeros((4, 300, 2))):
        with pytest.raises(ValueError, match="raw"):
            fd(bad)
    with pytest.raises(ValueError, match="snr_db"):
        fd(raw, snr_db=[1.0, 2.0])
    with pytest.raises(ValueError, match="snr_db"):
        fd(raw, snr_db=float("inf"))
    with pytest.raises(TypeError, match="return_tables"):
        fd(raw, return_tables="yes")
    with pytest.raises(ValueError, match="seed"):
        fd(raw, seed=-1)
    with pytest.raises(ValueError, match="stream"):
        fd(raw, stream=2 ** 32)
    with pytest.raises(P.IqError, match="no CPU fallback.*fading_reference"):
        fd(raw, snr_db=[10.0, float("nan"), 0.0, 3.0])
    paths, amps = R.tables(4)
    with pytest.raises(ValueError, match="paths"):
        fd.given(raw, paths[:3], amps, R.clock_of(0, 0, 4))
    with pytest.raises(ValueError, match="clock"):
        fd.given(raw, paths, amps, R.clock_of(0, 0, 3))
    with pytest.raises(TypeError, match="integers"):
        fd.given(raw, paths.astype(np.float64), amps, R.clock_of(0, 0, 4))
    with pytest.raises(P.IqError, match="no CPU fallback.*fading_reference"):
        fd.given(raw, paths, amps, R.clock_of(0, 0, 4))
    with pytest.raises(TypeError, match="Fading"):
        fading_reference(raw, paths, amps, R.clock_of(0, 0, 4), ws)
    with pytest.raises(ValueError, match="paths"):
        fading_reference(raw, paths[:, :4], amps, R.clock_of(0, 0, 4), fd)
    # FadedSynth
    fs = FadedSynth(ws, Fading(1100, 1024, taps=2))
    assert isinstance(fs, ShapedSynth) and (fs.length, fs.sps, fs.span, fs.seed, fs.class_names, fs.snrs_db) == (1024, 2, 8, 0, ["BPSK", "QPSK"], (20.0,))
    assert fs._clean.length == 1100 and fs._clean.snrs_db == () and ws.length == 1024 and ws.snrs_db == (20.0,) and "FadedSynth(" in repr(fs)
    rx = P.Receiver.for_synth(fs, timing="energy", device="cpu")
    assert rx.sps == 2 and P.ReceivedSynth(fs, rx).length == 512
    with pytest.raises(ValueError, match="balanced"):
        FadedSynth(ShapedSynth(["BPSK"], length=64, balanced=False, device="cpu"), Fading(64))
    with pytest.raises(TypeError, match="ShapedSynth"):
        FadedSynth(P.FrameSynth(["BPSK"], length=64, device="cpu"), Fading(64))
    with pytest.raises(TypeError, match="ShapedSynth"):
        FadedSynth(fs, Fading(1024))
    with pytest.raises(TypeError, match="Fading"):
        FadedSynth(ws, ws)
    with pytest.raises(TypeError, match="iq_waveform_t"):
        fs.struct()
    with pytest.raises(TypeError, match="return_tables"):
        fs.generate(4, return_tables=1.5)
    with pytest.raises(ValueError):
        fs.generate(-1)
    with pytest.raises(P.IqError, match="no CPU fallback.*fading_reference"):
        fs.generate(4)
    # fading_curve
    predict, base = (lambda raw: raw[:, 0, 0].long()), Fading(1024)
    for args, exc in (((3, ws, base, "doppler", [0.0]), TypeError), ((predict, ws, ws, "doppler", [0.0]), TypeError),
                      ((predict, ws, base, "speed", [0.0]), ValueError), ((predict, ws, base, "doppler", []), ValueError),
                      ((predict, ws, base, "doppler", 0.0), TypeError), ((predict, ws, base, "doppler", [0.0, 0.7]), ValueError),
                      ((predict, base, base, "doppler", [0.0]), TypeError)):
        with pytest.raises(exc):
            fading_curve(*args)
    with pytest.raises(ValueError, match="batch"):
        fading_curve(predict, ws, base, "clock_ppm", [0.0], batch=0)
    with pytest.raises(ValueError, match="n must"):
        fading_curve(predict, ws, base, "rice_k_db", [0.0], n=0)
    with pytest.raises(P.IqError, match="fading_reference"):
        fading_curve(predict, ws, base, "rice_k_db", [0.0, math.inf], n=8)
    for bad in ((0, 8), (17, 8), (9, 0), (9, 257)):
        with pytest.raises(ValueError):
            interp_table(*bad)
    with pytest.raises(ValueError, match="beta"):
        interp_table(9, 8, beta=-1.0)


# ---- the interpolation table
@pytest.mark.parametrize("K,n_frac", [(1, 1), (2, 64), (9, 128), (16, 256), (15, 7)])
def test_interpolation_table(K, n_frac):
    from vit_vs_raw_iq_amd import interp_table
    t = interp_table(K, n_frac)
    assert t.dtype == np.float32 and t.shape == (n_frac, K)
    # every entry is rounded once (half an ulp of at most |entry|) and the fp64 rows sum to 1
    assert np.all(np.abs(t.astype(np.float64).sum(axis=1) - 1.0) <= 2.0 ** -24 * np.abs(t).astype(np.float64).sum(axis=1) + 1e-15)
    if K % 2:
        spike = np.zeros(K, np.float32)
        spike[(K - 1) // 2] = 1.0
        assert np.allclose(t[0], spike, rtol=0, atol=1e-15) and t[0, (K - 1) // 2] == 1.0
    if K == 1 and n_frac == 1:
        assert t.tolist() == [[1.0]]
    if K >= 9:                                         # it interpolates: the peak moves from tap c towards tap c + 1
        c = (K - 1) // 2
        assert t[1, c] > t[1, c + 1] > 0 and t[n_frac - 1, c + 1] > t[n_frac - 1, c] > 0


# ---- the inputs of the GPU suite
def test_the_exact_cases_are_exact_in_fp32():
    from vit_vs_raw_iq_amd import Fading, fading_reference
    seen = dict(len_out=set(), K=set(), n_frac=set(), taps=set(), ns=set(), drift=set())
    for name, (kw, x, paths, amps, clock) in R.exact_cases().items():
        fd = Fading(**kw)
        y32 = R.restate32(x, paths, amps, clock, fd)
        y64 = fading_reference(x, paths, amps, clock, fd)
        assert np.array_equal(y32.astype(np.float64), y64), name          # nothing was rounded
        assert np.abs(y64).max() < 2 ** 24 and np.array_equal(y64, np.rint(y64)) and y64.any(), name
        for k, v in (("len_out", fd.length_out), ("K", fd.K), ("n_frac", fd.n_frac), ("taps", fd.taps), ("ns", fd.sinusoids),
                     ("drift", int(np.sign(clock[0, 1] - 2 ** 32)))):
            seen[k].add(v)
        m, f = R._positions(clock[0], fd.length_out, fd.delay_q16[0], fd.n_frac)
        seen.setdefault("front", set()).add(bool((m - (fd.K - 1) // 2 < 0).any()))
        seen.setdefault("end", set()).add(bool((m + fd.K - 1 - (fd.K - 1) // 2 >= fd.length_in).any()))
        if name == "last_phase":
            assert f.max() == 255
    assert seen["len_out"] >= {1, 2, 255, 256, 257, 1001} and seen["K"] >= {1, 2, 16} and seen["n_frac"] >= {1, 256}
    assert seen["taps"] >= {1, 8} and seen["ns"] >= {0, 1, 32} and seen["drift"] == {-1, 0, 1}
    assert seen["front"] == {False, True} and seen["end"] == {False, True}


@pytest.mark.parametrize("name", list(R.real_cases()))
def test_the_bound_follows_the_fp32_restatement_and_discriminates(name):
    from vit_vs_raw_iq_amd import Fading
    kw, x, paths, amps, clock, tap = R.real_cases()[name]
    fd = Fading(**kw)
    y, bound = R.definition64(x, paths, amps, clock, fd)
    y32 = R.restate32(x, paths, amps, clock, fd)
    err = np.maximum(np.abs(y32[..., 0] - y.real), np.abs(y32[..., 1] - y.imag))
    assert np.all(err <= bound), (name, (err / bound).max())
    assert (err / bound).max() > 0.01                            # the bound is of the size of the rounding, not far above it
    wrong, _ = R.definition64(x, paths, amps, clock, fd, bump_tap=tap)
    diff = np.maximum(np.abs(wrong.real - y.real), np.abs(wrong.imag - y.imag))
    ratio = (diff / bound).max(axis=1)
    print(name, "restatement / bound", (err / bound).max(), "wrong phase / bound per frame", ratio)
    assert np.all(ratio > 4.0), (name, ratio)
