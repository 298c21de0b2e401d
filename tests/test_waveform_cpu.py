"""CPU: vit_vs_raw_iq_amd.waveform -- the iq_waveform_t binding against include/iqvit.h, the refusals of iq_frames_waveform that
return before any HIP call, the pulse tables, argument validation of ShapedSynth (raised before any device work), and the host
fp64 definition `waveform_reference`: equal to synth_reference at the identity configuration, constant envelope for GMSK, and
band-limited where a 1-sample-per-symbol frame is white."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from waveform_ref import band_edge, out_of_band_fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iqvit.h")


def drawn_rows(n, cls=0, theta=0.0, q=0):
    d = np.zeros((n, 8))
    d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4], d[:, 5] = cls, np.nan, theta, 1.0, q, 1.0
    return d


def unit_taps(n):
    t = np.zeros((n, 8, 2))
    t[:, 0, 0] = 1.0
    return t


def test_waveform_struct_matches_the_header_and_the_symbol_is_exported():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import waveform as W
    src = open(HEADER).read()
    body = re.search(r"typedef struct iq_waveform \{(.*?)\} iq_waveform_t", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in N.Waveform._fields_]
    Wf = N.Waveform
    assert [getattr(Wf, f).offset for f in ("points", "classes", "n_classes", "snrs_db", "n_snrs", "balanced", "seed", "stream",
                                            "frame_base", "sps", "span", "n_phase", "timing", "pulse", "fpulse", "n_taps", "los",
                                            "tap_sigma")] == [0, 8, 16, 24, 32, 36, 40, 48, 56, 64, 68, 72, 76, 80, 88, 96, 100, 104]
    assert ctypes.sizeof(Wf) == 136
    decl = re.search(r"\biq_frames_waveform\(([^)]*)\)", re.sub(r"/\*.*?\*/", "", src, flags=re.S)).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["iq_frames_waveform"][1]) == 10
    assert (W.MAX_SPS, W.MAX_SPAN, W.MAX_PHASE, W.MAX_TAPS) == (16, 32, 64, 8)
    assert N.lib().iq_frames_waveform is not None


def test_frames_waveform_refuses_bad_arguments_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import ShapedSynth
    L = N.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(buf) + 15) // 16 * 16          # aligned host address: never dereferenced on these paths
    ARG, UNSUPPORTED = 1, 2
    ws = ShapedSynth(length=64, sps=2, span=3, n_phase=4, taps=2, device="cpu")

    def call(par="ok", raw=a, labels=a, snr=a, drawn=None, symbols=None, taps=None, n=2, length=64, edit=None):
        if par == "ok":
            par = ws.struct(points=a, pulse=a, fpulse=a)
        if edit:
            edit(par)
        return L.iq_frames_waveform(raw, labels, snr, drawn, symbols, taps, n, length,
                                    ctypes.byref(par) if par is not None else None, None)

    def put(**kw):
        def edit(p):
            for k, v in kw.items():
                setattr(p, k, v)
        return edit
    assert call(raw=None) == ARG and call(labels=None) == ARG and call(snr=None) == ARG and call(par=None) == ARG
    assert call(length=0) == ARG and call(length=-3) == ARG
    for field in ("n_classes", "sps", "span", "n_phase", "n_taps"):
        assert call(edit=put(**{field: 0})) == ARG and call(edit=put(**{field: -1})) == ARG, field
    assert call(edit=put(classes=None)) == ARG
    assert call(edit=put(timing=2)) == ARG and call(edit=put(timing=-1)) == ARG and call(edit=put(balanced=2)) == ARG
    assert call(edit=put(n_snrs=-1)) == ARG
    assert call(edit=put(points=None)) == ARG                                            # the first class is a constellation
    assert call(edit=put(pulse=None)) == ARG                                             # ... shaped by the fp32 table
    assert call(edit=put(fpulse=None)) == ARG                                            # GMSK is among the classes
    for kind, off, count in ((3, 0, 4), (-1, 0, 4), (0, 0, 0), (0, 0, -2), (0, -1, 4)):
        cls = (N.SynthClass * 2)(N.SynthClass(1, 0, 0), N.SynthClass(kind, off, count))
        assert call(edit=put(classes=cls, n_classes=2)) == ARG, (kind, off, count)
    only_cpm = (N.SynthClass * 1)(N.SynthClass(1, 0, 0))
    assert call(edit=put(classes=only_cpm, n_classes=1, points=None, pulse=None), n=0) == 0      # CPM alone needs fpulse only
    assert call(edit=put(classes=only_cpm, n_classes=1, fpulse=None), n=0) == ARG
    only_oqpsk = (N.SynthClass * 1)(N.SynthClass(2, 0, 0))
    assert call(edit=put(classes=only_oqpsk, n_classes=1, points=None, fpulse=None), n=0) == 0
    assert call(edit=put(classes=only_oqpsk, n_classes=1, pulse=None), n=0) == ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        sn = (ctypes.c_float * 2)(0.0, bad)
        assert call(edit=put(snrs_db=sn, n_snrs=2)) == ARG, bad
        assert call(edit=put(los=bad)) == ARG, bad
        sig = (ctypes.c_float * 8)(0.1, bad)
        assert call(edit=put(tap_sigma=sig)) == ARG, bad
        assert call(edit=put(tap_sigma=sig, n_taps=1), n=0) == 0                         # beyond L: not looked at
    assert call(edit=put(tap_sigma=(ctypes.c_float * 8)(-0.1, 0.1))) == ARG
    for field in ("raw", "labels", "snr", "drawn", "symbols", "taps"):
        assert call(**{field: a + 2}) == ARG, field
    for field in ("points", "pulse", "fpulse"):
        assert call(edit=put(**{field: a + 2})) == ARG, field
    assert call(edit=put(sps=17)) == UNSUPPORTED and call(edit=put(span=33)) == UNSUPPORTED
    assert call(edit=put(n_phase=65)) == UNSUPPORTED and call(edit=put(n_taps=9)) == UNSUPPORTED
    assert call(length=8193) == UNSUPPORTED                                              # 8 bytes per sample above 64 KB of LDS
    many = (N.SynthClass * 129)(*[N.SynthClass(2, 0, 0)] * 129)
    assert call(edit=put(classes=many, n_classes=129)) == UNSUPPORTED and call(edit=put(classes=many, n_classes=128), n=0) == 0
    assert call(edit=put(snrs_db=(ctypes.c_float * 65)(), n_snrs=65)) == UNSUPPORTED
    assert call(n=0) == 0 and call(n=-1) == 0                                            # no frames: nothing to do


def test_rrc_table_is_the_pulse_at_the_stated_times():
    from vit_vs_raw_iq_amd import rrc_table
    from vit_vs_raw_iq_amd.waveform import rrc_pulse
    for alpha in (0.0, 0.2, 0.35, 1.0):
        t = rrc_table(alpha, 1, 1, 1)
        assert t.dtype == np.float32 and t.shape == (1, 1, 1)
        assert t[0, 0, 0] == np.float32(1 - alpha + 4 * alpha / np.pi)                    # p(0) / sqrt(1)
    # the removable singularity at |t| = 1 / (4 alpha): the limit continues its neighbourhood (alpha = 0.25: t = 1)
    near = rrc_pulse(np.array([1 - 1e-6, 1.0, 1 + 1e-6]), 0.25)
    assert abs(near[1] - 0.5 * (near[0] + near[2])) < 1e-9 and abs(near[0] - near[2]) < 1e-5
    # unit energy: the integral of p^2 over a long span, sampled finely
    fine = rrc_pulse(np.arange(-40 * 64, 40 * 64 + 1) / 64.0, 0.35)
    assert abs((fine ** 2).sum() / 64 - 1) < 1e-3
    for sps, span, n_phase in ((8, 8, 32), (3, 5, 7), (4, 8, 1), (1, 32, 4)):
        tab = rrc_table(0.35, sps, span, n_phase)
        assert tab.shape == (n_phase, sps, span) and tab.dtype == np.float32 and np.all(np.isfinite(tab))
        # entry [q, r, i] against the formula, evaluated the plain way
        for q, r, i in ((0, 0, 0), (n_phase - 1, sps - 1, span - 1), (n_phase // 2, sps // 2, span // 2)):
            want = rrc_pulse(np.array([(span - 1) / 2 + (r + q / n_phase) / sps - i]), 0.35)[0] / math.sqrt(sps)
            assert abs(float(tab[q, r, i]) - want) <= 1e-6, (q, r, i)
        # q = 0 is symmetric in time, exactly: p is even and mirrored times are exact negatives
        z = tab[0]
        assert np.array_equal(z[0], z[0, ::-1])
        for r in range(1, sps):
            assert np.array_equal(z[r, 1:], z[sps - r, :0:-1]), r
        # one symbol's energy is spread over its sps * span samples: unit up to the truncation of the tails
        if span >= 8 and sps >= 2:
            assert abs((tab[0].astype(np.float64) ** 2).sum() - 1) < 2e-3
    for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(sps=0), dict(sps=17), dict(span=33), dict(n_phase=65)):
        kw = dict(alpha=0.35, sps=4, span=8, n_phase=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            rrc_table(**kw)


@pytest.mark.parametrize("sps", [2, 4, 8])
def test_gmsk_table_turns_a_quarter_per_symbol(sps):
    """Each entry is rounded to an integer, at most 1/2 off: a slice of sps * span entries sums to 2^30 within sps * span / 2,
    plus what the Gaussian leaves outside 8 symbols at bt = 0.3 (s = 0.44 symbols: the tails beyond 3.5 symbols from the bit's
    edge are below 1e-14 of a quarter turn -- nothing at 2^-32 turn)."""
    from vit_vs_raw_iq_amd import gmsk_table
    span, n_phase = 8, 32
    tab = gmsk_table(0.3, sps, span, n_phase)
    assert tab.dtype == np.int32 and tab.shape == (n_phase, sps, span)
    sums = tab.astype(np.int64).reshape(n_phase, -1).sum(axis=1)
    print("max |slice sum - 2^30| =", np.abs(sums - 2 ** 30).max())
    assert np.all(np.abs(sums - 2 ** 30) <= sps * span // 2)
    assert tab.min() >= 0                                                                # the phase of a bit never turns back
    # MSK in the limit of a wide filter: a bit turns 2^30 / sps in a sample, during the sps samples it lasts, and not outside them
    wide = gmsk_table(50.0, sps, 3, 1)[0].astype(np.int64)
    # (the two samples at the bit's edges share 1 % with their neighbours at bt = 50)
    assert wide.max() <= 2 ** 30 // sps and abs(wide.sum() - 2 ** 30) <= 2 and (wide >= 0.99 * 2 ** 30 / sps).sum() == sps
    with pytest.raises(ValueError):
        gmsk_table(0.0, sps, span, n_phase)


def test_shaped_synth_validates_its_arguments_before_any_device_work():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import FrameSynth, Impairments, ShapedSynth, Spectrogram, SynthStream, data as D, rrc_table, gmsk_table
    ws = ShapedSynth(device="cpu")
    assert isinstance(ws, FrameSynth)
    assert ws.class_names == D.CLASSES and ws.snrs_db == D.SNRS_DB and ws.length == 1024 and ws.balanced and ws.seed == 0
    assert (ws.sps, ws.span, ws.n_phase, ws.timing, ws.taps) == (8, 8, 32, True, 1)
    assert ws.n_symbols == (1024 + 8) // 8 + 8
    assert np.array_equal(ws.pulse, rrc_table(0.35, 8, 8, 32)) and np.array_equal(ws.fpulse, gmsk_table(0.3, 8, 8, 32))
    np.testing.assert_allclose(ws.los, 1.0 / math.sqrt(1 + 10 ** -0.6), rtol=1e-15)
    np.testing.assert_allclose(ws.tap_sigma, [math.sqrt(1 / (2 * (10 ** 0.6 + 1)))], rtol=1e-15)
    assert "sps=8" in repr(ws) and repr(ws).startswith("ShapedSynth(")
    ch = ShapedSynth(length=33, sps=3, span=5, n_phase=7, taps=3, rice_k_db=3.0, decay=0.25, device="cpu")
    K, p = 10 ** 0.3, np.array([1, 0.25, 0.0625]) / 1.3125
    assert ch.n_symbols == (33 + 2 + 3) // 3 + 5
    np.testing.assert_allclose(ch.los, math.sqrt(p[0] * K / (K + 1)), rtol=1e-15)
    np.testing.assert_allclose(ch.tap_sigma, [math.sqrt(p[0] / (2 * (K + 1))), math.sqrt(p[1] / 2), math.sqrt(p[2] / 2)], rtol=1e-15)
    np.testing.assert_allclose(ch.los ** 2 + 2 * sum(s ** 2 for s in ch.tap_sigma), 1.0, rtol=1e-14)       # unit mean channel gain
    s = ch.struct(frame_base=2 ** 40, stream=3)
    assert (s.n_classes, s.n_snrs, s.balanced, s.stream, s.frame_base) == (19, 4, 1, 3, 2 ** 40)
    assert (s.sps, s.span, s.n_phase, s.timing, s.n_taps) == (3, 5, 7, 1, 3) and s.los == np.float32(ch.los)
    assert list(s.tap_sigma) == [np.float32(v) for v in ch.tap_sigma] + [0.0] * 5
    own = ShapedSynth(["QPSK", "GMSK"], None, 64, sps=4, span=1, n_phase=1, pulse=np.ones((1, 4, 1)),
                      fpulse=np.full((1, 4, 1), 2 ** 28), device="cpu")
    assert own.pulse.dtype == np.float32 and own.fpulse.dtype == np.int32 and own.fpulse[0, 0, 0] == 2 ** 28
    bad = [
        (ValueError, dict(sps=0)), (ValueError, dict(sps=17)), (TypeError, dict(sps=2.5)), (ValueError, dict(span=0)),
        (ValueError, dict(span=33)), (ValueError, dict(n_phase=0)), (ValueError, dict(n_phase=65)), (ValueError, dict(alpha=1.5)),
        (ValueError, dict(alpha=float("nan"))), (TypeError, dict(alpha="0.35")), (ValueError, dict(bt=0.0)), (TypeError, dict(timing=2)),
        (ValueError, dict(taps=0)), (ValueError, dict(taps=9)), (TypeError, dict(taps=True)), (ValueError, dict(rice_k_db=float("inf"))),
        (ValueError, dict(rice_k_db=4000.0)), (ValueError, dict(decay=0.0)), (ValueError, dict(decay=1.5)), (TypeError, dict(decay=None)),
        (ValueError, dict(pulse=np.ones((32, 8, 7)))), (ValueError, dict(pulse=np.full((32, 8, 8), np.nan))),
        (TypeError, dict(pulse="abc")), (ValueError, dict(fpulse=np.ones((32, 8)))), (ValueError, dict(fpulse=np.full((32, 8, 8), 0.5))),
        (ValueError, dict(fpulse=np.full((32, 8, 8), 2 ** 31))), (ValueError, dict(length=8193)), (ValueError, dict(classes=[])),
    ]
    for exc, kw in bad:
        with pytest.raises(exc):
            ShapedSynth(device="cpu", **kw)
    for kw in (dict(n=-1), dict(n=4, frame_base=-1), dict(n=4, stream=2 ** 32), dict(n=1.5)):
        with pytest.raises((ValueError, TypeError)):
            ws.generate(**kw)
    with pytest.raises(P.IqError):
        ws.generate(4)                                                                    # a CPU device: no CPU path
    st = {"i_mean": 0.0, "i_std": 1.0, "q_mean": 0.0, "q_std": 1.0}
    plain = SynthStream(ws, st, "rawiq", 8)
    aug = SynthStream(ws, st, "vit", 8, h=32, w=32, stream=1, augment=Impairments.augmentation())
    assert plain.take == 1024 and aug.take == 512 and aug.synth is ws and len(aug.batches(3)) == 3
    spec = SynthStream(ws, st, "vit", 8, spectrogram=Spectrogram(64, 64, length=1024))
    assert spec.take == 1024 and spec.h == 64


def test_reference_at_the_identity_configuration_is_synth_reference():
    """sps = span = n_phase = 1, pulse 1.0, one tap (1, 0): the same table lookup, rotation and division."""
    from vit_vs_raw_iq_amd import FrameSynth, ShapedSynth, synth_reference, waveform_reference
    names = ["QPSK", "16QAM", "64APSK"]
    fs = FrameSynth(names, snrs_db=None, length=33, device="cpu")
    ws = ShapedSynth(names, None, 33, sps=1, span=1, n_phase=1, timing=False, taps=1, pulse=np.ones((1, 1, 1)), device="cpu")
    assert ws.n_symbols == 35
    rng = np.random.default_rng(3)
    for k, count in enumerate((4, 16, 64)):
        sym = rng.integers(0, count, (2, 35))
        d = drawn_rows(2, cls=k, theta=0.7 * (k + 1))
        got = waveform_reference(sym, d, unit_taps(2), ws)
        assert got.shape == (2, 33, 2) and got.dtype == np.float64
        assert np.array_equal(got, synth_reference(sym[:, :33], d[:, :4], fs))
    for sym, d, t in ((np.full((1, 35), 4), drawn_rows(1), unit_taps(1)), (np.zeros((1, 35), int), drawn_rows(1, cls=3), unit_taps(1)),
                      (np.zeros((1, 35), int), drawn_rows(1, q=1), unit_taps(1)), (np.zeros((1, 34), int), drawn_rows(1), unit_taps(1)),
                      (np.zeros((2, 35), int), drawn_rows(1), unit_taps(2)), (np.zeros((1, 35), int), drawn_rows(1), np.zeros((1, 8)))):
        with pytest.raises(ValueError):
            waveform_reference(sym, d, t, ws)
    with pytest.raises(TypeError):
        waveform_reference(np.zeros((1, 35), int), drawn_rows(1), unit_taps(1), fs)


def test_reference_gmsk_has_a_constant_envelope_and_turns_a_quarter_per_bit():
    from vit_vs_raw_iq_amd import ShapedSynth, waveform_reference
    ws = ShapedSynth(["QPSK", "GMSK"], None, 256, sps=8, span=8, n_phase=4, device="cpu")
    rng = np.random.default_rng(4)
    bits = rng.integers(0, 2, (3, ws.n_symbols))
    for q in (0, 3):
        got = waveform_reference(bits, drawn_rows(3, cls=1, q=q), unit_taps(3), ws)
        np.testing.assert_allclose((got ** 2).sum(axis=2), 1.0, rtol=0, atol=1e-9)
    # all ones: once the pulse is full every symbol adds 2^30 (up to the table's rounding), a quarter turn over 8 samples
    ones = waveform_reference(np.ones((1, ws.n_symbols), int), drawn_rows(1, cls=1), unit_taps(1), ws)
    z = ones[0, :, 0] + 1j * ones[0, :, 1]
    np.testing.assert_allclose(np.angle(z[8:] / z[:-8]), np.pi / 2, atol=1e-6)
    # an L-tap channel is the convolution of the shaped signal: u from a one-tap source one sample longer (the same NS)
    ch = ShapedSynth(["QPSK", "GMSK"], None, 256, sps=8, span=8, n_phase=4, taps=2, device="cpu")
    one = ShapedSynth(["QPSK", "GMSK"], None, 257, sps=8, span=8, n_phase=4, taps=1, device="cpu")
    assert ch.n_symbols == one.n_symbols
    cz = lambda a: a[0, :, 0] + 1j * a[0, :, 1]                                        # noqa: E731
    t = np.zeros((1, 8, 2))
    t[0, 0], t[0, 1] = (0.8, 0.1), (-0.3, 0.4)
    for k, hi in ((0, 4), (1, 2)):
        sym = rng.integers(0, hi, (1, ch.n_symbols))
        u = cz(waveform_reference(sym, drawn_rows(1, cls=k, q=2), unit_taps(1), one))
        v = complex(*t[0, 0]) * u[1:] + complex(*t[0, 1]) * u[:-1]                          # v[n] = h_0 u[n + 1] + h_1 u[n]
        v = v * np.exp(0.4j) / np.sqrt(np.mean(np.abs(v) ** 2))
        np.testing.assert_allclose(cz(waveform_reference(sym, drawn_rows(1, cls=k, q=2, theta=0.4), t, ch)), v, rtol=0, atol=1e-9)


@pytest.mark.parametrize("sps", [2, 4, 8])
def test_reference_is_band_limited_where_one_sample_per_symbol_is_white(sps):
    """QPSK through the root-raised cosine of roll-off 0.35, 8 symbols long: at most 1e-3 of a 1024-sample frame's power lies
    beyond (1 + alpha) / (2 sps) + 4 / len (the band edge plus the main lobe of the Hann window).  The same statistic for a
    1-sample-per-symbol frame, which is white, at the edge of sps = 4 (0.17 cycles per sample: 66 % of the axis lies beyond it) is
    above one half."""
    from vit_vs_raw_iq_amd import FrameSynth, ShapedSynth, synth_reference, waveform_reference
    ws = ShapedSynth(["QPSK"], None, 1024, sps=sps, span=8, alpha=0.35, n_phase=32, device="cpu")
    rng = np.random.default_rng(sps)
    n = 8
    sym = rng.integers(0, 4, (n, ws.n_symbols))
    d = drawn_rows(n, theta=0.3)
    d[:, 4] = rng.integers(0, 32, n)
    frac = out_of_band_fraction(waveform_reference(sym, d, unit_taps(n), ws), band_edge(0.35, sps, 1024))
    fs = FrameSynth(["QPSK"], None, 1024, device="cpu")
    white = out_of_band_fraction(synth_reference(rng.integers(0, 4, (n, 1024)), d[:, :4], fs), band_edge(0.35, 4, 1024))
    print(f"sps {sps}: out-of-band share of the shaped frames max {frac.max():.3e}, of 1-sps frames min {white.min():.3f}")
    assert np.all(frac <= 1e-3), frac
    assert np.all(white > 0.5), white
