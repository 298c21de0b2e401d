"""CPU: vit_vs_raw_iq_amd.synth -- the iq_synth_t binding against include/iqvit.h, the refusals of iq_frames_synth that return
before any HIP call, argument validation of FrameSynth / SynthStream (raised before any device work) and the host fp64
definition `synth_reference` against the recipe of data.py for hand-written symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iqvit.h")


def drawn_rows(n, cls=0, theta=0.0):
    d = np.zeros((n, 4))
    d[:, 0], d[:, 1], d[:, 2], d[:, 3] = cls, np.nan, theta, 1.0
    return d


def test_synth_structs_match_the_header_and_the_symbol_is_exported():
    import vit_vs_raw_iq_amd._native as N
    src = open(HEADER).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\}" % struct, src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip()
                for part in decl.split(",")]

    assert fields("iq_synth_class") == [f[0] for f in N.SynthClass._fields_] == ["kind", "offset", "count"]
    assert fields("iq_synth") == [f[0] for f in N.Synth._fields_]
    assert ctypes.sizeof(N.SynthClass) == 12
    S = N.Synth
    assert ctypes.sizeof(S) == 64
    assert [getattr(S, f).offset for f in ("points", "classes", "n_classes", "snrs_db", "n_snrs", "balanced", "seed", "stream",
                                           "frame_base")] == [0, 8, 16, 24, 32, 36, 40, 48, 56]
    decl = re.search(r"\biq_frames_synth\(([^)]*)\)", re.sub(r"/\*.*?\*/", "", src, flags=re.S)).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["iq_frames_synth"][1]) == 9
    assert re.search(r"#define IQ_SITE_SYNTH 0xFFFFFFFEu", src) and re.search(r"#define IQ_SITE_IMPAIR 0xFFFFFFFFu", src)
    from vit_vs_raw_iq_amd import synth as S_
    assert int(re.search(r"#define IQ_SYNTH_MAX_CLASSES (\d+)", src).group(1)) == S_.MAX_CLASSES
    assert int(re.search(r"#define IQ_SYNTH_MAX_SNRS (\d+)", src).group(1)) == S_.MAX_SNRS
    assert N.lib().iq_frames_synth is not None


def test_frames_synth_refuses_bad_arguments_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import FrameSynth
    L = N.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(buf) + 15) // 16 * 16          # aligned host address: never dereferenced on these paths
    ARG, UNSUPPORTED = 1, 2
    fs = FrameSynth(length=64)

    def call(par="ok", raw=a, labels=a, snr=a, n=2, length=64, edit=None):
        if par == "ok":
            par = fs.struct(points=a)
        if edit:
            edit(par)
        return L.iq_frames_synth(raw, labels, snr, None, None, n, length, ctypes.byref(par) if par is not None else None, None)
    assert call(raw=None) == ARG and call(labels=None) == ARG and call(snr=None) == ARG and call(par=None) == ARG
    assert call(length=0) == ARG and call(length=-3) == ARG
    assert call(edit=lambda p: setattr(p, "n_classes", 0)) == ARG
    assert call(edit=lambda p: setattr(p, "n_classes", -1)) == ARG
    assert call(edit=lambda p: setattr(p, "points", None)) == ARG                       # the first class is a constellation
    assert call(edit=lambda p: setattr(p, "balanced", 2)) == ARG
    assert call(edit=lambda p: setattr(p, "n_snrs", -1)) == ARG
    for kind, off, count in ((3, 0, 4), (-1, 0, 4), (0, 0, 0), (0, 0, -2), (0, -1, 4)):
        cls = (N.SynthClass * 2)(N.SynthClass(1, 0, 0), N.SynthClass(kind, off, count))

        def edit(p, cls=cls):
            p.classes, p.n_classes = cls, 2
        assert call(edit=edit) == ARG, (kind, off, count)
    only_shaped = (N.SynthClass * 2)(N.SynthClass(1, 0, 0), N.SynthClass(2, 0, 0))

    def shaped(p):
        p.classes, p.n_classes, p.points = only_shaped, 2, None
    assert call(edit=shaped, n=0) == 0                                                    # no constellation: no table needed
    for bad in (float("nan"), float("inf"), -float("inf")):
        sn = (ctypes.c_float * 2)(0.0, bad)

        def edit(p, sn=sn):
            p.snrs_db, p.n_snrs = sn, 2
        assert call(edit=edit) == ARG, bad
    assert call(length=8193) == UNSUPPORTED                                               # 8 bytes per sample above 64 KB of LDS
    assert call(n=0) == 0 and call(n=-1) == 0                                             # no frames: nothing to do


def test_frame_synth_and_stream_validate_their_arguments_before_any_device_work():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import FrameSynth, Impairments, SynthStream, data as D, train_on_stream
    fs = FrameSynth(device="cpu")
    assert fs.class_names == D.CLASSES and fs.snrs_db == D.SNRS_DB and fs.length == 1024 and fs.balanced and fs.seed == 0
    assert fs.descriptors[D.CLASSES.index("GMSK")] == (1, 0, 0) and fs.descriptors[D.CLASSES.index("OQPSK")] == (2, 0, 0)
    assert fs.descriptors[0] == (0, 0, 2) and fs.descriptors[1] == (0, 2, 4)              # OOK, then 4ASK behind it
    assert fs.points.dtype == np.float32 and fs.points.shape == (sum(len(D.constellation(c)) for c in D.CLASSES[:17]), 2)
    off = fs.descriptors[D.CLASSES.index("16QAM")][1]
    c = D.constellation("16QAM")
    assert np.array_equal(fs.points[off:off + 16], np.stack([c.real, c.imag], 1).astype(np.float32))
    s = fs.struct(frame_base=2 ** 40, stream=3)
    assert (s.n_classes, s.n_snrs, s.balanced, s.seed, s.stream, s.frame_base) == (19, 4, 1, 0, 3, 2 ** 40)
    custom = FrameSynth({"ring": np.exp(2j * np.pi * np.arange(3) / 3) * 5, "GMSK": None, "pair": [1, -1]}, snrs_db=None, length=8)
    assert custom.descriptors == [(0, 0, 3), (1, 0, 0), (0, 3, 2)] and custom.snrs_db == ()
    np.testing.assert_allclose((custom.points.astype(np.float64) ** 2).sum(1), 1.0, rtol=1e-6)     # scaled to unit power
    bad = [
        (ValueError, dict(classes=[])), (ValueError, dict(classes=["QPSK", "17QAM"])), (ValueError, dict(classes=["QPSK", "QPSK"])),
        (TypeError, dict(classes=[3])), (ValueError, dict(classes={"x": []})), (ValueError, dict(classes={"x": [0, 0]})),
        (ValueError, dict(classes={"x": [1, float("nan")]})), (TypeError, dict(classes={"x": "abc"})),
        (ValueError, dict(classes=[f"c{i}" for i in range(200)])),
        (ValueError, dict(snrs_db=[0.0, float("nan")])), (ValueError, dict(snrs_db=[float("inf")])), (TypeError, dict(snrs_db=["3"])),
        (TypeError, dict(snrs_db=[True])), (ValueError, dict(snrs_db=list(range(65)))),
        (ValueError, dict(length=0)), (ValueError, dict(length=8193)), (TypeError, dict(length=12.5)),
        (ValueError, dict(seed=-1)), (ValueError, dict(seed=2 ** 64)), (TypeError, dict(balanced=2)),
    ]
    for exc, kw in bad:
        with pytest.raises(exc):
            FrameSynth(**kw)
    for kw in (dict(n=-1), dict(n=4, frame_base=-1), dict(n=4, stream=2 ** 32), dict(n=1.5)):
        with pytest.raises((ValueError, TypeError)):
            fs.generate(**kw)
    with pytest.raises(P.IqError):
        fs.generate(4)                                                                     # a CPU device: no CPU path
    st = {"i_mean": 0.0, "i_std": 1.0, "q_mean": 0.0, "q_std": 1.0}
    ok = SynthStream(fs, st, "vit", 8, h=32, w=32, stream=1, augment=Impairments.augmentation())
    assert ok.take == 512 and ok.stream == 1 and len(ok.batches(3)) == 3
    for exc, args, kw in ((TypeError, (None, st, "rawiq", 8), {}), (ValueError, (fs, st, "image", 8), {}),
                          (ValueError, (fs, st, "rawiq", 0), {}), (ValueError, (fs, st, "vit", 8), dict(h=64, w=64)),
                          (ValueError, (fs, {"i_mean": 0.0, "i_std": 0.0, "q_mean": 0.0, "q_std": 1.0}, "rawiq", 8), {}),
                          (TypeError, (fs, st, "rawiq", 8), dict(augment=0.5)), (ValueError, (fs, st, "rawiq", 8), dict(stream=-1)),
                          (ValueError, (FrameSynth(length=512, device="cpu"), st, "rawiq", 8), dict(augment=Impairments.augmentation()))):
        with pytest.raises(exc):
            SynthStream(*args, **kw)
    with pytest.raises(ValueError):
        ok.get(-1)
    with pytest.raises(TypeError):
        train_on_stream(None, fs, 3)
    with pytest.raises(ValueError):
        train_on_stream(None, ok, -1)


def test_reference_returns_the_constellation_points_for_handwritten_symbols():
    """Every point once: mean |s|^2 is 1 up to the fp32 rounding of the table (2^-24 relative per coordinate), so the frame is
    the fp32 table itself to 1e-7, and the table is data.constellation to 2^-24 of the largest coordinate."""
    from vit_vs_raw_iq_amd import FrameSynth, data as D, synth_reference
    names = ["QPSK", "16QAM", "GMSK", "64APSK"]
    fs = FrameSynth(names, snrs_db=None, length=64, device="cpu")
    for k, name in ((0, "QPSK"), (1, "16QAM"), (3, "64APSK")):
        c = D.constellation(name)
        m = len(c)
        sym = np.arange(64)[None, :] % m                      # 64 is a multiple of 4, 16 and 64: every point equally often
        got = synth_reference(sym, drawn_rows(1, cls=k), fs)
        assert got.shape == (1, 64, 2) and got.dtype == np.float64
        z = got[0, :, 0] + 1j * got[0, :, 1]
        np.testing.assert_allclose(z, c[sym[0]], rtol=0, atol=2e-7 * np.abs(c).max())
        # a carrier phase turns every point by the same angle, the power stays 1
        rot = synth_reference(sym, drawn_rows(1, cls=k, theta=0.7), fs)
        np.testing.assert_allclose(rot[0, :, 0] + 1j * rot[0, :, 1], z * np.exp(0.7j), rtol=0, atol=1e-12)
        np.testing.assert_allclose((rot ** 2).sum(2).mean(), 1.0, rtol=1e-9)
    # a frame that uses one point only is scaled to unit power, as make_dataset scales it
    c = D.constellation("16QAM")
    one = synth_reference(np.zeros((1, 64), np.int64), drawn_rows(1, cls=1), fs)
    np.testing.assert_allclose(one[0, :, 0] + 1j * one[0, :, 1], np.full(64, c[0] / abs(c[0])), rtol=0, atol=2e-7)
    for bad_sym, bad_drawn in ((np.full((1, 64), 4), drawn_rows(1, cls=0)), (np.zeros((1, 64), int), drawn_rows(1, cls=4)),
                               (np.zeros((2, 64), int), drawn_rows(1))):
        with pytest.raises(ValueError):
            synth_reference(bad_sym, bad_drawn, fs)


def test_reference_gmsk_is_the_cumulative_phase_of_the_smoothed_bits():
    """symbols[n] = M_n mod 16 with M_n = sum_{i<=n} b_i + 2 b_{i+1} + b_{i+2}: the phase pi M_n / 8 is cumsum(convolve(bits,
    [.25, .5, .25]) * pi / 2) of data._frame.  64 samples: the fp64 cumsum of the recipe drifts by less than 64 * 2^-53 * 50 rad
    = 4e-13 and the division by sqrt(1 + 1e-12) moves a unit sample by 5e-13: inside 1e-12."""
    from vit_vs_raw_iq_amd import FrameSynth, synth_reference
    fs = FrameSynth(["QPSK", "GMSK"], snrs_db=None, length=64, device="cpu")
    rng = np.random.default_rng(5)
    for _ in range(4):
        bits = rng.integers(0, 2, 64 + 2) * 2 - 1
        m = bits[:-2] + 2 * bits[1:-1] + bits[2:]
        sym = (np.cumsum(m) % 16)[None, :]
        got = synth_reference(sym, drawn_rows(1, cls=1), fs)
        recipe = np.exp(1j * np.cumsum(np.convolve(bits, [0.25, 0.5, 0.25], mode="valid") * (np.pi / 2)))
        np.testing.assert_allclose(got[0, :, 0] + 1j * got[0, :, 1], recipe, rtol=0, atol=1e-12)


@pytest.mark.parametrize("n", [64, 33])
def test_reference_oqpsk_is_the_frame_of_data_py_for_the_same_bits(n):
    """symbols[n] = 2 I + Q with I[n] = t_{n/2} and Q[n] = t_{K0 + (n+1)/2}, K0 = n/2 + 1: data._frame draws n/2 + 1 bits for I,
    then n/2 + 1 bits for Q, repeats each twice and delays Q by one sample."""
    from vit_vs_raw_iq_amd import FrameSynth, data as D, synth_reference
    fs = FrameSynth(["OQPSK"], snrs_db=None, length=n, device="cpu")

    class Bits:                                   # stands in for the generator of data._frame: hands out the given bits
        def __init__(self, t):
            self.t, self.pos = t, 0

        def integers(self, lo, hi, count):
            out = self.t[self.pos:self.pos + count]
            self.pos += count
            return out
    rng = np.random.default_rng(9)
    t = rng.integers(0, 2, 2 * (n // 2 + 1))
    k0 = n // 2 + 1
    idx = np.arange(n)
    sym = (2 * t[idx // 2] + t[k0 + (idx + 1) // 2])[None, :]
    got = synth_reference(sym, drawn_rows(1), fs)
    recipe = D._frame(Bits(t), "OQPSK", n)
    np.testing.assert_allclose(got[0, :, 0] + 1j * got[0, :, 1], recipe, rtol=0, atol=1e-12)
