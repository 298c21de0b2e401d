"""CPU: vit_vs_raw_iq_amd.cyclic -- the host fp64 definition (cyclic_reference) pinned to an independent statement and to the
physics it is for: a direct numpy.fft evaluation with the phase reference exp(-2 pi i k j0 / Np); a tone lights one element per
channel; a rectangular-pulse signal of sps samples per symbol shows its symbol-rate line at alpha = +-Np/sps, noise does not, and
the conjugate channel separates BPSK from QPSK; the coherence does not depend on the level of the frame.  Then the
iq_cyclic_t binding against include/iqvit.h, the refusals of iq_frames_cyclic that return before any HIP call, argument
validation, the `spectrogram=` keyword of the input paths, and the shared host evaluations of tests/cyclic_ref.py against each
other."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import cyclic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iqvit.h")

# (n_fft, columns, hop, pad, length): windows over the front (negative j0) and past the end, a hop that does not divide n_fft,
# one column, the default geometry
GEOMS = [(32, 9, 5, 13, 64), (64, 7, 29, 40, 200), (96, 1, 1, 0, 100), (64, None, None, 0, 1024), (32, 20, 8, 31, 150)]


def frames(n, length, seed):
    return np.random.default_rng(seed).standard_normal((n, 2, length))


def fft_image(x, cs):
    """numpy.fft does the transform: X[t] = FFT of the windowed zero-padded slice, Y = X exp(-2 pi i k j0 / Np) with the TRUE
    (possibly negative) j0, the Gram matrices by einsum, the image element by element from the definition's index rule."""
    from vit_vs_raw_iq_amd.spectrogram import _window
    n, T = cs.n_fft, cs.columns
    w = _window(cs.window, n)
    z = x[:, 0] + 1j * x[:, 1]
    Y = np.zeros((len(x), T, n), complex)
    for t in range(T):
        j0 = t * cs.hop - cs.pad
        sl = np.zeros((len(x), n), complex)
        for m in range(n):
            if 0 <= j0 + m < cs.length:
                sl[:, m] = z[:, j0 + m]
        Y[:, t] = np.fft.fft(sl * w, axis=1) * np.exp(-2j * np.pi * np.arange(n) * j0 / n)
    S = np.einsum("btk,btl->bkl", Y, np.conj(Y))
    Sc = np.einsum("btk,btl->bkl", Y, Y)
    D = (np.abs(Y) ** 2).sum(axis=1)
    inv2 = cs.inv_norm ** 2
    chans = {"scf": [0], "conj": [1], "both": [0, 1]}[cs.kind]
    out = np.empty((len(x), len(chans), n, n))
    for ci, c in enumerate(chans):
        for rho in range(n):
            a = (rho + n // 2) % n
            for kap in range(n):
                k = (kap + n // 2) % n
                l = (a - k) % n if c else (k - a) % n
                P = np.abs((Sc if c else S)[:, k, l]) ** 2 * inv2
                if cs.mode == "power":
                    v = P
                elif cs.mode == "log":
                    v = np.log10(P + cs.floor)
                else:
                    v = P / (D[:, k] * D[:, l] * inv2 + cs.floor)
                out[:, ci, rho, kap] = v * cs.scale + cs.shift
    return out


def make(geom, **kw):
    from vit_vs_raw_iq_amd import CyclicSpectrum
    n_fft, columns, hop, pad, length = geom
    return CyclicSpectrum(n_fft, length, hop, pad, columns, **kw)


@pytest.mark.parametrize("geom", GEOMS[:3] + GEOMS[4:])
@pytest.mark.parametrize("kind,mode,window", [("both", "power", "hann"), ("scf", "coherence", "rect"), ("conj", "log", "hann")])
def test_reference_is_the_phase_referenced_fft_of_the_windowed_slices(geom, kind, mode, window):
    """Matrix products of the definition against numpy's FFT: rounding only, 1e-10 relative to the largest element (and to 1)."""
    from vit_vs_raw_iq_amd import cyclic_reference
    cs = make(geom, kind=kind, mode=mode, window=window, floor=1e-3, scale=1.5, shift=-0.25)
    assert geom[3] == 0 or (0 * cs.hop - cs.pad) < 0                    # pad > 0: window 0 starts at a negative j0
    x = frames(2, geom[4], 5)
    ref, want = cyclic_reference(x, cs), fft_image(x, cs)
    assert ref.shape == want.shape == (2, cs.channels, cs.n_fft, cs.n_fft) and ref.dtype == np.float64
    assert np.abs(ref - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


def test_default_geometry():
    from vit_vs_raw_iq_amd import CyclicSpectrum
    cs = CyclicSpectrum(64)
    assert (cs.n_fft, cs.width, cs.length, cs.hop, cs.pad, cs.columns, cs.channels) == (64, 64, 1024, 16, 0, 61, 2)
    assert (cs.kind, cs.mode, cs.window) == ("both", "coherence", "hann")
    assert (cs.columns - 1) * cs.hop + cs.n_fft <= cs.length < cs.columns * cs.hop + cs.n_fft      # every whole window, no more
    assert CyclicSpectrum(224).columns == 15 and CyclicSpectrum(64, 40).columns == 1
    assert CyclicSpectrum(32, 100, 4, 8).columns == 20                  # pad counts: windows from -8 .. 68
    assert cs.table.shape == (2, 64, 64) and cs.rot.shape == (2, 64) and cs.table.dtype == cs.rot.dtype == np.float32
    r = np.arange(64)
    assert np.array_equal(cs.rot, np.stack([np.cos(2 * np.pi * r / 64), np.sin(2 * np.pi * r / 64)]).astype(np.float32))
    assert abs(cs.inv_norm - 1.0 / (61 * 24.0)) < 1e-12                 # periodic Hann: sum w^2 = 3 n / 8
    assert "CyclicSpectrum(n_fft=64" in repr(cs) and "kind='both'" in repr(cs)
    assert CyclicSpectrum(32, kind="scf").channels == 1 and CyclicSpectrum(32, kind="conj").channels == 1


@pytest.mark.parametrize("n_fft,k0", [(32, 0), (32, 5), (64, 32), (64, 63), (96, 49)])
def test_a_tone_lights_one_element_per_channel(n_fft, k0):
    """z[j] = exp(2 pi i k0 j / Np), rect window, whole windows: X[t,k] = Np exp(2 pi i k0 j0 / Np) at k = k0 and 0 elsewhere,
    the phase reference removes the exponential, so S[k0,k0] = Sc[k0,k0] = T Np^2.  SCF: (a = 0, k = k0).  Conjugate: l = a - k
    = k0 gives a = 2 k0 mod Np.  With inv_norm = 1 / (T Np) the lit element is Np^2; everything else is rounding (1e-20 Np^2)."""
    from vit_vs_raw_iq_amd import CyclicSpectrum, cyclic_reference
    length, hop = 400, 29
    j = np.arange(length)
    z = np.exp(2j * np.pi * k0 * j / n_fft)
    cs = CyclicSpectrum(n_fft, length, hop, window="rect", mode="power")
    assert cs.columns >= 10 and abs(cs.inv_norm * cs.columns * n_fft - 1) < 1e-12
    img = cyclic_reference(np.stack([z.real, z.imag])[None], cs)[0]
    h = n_fft // 2
    col = (k0 + h) % n_fft
    for ch, a in ((0, 0), (1, (2 * k0) % n_fft)):
        row = (a + h) % n_fft
        assert np.unravel_index(img[ch].argmax(), img[ch].shape) == (row, col)
        assert abs(img[ch, row, col] - n_fft ** 2) < 1e-9 * n_fft ** 2
        rest = img[ch].copy()
        rest[row, col] = 0.0
        assert rest.max() < 1e-18 * n_fft ** 2


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_symbol_rate_line_and_the_conjugate_line_of_bpsk(seed):
    from vit_vs_raw_iq_amd import CyclicSpectrum, cyclic_reference
    cs = CyclicSpectrum(64, 1024)                                        # hop 16, Hann, both channels, squared coherence
    R.check_symbol_rate_line(cyclic_reference(R.rect_pulse_frames(seed), cs))


def test_without_the_phase_reference_the_rows_smear():
    """The same frames through the same definition with rot = (1, 0): the neighbour row of the line is no longer dark."""
    from vit_vs_raw_iq_amd import CyclicSpectrum
    cs = CyclicSpectrum(64, 1024)
    cs.rot = np.stack([np.ones(64), np.zeros(64)]).astype(np.float32)
    rows = R.real_forward(R.rect_pulse_frames(1), cs, np.float64).max(axis=3)
    assert rows[0, 0, 32 + 7] > 0.5 and rows[1, 0, 32 + 7] > 0.5


def test_coherence_does_not_depend_on_the_level_of_the_frame():
    """x -> g x multiplies P by g^4 and D[k] D[l] by g^4: only the floor breaks the ratio, by a relative floor / (D D inv2) at
    most.  With floor 1e-12 and unit-power frames (D D inv2 about 1 in band, above 1e-4 anywhere at 20 dB) that is below 1e-7."""
    from vit_vs_raw_iq_amd import CyclicSpectrum, cyclic_reference
    cs = CyclicSpectrum(64, 1024, floor=1e-12)
    x = R.rect_pulse_frames(4)
    base = cyclic_reference(x, cs)
    for g in (0.5, 3.0, 40.0):
        assert np.abs(cyclic_reference(g * x, cs) - base).max() < 1e-7
    # power mode scales with g^4
    cs = CyclicSpectrum(64, 1024, mode="power")
    np.testing.assert_allclose(cyclic_reference(2.0 * x, cs), 16.0 * cyclic_reference(x, cs), rtol=1e-12)


def test_cyclic_struct_matches_the_header_and_the_symbol_is_exported():
    import vit_vs_raw_iq_amd._native as N
    src = open(HEADER).read()
    body = re.search(r"typedef struct iq_cyclic \{(.*?)\}", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip()
              for part in decl.split(",")]
    S = N.Cyclic
    assert fields == [f[0] for f in S._fields_] == ["n_fft", "hop", "pad", "columns", "kind", "mode", "inv_norm", "floor", "scale",
                                                    "shift"]
    assert ctypes.sizeof(S) == 40 and [getattr(S, f).offset for f in fields] == list(range(0, 40, 4))
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"\biq_frames_cyclic\(([^)]*)\)", plain).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["iq_frames_cyclic"][1]) == 8
    assert N.lib().iq_frames_cyclic is not None
    from vit_vs_raw_iq_amd import CyclicSpectrum
    par = CyclicSpectrum(96, 500, 7, 3, 11, kind="conj", mode="log", floor=0.5, scale=2.0, shift=-1.0).struct()
    assert (par.n_fft, par.hop, par.pad, par.columns, par.kind, par.mode) == (96, 7, 3, 11, 1, 1)
    assert (par.floor, par.scale, par.shift) == (0.5, 2.0, -1.0)


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    cases = R.refusal_calls(L, a)
    assert len(cases) > 50
    for what, run, expect in cases:
        assert run() == expect, what


def test_cyclic_spectrum_validates_its_arguments_before_any_device_work():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import CyclicSpectrum, cyclic_reference
    bad = [
        (ValueError, dict(n_fft=0)), (ValueError, dict(n_fft=48)), (ValueError, dict(n_fft=288)), (TypeError, dict(n_fft=32.0)),
        (TypeError, dict(n_fft=True)), (ValueError, dict(length=0)), (ValueError, dict(length=8193)), (ValueError, dict(hop=0)),
        (TypeError, dict(hop=1.5)), (ValueError, dict(pad=-1)), (TypeError, dict(pad=2.0)), (ValueError, dict(columns=0)),
        (TypeError, dict(columns=3.0)), (ValueError, dict(window="hamming")), (ValueError, dict(kind="scf+conj")),
        (ValueError, dict(kind=2)), (ValueError, dict(mode="db")), (ValueError, dict(floor=0.0)), (ValueError, dict(floor=-1e-3)),
        (ValueError, dict(floor=1e-60)), (ValueError, dict(floor=float("nan"))), (TypeError, dict(floor="1e-3")),
        (ValueError, dict(scale=float("inf"))), (TypeError, dict(scale=None)), (ValueError, dict(shift=float("nan"))),
        (TypeError, dict(shift=True)),
    ]
    for exc, kw in bad:
        args = dict(n_fft=32)
        args.update(kw)
        with pytest.raises(exc):
            CyclicSpectrum(**args)
    cs = CyclicSpectrum(32, 128)
    for x in (torch.zeros(2, 128, 2), torch.zeros(2, 2, 100), torch.zeros(2, 128), np.zeros((2, 2, 128)), None):
        with pytest.raises(ValueError):
            cs(x)
    with pytest.raises(P.IqError):
        cs(torch.zeros(2, 2, 128))                                        # a CPU tensor: no CPU path
    with pytest.raises(P.IqError):
        cs.fit(torch.zeros(2, 2, 128))
    with pytest.raises(ValueError):
        cs.fit(torch.zeros(2, 2, 64))
    with pytest.raises(ValueError):
        cyclic_reference(np.zeros((2, 2, 100)), cs)
    with pytest.raises(TypeError):
        cyclic_reference(np.zeros((2, 2, 128)), None)
    with pytest.raises(TypeError):
        cyclic_reference(np.zeros((2, 2, 128)), P.Spectrogram(32, 64, 128))


def fake_vit(in_channels, h, w):
    return types.SimpleNamespace(encoder=types.SimpleNamespace(_geom=dict(kind=0, in_channels=in_channels, img_h=h, img_w=w)))


def test_for_model_takes_a_square_image_of_one_or_two_channels():
    from vit_vs_raw_iq_amd import CyclicSpectrum
    two = CyclicSpectrum.for_model(fake_vit(2, 64, 64), 1024, mode="log")
    assert (two.n_fft, two.width, two.length, two.kind, two.channels, two.mode) == (64, 64, 1024, "both", 2, "log")
    one = CyclicSpectrum.for_model(fake_vit(1, 96, 96), 512)
    assert (one.n_fft, one.length, one.kind, one.channels) == (96, 512, "scf", 1)
    assert CyclicSpectrum.for_model(fake_vit(1, 32, 32), kind="conj").kind == "conj"
    for model in (fake_vit(1, 32, 64), fake_vit(3, 64, 64), fake_vit(2, 48, 48)):
        with pytest.raises(ValueError):
            CyclicSpectrum.for_model(model, 1024)
    with pytest.raises(ValueError):
        CyclicSpectrum.for_model(fake_vit(2, 64, 64), kind="scf")
    with pytest.raises(ValueError):
        CyclicSpectrum.for_model(fake_vit(1, 64, 64), kind="both")
    with pytest.raises(TypeError):
        CyclicSpectrum.for_model(types.SimpleNamespace(_geom=dict(kind=1)), 1024)
    with pytest.raises(TypeError):
        CyclicSpectrum.for_model(object())


def test_the_input_paths_take_a_cyclic_spectrum_where_they_take_a_spectrogram():
    """Construction only (no device): the geometry comes from n_fft / width, the layout must be 'vit', the lengths must agree, and
    what is neither front end is refused with the message the paths always gave."""
    from vit_vs_raw_iq_amd import CyclicSpectrum, FrameSynth, SynthStream, data as D
    from vit_vs_raw_iq_amd.impairments import _front_end
    stats = {"i_mean": 0.0, "i_std": 1.0, "q_mean": 0.0, "q_std": 1.0}
    cs = CyclicSpectrum(64, 1024)
    assert _front_end(cs, "vit", 1024) is cs and _front_end(None, "rawiq", 1024) is None
    with pytest.raises(ValueError, match="layout must be 'vit'"):
        D.DeviceInputPipeline(stats, "rawiq", batch=4, spectrogram=cs)              # refused before any device work
    with pytest.raises(ValueError, match="layout must be 'vit'"):
        _front_end(cs, "rawiq", 1024)
    with pytest.raises(ValueError, match="1024 samples, these have 512"):
        _front_end(cs, "vit", 512)
    with pytest.raises(TypeError, match="spectrogram must be a Spectrogram or None, got int"):
        _front_end(3, "vit", 1024)
    fs = FrameSynth(["BPSK", "QPSK"], snrs_db=(10.0,), length=1024, seed=1, device="cpu")
    st = SynthStream(fs, stats, "vit", 4, spectrogram=cs)
    assert (st.take, st.h, st.w) == (1024, 64, 64)
    with pytest.raises(ValueError):
        SynthStream(fs, stats, "rawiq", 4, spectrogram=cs)


# (n_fft, columns, hop, pad, length, n_frames): the geometries of the GPU file's exact cases lie in cyclic_ref.int_case's range
@pytest.mark.parametrize("geom", [(32, 3, 5, 7, 61, 2), (64, 33, 16, 20, 301, 1), (96, 40, 29, 95, 400, 2)])
def test_shared_host_evaluations_agree_with_each_other(geom):
    """The int64 evaluation is the real-arithmetic one on integer data (float64 holds these integers exactly) and equals the
    product's complex-valued reference evaluated on the same integer tables; the real-arithmetic one in float64 is the
    reference up to the fp32 rounding of the tables."""
    from vit_vs_raw_iq_amd import CyclicSpectrum, cyclic_reference
    n_fft, columns, hop, pad, length, n = geom
    table, rot, x = R.int_case(n_fft, columns, hop, pad, length, n, seed=3)
    assert set(np.unique(table)) <= {-1, 0, 1} and np.all(np.abs(rot).sum(axis=0) == 1) and np.abs(x).max() == 1
    for kind, name in enumerate(("scf", "conj", "both")):
        want = R.int_forward(x, table, rot, (n_fft, columns, hop, pad), kind)
        assert want.dtype == np.int64 and want.shape == (n, 2 if kind == 2 else 1, n_fft, n_fft) and want.max() > 0
        cs = CyclicSpectrum(n_fft, length, hop, pad, columns, window="rect", kind=name, mode="power")
        cs.inv_norm = 1.0
        cs.table, cs.rot = table.astype(np.float32), rot.astype(np.float32)
        assert np.array_equal(R.real_forward(x, cs, np.float64), want.astype(np.float64))
        assert np.array_equal(R.real_forward(x, cs, np.float32), want.astype(np.float32))
    both = R.int_forward(x, table, rot, (n_fft, columns, hop, pad), 2)
    assert np.array_equal(both[:, :1], R.int_forward(x, table, rot, (n_fft, columns, hop, pad), 0))
    assert np.array_equal(both[:, 1:], R.int_forward(x, table, rot, (n_fft, columns, hop, pad), 1))
    # real tables: the float64 restatement against the complex-valued definition
    for mode in ("power", "log", "coherence"):
        cs = CyclicSpectrum(n_fft, length, hop, pad, columns, mode=mode, floor=1e-3)
        xr = frames(n, length, 8)
        ref = cyclic_reference(xr, cs)
        assert np.abs(R.real_forward(xr, cs, np.float64) - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())
