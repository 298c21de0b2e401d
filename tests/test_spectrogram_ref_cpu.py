"""CPU: vit_vs_raw_iq_amd.spectrogram -- the host fp64 definition against numpy.fft, torch.stft and torch autograd, the default
geometry, the iq_spectrogram_t binding against include/iqvit.h, the refusals of iq_frames_spectrogram / _bwd that return before
any HIP call, argument validation, the `spectrogram=None` defaults of the four input paths, and the shared host evaluations of
tests/spectrogram_ref.py against each other."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import spectrogram_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iqvit.h")

# (n_fft, width, hop, pad, length): windows over both ends, hop above n_fft, one column, the two default geometries
GEOMS = [(32, 64, 16, 8, 1024), (32, 31, 4, 31, 100), (64, 5, 67, 0, 300), (96, 1, 1, 40, 100), (224, 224, 4, 46, 1024)]


def frames(n, length, seed):
    return np.random.default_rng(seed).standard_normal((n, 2, length))


def fft_image(x, spec):
    """|FFT of the windowed, zero-padded slice|^2 * inv_norm per column, rows in fftshift order: numpy.fft does the transform."""
    from vit_vs_raw_iq_amd.spectrogram import _window
    w = _window(spec.window, spec.n_fft)
    z = x[:, 0] + 1j * x[:, 1]
    out = np.empty((len(x), 1, spec.n_fft, spec.width))
    for t in range(spec.width):
        sl = np.zeros((len(x), spec.n_fft), complex)
        for m in range(spec.n_fft):
            j = t * spec.hop - spec.pad + m
            if 0 <= j < spec.length:
                sl[:, m] = z[:, j]
        X = np.fft.fftshift(np.fft.fft(sl * w, axis=1), axes=1)
        out[:, 0, :, t] = (X.real ** 2 + X.imag ** 2) * spec.inv_norm
    return out


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("window", ["hann", "rect"])
def test_reference_is_the_fft_of_the_windowed_zero_padded_slices(geom, window):
    """Power mode, scale 1, shift 0: the matrix product of the definition and numpy's FFT differ by rounding only.  Values are
    O(n_fft) at most (unit-variance samples, inv_norm = 1 / sum w^2 makes P O(1)): 1e-12 absolute."""
    from vit_vs_raw_iq_amd import Spectrogram, spectrogram_reference
    n_fft, width, hop, pad, length = geom
    spec = Spectrogram(n_fft, width, length, hop, pad, window=window, mode="power")
    x = frames(2, length, 3)
    got = spectrogram_reference(x, spec)
    assert got.shape == (2, 1, n_fft, width) and got.dtype == np.float64
    np.testing.assert_allclose(got, fft_image(x, spec), rtol=0, atol=1e-12 * max(1.0, fft_image(x, spec).max()))
    # log mode, scale and shift are the stated functions of that power
    lg = Spectrogram(n_fft, width, length, hop, pad, window=window, mode="log", floor=1e-3, scale=0.7, shift=-0.2)
    np.testing.assert_allclose(spectrogram_reference(x, lg), np.log10(fft_image(x, spec) + 1e-3) * 0.7 - 0.2, rtol=0, atol=1e-11)


@pytest.mark.parametrize("geom", GEOMS)
def test_reference_is_torch_stft_of_the_padded_signal(geom):
    from vit_vs_raw_iq_amd import Spectrogram, spectrogram_reference
    n_fft, width, hop, pad, length = geom
    spec = Spectrogram(n_fft, width, length, hop, pad, window="hann", mode="power")
    x = frames(2, length, 4)
    total = (width - 1) * hop + n_fft
    z = np.zeros((2, max(total, pad + length)), complex)
    z[:, pad:pad + length] = x[:, 0] + 1j * x[:, 1]
    S = torch.stft(torch.from_numpy(z[:, :total]), n_fft, hop_length=hop, win_length=n_fft,
                   window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64), center=False, onesided=False,
                   return_complex=True).numpy()                                   # (B, n_fft bins, width)
    assert S.shape == (2, n_fft, width)
    want = np.fft.fftshift(np.abs(S) ** 2, axes=1)[:, None] * spec.inv_norm
    np.testing.assert_allclose(spectrogram_reference(x, spec), want, rtol=0, atol=1e-10 * max(1.0, want.max()))


@pytest.mark.parametrize("geom", GEOMS[:4])
@pytest.mark.parametrize("mode", ["power", "log"])
def test_reference_backward_is_torch_autograd_of_the_formula(geom, mode):
    from vit_vs_raw_iq_amd import Spectrogram, spectrogram_reference, spectrogram_reference_bwd
    from vit_vs_raw_iq_amd.spectrogram import _twiddles, _window
    n_fft, width, hop, pad, length = geom
    spec = Spectrogram(n_fft, width, length, hop, pad, window="hann", mode=mode, floor=1e-3, scale=1.3, shift=0.4)
    x = frames(2, length, 5)
    dout = np.random.default_rng(6).standard_normal((2, 1, n_fft, width))
    c, s = (torch.from_numpy(a) for a in _twiddles(n_fft, _window("hann", n_fft)))
    j, inside = R.window_index(n_fft, width, hop, pad, length)
    xt = torch.from_numpy(x).requires_grad_(True)
    mask = torch.from_numpy(inside)[None].double()
    ci = xt[:, 0][:, np.clip(j, 0, length - 1)] * mask
    cq = xt[:, 1][:, np.clip(j, 0, length - 1)] * mask
    re, im = ci @ c + cq @ s, cq @ c - ci @ s
    P = (re ** 2 + im ** 2) * spec.inv_norm
    v = torch.log10(P + spec.floor) if mode == "log" else P
    img = (v * spec.scale + spec.shift)[:, :, R.row_bins(n_fft)].permute(0, 2, 1)[:, None]
    np.testing.assert_allclose(img.detach().numpy(), spectrogram_reference(x, spec), rtol=0, atol=1e-11)
    (img * torch.from_numpy(dout)).sum().backward()
    want = xt.grad.numpy()
    got = spectrogram_reference_bwd(x, dout, spec)
    assert got.shape == (2, 2, length)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10 * max(1.0, np.abs(want).max()))


def test_default_hop_and_pad_centre_the_windows_on_the_frame():
    from vit_vs_raw_iq_amd import AMCTransformerViT, Spectrogram
    a = Spectrogram(224, 224, 1024)
    assert (a.hop, a.pad) == (4, 46)
    b = Spectrogram(32, 64, 1024)
    assert (b.hop, b.pad) == (16, 8)
    assert (b.window, b.mode, b.floor, b.scale, b.shift) == ("hann", "log", 1e-3, 1.0, 0.0)
    assert Spectrogram(32, 2048, 1024).hop == 1 and Spectrogram(32, 2, 100).pad == 0          # hop floor 1; windows inside
    assert Spectrogram(32, 5, 100, hop=20).pad == 6                                            # ceil((4*20 + 32 - 100) / 2)
    assert Spectrogram(32, 4, 100, hop=23).pad == 1                                            # ceil(1 / 2)
    np.testing.assert_allclose(a.inv_norm, 1.0 / (0.375 * 224), rtol=1e-12)                    # periodic Hann: sum w^2 = 3n/8
    np.testing.assert_allclose(Spectrogram(64, 8, window="rect").inv_norm, 1.0 / 64, rtol=0)
    assert a.table.shape == (2, 224, 224) and a.table.dtype == np.float32
    m, k = 5, 77
    w = 0.5 - 0.5 * np.cos(2 * np.pi * m / 224)
    np.testing.assert_allclose(a.table[:, m, k], [w * np.cos(2 * np.pi * k * m / 224), w * np.sin(2 * np.pi * k * m / 224)],
                               rtol=0, atol=6e-8)
    vit = AMCTransformerViT(in_channels=1, img_size_h=32, img_size_w=64, patch_size=16, num_classes=11, d_model=128, n_head=8,
                            n_layers=2, ffn_hidden=512, drop_prob=0.0, device="cpu")
    f = Spectrogram.for_model(vit, 1024, mode="power")
    assert (f.n_fft, f.width, f.hop, f.pad, f.mode) == (32, 64, 16, 8, "power")
    with pytest.raises(TypeError):
        Spectrogram.for_model(object())
    s = f.struct()
    assert (s.n_fft, s.hop, s.pad, s.width, s.mode) == (32, 16, 8, 64, 0) and s.floor == np.float32(1e-3)
    assert b.struct().mode == 1


def test_spectrogram_struct_matches_the_header_and_the_symbols_are_exported():
    import vit_vs_raw_iq_amd._native as N
    src = open(HEADER).read()
    body = re.search(r"typedef struct iq_spectrogram \{(.*?)\}", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip()
              for part in decl.split(",")]
    S = N.Spectrogram
    assert fields == [f[0] for f in S._fields_] == ["n_fft", "hop", "pad", "width", "mode", "inv_norm", "floor", "scale", "shift"]
    assert ctypes.sizeof(S) == 36 and [getattr(S, f).offset for f in fields] == list(range(0, 36, 4))
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, count in (("iq_frames_spectrogram", 7), ("iq_frames_spectrogram_bwd", 8)):
        decl = re.search(r"\b%s\(([^)]*)\)" % name, plain).group(1)
        assert len(decl.split(",")) == len(N.SIGNATURES[name][1]) == count
        assert getattr(N.lib(), name) is not None


def test_spectrogram_entry_points_refuse_bad_arguments_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import Spectrogram
    L = N.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(buf) + 15) // 16 * 16          # aligned host address: never dereferenced on these paths
    ARG, UNSUPPORTED = 1, 2
    base = Spectrogram(32, 8, 64)

    def call(bwd, x=a, table=a, io=a, dx=a, n=2, length=64, par="ok", **edit):
        if par == "ok":
            par = base.struct()
            for k, v in edit.items():
                setattr(par, k, v)
        p = ctypes.byref(par) if par is not None else None
        if bwd:
            return L.iq_frames_spectrogram_bwd(x, table, io, dx, n, length, p, None)
        return L.iq_frames_spectrogram(x, table, io, n, length, p, None)

    for bwd in (False, True):
        assert call(bwd, x=None) == ARG and call(bwd, table=None) == ARG and call(bwd, io=None) == ARG and call(bwd, par=None) == ARG
        assert call(bwd, length=0) == ARG and call(bwd, length=-5) == ARG
        assert call(bwd, hop=0) == ARG and call(bwd, hop=-1) == ARG and call(bwd, width=0) == ARG and call(bwd, pad=-1) == ARG
        assert call(bwd, mode=2) == ARG and call(bwd, mode=-1) == ARG
        for field in ("inv_norm", "floor", "scale", "shift"):
            for bad in (float("nan"), float("inf"), -float("inf")):
                assert call(bwd, **{field: bad}) == ARG, (field, bad)
        assert call(bwd, mode=1, floor=0.0) == ARG and call(bwd, mode=1, floor=-1.0) == ARG
        assert call(bwd, mode=0, floor=0.0, n=0) == 0                                    # the floor is not used in mode 0
        assert call(bwd, x=a + 2) == ARG and call(bwd, io=a + 1) == ARG and call(bwd, table=a + 4) == ARG
        for n_fft in (0, 16, 31, 33, 48, 288, 512, -32):
            assert call(bwd, n_fft=n_fft) == UNSUPPORTED, n_fft
        assert call(bwd, length=8193) == UNSUPPORTED                                     # 8 bytes per sample above 64 KB of LDS
        assert call(bwd, n=0) == 0 and call(bwd, n=-1) == 0                              # no frames: nothing to do
        for n_fft in range(32, 257, 32):
            assert call(bwd, n_fft=n_fft, n=0) == 0
        assert call(bwd, length=8192, n=0) == 0
    assert call(True, dx=None) == ARG and call(True, dx=a + 2) == ARG


def test_spectrogram_validates_its_arguments_before_any_device_work():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import Spectrogram, spectrogram_reference, spectrogram_reference_bwd
    bad = [
        (ValueError, dict(n_fft=0)), (ValueError, dict(n_fft=48)), (ValueError, dict(n_fft=288)), (TypeError, dict(n_fft=32.0)),
        (TypeError, dict(n_fft=True)), (ValueError, dict(width=0)), (TypeError, dict(width="64")), (ValueError, dict(length=0)),
        (ValueError, dict(length=8193)), (ValueError, dict(hop=0)), (TypeError, dict(hop=1.5)), (ValueError, dict(pad=-1)),
        (TypeError, dict(pad=2.0)), (ValueError, dict(window="hamming")), (ValueError, dict(mode="db")),
        (ValueError, dict(floor=0.0)), (ValueError, dict(floor=-1e-3)), (ValueError, dict(floor=1e-60)),
        (ValueError, dict(floor=float("nan"))), (TypeError, dict(floor="1e-3")), (ValueError, dict(scale=float("inf"))),
        (TypeError, dict(scale=None)), (ValueError, dict(shift=float("nan"))), (TypeError, dict(shift=True)),
    ]
    for exc, kw in bad:
        args = dict(n_fft=32, width=64)
        args.update(kw)
        with pytest.raises(exc):
            Spectrogram(**args)
    spec = Spectrogram(32, 64, 128)
    for x in (torch.zeros(2, 128, 2), torch.zeros(2, 2, 100), torch.zeros(2, 128), np.zeros((2, 2, 128)), None):
        with pytest.raises(ValueError):
            spec(x)
    with pytest.raises(P.IqError):
        spec(torch.zeros(2, 2, 128))                                                      # a CPU tensor: no CPU path
    with pytest.raises(P.IqError):
        spec.fit(torch.zeros(2, 2, 128))
    with pytest.raises(ValueError):
        spec.fit(torch.zeros(2, 2, 64))
    with pytest.raises(ValueError):
        spectrogram_reference(np.zeros((2, 2, 100)), spec)
    with pytest.raises(TypeError):
        spectrogram_reference(np.zeros((2, 2, 128)), None)
    with pytest.raises(ValueError):
        spectrogram_reference_bwd(np.zeros((2, 2, 128)), np.zeros((2, 1, 32, 63)), spec)


def test_spectrogram_none_leaves_the_four_input_paths_as_they_were():
    """The keyword is last, defaults to None, and with None each path accepts and refuses exactly what it did: the calls below are
    those of test_synth_cpu.py / test_impairments_cpu.py.  With a Spectrogram the layout must be 'vit' and the lengths must
    agree; impairment_curve also wants the model's image geometry."""
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import FrameSynth, Impairments, Spectrogram, SynthStream, data as D, impair, impairment_curve
    for fn in (D.DeviceInputPipeline.__init__, SynthStream.__init__, impair, impairment_curve):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "spectrogram" and last.default is None, fn
    st = {"i_mean": 0.0, "i_std": 1.0, "q_mean": 0.0, "q_std": 1.0}
    fs = FrameSynth(device="cpu")
    ok = SynthStream(fs, st, "vit", 8, h=32, w=32, stream=1, augment=Impairments.augmentation())
    assert (ok.take, ok.h, ok.w, ok.spectrogram) == (512, 32, 32, None)
    assert SynthStream(fs, st, "rawiq", 8).take == 1024
    with pytest.raises(ValueError):
        SynthStream(fs, st, "vit", 8, h=64, w=64)                                          # 2048 samples per channel of 1024
    spec = Spectrogram(32, 64, 1024)
    with_spec = SynthStream(fs, st, "vit", 8, h=64, w=64, spectrogram=spec)                # h, w are the spectrogram's
    assert (with_spec.take, with_spec.h, with_spec.w) == (1024, 32, 64) and with_spec.spectrogram is spec
    with pytest.raises(ValueError):
        SynthStream(fs, st, "rawiq", 8, spectrogram=spec)
    with pytest.raises(ValueError):
        SynthStream(fs, st, "vit", 8, spectrogram=Spectrogram(32, 64, 512))
    with pytest.raises(TypeError):
        SynthStream(fs, st, "vit", 8, spectrogram="hann")
    raw = torch.zeros(4, 1024, 2)
    with pytest.raises(P.IqError):
        impair(raw, st, "vit", Impairments())                                              # valid arguments, a CPU tensor
    with pytest.raises(P.IqError):
        impair(raw, st, "vit", Impairments(), spectrogram=spec)
    with pytest.raises(ValueError):
        impair(raw, st, "vit", Impairments(), h=64, w=64)
    with pytest.raises(ValueError):
        impair(raw, st, "rawiq", Impairments(), spectrogram=spec)
    with pytest.raises(ValueError):
        impair(raw[:, :512], st, "vit", Impairments(), spectrogram=spec)
    with pytest.raises(TypeError):
        impair(raw, st, "vit", Impairments(), spectrogram=3)
    kw = dict(in_channels=1, img_size_h=32, img_size_w=32, patch_size=16, num_classes=11, d_model=128, n_head=8, n_layers=2,
              ffn_hidden=512, drop_prob=0.0, device="cpu")
    vit = P.AMCTransformerViT(**kw)
    lab = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(P.IqError):
        impairment_curve(vit, raw, lab, st, "cfo", [0.0])                                  # valid arguments, a CPU tensor
    with pytest.raises(ValueError):
        impairment_curve(vit, raw, lab, st, "cfo", [0.0], spectrogram=spec)                # 32x64 image, 32x32 model
    with pytest.raises(P.IqError):
        impairment_curve(vit, raw, lab, st, "cfo", [0.0], spectrogram=Spectrogram(32, 32, 1024))
    with pytest.raises(TypeError):
        impairment_curve(vit, raw, lab, st, "cfo", [0.0], spectrogram=True)
    with pytest.raises(ValueError):
        D.DeviceInputPipeline(st, "image", 8)
    with pytest.raises(ValueError):
        D.DeviceInputPipeline(st, "vit", 8, h=64, w=64)
    with pytest.raises(ValueError):
        D.DeviceInputPipeline(st, "rawiq", 8, spectrogram=spec)
    with pytest.raises(TypeError):
        D.DeviceInputPipeline(st, "vit", 8, spectrogram=object())
    with pytest.raises(P.IqError):
        D.DeviceInputPipeline(st, "vit", 8, device="cpu")
    with pytest.raises(P.IqError):
        D.DeviceInputPipeline(st, "vit", 8, device="cpu", spectrogram=spec)


@pytest.mark.parametrize("geom", [(32, 31, 4, 8, 100), (96, 33, 99, 95, 100), (256, 5, 1, 0, 300)])
def test_shared_host_evaluations_agree_with_each_other(geom):
    """The int64 evaluation is the real-arithmetic one on integer data (float64 holds these integers exactly), and the
    real-arithmetic one in float64 is the product's complex-valued reference up to the fp32 rounding of the table."""
    from vit_vs_raw_iq_amd import Spectrogram, spectrogram_reference, spectrogram_reference_bwd
    n_fft, width, hop, pad, length = geom
    table, x, dout = R.int_case(n_fft, width, hop, pad, length, 2, seed=1)
    fake = types.SimpleNamespace(n_fft=n_fft, width=width, hop=hop, pad=pad, table=table.astype(np.float32), inv_norm=1.0,
                                 floor=1.0, scale=1.0, shift=0.0, mode="power")
    img = R.int_forward(x, table, geom[:4])
    assert img.shape == (2, 1, n_fft, width) and img.max() < 2 ** 23
    assert np.array_equal(img, R.real_forward(x, fake, np.float64))
    dx, bound = R.int_backward(x, table, dout, geom[:4])
    assert bound < 2 ** 24
    assert np.array_equal(dx, R.real_backward(x, dout, fake, np.float64))
    spec = Spectrogram(n_fft, width, length, hop, pad, mode="log", scale=0.8, shift=0.1)
    xf = frames(2, length, 8)
    ref = spectrogram_reference(xf, spec)
    np.testing.assert_allclose(R.real_forward(xf, spec, np.float64), ref, rtol=0, atol=2e-5)
    d = np.random.default_rng(9).standard_normal(ref.shape)
    want = spectrogram_reference_bwd(xf, d, spec)
    np.testing.assert_allclose(R.real_backward(xf, d, spec, np.float64), want, rtol=0, atol=2e-5 * max(1.0, np.abs(want).max()))
    assert R.real_forward(xf, spec, np.float32).dtype == np.float32
