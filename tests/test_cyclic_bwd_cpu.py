"""CPU: the adjoint of the cyclic-spectrum front end on the host.  cyclic_reference_bwd (the analytic fp64 adjoint) against torch
autograd through a torch restatement of cyclic_reference, all kinds and modes; the shared evaluations of tests/cyclic_bwd_ref.py
against it (real arithmetic in float64, int64 on the integer cases of the GPU file, whose exactness bounds are asserted here);
the zero frame; then the binding of iq_frames_cyclic_bwd against include/iqvit.h, its refusals with host addresses, and the
`differentiable` keyword."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cyclic_bwd_ref as A
import cyclic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iqvit.h")
KINDS = ("scf", "conj", "both")
MODES = ("power", "log", "coherence")

# (n_fft, columns, hop, pad, length)
GEOMS = {
    # windows from -13, 27, 67, 107: the first starts in front of the frame, the last runs past its end (120), and hop 40 >
    # n_fft leaves the samples 19..26, 59..66 and 99..106 uncovered
    "pad_end_uncovered": (32, 4, 40, 13, 120),
    # n_fft / 2 = 48 is no multiple of 32; windows in front of the frame and past its end
    "half_not_a_tile": (96, 5, 17, 30, 120),
}


def uncovered(geom):
    n_fft, columns, hop, pad, length = geom
    seen = np.zeros(length, bool)
    for t in range(columns):
        seen[max(0, t * hop - pad):max(0, min(length, t * hop - pad + n_fft))] = True
    return ~seen


def torch_image(x, cs):
    """cyclic_reference in torch (complex128), differentiable with respect to x (B, 2, len)."""
    from vit_vs_raw_iq_amd.spectrogram import _twiddles, _window
    n, T = cs.n_fft, cs.columns
    c, s = _twiddles(n, _window(cs.window, n))
    E = torch.from_numpy(c - 1j * s)
    j0 = np.arange(T, dtype=np.int64) * cs.hop - cs.pad
    j = j0[:, None] + np.arange(n, dtype=np.int64)[None, :]
    inside = torch.from_numpy((j >= 0) & (j < cs.length))
    z = torch.complex(x[:, 0], x[:, 1])
    cols = torch.where(inside[None], z[:, torch.from_numpy(np.clip(j, 0, cs.length - 1))], torch.zeros((), dtype=z.dtype))
    r = (np.arange(n, dtype=np.int64)[None, :] * (j0 % n)[:, None]) % n
    Y = (cols @ E) * torch.from_numpy(np.exp(-2j * np.pi * r / n))[None]
    D = (Y.real ** 2 + Y.imag ** 2).sum(dim=1)
    Yt = Y.transpose(1, 2)
    inv2 = cs.inv_norm ** 2
    a = (np.arange(n) + n // 2) % n
    k = (np.arange(n) + n // 2) % n
    chans = []
    for conj in ((False,), (True,), (False, True))[KINDS.index(cs.kind)]:
        G = Yt @ (Y if conj else Y.conj())
        l = (a[:, None] - k[None, :]) % n if conj else (k[None, :] - a[:, None]) % n
        kk = np.broadcast_to(k[None, :], l.shape)
        g = G[:, torch.from_numpy(kk.copy()), torch.from_numpy(l)]
        P = (g.real ** 2 + g.imag ** 2) * inv2
        if cs.mode == "power":
            v = P
        elif cs.mode == "log":
            v = torch.log10(P + cs.floor)
        else:
            v = P / (D[:, torch.from_numpy(kk.copy())] * D[:, torch.from_numpy(l)] * inv2 + cs.floor)
        chans.append(v * cs.scale + cs.shift)
    return torch.stack(chans, dim=1)


def make(geom, **kw):
    from vit_vs_raw_iq_amd import CyclicSpectrum
    n_fft, columns, hop, pad, length = geom
    return CyclicSpectrum(n_fft, length, hop, pad, columns, **kw)


def case(geom, kind, mode, seed=3):
    cs = make(geom, kind=kind, mode=mode, floor=1e-2, scale=1.5, shift=-0.25)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, 2, geom[4]))
    dout = rng.standard_normal((2, cs.channels, cs.n_fft, cs.n_fft))
    return cs, x, dout


def test_the_geometries_are_what_their_names_say():
    n_fft, columns, hop, pad, length = GEOMS["pad_end_uncovered"]
    starts = np.arange(columns) * hop - pad
    assert pad > 0 and starts[0] < 0 and starts[-1] < length < starts[-1] + n_fft
    assert np.flatnonzero(uncovered(GEOMS["pad_end_uncovered"])).tolist() == [*range(19, 27), *range(59, 67), *range(99, 107)]
    n_fft, columns, hop, pad, length = GEOMS["half_not_a_tile"]
    assert (n_fft // 2) % 32 != 0 and (columns - 1) * hop - pad + n_fft > length      # and windows past the end


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(GEOMS))
def test_reference_bwd_is_the_gradient_torch_autograd_finds(name, kind, mode):
    """fp64 on both sides: rounding only, 1e-9 relative to the largest gradient element."""
    from vit_vs_raw_iq_amd import cyclic_reference, cyclic_reference_bwd
    cs, x, dout = case(GEOMS[name], kind, mode)
    xt = torch.from_numpy(x).requires_grad_(True)
    img = torch_image(xt, cs)
    assert np.abs(img.detach().numpy() - cyclic_reference(x, cs)).max() <= 1e-10 * max(1.0, float(img.detach().abs().max()))
    (img * torch.from_numpy(dout)).sum().backward()
    want = xt.grad.numpy()
    got = cyclic_reference_bwd(x, dout, cs)
    assert got.shape == x.shape and got.dtype == np.float64 and np.abs(want).max() > 0
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    dark = uncovered(GEOMS[name])
    assert np.all(got[:, :, dark] == 0.0) and np.all(want[:, :, dark] == 0.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(GEOMS))
def test_real_backward_in_float64_restates_the_reference(name, kind, mode):
    """The same formulae without complex numbers, from the tables ROUNDED to fp32: 1e-5 relative (the tables' 6e-8, amplified by
    the coherence's division), and the float32 evaluation is a different, coarser number (E32 > 0)."""
    from vit_vs_raw_iq_amd import cyclic_reference_bwd
    cs, x, dout = case(GEOMS[name], kind, mode)
    ref = cyclic_reference_bwd(x, dout, cs)
    r64 = A.real_backward(x, dout, cs, np.float64)
    assert np.abs(r64 - ref).max() <= 1e-5 * np.abs(ref).max()
    r32 = A.real_backward(x, dout, cs, np.float32)
    e32 = np.abs(r32.astype(np.float64) - ref).max()
    assert 0 < e32 <= 1e-2 * np.abs(ref).max()


@pytest.mark.parametrize("name", list(A.EXACT))
def test_int_backward_is_the_reference_on_the_integer_cases_and_its_bounds_hold(name):
    """int_backward asserts the 2^24 bounds of every partial sum; the reference takes the integer tables in the place of its own.
    float64 holds every integer on the way (they are below 2^24 in absolute sum), so the two agree exactly."""
    from vit_vs_raw_iq_amd import CyclicSpectrum, cyclic_reference_bwd
    n_fft, columns, hop, pad, length, n = A.EXACT[name]
    table, rot, x = R.int_case(n_fft, columns, hop, pad, length, n, seed=n_fft + columns)
    for kind, kname in enumerate(KINDS):
        dout = A.int_dout(n_fft, 2 if kind == 2 else 1, n, seed=n_fft + columns + kind, density=A.DENSITY)
        assert set(np.unique(dout)) == {-1, 0, 1}
        want = A.int_backward(x, table, rot, dout, (n_fft, columns, hop, pad), kind)
        assert want.dtype == np.int64 and want.shape == x.shape and np.abs(want).max() > 0
        cs = CyclicSpectrum(n_fft, length, hop, pad, columns, window="rect", kind=kname, mode="power")
        cs.inv_norm = 1.0
        assert np.array_equal(cyclic_reference_bwd(x, dout, cs, table=table, rot=rot), want.astype(np.float64))
        cs.table, cs.rot = table.astype(np.float32), rot.astype(np.float32)
        assert np.array_equal(A.real_backward(x, dout, cs, np.float64), want.astype(np.float64))
        assert np.array_equal(A.real_backward(x, dout, cs, np.float32), want.astype(np.float32))


@pytest.mark.parametrize("mode", MODES)
def test_the_zero_frame_has_exactly_zero_gradient(mode):
    from vit_vs_raw_iq_amd import cyclic_reference_bwd
    cs, x, dout = case(GEOMS["half_not_a_tile"], "both", mode)
    x[1] = 0.0
    for got in (cyclic_reference_bwd(x, dout, cs), A.real_backward(x, dout, cs, np.float64), A.real_backward(x, dout, cs, np.float32)):
        assert np.all(got[1] == 0.0) and np.abs(got[0]).max() > 0


def test_the_symbol_is_declared_bound_and_exported_with_nine_arguments():
    import vit_vs_raw_iq_amd._native as N
    plain = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\biq_frames_cyclic_bwd\(([^)]*)\)", plain).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["iq_frames_cyclic_bwd"][1]) == 9
    assert N.SIGNATURES["iq_frames_cyclic_bwd"][1][7] is N.SIGNATURES["iq_frames_cyclic"][1][6]      # the same iq_cyclic_t
    assert N.lib().iq_frames_cyclic_bwd is not None


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    cases = A.refusal_calls(L, a)
    assert len([c for c in cases if c[2] != 0]) > 45
    for what, run, expect in cases:
        assert run() == expect, what


def test_the_differentiable_keyword():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import CyclicSpectrum
    from test_cyclic_ref_cpu import fake_vit
    assert CyclicSpectrum(32).differentiable is False and CyclicSpectrum(32, differentiable=True).differentiable is True
    assert repr(CyclicSpectrum(32)).endswith("differentiable=False)")
    assert repr(CyclicSpectrum(32, differentiable=True)).endswith("differentiable=True)")
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(TypeError):
            CyclicSpectrum(32, differentiable=bad)
    assert CyclicSpectrum.for_model(fake_vit(2, 64, 64), 1024, differentiable=True).differentiable is True
    assert CyclicSpectrum.for_model(fake_vit(2, 64, 64), 1024).differentiable is False
    # the header's LDS rule is mirrored at construction; without the keyword the same geometry is still taken
    for n_fft, ok, refused in ((256, 4280, 4281), (32, 8032, 8033)):
        assert CyclicSpectrum(n_fft, ok, differentiable=True).length == ok
        with pytest.raises(ValueError, match="differentiable=True"):
            CyclicSpectrum(n_fft, refused, differentiable=True)
        assert CyclicSpectrum(n_fft, refused).differentiable is False
    for n_fft in range(32, 257, 32):
        assert A.adjoint_lds_bytes(n_fft, 4096) <= 160 * 1024
        CyclicSpectrum(n_fft, 4096, differentiable=True)
    # a CPU tensor is refused as a CPU tensor, whether or not it requires grad and whatever the keyword says
    x = torch.zeros(2, 2, 128, requires_grad=True)
    for flag in (False, True):
        with pytest.raises(P.IqError, match="CPU tensor"):
            CyclicSpectrum(32, 128, differentiable=flag)(x)
