"""GPU (MI355X): the adjoint of the cyclic-spectrum front end (csrc/cyclic.hip, iq_frames_cyclic_bwd, CyclicSpectrum(...,
differentiable=True)).

1. Exact: the integer cases of tests/cyclic_bwd_ref.py (the ten geometries of the forward's EXACT, all three kinds) make every
   fp32 partial sum of the kernel an integer below 2^24 (int_backward asserts it), so dx equals the int64 evaluation bit for
   bit.  x, the tables and dout lie between NaN guards, dx between sentinels and is pre-filled with the sentinel, the launched
   kernel is asserted by name (Y kept whole or recomputed, by the header's rule).
2. Real tables against the host fp64 adjoint in all three modes.  The tolerance is measured on the reference, never on the
   kernel: E32 = the largest error of the same formulae in numpy float32 arithmetic (cyclic_bwd_ref.real_backward); the kernel
   is allowed FACTOR * E32 with the project's FACTOR = 4 of the cyclic forward and of the spectrogram's backward: the kernel adds
   the same fp32 terms in another order than numpy.  The measured ratios are printed (profiles/cyclic_bwd.txt records them).
   The all-zero frame's gradient is exactly 0.
3. Through Python: x.grad of model(cs(x)) equals the chain done by hand through the C ABI bit for bit; the images of a
   differentiable front end are those of the default one; the default one still refuses.
4. Independence: a frame's gradient does not depend on the other frames of the call, its position, or a NaN neighbour with NaN
   dout; two runs agree bit for bit.  fit() between forward and backward does not change the gradient of the earlier call.
5. Refusals: every ARG / UNSUPPORTED case of the header on the device, with no kernel launched.
"""
import ctypes

import numpy as np
import pytest
import torch

import cyclic_bwd_ref as A
import cyclic_ref as R
from frontend_gpu import GUARD, SENTINEL, abi_call, bits, dev, on_device, same_bits, small_vit
from prof_names import kernel_launches
from test_gpu_cyclic import struct, zscored_frames

pytestmark = pytest.mark.gpu

# (n_fft, columns, hop, pad, len, n_frames): the forward's ten geometries, and one more for the backward's own second shape: 65
# columns = three chunks (the last of one column) at eight tiles, where Y no longer fits beside the frame and its gradient and
# every band recomputes it chunk by chunk in both passes; two frames
EXACT = dict(A.EXACT, three_chunks_recomputed=(256, 65, 13, 100, 1100, 2))


def keeps_y(n_fft, columns, length):
    """The header's rule for the backward: every 32-column chunk of Y stays in LDS when the frame, its gradient, rot, D, the
    working tiles and the chunks fit in 160 KB; otherwise one chunk at a time is recomputed."""
    chunks = (columns + 31) // 32
    return 4 * (2 * ((2 * length + 3) & ~3) + 3 * n_fft + 6624 + chunks * 64 * (n_fft + 1)) <= 160 * 1024


def kernel_name(par, length):
    flag = lambda b: "true" if b else "false"   # noqa: E731
    return f"cyclic_bwd_kernel<{flag(par.kind != 1)}, {flag(par.kind != 0)}, {flag(keeps_y(par.n_fft, par.columns, length))}>"


def abi_backward(x, table, rot, dout, par, expect_kernel=True):
    """x (n, 2, len), table, rot, dout (n, C, n_fft, n_fft) numpy -> dx (n, 2, len) numpy through the C ABI.  The four operands lie
    between NaN guards (a read outside any of them poisons dx), dx between sentinels and is pre-filled with the sentinel (an
    element the kernel does not write shows)."""
    n, _, length = x.shape
    return abi_call("iq_frames_cyclic_bwd", kernel_name(par, length), (x, table, rot, dout), (n, 2, length), n, length, par,
                    expect_kernel)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. exact
# ---------------------------------------------------------------------------------------------------------------------------
# Y is kept whole in the backward for all but the widest with more than one chunk
KEPT = {"eight_tiles_two_chunks": False, "three_chunks_recomputed": False}


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("name", list(EXACT))
def test_dx_equals_the_int64_evaluation_bit_for_bit(name, kind):
    """Mode 'power', inv_norm = scale = 1.  int_backward asserts that every sum of absolute terms is below 2^24."""
    n_fft, columns, hop, pad, length, n = EXACT[name]
    assert keeps_y(n_fft, columns, length) == KEPT.get(name, True)       # abi_backward asserts the kernel of that shape by name
    table, rot, x = R.int_case(n_fft, columns, hop, pad, length, n, seed=n_fft + columns)
    dout = A.int_dout(n_fft, 2 if kind == 2 else 1, n, seed=n_fft + columns + kind, density=A.DENSITY)
    want = A.int_backward(x, table, rot, dout, (n_fft, columns, hop, pad), kind)
    got = abi_backward(x, table, rot, dout, struct(n_fft, columns, hop, pad, kind=kind))
    assert not np.isnan(got).any() and not np.any(got == SENTINEL)
    assert np.abs(want).max() > 0 and np.array_equal(bits(got), bits(want))


def test_an_offset_frame_pointer_takes_the_scalar_staging_path():
    """x 8 bytes off a 16-byte boundary with an even length: the float4 staging of the frame is not used; dx 4 bytes off."""
    import vit_vs_raw_iq_amd._native as N
    n_fft, columns, hop, pad, length, n = 64, 20, 5, 9, 100, 2
    table, rot, x = R.int_case(n_fft, columns, hop, pad, length, n, seed=77)
    dout = A.int_dout(n_fft, 2, n, seed=78, density=A.DENSITY)
    par = struct(n_fft, columns, hop, pad)
    buf = torch.full((2 + x.size + GUARD,), float("nan"), dtype=torch.float32, device=dev())
    buf[2:2 + x.size] = torch.from_numpy(x.astype(np.float32).reshape(-1)).to(dev())
    tab = torch.from_numpy(table.astype(np.float32)).to(dev())
    rt = torch.from_numpy(rot.astype(np.float32)).to(dev())
    d = torch.from_numpy(dout.astype(np.float32)).to(dev())
    dx = torch.full((1 + x.size + GUARD,), SENTINEL, dtype=torch.float32, device=dev())
    assert buf.data_ptr() % 16 == 0 and dx.data_ptr() % 16 == 0
    N.check(N.lib().iq_frames_cyclic_bwd(buf.data_ptr() + 8, tab.data_ptr(), rt.data_ptr(), d.data_ptr(), dx.data_ptr() + 4, n,
                                         length, ctypes.byref(par), N.stream_handle()), "iq_frames_cyclic_bwd")
    want = A.int_backward(x, table, rot, dout, (n_fft, columns, hop, pad), 2)
    got = dx.cpu().numpy()
    assert np.array_equal(bits(got[1:1 + x.size]), bits(want).reshape(-1))
    assert got[0] == SENTINEL and np.all(got[1 + x.size:] == SENTINEL)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. real tables against fp64
# ---------------------------------------------------------------------------------------------------------------------------
FACTOR = 4                      # allowed multiple of E32 (see the module docstring)
REAL_GEOMS = {"64_hop16": (64, 16), "224_hop56": (224, 56)}


@pytest.mark.parametrize("mode", ["power", "log", "coherence"])
@pytest.mark.parametrize("name", list(REAL_GEOMS))
def test_x_grad_against_the_fp64_adjoint(name, mode):
    from vit_vs_raw_iq_amd import CyclicSpectrum, cyclic_reference_bwd
    n_fft, hop = REAL_GEOMS[name]
    floor = 1e-3 if mode == "log" else 1e-6
    cs = CyclicSpectrum(n_fft, 1024, hop, window="hann", kind="both", mode=mode, floor=floor, scale=1.5, shift=-0.25,
                        differentiable=True)
    assert cs.columns == (61 if n_fft == 64 else 15)
    xh = zscored_frames()
    dout = np.random.default_rng(n_fft + len(mode)).standard_normal((len(xh), 2, n_fft, n_fft)).astype(np.float32)
    x = on_device(xh).requires_grad_(True)
    (cs(x) * on_device(dout)).sum().backward()
    got = x.grad.cpu().numpy()
    ref = cyclic_reference_bwd(xh, dout, cs)
    e32 = np.abs(A.real_backward(xh, dout, cs, np.float32).astype(np.float64) - ref).max()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"{name} {mode}: E32 {e32:.3e}, kernel {err:.3e} ({err / e32:.2f} E32), largest |dx| {np.abs(ref).max():.3e}")
    assert e32 > 0
    assert err <= FACTOR * e32
    assert np.all(got[-1] == 0.0) and np.abs(got[:-1]).max() > 0         # the zero frame


# ---------------------------------------------------------------------------------------------------------------------------
# 3. through Python
# ---------------------------------------------------------------------------------------------------------------------------
def test_x_grad_through_a_vit_equals_the_chained_abi_calls():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import CyclicSpectrum
    m = small_vit(2, 64, 64)
    cs = CyclicSpectrum.for_model(m, 1024, differentiable=True)
    plain = CyclicSpectrum.for_model(m, 1024)
    assert (cs.n_fft, cs.kind, cs.differentiable, plain.differentiable) == (64, "both", True, False)
    x0 = on_device(zscored_frames()[[0, 1, 2, 4, 7, 8]])
    x = x0.clone().requires_grad_(True)
    img = cs(x)
    assert img.requires_grad and same_bits(img.detach(), plain(x0)) and same_bits(cs(x0), plain(x0))
    with torch.no_grad():
        assert cs(x).requires_grad is False and same_bits(cs(x), plain(x0))
    m(img).sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and float(x.grad.abs().max()) > 0
    with pytest.raises(RuntimeError, match="not differentiable"):
        plain(x)
    # the same chain by hand: image through the C ABI, d(image) from the model, then the adjoint through the C ABI
    par, tab, rot = cs.struct(), cs.table_on(dev()), cs.rot_on(dev())
    im = torch.empty(6, 2, 64, 64, device=dev())
    N.check(N.lib().iq_frames_cyclic(x0.data_ptr(), tab.data_ptr(), rot.data_ptr(), im.data_ptr(), 6, 1024, ctypes.byref(par),
                                     N.stream_handle()), "iq_frames_cyclic")
    assert same_bits(im, img.detach())
    im.requires_grad_(True)
    m(im).sum().backward()
    dx = torch.full_like(x0, SENTINEL)
    N.check(N.lib().iq_frames_cyclic_bwd(x0.data_ptr(), tab.data_ptr(), rot.data_ptr(), im.grad.contiguous().data_ptr(),
                                         dx.data_ptr(), 6, 1024, ctypes.byref(par), N.stream_handle()), "iq_frames_cyclic_bwd")
    assert same_bits(dx, x.grad)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. independence, fit()
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["log", "coherence"])
def test_a_frame_does_not_depend_on_the_call_it_is_part_of(mode):
    from vit_vs_raw_iq_amd import CyclicSpectrum
    n_fft, hop, pad, length = 64, 7, 20, 301                            # odd length: the frames of a call alternate in alignment
    rng = np.random.default_rng(12)
    x = rng.standard_normal((3, 2, length)).astype(np.float32)
    dout = rng.standard_normal((3, 2, n_fft, n_fft)).astype(np.float32)
    cs = CyclicSpectrum(n_fft, length, hop, pad, mode=mode)
    assert cs.columns > 32
    par = cs.struct()
    dx = abi_backward(x, cs.table, cs.rot, dout, par)
    assert np.isfinite(dx).all() and np.abs(dx).max() > 0
    assert np.array_equal(bits(abi_backward(x, cs.table, cs.rot, dout, par, expect_kernel=False)), bits(dx))    # two runs
    order = [2, 0, 1]
    assert np.array_equal(bits(abi_backward(x[order], cs.table, cs.rot, dout[order], par, expect_kernel=False)), bits(dx[order]))
    for b in range(3):
        one = abi_backward(x[b:b + 1], cs.table, cs.rot, dout[b:b + 1], par, expect_kernel=False)
        assert np.array_equal(bits(one[0]), bits(dx[b])), b
    # NaN neighbours with NaN dout on both sides change nothing
    px, pd = x.copy(), dout.copy()
    px[0], px[2], pd[0], pd[2] = np.nan, np.nan, np.nan, np.nan
    got = abi_backward(px, cs.table, cs.rot, pd, par, expect_kernel=False)
    assert np.array_equal(bits(got[1]), bits(dx[1]))
    end = (cs.columns - 1) * hop - pad + n_fft                           # the windows cover [0, end); behind it dx is 0 by contract
    assert 0 < end < length and np.all(dx[:, :, end:] == 0.0)
    for b in (0, 2):
        assert np.isnan(got[b, :, :end]).all() and np.all(got[b, :, end:] == 0.0)


def test_fit_between_forward_and_backward_does_not_change_the_gradient_of_the_earlier_call():
    from vit_vs_raw_iq_amd import CyclicSpectrum
    x0 = on_device(zscored_frames()[:4])
    w = torch.from_numpy(np.random.default_rng(5).standard_normal((4, 2, 64, 64)).astype(np.float32)).to(dev())
    cs = CyclicSpectrum(64, 1024, scale=2.0, shift=0.5, differentiable=True)
    x = x0.clone().requires_grad_(True)
    (cs(x) * w).sum().backward()
    want = x.grad.clone()
    x = x0.clone().requires_grad_(True)
    loss = (cs(x) * w).sum()
    cs.fit(x0)
    assert cs.scale != 2.0
    loss.backward()
    assert same_bits(x.grad, want)
    x = x0.clone().requires_grad_(True)
    (cs(x) * w).sum().backward()
    assert not same_bits(x.grad, want)                                   # a call after fit() has the new scale


# ---------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_header_returns_before_any_launch():
    """The cases of tests/test_cyclic_bwd_cpu.py with DEVICE pointers and a live stream: the status is the header's, no kernel is
    recorded and the buffer keeps its sentinel."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    buf = torch.full((8192 * 2 * 2 + 64,), SENTINEL, dtype=torch.float32, device=dev())
    a = buf.data_ptr()
    assert a % 16 == 0
    cases = A.refusal_calls(L, a)
    refused = [c for c in cases if c[2] != 0]
    assert len(refused) > 45
    statuses = []
    launched = kernel_launches(L, lambda: statuses.extend(run() for _, run, _ in cases))
    torch.cuda.synchronize()
    for (what, _, expect), got in zip(cases, statuses):
        assert got == expect, what
    assert launched == {}
    assert bool((buf == SENTINEL).all())
