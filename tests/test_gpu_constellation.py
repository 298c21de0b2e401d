"""GPU (MI355X): the constellation front end (csrc/constellation.hip, iq_frames_constellation / _bwd,
vit_vs_raw_iq_amd.constellation).

1. Exact: integer tables and points on a dyadic grid (tests/constellation_ref.EXACT) make every weight an integer and every fp32
   partial sum an integer below 2^24 (asserted in the helper), so the image and the gradient equal an int64 host evaluation bit
   for bit.  The inputs lie between NaN guards, the outputs between sentinels, the launched kernel is asserted by name.
2. Structure: one point lights exactly the pixels within `radius` and its patch is the outer product of the two profiles;
   permuting the points of an integer frame changes nothing; noiseless QPSK gives four maxima at the predicted pixels.
3. Log mode against the host fp64 definition.  The tolerance is measured on the reference, never on the kernel: E32 = the largest
   error of the same definition evaluated in numpy float32 arithmetic (constellation_ref.real_forward / real_backward); the
   kernel is allowed FACTOR * E32 (its sum is an ordered fmaf chain, the device has its own log10f).  No element is excluded.
   FACTOR started at 8, the spectrogram suite's first figure.  Measured on an MI355X the kernel is at 0.74 / 0.99 E32 forward and
   1.000 / 0.68 E32 backward (profiles/constellation.txt), so it was lowered to 3: twice the largest ratio, rounded up (2.0 sits
   on the print's last digit, so the next whole number was taken).  The backward's E32 at 224 x 224 (1.5 of a largest |dx| of
   165) is one point whose t lies within fp32 rounding of a table knot: fp32 takes the neighbouring segment's slope, the
   numpy-float32 evaluation and the kernel alike -- the gradient of a piecewise linear profile is a step function there.
4. Backward: two runs agree bit for bit (in 1.), x.grad through con(x) -> a small ViT -> sum() equals the chained C-ABI calls bit
   for bit, in both modes.
5. Independence: a frame's image and gradient do not depend on the other frames of the call or its position in it.
6. Refusals: every IQ_STATUS_ARG and IQ_STATUS_UNSUPPORTED of the header, outputs untouched.
7. Integration: the `spectrogram=` keyword of SynthStream, DeviceInputPipeline, impair and impairment_curve; a ViT trained on
   constellations of received symbols; Constellation.fit.
"""
import ctypes

import numpy as np
import pytest
import torch

import constellation_ref as R
from frontend_gpu import GUARD, SENTINEL, abi_call, bits, dev, on_device, same_bits, small_vit
from prof_names import kernel_launches

pytestmark = pytest.mark.gpu

def abi_forward(x, table, par, expect_kernel=True):
    """x (n, 2, len), table numpy -> image (n, 1, height, width) numpy through the C ABI.  x and the table lie between NaN guards
    (a read outside either poisons the image: a NaN weight reaches every pixel of its tile), the image between sentinels."""
    n, _, length = x.shape
    return abi_call("iq_frames_constellation", "constellation_fwd_kernel", (x, table), (n, 1, par.height, par.width), n, length,
                    par, expect_kernel)


def abi_backward(x, table, dout, par, expect_kernel=True):
    """-> dx (n, 2, len) numpy through the C ABI; dx lies between sentinels and is pre-filled with the sentinel."""
    n, _, length = x.shape
    return abi_call("iq_frames_constellation_bwd", "constellation_bwd_kernel", (x, table, dout), (n, 2, length), n, length, par,
                    expect_kernel)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. exact
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.EXACT))
def test_forward_and_backward_equal_the_int64_evaluation_bit_for_bit(name):
    """Mode 0, unit scales, inv_norm = scale = 1 (constellation_ref.EXACT says which case reaches which branch).  The bounds are
    the largest sums of absolute values of the terms of one pixel / one dx element: below 2^24, so every partial sum of the
    kernel, in any order, is an exact integer."""
    case = R.int_case(name)
    con = R.as_constellation(case)
    par, x = con.struct(), case["x"]
    want, bound = R.int_forward(case)
    got = abi_forward(x, con.table, par)
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(want))
    want_dx, bound_dx = R.int_backward(case)
    print(f"{name}: largest sum of absolute terms of a pixel {bound}, of a dx element {bound_dx} (2^24 = {2 ** 24})")
    assert bound < 2 ** 24 and bound_dx < 2 ** 24
    dx = abi_backward(x, con.table, case["dout"], par)
    assert np.array_equal(bits(dx), bits(want_dx))
    again = abi_backward(x, con.table, case["dout"], par, expect_kernel=False)
    assert np.array_equal(bits(dx), bits(again))
    # dropped samples: NaN, infinite or out of reach of every pixel -> exactly +0
    with np.errstate(invalid="ignore"):
        reach = case["radius"] + 0.5
        out = ~((x[:, 0] > -reach) & (x[:, 0] < case["width"] + reach) & (x[:, 1] > -reach) & (x[:, 1] < case["height"] + reach))
    if "nonfinite" in name or "border" in name:
        assert out.sum() > 0
    assert np.all(bits(dx.transpose(0, 2, 1))[out] == 0)
    if name == "empty_tiles_hold_shift":
        assert np.all(bits(got[:, :, 32:, :]) == bits(np.float32(5.0))) and np.all(bits(got[:, :, :, 32:]) == bits(np.float32(5.0)))
        assert got[:, :, :32, :32].max() > 5.0
    if name == "len8192_one_pixel":
        assert got.max() == 8192 * 16.0 and (got > 0).sum() == 9          # the table [4, 2, 0]: 3 x 3 lit pixels


def test_an_offset_frame_pointer_takes_the_scalar_staging_path():
    """x 4 bytes off a 16-byte boundary with an even length: the float4 staging of the frame is not used."""
    import vit_vs_raw_iq_amd._native as N
    case = R.int_case("len64_tile_edges")
    con = R.as_constellation(case)
    par, x = con.struct(), case["x"]
    buf = torch.full((1 + x.size + GUARD,), float("nan"), dtype=torch.float32, device=dev())
    buf[1:1 + x.size] = on_device(x).reshape(-1)
    tab = on_device(con.table)
    out = torch.empty(1, 1, par.height, par.width, device=dev())
    dx = torch.empty(1, 2, x.shape[2], device=dev())
    dout = on_device(case["dout"])
    assert buf.data_ptr() % 16 == 0
    N.check(N.lib().iq_frames_constellation(buf.data_ptr() + 4, tab.data_ptr(), out.data_ptr(), 1, x.shape[2], ctypes.byref(par),
                                            N.stream_handle()), "iq_frames_constellation")
    N.check(N.lib().iq_frames_constellation_bwd(buf.data_ptr() + 4, tab.data_ptr(), dout.data_ptr(), dx.data_ptr(), 1, x.shape[2],
                                                ctypes.byref(par), N.stream_handle()), "iq_frames_constellation_bwd")
    assert np.array_equal(bits(out.cpu().numpy()), bits(R.int_forward(case)[0]))
    assert np.array_equal(bits(dx.cpu().numpy()), bits(R.int_backward(case)[0]))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. structure
# ---------------------------------------------------------------------------------------------------------------------------
def profile32(u, n_pix, con):
    """The weights of one pixel coordinate u (exact in fp32) as the header words them, step by step in fp32 (the fused
    multiply-add through fp64, whose product of two fp32 numbers is exact)."""
    f32 = np.float32
    tab = con.table
    w = np.zeros(n_pix, f32)
    for c in range(n_pix):
        e = f32(u) - f32(c + 0.5)
        t = f32(abs(e) * f32(con.n_frac))
        if t < con.radius * con.n_frac:
            i = int(np.floor(t))
            w[c] = f32(np.float64(f32(t - f32(i))) * np.float64(f32(tab[i + 1] - tab[i])) + np.float64(tab[i]))
    return w


def test_one_point_lights_the_outer_product_of_its_two_profiles():
    from vit_vs_raw_iq_amd import Constellation
    con = Constellation(96, 64, 3, mode="power", inv_norm=1.0)             # gaussian sigma 1, radius 4, n_frac 8
    con.x_scale = con.y_scale = 1.0
    con.x_off = con.y_off = 0.0
    u, v = 30.3125, 65.8125                                                # windows across a tile edge on both axes
    x = np.full((1, 2, 3), np.nan, np.float32)
    x[0, :, 1] = u, v
    img = abi_forward(x, con.table, con.struct())[0, 0]
    a, b = profile32(v, 96, con), profile32(u, 64, con)
    assert (a > 0).sum() == 8 and (b > 0).sum() == 8
    lit = np.outer(a > 0, b > 0)
    rows, cols = np.arange(96) + 0.5, np.arange(64) + 0.5
    assert np.array_equal(lit, np.outer(np.abs(rows - v) < 4, np.abs(cols - u) < 4))
    assert np.all(bits(img[~lit]) == 0) and np.all(img[lit] > 0)
    assert np.array_equal(bits(img), bits(np.outer(a, b).astype(np.float32)))       # one product per pixel, rounded once


def test_permuting_the_points_of_an_integer_frame_leaves_the_image_unchanged():
    case = R.int_case("len1024_nonfinite_256x256_nfrac2")
    con = R.as_constellation(case)
    img = abi_forward(case["x"], con.table, con.struct())
    perm = np.random.default_rng(8).permutation(case["x"].shape[2])
    assert np.array_equal(bits(abi_forward(case["x"][:, :, perm], con.table, con.struct(), expect_kernel=False)), bits(img))


def test_noiseless_qpsk_gives_four_maxima_at_the_predicted_pixels():
    from vit_vs_raw_iq_amd import Constellation
    con = Constellation(64, 96, 256)                                       # extent 3, gaussian sigma 1, log, default floor
    rng = np.random.default_rng(9)
    sym = rng.choice([-1.0, 1.0], (2, 2, 256)).astype(np.float32)
    img = con(on_device(sym)).cpu().numpy()
    cols = [int(np.floor(s * con.x_scale + con.x_off)) for s in (-1.0, 1.0)]
    rows = [int(np.floor(s * con.y_scale + con.y_off)) for s in (-1.0, 1.0)]
    assert cols == [32, 64] and rows == [21, 42]
    dark32 = np.float32(np.log10(np.float32(con.floor)))
    for f in range(2):
        im = img[f, 0]
        far = np.ones_like(im, bool)
        for r in rows:
            for c in cols:
                far[max(0, r - 5):r + 6, max(0, c - 5):c + 6] = False
                blob = im[r - 5:r + 6, c - 5:c + 6]
                assert blob.max() == im[r, c] and im[r, c] > dark32 + 2.0          # two decades over the empty level
        dark = im[far]
        assert dark.size > 64 * 96 // 2 and np.all(bits(dark) == bits(dark)[0])    # nothing else above the floor
        assert abs(float(dark[0]) - float(dark32)) <= 4 * np.spacing(abs(dark32))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. log mode against fp64
# ---------------------------------------------------------------------------------------------------------------------------
def zscored_frames(indices, length):
    """Frames `indices` of a FrameSynth stream (frame j: class j % 4, noise at -8 dB for even j // 4 and +20 dB for odd; fixed
    seed), z-scored as the input pipeline hands them on, and one all-zero frame behind them -> (len(indices) + 1, 2, length)."""
    from vit_vs_raw_iq_amd import FrameSynth, Impairments, impair
    fs = FrameSynth(["BPSK", "QPSK", "16QAM", "GMSK"], snrs_db=(-8.0, 20.0), length=length, seed=11, device=dev())
    raw = torch.cat([fs.generate(1, j, 0)[0] for j in indices])
    x = impair(raw, fs.stats(64), "rawiq", Impairments())
    return torch.cat([x, torch.zeros(1, 2, length, device=dev())])


# name -> (height, width, len, frame indices): 224 x 224 from 1024 points with 3 frames (QPSK at -8 dB, 16QAM at +20 dB, zeros),
# 32 x 64 from 128 points with 6 frames
LOG_GEOMS = {"cfg_b_224x224": (224, 224, 1024, (1, 6)), "ref_32x64": (32, 64, 128, (0, 3, 4, 5, 7))}
FACTOR = 3                      # allowed multiple of E32 (see the module docstring)


@pytest.mark.parametrize("name", list(LOG_GEOMS))
def test_log_constellation_and_its_gradient_against_the_fp64_definition(name):
    from vit_vs_raw_iq_amd import Constellation, constellation_reference, constellation_reference_bwd
    height, width, length, indices = LOG_GEOMS[name]
    con = Constellation(height, width, length, profile="gaussian", sigma=1.0, radius=4, n_frac=8, mode="log")
    x = zscored_frames(indices, length).requires_grad_(True)
    xh = x.detach().cpu().numpy()
    img = con(x)
    ref = constellation_reference(xh, con)
    e32 = np.abs(R.real_forward(xh, con, np.float32).astype(np.float64) - ref).max()
    err = np.abs(img.detach().cpu().numpy().astype(np.float64) - ref).max()
    print(f"{name} forward: E32 {e32:.3e}, kernel {err:.3e} ({err / e32:.3f} E32), image range [{ref.min():.2f}, {ref.max():.2f}]")
    dout = torch.from_numpy(np.random.default_rng(4).standard_normal(ref.shape).astype(np.float32)).to(dev())
    img.backward(dout)
    dh = dout.cpu().numpy()
    ref_dx = constellation_reference_bwd(xh, dh, con)
    e32_dx = np.abs(R.real_backward(xh, dh, con, np.float32).astype(np.float64) - ref_dx).max()
    err_dx = np.abs(x.grad.cpu().numpy().astype(np.float64) - ref_dx).max()
    print(f"{name} backward: E32 {e32_dx:.3e}, kernel {err_dx:.3e} ({err_dx / e32_dx:.3f} E32), largest |dx| {np.abs(ref_dx).max():.3e}")
    assert e32 > 0 and e32_dx > 0
    assert err <= FACTOR * e32
    assert err_dx <= FACTOR * e32_dx


# ---------------------------------------------------------------------------------------------------------------------------
# 4. through Python, 5. independence
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["power", "log"])
def test_x_grad_through_a_vit_equals_the_chained_abi_calls(mode):
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import Constellation
    m = small_vit(1, 32, 64)
    con = Constellation.for_model(m, 128, mode=mode, scale=50.0 if mode == "power" else 1.0)
    assert (con.height, con.width) == (32, 64)
    x0 = zscored_frames((0, 1, 2, 4, 7), 128)
    x = x0.clone().requires_grad_(True)
    m(con(x)).sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and float(x.grad.abs().max()) > 0
    par, tab = con.struct(), con.table_on(dev())
    img = torch.empty(6, 1, 32, 64, device=dev())
    N.check(N.lib().iq_frames_constellation(x0.data_ptr(), tab.data_ptr(), img.data_ptr(), 6, 128, ctypes.byref(par),
                                            N.stream_handle()), "iq_frames_constellation")
    assert torch.equal(img.view(torch.int32), con(x0).view(torch.int32))
    img.requires_grad_(True)
    m(img).sum().backward()
    dx = torch.full_like(x0, SENTINEL)
    N.check(N.lib().iq_frames_constellation_bwd(x0.data_ptr(), tab.data_ptr(), img.grad.contiguous().data_ptr(), dx.data_ptr(),
                                                6, 128, ctypes.byref(par), N.stream_handle()), "iq_frames_constellation_bwd")
    assert torch.equal(dx.view(torch.int32), x.grad.view(torch.int32))
    again = torch.full_like(x0, SENTINEL)
    N.check(N.lib().iq_frames_constellation_bwd(x0.data_ptr(), tab.data_ptr(), img.grad.contiguous().data_ptr(),
                                                again.data_ptr(), 6, 128, ctypes.byref(par), N.stream_handle()),
            "iq_frames_constellation_bwd")
    assert torch.equal(dx.view(torch.int32), again.view(torch.int32))


def test_a_frame_does_not_depend_on_the_call_it_is_part_of():
    from vit_vs_raw_iq_amd import Constellation
    height, width, length = 64, 96, 300
    rng = np.random.default_rng(12)
    x = rng.standard_normal((5, 2, length)).astype(np.float32)
    dout = rng.standard_normal((5, 1, height, width)).astype(np.float32)
    con = Constellation(height, width, length, sigma=1.5, mode="log")
    par = con.struct()
    img = abi_forward(x, con.table, par)
    dx = abi_backward(x, con.table, dout, par)
    order = [3, 0, 4, 2, 1]
    img_p = abi_forward(x[order], con.table, par, expect_kernel=False)
    dx_p = abi_backward(x[order], con.table, dout[order], par, expect_kernel=False)
    assert np.array_equal(bits(img_p), bits(img[order])) and np.array_equal(bits(dx_p), bits(dx[order]))
    for b in range(5):
        one = abi_forward(x[b:b + 1], con.table, par, expect_kernel=False)
        one_dx = abi_backward(x[b:b + 1], con.table, dout[b:b + 1], par, expect_kernel=False)
        assert np.array_equal(bits(one[0]), bits(img[b])) and np.array_equal(bits(one_dx[0]), bits(dx[b])), b


# ---------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import Constellation, IqError
    L = N.lib()
    ARG, UNSUPPORTED = 1, 2
    length = 64
    con = Constellation(32, 64, length)
    x = torch.zeros(2, 2, length, device=dev())
    tab = con.table_on(dev())
    out = torch.full((2, 1, 32, 64), SENTINEL, device=dev())
    dout = torch.ones(2, 1, 32, 64, device=dev())
    dx = torch.full((2, 2, length), SENTINEL, device=dev())
    big = torch.zeros(1, 2, 8193, device=dev())
    big_dx = torch.full((1, 2, 8193), SENTINEL, device=dev())
    st = N.stream_handle()

    def both(par, want, xp=None, tp=None, op=None, dp=None, gp=None, n=2, ln=length):
        xp = x.data_ptr() if xp is None else xp
        tp = tab.data_ptr() if tp is None else tp
        pp = ctypes.byref(par) if par is not None else None
        got = L.iq_frames_constellation(xp, tp, out.data_ptr() if op is None else op, n, ln, pp, st)
        got_b = L.iq_frames_constellation_bwd(xp, tp, dout.data_ptr() if dp is None else dp, dx.data_ptr() if gp is None else gp,
                                              n, ln, pp, st)
        assert (got, got_b) == (want, want), (got, got_b, want)

    def par(**kw):
        p = con.struct()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    nan, inf = float("nan"), float("inf")
    # IQ_STATUS_ARG
    assert L.iq_frames_constellation(None, tab.data_ptr(), out.data_ptr(), 2, length, ctypes.byref(par()), st) == ARG
    assert L.iq_frames_constellation(x.data_ptr(), None, out.data_ptr(), 2, length, ctypes.byref(par()), st) == ARG
    assert L.iq_frames_constellation(x.data_ptr(), tab.data_ptr(), None, 2, length, ctypes.byref(par()), st) == ARG
    assert L.iq_frames_constellation_bwd(x.data_ptr(), tab.data_ptr(), None, dx.data_ptr(), 2, length, ctypes.byref(par()), st) == ARG
    assert L.iq_frames_constellation_bwd(x.data_ptr(), tab.data_ptr(), dout.data_ptr(), None, 2, length, ctypes.byref(par()), st) == ARG
    assert L.iq_frames_constellation_bwd(None, tab.data_ptr(), dout.data_ptr(), dx.data_ptr(), 2, length, ctypes.byref(par()), st) == ARG
    assert L.iq_frames_constellation_bwd(x.data_ptr(), None, dout.data_ptr(), dx.data_ptr(), 2, length, ctypes.byref(par()), st) == ARG
    both(None, ARG)
    both(par(), ARG, ln=0)
    both(par(), ARG, ln=-5)
    both(par(mode=2), ARG)
    both(par(mode=-1), ARG)
    for field in ("x_scale", "x_off", "y_scale", "y_off", "inv_norm", "floor", "scale", "shift"):
        for bad in (nan, inf, -inf):
            both(par(**{field: bad}), ARG)
    both(par(floor=0.0), ARG)
    both(par(floor=-1.0), ARG)
    both(par(), ARG, xp=x.data_ptr() + 2)
    both(par(), ARG, tp=tab.data_ptr() + 1)
    both(par(), ARG, op=out.data_ptr() + 2, dp=dout.data_ptr() + 2)
    both(par(), ARG, op=out.data_ptr() + 1, gp=dx.data_ptr() + 3)
    # an argument error comes before an unsupported size (the neighbours' order)
    both(par(mode=3, height=48), ARG)
    # IQ_STATUS_UNSUPPORTED
    for field in ("height", "width"):
        for bad in (0, 16, 48, 288, -32):
            both(par(**{field: bad}), UNSUPPORTED)
    for bad in (0, 17, -1):
        both(par(radius=bad), UNSUPPORTED)
    for bad in (0, 65, -1):
        both(par(n_frac=bad), UNSUPPORTED)
    both(par(), UNSUPPORTED, xp=big.data_ptr(), gp=big_dx.data_ptr(), n=1, ln=8193)
    # floor <= 0 is allowed in mode 0; n_frames <= 0 succeeds and launches nothing
    assert kernel_launches(L, lambda: both(par(), 0, n=0)) == {}
    assert kernel_launches(L, lambda: both(par(height=48), UNSUPPORTED)) == {}
    both(par(), 0, n=-3)
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL) and torch.all(dx == SENTINEL) and torch.all(big_dx == SENTINEL)
    # mode 0 takes any finite floor; len 8192 is taken
    p0 = par(mode=0, floor=0.0)
    assert L.iq_frames_constellation(x.data_ptr(), tab.data_ptr(), out.data_ptr(), 2, length, ctypes.byref(p0), st) == 0
    # Python: argument checks before any device work, CPU tensors refused
    with pytest.raises(IqError, match="no CPU fallback"):
        con(torch.zeros(2, 2, length))
    with pytest.raises(ValueError):
        con(torch.zeros(2, 2, length + 1, device=dev()))
    with pytest.raises(ValueError):
        Constellation(48, 64, length)
    with pytest.raises(ValueError):
        Constellation(32, 64, 8193)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. integration
# ---------------------------------------------------------------------------------------------------------------------------
STATS = {"i_mean": 0.01, "i_std": 0.9, "q_mean": -0.02, "q_std": 1.1}


def direct(raw, layout, h, w, imp=None, seed=0, step=0, frame_base=0):
    """The parent's output: iq_frames_preprocess / iq_frames_impair called directly."""
    import vit_vs_raw_iq_amd._native as N
    B, length = raw.shape[0], raw.shape[1]
    take = length if layout == "rawiq" else h * w // 2
    out = torch.empty(B, 2, take, device=dev())
    st = (ctypes.c_float * 4)(STATS["i_mean"], STATS["i_std"], STATS["q_mean"], STATS["q_std"])
    if imp is None:
        N.check(N.lib().iq_frames_preprocess(raw.data_ptr(), out.data_ptr(), B, length, take, st, N.stream_handle()),
                "iq_frames_preprocess")
    else:
        par = imp.struct(seed, step, frame_base)
        N.check(N.lib().iq_frames_impair(raw.data_ptr(), out.data_ptr(), None, B, length, take, st, ctypes.byref(par),
                                         N.stream_handle()), "iq_frames_impair")
    return out.view(B, 1, h, w) if layout == "vit" else out


def test_the_spectrogram_keyword_is_the_rawiq_call_followed_by_the_constellation():
    from vit_vs_raw_iq_amd import Constellation, FrameSynth, Impairments, SynthStream, data as D, impair
    fs = FrameSynth(["BPSK", "QPSK", "16QAM", "GMSK"], snrs_db=(0.0, 20.0), length=1024, seed=5, device=dev())
    con = Constellation(32, 64, 1024)
    aug = Impairments(phase=(-1.0, 1.0), cfo=(-0.01, 0.01), shift_max=100, snr_db=(5.0, 15.0))
    raw = fs.generate(8, 24, 0)[0]
    for imp in (None, aug):
        x, y, z = SynthStream(fs, STATS, "vit", 8, augment=imp, spectrogram=con).get(3)
        x0, y0, z0 = SynthStream(fs, STATS, "rawiq", 8, augment=imp).get(3)
        assert x.shape == (8, 1, 32, 64) and same_bits(x, con(x0)) and torch.equal(y, y0) and same_bits(z, z0)
        # spectrogram=None: the parent's outputs, bit for bit
        want = direct(raw, "vit", 32, 32, imp, seed=fs.seed, step=0, frame_base=24)
        assert same_bits(SynthStream(fs, STATS, "vit", 8, h=32, w=32, augment=imp).get(3)[0], want)
        assert same_bits(x0, direct(raw, "rawiq", 0, 0, imp, seed=fs.seed, step=0, frame_base=24))
        host = raw.cpu().numpy()
        got = D.DeviceInputPipeline(STATS, "vit", batch=8, augment=imp, seed=9, spectrogram=con)(host)
        plain = D.DeviceInputPipeline(STATS, "rawiq", batch=8, augment=imp, seed=9)(host)
        assert got.shape == (8, 1, 32, 64) and same_bits(got, con(plain))
        assert same_bits(plain, direct(raw, "rawiq", 0, 0, imp, seed=9))
        assert same_bits(D.DeviceInputPipeline(STATS, "vit", batch=8, h=32, w=32, augment=imp, seed=9)(host),
                         direct(raw, "vit", 32, 32, imp, seed=9))
    got, drawn = impair(raw, STATS, "vit", aug, seed=4, step=2, frame_base=7, return_drawn=True, spectrogram=con)
    plain, drawn0 = impair(raw, STATS, "rawiq", aug, seed=4, step=2, frame_base=7, return_drawn=True)
    assert got.shape == (8, 1, 32, 64) and same_bits(got, con(plain)) and same_bits(drawn, drawn0)
    assert same_bits(plain, direct(raw, "rawiq", 0, 0, aug, seed=4, step=2, frame_base=7))
    assert same_bits(impair(raw, STATS, "vit", aug, seed=4, step=2, frame_base=7), direct(raw, "vit", 32, 64, aug, 4, 2, 7))


def test_a_vit_trains_on_constellations_of_received_symbols_and_the_curve_runs():
    from vit_vs_raw_iq_amd import (Constellation, Impairments, ReceivedSynth, Receiver, ShapedSynth, SynthStream, impair,
                                   impairment_curve, train_on_stream)
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    ws = ShapedSynth(["BPSK", "QPSK", "16QAM", "OQPSK"], snrs_db=(20.0,), length=1024, seed=11, sps=8)
    rs = ReceivedSynth(ws, Receiver.for_synth(ws))
    assert rs.length == 128
    stats = rs.stats(n_subset=64)
    m = small_vit(1, 32, 64).train()
    con = Constellation.for_model(m, rs.length)
    sym, y, _ = rs.generate(64, 0, 1)
    x = impair(sym, stats, "rawiq", Impairments())
    con.fit(x)
    img = con(x)
    assert abs(float(img.mean())) < 1e-3 and abs(float(img.std()) - 1.0) < 1e-3
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-3)
    assert train_on_stream(tr, SynthStream(rs, stats, "vit", 32, spectrogram=con), 4) == 4
    loss, _, frames = tr.read_stats()
    assert frames == 128 and np.isfinite(loss) and loss > 0
    after = m.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    assert sum(int(not torch.equal(before[k], after[k])) for k in before) >= len(before) // 2
    values = [0.0, 0.5, 1.0]
    curve = impairment_curve(m, sym, y, stats, "phase", values, spectrogram=con, batch=32)
    assert len(curve) == 3 and all(0.0 <= a <= 1.0 for a in curve)
    assert curve == impairment_curve(m, sym, y, stats, "phase", values, spectrogram=con, batch=64)
    with pytest.raises(ValueError):
        impairment_curve(m, sym, y, stats, "phase", values, spectrogram=Constellation(32, 32, rs.length))
    with pytest.raises(ValueError):
        impairment_curve(m, sym, y, stats, "phase", values, spectrogram=Constellation(64, 64, rs.length))
