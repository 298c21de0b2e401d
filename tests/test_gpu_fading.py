"""iq_frames_fade on the device (csrc/fading.hip): bit for bit against the fp32 restatement of tests/fading_ref.py where every
operation is exact, under the derived running-error bound against fading_reference where the tables are real, what the drawn mode
draws, the tail (unit power, noise at the given SNR), the invariances of a keyed per-frame kernel, the refusals, and the plumbing
(FadedSynth through SynthStream and ReceivedSynth, a captured call, fading_curve).  Every call of the C ABI goes through
frontend_gpu.abi_call: fenced outputs, NaN around the operands, the launched kernel asserted by name."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fading_ref as R
from frontend_gpu import ISENT, SENTINEL, abi_call, bits, dev, on_device, same_bits
from prof_names import kernel_launches

pytestmark = pytest.mark.gpu

KERNEL = "frames_fade_kernel"
NEUTRAL = dict(taps=1, rice_k_db=math.inf, sinusoids=0, doppler=0.0, clock_ppm=0.0, start=0, timing=False, K=1, n_frac=1, normalise=False)
GIVEN, DRAWN = 0, 1


def fade(fd, x, mode=DRAWN, paths=None, amps=None, clock=None, snr=None, seed=0, stream=0, base=0):
    """One guarded call -> y (n, len_out, 2) fp32, paths_out int64 (n, 8, 33, 2), amps_out fp32 (n, 8, 33), clock_out int64 (n, 2)."""
    n = len(x)
    side = [fd.interp, snr, None if paths is None else np.asarray(paths).astype(np.int32), amps,
            None if clock is None else np.ascontiguousarray(clock, dtype=np.int64).view(np.int32).reshape(n, 4)]

    def par(interp, snr_db, p, a, c):
        return fd.struct(mode, interp=interp, snr_db=snr_db, paths=p, amps=a, clock=c, seed=seed, stream=stream, frame_base=base)
    y, po, ao, co = abi_call("iq_frames_fade", KERNEL, [x], [(n, fd.length_out, 2), (np.int32, n, 8, 33, 2), (n, 8, 33), (np.int32, n, 4)],
                             n, fd.length_out, par, side=side)
    return y, po.astype(np.int64), ao, np.ascontiguousarray(co).view(np.int64).reshape(n, 2)


def frames(seed, n, length):
    return np.random.default_rng(seed).standard_normal((n, length, 2)).astype(np.float32)


def c64(y):
    return y[..., 0].astype(np.float64) + 1j * y[..., 1].astype(np.float64)


# ---- exact
@pytest.mark.parametrize("name", list(R.exact_cases()))
def test_exact_cases_bit_for_bit(name):
    from vit_vs_raw_iq_amd import Fading
    kw, x, paths, amps, clock = R.exact_cases()[name]
    fd = Fading(**kw)
    y, po, ao, co = fade(fd, x, GIVEN, paths, amps, clock)
    assert np.array_equal(bits(y), bits(R.restate32(x, paths, amps, clock, fd)))
    assert np.array_equal(po, paths) and np.array_equal(bits(ao), bits(amps)) and np.array_equal(co, clock)      # what was used


def test_the_largest_frames_that_fit_and_one_size_above_refused():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import Fading
    rng = np.random.default_rng(5)
    table = rng.integers(-3, 4, size=(256, 16)).astype(np.float32)
    fd = Fading(8192, 8192, taps=2, sinusoids=1, K=16, n_frac=256, delay=(0.0, 2.75), normalise=False, interp=table)
    x = R.integer_frames(rng, 1, 8192)
    paths, amps = R.tables(1)
    paths[0, :2, :2] = rng.integers(-2, 2, size=(2, 2, 2)) * 2 ** 30
    amps[0, :2, :2] = [[2.0, -1.0], [1.0, 3.0]]
    clock = R.clock_of((9 << 32) + 0xFFFFFFFF, -(1 << 21))
    y, _, _, _ = fade(fd, x, GIVEN, paths, amps, clock)
    assert np.array_equal(bits(y), bits(R.restate32(x, paths, amps, clock, fd)))
    # one sample more, on either side: refused before any launch, the output untouched
    L = N.lib()
    out = torch.full((8193 * 2,), SENTINEL, dtype=torch.float32, device=dev())
    xin, tab = torch.zeros(8193 * 2, device=dev()), on_device(table)
    for len_in, len_out in ((8193, 8192), (8192, 8193)):
        par = fd.struct(DRAWN, interp=tab.data_ptr())
        par.len_in = len_in
        rc = []
        assert kernel_launches(L, lambda: rc.append(L.iq_frames_fade(xin.data_ptr(), out.data_ptr(), None, None, None, 1, len_out,
                                                                      ctypes.byref(par), N.stream_handle()))) == {}
        assert rc == [2] and bool((out == SENTINEL).all())


def test_the_neutral_setting_returns_its_input_bit_for_bit():
    from vit_vs_raw_iq_amd import Fading
    for length in (1, 255, 1000):
        x = frames(length, 3, length)
        fd = Fading(length, length, **NEUTRAL)
        y, po, ao, co = fade(fd, x, DRAWN, seed=11, base=5)
        assert np.array_equal(bits(y), bits(x))
        assert not po.any() and ao[:, 0, 0].tolist() == [1.0] * 3 and np.count_nonzero(ao) == 3 and np.array_equal(co, R.clock_of(0, 0, 3))
    # and through the Python surface, with a Kaiser table whose phase 0 is the unit spike
    xd = on_device(frames(1, 4, 512))
    assert same_bits(Fading(512, 512, **{**NEUTRAL, "K": 9, "n_frac": 128, "start": 0})(xd, seed=3), xd)


# ---- real tables under the derived bound
@pytest.mark.parametrize("name", list(R.real_cases()))
def test_real_tables_under_the_derived_bound(name):
    from vit_vs_raw_iq_amd import Fading, fading_reference
    kw, x, paths, amps, clock, _ = R.real_cases()[name]
    fd = Fading(**kw)
    y, po, ao, co = fade(fd, x, GIVEN, paths, amps, clock)
    ref = fading_reference(x, po, ao, co, fd)                      # the device's own tables
    _, bound = R.definition64(x, po, ao, co, fd)
    err = np.abs(y.astype(np.float64) - ref).max(axis=2)
    print(name, "worst error / bound", (err / bound).max())
    assert np.all(err <= bound), (err / bound).max()


def test_a_drawn_channel_under_the_derived_bound():
    from vit_vs_raw_iq_amd import Fading, fading_reference
    fd = Fading(600, 513, taps=4, sinusoids=16, doppler=(1e-4, 4e-3), clock_ppm=(-200.0, 200.0), timing=True, normalise=False)
    x = frames(9, 6, 600)
    y, po, ao, co = fade(fd, x, DRAWN, seed=2 ** 40 + 7, stream=3, base=2 ** 33)
    _, bound = R.definition64(x, po, ao, co, fd)
    err = np.abs(y.astype(np.float64) - fading_reference(x, po, ao, co, fd)).max(axis=2)
    print("drawn: worst error / bound", (err / bound).max())
    assert np.all(err <= bound) and np.isfinite(y).all() and np.abs(y).max() > 0.1
    fn = Fading(**{**fd._kw, "normalise": True})
    yn, _, _, _ = fade(fn, x, DRAWN, seed=2 ** 40 + 7, stream=3, base=2 ** 33)
    refn = fading_reference(x, po, ao, co, fn)
    # the scaling: one more rounding per sample and the power's own error (below): a relative (len / 256 + 20) u on top of the bound
    scale = 1.0 / np.sqrt((np.abs(c64(y)) ** 2).mean(axis=1, keepdims=True))
    assert np.all(np.abs(yn.astype(np.float64) - refn).max(axis=2) <= bound * scale + (513 / 256 + 20) * R.U * np.abs(refn).max(axis=2))


# ---- what the drawn mode draws
def test_what_the_drawn_mode_draws():
    from vit_vs_raw_iq_amd import Fading
    B, taps, ns = 64, 8, 32
    fd = Fading(16, 16, taps=taps, sinusoids=ns, doppler=1e-3, clock_ppm=(-100.0, 200.0), timing=True, start=2, rice_k_db=3.0, decay=0.8)
    _, po, ao, co = fade(fd, frames(0, B, 16), DRAWN, seed=5, stream=1, base=1000)
    fd_inc = int(np.rint(float(np.float32(1e-3)) * 2.0 ** 32))
    inc = po[:, :, :, 1]
    assert np.abs(inc).max() <= fd_inc and np.abs(inc).max() > 0.99 * fd_inc
    assert not po[:, :, 0, 0].any() and len(np.unique(po[:, :, 1:, 0])) > 0.99 * B * taps * ns          # the line of sight starts at phase 0
    d = co[:, 1] - 2 ** 32
    assert d.min() >= fd.drift[0] and d.max() <= fd.drift[1] and len(np.unique(d)) > B // 2
    assert np.array_equal(co[:, 0] >> 32, np.full(B, 2)) and len(np.unique(co[:, 0] & 0xFFFFFFFF)) > B // 2
    scale = np.sqrt(np.float32(2.0) / np.float32(ns))
    for l in range(taps):
        assert np.array_equal(bits(ao[:, l, 0]), bits(np.full(B, fd.los[l])))
        assert np.array_equal(bits(ao[:, l, 1:]), bits(np.full((B, ns), np.float32(fd.tap_sigma[l]) * scale)))
    # E|g_l|^2 = los^2 + 2 sigma^2 by construction of the amplitudes (sum of squares; fp32 rounding of each amplitude: 2 u each)
    power = (ao.astype(np.float64) ** 2).sum(axis=2)[0]
    want = np.array([lo * lo + 2 * s * s for lo, s in zip(fd.los, fd.tap_sigma)])
    assert np.allclose(power, want, rtol=8 * R.U, atol=0)
    # Clarke: the mean of cos(2 pi n inc 2^-32) over N paths is J0(2 pi n fd) within five standard errors; the variance of a cosine
    # is at most 1/2, so sqrt(1 / N) bounds the standard error
    N = inc.size
    assert N >= 16384
    for lag in (100, 300, 700):
        got = np.cos(2 * np.pi * lag * inc.astype(np.float64) / 2.0 ** 32).mean()
        j0 = float(torch.special.bessel_j0(torch.tensor(2 * np.pi * lag * fd_inc / 2.0 ** 32, dtype=torch.float64)))
        print("lag", lag, "mean", got, "J0", j0, "standard errors", abs(got - j0) * math.sqrt(N))
        assert abs(got - j0) <= 5.0 * math.sqrt(1.0 / N)
    # a range of Doppler spreads: one fd per frame, inside the range; fewer taps and paths leave the other slots zero
    fr = Fading(16, 16, taps=2, sinusoids=8, doppler=(1e-3, 5e-3))
    _, po, ao, _ = fade(fr, frames(0, 32, 16), DRAWN, seed=6)
    peak = np.abs(po[:, :, :, 1]).reshape(32, -1).max(axis=1)
    assert peak.max() <= np.rint(float(np.float32(5e-3)) * 2.0 ** 32) and peak.min() > 0.5 * 1e-3 * 2.0 ** 32 and len(np.unique(peak)) > 16
    assert not po[:, 2:].any() and not po[:, :, 9:].any() and not ao[:, 2:].any() and not ao[:, :, 9:].any()


# ---- the tail
def test_normalisation_gives_unit_power():
    from vit_vs_raw_iq_amd import Fading
    for length, taps in ((1, 1), (255, 2), (1000, 3)):
        fd = Fading(length + 10, length, taps=taps, sinusoids=4, doppler=2e-3)
        y, _, _, _ = fade(fd, 3.0 * frames(length, 4, length + 10), DRAWN, seed=1)
        p = (np.abs(c64(y)) ** 2).mean(axis=1)
        # the power sum (len / 256 additions per thread, a butterfly, four wave sums), the reciprocal square root (three
        # operations) and one rounding of every output sample, squared: (len / 256 + 20) u; the 1e-12 under the root is below that
        assert np.all(np.abs(p - 1.0) <= (length / 256 + 20) * R.U), p


def test_the_noise_has_the_given_power_and_a_nan_switches_it_off_for_that_frame_only():
    from vit_vs_raw_iq_amd import Fading
    B, length = 8, 2048
    fd = Fading(length, length, taps=2, sinusoids=4, doppler=1e-3)
    x = frames(4, B, length)
    snr = np.array([0.0, 10.0, np.nan, 20.0, -5.0, np.nan, 3.0, 30.0], np.float32)
    clean, _, _, _ = fade(fd, x, DRAWN, seed=8)
    noisy, _, _, _ = fade(fd, x, DRAWN, snr=snr, seed=8)
    for i in range(B):
        if np.isnan(snr[i]):
            assert np.array_equal(bits(noisy[i]), bits(clean[i]))
            continue
        w = c64(noisy[i]) - c64(clean[i])
        want = 10.0 ** (-snr[i] / 10.0)
        got = (np.abs(w) ** 2).mean()
        # |w|^2 is exponential: its deviation is its mean; the rounding of signal + noise (u of a value of a few units) is far below
        print("snr", snr[i], "noise power", got, "wanted", want, "standard errors", abs(got - want) / (want / math.sqrt(length)))
        assert abs(got - want) <= 5.0 * want / math.sqrt(length)
        assert abs(w.real.mean()) <= 5.0 * math.sqrt(want / 2 / length) and abs(w.imag.mean()) <= 5.0 * math.sqrt(want / 2 / length)
    # the noise of a frame is keyed by its index, not by its place in the call
    again, _, _, _ = fade(fd, x[3:5], DRAWN, snr=snr[3:5], seed=8, base=3)
    assert np.array_equal(bits(again), bits(noisy[3:5]))


# ---- invariances
def test_batch_invariance_run_to_run_identity_and_stream_cuts():
    from vit_vs_raw_iq_amd import Fading
    fd = Fading(300, 257, taps=3, sinusoids=8, doppler=(0.0, 3e-3), clock_ppm=(-100.0, 100.0), timing=True)
    x = frames(2, 5, 300)
    snr = np.array([5.0, 10.0, np.nan, 15.0, 20.0], np.float32)
    whole = fade(fd, x, DRAWN, snr=snr, seed=21, stream=2, base=2 ** 32 - 2)          # the frame index crosses 2^32
    again = fade(fd, x, DRAWN, snr=snr, seed=21, stream=2, base=2 ** 32 - 2)
    for a, b in zip(whole, again):
        assert np.array_equal(a, b) and a.tobytes() == b.tobytes()
    for lo, hi in ((0, 2), (2, 5), (4, 5)):
        part = fade(fd, x[lo:hi], DRAWN, snr=snr[lo:hi], seed=21, stream=2, base=2 ** 32 - 2 + lo)
        for a, b in zip(whole, part):
            assert a[lo:hi].tobytes() == b.tobytes()
    other = fade(fd, x, DRAWN, snr=snr, seed=21, stream=3, base=2 ** 32 - 2)
    assert not np.array_equal(other[1], whole[1]) and not np.array_equal(other[0], whole[0])


def test_a_nan_frame_stays_alone():
    from vit_vs_raw_iq_amd import Fading
    fd = Fading(200, 200, taps=2, sinusoids=2, doppler=1e-3)
    x = frames(3, 3, 200)
    good, _, _, _ = fade(fd, x, DRAWN, seed=4)
    x[1] = np.nan
    bad, _, _, _ = fade(fd, x, DRAWN, seed=4)
    assert np.isnan(bad[1]).all() and np.array_equal(bits(bad[[0, 2]]), bits(good[[0, 2]]))


# ---- refusals
def test_every_refusal_comes_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import Fading
    L = N.lib()
    fd = Fading(64, 64, taps=2, sinusoids=4, doppler=1e-3)
    x, tab = on_device(frames(0, 2, 64)), on_device(fd.interp)
    y = torch.full((2, 64, 2), SENTINEL, dtype=torch.float32, device=dev())
    po = torch.full((2, 8, 33, 2), ISENT, dtype=torch.int32, device=dev())
    changes = [dict(mode=2), dict(len_in=0), dict(n_taps=0), dict(K=0), dict(n_frac=0), dict(n_sin=-1), dict(fd_hi=0.6), dict(fd_lo=0.1),
               dict(d_lo=1), dict(normalise=3), dict(interp=None), dict(mode=0), dict(snr_db=tab.data_ptr() + 2),
               dict(n_taps=9), dict(n_sin=33), dict(K=17), dict(n_frac=257), dict(len_in=8193)]
    for ch in changes:
        par = fd.struct(DRAWN, interp=tab.data_ptr())
        for k, v in ch.items():
            setattr(par, k, v)
        rc = []
        assert kernel_launches(L, lambda: rc.append(L.iq_frames_fade(x.data_ptr(), y.data_ptr(), po.data_ptr(), None, None, 2, 64,
                                                                      ctypes.byref(par), N.stream_handle()))) == {}, ch
        assert rc[0] in (1, 2), ch
    par = fd.struct(DRAWN, interp=tab.data_ptr())
    par.delay[1] = -1
    assert L.iq_frames_fade(x.data_ptr(), y.data_ptr(), po.data_ptr(), None, None, 2, 64, ctypes.byref(par), N.stream_handle()) == 1
    par = fd.struct(DRAWN, interp=tab.data_ptr())
    assert kernel_launches(L, lambda: L.iq_frames_fade(x.data_ptr(), y.data_ptr(), po.data_ptr(), None, None, 0, 64, ctypes.byref(par),
                                                       N.stream_handle())) == {}
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((po == ISENT).all())


# ---- plumbing
def _synths(snrs=(20.0,)):
    from vit_vs_raw_iq_amd import FadedSynth, Fading, ShapedSynth
    ws = ShapedSynth(["BPSK", "QPSK", "8PSK", "16QAM"], snrs_db=snrs, length=1024, sps=4, seed=12, device=dev())
    fd = Fading(1100, 1024, taps=2, sinusoids=8, doppler=(0.0, 1e-3), clock_ppm=(0.0, 50.0))
    return ws, fd, FadedSynth(ws, fd)


def test_faded_synth_is_a_keyed_stream_and_goes_through_synthstream_and_receivedsynth():
    from vit_vs_raw_iq_amd import Fading, ReceivedSynth, Receiver, SynthStream, fading_reference
    ws, fd, fs = _synths(snrs=(10.0, 20.0))
    raw, y, z, paths, amps, clock = fs.generate(12, 4, stream=1, return_tables=True)
    assert raw.shape == (12, 1024, 2) and torch.isfinite(raw).all()
    assert torch.equal(y, ws.generate(12, 4, stream=1)[1]) and torch.equal(y.cpu(), (torch.arange(4, 16) % 4))
    assert z.cpu().tolist() == [(10.0, 20.0)[(j // 4) % 2] for j in range(4, 16)]
    # the noiseless part is the channel applied to the synth's noiseless frames at the channel's input length
    quiet = Fading(**{**fd._kw})(fs._clean.generate(12, 4, stream=1)[0], None, ws.seed, 1, 4)
    ref = fading_reference(fs._clean.generate(12, 4, stream=1)[0], paths, amps, clock, fd)
    assert np.abs(quiet.cpu().numpy() - ref).max() < 1e-4
    resid = (raw - quiet).cpu().numpy()
    first = (z == z[0]).cpu().numpy()                      # eight frames of 1024 samples at one SNR: a standard error of 1.1 %
    assert first.sum() == 8 and abs((resid[first] ** 2).sum(axis=2).mean() / 10.0 ** (-z[0].item() / 10) - 1) < 5 * 0.011
    # cut differently, the same frames
    assert same_bits(torch.cat([fs.generate(5, 4, stream=1)[0], fs.generate(7, 9, stream=1)[0]]), raw)
    stats = dict(i_mean=0.0, i_std=1.0, q_mean=0.0, q_std=1.0)
    a = SynthStream(fs, stats, "rawiq", batch=8, stream=1)
    b = SynthStream(fs, stats, "rawiq", batch=4, stream=1)
    xa, ya, za = a.get(1)
    assert xa.shape == (8, 2, 1024) and same_bits(xa, torch.cat([b.get(2)[0], b.get(3)[0]])) and torch.equal(ya, torch.arange(8, 16, device=dev()) % 4)
    assert same_bits(xa[0], fs.generate(1, 8, stream=1)[0][0].t().contiguous())
    rs = ReceivedSynth(fs, Receiver.for_synth(fs))
    sym, ys, zs = rs.generate(8, 8, stream=1)
    assert sym.shape == (8, 256, 2) and torch.isfinite(sym).all() and torch.equal(ys, ya) and float(sym.pow(2).sum(-1).mean()) > 0.1


def test_one_captured_and_replayed_call():
    from vit_vs_raw_iq_amd import Fading
    fd = Fading(520, 500, taps=3, sinusoids=8, doppler=(0.0, 2e-3), clock_ppm=(-20.0, 20.0), timing=True)
    xs = on_device(frames(6, 8, 520))
    a, b = xs[:4].clone(), xs[4:].clone()
    snr = torch.tensor([10.0, float("nan"), 0.0, 20.0], device=dev())
    eager_a, eager_b = fd(a, snr, seed=3, frame_base=10), fd(b, snr, seed=3, frame_base=10)     # also: the table is on the device
    torch.cuda.synchronize()
    held_in = a.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        held = fd(held_in, snr, seed=3, frame_base=10)
    held.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(held, eager_a)
    held_in.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(held, eager_b)


def test_fading_curve_at_the_neutral_value_is_the_plain_accuracy():
    from vit_vs_raw_iq_amd import FadedSynth, Fading, ShapedSynth, fading_curve
    ws = ShapedSynth(["BPSK", "QPSK", "16QAM"], snrs_db=(), length=512, sps=4, seed=2, device=dev())
    neutral = Fading(512, 512, **NEUTRAL)

    def predict(raw):                                       # a fixed rule on the fourth moment: some frames right, some wrong
        k = raw.pow(2).sum(-1).pow(2).mean(1) / raw.pow(2).sum(-1).mean(1).pow(2)
        return (k > 1.45).long() + (k > 1.6).long()
    n = 96
    raw, y, _ = ws.generate(n, 0, stream=1)
    assert same_bits(FadedSynth(ws, neutral).generate(n, 0, stream=1)[0], raw)
    plain = float((predict(raw) == y).float().mean())
    assert 0.0 < plain < 1.0
    assert fading_curve(predict, ws, neutral, "doppler", [0.0], n=n, batch=32, stream=1) == [plain]
    assert fading_curve(predict, ws, neutral, "clock_ppm", [0.0], n=n, batch=96, stream=1) == [plain]
    # the result does not depend on the batch; a moving channel changes the frames
    moving = Fading(560, 512, taps=2, sinusoids=8, normalise=True)
    c1 = fading_curve(predict, ws, moving, "doppler", [0.0, 2e-3], n=n, batch=17, stream=1)
    c2 = fading_curve(predict, ws, moving, "doppler", [0.0, 2e-3], n=n, batch=96, stream=1)
    assert c1 == c2 and all(0.0 <= v <= 1.0 for v in c1)
    assert len(fading_curve(predict, ws, moving, "rice_k_db", [-10.0, 10.0, math.inf], n=24, batch=24, stream=1)) == 3
