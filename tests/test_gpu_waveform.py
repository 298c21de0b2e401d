"""GPU (MI355X): pulse-shaped labelled frames made on the device (csrc/waveform.hip, iq_frames_waveform,
vit_vs_raw_iq_amd.waveform).

1. The integer part -- class, SNR, timing phase, symbols -- against the host restatement of tests/waveform_ref.py (the counter
   layout of include/iqvit.h on tests/dropout_ref.philox4x32): equal as integers, bitwise for the SNR.
2. The channel taps against an fp64 Box-Muller of the same words.
3. The deterministic part (shaping, channel, carrier phase, unit power) against the host fp64 definition waveform_reference.
4. Identity: sps = span = n_phase = 1, pulse 1.0, no timing, one tap = iq_frames_synth, bit for bit, noise included.
5. Exact structure with an all-ones pulse.  6. Occupied bandwidth of the kernel's output.  7. Keying.  8. Noise statistics.
9. Refusals leave the outputs untouched; outputs carved out of a patterned buffer leave every byte around them unchanged.
10. SynthStream / hipGraph / train_on_stream take a ShapedSynth as they take a FrameSynth.

Shapes: (a) len 1024, sps 8, span 8, 32 phases, 3 taps -- the task; (b) len 33, sps 3, span 5, 7 phases, 2 taps -- odd
everywhere: the Philox tail, the OQPSK offset sps/2 = 1, a partial scan chunk, 8-byte stores; (c) len 8192, sps 1, span 32,
8 taps -- the LDS limit, 19 frames.  76 frames = 19 classes x 4 SNRs, no multiple of any block size.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from frontend_gpu import dev, same_bits
from waveform_ref import band_edge, host_frame, out_of_band_fraction

pytestmark = pytest.mark.gpu

SHAPES = {"a": dict(length=1024, sps=8, span=8, n_phase=32, taps=3),
          "b": dict(length=33, sps=3, span=5, n_phase=7, taps=2),
          "c": dict(length=8192, sps=1, span=32, n_phase=4, taps=8)}
FRAMES = {"a": 76, "b": 76, "c": 19}
EVERYTHING = dict(return_drawn=True, return_symbols=True, return_taps=True)


def check_integers(ws, n, frame_base, stream, frames):
    raw, y, z, drawn, sym, taps = ws.generate(n, frame_base, stream, **EVERYTHING)
    y, z, drawn, sym = y.cpu().numpy(), z.cpu().numpy(), drawn.cpu().numpy(), sym.cpu().numpy()
    assert y.dtype == np.int64 and z.dtype == np.float32 and sym.dtype == np.int32
    assert raw.shape == (n, ws.length, 2) and sym.shape == (n, ws.n_symbols) and drawn.shape == (n, 8) and taps.shape == (n, 8, 2)
    assert np.all(drawn[:, 6:] == 0)
    kinds, phases = set(), set()
    for i in frames:
        cls, snr, theta, q, ref, _ = host_frame(ws, frame_base + i, stream)
        kinds.add(ws.descriptors[cls][0])
        phases.add(q)
        assert y[i] == cls and drawn[i, 0] == cls, (i, y[i], cls)
        assert z[i].view(np.int32) == snr.view(np.int32) and drawn[i, 1].view(np.int32) == snr.view(np.int32), (i, z[i], snr)
        assert abs(float(drawn[i, 2]) - float(theta)) <= 2.0 ** -23 * float(theta), (i, drawn[i, 2], theta)       # one fp32 product
        assert drawn[i, 4] == q, (i, drawn[i, 4], q)
        assert np.array_equal(sym[i].astype(np.int64), ref), (i, ws.class_names[cls], np.flatnonzero(sym[i] != ref)[:8])
    return kinds, phases


@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_symbols_labels_snrs_and_timing_phases_are_the_host_restatement(shape):
    from vit_vs_raw_iq_amd import ShapedSynth
    ws = ShapedSynth(seed=0x1234567800000011, **SHAPES[shape])
    # balanced: every class at every SNR (a third of the frames at the LDS limit, GMSK and OQPSK among them)
    kinds, phases = check_integers(ws, 76, 0, 0, range(76) if shape != "c" else range(1, 76, 3))
    assert kinds == {0, 1, 2} and len(phases) > 1
    # a frame index past 2^32 (its high word is part of the key) on another stream: classes 11..18, 0..12
    assert check_integers(ws, 21, 2 ** 32 + 5, 1, range(21))[0] == {0, 1, 2}
    if shape != "c":
        # class and SNR drawn from words 1 and 2 of the frame's parameters
        un = ShapedSynth(seed=7, balanced=False, **SHAPES[shape])
        assert 0 in check_integers(un, 76, 2 ** 32 + 5, 1, range(0, 76, 3))[0]
        g = ShapedSynth(["GMSK", "OQPSK", "QPSK"], None, seed=9, balanced=False, **SHAPES[shape])
        assert check_integers(g, 12, 3, 0, range(12))[0] == {0, 1, 2}
        # no timing: q = 0 whatever word 3 holds
        fixed = ShapedSynth(seed=9, timing=False, **SHAPES[shape])
        assert check_integers(fixed, 19, 0, 0, range(19))[1] == {0}


@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_channel_taps_match_an_fp64_box_muller_of_the_host_words(shape):
    """g = r (cos, sin)(2 pi u_b), r = sqrt(-2 log u_a), u_a in [2^-24, 1], u_b a 24-bit fraction (exact in fp32).  fp32: logf is
    within 1 ulp, so -2 log u_a (at most 33.3) carries 2^-23 relative; the square root halves that and adds 2^-24: r within
    1.2e-7 relative, r <= 5.77.  sincospif of the exact argument 2 u_b is within 2 ulp of values <= 1: 2.4e-7 absolute.  The
    product r * cos and the product with tap_sigma add 2^-24 relative each.  |g| <= 5.77, so the error of tap_sigma * g is at most
    tap_sigma * 5.77 * (1.2e-7 + 2.4e-7 + 1.2e-7) = 2.8e-6 tap_sigma; adding los (exact: the fp32 value the kernel is given)
    rounds once more, 2^-24 |h| <= 6e-8 (los + 5.77 tap_sigma) -- with los <= 3 tap_sigma[0] in these profiles another 5e-7
    tap_sigma.  Bound: 1e-5 tap_sigma, absolute.  Taps beyond L are exactly zero; L = 1 is the tap (1, 0) with nothing drawn."""
    from vit_vs_raw_iq_amd import ShapedSynth
    ws = ShapedSynth(seed=21, **SHAPES[shape])
    n, L = FRAMES[shape], SHAPES[shape]["taps"]
    for base, stream in ((0, 0), (2 ** 32 + 5, 1)):
        _, _, _, drawn, _, taps = ws.generate(n, base, stream, **EVERYTHING)
        got, d = taps.cpu().numpy().astype(np.float64), drawn.cpu().numpy().astype(np.float64)
        ref = np.stack([host_frame(ws, base + i, stream)[5] for i in range(n)])
        bound = 1e-5 * np.array(list(ws.tap_sigma) + [0.0] * (8 - L))[None, :, None]
        err = np.abs(got - ref)
        print(f"shape {shape}: max |tap - fp64| / tap_sigma = {(err[:, :L] / np.array(ws.tap_sigma)[None, :, None]).max():.3e}")
        assert np.all(err <= bound), (err / np.maximum(bound, 1e-30)).max()
        assert np.all(got[:, L:] == 0)
        power = (got ** 2).sum(axis=(1, 2))
        assert np.all(np.abs(d[:, 5] - power) <= 2e-6 * power)          # 2 L fp32 fmaf
    one = ShapedSynth(seed=21, **dict(SHAPES[shape], taps=1))
    _, _, _, drawn, _, taps = one.generate(5, 0, 0, **EVERYTHING)
    want = torch.zeros(5, 8, 2)
    want[:, 0, 0] = 1.0
    assert torch.equal(taps.cpu(), want) and torch.equal(drawn[:, 5].cpu(), torch.ones(5))


@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_deterministic_part_matches_the_fp64_reference(shape):
    """The bounds tests/test_gpu_synth.py carries for the same rotate-and-scale: 1e-4 of the frame's peak, absolute, and 1e-5 on
    the power of the result.  In front of it here: a shaped sample is a product and span - 1 fmaf, each rounding once, so it is
    within span 2^-24 sum_i |a_i p_i| of the exact sum over the fp32 table; the channel is L complex products accumulated the same
    way: together (span + L) 2^-24 sum |a_i p_i| <= 40 * 6e-8 = 2.4e-6 of sum |a_i p_i| at the largest span, and that sum is a
    few times the frame's peak (the tails of the pulse are small) -- well inside the 1e-4.  GMSK: the phase is exact as an
    integer; its conversion to fp32 rounds at 2^-25 turn = 2e-7 rad."""
    from vit_vs_raw_iq_amd import ShapedSynth, waveform_reference
    n = FRAMES[shape]
    ws = ShapedSynth(snrs_db=None, seed=3, **SHAPES[shape])
    raw, y, z, drawn, sym, taps = ws.generate(n, 0, 0, **EVERYTHING)
    assert z.isnan().all() and drawn[:, 1].isnan().all()
    assert {ws.descriptors[k][0] for k in y.cpu().tolist()} == {0, 1, 2}
    ref = waveform_reference(sym, drawn, taps, ws)
    got = raw.cpu().numpy().astype(np.float64)
    peak = np.abs(ref).reshape(n, -1).max(axis=1)
    err = np.abs(got - ref).reshape(n, -1).max(axis=1)
    power = (got ** 2).sum(axis=2).mean(axis=1)
    print(f"shape {shape}: max |raw - fp64 reference| / frame peak = {(err / peak).max():.3e}, max |mean |s|^2 - 1| = "
          f"{np.abs(power - 1).max():.3e}")
    assert np.all(err <= 1e-4 * peak), (err / peak)
    assert np.all(np.abs(power - 1) <= 1e-5), power
    # the same without the channel and without timing: v = u
    plain = ShapedSynth(snrs_db=None, seed=3, timing=False, **dict(SHAPES[shape], taps=1))
    m = min(n, 38)
    raw, y, z, drawn, sym, taps = plain.generate(m, 0, 0, **EVERYTHING)
    ref = waveform_reference(sym, drawn, taps, plain)
    got = raw.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - ref).reshape(m, -1).max(axis=1) <= 1e-4 * np.abs(ref).reshape(m, -1).max(axis=1))
    assert np.all(np.abs((got ** 2).sum(axis=2).mean(axis=1) - 1) <= 1e-5)


def test_a_constellation_too_large_for_lds_is_read_from_memory():
    """More than 1024 points: the kernel reads the table in place.  The same frames against the reference."""
    from vit_vs_raw_iq_amd import ShapedSynth, waveform_reference
    ring = np.exp(2j * np.pi * np.arange(1500) / 1500) * (1 + 0.5 * (np.arange(1500) % 3))
    ws = ShapedSynth({"QPSK": None, "ring": ring}, None, seed=5, **SHAPES["b"])
    raw, y, z, drawn, sym, taps = ws.generate(8, 0, 0, **EVERYTHING)
    assert sym[1].max().item() > 1024
    ref = waveform_reference(sym, drawn, taps, ws)
    got = raw.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - ref).reshape(8, -1).max(axis=1) <= 1e-4 * np.abs(ref).reshape(8, -1).max(axis=1))


@pytest.mark.parametrize("length", [1024, 33])
def test_identity_configuration_is_iq_frames_synth_bit_for_bit(length):
    from vit_vs_raw_iq_amd import FrameSynth, ShapedSynth, data as D
    names = [c for c in D.CLASSES if c not in ("GMSK", "OQPSK")]
    for balanced in (True, False):
        fs = FrameSynth(names, length=length, seed=0x500000007, balanced=balanced)
        ws = ShapedSynth(names, length=length, seed=0x500000007, balanced=balanced, sps=1, span=1, n_phase=1, timing=False, taps=1,
                         pulse=np.ones((1, 1, 1)))
        assert ws.n_symbols == length + 2
        for base, stream in ((0, 0), (2 ** 32 + 40, 1)):
            a = fs.generate(76, base, stream, return_drawn=True, return_symbols=True)
            b = ws.generate(76, base, stream, return_drawn=True, return_symbols=True)
            assert torch.equal(a[0], b[0]) and same_bits(a[0], b[0])
            assert torch.equal(a[1], b[1]) and same_bits(a[2], b[2])
            assert same_bits(a[3], b[3][:, :4])
            assert torch.equal(a[4], b[4][:, :length])


def test_an_all_ones_pulse_of_one_symbol_gives_the_exact_structure():
    """span 1, sps 4, table of ones: a constellation frame is piecewise constant over each symbol, OQPSK's I changes only at
    n % 4 == 0 and its Q only at n % 4 == 2, and GMSK (a constant 2^28 per sample: a sixteenth of a turn) has unit envelope."""
    from vit_vs_raw_iq_amd import ShapedSynth
    length = 131
    ws = ShapedSynth(["QPSK", "OQPSK", "GMSK"], None, length, seed=6, sps=4, span=1, n_phase=1, taps=1, pulse=np.ones((1, 4, 1)),
                     fpulse=np.full((1, 4, 1), 2 ** 28))
    raw, y, z, drawn, sym, taps = ws.generate(12, 0, 0, **EVERYTHING)
    raw64, d, s = raw.cpu().numpy().astype(np.float64), drawn.cpu().numpy().astype(np.float64), sym.cpu().numpy()
    bits = raw.cpu().contiguous().view(torch.int32).numpy().astype(np.int64)
    bits = bits[:, :, 0] * 2 ** 32 + (bits[:, :, 1] & 0xFFFFFFFF)                      # one integer per complex sample
    n = np.arange(length)
    for i in range(12):
        z64 = (raw64[i, :, 0] + 1j * raw64[i, :, 1]) * np.exp(-1j * d[i, 2])           # the carrier phase taken off
        if i % 3 == 0:
            groups = bits[i, :128].reshape(32, 4)
            assert np.all(groups == groups[:, :1])
            assert len(set(groups[:, 0])) == 4 and np.array_equal(np.unique(s[i, :32]), np.arange(4))
        elif i % 3 == 1:
            same = bits[i, 1:] == bits[i, :-1]
            assert np.all(same[(n[1:] % 4 == 1) | (n[1:] % 4 == 3)])                    # nothing changes at n % 4 in {1, 3}
            di, dq = np.abs(np.diff(z64.real)), np.abs(np.diff(z64.imag))
            assert np.all(dq[n[1:] % 4 == 0] <= 1e-6) and np.all(di[n[1:] % 4 == 2] <= 1e-6)
            assert (di[n[1:] % 4 == 0] > 1).any() and (dq[n[1:] % 4 == 2] > 1).any()
            np.testing.assert_array_equal(z64.real > 0, (s[i][n // 4] >> 1) == 1)
            np.testing.assert_array_equal(z64.imag > 0, (s[i][(n + 2) // 4] & 1) == 1)
        else:
            assert np.all(np.abs((raw64[i] ** 2).sum(axis=1) - 1) <= 1e-4)
            step = np.angle(z64[1:] / z64[:-1])
            np.testing.assert_allclose(np.abs(step), np.pi / 8, atol=1e-5)
            np.testing.assert_array_equal(step > 0, s[i][n[1:] // 4] == 1)


@pytest.mark.parametrize("sps", [2, 4, 8])
def test_kernel_output_is_band_limited(sps):
    """The condition of tests/test_waveform_cpu.py on the kernel's own noiseless frames: QPSK, alpha 0.35, span 8, len 1024."""
    from vit_vs_raw_iq_amd import ShapedSynth
    ws = ShapedSynth(["QPSK"], None, 1024, seed=sps, sps=sps, span=8, alpha=0.35, n_phase=32)
    raw, _, _, drawn = ws.generate(8, 0, 0, return_drawn=True)
    frac = out_of_band_fraction(raw.cpu().numpy(), band_edge(0.35, sps, 1024))
    print(f"sps {sps}: out-of-band share max {frac.max():.3e}; timing phases {sorted(set(drawn[:, 4].cpu().tolist()))}")
    assert np.all(frac <= 1e-3), frac


def test_frames_are_keyed_and_do_not_depend_on_how_the_stream_is_cut():
    from vit_vs_raw_iq_amd import ShapedSynth
    ws = ShapedSynth(seed=7, **SHAPES["a"])
    a = ws.generate(76, 0, 0, **EVERYTHING)
    b = ws.generate(76, 0, 0, **EVERYTHING)
    for u, v in zip(a, b):
        assert torch.equal(u, v) if u.dtype != torch.float32 else same_bits(u, v)
    # frames 40..75 of one call = a 36-frame call at frame_base 40 = calls of 5 and 31 frames, noise and taps included
    for base, count in ((40, 36), (40, 5), (45, 31)):
        t = ws.generate(count, base, 0, **EVERYTHING)
        for u, v in zip(t, a):
            w = v[base:base + count]
            assert torch.equal(u, w) if u.dtype != torch.float32 else same_bits(u, w)
    odd = ShapedSynth(seed=7, **SHAPES["b"])                      # and on the 8-byte store path
    assert same_bits(odd.generate(36, 40, 0)[0], odd.generate(76, 0, 0)[0][40:])
    for other, base, stream in ((ShapedSynth(seed=8, **SHAPES["a"]), 0, 0), (ShapedSynth(seed=7 + 2 ** 32, **SHAPES["a"]), 0, 0),
                                (ws, 0, 1), (ws, 76 * 2 ** 32, 0)):          # the last: the same low word, the same classes
        o = other.generate(76, base, stream, **EVERYTHING)
        assert torch.equal(o[1], a[1])                            # balanced: the same labels ...
        assert not torch.equal(o[3][:, 2], a[3][:, 2])            # ... another carrier phase,
        assert not torch.equal(o[4], a[4])                        # other symbols,
        assert not torch.equal(o[5], a[5])                        # another channel
        assert (o[0] != a[0]).flatten(1).any(1).all()             # and no frame in common


def test_timing_phase_is_uniform():
    """6-sigma bounds on a fixed seed."""
    from vit_vs_raw_iq_amd import ShapedSynth
    n, n_phase = 4096, 32
    ws = ShapedSynth(["QPSK"], None, 32, seed=1, sps=4, span=4, n_phase=n_phase)
    q = ws.generate(n, 0, 0, return_drawn=True)[3][:, 4].cpu().numpy()
    counts = np.bincount(q.astype(np.int64), minlength=n_phase)
    bound = 6 * math.sqrt(n * (1 / n_phase) * (1 - 1 / n_phase))
    print("timing phase counts", counts.tolist(), f"(expected {n / n_phase:.0f} +- {bound:.1f})")
    assert len(counts) == n_phase and np.all(q == np.rint(q)) and np.all(np.abs(counts - n / n_phase) <= bound)


def test_noise_is_what_the_snr_says():
    """Noisy minus noiseless for the same frames at 0 dB: per component N(0, 0.5 * 10^(-snr/10)); 6-sigma bounds as
    tests/test_gpu_synth.py (mean, variance, I-Q and lag-1 correlation)."""
    from vit_vs_raw_iq_amd import ShapedSynth
    for snr in (0.0, 10.0):
        noisy = ShapedSynth(snrs_db=(snr,), seed=2, **SHAPES["a"])
        clean = ShapedSynth(snrs_db=None, seed=2, **SHAPES["a"])
        raw, y, z = noisy.generate(8, 0, 0)
        assert torch.equal(z.cpu(), torch.full((8,), snr)) and torch.equal(y, clean.generate(8, 0, 0)[1])
        sigma = math.sqrt(0.5 * 10 ** (-snr / 10))
        r = (raw.cpu().numpy().astype(np.float64) - clean.generate(8, 0, 0)[0].cpu().numpy().astype(np.float64)) / sigma
        n = r.size
        iq = (r[:, :, 0] * r[:, :, 1]).mean() / r.std() ** 2
        lag = (r[:, 1:, :] * r[:, :-1, :]).mean() / r.var()
        print(f"snr {snr}: mean {r.mean():+.4f}, variance {r.var():.4f}, I-Q correlation {iq:+.4f}, lag-1 {lag:+.4f}, max {np.abs(r).max():.3f}")
        assert n == 16384 and abs(r.mean()) <= 6 / math.sqrt(n) and abs(r.var() - 1) <= 6 * math.sqrt(2 / n)
        assert abs(iq) <= 6 / math.sqrt(n / 2) and abs(lag) <= 6 / math.sqrt(n / 2)
        assert np.abs(r).max() < 6.0                                                          # 24-bit uniforms: |g| <= 5.77


def test_refusals_return_their_code_and_leave_the_outputs_untouched():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import ShapedSynth
    L = N.lib()
    sentinel = 1234.5
    ws = ShapedSynth(seed=1, **SHAPES["b"])
    n, length, NS = 8, 33, ws.n_symbols
    raw = torch.full((n, length, 2), sentinel, device=dev())
    y = torch.full((n,), 77, dtype=torch.int64, device=dev())
    z = torch.full((n,), sentinel, device=dev())
    drawn = torch.full((n, 8), sentinel, device=dev())
    sym = torch.full((n, NS), 77, dtype=torch.int32, device=dev())
    taps = torch.full((n, 8, 2), sentinel, device=dev())
    table = torch.from_numpy(ws.points).to(dev())
    pulse, fpulse = torch.from_numpy(ws.pulse).to(dev()), torch.from_numpy(ws.fpulse).to(dev())
    ARG, UNSUPPORTED = 1, 2

    def call(length=length, edit=None, par="ok", **ptrs):
        p = dict(raw=raw.data_ptr(), labels=y.data_ptr(), snr=z.data_ptr(), drawn=drawn.data_ptr(), symbols=sym.data_ptr(),
                 taps=taps.data_ptr())
        p.update(ptrs)
        if par == "ok":
            par = ws.struct(points=table.data_ptr(), pulse=pulse.data_ptr(), fpulse=fpulse.data_ptr())
        if edit:
            edit(par)
        return L.iq_frames_waveform(p["raw"], p["labels"], p["snr"], p["drawn"], p["symbols"], p["taps"], n, length,
                                    ctypes.byref(par) if par is not None else None, N.stream_handle())

    def put(**kw):
        def edit(p):
            for k, v in kw.items():
                setattr(p, k, v)
        return edit
    assert call(raw=None) == ARG and call(labels=None) == ARG and call(snr=None) == ARG and call(par=None) == ARG
    assert call(edit=put(classes=None)) == ARG
    assert call(length=0) == ARG
    for field in ("n_classes", "sps", "span", "n_phase", "n_taps"):
        assert call(edit=put(**{field: 0})) == ARG, field
    assert call(edit=put(timing=2)) == ARG and call(edit=put(balanced=2)) == ARG and call(edit=put(balanced=-1)) == ARG
    assert call(edit=put(points=None)) == ARG and call(edit=put(pulse=None)) == ARG and call(edit=put(fpulse=None)) == ARG
    for kind, off, count in ((3, 0, 4), (-1, 0, 4), (0, 0, 0), (0, -1, 4)):
        cls = (N.SynthClass * 1)(N.SynthClass(kind, off, count))
        assert call(edit=put(classes=cls, n_classes=1)) == ARG, (kind, off, count)
    for bad in (float("nan"), float("inf")):
        assert call(edit=put(snrs_db=(ctypes.c_float * 1)(bad), n_snrs=1)) == ARG, bad
        assert call(edit=put(los=bad)) == ARG, bad
        assert call(edit=put(tap_sigma=(ctypes.c_float * 8)(0.1, bad))) == ARG, bad
    assert call(edit=put(tap_sigma=(ctypes.c_float * 8)(0.1, -0.1))) == ARG
    assert call(raw=raw.data_ptr() + 4) == ARG and call(drawn=drawn.data_ptr() + 8) == ARG and call(taps=taps.data_ptr() + 4) == ARG
    assert call(symbols=sym.data_ptr() + 2) == ARG and call(edit=put(pulse=pulse.data_ptr() + 2)) == ARG
    assert call(labels=y.data_ptr() + 4) == ARG and call(snr=z.data_ptr() + 2) == ARG
    assert call(edit=put(points=table.data_ptr() + 4)) == ARG and call(edit=put(fpulse=fpulse.data_ptr() + 2)) == ARG
    assert call(length=-3) == ARG and call(edit=put(n_snrs=-1)) == ARG and call(edit=put(timing=-1)) == ARG
    assert call(edit=put(snrs_db=None)) == ARG                                             # four SNR values and no array
    assert call(edit=put(sps=17)) == UNSUPPORTED and call(edit=put(span=33)) == UNSUPPORTED
    assert call(edit=put(n_phase=65)) == UNSUPPORTED and call(edit=put(n_taps=9)) == UNSUPPORTED
    assert call(length=8193) == UNSUPPORTED                                                # 65544 bytes of LDS for one frame
    many = (N.SynthClass * 129)(*[N.SynthClass(2, 0, 0)] * 129)
    assert call(edit=put(classes=many, n_classes=129)) == UNSUPPORTED
    assert call(edit=put(snrs_db=(ctypes.c_float * 65)(), n_snrs=65)) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (raw, z, drawn, taps):
        assert torch.equal(t, torch.full_like(t, sentinel))
    assert torch.equal(y, torch.full_like(y, 77)) and torch.equal(sym, torch.full_like(sym, 77))


def test_outputs_carved_out_of_a_patterned_buffer_leave_every_byte_around_them_unchanged():
    """Shape (b): 33 samples, 8-byte stores, 21 symbol words of which the last Philox call holds one."""
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import ShapedSynth
    ws = ShapedSynth(seed=1, **SHAPES["b"])
    n, length, NS = 7, 33, ws.n_symbols
    sizes = {"raw": n * length * 8, "labels": n * 8, "snr": n * 4, "drawn": n * 32, "symbols": n * NS * 4, "taps": n * 64}
    pad = 256
    offs, total = {}, pad
    for k, v in sizes.items():
        offs[k] = total
        total += (v + 15) // 16 * 16 + pad
    pattern = torch.arange(total, dtype=torch.int64).mul_(37).add_(11).remainder_(251).to(torch.uint8).to(dev())
    buf = pattern.clone()
    table = torch.from_numpy(ws.points).to(dev())
    pulse, fpulse = torch.from_numpy(ws.pulse).to(dev()), torch.from_numpy(ws.fpulse).to(dev())
    par = ws.struct(5, 2, points=table.data_ptr(), pulse=pulse.data_ptr(), fpulse=fpulse.data_ptr())
    p = {k: buf.data_ptr() + o for k, o in offs.items()}
    assert buf.data_ptr() % 16 == 0 and (p["raw"] % 16) == 0
    N.check(N.lib().iq_frames_waveform(p["raw"], p["labels"], p["snr"], p["drawn"], p["symbols"], p["taps"], n, length,
                                       ctypes.byref(par), N.stream_handle()), "iq_frames_waveform")
    torch.cuda.synchronize()
    inside = torch.zeros(total, dtype=torch.bool, device=dev())
    for k, v in sizes.items():
        inside[offs[k]:offs[k] + v] = True
    assert torch.equal(buf[~inside], pattern[~inside])
    want = ws.generate(n, 5, 2, **EVERYTHING)
    for k, t in zip(("raw", "labels", "snr", "drawn", "symbols", "taps"), want):
        assert torch.equal(buf[offs[k]:offs[k] + sizes[k]], t.contiguous().view(torch.uint8).flatten()), k


def preprocess(raw, take, stats):
    import vit_vs_raw_iq_amd._native as N
    B, length = raw.shape[0], raw.shape[1]
    out = torch.empty(B, 2, take, device=raw.device)
    st = (ctypes.c_float * 4)(stats["i_mean"], stats["i_std"], stats["q_mean"], stats["q_std"])
    N.check(N.lib().iq_frames_preprocess(raw.data_ptr(), out.data_ptr(), B, length, take, st, N.stream_handle()),
            "iq_frames_preprocess")
    return out


def test_stream_is_generate_then_the_input_pipeline():
    from vit_vs_raw_iq_amd import Impairments, ShapedSynth, Spectrogram, SynthStream, impair
    ws = ShapedSynth(seed=5, **SHAPES["a"])
    stats = ws.stats(n_subset=76)
    raw76 = ws.generate(76, 0, 0)[0].cpu().numpy().astype(np.float64)
    assert abs(stats["i_mean"] - raw76[:, :, 0].mean()) < 1e-4 and abs(stats["q_std"] - raw76[:, :, 1].std(ddof=1)) < 1e-4
    B, s = 12, 3
    raw, y, z = ws.generate(B, s * B, 0)
    aug = Impairments.augmentation().replace(snr_db=(5.0, 15.0))
    for layout, h, w, take in (("rawiq", 32, 64, 1024), ("vit", 32, 64, 1024), ("vit", 32, 32, 512)):
        x, ys, zs = SynthStream(ws, stats, layout, B, h=h, w=w).get(s)
        assert x.shape == ((B, 2, 1024) if layout == "rawiq" else (B, 1, h, w))
        assert same_bits(x.reshape(B, 2, take), preprocess(raw, take, stats)) and torch.equal(ys, y) and same_bits(zs, z)
        xa, ya, _ = SynthStream(ws, stats, layout, B, h=h, w=w, augment=aug).get(s)
        assert same_bits(xa, impair(raw, stats, layout, aug, seed=ws.seed, step=0, frame_base=s * B, h=h, w=w)) and torch.equal(ya, y)
        assert not torch.equal(xa, x)
    spec = Spectrogram(64, 64, length=1024)
    xs, ysp, _ = SynthStream(ws, stats, "vit", B, spectrogram=spec).get(s)
    assert xs.shape == (B, 1, 64, 64) and same_bits(xs, spec(preprocess(raw, 1024, stats))) and torch.equal(ysp, y)
    xsa, _, _ = SynthStream(ws, stats, "vit", B, spectrogram=spec, augment=aug).get(s)
    assert same_bits(xsa, impair(raw, stats, "vit", aug, seed=ws.seed, step=0, frame_base=s * B, spectrogram=spec))
    got = [t[1] for t in SynthStream(ws, stats, "rawiq", B, stream=1).batches(2, first_step=1)]
    assert len(got) == 2 and torch.equal(got[0], ws.generate(B, B, 1)[1]) and torch.equal(got[1], ws.generate(B, 2 * B, 1)[1])


def test_graph_replay_of_generate_equals_eager():
    from vit_vs_raw_iq_amd import ShapedSynth
    ws = ShapedSynth(seed=9, **SHAPES["a"])
    eager = ws.generate(76, 19, 0, **EVERYTHING)           # also: the tables are on the device before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        held = ws.generate(76, 19, 0, **EVERYTHING)
    for t in held:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for u, v in zip(held, eager):
        assert torch.equal(u, v) if u.dtype != torch.float32 else same_bits(u, v)


FOUR = ["BPSK", "QPSK", "GMSK", "OQPSK"]
TRAIN_STEPS = 100        # the first candidate (the step count of tests/test_gpu_synth.py) clears the bound on an MI355X: held-out
                         # accuracy 1.0000 (profiles/waveform.txt); the bound below is derived and stays whatever the budget becomes


@functools.lru_cache(maxsize=None)
def four_class_source():
    """(ShapedSynth of BPSK / QPSK / GMSK / OQPSK at 20 dB, 4 samples per symbol, its statistics): made once, never modified."""
    from vit_vs_raw_iq_amd import ShapedSynth
    ws = ShapedSynth(FOUR, snrs_db=(20.0,), length=1024, seed=11, sps=4)
    return ws, ws.stats(n_subset=1024)


def test_a_model_trained_on_the_shaped_stream_beats_chance_on_frames_of_another_stream(tmp_path):
    """Every step trains on 256 frames that were never used; the accuracy on 2048 frames of stream 1 must exceed chance by 6
    standard deviations of a 2048-frame estimate at chance: 1/4 + 6 sqrt((1/4)(3/4)/2048) = 0.3074."""
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import SynthStream, train_on_stream
    from vit_vs_raw_iq_amd.evaluation import evaluate_model_with_confusion
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    ws, stats = four_class_source()
    torch.manual_seed(0)
    m = P.AMCTransformerRawIQ(in_channels=2, seq_length=1024, num_classes=4, d_model=128, n_head=8, n_layers=2, ffn_hidden=256,
                              drop_prob=0.0, device="cuda", use_cls_token=True, embedding_type="segment", segment_size=16)
    m = m.to(dev()).train()
    tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-3)
    assert train_on_stream(tr, SynthStream(ws, stats, "rawiq", 256), TRAIN_STEPS) == TRAIN_STEPS
    loss, acc_train, frames = tr.read_stats()
    assert frames == TRAIN_STEPS * 256
    held = SynthStream(ws, stats, "rawiq", 256, stream=1)
    res = evaluate_model_with_confusion(m, held.batches(8), dev(), FOUR, tmp_path, prefix="waveform")
    bound = 0.25 + 6 * math.sqrt(0.25 * 0.75 / 2048)
    print(f"{TRAIN_STEPS} steps of 256 fresh frames: running train loss {loss:.4f}, accuracy {acc_train:.4f}; "
          f"held-out accuracy on 2048 frames of stream 1 {res['overall_accuracy']:.4f} (bound {bound:.4f})")
    _, y, z = ws.generate(2048, 0, 1)
    assert np.array_equal(res["labels"], y.cpu().numpy()) and np.array_equal(res["labels"], np.arange(2048) % 4)
    assert np.all(res["snrs"] == np.float32(20.0)) and res["confusion_matrix"].sum() == 2048
    assert res["overall_accuracy"] > bound
