"""GPU (MI355X): the cyclic-spectrum front end (csrc/cyclic.hip, iq_frames_cyclic, vit_vs_raw_iq_amd.cyclic).

1. Exact: integer tables, rot and frames (tests/cyclic_ref.int_case) make every fp32 partial sum of both MFMA stages an integer
   below 2^24, so the image equals an int64 host evaluation bit for bit, for all three kinds.  The operands lie between NaN
   guards, the image between sentinels, the launched kernel is asserted by name.  EXACT says which case reaches which branch.
2. Real tables against the host fp64 definition, in all three modes.  The tolerance is measured on the reference, never on the
   kernel: E32 = the largest error of the same definition evaluated in numpy float32 arithmetic (cyclic_ref.real_forward); the
   kernel is allowed FACTOR * E32 with the spectrogram test's FACTOR = 4 and for its reasons: the kernel's sums are ordered
   fmaf chains (here 64 .. 448 terms for X, then up to 122 for S) where numpy's float32 products sum pairwise or in blocks, and
   the device has its own log10f and division.  The second stage does not change the rule: both evaluations feed the same
   rounded Y into it, and E32 already contains the error the first stage hands to the second.  The measured ratio is printed.
   No element is excluded.  The all-zero frame gives exactly the epilogue of P = 0.
3. Structure on the device: the tone and the symbol-rate line of tests/test_cyclic_ref_cpu.py through CyclicSpectrum (rows and
   columns in fftshift order), kind 'both' = 'scf' and 'conj' stacked.
4. Independence: a frame's image does not depend on the other frames of the call, its position, or a NaN neighbour; two runs agree.
5. Plumbing: the `spectrogram=` keyword of SynthStream, DeviceInputPipeline, impair and impairment_curve, hipGraph replay, a
   two-channel ViT trained on cyclic images of never-repeated frames, for_model, requires_grad.
6. Refusals: every ARG / UNSUPPORTED case of the header on the device, with no kernel launched.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cyclic_ref as R
from frontend_gpu import GUARD, SENTINEL, abi_call, bits, dev, on_device, same_bits, small_vit
from prof_names import kernel_launches

pytestmark = pytest.mark.gpu

KINDS = ("scf", "conj", "both")


def struct(n_fft, columns, hop, pad, kind=2, mode=0, inv_norm=1.0, floor=1.0, scale=1.0, shift=0.0):
    import vit_vs_raw_iq_amd._native as N
    return N.Cyclic(n_fft=n_fft, hop=hop, pad=pad, columns=columns, kind=kind, mode=mode, inv_norm=inv_norm, floor=floor,
                    scale=scale, shift=shift)


def keeps_y(n_fft, columns, length):
    """The header's rule for the launch shape: every 32-column chunk of Y stays in LDS (one workgroup per frame) when frame + rot
    + D + the chunks + the band's values fit in 144 KB; otherwise one workgroup per (frame, band) holds one chunk at a time."""
    chunks = (columns + 31) // 32
    floats = ((2 * length + 3) & ~3) + 3 * n_fft + chunks * 64 * (n_fft + 1) + 64 * n_fft
    return 4 * floats <= 144 * 1024


def kernel_name(par, length):
    flag = lambda b: "true" if b else "false"   # noqa: E731
    return f"cyclic_kernel<{flag(par.kind != 1)}, {flag(par.kind != 0)}, {flag(keeps_y(par.n_fft, par.columns, length))}>"


def abi_forward(x, table, rot, par, expect_kernel=True):
    """x (n, 2, len), table (2, n_fft, n_fft), rot (2, n_fft) numpy -> image (n, C, n_fft, n_fft) numpy through the C ABI.  x and
    both tables lie between NaN guards (a read outside any of them poisons the image), the image between sentinels and is
    pre-filled with the sentinel (an element the kernel does not write shows)."""
    n, _, length = x.shape
    return abi_call("iq_frames_cyclic", kernel_name(par, length), (x, table, rot), (n, 2 if par.kind == 2 else 1, par.n_fft, par.n_fft),
                    n, length, par, expect_kernel)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. exact
# ---------------------------------------------------------------------------------------------------------------------------
# (n_fft, columns, hop, pad, len, n_frames, Y kept in LDS).  The kernel works in 32 x 32 tiles: bands of 32 channels, wave w owns
# the bin tiles (stage 1) and l tiles (stage 2) w and w + 4 of n_fft / 32 (1, 2, 3, 5, 7, 8 occur: one wave, two, three, a second
# slot for one wave, for three, for all four); time runs in chunks of 32 columns, two columns per MFMA.  Two launch shapes: Y kept
# whole in LDS and the bands looped over in one workgroup per frame (with 1, 2, 3, 5 bands and 1 or 3 chunks), or one workgroup
# per (frame, band) with one chunk at a time (7 and 8 bands, 1 and 2 chunks).
EXACT = {
    # one tile, one column: half of the only MFMA step is the zero row; windows end inside the frame
    "one_tile_one_column": (32, 1, 1, 0, 100, 1, True),
    # two columns = one full step; hop divides n_fft (r takes few values); odd length: scalar staging, frames 1 and 2 of the
    # call start 8 bytes off / on a 16-byte boundary
    "two_columns_odd_len": (64, 2, 16, 0, 101, 3, True),
    # three columns: an odd count ends on a zero row; hop 5 does not divide n_fft; pad 7: window 0 over the front (negative j0);
    # n_fft / 2 = 48: the fftshift wrap falls inside a tile
    "three_columns_wrap": (96, 3, 5, 7, 300, 1, True),
    # 31 columns: one short of a chunk; five tiles (wave 0 takes a second); hop 29; windows run past the end of a 900-sample frame
    "chunk_minus_one": (160, 31, 29, 40, 900, 1, True),
    # exactly one chunk
    "one_chunk": (32, 32, 16, 0, 1024, 1, True),
    # 33 columns: a second chunk of one column; seven tiles; wrap inside a tile (112); front and end both crossed; three frames
    "chunk_plus_one": (224, 33, 29, 100, 1024, 3, False),
    # 40 columns, eight tiles: every wave has two slots in both stages; pad n_fft - 1: window 0 holds one sample
    "eight_tiles_two_chunks": (256, 40, 4, 255, 1024, 1, False),
    # 70 columns: three chunks, the last of six columns; odd length, three frames; windows far behind the end
    "three_chunks": (64, 70, 5, 9, 333, 3, True),
    # the longest frame that still keeps Y at n_fft 256 with one chunk (exactly 144 KB of LDS), and one sample more
    "cache_limit": (256, 3, 97, 0, 1632, 1, True),
    "past_cache_limit": (256, 3, 97, 0, 1633, 1, False),
}


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("name", list(EXACT))
def test_image_equals_the_int64_evaluation_bit_for_bit(name, kind):
    """Mode 'power', inv_norm = scale = 1, shift = 0.  int_forward asserts that every sum of absolute terms is below 2^24."""
    n_fft, columns, hop, pad, length, n, kept = EXACT[name]
    assert keeps_y(n_fft, columns, length) == kept                       # abi_forward asserts the kernel of that shape by name
    table, rot, x = R.int_case(n_fft, columns, hop, pad, length, n, seed=n_fft + columns)
    want = R.int_forward(x, table, rot, (n_fft, columns, hop, pad), kind)
    got = abi_forward(x, table, rot, struct(n_fft, columns, hop, pad, kind=kind))
    assert not np.isnan(got).any() and not np.any(got == SENTINEL)
    assert want.max() > 0 and np.array_equal(bits(got), bits(want))


def test_an_offset_frame_pointer_takes_the_scalar_staging_path():
    """x 8 bytes off a 16-byte boundary with an even length: the float4 staging of the frame is not used."""
    import vit_vs_raw_iq_amd._native as N
    n_fft, columns, hop, pad, length, n = 64, 20, 5, 9, 100, 2
    table, rot, x = R.int_case(n_fft, columns, hop, pad, length, n, seed=77)
    par = struct(n_fft, columns, hop, pad)
    buf = torch.full((2 + x.size + GUARD,), float("nan"), dtype=torch.float32, device=dev())
    buf[2:2 + x.size] = torch.from_numpy(x.astype(np.float32).reshape(-1)).to(dev())
    tab = torch.from_numpy(table.astype(np.float32)).to(dev())
    rt = torch.from_numpy(rot.astype(np.float32)).to(dev())
    out = torch.empty(n, 2, n_fft, n_fft, device=dev())
    assert buf.data_ptr() % 16 == 0
    N.check(N.lib().iq_frames_cyclic(buf.data_ptr() + 8, tab.data_ptr(), rt.data_ptr(), out.data_ptr(), n, length,
                                     ctypes.byref(par), N.stream_handle()), "iq_frames_cyclic")
    assert np.array_equal(bits(out.cpu().numpy()), bits(R.int_forward(x, table, rot, (n_fft, columns, hop, pad), 2)))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. real tables against fp64
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zscored_frames():
    """Frames of a FrameSynth stream (one sample per symbol) and of a ShapedSynth stream (RRC, 8 samples per symbol), each BPSK /
    QPSK / 16QAM / GMSK at 0 dB and at 20 dB, z-scored as the input pipeline hands them on, and one all-zero frame behind them
    -> host float32 (9, 2, 1024).  Made once, never modified."""
    from vit_vs_raw_iq_amd import FrameSynth, Impairments, ShapedSynth, impair
    names = ["BPSK", "QPSK", "16QAM", "GMSK"]
    parts = []
    for src, idx in ((FrameSynth(names, snrs_db=(0.0, 20.0), length=1024, seed=11, device=dev()), (0, 5, 2, 7)),
                     (ShapedSynth(names, snrs_db=(0.0, 20.0), length=1024, seed=12, device=dev()), (1, 4, 3, 6))):
        raw = torch.cat([src.generate(1, j, 0)[0] for j in idx])
        snr = torch.cat([src.generate(1, j, 0)[2] for j in idx]).cpu().tolist()
        assert set(snr) == {0.0, 20.0}                                   # two SNRs from each source
        parts.append(impair(raw, src.stats(64), "rawiq", Impairments()))
    x = torch.cat(parts + [torch.zeros(1, 2, 1024, device=dev())]).cpu().numpy()
    x.setflags(write=False)
    return x


FACTOR = 4                      # allowed multiple of E32 (see the module docstring)
REAL_GEOMS = {"64_hop16": (64, 16), "224_hop56": (224, 56)}


@pytest.mark.parametrize("mode", ["power", "log", "coherence"])
@pytest.mark.parametrize("name", list(REAL_GEOMS))
def test_image_against_the_fp64_definition(name, mode):
    from vit_vs_raw_iq_amd import CyclicSpectrum, cyclic_reference
    n_fft, hop = REAL_GEOMS[name]
    floor = 1e-3 if mode == "log" else 1e-6
    cs = CyclicSpectrum(n_fft, 1024, hop, window="hann", kind="both", mode=mode, floor=floor, scale=1.5, shift=-0.25)
    assert cs.columns == (61 if n_fft == 64 else 15)
    xh = zscored_frames()
    img = cs(on_device(xh)).cpu().numpy()
    ref = cyclic_reference(xh, cs)
    e32 = np.abs(R.real_forward(xh, cs, np.float32).astype(np.float64) - ref).max()
    err = np.abs(img.astype(np.float64) - ref).max()
    print(f"{name} {mode}: E32 {e32:.3e}, kernel {err:.3e} ({err / e32:.2f} E32), image range [{ref.min():.3f}, {ref.max():.3f}]")
    assert e32 > 0
    assert err <= FACTOR * e32
    # the zero frame: P = 0 and D = 0 exactly
    f32 = np.float32
    zero = img[-1]
    assert np.all(bits(zero) == bits(zero).flat[0])
    if mode == "log":
        want = f32(np.log10(f32(floor))) * f32(1.5) + f32(-0.25)
        assert abs(float(zero.flat[0]) - float(want)) <= 4 * np.spacing(abs(want))     # the device has its own log10f
    else:
        assert bits(zero).flat[0] == bits(np.array(-0.25)).flat[0]                       # 0 * scale + shift; 0 / floor = 0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. structure on the device
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [32, 96])
def test_a_tone_lights_one_element_per_channel_in_fftshift_order(n_fft):
    """As tests/test_cyclic_ref_cpu.py: the lit element is Np^2 at (row of a = 0 resp. 2 k0, column of k0).  fp32: the peak to
    1e-5 relative (sums of Np and of T equal terms).  Off the tone |X| is the rounding of Np cancelling terms of size 1 (samples
    and table rounded to fp32, an fmaf chain of 2 Np terms): below 2 Np 2^-24 Np < 1e-5 of the peak's |X| = Np.  A Gram element
    with one factor off the tone is then below 1e-5 of the peak's, and P, its square, below 1e-10: the bound is 1e-9."""
    from vit_vs_raw_iq_amd import CyclicSpectrum
    length, hop = 400, 29
    k0s = [0, 1, n_fft // 2 - 1, n_fft // 2, n_fft - 1]
    j = np.arange(length)
    z = np.exp(2j * np.pi * np.array(k0s)[:, None] * j[None, :] / n_fft)
    cs = CyclicSpectrum(n_fft, length, hop, window="rect", mode="power")
    img = cs(on_device(np.stack([z.real, z.imag], axis=1))).cpu().numpy().astype(np.float64)
    h = n_fft // 2
    for f, k0 in enumerate(k0s):
        col = (k0 + h) % n_fft
        for ch, a in ((0, 0), (1, (2 * k0) % n_fft)):
            row = (a + h) % n_fft
            assert np.unravel_index(img[f, ch].argmax(), (n_fft, n_fft)) == (row, col), (k0, ch)
            assert abs(img[f, ch, row, col] - n_fft ** 2) < 1e-5 * n_fft ** 2
            rest = img[f, ch].copy()
            rest[row, col] = 0.0
            assert rest.max() < 1e-9 * n_fft ** 2, (k0, ch)


def test_the_symbol_rate_line_and_the_conjugate_line_of_bpsk_on_the_device():
    from vit_vs_raw_iq_amd import CyclicSpectrum
    cs = CyclicSpectrum(64, 1024)
    for seed in (1, 2, 3):
        R.check_symbol_rate_line(cs(on_device(R.rect_pulse_frames(seed))).cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("mode", ["power", "coherence"])
def test_both_is_scf_and_conj_stacked_bit_for_bit(mode):
    from vit_vs_raw_iq_amd import CyclicSpectrum
    x = on_device(zscored_frames()[[1, 6, 8]])
    for n_fft, hop, pad in ((96, 7, 30), (160, 40, 0)):
        img = {k: CyclicSpectrum(n_fft, 1024, hop, pad, kind=k, mode=mode)(x) for k in KINDS}
        assert img["both"].shape == (3, 2, n_fft, n_fft) and img["scf"].shape == img["conj"].shape == (3, 1, n_fft, n_fft)
        assert same_bits(img["both"], torch.cat([img["scf"], img["conj"]], dim=1))
        assert not torch.equal(img["scf"], img["conj"])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. independence and isolation
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["log", "coherence"])
def test_a_frame_does_not_depend_on_the_call_it_is_part_of(mode):
    from vit_vs_raw_iq_amd import CyclicSpectrum
    n_fft, hop, pad, length = 64, 7, 20, 301                            # odd length: the frames of a call alternate in alignment
    x = np.random.default_rng(12).standard_normal((3, 2, length)).astype(np.float32)
    cs = CyclicSpectrum(n_fft, length, hop, pad, mode=mode)
    assert cs.columns > 32
    par = cs.struct()
    img = abi_forward(x, cs.table, cs.rot, par)
    assert np.array_equal(bits(abi_forward(x, cs.table, cs.rot, par, expect_kernel=False)), bits(img))      # two runs
    order = [2, 0, 1]
    assert np.array_equal(bits(abi_forward(x[order], cs.table, cs.rot, par, expect_kernel=False)), bits(img[order]))
    for b in range(3):
        one = abi_forward(x[b:b + 1], cs.table, cs.rot, par, expect_kernel=False)
        assert np.array_equal(bits(one[0]), bits(img[b])), b
    # NaN neighbours on both sides change nothing
    poisoned = x.copy()
    poisoned[0], poisoned[2] = np.nan, np.nan
    got = abi_forward(poisoned, cs.table, cs.rot, par, expect_kernel=False)
    assert np.array_equal(bits(got[1]), bits(img[1])) and np.isnan(got[0]).all() and np.isnan(got[2]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. plumbing
# ---------------------------------------------------------------------------------------------------------------------------
STATS = {"i_mean": 0.01, "i_std": 0.9, "q_mean": -0.02, "q_std": 1.1}


def test_the_spectrogram_keyword_is_the_rawiq_call_followed_by_the_cyclic_spectrum():
    from vit_vs_raw_iq_amd import CyclicSpectrum, FrameSynth, Impairments, SynthStream, data as D, impair
    fs = FrameSynth(["BPSK", "QPSK", "16QAM", "GMSK"], snrs_db=(0.0, 20.0), length=1024, seed=5, device=dev())
    cs = CyclicSpectrum(64, 1024)
    aug = Impairments(phase=(-1.0, 1.0), cfo=(-0.01, 0.01), shift_max=100, snr_db=(5.0, 15.0))
    raw = fs.generate(8, 24, 0)[0]
    for imp in (None, aug):
        x, y, z = SynthStream(fs, STATS, "vit", 8, augment=imp, spectrogram=cs).get(3)
        x0, y0, z0 = SynthStream(fs, STATS, "rawiq", 8, augment=imp).get(3)
        assert x.shape == (8, 2, 64, 64) and same_bits(x, cs(x0)) and torch.equal(y, y0) and same_bits(z, z0)
        host = raw.cpu().numpy()
        got = D.DeviceInputPipeline(STATS, "vit", batch=8, augment=imp, seed=9, spectrogram=cs)(host)
        plain = D.DeviceInputPipeline(STATS, "rawiq", batch=8, augment=imp, seed=9)(host)
        assert got.shape == (8, 2, 64, 64) and same_bits(got, cs(plain))
    got, drawn = impair(raw, STATS, "vit", aug, seed=4, step=2, frame_base=7, return_drawn=True, spectrogram=cs)
    plain, drawn0 = impair(raw, STATS, "rawiq", aug, seed=4, step=2, frame_base=7, return_drawn=True)
    assert got.shape == (8, 2, 64, 64) and same_bits(got, cs(plain)) and same_bits(drawn, drawn0)
    assert torch.isfinite(got).all() and float(got.max()) > 0.5


def test_graph_replay_equals_eager():
    from vit_vs_raw_iq_amd import CyclicSpectrum
    cs = CyclicSpectrum(96, 1024, 24)
    xs = on_device(zscored_frames()[:8])
    a, b = xs[:4].clone(), xs[4:].clone()
    eager_a, eager_b = cs(a), cs(b)                                     # also: both tables are on the device before the capture
    torch.cuda.synchronize()
    held_in = a.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        held = cs(held_in)
    held.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(held, eager_a)
    held_in.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(held, eager_b) and not same_bits(eager_a, eager_b)


def test_a_two_channel_vit_trains_on_cyclic_images_of_fresh_frames_and_the_curve_runs():
    """BPSK / QPSK / GMSK / OQPSK at 4 samples per symbol and 20 dB: the classes differ in exactly what the two channels show.
    Twelve steps of 32 never-repeated frames; the mean loss of the last four steps is below that of the first four."""
    from vit_vs_raw_iq_amd import CyclicSpectrum, Impairments, ShapedSynth, Spectrogram, SynthStream, impair, impairment_curve, train_on_stream
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    ws = ShapedSynth(["BPSK", "QPSK", "GMSK", "OQPSK"], snrs_db=(20.0,), length=1024, seed=11, sps=4, device=dev())
    stats = ws.stats(64)
    m = small_vit(2, 64, 64).train()
    cs = CyclicSpectrum.for_model(m, 1024)
    assert (cs.n_fft, cs.kind, cs.channels, cs.mode) == (64, "both", 2, "coherence")
    raw, y, _ = ws.generate(64, 0, 1)
    x = impair(raw, stats, "rawiq", Impairments())
    cs.fit(x)
    img = cs(x)
    assert img.shape == (64, 2, 64, 64) and abs(float(img.mean())) < 1e-3 and abs(float(img.std()) - 1.0) < 1e-3
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-3)
    stream = SynthStream(ws, stats, "vit", 32, spectrogram=cs)
    assert train_on_stream(tr, stream, 4) == 4
    first, _, frames = tr.read_stats()
    assert train_on_stream(tr, stream, 4, first_step=4) == 8
    tr.read_stats()
    assert train_on_stream(tr, stream, 4, first_step=8) == 12
    last, _, _ = tr.read_stats()
    print(f"mean loss of steps 0-3 {first:.4f}, of steps 8-11 {last:.4f}")
    assert frames == 128 and np.isfinite(first) and np.isfinite(last) and 0 < last < first
    after = m.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    assert sum(int(not torch.equal(before[k], after[k])) for k in before) >= len(before) // 2
    values = [0.0, 0.01, 0.05]
    curve = impairment_curve(m, raw, y, stats, "cfo", values, spectrogram=cs, batch=32)
    assert len(curve) == 3 and all(0.0 <= a <= 1.0 for a in curve)
    assert curve == impairment_curve(m, raw, y, stats, "cfo", values, spectrogram=cs, batch=64)
    with pytest.raises(ValueError):
        impairment_curve(m, raw, y, stats, "cfo", values, spectrogram=CyclicSpectrum(32, 1024))
    with pytest.raises(RuntimeError):                                     # a one-channel image into the two-channel model
        impairment_curve(m, raw, y, stats, "cfo", values, spectrogram=Spectrogram(64, 64, 1024))


def test_for_model_and_requires_grad():
    from vit_vs_raw_iq_amd import CyclicSpectrum
    assert CyclicSpectrum.for_model(small_vit(1, 32, 32), 256).kind == "scf"
    with pytest.raises(ValueError):
        CyclicSpectrum.for_model(small_vit(1, 32, 64), 1024)             # not square
    with pytest.raises(ValueError):
        CyclicSpectrum.for_model(small_vit(3, 32, 32), 1024)             # three channels
    cs = CyclicSpectrum(32, 128)
    x = torch.zeros(2, 2, 128, device=dev())
    with pytest.raises(RuntimeError, match="not differentiable"):
        cs(x.clone().requires_grad_(True))
    assert cs(x).requires_grad is False


# ---------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_header_returns_before_any_launch():
    """The cases of tests/test_cyclic_ref_cpu.py with DEVICE pointers and a live stream: the status is the header's, no kernel is
    recorded and the output keeps its sentinel."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    buf = torch.full((8192 * 2 * 2 + 64,), SENTINEL, dtype=torch.float32, device=dev())
    a = buf.data_ptr()
    assert a % 16 == 0
    cases = R.refusal_calls(L, a)
    refused = [c for c in cases if c[2] != 0]
    assert len(refused) > 40
    statuses = []
    launched = kernel_launches(L, lambda: statuses.extend(run() for _, run, _ in cases))
    torch.cuda.synchronize()
    for (what, _, expect), got in zip(cases, statuses):
        assert got == expect, what
    assert launched == {}
    assert bool((buf == SENTINEL).all())
