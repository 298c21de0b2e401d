"""GPU (MI355X): labelled synthetic frames made on the device (csrc/synth.hip, iq_frames_synth, vit_vs_raw_iq_amd.synth).

1. The integer part -- class, SNR, symbols -- against a host restatement built here from tests/dropout_ref.philox4x32 and the
   layout written in include/iqvit.h: equal as integers (bitwise for the SNR).
2. The deterministic part (table lookup, carrier phase, unit power) against the host fp64 definition synth_reference.
3. Keying: same arguments = same bits; a frame does not depend on how the stream is cut into calls, noise included; seed (both
   words), stream and the high word of the frame index all change the frames.
4. Distributions and 5. noise statistics: 6-sigma bounds on fixed seeds -- a failure is a defect, not chance.
6. Refusals leave the output untouched.  7. SynthStream against generate + iq_frames_preprocess / impairments.impair.
8. A small raw-IQ classifier trained with train_on_stream on fresh frames beats chance on another stream by 6 sigma;
   evaluate_model_with_confusion takes stream.batches(...).  9. hipGraph replay against eager launches.

Lengths: 1024 (the task), 33 (odd and no multiple of 4: the Philox tail, the OQPSK odd end, a partial scan chunk, 8-byte
stores), 8192 (the LDS limit).  76 frames = 19 classes x 4 SNRs, no multiple of any block size.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from dropout_ref import philox4x32
from frontend_gpu import dev, same_bits

pytestmark = pytest.mark.gpu

SITE_SYNTH = 0xFFFFFFFE
M32 = 0xFFFFFFFF
FOUR = ["OOK", "BPSK", "QPSK", "16QAM"]


# ---------------------------------------------------------------------------------------------------------------------------
# host restatement of the integer part (include/iqvit.h, iq_frames_synth)
# ---------------------------------------------------------------------------------------------------------------------------
def words(seed, stream, j, c):
    """Philox words of frame j for the counter values c (array) -> (len(c), 4) Python-int-safe uint64 array."""
    c = np.asarray(c, dtype=np.uint64)
    key = np.array([seed & M32, ((seed >> 32) ^ (j >> 32)) & M32], dtype=np.uint64)
    ctr = np.stack([c, np.full_like(c, j & M32), np.full_like(c, SITE_SYNTH), np.full_like(c, stream)], axis=-1)
    return philox4x32(ctr, key, 7)


def host_frame(fs, j, stream):
    """-> (class, snr as np.float32 (NaN without noise), theta as np.float32, symbols (len,) int64) of frame j"""
    K, ns, length = fs.n_classes, len(fs.snrs_db), fs.length
    par = [int(v) for v in words(fs.seed, stream, j, [0xFFFFFFFF])[0]]
    if fs.balanced:
        cls, si = j % K, (j // K) % ns if ns else 0
    else:
        cls, si = (par[1] * K) >> 32, (par[2] * ns) >> 32
    snr = np.float32(fs.snrs_db[si]) if ns else np.float32(np.nan)
    theta = np.float32(2 * np.pi) * np.float32((par[0] >> 8) * 2.0 ** -24)
    w = words(fs.seed, stream, j, np.arange((length + 2 + 3) // 4)).reshape(-1)[:length + 2].astype(np.int64)
    kind, _, count = fs.descriptors[cls]
    n = np.arange(length)
    if kind == 0:
        sym = (w[:length] * count) >> 32                       # 32-bit word * count < 2^63
    elif kind == 1:
        b = 2 * (w & 1) - 1
        sym = np.cumsum(b[:-2] + 2 * b[1:-1] + b[2:]) % 16
    else:
        t = w & 1
        sym = 2 * t[n // 2] + t[length // 2 + 1 + (n + 1) // 2]
    return cls, snr, theta, sym


def check_integers(fs, n, frame_base, stream, frames):
    raw, y, z, drawn, sym = fs.generate(n, frame_base, stream, return_drawn=True, return_symbols=True)
    y, z, drawn, sym = y.cpu().numpy(), z.cpu().numpy(), drawn.cpu().numpy(), sym.cpu().numpy()
    assert y.dtype == np.int64 and z.dtype == np.float32 and sym.dtype == np.int32 and raw.shape == (n, fs.length, 2)
    kinds = set()
    for i in frames:
        cls, snr, theta, ref = host_frame(fs, frame_base + i, stream)
        kinds.add(fs.descriptors[cls][0])
        assert y[i] == cls and drawn[i, 0] == cls, (i, y[i], cls)
        assert z[i].view(np.int32) == snr.view(np.int32) and drawn[i, 1].view(np.int32) == snr.view(np.int32), (i, z[i], snr)
        assert abs(float(drawn[i, 2]) - float(theta)) <= 2.0 ** -23 * float(theta), (i, drawn[i, 2], theta)       # one fp32 product
        assert np.array_equal(sym[i].astype(np.int64), ref), (i, fs.class_names[cls], np.flatnonzero(sym[i] != ref)[:8])
    return kinds


@pytest.mark.parametrize("length", [1024, 33, 8192])
def test_symbols_labels_and_snrs_are_the_host_restatement(length):
    from vit_vs_raw_iq_amd import FrameSynth
    fs = FrameSynth(length=length, seed=0x1234567800000011)
    # balanced: every class at every SNR (a third of the frames at the LDS limit, GMSK and OQPSK among them)
    assert check_integers(fs, 76, 0, 0, range(76) if length != 8192 else range(1, 76, 3)) == {0, 1, 2}
    # a frame index past 2^32 (its high word is part of the key) on another stream: classes 11..18, 0..12
    assert check_integers(fs, 21, 2 ** 32 + 5, 1, range(21)) == {0, 1, 2}
    if length != 8192:
        # class and SNR drawn from words 1 and 2 of the frame's parameters
        un = FrameSynth(length=length, seed=7, balanced=False)
        kinds = check_integers(un, 76, 2 ** 32 + 5, 1, range(0, 76, 3))
        assert 0 in kinds
        g = FrameSynth(["GMSK", "OQPSK", "QPSK"], snrs_db=None, length=length, seed=9, balanced=False)
        assert check_integers(g, 12, 3, 0, range(12)) == {0, 1, 2}


@pytest.mark.parametrize("length", [1024, 33, 8192])
def test_deterministic_part_matches_the_fp64_reference(length):
    """fp32 bound, as for the rotate-and-scale of the impairments: the phase in turns rounds at 2^-24 turns = 4e-7 rad, the
    table, the two products, the reciprocal square root and the scaling add a few ulp: 1e-4 of the frame's peak, absolute.  The
    power of the result: each of len squared fp32 samples is within 2.4e-7 relative, the fp32 power sum the kernel divides by
    within len * 2^-24 / 4 of the true one in the worst case of its 4 x 64 x (len / 256) tree: 1e-5."""
    from vit_vs_raw_iq_amd import FrameSynth, synth_reference
    n = 76 if length != 8192 else 19
    fs = FrameSynth(snrs_db=None, length=length, seed=3)
    raw, y, z, drawn, sym = fs.generate(n, 0, 0, return_drawn=True, return_symbols=True)
    assert z.isnan().all() and drawn[:, 1].isnan().all()
    ref = synth_reference(sym, drawn, fs)
    got = raw.cpu().numpy().astype(np.float64)
    peak = np.abs(ref).reshape(n, -1).max(axis=1)
    err = np.abs(got - ref).reshape(n, -1).max(axis=1)
    power = (got ** 2).sum(axis=2).mean(axis=1)
    print(f"len {length}: max |raw - fp64 reference| / frame peak = {(err / peak).max():.3e}, max |mean |s|^2 - 1| = "
          f"{np.abs(power - 1).max():.3e}")
    assert np.all(err <= 1e-4 * peak), (err / peak)
    assert np.all(np.abs(power - 1) <= 1e-5), power
    d = drawn.cpu().numpy().astype(np.float64)
    assert np.all((d[:, 2] >= 0) & (d[:, 2] < 2 * np.pi + 1e-6)) and len(set(d[:, 2])) == n
    # the power before the normalisation, recomputed from the symbols: 1 for GMSK and OQPSK, the table's otherwise
    s_np, y_np = sym.cpu().numpy(), y.cpu().numpy()
    table = (fs.points.astype(np.float64) ** 2).sum(axis=1)
    for i in range(n):
        kind, off, _ = fs.descriptors[y_np[i]]
        want = table[off + s_np[i]].mean() if kind == 0 else 1.0
        assert abs(d[i, 3] - want) <= 1e-5 * want, (i, d[i, 3], want)


def test_frames_are_keyed_and_do_not_depend_on_how_the_stream_is_cut():
    from vit_vs_raw_iq_amd import FrameSynth
    fs = FrameSynth(length=1024, seed=7)
    a = fs.generate(76, 0, 0, return_drawn=True, return_symbols=True)
    b = fs.generate(76, 0, 0, return_drawn=True, return_symbols=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v) if u.dtype != torch.float32 else same_bits(u, v)
    # frames 40..75 of one call = a 36-frame call at frame_base 40, noise included
    t = fs.generate(36, 40, 0, return_drawn=True, return_symbols=True)
    assert same_bits(t[0], a[0][40:]) and torch.equal(t[1], a[1][40:]) and same_bits(t[2], a[2][40:])
    assert same_bits(t[3], a[3][40:]) and torch.equal(t[4], a[4][40:])
    odd = FrameSynth(length=33, seed=7)                          # and on the 8-byte store path
    assert same_bits(odd.generate(36, 40, 0)[0], odd.generate(76, 0, 0)[0][40:])
    for other, base, stream in ((FrameSynth(length=1024, seed=8), 0, 0), (FrameSynth(length=1024, seed=7 + 2 ** 32), 0, 0),
                                (fs, 0, 1), (fs, 76 * 2 ** 32, 0)):          # the last: the same low word, the same classes
        o = other.generate(76, base, stream, return_drawn=True, return_symbols=True)
        assert torch.equal(o[1], a[1])                            # balanced: the same labels ...
        assert not torch.equal(o[3][:, 2], a[3][:, 2])            # ... another carrier phase,
        assert not torch.equal(o[4], a[4])                        # other symbols
        diff = (o[0] != a[0]).flatten(1).any(1)
        assert diff.all()                                         # and no frame in common


def test_drawn_classes_snrs_phases_and_symbols_follow_their_distributions():
    """6-sigma bounds on fixed seeds."""
    from vit_vs_raw_iq_amd import FrameSynth
    n = 4096
    fs = FrameSynth(length=32, seed=1, balanced=False)
    raw, y, z, drawn = fs.generate(n, 0, 0, return_drawn=True)
    y, z, d = y.cpu().numpy(), z.cpu().numpy(), drawn.cpu().numpy().astype(np.float64)
    K, ns = 19, 4
    counts = np.bincount(y, minlength=K)
    assert len(counts) == K
    bound = 6 * math.sqrt(n * (1 / K) * (1 - 1 / K))
    print("class counts", counts.tolist(), f"(expected {n / K:.1f} +- {bound:.1f})")
    assert np.all(np.abs(counts - n / K) <= bound)
    scount = [int((z == np.float32(s)).sum()) for s in fs.snrs_db]
    print("snr counts", scount)
    assert sum(scount) == n and all(abs(c - n / ns) <= 6 * math.sqrt(n * 0.25 * 0.75) for c in scount)
    # class and SNR are drawn from different words: their joint table is not degenerate
    assert len({(int(a), float(b)) for a, b in zip(y, z)}) == K * ns
    th = d[:, 2]
    assert th.min() >= 0 and th.max() < 2 * np.pi + 1e-6
    width = 2 * np.pi
    print(f"theta: mean {th.mean():.4f} (pi +- {6 * width / math.sqrt(12 * n):.4f}), variance / uniform {th.var() / (width ** 2 / 12):.4f}")
    assert abs(th.mean() - np.pi) <= 6 * width / math.sqrt(12 * n)
    # variance of the sample variance of a uniform: (4/5 - 1) ... kurtosis 9/5 -> sd = var * sqrt((9/5 - 1) / n)
    assert abs(th.var() - width ** 2 / 12) <= 6 * (width ** 2 / 12) * math.sqrt(0.8 / n)
    # 16QAM point counts over 64 x 1024 symbols
    q = FrameSynth(["16QAM"], snrs_db=None, length=1024, seed=2)
    sym = q.generate(64, 0, 0, return_symbols=True)[3].cpu().numpy()
    pc = np.bincount(sym.reshape(-1), minlength=16)
    print("16QAM point counts", pc.tolist())
    assert len(pc) == 16 and np.all(np.abs(pc - 4096) <= 6 * math.sqrt(4096 * 15 / 16))
    # GMSK: the bits are balanced.  b_n + 2 b_{n+1} + b_{n+2} = 4 iff three +1 in a row (1/8), -4 iff three -1; the mean step
    # is 0.  Recover the steps from the phase symbols.
    g = FrameSynth(["GMSK"], snrs_db=None, length=1024, seed=2)
    gs = g.generate(64, 0, 0, return_symbols=True)[3].cpu().numpy().astype(np.int64)
    step = np.diff(np.concatenate([np.zeros((64, 1), np.int64), gs], axis=1), axis=1)
    step = (step + 8) % 16 - 8                                    # steps are in {-4, -2, 0, 2, 4}
    assert set(np.unique(step)) == {-4, -2, 0, 2, 4}
    m = step.size
    frac = {v: float((step == v).mean()) for v in (-4, -2, 0, 2, 4)}
    print("GMSK step shares", frac)
    for v, p in ((-4, 1 / 8), (-2, 1 / 4), (0, 1 / 4), (2, 1 / 4), (4, 1 / 8)):
        assert abs(frac[v] - p) <= 6 * math.sqrt(p * (1 - p) / m) * math.sqrt(5)      # a step shares bits with 4 others: 5x the variance at most
    # the middle bit of each step decides its sign when it is not 0: b_{n+1} = sign(step); its share is the bit balance
    nz = step[step != 0]
    assert abs((nz > 0).mean() - 0.5) <= 6 * 0.5 / math.sqrt(len(nz)) * math.sqrt(5)
    # OQPSK: the four (I, Q) pairs are equally likely
    o = FrameSynth(["OQPSK"], snrs_db=None, length=1024, seed=2)
    os_ = o.generate(64, 0, 0, return_symbols=True)[3].cpu().numpy()
    oc = np.bincount(os_.reshape(-1), minlength=4)
    print("OQPSK pair counts", oc.tolist())
    assert len(oc) == 4 and np.all(np.abs(oc - 16384) <= 6 * math.sqrt(65536 * 3 / 16) * math.sqrt(3))   # a pair shares a bit with both neighbours


def test_noise_statistics_at_each_snr():
    """The bounds of test_noise_statistics_at_a_fixed_snr (tests/test_gpu_impairments.py), on the residual raw - noiseless."""
    from vit_vs_raw_iq_amd import FrameSynth, synth_reference
    fs = FrameSynth(snrs_db=(0.0,), length=1024, seed=2)
    raw, y, z, drawn, sym = fs.generate(8, 0, 0, return_drawn=True, return_symbols=True)
    assert torch.equal(z.cpu(), torch.zeros(8))
    sigma = math.sqrt(0.5)
    r = (raw.cpu().numpy().astype(np.float64) - synth_reference(sym, drawn, fs)) / sigma       # (8, 1024, 2)
    n = r.size
    assert n == 16384
    iq = (r[:, :, 0] * r[:, :, 1]).mean() / r.std() ** 2
    lag = (r[:, 1:, :] * r[:, :-1, :]).mean() / r.var()
    print(f"noise: mean {r.mean():+.4f}, variance {r.var():.4f}, I-Q correlation {iq:+.4f}, lag-1 {lag:+.4f}, max {np.abs(r).max():.3f}")
    assert abs(r.mean()) <= 6 / math.sqrt(n)
    assert abs(r.var() - 1) <= 6 * math.sqrt(2 / n)
    assert abs(iq) <= 6 / math.sqrt(n / 2) and abs(lag) <= 6 / math.sqrt(n / 2)
    assert np.abs(r).max() < 6.0                                                               # 24-bit uniforms: |g| <= 5.77
    # the SNR of every frame, at each of the four values (unit signal power: the estimate is -10 log10 of the noise power)
    four = FrameSynth(length=1024, seed=4)
    raw, y, z, drawn, sym = four.generate(76, 0, 0, return_drawn=True, return_symbols=True)
    resid = raw.cpu().numpy().astype(np.float64) - synth_reference(sym, drawn, four)
    est = -10 * np.log10((resid ** 2).sum(axis=2).mean(axis=1))
    zz = z.cpu().numpy().astype(np.float64)
    assert sorted(set(zz)) == sorted(four.snrs_db)
    print("per-frame SNR estimate - nominal:", np.round(est - zz, 3).tolist())
    assert np.all(np.abs(est - zz) <= 1.0)


def test_refusals_return_their_code_and_leave_the_output_untouched():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import FrameSynth
    L = N.lib()
    sentinel = 1234.5
    raw = torch.full((8, 1024, 2), sentinel, device=dev())
    y = torch.full((8,), 77, dtype=torch.int64, device=dev())
    z = torch.full((8,), sentinel, device=dev())
    drawn = torch.full((8, 4), sentinel, device=dev())
    sym = torch.full((8, 1024), 77, dtype=torch.int32, device=dev())
    fs = FrameSynth(length=1024)
    table = torch.from_numpy(fs.points).to(dev())
    ARG, UNSUPPORTED = 1, 2

    def call(r=raw.data_ptr(), lab=y.data_ptr(), s=z.data_ptr(), par="ok", length=1024, edit=None):
        if par == "ok":
            par = fs.struct(points=table.data_ptr())
        if edit:
            edit(par)
        return L.iq_frames_synth(r, lab, s, drawn.data_ptr(), sym.data_ptr(), 8, length,
                                 ctypes.byref(par) if par is not None else None, N.stream_handle())
    assert call(r=None) == ARG and call(lab=None) == ARG and call(s=None) == ARG and call(par=None) == ARG
    assert call(length=0) == ARG
    assert call(edit=lambda p: setattr(p, "n_classes", 0)) == ARG
    assert call(edit=lambda p: setattr(p, "points", None)) == ARG
    for kind, off, count in ((3, 0, 4), (-1, 0, 4), (0, 0, 0)):
        cls = (N.SynthClass * 1)(N.SynthClass(kind, off, count))

        def edit(p, cls=cls):
            p.classes, p.n_classes = cls, 1
        assert call(edit=edit) == ARG, (kind, off, count)
    for bad in (float("nan"), float("inf")):
        sn = (ctypes.c_float * 1)(bad)

        def edit(p, sn=sn):
            p.snrs_db, p.n_snrs = sn, 1
        assert call(edit=edit) == ARG, bad
    assert call(length=8193) == UNSUPPORTED                                                # 65544 bytes of LDS for one frame
    torch.cuda.synchronize()
    assert torch.equal(raw, torch.full_like(raw, sentinel)) and torch.equal(z, torch.full_like(z, sentinel))
    assert torch.equal(drawn, torch.full_like(drawn, sentinel))
    assert torch.equal(y, torch.full_like(y, 77)) and torch.equal(sym, torch.full_like(sym, 77))


def preprocess(raw, take, stats):
    import vit_vs_raw_iq_amd._native as N
    B, length = raw.shape[0], raw.shape[1]
    out = torch.empty(B, 2, take, device=raw.device)
    st = (ctypes.c_float * 4)(stats["i_mean"], stats["i_std"], stats["q_mean"], stats["q_std"])
    N.check(N.lib().iq_frames_preprocess(raw.data_ptr(), out.data_ptr(), B, length, take, st, N.stream_handle()),
            "iq_frames_preprocess")
    return out


def test_stream_is_generate_then_the_input_pipeline():
    from vit_vs_raw_iq_amd import FrameSynth, Impairments, SynthStream, impair
    fs = FrameSynth(length=1024, seed=5)
    stats = fs.stats(n_subset=76)
    raw76 = fs.generate(76, 0, 0)[0].cpu().numpy().astype(np.float64)
    assert abs(stats["i_mean"] - raw76[:, :, 0].mean()) < 1e-4 and abs(stats["q_std"] - raw76[:, :, 1].std(ddof=1)) < 1e-4
    B, s = 12, 3
    raw, y, z = fs.generate(B, s * B, 0)
    aug = Impairments.augmentation().replace(snr_db=(5.0, 15.0))
    for layout, h, w, take in (("rawiq", 32, 64, 1024), ("vit", 32, 64, 1024), ("vit", 32, 32, 512)):
        st = SynthStream(fs, stats, layout, B, h=h, w=w)
        x, ys, zs = st.get(s)
        assert x.shape == ((B, 2, 1024) if layout == "rawiq" else (B, 1, h, w))
        assert same_bits(x.reshape(B, 2, take), preprocess(raw, take, stats)) and torch.equal(ys, y) and same_bits(zs, z)
        xa, ya, _ = SynthStream(fs, stats, layout, B, h=h, w=w, augment=aug).get(s)
        assert same_bits(xa, impair(raw, stats, layout, aug, seed=fs.seed, step=0, frame_base=s * B, h=h, w=w)) and torch.equal(ya, y)
        assert not torch.equal(xa, x)
    # another stream: its own frames (and its own impairment draws), the same balanced labels
    v = SynthStream(fs, stats, "rawiq", B, stream=1, augment=aug)
    raw1 = fs.generate(B, s * B, 1)[0]
    xv, yv, _ = v.get(s)
    assert same_bits(xv, impair(raw1, stats, "rawiq", aug, seed=fs.seed, step=1, frame_base=s * B)) and torch.equal(yv, y)
    # streams 0 and 1 share no frame: no frame of 76 of one equals any frame of the other
    a = fs.generate(76, 0, 0)[0].flatten(1)
    b = fs.generate(76, 0, 1)[0].flatten(1)
    assert not (a[:, None, :64] == b[None, :, :64]).all(-1).any()
    got = [t[1] for t in SynthStream(fs, stats, "rawiq", B).batches(2, first_step=1)]
    assert len(got) == 2 and torch.equal(got[0], fs.generate(B, B, 0)[1]) and torch.equal(got[1], fs.generate(B, 2 * B, 0)[1])


def small_model():
    import vit_vs_raw_iq_amd as P
    return P.AMCTransformerRawIQ(in_channels=2, seq_length=1024, num_classes=4, d_model=128, n_head=8, n_layers=2, ffn_hidden=256,
                                 drop_prob=0.0, device="cuda", use_cls_token=True, embedding_type="segment", segment_size=16)


@functools.lru_cache(maxsize=None)
def four_class_source():
    """(FrameSynth of OOK / BPSK / QPSK / 16QAM at 20 dB, its statistics): made once, never modified."""
    from vit_vs_raw_iq_amd import FrameSynth
    fs = FrameSynth(FOUR, snrs_db=(20.0,), length=1024, seed=11)
    return fs, fs.stats(n_subset=1024)


TRAIN_STEPS = 100        # first candidate of "the smallest multiple of 100 that clears the bound": not yet confirmed on a device
                         # (profiles/synth.txt); the bound below is derived and stays whatever the budget becomes


def test_a_model_trained_on_the_stream_beats_chance_on_frames_of_another_stream(tmp_path):
    """Every step trains on 256 frames that were never used; the accuracy on 2048 frames of stream 1 must exceed chance by 6
    standard deviations of a 2048-frame estimate at chance: 1/4 + 6 sqrt((1/4)(3/4)/2048) = 0.3074."""
    from vit_vs_raw_iq_amd import SynthStream, train_on_stream
    from vit_vs_raw_iq_amd.evaluation import evaluate_model_with_confusion
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    fs, stats = four_class_source()
    torch.manual_seed(0)
    m = small_model().to(dev()).train()
    tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-3)
    train = SynthStream(fs, stats, "rawiq", 256)
    assert train_on_stream(tr, train, TRAIN_STEPS) == TRAIN_STEPS
    loss, acc_train, frames = tr.read_stats()
    assert frames == TRAIN_STEPS * 256
    held = SynthStream(fs, stats, "rawiq", 256, stream=1)
    res = evaluate_model_with_confusion(m, held.batches(8), dev(), FOUR, tmp_path, prefix="synth")
    bound = 0.25 + 6 * math.sqrt(0.25 * 0.75 / 2048)
    print(f"{TRAIN_STEPS} steps of 256 fresh frames: running train loss {loss:.4f}, accuracy {acc_train:.4f}; "
          f"held-out accuracy on 2048 frames of stream 1 {res['overall_accuracy']:.4f} (bound {bound:.4f})")
    _, y, z = fs.generate(2048, 0, 1)
    assert np.array_equal(res["labels"], y.cpu().numpy()) and np.array_equal(res["labels"], np.arange(2048) % 4)
    assert np.array_equal(res["snrs"], z.cpu().numpy()) and np.all(res["snrs"] == np.float32(20.0))
    assert res["confusion_matrix"].sum() == 2048 and (tmp_path / "synth_classification_report.txt").exists()
    assert m.training
    assert res["overall_accuracy"] > bound


def test_graph_replay_of_the_step_on_stream_batches_equals_eager():
    """As test_graph_replay_equals_eager (tests/test_gpu_trainer.py): the same parameters, bit for bit, and the same loss to 1e-5."""
    from vit_vs_raw_iq_amd import SynthStream, train_on_stream
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    fs, stats = four_class_source()
    torch.manual_seed(1)
    sd = {k: v.detach().clone() for k, v in small_model().state_dict().items()}
    outs = []
    for use_graph in (False, True):
        m = small_model()
        m.load_state_dict(sd)
        m.to(dev()).train()
        tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-3, use_graph=use_graph, dropout_seed=77)
        train_on_stream(tr, SynthStream(fs, stats, "rawiq", 64), 3, first_step=2)
        loss, _, frames = tr.read_stats()
        assert frames == 3 * 64
        outs.append((loss, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    assert abs(outs[0][0] - outs[1][0]) < 1e-5
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k
