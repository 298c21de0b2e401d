"""GPU (MI355X): channel impairments on the device (csrc/impair.hip, iq_frames_impair, vit_vs_raw_iq_amd.impairments).

1. Identity: with nothing switched on the call is iq_frames_preprocess bit for bit (both layouts, a frame shorter than a
   workgroup, an odd length that takes the 8-byte load / 4-byte store path, -0.0 samples).
2. The deterministic part (shift, conjugate, phase + quarter turns + frequency offset, gain) against the host fp64 definition
   impair_reference, rebuilt from the `drawn` table the kernel returns.
3. Reproducibility and keying: same (seed, step, frame_base) = same bits; another step or seed = other draws; a frame's result
   does not depend on how the stream of frames is cut into calls, noise included.
4. The distributions of the drawn parameters, 5. the statistics of the noise: 6-sigma bounds on fixed seeds.
6. Refusals leave the output untouched.  7. DeviceInputPipeline(augment=...).  8. impairment_curve on a trained classifier.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from frontend_gpu import dev, same_bits

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def dataset(n=8, length=1024):
    """(raw frames (n, length, 2) fp32 numpy, the same on the device, stats dict): computed once, never modified."""
    from vit_vs_raw_iq_amd import data as D
    X, _, _ = D.make_dataset(n, seed=1, n_symbols=length)
    mean, std = D.zscore_stats(X)
    stats = {"i_mean": float(mean[0]), "i_std": float(std[0]), "q_mean": float(mean[1]), "q_std": float(std[1])}
    return X, torch.from_numpy(X).to(dev()), stats


def cstats(stats):
    return (ctypes.c_float * 4)(stats["i_mean"], stats["i_std"], stats["q_mean"], stats["q_std"])


def raw_call(raw, take, stats, par, want_drawn=False, out=None):
    """iq_frames_impair through the C ABI -> (status, out (B, 2, take), drawn or None)"""
    import vit_vs_raw_iq_amd._native as N
    B, length = raw.shape[0], raw.shape[1]
    if out is None:
        out = torch.empty(B, 2, take, device=raw.device)
    drawn = torch.empty(B, 8, device=raw.device) if want_drawn else None
    rc = N.lib().iq_frames_impair(raw.data_ptr(), out.data_ptr(), N.ptr(drawn), B, length, take, cstats(stats),
                                  ctypes.byref(par), N.stream_handle())
    return rc, out, drawn


def preprocess(raw, take, stats):
    import vit_vs_raw_iq_amd._native as N
    B, length = raw.shape[0], raw.shape[1]
    out = torch.empty(B, 2, take, device=raw.device)
    N.check(N.lib().iq_frames_preprocess(raw.data_ptr(), out.data_ptr(), B, length, take, cstats(stats), N.stream_handle()),
            "iq_frames_preprocess")
    return out


@pytest.mark.parametrize("length,take", [(1024, 1024), (1024, 512), (32, 32), (32, 16), (33, 33), (33, 7)])
def test_identity_is_bit_exact(length, take):
    from vit_vs_raw_iq_amd import Impairments
    _, raw, stats = dataset(8, length)
    raw = raw.clone()
    raw[0, 0, 0] = -0.0
    raw[1, 3, 1] = -0.0
    raw[2, 5, :] = -0.0
    ident = Impairments().struct(seed=3, step=9, frame_base=11)
    for st in (stats, {"i_mean": 0.0, "i_std": 1.0, "q_mean": 0.0, "q_std": 2.0}):       # mean 0 keeps the sign of -0.0 visible
        ref = preprocess(raw, take, st)
        rc, out, drawn = raw_call(raw, take, st, ident, want_drawn=True)
        assert rc == 0
        assert same_bits(out, ref)
        d = drawn.cpu()
        assert torch.equal(d[:, :5], torch.zeros(8, 5)) and torch.equal(d[:, 5], torch.ones(8))
        assert d[:, 6].isnan().all() and torch.equal(d[:, 7], torch.zeros(8))
    assert (preprocess(raw, take, {"i_mean": 0.0, "i_std": 1.0, "q_mean": 0.0, "q_std": 2.0}).view(torch.int32)[0, 0, 0].item()
            == -2 ** 31)                                                                 # the -0.0 did reach the output


@pytest.mark.parametrize("length,layout,h,w", [(1024, "rawiq", 0, 0), (1024, "vit", 32, 32), (33, "rawiq", 0, 0)])
def test_deterministic_part_matches_the_fp64_reference(length, layout, h, w):
    """fp32 bound: |f n| <= 10.24 turns rounds at about 1e-6 turns = 6e-6 rad, plus a few ulp of the sincos and of the two
    products: 1e-4 of the frame's peak |z-scored sample|, absolute."""
    from vit_vs_raw_iq_amd import Impairments, impair, impair_reference
    X, raw, stats = dataset(8, length)
    imp = Impairments(phase=(-math.pi, math.pi), cfo=(-0.01, 0.01), rot90=True, conj=True, shift_max=length - 1,
                      gain_db=(-3.0, 3.0))
    out, drawn = impair(raw, stats, layout, imp, seed=5, step=2, frame_base=0, h=h, w=w, return_drawn=True)
    d = drawn.cpu().numpy().astype(np.float64)
    assert np.all(d[:, 2] == np.round(d[:, 2])) and np.all((d[:, 2] >= 0) & (d[:, 2] <= 3))
    assert np.all((d[:, 3] == 0) | (d[:, 3] == 1))
    assert np.all(d[:, 4] == np.round(d[:, 4])) and np.all((d[:, 4] >= 0) & (d[:, 4] <= length - 1))
    assert np.all(np.abs(d[:, 0]) <= np.float32(math.pi)) and np.all(np.abs(d[:, 1]) <= np.float32(0.01))
    assert np.all((d[:, 5] >= 10 ** (-3 / 20) * (1 - 1e-6)) & (d[:, 5] <= 10 ** (3 / 20) * (1 + 1e-6)))
    assert np.isnan(d[:, 6]).all() and np.all(d[:, 7] == 0)
    assert len(set(d[:, 4])) > 1 and len(set(d[:, 0])) == 8                              # the frames do differ
    ref = impair_reference(X, d, stats, layout, h or 32, w or 64)
    got = out.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    B = len(X)
    peak = np.abs(ref.reshape(B, -1)).max(axis=1)
    err = np.abs(got - ref).reshape(B, -1).max(axis=1)
    print(f"len {length} {layout}: max |out - fp64 reference| / frame peak = {(err / peak).max():.3e}")
    assert np.all(err <= 1e-4 * peak), (err / peak)


def test_reproducible_and_keyed_by_seed_step_and_absolute_frame_index():
    from vit_vs_raw_iq_amd import Impairments, impair
    _, raw, stats = dataset()
    imp = Impairments(phase=(-math.pi, math.pi), cfo=(-0.01, 0.01), rot90=True, conj=True, shift_max=1023, gain_db=(-3.0, 3.0),
                      snr_db=(0.0, 20.0))
    a, da = impair(raw, stats, "rawiq", imp, seed=7, step=3, return_drawn=True)
    b, db = impair(raw, stats, "rawiq", imp, seed=7, step=3, return_drawn=True)
    assert same_bits(a, b) and same_bits(da, db)
    _, d_step = impair(raw, stats, "rawiq", imp, seed=7, step=4, return_drawn=True)
    _, d_seed = impair(raw, stats, "rawiq", imp, seed=8, step=3, return_drawn=True)
    _, d_hi = impair(raw, stats, "rawiq", imp, seed=7 + 2 ** 32, step=3, return_drawn=True)
    for other in (d_step, d_seed, d_hi):
        assert not torch.equal(other[:, 0], da[:, 0]) and not torch.equal(other[:, 1], da[:, 1])
    # frames 4..7 of the 8-frame call = a 4-frame call on raw[4:] at frame_base 4, noise included
    t, dt = impair(raw[4:], stats, "rawiq", imp, seed=7, step=3, frame_base=4, return_drawn=True)
    assert same_bits(t, a[4:]) and same_bits(dt, da[4:])
    v = impair(raw[4:], stats, "vit", imp, seed=7, step=3, frame_base=4, h=32, w=32)       # and the image is a prefix of it
    assert same_bits(v.view(4, 2, 512), a[4:, :, :512])
    z, dz = impair(raw[4:], stats, "rawiq", imp, seed=7, step=3, frame_base=0, return_drawn=True)
    assert same_bits(dz[:, :7], da[:4, :7]) and not torch.equal(z, a[4:])
    # the high word of the frame index is part of the key
    _, dbig = impair(raw[:4], stats, "rawiq", imp, seed=7, step=3, frame_base=2 ** 32, return_drawn=True)
    assert not torch.equal(dbig[:, 0], da[:4, 0])


def test_drawn_parameters_follow_their_distributions():
    """6-sigma bounds on a fixed seed: a failure is a defect, not chance."""
    from vit_vs_raw_iq_amd import Impairments, impair
    n = 4096
    g = torch.Generator().manual_seed(0)
    raw = torch.randn(n, 32, 2, generator=g).to(dev())
    stats = {"i_mean": 0.0, "i_std": 1.0, "q_mean": 0.0, "q_std": 1.0}
    imp = Impairments(phase=(-math.pi, math.pi), cfo=(-0.01, 0.01), rot90=True, conj=True, shift_max=31)
    _, drawn = impair(raw, stats, "rawiq", imp, seed=1, step=0, return_drawn=True)
    d = drawn.cpu().numpy().astype(np.float64)
    for col, lo, hi in ((0, -math.pi, math.pi), (1, -0.01, 0.01)):
        v = d[:, col]
        assert v.min() >= float(np.float32(lo)) and v.max() <= float(np.float32(hi))
        width = hi - lo
        print(f"column {col}: mean {v.mean():+.5f} (bound {6 * width / math.sqrt(12 * n):.5f}), "
              f"variance / uniform variance {v.var() / (width ** 2 / 12):.4f}")
        assert abs(v.mean() - (lo + hi) / 2) <= 6 * width / math.sqrt(12 * n)
        assert abs(v.var() - width ** 2 / 12) <= 0.1 * width ** 2 / 12
    k = d[:, 2]
    assert set(np.unique(k)) == {0.0, 1.0, 2.0, 3.0}
    counts = [int((k == i).sum()) for i in range(4)]
    print("k counts", counts, "conj", int(d[:, 3].sum()))
    assert all(abs(c - 1024) <= 6 * math.sqrt(768) for c in counts)
    assert set(np.unique(d[:, 3])) == {0.0, 1.0} and abs(d[:, 3].sum() - 2048) <= 6 * 32
    s = d[:, 4]
    assert np.all(s == np.round(s)) and s.min() == 0 and s.max() == 31
    assert np.all(d[:, 5] == 1.0) and np.isnan(d[:, 6]).all()


def test_noise_statistics_at_a_fixed_snr():
    from vit_vs_raw_iq_amd import Impairments, impair
    X, raw, stats = dataset()
    out, drawn = impair(raw, stats, "rawiq", Impairments(snr_db=0), seed=2, step=0, return_drawn=True)
    d = drawn.cpu().numpy().astype(np.float64)
    assert np.all(d[:, :5] == 0) and np.all(d[:, 5] == 1) and np.all(d[:, 6] == 0)
    x64 = X.astype(np.float64)
    p_given = (x64 ** 2).sum(axis=2).mean(axis=1)                                          # mean |s|^2 per frame
    np.testing.assert_allclose(d[:, 7], np.sqrt(p_given / 2), rtol=1e-5)
    o = out.cpu().numpy().astype(np.float64)
    mean = np.array([float(np.float32(stats["i_mean"])), float(np.float32(stats["q_mean"]))])
    std = np.array([float(np.float32(stats["i_std"])), float(np.float32(stats["q_std"]))])
    resid = o * std[None, :, None] + mean[None, :, None] - np.transpose(x64, (0, 2, 1))    # (8, 2, 1024): the noise itself
    snr_est = 10 * np.log10(p_given / (resid ** 2).sum(axis=1).mean(axis=1))
    r = resid / d[:, 7][:, None, None]
    n = r.size
    assert n == 16384
    iq = (r[:, 0] * r[:, 1]).mean() / r.std() ** 2
    lag = (r[:, :, 1:] * r[:, :, :-1]).mean() / r.var()
    print(f"noise: mean {r.mean():+.4f}, variance {r.var():.4f}, I-Q correlation {iq:+.4f}, lag-1 {lag:+.4f}, "
          f"per-frame SNR estimate {np.round(snr_est, 3)}")
    assert abs(r.mean()) <= 6 / math.sqrt(n)
    assert abs(r.var() - 1) <= 6 * math.sqrt(2 / n)
    assert abs(iq) <= 6 / math.sqrt(n / 2) and abs(lag) <= 6 / math.sqrt(n / 2)
    assert np.all(np.abs(snr_est) <= 1.0)
    assert np.abs(r).max() < 6.0                                                           # 24-bit uniforms: |g| <= 5.77


def test_refusals_return_their_code_and_leave_the_output_untouched():
    from vit_vs_raw_iq_amd import Impairments
    _, raw, stats = dataset()
    sentinel = 1234.5
    out = torch.full((8, 2, 1024), sentinel, device=dev())
    drawn = torch.full((8, 8), sentinel, device=dev())
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    ARG, UNSUPPORTED = 1, 2
    ok = Impairments(snr_db=10.0).struct()

    def call(imp=ok, r=raw.data_ptr(), o=out.data_ptr(), st=cstats(stats), length=1024, take=1024):
        return L.iq_frames_impair(r, o, drawn.data_ptr(), 8, length, take, st, ctypes.byref(imp) if imp is not None else None,
                                  N.stream_handle())
    assert call(r=None) == ARG and call(o=None) == ARG and call(st=None) == ARG and call(imp=None) == ARG
    assert call(take=1025) == ARG
    nan, inf = float("nan"), float("inf")
    for field, lo, hi in (("phase", 1.0, 0.0), ("cfo", 0.1, -0.1), ("gain_db", 3.0, -3.0), ("snr_db", 10.0, 0.0),
                          ("phase", nan, 0.0), ("cfo", 0.0, nan), ("gain_db", nan, nan), ("snr_db", nan, 0.0),
                          ("snr_db", 0.0, nan), ("phase", 0.0, inf), ("cfo", -inf, 0.0), ("gain_db", -inf, inf),
                          ("snr_db", 0.0, inf)):
        s = Impairments(snr_db=10.0).struct()
        setattr(s, field + "_lo", lo)
        setattr(s, field + "_hi", hi)
        assert call(imp=s) == ARG, (field, lo, hi)
    for v in (-1, 1024, 5000):
        s = Impairments().struct()
        s.shift_max = v
        assert call(imp=s) == ARG, v
    assert call(length=8193, take=8193) == UNSUPPORTED                                     # 65544 bytes of LDS for one frame
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, sentinel)) and torch.equal(drawn, torch.full_like(drawn, sentinel))


def test_longest_supported_frame():
    """len * 8 = 64 KB exactly is supported (the workgroup asks for more than the default 48 KB of dynamic LDS)."""
    from vit_vs_raw_iq_amd import Impairments, impair, impair_reference
    g = torch.Generator().manual_seed(4)
    X = torch.randn(2, 8192, 2, generator=g)
    stats = {"i_mean": 0.1, "i_std": 0.9, "q_mean": -0.2, "q_std": 1.1}
    ident = impair(X.to(dev()), stats, "rawiq", Impairments())
    assert same_bits(ident, preprocess(X.to(dev()), 8192, stats))
    imp = Impairments(phase=(-1.0, 1.0), conj=True, shift_max=8191, gain_db=(-1.0, 1.0))
    out, drawn = impair(X.to(dev()), stats, "rawiq", imp, seed=1, return_drawn=True)
    ref = impair_reference(X, drawn, stats, "rawiq")
    err = np.abs(out.cpu().numpy() - ref).reshape(2, -1).max(axis=1)
    assert np.all(err <= 1e-4 * np.abs(ref).reshape(2, -1).max(axis=1))


def test_input_pipeline_with_and_without_augmentation():
    from vit_vs_raw_iq_amd import Impairments, data as D, impair
    X, raw, stats = dataset()
    for layout, h, w, take in (("rawiq", 32, 64, 1024), ("vit", 32, 32, 512)):
        plain = D.DeviceInputPipeline(stats, layout, batch=8, h=h, w=w)
        a = plain(X)
        assert torch.equal(a.cpu(), torch.from_numpy(D.preprocess_reference(X, stats, layout, h, w)))     # today's output
        assert same_bits(a.reshape(8, 2, take), preprocess(raw, take, stats))
        fixed = D.DeviceInputPipeline(stats, layout, batch=8, h=h, w=w, augment=Impairments(phase=0.5))
        for step in (0, 1):
            assert same_bits(fixed(X), impair(raw, stats, layout, Impairments(phase=0.5), step=step, h=h, w=w))
        aug = Impairments.augmentation().replace(snr_db=(5.0, 15.0))
        pipe = D.DeviceInputPipeline(stats, layout, batch=8, h=h, w=w, augment=aug, seed=21)
        got = [pipe(X), pipe(X)]
        for step in (0, 1):
            assert same_bits(got[step], impair(raw, stats, layout, aug, seed=21, step=step, h=h, w=w))
        assert not torch.equal(got[0], got[1])                                            # every get() draws afresh
        pipe.submit(X[:5])
        assert same_bits(pipe.get(step=7), impair(raw[:5], stats, layout, aug, seed=21, step=7, h=h, w=w))
    with pytest.raises(TypeError):
        D.DeviceInputPipeline(stats, "rawiq", batch=8, augment=0.5)
    with pytest.raises(ValueError):
        D.DeviceInputPipeline(stats, "rawiq", batch=8, length=512, augment=Impairments.augmentation())    # shift_max 1023


def build(kind, kw):
    import vit_vs_raw_iq_amd as P
    cls = P.AMCTransformerViT if kind == "vit" else P.AMCTransformerRawIQ
    return cls(drop_prob=0.0, device="cuda", **kw)


def trained_rawiq():
    """A small raw-IQ classifier trained on four classes of the synthetic task (data.py) at 8 dB: the recipe of
    tests/test_gpu_input_grad.py, keeping the raw held-out frames and the statistics."""
    from vit_vs_raw_iq_amd import data as D
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    d = dev()
    X, Y, _ = D.make_dataset(640, seed=3, classes=["BPSK", "QPSK", "16QAM", "OOK"], snrs_db=(8.0,), n_symbols=1024)
    mean, std = D.zscore_stats(X)
    x = torch.from_numpy(D.to_rawiq(X, mean, std)).float().to(d)
    y = torch.from_numpy(Y).long().to(d)
    torch.manual_seed(0)
    m = build("rawiq", dict(in_channels=2, seq_length=1024, num_classes=4, d_model=64, n_head=4, n_layers=2, ffn_hidden=128,
                            use_cls_token=True, embedding_type="segment", segment_size=64)).to(d)
    tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-3)
    for epoch in range(6):
        for i in range(0, 512, 64):
            tr.step(x[i:i + 64], y[i:i + 64])
    return m.eval(), x[512:], y[512:], torch.from_numpy(X[512:]).to(d), (mean, std)


def test_impairment_curve_of_a_trained_model():
    from vit_vs_raw_iq_amd import Impairments, impairment_curve
    m, x, y, raw, stats = trained_rawiq()
    with torch.no_grad():
        clean = (m(x).argmax(1) == y).float().mean().item()
    assert impairment_curve(m, raw, y, stats, "phase", [0.0]) == [clean]
    assert impairment_curve(m, raw, y, stats, "shift", [0]) == [clean]
    base = Impairments(phase=(-math.pi, math.pi), snr_db=(0.0, 10.0), shift_max=1023)
    for kind, values in (("snr_db", [-20, 0.0, 30]), ("phase", [0.0, 0.4, math.pi / 2]), ("cfo", [0.0, 1e-4, 1e-2]),
                         ("shift", [0, 1, 517]), ("gain_db", [-6.0, 0.0, 6.0])):
        a = impairment_curve(m, raw, y, stats, kind, values, batch=32, seed=5)
        b = impairment_curve(m, raw, y, stats, kind, values, batch=128, seed=5)
        print(f"trained raw-IQ, clean accuracy {clean:.4f}: {kind} {values} -> {a}")
        assert a == b and all(0.0 <= v <= 1.0 for v in a)
    a = impairment_curve(m, raw, y, stats, "gain_db", [0.0], base=base, batch=32, seed=5)
    assert a == impairment_curve(m, raw, y, stats, "gain_db", [0.0], base=base, batch=128, seed=5)
    snr = impairment_curve(m, raw, y, stats, "snr_db", [-20, 30])
    print(f"accuracy at -20 dB {snr[0]:.4f}, at 30 dB {snr[1]:.4f}, clean {clean:.4f}")
    assert snr[0] <= snr[1]                      # (measured accuracies: none recorded yet -- this file has not run on a device)
    assert not m.training
    m.train()
    impairment_curve(m, raw, y, stats, "phase", [0.1])
    assert m.training


def test_impairment_curve_takes_the_image_geometry_from_a_vit():
    from vit_vs_raw_iq_amd import data as D, impairment_curve
    X, raw, stats = dataset()
    torch.manual_seed(0)
    m = build("vit", dict(in_channels=1, img_size_h=32, img_size_w=32, patch_size=16, num_classes=4, d_model=64, n_head=4,
                          n_layers=1, ffn_hidden=128)).to(dev()).eval()
    y = torch.arange(8, device=dev()) % 4
    x = torch.from_numpy(D.preprocess_reference(X, stats, "vit", 32, 32)).to(dev())
    with torch.no_grad():
        clean = (m(x).argmax(1) == y).float().mean().item()
    assert impairment_curve(m, raw, y, stats, "gain_db", [0.0], batch=3) == [clean]
