"""CPU: vit_vs_raw_iq_amd.impairments -- argument validation (raised before any device work), the host fp64 definition
`impair_reference` (identity, power, quarter turns, shifts), the iq_impair_t binding against include/iqvit.h and the refusals
of iq_frames_impair that return before any HIP call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iqvit.h")
IDENT_STATS = {"i_mean": 0.0, "i_std": 1.0, "q_mean": 0.0, "q_std": 1.0}


def frames(n=8, length=1024):
    from vit_vs_raw_iq_amd import data as D
    X, _, _ = D.make_dataset(n, seed=1, n_symbols=length)
    return X


def drawn_rows(n, theta=0.0, f=0.0, k=0, conj=0, s=0, g=1.0):
    d = np.zeros((n, 8))
    d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4], d[:, 5], d[:, 6] = theta, f, k, conj, s, g, np.nan
    return d


def test_impairments_validation_and_fixed_values():
    from vit_vs_raw_iq_amd import Impairments
    a = Impairments(phase=0.5, cfo=(-0.01, 0.01), shift_max=3, snr_db=10)
    assert a.phase == (0.5, 0.5) and a.cfo == (-0.01, 0.01) and a.snr_db == (10.0, 10.0) and a.gain_db is None
    s = a.struct(seed=7, step=2, frame_base=5)
    assert (s.phase_lo, s.phase_hi) == (0.5, 0.5) and s.shift_max == 3 and (s.seed, s.step, s.frame_base) == (7, 2, 5)
    assert (s.gain_db_lo, s.gain_db_hi) == (0.0, 0.0) and s.snr_db_lo == 10.0 and s.rot90 == 0 and s.conj == 0
    s0 = Impairments().struct()
    assert math.isnan(s0.snr_db_lo) and math.isnan(s0.snr_db_hi) and s0.phase_lo == 0.0 and s0.shift_max == 0
    aug = Impairments.augmentation()
    assert aug.phase == (-math.pi, math.pi) and aug.rot90 and aug.conj and aug.shift_max == 1023
    assert aug.gain_db == (-1.0, 1.0) and aug.snr_db is None and aug.cfo is None
    assert Impairments.augmentation(128).shift_max == 127
    bad = [
        (ValueError, dict(phase=(1.0, 0.0)), "1.0"),
        (ValueError, dict(snr_db=(5.0, -5.0)), "5.0"),
        (ValueError, dict(cfo=float("nan")), "nan"),
        (ValueError, dict(gain_db=(0.0, float("nan"))), "nan"),
        (ValueError, dict(phase=float("inf")), "inf"),
        (ValueError, dict(phase=(0.0, 1.0, 2.0)), "2.0"),
        (TypeError, dict(phase=True), "True"),
        (TypeError, dict(snr_db=(False, 3.0)), "False"),
        (TypeError, dict(gain_db="3"), "'3'"),
        (TypeError, dict(rot90=2), "2"),
        (TypeError, dict(conj="yes"), "yes"),
        (ValueError, dict(shift_max=-1), "-1"),
        (TypeError, dict(shift_max=1.5), "1.5"),
        (TypeError, dict(shift_max=True), "True"),
    ]
    for exc, kw, shown in bad:
        with pytest.raises(exc) as e:
            Impairments(**kw)
        assert shown in str(e.value), (kw, str(e.value))
    for kw in (dict(seed=-1), dict(step=2 ** 32), dict(frame_base=-3)):
        with pytest.raises(ValueError):
            Impairments().struct(**kw)


def test_impair_and_curve_argument_errors_are_raised_before_any_device_work():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import Impairments, impair, impairment_curve
    m = P.AMCTransformerRawIQ(in_channels=2, seq_length=64, num_classes=4, d_model=64, n_head=4, n_layers=1, ffn_hidden=128,
                              drop_prob=0.0, device="cpu", use_cls_token=True, embedding_type="segment", segment_size=16)
    raw = torch.randn(4, 64, 2)
    y = torch.tensor([0, 1, 2, 3])
    st = ((0.0, 0.0), (1.0, 1.0))
    bad = [
        (ValueError, impairment_curve, (m, raw, y, st, "doppler", [0.0]), {}),                    # unknown kind
        (TypeError, impairment_curve, (m, raw, y, st, "phase", [True]), {}),
        (ValueError, impairment_curve, (m, raw, y, st, "snr_db", [float("nan")]), {}),
        (TypeError, impairment_curve, (m, raw, y, st, "shift", [1.5]), {}),
        (ValueError, impairment_curve, (m, raw, y, st, "shift", [64]), {}),                       # not below the frame length
        (ValueError, impairment_curve, (m, raw, y, st, "phase", [0.0]), dict(layout="vit")),
        (ValueError, impairment_curve, (m, raw, y, st, "phase", [0.0]), dict(batch=0)),
        (TypeError, impairment_curve, (m, raw, y, st, "phase", [0.0]), dict(base=0.1)),
        (ValueError, impairment_curve, (m, raw, torch.tensor([0, 1, 2, 4]), st, "phase", [0.0]), {}),
        (ValueError, impairment_curve, (m, raw[:, :, 0], y, st, "phase", [0.0]), {}),
        (TypeError, impairment_curve, (torch.nn.Linear(2, 2), raw, y, st, "phase", [0.0]), {}),
        (TypeError, impair, (raw, st, "rawiq", None), {}),
        (ValueError, impair, (raw, st, "image", Impairments()), {}),
        (ValueError, impair, (raw, st, "vit", Impairments()), {}),                                # 32x64 image from 64 samples
        (ValueError, impair, (raw, st, "rawiq", Impairments(shift_max=64)), {}),
        (ValueError, impair, (raw, ((0.0, 0.0), (1.0, 0.0)), "rawiq", Impairments()), {}),        # std 0
        (TypeError, impair, (raw, 3.0, "rawiq", Impairments()), {}),
    ]
    for exc, fn, args, kw in bad:
        with pytest.raises(exc):
            fn(*args, **kw)
    for fn, args in ((impair, (raw, st, "rawiq", Impairments())), (impairment_curve, (m, raw, y, st, "phase", [0.0]))):
        with pytest.raises(P.IqError):                                                            # a CPU tensor: no CPU path
            fn(*args)
    assert m._plan is None and m.training


def test_reference_with_an_identity_row_is_the_preprocessing():
    """impair_reference is fp64, data.preprocess_reference fp32: the fp32 path rounds twice (subtract, divide), each within
    2^-24 relative of the result, so the two agree to 2 * 2^-24 = 1.2e-7 relative (2.5e-7 allowed for the product of both)."""
    from vit_vs_raw_iq_amd import data as D, impair_reference
    X = frames()
    mean, std = D.zscore_stats(X)
    stats = {"i_mean": float(mean[0]), "i_std": float(std[0]), "q_mean": float(mean[1]), "q_std": float(std[1])}
    d = drawn_rows(len(X))
    for layout, h, w, shape in (("rawiq", 32, 64, (8, 2, 1024)), ("vit", 32, 64, (8, 1, 32, 64)), ("vit", 32, 32, (8, 1, 32, 32))):
        ref = D.preprocess_reference(X, stats, layout, h, w)
        got = impair_reference(X, d, stats, layout, h, w)
        assert got.shape == shape == ref.shape and got.dtype == np.float64
        np.testing.assert_allclose(got, ref.astype(np.float64), rtol=2.5e-7, atol=0)
        assert np.array_equal(impair_reference(X, d, (mean, std), layout, h, w), got)              # both forms of stats


def power(z):
    """Sum of squares per frame, of (B, len, 2) raw frames or of the (B, 2, len) layout."""
    return (np.asarray(z, np.float64) ** 2).sum(axis=(1, 2))


def test_rotation_and_conjugation_keep_the_power_of_every_frame():
    from vit_vs_raw_iq_amd import impair_reference
    X = frames()
    p0 = power(X)
    rng = np.random.default_rng(0)
    d = drawn_rows(len(X), theta=rng.uniform(-np.pi, np.pi, len(X)), f=rng.uniform(-0.01, 0.01, len(X)),
                   k=rng.integers(0, 4, len(X)), conj=rng.integers(0, 2, len(X)), s=rng.integers(0, 1024, len(X)))
    assert d[:, 3].any() and not d[:, 3].all()
    p1 = power(impair_reference(X, d, IDENT_STATS, "rawiq"))
    np.testing.assert_allclose(p1, p0, rtol=1e-12)
    d[:, 5] = 2.0                                                  # and a gain of 2 is 4x the power
    np.testing.assert_allclose(power(impair_reference(X, d, IDENT_STATS, "rawiq")), 4 * p0, rtol=1e-12)
    # conjugation alone: I kept, Q negated, exactly
    c = impair_reference(X, drawn_rows(len(X), conj=1), IDENT_STATS, "rawiq")
    assert np.array_equal(c[:, 0], X[:, :, 0].astype(np.float64)) and np.array_equal(c[:, 1], -X[:, :, 1].astype(np.float64))
    # the order: conjugate BEFORE the rotation, rotation index = OUTPUT sample index (after the shift)
    one = impair_reference(X[:1], drawn_rows(1, theta=0.3, f=0.002, conj=1, s=5, g=1.5), IDENT_STATS, "rawiq")[0]
    z = np.roll(X[0, :, 0].astype(np.float64) + 1j * X[0, :, 1], -5).conj() * np.exp(1j * (0.3 + 2 * np.pi * 0.002 * np.arange(1024))) * 1.5
    np.testing.assert_allclose(one[0] + 1j * one[1], z, rtol=0, atol=1e-12)


def test_two_quarter_turns_are_a_phase_of_pi():
    from vit_vs_raw_iq_amd import impair_reference
    X = frames()
    a = impair_reference(X, drawn_rows(len(X), k=2), IDENT_STATS, "rawiq")
    b = impair_reference(X, drawn_rows(len(X), theta=np.pi), IDENT_STATS, "rawiq")
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * np.abs(X).max())
    np.testing.assert_allclose(a, -np.transpose(X, (0, 2, 1)).astype(np.float64), rtol=0, atol=1e-12 * np.abs(X).max())


def test_a_shift_and_its_complement_are_the_identity():
    from vit_vs_raw_iq_amd import impair_reference
    X = frames()
    for s in (1, 37, 512, 1023):
        once = impair_reference(X, drawn_rows(len(X), s=s), IDENT_STATS, "rawiq")
        assert np.array_equal(once[:, :, 0], X[:, s, :].astype(np.float64))                       # out[0] = in[s]
        back = impair_reference(np.transpose(once, (0, 2, 1)), drawn_rows(len(X), s=1024 - s), IDENT_STATS, "rawiq")
        assert np.array_equal(back, np.transpose(X, (0, 2, 1)).astype(np.float64))


def test_impair_struct_matches_the_header_and_the_symbol_is_exported():
    import vit_vs_raw_iq_amd._native as N
    src = open(HEADER).read()
    body = re.search(r"typedef struct iq_impair \{(.*?)\}", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in N.Impair._fields_]
    assert ctypes.sizeof(N.Impair) == 72 and N.Impair.seed.offset == 48 and N.Impair.frame_base.offset == 64
    decl = re.search(r"\biq_frames_impair\(([^)]*)\)", re.sub(r"/\*.*?\*/", "", src, flags=re.S)).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["iq_frames_impair"][1]) == 9
    assert re.search(r"#define IQ_SITE_IMPAIR 0xFFFFFFFFu", src)
    assert N.lib().iq_frames_impair is not None


def test_frames_impair_refuses_bad_arguments_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import Impairments
    L = N.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(buf) + 15) // 16 * 16          # aligned host address: never dereferenced on these paths
    st = (ctypes.c_float * 4)(0.0, 1.0, 0.0, 1.0)
    ok = Impairments().struct()
    ARG, UNSUPPORTED = 1, 2

    def call(imp=ok, raw=a, out=a, stats=st, n=2, length=64, take=64):
        return L.iq_frames_impair(raw, out, None, n, length, take, stats, ctypes.byref(imp) if imp is not None else None, None)
    assert call(raw=None) == ARG and call(out=None) == ARG and call(stats=None) == ARG and call(imp=None) == ARG
    assert call(take=65) == ARG and call(length=0, take=0) == ARG
    assert call(stats=(ctypes.c_float * 4)(0.0, 0.0, 0.0, 1.0)) == ARG
    nan, inf = float("nan"), float("inf")
    for field, lo, hi in (("phase", 1.0, 0.0), ("cfo", 0.1, -0.1), ("gain_db", 3.0, -3.0), ("snr_db", 10.0, 0.0),
                          ("phase", nan, 0.0), ("cfo", 0.0, nan), ("gain_db", nan, nan), ("snr_db", nan, 0.0),
                          ("snr_db", 0.0, nan), ("phase", 0.0, inf), ("cfo", -inf, 0.0), ("gain_db", 0.0, inf),
                          ("snr_db", 0.0, inf), ("snr_db", -inf, inf)):
        s = Impairments().struct()
        setattr(s, field + "_lo", lo)
        setattr(s, field + "_hi", hi)
        assert call(imp=s) == ARG, (field, lo, hi)
    for field, v in (("shift_max", -1), ("shift_max", 64), ("rot90", 2), ("conj", -1)):
        s = Impairments().struct()
        setattr(s, field, v)
        assert call(imp=s) == ARG, (field, v)
    assert call(length=8193, take=8193) == UNSUPPORTED                # 8 bytes per sample above 64 KB of LDS
    assert call(n=0) == 0                                              # no frames: nothing to do
