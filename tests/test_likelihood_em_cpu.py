"""Host only: the hybrid likelihood classifier's fp64 definition (vit_vs_raw_iq_amd.likelihood_em.likelihood_em_reference) one step
at a time against the direct statement on numpy.logaddexp and its maximiser (tests/likelihood_em_ref.py), what the EM is for (a
noiseless frame, the truth up to the class's symmetry, the blind SNR estimate), the ctypes binding against include/iqvit.h, every
refusal of iq_frames_likelihood_em that returns before a HIP call, the argument checks of HybridLikelihoodClassifier, and the
inputs of the GPU suite against what its exact cases, its one-pass bound, its allowance and its decision set assume."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import likelihood_em_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables(names, length=16, **kw):
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier
    clf = HybridLikelihoodClassifier(length, classes=names, **kw)
    return clf, clf.points, [d[1:] for d in clf.descriptors]


def symmetric_distance(h, truth, order):
    """|h - truth e^{j 2 pi m / order}| at the nearest image under the class's rotational symmetry."""
    return np.min(np.abs(h - truth * np.exp(2j * np.pi * np.arange(order) / order)))


def test_one_step_at_a_time_is_the_direct_statement():
    """Three classes, three frames, a given start, both layouts: Lambda at the start is the plain logaddexp sum, the state after
    one update is the weighted least-squares gain and the weighted distance at the old gain, and so on for three steps."""
    from vit_vs_raw_iq_amd import likelihood_em_reference
    clf, points, classes = tables(["BPSK", "8PSK", "16QAM"])
    pc = points[:, 0].astype(np.float64) + 1j * points[:, 1]
    x, _ = E.real_frames(3, 16, "8PSK", 10.0, 1, gain=1.4)
    y = E.to_complex(x)
    h0, v0 = E.given_start(x, points, classes, 2)
    for planar in (False, True):
        h, v = h0.astype(np.float64) @ np.array([1, 1j]), v0.astype(np.float64)
        for iters in range(4):
            r = likelihood_em_reference(E.in_layout(x, planar), points, classes, None, iters, 0.02, 0.0, h0=h0, v0=v0, planar=planar, trace=True)
            assert r.loglik.shape == (3, 3) and r.start_ll.shape == (3, 3, 1) and r.trace.shape == (iters + 1, 3, 3, 1)
            for b in range(3):
                for c, (off, M) in enumerate(classes):
                    assert np.isclose(r.h[b, c], h[b, c], rtol=1e-11) and np.isclose(r.v[b, c], v[b, c], rtol=1e-11)
                    assert np.isclose(r.loglik[b, c], E.loglik_plain(y[b], pc[off:off + M], h[b, c], v[b, c]), rtol=1e-11)
            assert np.array_equal(r.trace[-1], r.start_ll) and not r.best_start.any() and np.array_equal(r.pred, np.argmax(r.loglik, axis=1))
            assert np.allclose(r.snr_db, 10 * np.log10(np.abs(r.h[np.arange(3), r.pred]) ** 2 / r.v[np.arange(3), r.pred]), rtol=1e-12)
            for b in range(3):                           # one more step, stated directly
                for c, (off, M) in enumerate(classes):
                    h[b, c], v[b, c] = E.update_plain(y[b], pc[off:off + M], h[b, c], v[b, c])
    # the helper that carries the bound says the same, with bounds that are positive and small
    both = E.reference_and_bound(x, points, classes, None, 3, 0.02, 0.0, h0, v0)
    assert np.allclose(both["loglik"], r.loglik, rtol=1e-12) and np.allclose(both["h"], r.h, rtol=1e-12) and np.allclose(both["v"], r.v, rtol=1e-12)
    assert np.all(both["Ell"] > 0) and np.all(both["Ehb"] > 0) and np.all(both["Evb"] > 0)
    assert np.all(both["Ell"] < 1e-4 * np.abs(r.loglik)) and np.all(both["Ehb"] < 1e-4 * np.abs(r.h)) and np.all(both["Evb"] < 1e-4 * r.v)


def test_lambda_never_decreases_and_ends_at_a_maximum():
    """Real frames of four classes from the table's starts: every step of every start raises Lambda (the ECM property), and the
    state of a frame's own class after 200 steps is a local maximum of the direct statement in h and in v."""
    from vit_vs_raw_iq_amd import likelihood_em_reference
    clf, points, classes = tables(["QPSK", "8PSK", "16QAM", "16APSK"], starts=8)
    x = np.concatenate([E.real_frames(2, 16, n, snr, 3 + i, gain=g)[0] for i, (n, snr, g) in
                        enumerate((("QPSK", 6.0, 0.5), ("16QAM", 15.0, 2.0), ("16APSK", 0.0, 1.0)))])
    r = likelihood_em_reference(x, points, classes, clf.starts, 40, 0.02, 1e-6, trace=True)
    step = np.diff(r.trace, axis=0)
    assert np.all(step >= -1e-9 * np.abs(r.trace[1:])) and np.any(step > 1.0)
    r = likelihood_em_reference(x, points, classes, clf.starts, 200, 0.02, 1e-6)
    pc = points[:, 0].astype(np.float64) + 1j * points[:, 1]
    y = E.to_complex(x)
    for b, c in ((0, 0), (1, 0), (2, 2), (3, 2)):          # a frame's own class: there 200 steps have converged (a wrong class at
        off, M = classes[c]                               # 0 dB is still creeping along a flat ridge)
        h, v, top = r.h[b, c], r.v[b, c], r.loglik[b, c]
        for dh, dv in ((1e-3, 0), (-1e-3, 0), (1e-3j, 0), (-1e-3j, 0), (0, 1e-3), (0, -1e-3)):
            assert E.loglik_plain(y[b], pc[off:off + M], h * (1 + dh), v * (1 + dv)) <= top + 1e-9 * abs(top), (b, c, dh, dv)


def test_a_noiseless_frame_returns_its_gain_and_the_floor():
    from vit_vs_raw_iq_amd import likelihood_em_reference
    clf, points, classes = tables(["QPSK", "16QAM", "32APSK"], length=64)
    k = 1
    off, M = classes[k]
    rng = np.random.default_rng(0)
    truth = 1.7 * np.exp(0.4j)
    s = points[off + rng.integers(0, M, 64)].astype(np.float64) @ np.array([1, 1j])
    x = E.from_complex((truth * s)[None], dtype=np.float64)
    r = likelihood_em_reference(x, points, classes, clf.starts, 32, 0.02, 1e-6)
    assert r.pred[0] == k and symmetric_distance(r.h[0, k], truth, 4) < 1e-9 * abs(truth)
    assert r.v[0, k] == 1e-6 * np.mean((truth * s).real ** 2 + (truth * s).imag ** 2)        # the floor, exactly
    assert abs(r.snr_db[0] - 10 * np.log10(abs(truth) ** 2 / r.v[0, k])) < 1e-9


def test_the_chosen_gain_is_the_truth_up_to_the_classes_symmetry():
    """20 dB, 128 symbols, a random gain and phase per frame: the winning start's h lies at an image of the truth under the class's
    symmetry (BPSK 2, QPSK 4, 8PSK 8, 16QAM 4) within five standard deviations of the least-squares gain, sqrt(v / len)."""
    from vit_vs_raw_iq_amd import likelihood_em_reference
    clf, points, classes = tables(["BPSK", "QPSK", "8PSK", "16QAM"], length=128)
    rng = np.random.default_rng(5)
    for c, (name, order) in enumerate((("BPSK", 2), ("QPSK", 4), ("8PSK", 8), ("16QAM", 4))):
        pts = points[classes[c][0]:classes[c][0] + classes[c][1]].astype(np.float64) @ np.array([1, 1j])
        truth = rng.uniform(0.3, 3.0, 3) * np.exp(2j * np.pi * rng.uniform(0, 1, 3))
        y = truth[:, None] * pts[rng.integers(0, len(pts), (3, 128))]
        y = y + np.abs(truth)[:, None] * np.sqrt(0.01 / 2) * (rng.standard_normal((3, 128)) + 1j * rng.standard_normal((3, 128)))
        r = likelihood_em_reference(E.from_complex(y), points, classes, clf.starts, 32, E.F0, E.FLOOR)
        assert np.all(r.pred == c), name
        for b in range(3):
            assert symmetric_distance(r.h[b, c], truth[b], order) < 5.0 * abs(truth[b]) * np.sqrt(0.01 / 128), (name, b)


def test_the_blind_snr_estimate():
    """Six frames each of four classes, 128 symbols, gain 1.7.  What the host definition achieves, with the margin beside it:
    20 dB: median 19.97, every frame within [19.15, 20.72]  -> median within 0.25 dB, every frame within 1.5 dB
     8 dB: median  8.17, every frame within [6.76, 9.16]    -> median within 0.5 dB, every frame within 2.5 dB
     0 dB: the decision is mostly wrong there (0.29 correct) and the estimate of the TRUE class is what means something:
           median 0.52, within [-1.94, 3.73]                -> median within 1.5 dB"""
    from vit_vs_raw_iq_amd import likelihood_em_reference
    clf, points, classes = tables(["BPSK", "QPSK", "8PSK", "16QAM"], length=128)
    for snr, med, each in ((20.0, 0.25, 1.5), (8.0, 0.5, 2.5), (0.0, 1.5, None)):
        x = np.concatenate([E.real_frames(6, 128, name, snr, 100 + i + int(snr), gain=1.7)[0] for i, name in enumerate(clf.class_names)])
        y = np.repeat(np.arange(4), 6)
        r = likelihood_em_reference(x, points, classes, clf.starts, 32, E.F0, E.FLOOR)
        own = 10 * np.log10(np.abs(r.h[np.arange(24), y]) ** 2 / r.v[np.arange(24), y])
        print(f"{snr:4.0f} dB: correct {(r.pred == y).mean():.2f}, estimate of the true class: median {np.median(own):.2f}, "
              f"[{own.min():.2f}, {own.max():.2f}]")
        assert abs(np.median(own) - snr) < med
        if each is not None:
            assert np.all(r.pred == y) and np.array_equal(r.snr_db, own) and np.all(np.abs(own - snr) < each)


def test_dead_states_are_nan_and_pred_passes_them_over():
    from vit_vs_raw_iq_amd import likelihood_em_reference
    pts = np.array([0, 1, -1, 1j, -1j])
    classes = [(0, 1), (1, 2), (1, 4)]
    x = E.real_frames(3, 32, "BPSK", 12.0, 7)[0]
    x[1] = 0.0                                            # M2 = 0: no start
    x[2, 5, 0] = np.nan
    st = np.array([0.0, 1.0, 2.0])
    r = likelihood_em_reference(x, pts, classes, st, 3, 0.02, 1e-6)
    assert np.isnan(r.loglik[0, 0]) and r.best_start[0, 0] == -1 and np.isnan(r.h[0, 0]) and np.isnan(r.v[0, 0])     # Bq = 0
    assert np.isfinite(r.loglik[0, 1:]).all() and r.pred[0] == 1 and np.isfinite(r.snr_db[0])
    for b in (1, 2):
        assert np.isnan(r.loglik[b]).all() and np.all(r.best_start[b] == -1) and r.pred[b] == -1 and np.isnan(r.snr_db[b])
        assert np.isnan(r.start_ll[b]).all()
    r0 = likelihood_em_reference(x[:1], pts, classes, st, 0, 0.02, 1e-6)                       # no update: the origin is a class
    assert np.isfinite(r0.loglik).all()
    lam = np.array([[np.nan, 1.0, 3.0, 3.0], [np.nan] * 4, [-np.inf, np.nan, -np.inf, np.nan]])
    at, top = E.first_valid_largest(lam, 1)
    assert np.array_equal(at, [2, -1, 0]) and np.array_equal(top, [3.0, np.nan, -np.inf], equal_nan=True)
    from vit_vs_raw_iq_amd.likelihood_em import _first_valid_largest
    at2, top2 = _first_valid_largest(lam, 1)
    assert np.array_equal(at2, at) and np.array_equal(top2, top, equal_nan=True)


def test_binding_struct_matches_the_header():
    import vit_vs_raw_iq_amd._native as N
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iqvit.h")).read(), flags=re.S)
    body = re.search(r"typedef struct iq_likelihood_em \{(.*?)\}", src, flags=re.S).group(1)
    names = [w for d in body.split(";") if d.strip() for w in re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", d.strip())]
    want = ["points", "classes", "n_classes", "starts", "n_starts", "iters", "planar", "mode", "f0", "floor", "h0", "v0"]
    assert names == [f[0] for f in N.LikelihoodEm._fields_] == want
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert [f[1] for f in N.LikelihoodEm._fields_] == [P, ctypes.POINTER(N.SynthClass), I, P, I, I, I, I, F, F, P, P]
    assert ctypes.sizeof(N.LikelihoodEm) == 72
    assert [getattr(N.LikelihoodEm, f).offset for f in names] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56, 64]
    enum = re.search(r"enum \{ IQ_EM_TABLE = (\d), IQ_EM_GIVEN = (\d) \}", src)
    assert [int(v) for v in enum.groups()] == [0, 1]
    decl = re.search(r"int iq_frames_likelihood_em\((.*?)\);", src, flags=re.S).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["iq_frames_likelihood_em"][1]) == 12
    assert hasattr(N.lib(), "iq_frames_likelihood_em")                           # the symbol is exported
    from vit_vs_raw_iq_amd.likelihood_em import MAX_ITERS, MAX_STARTS, MODES
    assert (MAX_STARTS, MAX_ITERS, MODES) == (256, 4096, ("table", "given"))


def test_every_refusal_returns_before_a_hip_call():
    """Pointers that are never dereferenced: a refusal looks at their value only (the class list is host memory and is read)."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    ARG, UNSUPPORTED = 1, 2
    A = 0x10000                                            # "an aligned pointer"
    OUT = ("loglik", "h", "v", "best_start", "start_ll", "pred", "snr_db")

    def call(x=A, n=1, length=512, par="ok", classes=((0, 0, 16), (0, 16, 4)), n_classes=None, **kw):
        outs = {k: kw.pop(k, A) for k in OUT}
        arr = None if classes is None else (N.SynthClass * max(1, len(classes)))(*[N.SynthClass(*c) for c in classes])
        ok = dict(points=A, classes=arr, n_classes=len(classes or ()) if n_classes is None else n_classes, starts=A, n_starts=16, iters=32,
                  planar=0, mode=0, f0=0.02, floor=1e-6, h0=None, v0=None)
        p = None if par is None else N.LikelihoodEm(**{**ok, **kw})
        return L.iq_frames_likelihood_em(x, *(outs[k] for k in OUT), n, length, ctypes.byref(p) if p is not None else None, None)
    # (a valid call with n = 1 would launch: none is made here)
    assert call(x=None) == ARG and call(loglik=None) == ARG and call(par=None) == ARG
    assert call(points=None) == ARG and call(classes=None, n_classes=2) == ARG
    assert call(mode=2) == ARG and call(mode=-1) == ARG
    assert call(starts=None) == ARG and call(n_starts=0) == ARG and call(n_starts=-3) == ARG
    assert call(mode=1) == ARG and call(mode=1, h0=A) == ARG and call(mode=1, v0=A) == ARG
    assert call(h=None) == ARG and call(v=None) == ARG and call(h=None, v=None, snr_db=None, n=0) == 0       # snr_db reads h and v
    assert call(length=0) == ARG and call(length=-4) == ARG and call(n_classes=0) == ARG and call(n_classes=-1) == ARG
    assert call(iters=-1) == ARG and call(planar=2) == ARG and call(planar=-1) == ARG
    for f0 in (0.0, 1.0, 1.5, -0.1, float("nan"), float("inf")):
        assert call(f0=f0) == ARG, f0
    for floor in (-1e-9, float("nan"), float("inf")):
        assert call(floor=floor) == ARG, floor
    assert call(floor=0.0, n=0) == 0
    # alignment: interleaved frames, the points, h0 and h 8 bytes, planar frames and everything else 4
    assert call(x=A + 4) == ARG and call(x=A + 2, planar=1) == ARG and call(points=A + 4) == ARG and call(h=A + 4) == ARG
    assert call(mode=1, h0=A + 4, v0=A) == ARG and call(mode=1, h0=A, v0=A + 2) == ARG and call(mode=1, h0=A, v0=A, n=0) == 0
    for name in ("loglik", "v", "best_start", "start_ll", "pred", "snr_db", "starts"):
        assert call(**{name: A + 2}) == ARG, name
    # the class list
    assert call(classes=((1, 0, 4),)) == ARG and call(classes=((2, 0, 4),)) == ARG and call(classes=((0, 0, 4), (-1, 4, 4))) == ARG
    assert call(classes=((0, 0, 0),)) == ARG and call(classes=((0, 0, -3),)) == ARG and call(classes=((0, -1, 4),)) == ARG
    assert call(classes=((0, 2 ** 31 - 2, 4),)) == ARG                                        # offset + count past the int range
    # the limits
    many = tuple((0, i, 1) for i in range(65))
    assert call(classes=many) == UNSUPPORTED and call(classes=many[:64], n=0) == 0
    assert call(n_starts=257) == UNSUPPORTED and call(n_starts=256, n=0) == 0
    assert call(mode=1, h0=A, v0=A, n_starts=257, starts=None, n=0) == 0                      # a given start: the table is not looked at
    assert call(iters=4097) == UNSUPPORTED and call(iters=4096, n=0) == 0 and call(iters=0, n=0) == 0
    assert call(classes=((0, 0, 2049),)) == UNSUPPORTED and call(classes=((0, 2040, 9),)) == UNSUPPORTED
    assert call(classes=((0, 0, 2048),), n=0) == 0 and call(classes=((0, 2047, 1), (0, 0, 2)), n=0) == 0
    assert call(length=8193) == UNSUPPORTED and call(length=8192, n=0) == 0
    assert call(n_starts=257, mode=5) == ARG and call(length=8193, classes=((1, 0, 4),)) == ARG       # ARG comes first
    # n_frames <= 0 is success, nothing launched; the optional pointers may be NULL
    for n in (0, -3):
        assert call(n=n) == 0 and call(n=n, h=None, v=None, best_start=None, start_ll=None, pred=None, snr_db=None, planar=1) == 0


def test_python_argument_checks():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier, LikelihoodClassifier, likelihood_em_reference
    from vit_vs_raw_iq_amd.evaluation import evaluate_hybrid_with_confusion
    for kw, exc in ((dict(length=0), ValueError), (dict(length=8193), ValueError), (dict(length=8.0), TypeError),
                    (dict(length=64, classes=[]), ValueError), (dict(length=64, classes="QPSK"), TypeError),
                    (dict(length=64, classes=["QPSK", "QPSK"]), ValueError), (dict(length=64, classes=["GMSK"]), ValueError),
                    (dict(length=64, classes=[("a", [0, 0])]), ValueError), (dict(length=64, classes=[("a", np.ones(2049))]), ValueError),
                    (dict(length=64, starts=0), ValueError), (dict(length=64, starts=257), ValueError),
                    (dict(length=64, starts=16.0), TypeError), (dict(length=64, starts=True), TypeError),
                    (dict(length=64, starts=[]), ValueError), (dict(length=64, starts=[0.0, np.inf]), ValueError),
                    (dict(length=64, starts="many"), TypeError),
                    (dict(length=64, iters=-1), ValueError), (dict(length=64, iters=4097), ValueError), (dict(length=64, iters=8.0), TypeError),
                    (dict(length=64, init_noise=0.0), ValueError), (dict(length=64, init_noise=1.0), ValueError),
                    (dict(length=64, init_noise=1e-60), ValueError), (dict(length=64, init_noise="x"), TypeError),
                    (dict(length=64, floor=-1e-6), ValueError), (dict(length=64, floor=np.nan), ValueError), (dict(length=64, floor=None), TypeError),
                    (dict(length=64, layout="interleaved"), ValueError), (dict(length=64, device="cpu"), TypeError)):
        with pytest.raises(exc):
            HybridLikelihoodClassifier(**kw)
    with pytest.raises(ValueError, match="starts"):
        HybridLikelihoodClassifier(64, starts=300)
    clf = HybridLikelihoodClassifier(500)
    lik = LikelihoodClassifier(500)
    assert clf.class_names == lik.class_names and clf.descriptors == lik.descriptors and np.array_equal(clf.points, lik.points)
    assert (clf.n_classes, clf.n_starts, clf.iters, clf.init_noise, clf.floor, clf.layout, clf.planar) == (17, 16, 32, 0.02, 1e-6, "frames", 0)
    assert np.allclose(clf.angles, 2 * np.pi * np.arange(16) / 16) and clf.starts.dtype == np.float32 and clf.starts.shape == (16, 2)
    assert np.array_equal(clf.starts, np.stack([np.cos(clf.angles), np.sin(clf.angles)], axis=1).astype(np.float32))
    assert clf.frame_shape(3) == (3, 500, 2) and HybridLikelihoodClassifier(500, layout="planar").frame_shape(3) == (3, 2, 500)
    own = HybridLikelihoodClassifier(8, classes={"two": [1, -1]}, starts=[0.0, 0.1], iters=0, init_noise=0.5, floor=0)
    assert own.descriptors == [(0, 0, 2)] and own.n_starts == 2 and "iters=0" in repr(own)
    par = own.struct()
    assert (par.n_classes, par.n_starts, par.iters, par.mode, par.planar) == (1, 2, 0, 0, 0) and par.f0 == 0.5 and par.floor == 0.0
    assert own.struct(h0=64, v0=64).mode == 1
    # calls: the checks come before any device work, and a CPU tensor has no path
    x = torch.zeros(2, 500, 2)
    for kw, exc in ((dict(h0=torch.zeros(2, 17, 2)), ValueError), (dict(v0=torch.ones(2, 17)), ValueError),
                    (dict(h0=torch.zeros(2, 16, 2), v0=torch.ones(2, 17)), ValueError), (dict(h0=torch.zeros(2, 17, 2), v0=torch.ones(2, 16)), ValueError),
                    (dict(h0=torch.zeros(2, 17, 2, dtype=torch.int32), v0=torch.ones(2, 17)), TypeError),
                    (dict(h0=torch.zeros(2, 17, 2), v0="x"), TypeError), (dict(return_estimates=2), TypeError),
                    (dict(return_starts="yes"), TypeError)):
        with pytest.raises(exc):
            clf(x, **kw)
    for bad in (torch.zeros(2, 2, 500), torch.zeros(2, 499, 2), torch.zeros(500, 2), np.zeros((2, 500, 2))):
        with pytest.raises(ValueError):
            clf(bad)
    for call in (clf, clf.predict, clf.estimate):
        with pytest.raises(P.IqError, match="no CPU fallback"):
            call(x)
    with pytest.raises(P.IqError, match="likelihood_em_reference"):
        clf(x, h0=torch.zeros(2, 17, dtype=torch.complex64), v0=1.0)                           # complex h0, one v0 for all: accepted
    with pytest.raises(ValueError):
        evaluate_hybrid_with_confusion(clf, [], "cpu", ["a", "b"], "/nonexistent")
    args = dict(x=np.zeros((1, 4, 2)), points=clf.points, classes=[(0, 2)], starts=clf.angles)
    for kw in (dict(classes=[(0, 900)]), dict(classes=[(1, 0, 4)]), dict(classes=[(0, 0)]), dict(iters=-1), dict(h0=np.ones((1, 1, 2))),
               dict(x=np.zeros((1, 4, 3)))):
        with pytest.raises(ValueError):
            likelihood_em_reference(**{**args, **kw})


# ---- the inputs of the GPU suite
def test_exact_cases_are_exact_in_fp32():
    """What the bit-for-bit GPU test assumes: on the integer cases (h, v) of the definition are fp32 numbers after 0, 1 and 2
    updates, they do move, L at the start is a whole number of sixteenths below 2^24 of them, and the header's rounding of Lambda
    differs from the definition's Lambda by no more than the rounding of its logarithm."""
    from vit_vs_raw_iq_amd import likelihood_em_reference
    assert all(np.all(E.EXACT_POINTS[o:o + m] == E.EXACT_POINTS[o]) and m & (m - 1) == 0 for o, m in E.EXACT_CLASSES)
    assert [float((E.EXACT_POINTS[o] ** 2).sum()) for o, _ in E.EXACT_CLASSES] == [1.0, 2.0, 1.0, 0.0]
    fits = lambda a: np.array_equal(E.f32(a), a, equal_nan=True)                              # noqa: E731
    for length in E.EXACT_LENGTHS:
        x, h0, v0 = E.exact_case(3, length, length)
        assert np.array_equal(np.log2(v0), np.round(np.log2(v0))) and np.array_equal(x, np.round(x)) and np.abs(x).max() <= 4
        states = []
        for iters in (0, 1, 2):
            r = likelihood_em_reference(x, E.EXACT_POINTS, E.EXACT_CLASSES, None, iters, 0.5, 0.0, h0=h0, v0=v0)
            assert fits(r.h.real) and fits(r.h.imag) and fits(r.v), (length, iters)
            assert np.isfinite(r.loglik[:, :3]).all() and np.isnan(r.loglik[:, 3]).all() == (iters > 0)
            states.append((r.h[:, :3], r.v[:, :3]))
        assert np.all(states[1][1] != states[0][1]) and np.any(states[2][1] != states[1][1]) and np.all(states[1][0] != states[0][0])
        assert np.array_equal(states[2][0], states[1][0])                # (one point: the responsibilities, and so h, are settled at once)
        L = E.exact_L(x, h0, v0)
        assert np.array_equal(L * 16, np.round(L * 16)) and np.abs(L).max() * 16 < 2 ** 24
        r = likelihood_em_reference(x, E.EXACT_POINTS, E.EXACT_CLASSES, None, 0, 0.5, 0.0, h0=h0, v0=v0)
        want = E.lambda_as_the_header_rounds_it(L, v0.astype(np.float64), length)
        assert np.array_equal(E.f32(want), want) and np.all(np.abs(want - r.loglik) <= 4 * E.U * (np.abs(r.loglik) + length * 8.0))
    for length in E.EXACT_EDGES:
        x, h0, v0 = E.exact_case(3, length, length, tiled=False)
        L = E.exact_L(x, h0, v0)
        assert np.array_equal(L * 16, np.round(L * 16)) and np.abs(L).max() * 16 < 2 ** 24


def test_the_bound_follows_the_definition_on_the_gpu_cases():
    """reference_and_bound restates the definition to carry the bound: on every bounded case of the GPU suite it gives the
    package's numbers, its bounds are positive, far below what they bound and, for Lambda, larger where the state is inexact."""
    from vit_vs_raw_iq_amd import likelihood_em_reference
    for name, points, classes, starts, x in E.bounded_cases():
        assert len(x) <= 4 and x.shape[1] <= 257
        for iters in (0, E.BOUNDED_ITERS):
            ref = E.reference_and_bound(x, points, classes, starts, iters, E.F0, E.FLOOR)
            r = likelihood_em_reference(x, points, classes, starts, iters, E.F0, E.FLOOR)
            assert np.allclose(ref["start_ll"], r.start_ll, rtol=1e-11) and np.array_equal(ref["best_start"], r.best_start), name
            assert np.allclose(ref["h"], r.h, rtol=1e-11) and np.allclose(ref["v"], r.v, rtol=1e-11) and np.array_equal(ref["pred"], r.pred), name
            assert np.all(ref["ELam"] > 0) and np.all(ref["Eh"] > 0) and np.all(ref["Ev"] > 0), name
            assert np.all(ref["ELam"] < 1e-3 * np.abs(ref["start_ll"])) and np.all(ref["Eh"] < 1e-3 * np.abs(ref["H"])) and np.all(ref["Ev"] < 1e-3 * ref["V"])
        h0, v0 = E.given_start(x, points, classes, 5)
        assert np.array_equal(E.f32(h0), h0) and np.all(v0 > 0)
        exact = E.reference_and_bound(x, points, classes, None, 0, E.F0, E.FLOOR, h0, v0)
        assert np.all(exact["Eh"] == 0) and np.all(exact["Ev"] == 0)                           # a given state is exact on both sides
        step = E.reference_and_bound(x, points, classes, None, 1, E.F0, E.FLOOR, h0, v0)
        assert np.all(step["Eh"] > 0) and np.all(step["ELam"] > 0) and np.any(np.abs(step["H"][..., 0] - (h0.astype(np.float64) @ np.array([1, 1j]))) > 1e-3)
    sizes = sorted({m for _, _, classes, _, _ in E.bounded_cases() for _, m in classes})
    assert {1, 2, 16, 256} <= set(sizes) and sorted(len(s) for _, _, _, s, _ in E.bounded_cases()) == [1, 4, 5, 16]


def test_the_allowance_of_several_steps_is_measured_and_pinned():
    """The fp64 definition with a perturbation of the one-pass bound's size injected after every update, eight patterns: the
    deviation of the final state (of the winning start, the one the device hands out) and of every start's Lambda, relative to
    the one-pass bounds, stays below HALF of FACTOR on every bounded case of the GPU suite."""
    worst = np.zeros(3)
    for name, points, classes, starts, x in E.bounded_cases():
        rh, rv, rl, clean = E.amplification(x, points, classes, starts, E.BOUNDED_ITERS, E.F0, E.FLOOR)
        got = np.array([np.nanmax(E.at_best(rh, clean)), np.nanmax(E.at_best(rv, clean)), np.nanmax(rl)])
        print(f"{name}: deviation / one-pass bound: h {got[0]:.1f}, v {got[1]:.1f}, Lambda {got[2]:.1f}")
        worst = np.maximum(worst, got)
    assert np.all(2.0 * worst <= E.FACTOR) and np.all(worst > 1.0)                             # (and the steps do amplify)


def test_decision_set_is_what_the_gpu_test_assumes():
    """The 28 frames at 20 dB under gains in [0.3, 3]: every class of the classifier is there, the fp64 definition classifies at
    least 0.95 of them (the issue's host runs: 0.97 of the 17-class set), at most 2 % have a best-minus-second margin below twice
    the allowance, the estimated SNR's median is within 0.25 dB of 20, and the allowance of Lambda holds with its margin of two on
    EVERY frame of the set (two patterns, 32 steps): the GPU suite allows FACTOR on every frame.  The state is not pinned here --
    a winning start near the boundary of two basins deviates far more -- and the GPU suite does not compare it on this set."""
    from vit_vs_raw_iq_amd import LikelihoodClassifier, likelihood_em_reference, likelihood_reference
    X, Y, gain = E.decision_set()
    clf = E.decision_classifier()
    assert X.shape == (28, 128, 2) and np.array_equal(np.bincount(Y), np.full(14, 2)) and clf.n_classes == 14
    assert (clf.n_starts, clf.iters, np.float32(clf.init_noise), np.float32(clf.floor)) == (16, 32, E.F0, E.FLOOR)
    assert gain.min() >= 0.3 and gain.max() <= 3.0 and gain.max() / gain.min() > 4
    args = (X, clf.points, [d[1:] for d in clf.descriptors], clf.starts, clf.iters, E.F0, E.FLOOR)
    rh, rv, rl, ref = E.amplification(*args, patterns=E.PATTERNS[:2])
    print(f"deviation / one-pass bound on all {len(X)} frames: Lambda of any start {np.nanmax(rl):.1f} (state of the winning start: "
          f"h {np.nanmax(E.at_best(rh, ref)):.1f}, v {np.nanmax(E.at_best(rv, ref)):.1f}, not asserted)")
    assert 2.0 * np.nanmax(rl) <= E.FACTOR
    ok = E.decided(ref)
    worst = E.FACTOR * np.nanmax(ref["Ell"], axis=1)
    print(f"correct {(ref['pred'] == Y).mean():.3f}, decided {ok.mean():.3f}, smallest margin {E.margin(ref['loglik']).min():.3f}, "
          f"largest allowance {worst.max():.4f}")
    assert (ref["pred"] == Y).mean() >= 0.95 and ok.mean() >= 1.0 - E.DECISION_CAP
    at = (np.arange(len(X)), ref["pred"])
    snr = 10 * np.log10(np.abs(ref["h"][at]) ** 2 / ref["v"][at])
    assert abs(np.median(snr) - E.DECISION_SNR_DB) < 0.25
    r = likelihood_em_reference(X[:2], clf.points, clf.descriptors, clf.starts, clf.iters, E.F0, E.FLOOR)
    assert np.allclose(r.start_ll, ref["start_ll"][:2], rtol=1e-11) and np.array_equal(r.pred, ref["pred"][:2])
    # starts the device may take for the maximum: the definition's own is always among them
    ties = E.start_ties(ref, E.FACTOR)
    assert np.all(np.take_along_axis(ties, ref["best_start"][..., None], axis=2))
    # what estimate() is for: LikelihoodClassifier's definition handed the hybrid's (sigma2, |h|) decides as handed the truth
    lik = LikelihoodClassifier(128, classes=clf.class_names)
    truth = likelihood_reference(X, gain ** 2 * 10.0 ** (-E.DECISION_SNR_DB / 10.0), gain, lik.points, lik.descriptors, lik.angles)
    blind = likelihood_reference(X, ref["v"][at], np.abs(ref["h"][at]), lik.points, lik.descriptors, lik.angles)
    assert np.array_equal(truth[3], Y) and np.array_equal(blind[3], truth[3])
