"""Host only: the likelihood classifier's fp64 definition (vit_vs_raw_iq_amd.likelihood.likelihood_reference) against the direct
statement on numpy.logaddexp (tests/likelihood_ref.py) and on hand-written frames, the ctypes binding against include/iqvit.h, every
refusal of iq_frames_likelihood that returns before a HIP call, the argument checks of LikelihoodClassifier, noise_for in both
conventions, and the inputs of the GPU suite against what its exact cases and its bound (derived in tests/likelihood_ref.py) assume."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import likelihood_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables(names):
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    clf = LikelihoodClassifier(16, classes=names)
    return clf, clf.points, [d[1:] for d in clf.descriptors]


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_reference_is_the_direct_statement(mode):
    """Four classes, five rotations, three frames with their own sigma2 and gain, both layouts: every L[b, c, r] is the plain
    logaddexp sum, and loglik the maximum or the log of the mean over r."""
    from vit_vs_raw_iq_amd import likelihood_reference
    clf, points, classes = tables(["BPSK", "QPSK", "8PSK", "16QAM"])
    pc = points[:, 0].astype(np.float64) + 1j * points[:, 1]
    angles = np.array([0.0, 0.3, 1.1, 2.0, 4.5])
    x, _ = R.real_frames(3, 16, "QPSK", 10.0, 1)
    s2, gain = np.array([0.1, 0.5, 2.0]), np.array([1.0, 0.8, 1.3])
    y = R.to_complex(x)
    for planar in (False, True):
        ll, L, best, pred = likelihood_reference(R.in_layout(x, planar), s2, gain, points, classes, angles, mode, planar=planar)
        assert ll.shape == (3, 4) and L.shape == (3, 4, 5) and best.shape == (3, 4) and pred.shape == (3,)
        for b in range(3):
            for c, (off, M) in enumerate(classes):
                want = [R.loglik_plain(y[b], s2[b], gain[b], pc[off:off + M], th) for th in angles]
                assert np.allclose(L[b, c], want, rtol=1e-11, atol=1e-11)
                assert best[b, c] == int(np.argmax(L[b, c]))
                assert np.isclose(ll[b, c], max(want) if mode == "max" else R.logmeanexp_plain(want), rtol=1e-11)
            assert pred[b] == int(np.argmax(ll[b]))
    # the table of (cos, sin) in place of the angles, the kinds in the descriptors, complex points: the same numbers
    table = np.stack([np.cos(angles), np.sin(angles)], axis=1)
    again = likelihood_reference(x, s2, gain, pc, [(0,) + c for c in classes], table, ("max", "mean").index(mode))
    assert np.allclose(again[0], ll, rtol=1e-12) and np.array_equal(again[3], pred)
    # and the helper that carries the bound says the same
    both = R.reference_and_bound(x, s2, gain, points, classes, table, mode)
    assert np.allclose(both["L"], L, rtol=1e-12) and np.allclose(both["loglik"], ll, rtol=1e-12)
    assert np.array_equal(both["best_rot"], best) and np.array_equal(both["pred"], pred) and np.all(both["E"] > 0)


def test_a_clean_frame_finds_its_class_and_its_rotation():
    """16QAM symbols turned by rotation 5 of 64, sigma2 tiny: the maximum lies at 16QAM and at rotations 5, 21, 37, 53 (the
    constellation's quarter turns), the first of which wins."""
    from vit_vs_raw_iq_amd import LikelihoodClassifier, likelihood_reference
    clf = LikelihoodClassifier(64)
    classes = [d[1:] for d in clf.descriptors]
    k = clf.class_names.index("16QAM")
    off, M = classes[k]
    rng = np.random.default_rng(0)
    s = clf.points[off + rng.integers(0, M, 64)].astype(np.float64) @ np.array([1, 1j])
    x = R.from_complex((s * np.exp(1j * clf.angles[5]))[None], dtype=np.float64)
    ll, L, best, pred = likelihood_reference(x, 1e-3, None, clf.points, classes, clf.angles, "max")
    assert pred[0] == k and best[0, k] == 5 and np.isfinite(ll).all()
    assert np.allclose(L[0, k, [5, 21, 37, 53]], L[0, k, 5], atol=1e-6) and L[0, k, 5] > L[0, k, 6] + 100
    assert abs(ll[0, k] - 64 * np.log(1 / 16)) < 1e-6                     # every symbol sits on a point: the mixture weight is left
    # a noisy QPSK frame under a phase that is not on the grid, at its true variance
    x4, s4 = R.real_frames(1, 64, "QPSK", 20.0, 4)
    assert likelihood_reference(x4, s4, None, clf.points, classes, clf.angles, "mean")[3][0] == clf.class_names.index("QPSK")


def test_max_bounds_mean_and_one_rotation_makes_them_equal():
    from vit_vs_raw_iq_amd import likelihood_reference
    clf, points, classes = tables(["BPSK", "8PSK", "16APSK", "32QAM"])
    x, s2 = R.real_frames(4, 16, "8PSK", 6.0, 2)
    mx = likelihood_reference(x, s2, None, points, classes, clf.angles, "max")
    mn = likelihood_reference(x, s2, None, points, classes, clf.angles, "mean")
    assert np.all(mx[0] >= mn[0]) and np.any(mx[0] > mn[0] + 1e-3) and np.array_equal(mx[1], mn[1]) and np.array_equal(mx[2], mn[2])
    assert np.all(mn[0] >= mx[0] - np.log(64))                                # the mean holds at least the largest term
    one = [likelihood_reference(x, s2, None, points, classes, np.array([0.7]), m) for m in ("max", "mean")]
    assert np.array_equal(one[0][0], one[1][0]) and np.array_equal(one[0][0], one[0][1][:, :, 0]) and not one[0][2].any()


def test_permuting_the_points_of_a_class_changes_nothing_beyond_rounding():
    from vit_vs_raw_iq_amd import likelihood_reference
    clf, points, classes = tables(["16QAM", "32APSK"])
    x, s2 = R.real_frames(2, 16, "16QAM", 12.0, 3)
    base = likelihood_reference(x, s2, None, points, classes, clf.angles, "mean")
    perm = points.copy()
    rng = np.random.default_rng(1)
    for off, M in classes:
        perm[off:off + M] = points[off + rng.permutation(M)]
    other = likelihood_reference(x, s2, None, perm, classes, clf.angles, "mean")
    assert np.allclose(other[1], base[1], rtol=1e-12, atol=1e-10) and np.array_equal(other[3], base[3])
    # (best_rot may move between the quarter turns of these constellations, equal maxima that only rounding orders)
    assert np.allclose(np.take_along_axis(base[1], other[2][..., None], axis=2)[..., 0], base[1].max(axis=2), rtol=1e-12)
    assert np.array_equal(other[2] % 16, base[2] % 16)


def test_a_wrong_class_at_high_snr_stays_finite_and_a_bad_variance_is_nan():
    from vit_vs_raw_iq_amd import likelihood_reference
    clf, points, classes = tables(["BPSK", "QPSK", "256QAM"])
    x, _ = R.real_frames(3, 16, "256QAM", 40.0, 5)
    ll, L, best, pred = likelihood_reference(x, 1e-4, None, points, classes, clf.angles, "mean")
    assert np.isfinite(L).all() and np.isfinite(ll).all() and ll[:, 0].max() < -1e4           # exp(-1e4) is 0 in fp64
    assert np.all(pred == 2)
    for bad in (0.0, -1.0, np.nan, np.inf):
        ll, L, best, pred = likelihood_reference(x, np.array([1e-4, bad, 1e-4]), None, points, classes, clf.angles, "max")
        assert np.isnan(ll[1]).all() and np.isnan(L[1]).all() and np.all(best[1] == -1) and pred[1] == -1
        assert np.isfinite(ll[[0, 2]]).all() and np.all(pred[[0, 2]] == 2) and np.all(best[[0, 2]] >= 0)


def test_binding_struct_matches_the_header():
    import vit_vs_raw_iq_amd._native as N
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iqvit.h")).read(), flags=re.S)
    body = re.search(r"typedef struct iq_likelihood \{(.*?)\}", src, flags=re.S).group(1)
    names = [w for d in body.split(";") if d.strip() for w in re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", d.strip())]
    assert names == [f[0] for f in N.Likelihood._fields_] == ["points", "classes", "n_classes", "rot", "n_rot", "planar", "mode", "gain"]
    assert [f[1] for f in N.Likelihood._fields_] == [ctypes.c_void_p, ctypes.POINTER(N.SynthClass), ctypes.c_int, ctypes.c_void_p,
                                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert ctypes.sizeof(N.Likelihood) == 56
    assert [getattr(N.Likelihood, f).offset for f in names] == [0, 8, 16, 24, 32, 36, 40, 48]
    enum = re.search(r"enum \{ IQ_LIK_MAX = (\d), IQ_LIK_MEAN = (\d) \}", src)
    assert [int(v) for v in enum.groups()] == [0, 1]
    decl = re.search(r"int iq_frames_likelihood\((.*?)\);", src, flags=re.S).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["iq_frames_likelihood"][1]) == 10
    assert hasattr(N.lib(), "iq_frames_likelihood")                              # the symbol is exported
    from vit_vs_raw_iq_amd.likelihood import MAX_CLASSES, MAX_POINTS, MAX_ROTATIONS, MODES
    assert (MAX_CLASSES, MAX_ROTATIONS, MAX_POINTS, MODES) == (64, 256, 2048, ("max", "mean"))


def test_every_refusal_returns_before_a_hip_call():
    """Pointers that are never dereferenced: a refusal looks at their value only (the class list is host memory and is read)."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    ARG, UNSUPPORTED = 1, 2
    A = 0x10000                                            # "an aligned pointer"

    def call(x=A, sigma2=A, loglik=A, rot_ll=A, best_rot=A, pred=A, n=1, length=512, par="ok", classes=((0, 0, 16), (0, 16, 4)),
             n_classes=None, **fields):
        arr = None if classes is None else (N.SynthClass * max(1, len(classes)))(*[N.SynthClass(*c) for c in classes])
        ok = dict(points=A, classes=arr, n_classes=len(classes or ()) if n_classes is None else n_classes, rot=A, n_rot=64, planar=0,
                  mode=0, gain=A)
        p = None if par is None else N.Likelihood(**{**ok, **fields})
        return L.iq_frames_likelihood(x, sigma2, loglik, rot_ll, best_rot, pred, n, length, ctypes.byref(p) if p is not None else None, None)
    # (a valid call with n = 1 would launch: none is made here)
    assert call(x=None) == ARG and call(sigma2=None) == ARG and call(loglik=None) == ARG and call(par=None) == ARG
    assert call(points=None) == ARG and call(classes=None, n_classes=2) == ARG and call(rot=None) == ARG
    assert call(length=0) == ARG and call(length=-4) == ARG and call(n_classes=0) == ARG and call(n_classes=-1) == ARG
    assert call(n_rot=0) == ARG and call(n_rot=-2) == ARG
    assert call(planar=2) == ARG and call(planar=-1) == ARG and call(mode=2) == ARG and call(mode=-1) == ARG
    # alignment: interleaved frames and the points 8 bytes, planar frames and everything else 4
    assert call(x=A + 4) == ARG and call(x=A + 2, planar=1) == ARG and call(points=A + 4) == ARG
    for name in ("sigma2", "loglik", "rot_ll", "best_rot", "pred", "rot", "gain"):
        assert call(**{name: A + 2}) == ARG, name
    # the class list
    assert call(classes=((1, 0, 4),)) == ARG and call(classes=((2, 0, 4),)) == ARG and call(classes=((0, 0, 4), (-1, 4, 4))) == ARG
    assert call(classes=((0, 0, 0),)) == ARG and call(classes=((0, 0, -3),)) == ARG and call(classes=((0, -1, 4),)) == ARG
    assert call(classes=((0, 2 ** 31 - 2, 4),)) == ARG                                        # offset + count past the int range
    # the limits
    many = tuple((0, i, 1) for i in range(65))
    assert call(classes=many) == UNSUPPORTED and call(classes=many[:64], n=0) == 0
    assert call(n_rot=257) == UNSUPPORTED and call(n_rot=256, n=0) == 0
    assert call(classes=((0, 0, 2049),)) == UNSUPPORTED and call(classes=((0, 2040, 9),)) == UNSUPPORTED
    assert call(classes=((0, 0, 2048),), n=0) == 0 and call(classes=((0, 2047, 1), (0, 0, 2)), n=0) == 0
    assert call(length=8193) == UNSUPPORTED and call(length=8192, n=0) == 0
    assert call(n_rot=257, mode=5) == ARG and call(length=8193, classes=((1, 0, 4),)) == ARG       # ARG comes first
    assert call(classes=many[:64] + ((1, 0, 1),)) == UNSUPPORTED                 # (a class the kernel could not use is not looked at)
    # n_frames <= 0 is success, nothing launched; the optional pointers may be NULL
    for n in (0, -3):
        assert call(n=n) == 0 and call(n=n, rot_ll=None, best_rot=None, pred=None, gain=None, planar=1, mode=1) == 0


def test_python_argument_checks():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import LikelihoodClassifier, likelihood_reference
    from vit_vs_raw_iq_amd import data as D
    from vit_vs_raw_iq_amd.evaluation import evaluate_likelihood_with_confusion
    for kw, exc in ((dict(length=0), ValueError), (dict(length=8193), ValueError), (dict(length=8.0), TypeError),
                    (dict(length=64, classes=[]), ValueError), (dict(length=64, classes="QPSK"), TypeError),
                    (dict(length=64, classes=["QPSK", "QPSK"]), ValueError), (dict(length=64, classes=["GMSK"]), ValueError),
                    (dict(length=64, classes=["OQPSK", "QPSK"]), ValueError), (dict(length=64, classes=["nothing"]), ValueError),
                    (dict(length=64, classes=[3]), TypeError), (dict(length=64, classes=[("a", [1, 2], 3)]), TypeError),
                    (dict(length=64, classes=[("a", [])]), ValueError), (dict(length=64, classes=[("a", [0, 0])]), ValueError),
                    (dict(length=64, classes=[("a", [1, np.nan])]), ValueError),
                    (dict(length=64, classes=[(f"c{i}", [1]) for i in range(65)]), ValueError),
                    (dict(length=64, classes=[("a", np.ones(2049))]), ValueError),
                    (dict(length=64, rotations=0), ValueError), (dict(length=64, rotations=257), ValueError),
                    (dict(length=64, rotations=64.0), TypeError), (dict(length=64, rotations=True), TypeError),
                    (dict(length=64, rotations=[]), ValueError), (dict(length=64, rotations=np.zeros(257)), ValueError),
                    (dict(length=64, rotations=[0.0, np.inf]), ValueError), (dict(length=64, rotations=np.zeros((2, 2))), TypeError),
                    (dict(length=64, rotations="many"), TypeError),
                    (dict(length=64, mode="glrt"), ValueError), (dict(length=64, mode=0), ValueError),
                    (dict(length=64, layout="interleaved"), ValueError), (dict(length=64, device="cpu"), TypeError)):
        with pytest.raises(exc):
            LikelihoodClassifier(**kw)
    clf = LikelihoodClassifier(500)
    assert clf.class_names == D.CLASSES[:17] == list(P.likelihood.TABLE_CLASSES) and clf.n_classes == 17 and clf.points.shape == (812, 2)
    assert (clf.n_rotations, clf.mode, clf.layout, clf.planar) == (64, "max", "frames", 0)
    assert clf.frame_shape(3) == (3, 500, 2) and LikelihoodClassifier(500, layout="planar").frame_shape(3) == (3, 2, 500)
    assert np.allclose(clf.angles, 2 * np.pi * np.arange(64) / 64) and clf.rot.dtype == np.float32 and clf.rot.shape == (64, 2)
    assert np.array_equal(clf.rot, np.stack([np.cos(clf.angles), np.sin(clf.angles)], axis=1).astype(np.float32))
    assert np.array_equal(clf.rot[0], [1, 0]) and np.array_equal(clf.rot[32, :1], [-1])
    for name, (kind, off, M) in zip(clf.class_names, clf.descriptors):                        # the table is FrameSynth's
        want = D.constellation(name)
        assert kind == 0 and np.array_equal(clf.points[off:off + M], np.stack([want.real, want.imag], axis=1).astype(np.float32))
    own = LikelihoodClassifier(8, classes=[("ring", np.exp(2j * np.pi * np.arange(3) / 3) * 5), "BPSK"], rotations=[0.0, 0.1], mode="mean")
    assert own.class_names == ["ring", "BPSK"] and own.descriptors == [(0, 0, 3), (0, 3, 2)] and own.n_rotations == 2
    assert np.allclose((own.points[:3] ** 2).sum(axis=1), 1.0)                                # scaled to unit power
    assert LikelihoodClassifier(8, classes={"two": [1, -1]}).descriptors == [(0, 0, 2)]
    # calls: the checks come before any device work, and a CPU tensor has no path
    x = torch.zeros(2, 500, 2)
    for kw, exc in ((dict(), ValueError), (dict(sigma2=0.1, snr_db=10.0), ValueError), (dict(sigma2=[0.1, 0.2, 0.3]), ValueError),
                    (dict(sigma2="x"), TypeError), (dict(sigma2=torch.zeros(2, dtype=torch.bool)), TypeError),
                    (dict(snr_db=torch.zeros(3)), ValueError), (dict(sigma2=0.1, gain=[1.0]), ValueError),
                    (dict(sigma2=0.1, gain=1j), TypeError), (dict(sigma2=0.1, return_rot=2), TypeError),
                    (dict(sigma2=0.1, return_best="yes"), TypeError)):
        with pytest.raises(exc):
            clf(x, **kw)
    for bad in (torch.zeros(2, 2, 500), torch.zeros(2, 499, 2), torch.zeros(500, 2), np.zeros((2, 500, 2))):
        with pytest.raises(ValueError):
            clf(bad, sigma2=0.1)
    for call in (clf, clf.predict):
        with pytest.raises(P.IqError, match="no CPU fallback"):
            call(x, sigma2=0.1)
        with pytest.raises(P.IqError, match="no CPU fallback"):
            call(x, snr_db=torch.tensor([0.0, 8.0]), gain=[1.0, 0.5])
    with pytest.raises(ValueError):
        evaluate_likelihood_with_confusion(clf, [], "cpu", ["a", "b"], "/nonexistent")
    for kw in (dict(mode="glrt"), dict(classes=[(0, 900)]), dict(classes=[(1, 0, 4)]), dict(classes=[(0, 0)])):
        args = dict(x=np.zeros((1, 4, 2)), sigma2=1.0, gain=None, points=clf.points, classes=[(0, 2)], angles=clf.angles, mode="max")
        with pytest.raises(ValueError):
            likelihood_reference(**{**args, **kw})
    with pytest.raises(ValueError):
        likelihood_reference(np.zeros((1, 4, 3)), 1.0, None, clf.points, [(0, 2)], clf.angles)


def test_noise_for_both_conventions():
    from vit_vs_raw_iq_amd import LikelihoodClassifier, noise_for
    assert noise_for(10.0) == (1.0, pytest.approx(0.1)) and noise_for(0.0, normalised=False) == (1.0, 1.0)
    g, s2 = noise_for(10.0, normalised=True)
    assert g == pytest.approx(1 / np.sqrt(1.1)) and s2 == pytest.approx(0.1 / 1.1) and g * g + s2 == pytest.approx(1.0)
    snr = np.array([-8.0, 0.0, 8.0, 20.0])
    g, s2 = noise_for(snr, True)
    assert g.shape == s2.shape == (4,) and np.allclose(g * g + s2, 1.0) and np.allclose(s2 / (g * g), 10 ** (-snr / 10))
    gt, st = noise_for(torch.from_numpy(snr), True)
    assert isinstance(gt, torch.Tensor) and np.allclose(gt.numpy(), g) and np.allclose(st.numpy(), s2)
    g1, s1 = noise_for(torch.tensor([20.0]))
    assert g1.item() == 1.0 and s1.item() == pytest.approx(0.01)
    assert LikelihoodClassifier.noise_for(10.0) == noise_for(10.0)
    with pytest.raises(TypeError):
        noise_for(10.0, normalised="yes")
    # the normalised convention is what dividing a generator's frame by its rms does: the likelihood under (g, s2) of the scaled
    # frame orders the classes as (1, sigma2) orders them on the frame itself, and differs by no more than rounding
    from vit_vs_raw_iq_amd import likelihood_reference
    clf = LikelihoodClassifier(32, classes=["QPSK", "16QAM", "8PSK"])
    classes = [d[1:] for d in clf.descriptors]
    x, sig = R.real_frames(2, 32, "16QAM", 12.0, 9)
    g, s2 = noise_for(12.0, True)
    a = likelihood_reference(x, sig, None, clf.points, classes, clf.angles)[0]
    b = likelihood_reference(x.astype(np.float64) * g, s2, g, clf.points, classes, clf.angles)[0]
    assert np.allclose(a, b, rtol=1e-6)


def test_exact_cases_are_exact_in_fp32():
    """What the bit-for-bit GPU test assumes: on the integer cases every value of the definition is an fp32 number, the
    per-rotation tables differ between rotations, and the class of the origin ties over all four."""
    from vit_vs_raw_iq_amd import likelihood_reference
    assert len(R.EXACT_POINTS) == 12 and all(np.all(R.EXACT_POINTS[o:o + m] == R.EXACT_POINTS[o]) and m & (m - 1) == 0 for o, m in R.EXACT_CLASSES)
    for length in (1, 65, 257, 8192):
        x, s2, gain = R.exact_case(3, length, length)
        assert np.array_equal(np.log2(s2), np.round(np.log2(s2)))
        ll, L, best, pred = likelihood_reference(x, s2, gain, R.EXACT_POINTS, R.EXACT_CLASSES, R.QUARTER_TURNS, "max")
        assert np.array_equal(R.f32(L), L) and np.array_equal(L * 16, np.round(L * 16)) and np.abs(L).max() * 16 < 2 ** 24
        assert np.all(L[:, 3] == L[:, 3, :1]) and np.all(best[:, 3] == 0)
        if length > 1:
            assert np.any(L[:, 0] != L[:, 0, :1]) and np.any(best[:, :3] > 0)
        one = [likelihood_reference(x, s2, gain, R.EXACT_POINTS, R.EXACT_CLASSES, R.QUARTER_TURNS[1:2], m)[0] for m in ("max", "mean")]
        assert np.array_equal(one[0], one[1]) and np.array_equal(one[0], L[:, :, 1])


def test_the_bound_is_small_and_grows_with_q():
    """The derived bound on real frames: positive, far below the values it bounds, and larger at a smaller sigma2 (q amplifies
    the rounding of the rotation and of d)."""
    clf, points, classes = tables(["QPSK", "16QAM", "64QAM"])
    x, _ = R.real_frames(2, 16, "16QAM", 20.0, 6)
    prev = None
    for s2 in (10.0, 1.0, 1e-2, 1e-4):
        for mode in ("max", "mean"):
            ref = R.reference_and_bound(x, np.float32(s2), None, points, classes, clf.rot, mode)
            assert np.all(ref["E"] > 0) and np.all(ref["Ell"] >= ref["E"].max(axis=2))
            assert np.all(ref["Ell"] <= 1e-4 * np.maximum(np.abs(ref["loglik"]), 1.0))
        assert prev is None or ref["E"].max() > prev
        prev = ref["E"].max()
    assert R.U == 2.0 ** -24 and R.SLACK < 1.001


def test_decision_set_is_what_the_gpu_test_assumes():
    """The 68 frames at 20 dB: the fp64 definition classifies every one correctly in both modes, and on EVERY frame the margin
    between the best and the second class exceeds twice the bound, so the device must decide every frame as the definition does.
    The package's own definition agrees with the helper that carries the bound (on the first 8 frames: it is the slower one)."""
    from vit_vs_raw_iq_amd import LikelihoodClassifier, likelihood_reference
    X, Y, s2 = R.decision_set()
    assert X.shape == (68, 128, 2) and np.array_equal(np.bincount(Y), np.full(17, 4)) and s2 == np.float32(0.01)
    for mode in ("max", "mean"):
        ref = R.decision_reference(mode)
        assert np.array_equal(ref["pred"], Y), mode                                            # 68 of 68
        worst = ref["Ell"].max(axis=1)
        print(f"{mode}: smallest margin {R.margin(ref['loglik']).min():.3f}, largest bound {worst.max():.4f}")
        assert np.all(R.margin(ref["loglik"]) > 2.0 * worst), mode
    clf = LikelihoodClassifier(128)
    ll, L, best, pred = likelihood_reference(X[:8], s2, None, clf.points, clf.descriptors, clf.rot, "max")
    ref = R.decision_reference("max")
    assert np.allclose(L, ref["L"][:8], rtol=1e-12) and np.array_equal(best, ref["best_rot"][:8]) and np.array_equal(pred, Y[:8])
    # rotations the device may take for the maximum: the first largest of the definition is always among them
    ties = R.rotation_ties(ref["L"], ref["E"])
    assert np.all(np.take_along_axis(ties, ref["best_rot"][..., None], axis=2))
    assert (ties.sum(axis=2) == 1).sum() > 50 and ties.sum(axis=2).max() <= 32
