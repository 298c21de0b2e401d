"""Host only: the fp64 definitions of the likelihood gradients (tests/likelihood_bwd_ref.py) against torch autograd of the plain
logsumexp statements and against central differences of the EM definition, the inertness of skipping zero weights, the exact
cases, the two ctypes bindings against include/iqvit.h, every refusal of iq_frames_likelihood_bwd and iq_frames_likelihood_em_bwd
that returns before a HIP call, the differentiable= argument with the unchanged default, and the host FGSM table of the decision
set."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import likelihood_bwd_ref as G
import likelihood_em_ref as EM
import likelihood_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_case():
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    clf = LikelihoodClassifier(16, classes=["BPSK", "QPSK", "8PSK", "16QAM"], rotations=[0.0, 0.3, 1.1, 2.0, 4.5])
    x, _ = R.real_frames(3, 16, "QPSK", 10.0, 1)
    dl = np.random.default_rng(0).standard_normal((3, 4))
    return clf, [d[1:] for d in clf.descriptors], x, np.array([0.1, 0.5, 2.0]), np.array([1.0, 0.8, 1.3]), dl


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_definition_is_autograd_of_the_plain_statement(mode):
    """Four classes, five rotations, three frames with their own sigma2 and a gain different from 1, both layouts: dx of the
    definition, fed the definition's own forward, is what torch autograd makes of logsumexp, to rounding."""
    from vit_vs_raw_iq_amd import likelihood_reference
    clf, classes, x, s2, gain, dl = small_case()
    table = np.stack([np.cos(clf.angles), np.sin(clf.angles)], axis=1)
    for planar in (False, True):
        xl = R.in_layout(x, planar).astype(np.float64)
        ll, L, best, _ = likelihood_reference(xl, s2, gain, clf.points, classes, clf.angles, mode, planar=planar)
        xt = torch.tensor(xl, requires_grad=True)
        out = G.loglik_plain_torch(xt, s2, gain, clf.points, classes, clf.angles, mode, planar)
        assert np.allclose(out.detach().numpy(), ll, rtol=1e-12)
        (out * torch.tensor(dl)).sum().backward()
        dx, E = G.likelihood_reference_bwd(xl, s2, gain, clf.points, classes, table, mode, dl, loglik=ll, rot_ll=L, best_rot=best,
                                           planar=planar, bound=True)
        assert dx.shape == xl.shape == E.shape and np.abs(dx).max() > 1.0
        assert np.abs(dx - xt.grad.numpy()).max() <= 1e-13 * np.abs(dx).max()
        assert np.all(E > 0) and E.max() < 1e-4 * np.abs(dx).max()                  # the fp32 bound: positive and far below dx


def test_em_definition_is_autograd_at_a_fixed_state_and_central_differences_at_a_converged_one():
    """The partial derivative at a held (h, v) against autograd; and, at 1000 iterations from a given start, against central
    differences of likelihood_em_reference's Lambda, which re-estimates (h, v) on every perturbed frame: the total derivative.
    The envelope argument makes them equal at a converged interior point, for a wrong class (BPSK on QPSK frames) as well.
    (Enough iterations: at 200 the BPSK chain of the second frame, which this start sends past h = 0, is still moving, and the
    two differ in the second digit; every other chain agrees to 1e-9 there already.)"""
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier, likelihood_em_reference
    clf = HybridLikelihoodClassifier(24, classes=["BPSK", "QPSK", "8PSK"])
    classes = [d[1:] for d in clf.descriptors]
    x = R.real_frames(2, 24, "QPSK", 12.0, 3, gain=0.8)[0].astype(np.float64)
    rng = np.random.default_rng(1)
    h = 0.8 * np.exp(2j * np.pi * rng.uniform(0, 1, (2, 3)))
    v = rng.uniform(0.05, 0.3, (2, 3))
    dl = rng.standard_normal((2, 3))
    for planar in (False, True):
        xl = R.in_layout(x, planar)
        xt = torch.tensor(xl, requires_grad=True)
        (G.lambda_plain_torch(xt, clf.points, classes, h, v, planar) * torch.tensor(dl)).sum().backward()
        dx, E = G.likelihood_em_reference_bwd(xl, clf.points, classes, dl, h, v, planar=planar, bound=True)
        assert np.abs(dx - xt.grad.numpy()).max() <= 1e-13 * np.abs(dx).max()
        assert np.all(E > 0) and E.max() < 1e-4 * np.abs(dx).max()
    # the total derivative
    run = lambda frames: likelihood_em_reference(frames, clf.points, classes, clf.starts, iters=1000, h0=h0, v0=v0)   # noqa: E731
    h0, v0 = np.full((2, 3), 0.7 + 0.3j), np.full((2, 3), 0.1)
    base = run(x)
    dx = G.likelihood_em_reference_bwd(x, clf.points, classes, np.ones((2, 3)), base.h, base.v)
    step = 1e-5
    for b, n, k in ((0, 0, 0), (0, 7, 1), (1, 23, 0), (1, 11, 1)):
        up, dn = x.copy(), x.copy()
        up[b, n, k] += step
        dn[b, n, k] -= step
        fd = (run(up).loglik[b] - run(dn).loglik[b]).sum() / (2 * step)
        assert abs(fd - dx[b, n, k]) <= 1e-6 * max(1.0, abs(dx[b, n, k])), (b, n, k, fd, dx[b, n, k])


def test_skipping_zero_weights_is_inert():
    """A class with weight 0 adds nothing: the gradient is that of the classes asked about alone, bit for bit, whatever the
    skipped class holds (NaN points, a NaN forward result, a dead EM state); with every weight 0 dx is 0."""
    from vit_vs_raw_iq_amd import likelihood_reference
    clf, classes, x, s2, gain, dl = small_case()
    table = np.stack([np.cos(clf.angles), np.sin(clf.angles)], axis=1)
    dl[:, 2] = 0.0
    for mode in ("max", "mean"):
        ll, L, best, _ = likelihood_reference(x, s2, gain, clf.points, classes, clf.angles, mode)
        whole = G.likelihood_reference_bwd(x, s2, gain, clf.points, classes, table, mode, dl, ll, L, best)
        keep = [0, 1, 3]
        part = G.likelihood_reference_bwd(x, s2, gain, clf.points, [classes[c] for c in keep], table, mode, dl[:, keep], ll[:, keep],
                                          L[:, keep], best[:, keep])
        assert np.array_equal(whole, part)
        pts, llb, Lb, bb = clf.points.copy(), ll.copy(), L.copy(), best.copy()
        pts[classes[2][0]:classes[2][0] + classes[2][1]] = np.nan
        llb[:, 2], Lb[:, 2], bb[:, 2] = np.nan, np.nan, -1
        assert np.array_equal(G.likelihood_reference_bwd(x, s2, gain, pts, classes, table, mode, dl, llb, Lb, bb), whole)
        assert not G.likelihood_reference_bwd(x, s2, gain, clf.points, classes, table, mode, np.zeros((3, 4)), ll, L, best).any()
    h, v = np.full((3, 4), 0.9 + 0.1j), np.full((3, 4), 0.2)
    whole = G.likelihood_em_reference_bwd(x, clf.points, classes, dl, h, v)
    h[:, 2], v[0, 2], v[1, 2] = np.nan, 0.0, np.inf
    assert np.isfinite(whole).all() and np.array_equal(G.likelihood_em_reference_bwd(x, clf.points, classes, dl, h, v), whole)
    # bad data with a weight: its own frame only
    dl[1, 2] = 1.0
    bad = G.likelihood_em_reference_bwd(x, clf.points, classes, dl, h, v)
    assert np.isnan(bad[1]).all() and np.array_equal(bad[[0, 2]], whole[[0, 2]])
    for s in (0.0, -1.0, np.nan, np.inf):
        ll, L, best, _ = likelihood_reference(x, np.array([0.1, s, 2.0]), gain, clf.points, classes, clf.angles, "max")
        got = G.likelihood_reference_bwd(x, np.array([0.1, s, 2.0]), gain, clf.points, classes, table, "max", dl, ll, L, best)
        assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()


def test_exact_cases_are_exact_in_fp32():
    """What the bit-for-bit GPU test assumes.  Every class of likelihood_ref's exact table is copies of one point, so m = p with
    nothing rounded; integer frames, quarter turns, power-of-two sigma2 and weights: every dx is a multiple of 2^-7 far below 2^17,
    an fp32 number on both sides.  The origin class ties over all four rotations: every share of 'mean' is exactly 1/4."""
    from vit_vs_raw_iq_amd import likelihood_reference
    for length in (1, 65, 513):
        x, s2, gain = R.exact_case(3, length, length)
        dl = G.exact_weights(3, 4, length)
        assert (dl == 0).any() or length == 1
        ll, L, best, _ = likelihood_reference(x, s2, gain, R.EXACT_POINTS, R.EXACT_CLASSES, R.QUARTER_TURNS, "max")
        dx = G.likelihood_reference_bwd(x, s2, gain, R.EXACT_POINTS, R.EXACT_CLASSES, R.QUARTER_TURNS, "max", dl, best_rot=best)
        assert np.array_equal(R.f32(dx), dx) and np.array_equal(dx * 128, np.round(dx * 128)) and np.abs(dx).max() < 2 ** 17
        assert np.any(dx != 0)
        # by hand: -2 q w (y - a s rotated back to y's frame), summed over the classes
        y = R.to_complex(x)
        want = np.zeros_like(y)
        s = np.array([R.EXACT_POINTS[o] for o, _ in R.EXACT_CLASSES], np.float64) @ np.array([1, 1j])
        turn = R.QUARTER_TURNS.astype(np.float64) @ np.array([1, 1j])
        for c in range(4):
            want += (-2.0 / s2 * dl[:, c])[:, None] * (y - (gain[:, None] * s[c]) * turn[best[:, c]][:, None])
        assert np.array_equal(dx, R.from_complex(want, dtype=np.float64))
        # 'mean' on the origin class alone
        only = np.zeros_like(dl)
        only[:, 3] = dl[:, 3] if dl[:, 3].any() else 1.0
        llm, Lm, _, _ = likelihood_reference(x, s2, gain, R.EXACT_POINTS, R.EXACT_CLASSES, R.QUARTER_TURNS, "mean")
        assert np.array_equal(llm[:, 3], Lm[:, 3, 0]) and np.all(Lm[:, 3] == Lm[:, 3, :1])
        dm = G.likelihood_reference_bwd(x, s2, gain, R.EXACT_POINTS, R.EXACT_CLASSES, R.QUARTER_TURNS, "mean", only, llm, Lm)
        assert np.array_equal(dm, R.from_complex((-2.0 / s2 * only[:, 3])[:, None] * y, dtype=np.float64)) and np.array_equal(R.f32(dm), dm)
    x, _, _ = EM.exact_case(3, 129, 5, tiled=False)
    h, v = G.exact_em_state(3, 4, 6)
    dl = G.exact_weights(3, 4, 7)
    dx = G.likelihood_em_reference_bwd(x, EM.EXACT_POINTS, EM.EXACT_CLASSES, dl, h, v)
    assert np.array_equal(R.f32(dx), dx) and np.array_equal(dx * 64, np.round(dx * 64)) and np.any(dx != 0)
    assert {tuple(t) for t in h.reshape(-1, 2)} == {(1, 0), (0, 1), (2, 0), (0.5, 0)}


def test_bindings_match_the_header():
    import vit_vs_raw_iq_amd._native as N
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iqvit.h")).read(), flags=re.S)
    for name, count, struct, ptr in (("iq_frames_likelihood_bwd", 11, N.Likelihood, "iq_likelihood_t"),
                                     ("iq_frames_likelihood_em_bwd", 9, N.LikelihoodEm, "iq_likelihood_em_t")):
        decl = re.search(r"int " + name + r"\((.*?)\);", src, flags=re.S).group(1)
        res, args = N.SIGNATURES[name]
        assert len(decl.split(",")) == len(args) == count and res is ctypes.c_int
        assert f"const {ptr}* par" in decl and args[-2] is ctypes.POINTER(struct) and args[-4:-2] == [ctypes.c_int, ctypes.c_int]
        assert all(a is ctypes.c_void_p for a in args[:-4] + args[-1:])
        assert hasattr(N.lib(), name)                                            # the symbol is exported
    # the forward's structs and declarations stay as they were
    assert ctypes.sizeof(N.Likelihood) == 56 and ctypes.sizeof(N.LikelihoodEm) == 72
    assert len(N.SIGNATURES["iq_frames_likelihood"][1]) == 10 and len(N.SIGNATURES["iq_frames_likelihood_em"][1]) == 12


def test_every_refusal_returns_before_a_hip_call():
    """Pointers that are never dereferenced: a refusal looks at their value only (the class list is host memory and is read)."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    ARG, UNSUPPORTED = 1, 2
    A = 0x10000                                            # "an aligned pointer"

    def classes_of(classes):
        return None if classes is None else (N.SynthClass * max(1, len(classes)))(*[N.SynthClass(*c) for c in classes])

    def lik(x=A, sigma2=A, dloglik=A, loglik=A, rot_ll=A, best_rot=A, dx=A, n=1, length=512, par="ok",
            classes=((0, 0, 16), (0, 16, 4)), n_classes=None, **fields):
        ok = dict(points=A, classes=classes_of(classes), n_classes=len(classes or ()) if n_classes is None else n_classes, rot=A, n_rot=64,
                  planar=0, mode=0, gain=A)
        p = None if par is None else N.Likelihood(**{**ok, **fields})
        return L.iq_frames_likelihood_bwd(x, sigma2, dloglik, loglik, rot_ll, best_rot, dx, n, length, ctypes.byref(p) if p is not None else None,
                                          None)

    def em(x=A, dloglik=A, h=A, v=A, dx=A, n=1, length=512, par="ok", classes=((0, 0, 16), (0, 16, 4)), n_classes=None, **fields):
        ok = dict(points=A, classes=classes_of(classes), n_classes=len(classes or ()) if n_classes is None else n_classes, starts=None,
                  n_starts=0, iters=-1, planar=0, mode=7, f0=5.0, floor=-1.0, h0=None, v0=None)        # what it ignores: nonsense
        p = None if par is None else N.LikelihoodEm(**{**ok, **fields})
        return L.iq_frames_likelihood_em_bwd(x, dloglik, h, v, dx, n, length, ctypes.byref(p) if p is not None else None, None)
    # (a valid call with n = 1 would launch: none is made here)
    for call, required in ((lik, ("x", "sigma2", "dloglik", "dx", "points", "rot")), (em, ("x", "dloglik", "h", "v", "dx", "points"))):
        for name in required:
            assert call(**{name: None}) == ARG, name
        assert call(par=None) == ARG and call(classes=None, n_classes=2) == ARG
        assert call(length=0) == ARG and call(length=-4) == ARG and call(n_classes=0) == ARG and call(n_classes=-1) == ARG
        assert call(planar=2) == ARG and call(planar=-1) == ARG
        # alignment: interleaved frames and the points 8 bytes, planar frames and everything else 4
        assert call(x=A + 4) == ARG and call(dx=A + 4) == ARG and call(x=A + 2, planar=1) == ARG and call(dx=A + 2, planar=1) == ARG
        assert call(x=A + 4, dx=A + 4, planar=1, n=0) == 0 and call(points=A + 4) == ARG
        # the class list
        assert call(classes=((1, 0, 4),)) == ARG and call(classes=((2, 0, 4),)) == ARG and call(classes=((0, 0, 4), (-1, 4, 4))) == ARG
        assert call(classes=((0, 0, 0),)) == ARG and call(classes=((0, 0, -3),)) == ARG and call(classes=((0, -1, 4),)) == ARG
        assert call(classes=((0, 2 ** 31 - 2, 4),)) == ARG                                    # offset + count past the int range
        # the limits
        many = tuple((0, i, 1) for i in range(65))
        assert call(classes=many) == UNSUPPORTED and call(classes=many[:64], n=0) == 0
        assert call(classes=((0, 0, 2049),)) == UNSUPPORTED and call(classes=((0, 2040, 9),)) == UNSUPPORTED
        assert call(classes=((0, 0, 2048),), n=0) == 0 and call(classes=((0, 2047, 1), (0, 0, 2)), n=0) == 0
        assert call(length=8193) == UNSUPPORTED and call(length=8192, n=0) == 0
        assert call(length=8193, classes=((1, 0, 4),)) == ARG                                 # ARG comes first
        for n in (0, -3):
            assert call(n=n) == 0
    assert lik(n_rot=0) == ARG and lik(n_rot=-2) == ARG and lik(mode=2) == ARG and lik(mode=-1) == ARG
    for name in ("sigma2", "dloglik", "loglik", "rot_ll", "best_rot", "rot", "gain"):
        assert lik(**{name: A + 2}) == ARG, name
    assert lik(n_rot=257) == UNSUPPORTED and lik(n_rot=256, n=0) == 0 and lik(n_rot=257, mode=5) == ARG
    # what each mode reads must be there; what it does not read may be NULL
    assert lik(best_rot=None, mode=0) == ARG and lik(loglik=None, mode=1) == ARG and lik(rot_ll=None, mode=1) == ARG
    assert lik(loglik=None, rot_ll=None, gain=None, mode=0, n=0) == 0 and lik(best_rot=None, mode=1, n=0) == 0
    assert em(h=A + 4) == ARG and em(dloglik=A + 2) == ARG and em(v=A + 2) == ARG
    assert em(n=0, n_starts=1000, iters=10 ** 6) == 0                                         # (ignored, not refused)


def test_differentiable_argument_and_the_unchanged_default():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier, LikelihoodClassifier
    for cls in (LikelihoodClassifier, HybridLikelihoodClassifier):
        for bad in (2, "yes", None, 1.0):
            with pytest.raises(TypeError):
                cls(64, differentiable=bad)
        plain, on = cls(64, classes=["BPSK", "QPSK"]), cls(64, classes=["BPSK", "QPSK"], differentiable=True)
        assert plain.differentiable is False and on.differentiable is True
        assert "differentiable" not in repr(plain) and repr(on) == repr(plain)[:-1] + ", differentiable=True)"
        noise = dict(sigma2=0.1) if cls is LikelihoodClassifier else {}
        x = torch.zeros(2, 64, 2, requires_grad=True)
        for clf in (plain, on):
            with pytest.raises(P.IqError, match="no CPU fallback"):
                clf(x, **noise)
            with pytest.raises(P.IqError, match="no CPU fallback"):
                clf.input_gradient(x, torch.zeros(2, 2), **noise)
            # input_gradient: the shape and the noise are checked before the device
            with pytest.raises(ValueError):
                clf.input_gradient(torch.zeros(2, 63, 2), torch.zeros(2, 2), **noise)
            for bad, exc in ((torch.zeros(2, 3), ValueError), (torch.zeros(3, 2), ValueError), (np.zeros((2, 2)), TypeError),
                             (torch.zeros(2, 2, dtype=torch.bool), TypeError)):
                with pytest.raises(exc):
                    clf.input_gradient(x, bad, **noise)
    with pytest.raises(ValueError):
        LikelihoodClassifier(64).input_gradient(torch.zeros(2, 64, 2), torch.zeros(2, 17))         # no noise given
    with pytest.raises(TypeError):
        HybridLikelihoodClassifier(64).input_gradient(torch.zeros(2, 64, 2), torch.zeros(2, 17), sigma2=0.1)


def test_attack_argument_checks():
    """fgsm / pgd / robustness_curve with a classifier in place of a model: everything is refused before the device, a CPU frame
    last; and a model takes neither loss= nor the noise keywords."""
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier, LikelihoodClassifier, fgsm, pgd, robustness_curve
    clf = LikelihoodClassifier(64, classes=["BPSK", "QPSK"])
    x, y = torch.zeros(2, 64, 2), torch.tensor([0, 1])
    with pytest.raises(ValueError, match="loss"):
        fgsm(clf, x, y, 0.1, sigma2=0.1, loss="hinge")
    with pytest.raises(ValueError):
        fgsm(clf, x, y, 0.1)                                                         # no noise
    with pytest.raises(ValueError):
        fgsm(clf, x, torch.tensor([0, 2]), 0.1, sigma2=0.1)                          # a label out of range
    with pytest.raises(ValueError):
        fgsm(LikelihoodClassifier(64, classes=["BPSK"]), x, torch.tensor([0, 0]), 0.1, sigma2=0.1)   # a margin needs two classes
    with pytest.raises(TypeError):
        fgsm(HybridLikelihoodClassifier(64, classes=["BPSK", "QPSK"]), x, y, 0.1, sigma2=0.1)       # the hybrid takes no noise
    with pytest.raises(ValueError):
        pgd(clf, x, y, 0.1, 0.05, 0, sigma2=0.1)
    with pytest.raises(TypeError):
        robustness_curve(clf, x, y, [0.0], sigma2=0.1, steps=3)                      # a pgd keyword under fgsm
    for call in (lambda: fgsm(clf, x, y, 0.1, sigma2=0.1), lambda: pgd(clf, x, y, 0.1, 0.05, 2, snr_db=10.0, loss="ce"),
                 lambda: robustness_curve(clf, x, y, [0.0, 0.1], sigma2=0.1, gain=1.0)):
        with pytest.raises(P.IqError, match="no CPU fallback"):
            call()
    model = object.__new__(P.AMCTransformerRawIQ)                                    # (never built: the keywords are refused first)
    for kw in (dict(loss="margin"), dict(sigma2=0.1), dict(loss="ce")):
        with pytest.raises(TypeError):
            fgsm(model, x, y, 0.1, **kw)
        with pytest.raises(TypeError):
            pgd(model, x, y, 0.1, 0.05, 2, **kw)
        with pytest.raises(TypeError):
            robustness_curve(model, x, y, [0.1], **kw)


def test_host_fgsm_table_of_the_decision_set():
    """One FGSM step on the margin loss takes decisions away that random signs of the same size leave alone.  Measured here at
    eps 0.05: clean 68/68, FGSM 0.338, random signs 0.926."""
    X, Y, _ = R.decision_set()
    t = G.host_fgsm()
    assert np.abs(t["x_adv"].astype(np.float64) - X).max() <= G.FGSM_EPS + 2.0 ** -24 * np.abs(t["x_adv"]).max()      # (rounded to fp32)
    assert np.mean(t["g"] != 0) > 0.9                  # (an exact 0: two real-valued classes at one rotation cancel in Im)
    clean, adv, rand = G.host_accuracy(X), G.host_accuracy(t["x_adv"]), G.host_accuracy(t["x_rand"])
    print(f"eps {G.FGSM_EPS}: clean {clean:.3f}, FGSM {adv:.3f}, random signs {rand:.3f}")
    assert clean == 1.0
    assert adv <= 0.5 * rand
