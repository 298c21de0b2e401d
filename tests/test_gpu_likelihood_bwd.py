"""GPU (MI355X): the gradients of the two likelihood classifiers with respect to the frame (csrc/likelihood_bwd.hip,
iq_frames_likelihood_bwd and iq_frames_likelihood_em_bwd; LikelihoodClassifier / HybridLikelihoodClassifier(differentiable=True),
input_gradient; adversarial.fgsm / pgd / robustness_curve on a classifier).

Every call through the C ABI here (`lik_bwd`, `em_bwd`, `lik_fwd`) carves its operands out of NaN-filled buffers and dx out of a
sentinel-filled one and checks the guards, that the operands hold what they held, and the kernel's name, afterwards.

The definitions (tests/likelihood_bwd_ref.py) are handed the DEVICE's forward outputs (loglik, rot_ll, best_rot; h, v), so both
sides weigh the same hypotheses and only the backward's arithmetic differs: the forward has its own suites and bounds.

1. Bit for bit: the integer cases at both sides of a lane pair, a wave and the 512-symbol block.      2. Bounded: real tables under
the derived bound.      3. Zero weights, bad frames, reproducibility.      4. Refusals.      5. Autograd, the chain, hipGraph.
6. The attack on the 20 dB decision set.
(The timing is scripts/likelihood_bwd_prof.py -> profiles/likelihood_bwd.txt; nothing is asserted about it.)
"""
import ctypes

import numpy as np
import pytest
import torch

import likelihood_bwd_ref as G
import likelihood_em_ref as EM
import likelihood_ref as R
from frontend_gpu import SENTINEL, abi_call, bits, dev, on_device, same_bits
from prof_names import kernel_launches

pytestmark = pytest.mark.gpu

MODES = ("max", "mean")


def _shape(x, planar):
    x = np.asarray(x, dtype=np.float32)
    return x, x.shape[0], x.shape[2] if planar else x.shape[1]


def _class_array(classes):
    import vit_vs_raw_iq_amd._native as N
    return (N.SynthClass * len(classes))(*[N.SynthClass(0, int(o), int(m)) for o, m in classes])


def lik_fwd(x, sigma2, gain, points, classes, rot, mode, planar=0):
    """One guarded iq_frames_likelihood call -> (loglik (B, C), rot_ll (B, C, R) fp32, best_rot (B, C) int32): what the backward reads."""
    import vit_vs_raw_iq_amd._native as N
    x, B, length = _shape(x, planar)
    arr, Cn, Rn = _class_array(classes), len(classes), len(rot)
    sigma2 = np.broadcast_to(np.asarray(sigma2, np.float32), (B,))
    gain = None if gain is None else np.broadcast_to(np.asarray(gain, np.float32), (B,))
    par = lambda p, r, g: N.Likelihood(points=p, classes=arr, n_classes=Cn, rot=r, n_rot=Rn, planar=planar, mode=MODES.index(mode), gain=g)  # noqa: E731
    ll, L, best, _ = abi_call("iq_frames_likelihood", "frames_likelihood_kernel", (x, sigma2), [(B, Cn), (B, Cn, Rn), (np.int32, B, Cn), None],
                              B, length, par, side=(points, rot, gain))
    return ll, L, best


def lik_bwd(x, sigma2, gain, points, classes, rot, mode, dloglik, fwd, planar=0):
    """One guarded iq_frames_likelihood_bwd call on the forward outputs `fwd` = (loglik, rot_ll, best_rot) -> dx float64, x's layout."""
    import vit_vs_raw_iq_amd._native as N
    x, B, length = _shape(x, planar)
    arr, Cn, Rn = _class_array(classes), len(classes), len(rot)
    sigma2 = np.broadcast_to(np.asarray(sigma2, np.float32), (B,))
    gain = None if gain is None else np.broadcast_to(np.asarray(gain, np.float32), (B,))
    par = lambda p, r, g: N.Likelihood(points=p, classes=arr, n_classes=Cn, rot=r, n_rot=Rn, planar=planar, mode=MODES.index(mode), gain=g)  # noqa: E731
    ins = (x, sigma2, np.asarray(dloglik, np.float32), np.asarray(fwd[0], np.float32), np.asarray(fwd[1], np.float32), np.asarray(fwd[2], np.int32))
    return abi_call("iq_frames_likelihood_bwd", "frames_likelihood_bwd_kernel", ins, x.shape, B, length, par,
                    side=(points, rot, gain)).astype(np.float64)


def em_bwd(x, points, classes, dloglik, h, v, planar=0):
    """One guarded iq_frames_likelihood_em_bwd call -> dx float64, x's layout.  What the entry ignores is set to nonsense."""
    import vit_vs_raw_iq_amd._native as N
    x, B, length = _shape(x, planar)
    arr = _class_array(classes)
    par = lambda p: N.LikelihoodEm(points=p, classes=arr, n_classes=len(classes), starts=None, n_starts=-1, iters=-1, planar=planar,  # noqa: E731
                                   mode=9, f0=7.0, floor=-1.0, h0=None, v0=None)
    ins = (x, np.asarray(dloglik, np.float32), np.asarray(h, np.float32), np.asarray(v, np.float32))
    return abi_call("iq_frames_likelihood_em_bwd", "frames_likelihood_em_bwd_kernel", ins, x.shape, B, length, par,
                    side=(points,)).astype(np.float64)


def weights(B, Cn, seed):
    """dloglik with a zero in every frame (where there is more than one class) and values of both signs."""
    dl = np.random.default_rng(seed).standard_normal((B, Cn)).astype(np.float32)
    if Cn > 1:
        dl[np.arange(B), np.arange(B) % Cn] = 0.0
    return dl


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", G.EXACT_LENGTHS + (G.LONGEST,))
def test_integer_cases_are_exact(length):
    """tests/test_likelihood_bwd_cpu.py has shown that nothing rounds on these inputs: every class is copies of one point, so
    m = p exactly.  'max' on all classes; 'mean' on the class of the origin, whose four rotations tie (every share is 1/4); EM
    with h in {1, j, 2, 1/2} and v a power of two."""
    once = length == G.LONGEST
    for n_frames in ((1,) if once else (1, 3)):
        x, s2, gain = R.exact_case(n_frames, length, 10 * length + n_frames)
        dl = G.exact_weights(n_frames, 4, length + n_frames)
        only = np.zeros_like(dl)
        only[:, 3] = np.where(dl[:, 3] == 0, 1.0, dl[:, 3])
        xe = EM.exact_case(n_frames, length, 7 * length + n_frames, tiled=False)[0]
        h, v = G.exact_em_state(n_frames, 4, length)
        for planar in ((0,) if once else (0, 1)):
            xl = R.in_layout(x, planar)
            for g in ((gain,) if once else (None, gain)):
                tag = (length, n_frames, planar, g is not None)
                args = (xl, s2, g, R.EXACT_POINTS, R.EXACT_CLASSES, R.QUARTER_TURNS)
                fwd = lik_fwd(*args, "max", planar)
                want = G.likelihood_reference_bwd(*args, "max", dl, best_rot=fwd[2], planar=bool(planar))
                assert np.array_equal(lik_bwd(*args, "max", dl, fwd, planar), want) and np.any(want != 0), tag
                fwd = lik_fwd(*args, "mean", planar)
                want = G.likelihood_reference_bwd(*args, "mean", only, fwd[0], fwd[1], planar=bool(planar))
                assert np.array_equal(lik_bwd(*args, "mean", only, fwd, planar), want), tag
            xel = R.in_layout(xe, planar)
            want = G.likelihood_em_reference_bwd(xel, EM.EXACT_POINTS, EM.EXACT_CLASSES, dl, h, v, planar=bool(planar))
            assert np.array_equal(em_bwd(xel, EM.EXACT_POINTS, EM.EXACT_CLASSES, dl, h, v, planar), want) and np.any(want != 0), (length, planar)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bounded
# ---------------------------------------------------------------------------------------------------------------------------
def _sizes_case():
    """Classes of 1, 2, 64 and 256 points whose ranges lie out of order in one table; frames of the 64-point class."""
    sizes, order = [1, 2, 64, 256], [2, 0, 3, 1]
    table, classes, off = [], [None] * 4, 0
    for i in order:
        classes[i] = (off, sizes[i])
        table.append(R.random_table(sizes[i], 70 + i))
        off += sizes[i]
    points = np.concatenate(table)
    return points, classes, points[classes[2][0]:classes[2][0] + 64].astype(np.float64) @ np.array([1, 1j])


def _bounded_cases():
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    from vit_vs_raw_iq_amd.likelihood import rotation_table
    full = lambda Rn: rotation_table(2 * np.pi * np.arange(Rn) / Rn)                  # noqa: E731
    points, classes, frames_of = _sizes_case()
    yield "sizes_R4", points, classes, full(4), R.real_frames(2, G.REAL_LENGTH, frames_of, 15.0, 1, gain=0.7)[0], \
        np.array([1.0, 1e-3], np.float32), np.array([0.7, 0.7], np.float32)
    clf = LikelihoodClassifier(G.REAL_LENGTH)
    x, s2 = R.real_frames(2, G.REAL_LENGTH, "16QAM", 15.0, 4)
    yield "C17_R64", clf.points, [d[1:] for d in clf.descriptors], clf.rot, x, s2, None
    few = [clf.descriptors[i][1:] for i in (3, 12, 5)]                                # BPSK, 16QAM, 8PSK
    yield "C3_R1_two_blocks", clf.points, few, full(1), R.real_frames(2, G.BLOCK_EDGE_LENGTH, "8PSK", 10.0, 5)[0], \
        np.array([0.1, 1e-2], np.float32), None
    yield "C1_R4", clf.points, [clf.descriptors[4][1:]], full(4), R.real_frames(3, 65, "QPSK", 20.0, 6)[0], np.float32(0.01), None


def _within(got, want, E, tag):
    err = np.abs(got - want)
    print(f"{tag}: |dx - ref| / bound {float((err / E).max()):.4f} (bound up to {E.max():.2e}, |dx| up to {np.abs(want).max():.3g})")
    assert np.isfinite(got).all(), tag
    assert np.all(err <= E), tag
    return err


@pytest.mark.parametrize("case", list(_bounded_cases()), ids=lambda c: c[0])
def test_real_tables_stay_within_the_derived_bound(case):
    name, points, classes, rot, x, s2, gain = case
    dl = weights(len(x), len(classes), 3)
    for planar, mode in enumerate(MODES):                 # one layout per mode: the layouts differ in the loads only (test 1 has both)
        xl = R.in_layout(x, planar)
        fwd = lik_fwd(xl, s2, gain, points, classes, rot, mode, planar)
        want, E = G.likelihood_reference_bwd(xl, s2, gain, points, classes, rot, mode, dl, *fwd, planar=bool(planar), bound=True)
        err = _within(lik_bwd(xl, s2, gain, points, classes, rot, mode, dl, fwd, planar), want, E, f"{name} {mode}")
        assert np.any(err > 0)                            # (fp32 did round: the test is not vacuous)


def test_em_gradients_stay_within_the_derived_bound():
    """A given state per (frame, class) on the table of all sizes; and the device's own EM estimate through the class."""
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier
    points, classes, frames_of = _sizes_case()
    x = R.real_frames(2, G.REAL_LENGTH, frames_of, 15.0, 1, gain=0.7)[0]
    h, v = EM.given_start(x, points, classes, 9)
    dl = weights(2, 4, 4)
    want, E = G.likelihood_em_reference_bwd(x, points, classes, dl, h, v, bound=True)
    assert np.any(_within(em_bwd(x, points, classes, dl, h, v), want, E, "EM sizes") > 0)
    clf = HybridLikelihoodClassifier(G.BLOCK_EDGE_LENGTH, classes=["BPSK", "QPSK", "16QAM", "64QAM"], iters=8, layout="planar")
    x = R.in_layout(R.real_frames(2, G.BLOCK_EDGE_LENGTH, "16QAM", 12.0, 2, gain=2.5)[0], 1)
    _, hd, vd, _ = clf(on_device(x), return_estimates=True)
    hd, vd = hd.cpu().numpy(), vd.cpu().numpy()
    classes = [d[1:] for d in clf.descriptors]
    want, E = G.likelihood_em_reference_bwd(x, clf.points, classes, dl, hd, vd, planar=True, bound=True)
    got = em_bwd(x, clf.points, classes, dl, hd, vd, 1)
    assert np.any(_within(got, want, E, "EM C4 planar") > 0)
    assert np.array_equal(bits(clf.input_gradient(on_device(x), on_device(dl)).cpu().numpy()), bits(got))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. zero weights, bad frames, reproducibility
# ---------------------------------------------------------------------------------------------------------------------------
def _iso_case():
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    clf = LikelihoodClassifier(G.REAL_LENGTH, classes=["BPSK", "8PSK", "16QAM", "64QAM"], rotations=16)
    x, s2 = R.real_frames(3, G.REAL_LENGTH, "16QAM", 12.0, 8)
    return clf.points, [d[1:] for d in clf.descriptors], clf.rot, x, s2, np.array([1.0, 0.9, 1.1], np.float32)


@pytest.mark.parametrize("mode", MODES)
def test_a_class_with_weight_zero_is_not_read(mode):
    """The one-class gradient: NaN points, a NaN loglik and rot_ll and a best_rot of -1 in a class whose weight is 0 leave dx
    finite, and bit for bit what the classes asked about give without it."""
    points, classes, rot, x, s2, gain = _iso_case()
    dl = weights(3, 4, 5)
    dl[:, 1] = 0.0
    fwd = lik_fwd(x, s2, gain, points, classes, rot, mode)
    whole = lik_bwd(x, s2, gain, points, classes, rot, mode, dl, fwd)
    bad = points.copy()
    bad[classes[1][0]:classes[1][0] + classes[1][1]] = np.nan
    ll, L, best = (a.copy() for a in fwd)
    ll[:, 1], L[:, 1], best[:, 1] = np.nan, np.nan, -1
    got = lik_bwd(x, s2, gain, bad, classes, rot, mode, dl, (ll, L, best))
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(whole))
    keep = [0, 2, 3]
    part = lik_bwd(x, s2, gain, points, [classes[c] for c in keep], rot, mode, dl[:, keep], tuple(a[:, keep] for a in fwd))
    assert np.array_equal(bits(part), bits(whole))
    one = np.zeros_like(dl)
    one[:, 2] = 1.0                                       # d loglik[:, 2] / d x alone
    assert np.isfinite(lik_bwd(x, s2, gain, bad, classes, rot, mode, one, (ll, L, best))).all()
    assert not lik_bwd(x, s2, gain, bad, classes, rot, mode, np.zeros_like(dl), (ll, L, best)).any()
    # EM: a dead state with weight 0
    h, v = EM.given_start(x, points, classes, 3)
    base = em_bwd(x, points, classes, dl, h, v)
    h[:, 1], v[:, 1] = np.nan, np.nan
    assert np.array_equal(bits(em_bwd(x, bad, classes, dl, h, v)), bits(base)) and np.isfinite(base).all()


def test_a_frames_gradient_depends_on_neither_its_neighbours_nor_the_run():
    points, classes, rot, x, s2, gain = _iso_case()
    dl = weights(3, 4, 6)
    h, v = EM.given_start(x, points, classes, 4)
    fwd = lik_fwd(x, s2, gain, points, classes, rot, "mean")
    whole = lik_bwd(x, s2, gain, points, classes, rot, "mean", dl, fwd)
    whole_em = em_bwd(x, points, classes, dl, h, v)
    assert np.array_equal(bits(lik_bwd(x, s2, gain, points, classes, rot, "mean", dl, fwd)), bits(whole))          # run to run
    assert np.array_equal(bits(em_bwd(x, points, classes, dl, h, v)), bits(whole_em))
    for b in range(3):
        alone = lik_bwd(x[b:b + 1], s2[b:b + 1], gain[b:b + 1], points, classes, rot, "mean", dl[b:b + 1], tuple(a[b:b + 1] for a in fwd))
        assert np.array_equal(bits(alone), bits(whole[b:b + 1])), b
        assert np.array_equal(bits(em_bwd(x[b:b + 1], points, classes, dl[b:b + 1], h[b:b + 1], v[b:b + 1])), bits(whole_em[b:b + 1])), b
    # a neighbour whose variance the forward refuses: NaN there, not a bit elsewhere
    for bad in (0.0, np.nan, -1.0, np.inf):
        s2b = s2.copy()
        s2b[1] = bad
        for mode in MODES:
            f = lik_fwd(x, s2b, gain, points, classes, rot, mode)
            got = lik_bwd(x, s2b, gain, points, classes, rot, mode, dl, f)
            assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all(), (bad, mode)
            if mode == "mean":
                assert np.array_equal(bits(got[[0, 2]]), bits(whole[[0, 2]])), bad
    # a dead (h, v) somebody asked about: its own frame only
    for hb, vb in ((np.nan, 0.1), (0.5, np.nan), (0.5, 0.0), (np.inf, 0.1), (0.5, np.inf), (0.5, 1e-39)):
        h2, v2 = h.copy(), v.copy()
        h2[1, 3, 0], v2[1, 3] = hb, vb
        assert dl[1, 3] != 0
        got = em_bwd(x, points, classes, dl, h2, v2)
        assert np.isnan(got[1]).all() and np.array_equal(bits(got[[0, 2]]), bits(whole_em[[0, 2]])), (hb, vb)
    # a NaN sample stays in its symbol
    xb = x.copy()
    xb[2, 77, 0] = np.nan
    got = lik_bwd(xb, s2, gain, points, classes, rot, "mean", dl, fwd)
    assert np.isnan(got[2, 77]).all() and np.isfinite(np.delete(got[2], 77, axis=0)).all() and np.array_equal(bits(got[:2]), bits(whole[:2]))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier, LikelihoodClassifier
    lib = N.lib()
    ARG, UNSUPPORTED = 1, 2
    B, length = 2, 8192
    x = torch.zeros(B, length + 1, 2, device=dev())
    dx = torch.full((B, length + 1, 2), SENTINEL, device=dev())
    s2 = torch.ones(B, device=dev())
    points, rot = torch.zeros(2049, 2, device=dev()), torch.zeros(257, 2, device=dev())
    dl, ll, table = torch.ones(B, 65, device=dev()), torch.zeros(B, 65, device=dev()), torch.zeros(B, 65, 257, device=dev())
    best = torch.zeros(B, 65, dtype=torch.int32, device=dev())
    h, v = torch.ones(B, 65, 2, device=dev()), torch.ones(B, 65, device=dev())

    def classes_of(classes):
        return (N.SynthClass * len(classes))(*[N.SynthClass(*c) for c in classes])

    def lik(n=B, length=length, classes=((0, 0, 4),), par="ok", **kw):
        ptrs = dict(x=x.data_ptr(), sigma2=s2.data_ptr(), dloglik=dl.data_ptr(), loglik=ll.data_ptr(), rot_ll=table.data_ptr(),
                    best_rot=best.data_ptr(), dx=dx.data_ptr())
        ptrs.update({k: kw.pop(k) for k in list(kw) if k in ptrs})
        fields = dict(points=points.data_ptr(), classes=classes_of(classes), n_classes=len(classes), rot=rot.data_ptr(), n_rot=64, planar=0,
                      mode=0, gain=None)
        p = None if par is None else N.Likelihood(**{**fields, **kw})
        return lib.iq_frames_likelihood_bwd(*ptrs.values(), n, length, ctypes.byref(p) if p is not None else None, N.stream_handle())

    def em(n=B, length=length, classes=((0, 0, 4),), par="ok", **kw):
        ptrs = dict(x=x.data_ptr(), dloglik=dl.data_ptr(), h=h.data_ptr(), v=v.data_ptr(), dx=dx.data_ptr())
        ptrs.update({k: kw.pop(k) for k in list(kw) if k in ptrs})
        fields = dict(points=points.data_ptr(), classes=classes_of(classes), n_classes=len(classes), starts=None, n_starts=0, iters=-1,
                      planar=0, mode=5, f0=3.0, floor=-1.0, h0=None, v0=None)
        p = None if par is None else N.LikelihoodEm(**{**fields, **kw})
        return lib.iq_frames_likelihood_em_bwd(*ptrs.values(), n, length, ctypes.byref(p) if p is not None else None, N.stream_handle())

    def refused():
        for call, required in ((lik, ("x", "sigma2", "dloglik", "dx", "points", "rot")), (em, ("x", "dloglik", "h", "v", "dx", "points"))):
            for name in required:
                assert call(**{name: None}) == ARG, name
            assert call(par=None) == ARG and call(length=0) == ARG and call(planar=2) == ARG
            assert call(x=x.data_ptr() + 4) == ARG and call(dx=dx.data_ptr() + 4) == ARG and call(dx=dx.data_ptr() + 2, planar=1) == ARG
            assert call(points=points.data_ptr() + 4) == ARG and call(dloglik=dl.data_ptr() + 2) == ARG
            assert call(classes=((1, 0, 4),)) == ARG and call(classes=((0, 0, 0),)) == ARG and call(classes=((0, -1, 4),)) == ARG
            # one past every limit
            assert call(classes=tuple((0, i, 1) for i in range(65))) == UNSUPPORTED
            assert call(classes=((0, 0, 2049),)) == UNSUPPORTED and call(length=8193) == UNSUPPORTED
            assert call(n=0) == 0 and call(n=-2) == 0                                          # nothing to do
        assert lik(n_rot=0) == ARG and lik(mode=2) == ARG and lik(mode=-1) == ARG and lik(n_rot=257) == UNSUPPORTED
        assert lik(best_rot=None, mode=0) == ARG and lik(loglik=None, mode=1) == ARG and lik(rot_ll=None, mode=1) == ARG
        assert lik(rot_ll=table.data_ptr() + 2) == ARG and lik(gain=s2.data_ptr() + 1) == ARG
        assert em(h=h.data_ptr() + 4) == ARG and em(v=v.data_ptr() + 2) == ARG
    assert kernel_launches(lib, refused) == {}                                                # not one launch
    torch.cuda.synchronize()
    assert torch.equal(dx, torch.full_like(dx, SENTINEL))
    # the limits themselves run, with what a mode does not read left out: 64 classes, 256 rotations, a 2048-point class, MAX_LENGTH
    many = tuple((0, i, 1) for i in range(64))
    assert lik(classes=many, n_rot=2, length=64, loglik=None, rot_ll=None) == 0 and em(classes=many, length=64) == 0
    assert lik(n_rot=256, length=64, mode=1, best_rot=None) == 0 and lik(classes=((0, 0, 2048),), n_rot=1, length=64) == 0
    assert em(classes=((0, 0, 2048),), length=64) == 0 and lik(n_rot=1) == 0 and em() == 0
    torch.cuda.synchronize()
    flat = dx.view(-1)                                                                        # B frames of 8192 of the buffer's 8193 rows
    assert not bool(flat[:B * length * 2].any()) and bool((flat[B * length * 2:] == SENTINEL).all())  # (all-zero frames and tables: dx = 0)
    for clf, noise in ((LikelihoodClassifier(8, classes=["BPSK"]), dict(sigma2=1.0)), (HybridLikelihoodClassifier(8, classes=["BPSK"]), {})):
        assert clf.input_gradient(torch.zeros(0, 8, 2, device=dev()), torch.zeros(0, 1, device=dev()), **noise).shape == (0, 8, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. autograd, the chain, hipGraph
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_autograd_equals_input_gradient_equals_the_two_calls_by_hand(mode):
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    names = ["BPSK", "QPSK", "16QAM", "32APSK"]
    layout = "planar" if mode == "mean" else "frames"
    clf = LikelihoodClassifier(G.REAL_LENGTH, classes=names, rotations=16, mode=mode, layout=layout, differentiable=True)
    plain = LikelihoodClassifier(G.REAL_LENGTH, classes=names, rotations=16, mode=mode, layout=layout)
    xs, s2 = R.real_frames(3, G.REAL_LENGTH, "16QAM", 14.0, 2, gain=0.9)
    xs = R.in_layout(xs, clf.planar)
    dl = weights(3, 4, 7)
    x = on_device(xs).requires_grad_()
    gain = torch.full((3,), 0.9, device=dev())
    ll, table, best = clf(x, sigma2=s2, gain=gain, return_rot=True, return_best=True)
    assert ll.requires_grad and not table.requires_grad and not best.requires_grad and best.dtype == torch.int32
    for a, b in zip((ll, table, best), plain(x, sigma2=s2, gain=gain, return_rot=True, return_best=True)):
        assert torch.equal(a.detach(), b) and not b.requires_grad                          # the default detaches, as it did
    (dx,) = torch.autograd.grad(ll, x, on_device(dl))
    again = clf(x, sigma2=s2, gain=gain)                                                   # no extras asked for: a bare tensor
    assert isinstance(again, torch.Tensor) and same_bits(torch.autograd.grad(again, x, on_device(dl))[0], dx)
    for c in (clf, plain):
        assert same_bits(c.input_gradient(x, on_device(dl), sigma2=s2, gain=gain), dx)
    classes = [d[1:] for d in clf.descriptors]
    fwd = lik_fwd(xs, s2, np.float32(0.9), clf.points, classes, clf.rot, mode, clf.planar)
    assert np.array_equal(bits(fwd[0]), bits(ll.detach().cpu().numpy()))
    hand = lik_bwd(xs, s2, np.float32(0.9), clf.points, classes, clf.rot, mode, dl, fwd, clf.planar)
    assert np.array_equal(bits(hand), bits(dx.cpu().numpy())) and float(dx.abs().max()) > 0


def test_hybrid_autograd_equals_input_gradient_equals_the_two_calls_by_hand():
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier
    names = ["BPSK", "QPSK", "16QAM"]
    clf = HybridLikelihoodClassifier(G.REAL_LENGTH, classes=names, iters=8, differentiable=True)
    plain = HybridLikelihoodClassifier(G.REAL_LENGTH, classes=names, iters=8)
    xs = R.real_frames(3, G.REAL_LENGTH, "QPSK", 12.0, 3, gain=1.7)[0]
    dl = weights(3, 3, 8)
    x = on_device(xs).requires_grad_()
    lam, h, v, best, starts = clf(x, return_estimates=True, return_starts=True)
    assert lam.requires_grad and not any(t.requires_grad for t in (h, v, best, starts))
    for a, b in zip((lam, h, v, best, starts), plain(x, return_estimates=True, return_starts=True)):
        assert torch.equal(a.detach(), b) and not b.requires_grad
    (dx,) = torch.autograd.grad(lam, x, on_device(dl))
    for c in (clf, plain):
        assert same_bits(c.input_gradient(x, on_device(dl)), dx)
    hand = em_bwd(xs, clf.points, [d[1:] for d in clf.descriptors], dl, h.cpu().numpy(), v.cpu().numpy())
    assert np.array_equal(bits(hand), bits(dx.cpu().numpy())) and float(dx.abs().max()) > 0
    # a warm start goes the same way
    lam2 = clf(x, h0=h, v0=v)
    assert same_bits(torch.autograd.grad(lam2, x, on_device(dl))[0], clf.input_gradient(x, on_device(dl), h0=h, v0=v))


def test_gradients_reach_the_raw_frame_through_receiver_and_carrier():
    """ShapedSynth -> Receiver -> Carrier -> classifier: x.grad of the raw frame is the chained adjoint calls, bit for bit."""
    from vit_vs_raw_iq_amd import Carrier, HybridLikelihoodClassifier, LikelihoodClassifier, Receiver, ShapedSynth, noise_for
    names = ["BPSK", "QPSK", "16QAM"]
    ws = ShapedSynth(names, snrs_db=(20.0,), length=1024, seed=11, sps=2, device=dev())
    raw, y, z = ws.generate(6, 0, 0)
    rx, cr = Receiver.for_synth(ws, timing="energy"), Carrier(512, order=4, layout="interleaved")
    gain, s2 = noise_for(z, normalised=True)
    dl = on_device(weights(6, 3, 9))
    for clf, noise in ((LikelihoodClassifier(512, classes=names, mode="mean", differentiable=True), dict(sigma2=s2, gain=gain)),
                       (HybridLikelihoodClassifier(512, classes=names, iters=8, differentiable=True), {})):
        x = raw.clone().requires_grad_()
        sym = cr(rx(x))
        ll = clf(sym, **noise)
        dsym = clf.input_gradient(sym.detach(), dl, **noise)
        (want,) = torch.autograd.grad(sym, x, dsym, retain_graph=True)
        ll.backward(dl)
        assert same_bits(x.grad, want) and float(x.grad.abs().max()) > 0 and bool(torch.isfinite(x.grad).all())


def test_a_captured_attack_step_replays_as_eager():
    """A capture fails on any host synchronisation: forward, margin weights, backward and the L-infinity step are captured whole."""
    import vit_vs_raw_iq_amd.adversarial as A
    from vit_vs_raw_iq_amd import LikelihoodClassifier, fgsm
    clf = LikelihoodClassifier(G.REAL_LENGTH, classes=["QPSK", "16QAM", "32APSK"], rotations=32, mode="mean")
    x0 = on_device(R.real_frames(5, G.REAL_LENGTH, "16QAM", 15.0, 3)[0])
    y = torch.ones(5, dtype=torch.int64, device=dev())
    s2 = torch.full((5,), 0.03, device=dev())
    eager = fgsm(clf, x0, y, 0.05, sigma2=s2)             # also: the tables are on the device before the capture
    assert float((eager - x0).abs().max()) == pytest.approx(0.05, rel=1e-5)
    xa = x0.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    nan = float("nan")
    with torch.cuda.graph(graph):
        A._clf_attack(clf, x0, y, (s2, None), 0.05, 0.05, 1, xa, nan, nan, 256, "margin")
    xa.copy_(x0)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(xa, eager)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the attack
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attacked():
    """fgsm on the decision set at eps 0.05 with the margin loss, and the definition on the very frames it returned (one fp64
    pass with the forward bound over the 68 frames: computed once for the tests below)."""
    from vit_vs_raw_iq_amd import LikelihoodClassifier, fgsm
    clf = LikelihoodClassifier(128)
    X, Y, s2 = R.decision_set()
    xd, yd = on_device(X), torch.from_numpy(np.array(Y)).to(dev())
    x_adv = fgsm(clf, xd, yd, G.FGSM_EPS, sigma2=float(s2))
    ref = R.reference_and_bound(x_adv.cpu().numpy(), s2, None, clf.points, [d[1:] for d in clf.descriptors], clf.rot, "max")
    return dict(clf=clf, xd=xd, yd=yd, x_adv=x_adv, ref=ref)


def test_the_devices_gradient_of_the_margin_is_the_definitions(attacked):
    """The margin weights from the device's own loglik; the definition at the device's own best_rot: within the bound, and of
    the same sign wherever the definition's |g| exceeds the bound; one FGSM step is x + eps sign(g), rounded once."""
    clf, xd = attacked["clf"], attacked["xd"]
    X, Y, s2 = R.decision_set()
    ll, best = clf(xd, sigma2=float(s2), return_best=True)
    dl = G.margin_weights(ll.cpu().numpy(), Y)
    assert np.array_equal(np.sort(dl, axis=1)[:, [0, -1]], np.tile([-1.0, 1.0], (68, 1))) and np.count_nonzero(dl) == 136
    g = clf.input_gradient(xd, on_device(dl), sigma2=float(s2)).cpu().numpy().astype(np.float64)
    want, E = G.likelihood_reference_bwd(X, s2, None, clf.points, [d[1:] for d in clf.descriptors], clf.rot, "max", dl,
                                         best_rot=best.cpu().numpy(), bound=True)
    _within(g, want, E, "margin gradient")
    sure = np.abs(want) > E
    assert sure.mean() > 0.7 and np.array_equal(np.sign(g[sure]), np.sign(want[sure]))
    step = X + np.float32(G.FGSM_EPS) * np.sign(g).astype(np.float32)                     # (fp32, as iq_linf_step adds it)
    assert np.array_equal(bits(attacked["x_adv"].cpu().numpy()), bits(step))


def test_the_attacked_frames_are_decided_as_the_definition_decides_them(attacked):
    """Wherever the definition's margin on an attacked frame exceeds twice the forward bound the device decides as it does; the
    attack takes more decisions away than random signs of the same size."""
    clf, ref = attacked["clf"], attacked["ref"]
    X, Y, s2 = R.decision_set()
    pred = clf.predict(attacked["x_adv"], sigma2=float(s2)).cpu().numpy()
    decided = R.margin(ref["loglik"]) > 2.0 * ref["Ell"].max(axis=1)
    assert decided.mean() > 0.9 and np.array_equal(pred[decided], ref["pred"][decided])
    rand = on_device(G.host_fgsm()["x_rand"])
    acc_adv, acc_rand = float(np.mean(pred == Y)), float(np.mean(clf.predict(rand, sigma2=float(s2)).cpu().numpy() == Y))
    print(f"eps {G.FGSM_EPS}: device FGSM accuracy {acc_adv:.3f}, random signs {acc_rand:.3f}")
    assert acc_adv < acc_rand


def test_pgd_of_one_step_is_fgsm_and_the_curve_starts_at_the_clean_accuracy(attacked):
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier, fgsm, pgd, robustness_curve
    clf, xd, yd = attacked["clf"], attacked["xd"], attacked["yd"]
    _, Y, s2 = R.decision_set()
    assert same_bits(pgd(clf, xd, yd, G.FGSM_EPS, G.FGSM_EPS, 1, sigma2=float(s2)), attacked["x_adv"])
    assert same_bits(fgsm(clf, xd, yd, G.FGSM_EPS, snr_db=R.DECISION_SNR_DB, batch=20), attacked["x_adv"])        # chunks of 20 frames
    curve = robustness_curve(clf, xd, yd, [0.0, G.FGSM_EPS], sigma2=float(s2))
    assert curve[0] == 1.0 and curve[1] == float(np.mean(clf.predict(attacked["x_adv"], sigma2=float(s2)).cpu().numpy() == Y))
    # the cross entropy through iq_ce_fwd_bwd, and the hybrid in place of the classifier: the ball is kept, and two runs agree
    ce = pgd(clf, xd[:8], yd[:8], 0.02, 0.01, 3, sigma2=float(s2), loss="ce", random_start=True, seed=1)
    ball = 0.02 + 2.0 ** -24 * (float(xd[:8].abs().max()) + 0.02)                         # (x0 +- eps is rounded once, in fp32)
    assert float((ce - xd[:8]).abs().max()) <= ball and same_bits(ce, pgd(clf, xd[:8], yd[:8], 0.02, 0.01, 3, sigma2=float(s2), loss="ce", random_start=True, seed=1))
    hyb = HybridLikelihoodClassifier(128, classes=clf.class_names[:8], iters=8)
    adv = fgsm(hyb, xd[:8], yd[:8].clamp(max=7), 0.05)
    assert float((adv - xd[:8]).abs().max()) == pytest.approx(0.05, rel=1e-5) and bool(torch.isfinite(adv).all())
    assert robustness_curve(hyb, xd[:8], yd[:8].clamp(max=7), [0.0])[0] == float(np.mean(hyb.predict(xd[:8]).cpu().numpy() == Y[:8].clip(max=7)))
