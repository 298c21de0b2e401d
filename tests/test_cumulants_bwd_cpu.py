"""Host only: the fp64 definition of the cumulant classifier's gradient (cumulants_reference_bwd) against torch autograd of a plain
statement of the forward, the zero rules, the refused frames, the ctypes binding against include/iqvit.h, every refusal of
iq_frames_cumulants_bwd that returns before a HIP call, the differentiable= / input_gradient / attack / transfer_table argument
checks with the unchanged default, the inputs of the GPU suite (exact where claimed, the bound following the definition and
small enough to be a check) and the host FGSM table of the decision set."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cumulants_bwd_ref as G
import cumulants_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["BPSK", "QPSK", "8PSK", "16QAM", "64QAM"]


def tables(length=64):
    from vit_vs_raw_iq_amd import CumulantClassifier
    clf = CumulantClassifier(length, classes=NAMES)
    return clf.mu, clf.w, clf.bias


def test_torch_statement_is_the_definition():
    """The fp64 torch statement of the forward formulas is pinned to cumulants_reference: 1.5e-11 at worst on these sets (the
    shortest frames with half their variance taken as noise, where P is small and the features large)."""
    from vit_vs_raw_iq_amd import cumulants_reference
    mu, w, bias = tables()
    worst = 0.0
    for length in (2, 3, 64, 257):
        x, s2 = R.real_frames(8, length, "16QAM", 10, seed=length)
        for sig in (None, 0.5 * s2):
            feat, score = G.torch_forward(torch.tensor(x.astype(np.float64)), sig, mu, w, bias)
            f0, _, s0, _ = cumulants_reference(x, sig, mu, w, bias)
            ok = ~np.isnan(f0[:, 0])
            assert ok.sum() >= 6
            worst = max(worst, np.abs(feat.numpy() - f0)[ok].max(), (np.abs(score.numpy() - s0) / (1 + np.abs(s0)))[ok].max())
    print(f"torch statement against cumulants_reference: {worst:.2e}")
    assert worst < 1e-10


@pytest.mark.parametrize("length", [2, 3, 64, 257])
def test_definition_is_autograd_of_the_plain_statement(length):
    """dscore alone, dfeat alone and both; blind and with sigma2; both layouts."""
    from vit_vs_raw_iq_amd import cumulants_reference, cumulants_reference_bwd
    mu, w, bias = tables()
    x, s2 = R.real_frames(8, length, "16QAM", 10, seed=length)
    ds, df = G.cotangents(8, 5, 3, sparse=False)
    for sig in (None, 0.5 * s2):
        ok = ~np.isnan(cumulants_reference(x, sig)[0][:, 0])
        assert ok.sum() >= 6
        for dscore, dfeat in ((ds, None), (None, df), (ds, df)):
            xt = torch.tensor(x.astype(np.float64), requires_grad=True)
            feat, score = G.torch_forward(xt, sig, mu, w, bias)
            loss = 0.0
            if dscore is not None:
                loss = loss + (torch.tensor(dscore.astype(np.float64)) * score)[torch.tensor(ok)].sum()
            if dfeat is not None:
                loss = loss + (torch.tensor(dfeat.astype(np.float64)) * feat)[torch.tensor(ok)].sum()
            want = torch.autograd.grad(loss, xt)[0].numpy()
            for planar in (False, True):
                dx = cumulants_reference_bwd(R.in_layout(x, planar), dscore, dfeat, sig, mu, w, bias, planar=planar)
                assert dx.shape == R.in_layout(x, planar).shape and dx.dtype == np.float64
                dx = np.transpose(dx, (0, 2, 1)) if planar else dx
                assert np.isnan(dx[~ok]).all() and np.abs(dx[ok]).max() > 1e-3
                assert np.abs(dx[ok] - want[ok]).max() <= 1e-11 * np.abs(want[ok]).max()


def test_zero_rules():
    """A clean 8PSK frame has |C40| = 0 exactly in the fp32 restatement of an integer frame and ~1e-17 in fp64: the gradient is
    finite.  A class of weight 0 with NaN mu is inert: the gradient is that of the classes asked about, bit for bit."""
    from vit_vs_raw_iq_amd import cumulants_reference_bwd
    from vit_vs_raw_iq_amd import data as D
    mu, w, bias = tables()
    pts = D.constellation("8PSK")
    y = np.tile(pts, 8)
    x = np.stack([y.real, y.imag], axis=1)[None]
    df = np.ones((1, 10))
    dx = cumulants_reference_bwd(x, None, df)
    assert np.isfinite(dx).all() and np.abs(dx).max() > 0.1
    # an exact zero: the four points of a square have C41 = C61 = 0 and M20 = 0 exactly
    sq = np.array([[[1, 1], [-1, 1], [-1, -1], [1, -1]]], np.float64)
    dx = cumulants_reference_bwd(sq, None, df)
    assert np.isfinite(dx).all()
    x, _ = R.real_frames(4, 64, "QPSK", 10, seed=1)
    ds, _ = G.cotangents(4, 5, 2, sparse=False)
    ds[:, 2] = 0
    whole = cumulants_reference_bwd(x, ds, None, None, mu, w, bias)
    mu2 = mu.copy()
    mu2[2] = np.nan
    assert np.isfinite(whole).all() and np.array_equal(cumulants_reference_bwd(x, ds, None, None, mu2, w, bias), whole)
    keep = [0, 1, 3, 4]
    assert np.array_equal(cumulants_reference_bwd(x, ds[:, keep], None, None, mu[keep], w[keep], bias[keep]), whole)
    ds[1, 2] = 1.0                                        # asked about: its own frame only
    bad = cumulants_reference_bwd(x, ds, None, None, mu2, w, bias)
    assert np.isnan(bad[1]).all() and np.array_equal(bad[[0, 2, 3]], whole[[0, 2, 3]])
    with pytest.raises(ValueError):
        cumulants_reference_bwd(x)
    with pytest.raises(ValueError):
        cumulants_reference_bwd(x, ds)                    # dscore without mu


def test_a_refused_p_is_nan_in_that_frame_only():
    from vit_vs_raw_iq_amd import cumulants_reference_bwd
    x, s2 = R.real_frames(3, 32, "QPSK", 10, seed=2)
    df = np.ones((3, 10))
    base = cumulants_reference_bwd(x, None, df)
    assert np.isnan(cumulants_reference_bwd(x[:, :1], None, df)).all()                       # len = 1
    z = x.copy()
    z[1] = 0
    got = cumulants_reference_bwd(z, None, df)
    assert np.isnan(got[1]).all() and np.array_equal(got[[0, 2]], base[[0, 2]])
    sig = np.array([0.0, 5.0, 0.0])                                                          # above the variance
    got = cumulants_reference_bwd(x, None, df, sig)
    assert np.isnan(got[1]).all() and np.array_equal(got[[0, 2]], base[[0, 2]])
    z = x.copy()
    z[2, 5, 0] = np.nan
    got = cumulants_reference_bwd(z, None, df)
    assert np.isnan(got[2]).all() and np.array_equal(got[[0, 1]], base[[0, 1]])


def test_binding_matches_the_header():
    import vit_vs_raw_iq_amd._native as N
    text = open(os.path.join(ROOT, "include", "iqvit.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"int iq_frames_cumulants_bwd\((.*?)\);", src, flags=re.S).group(1)
    res, args = N.SIGNATURES["iq_frames_cumulants_bwd"]
    assert len(decl.split(",")) == len(args) == 8 and res is ctypes.c_int
    assert "const iq_cumulants_t* par" in decl and args[-2] is ctypes.POINTER(N.Cumulants) and args[-4:-2] == [ctypes.c_int] * 2
    assert all(a is ctypes.c_void_p for a in args[:-4] + args[-1:])
    assert hasattr(N.lib(), "iq_frames_cumulants_bwd")
    assert ctypes.sizeof(N.Cumulants) == 48 and len(N.SIGNATURES["iq_frames_cumulants"][1]) == 9       # the forward's stay
    assert "There is no backward" not in text and "iq_frames_cumulants_bwd (below)" in text
    kernel = open(os.path.join(ROOT, "vit-vs-raw-iq_amd", "csrc", "cumulants_bwd.hip")).read()
    assert re.search(r"CUM_WAVE_LEN = 256;", kernel) and '#include "cumulants_common.h"' in kernel


def test_every_refusal_returns_before_a_hip_call():
    """Pointers that are never dereferenced: a refusal looks at their value only."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    ARG, UNSUPPORTED = 1, 2
    A = 0x10000                                            # "an aligned pointer"

    def call(x=A, dscore=A, dfeat=A, dx=A, n=1, length=512, par="ok", **fields):
        ok = dict(planar=0, sigma2=A, mu=A, w=A, bias=A, n_classes=17)
        p = None if par is None else N.Cumulants(**{**ok, **fields})
        return L.iq_frames_cumulants_bwd(x, dscore, dfeat, dx, n, length, ctypes.byref(p) if p is not None else None, None)
    # (a valid call with n = 1 would launch: none is made here)
    assert call(x=None) == ARG and call(dx=None) == ARG and call(par=None) == ARG and call(dscore=None, dfeat=None) == ARG
    assert call(length=0) == ARG and call(length=-4) == ARG and call(planar=2) == ARG and call(planar=-1) == ARG
    assert call(n_classes=-1) == ARG and call(mu=None) == ARG and call(w=None) == ARG
    assert call(n_classes=0) == ARG and call(n_classes=0, mu=None, w=None) == ARG            # dscore without classes
    assert call(x=A + 4) == ARG and call(dx=A + 4) == ARG and call(x=A + 2, planar=1) == ARG and call(dx=A + 2, planar=1) == ARG
    for name in ("dscore", "dfeat", "sigma2", "mu", "w", "bias"):
        assert call(**{name: A + 2}) == ARG, name
    assert call(n_classes=65) == UNSUPPORTED and call(n_classes=64, n=0) == 0
    assert call(length=8193) == UNSUPPORTED and call(length=8192, n=0) == 0
    assert call(n=2 ** 31 // 20 + 1, dscore=None, n_classes=0, mu=None, w=None) == UNSUPPORTED         # n * 20 past the int range
    assert call(n=2 ** 31 // 64 + 1, n_classes=64) == UNSUPPORTED
    assert call(n_classes=65, planar=3) == ARG and call(length=8193, x=None) == ARG                    # ARG comes first
    for n in (0, -3):
        assert call(n=n) == 0 and call(n=n, dscore=None, sigma2=None, bias=None, planar=1) == 0
        assert call(n=n, dfeat=None) == 0 and call(n=n, dscore=None, n_classes=0, mu=None, w=None, bias=None) == 0
        assert call(n=n, x=A + 4, dx=A + 4, planar=1) == 0


def test_differentiable_argument_input_gradient_and_the_unchanged_default():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import CumulantClassifier
    for bad in (2, "yes", None, 1.0):
        with pytest.raises(TypeError):
            CumulantClassifier(64, differentiable=bad)
    plain, on = CumulantClassifier(64, classes=NAMES[:2]), CumulantClassifier(64, classes=NAMES[:2], differentiable=True)
    assert plain.differentiable is False and on.differentiable is True
    assert "differentiable" not in repr(plain) and repr(on) == repr(plain)[:-1] + ", differentiable=True)"
    assert CumulantClassifier(64, None, "planar").planar == 1                               # the positional order stays
    x = torch.zeros(2, 64, 2, requires_grad=True)
    for clf in (plain, on):
        for call in (lambda: clf(x), lambda: clf.features(x, sigma2=0.1), lambda: clf.input_gradient(x, torch.zeros(2, 2)),
                     lambda: clf.input_gradient(x, dfeat=torch.zeros(2, 10), snr_db=10.0)):
            with pytest.raises(P.IqError, match="no CPU fallback"):
                call()
        with pytest.raises(ValueError):
            clf.input_gradient(x)                                                            # neither gradient
        with pytest.raises(ValueError):
            clf.input_gradient(torch.zeros(2, 63, 2), torch.zeros(2, 2))
        with pytest.raises(ValueError):
            clf.input_gradient(x, torch.zeros(2, 2), sigma2=0.1, snr_db=3.0)
        for bad, exc in ((torch.zeros(2, 3), ValueError), (torch.zeros(3, 2), ValueError), (np.zeros((2, 2)), TypeError),
                         (torch.zeros(2, 2, dtype=torch.bool), TypeError)):
            with pytest.raises(exc):
                clf.input_gradient(x, bad)
        for bad, exc in ((torch.zeros(2, 9), ValueError), (np.zeros((2, 10)), TypeError)):
            with pytest.raises(exc):
                clf.input_gradient(x, dfeat=bad)
    # a class without a description: the scores are refused, the features are not
    shaped = CumulantClassifier(64, classes=["BPSK", "GMSK"], differentiable=True)
    with pytest.raises(ValueError, match="fit"):
        shaped.input_gradient(x, torch.zeros(2, 2))
    with pytest.raises(P.IqError, match="no CPU fallback"):
        shaped.input_gradient(x, dfeat=torch.zeros(2, 10))


def test_attack_argument_checks():
    """fgsm / pgd / robustness_curve with the cumulant classifier in place of a model: everything is refused before the device,
    a CPU frame last; the noise is optional (blind), gain= is refused in the classifier's own words."""
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import CumulantClassifier, fgsm, pgd, robustness_curve
    clf = CumulantClassifier(64, classes=NAMES[:2])
    x, y = torch.zeros(2, 64, 2), torch.tensor([0, 1])
    with pytest.raises(ValueError, match="loss"):
        fgsm(clf, x, y, 0.1, loss="hinge")
    with pytest.raises(ValueError):
        fgsm(clf, x, torch.tensor([0, 2]), 0.1)                                              # a label out of range
    with pytest.raises(ValueError):
        fgsm(CumulantClassifier(64, classes=["BPSK"]), x, torch.tensor([0, 0]), 0.1)         # a margin needs two classes
    with pytest.raises(ValueError):
        fgsm(clf, x, y, 0.1, sigma2=0.1, snr_db=3.0)
    with pytest.raises(ValueError):
        fgsm(clf, torch.zeros(2, 2, 64), y, 0.1)                                             # the other layout
    with pytest.raises(ValueError, match="fit"):
        fgsm(CumulantClassifier(64, classes=["BPSK", "OQPSK"]), x, y, 0.1)
    for call in (lambda: fgsm(clf, x, y, 0.1, gain=1.0), lambda: pgd(clf, x, y, 0.1, 0.05, 2, gain=1.0),
                 lambda: robustness_curve(clf, x, y, [0.1], gain=1.0)):
        with pytest.raises(TypeError, match="CumulantClassifier takes the noise as sigma2= or snr_db="):
            call()
    with pytest.raises(ValueError):
        pgd(clf, x, y, 0.1, 0.05, 0)
    with pytest.raises(TypeError):
        robustness_curve(clf, x, y, [0.0], steps=3)                                          # a pgd keyword under fgsm
    for call in (lambda: fgsm(clf, x, y, 0.1), lambda: fgsm(clf, x, y, 0.1, sigma2=0.1), lambda: pgd(clf, x, y, 0.1, 0.05, 2, snr_db=10.0, loss="ce"),
                 lambda: robustness_curve(clf, x, y, [0.0, 0.1], sigma2=[0.1, 0.2])):
        with pytest.raises(P.IqError, match="no CPU fallback"):
            call()


def test_transfer_table_argument_checks():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import CumulantClassifier, HybridLikelihoodClassifier, LikelihoodClassifier, transfer_table
    cum, lik, em = (cls(64, classes=NAMES[:2]) for cls in (CumulantClassifier, LikelihoodClassifier, HybridLikelihoodClassifier))
    x, y = torch.zeros(2, 64, 2), torch.tensor([0, 1])
    ok = [cum, (lik, dict(sigma2=0.1)), em]
    with pytest.raises(ValueError, match="attack"):
        transfer_table(ok, ok, x, y, 0.1, attack="cw")
    with pytest.raises(ValueError):
        transfer_table(ok, ok, x, y, -0.1)
    with pytest.raises(ValueError):
        transfer_table([], ok, x, y, 0.1)
    with pytest.raises(ValueError):
        transfer_table(ok, [], x, y, 0.1)
    with pytest.raises(TypeError):
        transfer_table(ok, ok, x, y, 0.1, steps=3)                                           # a pgd keyword under fgsm
    with pytest.raises(TypeError):
        transfer_table(ok, ok, x, y, 0.1, gain=1.0)                                          # noise goes with its classifier
    with pytest.raises(TypeError, match="a source"):
        transfer_table([lambda f: f], ok, x, y, 0.1)                                         # a callable cannot be attacked
    with pytest.raises(TypeError, match="a target"):
        transfer_table(ok, [3], x, y, 0.1)
    with pytest.raises(ValueError, match="share length and layout"):
        transfer_table(ok, [CumulantClassifier(65, classes=NAMES[:2])], x, y, 0.1)
    with pytest.raises(ValueError, match="share length and layout"):
        transfer_table([cum], [(LikelihoodClassifier(64, classes=NAMES[:2], layout="planar"), dict(sigma2=0.1))], x, y, 0.1)
    with pytest.raises(ValueError):
        transfer_table([cum], [lik], x, y, 0.1)                                              # the likelihood test needs its noise
    with pytest.raises(TypeError, match="CumulantClassifier takes the noise"):
        transfer_table([(cum, dict(gain=1.0))], [cum], x, y, 0.1)
    with pytest.raises(ValueError):
        transfer_table(ok, ok, x, torch.tensor([0, 5]), 0.1)
    for attack, kw in (("fgsm", {}), ("pgd", dict(steps=2, alpha=0.05, loss="ce"))):
        with pytest.raises(P.IqError, match="no CPU fallback"):
            transfer_table(ok, ok + [lambda f: f], x, y, 0.1, attack=attack, **kw)


def test_exact_cases_are_exact_where_claimed():
    """The forward sums of the integer frames are exact (restate_bwd_fp32 asserts it); the features formed from this module's
    cumulants are cumulants_ref.algebra's bit for bit; the restatement is the fp64 definition to fp32 rounding; span 1 leaves
    |C| = 0 exactly somewhere, so the zero rule is exercised; and `sum g` is not exact, so its order is modelled."""
    from vit_vs_raw_iq_amd import cumulants_reference_bwd
    for length, B, C, span in ((2, 3, 1, 2), (65, 5, 17, 2), (257, 3, 64, 1), (1025, 2, 0, 2), (8192, 1, 1, 1)):
        x = R.exact_case(B, length, length, span=span)
        mu, w, _ = R.exact_tables(max(C, 1), 2)
        ds, df = G.cotangents(B, C, 4)
        got = G.restate_bwd_fp32(x, ds, df, None, mu if C else None, w if C else None)
        want = cumulants_reference_bwd(x, ds, df, None, mu if C else None, w if C else None)
        assert got.dtype == np.float32 and np.isfinite(got).all() and np.any(got != 0)
        if length > 2:            # (two symbols +-v: every cumulant cancels to 0 or to rounding, and which decides the subgradient)
            assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
    x = R.exact_case(4, 64, 1, span=1)
    ref = R.restate_fp32(x)
    s = list(ref["mom"][:, 2:19].T)
    c = G.cumulants(R.F32, s)
    P, feat = R.algebra(R.F32, (ref["mom"][:, 0], ref["mom"][:, 1]), s, np.zeros(4, np.float32))
    assert np.array_equal(R.F32.div(R.F32.cabs(c["C40"]), R.F32.mul(P, P)), feat[2])
    assert np.array_equal(R.F32.div(c["C63"], R.F32.mul(R.F32.mul(P, P), P)), feat[8])
    assert any(np.any(R.F32.cabs(c[k]) == 0) for k in ("C41", "C61", "C40", "C80"))
    g = np.random.default_rng(0).standard_normal((2, 700)).astype(np.float32)
    for length in (200, 700):
        t = G.F32b.total(g[:, :length], length)
        assert t.dtype == np.float32 and np.abs(t - g[:, :length].astype(np.float64).sum(axis=1)).max() < 1e-4


def test_the_bound_follows_the_definition_and_is_small_enough_to_check():
    """The values the bound is carried with are cumulants_reference_bwd's; on every frame the GPU suite compares, the bound is at
    most COND = 0.05 of that frame's max |dx|; and no more than DECISION_SHARE of a set is left out."""
    from vit_vs_raw_iq_amd import cumulants_reference_bwd
    for case in G.REAL_CASES:
        for length in G.REAL_LENGTHS:
            x, s2, ds, df, mu, w, bias, ref = G.real_case(*case, length)
            use = ref["usable"]
            left_out = int((~use).sum())
            rel = (ref["Edx"].max(axis=(1, 2)) / ref["scale"])[use]
            print(f"{case} len {length}: left out {left_out} of {len(use)}, bound / scale median {np.median(rel):.1e} max {rel.max():.1e}")
            assert left_out <= R.DECISION_SHARE * len(use)
            assert rel.max() <= G.COND and np.all(ref["Edx"][use] > 0)
            want = cumulants_reference_bwd(x, ds, df, s2, mu, w, bias)
            assert np.abs(ref["dx"][use] - want[use]).max() <= 2.0 ** -29 * ref["scale"][use].max()


def test_host_fgsm_table_of_the_decision_set():
    """One signed step on the margin loss takes decisions away that random signs of the same size leave alone.  Measured here in
    fp64 at eps 0.05, known sigma2: clean 0.840, one signed step 0.227, random signs 0.820."""
    X, Y, _ = R.decision_set(G.FGSM_SNR)
    t = G.host_fgsm()
    assert np.abs(t["x_adv"].astype(np.float64) - X).max() <= G.FGSM_EPS + 2.0 ** -24 * np.abs(t["x_adv"]).max()
    assert np.isfinite(t["g"]).all() and np.mean(t["g"] != 0) > 0.9
    clean, adv, rand = G.host_accuracy(X), G.host_accuracy(t["x_adv"]), G.host_accuracy(t["x_rand"])
    print(f"eps {G.FGSM_EPS}: clean {clean:.3f}, FGSM {adv:.3f}, random signs {rand:.3f}")
    assert adv <= 0.5 * rand
