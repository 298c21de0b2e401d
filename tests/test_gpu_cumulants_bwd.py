"""iq_frames_cumulants_bwd on the MI355X (csrc/cumulants_bwd.hip) against tests/cumulants_bwd_ref.py: the integer cases bit for bit
against the fp32 restatement, real frames against the fp64 definition under the derived bound, masking and isolation, batch
invariance and run-to-run identity, the refusals, autograd = input_gradient = the ABI call, the chain down to the raw frame, a
captured attack step, and the attacks and the transfer table on the 20 dB decision set.  Every ABI call runs with dx between
sentinels and every operand between NaN guards.  (The timing is scripts/cumulants_bwd_prof.py -> profiles/cumulants_bwd.txt;
nothing is asserted about it.)"""
import ctypes

import numpy as np
import pytest
import torch

import cumulants_bwd_ref as G
import cumulants_ref as R
from frontend_gpu import SENTINEL, bits, dev, guarded, guards_intact, on_device, same_bits
from prof_names import kernel_launches

pytestmark = pytest.mark.gpu


def kernel_for(length):
    return "frames_cumulants_bwd_kernel<false>" if length <= R.WAVE_ROUTE_MAX else "frames_cumulants_bwd_kernel<true>"


def bwd(x, dscore=None, dfeat=None, sigma2=None, mu=None, w=None, planar=0, expect_kernel=True):
    """One guarded iq_frames_cumulants_bwd call on x (B, len, 2), laid out as `planar` says -> dx (B, len, 2) float32.  Every
    operand lies between NaN guards, dx between sentinels and pre-filled with the sentinel; afterwards every guard must be intact
    and every operand hold the bits it held.  With expect_kernel the call must launch exactly the instance of the length."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    x = np.asarray(x, dtype=np.float32)
    B, length = x.shape[:2]
    Cn = 0 if mu is None else len(mu)
    sigma2 = None if sigma2 is None else np.broadcast_to(np.asarray(sigma2, np.float32), (B,))
    ops = [None if a is None else guarded(a, np.nan) + (np.ascontiguousarray(a, dtype=np.float32),)
           for a in (R.in_layout(x, planar), dscore, dfeat, sigma2, mu, w)]
    ptr = [None if b is None else b[1].data_ptr() for b in ops]
    out, dx = guarded(np.full(x.shape, SENTINEL), SENTINEL)
    par = N.Cumulants(planar=planar, sigma2=ptr[3], mu=ptr[4], w=ptr[5], bias=None, n_classes=Cn)

    def run():
        N.check(L.iq_frames_cumulants_bwd(ptr[0], ptr[1], ptr[2], dx.data_ptr(), B, length, ctypes.byref(par), N.stream_handle()),
                "iq_frames_cumulants_bwd")
    if expect_kernel:
        assert kernel_launches(L, run) == {kernel_for(length): 1}
    else:
        run()
    torch.cuda.synchronize()
    assert guards_intact(out, SENTINEL)
    for buf, view, a in filter(None, ops):
        assert guards_intact(buf, np.nan) and np.array_equal(view.cpu().numpy().view(np.int32), a.reshape(-1).view(np.int32))
    got = dx.cpu().numpy().reshape((B, 2, length) if planar else (B, length, 2))
    assert not np.any(got == np.float32(SENTINEL))                                         # every element is written
    return np.ascontiguousarray(np.transpose(got, (0, 2, 1))) if planar else got


def same(a, b):
    """Two float32 arrays: NaN where the other has NaN, the same bits elsewhere."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
def check_exact(x, s2, tables, C, planar, seed, both=True):
    mu, w = (None, None) if C == 0 else (tables[0][:C], tables[1][:C])
    ds, df = G.cotangents(len(x), C, seed)
    df = df if both or C == 0 else None
    want = G.restate_bwd_fp32(x, ds, df, s2, mu, w)
    got = bwd(x, ds, df, s2, mu, w, planar)
    assert same(got, want), (x.shape, s2 is not None, C, planar, both)
    assert np.isfinite(got).all() and np.any(got != 0)


@pytest.mark.parametrize("length", G.BWD_EXACT_LENGTHS)
def test_integer_cases_are_exact(length):
    """Spans 1 and 2; batches 1, 3, 5 (a workgroup of the wave route part empty) and 65; both layouts; C = 0 with dfeat only, 1,
    17 and 64; blind and with sigma2.  The large products (65 frames of 1025 and more) take one C each, in turn."""
    tables = R.exact_tables(64, 9)
    turn = G.BWD_EXACT_LENGTHS.index(length)
    for i, B in enumerate(G.BWD_EXACT_BATCHES):
        x = R.exact_case(B, length, 100 * length + B)
        Cs = G.EXACT_CLASSES if B * length <= 20000 else (G.EXACT_CLASSES[(turn + i) % 4],)
        for k, C in enumerate(Cs):
            s2 = None if (i + k) % 2 else np.full(B, 0.125, np.float32)
            for planar in ((0, 1) if B == 3 else ((i + k + turn) % 2,)):
                check_exact(x, s2, tables, C, planar, seed=length + k, both=bool(k % 2))
    if length <= 2048:                                       # all 17 sums (exact_case: with span 1 three of them are zero)
        x = R.exact_case(3, length, 7 * length, span=2)
        check_exact(x, None, tables, 17, 0, seed=1)
        check_exact(x, np.full(3, 0.25, np.float32), tables, 64, 1, seed=2)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. real frames under the derived bound
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.REAL_CASES, ids=lambda c: f"{c[0]}-{c[1]}dB-{'blind' if c[2] else 'sigma2'}")
def test_real_frames_stay_within_the_derived_bound(case):
    for planar, length in enumerate(G.REAL_LENGTHS):
        x, s2, ds, df, mu, w, bias, ref = G.real_case(*case, length)
        got = bwd(x, ds, df, s2, mu, w, planar).astype(np.float64)
        use = ref["usable"]
        assert (~use).sum() <= R.DECISION_SHARE * len(use) and np.isfinite(got).all()
        err = np.abs(got - ref["dx"])[use]
        worst = (err.max(axis=(1, 2)) / ref["scale"][use]).max()
        print(f"{case} len {length}: worst error {worst:.1e} of the frame's max |dx|, worst error / bound {(err / ref['Edx'][use]).max():.1e}")
        assert np.all(err <= ref["Edx"][use]), (case, length)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. masking and isolation
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [96, 300])
def test_a_class_with_weight_zero_is_not_read_and_bad_data_stays_in_its_frame(length):
    from vit_vs_raw_iq_amd import CumulantClassifier
    clf = CumulantClassifier(length, classes=["BPSK", "QPSK", "8PSK", "16QAM", "64QAM"])
    x, s2 = R.real_frames(6, length, "16QAM", 12, seed=length)
    ds, df = G.cotangents(6, 5, 3, sparse=False)
    ds[:, 2] = 0
    base = bwd(x, ds, df, s2, clf.mu, clf.w)
    mu = clf.mu.copy()
    mu[2] = np.nan
    assert np.isfinite(base).all() and same(bwd(x, ds, df, s2, mu, clf.w), base)
    keep = [0, 1, 3, 4]
    assert same(bwd(x, ds[:, keep], df, s2, clf.mu[keep], clf.w[keep]), base)
    ds2 = ds.copy()
    ds2[1, 2] = 1.0                                           # asked about: its own frame only
    bad = bwd(x, ds2, df, s2, mu, clf.w)
    assert np.isnan(bad[1]).all() and same(bad[[0, 2, 3, 4, 5]], base[[0, 2, 3, 4, 5]])
    # a refused sigma2, an all-zero frame and a NaN sample: each its own frame only
    z, sig = x.copy(), s2.copy()
    sig[0] = 50.0
    z[2] = 0
    z[4, length // 2, 1] = np.nan
    got = bwd(z, ds, df, sig, clf.mu, clf.w, planar=1)
    assert np.isnan(got[[0, 2, 4]]).all() and same(got[[1, 3, 5]], base[[1, 3, 5]])
    assert not np.isnan(bwd(z, None, df, None, planar=0)[0]).any()                        # blind: frame 0 is fine again


def test_a_frame_of_one_symbol_is_refused_as_data():
    assert np.isnan(bwd(np.ones((5, 1, 2), np.float32), None, np.ones((5, 10), np.float32))).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. invariance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [130, 300])
def test_a_frames_gradient_depends_on_neither_its_neighbours_nor_the_run(length):
    from vit_vs_raw_iq_amd import CumulantClassifier
    clf = CumulantClassifier(length, classes=["BPSK", "QPSK", "8PSK", "16QAM"])
    x, s2 = R.real_frames(7, length, "QPSK", 10, seed=length)
    ds, df = G.cotangents(7, 4, 5)
    whole = bwd(x, ds, df, s2, clf.mu, clf.w)
    assert same(bwd(x, ds, df, s2, clf.mu, clf.w), whole)                                   # two runs
    for b in (0, 3, 6):
        assert same(bwd(x[b:b + 1], ds[b:b + 1], df[b:b + 1], s2[b:b + 1], clf.mu, clf.w), whole[b:b + 1])
    order = [6, 2, 5, 0]
    assert same(bwd(x[order], ds[order], df[order], s2[order], clf.mu, clf.w, planar=1), whole[order])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import CumulantClassifier
    lib = N.lib()
    ARG, UNSUPPORTED = 1, 2
    B, length = 2, 8192
    x = torch.zeros(B, length + 1, 2, device=dev())
    x[:, ::2, 0] = 1.0                                        # (a variance: P is accepted)
    dx = torch.full((B, length + 1, 2), SENTINEL, device=dev())
    s2, ds, df = torch.zeros(B, device=dev()), torch.ones(B, 65, device=dev()), torch.ones(B, 10, device=dev())
    mu, w = torch.zeros(65, 10, device=dev()), torch.ones(65, 10, device=dev())

    def call(n=B, length=length, par="ok", **kw):
        ptrs = dict(x=x.data_ptr(), dscore=ds.data_ptr(), dfeat=df.data_ptr(), dx=dx.data_ptr())
        ptrs.update({k: kw.pop(k) for k in list(kw) if k in ptrs})
        fields = dict(planar=0, sigma2=s2.data_ptr(), mu=mu.data_ptr(), w=w.data_ptr(), bias=None, n_classes=17)
        p = None if par is None else N.Cumulants(**{**fields, **kw})
        return lib.iq_frames_cumulants_bwd(*ptrs.values(), n, length, ctypes.byref(p) if p is not None else None, N.stream_handle())

    def refused():
        assert call(x=None) == ARG and call(dx=None) == ARG and call(par=None) == ARG and call(dscore=None, dfeat=None) == ARG
        assert call(length=0) == ARG and call(planar=2) == ARG and call(n_classes=-1) == ARG
        assert call(mu=None) == ARG and call(w=None) == ARG and call(n_classes=0) == ARG
        assert call(x=x.data_ptr() + 4) == ARG and call(dx=dx.data_ptr() + 4) == ARG and call(dx=dx.data_ptr() + 2, planar=1) == ARG
        assert call(dscore=ds.data_ptr() + 2) == ARG and call(dfeat=df.data_ptr() + 2) == ARG and call(sigma2=s2.data_ptr() + 1) == ARG
        assert call(n_classes=65) == UNSUPPORTED and call(length=8193) == UNSUPPORTED          # one past every limit
        assert call(n=2 ** 31 // 20 + 1, length=1) == UNSUPPORTED
        assert call(n=0) == 0 and call(n=-2) == 0                                              # nothing to do
    assert kernel_launches(lib, refused) == {}                                                # not one launch
    torch.cuda.synchronize()
    assert torch.equal(dx, torch.full_like(dx, SENTINEL))
    # the limits themselves run, each on its instance: 64 classes, the longest frame, the threshold and one past it
    for kw, name in ((dict(n_classes=64, length=64), "<false>"), (dict(length=8192), "<true>"), (dict(length=256), "<false>"),
                     (dict(length=257), "<true>"), (dict(length=8192, dscore=None, n_classes=0, mu=None, w=None), "<true>")):
        assert kernel_launches(lib, lambda: call(**kw) == 0 or pytest.fail(str(kw))) == {"frames_cumulants_bwd_kernel" + name: 1}, kw
    torch.cuda.synchronize()
    flat = dx.view(-1)                                        # B frames of 8192 of the buffer's 8193 rows
    assert bool(torch.isfinite(flat[:B * length * 2]).all()) and bool((flat[B * length * 2:] == SENTINEL).all())
    clf = CumulantClassifier(8, classes=["BPSK"])
    assert clf.input_gradient(torch.zeros(0, 8, 2, device=dev()), torch.zeros(0, 1, device=dev())).shape == (0, 8, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. autograd, the chain, hipGraph
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,length", [("frames", 200), ("planar", 700)])
def test_autograd_equals_input_gradient_equals_the_abi_call(layout, length):
    from vit_vs_raw_iq_amd import CumulantClassifier
    names = ["BPSK", "QPSK", "16QAM", "64QAM"]
    clf = CumulantClassifier(length, classes=names, layout=layout, differentiable=True)
    plain = CumulantClassifier(length, classes=names, layout=layout)
    xs, s2 = R.real_frames(3, length, "16QAM", 14.0, 2)
    ds, df = G.cotangents(3, 4, 7)
    x = on_device(R.in_layout(xs, clf.planar)).requires_grad_()
    score, feat, mom = clf(x, sigma2=s2, return_features=True, return_moments=True)
    assert score.requires_grad and not feat.requires_grad and not mom.requires_grad
    for a, b in zip((score, feat, mom), plain(x, sigma2=s2, return_features=True, return_moments=True)):
        assert torch.equal(a.detach(), b) and not b.requires_grad                          # the default detaches, as it did
    (dx,) = torch.autograd.grad(score, x, on_device(ds))
    again = clf(x, sigma2=s2)                                                              # no extras asked for: a bare tensor
    assert isinstance(again, torch.Tensor) and same_bits(torch.autograd.grad(again, x, on_device(ds))[0], dx)
    for c in (clf, plain):
        assert same_bits(c.input_gradient(x, on_device(ds), sigma2=s2), dx)
    back = (lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 1)))) if clf.planar else (lambda a: a)      # -> (B, len, 2)
    assert np.array_equal(bits(bwd(xs, ds, None, s2, clf.mu, clf.w, clf.planar)), bits(back(dx.cpu().numpy())))
    assert float(dx.abs().max()) > 0
    # the features, blind; and both gradients in one call, the noise as snr_db
    f, m2 = clf.features(x, return_moments=True)
    assert f.requires_grad and not m2.requires_grad and torch.equal(f.detach(), plain.features(x)) and not plain.features(x).requires_grad
    (dxf,) = torch.autograd.grad(f, x, on_device(df))
    assert same_bits(plain.input_gradient(x, dfeat=on_device(df)), dxf)
    assert np.array_equal(bits(bwd(xs, None, df, None, planar=clf.planar)), bits(back(dxf.cpu().numpy())))
    both = plain.input_gradient(x, on_device(ds), on_device(df), snr_db=14.0)
    assert np.array_equal(bits(bwd(xs, ds, df, np.float32(10.0 ** -1.4), clf.mu, clf.w, clf.planar)), bits(back(both.cpu().numpy())))


def test_gradients_reach_the_raw_frame_through_receiver_and_carrier():
    """ShapedSynth -> Receiver -> Carrier -> classifier: x.grad of the raw frame is the chained adjoint calls, bit for bit."""
    from vit_vs_raw_iq_amd import Carrier, CumulantClassifier, Receiver, ShapedSynth
    names = ["BPSK", "QPSK", "16QAM"]
    ws = ShapedSynth(names, snrs_db=(20.0,), length=1024, seed=11, sps=2, device=dev())
    raw = ws.generate(6, 0, 0)[0]
    rx, cr = Receiver.for_synth(ws, timing="energy"), Carrier(512, order=4, layout="interleaved")
    clf = CumulantClassifier(512, classes=names, differentiable=True)
    ds = on_device(G.cotangents(6, 3, 9)[0])
    x = raw.clone().requires_grad_()
    sym = cr(rx(x))
    score = clf(sym)
    dsym = clf.input_gradient(sym.detach(), ds)
    (want,) = torch.autograd.grad(sym, x, dsym, retain_graph=True)
    score.backward(ds)
    assert same_bits(x.grad, want) and float(x.grad.abs().max()) > 0 and bool(torch.isfinite(x.grad).all())


def test_a_captured_attack_step_replays_as_eager():
    """A capture fails on any host synchronisation: forward, margin weights, backward and the L-infinity step are captured whole."""
    import vit_vs_raw_iq_amd.adversarial as A
    from vit_vs_raw_iq_amd import CumulantClassifier, fgsm
    clf = CumulantClassifier(300, classes=["QPSK", "16QAM", "64QAM"])
    x0 = on_device(R.real_frames(5, 300, "16QAM", 15.0, 3)[0])
    y = torch.ones(5, dtype=torch.int64, device=dev())
    s2 = torch.full((5,), 0.03, device=dev())
    eager = fgsm(clf, x0, y, 0.05, sigma2=s2)             # also: the tables are on the device before the capture
    assert float((eager - x0).abs().max()) == pytest.approx(0.05, rel=1e-5)
    xa = x0.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    nan = float("nan")
    with torch.cuda.graph(graph):
        A._clf_attack(clf, x0, y, (s2,), 0.05, 0.05, 1, xa, nan, nan, 256, "margin")
    xa.copy_(x0)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(xa, eager)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the attacks
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attacked():
    """fgsm on the 20 dB decision set at eps 0.05 with the margin loss and the known sigma2: computed once for the tests below."""
    from vit_vs_raw_iq_amd import fgsm
    clf = G.decision_classifier()
    X, Y, s2 = R.decision_set(G.FGSM_SNR)
    xd, yd = on_device(X), torch.from_numpy(np.array(Y)).to(dev())
    return dict(clf=clf, xd=xd, yd=yd, x_adv=fgsm(clf, xd, yd, G.FGSM_EPS, sigma2=float(s2)))


def test_fgsm_takes_the_decisions_random_signs_leave(attacked):
    """Decided as the host table decides it: one signed step leaves at most half of what random signs leave.  The step itself is
    x + eps sign(g) of the device's own gradient of the margin, rounded once."""
    clf, xd = attacked["clf"], attacked["xd"]
    X, Y, s2 = R.decision_set(G.FGSM_SNR)
    ds = G.margin_dscore(clf(xd, sigma2=float(s2)).cpu().numpy(), Y)
    g = clf.input_gradient(xd, on_device(ds), sigma2=float(s2)).cpu().numpy()
    assert np.array_equal(bits(attacked["x_adv"].cpu().numpy()), bits(X + np.float32(G.FGSM_EPS) * np.sign(g).astype(np.float32)))
    host = G.host_fgsm()
    assert np.mean(np.sign(g) == np.sign(host["g"])) > 0.97                                  # (where |g| is near 0 the signs may differ)
    acc = lambda x: float(np.mean(clf.predict(x, sigma2=float(s2)).cpu().numpy() == Y))      # noqa: E731
    clean, adv, rand = acc(xd), acc(attacked["x_adv"]), acc(on_device(host["x_rand"]))
    print(f"eps {G.FGSM_EPS}: device clean {clean:.3f}, FGSM {adv:.3f}, random signs {rand:.3f}")
    assert adv <= 0.5 * rand


def test_pgd_and_the_curve(attacked):
    from vit_vs_raw_iq_amd import fgsm, pgd, robustness_curve
    clf, xd, yd = attacked["clf"], attacked["xd"], attacked["yd"]
    _, Y, s2 = R.decision_set(G.FGSM_SNR)
    s2 = float(s2)
    assert same_bits(pgd(clf, xd, yd, G.FGSM_EPS, G.FGSM_EPS, 1, sigma2=s2), attacked["x_adv"])
    assert same_bits(fgsm(clf, xd, yd, G.FGSM_EPS, snr_db=float(G.FGSM_SNR), batch=50), attacked["x_adv"])     # chunks of 50 frames
    acc = lambda x, **kw: float(np.mean(clf.predict(x, **kw).cpu().numpy() == Y))           # noqa: E731
    curve = robustness_curve(clf, xd, yd, [0.0, 0.01, 0.02, G.FGSM_EPS], sigma2=s2)
    assert curve[0] == acc(xd, sigma2=s2) and curve[3] == acc(attacked["x_adv"], sigma2=s2) and curve[3] <= curve[1]
    pg = pgd(clf, xd, yd, G.FGSM_EPS, G.FGSM_EPS / 4, 10, sigma2=s2)
    ball = G.FGSM_EPS + 2.0 ** -24 * (float(xd.abs().max()) + G.FGSM_EPS)                   # (x0 +- eps is rounded once, in fp32)
    assert float((pg - xd).abs().max()) <= ball
    pcurve = robustness_curve(clf, xd, yd, [0.0, 0.01, 0.02, G.FGSM_EPS], attack="pgd", sigma2=s2)
    rand = acc(on_device(G.host_fgsm()["x_rand"]), sigma2=s2)
    print(f"FGSM curve {curve}, PGD curve {pcurve}, PGD(eps / 4 x 10) {acc(pg, sigma2=s2):.3f}, random signs {rand:.3f}")
    assert acc(pg, sigma2=s2) <= 0.5 * rand and pcurve[3] <= 0.5 * rand
    # blind, and the cross entropy through iq_ce_fwd_bwd: the ball is kept and two runs agree
    ce = pgd(clf, xd[:8], yd[:8], 0.02, 0.01, 3, loss="ce", random_start=True, seed=1)
    assert float((ce - xd[:8]).abs().max()) <= 0.02 + 2.0 ** -24 * (float(xd[:8].abs().max()) + 0.02)
    assert same_bits(ce, pgd(clf, xd[:8], yd[:8], 0.02, 0.01, 3, loss="ce", random_start=True, seed=1))
    assert robustness_curve(clf, xd, yd, [0.0])[0] == acc(xd)


def test_the_transfer_table(attacked):
    """Across the three classical classifiers and a callable: row 0 is clean, the diagonal is each classifier's own
    robustness_curve entry, and every source is attacked once."""
    import vit_vs_raw_iq_amd.adversarial as A
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier, LikelihoodClassifier, robustness_curve, transfer_table
    clf, xd, yd = attacked["clf"], attacked["xd"][:64], attacked["yd"][:64]
    _, Y, s2 = R.decision_set(G.FGSM_SNR)
    s2 = float(s2)
    lik = LikelihoodClassifier(R.DECISION_LENGTH, classes=R.decision_classes(), rotations=16)
    em = HybridLikelihoodClassifier(R.DECISION_LENGTH, classes=R.decision_classes(), iters=4)
    parties = [(clf, dict(sigma2=s2)), (lik, dict(sigma2=s2)), em]
    calls = []
    fgsm0 = A.fgsm
    A.fgsm = lambda model, *a, **kw: calls.append(model) or fgsm0(model, *a, **kw)
    try:
        table = transfer_table(parties, parties + [lambda f: clf.predict(f)], xd, yd, G.FGSM_EPS)
    finally:
        A.fgsm = fgsm0
    assert calls == [clf, lik, em]                                                           # once each, not once per target
    assert len(table) == 4 and all(len(row) == 4 for row in table)
    for i, (c, kw) in enumerate(((clf, dict(sigma2=s2)), (lik, dict(sigma2=s2)), (em, {}))):
        curve = robustness_curve(c, xd, yd, [0.0, G.FGSM_EPS], **kw)
        assert table[0][i] == curve[0] and table[i + 1][i] == curve[1], (i, table, curve)
    blind = [float(np.mean(clf.predict(x).cpu().numpy() == Y[:64])) for x in (xd, attacked["x_adv"][:64])]
    assert table[0][3] == blind[0] and table[1][3] == blind[1]                               # the callable: clf, blind
    print("transfer table (rows clean, cumulants, likelihood, hybrid; columns the same and the blind cumulants):")
    for row in table:
        print("   " + "  ".join(f"{v:.3f}" for v in row))
    assert table[1][0] <= 0.5 * table[0][0]
