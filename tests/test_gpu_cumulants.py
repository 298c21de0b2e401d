"""GPU (MI355X): the cumulant classifier on the device (csrc/cumulants.hip, iq_frames_cumulants, vit_vs_raw_iq_amd.cumulants).

Every call through the C ABI here (`run`) carves its operands out of NaN-filled buffers and its outputs out of sentinel-filled ones
and checks the guards, and that the operands hold what they held, afterwards.

1. Bit for bit: integer frames c + pattern (tests/cumulants_ref.py, exact_case) -- the mean and the moments equal the fp64
   definition exactly, the features and scores the fp32 restatement of the header, pred the first largest, at every length edge
   of both routes, batch, layout, class count, with and without sigma2, each optional output alone and all together.
   (P = C21 - sigma2 with a sigma2 is one more fp32 subtraction of a rounded moment: it is held to the restatement, and to the
   definition where sigma2 is NULL.)
2. Bounded: FrameSynth's frames at 20, 8 and 0 dB against cumulants_reference under the bound derived in tests/cumulants_ref.py.
3. Decisions: the sets tests/test_cumulants_cpu.py has checked, and the chain ShapedSynth -> Receiver -> Carrier -> classifier:
   wherever the bound settles the decision the device decides as the definition does, and at most 2 % of a set is left open.
4. Isolation, batch invariance, run-to-run identity.          5. fit, refusals, hipGraph, the evaluation reports.
(The timing is scripts/cumulants_prof.py -> profiles/cumulants.txt; nothing is asserted about it.)
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import cumulants_ref as R
from frontend_gpu import ISENT, abi_call, bits, dev, on_device, same_bits
from prof_names import kernel_launches

pytestmark = pytest.mark.gpu

NAMES = ("feat", "mom", "score", "pred")


def kernel_for(length):
    return "frames_cumulants_kernel<false>" if length <= R.WAVE_ROUTE_MAX else "frames_cumulants_kernel<true>"


def run(x, sigma2=None, mu=None, w=None, bias=None, planar=0, want=(True, True, True, True), expect_kernel=True):
    """One guarded iq_frames_cumulants call on x (B, len, 2), laid out as `planar` says -> dict(feat (B, 10), mom (B, 20),
    score (B, C) float32, pred (B,) int32), None for what was not asked for (or cannot be: score and pred without classes)."""
    import vit_vs_raw_iq_amd._native as N
    x = np.asarray(x, dtype=np.float32)
    B, length = x.shape[:2]
    Cn = 0 if mu is None else len(mu)
    want = (want[0], want[1], want[2] and Cn > 0, want[3] and Cn > 0)
    sigma2 = None if sigma2 is None else np.broadcast_to(np.asarray(sigma2, np.float32), (B,))

    def par(sigma2, mu, w, bias):
        return N.Cumulants(planar=planar, sigma2=sigma2, mu=mu, w=w, bias=bias, n_classes=Cn)
    outs = [(B, R.F) if want[0] else None, (B, R.MOMENTS) if want[1] else None, (B, Cn) if want[2] else None,
            (np.int32, B) if want[3] else None]
    got = abi_call("iq_frames_cumulants", kernel_for(length), (R.in_layout(x, planar),), outs, B, length, par, expect_kernel,
                   side=(sigma2, mu if Cn else None, w if Cn else None, bias if Cn else None))
    return dict(zip(NAMES, got))


def same(a, b):
    """Two float32 arrays: NaN where the other has NaN, the same bits elsewhere."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
def check_exact(x, s2, tables, C, planar, want=(True, True, True, True)):
    from vit_vs_raw_iq_amd import cumulants_reference
    mu, w, bias = (None, None, None) if C == 0 else (t[:C] for t in tables)
    r = R.restate_fp32(x, s2, mu, w, bias)
    ref_mom = cumulants_reference(x, s2)[1].astype(np.float32)
    got = run(x, s2, mu, w, bias, planar, want)
    tag = (x.shape, s2 is not None, C, planar, want)
    for k, on in zip(NAMES, want):
        assert (got[k] is not None) == (on and (C > 0 or k in ("feat", "mom"))), (tag, k)
    if got["mom"] is not None:
        upto = 20 if s2 is None else 19
        assert same(got["mom"][:, :upto], ref_mom[:, :upto]), tag                              # the fp64 definition, rounded once
        assert same(got["mom"], r["mom"]), tag
    if got["feat"] is not None:
        assert same(got["feat"], r["feat"]), tag
    if got["score"] is not None:
        assert same(got["score"], r["score"]), tag
    if got["pred"] is not None:
        assert np.array_equal(got["pred"], r["pred"]), tag
    return got


@pytest.mark.parametrize("length", R.EXACT_LENGTHS)
def test_integer_cases_are_exact(length):
    tables = R.exact_tables(64, 9)
    for i, B in enumerate(R.EXACT_BATCHES):                  # 65: the wave route ends in a workgroup with one frame of four
        x = R.exact_case(B, length, 100 * length + B)
        for j, s2 in enumerate((None, np.full(B, 0.125, np.float32))):
            for k, C in enumerate((0, 1, 17, 64)):
                for planar in ((0, 1) if B == 3 else ((i + j + k) % 2,)):
                    check_exact(x, s2, tables, C, planar)
    if length <= 2048:                                       # all 17 sums (exact_case: with span 1 three of them are zero)
        x = R.exact_case(3, length, 7 * length, span=2)
        check_exact(x, None, tables, 17, 0)
        check_exact(x, np.full(3, 0.25, np.float32), tables, 64, 1)


@pytest.mark.parametrize("length", [64, 257])
def test_each_output_alone_and_all_together(length):
    tables = R.exact_tables(17, 4)
    x = R.exact_case(5, length, length)
    whole = check_exact(x, None, tables, 17, 0)
    for only in range(4):
        want = tuple(k == only for k in range(4))
        got = check_exact(x, None, tables, 17, 0, want)
        assert np.array_equal(bits(got[NAMES[only]]) if only < 3 else got["pred"], bits(whole[NAMES[only]]) if only < 3 else whole["pred"])
    for want in ((True, True, False, False), (False, False, True, True), (True, False, False, True)):
        check_exact(x, np.full(5, 0.125, np.float32), tables, 17, 1, want)
    for only in (0, 1):                                      # without classes there are two outputs
        check_exact(x, None, tables, 0, 1, tuple(k == only for k in range(4)))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bounded
# ---------------------------------------------------------------------------------------------------------------------------
def check_bounded(x, s2, clf, planar, tag):
    """Device against cumulants_reference under the derived bound; -> (got, ref)."""
    from vit_vs_raw_iq_amd import cumulants_reference
    ref = R.reference_and_bound(x, s2, clf.mu, clf.w, clf.bias)
    feat, mom, score, pred = cumulants_reference(x, s2, clf.mu, clf.w, clf.bias)
    got = run(x, s2, clf.mu, clf.w, clf.bias, planar)
    assert ref["ok"].all() and np.isfinite(got["feat"]).all() and np.isfinite(got["score"]).all(), tag
    em, ef, es = np.abs(got["mom"] - mom), np.abs(got["feat"] - feat), np.abs(got["score"] - score)
    with np.errstate(all="ignore"):
        print(f"{tag}: |mom - ref| / bound {float(np.nanmax(em / ref['Emom'])):.4f}, |feat - ref| / bound {float(np.nanmax(ef / ref['Efeat'])):.4f} "
              f"(bound up to {ref['Efeat'].max():.2e}), |score - ref| / bound {float(np.nanmax(es / ref['Escore'])):.4f}")
    assert np.all(em <= ref["Emom"]) and np.all(ef <= ref["Efeat"]) and np.all(es <= ref["Escore"]), tag
    assert np.array_equal(got["pred"], R.first_largest(got["score"].astype(np.float64))), tag  # the first largest of its OWN scores
    sure = R.decided(ref)
    assert np.array_equal(got["pred"][sure], pred[sure]), tag
    assert np.any(ef > 0)                                    # (fp32 did round: the test is not vacuous)
    return got, ref, sure


@pytest.mark.parametrize("length", [128, 1000])
def test_generated_frames_stay_within_the_derived_bound(length):
    """FrameSynth's frames of all 19 classes at 20, 8 and 0 dB (GMSK and OQPSK as frames: the 17 table classes score them),
    one route per length, blind in one layout and with the frames' own sigma2 in the other."""
    from vit_vs_raw_iq_amd import CumulantClassifier, FrameSynth, noise_for
    from vit_vs_raw_iq_amd import data as D
    clf = CumulantClassifier(length)
    fs = FrameSynth(D.CLASSES, snrs_db=(20.0, 8.0, 0.0), length=length, seed=7, device=dev())
    raw, y, z = fs.generate(57, 0, 0)
    x, s2 = raw.cpu().numpy(), noise_for(z)[1].float().cpu().numpy()
    assert sorted(set(z.cpu().numpy().tolist())) == [0.0, 8.0, 20.0]
    check_bounded(x, None, clf, 0, f"len {length} blind")
    check_bounded(x, s2, clf, 1, f"len {length} known sigma2")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. decisions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snr,blind", [(20.0, False), (8.0, False), (20.0, True)])
def test_the_decision_sets_are_decided_as_the_definition_decides_them(snr, blind):
    """make_dataset's 256 frames, uploaded as they are.  tests/test_cumulants_cpu.py has shown that the bound settles all but at
    most 2 % of them: on the settled ones pred must equal the definition's."""
    from vit_vs_raw_iq_amd import CumulantClassifier
    X, Y, s2 = R.decision_set(snr)
    clf = CumulantClassifier(R.DECISION_LENGTH, classes=R.decision_classes())
    s2 = None if blind else np.full(len(X), s2, np.float32)
    got, ref, sure = check_bounded(X, s2, clf, 0, f"decision {snr} dB blind={blind}")
    assert np.array_equal(ref["pred"], R.decision_reference(snr, blind)["pred"])
    assert (~sure).mean() <= R.DECISION_SHARE
    assert np.mean(got["pred"] == Y) >= np.mean(ref["pred"] == Y) - R.DECISION_SHARE
    # the same through the class
    xd = on_device(X)
    kw = {} if blind else dict(snr_db=snr)
    score, feat, mom = clf(xd, return_features=True, return_moments=True, **kw)
    for k, t in (("score", score), ("feat", feat), ("mom", mom)):
        assert t.dtype == torch.float32 and np.array_equal(bits(t.cpu().numpy()), bits(got[k])), k
    pred = clf.predict(xd, **kw)
    assert pred.dtype == torch.int64 and np.array_equal(pred.cpu().numpy(), got["pred"])
    assert same_bits(clf.features(xd, **kw), feat) and same_bits(clf(xd, **kw), score)
    if not blind:
        assert same_bits(clf(xd, sigma2=torch.full((len(X),), float(s2[0]))), score)


def test_the_loop_closes_behind_receiver_and_carrier():
    """ShapedSynth -> Receiver (normalise=True) -> Carrier -> classifier, blind and with noise_for(snr, normalised=True)."""
    from vit_vs_raw_iq_amd import Carrier, CumulantClassifier, Receiver, ShapedSynth, noise_for
    names = ["BPSK", "QPSK", "16QAM"]
    ws = ShapedSynth(names, snrs_db=(20.0,), length=1024, seed=11, sps=2, device=dev())
    raw, y, z = ws.generate(102, 0, 0)
    sym = Carrier(512, order=4, layout="interleaved")(Receiver.for_synth(ws, timing="energy")(raw))
    assert sym.shape == (102, 512, 2)
    clf = CumulantClassifier(512, classes=names)
    x = sym.cpu().numpy()
    for s2 in (None, noise_for(z, normalised=True)[1].float().cpu().numpy()):
        got, ref, sure = check_bounded(x, s2, clf, 0, f"chain, sigma2 {'known' if s2 is not None else 'blind'}")
        assert (~sure).mean() <= R.DECISION_SHARE
        kw = {} if s2 is None else dict(sigma2=torch.from_numpy(s2))
        pred = clf.predict(sym, **kw).cpu().numpy()
        assert np.array_equal(pred, got["pred"])
        print(f"chain accuracy {np.mean(pred == y.cpu().numpy()):.3f}")
        assert np.mean(pred == y.cpu().numpy()) >= 0.9


# ---------------------------------------------------------------------------------------------------------------------------
# 4. isolation and determinism
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [130, 300])
def test_a_frames_outputs_depend_on_neither_its_neighbours_nor_the_run(length):
    from vit_vs_raw_iq_amd import CumulantClassifier
    clf = CumulantClassifier(length, classes=["BPSK", "8PSK", "16QAM", "64QAM"])
    t = (clf.mu, clf.w, clf.bias)
    x, s2 = R.real_frames(6, length, "16QAM", 12.0, 8)
    whole = run(x, s2, *t)
    again = run(x, s2, *t)
    for k in NAMES:
        assert np.array_equal(whole[k].view(np.int32), again[k].view(np.int32)), k             # run to run, bit for bit
    for b in (0, 2, 5):                                      # alone, and first / last of another batch
        for rows in ([b], [b, 1, 3], [1, 3, 4, 0, b]):
            part = run(x[rows], s2[rows], *t)
            at = rows.index(b)
            for k in NAMES:
                assert np.array_equal(part[k][at:at + 1].view(np.int32), whole[k][b:b + 1].view(np.int32)), (k, b, rows)
    # a zero frame, a refused sigma2 and a NaN sample between good frames: NaN and -1 there, not a bit elsewhere
    xb, sb = x.copy(), s2.copy()
    xb[1] = 0.0
    sb[3] = whole["mom"][3, 4] * 2                           # twice the frame's variance
    xb[4, length // 2, 1] = np.nan
    for sig, bad in ((sb, [1, 3, 4]), (None, [1, 4])):
        base = whole if sig is not None else run(x, None, *t)
        got = run(xb, sig, *t)
        good = [b for b in range(6) if b not in bad]
        assert np.isnan(got["feat"][bad]).all() and np.isnan(got["score"][bad]).all() and np.all(got["pred"][bad] == -1)
        assert got["mom"][1, 19] == (0.0 if sig is None else -sig[1]) and np.isfinite(got["mom"][[1, 3]]).all()   # mom is as computed
        for k in NAMES:
            assert np.array_equal(got[k][good].view(np.int32), base[k][good].view(np.int32)), k
    for sig in (np.inf, np.nan, -np.inf):
        sb = s2.copy()
        sb[2] = sig
        got = run(x, sb, *t)
        assert np.isnan(got["feat"][2]).all() and got["pred"][2] == -1
        assert np.array_equal(got["score"][[0, 1, 3, 4, 5]].view(np.int32), whole["score"][[0, 1, 3, 4, 5]].view(np.int32))
    one = run(x[:, :1], None, *t)                            # len = 1: no variance
    assert np.isnan(one["feat"]).all() and np.all(one["pred"] == -1) and np.array_equal(one["mom"][:, :2], x[:, 0])


def test_a_tie_goes_to_the_first_listed():
    from vit_vs_raw_iq_amd import CumulantClassifier
    xs = np.concatenate([R.real_frames(3, 64, n, snr, 7)[0] for n in ("16PSK", "32PSK") for snr in (20.0, 0.0)])
    for names in (["32PSK", "16PSK"], ["16PSK", "32PSK"]):
        clf = CumulantClassifier(64, classes=names)
        got = run(xs, None, clf.mu, clf.w, clf.bias)
        assert np.array_equal(got["score"][:, 0].view(np.int32), got["score"][:, 1].view(np.int32)) and not got["pred"].any()
        assert not clf.predict(on_device(xs)).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. fit and plumbing
# ---------------------------------------------------------------------------------------------------------------------------
def test_fit_gives_tables_the_device_and_the_definition_decide_alike_with():
    from vit_vs_raw_iq_amd import CumulantClassifier, FrameSynth, noise_for
    names = ["BPSK", "QPSK", "GMSK", "OQPSK"]
    fs = FrameSynth(names, snrs_db=(8.0, 20.0), length=128, seed=5, device=dev())
    for blind in (True, False):
        clf = CumulantClassifier(128, classes=names)
        assert np.isnan(clf.mu[2:]).all()
        with pytest.raises(ValueError, match="fit"):
            clf.predict(torch.zeros(1, 128, 2, device=dev()))
        assert clf.fit(fs, 40, blind=blind, batch=100) is clf
        assert np.isfinite(clf.mu).all() and np.isfinite(clf.bias).all() and np.all(clf.w > 0) and np.isfinite(clf.w).all()
        assert clf.fitted["blind"] == blind and np.array_equal(clf.fitted["frames"], [80, 80, 80, 80]) and clf.indistinguishable() == []
        raw, y, z = fs.generate(64, 0, 3)                    # another stream than the one fitted on
        s2 = None if blind else noise_for(z)[1].float().cpu().numpy()
        got, ref, sure = check_bounded(raw.cpu().numpy(), s2, clf, 0, f"fitted, blind={blind}")
        kw = {} if blind else dict(snr_db=z)
        pred = clf.predict(raw, **kw).cpu().numpy()
        assert np.array_equal(pred, got["pred"])                                               # the tables went up again after fit()
        # QPSK and OQPSK at one sample per symbol have the same marginal distribution, hence the same cumulants: between those
        # two the features can do no better than a coin, so 0.75 is what four classes can reach and 0.6 what is asked
        print(f"fitted blind={blind}: accuracy {np.mean(pred == y.cpu().numpy()):.3f}, settled {sure.mean():.3f}")
        assert np.mean(pred == y.cpu().numpy()) >= 0.6
    # one SNR of the list
    at20 = CumulantClassifier(128, classes=names).fit(fs, 10, snr_db=20.0)
    assert np.array_equal(at20.fitted["frames"], [10, 10, 10, 10]) and at20.fitted["snr_db"] == 20.0
    # a class that draws no frame (here: none has a variance) raises
    with pytest.raises(ValueError, match="drew no frame"):
        CumulantClassifier(1, classes=names).fit(FrameSynth(names, snrs_db=(20.0,), length=1, device=dev()), 3)


def test_refusals_return_their_code_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import CumulantClassifier
    lib = N.lib()
    ARG, UNSUPPORTED = 1, 2
    sentinel = 1234.5
    B, length = 2, 8192
    x = torch.ones(B, length + 1, 2, device=dev())
    s2 = torch.full((B,), 0.5, device=dev())
    mu, w, bias = torch.zeros(65, 10, device=dev()), torch.ones(65, 10, device=dev()), torch.zeros(65, device=dev())
    feat, mom, score = (torch.full((B, k), sentinel, device=dev()) for k in (10, 20, 65))
    pred = torch.full((B,), ISENT, dtype=torch.int32, device=dev())
    codes = []

    def call(n=B, length=length, par="ok", **kw):
        ptrs = dict(x=x.data_ptr(), feat=feat.data_ptr(), mom=mom.data_ptr(), score=score.data_ptr(), pred=pred.data_ptr())
        ptrs.update({k: kw.pop(k) for k in list(kw) if k in ptrs})
        fields = dict(planar=0, sigma2=s2.data_ptr(), mu=mu.data_ptr(), w=w.data_ptr(), bias=bias.data_ptr(), n_classes=17)
        p = None if par is None else N.Cumulants(**{**fields, **kw})
        codes.append(lib.iq_frames_cumulants(ptrs["x"], ptrs["feat"], ptrs["mom"], ptrs["score"], ptrs["pred"], n, length,
                                             ctypes.byref(p) if p is not None else None, N.stream_handle()))
        return codes[-1]

    def refused():
        assert call(x=None) == ARG and call(par=None) == ARG and call(feat=None, mom=None, score=None, pred=None) == ARG
        assert call(length=0) == ARG and call(planar=2) == ARG and call(n_classes=-1) == ARG and call(mu=None) == ARG and call(w=None) == ARG
        assert call(n_classes=0) == ARG and call(n_classes=0, score=None) == ARG
        assert call(x=x.data_ptr() + 4) == ARG and call(x=x.data_ptr() + 2, planar=1) == ARG
        assert call(feat=feat.data_ptr() + 2) == ARG and call(bias=bias.data_ptr() + 1) == ARG and call(sigma2=s2.data_ptr() + 2) == ARG
        assert call(n_classes=65) == UNSUPPORTED and call(length=8193) == UNSUPPORTED
        assert call(n=0) == 0 and call(n=-2) == 0
    assert kernel_launches(lib, refused) == {}                                                # not one launch
    torch.cuda.synchronize()
    for t, v in ((feat, sentinel), (mom, sentinel), (score, sentinel), (pred, ISENT)):
        assert torch.equal(t, torch.full_like(t, v))
    # the limits themselves run: 64 classes, MAX_LENGTH symbols, NULL sigma2 and bias
    assert call(n_classes=64) == 0 and call(n_classes=64, length=64, sigma2=None, bias=None) == 0
    torch.cuda.synchronize()
    assert bool((pred == -1).all()) and bool(torch.isnan(feat).all())                         # constant frames: no variance
    clf = CumulantClassifier(8, classes=["BPSK", "QPSK"])
    empty = torch.zeros(0, 8, 2, device=dev())
    assert clf(empty).shape == (0, 2) and clf.predict(empty, sigma2=1.0).shape == (0,) and clf.features(empty).shape == (0, 10)


def test_graph_replay_equals_eager():
    """A capture fails on any host synchronisation: the classifier with all its outputs, features and predict, captured whole."""
    from vit_vs_raw_iq_amd import CumulantClassifier
    outs = []
    for length in (130, 300):                                # one route each
        clf = CumulantClassifier(length, classes=["QPSK", "16QAM", "32APSK"])
        x0 = on_device(R.real_frames(5, length, "16QAM", 15.0, 3)[0])
        s2, snr = torch.full((5,), 0.03, device=dev()), torch.full((5,), 15.0, device=dev())    # (device tensors: a number would be copied up)

        def go():
            score, feat, mom = clf(x0, sigma2=s2, return_features=True, return_moments=True)
            return score, feat, mom, clf.predict(x0), clf.features(x0), clf(x0, snr_db=snr)
        eager = go()                                          # also: the tables are on the device before the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            held = go()
        for t in held:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(held, eager):
            assert torch.equal(a, b)
        outs.append(eager)
    assert len(outs) == 2


def _expected_report(res, class_names, prefix):
    """The report file's text from a result dictionary, through the helpers the evaluations share."""
    from vit_vs_raw_iq_amd.evaluation import TARGET_SNRS, classification_report_text, report_text
    K = len(class_names)
    y, p, z = res["labels"], res["predictions"], res["snrs"]
    cm = np.bincount(y * K + p, minlength=K * K).reshape(K, K)
    assert np.array_equal(cm, res["confusion_matrix"])
    snr_acc = {s: float(np.mean(p[np.abs(z - s) <= 0.5] == y[np.abs(z - s) <= 0.5])) for s in TARGET_SNRS if np.any(np.abs(z - s) <= 0.5)}
    assert snr_acc == pytest.approx(res["snr_accuracies"]) and list(snr_acc) == list(res["snr_accuracies"])
    return report_text(prefix, float(np.mean(p == y)), res["snr_accuracies"], classification_report_text(cm, class_names, digits=4))


def test_the_evaluation_writes_the_report_compare_models_reads(tmp_path):
    from vit_vs_raw_iq_amd import CumulantClassifier, FrameSynth
    from vit_vs_raw_iq_amd.evaluation import evaluate_cumulants_with_confusion
    names = ["BPSK", "QPSK", "8PSK", "16QAM"]
    clf = CumulantClassifier(128, classes=names)
    fs = FrameSynth(names, snrs_db=(0.0, 8.0, 20.0), length=128, seed=2, device=dev())
    loader = [fs.generate(24, 24 * i, 1) for i in range(2)]
    for known in (False, True):
        prefix = "cum_known" if known else "cum"
        res = evaluate_cumulants_with_confusion(clf, loader, dev(), names, tmp_path, prefix=prefix, known_noise=known)
        text = (tmp_path / f"{prefix}_classification_report.txt").read_text()
        assert text == _expected_report(res, names, prefix)
        # the three patterns compare_models.py reads
        assert float(re.search(r"Overall Accuracy:\s+([\d.]+)%", text).group(1)) == pytest.approx(res["overall_accuracy"] * 100, abs=0.006)
        assert [int(s) for s in re.findall(r"SNR\s+([+-]?\d+)\s+dB:\s+[\d.]+%", text)] == [0, 8]
        assert re.search(r"weighted avg\s+[\d.]+\s+[\d.]+\s+[\d.]+\s+48", text)
        assert res["confusion_matrix"].sum() == 48
        kw = [dict(snr_db=z) if known else {} for _, _, z in loader]
        want = torch.cat([clf.predict(x, **k) for (x, _, _), k in zip(loader, kw)]).cpu().numpy()
        blind = torch.cat([clf.predict(x) for x, _, _ in loader]).cpu().numpy()
        assert np.array_equal(res["predictions"], np.maximum(np.where(want < 0, blind, want), 0))
        print(f"known_noise={known}: accuracy {res['overall_accuracy']:.3f}")
    with pytest.raises(ValueError):
        evaluate_cumulants_with_confusion(clf, loader, dev(), names[:3], tmp_path)
