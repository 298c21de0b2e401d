"""GPU (MI355X): the likelihood classifier on the device (csrc/likelihood.hip, iq_frames_likelihood, vit_vs_raw_iq_amd.likelihood).

Every call through the C ABI here (`run`) carves its operands out of NaN-filled buffers and its outputs out of sentinel-filled ones
and checks the guards, and that the operands hold what they held, afterwards.

1. Bit for bit: integer frames and points, sigma2 a power of two, quarter turns, classes of one point or 2^k copies of it -- loglik,
   the per-rotation table, best_rot and pred equal the fp64 definition exactly at every length edge, layout, gain and batch.
2. Bounded: real tables against fp64 under the bound derived in tests/likelihood_ref.py, at every class size, rotation count,
   class count and sigma2 asked for.
3. Decisions: the 68 frames at 20 dB, and the loop closed on the device (FrameSynth; ShapedSynth -> Receiver -> Carrier).
4. Isolation, run-to-run identity, refusals, n_frames = 0.          5. hipGraph, the evaluation reports.

best_rot.  A constellation with a k-fold rotational symmetry (every class of the project's table has one: k = 2 .. 32) has k
equal maxima over a full circle of rotations in exact arithmetic, and only rounding orders them -- fp64's in the definition, fp32's
on the device.  So best_rot is held to three things: it is the first largest of the device's OWN table, exactly; that table is the
definition's within the bound; and it is one of the rotations the definition puts within the two bounds of its maximum
(likelihood_ref.rotation_ties), which where that set is a single rotation means equality.  Where the arithmetic is exact (1) and
ties are exact too, best_rot must equal the definition's outright.
(The timing is scripts/likelihood_prof.py -> profiles/likelihood.txt; nothing is asserted about it.)
"""
import ctypes

import numpy as np
import pytest
import torch

import likelihood_ref as R
from frontend_gpu import ISENT, abi_call, bits, dev, on_device, same_bits
from prof_names import kernel_launches

pytestmark = pytest.mark.gpu


def run(x, sigma2, gain, points, classes, rot, mode="max", planar=0, want=(True, True, True), expect_kernel=True):
    """One guarded iq_frames_likelihood call -> dict(loglik (B, C), L (B, C, R) float64, best_rot (B, C), pred (B,) int64)."""
    import vit_vs_raw_iq_amd._native as N
    x = np.asarray(x, dtype=np.float32)
    B, length = x.shape[0], x.shape[2] if planar else x.shape[1]
    Cn, Rn = len(classes), len(rot)
    sigma2 = np.broadcast_to(np.asarray(sigma2, np.float32), (B,))
    gain = None if gain is None else np.broadcast_to(np.asarray(gain, np.float32), (B,))
    arr = (N.SynthClass * Cn)(*[N.SynthClass(0, int(o), int(m)) for o, m in classes])

    def par(points, rot, gain):
        return N.Likelihood(points=points, classes=arr, n_classes=Cn, rot=rot, n_rot=Rn, planar=planar,
                            mode=("max", "mean").index(mode), gain=gain)
    launches = {"frames_likelihood_kernel": 1, **({"likelihood_decide_kernel": 1} if want[2] else {})}
    outs = [(B, Cn), (B, Cn, Rn) if want[0] else None, (np.int32, B, Cn) if want[1] else None, (np.int32, B) if want[2] else None]
    got = abi_call("iq_frames_likelihood", launches, (x, sigma2), outs, B, length, par, expect_kernel, side=(points, rot, gain))
    return dict(zip(("loglik", "L", "best_rot", "pred"),
                    (None if a is None else a.astype(np.int64 if a.dtype == np.int32 else np.float64) for a in got)))


def check_against(got, ref, tag):
    """The asserts every bounded comparison makes (the module's docstring has the reasons for best_rot's)."""
    eL, ell = np.abs(got["L"] - ref["L"]), np.abs(got["loglik"] - ref["loglik"])
    print(f"{tag}: |L - ref| / bound {float((eL / ref['E']).max()):.4f} (bound up to {ref['E'].max():.2e}, |L| up to {np.abs(ref['L']).max():.3g}), "
          f"|loglik - ref| / bound {float((ell / ref['Ell']).max()):.4f}")
    assert np.isfinite(got["L"]).all() and np.isfinite(got["loglik"]).all(), tag
    assert np.all(eL <= ref["E"]), tag
    assert np.all(ell <= ref["Ell"]), tag
    assert np.array_equal(got["best_rot"], np.argmax(got["L"], axis=2)), tag           # (argmax: the first largest, the kernel's walk)
    assert np.array_equal(got["pred"], np.argmax(got["loglik"], axis=1)), tag
    ties = R.rotation_ties(ref["L"], ref["E"])
    assert np.all(np.take_along_axis(ties, got["best_rot"][..., None], axis=2)), tag
    single = ties.sum(axis=2) == 1
    assert np.array_equal(got["best_rot"][single], ref["best_rot"][single]), tag
    return eL


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", R.EXACT_LENGTHS)
def test_integer_cases_are_exact(length):
    """tests/likelihood_ref.py, exact_case: nothing rounds in fp32 or fp64, every exponential is exp2(0) and every logarithm
    log2(1).  Ties between rotations (the class at the origin) are exact on both sides and go to the first."""
    from vit_vs_raw_iq_amd import likelihood_reference
    for n_frames in (1, 3):
        x, s2, gain = R.exact_case(n_frames, length, 10 * length + n_frames)
        for planar in (0, 1):
            for g in (None, gain):
                ll, L, best, pred = likelihood_reference(R.in_layout(x, planar), s2, g, R.EXACT_POINTS, R.EXACT_CLASSES,
                                                         R.QUARTER_TURNS, "max", planar=bool(planar))
                got = run(R.in_layout(x, planar), s2, g, R.EXACT_POINTS, R.EXACT_CLASSES, R.QUARTER_TURNS, "max", planar)
                tag = (length, n_frames, planar, g is not None)
                assert np.array_equal(got["L"], L), tag
                assert np.array_equal(got["loglik"], ll), tag
                assert np.array_equal(got["best_rot"], best) and np.array_equal(got["pred"], pred), tag
        # one rotation: the log of the mean of one term is the term
        for mode in ("max", "mean"):
            got = run(x, s2, gain, R.EXACT_POINTS, R.EXACT_CLASSES, R.QUARTER_TURNS[1:2], mode)
            assert np.array_equal(got["loglik"], L[:, :, 1]) and np.array_equal(got["L"][:, :, 0], L[:, :, 1]) and not got["best_rot"].any()
            assert np.array_equal(got["pred"], np.argmax(L[:, :, 1], axis=1))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bounded
# ---------------------------------------------------------------------------------------------------------------------------
def _sizes_case():
    """Classes of 1, 2, 3, 63, 64, 65 and 256 points whose ranges lie out of order in one table."""
    sizes = [1, 2, 3, 63, 64, 65, 256]
    order = [3, 0, 6, 1, 5, 2, 4]                        # where each class lies in the table
    table, classes, off = [], [None] * len(sizes), 0
    for i in order:
        classes[i] = (off, sizes[i])
        table.append(R.random_table(sizes[i], 40 + i))
        off += sizes[i]
    points = np.concatenate(table)
    frames_of = points[classes[4][0]:classes[4][0] + 64].astype(np.float64) @ np.array([1, 1j])
    return points, classes, frames_of


def _bounded_cases():
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    from vit_vs_raw_iq_amd.likelihood import rotation_table
    full = lambda Rn: rotation_table(2 * np.pi * np.arange(Rn) / Rn)                  # noqa: E731
    points, classes, frames_of = _sizes_case()
    yield "sizes_R63", points, classes, full(63), R.real_frames(2, 130, frames_of, 15.0, 1)[0], np.array([10.0, 1e-2], np.float32), None
    yield "sizes_R64", points, classes, full(64), R.real_frames(2, 65, frames_of, 25.0, 2, gain=0.7)[0], np.array([1.0, 1e-3], np.float32), \
        np.array([0.7, 0.7], np.float32)
    big = R.random_table(2048, 7)
    yield "M2048_R2", big, [(0, 2048)], full(2), R.real_frames(2, 70, big.astype(np.float64) @ np.array([1, 1j]), 30.0, 3)[0], \
        np.array([1.0, 1e-4], np.float32), None
    clf = LikelihoodClassifier(128)
    x, s2 = R.real_frames(3, 128, "16QAM", 10.0, 4)
    yield "C17_R64", clf.points, [d[1:] for d in clf.descriptors], clf.rot, x, s2, None
    many = R.random_table(100, 8)
    yield "C64_R1", many, [((7 * i) % 96, 1 + i % 5) for i in range(64)], full(1), R.real_frames(2, 257, "QPSK", 8.0, 5)[0], \
        np.array([0.2, 1e-4], np.float32), None
    yield "C1_R256", clf.points, [clf.descriptors[12][1:]], full(256), R.real_frames(2, 64, "16QAM", 40.0, 6)[0], \
        np.array([1e-4, 1e-1], np.float32), None


@pytest.mark.parametrize("case", list(_bounded_cases()), ids=lambda c: c[0])
def test_real_tables_stay_within_the_derived_bound(case):
    name, points, classes, rot, x, s2, gain = case
    for k, mode in enumerate(("max", "mean")):
        planar = k                                       # one layout per mode: the layouts differ in the loads only (test 1 has both)
        ref = R.reference_and_bound(x, s2, gain, points, classes, rot, mode)
        got = run(R.in_layout(x, planar), s2, gain, points, classes, rot, mode, planar)
        eL = check_against(got, ref, f"{name} {mode}")
        assert np.any(eL > 0)                            # (fp32 did round: the test is not vacuous)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. decisions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["max", "mean"])
def test_the_20_dB_frames_are_decided_as_the_definition_decides_them(mode):
    """make_dataset's 68 frames, uploaded as they are.  tests/test_likelihood_cpu.py has shown that the definition classifies all
    of them correctly and that every frame's margin exceeds twice the bound: pred must equal the definition's on every frame."""
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    X, Y, s2 = R.decision_set()
    ref = R.decision_reference(mode)
    clf = LikelihoodClassifier(128, mode=mode)
    got = run(X, s2, None, clf.points, [d[1:] for d in clf.descriptors], clf.rot, mode)
    check_against(got, ref, f"decision {mode}")
    assert np.array_equal(got["pred"], ref["pred"]) and np.array_equal(got["pred"], Y)
    # the same through the class
    xd = on_device(X)
    ll, table, best = clf(xd, sigma2=float(s2), return_rot=True, return_best=True)
    assert np.array_equal(ll.cpu().numpy().astype(np.float64), got["loglik"]) and np.array_equal(table.cpu().numpy().astype(np.float64), got["L"])
    assert best.dtype == torch.int32 and np.array_equal(best.cpu().numpy(), got["best_rot"])
    pred = clf.predict(xd, snr_db=R.DECISION_SNR_DB)
    assert pred.dtype == torch.int64 and np.array_equal(pred.cpu().numpy(), Y)
    assert same_bits(clf(xd, snr_db=torch.full((68,), R.DECISION_SNR_DB)), ll)


def _closed(frames, sigma2, gain, clf, tag):
    """Device frames -> predictions of the device and of the definition on the very same frames; they must agree on every
    frame, which the margins of these (keyed, hence fixed) frames allow: that is asserted too, as a property of the inputs."""
    s2 = sigma2.float().cpu().numpy()
    g = None if gain is None else gain.float().cpu().numpy()
    x = frames.cpu().numpy()
    ref = R.reference_and_bound(x, s2, g, clf.points, [d[1:] for d in clf.descriptors], clf.rot, clf.mode, planar=bool(clf.planar))
    ll = clf(frames, sigma2=sigma2, gain=gain).cpu().numpy().astype(np.float64)
    pred = clf.predict(frames, sigma2=sigma2, gain=gain).cpu().numpy()
    worst = ref["Ell"].max(axis=1)
    print(f"{tag}: smallest margin {R.margin(ref['loglik']).min():.3f}, largest bound {worst.max():.4f}")
    assert np.all(np.abs(ll - ref["loglik"]) <= ref["Ell"])
    assert np.all(R.margin(ref["loglik"]) > 2.0 * worst)
    assert np.array_equal(pred, ref["pred"])
    return pred


def test_the_loop_closes_on_the_device_from_the_generator():
    """FrameSynth -> clf with snr_db from the stream's own labels."""
    from vit_vs_raw_iq_amd import FrameSynth, LikelihoodClassifier, noise_for
    clf = LikelihoodClassifier(128)
    fs = FrameSynth(clf.class_names, snrs_db=(20.0,), length=128, seed=5, device=dev())
    raw, y, z = fs.generate(34, 0, 0)
    pred = _closed(raw, noise_for(z)[1], None, clf, "FrameSynth")
    assert np.array_equal(clf.predict(raw, snr_db=z).cpu().numpy(), pred)
    assert (pred == y.cpu().numpy()).mean() >= 0.9


def test_the_loop_closes_on_the_device_behind_receiver_and_carrier():
    """ShapedSynth -> Receiver (normalise=True) -> Carrier -> clf with noise_for(snr, normalised=True)."""
    from vit_vs_raw_iq_amd import Carrier, LikelihoodClassifier, Receiver, ShapedSynth, noise_for
    names = ["BPSK", "QPSK", "16QAM"]
    ws = ShapedSynth(names, snrs_db=(20.0,), length=1024, seed=11, sps=2, device=dev())
    raw, y, z = ws.generate(12, 0, 0)
    sym = Carrier(512, order=4, layout="interleaved")(Receiver.for_synth(ws, timing="energy")(raw))
    assert sym.shape == (12, 512, 2)
    clf = LikelihoodClassifier(512, classes=names, mode="mean")
    gain, s2 = noise_for(z, normalised=True)
    pred = _closed(sym, s2, gain, clf, "ShapedSynth -> Receiver -> Carrier")
    assert (pred == y.cpu().numpy()).mean() >= 0.9


# ---------------------------------------------------------------------------------------------------------------------------
# 4. isolation and robustness
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_frames_outputs_depend_on_neither_its_neighbours_nor_the_run():
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    clf = LikelihoodClassifier(130, classes=["BPSK", "8PSK", "16QAM", "64QAM"], rotations=16)
    args = (clf.points, [d[1:] for d in clf.descriptors], clf.rot)
    x, s2 = R.real_frames(3, 130, "16QAM", 12.0, 8)
    whole = run(x, s2, [1.0, 0.9, 1.1], *args, "mean")
    again = run(x, s2, [1.0, 0.9, 1.1], *args, "mean")
    for k in whole:
        assert np.array_equal(bits(whole[k]), bits(again[k])), k                              # run to run, bit for bit
    for b in range(3):
        alone = run(x[b:b + 1], s2[b:b + 1], [[1.0, 0.9, 1.1][b]], *args, "mean")
        for k in whole:
            assert np.array_equal(bits(whole[k][b:b + 1]), bits(alone[k])), (k, b)
    # a neighbour whose variance is refused: NaN and -1 there, not a bit elsewhere
    for bad in (0.0, np.nan, -1.0, np.inf):
        s2b = s2.copy()
        s2b[1] = bad
        got = run(x, s2b, [1.0, 0.9, 1.1], *args, "mean")
        assert np.isnan(got["loglik"][1]).all() and np.isnan(got["L"][1]).all() and np.all(got["best_rot"][1] == -1) and got["pred"][1] == -1
        for k in whole:
            assert np.array_equal(bits(got[k][[0, 2]]), bits(whole[k][[0, 2]])), (k, bad)
    # the optional outputs are optional
    only = run(x, s2, [1.0, 0.9, 1.1], *args, "mean", want=(False, False, False))
    assert np.array_equal(bits(only["loglik"]), bits(whole["loglik"]))


def test_refusals_return_their_code_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    lib = N.lib()
    ARG, UNSUPPORTED = 1, 2
    sentinel = 1234.5
    B, length = 2, 8192
    x = torch.zeros(B, length + 1, 2, device=dev())
    s2 = torch.ones(B, device=dev())
    points, rot = torch.zeros(2049, 2, device=dev()), torch.zeros(257, 2, device=dev())
    loglik, table = torch.full((B, 65), sentinel, device=dev()), torch.full((B, 65, 257), sentinel, device=dev())
    best, pred = torch.full((B, 65), ISENT, dtype=torch.int32, device=dev()), torch.full((B,), ISENT, dtype=torch.int32, device=dev())
    codes = []

    def call(n=B, length=length, classes=((0, 0, 4),), par="ok", **kw):
        ptrs = dict(x=x.data_ptr(), sigma2=s2.data_ptr(), loglik=loglik.data_ptr(), rot_ll=table.data_ptr(), best_rot=best.data_ptr(),
                    pred=pred.data_ptr())
        ptrs.update({k: kw.pop(k) for k in list(kw) if k in ptrs})
        arr = (N.SynthClass * len(classes))(*[N.SynthClass(*c) for c in classes])
        fields = dict(points=points.data_ptr(), classes=arr, n_classes=len(classes), rot=rot.data_ptr(), n_rot=64, planar=0, mode=0, gain=None)
        p = None if par is None else N.Likelihood(**{**fields, **kw})
        codes.append(lib.iq_frames_likelihood(ptrs["x"], ptrs["sigma2"], ptrs["loglik"], ptrs["rot_ll"], ptrs["best_rot"], ptrs["pred"], n,
                                              length, ctypes.byref(p) if p is not None else None, N.stream_handle()))
        return codes[-1]

    def refused():
        assert call(x=None) == ARG and call(sigma2=None) == ARG and call(loglik=None) == ARG and call(par=None) == ARG
        assert call(points=None) == ARG and call(rot=None) == ARG and call(length=0) == ARG and call(n_rot=0) == ARG
        assert call(planar=2) == ARG and call(mode=2) == ARG and call(mode=-1) == ARG
        assert call(x=x.data_ptr() + 4) == ARG and call(x=x.data_ptr() + 2, planar=1) == ARG and call(points=points.data_ptr() + 4) == ARG
        assert call(rot_ll=table.data_ptr() + 2) == ARG and call(gain=s2.data_ptr() + 1) == ARG
        assert call(classes=((1, 0, 4),)) == ARG and call(classes=((0, 0, 0),)) == ARG and call(classes=((0, -1, 4),)) == ARG
        # one past every limit
        assert call(classes=tuple((0, i, 1) for i in range(65))) == UNSUPPORTED
        assert call(n_rot=257) == UNSUPPORTED and call(classes=((0, 0, 2049),)) == UNSUPPORTED and call(length=8193) == UNSUPPORTED
        # nothing to do
        assert call(n=0) == 0 and call(n=-2) == 0
    assert kernel_launches(lib, refused) == {}                                                # not one launch
    torch.cuda.synchronize()
    for t, v in ((loglik, sentinel), (table, sentinel), (best, ISENT), (pred, ISENT)):
        assert torch.equal(t, torch.full_like(t, v))
    # the limits themselves run: 64 classes, 256 rotations, a 2048-point class, MAX_LENGTH symbols
    assert call(classes=tuple((0, i, 1) for i in range(64)), n_rot=2, length=64) == 0
    assert call(n_rot=256, length=64) == 0 and call(classes=((0, 0, 2048),), n_rot=1, length=64) == 0 and call(n_rot=1) == 0
    torch.cuda.synchronize()
    assert bool((pred[:B] == 0).all())                                                        # all-zero tables: every class ties
    clf = LikelihoodClassifier(8, classes=["BPSK"])
    empty = clf(torch.zeros(0, 8, 2, device=dev()), sigma2=1.0)
    assert empty.shape == (0, 1) and clf.predict(torch.zeros(0, 8, 2, device=dev()), sigma2=1.0).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. plumbing
# ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    """A capture fails on any host synchronisation: the classifier with all its outputs, and predict, are captured whole."""
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    clf = LikelihoodClassifier(130, classes=["QPSK", "16QAM", "32APSK"], rotations=32, mode="mean")
    x0 = on_device(R.real_frames(5, 130, "16QAM", 15.0, 3)[0])
    s2 = torch.full((5,), 0.03, device=dev())
    gain = torch.ones(5, device=dev())

    def go():
        ll, table, best = clf(x0, sigma2=s2, gain=gain, return_rot=True, return_best=True)
        return ll, table, best, clf.predict(x0, sigma2=s2)
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
    assert bool((eager[3] == 1).all())


def _expected_report(res, class_names, prefix):
    """The report file's text from a result dictionary, through the helpers the two evaluations share."""
    from vit_vs_raw_iq_amd.evaluation import TARGET_SNRS, classification_report_text, report_text
    K = len(class_names)
    y, p, z = res["labels"], res["predictions"], res["snrs"]
    cm = np.bincount(y * K + p, minlength=K * K).reshape(K, K)
    assert np.array_equal(cm, res["confusion_matrix"])
    snr_acc = {s: float(np.mean(p[np.abs(z - s) <= 0.5] == y[np.abs(z - s) <= 0.5])) for s in TARGET_SNRS if np.any(np.abs(z - s) <= 0.5)}
    assert snr_acc == pytest.approx(res["snr_accuracies"]) and list(snr_acc) == list(res["snr_accuracies"])
    return report_text(prefix, float(np.mean(p == y)), res["snr_accuracies"], classification_report_text(cm, class_names, digits=4))


def test_the_evaluation_writes_the_report_compare_models_reads(tmp_path):
    import re
    from vit_vs_raw_iq_amd import FrameSynth, LikelihoodClassifier
    from vit_vs_raw_iq_amd.evaluation import evaluate_likelihood_with_confusion
    names = ["BPSK", "QPSK", "8PSK", "16QAM"]
    clf = LikelihoodClassifier(128, classes=names, rotations=32)
    fs = FrameSynth(names, snrs_db=(0.0, 8.0, 20.0), length=128, seed=2, device=dev())
    loader = [fs.generate(24, 24 * i, 1) for i in range(2)]
    res = evaluate_likelihood_with_confusion(clf, loader, dev(), names, tmp_path, prefix="lik")
    text = (tmp_path / "lik_classification_report.txt").read_text()
    assert text == _expected_report(res, names, "lik")
    # the three patterns compare_models.py reads
    assert float(re.search(r"Overall Accuracy:\s+([\d.]+)%", text).group(1)) == pytest.approx(res["overall_accuracy"] * 100, abs=0.006)
    assert [int(s) for s in re.findall(r"SNR\s+([+-]?\d+)\s+dB:\s+[\d.]+%", text)] == [0, 8]
    assert re.search(r"weighted avg\s+[\d.]+\s+[\d.]+\s+[\d.]+\s+48", text)
    assert res["confusion_matrix"].sum() == 48 and res["overall_accuracy"] > 0.6 and res["snr_accuracies"][8] >= res["snr_accuracies"][0]
    assert np.array_equal(res["predictions"], torch.cat([clf.predict(x, snr_db=z) for x, _, z in loader]).cpu().numpy())
    with pytest.raises(ValueError):
        evaluate_likelihood_with_confusion(clf, loader, dev(), names[:3], tmp_path)


def test_the_model_evaluation_writes_what_it_wrote(tmp_path):
    """evaluate_model_with_confusion after the accumulation and the report moved into shared helpers: the file is, byte for byte,
    the text the parent's code wrote -- the header lines written out here as the parent had them, the table from
    classification_report_text -- and the result dictionary has the same entries."""
    from frontend_gpu import small_vit
    from vit_vs_raw_iq_amd.evaluation import classification_report_text, evaluate_model_with_confusion
    model = small_vit(1, 32, 32).train()
    names = ["a", "b", "c", "d"]
    g = torch.Generator().manual_seed(4)
    loader = [(torch.randn(16, 1, 32, 32, generator=g), torch.randint(0, 4, (16,), generator=g),
               torch.tensor([-8.0, 0.0, 8.0, 3.0]).repeat(4)) for _ in range(2)]
    res = evaluate_model_with_confusion(model, loader, dev(), names, tmp_path, prefix="test")
    assert model.training                                                                     # the mode it came in
    text = (tmp_path / "test_classification_report.txt").read_text()
    assert text == _expected_report(res, names, "test")
    parent = "Classification Report - Test Set\n" + "=" * 80 + "\n\n" + f"Overall Accuracy: {res['overall_accuracy'] * 100:.2f}%\n\n"
    parent += "Accuracy by SNR:\n" + "".join(f"  SNR {s:+3d} dB: {a * 100:.2f}%\n" for s, a in res["snr_accuracies"].items())
    parent += "\n" + "=" * 80 + "\n\n" + classification_report_text(res["confusion_matrix"], names, digits=4)
    assert text == parent
    assert sorted(res) == ["confusion_matrix", "labels", "overall_accuracy", "predictions", "snr_accuracies", "snrs"]
    assert list(res["snr_accuracies"]) == [-8, 0, 8] and res["labels"].shape == res["predictions"].shape == (32,)
    model.eval()
    with torch.no_grad():
        want = torch.cat([model(x.to(dev())).argmax(1) for x, _, _ in loader]).cpu().numpy()
    assert np.array_equal(res["predictions"], want)
