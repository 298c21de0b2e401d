"""GPU (MI355X): the hybrid likelihood classifier on the device (csrc/likelihood_em.hip, iq_frames_likelihood_em,
vit_vs_raw_iq_amd.likelihood_em).

Every call through the C ABI here (`run`) carves its operands out of NaN-filled buffers and its outputs out of sentinel-filled ones
and checks the guards, and that the operands hold what they held, afterwards.

1. Bit for bit: integer frames and points, given starts of powers of two, classes of one point or 2^j copies of it.  (h, v),
   best_start and pred equal the fp64 definition exactly after 0, 1 and 2 updates at power-of-two lengths, in both layouts and
   batches of 1 and 3.  Lambda holds a logarithm of pi v and cannot equal an fp64 value: where v is a power of two (no update) it
   equals the header's expression rounded as the header orders it (likelihood_em_ref.lambda_as_the_header_rounds_it: log2 of a
   power of two and of 1 are exact on the device), at those lengths and at the lane-chain edges; after an update v is no power
   of two, q rounds, and Lambda is held to the derived bound of its own pass (the state being exact).
2. Bounded: real tables against fp64.  One pass and one step under the one-pass bound derived in tests/likelihood_em_ref.py (a
   given start; the table's starts with the start's own rounding carried by the gradient); 8 steps under FACTOR times it, the
   allowance tests/test_likelihood_em_cpu.py measured against the reference on these very inputs and pinned.
3. Decisions: the 28 frames at 20 dB under an unknown gain, and ShapedSynth -> Receiver -> Carrier -> classifier, no noise argument
   anywhere.
4. Behaviour: scaling by a power of two, the floor on a noiseless frame, isolation, batch invariance, run-to-run identity,
   refusals, how pred passes NaN over.
5. hipGraph, estimate() into LikelihoodClassifier, the evaluation report.

best_start.  Starts that converge to the images of one optimum under the class's rotational symmetry are equal maxima in exact
arithmetic and only rounding orders them.  So best_start is held to: it is the first largest of the device's OWN start_ll (NaNs
passed over), exactly; that table is the definition's within the allowance; and it is one of the starts the definition puts
within the two allowances of its maximum (likelihood_em_ref.start_ties).  (h, v) are compared where the device took the
definition's start.
(The timing is scripts/likelihood_em_prof.py -> profiles/likelihood_em.txt; nothing is asserted about it.)
"""
import ctypes

import numpy as np
import pytest
import torch

import likelihood_em_ref as E
from frontend_gpu import ISENT, abi_call, dev, on_device
from prof_names import kernel_launches

pytestmark = pytest.mark.gpu

ALL = ("h", "v", "best_start", "start_ll", "pred", "snr_db")


def run(x, points, classes, starts, iters, f0=E.F0, floor=E.FLOOR, h0=None, v0=None, planar=0, want=ALL, expect_kernel=True):
    """One guarded iq_frames_likelihood_em call -> dict(loglik (B, C), h complex (B, C), v, best_start, start_ll (B, C, T), pred,
    snr_db), float64 / int64, None for what was not asked for."""
    import vit_vs_raw_iq_amd._native as N
    x = np.asarray(x, dtype=np.float32)
    B, length = x.shape[0], x.shape[2] if planar else x.shape[1]
    Cn, T = len(classes), 1 if h0 is not None else len(starts)
    arr = (N.SynthClass * Cn)(*[N.SynthClass(0, int(o), int(m)) for o, m in classes])

    def par(points, starts, h0, v0):
        return N.LikelihoodEm(points=points, classes=arr, n_classes=Cn, starts=starts, n_starts=T, iters=iters, planar=planar,
                              mode=int(h0 is not None), f0=f0, floor=floor, h0=h0, v0=v0)
    shapes = dict(h=(B, Cn, 2), v=(B, Cn), best_start=(np.int32, B, Cn), start_ll=(B, Cn, T), pred=(np.int32, B), snr_db=(B,))
    launches = {"frames_likelihood_em_kernel": 1, **({"likelihood_em_decide_kernel": 1} if "pred" in want or "snr_db" in want else {})}
    got = abi_call("iq_frames_likelihood_em", launches, (x,), [(B, Cn)] + [shapes[k] if k in want else None for k in ALL], B, length, par,
                   expect_kernel, side=(points, starts, h0, v0))
    out = dict(zip(("loglik",) + ALL, (None if a is None else a.astype(np.int64 if a.dtype == np.int32 else np.float64) for a in got)))
    if out["h"] is not None:
        out["h"] = out["h"][..., 0] + 1j * out["h"][..., 1]
    return out


def same(a, b):
    """Equal as fp64 values, NaN in the same places."""
    return np.array_equal(a, b, equal_nan=True)


def own_walk(got):
    """best_start, loglik and pred are the first largest of the device's OWN tables, NaNs passed over."""
    best, top = E.first_valid_largest(got["start_ll"], 2)
    assert np.array_equal(got["best_start"], best) and same(got["loglik"], top)
    assert np.array_equal(got["pred"], E.first_valid_largest(got["loglik"], 1)[0])


def check_against(got, ref, factor, tag, state=True):
    """The asserts every bounded comparison makes (the module's docstring has the reasons for best_start's)."""
    eL = np.abs(got["start_ll"] - ref["start_ll"])
    print(f"{tag}: |Lambda - ref| / allowance {float((eL / (factor * ref['ELam'])).max()):.4f} (allowance up to {factor * ref['ELam'].max():.2e}, "
          f"|Lambda| up to {np.abs(ref['start_ll']).max():.3g})")
    assert np.isfinite(got["start_ll"]).all() and np.all(eL <= factor * ref["ELam"]), tag
    own_walk(got)
    ties = E.start_ties(ref, factor)
    assert np.all(np.take_along_axis(ties, got["best_start"][..., None], axis=2)), tag
    single = ties.sum(axis=2) == 1
    assert np.array_equal(got["best_start"][single], ref["best_start"][single]), tag
    if state:
        at = got["best_start"] == ref["best_start"]
        eh, ev = np.abs(got["h"] - ref["h"])[at], np.abs(got["v"] - ref["v"])[at]
        print(f"{tag}: |h - ref| / allowance {float((eh / (factor * ref['Ehb'][at])).max()):.4f}, |v - ref| / allowance "
              f"{float((ev / (factor * ref['Evb'][at])).max()):.4f} on {int(at.sum())} of {at.size}")
        assert at.any() and np.all(eh <= factor * ref["Ehb"][at]) and np.all(ev <= factor * ref["Evb"][at]), tag
    snr = 10.0 * np.log10(np.abs(got["h"][np.arange(len(got["pred"])), got["pred"]]) ** 2 / got["v"][np.arange(len(got["pred"])), got["pred"]])
    assert np.allclose(got["snr_db"], snr, rtol=0, atol=1e-4), tag                  # (of the device's own h and v: 10 log10 within 1e-4 dB)
    return eL


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", E.EXACT_LENGTHS)
def test_integer_cases_are_exact(length):
    from vit_vs_raw_iq_amd import likelihood_em_reference
    for iters in (0, 1, 2):
        for n_frames in (1, 3):
            x, h0, v0 = E.exact_case(n_frames, length, 10 * length + 3 * iters + n_frames)
            ref = likelihood_em_reference(x, E.EXACT_POINTS, E.EXACT_CLASSES, None, iters, 0.5, 0.0, h0=h0, v0=v0)
            for planar in (0, 1):
                got = run(E.in_layout(x, planar), E.EXACT_POINTS, E.EXACT_CLASSES, None, iters, 0.5, 0.0, h0, v0, planar)
                tag = (length, iters, n_frames, planar)
                assert same(got["h"].real, ref.h.real) and same(got["h"].imag, ref.h.imag) and same(got["v"], ref.v), tag
                assert np.array_equal(got["best_start"], ref.best_start) and same(got["loglik"], got["start_ll"][..., 0]), tag
                own_walk(got)
                if iters == 0:
                    want = E.lambda_as_the_header_rounds_it(E.exact_L(x, h0, v0), v0.astype(np.float64), length)
                    assert same(got["loglik"], want) and np.all(got["best_start"] == 0), tag
                    assert same(got["h"].real, h0[..., 0].astype(np.float64)) and same(got["h"].imag, h0[..., 1].astype(np.float64)), tag
                    assert same(got["v"], v0.astype(np.float64)), tag
                else:                                    # the class of the origin is dead (Bq = 0) and pred passes it over
                    bound = E.reference_and_bound(x, E.EXACT_POINTS, E.EXACT_CLASSES, None, iters, 0.5, 0.0, h0, v0)
                    assert np.all(np.abs(got["loglik"] - ref.loglik)[:, :3] <= bound["Ell"][:, :3]), tag
                    assert np.isnan(got["loglik"][:, 3]).all() and np.isnan(got["h"][:, 3]).all() and np.isnan(got["v"][:, 3]).all(), tag
                    assert np.all(got["best_start"][:, 3] == -1) and np.all(got["pred"] >= 0) and np.all(got["pred"] < 3), tag
                    lead = np.sort(ref.loglik[:, :3], axis=1)
                    clear = lead[:, 2] - lead[:, 1] > 2.0 * bound["Ell"][:, :3].max(axis=1)
                    assert np.array_equal(got["pred"][clear], ref.pred[clear]), tag


@pytest.mark.parametrize("length", E.EXACT_EDGES)
def test_one_pass_is_exact_at_the_lane_chain_edges(length):
    """No update: nothing is divided, so any length is exact.  One and two symbols per lane step, the odd tail, a third step."""
    for n_frames, planar in ((1, 1), (3, 0)):
        x, h0, v0 = E.exact_case(n_frames, length, 7 * length + n_frames, tiled=False)
        got = run(E.in_layout(x, planar), E.EXACT_POINTS, E.EXACT_CLASSES, None, 0, 0.5, 0.0, h0, v0, planar)
        want = E.lambda_as_the_header_rounds_it(E.exact_L(x, h0, v0), v0.astype(np.float64), length)
        assert same(got["loglik"], want) and same(got["start_ll"][..., 0], want), (length, n_frames)
        assert same(got["h"].real, h0[..., 0].astype(np.float64)) and same(got["h"].imag, h0[..., 1].astype(np.float64))
        own_walk(got)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bounded
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(E.bounded_cases()), ids=lambda c: c[0])
def test_real_tables_stay_within_the_derived_bound(case):
    name, points, classes, starts, x = case
    # one pass from the table's starts: the derived bound, the starts' own rounding carried by the gradient
    ref = E.reference_and_bound(x, points, classes, starts, 0, E.F0, E.FLOOR)
    eL = check_against(run(x, points, classes, starts, 0), ref, 1.0, f"{name} table, one pass", state=False)
    assert np.any(eL > 0)                                # (fp32 did round: the test is not vacuous)
    # a given start: one pass, then one step, both under the derived bound
    h0, v0 = E.given_start(x, points, classes, 5)
    ref = E.reference_and_bound(E.in_layout(x, 1), points, classes, None, 0, E.F0, E.FLOOR, h0, v0, planar=True)
    got = run(E.in_layout(x, 1), points, classes, None, 0, h0=h0, v0=v0, planar=1)
    check_against(got, ref, 1.0, f"{name} given, one pass", state=False)
    assert same(got["h"].real, h0[..., 0].astype(np.float64)) and same(got["v"], v0.astype(np.float64))
    ref = E.reference_and_bound(x, points, classes, None, 1, E.F0, E.FLOOR, h0, v0)
    check_against(run(x, points, classes, None, 1, h0=h0, v0=v0), ref, 1.0, f"{name} given, one step")
    # eight steps from the table: the measured allowance
    ref = E.reference_and_bound(x, points, classes, starts, E.BOUNDED_ITERS, E.F0, E.FLOOR)
    check_against(run(E.in_layout(x, 1), points, classes, starts, E.BOUNDED_ITERS, planar=1), ref, E.FACTOR, f"{name} table, 8 steps")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. decisions
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_20_dB_frames_under_an_unknown_gain_are_decided_as_the_definition_decides_them():
    """tests/test_likelihood_em_cpu.py has shown that the definition classifies the set, that at most 2 % of it is too close to
    call and that the allowance of Lambda holds on every frame of it: every other frame must be decided as the definition decides
    it.  (The state is not compared here: its allowance is pinned on the bounded cases only.)"""
    X, Y, gain = E.decision_set()
    ref, clf = E.decision_reference(), E.decision_classifier()
    got = run(X, clf.points, [d[1:] for d in clf.descriptors], clf.starts, clf.iters)
    check_against(got, ref, E.FACTOR, "decision set", state=False)     # (the allowance is pinned for Lambda on this set, not for the state)
    ok = E.decided(ref)
    assert ok.mean() >= 1.0 - E.DECISION_CAP and np.array_equal(got["pred"][ok], ref["pred"][ok])
    # the same through the class
    xd = on_device(X)
    ll, h, v, best, table = clf(xd, return_estimates=True, return_starts=True)
    assert same(ll.cpu().numpy().astype(np.float64), got["loglik"]) and same(table.cpu().numpy().astype(np.float64), got["start_ll"])
    assert best.dtype == torch.int32 and np.array_equal(best.cpu().numpy(), got["best_start"])
    assert same((h.cpu().numpy().astype(np.float64) @ np.array([1, 1j])), got["h"]) and same(v.cpu().numpy().astype(np.float64), got["v"])
    pred = clf.predict(xd)
    assert pred.dtype == torch.int64 and np.array_equal(pred.cpu().numpy(), got["pred"])
    p2, snr, sigma2, g = clf.estimate(xd)
    assert torch.equal(p2, pred) and same(snr.cpu().numpy().astype(np.float64), got["snr_db"])
    at = (np.arange(len(X)), got["pred"])
    assert same(sigma2.cpu().numpy().astype(np.float64), got["v"][at])
    assert np.allclose(g.cpu().numpy(), np.abs(got["h"][at]), rtol=1e-6)
    print(f"estimated SNR: median {np.median(got['snr_db']):.2f} dB, gain error up to {np.abs(np.abs(got['h'][at]) / gain - 1).max():.3f}")


def test_the_chain_from_the_waveform_is_decided_with_no_noise_argument():
    """ShapedSynth -> Receiver -> Carrier -> classifier; the definition is evaluated on the very symbols the device produced."""
    from vit_vs_raw_iq_amd import Carrier, HybridLikelihoodClassifier, Receiver, ShapedSynth
    names = ["BPSK", "QPSK", "16QAM"]
    ws = ShapedSynth(names, snrs_db=(20.0,), length=1024, seed=11, sps=2, device=dev())
    raw, y, z = ws.generate(12, 0, 0)
    sym = Carrier(512, order=4, layout="interleaved")(Receiver.for_synth(ws, timing="energy")(raw))
    clf = HybridLikelihoodClassifier(512, classes=names)
    args = (sym.cpu().numpy(), clf.points, [d[1:] for d in clf.descriptors], clf.starts, clf.iters, E.F0, E.FLOOR)
    _, _, rl, ref = E.amplification(*args, patterns=E.PATTERNS[:2])                      # (the clean run is the reference)
    ratio = np.nanmax(rl)
    print(f"chain: deviation of Lambda / one-pass bound under injection: {ratio:.1f}")
    assert 2.0 * ratio <= E.CHAIN_FACTOR                 # a property of these (keyed, hence fixed) frames, measured against the reference
    ll, table = clf(sym, return_starts=True)
    used = np.abs(table.cpu().numpy() - ref["start_ll"]) / (E.CHAIN_FACTOR * ref["ELam"])
    ok = E.decided(ref, E.CHAIN_FACTOR)
    pred = clf.predict(sym).cpu().numpy()
    print(f"chain: |Lambda - ref| / allowance {used.max():.4f}, {int(ok.sum())} of {len(ok)} decided, accuracy {(pred == y.cpu().numpy()).mean():.3f}")
    assert np.all(used <= 1.0)
    assert ok.mean() >= 1.0 - E.DECISION_CAP and np.array_equal(pred[ok], ref["pred"][ok])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. behaviour
# ---------------------------------------------------------------------------------------------------------------------------
def _small():
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier
    clf = HybridLikelihoodClassifier(130, classes=["BPSK", "8PSK", "16QAM", "64QAM"], starts=5, iters=6)
    return clf, (clf.points, [d[1:] for d in clf.descriptors], clf.starts, clf.iters), E.real_frames(3, 130, "16QAM", 12.0, 8, gain=1.3)[0]


def test_a_power_of_two_scales_the_estimates_exactly_and_moves_no_decision():
    """Every product, sum and quotient of the definition is homogeneous in the frame (h by 2^j, v and d by 4^j, q by 4^-j, every
    exponent unchanged), so scaling by a power of two changes exponents only -- except in Lambda, whose log2(v) does not round
    alike at another exponent.  With ONE start (h, v), pred and best_start are held exactly.  With the table's starts, two that
    converge to two images of one optimum tie in exact arithmetic and Lambda's rounding orders them, so there best_start may move
    -- but only inside the set the definition itself puts within the two allowances of its maximum
    (likelihood_em_ref.start_ties, on a bounded case, where the allowance is pinned); where it did not move, (h, v) scale
    exactly; pred never moves.  The floor scales with the frame and is not hit."""
    name, points, classes, starts, x = list(E.bounded_cases())[1]
    args = (points, classes, starts, E.BOUNDED_ITERS)
    ties = E.start_ties(E.reference_and_bound(x, *args, E.F0, E.FLOOR), E.FACTOR)
    base = run(x, *args)
    one = run(x, points, classes, starts[3:4], E.BOUNDED_ITERS)
    for j in (-3, 2):
        got = run(x * np.float32(2.0 ** j), *args)
        assert np.array_equal(got["pred"], base["pred"]) and np.allclose(got["snr_db"], base["snr_db"], rtol=0, atol=1e-4)
        assert np.all(np.take_along_axis(ties, got["best_start"][..., None], axis=2))
        at = got["best_start"] == base["best_start"]
        print(f"scale 2^{j}: best_start kept on {int(at.sum())} of {at.size}")
        assert same(got["h"][at], base["h"][at] * 2.0 ** j) and same(got["v"][at], base["v"][at] * 4.0 ** j)
        assert np.array_equal(got["best_start"][ties.sum(axis=2) == 1], base["best_start"][ties.sum(axis=2) == 1])
        alone = run(x * np.float32(2.0 ** j), points, classes, starts[3:4], E.BOUNDED_ITERS)
        assert same(alone["h"], one["h"] * 2.0 ** j) and same(alone["v"], one["v"] * 4.0 ** j) and np.array_equal(alone["pred"], one["pred"])
        assert not alone["best_start"].any()
    assert np.all(base["v"] > 10 * float(E.FLOOR) * np.mean(np.abs(E.to_complex(x)) ** 2, axis=1)[:, None])      # the floor was not hit


def test_a_noiseless_frame_ends_at_the_floor_times_its_power():
    """The frame's symbols ARE the class's points times a power-of-two gain g: the EM ends at h = g and V = 0, so v' is the floor,
    floor * M2, and with integer points, |s|^2 = 2 and floor = 2^-20 both are exact in fp32: (h, v) bit for bit, at a length
    on and off the lane-chain edge.  A class that cannot explain the frame stays far above its floor."""
    from vit_vs_raw_iq_amd import likelihood_em_reference
    pts = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1], [1, 0], [-1, 0]], np.float32)
    classes, floor = [(0, 4), (4, 2)], np.float32(2.0 ** -20)
    rng = np.random.default_rng(3)
    g = np.array([0.25, 4.0, 1.0])
    for length, planar in ((64, 0), (130, 1)):
        x = (pts[rng.integers(0, 4, (3, length))] * g[:, None, None]).astype(np.float32)
        M2 = 2.0 * g ** 2
        h0 = np.stack([np.stack([0.75 * g, 0.125 * g], axis=1)] * 2, axis=1).astype(np.float32)
        v0 = np.stack([M2 / 4] * 2, axis=1).astype(np.float32)
        ref = likelihood_em_reference(x, pts, classes, None, 8, 0.5, floor, h0=h0, v0=v0)
        assert np.array_equal(ref.h[:, 0], g + 0j) and np.array_equal(ref.v[:, 0], float(floor) * M2)        # (of the definition)
        got = run(E.in_layout(x, planar), pts, classes, None, 8, 0.5, floor, h0, v0, planar)
        assert same(got["h"][:, 0], g + 0j) and same(got["v"][:, 0], float(floor) * M2), length
        assert np.all(got["v"][:, 1] > 0.25 * M2) and np.all(got["pred"] == 0)
        assert np.allclose(got["snr_db"], 10 * np.log10(g ** 2 / (float(floor) * M2)), rtol=0, atol=1e-4)
        none = run(E.in_layout(x, planar), pts, classes, None, 8, 0.5, 0.0, h0, v0, planar)                  # no floor: V = 0 is no variance
        assert np.isnan(none["loglik"][:, 0]).all() and np.all(none["pred"] == 1)


def test_a_frames_outputs_depend_on_neither_its_neighbours_nor_the_run():
    clf, args, x = _small()
    whole, again = run(x, *args), run(x, *args)
    for k in whole:
        assert same(whole[k], again[k]), k                                                       # run to run, every bit (the values are fp32's)
    for b in range(3):
        alone = run(x[b:b + 1], *args)
        for k in whole:
            assert same(whole[k][b:b + 1], alone[k]), (k, b)
    # a NaN sample, an all-zero frame and a frame of subnormal power next to good ones: NaN, -1 there, not a bit elsewhere
    for kind in ("nan", "zero", "tiny"):                 # (tiny: its power is below the smallest normal fp32 number: no variance)
        xb = x.copy()
        if kind == "nan":
            xb[1, 77, 1] = np.nan
        elif kind == "zero":
            xb[1] = 0.0
        else:
            xb[1] *= np.float32(2.0 ** -70)
        got = run(xb, *args)
        assert np.isnan(got["loglik"][1]).all() and np.isnan(got["h"][1]).all() and np.isnan(got["v"][1]).all() and np.isnan(got["start_ll"][1]).all()
        assert np.all(got["best_start"][1] == -1) and got["pred"][1] == -1 and np.isnan(got["snr_db"][1])
        for k in whole:
            assert same(got[k][[0, 2]], whole[k][[0, 2]]), (k, kind)
    # the optional outputs are optional
    only = run(x, *args, want=())
    assert same(only["loglik"], whole["loglik"]) and all(only[k] is None for k in ALL)
    some = run(x, *args, want=("pred", "start_ll"))
    assert same(some["start_ll"], whole["start_ll"]) and np.array_equal(some["pred"], whole["pred"])


def test_pred_passes_a_class_no_state_explains_over():
    """A class of the origin alone dies at its first update (Bq = 0): NaN there, and the frame is decided among the others -- also
    where the dead class comes first; a frame whose every class is dead gets -1."""
    x = E.real_frames(2, 64, "QPSK", 15.0, 9)[0]
    pts = np.array([[0, 0], [1, 0], [-1, 0], [0.7071, 0.7071], [-0.7071, 0.7071], [-0.7071, -0.7071], [0.7071, -0.7071]], np.float32)
    from vit_vs_raw_iq_amd.likelihood import rotation_table
    starts = rotation_table(2 * np.pi * np.arange(8) / 8)
    got = run(x, pts, [(0, 1), (1, 2), (3, 4)], starts, 32)
    assert np.isnan(got["loglik"][:, 0]).all() and np.all(got["best_start"][:, 0] == -1) and np.isfinite(got["loglik"][:, 1:]).all()
    # (64 symbols estimate the variance to 1 / sqrt(64) = 12 %, half a dB: 3 dB is six of those)
    assert np.all(got["pred"] == 2) and np.isfinite(got["snr_db"]).all() and np.all(np.abs(got["snr_db"] - 15.0) < 3.0)
    dead = run(x, pts, [(0, 1)], starts, 4)
    assert np.isnan(dead["loglik"]).all() and np.all(dead["pred"] == -1) and np.isnan(dead["snr_db"]).all()
    alive = run(x, pts, [(0, 1)], starts, 0)             # without an update the origin is a class like any other
    assert np.isfinite(alive["loglik"]).all() and np.all(alive["pred"] == 0)


def test_refusals_return_their_code_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier
    lib = N.lib()
    ARG, UNSUPPORTED = 1, 2
    sentinel = 1234.5
    B, length = 2, 8192
    x = torch.zeros(B, length + 1, 2, device=dev())
    points, starts = torch.zeros(2049, 2, device=dev()), torch.zeros(257, 2, device=dev())
    fl = lambda *s: torch.full(s, sentinel, device=dev())                                      # noqa: E731
    il = lambda *s: torch.full(s, ISENT, dtype=torch.int32, device=dev())                      # noqa: E731
    bufs = dict(loglik=fl(B, 65), h=fl(B, 65, 2), v=fl(B, 65), best_start=il(B, 65), start_ll=fl(B, 65, 257), pred=il(B), snr_db=fl(B))
    h0, v0 = torch.ones(B, 65, 2, device=dev()), torch.ones(B, 65, device=dev())

    def call(n=B, length=length, classes=((0, 0, 4),), par="ok", **kw):
        ptrs = dict(x=x.data_ptr(), **{k: t.data_ptr() for k, t in bufs.items()})
        ptrs.update({k: kw.pop(k) for k in list(kw) if k in ptrs})
        arr = (N.SynthClass * len(classes))(*[N.SynthClass(*c) for c in classes])
        fields = dict(points=points.data_ptr(), classes=arr, n_classes=len(classes), starts=starts.data_ptr(), n_starts=16, iters=2, planar=0,
                      mode=0, f0=0.02, floor=1e-6, h0=None, v0=None)
        p = None if par is None else N.LikelihoodEm(**{**fields, **kw})
        return lib.iq_frames_likelihood_em(ptrs["x"], *(ptrs[k] for k in ("loglik",) + ALL), n, length,
                                           ctypes.byref(p) if p is not None else None, N.stream_handle())

    def refused():
        assert call(x=None) == ARG and call(loglik=None) == ARG and call(par=None) == ARG and call(points=None) == ARG
        assert call(starts=None) == ARG and call(n_starts=0) == ARG and call(mode=1) == ARG and call(mode=1, h0=h0.data_ptr()) == ARG
        assert call(mode=2) == ARG and call(mode=-1) == ARG and call(length=0) == ARG and call(iters=-1) == ARG and call(planar=2) == ARG
        assert call(h=None) == ARG and call(v=None) == ARG                                       # snr_db reads them
        for f0 in (0.0, 1.0, -0.1, float("nan")):
            assert call(f0=f0) == ARG
        assert call(floor=-1e-6) == ARG and call(floor=float("inf")) == ARG and call(floor=float("nan")) == ARG
        assert call(x=x.data_ptr() + 4) == ARG and call(x=x.data_ptr() + 2, planar=1) == ARG and call(points=points.data_ptr() + 4) == ARG
        assert call(h=bufs["h"].data_ptr() + 4) == ARG and call(start_ll=bufs["start_ll"].data_ptr() + 2) == ARG
        assert call(mode=1, h0=h0.data_ptr() + 4, v0=v0.data_ptr()) == ARG and call(mode=1, h0=h0.data_ptr(), v0=v0.data_ptr() + 2) == ARG
        assert call(classes=((1, 0, 4),)) == ARG and call(classes=((0, 0, 0),)) == ARG and call(classes=((0, -1, 4),)) == ARG
        # one past every limit
        assert call(classes=tuple((0, i, 1) for i in range(65))) == UNSUPPORTED and call(n_starts=257) == UNSUPPORTED
        assert call(classes=((0, 0, 2049),)) == UNSUPPORTED and call(length=8193) == UNSUPPORTED and call(iters=4097) == UNSUPPORTED
        # nothing to do
        assert call(n=0) == 0 and call(n=-2) == 0
    assert kernel_launches(lib, refused) == {}                                                # not one launch
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t, torch.full_like(t, ISENT if t.dtype == torch.int32 else sentinel)), k
    # the limits themselves run: 64 classes, 256 starts, a 2048-point class with MAX_LENGTH symbols (the largest LDS), a given start
    assert call(classes=tuple((0, i, 1) for i in range(64)), n_starts=2, length=64) == 0
    assert call(n_starts=256, iters=0, length=64) == 0 and call(classes=((0, 0, 2048),), n_starts=4, iters=1) == 0
    assert call(mode=1, h0=h0.data_ptr(), v0=v0.data_ptr(), starts=None, n_starts=0, length=64) == 0
    assert call(snr_db=None, h=None, v=None, best_start=None, start_ll=None, pred=None, length=64) == 0
    torch.cuda.synchronize()
    assert bool((bufs["pred"] == -1).all())                                                    # all-zero frames: M2 = 0, every class dead
    clf = HybridLikelihoodClassifier(8, classes=["BPSK"])
    empty = torch.zeros(0, 8, 2, device=dev())
    assert clf(empty).shape == (0, 1) and clf.predict(empty).shape == (0,) and all(t.shape[0] == 0 for t in clf.estimate(empty))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. plumbing
# ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    """A capture fails on any host synchronisation: the classifier with all its outputs, a given start, and estimate, captured whole."""
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier
    clf = HybridLikelihoodClassifier(130, classes=["QPSK", "16QAM", "32APSK"], starts=8, iters=12)
    x0 = on_device(E.real_frames(5, 130, "16QAM", 15.0, 3, gain=0.6)[0])

    def go():
        ll, h, v, best, table = clf(x0, return_estimates=True, return_starts=True)
        warm = clf(x0, h0=h, v0=v)                        # a warm start from the estimates
        return (ll, h, v, best, table, warm) + clf.estimate(x0)
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
    # more steps never lower the likelihood (in exact arithmetic; Lambda's own rounding is far below a thousandth of it)
    assert bool((eager[5] >= eager[0] - 1e-3 * eager[0].abs()).all())


def test_estimate_gives_the_likelihood_classifier_what_it_lacked():
    """LikelihoodClassifier handed the hybrid's (sigma2, gain) decides the decision set as it does handed the truth (which
    tests/test_likelihood_em_cpu.py has shown of the two definitions)."""
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    X, Y, gain = E.decision_set()
    clf = E.decision_classifier()
    lik = LikelihoodClassifier(128, classes=clf.class_names)
    xd = on_device(X)
    pred, snr, sigma2, g = clf.estimate(xd)
    truth = lik.predict(xd, sigma2=torch.from_numpy((gain ** 2 * 10.0 ** (-E.DECISION_SNR_DB / 10.0)).astype(np.float32)),
                        gain=torch.from_numpy(gain.astype(np.float32)))
    blind = lik.predict(xd, sigma2=sigma2, gain=g)
    assert torch.equal(blind, truth) and np.array_equal(truth.cpu().numpy(), Y)
    assert abs(float(snr.median()) - E.DECISION_SNR_DB) < 1.0


def test_the_evaluation_writes_the_report_compare_models_reads(tmp_path):
    import re
    from test_gpu_likelihood import _expected_report
    from vit_vs_raw_iq_amd import FrameSynth, HybridLikelihoodClassifier
    from vit_vs_raw_iq_amd.evaluation import evaluate_hybrid_with_confusion
    names = ["BPSK", "QPSK", "8PSK", "16QAM"]
    clf = HybridLikelihoodClassifier(128, classes=names, starts=8, iters=16)
    fs = FrameSynth(names, snrs_db=(0.0, 8.0, 20.0), length=128, seed=2, device=dev())
    loader = [fs.generate(24, 24 * i, 1) for i in range(2)]
    res = evaluate_hybrid_with_confusion(clf, loader, dev(), names, tmp_path, prefix="hyb")
    text = (tmp_path / "hyb_classification_report.txt").read_text()
    assert text == _expected_report(res, names, "hyb")
    assert float(re.search(r"Overall Accuracy:\s+([\d.]+)%", text).group(1)) == pytest.approx(res["overall_accuracy"] * 100, abs=0.006)
    assert [int(s) for s in re.findall(r"SNR\s+([+-]?\d+)\s+dB:\s+[\d.]+%", text)] == [0, 8]
    assert re.search(r"weighted avg\s+[\d.]+\s+[\d.]+\s+[\d.]+\s+48", text)
    assert res["confusion_matrix"].sum() == 48
    assert np.array_equal(res["predictions"], torch.cat([clf.predict(x) for x, _, _ in loader]).cpu().numpy())
    with pytest.raises(ValueError):
        evaluate_hybrid_with_confusion(clf, loader, dev(), names[:3], tmp_path)
