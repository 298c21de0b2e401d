"""GPU (MI355X): the blind equaliser on the device (csrc/equaliser.hip, iq_frames_equalise / _bwd, vit_vs_raw_iq_amd.equaliser).

Every call through the C ABI here (`forward`, `backward`) carves its operands out of NaN-filled buffers and its outputs out of
sentinel-filled ones and checks the guards afterwards.

1. GIVEN: integer frames and weights -- out equals the fp64 definition bit for bit at every length edge, tap count and layout.
2. CMA, one and two steps, on integer frames that keep every intermediate an fp32 number (tests/equaliser_ref.py, checked on the
   host): w_out, out and est equal the definition bit for bit.
3. Chaining: iters = T is T calls of iters = 1 fed w_out -> w0; iters = 0 is GIVEN with w0.  Bit for bit, on real frames.
4. One step from an arbitrary w0 on real frames against fp64, under the bound derived in tests/equaliser_ref.py.
5. A whole run at the defaults: ||w - w_ref||_2 within iters times the one-step bound (no expansion: checked on the host).
7. Closed loop: ShapedSynth (sps 2, 4 channel taps, 20 dB) -> Receiver -> Equaliser: w and J(after) against the definition's own
   run, under allowances scaled by the growth factor of those frames; then Carrier and Constellation.
8. Adjoint identity in integers, x.grad.  9. Isolation.  10. Refusals.  11. hipGraph, SynthStream, train_on_stream.
(6, the timing, is scripts/equaliser_prof.py -> profiles/equaliser.txt; nothing is asserted about it.)
"""
import ctypes

import numpy as np
import pytest
import torch

import equaliser_ref as R
from frontend_gpu import abi_call, bits, dev, on_device, same_bits

pytestmark = pytest.mark.gpu

IDENT = dict(i_mean=0.0, i_std=1.0, q_mean=0.0, q_std=1.0)


def forward(x, L, iters=0, mu=0.0, modulus=1.0, planar=0, w=None, w0=None, want=(True, True), expect_kernel=True):
    """One guarded iq_frames_equalise call -> dict(out, w, est) as float64 numpy.  w: IQ_EQ_GIVEN."""
    import vit_vs_raw_iq_amd._native as N
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, length = x.shape[0], x.shape[2] if planar else x.shape[1]
    assert all(a is None or np.shape(a) == (B, L, 2) for a in (w, w0))

    def par(w, w0):
        return N.Equaliser(taps=L, iters=iters, planar=planar, mode=0 if w is not None else 1, mu=mu, modulus=modulus, w=w, w0=w0)
    got = abi_call("iq_frames_equalise", f"frames_equalise_kernel<{L}>", (x,),
                   [x.shape, (B, L, 2) if want[0] else None, (B, 4) if want[1] else None], B, length, par, expect_kernel, side=(w, w0))
    return dict(zip(("out", "w", "est"), (None if a is None else a.astype(np.float64) for a in got)))


def backward(dout, w, planar=0, mode=0):
    """One guarded iq_frames_equalise_bwd call -> dx float64."""
    import vit_vs_raw_iq_amd._native as N
    dout, w = np.ascontiguousarray(dout, dtype=np.float32), np.ascontiguousarray(w, dtype=np.float32)
    B, length, L = dout.shape[0], dout.shape[2] if planar else dout.shape[1], w.shape[1]

    def par(w):
        return N.Equaliser(taps=L, iters=3, planar=planar, mode=mode, mu=0.5, modulus=1.0, w=w, w0=None)
    return abi_call("iq_frames_equalise_bwd", f"frames_equalise_bwd_kernel<{L}>", (dout,), dout.shape, B, length, par,
                    side=(w,)).astype(np.float64)


def in_layout(x, planar):
    """(B, len, 2) -> the layout asked for."""
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1))) if planar else x


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. GIVEN, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [0, 1])
@pytest.mark.parametrize("L", [1, 2, 3, 11, 31, 32])
def test_given_integer_frames_and_weights_are_exact(L, planar):
    """Frames in [-3, 3], weights in [-2, 2]: every term and every partial sum of y is a small integer.  J is a sum of squares up
    to 10^11 and is not exact: it stays within the relative error of its sum of positive terms, gamma_k, k = ceil(len / 256) +
    11 (the thread's chain, 6 + 2 levels of adds, the square inside the fmaf, the division; d itself is exact)."""
    from vit_vs_raw_iq_amd import equaliser_reference, equaliser_reference_bwd
    for length in sorted({1, 2, L - 1, L, L + 1, 255, 256, 257, 1023, 1025, 8192} - {0}):
        B = 2
        x = R.integer_frames(B, length, 100 * L + length, planar=bool(planar))
        w = R.integer_weights(B, L, length)
        out_ref, w_ref, est_ref = equaliser_reference(x, L, 0, 0.0, planar=bool(planar), w=w)
        got = forward(x, L, iters=7, mu=0.25, planar=planar, w=w)
        assert np.array_equal(got["out"], out_ref), (L, length)
        assert np.array_equal(got["w"], w_ref) and np.all(np.isnan(got["est"][:, 0])) and np.array_equal(got["est"][:, 2:], est_ref[:, 2:])
        assert np.all(np.abs(got["est"][:, 1] - est_ref[:, 1]) <= R.gamma(-(-length // 256) + 11) * est_ref[:, 1]), (L, length)
        # the adjoint on the same integers
        assert np.array_equal(backward(x, w, planar), equaliser_reference_bwd(x, w, bool(planar))), (L, length)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. CMA, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.EXACT_CMA, ids=lambda c: f"len{c[0]}_L{c[1]}_R{c[3]}")
def test_one_and_two_steps_on_integer_frames_are_exact(case):
    from vit_vs_raw_iq_amd import equaliser_reference
    length, L, ratio, modulus, off, seeds, steps = case
    x, mu = R.exact_cma_case(length, L, ratio, modulus, off, seeds)
    for iters in range(1, steps + 1):
        for planar in (0, 1):
            xl = in_layout(x, planar)
            out_ref, w_ref, est_ref = equaliser_reference(xl, L, iters, mu, float(modulus), planar=bool(planar))
            assert np.array_equal(f32(w_ref), w_ref) and np.array_equal(f32(out_ref), out_ref) and np.array_equal(f32(est_ref), est_ref)
            got = forward(xl, L, iters, mu, float(modulus), planar)
            assert np.array_equal(got["w"], w_ref), (iters, planar)
            assert np.array_equal(got["out"], out_ref), (iters, planar)
            assert np.array_equal(got["est"], est_ref), (iters, planar, got["est"], est_ref)
    assert R.moves(x, L, mu, modulus, steps)                                             # (no step leaves w where it was)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. chaining identities
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,name,L,planar", [(3, "qpsk", 11, 0), (5, "8psk", 4, 1), (5, "qpsk_1025", 32, 0)])
def test_T_steps_are_T_calls_of_one_step(T, name, L, planar):
    x = in_layout(R.run_frames(name), planar)
    mu = 0.2
    whole = forward(x, L, T, mu, 1.0, planar)
    w0, first = None, None
    for t in range(T):
        step = forward(x, L, 1, mu, 1.0, planar, w0=w0)
        first = step if first is None else first
        w0 = step["w"]
    assert np.array_equal(bits(step["w"]), bits(whole["w"])) and np.array_equal(bits(step["out"]), bits(whole["out"]))
    assert np.array_equal(bits(step["est"][:, 1:]), bits(whole["est"][:, 1:])) and np.array_equal(bits(first["est"][:, 0]), bits(whole["est"][:, 0]))
    assert np.any(whole["w"] != first["w"])
    # iters = 0 is GIVEN with w0, but for est[0]
    zero = forward(x, L, 0, mu, 1.0, planar, w0=whole["w"])
    given = forward(x, L, T, mu, 1.0, planar, w=whole["w"])
    for k in ("out", "w"):
        assert np.array_equal(bits(zero[k]), bits(given[k])) and np.array_equal(bits(zero[k]), bits(whole[k]))
    assert np.array_equal(bits(zero["est"][:, 1:]), bits(given["est"][:, 1:])) and np.all(np.isnan(given["est"][:, 0]))
    assert np.array_equal(bits(zero["est"][:, 0]), bits(zero["est"][:, 1]))
    # no start given: the unit spike at L // 2
    spike = forward(x, L, T, mu, 1.0, planar, w0=R.weights(R.spike(len(x), L)))
    assert np.array_equal(bits(spike["w"]), bits(whole["w"])) and np.array_equal(bits(spike["est"]), bits(whole["est"]))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. one step against fp64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L,planar,modulus", [("qpsk", 11, 0, 1.0), ("8psk", 4, 1, 1.0), ("qpsk_1025", 32, 0, 1.25), ("qpsk", 1, 1, 1.0)])
def test_one_step_from_an_arbitrary_start_stays_within_the_derived_bound(name, L, planar, modulus):
    from vit_vs_raw_iq_amd import equaliser_reference
    xs = R.run_frames(name)
    z = R.to_complex(xs)
    B = len(z)
    rng = np.random.default_rng(L)
    w0 = R.weights(R.spike(B, L) + 0.3 * (rng.standard_normal((B, L)) + 1j * rng.standard_normal((B, L))))
    w0c = w0[:, :, 0].astype(np.float64) + 1j * w0[:, :, 1]
    mu = float(np.float32(0.2))
    x = in_layout(xs, planar)
    out_ref, w_ref, est_ref = equaliser_reference(x, L, 1, mu, modulus, planar=bool(planar), w0=w0)
    dw, dJ = R.one_step_bound(z, w0c, mu, modulus)
    got = forward(x, L, 1, mu, modulus, planar, w0=w0)
    err = np.abs(got["w"] - w_ref).max(axis=2)
    eJ = np.abs(got["est"][:, 0] - est_ref[:, 0])
    print(f"{name} L {L}: |w - ref| / bound {float((err / dw).max()):.4f} (bound {dw.max():.2e}), |J - ref| / bound {float((eJ / dJ).max()):.4f}")
    assert np.all(err <= dw) and np.all(eJ <= dJ)
    assert np.any(err > 0)                                                                # (fp32 did round: the test is not vacuous)
    # out and J(after) at the device's own weights
    wd = got["w"][:, :, 0] + 1j * got["w"][:, :, 1]
    out_own, _, est_own = equaliser_reference(x, L, 0, 0.0, modulus, planar=bool(planar), w=got["w"])
    dy = R.filter_bound(z, wd)
    eo = np.abs(R.to_complex(got["out"], bool(planar)) - R.to_complex(out_own, bool(planar)))
    assert np.all(np.abs(eo.real) <= dy) and np.all(np.abs(eo.imag) <= dy)
    assert np.all(np.abs(got["est"][:, 1] - est_own[:, 1]) <= R.one_step_bound(z, wd, mu, modulus)[1])
    assert np.all(np.abs(got["est"][:, 2] - est_own[:, 2]) <= R.gamma(2 * L) * est_own[:, 2]) and np.array_equal(got["est"][:, 3], est_own[:, 3])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a whole run at the defaults
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.RUNS))
def test_a_whole_run_at_the_defaults_drifts_no_further_than_its_steps_allow(name):
    from vit_vs_raw_iq_amd import Equaliser, equaliser_reference
    xs = R.run_frames(name)
    z = R.to_complex(xs)
    B, n = z.shape
    eq = Equaliser(n)
    assert (eq.taps, eq.iters, eq.mu) == (11, 64, 0.2)
    mu = float(np.float32(eq.mu))
    out, w, est = eq(on_device(xs), return_w=True, return_est=True)
    out_ref, w_ref, est_ref = equaliser_reference(xs, eq.taps, eq.iters, mu)
    allowed, step = R.run_bound(z, R.spike(B, eq.taps), mu, 1.0, eq.iters)
    wd = w.cpu().numpy().astype(np.float64)
    drift = R.norm2((wd - w_ref)[:, :, 0] + 1j * (wd - w_ref)[:, :, 1])
    e = est.cpu().numpy().astype(np.float64)
    print(f"{name}: ||w - ref||_2 {drift.max():.3e} of {allowed.min():.3e} allowed ({float((drift / step).max()):.2f} one-step bounds); "
          f"median J {np.median(e[:, 0]):.4f} -> {np.median(e[:, 1]):.4f} (definition {np.median(est_ref[:, 1]):.4f})")
    assert np.all(drift <= allowed)
    same = forward(xs, eq.taps, eq.iters, eq.mu, 1.0, 0)
    assert np.array_equal(same["w"], wd) and np.array_equal(same["out"], out.cpu().numpy().astype(np.float64)) and np.array_equal(same["est"], e)
    # J(after) and out: the definition at the device's own weights
    wc = wd[:, :, 0] + 1j * wd[:, :, 1]
    out_own, _, est_own = equaliser_reference(xs, eq.taps, 0, 0.0, w=wd)
    assert np.all(np.abs(e[:, 1] - est_own[:, 1]) <= R.one_step_bound(z, wc, mu, 1.0)[1])
    eo = np.abs(R.to_complex(out.cpu().numpy()) - R.to_complex(out_own))
    assert np.all(np.maximum(np.abs(eo.real), np.abs(eo.imag)) <= R.filter_bound(z, wc))
    assert np.all(e[:, 1] < e[:, 0]) and np.array_equal(e[:, 3], est_ref[:, 3])


# ---------------------------------------------------------------------------------------------------------------------------
# 7. closed loop
# ---------------------------------------------------------------------------------------------------------------------------
def check_closed_loop(sym, tag, cap=None):
    """sym: device (B, 512, 2) received symbols of one class -> the asserts of test 7; returns out.  cap: the growth factor
    asserted for these frames on the host (R.CLOSED_GROWTH); None: the factor is measured here, in fp64, on these very frames
    (a property of the definition's iteration, not of the device).  The allowances are derived in tests/equaliser_ref.py: the
    weights may differ from the definition's by G * iters one-step bounds, J(after) by what that ball of weights can move J
    plus the bound of evaluating J once."""
    from vit_vs_raw_iq_amd import Equaliser, equaliser_reference
    eq = Equaliser(sym.shape[1])
    out, w, est = eq(sym, return_w=True, return_est=True)
    e, wd = est.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
    xs = sym.cpu().numpy()
    z, wc = R.to_complex(xs), wd[:, :, 0] + 1j * wd[:, :, 1]
    mu = float(np.float32(eq.mu))
    _, w_ref, est_ref = equaliser_reference(xs, eq.taps, eq.iters, mu)
    wr = w_ref[:, :, 0] + 1j * w_ref[:, :, 1]
    G, allowed, step = R.growth(z, R.spike(len(z), eq.taps), mu, 1.0, eq.iters)
    if cap is not None:
        assert np.all(G <= cap)                                                           # (what the host test asserted)
        allowed = cap * eq.iters * step
    _, _, est_own = equaliser_reference(xs, eq.taps, 0, 0.0, w=wd)
    dJ0 = R.one_step_bound(z, R.spike(len(z), eq.taps), mu, 1.0)[1]
    dJ1 = R.one_step_bound(z, wc, mu, 1.0)[1]
    dJw = R.j_drift_bound(z, wr, allowed, 1.0)
    drift = R.norm2(wc - wr)
    eJ = np.abs(e[:, 1] - est_ref[:, 1])
    print(f"{tag}: median J {np.median(e[:, 0]):.4f} -> {np.median(e[:, 1]):.4f} (definition's own run {np.median(est_ref[:, 1]):.4f}); "
          f"growth {G.max():.2f}; ||w - w_ref||_2 {drift.max():.2e} of {allowed.min():.2e} allowed ({float((drift / step).max()):.2f} one-step "
          f"bounds); |J(after) - definition's run| {eJ.max():.2e} of {(dJw + dJ1).min():.2e} allowed; "
          f"|J - definition at these weights| / bound {float((np.abs(e[:, 1] - est_own[:, 1]) / dJ1).max()):.3f}")
    assert np.all(e[:, 1] <= e[:, 0])
    assert np.all(np.abs(e[:, 0] - est_ref[:, 0]) <= dJ0)
    assert np.all(drift <= allowed)                                                       # the 64 steps, against the definition's
    assert np.all(eJ <= dJw + dJ1)
    assert np.all(np.abs(e[:, 1] - est_own[:, 1]) <= dJ1)                                 # and the last filter and J alone
    assert np.median(e[:, 0]) >= 2 * np.median(e[:, 1])
    return out


_DEVICE_FRAMES = {}


def device_symbols():
    """ShapedSynth (BPSK, QPSK, 8PSK; sps 2, 4 channel taps, 20 dB, 1024 samples) -> Receiver, 24 frames per class: made once."""
    if not _DEVICE_FRAMES:
        from vit_vs_raw_iq_amd import Receiver, ShapedSynth
        ws = ShapedSynth(list(R.CLOSED["classes"]), snrs_db=(20.0,), length=1024, seed=11, sps=2, taps=4, device=dev())
        raw, y, _ = ws.generate(72, 0, 0)
        _DEVICE_FRAMES["sym"], _DEVICE_FRAMES["y"] = Receiver.for_synth(ws, timing="energy")(raw), y
    return _DEVICE_FRAMES["sym"], _DEVICE_FRAMES["y"]


@pytest.mark.parametrize("k,cls", list(enumerate(R.CLOSED["classes"])))
def test_the_loop_closes_on_the_device(k, cls):
    """ShapedSynth -> Receiver -> Equaliser at the defaults, on the device's own frames.  On every frame J(after) <= J(before);
    J(before) is the definition's within the derived bound; the weights and J(after) are those of the definition's own 64 steps
    within the allowance scaled by the growth factor of these frames (on which the early steps expand an error, see
    tests/test_equaliser_cpu.py); J(after) is also the definition's at the device's own weights within the bound of one
    evaluation; the median J falls at least twofold."""
    sym, y = device_symbols()
    assert sym.shape == (72, 512, 2)
    out = check_closed_loop(sym[y == k].contiguous(), cls)
    assert out.shape == (24, 512, 2)


def test_the_equalised_symbols_go_through_carrier_and_constellation():
    """equaliser -> carrier -> constellation through Synchronised: the image is finite, and is the chain written out."""
    from vit_vs_raw_iq_amd import Carrier, Constellation, Equaliser, Synchronised
    sym, _ = device_symbols()
    sy = Synchronised(Constellation(32, 32, 512), Carrier(512, order=4), equaliser=Equaliser(512, layout="planar"))
    planar = sym.transpose(1, 2).contiguous()
    img = sy(planar)
    assert img.shape == (72, 1, 32, 32) and bool(torch.isfinite(img).all()) and float(img.abs().max()) > 0
    assert same_bits(img, sy.front(sy.carrier(sy.equaliser(planar))))
    # the planar equaliser computes what the other layout's does
    assert same_bits(sy.equaliser(planar).transpose(1, 2).contiguous(), Equaliser(512)(sym))
    sy.fit(planar)
    fitted = sy(planar)
    assert abs(float(fitted.mean())) < 1e-3 and abs(float(fitted.std()) - 1.0) < 1e-3


@pytest.mark.parametrize("cls", R.CLOSED["classes"])
def test_the_frames_of_the_host_test_close_the_loop_on_the_device_too(cls):
    """The keyed frames tests/test_equaliser_cpu.py took through the three definitions, through the device's receiver and
    equaliser, under the growth factor asserted for them there."""
    from vit_vs_raw_iq_amd import Receiver
    raw, ws, _ = R.closed_loop_raw(cls)
    rx = Receiver.for_synth(ws, timing="energy", device=dev())
    check_closed_loop(rx(on_device(raw)), cls + " (host frames)", cap=R.CLOSED_GROWTH[cls])


# ---------------------------------------------------------------------------------------------------------------------------
# 8. adjoint
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,length,planar", [(11, 300, 0), (32, 1025, 1), (2, 5, 0), (3, 1, 1)])
def test_adjoint_identity_is_exact_on_integers(L, length, planar):
    B = 3
    x = R.integer_frames(B, length, L, planar=bool(planar))
    dout = R.integer_frames(B, length, L + 1, planar=bool(planar))
    w = R.integer_weights(B, L, 5)
    out = forward(x, L, planar=planar, w=w)["out"]
    dx = backward(dout, w, planar, mode=1)                                               # (the mode is not looked at)
    assert np.array_equal(out, np.rint(out)) and np.array_equal(dx, np.rint(dx))
    lhs, rhs = (out.astype(np.int64) * dout.astype(np.int64)).sum(), (x.astype(np.int64) * dx.astype(np.int64)).sum()
    assert lhs == rhs and lhs != 0


@pytest.mark.parametrize("layout", ["frames", "planar"])
def test_gradients_reach_the_frame_with_the_weights_held_fixed(layout):
    from vit_vs_raw_iq_amd import Equaliser, equaliser_reference_bwd
    xs = in_layout(R.run_frames("qpsk"), layout == "planar")
    dh = np.random.default_rng(8).standard_normal(xs.shape).astype(np.float32)
    eq = Equaliser(300, layout=layout)
    x = on_device(xs).requires_grad_()
    out, w = eq(x, return_w=True)
    assert not w.requires_grad
    (dx,) = torch.autograd.grad(out, x, on_device(dh))
    wd = w.cpu().numpy()
    assert np.array_equal(dx.cpu().numpy().astype(np.float64), backward(dh, wd, eq.planar))
    ref = equaliser_reference_bwd(dh, wd, bool(eq.planar))
    z = R.to_complex(dh, bool(eq.planar))
    dy = R.filter_bound(z, wd[:, :, 0].astype(np.float64) + 1j * wd[:, :, 1], adjoint=True)
    err = R.to_complex(dx.cpu().numpy(), bool(eq.planar)) - R.to_complex(ref, bool(eq.planar))
    assert np.all(np.maximum(np.abs(err.real), np.abs(err.imag)) <= dy)
    # given the forward's weights the forward is the same, and two runs agree bit for bit
    assert same_bits(eq(x.detach(), w=w), out.detach())
    out2, w2 = eq(x.detach(), return_w=True)
    assert same_bits(out2, out.detach()) and same_bits(w2, w)


def test_gradients_through_synchronised_are_the_chain_written_out():
    from vit_vs_raw_iq_amd import Carrier, Constellation, Equaliser, Synchronised
    con, cr, eq = Constellation(32, 64, 300), Carrier(300, order=4), Equaliser(300, layout="planar")
    sy = Synchronised(con, cr, equaliser=eq)
    x0 = on_device(in_layout(R.run_frames("qpsk"), 1))
    g = on_device(np.random.default_rng(1).standard_normal((12, 1, 32, 64)))
    x = x0.clone().requires_grad_()
    (dx,) = torch.autograd.grad(sy(x), x, g)
    mid, w = eq(x0, return_w=True)
    mid2 = mid.detach().requires_grad_()
    (dmid,) = torch.autograd.grad(con(cr(mid2)), mid2, g)
    assert float(dx.abs().max()) > 0
    assert np.array_equal(dx.cpu().numpy().astype(np.float64), backward(dmid.cpu().numpy(), w.cpu().numpy(), 1))


# ---------------------------------------------------------------------------------------------------------------------------
# 9. isolation
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_frames_outputs_depend_on_neither_the_batch_nor_its_position():
    from vit_vs_raw_iq_amd import Equaliser
    xs = R.run_frames("qpsk")
    eq = Equaliser(300, iters=8)
    big = np.tile(xs, (22, 1, 1))[:257]                                                  # frame k is xs[k % 12]
    big[5] = 0.0
    x257 = on_device(big)
    r257 = eq(x257, return_w=True, return_est=True)
    r1 = eq(x257[7:8], return_w=True, return_est=True)
    r3 = eq(x257[6:9], return_w=True, return_est=True)
    for a, b, c in zip(r1, r3, r257):
        assert same_bits(a, b[1:2]) and same_bits(a, c[7:8]) and same_bits(a, c[19:20]) and same_bits(a, c[247:248])
    assert same_bits(r257[0][256:257], r257[0][4:5])                                      # 256 % 12 == 4
    assert not r257[0][5].any() and r257[2][5].tolist() == [1.0, 1.0, 1.0, 5.0]          # the zero frame: g = 0, J = R^2, the spike
    # a NaN frame poisons only itself
    bad = x257[:5].clone()
    bad[1, 17, 0] = float("nan")
    again = eq(bad, return_w=True, return_est=True)
    for a, c in zip(again, r257):
        assert same_bits(a[[0, 2, 3, 4]], c[[0, 2, 3, 4]])
    assert bool(torch.isnan(again[0][1]).all()) and bool(torch.isnan(again[1][1]).all()) and bool(torch.isnan(again[2][1, :3]).all())
    given = eq(bad, w=r257[1][:5], return_est=True)                                       # GIVEN: only the outputs the sample reaches
    assert int(torch.isnan(given[0][1, :, 0]).sum()) == 11 and same_bits(given[0][[0, 2, 3, 4]], r257[0][[0, 2, 3, 4]])
    assert eq(x257[:0]).shape == (0, 300, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_leave_the_outputs_untouched():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import Equaliser
    lib = N.lib()
    sentinel = 1234.5
    B, length = 3, 8192
    eq = Equaliser(length, taps=32, iters=2)
    x = torch.zeros(B, length, 2, device=dev())
    big = torch.zeros(8193 * 2 + 4, device=dev())
    out, w_out, est = (torch.full(s, sentinel, device=dev()) for s in ((B, length, 2), (B, 32, 2), (B, 4)))
    w = torch.zeros(B, 32, 2, device=dev())
    ARG, UNSUPPORTED = 1, 2
    ptrs = dict(x=x.data_ptr(), out=out.data_ptr(), w_out=w_out.data_ptr(), est=est.data_ptr())

    def fwd(length=length, par="ok", n=B, **kw):
        p = dict(ptrs)
        fields = {k: kw.pop(k) for k in list(kw) if k not in p}
        p.update(kw)
        if par == "ok":
            par = eq.struct(w.data_ptr(), w.data_ptr(), mode=1)
            for k, v in fields.items():
                setattr(par, k, v)
        return lib.iq_frames_equalise(p["x"], p["out"], p["w_out"], p["est"], n, length, ctypes.byref(par) if par is not None else None,
                                      N.stream_handle())

    def bwd(length=length, par="ok", n=B, **kw):
        p = dict(dout=x.data_ptr(), dx=out.data_ptr())
        fields = {k: kw.pop(k) for k in list(kw) if k not in p}
        p.update(kw)
        if par == "ok":
            par = eq.struct(w.data_ptr(), w.data_ptr(), mode=0)
            for k, v in fields.items():
                setattr(par, k, v)
        return lib.iq_frames_equalise_bwd(p["dout"], p["dx"], n, length, ctypes.byref(par) if par is not None else None, N.stream_handle())
    assert fwd(x=None) == ARG and fwd(out=None) == ARG and fwd(par=None) == ARG
    assert bwd(dout=None) == ARG and bwd(dx=None) == ARG and bwd(par=None) == ARG
    for call in (fwd, bwd):
        assert call(taps=0) == ARG and call(taps=-1) == ARG and call(length=0) == ARG and call(length=-1) == ARG and call(iters=-1) == ARG
        for bad in (float("inf"), float("nan")):
            assert call(mu=bad) == ARG and call(modulus=bad) == ARG
        assert call(mu=-0.25) == ARG and call(planar=2) == ARG and call(planar=-1) == ARG and call(mode=2) == ARG and call(mode=-1) == ARG
        assert call(w=w.data_ptr() + 2) == ARG and call(w0=w.data_ptr() + 2) == ARG
        # every edge of what is supported: one past it is refused
        assert call(taps=33) == UNSUPPORTED and call(iters=4097) == UNSUPPORTED
    assert fwd(x=big.data_ptr(), length=8193) == UNSUPPORTED and bwd(dout=big.data_ptr(), length=8193) == UNSUPPORTED
    assert fwd(x=x.data_ptr() + 4) == ARG and fwd(out=out.data_ptr() + 4) == ARG and bwd(dout=x.data_ptr() + 4) == ARG and bwd(dx=out.data_ptr() + 4) == ARG
    assert fwd(x=x.data_ptr() + 2, planar=1) == ARG and fwd(out=out.data_ptr() + 2, planar=1) == ARG
    assert fwd(w_out=w_out.data_ptr() + 2) == ARG and fwd(est=est.data_ptr() + 2) == ARG
    assert fwd(mode=0, w=None) == ARG and bwd(w=None) == ARG and bwd(w=None, mode=1) == ARG
    torch.cuda.synchronize()
    for t in (out, w_out, est):
        assert torch.equal(t, torch.full_like(t, sentinel))
    assert fwd(n=0) == 0 and fwd(n=-2) == 0 and bwd(n=0) == 0 and fwd(n=0, w=None, w0=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, sentinel))
    # the edges themselves run: 32 taps at 8192 samples; 4096 steps; the optional outputs may be NULL and w0 too
    assert fwd(w_out=None, est=None, w0=None) == 0 and bwd() == 0
    small = Equaliser(8, taps=1, iters=4096, mu=0.0)
    xs = on_device(R.integer_frames(2, 8, 3))
    o, e = small(xs, return_est=True)
    assert same_bits(o, xs) and torch.equal(e[:, 0], e[:, 1])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# 11. plumbing
# ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    """A capture fails on any host synchronisation: equaliser -> carrier -> constellation and the adjoints are captured whole."""
    from vit_vs_raw_iq_amd import Carrier, Constellation, Equaliser, Synchronised
    eq = Equaliser(300, layout="planar")
    sy = Synchronised(Constellation(32, 64, 300), Carrier(300, order=4), equaliser=eq)
    x0 = on_device(in_layout(R.run_frames("8psk"), 1))
    g = on_device(np.random.default_rng(2).standard_normal((12, 1, 32, 64)))

    def run():
        x = x0.clone().requires_grad_()
        img = sy(x)
        (dx,) = torch.autograd.grad(img, x, g)
        out, w, est = eq(x0, return_w=True, return_est=True)
        return img.detach(), dx, out, w, est
    eager = run()                                         # also: the carrier's tables are on the device before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = run()
    for t in held:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(held, eager):
        assert torch.equal(a, b)


def test_received_synth_with_both_stages_goes_into_the_stream_and_a_training_step():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import Carrier, Equaliser, ReceivedSynth, Receiver, ShapedSynth, SynthStream, train_on_stream
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    ws = ShapedSynth(["BPSK", "QPSK", "8PSK"], snrs_db=(20.0,), length=1024, seed=3, sps=2, taps=4, device=dev())
    rx = Receiver.for_synth(ws, timing="energy")
    eq, cr = Equaliser(512), Carrier(512, order=4, layout="interleaved")
    rs = ReceivedSynth(ws, rx, equaliser=eq, carrier=cr)
    B, s = 12, 2
    raw, y, z = ws.generate(B, s * B, 0)
    want = cr(eq(rx(raw)))
    got = rs.generate(B, s * B, 0)
    assert len(got) == 3 and same_bits(got[0], want) and torch.equal(got[1], y)
    assert same_bits(ReceivedSynth(ws, rx, equaliser=eq).generate(B, s * B, 0)[0], eq(rx(raw)))
    assert same_bits(ReceivedSynth(ws, rx, carrier=cr).generate(B, s * B, 0)[0], cr(rx(raw)))
    assert same_bits(ReceivedSynth(ws, rx).generate(B, s * B, 0)[0], rx(raw))
    sym, _, _, est = rs.generate(B, s * B, 0, return_est=True)
    assert same_bits(sym, want) and same_bits(est, rx(raw, return_est=True)[1])
    x, ys, zs = SynthStream(rs, IDENT, "rawiq", B).get(s)
    assert x.shape == (B, 2, 512) and same_bits(x, want.transpose(1, 2).contiguous()) and torch.equal(ys, y) and same_bits(zs, z)
    torch.manual_seed(0)
    m = P.AMCTransformerRawIQ(in_channels=2, seq_length=512, num_classes=3, d_model=128, n_head=8, n_layers=2, ffn_hidden=256,
                              drop_prob=0.0, device="cuda", use_cls_token=True, embedding_type="segment", segment_size=16)
    tr = FusedTrainer(m.to(dev()).train(), lr=1e-3, weight_decay=1e-3)
    assert train_on_stream(tr, SynthStream(rs, IDENT, "rawiq", 24), 1) == 1
    loss, acc, frames = tr.read_stats()
    assert frames == 24 and np.isfinite(loss)
