"""GPU (MI355X): the tracking equaliser on the device (csrc/equaliser_track.hip, iq_frames_equalise_track / _bwd,
vit_vs_raw_iq_amd.equaliser_track).

Every call through the C ABI here (`forward`, `backward`) carves its operands out of NaN-filled buffers and its outputs out of
sentinel-filled ones and checks the guards afterwards.

1. No steps: out has the bits of iq_frames_equalise under IQ_EQ_GIVEN with w = w0, in both layouts.
2. GIVEN: integer frames and weights and a power-of-two hop -- out and the adjoint equal the fp64 definition bit for bit at every
   segment, lane-chain and tap edge; a hop that is no power of two under the derived bound.
3. One and two segment steps on integer frames: w_out, out and est equal the fp32 restatement (tests/equaliser_track_ref.py) bit
   for bit.
4. One step and 8 steps on real frames against fp64, under the derived one-step bound and TRACK_GROWTH * 8 of them.
5. Adjoint identity in integers; autograd is the ABI call.  6. Isolation.  7. Refusals.  8. hipGraph, ReceivedSynth(FadedSynth)
   through SynthStream.  9. The closed loop on the device behind the moving channel.
(The timing is scripts/equaliser_track_prof.py -> profiles/equaliser_track.txt; nothing is asserted about it.)
"""
import ctypes

import numpy as np
import pytest
import torch

import equaliser_ref as E
import equaliser_track_ref as T
from frontend_gpu import abi_call, bits, dev, on_device, same_bits

pytestmark = pytest.mark.gpu

IDENT = dict(i_mean=0.0, i_std=1.0, q_mean=0.0, q_std=1.0)


def forward(x, L, seg, hop, iters=0, mu=0.0, modulus=1.0, planar=0, w=None, w0=None, taper=None, want_est=True):
    """One guarded iq_frames_equalise_track call -> dict(out, w, est) as float64 numpy.  w: IQ_EQT_GIVEN."""
    import vit_vs_raw_iq_amd._native as N
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, length = x.shape[0], x.shape[2] if planar else x.shape[1]
    S = T.n_segments(length, seg, hop)
    assert (w is None or np.shape(w) == (B, S, L, 2)) and (w0 is None or np.shape(w0) == (B, L, 2)) and (taper is None or np.shape(taper) == (seg,))

    def par(w, w0, taper):
        return N.EqualiserTrack(taps=L, iters=iters, planar=planar, mode=0 if w is not None else 1, seg=seg, hop=hop, mu=mu, modulus=modulus,
                                w=w, w0=w0, taper=taper)
    launches = {"track_filter_kernel": 1} if w is not None else {f"track_descent_kernel<{L}>": 1, "track_filter_kernel": 1}
    got = abi_call("iq_frames_equalise_track", launches, (x,), [x.shape, (B, S, L, 2), (B, 4) if want_est else None], B, length, par,
                   side=(w, w0, taper))
    return dict(zip(("out", "w", "est"), (None if a is None else a.astype(np.float64) for a in got)))


def backward(dout, w, seg, hop, planar=0, mode=0):
    """One guarded iq_frames_equalise_track_bwd call -> dx float64."""
    import vit_vs_raw_iq_amd._native as N
    dout, w = np.ascontiguousarray(dout, dtype=np.float32), np.ascontiguousarray(w, dtype=np.float32)
    B, length, L = dout.shape[0], dout.shape[2] if planar else dout.shape[1], w.shape[2]

    def par(w):
        return N.EqualiserTrack(taps=L, iters=3, planar=planar, mode=mode, seg=seg, hop=hop, mu=0.5, modulus=1.0, w=w, w0=None, taper=None)
    return abi_call("iq_frames_equalise_track_bwd", "track_bwd_kernel", (dout,), dout.shape, B, length, par, side=(w,)).astype(np.float64)


def block_given(x, w, planar):
    """iq_frames_equalise under IQ_EQ_GIVEN -> out, est float64."""
    import vit_vs_raw_iq_amd._native as N
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, L, length = x.shape[0], w.shape[1], x.shape[2] if planar else x.shape[1]

    def par(w):
        return N.Equaliser(taps=L, iters=0, planar=planar, mode=0, mu=0.0, modulus=1.0, w=w, w0=None)
    out, _, est = abi_call("iq_frames_equalise", f"frames_equalise_kernel<{L}>", (x,), [x.shape, None, (B, 4)], B, length, par, side=(w,))
    return out.astype(np.float64), est.astype(np.float64)


def in_layout(x, planar):
    """(B, len, 2) -> the layout asked for."""
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1))) if planar else x


def cplx(w):
    return w[..., 0].astype(np.float64) + 1j * w[..., 1]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. no steps
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [0, 1])
@pytest.mark.parametrize("name,L,seg,hop", [("qpsk", 11, 128, 64), ("qpsk_1025", 32, 512, 100), ("8psk", 1, 7, 3)])
def test_no_steps_give_the_bits_of_the_block_filter(name, L, seg, hop, planar):
    from vit_vs_raw_iq_amd import taper_table
    xs = E.run_frames(name)
    rng = np.random.default_rng(L)
    w0 = E.weights(E.spike(len(xs), L) + 0.3 * (rng.standard_normal((len(xs), L)) + 1j * rng.standard_normal((len(xs), L))))
    x = in_layout(xs, planar)
    got = forward(x, L, seg, hop, iters=0, mu=0.25, planar=planar, w0=w0, taper=taper_table(seg))
    out, est = block_given(x, w0, planar)
    S = T.n_segments(xs.shape[1], seg, hop)
    assert np.array_equal(bits(got["out"]), bits(out))
    assert np.array_equal(bits(got["w"]), bits(np.repeat(w0[:, None], S, axis=1)))
    assert np.array_equal(bits(got["est"][:, 1]), bits(est[:, 1])) and np.array_equal(bits(got["est"][:, 0]), bits(est[:, 1]))
    assert not got["est"][:, 2].any() and np.all(got["est"][:, 3] == S)
    # no start given: the unit spike, i.e. the frame itself
    spike = forward(x, L, seg, hop, iters=0, planar=planar, taper=taper_table(seg), want_est=False)
    assert np.array_equal(bits(spike["out"]), bits(x)) and spike["est"] is None


# ---------------------------------------------------------------------------------------------------------------------------
# 2. GIVEN
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.GIVEN_EXACT, ids=lambda c: f"len{c[0]}_seg{c[1]}_hop{c[2]}_L{c[3]}")
def test_given_integer_frames_and_weights_are_exact(case):
    """Frames in [-3, 3], weights in [-2, 2], hop a power of two: every word of w(n), every term and every partial sum of y is an
    fp32 number (tests/test_equaliser_track_cpu.py), in the forward and in the adjoint.  J is a sum of squares and is not exact: it
    stays within gamma_k of its sum of positive terms, k = ceil(len / 256) + 11 (as for the block kernel)."""
    from vit_vs_raw_iq_amd import equaliser_track_reference, equaliser_track_reference_bwd
    n, seg, hop, L = case
    S = T.n_segments(n, seg, hop)
    B = 2 if n < 8192 else 1
    for planar in ((0, 1) if n < 8192 else (n // seg % 2,)):
        x = E.integer_frames(B, n, n + L, planar=bool(planar))
        w = T.integer_segment_weights(B, S, L, n)
        out_ref, w_ref, est_ref = equaliser_track_reference(x, L, 0, 0.0, seg, hop, np.ones(seg), planar=bool(planar), w=w)
        got = forward(x, L, seg, hop, iters=7, mu=0.25, planar=planar, w=w)
        assert np.array_equal(got["out"], out_ref), (case, planar)
        assert np.array_equal(got["w"], w_ref) and np.all(np.isnan(got["est"][:, [0, 2]])) and np.all(got["est"][:, 3] == S)
        assert np.all(np.abs(got["est"][:, 1] - est_ref[:, 1]) <= E.gamma(-(-n // 256) + 11) * est_ref[:, 1]), (case, planar)
        assert np.array_equal(backward(x, w, seg, hop, planar), equaliser_track_reference_bwd(x, w, seg, hop, bool(planar))), (case, planar)
    if S > 1:                                              # (the weights do differ between the segments: interpolation happened)
        assert np.any(w[:, 0] != w[:, -1])


@pytest.mark.parametrize("case", T.GIVEN_ODD_HOP, ids=lambda c: f"len{c[0]}_seg{c[1]}_hop{c[2]}_L{c[3]}")
def test_given_with_a_hop_that_is_no_power_of_two_stays_within_the_bound(case):
    from vit_vs_raw_iq_amd import equaliser_track_reference, equaliser_track_reference_bwd
    n, seg, hop, L = case
    S = T.n_segments(n, seg, hop)
    x, w = E.integer_frames(2, n, n + L), T.integer_segment_weights(2, S, L, n)
    z = E.to_complex(x)
    got = forward(x, L, seg, hop, w=w)
    err = E.to_complex(got["out"]) - E.to_complex(equaliser_track_reference(x, L, 0, 0.0, seg, hop, np.ones(seg), w=w)[0])
    dy = T.filter_bound_t(z, cplx(w), seg, hop)
    assert np.all(np.maximum(np.abs(err.real), np.abs(err.imag)) <= dy)
    erb = E.to_complex(backward(x, w, seg, hop)) - E.to_complex(equaliser_track_reference_bwd(x, w, seg, hop))
    assert np.all(np.maximum(np.abs(erb.real), np.abs(erb.imag)) <= T.filter_bound_t(z, cplx(w), seg, hop, adjoint=True))
    assert np.any(err != 0) or L == 1                      # (fp32 did round)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. segment steps, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.EXACT_CMA, ids=lambda c: f"len{c[0]}_seg{c[1]}_hop{c[2]}_L{c[3]}")
def test_one_and_two_segment_steps_equal_the_fp32_restatement(case):
    n, seg, hop, L, mu, R, off, seeds, steps = case
    x, h = T.exact_cma_case(n, seg, hop, L, mu, R, off, seeds)
    for iters in range(1, steps + 1):
        for planar in (0, 1):
            xl = in_layout(x, planar)
            out, w, est = T.restate32(xl, L, iters, mu, seg, hop, h, float(R), planar=bool(planar))
            got = forward(xl, L, seg, hop, iters, mu, float(R), planar, taper=h)
            assert np.array_equal(bits(got["w"]), bits(w)), (iters, planar)
            assert np.array_equal(bits(got["out"]), bits(out)), (iters, planar)
            assert np.array_equal(bits(got["est"]), bits(est)), (iters, planar, got["est"], est)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. real frames against fp64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L,planar,seg,hop,kind", T.BOUNDED)
def test_one_step_and_eight_steps_stay_within_the_derived_bounds(name, L, planar, seg, hop, kind):
    from vit_vs_raw_iq_amd import equaliser_track_reference, taper_table
    xs = E.run_frames(name)
    z = E.to_complex(xs)
    h = taper_table(seg, kind)
    w0 = T.bounded_start(name, L)
    w0c = cplx(w0)
    mu = float(np.float32(T.BOUNDED_MU))
    x = in_layout(xs, planar)
    S = T.n_segments(xs.shape[1], seg, hop)
    # one step
    ref = equaliser_track_reference(x, L, 1, mu, seg, hop, h, planar=bool(planar), w0=w0)
    got = forward(x, L, seg, hop, 1, mu, 1.0, planar, w0=w0, taper=h)
    dw = T.segment_step_bound(z, np.repeat(w0c[:, None], S, axis=1), mu, 1.0, seg, hop, h)
    err = cplx(got["w"] - ref[1])
    print(f"{name} L {L} {seg}/{hop}: one step |w - ref| / bound {float((np.maximum(np.abs(err.real), np.abs(err.imag)) / dw).max()):.4f} (bound {dw.max():.2e})")
    assert np.all(np.abs(err.real) <= dw) and np.all(np.abs(err.imag) <= dw) and np.any(err != 0)
    # 8 steps
    ws = T.trajectory(z, w0c, mu, 1.0, T.BOUNDED_STEPS, seg, hop, h)
    step = np.max([T.norm2(T.segment_step_bound(z, w, mu, 1.0, seg, hop, h)) for w in ws[:-1]], axis=0)
    ref8 = equaliser_track_reference(x, L, T.BOUNDED_STEPS, mu, seg, hop, h, planar=bool(planar), w0=w0)
    got8 = forward(x, L, seg, hop, T.BOUNDED_STEPS, mu, 1.0, planar, w0=w0, taper=h)
    drift = T.norm2(cplx(got8["w"] - ref8[1]))
    allowed = T.TRACK_GROWTH * T.BOUNDED_STEPS * step
    print(f"{name}: 8 steps ||w - ref||_2 / allowed {float((drift / allowed).max()):.4f}")
    assert np.all(drift <= allowed) and np.any(got8["w"] != got["w"])
    # out, J(out), J under w0 and the movement: the definition at the device's own weights
    own = equaliser_track_reference(x, L, 0, 0.0, seg, hop, h, planar=bool(planar), w=got8["w"])
    wd = cplx(got8["w"])
    dy = T.filter_bound_t(z, wd, seg, hop)
    eo = E.to_complex(got8["out"], bool(planar)) - E.to_complex(own[0], bool(planar))
    assert np.all(np.maximum(np.abs(eo.real), np.abs(eo.imag)) <= dy)
    assert np.all(np.abs(got8["est"][:, 1] - own[2][:, 1]) <= T.j_bound(E.to_complex(own[0], bool(planar)), dy, 1.0))
    assert np.all(np.abs(got8["est"][:, 0] - ref8[2][:, 0]) <= E.one_step_bound(z, w0c, mu, 1.0)[1])
    moved = (np.abs(wd - w0c[:, None]) ** 2).sum(axis=2).max(axis=1)
    assert np.all(np.abs(got8["est"][:, 2] - moved) <= E.gamma(2 * L + 2) * moved + 1e-12) and np.all(got8["est"][:, 3] == S)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. adjoint
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,length,seg,hop,planar", [(11, 300, 128, 64, 0), (32, 1025, 512, 128, 1), (2, 5, 2, 1, 0), (3, 9, 9, 4, 1), (5, 200, 65, 16, 0)])
def test_adjoint_identity_is_exact_on_integers(L, length, seg, hop, planar):
    B, S = 3, T.n_segments(length, seg, hop)
    x = E.integer_frames(B, length, L, planar=bool(planar))
    dout = E.integer_frames(B, length, L + 1, planar=bool(planar))
    w = T.integer_segment_weights(B, S, L, 5)
    out = forward(x, L, seg, hop, planar=planar, w=w)["out"]
    dx = backward(dout, w, seg, hop, planar, mode=1)                                      # (the mode is not looked at)
    q = hop * hop                                                                         # out and dx are multiples of 1 / hop
    lhs = np.rint(out * hop).astype(np.int64) * dout.astype(np.int64)
    rhs = x.astype(np.int64) * np.rint(dx * hop).astype(np.int64)
    assert np.array_equal(out * hop, np.rint(out * hop)) and np.array_equal(dx * hop, np.rint(dx * hop)) and q > 0
    assert lhs.sum() == rhs.sum() and lhs.sum() != 0


@pytest.mark.parametrize("layout", ["frames", "planar"])
def test_gradients_reach_the_frame_with_the_weights_held_fixed(layout):
    from vit_vs_raw_iq_amd import Equaliser, TrackingEqualiser, equaliser_track_reference_bwd
    xs = in_layout(E.run_frames("qpsk"), layout == "planar")
    dh = np.random.default_rng(8).standard_normal(xs.shape).astype(np.float32)
    eq = TrackingEqualiser(300, layout=layout, track_iters=8)
    x = on_device(xs).requires_grad_()
    out, w, est = eq(x, return_w=True, return_est=True)
    assert not w.requires_grad and not est.requires_grad and w.shape == (12, 3, 11, 2)
    (dx,) = torch.autograd.grad(out, x, on_device(dh))
    wd = w.cpu().numpy()
    assert np.array_equal(dx.cpu().numpy().astype(np.float64), backward(dh, wd, eq.seg, eq.hop, eq.planar))
    ref = equaliser_track_reference_bwd(dh, wd, eq.seg, eq.hop, bool(eq.planar))
    err = E.to_complex(dx.cpu().numpy(), bool(eq.planar)) - E.to_complex(ref, bool(eq.planar))
    dy = T.filter_bound_t(E.to_complex(dh, bool(eq.planar)), cplx(wd), eq.seg, eq.hop, adjoint=True)
    assert np.all(np.maximum(np.abs(err.real), np.abs(err.imag)) <= dy)
    # the call is the parent's block descent, then the ABI call from its weights; given the weights the forward is the same
    w0 = Equaliser(300, layout=layout)(x.detach(), return_w=True)[1]
    same = forward(xs, 11, eq.seg, eq.hop, eq.track_iters, eq.track_mu, 1.0, eq.planar, w0=w0.cpu().numpy(), taper=eq.table)
    assert np.array_equal(same["w"], wd.astype(np.float64)) and np.array_equal(same["out"], out.detach().cpu().numpy().astype(np.float64))
    assert np.array_equal(same["est"], est.cpu().numpy().astype(np.float64))
    assert same_bits(eq(x.detach(), w0=w0), out.detach()) and same_bits(eq(x.detach(), w=w), out.detach())
    assert torch.equal(est[:, 0], Equaliser(300, layout=layout)(x.detach(), return_est=True)[1][:, 1])      # J under w0 is the block J(after)
    assert bool((est[:, 2] > 0).all()) and bool((est[:, 3] == 3).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 6. isolation
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_frames_outputs_depend_on_neither_the_batch_nor_its_position():
    from vit_vs_raw_iq_amd import TrackingEqualiser
    xs = E.run_frames("qpsk")
    eq = TrackingEqualiser(300, iters=8, track_iters=4)
    big = np.tile(xs, (2, 1, 1))[:8]
    x8 = on_device(big)
    r8 = eq(x8, return_w=True, return_est=True)
    r1 = eq(x8[7:8], return_w=True, return_est=True)
    r3 = eq(x8[5:8], return_w=True, return_est=True)
    again = eq(x8, return_w=True, return_est=True)
    for a, b, c, d in zip(r1, r3, r8, again):
        assert same_bits(a, b[2:3]) and same_bits(a, c[7:8]) and same_bits(c, d)
    # a NaN frame poisons only itself
    bad = x8.clone()
    bad[1, 17, 0] = float("nan")
    res = eq(bad, return_w=True, return_est=True)
    keep = [0, 2, 3, 4, 5, 6, 7]
    for a, c in zip(res, r8):
        assert same_bits(a[keep], c[keep])
    assert bool(torch.isnan(res[0][1]).all()) and bool(torch.isnan(res[1][1]).all()) and bool(torch.isnan(res[2][1, :3]).all())
    given = eq(bad, w=r8[1], return_est=True)                                             # GIVEN: only the outputs the sample reaches
    assert int(torch.isnan(given[0][1, :, 0]).sum()) == 11 and same_bits(given[0][keep], r8[0][keep])
    assert eq(x8[:0]).shape == (0, 300, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_leave_the_outputs_untouched():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import TrackingEqualiser
    lib = N.lib()
    sentinel = 1234.5
    B, length = 2, 8192
    eq = TrackingEqualiser(length, taps=32, seg=512, hop=32, track_iters=2)
    S = eq.segments
    assert S == 241
    x = torch.zeros(B, length, 2, device=dev())
    big = torch.zeros(8193 * 2 + 4, device=dev())
    out, w_out, est = (torch.full(s, sentinel, device=dev()) for s in ((B, length, 2), (B, 256, 32, 2), (B, 4)))
    w = torch.zeros(B, 256, 32, 2, device=dev())
    taper = eq.table_on(dev())
    ARG, UNSUPPORTED = 1, 2
    ptrs = dict(x=x.data_ptr(), out=out.data_ptr(), w_out=w_out.data_ptr(), est=est.data_ptr())

    def fwd(length=length, par="ok", n=B, **kw):
        p = dict(ptrs)
        fields = {k: kw.pop(k) for k in list(kw) if k not in p}
        p.update(kw)
        if par == "ok":
            par = eq.track_struct(w.data_ptr(), w.data_ptr(), taper.data_ptr(), mode=1)
            for k, v in fields.items():
                setattr(par, k, v)
        return lib.iq_frames_equalise_track(p["x"], p["out"], p["w_out"], p["est"], n, length, ctypes.byref(par) if par is not None else None,
                                            N.stream_handle())

    def bwd(length=length, par="ok", n=B, **kw):
        p = dict(dout=x.data_ptr(), dx=out.data_ptr())
        fields = {k: kw.pop(k) for k in list(kw) if k not in p}
        p.update(kw)
        if par == "ok":
            par = eq.track_struct(w.data_ptr(), w.data_ptr(), taper.data_ptr(), mode=0)
            for k, v in fields.items():
                setattr(par, k, v)
        return lib.iq_frames_equalise_track_bwd(p["dout"], p["dx"], n, length, ctypes.byref(par) if par is not None else None, N.stream_handle())
    assert fwd(x=None) == ARG and fwd(out=None) == ARG and fwd(par=None) == ARG
    assert bwd(dout=None) == ARG and bwd(dx=None) == ARG and bwd(par=None) == ARG
    for call in (fwd, bwd):
        assert call(taps=0) == ARG and call(length=0) == ARG and call(length=-1) == ARG and call(iters=-1) == ARG
        assert call(seg=0) == ARG and call(hop=0) == ARG and call(hop=513) == ARG and call(length=511) == ARG
        for bad in (float("inf"), float("nan")):
            assert call(mu=bad) == ARG and call(modulus=bad) == ARG
        assert call(mu=-0.25) == ARG and call(planar=2) == ARG and call(planar=-1) == ARG and call(mode=2) == ARG and call(mode=-1) == ARG
        assert call(w=w.data_ptr() + 2) == ARG and call(w0=w.data_ptr() + 2) == ARG and call(taper=taper.data_ptr() + 2) == ARG
        # every edge of what is supported: one past it is refused
        assert call(taps=33) == UNSUPPORTED and call(iters=4097) == UNSUPPORTED and call(seg=513, hop=512) == UNSUPPORTED
        assert call(hop=30) == UNSUPPORTED and call(seg=1, hop=1, length=257) == UNSUPPORTED                # 257 segments
    assert fwd(x=big.data_ptr(), length=8193) == UNSUPPORTED and bwd(dout=big.data_ptr(), length=8193) == UNSUPPORTED
    assert fwd(x=x.data_ptr() + 4) == ARG and fwd(out=out.data_ptr() + 4) == ARG and bwd(dout=x.data_ptr() + 4) == ARG and bwd(dx=out.data_ptr() + 4) == ARG
    assert fwd(x=x.data_ptr() + 2, planar=1) == ARG and fwd(out=out.data_ptr() + 2, planar=1) == ARG
    assert fwd(w_out=w_out.data_ptr() + 2) == ARG and fwd(est=est.data_ptr() + 2) == ARG
    assert fwd(mode=0, w=None) == ARG and bwd(w=None) == ARG and bwd(w=None, mode=1) == ARG
    assert fwd(taper=None) == ARG and fwd(w_out=None) == ARG
    torch.cuda.synchronize()
    for t in (out, w_out, est):
        assert torch.equal(t, torch.full_like(t, sentinel))
    assert fwd(n=0) == 0 and fwd(n=-2) == 0 and bwd(n=0) == 0 and fwd(n=0, w=None, w0=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, sentinel))
    # the edges themselves run: 32 taps, 8192 samples, 512-symbol segments; est and w0 may be NULL; GIVEN needs neither taper nor w_out
    assert fwd(est=None, w0=None) == 0 and bwd() == 0 and fwd(mode=0, taper=None, w_out=None, w0=None) == 0
    assert fwd(hop=30, length=512 + 255 * 30) == 0                                         # 256 segments
    torch.cuda.synchronize()
    assert not out.any()                                                                   # (zero frames: zero outputs)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. plumbing
# ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    """A capture fails on any host synchronisation: the block descent, the two tracking launches and the adjoint are captured whole."""
    from vit_vs_raw_iq_amd import Carrier, Constellation, Synchronised, TrackingEqualiser
    eq = TrackingEqualiser(300, layout="planar", track_iters=8)
    sy = Synchronised(Constellation(32, 64, 300), Carrier(300, order=4), equaliser=eq)
    x0 = on_device(in_layout(E.run_frames("8psk"), 1))
    g = on_device(np.random.default_rng(2).standard_normal((12, 1, 32, 64)))

    def run():
        x = x0.clone().requires_grad_()
        img = sy(x)
        (dx,) = torch.autograd.grad(img, x, g)
        out, w, est = eq(x0, return_w=True, return_est=True)
        return img.detach(), dx, out, w, est
    eager = run()                                         # also: the tables are on the device before the capture
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
    assert float(eager[1].abs().max()) > 0


def _moving(doppler=3e-4, seed=11):
    from vit_vs_raw_iq_amd import FadedSynth, Fading, Receiver, ShapedSynth
    ws = ShapedSynth(["QPSK"], snrs_db=(20.0,), length=1024, seed=seed, sps=2, device=dev())
    fd = Fading(1024 + 64, 1024, taps=3, rice_k_db=6.0, decay=0.5, sinusoids=16, doppler=doppler)
    return FadedSynth(ws, fd), Receiver.for_synth(ws, timing="energy")


def test_received_faded_synth_with_the_tracking_equaliser_goes_into_the_stream():
    from vit_vs_raw_iq_amd import Carrier, Equaliser, ReceivedSynth, SynthStream, TrackingEqualiser
    fs, rx = _moving()
    eq, cr = TrackingEqualiser(512), Carrier(512, order=4, layout="interleaved")
    rs = ReceivedSynth(fs, rx, equaliser=eq, carrier=cr)
    B, s = 8, 2
    raw, y, z = fs.generate(B, s * B, 0)
    want = cr(eq(rx(raw)))
    got = rs.generate(B, s * B, 0)
    assert len(got) == 3 and same_bits(got[0], want) and torch.equal(got[1], y) and bool(torch.isfinite(want).all())
    assert not same_bits(want, cr(Equaliser(512)(rx(raw))))                # (the block equaliser alone gives other symbols)
    x, ys, zs = SynthStream(rs, IDENT, "rawiq", B).get(s)
    assert x.shape == (B, 2, 512) and same_bits(x, want.transpose(1, 2).contiguous()) and torch.equal(ys, y) and same_bits(zs, z)


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the closed loop behind the moving channel
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_loop_closes_on_the_device_behind_the_moving_channel():
    """FadedSynth (QPSK, sps 2, 20 dB; 3 taps, Rice 6 dB, 16 sinusoids, 3e-4 cycles per sample) -> Receiver -> TrackingEqualiser at
    the defaults, 16 frames of the device's own.  From the device's own block solution the segments' weights are those of the
    definition's own 32 steps within G * 32 one-step bounds, G the growth factor of these very frames measured in fp64 (a property
    of the definition's iteration, not of the device; at least 1); J(out) is the definition's within what that ball of weights can
    move it plus the bound of evaluating it once; and the median J(out) is below the median J under the block solution alone."""
    from vit_vs_raw_iq_amd import Equaliser, TrackingEqualiser, equaliser_track_reference
    fs, rx = _moving()
    sym = rx(fs.generate(16, 0, 0)[0])
    assert sym.shape == (16, 512, 2)
    eq = TrackingEqualiser(512)
    out, w, est = eq(sym, return_w=True, return_est=True)
    w0 = Equaliser(512)(sym, return_w=True)[1].cpu().numpy()
    xs, e, wd = sym.cpu().numpy(), est.cpu().numpy().astype(np.float64), cplx(w.cpu().numpy())
    z, w0c = E.to_complex(xs), cplx(w0)
    mu = float(np.float32(eq.track_mu))
    out_ref, w_ref, est_ref = equaliser_track_reference(xs, eq.taps, eq.track_iters, mu, eq.seg, eq.hop, eq.table, w0=w0)
    G, step = T.growth(z, w0c, mu, 1.0, eq.track_iters, eq.seg, eq.hop, eq.table)
    allowed = np.maximum(G, 1.0) * eq.track_iters * step
    drift = T.norm2(wd - cplx(w_ref))
    dJ = T.j_drift_bound_t(z, cplx(w_ref), allowed.max(axis=1), 1.0, eq.seg, eq.hop)
    dJ1 = T.j_bound(E.to_complex(out_ref), T.filter_bound_t(z, wd, eq.seg, eq.hop), 1.0)
    eJ = np.abs(e[:, 1] - est_ref[:, 1])
    print(f"median J {np.median(e[:, 0]):.4f} under the block solution -> {np.median(e[:, 1]):.4f} tracked (definition {np.median(est_ref[:, 1]):.4f}); "
          f"growth {G.max():.2f}; ||w - w_ref||_2 / allowed {float((drift / allowed).max()):.3f}; |J - ref| / allowed {float((eJ / (dJ + dJ1)).max()):.3f}")
    assert np.all(drift <= allowed) and np.all(eJ <= dJ + dJ1)
    assert np.all(np.abs(e[:, 0] - est_ref[:, 0]) <= E.one_step_bound(z, w0c, mu, 1.0)[1])
    assert np.all(allowed < 0.01 * T.norm2(cplx(w_ref)))                                   # (the allowance still means something)
    assert np.median(e[:, 1]) < np.median(e[:, 0]) and np.all(e[:, 3] == 7)
