"""GPU (MI355X): carrier recovery on the device (csrc/carrier.hip, iq_frames_carrier / _bwd, vit_vs_raw_iq_amd.carrier).

Every call through the C ABI here (`forward`, `backward`) carves its operands out of NaN-filled buffers and its outputs out of
sentinel-filled ones and checks the guards afterwards.

1. Exact: integer tables (entries in {-1, 0, 1}) and integer frames, M in {1, 2}, refine 0 -- power, the peak bin and F equal the
   fp64 definition bit for bit at every geometry and frame-length edge; every partial sum is an fp32 integer (asserted).
2. GIVEN mode at quarter turns: out = z (-j)^q bit for bit, and the backward is the forward with the negated pair.
3. Peak logic on constructed powers (permutation tables: P is |z|^2 in a known order).
4. Real tables, M in {1, 2, 4, 8}, against fp64 under the bounds derived in tests/carrier_ref.py; no frame is left out.
5. Closed loop: FrameSynth -> impair (frequency offset and phase) -> Carrier: the M-th-power line of the output sits at bin 0.
6. Adjoint identity, batch invariance, refusals, Synchronised (against the definition, through SynthStream, captured, x.grad).
"""
import ctypes

import numpy as np
import pytest
import torch

import carrier_ref as R
import constellation_ref as CR
from frontend_gpu import ISENT, abi_call, dev, on_device, same_bits

pytestmark = pytest.mark.gpu

IDENT = dict(i_mean=0.0, i_std=1.0, q_mean=0.0, q_std=1.0)


def wrap32(v):
    return ((np.asarray(v).astype(np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def forward(x, order, n1, n2, k_max=None, refine=0, planar=1, tables=None, fth=None, power=True, expect_kernel=True):
    """One guarded iq_frames_carrier call -> dict(out, est, fth, power) as numpy (float64 / int64)."""
    import vit_vs_raw_iq_amd._native as N
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, length, Nd = x.shape[0], x.shape[2] if planar else x.shape[1], n1 * n2
    given = fth is not None

    def par(t1, t2, tw, f):
        return N.Carrier(order=order, n1=n1, n2=n2, k_max=Nd // 2 if k_max is None else k_max, refine=refine, planar=planar,
                         mode=0 if given else 1, t1=t1, t2=t2, tw=tw, fth=f)
    out, est, fth_out, p = abi_call("iq_frames_carrier", "frames_carrier_kernel", (x,),
                                    [x.shape, (B, 4), (np.int32, B, 2), (B, Nd) if power and not given else None], B, length, par,
                                    expect_kernel, side=(*(tables or (None,) * 3), np.asarray(fth, np.int32) if given else None))
    return dict(out=out.astype(np.float64), est=est.astype(np.float64), fth=fth_out.astype(np.int64),
                power=None if p is None else p.astype(np.float64))


def backward(dout, fth, planar=1, order=4, n1=32, n2=32):
    """One guarded iq_frames_carrier_bwd call -> dx float64."""
    import vit_vs_raw_iq_amd._native as N
    dout = np.ascontiguousarray(dout, dtype=np.float32)
    B, length = dout.shape[0], dout.shape[2] if planar else dout.shape[1]

    def par(f):
        return N.Carrier(order=order, n1=n1, n2=n2, k_max=0, refine=0, planar=planar, mode=0, t1=None, t2=None, tw=None, fth=f)
    return abi_call("iq_frames_carrier_bwd", "frames_carrier_bwd_kernel", (dout,), dout.shape, B, length, par,
                    side=(np.asarray(fth, np.int32),)).astype(np.float64)


def in_layout(x, planar):
    return x if planar else np.ascontiguousarray(np.transpose(x, (0, 2, 1)))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. exact
# ---------------------------------------------------------------------------------------------------------------------------
# (n1, n2, len, B, M, planar): 32 x 32 at len 1, 2, 31, 33, 1000, 1024 (one sample, one pair, around the tile edge, a partly
# and a wholly filled transform), both layouts, odd lengths; 64 x 32 and 32 x 64 (a transposed index shows where n1 != n2);
# 256 x 32 with a full 8192-sample frame, two frames
EXACT = [(32, 32, 1, 3, 1, 1), (32, 32, 2, 3, 2, 0), (32, 32, 31, 3, 2, 1), (32, 32, 33, 3, 1, 0), (32, 32, 1000, 3, 2, 1),
         (32, 32, 1024, 3, 1, 0), (32, 32, 1023, 2, 2, 0), (64, 32, 2047, 2, 2, 1), (32, 64, 2000, 2, 1, 0), (32, 64, 1999, 2, 2, 1),
         (256, 32, 8192, 2, 2, 1)]


@pytest.mark.parametrize("n1,n2,length,B,M,planar", EXACT)
def test_integer_tables_and_frames_are_exact(n1, n2, length, B, M, planar):
    from vit_vs_raw_iq_amd import carrier_reference
    tables = R.integer_tables(n1, n2, 7 * n1 + n2 + length)
    xp = R.integer_frames(B, length, length + M)
    assert R.exact_partial_sum_bound(xp, tables, M) < 2 ** 12
    x = in_layout(xp, planar)
    Nd = n1 * n2
    for k_max in (Nd // 2, 37):
        _, est_ref, fth_ref, p_ref = carrier_reference(x, tables, M, k_max=k_max, refine=False, planar=bool(planar))
        got = forward(x, M, n1, n2, k_max, 0, planar, tables)
        assert np.array_equal(got["power"], p_ref)
        assert np.array_equal(got["est"][:, 2], est_ref[:, 2])                       # the peak bin: refine 0, d = 0
        assert np.array_equal(got["fth"][:, 0], fth_ref[:, 0])
        assert np.array_equal(got["est"][:, 0], (fth_ref[:, 0] * 2.0 ** -32).astype(np.float32).astype(np.float64))
        z = R.to_complex(x, bool(planar))
        tol = R.th_tolerance(z, M, fth_ref[:, 0], np.zeros(B))
        assert np.all(R.circular(got["fth"][:, 1], fth_ref[:, 1], 2.0 ** 32 / M) <= tol)
        out_ref = carrier_reference(x, None, M, planar=bool(planar), fth=got["fth"])[0]
        assert np.all(np.abs(got["out"] - out_ref) <= R.out_bound(x))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. GIVEN mode
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar,length", [(1, 777), (0, 1024), (0, 1), (1, 8192)])
def test_given_quarter_turns_are_exact_and_the_backward_is_the_forward_negated(planar, length):
    from vit_vs_raw_iq_amd import carrier_reference, carrier_reference_bwd
    rng = np.random.default_rng(length)
    B = 6
    x = in_layout(rng.standard_normal((B, 2, length)).astype(np.float32), planar)
    q = np.array([[0, 0], [1, 0], [0, 1], [2, 3], [3, 2], [1, 1]])
    fth = wrap32(q * 2 ** 30)
    n1 = 256 if length > 1024 else 32                      # N >= len, whatever the mode
    got = forward(x, 4, n1, 32, planar=planar, fth=fth)
    z = R.to_complex(x, bool(planar))
    turns = (q[:, :1] * np.arange(length)[None, :] + q[:, 1:]) % 4
    want = z * (-1j) ** turns
    o = R.to_complex(got["out"], bool(planar))
    assert np.array_equal(o.real, want.real) and np.array_equal(o.imag, want.imag)      # (as values: a zero's sign is not compared)
    assert np.array_equal(got["fth"], fth)
    assert np.array_equal(got["est"][:, :2], np.stack([fth[:, 0] / 2.0 ** 32, fth[:, 1] / 2.0 ** 32 * 2 * np.pi], axis=1).astype(np.float32))
    assert np.all(np.isnan(got["est"][:, 2:]))
    dx = backward(x, fth, planar, n1=n1)
    neg = forward(x, 4, n1, 32, planar=planar, fth=wrap32(-fth))["out"]
    assert np.array_equal(dx, neg)
    # any phase: within the rotation's bound of the definition, forward and backward
    fth = rng.integers(-2 ** 31, 2 ** 31, (B, 2))
    assert np.all(np.abs(forward(x, 4, n1, 32, planar=planar, fth=fth)["out"] - carrier_reference(x, None, 4, planar=bool(planar), fth=fth)[0]) <= R.out_bound(x))
    assert np.all(np.abs(backward(x, fth, planar, n1=n1) - carrier_reference_bwd(x, fth, bool(planar))) <= R.out_bound(x))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. peak logic
# ---------------------------------------------------------------------------------------------------------------------------
# name -> ({signed bin: power}, k_max, peak bin, d or None where only the definition says)
PEAKS = {
    "at_zero_neighbour_wraps": ({0: 16, -1: 4, 1: 9}, 512, 0, None),
    "at_minus_k_max_outer_neighbour_counts": ({-5: 16, -6: 9, -4: 1, 100: 400}, 5, -5, None),
    "at_plus_k_max_outer_neighbour_counts": ({5: 16, 6: 9, 4: 1, -100: 400}, 5, 5, None),
    "at_minus_half": ({-512: 16, 511: 4, -511: 1}, 512, -512, None),
    "half_a_bin_up": ({7: 9, 6: 1, 8: 9}, 512, 7, 0.5),
    "tie_takes_the_lowest": ({3: 9, -7: 9, 100: 9}, 512, -7, 0.0),
    "k_max_0": ({0: 1, 5: 100}, 0, 0, None),
    "k_max_1_tie": ({1: 4, -1: 4, 0: 1, 2: 100}, 1, -1, None),
    "flat_top_no_parabola": ({10: 4, 9: 4, 11: 4}, 512, 9, None),
}


@pytest.mark.parametrize("name", list(PEAKS))
def test_peak_logic_on_constructed_powers(name):
    from vit_vs_raw_iq_amd import carrier_reference
    spec, k_max, s_hat, d = PEAKS[name]
    n1 = n2 = 32
    Nd = n1 * n2
    tables = R.permutation_tables(n1, n2)
    P = np.zeros(Nd)
    for s, v in spec.items():
        P[s % Nd] = v
    x = R.frame_with_power(P, n1, n2)
    _, est_ref, fth_ref, p_ref = carrier_reference(x, tables, 1, k_max=k_max, refine=True)
    assert np.array_equal(p_ref[0], P) and np.floor(est_ref[0, 2] + 0.5) in (s_hat, s_hat + 1)
    got = forward(x, 1, n1, n2, k_max, 1, 1, tables)
    assert np.array_equal(got["power"][0], P)
    assert abs(got["est"][0, 2] - est_ref[0, 2]) <= 2.0 ** -23 * max(1.0, abs(s_hat))
    if d is not None:
        assert got["est"][0, 2] == s_hat + d
    assert abs(got["fth"][0, 0] - fth_ref[0, 0]) <= 1                      # d: one fp32 division against one fp64 division
    flat = forward(x, 1, n1, n2, k_max, 0, 1, tables)
    assert flat["est"][0, 2] == s_hat and flat["fth"][0, 0] == int(wrap32(int(np.rint(s_hat / Nd * 2.0 ** 32))))


@pytest.mark.parametrize("planar", [1, 0])
def test_frames_without_a_line_give_zero_estimates(planar):
    """All zeros; a power of zero at the only bin searched; a non-finite sample.  F = TH = 0, est[1] = est[3] = 0, out = x."""
    n1 = n2 = 32
    tables = R.permutation_tables(n1, n2)
    P = np.zeros(n1 * n2)
    P[5] = 100
    xp = np.concatenate([np.zeros((1, 2, 1024), np.float32), R.frame_with_power(P, n1, n2), np.zeros((1, 2, 1024), np.float32)])
    xp[2, 0, 0] = np.inf
    x = in_layout(xp, planar)
    got = forward(x, 1, n1, n2, 0, 1, planar, tables)
    assert np.array_equal(got["fth"], np.zeros((3, 2))) and np.array_equal(got["est"], np.zeros((3, 4)))
    assert np.array_equal(got["out"][:2], x[:2].astype(np.float64))
    wide = forward(x[:1], 1, n1, n2, 512, 1, planar, tables)
    assert np.array_equal(wide["est"], [[0, 0, -512, 0]]) and np.array_equal(wide["fth"], [[0, 0]])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. real tables
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.REAL))
def test_real_tables_stay_within_the_derived_bounds(name):
    from vit_vs_raw_iq_amd import carrier_reference, dft_tables
    M, B, length, (n1, n2), _ = R.REAL[name]
    Nd = n1 * n2
    x = R.real_case(name)
    z = R.to_complex(x)
    tables = dft_tables(n1, n2)
    _, est0, fth0, p_ref = carrier_reference(x, tables, M, refine=False)
    _, est1, fth1, _ = carrier_reference(x, tables, M, refine=True)
    s_ref = est0[:, 2]
    lead = R.peak_lead(p_ref, s_ref)
    assert np.all(lead >= 2), lead                                          # every frame takes part
    dP = R.power_bound(p_ref, R.dw_bound(z, M, n1, n2))
    flat = forward(x, M, n1, n2, None, 0, 1, tables)
    fine = forward(x, M, n1, n2, None, 1, 1, tables)
    err = np.abs(flat["power"] - p_ref)
    print(f"{name}: |P - ref| / bound {float((err / dP).max()):.4f}, bound / peak {float((dP.max(axis=1) / p_ref.max(axis=1)).max()):.2e}, "
          f"lead {lead.min():.2f}")
    assert np.all(err <= dP)
    assert np.array_equal(fine["power"], flat["power"])
    # the peak bin and the unrefined F: exactly the definition's
    assert np.array_equal(flat["est"][:, 2], s_ref) and np.array_equal(flat["fth"][:, 0], fth0[:, 0])
    # the refined F and TH
    f_tol = R.f_tolerance(p_ref, dP, s_ref, M)
    df = np.abs(wrap32(fine["fth"][:, 0] - fth1[:, 0]))
    th_tol = R.th_tolerance(z, M, fth1[:, 0], f_tol)
    dth = R.circular(fine["fth"][:, 1], fth1[:, 1], 2.0 ** 32 / M)
    print(f"{name}: |F - ref| {df.max():.0f} of {f_tol.min():.0f} .. {f_tol.max():.0f} counts, |TH - ref| {dth.max():.0f} of "
          f"{th_tol.min():.0f} .. {th_tol.max():.0f} counts, quality {fine['est'][:, 3].min():.3f} .. {fine['est'][:, 3].max():.3f}")
    assert np.all(df <= f_tol) and np.all(dth <= th_tol)
    assert np.all(np.abs(fine["est"][:, 2] - est1[:, 2]) <= (f_tol * Nd * M / 2.0 ** 32) + 2.0 ** -23 * np.abs(s_ref).max())
    # out at the device's own estimate
    for got in (flat, fine):
        out_ref = carrier_reference(x, None, M, fth=got["fth"])[0]
        assert np.all(np.abs(got["out"] - out_ref) <= R.out_bound(x))
        assert np.array_equal(got["est"][:, 0], (got["fth"][:, 0] * 2.0 ** -32).astype(np.float32).astype(np.float64))
        assert np.array_equal(got["est"][:, 1], (got["fth"][:, 1] * 2.0 ** -32 * 2 * np.pi).astype(np.float32).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. closed loop
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,M", [("BPSK", 2), ("QPSK", 4), ("16QAM", 4)])
def test_the_loop_closes_on_the_device(cls, M):
    """FrameSynth at 20 dB -> impair (cfo within +-0.02 cycle per sample, any phase) -> Carrier.  The M-th-power line of the
    output sits at bin 0 of the padded periodogram with angle 0, and the frequency found is the carrier's (modulo 1 / M).  The
    lock quality follows the definition's within a tenth of the definition's own standard deviation over these frames (what tells
    one frame of the class from another)."""
    from vit_vs_raw_iq_amd import Carrier, FrameSynth, Impairments, carrier_reference, impair
    length, B = 512, 24
    fs = FrameSynth([cls], snrs_db=(20.0,), length=length, seed=17, device=dev())
    raw = fs.generate(B, 0, 0)[0]
    x, drawn = impair(raw, IDENT, "rawiq", Impairments(phase=(0.0, 6.28), cfo=(-0.02, 0.02)), seed=3, return_drawn=True)
    cr = Carrier(length, order=M)
    out, est, fth, power = cr(x, return_est=True, return_fth=True, return_power=True)
    assert out.shape == x.shape and est.shape == (B, 4) and fth.shape == (B, 2) and fth.dtype == torch.int32 and power.shape == (B, cr.n_dft)
    o = R.to_complex(out.cpu().numpy()) ** M
    spec = np.abs(np.fft.fft(o, cr.n_dft, axis=1))
    assert np.all(spec.argmax(axis=1) == 0)
    assert np.all(np.abs(np.angle(o.sum(axis=1))) <= 1e-3)
    e = est.cpu().numpy().astype(np.float64)
    cfo = drawn[:, 1].cpu().numpy().astype(np.float64)
    assert np.all(R.circular(e[:, 0], cfo, 1.0 / M) <= 0.25 / (M * length))              # a quarter cycle of w over the frame
    _, est_ref, _, _ = carrier_reference(x.cpu().numpy(), (cr.t1, cr.t2, cr.tw), M)
    margin = 0.1 * est_ref[:, 3].std()
    dq = np.abs(e[:, 3] - est_ref[:, 3]).max()
    print(f"{cls}: quality {est_ref[:, 3].min():.3f} .. {est_ref[:, 3].max():.3f}, std {est_ref[:, 3].std():.2e}, |device - definition| "
          f"{dq:.2e} of {margin:.2e}; |f - cfo| mod 1/M {R.circular(e[:, 0], cfo, 1.0 / M).max():.2e}")
    assert dq <= margin
    assert np.all((e[:, 3] > 0) & (e[:, 3] <= 1 + 1e-6))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. adjoint, invariance, refusals, Synchronised
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_adjoint_identity_at_a_fixed_estimate(layout):
    from vit_vs_raw_iq_amd import Carrier
    rng = np.random.default_rng(8)
    B, length = 5, 999
    shape = (B, 2, length) if layout == "planar" else (B, length, 2)
    xh, dh = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    cr = Carrier(length, order=4, layout=layout)
    x = on_device(xh).requires_grad_()
    out, fth = cr(x, return_fth=True)                      # the estimate of the forward is the backward's
    (dx,) = torch.autograd.grad(out, x, on_device(dh))
    lhs = float((out.detach().cpu().numpy().astype(np.float64) * dh).sum())
    rhs = float((xh.astype(np.float64) * dx.cpu().numpy().astype(np.float64)).sum())
    tol = float((np.abs(dh) * R.out_bound(xh)).sum() + (np.abs(xh) * R.out_bound(dh)).sum())
    print(f"{layout}: <out, dout> - <x, dx> = {lhs - rhs:.3e} of {tol:.3e}")
    assert abs(lhs - rhs) <= tol
    assert np.array_equal(dx.cpu().numpy().astype(np.float64), backward(dh, fth.cpu().numpy(), cr.planar))
    given = cr(x.detach(), fth=fth)
    assert same_bits(given, out.detach())
    # two runs agree bit for bit
    out2, fth2 = cr(x.detach(), return_fth=True)
    assert same_bits(out2, out.detach()) and torch.equal(fth2, fth)


def test_a_frames_outputs_do_not_depend_on_the_batch():
    from vit_vs_raw_iq_amd import Carrier
    x = on_device(R.real_case("qpsk_m4"))
    cr = Carrier(1000, order=4, n_dft=(64, 32))
    one = cr(x[2:3], return_est=True, return_fth=True, return_power=True)
    five = cr(x[:5], return_est=True, return_fth=True, return_power=True)
    for a, b in zip(one, five):
        assert torch.equal(a, b[2:3])
    # a NaN frame poisons only itself
    bad = x[:5].clone()
    bad[1, 0, 7] = float("nan")
    again = cr(bad, return_est=True, return_fth=True, return_power=True)
    for a, b in zip(again, five):
        keep = [0, 2, 3, 4]
        assert torch.equal(a[keep], b[keep])
    assert torch.equal(again[2][1], torch.zeros(2, dtype=torch.int32, device=dev()))
    assert cr(x[:0]).shape == (0, 2, 1000)


def test_refusals_return_their_code_and_leave_the_outputs_untouched():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import Carrier
    L = N.lib()
    sentinel = 1234.5
    B, length = 3, 1000
    cr = Carrier(length, order=4, n_dft=(32, 32))
    t1, t2, tw = cr.tables_on(dev())
    x = torch.zeros(B, 2, length, device=dev())
    out, est, power = (torch.full(s, sentinel, device=dev()) for s in ((B, 2, length), (B, 4), (B, 1024)))
    fout = torch.full((B, 2), ISENT, dtype=torch.int32, device=dev())
    fth = torch.zeros(B, 2, dtype=torch.int32, device=dev())
    ARG, UNSUPPORTED = 1, 2
    ptrs = dict(x=x.data_ptr(), out=out.data_ptr(), est=est.data_ptr(), fth_out=fout.data_ptr(), power=power.data_ptr())

    def fwd(length=length, par="ok", n=B, **kw):
        p = dict(ptrs)
        fields = {k: kw.pop(k) for k in list(kw) if k not in p}
        p.update(kw)
        if par == "ok":
            par = cr.struct((t1.data_ptr(), t2.data_ptr(), tw.data_ptr()), fth.data_ptr(), mode=1)
            for k, v in fields.items():
                setattr(par, k, v)
        return L.iq_frames_carrier(p["x"], p["out"], p["est"], p["fth_out"], p["power"], n, length,
                                   ctypes.byref(par) if par is not None else None, N.stream_handle())

    def bwd(length=length, par="ok", n=B, **kw):
        p = dict(dout=x.data_ptr(), dx=out.data_ptr())
        fields = {k: kw.pop(k) for k in list(kw) if k not in p}
        p.update(kw)
        if par == "ok":
            par = cr.struct((t1.data_ptr(), t2.data_ptr(), tw.data_ptr()), fth.data_ptr(), mode=0)
            for k, v in fields.items():
                setattr(par, k, v)
        return L.iq_frames_carrier_bwd(p["dout"], p["dx"], n, length, ctypes.byref(par) if par is not None else None, N.stream_handle())
    assert fwd(x=None) == ARG and fwd(out=None) == ARG and fwd(par=None) == ARG
    assert bwd(dout=None) == ARG and bwd(dx=None) == ARG and bwd(par=None) == ARG
    for call in (fwd, bwd):
        for order in (0, 3, 5, 16, -2):
            assert call(order=order) == ARG
        assert call(refine=2) == ARG and call(planar=2) == ARG and call(planar=-1) == ARG and call(mode=2) == ARG and call(mode=-1) == ARG
        assert call(k_max=-1) == ARG and call(k_max=513) == ARG and call(length=0) == ARG and call(length=-1) == ARG
        assert call(t1=t1.data_ptr() + 2) == ARG and call(t2=t2.data_ptr() + 1) == ARG and call(tw=tw.data_ptr() + 2) == ARG
        assert call(fth=fth.data_ptr() + 2) == ARG
        for n1, n2 in ((0, 32), (16, 64), (48, 32), (32, 288), (31, 33)):
            assert call(n1=n1, n2=n2, k_max=0) == UNSUPPORTED
        assert call(length=1025) == UNSUPPORTED and call(n1=256, n2=64) == UNSUPPORTED and call(n1=256, n2=32, length=8193) == UNSUPPORTED
    assert fwd(x=x.data_ptr() + 2) == ARG and fwd(out=out.data_ptr() + 2) == ARG and fwd(x=x.data_ptr() + 4, planar=0) == ARG
    assert fwd(out=out.data_ptr() + 4, planar=0) == ARG and bwd(dout=x.data_ptr() + 4, planar=0) == ARG and bwd(dx=out.data_ptr() + 2) == ARG
    assert fwd(est=est.data_ptr() + 2) == ARG and fwd(fth_out=fout.data_ptr() + 2) == ARG and fwd(power=power.data_ptr() + 2) == ARG
    assert fwd(t1=None) == ARG and fwd(t2=None) == ARG and fwd(tw=None) == ARG
    assert fwd(mode=0, fth=None, power=None) == ARG and fwd(mode=0) == ARG and bwd(fth=None) == ARG      # power with GIVEN
    torch.cuda.synchronize()
    for t in (out, est, power):
        assert torch.equal(t, torch.full_like(t, sentinel))
    assert torch.equal(fout, torch.full_like(fout, ISENT))
    assert fwd(n=0) == 0 and fwd(n=-2) == 0 and bwd(n=0) == 0 and fwd(n=0, mode=0, power=None, t1=None, t2=None, tw=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, sentinel)) and torch.equal(fout, torch.full_like(fout, ISENT))
    # the optional outputs may be NULL: the frames come out the same
    assert fwd(est=None, fth_out=None, power=None) == 0
    full = cr(x + 1.0, return_est=True)
    assert same_bits(cr(x + 1.0), full[0])


def synchronised(length=512, height=32, width=64, order=4, **kw):
    from vit_vs_raw_iq_amd import Carrier, Constellation, Synchronised
    con = Constellation(height, width, length, **kw)
    cr = Carrier(length, order=order)
    return Synchronised(con, cr), con, cr


def impaired_frames(length, B, classes=("BPSK", "QPSK", "16QAM")):
    from vit_vs_raw_iq_amd import FrameSynth, Impairments, impair
    fs = FrameSynth(list(classes), snrs_db=(20.0,), length=length, seed=5, device=dev())
    return impair(fs.generate(B, 0, 0)[0], IDENT, "rawiq", Impairments(phase=(0.0, 6.28), cfo=(-0.02, 0.02)), seed=9)


def test_synchronised_constellation_against_the_definitions():
    """Constellation(the definition's derotation at the device's own estimate) in fp64; the bound is the constellation suite's:
    FACTOR = 3 times the error of the same definition evaluated in numpy float32 (tests/test_gpu_constellation.py)."""
    from vit_vs_raw_iq_amd import carrier_reference, constellation_reference
    FACTOR = 3
    sy, con, cr = synchronised(profile="gaussian", sigma=1.0, radius=4, n_frac=8, mode="log")
    x = impaired_frames(512, 6)
    img = sy(x)
    assert img.shape == sy.image_shape(6) == (6, 1, 32, 64)
    assert same_bits(img, con(cr(x)))
    fth = cr(x, return_fth=True)[1].cpu().numpy()
    xr = carrier_reference(x.cpu().numpy(), None, 4, fth=fth)[0]
    ref = constellation_reference(xr, con)
    e32 = np.abs(CR.real_forward(xr, con, np.float32).astype(np.float64) - ref).max()
    err = np.abs(img.cpu().numpy().astype(np.float64) - ref).max()
    print(f"synchronised constellation: E32 {e32:.3e}, kernel {err:.3e} ({err / e32:.3f} E32)")
    assert e32 > 0 and err <= FACTOR * e32
    # fit: the front end's scaling on the derotated frames
    sy.fit(x)
    fitted = sy(x)
    assert abs(float(fitted.mean())) < 1e-3 and abs(float(fitted.std()) - 1.0) < 1e-3


def test_synchronised_goes_where_a_front_end_goes_and_gradients_reach_the_frame():
    from vit_vs_raw_iq_amd import FrameSynth, Impairments, SynthStream, impair
    sy, con, cr = synchronised()
    fs = FrameSynth(["BPSK", "QPSK", "16QAM"], snrs_db=(20.0,), length=512, seed=5, device=dev())
    aug = Impairments(phase=(0.0, 6.28), cfo=(-0.02, 0.02))
    xs, y, z = SynthStream(fs, IDENT, "vit", 8, augment=aug, spectrogram=sy).get(3)
    x0, y0, z0 = SynthStream(fs, IDENT, "rawiq", 8, augment=aug).get(3)
    assert xs.shape == (8, 1, 32, 64) and same_bits(xs, con(cr(x0))) and torch.equal(y, y0) and same_bits(z, z0)
    raw = fs.generate(8, 24, 0)[0]
    got = impair(raw, IDENT, "vit", aug, seed=4, step=2, frame_base=7, spectrogram=sy)
    assert same_bits(got, sy(impair(raw, IDENT, "rawiq", aug, seed=4, step=2, frame_base=7)))
    # x.grad: through both adjoints, equal to the chain written out
    w = on_device(np.random.default_rng(1).standard_normal((8, 1, 32, 64)))
    x = x0.clone().requires_grad_()
    (dx,) = torch.autograd.grad(sy(x), x, w)
    xa = x0.clone().requires_grad_()
    mid, fth = cr(xa, return_fth=True)
    mid2 = mid.detach().requires_grad_()
    (dmid,) = torch.autograd.grad(con(mid2), mid2, w)
    assert float(dx.abs().max()) > 0 and np.array_equal(dx.cpu().numpy().astype(np.float64),
                                                         backward(dmid.cpu().numpy(), fth.cpu().numpy(), 1))


def test_graph_replay_equals_eager():
    """A capture fails on any host synchronisation: carrier -> constellation -> both adjoints are captured whole."""
    sy, con, cr = synchronised()
    x0 = impaired_frames(512, 12)
    w = on_device(np.random.default_rng(2).standard_normal((12, 1, 32, 64)))

    def run():
        x = x0.clone().requires_grad_()
        img = sy(x)
        (dx,) = torch.autograd.grad(img, x, w)
        out, est, fth = cr(x0, return_est=True, return_fth=True)
        return img.detach(), dx, out, est, fth
    eager = run()                                         # also: the tables are on the device before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        held = run()
    for t in held:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(held, eager):
        assert torch.equal(a, b)
