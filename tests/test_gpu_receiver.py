"""GPU (MI355X): the receiver on the device (csrc/receiver.hip, iq_frames_receive / _bwd, vit_vs_raw_iq_amd.receiver).

1. Bit-exact: GIVEN mode, no normalisation, tables and frames of small integers -- sym and energy equal the fp64 definition bit
   for bit at every frame-length, tap-count, instant and sps edge (zero extension at both ends, every MFMA tile edge).
2. Real tables against fp64 under the derived dot-product bound 2 (J + 3) 2^-24 sum |x_j| |G_j| (+ 4 2^-24 |s| normalised).
3. Timing: a constructed symbol-rate line, ShapedSynth frames against the definition, ENERGY mode and its ties.
4. Loop closure on the device: ShapedSynth -> Receiver -> the transmitted symbols, under the caps of the host test (tests/receiver_ref.py).
5. Backward: against the fp64 adjoint, run to run, and the exact dot-product identity in integers.
6. Isolation, refusals, SynthStream / hipGraph / train_on_stream plumbing.
"""
import ctypes

import numpy as np
import pytest
import torch

from frontend_gpu import dev, same_bits
from receiver_ref import EPS, EVM_CAP, T0_CAP, abs_windows, circular_distance, complex_frames, dot_bound, evm, true_instant

pytestmark = pytest.mark.gpu


def to_dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(dev())


def integer_case(seed, B, length, sps, span, n_frac, lo=-1, hi=1):
    rng = np.random.default_rng(seed)
    J = sps * span
    raw = rng.integers(lo, hi + 1, (B, length, 2)).astype(np.float32)
    table = rng.integers(lo, hi + 1, (n_frac, J + 1)).astype(np.float32)
    raw[:, 0] = raw[:, -1] = 1.0                      # the frame ends and the outer taps take part
    table[:, 0] = table[:, -1] = 1.0
    us = np.array([0, n_frac - 1, sps * n_frac - 1])[np.arange(B) % 3]
    return raw, table, us


# (B, len, sps, span): J + 1 = 2, 17 and 513 (and 16 at sps 3); len = sps, 16 k +- 1, 8192; one frame and more than 256 CUs
EXACT = [(3, 1, 1, 1), (3, 2, 2, 8), (3, 3, 3, 5), (3, 8, 8, 2), (3, 16, 16, 1), (3, 16, 16, 32),
         (3, 17, 1, 16), (3, 31, 2, 8), (3, 255, 3, 5), (3, 257, 8, 2), (3, 273, 16, 32), (1, 4095, 1, 1),
         (3, 8192, 16, 32), (3, 8192, 1, 1), (3, 8192, 8, 2), (1, 511, 1, 16), (300, 47, 3, 5)]


@pytest.mark.parametrize("B,length,sps,span", EXACT)
def test_integer_frames_and_tables_are_exact(B, length, sps, span):
    from vit_vs_raw_iq_amd import Receiver, receiver_reference
    n_frac = 4
    raw, table, us = integer_case(length * 31 + sps, B, length, sps, span, n_frac)
    sym_ref, est_ref, en_ref = receiver_reference(raw, table, sps, "given", us, normalise=False)
    assert en_ref.sum(axis=1).max() < 2 ** 24 and np.abs(sym_ref).max() < 2 ** 24          # every partial sum is an fp32 integer
    rx = Receiver(sps, span, n_frac=n_frac, timing="given", normalise=False, table=table)
    sym, est, energy = rx(to_dev(raw), u=us, return_est=True, return_energy=True)
    assert sym.shape == (B, length // sps, 2) and est.shape == (B, 4) and energy.shape == (B, sps)
    assert np.array_equal(sym.cpu().numpy().astype(np.float64), sym_ref)
    assert np.array_equal(energy.cpu().numpy().astype(np.float64), en_ref)
    e = est.cpu().numpy().astype(np.float64)
    assert np.all(np.isnan(e[:, 0])) and np.array_equal(e[:, 1], us) and np.all(np.abs(e[:, 3] - est_ref[:, 3]) <= EPS * est_ref[:, 3])
    # without est and energy the sample-rate pass is skipped: the symbols are the same
    assert same_bits(rx(to_dev(raw), u=us), sym)
    # u = None is 0
    assert np.array_equal(rx(to_dev(raw)).cpu().numpy().astype(np.float64), receiver_reference(raw, table, sps, "given", None, False)[0])


REAL = [(5, 1024, 8, 8, 32), (5, 384, 3, 6, 8), (2, 8192, 16, 32, 4), (5, 100, 2, 4, 64), (3, 8192, 1, 32, 2)]


@pytest.mark.parametrize("B,length,sps,span,n_frac", REAL)
def test_real_tables_stay_within_the_dot_product_bound(B, length, sps, span, n_frac):
    """|sym - ref| <= 2 (J + 3) 2^-24 sum_j |x_j| |G_j| per component (v; with normalisation divided by rho, plus 4 2^-24 |s|).
    Energies: |y|^2 carries 2 (|re| + |im|) d + 2 d^2 of its components' bound d, the sum of N terms (N + 2) 2^-24 of itself."""
    from vit_vs_raw_iq_amd import Receiver, mf_table, receiver_reference
    rng = np.random.default_rng(length + sps)
    raw = rng.standard_normal((B, length, 2)).astype(np.float32)
    table = mf_table(0.35, sps, span, n_frac)
    us = rng.integers(0, sps * n_frac, B)
    J = sps * span
    bound_v = dot_bound(J + 1, abs_windows(raw, table, sps, us))
    worst = {}
    for normalise in (False, True):
        ref, est_ref, en_ref = receiver_reference(raw, table, sps, "given", us, normalise)
        rx = Receiver(sps, span, n_frac=n_frac, timing="given", normalise=normalise, table=table)
        sym, est, energy = rx(to_dev(raw), u=us, return_est=True, return_energy=True)
        err = np.abs(sym.cpu().numpy().astype(np.float64) - ref)
        bound = bound_v
        if normalise:
            bound = bound_v / np.sqrt(est_ref[:, 3] + 1e-12)[:, None, None] + 4 * EPS * np.abs(ref)
        worst[normalise] = float((err / bound).max())
        assert np.all(err <= bound), worst
    y_abs = abs_windows(raw, table[:1], 1, np.zeros(B, np.int64))                      # every sample, row 0
    d = dot_bound(J + 1, y_abs)
    y = receiver_reference(raw, table[:1], 1, "given", None, False)[0]                 # y(n) itself
    per = 2 * (np.abs(y[:, :, 0]) + np.abs(y[:, :, 1])) * d.max(axis=2) + 2 * d.max(axis=2) ** 2
    en_bound = np.stack([per[:, r::sps].sum(axis=1) for r in range(sps)], axis=1) + (length / sps + 2) * EPS * en_ref
    en_err = np.abs(energy.cpu().numpy().astype(np.float64) - en_ref)
    print(f"len {length} sps {sps} span {span}: |sym - ref| / bound {worst[False]:.4f} (v), {worst[True]:.4f} (normalised); "
          f"|E - ref| / bound {float((en_err / en_bound).max()):.4f}")
    assert np.all(en_err <= en_bound)


def delta_table(sps, span, n_frac):
    t = np.zeros((n_frac, sps * span + 1), np.float32)
    t[:, sps * span // 2] = 1.0
    return t


@pytest.mark.parametrize("sps,length", [(8, 1024), (3, 384), (16, 8192)])
def test_oerder_meyr_finds_a_constructed_symbol_rate_line(sps, length):
    """y = x through a delta table, |x[n]|^2 = 1 + cos(2 pi (n - t0) / sps): E[r] = (len / sps) (1 + cos(2 pi (r - t0) / sps)),
    X = (len / 2) exp(-2 pi j t0 / sps)."""
    from vit_vs_raw_iq_amd import Receiver
    t0 = np.array([0.0, 1.0, sps / 2.0, sps - 1.0, 0.37, 2.81, sps - 0.004, 1.5])
    n = np.arange(length)[None, :]
    amp = np.sqrt(1.0 + np.cos(2 * np.pi * (n - t0[:, None]) / sps))
    phase = np.random.default_rng(sps).uniform(0, 2 * np.pi, amp.shape)
    raw = np.stack([amp * np.cos(phase), amp * np.sin(phase)], axis=2)
    n_frac = 32
    rx = Receiver(sps, 2, n_frac=n_frac, timing="oerder_meyr", table=delta_table(sps, 2, n_frac))
    _, est = rx(to_dev(raw), return_est=True)
    e = est.cpu().numpy().astype(np.float64)
    dist = circular_distance(e[:, 0], t0, sps)
    print(f"sps {sps}: |t0 - constructed| {dist.max():.2e} samples; |X| / sum E {e[:, 2].min():.4f} .. {e[:, 2].max():.4f}")
    assert np.all(dist <= 1e-3)
    assert np.all(circular_distance(e[:, 1], np.rint(e[:, 0] * n_frac), sps * n_frac) == 0)
    assert np.all(np.abs(e[:, 2] - 0.5) <= 1e-3)


SHAPED = {"a": dict(length=1024, sps=8, span=8, alpha=0.35, n_phase=32), "b": dict(length=384, sps=3, span=6, alpha=0.5, n_phase=8)}


@pytest.mark.parametrize("shape", ["a", "b"])
def test_timing_and_symbols_on_shaped_frames_match_the_definition(shape):
    """Noisy three-tap ShapedSynth frames.  t0 within 1e-3 sample and u within one step of the definition's (circular); the
    symbols, with the definition fed the kernel's own u, within the bound of the normalised case."""
    from vit_vs_raw_iq_amd import Receiver, ShapedSynth, receiver_reference
    ws = ShapedSynth(["BPSK", "QPSK", "16QAM", "8PSK"], snrs_db=(10.0, 20.0), seed=3, taps=3, **SHAPED[shape])
    raw_t, _, _, drawn = ws.generate(24, 5, 0, return_drawn=True)
    raw = raw_t.cpu().numpy()
    sps, n_frac = ws.sps, ws.n_phase
    rx = Receiver.for_synth(ws)
    sym, est, energy = rx(raw_t, return_est=True, return_energy=True)
    e = est.cpu().numpy().astype(np.float64)
    _, est_ref, en_ref = receiver_reference(raw, rx.table, sps, "oerder_meyr")
    assert np.all(circular_distance(e[:, 0], est_ref[:, 0], sps) <= 1e-3)
    assert np.all(circular_distance(e[:, 1], est_ref[:, 1], sps * n_frac) <= 1)
    assert np.all((e[:, 1] >= 0) & (e[:, 1] < sps * n_frac) & (e[:, 1] == np.rint(e[:, 1])))
    assert np.all(np.abs(e[:, 2] - est_ref[:, 2]) <= 1e-4)
    us = e[:, 1].astype(np.int64)
    ref, est_g, _ = receiver_reference(raw, rx.table, sps, "given", us)
    bound = dot_bound(sps * ws.span + 1, abs_windows(raw, rx.table, sps, us)) / np.sqrt(est_g[:, 3] + 1e-12)[:, None, None] + 4 * EPS * np.abs(ref)
    err = np.abs(sym.cpu().numpy().astype(np.float64) - ref)
    assert np.all(err <= bound), float((err / bound).max())
    assert np.all(np.abs(e[:, 3] - est_g[:, 3]) <= 1e-5 * est_g[:, 3])
    # ENERGY mode: the definition's residue wherever the two best energies differ by more than fp32 can blur (1e-4 of the best)
    re = Receiver.for_synth(ws, timing="energy")
    _, est_e = re(raw_t, return_est=True)
    ee = est_e.cpu().numpy().astype(np.float64)
    top = np.sort(en_ref, axis=1)
    clear = top[:, -1] - top[:, -2] > 1e-4 * top[:, -1]
    assert clear.sum() >= 12
    assert np.array_equal(ee[clear, 1], n_frac * np.argmax(en_ref, axis=1)[clear]) and np.array_equal(ee[:, 0] * n_frac, ee[:, 1])
    assert same_bits(re(raw_t, return_energy=True)[1], energy)


def test_energy_mode_takes_the_lowest_residue_on_a_tie():
    from vit_vs_raw_iq_amd import Receiver, receiver_reference
    raw = np.zeros((3, 16, 2), np.float32)
    raw[0, 1, 0] = raw[0, 3, 1] = 2.0                      # E = {0, 4, 0, 4}
    raw[1, 6, 0] = raw[1, 4, 0] = raw[1, 7, 1] = 1.0       # E = {1, 0, 1, 1}
    rx = Receiver(4, 1, n_frac=8, timing="energy", normalise=False, table=delta_table(4, 1, 8))
    _, est, energy = rx(to_dev(raw), return_est=True, return_energy=True)
    _, est_ref, en_ref = receiver_reference(raw, rx.table, 4, "energy", normalise=False)
    assert np.array_equal(energy.cpu().numpy(), en_ref) and np.array_equal(est_ref[:, 1], [8, 0, 0])
    assert np.array_equal(est.cpu().numpy()[:, :2].astype(np.float64), est_ref[:, :2])


@pytest.mark.parametrize("shape", ["a", "b"])
def test_the_loop_closes_on_the_device(shape):
    """ShapedSynth (noiseless, one tap) -> Receiver -> the transmitted symbols found by transmitted_index, under the caps of the
    host test: t0 within 0.1 sample of the true instant, interior EVM at most 0.03 after one complex gain."""
    from vit_vs_raw_iq_amd import Receiver, ShapedSynth, transmitted_index
    ws = ShapedSynth(["QPSK", "16QAM"], snrs_db=None, seed=21, taps=1, **SHAPED[shape])
    n = 16 * ws.n_phase
    raw, y, _, drawn, symbols = ws.generate(n, 0, 0, return_drawn=True, return_symbols=True)
    rx = Receiver.for_synth(ws)
    sym, est = rx(raw, return_est=True)
    e, d, s = est.cpu().numpy().astype(np.float64), drawn.cpu().numpy().astype(np.float64), symbols.cpu().numpy()
    got, cls = complex_frames(sym.cpu().numpy()), y.cpu().numpy()
    q = d[:, 4]
    assert len(set(q.tolist())) == ws.n_phase                      # every timing phase is there
    dist = circular_distance(e[:, 0], true_instant(ws.sps, ws.span, ws.n_phase, q), ws.sps)
    k0 = transmitted_index(ws, q, e[:, 1])
    pts = ws.points[:, 0].astype(np.float64) + 1j * ws.points[:, 1].astype(np.float64)
    k = np.arange(ws.span, ws.length // ws.sps - ws.span)
    evms = []
    for i in range(n):
        _, off, _ = ws.descriptors[int(cls[i])]
        evms.append(evm(pts[off + s[i, k0[i] + k]], got[i, k]))
    print(f"{shape}: worst |t0 - true| {dist.max():.4f} samples (cap {T0_CAP}), worst EVM {max(evms):.4f} (cap {EVM_CAP})")
    assert dist.max() <= T0_CAP and max(evms) <= EVM_CAP


@pytest.mark.parametrize("B,length,sps,span,n_frac", [(4, 1024, 8, 8, 32), (4, 385, 3, 6, 8), (2, 8192, 16, 32, 4), (4, 100, 1, 4, 3)])
def test_backward_matches_the_fp64_adjoint_and_repeats_bit_for_bit(B, length, sps, span, n_frac):
    """dx[n] is a chain of T <= span + 1 terms: |dx - ref| <= 2 (T + 2) 2^-24 sum_k |dv_k| |G| + sum_k |G| D_k, D_k the error
    the kernel's dv carries.  Not normalised: dv = ds, D = 0.  Normalised: dv = (ds - s c) / rho from the fp32 s (error ds_k, the
    forward's bound), c = <ds, s> / n_out (a sum of n_out terms) and the fp32 rho (relative error eta / 2 + 3 eps, eta that of
    mean |v|^2: (2 sum |v| dv + (n_out + 2) eps sum |v|^2) / sum |v|^2):
    D_k = (3 eps (|ds_k| + |s_k c|) + |c| ds_k + |s_k| dc) / rho + (eta / 2 + 3 eps) |dv_k|, dc = (sum_i |ds_i| ds_i + (n_out + 2)
    eps sum_i |ds_i s_i|) / n_out, eps = 2^-24."""
    from vit_vs_raw_iq_amd import Receiver, mf_table, receiver_reference, receiver_reference_bwd
    rng = np.random.default_rng(7 * length + sps)
    raw = rng.standard_normal((B, length, 2)).astype(np.float32)
    table = mf_table(0.35, sps, span, n_frac)
    us = rng.integers(0, sps * n_frac, B)
    n_out, J = length // sps, sps * span
    w = rng.standard_normal((B, n_out, 2)).astype(np.float32)
    absG = np.abs(table.astype(np.float64))
    for normalise in (False, True):
        rx = Receiver(sps, span, n_frac=n_frac, timing="given", normalise=normalise, table=table)
        x = to_dev(raw).requires_grad_()
        sym = rx(x, u=us)
        (dx,) = torch.autograd.grad(sym, x, to_dev(w))
        (dx2,) = torch.autograd.grad(rx(x, u=us), x, to_dev(w))
        assert same_bits(dx, dx2)
        ref = receiver_reference_bwd(raw, w, table, sps, us, normalise)
        s_ref, est_ref, _ = receiver_reference(raw, table, sps, "given", us, normalise)
        adv = np.abs(w.astype(np.float64))
        D = np.zeros_like(adv)
        if normalise:
            rho = np.sqrt(est_ref[:, 3] + 1e-12)[:, None, None]
            bv = dot_bound(J + 1, abs_windows(raw, table, sps, us))
            ds = bv / rho + 4 * EPS * np.abs(s_ref)
            v2 = (np.abs(s_ref * rho) ** 2).sum(axis=(1, 2))
            eta = ((2 * (np.abs(s_ref * rho) * bv).sum(axis=(1, 2)) + (n_out + 2) * EPS * v2) / v2)[:, None, None]
            wc, sc = complex_frames(w), complex_frames(s_ref)
            c = ((wc.real * sc.real + wc.imag * sc.imag).sum(axis=1) / n_out)[:, None, None]
            dc = ((adv * ds).sum(axis=(1, 2)) + (n_out + 2) * EPS * (adv * np.abs(s_ref)).sum(axis=(1, 2)))[:, None, None] / n_out
            dv = (w - s_ref * c) / rho
            D = (3 * EPS * (adv + np.abs(s_ref * c)) + np.abs(c) * ds + np.abs(s_ref) * dc) / rho + (eta / 2 + 3 * EPS) * np.abs(dv)
            adv = np.abs(dv)
        bound = np.zeros((B, length, 2))
        for b in range(B):
            rh, fh = int(us[b]) // n_frac, int(us[b]) % n_frac
            acc = np.zeros((length + 2 * J + sps + 1, 2))
            for k in range(n_out):
                acc[rh + k * sps:rh + k * sps + J + 1] += (2 * (span + 3) * EPS * adv[b, k] + D[b, k])[None, :] * absG[fh][:, None]
            bound[b] = acc[J // 2:J // 2 + length]
        err = np.abs(dx.cpu().numpy().astype(np.float64) - ref)
        print(f"len {length} sps {sps} normalise {normalise}: |dx - ref| / bound {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
        assert np.all(err <= bound)


@pytest.mark.parametrize("B,length,sps,span", [(3, 257, 8, 2), (3, 255, 3, 5), (3, 16, 16, 32), (3, 8192, 16, 32), (3, 31, 1, 1)])
def test_backward_is_the_exact_adjoint_in_integers(B, length, sps, span):
    """<R x, w> = <x, R^T w> with integer frames, tables and cotangents, not normalised: both sides are integers below 2^24 per
    term, summed here in int64.  And R^T w is the fp64 adjoint bit for bit."""
    from vit_vs_raw_iq_amd import Receiver, receiver_reference_bwd
    n_frac = 4
    raw, table, us = integer_case(length + 5 * sps, B, length, sps, span, n_frac)
    rng = np.random.default_rng(length)
    w = rng.integers(-2, 3, (B, length // sps, 2)).astype(np.float32)
    rx = Receiver(sps, span, n_frac=n_frac, timing="given", normalise=False, table=table)
    x = to_dev(raw).requires_grad_()
    sym = rx(x, u=us)
    (dx,) = torch.autograd.grad(sym, x, to_dev(w))
    lhs = (sym.detach().cpu().numpy().astype(np.int64) * w.astype(np.int64)).sum(axis=(1, 2))
    rhs = (dx.cpu().numpy().astype(np.int64) * raw.astype(np.int64)).sum(axis=(1, 2))
    assert np.array_equal(lhs, rhs)
    assert np.array_equal(dx.cpu().numpy().astype(np.float64), receiver_reference_bwd(raw, w, table, sps, us, False))


def test_frames_are_independent():
    from vit_vs_raw_iq_amd import Receiver
    rng = np.random.default_rng(1)
    B, length, sps = 37, 385, 3
    raw = to_dev(rng.standard_normal((B, length, 2)))
    rx = Receiver(sps, 6, alpha=0.5, n_frac=8)
    out = rx(raw, return_est=True, return_energy=True)
    perm = torch.from_numpy(rng.permutation(B)).to(dev())
    for a, b in zip(rx(raw[perm].contiguous(), return_est=True, return_energy=True), out):
        assert same_bits(a, b[perm])
    # a NaN frame poisons only itself, forward and backward
    bad = raw.clone()
    bad[5, 100, 1] = float("nan")
    x = bad.requires_grad_()
    got = rx(x, return_est=True, return_energy=True)
    keep = torch.arange(B, device=dev()) != 5
    for a, b in zip(got, out):
        assert same_bits(a[keep], b[keep])
    assert torch.isnan(got[0][5]).all() and got[1][5, 1] == 0
    w = to_dev(rng.standard_normal((B, length // sps, 2)))
    (dx_bad,) = torch.autograd.grad(got[0], x, w)
    y = raw.clone().requires_grad_()
    (dx,) = torch.autograd.grad(rx(y), y, w)
    assert same_bits(dx_bad[keep], dx[keep]) and torch.isfinite(dx).all()


def test_buffers_around_inputs_and_outputs_stay_as_they_were():
    """Inputs carved out of NaN-filled buffers (a read outside them would poison the result), outputs out of patterned ones."""
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import Receiver, receiver_reference
    B, length, sps, span, n_frac = 7, 47, 3, 5, 4
    raw, table, us = integer_case(9, B, length, sps, span, n_frac)
    n_out = length // sps
    rx = Receiver(sps, span, n_frac=n_frac, timing="given", normalise=False, table=table)
    pad = 64

    def carve(values, dtype):
        flat = torch.as_tensor(np.ascontiguousarray(values)).to(dtype).flatten()
        buf = torch.full((flat.numel() + 2 * pad,), float("nan") if dtype.is_floating_point else -2 ** 31, dtype=dtype, device=dev())
        buf[pad:pad + flat.numel()] = flat.to(dev())
        return buf, buf.data_ptr() + pad * buf.element_size()
    raw_b, raw_p = carve(raw, torch.float32)
    tab_b, tab_p = carve(table, torch.float32)
    u_b, u_p = carve(us, torch.int32)
    sizes = {"sym": B * n_out * 8, "est": B * 16, "energy": B * sps * 4, "dx": B * length * 8}
    offs, total = {}, 256
    for k, v in sizes.items():
        offs[k] = total
        total += (v + 15) // 16 * 16 + 256
    pattern = torch.arange(total, dtype=torch.int64).mul_(37).add_(11).remainder_(251).to(torch.uint8).to(dev())
    buf = pattern.clone()
    p = {k: buf.data_ptr() + o for k, o in offs.items()}
    par = rx.struct(tab_p, u_p)
    N.check(N.lib().iq_frames_receive(raw_p, p["sym"], p["est"], p["energy"], B, length, ctypes.byref(par), N.stream_handle()),
            "iq_frames_receive")
    w = np.random.default_rng(2).integers(-2, 3, (B, n_out, 2))
    w_b, w_p = carve(w, torch.float32)
    N.check(N.lib().iq_frames_receive_bwd(w_p, None, None, p["dx"], B, length, ctypes.byref(par), N.stream_handle()),
            "iq_frames_receive_bwd")
    torch.cuda.synchronize()
    inside = torch.zeros(total, dtype=torch.bool, device=dev())
    for k, v in sizes.items():
        inside[offs[k]:offs[k] + v] = True
    assert torch.equal(buf[~inside], pattern[~inside])
    take = lambda k, shape: buf[offs[k]:offs[k] + sizes[k]].view(torch.float32).view(shape).cpu().numpy().astype(np.float64)   # noqa: E731
    sym_ref, _, en_ref = receiver_reference(raw, table, sps, "given", us, False)
    assert np.array_equal(take("sym", (B, n_out, 2)), sym_ref) and np.array_equal(take("energy", (B, sps)), en_ref)
    x = to_dev(raw).requires_grad_()
    (dx,) = torch.autograd.grad(rx(x, u=us), x, to_dev(w))
    assert np.array_equal(take("dx", (B, length, 2)), dx.cpu().numpy().astype(np.float64))
    for b in (raw_b, tab_b, w_b):
        assert torch.isnan(b[:pad]).all() and torch.isnan(b[-pad:]).all()


def test_refusals_return_their_code_and_leave_the_outputs_untouched():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import Receiver
    L = N.lib()
    sentinel = 1234.5
    B, length = 4, 64
    rx = Receiver(8, 4, n_frac=8)
    table = rx.table_on(dev())
    raw = torch.zeros(B, length, 2, device=dev())
    sym = torch.full((B, length // 8, 2), sentinel, device=dev())
    est = torch.full((B, 4), sentinel, device=dev())
    energy = torch.full((B, 8), sentinel, device=dev())
    dx = torch.full((B, length, 2), sentinel, device=dev())
    u = torch.zeros(B, dtype=torch.int32, device=dev())
    ARG, UNSUPPORTED = 1, 2

    def fwd(length=length, par="ok", **kw):
        p = dict(raw=raw.data_ptr(), sym=sym.data_ptr(), est=est.data_ptr(), energy=energy.data_ptr())
        fields = {k: kw.pop(k) for k in list(kw) if k not in p}
        p.update(kw)
        if par == "ok":
            par = rx.struct(table.data_ptr(), u.data_ptr())
            for k, v in fields.items():
                setattr(par, k, v)
        return L.iq_frames_receive(p["raw"], p["sym"], p["est"], p["energy"], B, length,
                                   ctypes.byref(par) if par is not None else None, N.stream_handle())

    def bwd(length=length, par="ok", **kw):
        p = dict(dsym=raw.data_ptr(), sym=sym.data_ptr(), est=est.data_ptr(), dx=dx.data_ptr())
        fields = {k: kw.pop(k) for k in list(kw) if k not in p}
        p.update(kw)
        if par == "ok":
            par = rx.struct(table.data_ptr(), u.data_ptr())
            for k, v in fields.items():
                setattr(par, k, v)
        return L.iq_frames_receive_bwd(p["dsym"], p["sym"], p["est"], p["dx"], B, length,
                                       ctypes.byref(par) if par is not None else None, N.stream_handle())
    assert fwd(raw=None) == ARG and fwd(sym=None) == ARG and fwd(par=None) == ARG and fwd(table=None) == ARG
    assert bwd(dsym=None) == ARG and bwd(dx=None) == ARG and bwd(par=None) == ARG and bwd(table=None) == ARG
    assert bwd(sym=None) == ARG and bwd(est=None) == ARG                       # normalise = 1 needs both
    for call in (fwd, bwd):
        assert call(length=0) == ARG and call(length=-8) == ARG
        for field in ("sps", "span", "n_frac"):
            assert call(**{field: 0}) == ARG and call(**{field: -1}) == ARG, field
        assert call(mode=3) == ARG and call(mode=-1) == ARG and call(normalise=2) == ARG and call(normalise=-1) == ARG
        assert call(table=table.data_ptr() + 2) == ARG and call(u=u.data_ptr() + 2) == ARG
        assert call(sps=17) == UNSUPPORTED and call(span=33) == UNSUPPORTED and call(n_frac=65) == UNSUPPORTED
        assert call(length=8193) == UNSUPPORTED and call(length=7) == UNSUPPORTED
    assert fwd(raw=raw.data_ptr() + 4) == ARG and fwd(sym=sym.data_ptr() + 4) == ARG
    assert fwd(est=est.data_ptr() + 2) == ARG and fwd(energy=energy.data_ptr() + 2) == ARG
    assert bwd(dsym=raw.data_ptr() + 4) == ARG and bwd(dx=dx.data_ptr() + 4) == ARG
    assert bwd(sym=sym.data_ptr() + 4) == ARG and bwd(est=est.data_ptr() + 2) == ARG
    assert fwd(sps=2, mode=1) == UNSUPPORTED                                   # Oerder-Meyr needs three samples per symbol
    torch.cuda.synchronize()
    for t in (sym, est, energy, dx):
        assert torch.equal(t, torch.full_like(t, sentinel))
    assert L.iq_frames_receive(raw.data_ptr(), sym.data_ptr(), None, None, 0, length,
                               ctypes.byref(rx.struct(table.data_ptr())), N.stream_handle()) == 0
    torch.cuda.synchronize()
    assert torch.equal(sym, torch.full_like(sym, sentinel))


def preprocess(raw, take, stats):
    import vit_vs_raw_iq_amd._native as N
    B, length = raw.shape[0], raw.shape[1]
    out = torch.empty(B, 2, take, device=raw.device)
    st = (ctypes.c_float * 4)(stats["i_mean"], stats["i_std"], stats["q_mean"], stats["q_std"])
    N.check(N.lib().iq_frames_preprocess(raw.data_ptr(), out.data_ptr(), B, length, take, st, N.stream_handle()),
            "iq_frames_preprocess")
    return out


def test_received_stream_is_generate_then_receive_then_the_input_pipeline():
    from vit_vs_raw_iq_amd import ReceivedSynth, Receiver, ShapedSynth, SynthStream
    ws = ShapedSynth(seed=5, length=1024, sps=8, taps=3)
    rx = Receiver.for_synth(ws)
    rs = ReceivedSynth(ws, rx)
    assert rs.length == 128 and rs.n_classes == ws.n_classes
    stats = rs.stats(n_subset=76)
    first = rs.generate(76, 0, 0)[0].cpu().numpy().astype(np.float64)
    assert abs(stats["i_mean"] - first[:, :, 0].mean()) < 1e-4 and abs(stats["q_std"] - first[:, :, 1].std(ddof=1)) < 1e-4
    B, s = 12, 3
    raw, y, z, drawn = ws.generate(B, s * B, 0, return_drawn=True)
    sym, est = rx(raw, return_est=True)
    got = rs.generate(B, s * B, 0, return_drawn=True, return_est=True)
    assert len(got) == 5 and same_bits(got[0], sym) and torch.equal(got[1], y) and same_bits(got[3], drawn) and same_bits(got[4], est)
    x, ys, zs = SynthStream(rs, stats, "rawiq", B).get(s)
    assert x.shape == (B, 2, 128) and same_bits(x, preprocess(sym, 128, stats)) and torch.equal(ys, y) and same_bits(zs, z)
    xv, _, _ = SynthStream(rs, stats, "vit", B, h=8, w=8).get(s)
    assert xv.shape == (B, 1, 8, 8) and same_bits(xv.reshape(B, 2, 32), preprocess(sym, 32, stats))


def test_graph_replay_equals_eager():
    """A capture fails on any host synchronisation: generate -> receive -> backward are captured whole."""
    from vit_vs_raw_iq_amd import ReceivedSynth, Receiver, ShapedSynth
    ws = ShapedSynth(seed=9, length=1024, sps=8, taps=2)
    rx = Receiver.for_synth(ws)
    rs = ReceivedSynth(ws, rx)
    w = to_dev(np.random.default_rng(4).standard_normal((76, 128, 2)))

    def run():
        sym, y, z, est = rs.generate(76, 19, 0, return_est=True)
        x = ws.generate(76, 19, 0)[0].requires_grad_()
        (dx,) = torch.autograd.grad(rx(x), x, w)
        return sym, est, dx
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
        assert same_bits(a, b)


FOUR = ["BPSK", "QPSK", "16QAM", "OQPSK"]
TRAIN_STEPS = 200


def test_a_model_trained_on_received_symbols_beats_chance_on_frames_of_another_stream(tmp_path):
    """A raw-IQ model at one sample per symbol (128 symbols, segments of 16) on a ReceivedSynth stream: every step trains on 256
    frames that were never used; the accuracy on 2048 frames of stream 1 must exceed 1.5 x chance = 0.375."""
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import ReceivedSynth, Receiver, ShapedSynth, SynthStream, train_on_stream
    from vit_vs_raw_iq_amd.evaluation import evaluate_model_with_confusion
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    ws = ShapedSynth(FOUR, snrs_db=(20.0,), length=1024, seed=11, sps=8)
    rs = ReceivedSynth(ws, Receiver.for_synth(ws))
    stats = rs.stats(n_subset=1024)
    torch.manual_seed(0)
    m = P.AMCTransformerRawIQ(in_channels=2, seq_length=128, num_classes=4, d_model=128, n_head=8, n_layers=2, ffn_hidden=256,
                              drop_prob=0.0, device="cuda", use_cls_token=True, embedding_type="segment", segment_size=16)
    m = m.to(dev()).train()
    tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-3)
    assert train_on_stream(tr, SynthStream(rs, stats, "rawiq", 256), TRAIN_STEPS) == TRAIN_STEPS
    loss, acc_train, frames = tr.read_stats()
    assert frames == TRAIN_STEPS * 256
    held = SynthStream(rs, stats, "rawiq", 256, stream=1)
    res = evaluate_model_with_confusion(m, held.batches(8), dev(), FOUR, tmp_path, prefix="receiver")
    bound = 1.5 * 0.25
    print(f"{TRAIN_STEPS} steps of 256 fresh frames: running train loss {loss:.4f}, accuracy {acc_train:.4f}; "
          f"held-out accuracy on 2048 frames of stream 1 {res['overall_accuracy']:.4f} (bound {bound:.4f})")
    assert np.array_equal(res["labels"], np.arange(2048) % 4) and res["confusion_matrix"].sum() == 2048
    assert res["overall_accuracy"] > bound
