"""CPU: the host side of the receiver (vit_vs_raw_iq_amd.receiver) -- its fp64 definitions against independent statements
(tests/receiver_ref.py), the tap table, the binding's struct, every Python refusal, and the end-to-end property of the
definition itself: a host transmitter's noiseless frames come back as their symbols at every timing phase.

Caps of the end-to-end property (conditions, not measurements): the Oerder-Meyr t0 within 0.1 sample (circular) of the true
instant; interior symbols (span dropped at each end) at an error-vector magnitude of at most 0.03 after one complex gain.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from receiver_ref import (EVM_CAP, T0_CAP, circular_distance, complex_frames, evm, host_transmit, matched_filter_by_convolution, torch_receive,
                          true_instant)


def small_case(seed, B, length, sps, span, n_frac):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((B, length, 2))
    table = rng.standard_normal((n_frac, sps * span + 1)).astype(np.float32)
    u = rng.integers(0, sps * n_frac, B)
    return raw, table, u


@pytest.mark.parametrize("length,sps,span,n_frac", [(64, 4, 3, 5), (37, 3, 5, 7), (16, 1, 1, 1), (50, 2, 4, 3), (48, 16, 2, 2)])
def test_reference_is_the_convolution_statement(length, sps, span, n_frac):
    from vit_vs_raw_iq_amd import receiver_reference
    raw, table, u = small_case(length, 3, length, sps, span, n_frac)
    for normalise in (False, True):
        sym, est, energy = receiver_reference(raw, table, sps, "given", u, normalise)
        assert sym.shape == (3, length // sps, 2) and est.shape == (3, 4) and energy.shape == (3, sps)
        for b in range(3):
            E, v = matched_filter_by_convolution(complex_frames(raw[b]), table, sps, int(u[b]))
            mean = np.mean(np.abs(v) ** 2)
            s = v / np.sqrt(mean + 1e-12) if normalise else v
            scale = max(1.0, np.abs(v).max())
            assert np.abs(complex_frames(sym[b]) - s).max() <= 1e-12 * scale
            assert np.abs(energy[b] - E).max() <= 1e-12 * E.max()
            assert np.isnan(est[b, 0]) and est[b, 1] == u[b] and abs(est[b, 3] - mean) <= 1e-12 * mean
            X = np.sum(E * np.exp(-2j * np.pi * np.arange(sps) / sps))
            assert abs(est[b, 2] - abs(X) / E.sum()) <= 1e-12


def test_reference_timing_modes():
    from vit_vs_raw_iq_amd import receiver_reference
    raw, table, _ = small_case(5, 4, 96, 4, 3, 8)
    _, est_g, energy = receiver_reference(raw, table, 4, "given")
    assert np.all(est_g[:, 1] == 0)
    _, est_e, _ = receiver_reference(raw, table, 4, "energy")
    assert np.array_equal(est_e[:, 1], 8 * np.argmax(energy, axis=1)) and np.array_equal(est_e[:, 0], np.argmax(energy, axis=1))
    sym_o, est_o, _ = receiver_reference(raw, table, 4, "oerder_meyr")
    X = energy @ np.exp(-2j * np.pi * np.arange(4) / 4)
    t0 = (-np.angle(X) * 4 / (2 * np.pi)) % 4
    assert np.allclose(est_o[:, 0], t0, atol=1e-12) and np.array_equal(est_o[:, 1], np.rint(t0 * 8) % 32)
    sym_g, _, _ = receiver_reference(raw, table, 4, "given", est_o[:, 1].astype(np.int64))
    assert np.array_equal(sym_g, sym_o)
    # ties go to the lowest residue: two equal deltas through a delta filter
    delta = np.zeros((1, 5), np.float32)
    delta[0, 2] = 1.0
    tie = np.zeros((1, 16, 2))
    tie[0, 1, 0] = tie[0, 3, 1] = 2.0
    _, est_t, en_t = receiver_reference(tie, delta, 4, "energy")
    assert np.array_equal(en_t[0], [0.0, 4.0, 0.0, 4.0]) and est_t[0, 1] == 1 and est_t[0, 0] == 1
    # an all-zero frame: no NaN, u = 0
    s0, e0, _ = receiver_reference(np.zeros((1, 16, 2)), delta, 4, "oerder_meyr")
    assert np.all(s0 == 0) and e0[0, 1] == 0 and e0[0, 2] == 0 and e0[0, 3] == 0


@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("length,sps,span,n_frac", [(40, 4, 3, 5), (37, 3, 5, 7), (12, 1, 1, 1), (35, 2, 4, 3)])
def test_reference_backward_is_autograd_of_the_torch_restatement(length, sps, span, n_frac, normalise):
    from vit_vs_raw_iq_amd import receiver_reference, receiver_reference_bwd
    raw, table, u = small_case(100 + length, 2, length, sps, span, n_frac)
    x = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
    sym = torch_receive(x, table, sps, u, normalise)
    assert np.abs(sym.detach().numpy() - receiver_reference(raw, table, sps, "given", u, normalise)[0]).max() <= 1e-12
    w = np.random.default_rng(7).standard_normal(tuple(sym.shape))
    (sym * torch.tensor(w)).sum().backward()
    dx = receiver_reference_bwd(raw, w, table, sps, u, normalise)
    assert dx.shape == raw.shape
    assert np.abs(dx - x.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(dx).max())


def test_mf_table():
    from vit_vs_raw_iq_amd import mf_table
    from vit_vs_raw_iq_amd.waveform import rrc_pulse
    for alpha, sps, span, n_frac in ((0.35, 8, 8, 32), (0.5, 3, 6, 8), (0.2, 2, 10, 4), (1.0, 4, 4, 1)):
        G = mf_table(alpha, sps, span, n_frac)
        J = sps * span
        assert G.shape == (n_frac, J + 1) and G.dtype == np.float32
        assert np.array_equal(G[0], G[0][::-1])                                      # row 0 is symmetric
        # unit energy, up to what the span cuts off: the tail of p^2 beyond +- span / 2, bounded by the full-line integral
        t = np.arange(-200 * sps, 200 * sps + 1) / sps
        full = np.sum(rrc_pulse(t, alpha) ** 2) / sps
        cut = np.sum(rrc_pulse(t[np.abs(t) > span / 2], alpha) ** 2) / sps
        e0 = float(np.sum(G[0].astype(np.float64) ** 2))
        assert abs(full - 1.0) < 2e-3 and abs(e0 - (full - cut)) < 1e-6, (alpha, sps, span, e0, full, cut)
        # definition, entry by entry
        f, j = np.meshgrid(np.arange(n_frac), np.arange(J + 1), indexing="ij")
        arg = (f / n_frac + J // 2 - j) / sps
        want = np.where(np.abs(arg) > span / 2 + 1e-12, 0.0, rrc_pulse(arg, alpha) / np.sqrt(sps))
        assert np.abs(G - want).max() <= 2.0 ** -24 * np.abs(want).max() + 1e-15
    # row f = row 0 of the table at n_frac times the rate, every n_frac-th tap: G[f][j] = sqrt(n_frac) G'[0][j n_frac - f]
    for alpha, sps, span, n_frac in ((0.35, 2, 6, 8), (0.5, 4, 4, 4), (0.25, 3, 6, 4)):
        G, fine = mf_table(alpha, sps, span, n_frac), mf_table(alpha, sps * n_frac, span, 1)
        J = sps * span
        for f in range(n_frac):
            idx = np.arange(J + 1) * n_frac - f
            want = np.where(idx >= 0, fine[0][np.clip(idx, 0, None)].astype(np.float64) * np.sqrt(n_frac), 0.0)
            assert np.abs(G[f] - want).max() <= 2.0 ** -22, (sps, n_frac, f)
    for bad, exc in (((1.5, 8, 8, 32), ValueError), ((-0.1, 8, 8, 32), ValueError), ((float("nan"), 8, 8, 32), ValueError),
                     (("a", 8, 8, 32), TypeError), ((0.35, 0, 8, 32), ValueError), ((0.35, 17, 8, 32), ValueError),
                     ((0.35, 8, 33, 32), ValueError), ((0.35, 8, 0, 32), ValueError), ((0.35, 8, 8, 65), ValueError),
                     ((0.35, 8, 8, 0), ValueError), ((0.35, 8.0, 8, 32), TypeError), ((0.35, True, 8, 32), TypeError)):
        with pytest.raises(exc):
            mf_table(*bad)


def test_binding_struct_matches_the_header():
    import vit_vs_raw_iq_amd._native as N
    src = open(os.path.join(ROOT, "include", "iqvit.h")).read()
    body = re.search(r"typedef struct iq_receiver \{(.*?)\}", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", d)[-1] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in N.Receiver._fields_]
    assert [f[1] for f in N.Receiver._fields_] == [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    assert ctypes.sizeof(N.Receiver) == 40 and N.Receiver.table.offset == 24 and N.Receiver.u.offset == 32
    enum = re.search(r"enum \{ IQ_RX_GIVEN = (\d), IQ_RX_OERDER_MEYR = (\d), IQ_RX_ENERGY = (\d) \}", src)
    from vit_vs_raw_iq_amd.receiver import MODES
    assert [int(v) for v in enum.groups()] == [MODES.index(m) for m in ("given", "oerder_meyr", "energy")]
    assert N.SIGNATURES["iq_frames_receive"][1][6] is not None and len(N.SIGNATURES["iq_frames_receive_bwd"][1]) == 8
    L = N.lib()
    par = N.Receiver(sps=8, span=8, n_frac=32, mode=1, normalise=1, table=None, u=None)
    assert L.iq_frames_receive(None, None, None, None, 1, 1024, ctypes.byref(par), None) == 1       # refused on the host
    assert L.iq_frames_receive_bwd(None, None, None, None, 1, 1024, ctypes.byref(par), None) == 1


def test_python_refusals():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import ReceivedSynth, Receiver, ShapedSynth, receiver_reference, receiver_reference_bwd, transmitted_index
    for kw, exc in ((dict(sps=0), ValueError), (dict(sps=17), ValueError), (dict(sps=8.0), TypeError), (dict(sps=8, span=0), ValueError),
                    (dict(sps=8, span=33), ValueError), (dict(sps=8, n_frac=0), ValueError), (dict(sps=8, n_frac=65), ValueError),
                    (dict(sps=8, alpha=2.0), ValueError), (dict(sps=8, alpha="x"), TypeError), (dict(sps=8, timing="gardner"), ValueError),
                    (dict(sps=2, timing="oerder_meyr"), ValueError), (dict(sps=8, normalise="yes"), TypeError),
                    (dict(sps=2, span=2, n_frac=2, timing="energy", table=np.zeros((2, 4))), ValueError),
                    (dict(sps=2, span=2, n_frac=2, timing="energy", table=np.full((2, 5), np.inf)), ValueError),
                    (dict(sps=2, span=2, n_frac=2, timing="energy", table=[["a"] * 5] * 2), TypeError)):
        with pytest.raises(exc):
            Receiver(**kw)
    rx = Receiver(8, device="cpu")
    assert rx.table.shape == (32, 65) and rx.mode == 1 and rx.n_out(1024) == 128
    assert Receiver(2, timing="energy", device="cpu").mode == 2 and Receiver(1, timing="given", span=1, n_frac=1, device="cpu").mode == 0
    with pytest.raises(ValueError, match=r"\(B, len, 2\)"):
        rx(torch.zeros(4, 2, 1024))
    with pytest.raises(ValueError, match=r"\(B, len, 2\)"):
        rx(np.zeros((4, 1024, 2)))
    with pytest.raises(ValueError, match="frame length"):
        rx(torch.zeros(4, 7, 2))
    with pytest.raises(ValueError, match="frame length"):
        rx(torch.zeros(1, 8193, 2))
    with pytest.raises(ValueError, match="timing='given'"):
        rx(torch.zeros(4, 1024, 2), u=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="return_est"):
        rx(torch.zeros(4, 1024, 2), return_est="yes")
    with pytest.raises(P.IqError, match="no CPU fallback"):
        rx(torch.zeros(4, 1024, 2))
    rg = Receiver(8, timing="given", device="cpu")
    with pytest.raises(TypeError, match="integers"):
        rg(torch.zeros(4, 1024, 2), u=torch.zeros(4))
    with pytest.raises(TypeError, match="integers"):
        rg(torch.zeros(4, 1024, 2), u=[0.5] * 4)
    with pytest.raises(ValueError, match="shape"):
        rg(torch.zeros(4, 1024, 2), u=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="sps \\* n_frac"):
        rg(torch.zeros(4, 1024, 2), u=[0, 1, 2, 256])
    with pytest.raises(P.IqError, match="no CPU fallback"):
        rg(torch.zeros(4, 1024, 2), u=[0, 1, 2, 255])
    ws = ShapedSynth(["QPSK"], None, length=1024, device="cpu")
    with pytest.raises(TypeError):
        Receiver.for_synth(P.FrameSynth(["QPSK"], None, device="cpu"))
    r2 = Receiver.for_synth(ws, timing="energy")
    assert (r2.sps, r2.span, r2.alpha, r2.n_frac, r2.mode) == (8, 8, 0.35, 32, 2)
    with pytest.raises(TypeError):
        ReceivedSynth(P.FrameSynth(["QPSK"], None, device="cpu"), r2)
    with pytest.raises(TypeError):
        ReceivedSynth(ws, "rx")
    with pytest.raises(ValueError, match="sps"):
        ReceivedSynth(ws, Receiver(4, device="cpu"))
    rs = ReceivedSynth(ws, r2)
    assert isinstance(rs, P.FrameSynth) and rs.length == 128 and rs.n_classes == 1 and rs.seed == ws.seed
    assert P.SynthStream(rs, dict(i_mean=0, i_std=1, q_mean=0, q_std=1), "rawiq", 4).take == 128
    with pytest.raises(P.IqError, match="no CPU fallback"):
        rs.generate(4)
    with pytest.raises(TypeError):
        rs.struct()
    with pytest.raises(ValueError):
        receiver_reference(np.zeros((1, 16, 3)), np.zeros((1, 5)), 4, "given")
    with pytest.raises(ValueError):
        receiver_reference(np.zeros((1, 16, 2)), np.zeros((1, 6)), 4, "given")
    with pytest.raises(ValueError):
        receiver_reference(np.zeros((1, 16, 2)), np.zeros((1, 5)), 4, "gardner")
    with pytest.raises(ValueError):
        receiver_reference(np.zeros((1, 16, 2)), np.zeros((1, 5)), 2, "oerder_meyr")
    with pytest.raises(ValueError):
        receiver_reference(np.zeros((2, 16, 2)), np.zeros((1, 5)), 4, "given", u=[0])
    with pytest.raises(ValueError):
        receiver_reference_bwd(np.zeros((1, 16, 2)), np.zeros((1, 3, 2)), np.zeros((1, 5)), 4)
    with pytest.raises(TypeError):
        transmitted_index("ws", 0, 0)
    # k0: q and u together span one symbol; sps 8, span 8: (u + q) / 256 + 3.5 rounded
    assert np.array_equal(transmitted_index(ws, [0, 31, 0, 16], [0, 0, 255, 128]), [4, 4, 4, 4])
    assert np.array_equal(transmitted_index(ws, [0, 31], [129, 224]), [4, 4])


E2E = {"a": dict(sps=8, span=8, alpha=0.35, n_phase=32, length=1024), "b": dict(sps=3, span=6, alpha=0.5, n_phase=8, length=384)}


@pytest.mark.parametrize("name", ["QPSK", "16QAM"])
@pytest.mark.parametrize("shape", ["a", "b"])
def test_definition_closes_the_loop_at_every_timing_phase(shape, name):
    """Host only: host_transmit (waveform._times in fp64) -> receiver_reference (Oerder-Meyr) -> the transmitted symbols.  Two
    frames per timing phase, seeds fixed here."""
    from vit_vs_raw_iq_amd import mf_table, receiver_reference
    from vit_vs_raw_iq_amd.data import constellation
    c = E2E[shape]
    sps, span, n_phase, length = c["sps"], c["span"], c["n_phase"], c["length"]
    pts = constellation(name)
    table = mf_table(c["alpha"], sps, span, n_phase)
    rng = np.random.default_rng({"a": 11, "b": 12}[shape] + len(name))
    n_sym = length // sps + span + 2
    frames, sent, qs = [], [], []
    for q in range(n_phase):
        for _ in range(2):
            idx = rng.integers(0, len(pts), n_sym)
            v = host_transmit(pts, idx, sps, span, c["alpha"], n_phase, q, length, theta=rng.uniform(0, 2 * np.pi))
            frames.append(np.stack([v.real, v.imag], axis=1))
            sent.append(pts[idx])
            qs.append(q)
    sym, est, _ = receiver_reference(np.stack(frames), table, sps, "oerder_meyr")
    n_out = length // sps
    worst_t, worst_e = 0.0, 0.0
    for i, q in enumerate(qs):
        dt = float(circular_distance(est[i, 0], true_instant(sps, span, n_phase, q), sps))
        k0 = int(np.rint((est[i, 1] / n_phase + q / n_phase) / sps + (span - 1) / 2.0))
        k = np.arange(span, n_out - span)
        e = evm(sent[i][k0 + k], complex_frames(sym[i])[k])
        worst_t, worst_e = max(worst_t, dt), max(worst_e, e)
    print(f"{shape} {name}: worst |t0 - true| {worst_t:.4f} samples (cap {T0_CAP}), worst EVM {worst_e:.4f} (cap {EVM_CAP})")
    assert worst_t <= T0_CAP and worst_e <= EVM_CAP
