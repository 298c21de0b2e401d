"""Host statements the receiver tests share: independent restatements of vit_vs_raw_iq_amd.receiver's fp64 definitions, a host
transmitter (the `_times` formula of waveform.py in fp64, no device), the error measures and the error bound of the kernel.

None of this calls the product's definition: `matched_filter_by_convolution` goes through numpy.convolve, `torch_receive`
through torch in fp64 (for autograd), `host_transmit` through waveform.rrc_pulse at waveform._times.
"""
import math

import numpy as np
import torch

EPS = 2.0 ** -24          # unit roundoff of fp32
# The caps of the end-to-end property, host and device (conditions, not measurements): the Oerder-Meyr t0 within 0.1 sample
# (circular) of the true instant; interior symbols at an error-vector magnitude of at most 0.03 after one complex gain.
T0_CAP, EVM_CAP = 0.1, 0.03


def matched_filter_by_convolution(x, table, sps, u):
    """x: complex (len,); table (n_frac, J + 1) -> (E (sps,), v (len // sps,)) at instant u, by another route than the
    definition's windows: the frame zero-stuffed to n_frac samples per sample, convolved with the taps of all rows interleaved
    into one filter at that rate, then decimated.  y(m + f / n_frac) = sum_j x[m + j - h] G[f][j]: with the fine filter
    c[(J - j) n_frac + f] = G[f][j], sample m n_frac + f of the fine convolution of the stuffed frame, delayed by (J - h) n_frac."""
    G = np.asarray(table, np.float64)
    n_frac, J = G.shape[0], G.shape[1] - 1
    h = J // 2
    length = len(x)
    stuffed = np.zeros(length * n_frac, np.complex128)
    stuffed[::n_frac] = x
    c = np.zeros((J + 1) * n_frac)
    for f in range(n_frac):
        c[(J - np.arange(J + 1)) * n_frac + f] = G[f]
    fine = np.convolve(stuffed, c)                                   # fine[(m + J - h) n_frac + f] = y(m + f / n_frac)
    y0 = np.convolve(x, G[0][::-1])[J - h:J - h + length]            # row 0 alone at the sample rate
    E = np.array([np.sum(np.abs(y0[r::sps]) ** 2) for r in range(sps)])
    n_out = length // sps
    idx = (np.arange(n_out) * sps + J - h) * n_frac + u
    return E, fine[idx]


def torch_receive(raw, table, sps, u, normalise):
    """fp64 torch restatement of GIVEN mode for autograd: raw (B, len, 2) tensor requiring grad -> sym (B, len // sps, 2)."""
    G = torch.as_tensor(np.asarray(table, np.float64))
    n_frac, J = G.shape[0], G.shape[1] - 1
    h = J // 2
    B, length = raw.shape[0], raw.shape[1]
    n_out = length // sps
    out = []
    for b in range(B):
        rh, fh = int(u[b]) // n_frac, int(u[b]) % n_frac
        xp = torch.nn.functional.pad(raw[b].T, (h, J - h + sps))     # (2, len + J + sps)
        win = xp.unfold(1, J + 1, 1)                                 # win[c, m, j] = x_c[m + j - h]
        v = win[:, rh + sps * torch.arange(n_out)] @ G[fh]           # (2, n_out)
        if normalise:
            v = v / torch.sqrt((v ** 2).sum() / n_out + 1e-12)
        out.append(v.T)
    return torch.stack(out)


def host_transmit(points, idx, sps, span, alpha, n_phase, q, length, theta=0.0):
    """The noiseless one-tap frame of a kind-0 class in fp64: symbols points[idx] through the root-raised cosine at the times
    of waveform._times, rotated by theta, divided by sqrt(mean |v|^2 + 1e-12).  idx: (>= length // sps + span + 1,) -> complex
    (length,)."""
    from vit_vs_raw_iq_amd.waveform import _times, rrc_pulse
    P = rrc_pulse(_times(sps, span, n_phase), alpha)[q] / math.sqrt(sps)           # (sps, span) fp64
    a = np.asarray(points, np.complex128)[np.asarray(idx)]
    n = np.arange(length)
    m, r = n // sps, n % sps
    v = (a[m[:, None] + np.arange(span)[None, :]] * P[r]).sum(axis=1) * np.exp(1j * theta)
    return v / np.sqrt(np.mean(np.abs(v) ** 2) + 1e-12)


def true_instant(sps, span, n_phase, q):
    """Symbol k sits at sample time (k - (span - 1) / 2) sps - q / n_phase: the instant modulo one symbol."""
    return (-(span - 1) / 2.0 * sps - q / float(n_phase)) % sps


def circular_distance(a, b, period):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % period
    return np.minimum(d, period - d)


def evm(sent, got):
    """Error-vector magnitude of `got` against `sent` (complex arrays) after removing the one complex gain that fits best."""
    g = np.vdot(sent, got) / np.vdot(sent, sent)
    return float(np.sqrt(np.sum(np.abs(got - g * sent) ** 2) / np.sum(np.abs(g * sent) ** 2)))


def complex_frames(a):
    a = np.asarray(a, np.float64)
    return a[..., 0] + 1j * a[..., 1]


def abs_windows(raw, table, sps, u):
    """sum_j |x_j| |G_j| of every symbol's dot product, per component: (B, n_out, 2).  raw (B, len, 2), u (B,)."""
    x = np.abs(np.asarray(raw, np.float64))
    G = np.abs(np.asarray(table, np.float64))
    n_frac, J = G.shape[0], G.shape[1] - 1
    h = J // 2
    B, length = x.shape[0], x.shape[1]
    n_out = length // sps
    out = np.empty((B, n_out, 2))
    for b in range(B):
        rh, fh = int(u[b]) // n_frac, int(u[b]) % n_frac
        xp = np.pad(x[b], ((h, J - h + sps), (0, 0)))
        win = np.lib.stride_tricks.sliding_window_view(xp, J + 1, axis=0)          # (m, 2, J + 1)
        out[b] = win[rh + sps * np.arange(n_out)] @ G[fh]
    return out


def dot_bound(n_terms, abs_sum):
    """The issue's bound on an fp32 dot product of n_terms = J + 1 terms against fp64: 2 (J + 3) 2^-24 sum |x_j| |G_j|."""
    return 2.0 * (n_terms + 2) * EPS * abs_sum
