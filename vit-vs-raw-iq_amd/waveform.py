"""Pulse-shaped labelled I/Q frames made on the device: FrameSynth at `sps` samples per symbol, behind a multipath channel.

synth.FrameSynth restates data.make_dataset: one sample per symbol, no pulse, so every class is spectrally white and the
spectrogram front end has nothing to look at.  Here one HIP kernel (csrc/waveform.hip, iq_frames_waveform) makes what an
over-the-air capture holds: symbols through a polyphase pulse filter (root-raised cosine by default), true OQPSK (the Q rail half
a symbol late), GMSK as continuous-phase modulation from a Gaussian phase-increment table, one timing phase per frame, and a
static Rician / Rayleigh multipath channel of up to 8 taps; then FrameSynth's carrier phase, unit power and AWGN.  The keying is
FrameSynth's (frame j of a stream is a pure function of (seed, stream, j); the counter layout is written out in include/iqvit.h),
and with sps = span = n_phase = 1, a pulse of 1.0, no timing and one tap the frames ARE FrameSynth's, bit for bit.

The tables are plain numbers to the kernel: `rrc_table` and `gmsk_table` fill them in fp64 here; pulse= / fpulse= take tables of
one's own.  There is no CPU path; `waveform_reference` is the host fp64 DEFINITION of the noiseless frame the tests compare
against.

  rrc_table(alpha, sps, span, n_phase) -> fp32 [n_phase, sps, span]     gmsk_table(bt, sps, span, n_phase) -> int32, same shape
  ShapedSynth(classes, snrs_db, length, seed, balanced, device, sps, span, alpha, bt, n_phase, timing, taps, rice_k_db, decay)
      a FrameSynth: .generate(n, frame_base, stream) -> (raw, y, z); .stats(); goes into SynthStream and train_on_stream as it is
  waveform_reference(symbols, drawn, taps, synth)                        host fp64, everything but the noise
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from . import data as D
from ._args import _flag, _index, _number
from .synth import KIND_GMSK, KIND_OQPSK, KIND_POINTS, FrameSynth

MAX_SPS, MAX_SPAN, MAX_PHASE, MAX_TAPS = 16, 32, 64, 8      # the limits of iq_frames_waveform


def _shape3(sps, span, n_phase):
    return (_index(n_phase, "n_phase", 1, MAX_PHASE), _index(sps, "sps", 1, MAX_SPS), _index(span, "span", 1, MAX_SPAN))


def _times(sps, span, n_phase):
    """t[q, r, i] = (span - 1) / 2 + (r + q / n_phase) / sps - i in symbol periods, from an integer numerator over 2 sps n_phase:
    times that mirror each other are exact negatives."""
    q = np.arange(n_phase, dtype=np.int64)[:, None, None]
    r = np.arange(sps, dtype=np.int64)[None, :, None]
    i = np.arange(span, dtype=np.int64)[None, None, :]
    num = (span - 1) * sps * n_phase + 2 * (r * n_phase + q) - 2 * i * sps * n_phase
    return num.astype(np.float64) / (2.0 * sps * n_phase)


def rrc_pulse(t, alpha):
    """The root-raised-cosine pulse of symbol period 1 and unit energy at times t (fp64), its removable singularities at t = 0
    and |t| = 1 / (4 alpha) filled with their limits.  Even in t by construction (it is evaluated at |t|)."""
    t = np.abs(np.asarray(t, dtype=np.float64))
    a = float(alpha)
    if a == 0.0:
        return np.sinc(t)
    out = np.empty_like(t)
    zero = t == 0.0
    edge = np.abs(4.0 * a * t - 1.0) < 1e-9
    rest = ~(zero | edge)
    out[zero] = 1.0 - a + 4.0 * a / np.pi
    out[edge] = a / np.sqrt(2.0) * ((1.0 + 2.0 / np.pi) * np.sin(np.pi / (4.0 * a)) + (1.0 - 2.0 / np.pi) * np.cos(np.pi / (4.0 * a)))
    x = t[rest]
    out[rest] = (np.sin(np.pi * x * (1.0 - a)) + 4.0 * a * x * np.cos(np.pi * x * (1.0 + a))) / (np.pi * x * (1.0 - (4.0 * a * x) ** 2))
    return out


def rrc_table(alpha, sps, span, n_phase):
    """fp32 [n_phase, sps, span]: entry [q, r, i] = p((span - 1) / 2 + (r + q / n_phase) / sps - i) / sqrt(sps), p the
    root-raised-cosine pulse of roll-off alpha in [0, 1]; computed in fp64, then rounded."""
    alpha = _number(alpha, "alpha")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], got {alpha!r}")
    n_phase, sps, span = _shape3(sps, span, n_phase)
    return (rrc_pulse(_times(sps, span, n_phase), alpha) / math.sqrt(sps)).astype(np.float32)


def gmsk_phase(t, bt):
    """F(t): the cumulative phase in turns of one bit of unit width through a Gaussian filter of bandwidth-time product bt,
    modulation index 1/2: F(-inf) = 0, F(+inf) = 1/4.  The frequency pulse is Phi((t + 1/2) / s) - Phi((t - 1/2) / s) with
    s = sqrt(ln 2) / (2 pi bt); its integral is H(t + 1/2) - H(t - 1/2), H(x) = x Phi(x / s) + s phi(x / s)."""
    t = np.asarray(t, dtype=np.float64)
    s = math.sqrt(math.log(2.0)) / (2.0 * math.pi * float(bt))
    erf = np.vectorize(math.erf, otypes=[np.float64])

    def H(x):
        return x * 0.5 * (1.0 + erf(x / (s * math.sqrt(2.0)))) + s * np.exp(-0.5 * (x / s) ** 2) / math.sqrt(2.0 * math.pi)
    return 0.25 * (H(t + 0.5) - H(t - 0.5))


def gmsk_table(bt, sps, span, n_phase):
    """int32 [n_phase, sps, span]: entry [q, r, i] = round(2^32 (F(t) - F(t - 1 / sps))) at the time t of rrc_table's entry: the
    phase a bit adds during that sample, in units of 2^-32 turn.  Every [q] slice sums to 2^30, a quarter turn per symbol, up to
    the rounding of its entries and the Gaussian tail outside the span."""
    bt = _number(bt, "bt")
    if not bt > 0.0:
        raise ValueError(f"bt must be positive, got {bt!r}")
    n_phase, sps, span = _shape3(sps, span, n_phase)
    t = _times(sps, span, n_phase)
    return np.rint(2.0 ** 32 * (gmsk_phase(t, bt) - gmsk_phase(t - 1.0 / sps, bt))).astype(np.int64).astype(np.int32)


def _table(v, what, dtype, shape):
    try:
        t = np.asarray(v)
        if t.dtype.kind not in "fiu":
            raise TypeError
    except (TypeError, ValueError):
        raise TypeError(f"{what} must be an array of numbers, got {v!r}") from None
    if t.shape != shape:
        raise ValueError(f"{what} must have shape (n_phase, sps, span) = {shape}, got {t.shape}")
    if dtype == np.float32:
        if not np.all(np.isfinite(t)):
            raise ValueError(f"{what} has a non-finite entry")
    elif t.dtype.kind == "f" and not np.array_equal(t, np.rint(t)) or t.min() < -2 ** 31 or t.max() >= 2 ** 31:
        raise ValueError(f"{what} must hold integers in [-2^31, 2^31)")
    return np.ascontiguousarray(t.astype(dtype))


class ShapedSynth(FrameSynth):
    """FrameSynth at `sps` samples per symbol.  classes, snrs_db, length, seed, balanced, device: as FrameSynth (constellations
    are shaped by `pulse`, 'GMSK' is CPM from `fpulse`, 'OQPSK' two offset rails shaped by `pulse`).  span: pulse length in
    symbols; alpha: roll-off of the root-raised cosine; bt: GMSK bandwidth-time product; n_phase: timing phases in the tables,
    one of which each frame draws when timing=True (q = 0 otherwise).  taps = L > 1 puts a static L-tap channel behind the
    shaping: power profile p_l = decay^l / sum, tap 0 Rician with K = 10^(rice_k_db / 10) (line of sight sqrt(p_0 K / (K + 1)),
    scatter sqrt(p_0 / (2 (K + 1))) per component), taps l >= 1 Rayleigh with sqrt(p_l / 2) per component, drawn per frame.
    pulse= / fpulse=: tables of one's own, (n_phase, sps, span).  Arguments are checked here, before any device work."""

    _drawn_columns = 8
    _no_cpu = ("ShapedSynth.generate runs on the MI355X only: there is no CPU fallback "
               "(waveform_reference is the host definition used by the tests)")

    def __init__(self, classes=D.CLASSES, snrs_db=D.SNRS_DB, length: int = 1024, seed: int = 0, balanced: bool = True,
                 device="cuda", sps: int = 8, span: int = 8, alpha: float = 0.35, bt: float = 0.3, n_phase: int = 32,
                 timing: bool = True, taps: int = 1, rice_k_db: float = 6.0, decay: float = 0.5, pulse=None, fpulse=None):
        super().__init__(classes, snrs_db, length, seed, balanced, device)
        self.n_phase, self.sps, self.span = _shape3(sps, span, n_phase)
        shape = (self.n_phase, self.sps, self.span)
        self.alpha, self.bt = _number(alpha, "alpha"), _number(bt, "bt")
        self.pulse = rrc_table(self.alpha, self.sps, self.span, self.n_phase) if pulse is None else _table(pulse, "pulse", np.float32, shape)
        self.fpulse = gmsk_table(self.bt, self.sps, self.span, self.n_phase) if fpulse is None else _table(fpulse, "fpulse", np.int32, shape)
        self.timing = _flag(timing, "timing")
        self.taps = _index(taps, "taps", 1, MAX_TAPS)
        self.rice_k_db, self.decay = _number(rice_k_db, "rice_k_db"), _number(decay, "decay")
        if not 0.0 < self.decay <= 1.0:
            raise ValueError(f"decay must be in (0, 1], got {self.decay!r}")
        if abs(self.rice_k_db) > 300.0:
            raise ValueError(f"rice_k_db must be within +-300 dB, got {self.rice_k_db!r}")
        k = 10.0 ** (self.rice_k_db / 10.0)
        p = np.power(self.decay, np.arange(self.taps, dtype=np.float64))
        p /= p.sum()
        self.los = math.sqrt(p[0] * k / (k + 1.0))
        self.tap_sigma = tuple([math.sqrt(p[0] / (2.0 * (k + 1.0)))] + [math.sqrt(v / 2.0) for v in p[1:]])
        self.n_symbols = (self.length + self.taps - 1 + self.sps) // self.sps + self.span      # NS of include/iqvit.h
        self._pulse_dev = self._fpulse_dev = None

    def struct(self, frame_base=0, stream=0, points=None, pulse=None, fpulse=None) -> N.Waveform:
        """The iq_waveform_t of one call (`points`, `pulse`, `fpulse`: the device addresses of the tables)."""
        sig = (C.c_float * 8)(*(list(self.tap_sigma) + [0.0] * (8 - self.taps)))
        return N.Waveform(points=points, classes=self._classes_c, n_classes=len(self.descriptors), snrs_db=self._snrs_c,
                          n_snrs=len(self.snrs_db), balanced=int(self.balanced), seed=self.seed,
                          stream=_index(stream, "stream", 0, 2 ** 32 - 1), frame_base=_index(frame_base, "frame_base", 0, 2 ** 64 - 1),
                          sps=self.sps, span=self.span, n_phase=self.n_phase, timing=int(self.timing), pulse=pulse, fpulse=fpulse,
                          n_taps=self.taps, los=self.los, tap_sigma=sig)

    def generate(self, n, frame_base=0, stream=0, return_drawn=False, return_symbols=False, return_taps=False):
        """Frames [frame_base, frame_base + n) of `stream` -> (raw (n, len, 2) fp32, y (n,) int64, z (n,) fp32 SNR in dB, NaN
        without noise), all on the device; then, if asked for, drawn (n, 8) fp32 = {class, snr_db, theta, mean |v|^2 before the
        normalisation, timing phase q, sum |h_l|^2, 0, 0}, symbols (n, n_symbols) int32 (constellation index; GMSK: the bit;
        OQPSK: 2 I + Q) and taps (n, 8, 2) fp32 (re, im), zeros beyond `taps`."""
        return self._generate(n, frame_base, stream, return_drawn, return_symbols, return_taps=return_taps)

    def _launch(self, par, n, raw, y, z, drawn, symbols, return_taps=False):
        d = self.device
        if self._pulse_dev is None:
            self._pulse_dev = torch.from_numpy(self.pulse).to(d)
            self._fpulse_dev = torch.from_numpy(self.fpulse).to(d)
        par.points, par.pulse, par.fpulse = self._points_ptr(), self._pulse_dev.data_ptr(), self._fpulse_dev.data_ptr()
        taps = torch.empty(n, 8, 2, dtype=torch.float32, device=d) if return_taps else None
        if n > 0:
            N.check(N.lib().iq_frames_waveform(raw.data_ptr(), y.data_ptr(), z.data_ptr(), N.ptr(drawn), N.ptr(symbols),
                                               N.ptr(taps), n, self.length, C.byref(par),
                                               torch.cuda.current_stream(d).cuda_stream), "iq_frames_waveform")
        return (taps,)

    def __repr__(self):
        return (f"ShapedSynth(classes={self.class_names!r}, snrs_db={self.snrs_db!r}, length={self.length}, seed={self.seed}, "
                f"balanced={self.balanced}, sps={self.sps}, span={self.span}, alpha={self.alpha}, bt={self.bt}, "
                f"n_phase={self.n_phase}, timing={self.timing}, taps={self.taps}, rice_k_db={self.rice_k_db}, decay={self.decay})")


def waveform_reference(symbols, drawn, taps, synth: ShapedSynth):
    """The noiseless frames in fp64 on the host, from the kernel's own `symbols` (n, n_symbols), `drawn` (n, 8; the class, theta
    and q columns are used) and `taps` (n, 8, 2), with the synth's fp32 / int32 tables: the shaped signal u as include/iqvit.h
    defines it (GMSK: integer phase mod 2^32, then exp(2 pi j PHI / 2^32)), v[n] = sum_l h_l u[n + L-1 - l], rotation by theta,
    division by sqrt(mean |v|^2 + 1e-12).  -> float64 array (n, len, 2)."""
    to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)   # noqa: E731
    if not isinstance(synth, ShapedSynth):
        raise TypeError(f"synth must be a ShapedSynth, got {type(synth).__name__}")
    sym = to_np(symbols).astype(np.int64)
    d = to_np(drawn).astype(np.float64)
    h = to_np(taps).astype(np.float64)
    length, L, sps, span, ns = synth.length, synth.taps, synth.sps, synth.span, synth.n_symbols
    if sym.ndim != 2 or sym.shape[1] < ns or d.shape != (len(sym), 8) or h.shape != (len(sym), 8, 2):
        raise ValueError(f"symbols must be (n, >= {ns}), drawn (n, 8) and taps (n, 8, 2), got {sym.shape}, {d.shape} and {h.shape}")
    table = synth.points[:, 0].astype(np.float64) + 1j * synth.points[:, 1].astype(np.float64)
    nu = length + L - 1
    n1 = np.arange(nu)
    m, r = n1 // sps, n1 % sps
    m2, r2 = (n1 + sps // 2) // sps, (n1 + sps // 2) % sps
    win = np.arange(span)[None, :]
    out = np.empty((len(sym), length, 2), np.float64)
    for i in range(len(sym)):
        k, q = int(d[i, 0]), int(d[i, 4])
        if not 0 <= k < synth.n_classes or k != d[i, 0]:
            raise ValueError(f"frame {i}: class {d[i, 0]!r} is not one of the {synth.n_classes} classes")
        if not 0 <= q < synth.n_phase or q != d[i, 4]:
            raise ValueError(f"frame {i}: timing phase {d[i, 4]!r} is not one of the {synth.n_phase} phases")
        kind, off, count = synth.descriptors[k]
        s = sym[i]
        if kind == KIND_POINTS:
            if s.min(initial=0) < 0 or s.max(initial=0) >= count:
                raise ValueError(f"frame {i}: symbol outside [0, {count}) of class {synth.class_names[k]!r}")
            P = synth.pulse[q].astype(np.float64)
            u = (table[off + s][m[:, None] + win] * P[r]).sum(axis=1)
        elif kind == KIND_OQPSK:
            if s.min(initial=0) < 0 or s.max(initial=0) > 3:
                raise ValueError(f"frame {i}: OQPSK symbol outside [0, 4)")
            P = synth.pulse[q].astype(np.float64)
            rail_i, rail_q = (2 * (s >> 1) - 1) / np.sqrt(2), (2 * (s & 1) - 1) / np.sqrt(2)
            u = (rail_i[m[:, None] + win] * P[r]).sum(axis=1) + 1j * (rail_q[m2[:, None] + win] * P[r2]).sum(axis=1)
        else:
            if s.min(initial=0) < 0 or s.max(initial=0) > 1:
                raise ValueError(f"frame {i}: GMSK bit outside {{0, 1}}")
            F = synth.fpulse[q].astype(np.int64)
            inc = ((2 * s - 1)[m[:, None] + win] * F[r]).sum(axis=1)
            phi = np.cumsum(inc) % 2 ** 32                      # |inc| < 32 * 2^31 and nu < 2^14: no int64 overflow
            phi = np.where(phi >= 2 ** 31, phi - 2 ** 32, phi)
            u = np.exp(2j * np.pi * phi.astype(np.float64) / 2.0 ** 32)
        if L > 1:
            hc = h[i, :L, 0] + 1j * h[i, :L, 1]
            v = sum(hc[l] * u[L - 1 - l:L - 1 - l + length] for l in range(L))
        else:
            v = u[:length]
        v = v * np.exp(1j * d[i, 2])
        v = v / np.sqrt(np.mean(np.abs(v) ** 2) + 1e-12)
        out[i, :, 0], out[i, :, 1] = v.real, v.imag
    return out
