"""Receiver for pulse-shaped frames on the device: matched filter, one timing estimate per frame, one sample per symbol.

waveform.ShapedSynth makes frames at `sps` samples per symbol; both model families were designed for one sample per symbol (the
format of RadioML and of synth.FrameSynth).  One HIP kernel (csrc/receiver.hip, iq_frames_receive) takes a batch of such frames
back: an interpolating matched filter from a table G [n_frac, sps * span + 1] (root-raised cosine by default), the energy of
the filtered frame at each of the `sps` sample phases (a sliding Toeplitz GEMM on the fp32 MFMA), a timing estimate from those
energies (Oerder-Meyr's closed form, or the strongest phase), the symbols at that instant, unit power.  The definition is
written out in include/iqvit.h.  iq_frames_receive_bwd is the adjoint with the timing held fixed: the receiver is differentiable
with respect to its input.  There is no CPU path; `receiver_reference` / `receiver_reference_bwd` are the host fp64 DEFINITIONS
the tests compare against.

  mf_table(alpha, sps, span, n_frac) -> fp32 [n_frac, sps * span + 1]
  Receiver(sps, span, alpha, n_frac, timing, normalise, table, device)   (raw (B, len, 2), u) -> (B, len // sps, 2)
  Receiver.for_synth(shaped, **kw)                                        sps, span, alpha, n_frac = n_phase of a ShapedSynth
  ReceivedSynth(shaped, receiver, equaliser=None, carrier=None)           a FrameSynth of length len // sps: goes into SynthStream
  receiver_reference(raw, table, sps, mode, u, normalise) -> sym, est, energy        receiver_reference_bwd(...) -> dx
  transmitted_index(shaped, q, u)                                         the transmitted symbol output 0 sits on
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from ._args import MAX_LENGTH, _flag, _index, _number
from .carrier import Carrier
from .equaliser import Equaliser
from .stage import DeviceTables, _host, integers, no_cpu, pack, stage_for
from .synth import FrameSynth
from .waveform import ShapedSynth, rrc_pulse

MAX_SPS, MAX_SPAN, MAX_FRAC = 16, 32, 64      # the limits of iq_frames_receive
MODES = ("given", "oerder_meyr", "energy")    # IQ_RX_GIVEN, IQ_RX_OERDER_MEYR, IQ_RX_ENERGY


def _shape3(sps, span, n_frac):
    return (_index(sps, "sps", 1, MAX_SPS), _index(span, "span", 1, MAX_SPAN), _index(n_frac, "n_frac", 1, MAX_FRAC))


def _mode(mode, sps):
    if mode not in MODES:
        raise ValueError(f"timing must be one of {MODES}, got {mode!r}")
    if mode == "oerder_meyr" and sps < 3:
        raise ValueError(f"timing 'oerder_meyr' needs sps >= 3 (the spectral line at the symbol rate), got sps = {sps}")
    return MODES.index(mode)


def mf_table(alpha, sps, span, n_frac):
    """fp32 [n_frac, J + 1], J = sps * span, h = J // 2: entry [f, j] = p((f / n_frac + h - j) / sps) / sqrt(sps), p the
    root-raised-cosine pulse of roll-off alpha in [0, 1] (waveform.rrc_pulse), zero where |argument| > span / 2; computed in fp64
    from an integer numerator over sps * n_frac (arguments that mirror each other are exact negatives: row 0 is symmetric when J
    is even), then rounded."""
    alpha = _number(alpha, "alpha")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], got {alpha!r}")
    sps, span, n_frac = _shape3(sps, span, n_frac)
    J = sps * span
    f = np.arange(n_frac, dtype=np.int64)[:, None]
    j = np.arange(J + 1, dtype=np.int64)[None, :]
    num = f + (J // 2 - j) * n_frac
    g = rrc_pulse(num.astype(np.float64) / float(sps * n_frac), alpha) / math.sqrt(sps)
    g[2 * np.abs(num) > span * sps * n_frac] = 0.0
    return g.astype(np.float32)


def _table(v, shape):
    try:
        t = np.asarray(v)
        if t.dtype.kind not in "fiu":
            raise TypeError
    except (TypeError, ValueError):
        raise TypeError(f"table must be an array of numbers, got {v!r}") from None
    if t.shape != shape:
        raise ValueError(f"table must have shape (n_frac, sps * span + 1) = {shape}, got {t.shape}")
    if not np.all(np.isfinite(t)):
        raise ValueError("table has a non-finite entry")
    return np.ascontiguousarray(t.astype(np.float32))


class Receiver(DeviceTables):
    """raw (B, len, 2) frames at `sps` samples per symbol -> (B, len // sps, 2) symbols.  span: matched-filter length in
    symbols; alpha: roll-off of its root-raised cosine; n_frac: fractional sampling phases in the table.  timing:
    'oerder_meyr' (the phase of the symbol-rate line of |y|^2: sps >= 3), 'energy' (the sample phase of most energy) or 'given'
    (the caller's u, in units of 1 / n_frac sample).  normalise: unit mean power per frame.  table=: a table of one's own,
    (n_frac, sps * span + 1).  Arguments are checked here, before any device work."""

    reference = "receiver_reference"

    def __init__(self, sps, span: int = 8, alpha: float = 0.35, n_frac: int = 32, timing: str = "oerder_meyr",
                 normalise: bool = True, table=None, device="cuda"):
        self.sps, self.span, self.n_frac = _shape3(sps, span, n_frac)
        self.alpha = _number(alpha, "alpha")
        self.timing = timing
        self.mode = _mode(timing, self.sps)
        self.normalise = _flag(normalise, "normalise")
        shape = (self.n_frac, self.sps * self.span + 1)
        self.table = mf_table(self.alpha, self.sps, self.span, self.n_frac) if table is None else _table(table, shape)
        self.device = torch.device(device)
        self._uploaded = {}

    @classmethod
    def for_synth(cls, shaped, **kw):
        """The receiver of a ShapedSynth's frames: its sps, span and alpha, n_frac = its n_phase, on its device."""
        if not isinstance(shaped, ShapedSynth):
            raise TypeError(f"shaped must be a ShapedSynth, got {type(shaped).__name__}")
        args = dict(sps=shaped.sps, span=shaped.span, alpha=shaped.alpha, n_frac=shaped.n_phase, device=shaped.device)
        args.update(kw)
        return cls(**args)

    def n_out(self, length):
        return length // self.sps

    def struct(self, table=None, u=None, mode=None) -> N.Receiver:
        """The iq_receiver_t of one call (`table`, `u`: device addresses)."""
        return N.Receiver(sps=self.sps, span=self.span, n_frac=self.n_frac, mode=self.mode if mode is None else mode,
                          normalise=int(self.normalise), table=table, u=u)

    def _check(self, raw, u):
        if not isinstance(raw, torch.Tensor) or raw.dim() != 3 or raw.shape[2] != 2:
            raise ValueError(f"raw must be a (B, len, 2) tensor, got {tuple(raw.shape) if hasattr(raw, 'shape') else raw!r}")
        if not self.sps <= raw.shape[1] <= MAX_LENGTH:
            raise ValueError(f"the frame length must be in [sps, {MAX_LENGTH}] = [{self.sps}, {MAX_LENGTH}], got {raw.shape[1]}")
        if u is not None:
            if self.mode != 0:
                raise ValueError(f"u is for timing='given', this receiver estimates it (timing={self.timing!r})")
            def in_range(arr):                   # (called before u is bound anew: u is still the caller's)
                if arr.size and (arr.min() < 0 or arr.max() >= self.sps * self.n_frac):
                    raise ValueError(f"u must be in [0, sps * n_frac) = [0, {self.sps * self.n_frac}), got {u!r}")
                return arr.astype(np.int32)
            u = integers(u, "u", (raw.shape[0],), raw.device, wrap=in_range)
        if not raw.is_cuda:
            raise no_cpu(self, "raw")
        return u

    def __call__(self, raw, u=None, return_est=False, return_energy=False):
        """raw: device (B, len, 2) fp32 -> sym (B, len // sps, 2) fp32 on the current stream, no host synchronisation;
        differentiable with respect to raw (the timing held fixed).  u: (B,) integers in [0, sps * n_frac), timing='given' only
        (None: 0); a host array is checked, a device tensor is not looked at (that would synchronise): the kernel reduces it
        modulo sps * n_frac.  Then, if asked for, est (B, 4) fp32 = {t0 in samples (NaN when given), u, |X| / sum E, mean |v|^2} and energy
        (B, sps) fp32."""
        return_est, return_energy = _flag(return_est, "return_est"), _flag(return_energy, "return_energy")
        u = self._check(raw, u)
        sym, est, energy = _ReceiveFn.apply(raw, self, u, return_est, return_energy)
        return pack(sym, est if return_est else None, energy)

    def __repr__(self):
        return (f"Receiver(sps={self.sps}, span={self.span}, alpha={self.alpha}, n_frac={self.n_frac}, timing={self.timing!r}, "
                f"normalise={self.normalise})")


class _ReceiveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, rx, u, want_est, want_energy):
        x = raw.contiguous().float()
        B, length = x.shape[0], x.shape[1]
        d = x.device
        grad = raw.requires_grad                      # (grad mode is off in here: the flag of the input says it)
        sym = torch.empty(B, length // rx.sps, 2, dtype=torch.float32, device=d)
        # the backward needs the forward's instant (est[:, 1], unless it was the caller's) and, normalised, its power (est[:, 3])
        est = torch.empty(B, 4, dtype=torch.float32, device=d) if want_est or (grad and (rx.mode != 0 or rx.normalise)) else None
        energy = torch.empty(B, rx.sps, dtype=torch.float32, device=d) if want_energy else None
        table = rx.table_on(d)
        if B > 0:
            par = rx.struct(table.data_ptr(), N.ptr(u))
            N.check(N.lib().iq_frames_receive(x.data_ptr(), sym.data_ptr(), N.ptr(est), N.ptr(energy), B, length, C.byref(par),
                                              torch.cuda.current_stream(d).cuda_stream), "iq_frames_receive")
        ctx.rx, ctx.u, ctx.table, ctx.length = rx, u, table, length
        ctx.save_for_backward(sym, est)
        ctx.mark_non_differentiable(*[t for t in (est, energy) if t is not None])
        return sym, est, energy

    @staticmethod
    def backward(ctx, dsym, _dest, _denergy):
        sym, est = ctx.saved_tensors
        rx = ctx.rx
        dsym = dsym.contiguous().float()
        B = dsym.shape[0]
        dx = torch.empty(B, ctx.length, 2, dtype=torch.float32, device=dsym.device)
        if B > 0:
            u = ctx.u if rx.mode == 0 else est[:, 1].to(torch.int32)     # the instant the forward chose, held fixed
            par = rx.struct(ctx.table.data_ptr(), N.ptr(u), mode=0)
            N.check(N.lib().iq_frames_receive_bwd(dsym.data_ptr(), sym.data_ptr(), N.ptr(est), dx.data_ptr(), B, ctx.length,
                                                  C.byref(par), torch.cuda.current_stream(dsym.device).cuda_stream),
                    "iq_frames_receive_bwd")
        return dx, None, None, None, None


class ReceivedSynth(FrameSynth):
    """A ShapedSynth seen through a Receiver: a FrameSynth whose frames are the received symbols, length = shaped.length // sps,
    labels, SNRs and keying those of `shaped`.  equaliser= (an equaliser.Equaliser) and carrier= (a carrier.Carrier), each of
    layout (B, length, 2) and of this length, then run on the symbols in that order.  Goes into SynthStream, train_on_stream,
    impair and evaluate_model_with_confusion as it is."""

    def __init__(self, shaped, receiver, equaliser=None, carrier=None):
        if not isinstance(shaped, ShapedSynth):
            raise TypeError(f"shaped must be a ShapedSynth, got {type(shaped).__name__}")
        if not isinstance(receiver, Receiver):
            raise TypeError(f"receiver must be a Receiver, got {type(receiver).__name__}")
        if receiver.sps != shaped.sps:
            raise ValueError(f"the receiver's sps ({receiver.sps}) is not the synth's ({shaped.sps})")
        if shaped.length < receiver.sps:
            raise ValueError(f"the synth's frames ({shaped.length} samples) are shorter than one symbol ({receiver.sps})")
        self.shaped, self.receiver = shaped, receiver
        self.class_names, self.descriptors, self.points = shaped.class_names, shaped.descriptors, shaped.points
        self.snrs_db, self.seed, self.balanced, self.device = shaped.snrs_db, shaped.seed, shaped.balanced, shaped.device
        self.length = receiver.n_out(shaped.length)
        for stage, cls, what in ((equaliser, Equaliser, "equaliser"), (carrier, Carrier, "carrier")):
            stage_for(stage, cls, what, False, self.length, "the receiver writes (B, length, 2) frames",
                      f"symbols, the receiver gives {self.length}")
        self.equaliser, self.carrier = equaliser, carrier

    def _stages(self, sym):
        if self.equaliser is not None:
            sym = self.equaliser(sym)
        return sym if self.carrier is None else self.carrier(sym)

    def struct(self, *args, **kw):
        raise TypeError("a ReceivedSynth has no iq_synth_t of its own: see .shaped.struct and .receiver.struct")

    def generate(self, n, frame_base=0, stream=0, return_est=False, **kw):
        """Frames [frame_base, frame_base + n) of `stream` of the ShapedSynth, received (then equalised, then derotated, where
        those stages were given) -> (sym (n, len // sps, 2) fp32, y, z), then what ShapedSynth.generate appends for its own
        keywords, then the receiver's est (n, 4) with return_est."""
        return_est = _flag(return_est, "return_est")
        raw, *rest = self.shaped.generate(n, frame_base, stream, **kw)
        if return_est:
            sym, est = self.receiver(raw, return_est=True)
            return (self._stages(sym), *rest, est)
        return (self._stages(self.receiver(raw)), *rest)

    def __repr__(self):
        more = "".join(f", {k}={v!r}" for k, v in (("equaliser", self.equaliser), ("carrier", self.carrier)) if v is not None)
        return f"ReceivedSynth({self.shaped!r}, {self.receiver!r}{more})"


def _windows(raw, table, sps):
    """-> x windows (B, len + 1, J + 1) complex128 with win[b, m, j] = x[m + j - h] (zero outside the frame), G fp64, J."""
    x = _host(raw).astype(np.float64)
    G = _host(table).astype(np.float64)
    sps = _index(sps, "sps", 1)
    if x.ndim != 3 or x.shape[2] != 2 or x.shape[1] < sps:
        raise ValueError(f"raw must be (B, len >= sps, 2), got {x.shape}")
    if G.ndim != 2 or G.shape[1] < 2 or (G.shape[1] - 1) % sps:
        raise ValueError(f"table must be (n_frac, sps * span + 1), got {G.shape}")
    J = G.shape[1] - 1
    h = J // 2
    z = x[:, :, 0] + 1j * x[:, :, 1]
    zp = np.pad(z, ((0, 0), (h, J - h + 1)))
    return np.lib.stride_tricks.sliding_window_view(zp, J + 1, axis=1), G, J


def _instants(u, B, period):
    u = np.zeros(B, np.int64) if u is None else _host(u).astype(np.int64).reshape(-1)
    if u.shape != (B,):
        raise ValueError(f"u must have shape ({B},), got {u.shape}")
    return u % period


def receiver_reference(raw, table, sps, mode, u=None, normalise=True):
    """The definition of include/iqvit.h in fp64 on the host, the fp32 table taken as given.  mode: 'given' (u: (B,) integers,
    None: 0), 'oerder_meyr' or 'energy'.  -> sym (B, len // sps, 2), est (B, 4), energy (B, sps), float64."""
    win, G, J = _windows(raw, table, sps)
    B, length, n_frac = win.shape[0], win.shape[1] - 1, G.shape[0]
    mode = _mode(mode, sps)
    n_out = length // sps
    energy = np.zeros((B, sps))
    for b in range(B):
        y = win[b, :length] @ G[0]
        p = y.real ** 2 + y.imag ** 2                               # (not |y|^2 through a square root: exact on integers)
        for r in range(sps):
            energy[b, r] = p[r::sps].sum()
    X = energy @ np.exp(-2j * np.pi * np.arange(sps) / sps)
    tot = energy.sum(axis=1)
    if mode == 0:
        t0 = np.full(B, np.nan)
        u = _instants(u, B, sps * n_frac)
    elif mode == 1:
        t0 = np.mod(-np.angle(X) * sps / (2.0 * np.pi), sps)
        u = np.where(np.isfinite(t0), np.rint(t0 * n_frac), 0.0).astype(np.int64) % (sps * n_frac)
    else:
        u = n_frac * np.argmax(energy, axis=1)
        t0 = (u // n_frac).astype(np.float64)
    sym = np.empty((B, n_out, 2))
    est = np.empty((B, 4))
    for b in range(B):
        rh, fh = int(u[b]) // n_frac, int(u[b]) % n_frac
        v = win[b, rh + sps * np.arange(n_out)] @ G[fh]
        mean = np.mean(v.real ** 2 + v.imag ** 2)
        if normalise:
            v = v / np.sqrt(mean + 1e-12)
        sym[b, :, 0], sym[b, :, 1] = v.real, v.imag
        with np.errstate(invalid="ignore", divide="ignore"):
            est[b] = (t0[b], u[b], 0.0 if tot[b] == 0 else np.abs(X[b]) / tot[b], mean)
    return sym, est, energy


def receiver_reference_bwd(raw, dsym, table, sps, u=None, normalise=True):
    """The analytic adjoint in fp64, the timing held at u ((B,) integers, None: 0): the gradient of sum(sym * dsym) with respect
    to raw, sym = receiver_reference(raw, table, sps, 'given', u, normalise)[0].  dsym: (B, len // sps, 2) -> (B, len, 2)."""
    win, G, J = _windows(raw, table, sps)
    B, length, n_frac = win.shape[0], win.shape[1] - 1, G.shape[0]
    n_out, h = length // sps, J // 2
    d = _host(dsym).astype(np.float64)
    if d.shape != (B, n_out, 2):
        raise ValueError(f"dsym must be {(B, n_out, 2)}, got {d.shape}")
    ds = d[:, :, 0] + 1j * d[:, :, 1]
    u = _instants(u, B, sps * n_frac)
    out = np.zeros((B, length, 2))
    for b in range(B):
        rh, fh = int(u[b]) // n_frac, int(u[b]) % n_frac
        dv = ds[b]
        if normalise:
            v = win[b, rh + sps * np.arange(n_out)] @ G[fh]
            rho = np.sqrt(np.mean(np.abs(v) ** 2) + 1e-12)
            s = v / rho
            dv = (dv - s * np.sum(dv.real * s.real + dv.imag * s.imag) / n_out) / rho
        dz = np.zeros(length + J + sps + 1, np.complex128)          # dz[n + h] collects dx[n]
        for k in range(n_out):
            dz[rh + k * sps:rh + k * sps + J + 1] += dv[k] * G[fh]
        out[b, :, 0], out[b, :, 1] = dz[h:h + length].real, dz[h:h + length].imag
    return out


def transmitted_index(shaped, q, u):
    """The index k0 of the transmitted symbol that output 0 of a receiver with n_frac = shaped.n_phase sits on, for frames of
    timing phase q received at instant u (arrays or tensors of equal shape): iq_frames_waveform puts symbol k at sample time
    (k - (span - 1) / 2) sps - q / n_phase, so k0 = rint((u / n_frac + q / n_phase) / sps + (span - 1) / 2).  -> int64 array."""
    if not isinstance(shaped, ShapedSynth):
        raise TypeError(f"shaped must be a ShapedSynth, got {type(shaped).__name__}")
    q, u = _host(q).astype(np.float64), _host(u).astype(np.float64)
    return np.rint((u + q) / (shaped.n_phase * shaped.sps) + (shaped.span - 1) / 2.0).astype(np.int64)
