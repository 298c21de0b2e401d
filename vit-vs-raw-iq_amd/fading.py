"""A fading channel on the device: tap gains that move with a Doppler spread, and a sample clock that drifts.

Every channel of waveform.ShapedSynth and impairments.impair is frozen for the length of a frame; the channel of RadioML 2018.01A
is not.  Here one HIP kernel (csrc/fading.hip, iq_frames_fade) passes raw (B, length_in, 2) frames through up to 8 taps, each the
sum of a line of sight and up to 32 scatterers with their own Doppler shifts (Clarke's model: shift = fd cos(arrival angle)), and
reads them at positions that advance by 1 + d 2^-32 samples per output sample through a windowed-sinc interpolator; then the
generators' tail (unit power, AWGN at a per-frame SNR).  Positions are int64 in units of 2^-32 sample and phases int32 in units of
2^-32 turn (the formulas and the counter layout are written out in include/iqvit.h); frame j of a stream is a pure function of
(seed, stream, j) and of its input.  There is no CPU path; `fading_reference` is the host fp64 DEFINITION of the noiseless output
the tests compare against.

  interp_table(K, n_frac, beta) -> fp32 [n_frac, K]      Kaiser-windowed sinc, rows sum to 1
  Fading(length_in, length_out, taps, rice_k_db, decay, delay, sinusoids, doppler, clock_ppm, start, timing, K, n_frac, normalise, interp)
      (raw, snr_db, seed, stream, frame_base) -> y (B, length_out, 2); .given(raw, paths, amps, clock); .margin(); .replace(**kw)
  fading_reference(raw, paths, amps, clock, fading)      host fp64, everything but the noise
  FadedSynth(shaped, fading)                             a ShapedSynth whose frames went through the channel
  fading_curve(predict, shaped, fading, kind, values, n, batch, stream) -> top-1 accuracy per value
"""
from __future__ import annotations

import copy
import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from ._args import MAX_LENGTH, _flag, _index, _number
from .waveform import MAX_TAPS, ShapedSynth

MAX_SINUSOIDS, MAX_K, MAX_FRAC = 32, 16, 256      # the limits of iq_frames_fade
SLOTS = (MAX_TAPS, MAX_SINUSOIDS + 1)              # the path table of a frame: [8][33]
KINDS = ("doppler", "clock_ppm", "rice_k_db")
_NO_CPU = ("{} runs on the MI355X only: there is no CPU fallback (fading_reference is the host definition used by the tests)")


def interp_table(K, n_frac, beta=8.0):
    """fp32 [n_frac, K]: entry [f, k] = sinc(t) w(t) / (the row's sum), t = k - (K - 1) // 2 - f / n_frac, w the Kaiser window of
    shape beta over |t| <= (K + 1) / 2; computed in fp64, then rounded.  Row f interpolates x at m + f / n_frac from
    x[m + k - (K - 1) // 2].  With an odd K row 0 is the unit spike; K = n_frac = 1 gives {1.0}."""
    K, n_frac = _index(K, "K", 1, MAX_K), _index(n_frac, "n_frac", 1, MAX_FRAC)
    beta = _number(beta, "beta")
    if beta < 0.0:
        raise ValueError(f"beta must be >= 0, got {beta!r}")
    k = np.arange(K, dtype=np.int64)[None, :]
    f = np.arange(n_frac, dtype=np.int64)[:, None]
    num = (k - (K - 1) // 2) * n_frac - f                                    # t from an integer numerator
    t = num.astype(np.float64) / n_frac
    w = np.i0(beta * np.sqrt(np.clip(1.0 - (2.0 * t / (K + 1)) ** 2, 0.0, None))) / np.i0(beta)
    h = np.where((num % n_frac == 0) & (num != 0), 0.0, np.sinc(t) * w)      # the zeros of the sinc, exactly
    return (h / h.sum(axis=1, keepdims=True)).astype(np.float32)


def _range(v, what):
    """a number or (lo, hi) -> (lo, hi)"""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what} must be a number or (lo, hi), got {v!r}")
        lo, hi = _number(v[0], f"{what} lo"), _number(v[1], f"{what} hi")
    else:
        lo = hi = _number(v, what)
    if lo > hi:
        raise ValueError(f"{what}: lo {lo!r} is above hi {hi!r}")
    return lo, hi


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _cis_pi(x):
    """cos(pi x) + j sin(pi x) in fp64 with the quarter turns taken out exactly (x = k / 2 + r, |r| <= 1 / 4, both exact for the x
    of e(p)): multiples of a quarter turn give exactly +-1 and 0, as sincospif does."""
    k = np.rint(2.0 * x)
    r = x - 0.5 * k
    return (np.cos(np.pi * r) + 1j * np.sin(np.pi * r)) * np.array([1, 1j, -1, -1j])[k.astype(np.int64) & 3]


class Fading:
    """The channel.  taps, rice_k_db, decay: the power profile of ShapedSynth (p_l = decay^l / sum, tap 0 Rician with K =
    10^(rice_k_db / 10), the rest Rayleigh; rice_k_db = inf: no scatter on tap 0), here per tap as a line of sight plus
    `sinusoids` scatterers of equal amplitude (0: line of sight only).  delay: per-tap delays in samples (default l for tap l),
    kept in units of 2^-16 sample.  doppler: the maximum Doppler shift in cycles per sample, a number or (lo, hi) drawn per
    frame; clock_ppm: the sample-clock offset in parts per million, likewise.  start: the position of output sample 0 in input
    samples (default: the largest delay, rounded up, plus the interpolator's reach to the left: no tap reads in front of the
    frame); timing: add a fractional start drawn per frame.  K, n_frac: the interpolator's size (interp: a table of one's own,
    (n_frac, K)).  normalise: unit mean power per frame.  Arguments are checked here, before any device work."""

    def __init__(self, length_in, length_out=None, taps: int = 1, rice_k_db: float = 6.0, decay: float = 0.5, delay=None,
                 sinusoids: int = 16, doppler=0.0, clock_ppm=0.0, start=None, timing: bool = False, K: int = 9, n_frac: int = 128,
                 normalise: bool = True, interp=None, beta: float = 8.0):
        self._kw = dict(length_in=length_in, length_out=length_out, taps=taps, rice_k_db=rice_k_db, decay=decay, delay=delay,
                        sinusoids=sinusoids, doppler=doppler, clock_ppm=clock_ppm, start=start, timing=timing, K=K, n_frac=n_frac,
                        normalise=normalise, interp=interp, beta=beta)
        self.length_in = _index(length_in, "length_in", 1, MAX_LENGTH)
        self.length_out = self.length_in if length_out is None else _index(length_out, "length_out", 1, MAX_LENGTH)
        self.taps = _index(taps, "taps", 1, MAX_TAPS)
        self.sinusoids = _index(sinusoids, "sinusoids", 0, MAX_SINUSOIDS)
        self.K, self.n_frac = _index(K, "K", 1, MAX_K), _index(n_frac, "n_frac", 1, MAX_FRAC)
        self.timing, self.normalise = _flag(timing, "timing"), _flag(normalise, "normalise")
        self.decay = _number(decay, "decay")
        if not 0.0 < self.decay <= 1.0:
            raise ValueError(f"decay must be in (0, 1], got {self.decay!r}")
        if isinstance(rice_k_db, float) and rice_k_db == math.inf:
            self.rice_k_db, frac_los = math.inf, 1.0
        else:
            self.rice_k_db = _number(rice_k_db, "rice_k_db")
            if abs(self.rice_k_db) > 300.0:
                raise ValueError(f"rice_k_db must be within +-300 dB or inf, got {self.rice_k_db!r}")
            k = 10.0 ** (self.rice_k_db / 10.0)
            frac_los = k / (k + 1.0)
        p = np.power(self.decay, np.arange(self.taps, dtype=np.float64))
        p /= p.sum()
        self.los = (math.sqrt(p[0] * frac_los),) + (0.0,) * (self.taps - 1)
        self.tap_sigma = (math.sqrt(p[0] * (1.0 - frac_los) / 2.0),) + tuple(math.sqrt(v / 2.0) for v in p[1:])
        if self.sinusoids == 0:
            self.tap_sigma = (0.0,) * self.taps                      # no scatterers: nothing carries that power
        if delay is None:
            delay = tuple(float(l) for l in range(self.taps))
        if isinstance(delay, (str, bytes)) or not hasattr(delay, "__len__"):
            raise TypeError(f"delay must be a sequence of {self.taps} numbers, got {delay!r}")
        if len(delay) != self.taps:
            raise ValueError(f"delay must have one entry per tap ({self.taps}), got {len(delay)}")
        self.delay = tuple(_number(v, "delay entry") for v in delay)
        if min(self.delay) < 0.0 or max(self.delay) >= 2 ** 15:
            raise ValueError(f"delays must be in [0, 32768) samples, got {self.delay!r}")
        self.delay_q16 = tuple(int(round(v * 65536.0)) for v in self.delay)
        self.doppler = _range(doppler, "doppler")
        if self.doppler[0] < 0.0 or self.doppler[1] > 0.5:
            raise ValueError(f"doppler must be in [0, 0.5] cycles per sample, got {doppler!r}")
        self.clock_ppm = _range(clock_ppm, "clock_ppm")
        if max(abs(v) for v in self.clock_ppm) > 4e5:
            raise ValueError(f"clock_ppm must be within +-400000, got {clock_ppm!r}")
        self.drift = tuple(int(round(v * 1e-6 * 2.0 ** 32)) for v in self.clock_ppm)      # d_lo, d_hi
        c = (self.K - 1) // 2
        self.start = (-(-max(self.delay_q16) // 65536) + c) if start is None else _index(start, "start", -2 ** 30, 2 ** 30)
        self.beta = _number(beta, "beta")
        if interp is None:
            self.interp = interp_table(self.K, self.n_frac, self.beta)
        else:
            try:
                t = np.asarray(interp)
                if t.dtype.kind not in "fiu":
                    raise TypeError
            except (TypeError, ValueError):
                raise TypeError(f"interp must be an array of numbers, got {interp!r}") from None
            if t.shape != (self.n_frac, self.K):
                raise ValueError(f"interp must have shape (n_frac, K) = {(self.n_frac, self.K)}, got {t.shape}")
            if not np.all(np.isfinite(t)):
                raise ValueError("interp has a non-finite entry")
            self.interp = np.ascontiguousarray(t.astype(np.float32))
        self._interp_dev = {}

    def replace(self, **kw):
        """A Fading with some arguments changed."""
        unknown = set(kw) - set(self._kw)
        if unknown:
            raise TypeError(f"unknown argument(s) {sorted(unknown)!r}")
        return Fading(**{**self._kw, **kw})

    def margin(self):
        """How many input samples beyond length_out the settings can reach: length_in >= length_out + margin() keeps every
        read inside the frame (delays only move reads to the left)."""
        last = self.start * 2 ** 32 + (2 ** 32 - 1 if self.timing else 0) + (self.length_out - 1) * (2 ** 32 + self.drift[1])
        return max(0, (last >> 32) + (self.K - 1 - (self.K - 1) // 2) + 1 - self.length_out)

    def struct(self, mode, interp=None, snr_db=None, paths=None, amps=None, clock=None, seed=0, stream=0, frame_base=0) -> N.Fading:
        """The iq_fading_t of one call (the pointers: device addresses)."""
        pad = lambda v, z: list(v) + [z] * (MAX_TAPS - self.taps)                          # noqa: E731
        return N.Fading(mode=mode, len_in=self.length_in, n_taps=self.taps, n_sin=self.sinusoids, K=self.K, n_frac=self.n_frac,
                        normalise=int(self.normalise), timing=int(self.timing), interp=interp, snr_db=snr_db, paths=paths, amps=amps,
                        clock=clock, delay=(C.c_int32 * 8)(*pad(self.delay_q16, 0)), los=(C.c_float * 8)(*pad(self.los, 0.0)),
                        tap_sigma=(C.c_float * 8)(*pad(self.tap_sigma, 0.0)), fd_lo=self.doppler[0], fd_hi=self.doppler[1],
                        d_lo=self.drift[0], d_hi=self.drift[1], start=self.start,
                        stream=_index(stream, "stream", 0, 2 ** 32 - 1), seed=_index(seed, "seed", 0, 2 ** 64 - 1),
                        frame_base=_index(frame_base, "frame_base", 0, 2 ** 64 - 1))

    def _check(self, raw, snr_db):
        if not isinstance(raw, torch.Tensor) or raw.dim() != 3 or raw.shape[2] != 2 or raw.shape[1] != self.length_in:
            raise ValueError(f"raw must be a (B, {self.length_in}, 2) tensor, got {tuple(raw.shape) if hasattr(raw, 'shape') else raw!r}")
        B = raw.shape[0]
        if snr_db is not None and not isinstance(snr_db, torch.Tensor):
            arr = np.asarray(snr_db, dtype=np.float64)
            if arr.ndim == 0:
                arr = np.full(B, float(arr))
            if arr.shape != (B,) or np.isinf(arr).any():
                raise ValueError(f"snr_db must be a number or ({B},) numbers (NaN: no noise), got {snr_db!r}")
            snr_db = torch.from_numpy(arr.astype(np.float32))
        if snr_db is not None and snr_db.shape != (B,):
            raise ValueError(f"snr_db must have shape ({B},), got {tuple(snr_db.shape)}")
        if not raw.is_cuda:
            raise N.IqError(_NO_CPU.format("Fading"))
        return None if snr_db is None else snr_db.to(device=raw.device, dtype=torch.float32).contiguous()

    def _run(self, mode, raw, snr_db, tables, want, seed, stream, frame_base):
        x = raw.contiguous().float()
        B, d = x.shape[0], x.device
        if d not in self._interp_dev:
            self._interp_dev[d] = torch.from_numpy(self.interp).to(d)
        y = torch.empty(B, self.length_out, 2, dtype=torch.float32, device=d)
        outs = (torch.empty((B,) + SLOTS + (2,), dtype=torch.int32, device=d), torch.empty((B,) + SLOTS, dtype=torch.float32, device=d),
                torch.empty(B, 2, dtype=torch.int64, device=d)) if want else (None, None, None)
        par = self.struct(mode, self._interp_dev[d].data_ptr(), N.ptr(snr_db), *(N.ptr(t) for t in tables), seed=seed, stream=stream,
                          frame_base=frame_base)
        if B > 0:
            N.check(N.lib().iq_frames_fade(x.data_ptr(), y.data_ptr(), *(N.ptr(t) for t in outs), B, self.length_out, C.byref(par),
                                           torch.cuda.current_stream(d).cuda_stream), "iq_frames_fade")
        return (y,) + outs if want else y

    def __call__(self, raw, snr_db=None, seed=0, stream=0, frame_base=0, return_tables=False):
        """raw: device (B, length_in, 2) fp32 -> y (B, length_out, 2) fp32 on the current stream, no host synchronisation: frame
        i is frame frame_base + i of `stream`, its clock and paths drawn from (seed, stream, frame_base + i).  snr_db: None, a
        number or (B,) values in dB, NaN for no noise on that frame.  With return_tables: (y, paths (B, 8, 33, 2) int32 =
        (phase, inc), amps (B, 8, 33) fp32, clock (B, 2) int64 = {T0, S}): what fading_reference reads."""
        want = _flag(return_tables, "return_tables")
        self.struct(1, seed=seed, stream=stream, frame_base=frame_base)      # the checks of the integers, before any device work
        snr_db = self._check(raw, snr_db)
        return self._run(1, raw, snr_db, (None, None, None), want, seed, stream, frame_base)

    def given(self, raw, paths, amps, clock, snr_db=None, seed=0, stream=0, frame_base=0):
        """The channel with everything given per frame: paths (B, 8, 33, 2) integers (phase, inc) in units of 2^-32 turn, amps
        (B, 8, 33), clock (B, 2) = {T0, S} in units of 2^-32 sample.  Only the noise is drawn.  -> y (B, length_out, 2)."""
        self.struct(0, seed=seed, stream=stream, frame_base=frame_base)
        B = raw.shape[0] if isinstance(raw, torch.Tensor) and raw.dim() == 3 else -1
        tabs = []
        for t, what, shape, dt in ((paths, "paths", SLOTS + (2,), torch.int32), (amps, "amps", SLOTS, torch.float32),
                                   (clock, "clock", (2,), torch.int64)):
            if not isinstance(t, torch.Tensor):
                try:
                    t = torch.from_numpy(np.ascontiguousarray(np.asarray(t)))
                except TypeError:
                    raise TypeError(f"{what} must be an array of numbers, got {t!r}") from None
            if B >= 0 and tuple(t.shape) != (B,) + shape:
                raise ValueError(f"{what} must have shape {(B,) + shape}, got {tuple(t.shape)}")
            if dt != torch.float32 and t.dtype.is_floating_point:
                raise TypeError(f"{what} must hold integers, got {t.dtype}")
            tabs.append((t, dt))
        snr_db = self._check(raw, snr_db)
        tabs = [t.to(device=raw.device, dtype=dt).contiguous() for t, dt in tabs]
        return self._run(0, raw, snr_db, tabs, False, seed, stream, frame_base)

    def __repr__(self):
        return (f"Fading(length_in={self.length_in}, length_out={self.length_out}, taps={self.taps}, rice_k_db={self.rice_k_db}, "
                f"decay={self.decay}, delay={self.delay!r}, sinusoids={self.sinusoids}, doppler={self.doppler!r}, "
                f"clock_ppm={self.clock_ppm!r}, start={self.start}, timing={self.timing}, K={self.K}, n_frac={self.n_frac}, "
                f"normalise={self.normalise})")


def fading_reference(raw, paths, amps, clock, fading: Fading):
    """The noiseless output in fp64 on the host from the tables a call used (return_tables) or was given: the integer positions
    and phases of include/iqvit.h (m = Q >> 32, f = ((Q mod 2^32) n_frac) >> 32; phase + n inc mod 2^32, converted as the kernel
    converts it: x = fp32((int32) p) 2^-31, then cos and sin of pi x in fp64, exact at the quarter turns), the fp32 interpolation table taken as given, the
    sums in fp64; division by sqrt(mean |y|^2 + 1e-12) when fading.normalise.  -> float64 array (B, length_out, 2)."""
    if not isinstance(fading, Fading):
        raise TypeError(f"fading must be a Fading, got {type(fading).__name__}")
    x = _host(raw).astype(np.float64)
    pt, am, ck = _host(paths).astype(np.int64), _host(amps).astype(np.float64), _host(clock).astype(np.int64)
    B = len(x)
    if x.shape != (B, fading.length_in, 2) or pt.shape != (B,) + SLOTS + (2,) or am.shape != (B,) + SLOTS or ck.shape != (B, 2):
        raise ValueError(f"raw must be (B, {fading.length_in}, 2), paths (B, 8, 33, 2), amps (B, 8, 33) and clock (B, 2), got "
                         f"{x.shape}, {pt.shape}, {am.shape} and {ck.shape}")
    K, nf, c, Lin = fading.K, fading.n_frac, (fading.K - 1) // 2, fading.length_in
    tab = fading.interp.astype(np.float64)
    n = np.arange(fading.length_out, dtype=np.int64)
    kk = np.arange(K, dtype=np.int64)[None, :]
    out = np.empty((B, fading.length_out, 2), np.float64)
    for i in range(B):
        z = x[i, :, 0] + 1j * x[i, :, 1]
        P = ck[i, 0] + n * ck[i, 1]
        y = np.zeros(fading.length_out, np.complex128)
        for l in range(fading.taps):
            Q = P - (fading.delay_q16[l] << 16)
            m, f = Q >> 32, ((Q & 0xFFFFFFFF) * nf) >> 32
            idx = m[:, None] + kk - c
            ok = (idx >= 0) & (idx < Lin)
            r = (np.where(ok, z[np.clip(idx, 0, Lin - 1)], 0.0) * tab[f]).sum(axis=1)
            g = np.zeros(fading.length_out, np.complex128)
            for s in range(fading.sinusoids + 1):
                if am[i, l, s] == 0.0:
                    continue
                p = (pt[i, l, s, 0] + n * pt[i, l, s, 1]) & 0xFFFFFFFF
                p = np.where(p >= 2 ** 31, p - 2 ** 32, p)
                xx = p.astype(np.float32).astype(np.float64) * 2.0 ** -31
                g += am[i, l, s] * _cis_pi(xx)
            y += g * r
        if fading.normalise:
            y = y / np.sqrt(np.mean(np.abs(y) ** 2) + 1e-12)
        out[i, :, 0], out[i, :, 1] = y.real, y.imag
    return out


class FadedSynth(ShapedSynth):
    """A ShapedSynth seen through a Fading: the frames of `shaped`, made without noise at fading.length_in samples, then faded,
    with the noise added behind the channel at the SNR of the balanced pattern (frame j: index (j // K) % n_snrs, as the
    generators).  length = fading.length_out; labels, classes, keying, sps and span are those of `shaped`, so ReceivedSynth,
    SynthStream, train_on_stream, impair and the front ends take it as it is.  balanced=False is refused: that SNR draw lives
    inside the generator's kernel."""

    _no_cpu = _NO_CPU.format("FadedSynth.generate")

    def __init__(self, shaped, fading):
        if not isinstance(shaped, ShapedSynth) or isinstance(shaped, FadedSynth):
            raise TypeError(f"shaped must be a ShapedSynth, got {type(shaped).__name__}")
        if not isinstance(fading, Fading):
            raise TypeError(f"fading must be a Fading, got {type(fading).__name__}")
        if not shaped.balanced:
            raise ValueError("FadedSynth needs a balanced ShapedSynth: with balanced=False the SNR of a frame is drawn inside "
                             "iq_frames_waveform, and the noise has to come after the channel")
        self.__dict__.update(shaped.__dict__)
        self.shaped, self.fading = shaped, fading
        clean = copy.copy(shaped)                        # the same tables and device copies; no noise, the channel's input length
        clean.snrs_db, clean._snrs_c = (), (C.c_float * 1)()
        clean.length = fading.length_in
        clean.n_symbols = (clean.length + clean.taps - 1 + clean.sps) // clean.sps + clean.span
        clean._no_cpu = self._no_cpu
        self._clean = clean
        self.length, self.n_symbols = fading.length_out, clean.n_symbols
        self._snrs_dev = None

    def struct(self, *args, **kw):
        raise TypeError("a FadedSynth has no iq_waveform_t of its own: see .shaped.struct and .fading.struct")

    def generate(self, n, frame_base=0, stream=0, return_tables=False, **kw):
        """Frames [frame_base, frame_base + n) of `stream` -> (raw (n, length_out, 2) fp32, y, z), then what ShapedSynth.generate
        appends for its own keywords (describing the frame in front of the channel), then paths, amps, clock with return_tables."""
        want = _flag(return_tables, "return_tables")
        n = _index(n, "n", 0, 2 ** 31 - 1)
        base = _index(frame_base, "frame_base", 0, 2 ** 63 - 1 - n)
        clean, y, z, *rest = self._clean.generate(n, base, stream, **kw)
        if self.snrs_db:
            if self._snrs_dev is None:
                self._snrs_dev = torch.tensor(self.snrs_db, dtype=torch.float32, device=self.device)
            j = torch.arange(base, base + n, dtype=torch.int64, device=self.device)
            z = self._snrs_dev[(j // self.n_classes) % len(self.snrs_db)]
        res = self.fading(clean, z if self.snrs_db else None, self.seed, stream, base, return_tables=want)
        return ((res[0], y, z, *rest) + tuple(res[1:])) if want else (res, y, z, *rest)

    def __repr__(self):
        return f"FadedSynth({self.shaped!r}, {self.fading!r})"


def fading_curve(predict, shaped, fading, kind, values, n=4096, batch=512, stream=1):
    """Top-1 accuracy of `predict` (device raw frames (B, length_out, 2) -> class indices (B,)) on frames 0 .. n-1 of `stream`
    of FadedSynth(shaped, fading.replace(kind=value)) for each value; kind: 'doppler' (cycles per sample), 'clock_ppm' or
    'rice_k_db'.  The frames are keyed by their index, so the result does not depend on `batch`; one host synchronisation per
    value.  -> a list of floats."""
    if not callable(predict):
        raise TypeError(f"predict must be callable, got {predict!r}")
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS!r}, got {kind!r}")
    if not isinstance(fading, Fading):
        raise TypeError(f"fading must be a Fading, got {type(fading).__name__}")
    n, batch = _index(n, "n", 1, 2 ** 31 - 1), _index(batch, "batch", 1, 2 ** 31 - 1)
    stream = _index(stream, "stream", 0, 2 ** 32 - 1)
    try:
        values = list(values)
    except TypeError:
        raise TypeError(f"values must be a sequence, got {values!r}") from None
    if not values:
        raise ValueError("values is empty")
    synths = [FadedSynth(shaped, fading.replace(**{kind: v})) for v in values]             # every value checked before any work
    out = []
    for fs in synths:
        hits = torch.zeros((), dtype=torch.int64, device=fs.device)
        for base in range(0, n, batch):
            raw, y, _ = fs.generate(min(batch, n - base), base, stream)
            hits += (predict(raw).reshape(-1).to(torch.int64) == y).sum()
        out.append(hits.item() / n)
    return out
