"""Carrier recovery on the device: a blind frequency and phase estimate per frame, and the derotation.

The transmitters turn every frame by a carrier phase drawn from U[0, 2 pi) and impairments.impair adds a phase and a frequency
offset; receiver.Receiver recovers symbol timing only, so a constellation image shows points turned by an arbitrary angle and,
under any frequency offset, rings.  One HIP kernel (csrc/carrier.hip, iq_frames_carrier) takes the offset out again by the
classic blind method: raise the frame to the M-th power, which removes M-PSK / QAM modulation and leaves a spectral line at
M f; find that line in a zero-padded periodogram of N = n1 * n2 points (a two-stage pair of small DFT GEMMs on the fp32 MFMA);
refine it by a parabola through the peak and its neighbours; read the phase at that frequency; derotate.  The definition is
written out in include/iqvit.h.  iq_frames_carrier_bwd is the adjoint with the estimate held fixed: the stage is differentiable
with respect to its input.  There is no CPU path; `carrier_reference` / `carrier_reference_bwd` are the host fp64 DEFINITIONS
the tests compare against.

What remains after it: the M-fold ambiguity (the output is the constellation turned by an unknown multiple of 2 pi / M) and the
constellation's own M-th-power angle (a diagonal QPSK comes out on the axes).  Threshold (host reference, M = 4 for QPSK and
16QAM, M = 2 for BPSK): locks at >= 10 dB, fails at 0 dB; 8PSK with M = 8 needs about 20 dB at 1024 symbols.

  dft_tables(n1, n2) -> (t1 [2, n1, n1], t2 [2, n2, n2], tw [2, n1 * n2]) fp32
  dft_factors(n_dft) -> (n1, n2)                     default_n_dft(length) -> N
  Carrier(length, order, n_dft, f_max, refine, layout, tables, device)      carrier(x, fth) -> out [, est, fth, power]
  Synchronised(front, carrier, equaliser=None)                             a FrontEnd: front(carrier(x)), or front(carrier(
                                                                           equaliser(x))); goes where spectrogram= does
  carrier_reference(x, tables, order, ...) -> out, est, fth, power         carrier_reference_bwd(dout, fth, planar) -> dx

For the `rawiq` layout there is receiver.ReceivedSynth(shaped, receiver, equaliser=, carrier=), a FrameSynth whose frames have
passed through the stages.  Not here: choosing M per frame, and decision-directed tracking.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from ._args import MAX_LENGTH, _flag, _index, _number
from .equaliser import Equaliser
from .frontend import FrontEnd
from .stage import Stage, _frames, _HeldFn, _host, _unframes, integers, no_cpu, pack, stage_for

ORDERS = (1, 2, 4, 8)
LAYOUTS = ("interleaved", "planar")          # iq_carrier_t.planar = 0, 1
MIN_FACTOR, MAX_FACTOR, FACTOR_STEP, MAX_DFT = 32, 256, 32, 8192


def _factor(v, what):
    v = _index(v, what, MIN_FACTOR, MAX_FACTOR)
    if v % FACTOR_STEP:
        raise ValueError(f"{what} must be a multiple of {FACTOR_STEP} in [{MIN_FACTOR}, {MAX_FACTOR}], got {v}")
    return v


def dft_factors(n_dft):
    """(n1, n2) with n1 * n2 = n_dft, each a multiple of 32 in [32, 256], n1 >= n2, of the smallest n1 + n2 (the work of the
    two stages is n_dft * (n1 + n2) complex products)."""
    n_dft = _index(n_dft, "n_dft", 1)
    best = None
    for n2 in range(MIN_FACTOR, MAX_FACTOR + 1, FACTOR_STEP):
        n1, r = divmod(n_dft, n2)
        if r == 0 and n2 <= n1 <= MAX_FACTOR and n1 % FACTOR_STEP == 0 and (best is None or n1 + n2 < sum(best)):
            best = (n1, n2)
    if best is None or n_dft > MAX_DFT:
        raise ValueError(f"n_dft must be n1 * n2 <= {MAX_DFT} with n1 and n2 multiples of {FACTOR_STEP} in [{MIN_FACTOR}, "
                         f"{MAX_FACTOR}] (1024 * j, j = 1 .. 8), got {n_dft}")
    return best


def default_n_dft(length):
    """The smallest allowed N >= 2 * length, capped at 8192 (padding by 2 cut the refined estimate's residual drift over the
    frame tenfold on the host reference, from 0.05 - 0.10 to 0.005 - 0.01 cycle)."""
    length = _index(length, "length", 1, MAX_LENGTH)
    return min(MAX_DFT, 1024 * -(-2 * length // 1024))


def dft_tables(n1, n2, dtype=np.float32):
    """(t1, t2, tw) fp32 (dtype=numpy.float64: before the rounding): t[0][m][k] = cos(2 pi m k / n), t[1][m][k] =
    sin(2 pi m k / n) for n = n1 and n2, tw[0][i] = cos(2 pi i / N), tw[1][i] = sin(2 pi i / N), N = n1 * n2; computed in fp64
    from the integer numerator reduced modulo n (the zeros are exact), then rounded."""
    n1, n2 = _factor(n1, "n1"), _factor(n2, "n2")

    def cs(num, n):
        num = num % n
        c, s = np.cos(2.0 * np.pi * num / n), np.sin(2.0 * np.pi * num / n)
        c[(4 * num) % (2 * n) == n] = 0.0                       # quarter turns: exact zeros
        s[(2 * num) % n == 0] = 0.0
        return np.stack([c, s]).astype(dtype)

    def square(n):
        i = np.arange(n, dtype=np.int64)
        return cs(i[:, None] * i[None, :], n)

    return square(n1), square(n2), cs(np.arange(n1 * n2, dtype=np.int64), n1 * n2)


def _tables(tables, n1, n2):
    if tables is None:
        return dft_tables(n1, n2)
    try:
        t1, t2, tw = (np.asarray(t) for t in tables)
        if any(t.dtype.kind not in "fiu" for t in (t1, t2, tw)):
            raise TypeError
    except (TypeError, ValueError):
        raise TypeError("tables must be three arrays of numbers (t1, t2, tw)") from None
    for t, shape, what in ((t1, (2, n1, n1), "t1"), (t2, (2, n2, n2), "t2"), (tw, (2, n1 * n2), "tw")):
        if t.shape != shape:
            raise ValueError(f"{what} must have shape {shape}, got {t.shape}")
        if not np.all(np.isfinite(t)):
            raise ValueError(f"{what} has a non-finite entry")
    return tuple(np.ascontiguousarray(t.astype(np.float32)) for t in (t1, t2, tw))


def _order(order):
    order = _index(order, "order", 1)
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order}")
    return order


def _phases(arr):
    if arr.size and (arr.min() < -2 ** 31 or arr.max() >= 2 ** 32):
        raise ValueError("fth holds 32-bit phases (units of 2^-32 turn): an entry is out of range")
    return (arr.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


class Carrier(Stage):
    """Frames of `length` samples -> the same frames with the carrier taken out.  order: M, the power that removes the
    modulation (2: BPSK, 4: QPSK and square QAM, 8: 8PSK; 1: a plain tone).  n_dft: the periodogram's size N >= length, an int
    (1024 * j, split by dft_factors) or a pair (n1, n2); None: default_n_dft(length).  f_max: the largest |frequency offset|
    searched, in cycles per sample (None: all of +- 1 / (2 M)); k_max = min(floor(f_max * M * N), N / 2).  refine: parabolic
    interpolation of the peak.  layout: 'planar' (B, 2, length), what the image front ends read, or 'interleaved'
    (B, length, 2), what the generators and the receiver write.  tables=: (t1, t2, tw) of one's own (dft_tables' shapes).
    Arguments are checked here, before any device work."""

    LAYOUTS, reference = LAYOUTS, "carrier_reference"

    def __init__(self, length, order: int = 4, n_dft=None, f_max=None, refine: bool = True, layout: str = "planar", tables=None,
                 device="cuda"):
        super().__init__(length, layout)
        self.order = _order(order)
        if n_dft is None:
            n_dft = default_n_dft(self.length)
        if isinstance(n_dft, (tuple, list)):
            if len(n_dft) != 2:
                raise ValueError(f"n_dft must be an integer or a pair (n1, n2), got {n_dft!r}")
            self.n1, self.n2 = _factor(n_dft[0], "n1"), _factor(n_dft[1], "n2")
            if self.n1 * self.n2 > MAX_DFT:
                raise ValueError(f"n1 * n2 must be <= {MAX_DFT}, got {self.n1 * self.n2}")
        else:
            self.n1, self.n2 = dft_factors(n_dft)
        self.n_dft = self.n1 * self.n2
        if self.n_dft < self.length:
            raise ValueError(f"n_dft ({self.n_dft}) must be >= length ({self.length})")
        if f_max is None:
            self.f_max, self.k_max = None, self.n_dft // 2
        else:
            self.f_max = _number(f_max, "f_max")
            if self.f_max < 0:
                raise ValueError(f"f_max must be >= 0, got {f_max!r}")
            self.k_max = min(int(math.floor(self.f_max * self.order * self.n_dft)), self.n_dft // 2)
        self.refine = _flag(refine, "refine")
        self.t1, self.t2, self.tw = _tables(tables, self.n1, self.n2)
        self.device = torch.device(device)

    def tables_on(self, device):
        """(t1, t2, tw) as fp32 tensors on `device`, uploaded once per device."""
        return self.table_on(device, ("t1", "t2", "tw"))

    def struct(self, tables=(None, None, None), fth=None, mode=1) -> N.Carrier:
        """The iq_carrier_t of one call (`tables`, `fth`: device addresses)."""
        return N.Carrier(order=self.order, n1=self.n1, n2=self.n2, k_max=self.k_max, refine=int(self.refine), planar=self.planar,
                         mode=mode, t1=tables[0], t2=tables[1], tw=tables[2], fth=fth)

    def __call__(self, x, fth=None, return_est=False, return_fth=False, return_power=False):
        """x: device frames in this carrier's layout, fp32 -> out of the same shape on the current stream, no host
        synchronisation; differentiable with respect to x (the estimate held fixed).  fth: (B, 2) integers (F, TH) in units of
        2^-32 cycle per sample / turn: nothing is estimated, out = x turned back by them.  Then, if asked for, est (B, 4) fp32 =
        {F in cycles per sample, TH in radians, peak bin s^ + d of the M-th power, lock quality in [0, 1]}, fth (B, 2) int32
        and power (B, N) fp32 (not with fth=)."""
        return_est, return_fth = _flag(return_est, "return_est"), _flag(return_fth, "return_fth")
        return_power = _flag(return_power, "return_power")
        if return_power and fth is not None:
            raise ValueError("return_power needs the estimate: it is not computed with fth=")
        self._check_shape(x)
        if fth is not None:
            fth = integers(fth, "fth", (x.shape[0], 2), x.device, " = (F, TH) per frame", _phases)
        if not x.is_cuda:
            raise no_cpu(self)
        out, fth_out, est, power = _HeldFn.apply(x, self, fth, return_est, return_power)
        return pack(out, est, fth_out if return_fth else None, power)

    def _forward(self, x, fth, want_est, want_power):
        B, d = x.shape[0], x.device
        out = torch.empty_like(x)
        est = torch.empty(B, 4, dtype=torch.float32, device=d) if want_est else None
        fth_out = torch.empty(B, 2, dtype=torch.int32, device=d)         # the backward's (F, TH), held fixed
        power = torch.empty(B, self.n_dft, dtype=torch.float32, device=d) if want_power else None
        if B > 0:
            if fth is None:
                t1, t2, tw = self.table_on(d, ("t1", "t2", "tw"))
                par = self.struct((t1.data_ptr(), t2.data_ptr(), tw.data_ptr()))
            else:
                par = self.struct(fth=fth.data_ptr(), mode=0)
            N.check(N.lib().iq_frames_carrier(x.data_ptr(), out.data_ptr(), N.ptr(est), fth_out.data_ptr(), N.ptr(power), B,
                                              self.length, C.byref(par), torch.cuda.current_stream(d).cuda_stream),
                    "iq_frames_carrier")
        return out, fth_out, (est, power)

    def _backward(self, dout, dx, fth, B):
        par = self.struct(fth=fth.data_ptr(), mode=0)
        N.check(N.lib().iq_frames_carrier_bwd(dout.data_ptr(), dx.data_ptr(), B, self.length, C.byref(par),
                                              torch.cuda.current_stream(dout.device).cuda_stream), "iq_frames_carrier_bwd")

    def __repr__(self):
        return (f"Carrier(length={self.length}, order={self.order}, n_dft=({self.n1}, {self.n2}), f_max={self.f_max}, "
                f"refine={self.refine}, layout={self.layout!r})")


class Synchronised(FrontEnd):
    """An image front end behind a carrier recovery: `front(carrier(x))`, a FrontEnd itself, so it goes wherever `spectrogram=`
    is accepted.  With equaliser= the blind equaliser runs first: `front(carrier(equaliser(x)))` (CMA leaves a rotation, which
    the carrier then takes out).  height, width, channels, length and differentiability are those of `front`; `fit` fits `front`
    on the subset after both stages.  The carrier and the equaliser must be planar (the front ends' layout) and of the front
    end's length."""

    reference = "carrier_reference"

    def __init__(self, front, carrier, equaliser=None):
        if not isinstance(front, FrontEnd):
            raise TypeError(f"front must be a FrontEnd (Spectrogram, CyclicSpectrum, Constellation), got {type(front).__name__}")
        for stage, cls, what in ((carrier, Carrier, "carrier"), (equaliser, Equaliser, "equaliser")):
            stage_for(stage, cls, what, True, front.length, "the front ends read planar (B, 2, length) frames",
                      f"samples, the front end for {front.length}", optional=cls is Equaliser)
        super().__init__(front.length)
        self.front, self.carrier, self.equaliser = front, carrier, equaliser
        self.height, self.width, self.channels = front.height, front.width, front.channels

    @property
    def differentiable(self):
        return self.front.differentiable

    def struct(self):
        raise TypeError("a Synchronised has no parameter struct of its own: see .front.struct and .carrier.struct")

    def __call__(self, x):
        """x: device (B, 2, length) fp32 -> the front end's image of the derotated frames, on the current stream, no host
        synchronisation; differentiable with respect to x where `front` is (the carrier estimate and the equaliser's weights
        held fixed)."""
        return self.front(self.carrier(x if self.equaliser is None else self.equaliser(x)))

    def fit(self, x_subset):
        """front.fit on the (equalised and) derotated subset.  -> self."""
        with torch.no_grad():
            self.front.fit(self.carrier(x_subset if self.equaliser is None else self.equaliser(x_subset)))
        return self

    def __repr__(self):
        if self.equaliser is None:
            return f"Synchronised({self.front!r}, {self.carrier!r})"
        return f"Synchronised({self.front!r}, {self.carrier!r}, equaliser={self.equaliser!r})"


# ---- the host definition

def _wrap32(v):
    """Integers (any width) -> the int32 they wrap to, as int64."""
    return ((np.asarray(v).astype(np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def _phasor(p):
    """e(p) of include/iqvit.h for integer phases p (int64, already wrapped): cos + j sin of pi * (float)(int32)p * 2^-31."""
    xf = np.asarray(p, dtype=np.int64).astype(np.float32).astype(np.float64) * 2.0 ** -31
    return np.cos(np.pi * xf) + 1j * np.sin(np.pi * xf)


def _fth(fth, B):
    f = _wrap32(_host(fth))
    if f.shape != (B, 2):
        raise ValueError(f"fth must have shape ({B}, 2), got {f.shape}")
    return f


def dft_reference(w, tables):
    """The two-stage transform of include/iqvit.h in fp64, the tables taken as given: w (B, N) complex -> W (B, N) complex,
    N = n1 * n2 from the tables' shapes.  With dft_tables' entries W is the N-point DFT of w."""
    t1, t2, tw = (_host(t).astype(np.float64) for t in tables)
    n1, n2 = t1.shape[1], t2.shape[1]
    T1, T2, TW = t1[0] - 1j * t1[1], t2[0] - 1j * t2[1], tw[0] - 1j * tw[1]
    A = np.einsum("ak,nab->nkb", T1, w.reshape(-1, n1, n2))               # [k1, b]
    Bm = A * TW[np.arange(n1)[:, None] * np.arange(n2)[None, :]]
    Wm = np.einsum("nkb,bq->nqk", Bm, T2)                                   # [k2, k1]: k = k1 + n1 k2
    return Wm.reshape(-1, n1 * n2)


def carrier_reference(x, tables, order, k_max=None, refine=True, planar=True, fth=None):
    """The definition of include/iqvit.h in fp64 on the host, the fp32 tables (t1, t2, tw) taken as given.  x: (B, 2, len)
    (planar) or (B, len, 2).  fth: (B, 2) integers: IQ_CR_GIVEN (tables may be None).  k_max None: N / 2.
    -> out (x's shape), est (B, 4), fth (B, 2) int64 holding int32 values, power (B, N) (None when given), float64."""
    z = _frames(x, planar)
    B, length = z.shape
    M = _order(order)
    n = np.arange(length, dtype=np.int64)
    est = np.full((B, 4), np.nan)
    if fth is not None:
        ft = _fth(fth, B)
        power = None
    else:
        n1, n2 = np.asarray(tables[0]).shape[1], np.asarray(tables[1]).shape[1]
        Nd = n1 * n2
        if Nd < length:
            raise ValueError(f"the tables' N = {Nd} is below the frame length {length}")
        k_max = Nd // 2 if k_max is None else _index(k_max, "k_max", 0, Nd // 2)
        w = z.copy()
        with np.errstate(all="ignore"):                      # a non-finite sample makes a non-finite line: defined below
            for _ in range(int(math.log2(M))):
                w = w * w
        wp = np.zeros((B, Nd), np.complex128)
        wp[:, :length] = w
        W = dft_reference(wp, tables)
        power = W.real ** 2 + W.imag ** 2
        s = np.arange(-k_max, min(k_max, Nd // 2 - 1) + 1, dtype=np.int64)
        ft = np.zeros((B, 2), np.int64)
        for i in range(B):
            P = power[i]
            key = np.where(np.isnan(P), np.inf, P)[s % Nd]
            sh = int(s[int(np.argmax(key))])
            kh = sh % Nd
            b = P[kh]
            d = 0.0
            if b == 0 or not np.isfinite(b):
                est[i] = (0.0, 0.0, sh, 0.0)
                continue
            if refine:
                a, c = P[(kh - 1) % Nd], P[(kh + 1) % Nd]
                with np.errstate(all="ignore"):
                    den = a - 2.0 * b + c
                    if den < 0 and np.isfinite(den):
                        d = float(np.clip(0.5 * (a - c) / den, -0.5, 0.5))
            F = int(_wrap32(int(np.rint((sh + d) / (Nd * M) * 2.0 ** 32))))
            G = _wrap32(F * M)
            S = np.sum(w[i] * np.conj(_phasor(_wrap32(G * n))))
            TH = int(_wrap32(int(np.rint(math.atan2(S.imag, S.real) / (2.0 * math.pi * M) * 2.0 ** 32))))
            ft[i] = (F, TH)
            pw = np.sum(w[i].real ** 2 + w[i].imag ** 2)
            q = (S.real ** 2 + S.imag ** 2) / (length * pw) if length * pw > 0 else 0.0
            est[i] = (F * 2.0 ** -32, TH * 2.0 ** -32 * 2.0 * math.pi, sh + d, q)
    if fth is not None:
        est[:, 0], est[:, 1] = ft[:, 0] * 2.0 ** -32, ft[:, 1] * 2.0 ** -32 * 2.0 * math.pi
    with np.errstate(invalid="ignore"):
        out = z * np.conj(_phasor(_wrap32(ft[:, :1] * n[None, :] + ft[:, 1:])))
    return _unframes(out, planar), est, ft, power


def carrier_reference_bwd(dout, fth, planar=True):
    """The adjoint in fp64 with the estimate held at fth ((B, 2) integers): the gradient of sum(out * dout) with respect to x,
    out = carrier_reference(x, ..., fth=fth)[0]:  dx[n] = dout[n] e(F n + TH).  dout in x's layout -> dx likewise."""
    dz = _frames(dout, planar)
    B, length = dz.shape
    ft = _fth(fth, B)
    n = np.arange(length, dtype=np.int64)
    return _unframes(dz * _phasor(_wrap32(ft[:, :1] * n[None, :] + ft[:, 1:])), planar)
