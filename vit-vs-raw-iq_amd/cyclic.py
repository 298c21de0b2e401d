"""Cyclic-spectrum front end on the device: planar (B, 2, len) I/Q frames -> the (B, C, n_fft, n_fft) spectral correlation image.

Beside the spectrogram (spectrogram.py) this is the second image a ViT can read.  A spectrogram discards the second-order
cyclostationarity of a signal; the spectral correlation function (SCF) keeps it: a linearly modulated signal correlates with a
copy of itself shifted in frequency by the symbol rate (a line at alpha = fs / sps), and a real constellation (BPSK, PAM) also
with its own conjugate.  One HIP kernel (csrc/cyclic.hip, iq_frames_cyclic) computes the first stage of the FFT accumulation
method: the spectrogram's channelizer, a phase reference per window, and the complex Gram matrices over time, both stages on
the fp32-input MFMA, the channelized frame never leaving the CU.  There is no CPU path; `cyclic_reference` is the host fp64
DEFINITION the tests compare against.  The adjoint is not implemented: an input that requires grad is refused.

With z[j] = I[j] + i Q[j], Np = n_fft, T = columns and window t's first sample j0 = t*hop - pad (samples outside [0, len) count
as zero):
  X[t,k]  = sum_m z[j0 + m] w[m] exp(-2 pi i k m / Np)                    the spectrogram's table (c, s)
  Y[t,k]  = X[t,k] (rc[r] - i rs[r]),  r = (k (j0 mod Np)) mod Np          rot: rc = cos(2 pi r / Np), rs = sin(2 pi r / Np)
  S[k,l]  = sum_t Y[t,k] conj(Y[t,l])       SCF at f = (f_k + f_l) / 2, alpha = f_k - f_l
  Sc[k,l] = sum_t Y[t,k] Y[t,l]             conjugate SCF at alpha = f_k + f_l
  D[k]    = sum_t |Y[t,k]|^2                PSD
  P = |S|^2 inv_norm^2 (Pc likewise), inv_norm = 1 / (T sum w^2)
  'power': v = P;  'log': v = log10(P + floor);  'coherence': v = P / (D[k] D[l] inv_norm^2 + floor), in [0, 1]
  image = v * scale + shift
Row rho holds cyclic bin a = (rho + Np/2) mod Np, column kappa channel k = (kappa + Np/2) mod Np (fftshift order); the SCF
channel reads l = (k - a) mod Np, the conjugate channel l = (a - k) mod Np.  Both tables are computed in fp64 and rounded to fp32
once; the kernel treats them as plain numbers.

  CyclicSpectrum(n_fft, length, hop, pad, columns, window, kind, mode, floor, scale, shift)   cs(x) -> image;  .fit;  .struct()
  CyclicSpectrum.for_model(model, length, **kw)          n_fft and kind from the ViT's (square) image and its channels
  cyclic_reference(x, cs)                                host fp64
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N
from .impairments import _index, _number
from .spectrogram import FFT_STEP, MAX_FFT, MAX_LENGTH, MIN_FFT, WINDOWS, _fit, _host, _on_device, _twiddles, _window

KINDS = ("scf", "conj", "both")
MODES = ("power", "log", "coherence")


class CyclicSpectrum:
    """The geometry and scaling of one front end.  Defaults: hop = n_fft // 4, columns = every window that lies wholly inside
    the frame with that hop and pad (at least one), inv_norm = 1 / (columns * sum w^2).  Arguments are checked here, before any
    device work; the tables go to a device at the first call for that device and stay there."""

    def __init__(self, n_fft, length=1024, hop=None, pad=0, columns=None, window="hann", kind="both", mode="coherence",
                 floor=1e-6, scale=1.0, shift=0.0):
        self.n_fft = _index(n_fft, "n_fft", MIN_FFT, MAX_FFT)
        if self.n_fft % FFT_STEP:
            raise ValueError(f"n_fft must be a multiple of {FFT_STEP}, got {n_fft!r}")
        self.width = self.n_fft
        self.length = _index(length, "length", 1, MAX_LENGTH)
        self.hop = self.n_fft // 4 if hop is None else _index(hop, "hop", 1, 2 ** 31 - 1)
        self.pad = _index(pad, "pad", 0, 2 ** 31 - 1)
        if columns is None:
            columns = max(1, (self.length + self.pad - self.n_fft) // self.hop + 1)
        self.columns = _index(columns, "columns", 1, 2 ** 31 - 1)
        if window not in WINDOWS:
            raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        self.window, self.kind, self.mode = window, kind, mode
        self.channels = 2 if kind == "both" else 1
        self.floor = _number(floor, "floor")
        if self.floor <= 0 or float(np.float32(self.floor)) <= 0:
            raise ValueError(f"floor must be positive (in fp32), got {floor!r}")
        self.scale, self.shift = _number(scale, "scale"), _number(shift, "shift")
        w = _window(window, self.n_fft)
        self.inv_norm = 1.0 / (self.columns * float(np.sum(w * w)))
        c, s = _twiddles(self.n_fft, w)
        self.table = np.stack([c, s]).astype(np.float32)           # (2, n_fft, n_fft): the spectrogram's table
        ang = 2.0 * np.pi * np.arange(self.n_fft) / self.n_fft
        self.rot = np.stack([np.cos(ang), np.sin(ang)]).astype(np.float32)     # (2, n_fft)
        self._tables, self._rots = {}, {}

    @classmethod
    def for_model(cls, model, length=1024, **kw):
        """A front end whose image is the input of `model` (an AMCTransformerViT or its encoder): a square image of n_fft =
        img_size_h = img_size_w; in_channels 1 gives kind 'scf' unless `kind` says 'conj', in_channels 2 gives 'both'."""
        geom = getattr(getattr(model, "encoder", model), "_geom", None)
        if not isinstance(geom, dict) or geom.get("kind") != 0:
            raise TypeError(f"expected a ViT model (image input), got {type(model).__name__}")
        if geom["img_h"] != geom["img_w"]:
            raise ValueError(f"a cyclic spectrum is a square image, the model expects {geom['img_h']}x{geom['img_w']}")
        if geom["in_channels"] not in (1, 2):
            raise ValueError(f"a cyclic spectrum has one or two channels, the model expects {geom['in_channels']}")
        kind = kw.pop("kind", "both" if geom["in_channels"] == 2 else "scf")
        cs = cls(geom["img_h"], length, kind=kind, **kw)
        if cs.channels != geom["in_channels"]:
            raise ValueError(f"kind {kind!r} has {cs.channels} channel(s), the model expects {geom['in_channels']}")
        return cs

    def struct(self) -> N.Cyclic:
        """The iq_cyclic_t of a call."""
        return N.Cyclic(n_fft=self.n_fft, hop=self.hop, pad=self.pad, columns=self.columns, kind=KINDS.index(self.kind),
                        mode=MODES.index(self.mode), inv_norm=self.inv_norm, floor=self.floor, scale=self.scale,
                        shift=self.shift)

    def table_on(self, device):
        """The fp32 (c, s) table on `device` (uploaded once per device)."""
        return _on_device(self._tables, self.table, device)

    def rot_on(self, device):
        """The fp32 rot table on `device` (uploaded once per device)."""
        return _on_device(self._rots, self.rot, device)

    def _check(self, x, what="x"):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != 2 or x.shape[2] != self.length:
            raise ValueError(f"{what} must be a (B, 2, {self.length}) tensor, got "
                             f"{tuple(x.shape) if hasattr(x, 'shape') else x!r}")
        if not x.is_cuda:
            raise N.IqError("CyclicSpectrum runs on the MI355X only: x is a CPU tensor and there is no CPU fallback "
                            "(cyclic_reference is the host definition used by the tests)")
        if x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("CyclicSpectrum is not differentiable: its adjoint is not implemented, pass x.detach() "
                               "(a Spectrogram carries gradients down to the signal)")

    def __call__(self, x):
        """x: device (B, 2, len) fp32 -> (B, channels, n_fft, n_fft) fp32 on the current stream, no host synchronisation."""
        self._check(x)
        x = x.detach().contiguous().float()
        B = x.shape[0]
        out = torch.empty(B, self.channels, self.n_fft, self.n_fft, dtype=torch.float32, device=x.device)
        par = self.struct()
        if B > 0:
            N.check(N.lib().iq_frames_cyclic(x.data_ptr(), self.table_on(x.device).data_ptr(), self.rot_on(x.device).data_ptr(),
                                             out.data_ptr(), B, self.length, C.byref(par),
                                             torch.cuda.current_stream(x.device).cuda_stream), "iq_frames_cyclic")
        return out

    def fit(self, x_subset):
        """Set scale and shift so that the images of `x_subset` (device (B, 2, len)) have zero mean and unit standard deviation
        (unbiased, floored at 1e-8): one call with scale 1 and shift 0, then a device mean / std.  One host synchronisation.
        -> self."""
        return _fit(self, x_subset)

    def __repr__(self):
        return (f"CyclicSpectrum(n_fft={self.n_fft}, length={self.length}, hop={self.hop}, pad={self.pad}, "
                f"columns={self.columns}, window={self.window!r}, kind={self.kind!r}, mode={self.mode!r}, floor={self.floor}, "
                f"scale={self.scale}, shift={self.shift})")


def cyclic_reference(x, cs):
    """The definition in fp64 on the host, from the formula (matrix products, no FFT).
    x: (B, 2, len) -> float64 (B, channels, n_fft, n_fft)."""
    if not isinstance(cs, CyclicSpectrum):
        raise TypeError(f"cs must be a CyclicSpectrum, got {type(cs).__name__}")
    x = _host(x).astype(np.float64)
    if x.ndim != 3 or x.shape[1] != 2 or x.shape[2] != cs.length:
        raise ValueError(f"x must be (B, 2, {cs.length}), got {x.shape}")
    n, T = cs.n_fft, cs.columns
    c, s = _twiddles(n, _window(cs.window, n))
    E = c - 1j * s                                                     # w[m] exp(-2 pi i k m / n)
    j0 = np.arange(T, dtype=np.int64) * cs.hop - cs.pad
    j = j0[:, None] + np.arange(n, dtype=np.int64)[None, :]
    inside = (j >= 0) & (j < cs.length)
    z = x[:, 0, :] + 1j * x[:, 1, :]
    cols = np.where(inside[None], z[:, np.clip(j, 0, cs.length - 1)], 0.0)        # (B, T, n)
    X = cols @ E                                                       # (B, T, bins)
    r = (np.arange(n, dtype=np.int64)[None, :] * (j0 % n)[:, None]) % n           # (T, bins); numpy's % is non-negative
    ang = 2.0 * np.pi * r / n
    Y = X * (np.cos(ang) - 1j * np.sin(ang))[None]
    D = (Y.real ** 2 + Y.imag ** 2).sum(axis=1)                        # (B, bins)
    Yt = Y.transpose(0, 2, 1)                                          # (B, bins, T)
    inv2 = cs.inv_norm ** 2
    a = (np.arange(n) + n // 2) % n                                    # cyclic bin of row rho
    k = (np.arange(n) + n // 2) % n                                    # channel of column kappa
    chans = []
    for conj in ((False,), (True,), (False, True))[KINDS.index(cs.kind)]:
        G = Yt @ (Y if conj else np.conj(Y))                           # (B, k, l)
        l = (a[:, None] - k[None, :]) % n if conj else (k[None, :] - a[:, None]) % n          # (rho, kappa)
        kk = np.broadcast_to(k[None, :], l.shape)
        g = G[:, kk, l]
        P = (g.real ** 2 + g.imag ** 2) * inv2
        if cs.mode == "power":
            v = P
        elif cs.mode == "log":
            v = np.log10(P + cs.floor)
        else:
            v = P / (D[:, kk] * D[:, l] * inv2 + cs.floor)
        chans.append(v * cs.scale + cs.shift)
    return np.ascontiguousarray(np.stack(chans, axis=1))
