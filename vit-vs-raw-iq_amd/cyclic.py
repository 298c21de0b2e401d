"""Cyclic-spectrum front end on the device: planar (B, 2, len) I/Q frames -> the (B, C, n_fft, n_fft) spectral correlation image.

Beside the spectrogram (spectrogram.py) this is the second image a ViT can read.  A spectrogram discards the second-order
cyclostationarity of a signal; the spectral correlation function (SCF) keeps it: a linearly modulated signal correlates with a
copy of itself shifted in frequency by the symbol rate (a line at alpha = fs / sps), and a real constellation (BPSK, PAM) also
with its own conjugate.  One HIP kernel (csrc/cyclic.hip, iq_frames_cyclic) computes the first stage of the FFT accumulation
method: the spectrogram's channelizer, a phase reference per window, and the complex Gram matrices over time, both stages on
the fp32-input MFMA, the channelized frame never leaving the CU.  iq_frames_cyclic_bwd is its adjoint (everything recomputed
from x, a deterministic gather, no atomics): a front end built with `differentiable=True` carries gradients down to the SIGNAL
(x.grad, saliency, FGSM / PGD on the frame); the default still refuses an input that requires grad, as it always did.  There is
no CPU path; `cyclic_reference` / `cyclic_reference_bwd` are the host fp64 DEFINITION the tests compare against.

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

The adjoint (written out in include/iqvit.h), with G_w = dL/dRe w + i dL/dIm w for L = sum(image * dout), rho = rc[r] + i rs[r],
g[k,l] = dout at the SCF element of the pair (k, l) and gc[k,l] at the conjugate one:
  u[k,l]   = scale (g[k,l] + g[l,k]) phi,  phi = 1 | 1 / (ln 10 (P + floor)) | 1 / den,  den = D[k] D[l] inv_norm^2 + floor
  H[k,l]   = 2 inv_norm^2 u[k,l] S[k,l]   (Hc from gc, Pc, Sc likewise)
  gD[k]    = -inv_norm^2 sum_l scale [(g[k,l] + g[l,k]) P + (gc[k,l] + gc[l,k]) Pc] D[l] / den^2   (coherence only)
  G_Y[t,k] = sum_l H[k,l] Y[t,l] + Hc[k,l] conj(Y[t,l]) + 2 gD[k] Y[t,k],   G_X = rho G_Y
  G_z[j]   = sum over (t, m) with j0 + m = j of sum_k w[m] exp(+2 pi i k m / Np) G_X[t,k];  dx = (Re G_z, Im G_z)
The backward kernel keeps the frame AND its gradient in LDS: `differentiable=True` refuses (at construction) a geometry with
4 * (2 * (2 length rounded up to 4) + 67 n_fft + 6688) bytes above 160 KB -- frames longer than 4280 samples at n_fft 256, than
8032 at n_fft 32; every n_fft works up to 4096 samples.

  CyclicSpectrum(n_fft, length, hop, pad, columns, window, kind, mode, floor, scale, shift, differentiable)
                                                         cs(x) -> image;  .fit;  .struct()
  CyclicSpectrum.for_model(model, length, **kw)          n_fft and kind from the ViT's (square) image and its channels
  cyclic_reference(x, cs), cyclic_reference_bwd(x, dout, cs)          host fp64
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from ._args import _index
from .frontend import FrontEnd, _FrontEndFn, _host, _image_geometry, _mode
from .spectrogram import FFT_STEP, MAX_FFT, MIN_FFT, WINDOWS, _twiddles, _window

KINDS = ("scf", "conj", "both")
MODES = ("power", "log", "coherence")
LDS_BYTES = 160 * 1024       # what one workgroup of the backward kernel may have


def adjoint_lds_bytes(n_fft, length):
    """LDS of iq_frames_cyclic_bwd at its smallest layout (include/iqvit.h): the frame, its gradient, rot, D, 32 columns of Y
    and six 32 x 33 tiles."""
    return 4 * (2 * ((2 * length + 3) & ~3) + 67 * n_fft + 6688)


class CyclicSpectrum(FrontEnd):
    """The geometry and scaling of one front end.  Defaults: hop = n_fft // 4, columns = every window that lies wholly inside
    the frame with that hop and pad (at least one), inv_norm = 1 / (columns * sum w^2).  Arguments are checked here, before any
    device work; the tables go to a device at the first call for that device and stay there.  differentiable=False (the
    default) refuses an input that requires grad; True sends such an input through iq_frames_cyclic_bwd on the way back (the
    images are the same bit for bit either way)."""

    reference = "cyclic_reference"

    def __init__(self, n_fft, length=1024, hop=None, pad=0, columns=None, window="hann", kind="both", mode="coherence",
                 floor=1e-6, scale=1.0, shift=0.0, differentiable=False):
        self.n_fft = self.height = self.width = _index(n_fft, "n_fft", MIN_FFT, MAX_FFT)
        if self.n_fft % FFT_STEP:
            raise ValueError(f"n_fft must be a multiple of {FFT_STEP}, got {n_fft!r}")
        super().__init__(length)
        self.hop = self.n_fft // 4 if hop is None else _index(hop, "hop", 1, 2 ** 31 - 1)
        self.pad = _index(pad, "pad", 0, 2 ** 31 - 1)
        if columns is None:
            columns = max(1, (self.length + self.pad - self.n_fft) // self.hop + 1)
        self.columns = _index(columns, "columns", 1, 2 ** 31 - 1)
        if window not in WINDOWS:
            raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        self.window, self.kind, self.mode = window, kind, _mode(mode, MODES)
        self.channels = 2 if kind == "both" else 1
        self._set_scaling(floor, scale, shift)
        if not isinstance(differentiable, bool):
            raise TypeError(f"differentiable must be a bool, got {differentiable!r}")
        if differentiable and adjoint_lds_bytes(self.n_fft, self.length) > LDS_BYTES:
            raise ValueError(f"differentiable=True: the adjoint keeps the frame and its gradient in LDS and needs "
                             f"{adjoint_lds_bytes(self.n_fft, self.length)} bytes at n_fft {self.n_fft}, length {self.length}; "
                             f"a workgroup has {LDS_BYTES}")
        self.differentiable = differentiable
        w = _window(window, self.n_fft)
        self.inv_norm = 1.0 / (self.columns * float(np.sum(w * w)))
        c, s = _twiddles(self.n_fft, w)
        self.table = np.stack([c, s]).astype(np.float32)           # (2, n_fft, n_fft): the spectrogram's table
        ang = 2.0 * np.pi * np.arange(self.n_fft) / self.n_fft
        self.rot = np.stack([np.cos(ang), np.sin(ang)]).astype(np.float32)     # (2, n_fft)

    @classmethod
    def for_model(cls, model, length=1024, **kw):
        """A front end whose image is the input of `model` (an AMCTransformerViT or its encoder): a square image of n_fft =
        img_size_h = img_size_w; in_channels 1 gives kind 'scf' unless `kind` says 'conj', in_channels 2 gives 'both'."""
        geom = _image_geometry(model)
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

    def rot_on(self, device):
        """The fp32 rot table on `device` (uploaded once per device)."""
        return self.table_on(device, "rot")

    def __call__(self, x):
        """x: device (B, 2, len) fp32 -> (B, channels, n_fft, n_fft) fp32 on the current stream, no host synchronisation;
        with differentiable=True differentiable with respect to x.  Nothing is recorded for backward unless a gradient is
        wanted."""
        self._check(x)
        if x.requires_grad and torch.is_grad_enabled():
            return _FrontEndFn.apply(x, self)
        return self._launch(x.detach())[1]

    def _forward(self, x, out, B, par, stream):
        N.check(N.lib().iq_frames_cyclic(x.data_ptr(), self.table_on(x.device).data_ptr(), self.rot_on(x.device).data_ptr(),
                                         out.data_ptr(), B, self.length, C.byref(par), stream), "iq_frames_cyclic")

    def _backward(self, x, dout, dx, B, par, stream):
        N.check(N.lib().iq_frames_cyclic_bwd(x.data_ptr(), self.table_on(x.device).data_ptr(), self.rot_on(x.device).data_ptr(),
                                             dout.data_ptr(), dx.data_ptr(), B, self.length, C.byref(par), stream),
                "iq_frames_cyclic_bwd")

    def __repr__(self):
        return (f"CyclicSpectrum(n_fft={self.n_fft}, length={self.length}, hop={self.hop}, pad={self.pad}, "
                f"columns={self.columns}, window={self.window!r}, kind={self.kind!r}, mode={self.mode!r}, floor={self.floor}, "
                f"scale={self.scale}, shift={self.shift}, differentiable={self.differentiable})")


def _channelized(x, cs, table=None, rot=None):
    """Y (B, T, bins) of the definition in fp64 with what the adjoint needs beside it: E[m,k] = c - i s, conj(rho)[t,k], the
    sample index (T, n) of every window element and the mask of those inside the frame.  table (2, n, n) / rot (2, n) replace
    the fp64 tables of `cs` (the tests' integer cases)."""
    if not isinstance(cs, CyclicSpectrum):
        raise TypeError(f"cs must be a CyclicSpectrum, got {type(cs).__name__}")
    x = _host(x).astype(np.float64)
    if x.ndim != 3 or x.shape[1] != 2 or x.shape[2] != cs.length:
        raise ValueError(f"x must be (B, 2, {cs.length}), got {x.shape}")
    n, T = cs.n_fft, cs.columns
    c, s = _twiddles(n, _window(cs.window, n)) if table is None else np.asarray(table, dtype=np.float64)
    E = c - 1j * s                                                     # w[m] exp(-2 pi i k m / n)
    j0 = np.arange(T, dtype=np.int64) * cs.hop - cs.pad
    j = j0[:, None] + np.arange(n, dtype=np.int64)[None, :]
    inside = (j >= 0) & (j < cs.length)
    z = x[:, 0, :] + 1j * x[:, 1, :]
    cols = np.where(inside[None], z[:, np.clip(j, 0, cs.length - 1)], 0.0)        # (B, T, n)
    X = cols @ E                                                       # (B, T, bins)
    r = (np.arange(n, dtype=np.int64)[None, :] * (j0 % n)[:, None]) % n           # (T, bins); numpy's % is non-negative
    if rot is None:
        ang = 2.0 * np.pi * r / n
        crho = np.cos(ang) - 1j * np.sin(ang)
    else:
        rot = np.asarray(rot, dtype=np.float64)
        crho = rot[0][r] - 1j * rot[1][r]
    return X * crho[None], E, crho, j, inside


def cyclic_reference(x, cs):
    """The definition in fp64 on the host, from the formula (matrix products, no FFT).
    x: (B, 2, len) -> float64 (B, channels, n_fft, n_fft)."""
    Y, _, _, _, _ = _channelized(x, cs)
    n = cs.n_fft
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


def cyclic_reference_bwd(x, dout, cs, table=None, rot=None):
    """The analytic adjoint in fp64: the gradient of sum(cyclic_reference(x) * dout) with respect to x, from the formulae of
    the module docstring.  dout: (B, channels, n_fft, n_fft) -> float64 (B, 2, len).  table (2, n_fft, n_fft) and rot (2, n_fft)
    replace the fp64 tables of `cs` (any numbers: the tests' integer cases)."""
    Y, E, crho, j, inside = _channelized(x, cs, table, rot)
    n, B = cs.n_fft, Y.shape[0]
    d = _host(dout).astype(np.float64)
    if d.shape != (B, cs.channels, n, n):
        raise ValueError(f"dout must be {(B, cs.channels, n, n)}, got {d.shape}")
    D = (Y.real ** 2 + Y.imag ** 2).sum(axis=1)                        # (B, bins)
    Yt = Y.transpose(0, 2, 1)
    inv2 = cs.inv_norm ** 2
    k, l = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    den = D[:, :, None] * D[:, None, :] * inv2 + cs.floor
    GY = np.zeros_like(Y)
    gD = np.zeros_like(D)
    for ch, conj in enumerate(((False,), (True,), (False, True))[KINDS.index(cs.kind)]):
        G = Yt @ (Y if conj else np.conj(Y))                           # S or Sc (B, k, l)
        a = (k + l) % n if conj else (k - l) % n
        g = d[:, ch, (a + n // 2) % n, (k + n // 2) % n]               # dout at the element of the pair (k, l)
        w = cs.scale * (g + g.transpose(0, 2, 1))
        P = (G.real ** 2 + G.imag ** 2) * inv2
        if cs.mode == "power":
            u = w
        elif cs.mode == "log":
            u = w / (math.log(10.0) * (P + cs.floor))
        else:
            u = w / den
            gD -= inv2 * (w * P * D[:, None, :] / den ** 2).sum(axis=2)
        H = 2.0 * inv2 * u * G
        GY += (np.conj(Y) if conj else Y) @ H.transpose(0, 2, 1)       # sum_l H[k,l] Y[t,l]  resp.  Hc[k,l] conj(Y[t,l])
    GY += 2.0 * gD[:, None, :] * Y
    dz = (GY * np.conj(crho)[None]) @ np.conj(E).T                     # G_X = rho G_Y; (B, T, n samples of the window)
    out = np.zeros((B, 2, cs.length))
    for t in range(cs.columns):
        ok = inside[t]
        out[:, 0, j[t, ok]] += dz[:, t, ok].real                       # the indices of one column are distinct
        out[:, 1, j[t, ok]] += dz[:, t, ok].imag
    return out
