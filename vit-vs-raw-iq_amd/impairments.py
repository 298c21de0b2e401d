"""Channel impairments on the device: training augmentation and accuracy-versus-channel curves.

What a modulation classifier meets between transmitter and ADC -- carrier phase, carrier frequency offset, timing, gain and
noise -- applied to RAW (B, len, 2) I/Q frames by one HIP kernel (csrc/impair.hip, iq_frames_impair) that also does the z-score
and layout of the input pipeline (data.py, iq_frames_preprocess).  The same call with random ranges is the usual augmentation of
this task: rotation, flip and Gaussian noise of I/Q frames (Huang et al. 2019, "Data augmentation for deep learning-based radio
modulation classification").  There is no CPU path; `impair_reference` is the host fp64 DEFINITION the tests compare against.

Per frame, in this fixed order (n is the output sample index, x = I + jQ):
  1. circular shift      x[n] <- x[(n + s) % len]                      s uniform in {0..shift_max}
  2. conjugate           Q <- -Q with probability 1/2                   (conj=True)
  3. rotate              x[n] <- x[n] exp(j (theta + k pi/2 + 2 pi f n))  theta ~ U[phase], f ~ U[cfo] cycles/sample,
                                                                        k uniform in {0,1,2,3} (rot90=True)
  4. gain                x <- 10^(dB/20) x                              dB ~ U[gain_db]
  5. noise               x <- x + w, w complex Gaussian of total power P / 10^(snr/10), P = mean |x|^2 of the frame as given
                         (after the gain): I and Q get half each; snr ~ U[snr_db], None = no noise
  6. z-score per channel, then the layout of the model: 'vit' (B, 1, h, w) = [first h*w/2 I | first h*w/2 Q], 'rawiq' (B, 2, len)

Random numbers are Philox4x32-7 keyed by (seed, step, frame_base + i) and, for the noise, the sample-pair index: frame i of a
stream of frames gets the same result whatever the batch size and however the stream is cut into calls.

  Impairments(phase, cfo, rot90, conj, shift_max, gain_db, snr_db)      the ranges; Impairments.augmentation() for training
  impair(raw, stats, layout, imp, seed, step, frame_base, h, w, return_drawn)
  impair_reference(raw, drawn, stats, layout, h, w)                     host fp64, everything but the noise samples
  impairment_curve(model, raw, labels, stats, kind, values, ...)        top-1 accuracy per value of one quantity
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from ._args import _flag, _index, _number
from .frontend import front_end
from .saliency import _batch, _classes, _forward, _resolve

KINDS = ("snr_db", "phase", "cfo", "shift", "gain_db")
_front_end = front_end       # the name this function had while it lived here


def _range(v, what):
    """None, a number (fixed value) or (lo, hi) -> None or (lo, hi) floats with lo <= hi."""
    if v is None:
        return None
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what} must be None, a number or (lo, hi), got {v!r}")
        lo, hi = _number(v[0], f"{what} lower bound"), _number(v[1], f"{what} upper bound")
        if lo > hi:
            raise ValueError(f"{what} lower bound {lo} is above the upper bound {hi}")
        return lo, hi
    v = _number(v, what)
    return v, v


class Impairments:
    """The ranges one call draws from.  Each of phase (rad), cfo (cycles per sample), gain_db and snr_db is None (off), a number
    (that value for every frame) or (lo, hi) (uniform per frame); rot90 / conj switch the quarter-turn and the Q flip on;
    shift_max = m draws a circular shift from {0..m} (must stay below the frame length)."""

    __slots__ = ("phase", "cfo", "rot90", "conj", "shift_max", "gain_db", "snr_db")

    def __init__(self, phase=None, cfo=None, rot90=False, conj=False, shift_max=0, gain_db=None, snr_db=None):
        self.phase = _range(phase, "phase")
        self.cfo = _range(cfo, "cfo")
        self.rot90 = _flag(rot90, "rot90")
        self.conj = _flag(conj, "conj")
        self.shift_max = _index(shift_max, "shift_max", 0, 2 ** 31 - 1)
        self.gain_db = _range(gain_db, "gain_db")
        self.snr_db = _range(snr_db, "snr_db")

    @classmethod
    def augmentation(cls, length: int = 1024):
        """The default for training: what leaves the class of a frame alone and a receiver cannot know -- any carrier phase
        (-pi, pi) plus the quarter turns and the I/Q flip of Huang et al. 2019, any circular start (shift_max = length - 1), a
        gain within +-1 dB.  No noise is added: it would lower the SNR the labels were recorded at."""
        return cls(phase=(-math.pi, math.pi), rot90=True, conj=True, shift_max=_index(length, "length", 1) - 1,
                   gain_db=(-1.0, 1.0))

    def replace(self, **kw):
        cur = {k: getattr(self, k) for k in self.__slots__}
        cur.update(kw)
        return Impairments(**cur)

    def struct(self, seed=0, step=0, frame_base=0) -> N.Impair:
        """The iq_impair_t of one call."""
        ph, cf, g = self.phase or (0.0, 0.0), self.cfo or (0.0, 0.0), self.gain_db or (0.0, 0.0)
        sn = self.snr_db or (math.nan, math.nan)
        return N.Impair(phase_lo=ph[0], phase_hi=ph[1], cfo_lo=cf[0], cfo_hi=cf[1], rot90=int(self.rot90), conj=int(self.conj),
                        shift_max=self.shift_max, gain_db_lo=g[0], gain_db_hi=g[1], snr_db_lo=sn[0], snr_db_hi=sn[1],
                        seed=_index(seed, "seed", 0, 2 ** 64 - 1), step=_index(step, "step", 0, 2 ** 32 - 1),
                        frame_base=_index(frame_base, "frame_base", 0, 2 ** 64 - 1))

    def __repr__(self):
        return "Impairments(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


def _stats4(stats):
    """{'i_mean','i_std','q_mean','q_std'} (data.normalization_stats) or (mean[2], std[2]) (data.zscore_stats) -> 4 floats."""
    if isinstance(stats, dict):
        v = [stats["i_mean"], stats["i_std"], stats["q_mean"], stats["q_std"]]
    else:
        try:
            mean, std = stats
            v = [mean[0], std[0], mean[1], std[1]]
        except (TypeError, ValueError, IndexError):
            raise TypeError("stats must be a dict with i_mean, i_std, q_mean, q_std or a (mean[2], std[2]) pair") from None
    v = [float(np.float32(x)) for x in v]
    if not (v[1] > 0 and v[3] > 0):
        raise ValueError(f"standard deviations must be positive, got {v[1]!r} and {v[3]!r}")
    return v


def _take(layout, length, h, w):
    if layout not in ("vit", "rawiq"):
        raise ValueError(f"unknown layout: {layout!r}")
    take = length if layout == "rawiq" else h * w // 2
    if take <= 0 or take > length:
        raise ValueError(f"image {h}x{w} needs {take} samples per channel, frames have {length}")
    return take


def impair(raw, stats, layout, imp, seed=0, step=0, frame_base=0, h=32, w=64, return_drawn=False, spectrogram=None):
    """raw: device (B, len, 2) fp32 frames -> the model input, (B, 1, h, w) for layout 'vit' or (B, 2, len) for 'rawiq'; with
    return_drawn also the fp32 (B, 8) table {theta, f, k, conj, s, g, snr_db, sigma per component} the kernel used.  With
    `spectrogram` (any frontend.FrontEnd; layout 'vit') the whole impaired frame goes through it on the same stream and the
    result is its (B, channels, height, width) image: h and w are not used."""
    if not isinstance(imp, Impairments):
        raise TypeError(f"imp must be an Impairments, got {type(imp).__name__}")
    if not isinstance(raw, torch.Tensor) or raw.dim() != 3 or raw.shape[2] != 2:
        raise ValueError(f"raw must be a (B, len, 2) tensor, got {tuple(raw.shape) if hasattr(raw, 'shape') else raw!r}")
    st = (C.c_float * 4)(*_stats4(stats))
    B, length = raw.shape[0], raw.shape[1]
    spec = front_end(spectrogram, layout, length)
    take = _take(layout, length, h, w) if spec is None else length
    if imp.shift_max >= max(length, 1):
        raise ValueError(f"shift_max {imp.shift_max} must be below the frame length {length}")
    par = imp.struct(seed, step, frame_base)
    if not raw.is_cuda:
        raise N.IqError("impair runs on the MI355X only: raw is a CPU tensor and there is no CPU fallback "
                        "(impair_reference is the host definition used by the tests)")
    raw = raw.contiguous().float()
    out = torch.empty(B, 2, take, dtype=torch.float32, device=raw.device)
    drawn = torch.empty(B, 8, dtype=torch.float32, device=raw.device) if return_drawn else None
    if B > 0:
        N.check(N.lib().iq_frames_impair(raw.data_ptr(), out.data_ptr(), N.ptr(drawn), B, length, take, st, C.byref(par),
                                         torch.cuda.current_stream(raw.device).cuda_stream), "iq_frames_impair")
    if spec is not None:
        x = spec(out)
    else:
        x = out.view(B, 1, h, w) if layout == "vit" else out
    return (x, drawn) if return_drawn else x


def impair_reference(raw, drawn, stats, layout, h=32, w=64):
    """The deterministic part in fp64 on the host: shift, conjugate, rotate, gain, z-score and layout with the per-frame values
    of `drawn` (columns theta, f, k, conj, s, g; the noise columns are not used).  -> float64 array in the model's layout."""
    to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)   # noqa: E731
    x = to_np(raw).astype(np.float64)
    d = to_np(drawn).astype(np.float64).reshape(-1, 8)
    if x.ndim != 3 or x.shape[2] != 2 or len(d) != len(x):
        raise ValueError(f"raw must be (B, len, 2) and drawn (B, 8), got {x.shape} and {d.shape}")
    i_mean, i_std, q_mean, q_std = _stats4(stats)
    B, length = x.shape[0], x.shape[1]
    take = _take(layout, length, h, w)
    n = np.arange(length)
    theta, f, k, cj, s, g = (d[:, c:c + 1] for c in range(6))
    z = x[:, :, 0] + 1j * x[:, :, 1]
    z = np.take_along_axis(z, (n[None, :] + s.astype(np.int64)) % length, axis=1)
    z = np.where(cj != 0, np.conj(z), z)
    z = z * np.exp(1j * (theta + k * (np.pi / 2) + 2 * np.pi * f * n[None, :])) * g
    out = np.stack([(z.real[:, :take] - i_mean) / i_std, (z.imag[:, :take] - q_mean) / q_std], axis=1)
    return out.reshape(B, 1, h, w) if layout == "vit" else out


def _fixed(base: Impairments, kind, v):
    """-> (Impairments with `kind` fixed at v, circular shift applied in front of it)"""
    if kind == "shift":
        return base, _index(v, "shift", 0)
    return base.replace(**{kind: _number(v, kind)}), 0


def impairment_curve(model, raw, labels, stats, kind, values, layout=None, base=None, batch=256, seed=0, spectrogram=None):
    """Top-1 accuracy (float) of `model` on the RAW frames per value of one quantity: kind 'snr_db' (dB), 'phase' (rad), 'cfo'
    (cycles/sample), 'shift' (samples) or 'gain_db' (dB) is fixed at each value, everything else comes from `base` (default:
    nothing else).  Chunks of `batch` frames go through `impair` with frame_base = the chunk's start and step 0, then through an
    eval forward of the plan model(x) uses, so the result does not depend on `batch`; one host synchronisation per value.  A
    fixed shift is a roll of the raw chunk on the device in front of the kernel, which composes with a random shift of `base`.
    The module's `training` flag is left alone.  With `spectrogram` (any frontend.FrontEnd whose height x width is the
    image of the ViT) every impaired frame becomes its image in front of the model."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    enc, plan_of, K = _resolve(model)
    batch = _batch(batch)
    seed = _index(seed, "seed", 0, 2 ** 64 - 1)
    if base is None:
        base = Impairments()
    if not isinstance(base, Impairments):
        raise TypeError(f"base must be an Impairments or None, got {type(base).__name__}")
    settings = [_fixed(base, kind, v) for v in values]
    geom = enc._geom
    own = "vit" if geom["kind"] == 0 else "rawiq"
    if layout is None:
        layout = own
    if layout != own:
        raise ValueError(f"layout {layout!r} does not fit a {type(model).__name__} (its input layout is {own!r})")
    if not isinstance(raw, torch.Tensor) or raw.dim() != 3 or raw.shape[2] != 2:
        raise ValueError(f"raw must be a (N, len, 2) tensor, got {tuple(raw.shape) if hasattr(raw, 'shape') else raw!r}")
    n, length = raw.shape[0], raw.shape[1]
    h, w = (geom["img_h"], geom["img_w"]) if own == "vit" else (0, 0)
    spec = front_end(spectrogram, layout, length)
    if spec is None:
        _take(layout, length, h, w)
    elif (spec.height, spec.width) != (h, w):
        raise ValueError(f"the spectrogram is {spec.height}x{spec.width}, the model's image {h}x{w}")
    for _, roll in settings:
        if roll >= max(length, 1):
            raise ValueError(f"shift {roll} must be below the frame length {length}")
    st = _stats4(stats)
    stats = {"i_mean": st[0], "i_std": st[1], "q_mean": st[2], "q_std": st[3]}
    lab = _classes(labels, n, K, "labels")
    if not raw.is_cuda:
        raise N.IqError("impairment_curve runs on the MI355X only: raw is a CPU tensor and there is no CPU fallback")
    raw = raw.contiguous().float()
    plan = plan_of()
    lab = lab.to(raw.device)
    out = []
    with torch.no_grad():
        for imp, roll in settings:
            correct = torch.zeros((), dtype=torch.int64, device=raw.device)
            for i in range(0, n, batch):
                chunk = raw[i:i + batch]
                if roll:
                    chunk = torch.roll(chunk, -roll, dims=1)
                x = enc._expect(impair(chunk, stats, layout, imp, seed=seed, step=0, frame_base=i, h=h, w=w, spectrogram=spec))
                correct += (_forward(plan, x).argmax(1) == lab[i:i + batch]).sum()
            out.append(correct.item() / max(1, n))
    return out
