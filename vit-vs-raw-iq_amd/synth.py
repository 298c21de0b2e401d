"""Labelled synthetic I/Q frames made on the device, as a stream: the transmitter in front of the channel of impairments.py.

data.make_dataset is a per-frame numpy loop on the host; the native trainer consumes frames several hundred times faster than it
makes them.  Here one HIP kernel (csrc/synth.hip, iq_frames_synth) makes a batch of RAW (B, len, 2) frames, their labels and
their SNRs in HBM, in the layout iq_frames_preprocess / iq_frames_impair read: every training step and every evaluation can
have frames that were never seen, with no host data and no H2D copy.  The recipe is make_dataset's, at 1 sample per symbol:

  1. symbols of the frame's class: a point of its constellation per sample (data.constellation), the GMSK approximation of
     data._frame (+-pi/2 phase steps smoothed over 3 symbols) or OQPSK (I and Q change on alternate samples)
  2. one carrier phase theta ~ U[0, 2 pi) for the frame          3. divide by sqrt(mean |s|^2 + 1e-12) of the frame
  4. complex AWGN, sigma = sqrt(0.5 * 10^(-snr/10)) per component

It follows the recipe, not make_dataset's numbers: the draws come from Philox4x32-7, not from numpy's PCG64.  Frame j of a
stream is a pure function of (seed, stream, j) -- key (seed lo, seed hi ^ j hi), counter (c, j lo, IQ_SITE_SYNTH, stream), the
layout is written out in include/iqvit.h -- so a frame is the same whatever the batch size and however the stream is cut into
calls, streams 0 (training), 1 (validation), ... are disjoint, and a third party can restate any frame exactly.  With
balanced=True frame j has class j % K and SNR index (j // K) % n_snrs, make_dataset's pattern; otherwise both are drawn.
There is no CPU path; `synth_reference` is the host fp64 DEFINITION of the noiseless frame the tests compare against.

  FrameSynth(classes, snrs_db, length, seed, balanced, device)       .generate(n, frame_base, stream) -> (raw, y, z); .stats()
  synth_reference(symbols, drawn, synth)                            host fp64, everything but the noise
  SynthStream(synth, stats, layout, batch, h, w, stream, augment)   .get(step) -> (x, y, z) in the model's layout; .batches(n)
  train_on_stream(trainer, stream, steps, first_step)               FusedTrainer.step on fresh batches, no host sync
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from . import data as D
from ._args import MAX_LENGTH, _flag, _index, _number
from .frontend import front_end
from .impairments import Impairments, _stats4, _take

KIND_POINTS, KIND_GMSK, KIND_OQPSK = 0, 1, 2
SHAPED = {"GMSK": KIND_GMSK, "OQPSK": KIND_OQPSK}
MAX_CLASSES, MAX_SNRS = 128, 64      # IQ_SYNTH_MAX_CLASSES, IQ_SYNTH_MAX_SNRS


def _points(name, pts):
    try:
        c = np.asarray(pts, dtype=np.complex128).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError(f"class {name!r}: the constellation must be an array of complex points, got {pts!r}") from None
    if c.size == 0:
        raise ValueError(f"class {name!r}: the constellation is empty")
    if not np.all(np.isfinite(c.real) & np.isfinite(c.imag)):
        raise ValueError(f"class {name!r}: the constellation has a non-finite point")
    p = float(np.mean(np.abs(c) ** 2))
    if not p > 0:
        raise ValueError(f"class {name!r}: the constellation has no power")
    return c / math.sqrt(p)


class FrameSynth:
    """The source.  classes: names data.constellation knows plus 'GMSK' and 'OQPSK', or {name: complex array} for constellations
    of one's own (a value of None takes the named recipe); every constellation is scaled to unit mean power in fp64 and then
    rounded to the fp32 table the kernel reads.  snrs_db: the SNR values in dB, None or () for noiseless frames.  Arguments are
    checked here, before any device work; the table goes to `device` at the first generate()."""

    _drawn_columns = 4
    _no_cpu = ("FrameSynth.generate runs on the MI355X only: there is no CPU fallback "
               "(synth_reference is the host definition used by the tests)")

    def __init__(self, classes=D.CLASSES, snrs_db=D.SNRS_DB, length: int = 1024, seed: int = 0, balanced: bool = True,
                 device="cuda"):
        items = list(classes.items()) if isinstance(classes, dict) else [(c, None) for c in classes]
        if not items:
            raise ValueError("classes is empty")
        if len(items) > MAX_CLASSES:
            raise ValueError(f"at most {MAX_CLASSES} classes, got {len(items)}")
        self.class_names, self.descriptors, tables, off = [], [], [], 0
        for name, pts in items:
            if not isinstance(name, str):
                raise TypeError(f"class names must be strings, got {name!r}")
            if name in self.class_names:
                raise ValueError(f"class {name!r} is listed twice")
            if pts is None and name in SHAPED:
                desc = (SHAPED[name], 0, 0)
            else:
                if pts is None:
                    try:
                        pts = D.constellation(name)
                    except KeyError:
                        raise ValueError(f"unknown class {name!r}: not a name of data.constellation, 'GMSK' or 'OQPSK'") from None
                c = _points(name, pts)
                desc = (KIND_POINTS, off, len(c))
                tables.append(c)
                off += len(c)
            self.class_names.append(name)
            self.descriptors.append(desc)
        pts64 = np.concatenate(tables) if tables else np.zeros(0, np.complex128)
        self.points = np.stack([pts64.real, pts64.imag], axis=1).astype(np.float32)           # (P, 2): the kernel's table
        snrs = [] if snrs_db is None else [_number(v, "snrs_db entry") for v in snrs_db]
        if len(snrs) > MAX_SNRS:
            raise ValueError(f"at most {MAX_SNRS} SNR values, got {len(snrs)}")
        self.snrs_db = tuple(snrs)
        self.length = _index(length, "length", 1, MAX_LENGTH)
        self.n_symbols = self.length                 # columns of `symbols`
        self.seed = _index(seed, "seed", 0, 2 ** 64 - 1)
        self.balanced = _flag(balanced, "balanced")
        self.device = torch.device(device)
        self._classes_c = (N.SynthClass * len(self.descriptors))(*[N.SynthClass(*d) for d in self.descriptors])
        self._snrs_c = (C.c_float * max(1, len(snrs)))(*snrs)
        self._points_dev = None

    @property
    def n_classes(self):
        return len(self.descriptors)

    def struct(self, frame_base=0, stream=0, points=None) -> N.Synth:
        """The iq_synth_t of one call (`points`: the device address of the table)."""
        return N.Synth(points=points, classes=self._classes_c, n_classes=len(self.descriptors), snrs_db=self._snrs_c,
                       n_snrs=len(self.snrs_db), balanced=int(self.balanced), seed=self.seed,
                       stream=_index(stream, "stream", 0, 2 ** 32 - 1), frame_base=_index(frame_base, "frame_base", 0, 2 ** 64 - 1))

    def generate(self, n, frame_base=0, stream=0, return_drawn=False, return_symbols=False):
        """Frames [frame_base, frame_base + n) of `stream` -> (raw (n, len, 2) fp32, y (n,) int64, z (n,) fp32 SNR in dB, NaN
        without noise), all on the device; then, if asked for, drawn (n, 4) fp32 = {class, snr_db, theta, mean |s|^2 before
        the normalisation} and symbols (n, len) int32 (constellation index; GMSK: phase in units of pi/8; OQPSK: 2 I + Q)."""
        return self._generate(n, frame_base, stream, return_drawn, return_symbols)

    def _generate(self, n, frame_base, stream, return_drawn, return_symbols, **extra):
        """generate() of this class and of its subclasses: the checks, the outputs every generator has, _launch, the tuple."""
        n = _index(n, "n", 0, 2 ** 31 - 1)
        par = self.struct(frame_base, stream)
        if self.device.type != "cuda":
            raise N.IqError(self._no_cpu)
        d = self.device
        raw = torch.empty(n, self.length, 2, dtype=torch.float32, device=d)
        y = torch.empty(n, dtype=torch.int64, device=d)
        z = torch.empty(n, dtype=torch.float32, device=d)
        drawn = torch.empty(n, self._drawn_columns, dtype=torch.float32, device=d) if return_drawn else None
        symbols = torch.empty(n, self.n_symbols, dtype=torch.int32, device=d) if return_symbols else None
        more = self._launch(par, n, raw, y, z, drawn, symbols, **extra)
        return (raw, y, z) + tuple(t for t in (drawn, symbols) + more if t is not None)

    def _points_ptr(self):
        if self._points_dev is None:
            self._points_dev = torch.from_numpy(self.points if len(self.points) else np.zeros((1, 2), np.float32)).to(self.device)
        return self._points_dev.data_ptr()

    def _launch(self, par, n, raw, y, z, drawn, symbols):
        """The tables to the device at the first call, then the kernel (n > 0) -> the further outputs of a subclass."""
        par.points = self._points_ptr()
        if n > 0:
            N.check(N.lib().iq_frames_synth(raw.data_ptr(), y.data_ptr(), z.data_ptr(), N.ptr(drawn), N.ptr(symbols), n,
                                            self.length, C.byref(par), torch.cuda.current_stream(self.device).cuda_stream),
                    "iq_frames_synth")
        return ()

    def stats(self, n_subset: int = 5000, stream: int = 0):
        """{'i_mean','i_std','q_mean','q_std'} as data.normalization_stats computes them (fp32 values, unbiased std floored at
        1e-8), from the first n_subset frames of `stream`.  One host synchronisation."""
        n_subset = _index(n_subset, "n_subset", 1, 2 ** 31 - 1)
        raw = self.generate(n_subset, 0, stream)[0]
        i_all, q_all = raw[:, :, 0].flatten(), raw[:, :, 1].flatten()
        std = (lambda v: max(v.std().item(), 1e-8) if v.numel() > 1 else 1e-8)
        return {"i_mean": i_all.mean().item(), "i_std": std(i_all), "q_mean": q_all.mean().item(), "q_std": std(q_all)}

    def __repr__(self):
        return (f"FrameSynth(classes={self.class_names!r}, snrs_db={self.snrs_db!r}, length={self.length}, seed={self.seed}, "
                f"balanced={self.balanced})")


def synth_reference(symbols, drawn, synth: FrameSynth):
    """The noiseless frames in fp64 on the host, from the kernel's own `symbols` (n, len) and `drawn` (n, 4; the class and theta
    columns are used): table lookup (the fp32 table, GMSK exp(j pi sym / 8), OQPSK (+-1 +- j) / sqrt 2), rotation by theta,
    division by sqrt(mean |s|^2 + 1e-12).  -> float64 array (n, len, 2)."""
    to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)   # noqa: E731
    if not isinstance(synth, FrameSynth):
        raise TypeError(f"synth must be a FrameSynth, got {type(synth).__name__}")
    sym = to_np(symbols).astype(np.int64)
    d = to_np(drawn).astype(np.float64).reshape(-1, 4)
    if sym.ndim != 2 or len(d) != len(sym):
        raise ValueError(f"symbols must be (n, len) and drawn (n, 4), got {sym.shape} and {d.shape}")
    table = synth.points[:, 0].astype(np.float64) + 1j * synth.points[:, 1].astype(np.float64)
    out = np.empty(sym.shape + (2,), np.float64)
    for i in range(len(sym)):
        k = int(d[i, 0])
        if not 0 <= k < synth.n_classes or k != d[i, 0]:
            raise ValueError(f"frame {i}: class {d[i, 0]!r} is not one of the {synth.n_classes} classes")
        kind, off, count = synth.descriptors[k]
        s = sym[i]
        if kind == KIND_POINTS:
            if s.min(initial=0) < 0 or s.max(initial=0) >= count:
                raise ValueError(f"frame {i}: symbol outside [0, {count}) of class {synth.class_names[k]!r}")
            v = table[off + s]
        elif kind == KIND_GMSK:
            v = np.exp(1j * np.pi * (s % 16) / 8)
        else:
            v = ((2 * (s >> 1) - 1) + 1j * (2 * (s & 1) - 1)) / np.sqrt(2)
        v = v * np.exp(1j * d[i, 2])
        v = v / np.sqrt(np.mean(np.abs(v) ** 2) + 1e-12)
        out[i, :, 0], out[i, :, 1] = v.real, v.imag
    return out


class _Batches:
    """`count` consecutive batches of a SynthStream from `first`, as (x, y, z) triples: what evaluate_model_with_confusion
    iterates over.  Can be iterated again: the frames are the same."""

    def __init__(self, stream, count, first):
        self.stream, self.count, self.first = stream, count, first

    def __len__(self):
        return self.count

    def __iter__(self):
        for s in range(self.first, self.first + self.count):
            yield self.stream.get(s)


class SynthStream:
    """Batches of a FrameSynth stream as model input: get(step) makes frames [step * batch, (step + 1) * batch) of `stream` and
    passes them through iq_frames_preprocess (z-score with `stats`, layout 'vit' (B, 1, h, w) or 'rawiq' (B, 2, len)) or, with
    `augment` (an impairments.Impairments), through iq_frames_impair with the synth's seed, step word = `stream` and the same
    frame_base.  With `spectrogram` (any frontend.FrontEnd; layout 'vit') that launch keeps the whole frame (take = len) and
    the front end follows: x is its (batch, channels, height, width) image, h and w are not used.  All on the current stream of
    the device, no host synchronisation."""

    def __init__(self, synth: FrameSynth, stats, layout: str, batch: int, h: int = 32, w: int = 64, stream: int = 0,
                 augment=None, spectrogram=None):
        if not isinstance(synth, FrameSynth):
            raise TypeError(f"synth must be a FrameSynth, got {type(synth).__name__}")
        self.synth, self.layout, self.h, self.w = synth, layout, h, w
        self._stats = (C.c_float * 4)(*_stats4(stats))
        self.spectrogram = front_end(spectrogram, layout, synth.length)
        if self.spectrogram is None:
            self.take = _take(layout, synth.length, h, w)
        else:
            self.take, self.h, self.w = synth.length, self.spectrogram.height, self.spectrogram.width
        self.batch = _index(batch, "batch", 1, 2 ** 31 - 1)
        self.stream = _index(stream, "stream", 0, 2 ** 32 - 1)
        if augment is not None:
            if not isinstance(augment, Impairments):
                raise TypeError(f"augment must be an Impairments or None, got {type(augment).__name__}")
            if augment.shift_max >= synth.length:
                raise ValueError(f"augment.shift_max {augment.shift_max} must be below the frame length {synth.length}")
        self.augment = augment

    def get(self, step):
        """-> (x in the model's layout, y (batch,) int64, z (batch,) fp32 SNR in dB) of batch `step`, device tensors."""
        base = _index(step, "step", 0) * self.batch
        raw, y, z = self.synth.generate(self.batch, base, self.stream)
        B, length = raw.shape[0], raw.shape[1]
        out = torch.empty(B, 2, self.take, dtype=torch.float32, device=raw.device)
        st = torch.cuda.current_stream(raw.device).cuda_stream
        if self.augment is None:
            N.check(N.lib().iq_frames_preprocess(raw.data_ptr(), out.data_ptr(), B, length, self.take, self._stats, st),
                    "iq_frames_preprocess")
        else:
            par = self.augment.struct(self.synth.seed, self.stream, base)
            N.check(N.lib().iq_frames_impair(raw.data_ptr(), out.data_ptr(), None, B, length, self.take, self._stats,
                                             C.byref(par), st), "iq_frames_impair")
        if self.spectrogram is not None:
            return self.spectrogram(out), y, z
        return (out.view(B, 1, self.h, self.w) if self.layout == "vit" else out), y, z

    def batches(self, count, first_step=0):
        """An iterable over batches first_step .. first_step + count - 1."""
        return _Batches(self, _index(count, "count", 0), _index(first_step, "first_step", 0))


def train_on_stream(trainer, stream: SynthStream, steps, first_step=0):
    """`steps` FusedTrainer.step calls on batches first_step .. first_step + steps - 1 of `stream`: every step sees frames that
    were never used.  Nothing here synchronises with the host; with use_graph=True the trainer copies each batch into the static
    buffers of its captured step, so generation stays outside the graph.  -> the step index to continue from."""
    if not isinstance(stream, SynthStream):
        raise TypeError(f"stream must be a SynthStream, got {type(stream).__name__}")
    steps, first_step = _index(steps, "steps", 0), _index(first_step, "first_step", 0)
    for s in range(first_step, first_step + steps):
        x, y, _ = stream.get(s)
        trainer.step(x, y)
    return first_step + steps
