"""What the spectrogram front end costs beside a training step ("Spectrogram front end"): microseconds per batch of
256 frames of 1024 samples for iq_frames_spectrogram and iq_frames_spectrogram_bwd at cfg B's 224 x 224 image (hop 4, pad 46)
and at the reference's 32 x 64 image (hop 16, pad 8), their fraction of the fp32 MFMA peak (8 W n_fft^2 flop per frame forward,
twice that backward: the recomputation and the adjoint; peak 155 TF), and, measured in the same process, the cfg B training
step (bench.py's ViT-Tiny/16 224 x 224, batch 256, dropout 0.1, hipGraph replay) on a fixed batch and on a fresh spectrogram
batch per step (train_on_stream on SynthStream(..., spectrogram=spec)).  Device events around a train of back-to-back calls
(about 0.1 s per window), legs interleaved over rounds so that clock and neighbour drift hits all alike; median (min).  These are
call times -- launch gaps and, at 32 x 64, the host's cost per call included -- not profiler kernel times.  Writes the table to
--out (default profiles/spectrogram.txt), keeping whatever follows the line "---" in an existing file (notes recorded by hand)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vit_vs_raw_iq_amd as P  # noqa: E402
from vit_vs_raw_iq_amd import FrameSynth, Spectrogram, SynthStream, train_on_stream  # noqa: E402
from vit_vs_raw_iq_amd.trainer import FusedTrainer  # noqa: E402

CFG_B = dict(in_channels=1, img_size_h=224, img_size_w=224, patch_size=16, num_classes=19, d_model=192, n_head=3, n_layers=12,
             ffn_hidden=768)
PEAK_F32_MFMA = 155e12


def train_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(calls)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrogram.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    length, batch = 1024, 256
    fs = FrameSynth(length=length, seed=1)
    stats = fs.stats(n_subset=1024)
    x = SynthStream(fs, stats, "rawiq", batch).get(0)[0]
    legs, flops = [], {}
    for n_fft, width in ((224, 224), (32, 64)):
        spec = Spectrogram(n_fft, width, length)
        spec(x)                                             # uploads the table
        xg = x.clone().requires_grad_(True)
        img = spec(xg)
        dout = torch.randn_like(img)

        def fwd(calls, spec=spec):
            with torch.no_grad():
                for _ in range(calls):
                    spec(x)

        def bwd(calls, img=img, dout=dout, xg=xg):
            for _ in range(calls):
                torch.autograd.grad(img, xg, dout, retain_graph=True)
        tag = f"{n_fft}x{width} hop {spec.hop} pad {spec.pad}"
        legs += [(f"spectrogram forward  {tag}", fwd, 400), (f"spectrogram backward {tag}", bwd, 100)]
        flops[legs[-2][0]] = 8.0 * batch * width * n_fft * n_fft
        flops[legs[-1][0]] = 16.0 * batch * width * n_fft * n_fft
    torch.manual_seed(0)
    model = P.AMCTransformerViT(drop_prob=0.1, device="cuda", **CFG_B).to(d).train()
    tr = FusedTrainer(model, lr=1e-4, weight_decay=1e-3, use_graph=True, dropout_seed=1234)
    spec_b = Spectrogram.for_model(model, length).fit(x)
    stream = SynthStream(fs, stats, "vit", batch, spectrogram=spec_b)
    x0, y0, _ = stream.get(0)
    pos = {"train": 0}

    def fixed(calls):
        for _ in range(calls):
            tr.step(x0, y0)

    def fresh(calls):
        pos["train"] = train_on_stream(tr, stream, calls, pos["train"])
    legs += [("cfg B step, fixed batch", fixed, 40), ("cfg B step, fresh spectrogram batch (train_on_stream)", fresh, 40)]
    for _, fn, calls in legs:                    # warm-up: code objects, graph capture, clocks
        train_ms(fn, calls)
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, calls in legs:
            times[name].append(train_ms(fn, calls))
    lines = [f"device: {torch.cuda.get_device_name(0)}; batches of {batch} frames of {length} complex samples; device events "
             f"around a train of calls, median (min) over {args.rounds} interleaved rounds; peak = {PEAK_F32_MFMA / 1e12:.0f} TF "
             "fp32-input MFMA",
             f"{'leg':<56} {'ms/batch':>18} {'TF':>8} {'of peak':>8}"]
    for name, _, _ in legs:
        med = statistics.median(times[name])
        line = f"{name:<56} {med:>9.4f} ({min(times[name]):>7.4f})"
        if name in flops:
            tf = flops[name] / (med * 1e-3) / 1e12
            line += f" {tf:>8.2f} {100 * tf * 1e12 / PEAK_F32_MFMA:>7.1f}%"
        lines.append(line)
    step = statistics.median(times["cfg B step, fixed batch"])
    for name in flops:
        lines.append(f"{name} / cfg B step: {100 * statistics.median(times[name]) / step:.1f} %")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    notes = ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n---\n" in old:
            notes = old[old.index("\n---\n") + 1:]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + notes)


if __name__ == "__main__":
    main()
