"""What the constellation front end costs beside a training step ("Constellation front end"): milliseconds per batch
of 256 frames for iq_frames_constellation and iq_frames_constellation_bwd (gaussian sigma 1, radius 4, n_frac 8, log mode) at
cfg B's 224 x 224 image from 1024 z-scored points and at the reference's 32 x 64 image from 128 points, the worst case (an
all-zero batch: every point in one pixel, the list of its tile is the whole frame) at 224 x 224, and, measured in the same
process, the cfg B training step (bench.py's ViT-Tiny/16 224 x 224, batch 256, dropout 0.1, hipGraph replay) on a fixed batch and
on a fresh constellation batch per step (train_on_stream on SynthStream(..., spectrogram=con)).  Beside the times two floors:
the DENSE bound 2 len H W n_frames flop at the 155 TF of the fp32-input MFMA (what a chain over all points would cost at peak --
the compaction has to beat it to earn its keep) and the WRITE floor, the image's bytes at the HBM rate.  Device events around a
train of back-to-back calls, legs interleaved over rounds so that clock and neighbour drift hits all alike; median (min).  These
are call times -- launch gaps and the host's cost per call included -- not profiler kernel times.  Writes the table to --out
(default profiles/constellation.txt), keeping whatever follows the line "---" in an existing file (notes recorded by hand)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vit_vs_raw_iq_amd as P  # noqa: E402
from vit_vs_raw_iq_amd import Constellation, FrameSynth, SynthStream, train_on_stream  # noqa: E402
from vit_vs_raw_iq_amd.trainer import FusedTrainer  # noqa: E402

CFG_B = dict(in_channels=1, img_size_h=224, img_size_w=224, patch_size=16, num_classes=19, d_model=192, n_head=3, n_layers=12,
             ffn_hidden=768)
PEAK_F32_MFMA = 155e12
HBM_BYTES_PER_S = 8e12          # the MI355X's HBM3E rate


def train_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(calls)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constellation.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    batch = 256
    legs, dense, write = [], {}, {}
    streams = {}
    for height, width, length in ((224, 224, 1024), (32, 64, 128)):
        fs = FrameSynth(length=length, seed=1)
        stats = fs.stats(n_subset=1024)
        streams[length] = (fs, stats)
        x = SynthStream(fs, stats, "rawiq", batch).get(0)[0]
        inputs = [("synth frames", x)]
        if height == 224:
            inputs.append(("all-zero batch (worst case)", torch.zeros_like(x)))
        con = Constellation(height, width, length, profile="gaussian", sigma=1.0, radius=4, n_frac=8, mode="log")
        for what, xin in inputs:
            con(xin)                                            # uploads the table
            xg = xin.clone().requires_grad_(True)
            img = con(xg)
            dout = torch.randn_like(img)

            def fwd(calls, con=con, xin=xin):
                with torch.no_grad():
                    for _ in range(calls):
                        con(xin)

            def bwd(calls, img=img, dout=dout, xg=xg):
                for _ in range(calls):
                    torch.autograd.grad(img, xg, dout, retain_graph=True)
            tag = f"{height}x{width} from {length} points, {what}"
            worst = what != "synth frames"
            legs += [(f"constellation forward  {tag}", fwd, 40 if worst else 400),
                     (f"constellation backward {tag}", bwd, 20 if worst else 100)]
            for name in (legs[-2][0], legs[-1][0]):
                dense[name] = 2.0 * length * height * width * batch / PEAK_F32_MFMA * 1e3
                write[name] = 4.0 * height * width * batch / HBM_BYTES_PER_S * 1e3
    torch.manual_seed(0)
    model = P.AMCTransformerViT(drop_prob=0.1, device="cuda", **CFG_B).to(d).train()
    tr = FusedTrainer(model, lr=1e-4, weight_decay=1e-3, use_graph=True, dropout_seed=1234)
    fs, stats = streams[1024]
    x = SynthStream(fs, stats, "rawiq", batch).get(0)[0]
    con_b = Constellation.for_model(model, 1024).fit(x)
    stream = SynthStream(fs, stats, "vit", batch, spectrogram=con_b)
    x0, y0, _ = stream.get(0)
    pos = {"train": 0}

    def fixed(calls):
        for _ in range(calls):
            tr.step(x0, y0)

    def fresh(calls):
        pos["train"] = train_on_stream(tr, stream, calls, pos["train"])
    legs += [("cfg B step, fixed batch", fixed, 40), ("cfg B step, fresh constellation batch (train_on_stream)", fresh, 40)]
    for _, fn, calls in legs:                    # warm-up: code objects, graph capture, clocks
        train_ms(fn, calls)
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, calls in legs:
            times[name].append(train_ms(fn, calls))
    lines = [f"device: {torch.cuda.get_device_name(0)}; batches of {batch} frames; gaussian sigma 1, radius 4, n_frac 8, log mode; "
             f"device events around a train of calls, median (min) over {args.rounds} interleaved rounds; dense bound = 2 len H W "
             f"n_frames flop at {PEAK_F32_MFMA / 1e12:.0f} TF (fp32-input MFMA), write floor = the image's bytes at "
             f"{HBM_BYTES_PER_S / 1e12:.0f} TB/s",
             f"{'leg':<72} {'ms/batch':>18} {'dense ms':>9} {'write ms':>9} {'t/dense':>8}"]
    for name, _, _ in legs:
        med = statistics.median(times[name])
        line = f"{name:<72} {med:>9.4f} ({min(times[name]):>7.4f})"
        if name in dense:
            line += f" {dense[name]:>9.4f} {write[name]:>9.4f} {med / dense[name]:>8.2f}"
        lines.append(line)
    step = statistics.median(times["cfg B step, fixed batch"])
    for name in dense:
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
