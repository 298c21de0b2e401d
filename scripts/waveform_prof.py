"""What the shaped frame source costs beside a training step ("Shaped frame source"): milliseconds per batch of 256
frames of 1024 samples at the task shape (19 classes, 4 SNRs, 8 samples per symbol, an 8-symbol root-raised cosine, 32 timing
phases, 3 channel taps) for iq_frames_waveform alone, for waveform + iq_frames_impair with the full training augmentation, and
for waveform + iq_frames_preprocess + the 224 x 224 spectrogram -- the forms SynthStream.get() takes -- beside iq_frames_synth
at the same length and, measured in the same process, the cfg C training step (bench.py's raw-IQ geometry: seg16 d128 h8 L6
F1024, batch 256, dropout 0.2, hipGraph replay) on a fixed batch and on a fresh shaped batch per step (train_on_stream).  Device
events around a train of calls, legs interleaved over rounds so that clock and neighbour drift hits all alike; median (min).
Writes the table to --out (default profiles/waveform.txt), keeping whatever follows the line "---" in an existing file (notes
recorded by hand)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vit_vs_raw_iq_amd as P  # noqa: E402
from vit_vs_raw_iq_amd import FrameSynth, Impairments, ShapedSynth, Spectrogram, SynthStream, train_on_stream  # noqa: E402
from vit_vs_raw_iq_amd.trainer import FusedTrainer  # noqa: E402

CFG_C = dict(in_channels=2, seq_length=1024, num_classes=19, d_model=128, n_head=8, n_layers=6, ffn_hidden=1024,
             use_cls_token=True, embedding_type="segment", segment_size=16)


def train_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(calls)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waveform.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    length, batch = 1024, 256
    ws = ShapedSynth(length=length, seed=1, sps=8, span=8, n_phase=32, taps=3)
    one = ShapedSynth(length=length, seed=1, sps=8, span=8, n_phase=32, taps=1)
    fs = FrameSynth(length=length, seed=1)
    stats = ws.stats(n_subset=1024)
    plain = SynthStream(ws, stats, "rawiq", batch)
    aug = SynthStream(ws, stats, "rawiq", batch, augment=Impairments.augmentation(length))
    spec = SynthStream(ws, stats, "vit", batch, spectrogram=Spectrogram(224, 224, length=length))
    torch.manual_seed(0)
    model = P.AMCTransformerRawIQ(drop_prob=0.2, device="cuda", **CFG_C).to(d).train()
    tr = FusedTrainer(model, lr=1e-4, weight_decay=1e-4, use_graph=True, dropout_seed=1234)
    x0, y0, _ = plain.get(0)
    pos = {}

    def loop(key, body):
        pos[key] = 0

        def go(calls):
            for s in range(pos[key], pos[key] + calls):
                body(s)
            pos[key] += calls
        return go

    def fixed(calls):
        for _ in range(calls):
            tr.step(x0, y0)

    legs = [("iq_frames_synth (1 sample per symbol)", loop("synth", lambda s: fs.generate(batch, s * batch, 0)), 400),
            ("iq_frames_waveform", loop("gen", lambda s: ws.generate(batch, s * batch, 0)), 400),
            ("iq_frames_waveform, 1 tap", loop("one", lambda s: one.generate(batch, s * batch, 0)), 400),
            ("waveform + iq_frames_preprocess", loop("plain", plain.get), 400),
            ("waveform + iq_frames_impair (augmentation)", loop("aug", aug.get), 400),
            ("waveform + preprocess + spectrogram 224x224", loop("spec", spec.get), 100),
            ("cfg C step, fixed batch", fixed, 100),
            ("cfg C step, fresh shaped batch (train_on_stream)", loop("train", lambda s: train_on_stream(tr, plain, 1, s)), 100)]
    for _, fn, calls in legs:                    # warm-up: code objects, graph capture, clocks
        train_ms(fn, calls)
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, calls in legs:
            times[name].append(train_ms(fn, calls))
    lines = [f"device: {torch.cuda.get_device_name(0)}; batches of {batch} frames of {length} complex samples, 19 classes, 4 SNRs, "
             f"sps 8, span 8, 32 timing phases, 3 taps; device events around a train of calls, median (min) over {args.rounds} "
             f"interleaved rounds",
             f"{'leg':<50} {'ms/batch':>18}"]
    for name, _, _ in legs:
        lines.append(f"{name:<50} {statistics.median(times[name]):>9.4f} ({min(times[name]):>7.4f})")
    step = statistics.median(times["cfg C step, fixed batch"])
    for name in ("iq_frames_synth (1 sample per symbol)", "iq_frames_waveform", "waveform + iq_frames_preprocess",
                 "waveform + iq_frames_impair (augmentation)"):
        lines.append(f"{name} / cfg C step: {100 * statistics.median(times[name]) / step:.1f} %")
    lines.append(f"{'frames':>7} {'iq_frames_waveform alone':<30} {'us/launch':>18} {'GB/s algorithmic':>18}")
    for n, calls in ((256, 400), (32768, 20)):
        gen = loop(f"gen{n}", lambda s, n=n: ws.generate(n, s * n, 0))
        train_ms(gen, calls)
        t = [1e3 * train_ms(gen, calls) for _ in range(args.rounds)]
        med, lo, nbytes = statistics.median(t), min(t), n * length * 8
        lines.append(f"{n:>7} {'':<30} {med:>9.2f} ({lo:>6.2f}) {nbytes / med / 1e3:>9.0f} ({nbytes / lo / 1e3:>6.0f})")
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
