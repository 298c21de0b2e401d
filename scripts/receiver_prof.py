"""What the receiver costs ("Receiver"): microseconds per batch of 256 frames for iq_frames_receive at 1024 and at
8192 samples (8 samples per symbol, an 8-symbol root-raised cosine, 32 fractional phases) in its three timing modes, for
GIVEN mode without the sample-rate pass (no est, no energy: the symbol pass alone), for the backward, for a ReceivedSynth
batch (waveform + receive) and a SynthStream batch of it (+ iq_frames_preprocess), beside iq_frames_waveform making the same
frames and, measured in the same process, the cfg C training step (bench.py's raw-IQ geometry: seg16 d128 h8 L6 F1024, batch
256, dropout 0.2, hipGraph replay) on a fixed batch.  Device events around a train of calls, legs interleaved over rounds so
that clock and neighbour drift hits all alike; median (min).  Writes the table to --out (default profiles/receiver.txt),
keeping whatever follows the line "---" in an existing file (notes recorded by hand)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vit_vs_raw_iq_amd as P  # noqa: E402
from vit_vs_raw_iq_amd import ReceivedSynth, Receiver, ShapedSynth, SynthStream  # noqa: E402
from vit_vs_raw_iq_amd.trainer import FusedTrainer  # noqa: E402

CFG_C = dict(in_channels=2, seq_length=1024, num_classes=19, d_model=128, n_head=8, n_layers=6, ffn_hidden=1024,
             use_cls_token=True, embedding_type="segment", segment_size=16)


def train_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "receiver.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    batch = 256
    legs = []
    for length in (1024, 8192):
        ws = ShapedSynth(length=length, seed=1, sps=8, span=8, n_phase=32, taps=3)
        raw = ws.generate(batch, 0, 0)[0]
        om, en, gv = (Receiver.for_synth(ws, timing=t) for t in ("oerder_meyr", "energy", "given"))
        rs = ReceivedSynth(ws, om)
        x = raw.clone().requires_grad_()
        w = torch.randn(batch, length // 8, 2, device=d)
        tag = f"{batch} x {length}: "
        legs += [(tag + "iq_frames_waveform", lambda ws=ws: ws.generate(batch, 0, 0), 200),
                 (tag + "iq_frames_receive, oerder_meyr", lambda om=om, raw=raw: om(raw), 200),
                 (tag + "iq_frames_receive, energy", lambda en=en, raw=raw: en(raw), 200),
                 (tag + "iq_frames_receive, given + est", lambda gv=gv, raw=raw: gv(raw, return_est=True), 200),
                 (tag + "iq_frames_receive, given (symbol pass alone)", lambda gv=gv, raw=raw: gv(raw), 200),
                 (tag + "receive + iq_frames_receive_bwd", lambda om=om, x=x, w=w: torch.autograd.grad(om(x), x, w), 200),
                 (tag + "ReceivedSynth.generate (waveform + receive)", lambda rs=rs: rs.generate(batch, 0, 0), 200)]
        if length == 1024:
            stream = SynthStream(rs, rs.stats(n_subset=1024), "rawiq", batch)
            legs.append((tag + "SynthStream.get (+ iq_frames_preprocess)", lambda stream=stream: stream.get(0), 200))
    torch.manual_seed(0)
    model = P.AMCTransformerRawIQ(drop_prob=0.2, device="cuda", **CFG_C).to(d).train()
    tr = FusedTrainer(model, lr=1e-4, weight_decay=1e-4, use_graph=True, dropout_seed=1234)
    ws = ShapedSynth(length=1024, seed=1, sps=8, span=8, n_phase=32, taps=3)
    x0, y0, _ = SynthStream(ws, ws.stats(n_subset=1024), "rawiq", batch).get(0)
    legs.append(("cfg C step, fixed batch", lambda: tr.step(x0, y0), 100))
    for _, fn, calls in legs:                    # warm-up: code objects, graph capture, clocks
        train_ms(fn, calls)
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, calls in legs:
            times[name].append(train_ms(fn, calls))
    lines = [f"device: {torch.cuda.get_device_name(0)}; batches of {batch} frames, sps 8, span 8 (65 taps), 32 fractional phases; "
             f"device events around a train of calls, median (min) over {args.rounds} interleaved rounds",
             f"{'leg':<70} {'us/batch':>20}"]
    for name, _, _ in legs:
        lines.append(f"{name:<70} {1e3 * statistics.median(times[name]):>10.2f} ({1e3 * min(times[name]):>8.2f})")
    step = statistics.median(times["cfg C step, fixed batch"])
    for length in (1024, 8192):
        tag = f"{batch} x {length}: "
        rx, wf = statistics.median(times[tag + "iq_frames_receive, oerder_meyr"]), statistics.median(times[tag + "iq_frames_waveform"])
        lines.append(f"{tag}receive (oerder_meyr) / waveform: {rx / wf:.2f}; / cfg C step: {100 * rx / step:.1f} %")
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
