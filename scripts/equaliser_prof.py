"""What the blind equaliser costs ("Blind equaliser"): milliseconds per batch of 256 frames for iq_frames_equalise at
the defaults (11 taps, 64 steps), for its GIVEN mode (the filter alone) and for iq_frames_equalise_bwd, at 128, 1024 and 8192
symbols, next to the receiver's launch that makes the same batch of symbols from sps = 2 frames.  Device events around a train of
back-to-back calls, legs interleaved over rounds so that clock and neighbour drift hits all alike; median (min).  These are call
times -- launch gaps and the host's cost per call included -- not profiler kernel times, and nothing is claimed from them.
Ahead of the table, the drift of a whole run against the fp64 definition on the frames of tests/equaliser_ref.py (GPU test 5),
in units of the derived one-step bound.  Writes to --out (default profiles/equaliser.txt), keeping whatever follows the line
"---" in an existing file (notes recorded by hand)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import equaliser_ref as R  # noqa: E402
from vit_vs_raw_iq_amd import Equaliser, Receiver, equaliser_reference  # noqa: E402

LENGTHS = (128, 1024, 8192)
SPS = 2


def train_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(calls)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def drift_lines(d):
    lines = []
    for name in R.RUNS:
        xs = R.run_frames(name)
        z = R.to_complex(xs)
        eq = Equaliser(z.shape[1])
        mu = float(np.float32(eq.mu))
        w = eq(torch.from_numpy(xs).to(d), return_w=True)[1].cpu().numpy().astype(np.float64)
        w_ref = equaliser_reference(xs, eq.taps, eq.iters, mu)[1]
        allowed, step = R.run_bound(z, R.spike(len(z), eq.taps), mu, 1.0, eq.iters)
        drift = R.norm2((w - w_ref)[:, :, 0] + 1j * (w - w_ref)[:, :, 1])
        lines.append(f"drift after {eq.iters} steps, {name:<10} ||w - w_fp64||_2 max {drift.max():.3e} = {float((drift / step).max()):.2f} "
                     f"one-step bounds ({eq.iters} allowed)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equaliser.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    batch = 256
    legs = []
    for length in LENGTHS:
        g = torch.Generator().manual_seed(length)
        ph = torch.randint(0, 4, (batch, length), generator=g).double() * (torch.pi / 2) + torch.pi / 4
        a = torch.polar(torch.ones_like(ph), ph)
        zc = a + 0.3 * torch.roll(a, 1, 1) - 0.15j * torch.roll(a, 2, 1)
        zc = zc / zc.abs().pow(2).mean(dim=1, keepdim=True).sqrt()
        x = (torch.view_as_real(zc) + 0.05 * torch.randn(batch, length, 2, generator=g).double()).float().to(d)
        eq = Equaliser(length)
        out, w = eq(x, return_w=True)
        xg = x.clone().requires_grad_(True)
        og = eq(xg)
        dout = torch.randn_like(og)
        raw_len = min(length * SPS, 8192)                    # the receiver's frame is bounded like every frame: 8192 samples
        rx = Receiver(SPS, timing="energy")
        raw = torch.randn(batch, raw_len, 2, generator=g).float().to(d)
        rx(raw)

        def fwd(calls, eq=eq, x=x):
            with torch.no_grad():
                for _ in range(calls):
                    eq(x)

        def given(calls, eq=eq, x=x, w=w):
            with torch.no_grad():
                for _ in range(calls):
                    eq(x, w=w)

        def bwd(calls, og=og, xg=xg, dout=dout):
            for _ in range(calls):
                torch.autograd.grad(og, xg, dout, retain_graph=True)

        def recv(calls, rx=rx, raw=raw):
            with torch.no_grad():
                for _ in range(calls):
                    rx(raw)
        tag = f"len {length:>4}"
        legs += [(f"equaliser, {eq.taps} taps, {eq.iters} steps   {tag}", fwd, 50), (f"equaliser, given weights     {tag}", given, 200),
                 (f"equaliser backward           {tag}", bwd, 200), (f"receiver, {raw_len:>4} samples sps {SPS} {tag}", recv, 200)]
    for _, fn, calls in legs:                                # warm-up: code objects, clocks
        train_ms(fn, calls)
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, calls in legs:
            times[name].append(train_ms(fn, calls))
    lines = drift_lines(d)
    lines += [f"device: {torch.cuda.get_device_name(0)}; batches of {batch} frames (B, len, 2); device events around a train of calls, "
              f"median (min) over {args.rounds} interleaved rounds",
              f"{'leg':<48} {'ms/batch':>18}"]
    for name, _, _ in legs:
        lines.append(f"{name:<48} {statistics.median(times[name]):>9.4f} ({min(times[name]):>7.4f})")
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
