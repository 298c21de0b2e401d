"""What carrier recovery costs ("Carrier recovery"): milliseconds per batch of 256 planar frames for iq_frames_carrier
(estimate and derotate, M = 4, refined), for its GIVEN mode (derotation alone) and for iq_frames_carrier_bwd, at (len 128,
N 1024), (len 1024, N 2048) and (len 8192, N 8192).  Beside the times two floors: the DFT bound, 8 N (n1 + n2) flop per frame
(four real MFMA products per complex term of the two stages) at the 155 TF of the fp32-input MFMA, and the memory floor, the
frame read twice and written once (GIVEN and the backward: read once) at the HBM rate.  Device events around a train of
back-to-back calls, legs interleaved over rounds so that clock and neighbour drift hits all alike; median (min).  These are call
times -- launch gaps and the host's cost per call included -- not profiler kernel times.  Writes the table to --out (default
profiles/carrier.txt), keeping whatever follows the line "---" in an existing file (notes recorded by hand)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vit_vs_raw_iq_amd import Carrier  # noqa: E402

PEAK_F32_MFMA = 155e12
HBM_BYTES_PER_S = 8e12          # the MI355X's HBM3E rate
SHAPES = ((128, 1024), (1024, 2048), (8192, 8192))


def train_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(calls)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carrier.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    batch = 256
    legs, dft, mem = [], {}, {}
    for length, n_dft in SHAPES:
        cr = Carrier(length, order=4, n_dft=n_dft)
        g = torch.Generator().manual_seed(length)
        sym = torch.randint(0, 4, (batch, length), generator=g).double() * (torch.pi / 2) + torch.pi / 4
        ph = sym + 2 * torch.pi * 0.011 * torch.arange(length).double() + 0.7
        x = (torch.stack([ph.cos(), ph.sin()], dim=1) + 0.1 * torch.randn(batch, 2, length, generator=g).double()).float().to(d)
        out, fth = cr(x, return_fth=True)                    # uploads the tables
        xg = x.clone().requires_grad_(True)
        og = cr(xg)
        dout = torch.randn_like(og)

        def est(calls, cr=cr, x=x):
            with torch.no_grad():
                for _ in range(calls):
                    cr(x)

        def given(calls, cr=cr, x=x, fth=fth):
            with torch.no_grad():
                for _ in range(calls):
                    cr(x, fth=fth)

        def bwd(calls, og=og, xg=xg, dout=dout):
            for _ in range(calls):
                torch.autograd.grad(og, xg, dout, retain_graph=True)
        tag = f"len {length:>4}, N {cr.n1} x {cr.n2}"
        legs += [(f"carrier estimate + derotate  {tag}", est, 200), (f"carrier derotate (given)     {tag}", given, 400),
                 (f"carrier backward             {tag}", bwd, 200)]
        dft[legs[-3][0]] = 8.0 * cr.n_dft * (cr.n1 + cr.n2) * batch / PEAK_F32_MFMA * 1e3
        mem[legs[-3][0]] = 24.0 * length * batch / HBM_BYTES_PER_S * 1e3
        mem[legs[-2][0]] = mem[legs[-1][0]] = 16.0 * length * batch / HBM_BYTES_PER_S * 1e3
    for _, fn, calls in legs:                                # warm-up: code objects, clocks
        train_ms(fn, calls)
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, calls in legs:
            times[name].append(train_ms(fn, calls))
    lines = [f"device: {torch.cuda.get_device_name(0)}; batches of {batch} planar frames, M = 4, refined; device events around a train "
             f"of calls, median (min) over {args.rounds} interleaved rounds; DFT bound = 8 N (n1 + n2) flop per frame at "
             f"{PEAK_F32_MFMA / 1e12:.0f} TF (fp32-input MFMA), memory floor = the frames' bytes at {HBM_BYTES_PER_S / 1e12:.0f} TB/s",
             f"{'leg':<56} {'ms/batch':>18} {'DFT ms':>9} {'memory ms':>10}"]
    for name, _, _ in legs:
        line = f"{name:<56} {statistics.median(times[name]):>9.4f} ({min(times[name]):>7.4f})"
        line += f" {dft[name]:>9.4f}" if name in dft else f" {'':>9}"
        lines.append(line + f" {mem[name]:>10.5f}")
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
