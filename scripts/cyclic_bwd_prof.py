"""What the cyclic-spectrum adjoint costs ("Cyclic-spectrum front end"): per batch of 256 frames of 1024 samples, kind
'both', squared coherence, Hann, at the two geometries of scripts/cyclic_prof.py (n_fft 64 / hop 16 / 61 columns and n_fft 224 /
hop 56 / 15 columns), three legs each, measured as that script measures (its train_ms and kernel_ms):
  forward               cs(x) without grad: iq_frames_cyclic, for scale
  forward + backward    cs(x).backward(dout) through CyclicSpectrum(differentiable=True): iq_frames_cyclic, iq_frames_cyclic_bwd
  torch eager fwd+bwd   the script's eager statement of the operation (complex64) under torch autograd
The kernel ms column is that of cyclic_bwd_kernel alone (for the forward leg, of cyclic_kernel).  Numbers are recorded, not
asserted.  Writes the table to --out (default profiles/cyclic_bwd.txt), keeping whatever follows the line "---" in an existing
file (notes recorded by hand)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from cyclic_prof import Eager, kernel_ms, train_ms  # noqa: E402
from vit_vs_raw_iq_amd import CyclicSpectrum, FrameSynth, SynthStream  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cyclic_bwd.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cyclic_bwd_prof.py measures on an MI355X"
    d = torch.device("cuda:0")
    length, batch = 1024, 256
    fs = FrameSynth(length=length, seed=1)
    x = SynthStream(fs, fs.stats(n_subset=1024), "rawiq", batch).get(0)[0]
    legs, kernels = [], {}
    for n_fft in (64, 224):
        cs = CyclicSpectrum(n_fft, length, differentiable=True)
        eager = Eager(cs, d)
        dout = torch.randn(batch, 2, n_fft, n_fft, device=d, generator=torch.Generator(device=d).manual_seed(n_fft))

        def grad_of(f):
            xg = x.clone().requires_grad_(True)
            f(xg).backward(dout)
            return xg.grad
        ga, gb = grad_of(cs), grad_of(eager)
        diff = float((ga - gb).abs().max())
        top = float(gb.abs().max())

        def fwd(calls, cs=cs):
            with torch.no_grad():
                for _ in range(calls):
                    cs(x)

        def both(calls, cs=cs, dout=dout):
            xg = x.clone().requires_grad_(True)
            for _ in range(calls):
                cs(xg).backward(dout)
                xg.grad = None

        def tor(calls, eager=eager, dout=dout):
            xg = x.clone().requires_grad_(True)
            for _ in range(calls):
                eager(xg).backward(dout)
                xg.grad = None
        names = (f"cyclic forward         n_fft {n_fft} hop {cs.hop} T {cs.columns}",
                 f"cyclic fwd + bwd       n_fft {n_fft} (max |x.grad - eager| {diff:.1e} of {top:.1e})",
                 f"torch eager fwd + bwd  n_fft {n_fft}")
        legs += [(names[0], fwd, 200), (names[1], both, 50), (names[2], tor, 10)]
        kernels[names[0]], kernels[names[1]] = "cyclic_kernel", "cyclic_bwd_kernel"
    for _, fn, calls in legs:                    # warm-up: code objects, clocks, torch's algorithm choices
        train_ms(fn, calls)
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, calls in legs:
            times[name].append(train_ms(fn, calls))
    kms = {name: kernel_ms(fn, 20).get(kernels[name]) for name, fn, _ in legs if name in kernels}
    lines = [f"device: {torch.cuda.get_device_name(0)}; batches of {batch} frames of {length} complex samples, both channels, "
             f"coherence; call ms: device events around a train of calls, median (min) over {args.rounds} interleaved rounds; "
             "kernel ms: event pair around each launch of the leg's kernel, mean of 20",
             f"{'leg':<72} {'call ms':>18} {'kernel ms':>10}"]
    for name, _, _ in legs:
        line = f"{name:<72} {statistics.median(times[name]):>9.4f} ({min(times[name]):>7.4f})"
        if kms.get(name) is not None:
            line += f" {kms[name]:>10.4f}"
        lines.append(line)
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
