"""What the likelihood classifier costs ("Likelihood classifier"): microseconds per launch of iq_frames_likelihood at
B = 256 frames, the 17 table classes (812 points), 64 rotations, 128 and 1024 symbols, in both modes, next to the bound the kernel
should approach: its evaluations (B R len sum_c M_c, one distance-and-exponential each in the second pass) divided by the
machine's exponential rate.  That rate is derived from MI355X_MICROARCH's cycle constants: v_exp_f32 issues one 64-lane
wave-instruction per 8 cycles on a SIMD, so 4 SIMDs x 64 / 8 = 32 exponentials per cycle and CU, times 256 CUs at the 2.4 GHz peak
clock = 1.97e13 per second.  The same table prices the other vector instructions at 2 cycles per wave-instruction with several
waves on a SIMD; the kernel's inner loops (counted in its ISA) issue 11 of them per evaluation besides the exponential, which gives
the second, tighter bound printed beside the first.  Device events around a train of back-to-back calls, legs interleaved over
rounds; median (min).  These are call times, not profiler kernel times.  Writes to --out (default profiles/likelihood.txt), keeping
whatever follows the line "---" in an existing file (notes recorded by hand)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vit_vs_raw_iq_amd import FrameSynth, LikelihoodClassifier  # noqa: E402

LENGTHS = (128, 1024)
CUS, CLOCK_HZ = 256, 2.4e9
EXP_PER_CYCLE_CU = 4 * 64 / 8                # v_exp_f32: 8 cycles per wave-instruction and SIMD
VALU_PER_CYCLE_CU = 4 * 64 / 2               # v_fma_f32 and its like: 2 cycles
VALU_PER_EVAL = 11                           # pass 1: 2 sub, mul, fma, half a min3; pass 2: 3 sub, 2 mul, fma, half a pk_add


def train_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    batch = 256
    legs = []
    for length in LENGTHS:
        for mode in ("max", "mean"):
            clf = LikelihoodClassifier(length, mode=mode)
            raw, y, z = FrameSynth(clf.class_names, snrs_db=(8.0, 20.0), length=length, seed=1, device=d).generate(batch)
            s2 = clf.noise_for(z)[1].float()
            acc = float((clf.predict(raw, sigma2=s2) == y).float().mean())
            evals = batch * clf.n_rotations * length * len(clf.points)
            legs.append((f"len {length:>4} {mode:<4}", lambda clf=clf, raw=raw, s2=s2: clf(raw, sigma2=s2), evals, acc))
    for _, fn, _, _ in legs:                                 # warm-up: code objects, clocks
        train_us(fn, 3)
    times = {name: [] for name, _, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, _, _ in legs:
            times[name].append(train_us(fn, args.calls))
    exp_rate = EXP_PER_CYCLE_CU * CUS * CLOCK_HZ
    all_rate = 1.0 / (1.0 / EXP_PER_CYCLE_CU + VALU_PER_EVAL / VALU_PER_CYCLE_CU) * CUS * CLOCK_HZ
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {batch} frames, 17 classes (812 points), 64 rotations; device events around a train "
             f"of {args.calls} calls, median (min) over {args.rounds} interleaved rounds",
             f"exponential rate {exp_rate:.3e} /s (32 per cycle and CU, 256 CUs, 2.4 GHz); with the {VALU_PER_EVAL} other vector instructions of an "
             f"evaluation {all_rate:.3e} evaluations/s",
             f"{'leg':<16} {'us/launch':>22} {'evaluations':>12} {'exp bound us':>13} {'time/bound':>11} {'VALU bound us':>14} {'time/bound':>11} "
             f"{'accuracy':>9}"]
    for name, _, evals, acc in legs:
        t = statistics.median(times[name])
        be, ba = evals / exp_rate * 1e6, evals / all_rate * 1e6
        lines.append(f"{name:<16} {t:>11.1f} ({min(times[name]):>8.1f}) {evals:>12.3e} {be:>13.1f} {t / be:>11.2f} {ba:>14.1f} {t / ba:>11.2f} {acc:>9.3f}")
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
