"""What the hybrid likelihood classifier costs ("Hybrid likelihood classifier"): microseconds per launch of
iq_frames_likelihood_em in its default configuration (16 starts, 32 updates: 16 * 33 = 528 passes) at B = 256 frames of 1024
symbols over the 17 table classes (812 points), beside iq_frames_likelihood at 64 rotations (64 passes) on the same frames in the
same run, and the time per pass of both.  A pass is B len sum_c M_c evaluations of a distance and an exponential; an update pass
of the new kernel also forms four weighted sums per evaluation (four fused multiply-adds) and reads the unscaled point and its
|s|^2 beside the scaled one.  Also timed: 128 symbols, and the new kernel's one-start modes (a given start, three waves idle).
Device events around a train of back-to-back calls after a warm-up, legs interleaved over rounds; median (min).  These are call
times, not profiler kernel times.  Writes to --out (default profiles/likelihood_em.txt), keeping whatever follows the line "---"
in an existing file (notes recorded by hand)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vit_vs_raw_iq_amd import FrameSynth, HybridLikelihoodClassifier, LikelihoodClassifier  # noqa: E402

LENGTHS = (1024, 128)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_em.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    batch = 256
    legs = []
    for length in LENGTHS:
        em, lik = HybridLikelihoodClassifier(length), LikelihoodClassifier(length)
        raw, y, z = FrameSynth(em.class_names, snrs_db=(8.0, 20.0), length=length, seed=1, device=d).generate(batch)
        s2 = lik.noise_for(z)[1].float()
        ll, h, v, _ = em(raw, return_estimates=True)
        acc_em = float((em.predict(raw) == y).float().mean())
        acc_lik = float((lik.predict(raw, sigma2=s2) == y).float().mean())
        legs.append((f"len {length:>4} hybrid 16 x 33", lambda em=em, raw=raw: em(raw), em.n_starts * (em.iters + 1), acc_em))
        legs.append((f"len {length:>4} hybrid given", lambda em=em, raw=raw, h=h, v=v: em(raw, h0=h, v0=v), em.iters + 1, float("nan")))
        legs.append((f"len {length:>4} known, 64 rot", lambda lik=lik, raw=raw, s2=s2: lik(raw, sigma2=s2), lik.n_rotations, acc_lik))
    for _, fn, _, _ in legs:                                 # warm-up: code objects, clocks
        train_us(fn, 2)
    times = {name: [] for name, _, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, _, _ in legs:
            times[name].append(train_us(fn, args.calls))
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {batch} frames, 17 classes (812 points); device events around a train of "
             f"{args.calls} calls, median (min) over {args.rounds} interleaved rounds, after a warm-up",
             f"{'leg':<26} {'us/launch':>24} {'passes':>7} {'us/pass':>9} {'accuracy':>9}"]
    per_pass = {}
    for name, _, passes, acc in legs:
        t = statistics.median(times[name])
        per_pass[name] = t / passes
        lines.append(f"{name:<26} {t:>12.1f} ({min(times[name]):>9.1f}) {passes:>7d} {t / passes:>9.2f} {acc:>9.3f}")
    for length in LENGTHS:
        a, b = per_pass[f"len {length:>4} hybrid 16 x 33"], per_pass[f"len {length:>4} known, 64 rot"]
        lines.append(f"len {length}: a pass of the hybrid kernel costs {a / b:.2f} rotations of the known-variance kernel")
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
