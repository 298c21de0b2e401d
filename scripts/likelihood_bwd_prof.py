"""What the likelihood gradients cost ("Likelihood gradients"): microseconds per launch of iq_frames_likelihood_bwd
('max', 'mean', and 'max' under the margin loss: two classes per frame) and of iq_frames_likelihood_em_bwd at B = 256 frames of
1024 symbols over the 17 table classes (812 points) and 64 rotations, beside the two forwards on the same frames in the same run.
The backward legs time the backward's C call alone, on forward outputs computed beforehand.  'mean' does the forward's
evaluations plus two fused multiply-adds and no logarithm, except that a rotation whose share is exactly 0 in fp32 is skipped:
the share of the (frame, class, rotation) triples that run is printed.  'max' runs one rotation of 64.  Then the device's FGSM
table on the 20 dB decision set (68 frames, 128 symbols; the frames are built by data.make_dataset as in the tests) beside
random signs of the same size.  Device events around a train of back-to-back calls after a warm-up, legs interleaved over
rounds; median (min).  These are call times, not profiler kernel times.  Writes to --out (default
profiles/likelihood_bwd.txt), keeping whatever follows the line "---" in an existing file (notes recorded by hand)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vit_vs_raw_iq_amd import FrameSynth, HybridLikelihoodClassifier, LikelihoodClassifier, fgsm  # noqa: E402
from vit_vs_raw_iq_amd import data as D  # noqa: E402
from vit_vs_raw_iq_amd.adversarial import _margin_grad  # noqa: E402

EPS = (0.01, 0.02, 0.05, 0.10)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_bwd.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    batch, length = 256, 1024
    clfs = {m: LikelihoodClassifier(length, mode=m) for m in ("max", "mean")}
    em = HybridLikelihoodClassifier(length)
    raw, y, z = FrameSynth(em.class_names, snrs_db=(8.0, 20.0), length=length, seed=1, device=d).generate(batch)
    s2 = clfs["max"].noise_for(z)[1].float().to(d)
    dl = torch.randn(batch, em.n_classes, device=d)
    legs, ran = [], float("nan")
    for m, clf in clfs.items():
        outs, held = clf._forward(raw, s2, None)
        legs.append((f"forward {m}", lambda clf=clf: clf(raw, sigma2=s2)))
        legs.append((f"backward {m}", lambda clf=clf, held=held: clf._backward(raw, dl, *held)))
        if m == "max":
            two = _margin_grad(outs[0], y)
            legs.append(("backward max, margin loss", lambda clf=clf, held=held, two=two: clf._backward(raw, two, *held)))
        else:
            share = torch.exp2((held[3] - held[2][..., None]).float() * 1.4426950408889634)
            ran = float((share > 0).float().mean())
    outs, held = em._forward(raw)
    legs.append(("forward hybrid 16 x 33", lambda: em(raw)))
    legs.append(("backward hybrid", lambda held=held: em._backward(raw, dl, *held)))
    for _, fn in legs:                                       # warm-up: code objects, clocks
        train_us(fn, 2)
    times = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            times[name].append(train_us(fn, args.calls))
    t = {name: statistics.median(v) for name, v in times.items()}
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {batch} frames of {length} symbols, 17 classes (812 points), 64 rotations; "
             f"device events around a train of {args.calls} calls, median (min) over {args.rounds} interleaved rounds, after a warm-up",
             f"{'leg':<28} {'us/launch':>24}"]
    lines += [f"{name:<28} {t[name]:>12.1f} ({min(times[name]):>9.1f})" for name, _ in legs]
    lines += [f"backward mean / forward mean {t['backward mean'] / t['forward mean']:.3f}   ({ran:.3f} of the (frame, class, rotation) "
              f"triples have a share above 0 and run)",
              f"backward max / backward mean {t['backward max'] / t['backward mean']:.4f}   (1 / 64 = {1 / 64:.4f}; against the forward: "
              f"{t['backward max'] / t['forward max']:.4f})",
              f"margin loss / backward max   {t['backward max, margin loss'] / t['backward max']:.3f}   (2 classes of 17; the points they hold differ)",
              f"backward hybrid / forward    {t['backward hybrid'] / t['forward hybrid 16 x 33']:.5f}   (1 pass of 528: {1 / 528:.5f})"]
    # the FGSM table of the decision set
    X, Y, _ = D.make_dataset(68, seed=3, classes=D.CLASSES[:17], snrs_db=(20.0,), n_symbols=128)
    clf = LikelihoodClassifier(128)
    xd, yd = torch.from_numpy(np.array(X, dtype=np.float32)).to(d), torch.from_numpy(np.array(Y)).to(d)
    acc = lambda x: float((clf.predict(x, snr_db=20.0) == yd).float().mean())                  # noqa: E731
    g = torch.Generator(device=d)
    g.manual_seed(0)
    signs = torch.randint(0, 2, xd.shape, generator=g, device=d).float() * 2 - 1
    lines += ["", f"FGSM on the margin loss, the decision set (68 frames, 17 classes, 128 symbols, 20 dB), LikelihoodClassifier(128) 'max'; clean {acc(xd):.3f}",
              f"{'eps':>6} {'FGSM':>8} {'random signs':>13}"]
    lines += [f"{e:>6.2f} {acc(fgsm(clf, xd, yd, e, snr_db=20.0)):>8.3f} {acc(xd + e * signs):>13.3f}" for e in EPS]
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
