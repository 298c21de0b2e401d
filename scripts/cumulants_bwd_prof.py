"""What the cumulant gradient costs ("Cumulant gradients"): microseconds per launch of iq_frames_cumulants_bwd at
256 x 1024 and 4096 x 128 symbols over the 16 decision classes -- every class asked about, the margin loss's two classes per
frame, and the features alone -- beside iq_frames_cumulants (scores) on the same batch in the same run, and beside the HBM bound
of 16 bytes per symbol (the frame read once, dx written once) at the 6.3 TB/s a copy achieves.  With --parent-lib PATH the
forward of another build of libiqvit.so (the parent commit's) is timed on the same batch in the same rounds; both forwards are the
bare C call.  The eager legs are call times with the host's path to the launch in them (the backward's through
CumulantClassifier._backward, which also allocates dx); the graph legs replay a captured train of launches and are the device's
time per launch.  Device events, legs interleaved over rounds after a warm-up; median (min).  Then the device's FGSM
and PGD curves on the 20 dB decision set (256 frames, 16 classes, 1024 symbols, known sigma2, margin loss; the frames are built
by data.make_dataset as in the tests) beside random signs, and the transfer table across the three classical classifiers.
Writes to --out (default profiles/cumulants_bwd.txt), keeping whatever follows the line "---" in an existing file (notes
recorded by hand)."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vit_vs_raw_iq_amd import (CumulantClassifier, HybridLikelihoodClassifier, LikelihoodClassifier, robustness_curve,  # noqa: E402
                               transfer_table)
from vit_vs_raw_iq_amd import _native as N  # noqa: E402
from vit_vs_raw_iq_amd import data as D  # noqa: E402
from vit_vs_raw_iq_amd.adversarial import _margin_grad  # noqa: E402

EPS = (0.0, 0.01, 0.02, 0.05)
HBM = 6.3e12                                       # bytes / s a float4 copy achieves on this part
SHAPES = ((256, 1024), (4096, 128))
TRAIN = 20                                         # launches per captured graph


def train_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def captured(fn):
    """fn() TRAIN times in one graph -> a function that replays it and counts as TRAIN calls."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(TRAIN):
            fn()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cumulants_bwd.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="another build of libiqvit.so whose iq_frames_cumulants is timed beside this one's")
    args = ap.parse_args()
    d = torch.device("cuda:0")
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None
    classes = [c for c in D.CLASSES[:17] if c != "32PSK"]
    lines = [f"device: {torch.cuda.get_device_name(0)}; 16 classes; device events around a train of {args.calls} calls (graph legs: a "
             f"replay of {TRAIN} captured launches), median (min) over {args.rounds} interleaved rounds, after a warm-up",
             f"{'leg':<44} {'us/launch':>20}  x forward  x HBM bound"]
    for batch, length in SHAPES:
        clf = CumulantClassifier(length, classes=classes)
        X, Y, _ = D.make_dataset(batch, seed=5, classes=classes, snrs_db=(20.0,), n_symbols=length)
        x, y = torch.from_numpy(np.array(X, dtype=np.float32)).to(d), torch.from_numpy(np.array(Y)).to(d)
        s2 = torch.full((batch,), 0.01, device=d)
        score = clf(x, sigma2=s2)
        every, two, df = torch.randn(batch, clf.n_classes, device=d), _margin_grad(score, y), torch.randn(batch, 10, device=d)
        out = torch.empty_like(score)
        mu, w, bias = clf.tables_on(d)
        par = clf.struct(s2.data_ptr(), mu.data_ptr(), w.data_ptr(), bias.data_ptr())

        def forward_of(lib, what):
            """The bare C call of `lib`'s forward (scores): the same host path for this build and the parent's."""
            def call():
                stream = torch.cuda.current_stream(d).cuda_stream          # (the capture's stream, inside a capture)
                N.check(lib.iq_frames_cumulants(ctypes.c_void_p(x.data_ptr()), None, None, ctypes.c_void_p(out.data_ptr()), None,
                                                batch, length, ctypes.byref(par), ctypes.c_void_p(stream)), what)
            return call
        legs = [("forward, scores", forward_of(N.lib(), "iq_frames_cumulants")),
                ("backward, every class", lambda: clf._backward(x, every, s2)),
                ("backward, margin loss (2 classes)", lambda: clf._backward(x, two, s2)),
                ("backward, features only", lambda: clf._backward(x, None, s2, df))]
        if parent is not None:
            legs.insert(1, ("forward, scores, parent build", forward_of(parent, "the parent build's iq_frames_cumulants")))
        legs = [(name, fn, 1) for name, fn in legs] + [(name + ", graph", captured(fn), TRAIN) for name, fn in legs]
        for _, fn, _ in legs:                                # warm-up: code objects, clocks
            train_us(fn, 2)
        times = {name: [] for name, _, _ in legs}
        for _ in range(args.rounds):
            for name, fn, per in legs:
                times[name].append(train_us(fn, max(1, args.calls // per)) / per)
        t = {name: statistics.median(v) for name, v in times.items()}
        bound = batch * length * 16 / HBM * 1e6
        lines.append(f"{batch} x {length}: HBM bound {bound:.2f} us ({batch * length * 16 / 1e6:.1f} MB at {HBM / 1e12:.1f} TB/s)")
        for name, _, _ in legs:
            base = t["forward, scores, graph" if name.endswith("graph") else "forward, scores"]
            lines.append(f"  {name:<42} {t[name]:>9.1f} ({min(times[name]):>8.1f})  {t[name] / base:>9.2f}  {t[name] / bound:>11.1f}")
        if parent is not None:
            lines.append(f"  backward, every class / the parent build's forward (graph): "
                         f"{t['backward, every class, graph'] / t['forward, scores, parent build, graph']:.2f}; this build's forward / the "
                         f"parent's: {t['forward, scores, graph'] / t['forward, scores, parent build, graph']:.3f}")
    # the curves and the transfer table of the decision set
    length = 1024
    X, Y, _ = D.make_dataset(256, seed=3, classes=classes, snrs_db=(20.0,), n_symbols=length)
    xd, yd = torch.from_numpy(np.array(X, dtype=np.float32)).to(d), torch.from_numpy(np.array(Y)).to(d)
    clf = CumulantClassifier(length, classes=classes)
    g = torch.Generator(device=d)
    g.manual_seed(0)
    signs = torch.randint(0, 2, xd.shape, generator=g, device=d).float() * 2 - 1
    acc = lambda x: float((clf.predict(x, snr_db=20.0) == yd).float().mean())                  # noqa: E731
    fg = robustness_curve(clf, xd, yd, EPS, snr_db=20.0)
    pg = robustness_curve(clf, xd, yd, EPS, attack="pgd", snr_db=20.0)
    lines += ["", "the decision set (256 frames, 16 classes, 1024 symbols, 20 dB), CumulantClassifier(1024), known sigma2, margin loss",
              f"{'eps':>6} {'FGSM':>8} {'PGD 10':>8} {'random signs':>13}"]
    lines += [f"{e:>6.2f} {a:>8.3f} {b:>8.3f} {acc(xd + e * signs):>13.3f}" for e, a, b in zip(EPS, fg, pg)]
    lik = LikelihoodClassifier(length, classes=classes)
    em = HybridLikelihoodClassifier(length, classes=classes)
    parties = [(clf, dict(snr_db=20.0)), (lik, dict(snr_db=20.0)), em]
    names = ("cumulants", "likelihood", "hybrid")
    for attack in ("fgsm", "pgd"):
        table = transfer_table(parties, parties, xd, yd, 0.05, attack=attack)
        lines += ["", f"transfer at eps 0.05, {attack} on the margin loss: accuracy of the column's classifier on the frames crafted against the row's",
                  f"{'':<12}" + "".join(f"{n:>12}" for n in names)]
        lines += [f"{n:<12}" + "".join(f"{v:>12.3f}" for v in row) for n, row in zip(("clean",) + names, table)]
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
