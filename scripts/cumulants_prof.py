"""What the cumulant classifier costs and what it gets right ("Cumulant classifier").

Time: microseconds per launch of iq_frames_cumulants at B = 256 frames of 128 and 1024 symbols, features only and with the 17
table classes, next to two things measured in the same trains: a device-to-device copy of the frames' bytes (the memory floor: the
kernel reads the frames once and writes next to nothing) and the same ten features written as torch expressions on the device
(complex64 tensors: what one would write without the kernel).  Device events around a train of back-to-back calls, legs
interleaved over rounds; median (min).  These are call times, not profiler kernel times: an eager call carries the host's
path to the launch (the argument checks, ctypes), so the two kernel legs are also replayed from a captured graph of the same
train, which leaves the device's time per launch.

Accuracy: make_dataset-style frames (data.make_dataset, seed 3, 1900 frames over the 19 classes, or 1700 over the 17 table
classes) of 128 and 1024 symbols at 20, 8 and 0 dB, classified on the device in three configurations: the 17 table classes with
table centroids and known sigma2; all 19 classes fitted (FrameSynth frames at that SNR, 400 per class) with known sigma2; all 19
fitted, blind.  The 17-class rows count the 16PSK / 32PSK tie against the classifier.  The likelihood classifier's accuracy on the
same 17-class frames (64 rotations, 'max') stands beside them.

Writes to --out (default profiles/cumulants.txt), keeping whatever follows the line "---" in an existing file."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vit_vs_raw_iq_amd import CumulantClassifier, FrameSynth, LikelihoodClassifier  # noqa: E402
from vit_vs_raw_iq_amd import data as D  # noqa: E402

LENGTHS = (128, 1024)
SNRS_DB = (20.0, 8.0, 0.0)


def train_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def graphed(fn, calls):
    """fn() `calls` times, captured once -> a function that replays the whole train."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [fn() for _ in range(calls)]
    graph.keep = keep
    return graph.replay


def torch_features(x):
    """The ten blind features of (B, len, 2) frames as torch expressions."""
    y = torch.view_as_complex(x)
    m = y.mean(dim=1, keepdim=True)
    z = y - m
    r = (z * z.conj()).real
    z2 = z * z
    z4 = z2 * z2
    mean = lambda t: t.mean(dim=1)                                                        # noqa: E731
    M20, M21, M40, M41, M42 = mean(z2), mean(r), mean(z4), mean(z2 * r), mean(r * r)
    M60, M61, M62, M63, M80 = mean(z4 * z2), mean(z4 * r), mean(z2 * r * r), mean(r * r * r), mean(z4 * z4)
    n20 = (M20 * M20.conj()).real
    C40, C41, C42 = M40 - 3 * M20 ** 2, M41 - 3 * M20 * M21, M42 - n20 - 2 * M21 ** 2
    C60 = M60 - 15 * M20 * M40 + 30 * M20 ** 3
    C61 = M61 - 5 * M21 * M40 - 10 * M20 * M41 + 30 * M20 ** 2 * M21
    C62 = M62 - 6 * M20 * M42 - 8 * M21 * M41 - M20.conj() * M40 + 6 * n20 * M20 + 24 * M21 ** 2 * M20
    C63 = M63 - 9 * M21 * M42 + 12 * M21 ** 3 - 6 * (M20 * M41.conj()).real + 18 * n20 * M21
    C80 = M80 - 28 * M20 * M60 - 35 * M40 ** 2 + 420 * M20 ** 2 * M40 - 630 * M20 ** 4
    P = M21
    return torch.stack([m[:, 0].abs() ** 2 / P, M20.abs() / P, C40.abs() / P ** 2, C41.abs() / P ** 2, C42 / P ** 2, C60.abs() / P ** 3,
                        C61.abs() / P ** 3, C62.abs() / P ** 3, C63 / P ** 3, C80.abs() / P ** 4], dim=1)


def timing(d, rounds, calls):
    batch = 256
    legs = []
    for length in LENGTHS:
        clf = CumulantClassifier(length)
        raw = FrameSynth(clf.class_names, snrs_db=(8.0, 20.0), length=length, seed=1, device=d).generate(batch)[0]
        dst = torch.empty_like(raw)
        err = float((torch_features(raw) - clf.features(raw)).abs().max())
        legs.append((f"len {length:>4} features only", lambda clf=clf, raw=raw: clf.features(raw), err))
        legs.append((f"len {length:>4} 17 classes, pred", lambda clf=clf, raw=raw: clf.predict(raw), None))
        legs.append((f"len {length:>4} copy of the frames", lambda raw=raw, dst=dst: dst.copy_(raw), None))
        for what, fn in (("features, graph", lambda clf=clf, raw=raw: clf.features(raw)), ("pred, graph", lambda clf=clf, raw=raw: clf.predict(raw)),
                         ("copy, graph", lambda raw=raw, dst=dst: dst.copy_(raw))):
            replay = graphed(fn, calls)
            legs.append((f"len {length:>4} {what}", lambda replay=replay: replay(), "graph"))
        legs.append((f"len {length:>4} torch expressions", lambda raw=raw: torch_features(raw), None))
    for _, fn, _ in legs:                                    # warm-up: code objects, clocks, the tables' upload
        train_us(fn, 3)
    times = {name: [] for name, _, _ in legs}
    for _ in range(rounds):
        for name, fn, kind in legs:
            times[name].append(train_us(fn, 1) / calls if kind == "graph" else train_us(fn, calls))
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {batch} frames; device events around a train of {calls} calls, median (min) over "
             f"{rounds} interleaved rounds", f"{'leg':<32} {'us/call':>22} {'x the copy':>11}"]
    for name, _, err in legs:
        t = statistics.median(times[name])
        copy = statistics.median(times[name[:8] + (" copy, graph" if err == "graph" else " copy of the frames")])
        note = "" if err is None or err == "graph" else f"   (largest |torch - kernel| over the features: {err:.2e})"
        lines.append(f"{name:<32} {t:>11.1f} ({min(times[name]):>8.1f}) {t / copy:>11.2f}{note}")
    return lines


def accuracy(d):
    lines = ["", "accuracy on data.make_dataset frames (seed 3; 100 per class); fitted: FrameSynth frames at that SNR, 400 per class",
             f"{'symbols':>7} {'SNR dB':>7} {'table 17, known':>16} {'likelihood 17':>14} {'fitted 19, known':>17} {'fitted 19, blind':>17}"]
    names17, names19 = D.CLASSES[:17], D.CLASSES
    for length in LENGTHS:
        for snr in SNRS_DB:
            X17, Y17, _ = D.make_dataset(1700, seed=3, classes=names17, snrs_db=(snr,), n_symbols=length)
            X19, Y19, _ = D.make_dataset(1900, seed=3, classes=names19, snrs_db=(snr,), n_symbols=length)
            x17, x19 = torch.from_numpy(X17).to(d), torch.from_numpy(X19).to(d)
            table = (CumulantClassifier(length).predict(x17, snr_db=snr).cpu().numpy() == Y17).mean()
            lik = np.mean([(LikelihoodClassifier(length).predict(x17[i:i + 425], snr_db=snr).cpu().numpy() == Y17[i:i + 425]).mean()
                           for i in range(0, 1700, 425)])
            fs = FrameSynth(names19, snrs_db=(snr,), length=length, seed=9, device=d)
            known = CumulantClassifier(length, classes=names19).fit(fs, 400, blind=False)
            blind = CumulantClassifier(length, classes=names19).fit(fs, 400, blind=True)
            a_known = (known.predict(x19, snr_db=snr).cpu().numpy() == Y19).mean()
            a_blind = (blind.predict(x19).cpu().numpy() == Y19).mean()
            lines.append(f"{length:>7} {snr:>7.0f} {table:>16.3f} {lik:>14.3f} {a_known:>17.3f} {a_blind:>17.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cumulants.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-accuracy", action="store_true")
    args = ap.parse_args()
    d = torch.device("cuda:0")
    lines = timing(d, args.rounds, args.calls)
    if not args.no_accuracy:
        lines += accuracy(d)
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
