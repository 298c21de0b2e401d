"""iq_frames_impair (full training augmentation plus noise) against iq_frames_preprocess on the same frames ("Channel
impairments"): microseconds per launch from device events around a train of launches, and GB/s of ALGORITHMIC bytes (the frame
read once, the two planar channels written once: n*len*8 + n*2*take*4).  Three legs per size, interleaved over rounds so that
clock and neighbour drift hits all alike: preprocess, impair with nothing switched on (the identity: what staging through LDS
costs), impair with Impairments.augmentation() + cfo + noise.  256 frames of 1024 samples is one training batch (4 MB of
traffic: launch-latency and cache territory); 32768 frames (537 MB) is past the 256 MiB Infinity Cache, i.e. the HBM figure.
Writes the table to --out (default profiles/impair.txt)."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vit_vs_raw_iq_amd._native as N  # noqa: E402
from vit_vs_raw_iq_amd import Impairments  # noqa: E402


def train_us(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impair.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    L = N.lib()
    st = N.stream_handle()
    stats = (C.c_float * 4)(0.01, 0.7, -0.02, 0.71)
    length = take = 1024
    full = Impairments.augmentation(length).replace(cfo=(-1e-3, 1e-3), snr_db=(0.0, 20.0))
    lines = [f"device: {torch.cuda.get_device_name(0)}; frames of {length} complex samples, take = {take}; device events around a "
             f"train of launches, median (min) over {args.rounds} interleaved rounds",
             f"{'frames':>7} {'leg':<34} {'us/launch':>18} {'GB/s algorithmic':>18}"]
    for n, launches in ((256, 400), (32768, 20)):
        raw = torch.randn(n, length, 2, device=d)
        out = torch.empty(n, 2, take, device=d)
        nbytes = n * length * 8 + n * 2 * take * 4
        step = [0]

        def pre():
            N.check(L.iq_frames_preprocess(raw.data_ptr(), out.data_ptr(), n, length, take, stats, st), "iq_frames_preprocess")

        def imp(which):
            def go():
                step[0] += 1
                par = which.struct(seed=1, step=step[0] & 0xFFFFFFFF)
                N.check(L.iq_frames_impair(raw.data_ptr(), out.data_ptr(), None, n, length, take, stats, C.byref(par), st),
                        "iq_frames_impair")
            return go
        legs = [("iq_frames_preprocess", pre), ("iq_frames_impair identity", imp(Impairments())),
                ("iq_frames_impair augmentation+noise", imp(full))]
        for _, fn in legs:                       # warm-up: code objects, clocks
            train_us(fn, launches)
        times = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, fn in legs:
                times[name].append(train_us(fn, launches))
        for name, _ in legs:
            med, lo = statistics.median(times[name]), min(times[name])
            lines.append(f"{n:>7} {name:<34} {med:>9.2f} ({lo:>6.2f}) {nbytes / med / 1e3:>9.0f} ({nbytes / lo / 1e3:>6.0f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
