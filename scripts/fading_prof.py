"""What the fading channel costs and what it does to the classical receivers ("Fading channel").  Three parts, written
to --out (default profiles/fading.txt), keeping whatever follows the line "---" in an existing file (notes recorded by hand):

1. The worst ratio of the device's error to the derived bound on the real-table cases of tests/fading_ref.py (a record, not a
   threshold: the tests assert the bound itself).
2. Microseconds per launch of iq_frames_fade on 256 frames of 4096 samples at 1 and 8 taps and 0, 8 and 32 sinusoids, next to a
   bound: the e(p) evaluations of the launch (B len L (NS + 1)) times the 47 vector instructions the kernel's inner loop spends on
   one (counted in its ISA: the integer phase, the conversion, sincospif's reduction and two polynomials, the packed fmaf),
   divided by the vector rate scripts/likelihood_prof.py uses (2 cycles per wave-instruction and SIMD, 256 CUs, 2.4 GHz).  Device
   events around a train of back-to-back calls, legs interleaved over rounds; median (min).  These are call times, not profiler
   kernel times.  There is no pass or fail on time: this kernel has no parent to compare with.
3. fading_curve tables: top-1 accuracy against the maximum Doppler shift and against the sample-clock offset of the chains
   Receiver -> Equaliser -> Carrier -> {likelihood, hybrid likelihood, cumulants} on the 20 dB decision set (the 16 table classes
   without 32PSK, 256 frames, 1024 symbols at 2 samples per symbol) behind a 3-tap Rician channel of 16 sinusoids per tap."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fading_ref as R  # noqa: E402
from vit_vs_raw_iq_amd import (Carrier, CumulantClassifier, Equaliser, Fading, HybridLikelihoodClassifier, LikelihoodClassifier,  # noqa: E402
                               ReceivedSynth, Receiver, ShapedSynth, fading_curve, fading_reference, noise_for)
from vit_vs_raw_iq_amd import data as D  # noqa: E402

CUS, CLOCK_HZ = 256, 2.4e9
VALU_PER_CYCLE_CU = 4 * 64 / 2               # as scripts/likelihood_prof.py: 2 cycles per wave-instruction and SIMD
VALU_PER_EVAL = 47                           # the inner loop of frames_fade_kernel, per path and sample
DOPPLER = (0.0, 1e-5, 1e-4, 3e-4, 1e-3)
CLOCK_PPM = (0.0, 10.0, 50.0, 100.0, 200.0)


def train_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def bound_lines(d):
    lines = []
    for name, (kw, x, paths, amps, clock, _) in R.real_cases().items():
        fd = Fading(**kw)
        y = fd.given(torch.from_numpy(x).to(d), paths, amps, clock).cpu().numpy().astype(np.float64)
        _, bound = R.definition64(x, paths, amps, clock, fd)
        err = np.abs(y - fading_reference(x, paths, amps, clock, fd)).max(axis=2)
        lines.append(f"error / derived bound, {name:<22} worst {(err / bound).max():.3f} (bound of the order of {bound.mean():.1e})")
    return lines


def time_lines(d, rounds, calls):
    batch, length = 256, 4096
    x = torch.randn(batch, length + 64, 2, device=d)
    legs = []
    for taps in (1, 8):
        for ns in (0, 8, 32):
            fd = Fading(length + 64, length, taps=taps, sinusoids=ns, doppler=(0.0, 1e-3), clock_ppm=(-50.0, 50.0), timing=True)
            legs.append((f"{taps} tap{'s' if taps > 1 else ' '} {ns:>2} sinusoids", lambda fd=fd: fd(x, seed=1), batch * length * taps * (ns + 1)))
    for _, fn, _ in legs:                                    # warm-up: code objects, clocks, the tables' upload
        train_us(fn, 3)
    times = {name: [] for name, _, _ in legs}
    for _ in range(rounds):
        for name, fn, _ in legs:
            times[name].append(train_us(fn, calls))
    rate = VALU_PER_CYCLE_CU / VALU_PER_EVAL * CUS * CLOCK_HZ
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {batch} frames of {length} samples, K = 9, n_frac = 128, unit power, no noise; device "
             f"events around a train of {calls} calls, median (min) over {rounds} interleaved rounds",
             f"bound: e(p) evaluations at {VALU_PER_EVAL} vector instructions each, 128 lane-instructions per cycle and CU, {CUS} CUs, 2.4 GHz = "
             f"{rate:.3e} evaluations/s (the interpolation and the tail are not in it)",
             f"{'leg':<24} {'us/launch':>22} {'evaluations':>12} {'bound us':>10} {'time/bound':>11}"]
    for name, _, evals in legs:
        t = statistics.median(times[name])
        b = evals / rate * 1e6
        lines.append(f"{name:<24} {t:>11.1f} ({min(times[name]):>8.1f}) {evals:>12.3e} {b:>10.1f} {t / b:>11.2f}")
    return lines


def curve_lines(d, n):
    classes = [c for c in D.CLASSES[:17] if c != "32PSK"]
    sps, symbols = 2, 1024
    length = sps * symbols
    ws = ShapedSynth(classes, snrs_db=(20.0,), length=length, sps=sps, seed=3, device=d)
    rx = Receiver.for_synth(ws, timing="energy")
    eq, cr = Equaliser(symbols), Carrier(symbols, layout="interleaved", device=d)
    base = Fading(length + 64, length, taps=3, rice_k_db=6.0, decay=0.5, sinusoids=16)
    gain, sigma2 = noise_for(20.0, normalised=True)
    lik, em, cum = (LikelihoodClassifier(symbols, classes=classes), HybridLikelihoodClassifier(symbols, classes=classes),
                    CumulantClassifier(symbols, classes=classes))
    cum.fit(ReceivedSynth(ws, rx, equaliser=eq, carrier=cr), 64, blind=True, stream=2)      # centroids behind the static chain, no channel
    chain = lambda raw: cr(eq(rx(raw)))                                                      # noqa: E731
    parties = (("likelihood", lambda raw: lik.predict(chain(raw), sigma2=sigma2, gain=gain)),
               ("hybrid", lambda raw: em.predict(chain(raw))), ("cumulants", lambda raw: cum.predict(chain(raw))))
    plain = [float((p(ws.generate(n, 0, 1)[0]) == ws.generate(n, 0, 1)[1]).float().mean()) for _, p in parties]
    lines = [f"fading_curve: Receiver(energy) -> Equaliser({eq.taps} taps, {eq.iters} steps) -> Carrier(order {cr.order}) -> classifier; {len(classes)} "
             f"classes, {n} frames of {symbols} symbols at {sps} samples per symbol, 20 dB; channel: {base!r}",
             "without any channel (the ShapedSynth's own frames):   " + "".join(f"{k:>12}" for k, _ in parties),
             f"{'':<54}" + "".join(f"{v:>12.3f}" for v in plain)]
    for kind, values in (("doppler", DOPPLER), ("clock_ppm", CLOCK_PPM)):
        cols = [fading_curve(p, ws, base, kind, values, n=n, batch=n, stream=1) for _, p in parties]
        lines += ["", f"{kind:<54}" + "".join(f"{k:>12}" for k, _ in parties)]
        lines += [f"{v:<54g}" + "".join(f"{c[i]:>12.3f}" for c in cols) for i, v in enumerate(values)]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fading.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    lines = bound_lines(d) + [""] + time_lines(d, args.rounds, args.calls) + [""] + curve_lines(d, args.frames)
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
