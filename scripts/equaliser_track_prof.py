"""What the tracking equaliser costs and what it buys ("Tracking equaliser").  Two parts, written to --out (default
profiles/equaliser_track.txt), keeping whatever follows the line "---" in an existing file (notes recorded by hand):

1. Microseconds per call of iq_frames_equalise_track on 256 frames of 1024 symbols (11 taps, the default 32 steps per segment) at
   seg / hop = 128 / 64 and 256 / 128: the CMA call (two launches: descent, then filter; est not asked for), the GIVEN call (the
   filter's launch alone), their difference (the descent's launch) and iq_frames_equalise_track_bwd (one launch), beside
   iq_frames_equalise at 64 steps on the same frames.  Device events around a train of back-to-back C calls, legs interleaved
   over rounds; median (min).  These are call times, not profiler kernel times.  Beside each a simple bound: its fmaf count (8 per
   tap, symbol and step in the descent, 6 per tap and output in the filter and the adjoint, 8 per tap, symbol and step plus 4 per
   tap and symbol in the block kernel) at the vector rate scripts/likelihood_prof.py uses (2 cycles per wave-instruction and SIMD,
   256 CUs, 2.4 GHz).  There is no pass or fail on time: the new kernels have no parent to compare with.
2. Accuracy on the 20 dB decision set of DESIGN.md's fading table (16 classes, --frames frames of 1024 symbols at sps = 2, channel 3
   taps, Rice 6 dB, decay 0.5, 16 sinusoids) of Receiver -> equaliser -> Carrier -> {likelihood, hybrid, cumulants}, with the block
   Equaliser and with TrackingEqualiser in its place, against the maximum Doppler shift; and the hybrid column per class for QPSK
   and 16QAM at Doppler 0 and 3e-4 on --class-frames frames."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vit_vs_raw_iq_amd._native as N  # noqa: E402
from vit_vs_raw_iq_amd import (Carrier, CumulantClassifier, Equaliser, FadedSynth, Fading, HybridLikelihoodClassifier,  # noqa: E402
                               LikelihoodClassifier, ReceivedSynth, Receiver, ShapedSynth, TrackingEqualiser, noise_for)
from vit_vs_raw_iq_amd import data as D  # noqa: E402

CUS, CLOCK_HZ = 256, 2.4e9
FMAF_PER_S = 4 * 64 / 2 * CUS * CLOCK_HZ     # as scripts/likelihood_prof.py: 2 cycles per wave-instruction and SIMD
DOPPLER = (0.0, 1e-5, 1e-4, 3e-4, 1e-3)


def train_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def time_lines(d, rounds, calls):
    batch, length, taps = 256, 1024, 11
    g = torch.Generator().manual_seed(length)
    ph = torch.randint(0, 4, (batch, length), generator=g).double() * (torch.pi / 2) + torch.pi / 4
    a = torch.polar(torch.ones_like(ph), ph)
    zc = a + 0.3 * torch.roll(a, 1, 1) - 0.15j * torch.roll(a, 2, 1)
    zc = zc / zc.abs().pow(2).mean(dim=1, keepdim=True).sqrt()
    x = (torch.view_as_real(zc) + 0.05 * torch.randn(batch, length, 2, generator=g).double()).float().to(d)
    out = torch.empty_like(x)
    lib, st = N.lib(), torch.cuda.current_stream(d).cuda_stream
    block = Equaliser(length)
    w0 = block(x, return_w=True)[1]
    wb = torch.empty_like(w0)
    legs, pairs = [], []

    def block_call():
        par = block.struct(None, None, mode=1)
        N.check(lib.iq_frames_equalise(x.data_ptr(), out.data_ptr(), wb.data_ptr(), None, batch, length, C.byref(par), st), "iq_frames_equalise")
    legs.append((f"iq_frames_equalise, {block.iters} steps", block_call, batch * length * taps * (8.0 * block.iters + 4.0)))
    for seg, hop in ((128, 64), (256, 128)):
        eq = TrackingEqualiser(length, seg=seg, hop=hop)
        S, taper = eq.segments, eq.table_on(d)
        w = torch.empty(batch, S, taps, 2, device=d)

        def cma(eq=eq, w=w, taper=taper):
            par = eq.track_struct(None, w0.data_ptr(), taper.data_ptr(), mode=1)
            N.check(lib.iq_frames_equalise_track(x.data_ptr(), out.data_ptr(), w.data_ptr(), None, batch, length, C.byref(par), st), "track")

        def given(eq=eq, w=w):
            par = eq.track_struct(w.data_ptr(), None, None, mode=0)
            N.check(lib.iq_frames_equalise_track(x.data_ptr(), out.data_ptr(), None, None, batch, length, C.byref(par), st), "track given")

        def bwd(eq=eq, w=w):
            par = eq.track_struct(w.data_ptr(), None, None, mode=0)
            N.check(lib.iq_frames_equalise_track_bwd(x.data_ptr(), out.data_ptr(), batch, length, C.byref(par), st), "track bwd")
        tag = f"{seg:>3} / {hop:<3} ({S:>2} segments)"
        descent = batch * S * seg * taps * 8.0 * eq.track_iters
        filt = batch * length * taps * 6.0
        pairs.append((tag, f"track CMA call (2 launches)  {tag}", f"track GIVEN call (filter)    {tag}", descent))
        legs += [(f"track CMA call (2 launches)  {tag}", cma, descent + filt), (f"track GIVEN call (filter)    {tag}", given, filt),
                 (f"track backward               {tag}", bwd, filt)]
    for _, fn, _ in legs:                                    # warm-up: code objects, clocks
        train_us(fn, 5)
    times = {name: [] for name, _, _ in legs}
    for _ in range(rounds):
        for name, fn, _ in legs:
            times[name].append(train_us(fn, calls))
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {batch} frames of {length} symbols, {taps} taps, 32 steps per segment; device events "
             f"around a train of {calls} C calls, median (min) over {rounds} interleaved rounds",
             f"bound: fmaf count at 128 lane-instructions per cycle and CU, {CUS} CUs, 2.4 GHz = {FMAF_PER_S:.3e} fmaf/s",
             f"{'leg':<52} {'us/call':>20} {'fmaf':>11} {'bound us':>9} {'time/bound':>11}"]
    med = {}
    for name, _, count in legs:
        t = med[name] = statistics.median(times[name])
        b = count / FMAF_PER_S * 1e6
        lines.append(f"{name:<52} {t:>10.1f} ({min(times[name]):>7.1f}) {count:>11.3e} {b:>9.2f} {t / b:>11.1f}")
    for tag, cma_name, given_name, count in pairs:           # the descent's launch: the CMA call less the filter's
        t, b = med[cma_name] - med[given_name], count / FMAF_PER_S * 1e6
        lines.append(f"{'descent launch (CMA - GIVEN) ' + tag:<52} {t:>10.1f} {'':>9} {count:>11.3e} {b:>9.2f} {t / b:>11.1f}")
    return lines


def accuracy_lines(d, n, n_class):
    classes = [c for c in D.CLASSES[:17] if c != "32PSK"]
    sps, symbols = 2, 1024
    length = sps * symbols
    ws = ShapedSynth(classes, snrs_db=(20.0,), length=length, sps=sps, seed=3, device=d)
    rx = Receiver.for_synth(ws, timing="energy")
    cr = Carrier(symbols, layout="interleaved", device=d)
    base = Fading(length + 64, length, taps=3, rice_k_db=6.0, decay=0.5, sinusoids=16)
    gain, sigma2 = noise_for(20.0, normalised=True)
    lik, em = LikelihoodClassifier(symbols, classes=classes), HybridLikelihoodClassifier(symbols, classes=classes)
    chains = {}
    for name, eq in (("block", Equaliser(symbols)), ("tracking", TrackingEqualiser(symbols))):
        cum = CumulantClassifier(symbols, classes=classes)
        cum.fit(ReceivedSynth(ws, rx, equaliser=eq, carrier=cr), 64, blind=True, stream=2)    # centroids behind the same chain, no channel
        chains[name] = (eq, cum)
    eqt = chains["tracking"][0]
    lines = [f"accuracy: Receiver(energy) -> equaliser -> Carrier(order {cr.order}) -> classifier; {len(classes)} classes, {n} frames of {symbols} "
             f"symbols at {sps} samples per symbol, 20 dB; channel: {base!r}", f"block: {chains['block'][0]!r}", f"tracking: {eqt!r}", "",
             f"{'max Doppler (cycles / sample)':<32}" + "".join(f"{k + ' ' + e:>22}" for e in chains for k in ("likelihood", "hybrid", "cumulants"))]

    def predictions(raw, eq, cum):
        sym = cr(eq(rx(raw)))
        return lik.predict(sym, sigma2=sigma2, gain=gain), em.predict(sym), cum.predict(sym)
    for fd in DOPPLER:
        raw, y, _ = FadedSynth(ws, base.replace(doppler=fd)).generate(n, 0, 1)
        row = [float((p == y).float().mean()) for eq, cum in chains.values() for p in predictions(raw, eq, cum)]
        lines.append(f"{fd:<32g}" + "".join(f"{v:>22.3f}" for v in row))
    lines += ["", f"hybrid column per class, {n_class} frames ({n_class // len(classes)} per class)",
              f"{'max Doppler':<14} {'class':<8} {'block':>8} {'tracking':>10}"]
    for fd in (0.0, 3e-4):
        raw, y, _ = FadedSynth(ws, base.replace(doppler=fd)).generate(n_class, 0, 1)
        hyb = {name: predictions(raw, eq, cum)[1] for name, (eq, cum) in chains.items()}
        for cls in ("QPSK", "8PSK", "16QAM", "64QAM"):
            m = y == classes.index(cls)
            lines.append(f"{fd:<14g} {cls:<8} {float((hyb['block'][m] == y[m]).float().mean()):>8.3f} {float((hyb['tracking'][m] == y[m]).float().mean()):>10.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equaliser_track.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--class-frames", type=int, default=1024)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    lines = time_lines(d, args.rounds, args.calls) + [""] + accuracy_lines(d, args.frames, args.class_frames)
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
