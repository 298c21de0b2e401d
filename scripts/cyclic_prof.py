"""What the cyclic-spectrum front end costs ("Cyclic-spectrum front end"): per batch of 256 frames of 1024 samples,
iq_frames_cyclic (kind 'both', squared coherence, Hann) at n_fft 64 (hop 16, 61 columns) and at n_fft 224 (hop 56, 15 columns),
and beside it on the same box iq_frames_spectrogram at the same n_fft (n_fft columns, its default hop and pad) and a torch-eager
statement of the same cyclic operation (unfold, complex matmul against the table, the phase reference, two batched complex Gram
matmuls, gather, coherence; complex64 on the device).  Two figures per leg:
  call ms     device events around a train of back-to-back calls (about 0.1 s per window), legs interleaved over rounds so that
              clock and neighbour drift hits all alike; median (min).  Launch gaps and the host's cost per call are included.
  kernel ms   the library's own event pair around each launch (iq_prof_enable / iq_prof_kernels), mean over the calls of a
              separate run; not available for the torch leg.
The flop figure counts what the kernel executes at these sizes, where every chunk of Y stays in LDS: the channelizer once (8 T
n^2 per frame) plus the Gram stage (16 T n^2 for both channels).  Numbers are recorded, not asserted.  Writes the table to --out (default
profiles/cyclic.txt), keeping whatever follows the line "---" in an existing file (notes recorded by hand)."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vit_vs_raw_iq_amd._native as N  # noqa: E402
from vit_vs_raw_iq_amd import CyclicSpectrum, FrameSynth, Spectrogram, SynthStream  # noqa: E402

PEAK_F32_MFMA = 155e12


def train_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(calls)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def kernel_ms(fn, calls):
    """{kernel name: mean ms per launch} from the library's event pairs while fn(calls) runs."""
    L = N.lib()
    ms, cnt = (C.c_double * 8)(), (C.c_longlong * 8)()
    torch.cuda.synchronize()
    L.iq_prof_enable(1)
    L.iq_prof_collect(ms, cnt)
    L.iq_prof_kernels(None, 0, 1)
    try:
        fn(calls)
        L.iq_prof_collect(ms, cnt)
    finally:
        L.iq_prof_enable(0)
    need = L.iq_prof_kernels(None, 0, 0)
    buf = C.create_string_buffer(need + 1)
    L.iq_prof_kernels(buf, need + 1, 1)
    out = {}
    for line in buf.value.decode().splitlines():
        f = line.split("\t")
        out[f[0].split("<")[0]] = float(f[3]) / max(1, int(f[2]))       # without the template arguments
    return out


class Eager:
    """The operation of CyclicSpectrum in torch ops on the device (complex64)."""

    def __init__(self, cs, device):
        n, T = cs.n_fft, cs.columns
        self.cs = cs
        t = torch.from_numpy(cs.table).to(device)
        self.E = torch.complex(t[0], -t[1])                                  # w[m] exp(-2 pi i k m / n), (m, k)
        j0 = np.arange(T, dtype=np.int64) * cs.hop - cs.pad
        r = (np.arange(n, dtype=np.int64)[None, :] * (j0 % n)[:, None]) % n
        rot = torch.from_numpy(cs.rot).to(device)
        r = torch.from_numpy(r).to(device)
        self.rot = torch.complex(rot[0][r], -rot[1][r])                       # (T, k)
        self.right = max(0, int(j0[-1]) + n - cs.length)
        h = (np.arange(n) + n // 2) % n
        k = np.broadcast_to(h[None, :], (n, n))
        a = h[:, None]
        self.k = torch.from_numpy(np.ascontiguousarray(k)).to(device)
        self.l_scf = torch.from_numpy((k - a) % n).to(device)
        self.l_conj = torch.from_numpy((a - k) % n).to(device)

    def __call__(self, x):
        cs = self.cs
        z = torch.nn.functional.pad(torch.complex(x[:, 0], x[:, 1]), (cs.pad, self.right))
        Y = (z.unfold(1, cs.n_fft, cs.hop)[:, :cs.columns] @ self.E) * self.rot
        D = (Y.real ** 2 + Y.imag ** 2).sum(dim=1)
        Yt = Y.transpose(1, 2)
        inv2 = cs.inv_norm ** 2
        den = D[:, self.k] * inv2
        out = []
        for G, l in ((Yt @ Y.conj(), self.l_scf), (Yt @ Y, self.l_conj)):
            g = G[:, self.k, l]
            P = (g.real ** 2 + g.imag ** 2) * inv2
            out.append(P / (den * D[:, l] + cs.floor) * cs.scale + cs.shift)
        return torch.stack(out, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cyclic.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cyclic_prof.py measures on an MI355X"
    d = torch.device("cuda:0")
    length, batch = 1024, 256
    fs = FrameSynth(length=length, seed=1)
    x = SynthStream(fs, fs.stats(n_subset=1024), "rawiq", batch).get(0)[0]
    legs, flops, kernels = [], {}, {}
    for n_fft in (64, 224):
        cs = CyclicSpectrum(n_fft, length)
        spec = Spectrogram(n_fft, n_fft, length)
        eager = Eager(cs, d)
        diff = float((cs(x) - eager(x)).abs().max())
        spec(x)

        def cyc(calls, cs=cs):
            for _ in range(calls):
                cs(x)

        def spc(calls, spec=spec):
            with torch.no_grad():
                for _ in range(calls):
                    spec(x)

        def tor(calls, eager=eager):
            with torch.no_grad():
                for _ in range(calls):
                    eager(x)
        names = (f"cyclic both/coherence  n_fft {n_fft} hop {cs.hop} T {cs.columns}",
                 f"spectrogram forward    {n_fft}x{n_fft} hop {spec.hop} pad {spec.pad}",
                 f"torch eager cyclic     n_fft {n_fft} (max |kernel - eager| {diff:.1e})")
        legs += [(names[0], cyc, 200), (names[1], spc, 200), (names[2], tor, 20)]
        T = cs.columns
        flops[names[0]] = batch * 24.0 * T * n_fft * n_fft
        flops[names[1]] = batch * 8.0 * n_fft * n_fft * n_fft
        kernels[names[0]], kernels[names[1]] = "cyclic_kernel", "spectrogram_fwd_kernel"
    for _, fn, calls in legs:                    # warm-up: code objects, clocks, torch's algorithm choices
        train_ms(fn, calls)
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, calls in legs:
            times[name].append(train_ms(fn, calls))
    kms = {name: kernel_ms(fn, 50).get(kernels[name]) for name, fn, _ in legs if name in kernels}
    lines = [f"device: {torch.cuda.get_device_name(0)}; batches of {batch} frames of {length} complex samples; call ms: device "
             f"events around a train of calls, median (min) over {args.rounds} interleaved rounds; kernel ms: event pair around "
             f"each launch, mean of 50; TF and share of the {PEAK_F32_MFMA / 1e12:.0f} TF fp32-input MFMA peak from the kernel ms and "
             "the flops the kernel executes",
             f"{'leg':<62} {'call ms':>18} {'kernel ms':>10} {'TF':>8} {'of peak':>8}"]
    for name, _, _ in legs:
        med = statistics.median(times[name])
        line = f"{name:<62} {med:>9.4f} ({min(times[name]):>7.4f})"
        if kms.get(name) is not None:
            tf = flops[name] / (kms[name] * 1e-3) / 1e12
            line += f" {kms[name]:>10.4f} {tf:>8.2f} {100 * tf * 1e12 / PEAK_F32_MFMA:>7.1f}%"
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
