"""Host time of one call through a front-end object (profiles/frontend_refactor.txt): microseconds per call of front(x) and of
front(x).sum().backward() for Spectrogram, CyclicSpectrum and Constellation, each at the smallest geometry of its exact test
and B = 1, so that the launch is negligible and what is timed is the Python path (checks, autograd function, struct, ctypes
call).  Host clock around 2,000 calls after a warm-up, one synchronisation at the end.  One JSON line per run; --tree names the
checkout whose package is imported, so that two trees can be timed alternately, one process per run."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=2000)
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

from vit_vs_raw_iq_amd import Constellation, CyclicSpectrum, Spectrogram  # noqa: E402

d = torch.device("cuda:0")
FRONTS = {"spectrogram": Spectrogram(32, 1, 100, hop=1, pad=0),
          "cyclic": CyclicSpectrum(32, 100, hop=1, pad=0, columns=1, differentiable=True),
          "constellation": Constellation(32, 32, 1, profile="triangle", n_frac=2)}


def timed(fn, calls):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


out = {"label": args.label, "calls": args.calls}
for name, front in FRONTS.items():
    x = torch.randn(1, 2, front.length, device=d)
    xg = x.clone().requires_grad_(True)
    out[name + "_fwd_us"] = round(timed(lambda: front(x), args.calls), 2)
    out[name + "_fwd_bwd_us"] = round(timed(lambda: front(xg).sum().backward(), args.calls), 2)
print(json.dumps(out))
