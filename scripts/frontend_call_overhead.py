"""Host time of one call through a front-end or stage object (profiles/frontend_refactor.txt, profiles/stage_refactor.txt):
microseconds per call of obj(x) and, where the object is differentiable, of obj(x).sum().backward().  --what fronts: Spectrogram,
CyclicSpectrum and Constellation, each at the smallest geometry of its exact test; --what stages: Receiver, Carrier, Equaliser and
LikelihoodClassifier, each at the smallest geometry its entry point accepts.  B = 1 throughout, so that the launch is negligible
and what is timed is the Python path (checks, autograd function, struct, ctypes call).  Host clock around 2,000 calls after a
warm-up, one synchronisation at the end.  One JSON line per run; --tree names the checkout whose package is imported, so that
two trees can be timed alternately, one process per run."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=2000)
ap.add_argument("--label", default="")
ap.add_argument("--what", choices=("fronts", "stages"), default="fronts")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

import vit_vs_raw_iq_amd as P  # noqa: E402

d = torch.device("cuda:0")
# name -> (the object, the shape of its x, the keywords of a call, differentiable)
OBJECTS = {
    "fronts": lambda: {
        "spectrogram": (P.Spectrogram(32, 1, 100, hop=1, pad=0), (1, 2, 100), {}, True),
        "cyclic": (P.CyclicSpectrum(32, 100, hop=1, pad=0, columns=1, differentiable=True), (1, 2, 100), {}, True),
        "constellation": (P.Constellation(32, 32, 1, profile="triangle", n_frac=2), (1, 2, 1), {}, True)},
    "stages": lambda: {
        "receiver": (P.Receiver(2, span=1, n_frac=1, timing="energy"), (1, 8, 2), {}, True),
        "carrier": (P.Carrier(32, n_dft=(32, 32)), (1, 2, 32), {}, True),
        "equaliser": (P.Equaliser(8, taps=1, iters=1), (1, 8, 2), {}, True),
        "likelihood": (P.LikelihoodClassifier(8, classes=["BPSK"], rotations=1), (1, 8, 2), dict(sigma2=1.0), False)},
}[args.what]()


def timed(fn, calls):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


out = {"label": args.label, "what": args.what, "calls": args.calls}
for name, (obj, shape, kw, differentiable) in OBJECTS.items():
    x = torch.randn(shape, device=d)
    out[name + "_fwd_us"] = round(timed(lambda: obj(x, **kw), args.calls), 2)
    if differentiable:
        xg = x.clone().requires_grad_(True)
        out[name + "_fwd_bwd_us"] = round(timed(lambda: obj(xg, **kw).sum().backward(), args.calls), 2)
print(json.dumps(out))
