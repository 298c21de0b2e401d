"""fp64 definition of the encoder-layer tail (everything after the attention core), stage by stage, for the tests.

Plain torch in float64, on whatever device its operands live on; no native library.  It restates, one product at a time, what
include/iqvit.h documents for iq_attn_out_ffn_chain_fwd, iq_ffn_chain_bwd and iq_qkv_dgrad_ffn_chain_bwd
(EncoderLayer.forward, encoder_layer.py:24-33, and its autograd):

  forward    Z1 = m0 s (A Wo^T + bo) + R          X1, mean1, rstd1 = LN(Z1)       H  = m1 s relu(X1 W1^T + b1)
             Z2 = m2 s (H W2^T + b2) + X1         X,  mean2, rstd2 = LN(Z2)       Yq = X Wq^T + bq
  backward   dX2 = gQKV Wqkv_t^T + residual0      dz2 = LN'(dX2; z2 ...)          dy2 = m2 s dz2
             gH  = (H > 0) s (dy2 W2t^T)          dX1 = gH W1t^T + residual       dz = LN'(dX1; z1 ...)   dy = m0 s dz
             dA  = dy Wot^T                       dgamma = colsum(dX xhat), dbeta = colsum(dX)

m0, m1, m2 are keep masks of tests/dropout_ref.py (host Philox) and s its quantised scale.  Every function takes its inputs as
given, so a GPU test can hand each stage the kernel's OWN stored (bf16-rounded) input of that stage: the stage's error is then
one bf16 rounding plus fp32 accumulation and the suite's per-kernel tolerances apply unchanged.  tail_forward / tail_backward
compose the stages without any rounding; tests/test_chain_ref_cpu.py checks that composition against torch.autograd of the
directly written expression, which is what entitles the GPU tests to trust the stages.

MaskInjector is the dropout of oracle/iq_oracle.py with the masks handed in instead of drawn: the model plan's dropout-on step
can then be compared with the oracle element by element.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from dropout_ref import dropout_scale, dropout_thresh, keep_groups, keep_mask

EPS = 1e-12                                   # LayerNorm.forward, layers_norm.py:11-19


def f64(t):
    return t.to(torch.float64)


_CHUNK = 1 << 17                              # groups of 8 elements per piece of work


def keep_mask_chunked(seed, step, site, p, n_elements):
    """dropout_ref.keep_mask(seed, step, site, p, n_elements), computed in pieces on a few threads (numpy releases the GIL):
    the 25 million hidden units of a 32,899-row batch take 0.2 s instead of 1.3 s.  p == 0 keeps everything (thresh 0)."""
    if dropout_thresh(p) == 0:
        return np.ones(n_elements, dtype=bool)
    groups = (n_elements + 7) // 8
    if groups <= _CHUNK:
        return keep_mask(seed, step, site, p, n_elements)
    out = np.empty(groups * 8, dtype=bool)

    def piece(lo):
        hi = min(lo + _CHUNK, groups)
        out[lo * 8:hi * 8] = keep_groups(seed, step, site, p, np.arange(lo, hi, dtype=np.uint64)).reshape(-1)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(piece, range(0, groups, _CHUNK)))
    return out[:n_elements]


def host_mask(seed, step, site, p, M, N, device=None):
    """The keep mask of dropout site (seed, step, site) over a row-major [M, N] tensor -> bool [M, N]."""
    m = torch.from_numpy(np.ascontiguousarray(keep_mask_chunked(seed, step, site, p, M * N))).view(M, N)
    return m if device is None else m.to(device)


def scale64(p):
    """dropout_scale(p): the fp32 value the kernels multiply by, as a Python float (exact in fp64)."""
    return float(dropout_scale(p))


# ------------------------------------------------------------------------------------------------
# stages
# ------------------------------------------------------------------------------------------------
def linear_drop_residual(A, W, b, keep, s, R):
    """keep * s * (A W^T + b) + R: Z1 (A = attention output, R = layer input) and Z2 (A = H, R = X1)."""
    return keep * (s * (f64(A) @ f64(W).t() + f64(b))) + f64(R)


def layer_norm(z, gamma, beta, eps=EPS):
    """-> x, mean [M], rstd [M]; biased variance."""
    z = f64(z)
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return f64(gamma) * ((z - mean) * rstd) + f64(beta), mean.squeeze(-1), rstd.squeeze(-1)


def hidden(X1, W1, b1, keep, s):
    """H = keep * s * relu(X1 W1^T + b1)."""
    return keep * (s * torch.relu(f64(X1) @ f64(W1).t() + f64(b1)))


def linear(X, W, b):
    """Yq = X Wq^T + bq."""
    return f64(X) @ f64(W).t() + f64(b)


def dgrad_residual(G, Wt, R):
    """dX = G Wt^T + R with Wt the TRANSPOSED weight [D, K]: dX2 (G = gQKV, Wt = Wqkv_t) and dX1 (G = gH, Wt = W1t)."""
    return f64(G) @ f64(Wt).t() + f64(R)


def layer_norm_bwd(dx, z, mean, rstd, gamma):
    """Backward of x = gamma * (z - mean) * rstd + beta for upstream dx, with the stored statistics:
    -> dz = rstd * (g - mean_D(g) - xhat * mean_D(g * xhat)), g = dx * gamma;  dgamma = colsum(dx * xhat);  dbeta = colsum(dx)."""
    dx = f64(dx)
    xhat = (f64(z) - f64(mean).unsqueeze(-1)) * f64(rstd).unsqueeze(-1)
    g = dx * f64(gamma)
    dz = f64(rstd).unsqueeze(-1) * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    return dz, (dx * xhat).sum(0), dx.sum(0)


def drop_bwd(dz, keep, s):
    """dy = keep * s * dz."""
    return keep * (s * f64(dz))


def gate_grad(dO, W2t, H_fwd, s):
    """gH = (H_fwd > 0) * s * (dO W2t^T), W2t [F, D]: the gradient at the FFN1 pre-activation ("H > 0" is ReLU and dropout1
    of the forward pass at once)."""
    return (f64(H_fwd) > 0) * (s * (f64(dO) @ f64(W2t).t()))


def out_proj_dgrad(dy, Wot):
    """dA = dy Wot^T, Wot [D, D] = Wo transposed."""
    return f64(dy) @ f64(Wot).t()


# ------------------------------------------------------------------------------------------------
# the stages composed, nothing rounded
# ------------------------------------------------------------------------------------------------
def tail_forward(A, R, w, masks, s):
    """w: dict Wo bo g1 be1 W1 b1 W2 b2 g2 be2 Wq bq;  masks = (m0, m1, m2) -> dict of every stage output."""
    m0, m1, m2 = masks
    o = {}
    o["Z1"] = linear_drop_residual(A, w["Wo"], w["bo"], m0, s, R)
    o["X1"], o["mean1"], o["rstd1"] = layer_norm(o["Z1"], w["g1"], w["be1"])
    o["H"] = hidden(o["X1"], w["W1"], w["b1"], m1, s)
    o["Z2"] = linear_drop_residual(o["H"], w["W2"], w["b2"], m2, s, o["X1"])
    o["X"], o["mean2"], o["rstd2"] = layer_norm(o["Z2"], w["g2"], w["be2"])
    o["Yq"] = linear(o["X"], w["Wq"], w["bq"])
    return o


def tail_backward(fwd, gQKV, residual0, w, masks, s):
    """Gradient of sum(Yq * gQKV) + sum(X * residual0) through tail_forward's stages, in the kernels' order and with their
    operands (transposed weights, residual = dz2) -> dict dz2 dy2 gH dz dy dA dgamma2 dbeta2 dgamma1 dbeta1."""
    m0, m1, m2 = masks
    o = {}
    dX2 = dgrad_residual(gQKV, f64(w["Wq"]).t(), residual0)                    # Wqkv_t [D, 3D] = Wq^T
    o["dz2"], o["dgamma2"], o["dbeta2"] = layer_norm_bwd(dX2, fwd["Z2"], fwd["mean2"], fwd["rstd2"], w["g2"])
    o["dy2"] = drop_bwd(o["dz2"], m2, s)
    o["gH"] = gate_grad(o["dy2"], f64(w["W2"]).t(), fwd["H"], s)               # W2t [F, D]
    dX1 = dgrad_residual(o["gH"], f64(w["W1"]).t(), o["dz2"])                  # W1t [D, F]
    o["dz"], o["dgamma1"], o["dbeta1"] = layer_norm_bwd(dX1, fwd["Z1"], fwd["mean1"], fwd["rstd1"], w["g1"])
    o["dy"] = drop_bwd(o["dz"], m0, s)
    o["dA"] = out_proj_dgrad(o["dy"], f64(w["Wo"]).t())                        # Wot [D, D]
    return o


# ------------------------------------------------------------------------------------------------
# the oracle's dropout with the masks handed in
# ------------------------------------------------------------------------------------------------
class MaskInjector:
    """Stands in for iq_oracle._dropout(x, p, train).  Call k (k = 0, 1, 2, ...) multiplies x by mask_fn(k, x.shape) and by
    `scale`: the oracle draws its masks in the order of the plan's site ids -- the embedding (encoder_forward) is site 0, and
    in layer l `_dropout(a)` is 1 + 3l, feed_forward's is 2 + 3l, the last is 3 + 3l -- so k IS the site.  x is [B, S, D] (or
    [B, S, F]) row-major: element (b, s, n) is element (b * S + s) * N + n of the plan's [B * S, N] activation, the class token
    row included.  train = False passes x through, as the oracle does.  `calls` records (site, (B * S, N))."""

    def __init__(self, mask_fn, scale):
        self.mask_fn, self.scale, self.calls = mask_fn, scale, []

    def __call__(self, x, p, train):
        if not train:
            return x
        site = len(self.calls)
        self.calls.append((site, (x.numel() // x.shape[-1], x.shape[-1])))     # as the plan sees it: [B * S, N]
        keep = self.mask_fn(site, tuple(x.shape))
        return x * keep.to(x.dtype) * self.scale


def philox_injector(seed, step, p):
    """The injector that hands out dropout_ref's masks for (seed, step, site) and its quantised scale -- not 1 / (1 - p)."""
    def mask_fn(site, shape):
        n = int(np.prod(shape))
        return torch.from_numpy(np.ascontiguousarray(keep_mask_chunked(seed, step, site, p, n))).view(shape)
    return MaskInjector(mask_fn, float(dropout_scale(p)))
