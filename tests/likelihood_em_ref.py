"""What tests/test_likelihood_em_cpu.py and tests/test_gpu_likelihood_em.py share: the mixture log-likelihood of one frame restated
on plain numpy (numpy.logaddexp) with its (h, v) maximiser, the integer cases that are exact in fp32, the real cases, the 20 dB
decision set with an unknown gain per frame, and the fp32 error bound of the device's EM.  A plain helper module like the other
*_ref.py files; the notation and the first half of the derivation are tests/likelihood_ref.py's.

THE ONE-PASS BOUND.  u = 2^-24.  The device follows include/iqvit.h operation by operation and the fp64 definition is handed the
same fp32 numbers (frames, points, starts, f0, floor and, where given, h0 and v0), so only the arithmetic differs.  To first order
in u, for one frame, class and start at a state (h, v) that both sides hold EXACTLY:

  scaled point    p_k = h s_k, each component a product and an fmaf, |Re h Re s| + |Im h Im s| <= |h| |s|:      |dp| <= 2 u |h| |s|
  difference      Re y - Re p_k: the error above and its own rounding (y is exact: nothing rotates it here):
                                                                              |d(dr)| <= e0 + u |dr|,  e0 = 2 u |h| max|s|
  distance, minimum, q, q2, exponent, exp2, S
                  as in likelihood_ref.py:  eps(d) = 2 sqrt(2 d) e0 + 4 u d;  term k has the relative error
                  r_k = q (eps(d_min) + eps(d_k)) + 5 u q (d_k - d_min) + 2 u;  S has sigma = sum_k e_k r_k / S + (M - 1) u
  the last pass   l_n and L as there (no rotation, 1 / M and the product 2 u):
                  EL = sum_n ( q eps(d_min) + u q d_min + sigma + 2 u + 4 u max(|ln(S / M)|, 1) + u |l_n| ) + (ceil(len / 64) + 6) u sum_n |l_n|
  Lambda          log2 v: 2 u max(|log2 v|, 1);  LOG2PI + .: the constant and the sum;  LN2 * .: the constant and the product;  the
                  fmaf:   Easm = len u (2 ln2 max(|log2 v|, 1) + 4 |ln(pi v)| + 2) + u |Lambda|
  point-sums      W = sum_k e_k c_k by M fmaf, c in (Re s, Im s, ss, d), ss_k with 2 u ss_k of its own and d_k with eps(d_k):
                  |dW| <= sum_k e_k |c_k| r_k + sum_k e_k |dc_k| + M u sum_k e_k |c_k|
  r, g            r = 1 / S: sigma + u;  g = W r: one more u.  With G = sum_k e_k |c_k| / S (>= |g|):
                  dg = (sum_k e_k |c_k| r_k + sum_k e_k |dc_k|) / S + G (M u + sigma + 2 u)
  over the symbols  two fmaf per symbol and lane and the butterfly, D = 2 ceil(len / 64) + 6 roundings deep, each below u times the
                  sum of the absolute terms:     EAr = sum_n (|Re y| dgr + |Im y| dgi) + D u sum_n (|Re y| Gr + |Im y| Gi),
                  EAi alike with Re y and Im y exchanged, EBq = sum_n dgB + D u sum_n GB, EV = sum_n dgV + D u sum_n GV
  update          h' = A / Bq:  Eh_c = EA_c / Bq + |A_c| EBq / Bq^2 + u |h'_c|,  Eh = |(Ehr, Ehi)|
                  t = V / len:  Et = EV / len + u t;   vfloor = floor M2 has (ceil(len / 64) + 10) u vfloor;  the larger of two
                  perturbed values moves by no more than the larger perturbation:  Ev = max(Et, Evfloor)

A STATE THAT IS NOT EXACT.  Lambda is differentiable in the state, and at (h, v) its gradient is known from the pass itself:
  dLambda / dv = (V - len v) / v^2,   dLambda = 2 Re(conj(dh) (A - h Bq) / v)   with A, Bq, V the update sums at (h, v).
So a state known to (Eh, Ev) only adds  2 q |A - h Bq| Eh + |V - len v| / v^2 Ev  to the bound of Lambda, to first order.  That
covers (a) the table's starts -- M2 has (ceil(len / 64) + 9) u, v0 = f0 M2 one more, a = sqrt(M2 - v0) half of the difference's
error plus its own u, h0 = a (c_t, s_t) one more: Ev0 = v0 (ceil(len / 64) + 10) u, Eh0 = |h0| (0.5 (M2 + v0) (ceil(len / 64) + 10)
/ (M2 - v0) + 2.5) u -- and (b) ONE step: Lambda after one update is bounded by its own pass plus the gradient times the update's
(Eh, Ev).  Both are derived; neither holds a measured number.

SEVERAL STEPS.  The EM map's Jacobian has no such closed form, and the slowly converging starts amplify.  No factor is invented:
`reference_and_bound(inject=(phi, sign))` runs the fp64 definition with a perturbation of the one-pass bound's size -- (Eh e^{j phi},
sign Ev), the bounds being those a clean run recorded at the same step, which are the perturbed run's own to first order -- added
to the state after EVERY update (and to the table's starts), and `amplification` takes the deviation of every start's final
(h, v, Lambda) from the clean run over such patterns (eight of them on the bounded cases, two on the decision set and the chain), relative to the one-pass bounds of the final update and
the last pass (Eh, Ev, ELam above).  tests/test_likelihood_em_cpu.py asserts, on the very inputs of the GPU suite, that twice that
ratio stays below FACTOR (the injected perturbation is first-order, hence the margin of
two); the GPU suite allows FACTOR times the one-pass bounds.  The measured ratios are recorded in profiles/likelihood_em.txt.

The bounds are multiplied by 1 + 2^-10 for the second-order terms.
"""
import functools

import numpy as np
import torch

from likelihood_ref import SLACK, U, f32, from_complex, in_layout, margin, random_table, real_frames, to_complex  # noqa: F401

# allowance of a run of several steps / the one-pass bounds of its final step: pinned by the CPU test at no less than twice the
# measured ratios, which are recorded in profiles/likelihood_em.txt.  Bounded cases, 8 steps, eight patterns: at most 38.2 for the
# winning start's state and 26.8 for any start's Lambda.  Decision set, 32 steps, every frame, two patterns: 139.3 for any start's
# Lambda (the state of a winning start near the boundary of two basins deviates up to 710 times: on that set the suite holds
# Lambda and the decisions to the allowance, not the state).
FACTOR = 512.0
# The chain's frames (512 symbols, 32 steps) exist on the device only: tests/test_gpu_likelihood_em.py measures them in the same
# way where it uses them (266.3 with two patterns) and asserts twice that below this.
CHAIN_FACTOR = 1024.0
BOUNDED_ITERS = 8
PATTERNS = tuple((phi, sign) for phi in (0.0, 0.5 * np.pi, np.pi, 1.5 * np.pi) for sign in (1.0, -1.0))


# ---- the direct statement
def loglik_plain(y, pts, h, v):
    """sum_n log( (1 / M) sum_k exp(-|y_n - h s_k|^2 / v) / (pi v) ) of ONE frame (complex y (n,)), one class (complex pts (M,))
    at one state, with numpy.logaddexp over k and nothing taken out first."""
    e = -np.abs(np.asarray(y)[:, None] - h * np.asarray(pts)[None, :]) ** 2 / v
    return float(np.sum(np.logaddexp.reduce(e, axis=1) - np.log(len(pts)) - np.log(np.pi * v)))


def update_plain(y, pts, h, v):
    """One ECM step stated directly: the responsibilities w_nk at (h, v) by a softmax; h' minimises sum w_nk |y_n - h s_k|^2 (a
    weighted least-squares fit); v' is that weighted distance at the OLD h, per symbol."""
    y, pts = np.asarray(y), np.asarray(pts)
    d = np.abs(y[:, None] - h * pts[None, :]) ** 2
    w = np.exp(-d / v - np.logaddexp.reduce(-d / v, axis=1)[:, None])
    h1 = np.sum(w * y[:, None] * np.conj(pts)[None, :]) / np.sum(w * np.abs(pts[None, :]) ** 2)
    return h1, float(np.sum(w * d) / len(y))


# ---- one pass of the fp64 definition, with the bound
def _pass(yre, yim, sr, si, hr, hi, v, bound):
    """yre, yim (b, n); sr, si (M,); hr, hi, v (b, T) -> dict of the update sums A (complex parts), Bq, V, of L and Lambda (b, T)
    and, with bound, EAr, EAi, EBq, EV, ELam0 (the last pass's own arithmetic) and the gradient sizes Gh, Gv."""
    M, n = len(sr), yre.shape[1]
    ss = sr * sr + si * si
    pr = hr[..., None] * sr - hi[..., None] * si
    pi = hr[..., None] * si + hi[..., None] * sr
    dr = yre[:, None, :, None] - pr[:, :, None, :]
    di = yim[:, None, :, None] - pi[:, :, None, :]
    d = dr * dr + di * di                                                           # (b, T, n, M)
    dmin = d.amin(dim=3)
    q = (1.0 / v)[..., None]                                                        # (b, T, 1)
    gap = d - dmin[..., None]
    e = torch.exp(-q[..., None] * gap)
    S = e.sum(dim=3)
    gr, gi = (e * sr).sum(dim=3) / S, (e * si).sum(dim=3) / S
    yr_, yi_ = yre[:, None], yim[:, None]
    out = dict(Ar=(yr_ * gr + yi_ * gi).sum(dim=2), Ai=(yi_ * gr - yr_ * gi).sum(dim=2), Bq=((e * ss).sum(dim=3) / S).sum(dim=2),
               V=((e * d).sum(dim=3) / S).sum(dim=2))
    lg = torch.log(S / M)
    ln = -q * dmin + lg
    out["L"] = ln.sum(dim=2)
    out["Lam"] = out["L"] - n * torch.log(np.pi * v)
    if not bound:
        return out
    e0 = (2.0 * U * torch.sqrt(hr * hr + hi * hi) * float(ss.max().sqrt()))[..., None]      # (b, T, 1)
    eps = lambda t, w: 2.0 * torch.sqrt(2.0 * t) * w + 4.0 * U * t                  # noqa: E731
    epsmin, epsd = eps(dmin, e0), eps(d, e0[..., None])
    rk = q[..., None] * (epsmin[..., None] + epsd) + 5.0 * U * q[..., None] * gap + 2.0 * U
    sig = (e * rk).sum(dim=3) / S + (M - 1) * U
    d1, d2 = -(-n // 64) + 6, 2 * -(-n // 64) + 6
    En = q * epsmin + U * q * dmin + sig + 2.0 * U + 4.0 * U * torch.clamp(lg.abs(), min=1.0) + U * ln.abs()
    lam = out["Lam"]
    asm = n * U * (2.0 * np.log(2.0) * torch.clamp(torch.log2(v).abs(), min=1.0) + 4.0 * torch.log(np.pi * v).abs() + 2.0) + U * lam.abs()
    out["ELam0"] = SLACK * (En.sum(dim=2) + d1 * U * ln.abs().sum(dim=2) + asm)

    def dg(cabs, dc):
        G = (e * cabs).sum(dim=3) / S
        return ((e * cabs * rk).sum(dim=3) + (e * dc).sum(dim=3)) / S + G * (M * U + sig + 2.0 * U), G
    zero = torch.zeros(())
    dgr, Gr = dg(sr.abs(), zero)
    dgi, Gi = dg(si.abs(), zero)
    dgB, GB = dg(ss, 2.0 * U * ss)
    dgV, GV = dg(d, epsd)
    ya, yb = yr_.abs(), yi_.abs()
    out["EAr"] = SLACK * ((ya * dgr + yb * dgi).sum(dim=2) + d2 * U * (ya * Gr + yb * Gi).sum(dim=2))
    out["EAi"] = SLACK * ((yb * dgr + ya * dgi).sum(dim=2) + d2 * U * (yb * Gr + ya * Gi).sum(dim=2))
    out["EBq"] = SLACK * (dgB.sum(dim=2) + d2 * U * GB.sum(dim=2))
    out["EV"] = SLACK * (dgV.sum(dim=2) + d2 * U * GV.sum(dim=2))
    rr, ri = out["Ar"] - hr * out["Bq"], out["Ai"] - hi * out["Bq"]
    out["Gh"] = 2.0 * torch.sqrt(rr * rr + ri * ri) / v
    out["Gv"] = (out["V"] - n * v).abs() / (v * v)
    return out


def _alive(hr, hi, v):
    return torch.isfinite(hr) & torch.isfinite(hi) & (v >= 2.0 ** -126) & torch.isfinite(v)      # (v a normal fp32 number)


def reference_and_bound(x, points, classes, starts, iters, f0, floor, h0=None, v0=None, planar=False, inject=None, steps=None,
                        record=False):
    """The definition on the fp32 numbers the device is handed, in fp64 (torch on the host), and the bounds derived above.
    points (P, 2), classes (offset, count), starts the (T, 2) table; h0 (B, C, 2) and v0 (B, C): the given start.  inject: None or
    (phi, sign), the perturbation added to the state after every update (module docstring); its sizes are `steps`, the (Ehs, Evs)
    a clean run with record=True returned: the one-pass bounds (iters + 1, B, C, T) of the table's starts and of every update.
    -> dict, per START (B, C, T): start_ll, H (complex), V and the one-pass bounds Eh, Ev (of the final update; of the table's
    start where iters = 0; 0 for a given start with iters = 0) and ELam (the last pass, with the gradient terms for (Eh, Ev));
    per CLASS (B, C): best_start, loglik, h, v, and Ehb, Evb, Ell, the bounds of the winning start; pred (B,)."""
    y = to_complex(x, planar)
    B, n = y.shape
    p = np.asarray(points, np.float64).reshape(-1, 2)
    f0, floor = float(f0), float(floor)
    Cn = len(classes)
    M2 = np.mean(y.real ** 2 + y.imag ** 2, axis=1)                             # (not numpy.abs: its square root rounds)
    d1 = -(-n // 64) + 6
    if h0 is None:
        st = np.asarray(starts, np.float64).reshape(-1, 2) @ np.array([1, 1j])
        T = len(st)
        v00 = f0 * M2
        H0 = np.broadcast_to((np.sqrt(M2 - v00)[:, None] * st[None, :])[:, None, :], (B, Cn, T))
        V0 = np.broadcast_to(v00[:, None, None], (B, Cn, T))
        EV0 = V0 * (d1 + 4) * U * SLACK
        EH0 = np.abs(H0) * (0.5 * ((M2 + v00) / (M2 - v00))[:, None, None] * (d1 + 4) + 2.5) * U * SLACK
    else:
        H0 = (np.asarray(h0, np.float64).reshape(B, Cn, 2) @ np.array([1, 1j]))[..., None]
        V0 = np.asarray(v0, np.float64).reshape(B, Cn, 1)
        T, EV0, EH0 = 1, np.zeros((B, Cn, 1)), np.zeros((B, Cn, 1))
    vfl = torch.from_numpy(floor * M2)
    Evfl = vfl * (d1 + 4) * U * SLACK
    yre, yim = torch.from_numpy(y.real.copy()), torch.from_numpy(y.imag.copy())
    res = {k: np.empty((B, Cn, T)) for k in ("start_ll", "V", "Eh", "Ev", "ELam")}
    res["H"] = np.empty((B, Cn, T), np.complex128)
    nan = torch.tensor(float("nan"), dtype=torch.float64)
    kick = None if inject is None else (np.cos(inject[0]), np.sin(inject[0]), inject[1])
    if record:
        res["Ehs"], res["Evs"] = np.empty((iters + 1, B, Cn, T)), np.empty((iters + 1, B, Cn, T))
    for c, (off, M) in enumerate(classes):
        sr, si = torch.from_numpy(p[off:off + M, 0].copy()), torch.from_numpy(p[off:off + M, 1].copy())
        step = max(1, (1 << 21) // (T * n * M))
        for b0 in range(0, B, step):
            sl = slice(b0, b0 + step)
            hr, hi = torch.from_numpy(H0[sl, c].real.copy()), torch.from_numpy(H0[sl, c].imag.copy())
            v = torch.from_numpy(V0[sl, c].copy())
            Eh, Ev = torch.from_numpy(EH0[sl, c].copy()), torch.from_numpy(EV0[sl, c].copy())
            if record:
                res["Ehs"][0, sl, c], res["Evs"][0, sl, c] = Eh.numpy(), Ev.numpy()
            if kick is not None:
                hr, hi, v = hr + kick[0] * Eh, hi + kick[1] * Eh, v + kick[2] * Ev
            for k in range(iters + 1):
                ok = _alive(hr, hi, v)
                hr, hi, v = torch.where(ok, hr, nan), torch.where(ok, hi, nan), torch.where(ok, v, nan)
                P = _pass(yre[sl], yim[sl], sr, si, hr, hi, v, bound=record or k >= iters - 1)
                if k == iters:
                    break
                Bq = P["Bq"]
                nr, ni, t = P["Ar"] / Bq, P["Ai"] / Bq, P["V"] / n
                if "EAr" in P:
                    Ehr = P["EAr"] / Bq + P["Ar"].abs() * P["EBq"] / (Bq * Bq) + U * nr.abs()
                    Ehi = P["EAi"] / Bq + P["Ai"].abs() * P["EBq"] / (Bq * Bq) + U * ni.abs()
                    Eh = torch.sqrt(Ehr * Ehr + Ehi * Ehi)
                    Ev = torch.maximum(P["EV"] / n + U * t, Evfl[sl, None].expand_as(t))
                hr, hi, v = nr, ni, torch.where(t < vfl[sl, None], vfl[sl, None], t)
                if record:
                    res["Ehs"][k + 1, sl, c], res["Evs"][k + 1, sl, c] = Eh.numpy(), Ev.numpy()
                if kick is not None:
                    kh, kv = torch.from_numpy(steps[0][k + 1, sl, c].copy()), torch.from_numpy(steps[1][k + 1, sl, c].copy())
                    hr, hi, v = hr + kick[0] * kh, hi + kick[1] * kh, v + kick[2] * kv
            res["start_ll"][sl, c], res["H"][sl, c], res["V"][sl, c] = P["Lam"].numpy(), (hr + 1j * hi).numpy(), v.numpy()
            res["Eh"][sl, c], res["Ev"][sl, c] = Eh.numpy(), Ev.numpy()
            res["ELam"][sl, c] = (P["ELam0"] + SLACK * (P["Gh"] * Eh + P["Gv"] * Ev)).numpy()
    return {**res, **over_starts(res)}


def first_valid_largest(v, axis):
    """Index of the first largest along `axis`, NaNs passed over, and the value; (-1, NaN) where all are NaN (the kernel's walk)."""
    v = np.moveaxis(v, axis, 0)
    at, best = np.full(v.shape[1:], -1, np.int64), np.full(v.shape[1:], np.nan)
    for i in range(len(v)):
        with np.errstate(invalid="ignore"):
            up = ~np.isnan(v[i]) & ((at < 0) | (v[i] > best))
        at[up], best[up] = i, v[i][up]
    return at, best


def over_starts(res):
    """The winner of every (frame, class) and of every frame, with the winning start's bounds."""
    best, loglik = first_valid_largest(res["start_ll"], 2)
    at = np.maximum(best, 0)[..., None]
    pick = lambda a, bad: np.where(best >= 0, np.take_along_axis(a, at, 2)[..., 0], bad)                # noqa: E731
    pred, _ = first_valid_largest(loglik, 1)
    return dict(best_start=best, loglik=loglik, h=pick(res["H"], complex(np.nan, np.nan)), v=pick(res["V"], np.nan), Ehb=pick(res["Eh"], np.nan),
                Evb=pick(res["Ev"], np.nan), Ell=pick(res["ELam"], np.nan), pred=pred)


def start_ties(ref, factor):
    """ties[b, c, t]: start t is within the two allowances of the largest -- the device may take it for the maximum.  Starts that
    converge to the images of one optimum under the class's rotational symmetry are equal maxima in exact arithmetic."""
    L, E = ref["start_ll"], factor * ref["ELam"]
    m = np.nanmax(L, axis=2, keepdims=True)
    at = np.take_along_axis(E, np.nanargmax(L, axis=2)[..., None], axis=2)
    with np.errstate(invalid="ignore"):
        return L + E >= m - at


def amplification(x, points, classes, starts, iters, f0, floor, h0=None, v0=None, planar=False, patterns=PATTERNS, clean=None):
    """The largest deviation of every start's final (h, v, Lambda) over the injected runs, relative to the clean run's one-pass
    bounds -> (ratio_h, ratio_v, ratio_Lam), each (B, C, T), and the clean run.  The device hands out the state of the WINNING
    start only and every start's Lambda, so the first two are asserted at `clean["best_start"]` (`at_best`) and the third everywhere."""
    if clean is None or "Ehs" not in clean:
        clean = reference_and_bound(x, points, classes, starts, iters, f0, floor, h0, v0, planar, record=True)
    rh, rv, rl = (np.zeros_like(clean["V"]) for _ in range(3))
    for pat in patterns:
        run = reference_and_bound(x, points, classes, starts, iters, f0, floor, h0, v0, planar, inject=pat,
                                  steps=(clean["Ehs"], clean["Evs"]))
        rh = np.maximum(rh, np.abs(run["H"] - clean["H"]) / clean["Eh"])
        rv = np.maximum(rv, np.abs(run["V"] - clean["V"]) / clean["Ev"])
        rl = np.maximum(rl, np.abs(run["start_ll"] - clean["start_ll"]) / clean["ELam"])
    return rh, rv, rl, clean


def at_best(a, ref):
    """a (B, C, T) at the reference's winning start -> (B, C) (NaN where there is none)."""
    best = ref["best_start"]
    return np.where(best >= 0, np.take_along_axis(a, np.maximum(best, 0)[..., None], 2)[..., 0], np.nan)


# ---- integer cases, exact in fp32
EXACT_LENGTHS = (64, 128, 256, 512)                       # powers of two: every division of an update is exact
EXACT_EDGES = (1, 63, 65, 255, 257, 1025)                 # the lane-chain edges, at iters = 0
# four classes: one point, 2 copies, 8 copies (|s|^2 = 1, 2, 1), and the origin alone (dead under any update: Bq = 0)
EXACT_POINTS = np.array([[0, 1]] + [[1, 1]] * 2 + [[-1, 0]] * 8 + [[0, 0]], np.float32)
EXACT_CLASSES = [(0, 1), (1, 2), (3, 8), (11, 1)]


def exact_case(n_frames, length, seed, tiled=True):
    """Integer frames in [-4, 4]; h0 a power of two times a quarter turn and v0 a power of two in [1/4, 4], per (frame, class).
    Every class is 2^j copies of one integer point s with |s|^2 in (1, 2), so every responsibility is exp2(0) = 1, S = M, 1 / S is
    exact and the update sums are sums of integers: A = sum y conj(s), Bq = len |s|^2, V = sum |y - h0 s|^2.  tiled: the frame is
    a block of four integer symbols repeated len / 4 times and then permuted, so that A / Bq = (block sum) / (4 |s|^2) is a
    multiple of 1/8 whatever len is, d at the SECOND pass a multiple of 1/64 below 2^8 and every partial sum of up to 512 of them
    below 2^24 sixty-fourths: with len a power of two nothing rounds in (h, v) through any number of updates.  Lambda is exact where
    v is a power of two (iters = 0): there l_n = -q d_min is a multiple of 1/4 and log2(v) an integer."""
    rng = np.random.default_rng(seed)
    if tiled and length % 4 == 0:
        block = rng.integers(-4, 5, size=(n_frames, 4, 2))
        x = np.stack([np.tile(block[b], (length // 4, 1))[rng.permutation(length)] for b in range(n_frames)])
    else:
        x = rng.integers(-4, 5, size=(n_frames, length, 2))
    Cn = len(EXACT_CLASSES)
    turn = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], np.float32)[rng.integers(0, 4, size=(n_frames, Cn))]
    h0 = (turn * (2.0 ** rng.integers(-1, 2, size=(n_frames, Cn, 1)))).astype(np.float32)
    v0 = (2.0 ** rng.integers(-2, 3, size=(n_frames, Cn))).astype(np.float32)
    return x.astype(np.float32), h0, v0


def exact_L(x, h0, v0):
    """L = -sum_n |y_n - h0 s|^2 / v0 of an exact case per (frame, class), s the class's one point: exact in fp64."""
    y = to_complex(x)
    h = h0[..., 0].astype(np.float64) + 1j * h0[..., 1].astype(np.float64)
    s = np.array([EXACT_POINTS[o] for o, _ in EXACT_CLASSES], np.float64) @ np.array([1, 1j])
    z = y[:, None, :] - (h * s[None, :])[:, :, None]
    return -(z.real ** 2 + z.imag ** 2).sum(axis=2) / v0.astype(np.float64)         # (not numpy.abs: its square root rounds)


def lambda_as_the_header_rounds_it(L, v, n):
    """fmaf(-(float)len, LN2 * (LOG2PI + log2(v)), L) with v a power of two and L exact: the two fp32 products and the sum as the
    header orders them, the fused step in fp64 (a 24-bit by 24-bit product is exact there) and one rounding to fp32."""
    f = np.float32
    ln2, log2pi = f(0.69314718055994530942), f(1.65149612947231879804)
    t = f(ln2 * f(log2pi + np.log2(v).astype(np.float32)))
    return (L.astype(np.float64) - float(n) * t.astype(np.float64)).astype(np.float32).astype(np.float64)


# ---- real cases
def given_start(x, points, classes, seed, planar=False):
    """A start per (frame, class) near enough to the truth to be of interest and far enough to move: the least-squares gain of the
    frame against its nearest points under a random phase, v0 between 0.05 and 0.5 of the frame's power; fp32 numbers."""
    rng = np.random.default_rng(seed)
    y = to_complex(x, planar)
    B, Cn = len(y), len(classes)
    M2 = np.mean(y.real ** 2 + y.imag ** 2, axis=1)                             # (not numpy.abs: its square root rounds)
    h0 = np.sqrt(M2)[:, None] * rng.uniform(0.6, 1.1, (B, Cn)) * np.exp(2j * np.pi * rng.uniform(0, 1, (B, Cn)))
    v0 = M2[:, None] * rng.uniform(0.05, 0.5, (B, Cn))
    return np.stack([h0.real, h0.imag], axis=2).astype(np.float32), v0.astype(np.float32)


def bounded_cases():
    """name, points (P, 2), classes, starts (T, 2), x (B, len, 2): class sizes 1, 2, 16 and 256, T = 1, 4, 5 (uneven over the four
    waves) and 16, B <= 4, len <= 257, lengths on both sides of the lane-chain edges."""
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier
    from vit_vs_raw_iq_amd.likelihood import rotation_table
    full = lambda T: rotation_table(2 * np.pi * np.arange(T) / T)                     # noqa: E731
    sizes, order = [1, 2, 16, 256], [2, 0, 3, 1]                                    # where each class lies in the table
    table, classes, off = [], [None] * 4, 0
    for i in order:
        classes[i] = (off, sizes[i])
        table.append(random_table(sizes[i], 60 + i))
        off += sizes[i]
    points = np.concatenate(table)
    of16 = points[classes[2][0]:classes[2][0] + 16].astype(np.float64) @ np.array([1, 1j])
    yield "sizes_T5", points, classes, full(5), real_frames(2, 130, of16, 15.0, 1, gain=0.7)[0]
    clf = HybridLikelihoodClassifier(257, classes=["BPSK", "QPSK", "16QAM", "64QAM"])
    yield "C4_T16", clf.points, [d[1:] for d in clf.descriptors], clf.starts, real_frames(3, 257, "16QAM", 12.0, 2, gain=2.5)[0]
    big = HybridLikelihoodClassifier(65, classes=["256QAM"])
    yield "M256_T4", big.points, [d[1:] for d in big.descriptors], full(4), real_frames(2, 65, "256QAM", 30.0, 3)[0]
    one = HybridLikelihoodClassifier(64, classes=["8PSK"])
    yield "C1_T1", one.points, [d[1:] for d in one.descriptors], rotation_table(np.array([0.3])), real_frames(4, 64, "8PSK", 8.0, 4, gain=0.4)[0]


F0, FLOOR = np.float32(0.02), np.float32(1e-6)            # the class's defaults, as the fp32 numbers the device is handed


# ---- the decision set: the table classes of up to 64 points at 20 dB, 128 symbols, an unknown gain per frame
DECISION_SNR_DB = 20.0
DECISION_PER_CLASS = 2
DECISION_CAP = 0.02                                       # at most this share of the set may be too close to call


@functools.lru_cache(maxsize=None)
def decision_classifier():
    """The classifier of the decision set: the defaults (16 starts, 32 iterations, f0 = 0.02) over the 14 table classes of up to
    64 points.  (With all 17 classes the host definition of the set takes minutes: 128APSK, 128QAM and 256QAM hold 512 of the
    table's 812 points.  Points are cut, not iterations.)"""
    from vit_vs_raw_iq_amd import HybridLikelihoodClassifier
    from vit_vs_raw_iq_amd import data as D
    from vit_vs_raw_iq_amd.likelihood import TABLE_CLASSES
    names = [c for c in TABLE_CLASSES if len(D.constellation(c)) <= 64]
    return HybridLikelihoodClassifier(128, classes=names)


@functools.lru_cache(maxsize=None)
def decision_set():
    """(X (28, 128, 2) fp32, Y (28,), gain (28,)): data.make_dataset's frames of the classifier's classes at 20 dB, every frame
    multiplied by its own gain in [0.3, 3].  Read-only."""
    from vit_vs_raw_iq_amd import data as D
    names = decision_classifier().class_names
    X, Y, Z = D.make_dataset(DECISION_PER_CLASS * len(names), seed=3, classes=names, snrs_db=(DECISION_SNR_DB,), n_symbols=128)
    gain = np.random.default_rng(17).uniform(0.3, 3.0, len(X))
    X = (X * gain[:, None, None]).astype(np.float32)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, gain


@functools.lru_cache(maxsize=None)
def decision_reference():
    """reference_and_bound of the decision set, computed once per process."""
    clf = decision_classifier()
    return reference_and_bound(decision_set()[0], clf.points, [d[1:] for d in clf.descriptors], clf.starts, clf.iters,
                               np.float32(clf.init_noise), np.float32(clf.floor))


def decided(ref, factor=FACTOR):
    """decided[b]: the frame's best-minus-second margin is at least twice its allowance (the largest over its classes)."""
    return margin(np.where(np.isnan(ref["loglik"]), -np.inf, ref["loglik"])) >= 2.0 * factor * np.nanmax(ref["Ell"], axis=1)
