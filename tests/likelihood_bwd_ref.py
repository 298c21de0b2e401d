"""What tests/test_likelihood_bwd_cpu.py and tests/test_gpu_likelihood_bwd.py share: the fp64 definitions of the two likelihood
gradients (iq_frames_likelihood_bwd, iq_frames_likelihood_em_bwd of include/iqvit.h), the plain logsumexp statements torch autograd
differentiates, the fp32 bound of the device's dx, the cases, and the host FGSM table.  A plain helper module like the other
*_ref.py files; the notation and the first half of the derivation are tests/likelihood_ref.py's.

THE DEFINITIONS take what the device's backward takes: the frames, the side arguments and the forward's per-(frame, class)
results (loglik, rot_ll, best_rot; h, v) -- whoever computed them.  The GPU suite hands them the DEVICE's forward outputs, so that
both sides weigh the same hypotheses and only the backward's own arithmetic differs; the forward has its own suite and bound.

THE BOUND.  u = 2^-24.  Every step below is DERIVED, to first order in u; nothing is measured.  For one frame, class, hypothesis
(weight w, rotation (c, s) or state (h, v)) and symbol, per component (Re or Im):

  scaled point    likelihood: p = a s_k, one product per component:  dp <= u |p_c|.   EM: p = h s_k, a product and an fmaf:
                  dp <= 2 u |h| |s_k|
  rotation        likelihood: y' as in likelihood_ref.py:  ey = 2 u (|Re y| + |Im y|).   EM: y is exact, ey = 0
  e_k             by the forward's instructions, so with the forward's relative error (likelihood_ref.py, likelihood_em_ref.py):
                  r_k = q (eps(d_min) + eps(d_k)) + 5 u q (d_k - d_min) + 2 u,  eps(d) = 2 sqrt(2 d) e0 + 4 u d,
                  e0 = u (2 sqrt(2) |y| + a max|s|) (likelihood), 2 u |h| max|s| (EM).  A term below 2^-126 is flushed to zero,
                  which against S >= 1 is below 2^-126 and is not counted
  m = W / S       the responsibilities pi_k = e_k / S inherit r_k: relative perturbations delta_k of the e_k move the weighted mean by
                  sum_k pi_k delta_k (p_k - m), so  sum_k pi_k r_k |p_k,c - m_c|;  the points' own errors  sum_k pi_k dp_k,c;  the M
                  fmaf of W, each partial sum below sum_k e_k |p_k,c|:  M u G_c, G_c = sum_k pi_k |p_k,c|;  the M - 1 additions of S,
                  r = 1 / S and W r:  (M + 1) u |m_c|.
                  dm_c = sum_k pi_k r_k |p_k,c - m_c| + sum_k pi_k dp_k,c + M u G_c + (M + 1) u |m_c|
  y' - m          df_c = ey + dm_c + u |y'_c - m_c|
  weight          'max' and EM: w = dloglik, exact.  'mean': w = (dloglik * exp2(LOG2E * (L_r - loglik))) * (1 / R): the difference,
                  the constant and the product 3 u |L_r - loglik|, exp2 2 u, the two products and 1 / R 3 u:
                  rho_w = 3 u |L_r - loglik| + 5 u.  A share below 2^-125 may be flushed to zero on the device, which then SKIPS
                  the hypothesis: there rho_w = 1 (the whole term, which is below 2^-125 |dloglik| 2 q |y' - m|)
  wq = w (-2 q)   q = 1 / sigma2 (or 1 / v): u;  -2 q exact;  the product u:  relative rho_w + 2 u
  g_c = wq f_c    dg_c = |wq| df_c + |g_c| (rho_w + 3 u)    (EM fuses this product into the sum: the same bound holds)
  back to y       likelihood: t = (fmaf(Re g, c, -(Im g s)), fmaf(Re g, s, Im g c)): a product and an fmaf,
                  dt_Re = |c| dg_Re + |s| dg_Im + 2 u (|Re g c| + |Im g s|), dt_Im alike.   EM: t = g
  the chain       dx adds its K nonzero terms (K <= C T) one after another, every partial sum below sum |t_c|:  K u sum |t_c|

  Edx[b, n, c] = sum over the terms of dt_c + K u sum over the terms of |t_c|, evaluated in fp64 on the data itself, and
  multiplied by 1 + 2^-10 for the second-order terms.
"""
import functools

import numpy as np
import torch

import likelihood_ref as R
from likelihood_ref import SLACK, U, from_complex, in_layout, to_complex  # noqa: F401

BLOCK = 512                                   # symbols per workgroup of csrc/likelihood_bwd.hip; a wave takes 128, a lane n and n + 64
# both sides of a lane pair (64), of a wave (128) and of the block (512), and two blocks and a symbol; 8192 runs once
EXACT_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)
LONGEST = 8192
REAL_LENGTH = 130                             # both symbols of a lane, two waves and a ragged end
BLOCK_EDGE_LENGTH = 514                       # two blocks' edge


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))               # (a copy: the source may be read-only)


def _soft_terms(yre, yim, pr, pi, q, w, rho_w, e0, ey, dpr, dpi, bound):
    """The terms g = w (-2 q) (y' - m) of a set of hypotheses.  yre, yim (b, T, n): the symbols in each hypothesis's frame;
    pr, pi (b, T, M): its points; q, w, rho_w (b, T); e0, ey (b, T, n); dpr, dpi (b, T, M).  -> gr, gi (b, T, n) and, with bound,
    dgr, dgi (else None)."""
    M = pr.shape[2]
    dr = yre[..., None] - pr[:, :, None, :]
    di = yim[..., None] - pi[:, :, None, :]
    d = dr * dr + di * di                                                            # (b, T, n, M)
    dmin = d.amin(dim=3)
    gap = d - dmin[..., None]
    qq = q[..., None]                                                                # (b, T, 1)
    e = torch.exp(-qq[..., None] * gap)
    pik = e / e.sum(dim=3, keepdim=True)
    mr, mi = (pik * pr[:, :, None, :]).sum(dim=3), (pik * pi[:, :, None, :]).sum(dim=3)
    wq = (w * (-2.0 * q))[..., None]
    fr, fi = yre - mr, yim - mi
    gr, gi = wq * fr, wq * fi
    if not bound:
        return gr, gi, None, None
    eps = lambda t, s: 2.0 * torch.sqrt(2.0 * t) * s + 4.0 * U * t                   # noqa: E731
    rk = qq[..., None] * (eps(dmin, e0)[..., None] + eps(d, e0[..., None])) + 5.0 * U * qq[..., None] * gap + 2.0 * U

    def dm(pc, m, dpc):
        pc, dpc = pc[:, :, None, :], dpc[:, :, None, :]
        return (pik * rk * (pc - m[..., None]).abs()).sum(dim=3) + (pik * dpc).sum(dim=3) + M * U * (pik * pc.abs()).sum(dim=3) \
            + (M + 1) * U * m.abs()
    rw = rho_w[..., None]
    dgr = wq.abs() * (ey + dm(pr, mr, dpr) + U * fr.abs()) + gr.abs() * (rw + 3.0 * U)
    dgi = wq.abs() * (ey + dm(pi, mi, dpi) + U * fi.abs()) + gi.abs() * (rw + 3.0 * U)
    return gr, gi, dgr, dgi


def likelihood_reference_bwd(x, sigma2, gain, points, classes, rot, mode, dloglik, loglik=None, rot_ll=None, best_rot=None,
                             planar=False, bound=False):
    """The definition of iq_frames_likelihood_bwd in fp64 (torch on the host) on the numbers the device is handed.  points (P, 2),
    classes (offset, count), rot the (R, 2) table, dloglik (B, C); 'max' reads best_rot (B, C), 'mean' loglik (B, C) and rot_ll
    (B, C, R).  A class whose dloglik is 0 is skipped, and so is a hypothesis whose weight is 0.
    -> dx float64 in x's layout; with bound=True (dx, Edx), Edx the bound derived above, of the same shape."""
    y = to_complex(x, planar)
    B, n = y.shape
    s2 = np.broadcast_to(np.asarray(sigma2, np.float64), (B,))
    a = np.ones(B) if gain is None else np.broadcast_to(np.asarray(gain, np.float64), (B,))
    p = np.asarray(points, np.float64).reshape(-1, 2)
    rot = np.asarray(rot, np.float64).reshape(-1, 2)
    Rn = len(rot)
    dl = np.asarray(dloglik, np.float64).reshape(B, len(classes))
    with np.errstate(invalid="ignore"):
        ok = (s2 > 0) & np.isfinite(s2)
    dx, E = np.zeros((B, n), np.complex128), np.zeros((B, n, 2))
    tsum, K = np.zeros((B, n, 2)), np.zeros(B)
    dx[~ok] = complex(np.nan, np.nan)
    yabs, y1 = np.abs(y), np.abs(y.real) + np.abs(y.imag)
    for c, (off, M) in enumerate(classes):
        rows = np.flatnonzero(ok & (dl[:, c] != 0))
        if mode == "max" and len(rows):
            br = np.asarray(best_rot).reshape(B, -1)[rows, c].astype(np.int64)
            lost = (br < 0) | (br >= Rn)
            dx[rows[lost]] = complex(np.nan, np.nan)
            rows, br = rows[~lost], br[~lost]
        if not len(rows):
            continue
        pc = p[off:off + M]
        smax = float(np.sqrt((pc ** 2).sum(axis=1)).max())
        T = 1 if mode == "max" else Rn
        step = max(1, (1 << 20) // (T * n * M))
        for i0 in range(0, len(rows), step):
            rw = rows[i0:i0 + step]
            b = len(rw)
            if mode == "max":
                cs = rot[br[i0:i0 + step]][:, None, :]                                    # (b, 1, 2)
                w, rho = dl[rw, c][:, None], np.zeros((b, 1))
            else:
                cs = np.broadcast_to(rot[None], (b, Rn, 2))
                gapL = np.asarray(rot_ll, np.float64).reshape(B, -1, Rn)[rw, c] - np.asarray(loglik, np.float64).reshape(B, -1)[rw, c][:, None]
                share = np.exp(gapL)
                w = dl[rw, c][:, None] * share / Rn
                rho = np.where(share < 2.0 ** -125, 1.0, 3.0 * U * np.abs(gapL) + 5.0 * U)
            cr, sr = cs[..., 0][..., None], cs[..., 1][..., None]                         # (b, T, 1)
            yr = y[rw][:, None, :] * (cr - 1j * sr)                                       # y' = y (c - j s)
            ar = a[rw][:, None]
            pr, pi = np.broadcast_to((ar * pc[None, :, 0])[:, None, :], (b, T, M)), np.broadcast_to((ar * pc[None, :, 1])[:, None, :], (b, T, M))
            e0 = _t(np.broadcast_to(U * (2.0 * np.sqrt(2.0) * yabs[rw][:, None, :] + np.abs(ar)[..., None] * smax), (b, T, n)))
            ey = _t(np.broadcast_to(2.0 * U * y1[rw][:, None, :], (b, T, n)))
            q = _t(np.broadcast_to((1.0 / s2[rw])[:, None], (b, T)))
            gr, gi, dgr, dgi = _soft_terms(_t(yr.real), _t(yr.imag), _t(pr), _t(pi), q, _t(w), _t(rho), e0, ey,
                                           _t(U * np.abs(pr)), _t(U * np.abs(pi)), bound)
            g = gr.numpy() + 1j * gi.numpy()
            live = (w != 0)[..., None]                                                    # an exact zero is skipped: it adds nothing
            t = np.where(live, g * (cr + 1j * sr), 0.0)                                   # back to y's frame
            dx[rw] += t.sum(axis=1)
            if bound:
                ca, sa, gra, gia = np.abs(cr), np.abs(sr), np.abs(gr.numpy()), np.abs(gi.numpy())
                dtr = ca * dgr.numpy() + sa * dgi.numpy() + 2.0 * U * (gra * ca + gia * sa)
                dti = sa * dgr.numpy() + ca * dgi.numpy() + 2.0 * U * (gra * sa + gia * ca)
                E[rw] += np.stack([np.where(live, dtr, 0.0).sum(axis=1), np.where(live, dti, 0.0).sum(axis=1)], axis=-1)
                tsum[rw] += np.stack([np.abs(t.real).sum(axis=1), np.abs(t.imag).sum(axis=1)], axis=-1)
                K[rw] += (w != 0).sum(axis=1)
    out = from_complex(dx, planar, np.float64)
    if not bound:
        return out
    E = SLACK * (E + K[:, None, None] * U * tsum)
    return out, np.ascontiguousarray(np.transpose(E, (0, 2, 1))) if planar else E


def likelihood_em_reference_bwd(x, points, classes, dloglik, h, v, planar=False, bound=False):
    """The definition of iq_frames_likelihood_em_bwd in fp64 on the numbers the device is handed: one hypothesis (h, v)[b, c] per
    class, held fixed.  h (B, C, 2) or complex (B, C), v (B, C), dloglik (B, C).  A class whose dloglik is 0 is skipped; a
    (frame, class) with a nonzero dloglik whose state is not (h finite, 2^-126 <= v < inf) makes its frame's dx NaN.
    -> dx float64 in x's layout; with bound=True (dx, Edx)."""
    y = to_complex(x, planar)
    B, n = y.shape
    p = np.asarray(points, np.float64).reshape(-1, 2)
    Cn = len(classes)
    h = np.asarray(h)
    h = h.astype(np.complex128).reshape(B, Cn) if np.iscomplexobj(h) else h.astype(np.float64).reshape(B, Cn, 2) @ np.array([1, 1j])
    v = np.asarray(v, np.float64).reshape(B, Cn)
    dl = np.asarray(dloglik, np.float64).reshape(B, Cn)
    with np.errstate(invalid="ignore"):
        alive = np.isfinite(h.real) & np.isfinite(h.imag) & (v >= 2.0 ** -126) & np.isfinite(v)
    dx, E = np.zeros((B, n), np.complex128), np.zeros((B, n, 2))
    tsum, K = np.zeros((B, n, 2)), np.zeros(B)
    for c, (off, M) in enumerate(classes):
        asked = dl[:, c] != 0
        dx[asked & ~alive[:, c]] = complex(np.nan, np.nan)
        rows = np.flatnonzero(asked & alive[:, c])
        pc = p[off:off + M] @ np.array([1, 1j])
        smax = float(np.abs(pc).max())
        step = max(1, (1 << 20) // (n * M))
        for i0 in range(0, len(rows), step):
            rw = rows[i0:i0 + step]
            b = len(rw)
            hp = (h[rw, c][:, None] * pc[None, :])[:, None, :]                            # (b, 1, M)
            dp = np.broadcast_to((2.0 * U * np.abs(h[rw, c])[:, None] * np.abs(pc)[None, :])[:, None, :], (b, 1, M))
            e0 = _t(np.broadcast_to((2.0 * U * np.abs(h[rw, c]) * smax)[:, None, None], (b, 1, n)))
            q = _t((1.0 / v[rw, c])[:, None])
            zero = torch.zeros(b, 1, n, dtype=torch.float64)
            gr, gi, dgr, dgi = _soft_terms(_t(y[rw].real[:, None, :]), _t(y[rw].imag[:, None, :]), _t(hp.real), _t(hp.imag), q,
                                           _t(dl[rw, c][:, None]), torch.zeros(b, 1, dtype=torch.float64), e0, zero, _t(dp), _t(dp), bound)
            dx[rw] += gr.numpy()[:, 0] + 1j * gi.numpy()[:, 0]
            if bound:
                E[rw] += np.stack([dgr.numpy()[:, 0], dgi.numpy()[:, 0]], axis=-1)
                tsum[rw] += np.stack([np.abs(gr.numpy()[:, 0]), np.abs(gi.numpy()[:, 0])], axis=-1)
                K[rw] += 1
    out = from_complex(dx, planar, np.float64)
    if not bound:
        return out
    E = SLACK * (E + K[:, None, None] * U * tsum)
    return out, np.ascontiguousarray(np.transpose(E, (0, 2, 1))) if planar else E


# ---- the plain statements, for torch autograd
def loglik_plain_torch(x, sigma2, gain, points, classes, angles, mode, planar=False):
    """loglik (B, C) as a plain logsumexp statement in torch fp64, nothing taken out first and no maximum located: x a (B, len, 2)
    (or planar) float64 tensor that may require grad.  'max' takes torch's maximum over the rotations."""
    xr, xi = (x[:, 0, :], x[:, 1, :]) if planar else (x[:, :, 0], x[:, :, 1])
    ang = torch.as_tensor(np.asarray(angles, np.float64))
    c, s = torch.cos(ang)[None, :, None], torch.sin(ang)[None, :, None]
    yr, yi = c * xr[:, None, :] + s * xi[:, None, :], c * xi[:, None, :] - s * xr[:, None, :]          # (B, R, n)
    q = 1.0 / torch.as_tensor(np.broadcast_to(np.asarray(sigma2, np.float64), (x.shape[0],)).copy())
    a = torch.as_tensor(np.broadcast_to(np.asarray(1.0 if gain is None else gain, np.float64), (x.shape[0],)).copy())
    p = torch.as_tensor(np.asarray(points, np.float64).reshape(-1, 2))
    out = []
    for off, M in classes:
        pr, pi = a[:, None] * p[off:off + M, 0][None, :], a[:, None] * p[off:off + M, 1][None, :]      # (B, M)
        d = (yr[..., None] - pr[:, None, None, :]) ** 2 + (yi[..., None] - pi[:, None, None, :]) ** 2
        L = (torch.logsumexp(-q[:, None, None, None] * d, dim=3) - np.log(M)).sum(dim=2)               # (B, R)
        out.append(L.max(dim=1).values if mode == "max" else torch.logsumexp(L, dim=1) - np.log(L.shape[1]))
    return torch.stack(out, dim=1)


def lambda_plain_torch(x, points, classes, h, v, planar=False):
    """Lambda (B, C) at the state (h, v) (complex (B, C), (B, C)) as a plain logsumexp statement in torch fp64."""
    xr, xi = (x[:, 0, :], x[:, 1, :]) if planar else (x[:, :, 0], x[:, :, 1])
    p = np.asarray(points, np.float64).reshape(-1, 2) @ np.array([1, 1j])
    out = []
    for c, (off, M) in enumerate(classes):
        hp = np.asarray(h)[:, c][:, None] * p[None, off:off + M]                                       # (B, M)
        d = (xr[..., None] - torch.as_tensor(hp.real.copy())[:, None, :]) ** 2 + (xi[..., None] - torch.as_tensor(hp.imag.copy())[:, None, :]) ** 2
        vc = torch.as_tensor(np.asarray(v, np.float64)[:, c].copy())
        out.append((torch.logsumexp(-d / vc[:, None, None], dim=2) - np.log(M) - torch.log(np.pi * vc)[:, None]).sum(dim=1))
    return torch.stack(out, dim=1)


# ---- integer cases, exact in fp32: likelihood_ref's frames, points and quarter turns, with integer or power-of-two weights
def exact_weights(n_frames, n_classes, seed):
    """dloglik in {-2, -1, 0, 1/2, 1, 4}: every product with it is exact, and a zero is among them."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([-2.0, -1.0, 0.0, 0.5, 1.0, 4.0], np.float32), size=(n_frames, n_classes))


def exact_em_state(n_frames, n_classes, seed):
    """h in {1, j, 2, 1/2} and v a power of two in [1/4, 4] per (frame, class)."""
    rng = np.random.default_rng(seed)
    h = np.array([[1, 0], [0, 1], [2, 0], [0.5, 0]], np.float32)[rng.integers(0, 4, size=(n_frames, n_classes))]
    return h, (2.0 ** rng.integers(-2, 3, size=(n_frames, n_classes))).astype(np.float32)


# ---- the losses of the attack
def margin_weights(loglik, labels):
    """d (max_{c != y} loglik_c - loglik_y) / d loglik: -1 at the label, +1 at the first largest other class."""
    loglik = np.asarray(loglik, np.float64)
    B = len(loglik)
    other = np.where(np.arange(loglik.shape[1])[None, :] == np.asarray(labels)[:, None], -np.inf, loglik)
    w = np.zeros_like(loglik)
    w[np.arange(B), labels] = -1.0
    w[np.arange(B), np.argmax(other, axis=1)] = 1.0                                      # (argmax: the first largest)
    return w


# ---- the host FGSM table of the decision set
FGSM_EPS = 0.05


@functools.lru_cache(maxsize=None)
def host_fgsm(eps=FGSM_EPS):
    """One FGSM step of size eps on the margin loss by the fp64 definition on likelihood_ref.decision_set() under
    LikelihoodClassifier(128) (64 rotations, 'max'), the attacked frames rounded to fp32; and random +-eps signs (seed 0) beside
    it.  -> dict(g: the gradient (68, 128, 2), x_adv, x_rand fp32): computed once per process, read-only."""
    from vit_vs_raw_iq_amd import LikelihoodClassifier
    clf = LikelihoodClassifier(128)
    X, Y, s2 = R.decision_set()
    ref = R.decision_reference("max")
    g = likelihood_reference_bwd(X, s2, None, clf.points, [d[1:] for d in clf.descriptors], clf.rot, "max",
                                 margin_weights(ref["loglik"], Y), best_rot=ref["best_rot"])
    x_adv = (X.astype(np.float64) + eps * np.sign(g)).astype(np.float32)
    x_rand = (X.astype(np.float64) + eps * np.random.default_rng(0).choice([-1.0, 1.0], size=X.shape)).astype(np.float32)
    for arr in (g, x_adv, x_rand):
        arr.setflags(write=False)
    return dict(g=g, x_adv=x_adv, x_rand=x_rand)


def host_accuracy(x):
    """The share of the decision set's labels the fp64 definition (vit_vs_raw_iq_amd.likelihood_reference) finds on frames x."""
    from vit_vs_raw_iq_amd import LikelihoodClassifier, likelihood_reference
    clf = LikelihoodClassifier(128)
    _, Y, s2 = R.decision_set()
    return float(np.mean(likelihood_reference(x, s2, None, clf.points, clf.descriptors, clf.rot, "max")[3] == Y))
