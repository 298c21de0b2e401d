"""L-infinity attacks on the model input (FGSM, PGD) and accuracy-versus-epsilon curves.

Every step runs on native kernels only, with no host synchronisation inside a chunk's loop: an eval forward of the plan
model.forward uses, iq_ce_fwd_bwd (smoothing 0) for d CE / d logits, iq_model_backward_input without parameter gradients,
then iq_linf_step:  x <- clamp(clamp(x + alpha sign(g), x0 - eps, x0 + eps), lo, hi).  Chunks of `batch` frames are attacked
one after another in the plan's workspace.  The module's `training` flag and every `p.grad` are left alone; a pending
backward() of an earlier forward raises afterwards, as after any later forward.  There is no CPU path.

  fgsm(model, src, labels, eps, clip=None, batch=256)         one step of size eps (Goodfellow et al. 2015)
  pgd(model, src, labels, eps, alpha, steps, random_start=False, seed=0, clip=None, batch=256)
                                                              `steps` steps of size alpha projected on the eps ball (Madry et
                                                              al. 2018); random_start draws the start uniformly in the ball
  robustness_curve(model, x, y, eps_list, attack="fgsm"|"pgd", batch=256, **kw)
                                                              top-1 accuracy (float) per eps; eps 0 = the clean accuracy.
                                                              PGD defaults: steps 10, alpha 2.5 eps / steps.

eps and alpha are in the units of the model's input, the z-scored frame (data.py): one unit is one standard deviation of the
channel.  clip = (lo, hi) bounds every element after each step (None or a None bound: unbounded).

The classical columns.  `model` may be a likelihood.LikelihoodClassifier, a likelihood_em.HybridLikelihoodClassifier or a
cumulants.CumulantClassifier: src is then a batch of device frames in the classifier's layout, and every step is the classifier's
forward, d loss / d loglik (the cumulant classifier's scores stand for loglik), its backward (iq_frames_likelihood_bwd /
iq_frames_likelihood_em_bwd / iq_frames_cumulants_bwd: the forward runs once per step) and the same iq_linf_step.
Keywords of that path only: the classifier's noise (sigma2= | snr_db=, gain=; the hybrid takes none; the cumulant classifier
takes sigma2= | snr_db= or neither, and no gain) and
  loss="margin" (the default)   max_{c != y} loglik_c - loglik_y: -1 at the label, +1 at the first largest other class.  At 20 dB
                                the classes lie 10 to several hundred nats apart, so softmax - onehot is exactly zero in fp32
                                for most frames and the cross entropy has no gradient to follow; the margin always has one.
  loss="ce"                     iq_ce_fwd_bwd on loglik as logits, as the model path.
There eps and alpha are in the FRAME's own units (a unit-power signal for the generators' frames), not in z-score units: the
model path's eps is eps_model = eps_frame / std of the channel.

  transfer_table(sources, targets, x, y, eps, attack="fgsm", **kw)     accuracies (len(sources) + 1, len(targets)): row 0 clean,
                                                              row i + 1 the frames crafted against sources[i], judged by
                                                              every target (a classifier, (classifier, {noise keywords}) or a
                                                              callable frames -> predictions)
"""
from __future__ import annotations

import math
import numbers
import operator

import torch

from . import _native as N
from .cumulants import CumulantClassifier
from .likelihood import LikelihoodClassifier
from .likelihood_em import HybridLikelihoodClassifier
from .saliency import _batch, _ce_grad, _classes, _forward, _input_grad, _resolve

LOSSES = ("margin", "ce")                    # of the classifier path


def _nonneg(v, what):
    if not isinstance(v, numbers.Real) or isinstance(v, bool) or not math.isfinite(float(v)) or float(v) < 0:
        raise ValueError(f"{what} must be a finite number >= 0, got {v!r}")
    return float(v)


def _clip(clip):
    if clip is None:
        return math.nan, math.nan
    try:
        lo, hi = clip
    except (TypeError, ValueError):
        raise ValueError(f"clip must be None or (lo, hi), got {clip!r}") from None
    lo = math.nan if lo is None else float(lo)
    hi = math.nan if hi is None else float(hi)
    if lo == lo and hi == hi and lo > hi:
        raise ValueError(f"clip lower bound {lo} is above the upper bound {hi}")
    return lo, hi


def _step(x, g, x0, alpha, eps, lo, hi):
    N.check(N.lib().iq_linf_step(N.ptr(x), N.ptr(g), N.ptr(x0), alpha, eps, lo, hi, x.numel(), N.stream_handle()), "iq_linf_step")


def _prepare(model, src, labels, batch):
    enc, plan_of, K = _resolve(model)
    batch = _batch(batch)
    n = src.shape[0] if isinstance(src, torch.Tensor) and src.dim() > 0 else 0
    lab = _classes(labels, n, K, "labels")
    return enc, plan_of, lab, batch


def _attack(plan, src, lab, eps, alpha, steps, start, lo, hi, batch):
    out = start
    with torch.no_grad():
        for i in range(0, src.shape[0], batch):
            x0, xa, y = src[i:i + batch], out[i:i + batch], lab[i:i + batch].contiguous()
            for _ in range(steps):
                logits = _forward(plan, xa)
                _step(xa, _input_grad(plan, xa, _ce_grad(plan, logits, y)), x0, alpha, eps, lo, hi)
    return out


# ---- the classical classifiers in place of a model

def _is_classifier(model):
    return isinstance(model, (LikelihoodClassifier, HybridLikelihoodClassifier, CumulantClassifier))


def _model_only(loss, noise):
    """The model path takes neither keyword of the classifier path."""
    if loss is not None or noise:
        raise TypeError(f"loss= and the noise keywords belong to the likelihood classifiers, not to a model: got "
                        f"{sorted(noise) + (['loss'] if loss is not None else [])}")


def _clf_prepare(clf, src, labels, batch, loss, noise):
    """-> (frames contiguous fp32, labels on their device, the classifier's side arguments for the whole batch, batch, loss)"""
    loss = "margin" if loss is None else loss
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
    if loss == "margin" and clf.n_classes < 2:
        raise ValueError("loss='margin' needs at least two classes")
    batch = _batch(batch)
    n = src.shape[0] if isinstance(src, torch.Tensor) and src.dim() > 0 else 0
    lab = _classes(labels, n, clf.n_classes, "labels")
    check = clf._side if isinstance(clf, CumulantClassifier) else clf._check
    side = check(src, **noise)                             # shape, noise and device, in the classifier's words
    return src.detach().contiguous().float(), lab.to(src.device), side, batch, loss


def _margin_grad(loglik, labels):
    """d (max_{c != y} loglik_c - loglik_y) / d loglik: -1 at the label, +1 at the first largest other class."""
    at = labels[:, None]
    other = loglik.scatter(1, at, float("-inf")).argmax(1, keepdim=True)
    return torch.zeros_like(loglik).scatter_(1, at, -1.0).scatter_(1, other, 1.0)


def _clf_ce_grad(loglik, labels):
    dl = torch.empty_like(loglik)
    B, K = loglik.shape
    N.check(N.lib().iq_ce_fwd_bwd(N.ptr(loglik), N.ptr(labels), B, K, 0.0, 1.0, None, None, N.ptr(dl), N.stream_handle()),
            "iq_ce_fwd_bwd")
    return dl


def _chunk(side, i, batch):
    return tuple(None if t is None else t[i:i + batch].contiguous() for t in side)


def _clf_attack(clf, src, lab, side, eps, alpha, steps, start, lo, hi, batch, loss):
    out = start
    with torch.no_grad():
        for i in range(0, src.shape[0], batch):
            x0, xa, y, args = src[i:i + batch], out[i:i + batch], lab[i:i + batch].contiguous(), _chunk(side, i, batch)
            for _ in range(steps):
                outs, held = clf._forward(xa, *args)
                loglik = outs[0].contiguous()
                dl = _margin_grad(loglik, y) if loss == "margin" else _clf_ce_grad(loglik, y)
                _step(xa, clf._backward(xa, dl, *held), x0, alpha, eps, lo, hi)
    return out


def _random_start(src, eps, seed, lo, hi):
    g = torch.Generator(device=src.device)
    g.manual_seed(seed)
    noise = torch.rand(src.shape, generator=g, device=src.device, dtype=torch.float32).mul_(2 * eps).sub_(eps)
    start = torch.minimum(torch.maximum(src + noise, src - eps), src + eps)
    if lo == lo:
        start.clamp_(min=lo)
    if hi == hi:
        start.clamp_(max=hi)
    return start


def fgsm(model, src, labels, eps, clip=None, batch=256, loss=None, **noise):
    if _is_classifier(model):
        eps = _nonneg(eps, "eps")
        lo, hi = _clip(clip)
        src, lab, side, batch, loss = _clf_prepare(model, src, labels, batch, loss, noise)      # (the device refusal comes last)
        return _clf_attack(model, src, lab, side, eps, eps, 1, src.clone(), lo, hi, batch, loss)
    _model_only(loss, noise)
    enc, plan_of, lab, batch = _prepare(model, src, labels, batch)
    eps = _nonneg(eps, "eps")
    lo, hi = _clip(clip)
    src = enc._expect(src)
    plan = plan_of()
    return _attack(plan, src, lab.to(src.device), eps, eps, 1, src.clone(), lo, hi, batch)


def pgd(model, src, labels, eps, alpha, steps, random_start=False, seed=0, clip=None, batch=256, loss=None, **noise):
    if _is_classifier(model):
        eps, alpha, steps, seed = _nonneg(eps, "eps"), _nonneg(alpha, "alpha"), operator.index(steps), operator.index(seed)
        if steps < 1:
            raise ValueError(f"steps must be >= 1, got {steps}")
        lo, hi = _clip(clip)
        src, lab, side, batch, loss = _clf_prepare(model, src, labels, batch, loss, noise)
        start = _random_start(src, eps, seed, lo, hi) if random_start and eps > 0 else src.clone()
        return _clf_attack(model, src, lab, side, eps, alpha, steps, start, lo, hi, batch, loss)
    _model_only(loss, noise)
    enc, plan_of, lab, batch = _prepare(model, src, labels, batch)
    eps = _nonneg(eps, "eps")
    alpha = _nonneg(alpha, "alpha")
    steps = operator.index(steps)
    if steps < 1:
        raise ValueError(f"steps must be >= 1, got {steps}")
    seed = operator.index(seed)
    lo, hi = _clip(clip)
    src = enc._expect(src)
    plan = plan_of()
    start = _random_start(src, eps, seed, lo, hi) if random_start and eps > 0 else src.clone()
    return _attack(plan, src, lab.to(src.device), eps, alpha, steps, start, lo, hi, batch)


def robustness_curve(model, x, y, eps_list, attack="fgsm", batch=256, **kw):
    if attack not in ("fgsm", "pgd"):
        raise ValueError(f"attack must be 'fgsm' or 'pgd', got {attack!r}")
    eps_list = [_nonneg(e, "eps") for e in eps_list]
    allowed = {"clip"} if attack == "fgsm" else {"clip", "alpha", "steps", "random_start", "seed"}
    if _is_classifier(model):
        allowed |= {"loss", "sigma2", "snr_db", "gain"}
    extra = set(kw) - allowed
    if extra:
        raise TypeError(f"unexpected keyword arguments for attack={attack!r}: {sorted(extra)}")
    steps = operator.index(kw.get("steps", 10))
    if steps < 1:
        raise ValueError(f"steps must be >= 1, got {steps}")
    if kw.get("alpha") is not None:
        _nonneg(kw["alpha"], "alpha")
    _clip(kw.get("clip"))
    if _is_classifier(model):
        return _clf_curve(model, x, y, eps_list, attack, batch, steps, kw)
    enc, plan_of, lab, batch = _prepare(model, x, y, batch)
    x = enc._expect(x)
    plan = plan_of()
    lab = lab.to(x.device)

    def accuracy(xs):
        correct = torch.zeros((), dtype=torch.int64, device=x.device)
        with torch.no_grad():
            for i in range(0, xs.shape[0], batch):
                correct += (_forward(plan, xs[i:i + batch]).argmax(1) == lab[i:i + batch]).sum()
        return correct.item() / max(1, xs.shape[0])

    out = []
    for eps in eps_list:
        if eps == 0:
            out.append(accuracy(x))
        elif attack == "fgsm":
            out.append(accuracy(fgsm(model, x, lab, eps, clip=kw.get("clip"), batch=batch)))
        else:
            alpha = kw.get("alpha")
            alpha = 2.5 * eps / steps if alpha is None else alpha
            out.append(accuracy(pgd(model, x, lab, eps, alpha, steps, random_start=kw.get("random_start", False),
                                    seed=kw.get("seed", 0), clip=kw.get("clip"), batch=batch)))
    return out


def _clf_pred(clf, x, side):
    """The decisions alone (int32), of frames and side arguments that are checked already."""
    if isinstance(clf, LikelihoodClassifier):
        return clf._launch(x, *side, False, False, True)[3]
    if isinstance(clf, CumulantClassifier):
        return clf._launch(x, *side, False, False, False, True)[3]
    return clf._launch(x, *side, False, True)[5]


def _clf_accuracy(clf, xs, lab, side, batch):
    correct = torch.zeros((), dtype=torch.int64, device=xs.device)
    with torch.no_grad():
        for i in range(0, xs.shape[0], batch):
            pred = _clf_pred(clf, xs[i:i + batch], _chunk(side, i, batch))
            correct += (pred == lab[i:i + batch]).sum()
    return correct.item() / max(1, xs.shape[0])


def _clf_curve(clf, x, y, eps_list, attack, batch, steps, kw):
    """robustness_curve of a classical classifier: the accuracy is that of clf.predict under the same noise keywords."""
    noise = {k: kw[k] for k in ("sigma2", "snr_db", "gain") if k in kw}
    x, lab, side, batch, loss = _clf_prepare(clf, x, y, batch, kw.get("loss"), noise)

    def accuracy(xs):
        return _clf_accuracy(clf, xs, lab, side, batch)

    out = []
    for eps in eps_list:
        if eps == 0:
            out.append(accuracy(x))
        elif attack == "fgsm":
            out.append(accuracy(fgsm(clf, x, lab, eps, clip=kw.get("clip"), batch=batch, loss=loss, **noise)))
        else:
            alpha = kw.get("alpha")
            alpha = 2.5 * eps / steps if alpha is None else alpha
            out.append(accuracy(pgd(clf, x, lab, eps, alpha, steps, random_start=kw.get("random_start", False),
                                    seed=kw.get("seed", 0), clip=kw.get("clip"), batch=batch, loss=loss, **noise)))
    return out


def _party(item, what, callable_ok):
    """A source or target of transfer_table -> (classifier or callable, its noise keywords)."""
    clf, noise = item if isinstance(item, tuple) and len(item) == 2 and isinstance(item[1], dict) else (item, {})
    if _is_classifier(clf):
        return clf, dict(noise)
    if callable_ok and not noise and callable(clf) and not isinstance(clf, tuple):
        return clf, None
    raise TypeError(f"{what} must be a LikelihoodClassifier, a HybridLikelihoodClassifier or a CumulantClassifier, or a pair "
                    f"(classifier, {{its noise keywords}}){', or a callable frames -> (B,) predictions' if callable_ok else ''}, "
                    f"got {item!r}")


def transfer_table(sources, targets, x, y, eps, attack="fgsm", batch=256, **kw):
    """Does a perturbation crafted against one classical classifier fool the others?  -> a (len(sources) + 1, len(targets)) list
    of rows of top-1 accuracies: row 0 the clean frames, row i + 1 the frames `attack` ("fgsm" | "pgd", with robustness_curve's
    keywords and PGD defaults, loss= among them) crafted at `eps` against sources[i], each judged by every target.  A source is
    a classical classifier or (classifier, {its noise keywords}); a target is either of those or any callable frames -> (B,)
    predictions (a model behind its own input layout).  All classifiers share length and layout, which is checked with every
    other argument before any device work.  Each source is attacked once, not once per target; a classifier target's accuracy
    is clf.predict's under its own keywords, so a diagonal entry is that classifier's robustness_curve entry."""
    if attack not in ("fgsm", "pgd"):
        raise ValueError(f"attack must be 'fgsm' or 'pgd', got {attack!r}")
    eps = _nonneg(eps, "eps")
    extra = set(kw) - ({"clip", "loss"} if attack == "fgsm" else {"clip", "loss", "alpha", "steps", "random_start", "seed"})
    if extra:
        raise TypeError(f"unexpected keyword arguments for attack={attack!r}: {sorted(extra)}")
    steps = operator.index(kw.get("steps", 10))
    if steps < 1:
        raise ValueError(f"steps must be >= 1, got {steps}")
    alpha = 2.5 * eps / steps if kw.get("alpha") is None else _nonneg(kw["alpha"], "alpha")
    _clip(kw.get("clip"))
    sources, targets = list(sources), list(targets)
    if not sources or not targets:
        raise ValueError("sources and targets must not be empty")
    src = [_party(s, "a source", False) for s in sources]
    tgt = [_party(t, "a target", True) for t in targets]
    clfs = [c for c, noise in src + tgt if noise is not None]
    for c in clfs[1:]:
        if (c.length, c.layout) != (clfs[0].length, clfs[0].layout):
            raise ValueError(f"all classifiers must share length and layout: {clfs[0]!r} against {c!r}")
    batch = _batch(batch)
    # every keyword of every party is checked before the first launch; the refusal of CPU frames, each party's last check,
    # comes after the other parties' checks too
    refused, prepared, judges = None, [], []
    for i, (c, noise) in enumerate(src + tgt):
        attacked = i < len(src)
        out = None
        if noise is not None:
            try:
                out = _clf_prepare(c, x, y, batch, kw.get("loss") if attacked else "ce", noise)     # (a judge has no loss)
            except N.IqError as e:
                refused = refused or e
        (prepared if attacked else judges).append(out)
    if refused is not None:
        raise refused
    x0, labels = prepared[0][:2]

    def judge(xs):
        row = []
        for (c, noise), held in zip(tgt, judges):
            if noise is None:
                with torch.no_grad():
                    pred = torch.as_tensor(c(xs)).to(xs.device)
                row.append((pred == labels).sum().item() / max(1, xs.shape[0]))
            else:
                row.append(_clf_accuracy(c, xs, held[1], held[2], batch))
        return row

    table = [judge(x0)]
    for (c, noise), (xs, lab, _, _, loss) in zip(src, prepared):
        if attack == "fgsm":
            adv = fgsm(c, xs, lab, eps, clip=kw.get("clip"), batch=batch, loss=loss, **noise)
        else:
            adv = pgd(c, xs, lab, eps, alpha, steps, random_start=kw.get("random_start", False), seed=kw.get("seed", 0),
                      clip=kw.get("clip"), batch=batch, loss=loss, **noise)
        table.append(judge(adv))
    return table
