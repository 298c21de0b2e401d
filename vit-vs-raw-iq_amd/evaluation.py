"""Evaluation + report writer.

Counterpart of evaluate_model_with_confusion (reference: Transformer_Thesis/ViT/training/utils.py:284-466).
The model runs on the MI355X path; predictions are reduced to a K x K confusion matrix ON DEVICE (one
bincount per batch, no per-batch host sync -- the reference copies every batch to numpy, :311-320) and the
text report is written in the exact layout of :392-401 so that Transformer_Thesis/compare_models.py
(regexes at :39, :44, :49) parses it unchanged.  Per-SNR accuracy uses the reference's +-0.5 dB windows at
-8 / 0 / +8 dB (:349-377).  The per-class table reproduces sklearn.metrics.classification_report(digits=4)
from the confusion matrix (checked against sklearn in tests/test_host_cpu.py).  Plots are not produced.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np
import torch

TARGET_SNRS = (-8, 0, 8)


def classification_report_text(cm: np.ndarray, class_names: Sequence[str], digits: int = 4) -> str:
    """sklearn-compatible classification report from a confusion matrix (rows = true, cols = predicted)."""
    cm = np.asarray(cm, dtype=np.float64)
    support = cm.sum(axis=1)
    pred = cm.sum(axis=0)
    tp = np.diag(cm)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = np.where(pred > 0, tp / pred, 0.0)
        recall = np.where(support > 0, tp / support, 0.0)
        f1 = np.where(precision + recall > 0, 2 * precision * recall / (precision + recall), 0.0)
    total = support.sum()
    accuracy = tp.sum() / total if total > 0 else 0.0
    headers = ["precision", "recall", "f1-score", "support"]
    longest_last_line_heading = "weighted avg"
    name_width = max(len(cn) for cn in class_names)
    width = max(name_width, len(longest_last_line_heading), digits)
    head_fmt = "{:>{width}s} " + " {:>9}" * len(headers)
    report = head_fmt.format("", *headers, width=width)
    report += "\n\n"
    row_fmt = "{:>{width}s} " + " {:>9.{digits}f}" * 3 + " {:>9}\n"
    for i, name in enumerate(class_names):
        report += row_fmt.format(name, precision[i], recall[i], f1[i], int(support[i]), width=width, digits=digits)
    report += "\n"
    row_fmt_accuracy = "{:>{width}s} " + " {:>9.{digits}}" * 2 + " {:>9.{digits}f}" + " {:>9}\n"
    report += row_fmt_accuracy.format("accuracy", "", "", accuracy, int(total), width=width, digits=digits)
    macro = (precision.mean(), recall.mean(), f1.mean())
    w = support / total if total > 0 else support
    weighted = ((precision * w).sum(), (recall * w).sum(), (f1 * w).sum())
    report += row_fmt.format("macro avg", *macro, int(total), width=width, digits=digits)
    report += row_fmt.format("weighted avg", *weighted, int(total), width=width, digits=digits)
    return report


def report_text(prefix: str, overall: float, snr_acc: Dict[int, float], body: str) -> str:
    """The report file's text: the layout compare_models.py parses."""
    text = f"Classification Report - {prefix.capitalize()} Set\n"
    text += "=" * 80 + "\n\n"
    text += f"Overall Accuracy: {overall * 100:.2f}%\n\n"
    text += "Accuracy by SNR:\n"
    for snr, acc in snr_acc.items():
        text += f"  SNR {snr:+3d} dB: {acc * 100:.2f}%\n"
    text += "\n" + "=" * 80 + "\n\n"
    return text + body


def write_report(path: Path, prefix: str, overall: float, snr_acc: Dict[int, float], body: str) -> None:
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        f.write(report_text(prefix, overall, snr_acc, body))


def _evaluate_with_confusion(predict, dataloader: Iterable, device: torch.device, class_names: List[str], save_dir: Path,
                             prefix: str) -> Dict:
    """What the two evaluations below share: predict(x, y, z) -> (B,) class indices on the device for every batch of
    `dataloader`, the K x K confusion matrices accumulated on the device, the report file, the result dictionary."""
    K = len(class_names)
    cm = torch.zeros(K * K, dtype=torch.int64, device=device)
    cm_snr = {s: torch.zeros(K * K, dtype=torch.int64, device=device) for s in TARGET_SNRS}
    preds, labels_all, snrs_all = [], [], []
    for x, y, z in dataloader:
        x = x.to(device, non_blocking=True)
        y = y.to(device, non_blocking=True).long()
        z = z.to(device, non_blocking=True).float()
        p = predict(x, y, z)
        idx = y * K + p
        cm += torch.bincount(idx, minlength=K * K)
        for s in TARGET_SNRS:
            m = (z - s).abs() <= 0.5
            cm_snr[s] += torch.bincount(idx[m], minlength=K * K)
        preds.append(p)
        labels_all.append(y)
        snrs_all.append(z)
    cm_np = cm.view(K, K).cpu().numpy()                       # single host transfer
    overall = float(np.trace(cm_np) / max(cm_np.sum(), 1))
    snr_acc = {}
    for s in TARGET_SNRS:
        c = cm_snr[s].view(K, K).cpu().numpy()
        if c.sum() > 0:
            snr_acc[s] = float(np.trace(c) / c.sum())
    save_dir = Path(save_dir)
    write_report(save_dir / f"{prefix}_classification_report.txt", prefix, overall, snr_acc,
                 classification_report_text(cm_np, class_names, digits=4))
    return {"overall_accuracy": overall, "snr_accuracies": snr_acc, "confusion_matrix": cm_np,
            "predictions": torch.cat(preds).cpu().numpy() if preds else np.zeros(0, np.int64),
            "labels": torch.cat(labels_all).cpu().numpy() if labels_all else np.zeros(0, np.int64),
            "snrs": torch.cat(snrs_all).cpu().numpy() if snrs_all else np.zeros(0, np.float32)}


@torch.no_grad()
def evaluate_model_with_confusion(model: torch.nn.Module, dataloader: Iterable, device: torch.device,
                                  class_names: List[str], save_dir: Path, prefix: str = "test") -> Dict:
    """`dataloader` yields (inputs, labels, snrs) like the reference's DataLoader (V/training/utils.py:311)."""
    device = torch.device(device)
    was_training = model.training
    model.eval()
    res = _evaluate_with_confusion(lambda x, y, z: model(x).argmax(1), dataloader, device, class_names, save_dir, prefix)
    model.train(was_training)
    return res


@torch.no_grad()
def evaluate_likelihood_with_confusion(clf, dataloader: Iterable, device: torch.device, class_names: List[str], save_dir: Path,
                                       prefix: str = "test") -> Dict:
    """The same evaluation and the same report file for a likelihood.LikelihoodClassifier: compare_models.py reads it as a
    third column beside the two learned models.  `dataloader` yields (frames, labels, snrs) with UN-NORMALISED frames in the
    classifier's layout, a unit-power signal plus noise at the finite SNR `snrs` (dB) as the generators emit them; labels index
    `class_names`, which must be the classifier's classes."""
    device = torch.device(device)
    if list(class_names) != list(clf.class_names):
        raise ValueError(f"class_names must be the classifier's classes {clf.class_names!r}, got {list(class_names)!r}")
    return _evaluate_with_confusion(lambda x, y, z: clf.predict(x, snr_db=z), dataloader, device, class_names, save_dir, prefix)


@torch.no_grad()
def evaluate_cumulants_with_confusion(clf, dataloader: Iterable, device: torch.device, class_names: List[str], save_dir: Path,
                                      prefix: str = "test", known_noise: bool = False) -> Dict:
    """The same evaluation and the same report file for a cumulants.CumulantClassifier: a fourth column for compare_models.py.
    `dataloader` yields (frames, labels, snrs) with frames in the classifier's layout; labels index `class_names`, which must
    be the classifier's classes.  known_noise: False decides blind; True hands the classifier snr_db = `snrs` (generator
    convention: a unit-power signal plus noise), and a frame whose noise variance is then at or above its own variance is
    decided blind.  A frame without any variance (pred -1 in both) is counted under class 0."""
    device = torch.device(device)
    if list(class_names) != list(clf.class_names):
        raise ValueError(f"class_names must be the classifier's classes {clf.class_names!r}, got {list(class_names)!r}")
    if not isinstance(known_noise, bool):
        raise TypeError(f"known_noise must be True or False, got {known_noise!r}")

    def predict(x, y, z):
        p = clf.predict(x)
        if known_noise:
            k = clf.predict(x, snr_db=z)
            p = torch.where(k < 0, p, k)
        return p.clamp_(min=0)
    return _evaluate_with_confusion(predict, dataloader, device, class_names, save_dir, prefix)


@torch.no_grad()
def evaluate_hybrid_with_confusion(clf, dataloader: Iterable, device: torch.device, class_names: List[str], save_dir: Path,
                                   prefix: str = "test") -> Dict:
    """The same evaluation and the same report file for a likelihood_em.HybridLikelihoodClassifier: a further column for
    compare_models.py.  `dataloader` yields (frames, labels, snrs) with frames in the classifier's layout; labels index
    `class_names`, which must be the classifier's classes.  The classifier is handed the frames and nothing else: `snrs` only
    sorts the results.  A frame no class can explain (pred -1) is counted under class 0."""
    device = torch.device(device)
    if list(class_names) != list(clf.class_names):
        raise ValueError(f"class_names must be the classifier's classes {clf.class_names!r}, got {list(class_names)!r}")
    return _evaluate_with_confusion(lambda x, y, z: clf.predict(x).clamp_(min=0), dataloader, device, class_names, save_dir, prefix)
