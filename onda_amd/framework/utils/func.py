"""Drop-in for the hot-path helpers of ``framework/utils/func.py``: ``bce_loss`` (:28-32), ``loss_calc`` (:35-42),
``lr_poly`` (:45-47), ``prob_2_entropy`` (:71-74) and the evaluation helpers ``fast_hist`` / ``per_class_iu`` (:77-85)."""
import numpy as np
import torch
from torch import nn

from .loss import cross_entropy_2d


def bce_loss(y_pred, y_label):
    """BCEWithLogitsLoss against the constant target `y_label`, on y_pred's own device (the reference's
    ``y_pred.get_device()`` is -1 for a CPU tensor and fails there)."""
    return nn.BCEWithLogitsLoss()(y_pred, torch.full_like(y_pred, float(y_label), dtype=torch.float32))


def loss_calc(pred, label, device, soft=False):
    return cross_entropy_2d(pred, label.long().to(device), soft)


def lr_poly(base_lr, iter, max_iter, power):
    return base_lr * ((1 - float(iter) / max_iter) ** power)


def prob_2_entropy(prob):
    """Probability maps [n,c,h,w] -> weighted self-information maps, the reference's expression in plain torch: for callers
    that hold probabilities.  ADVENT's own softmax(interp(out)) input goes through ``ops.upsample_entropy`` instead."""
    n, c, h, w = prob.size()
    return -torch.mul(prob, torch.log2(prob + 1e-30)) / np.log2(c)


def fast_hist(a, b, n):
    k = (a >= 0) & (a < n)
    return np.bincount(n * a[k].astype(int) + b[k], minlength=n ** 2).reshape(n, n)


def per_class_iu(hist):
    return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist) + np.finfo(float).eps)
