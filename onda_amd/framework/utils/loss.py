"""Drop-in for the hot-path functions of ``framework/utils/loss.py``: ``CXE`` (:12-13), ``cross_entropy_2d``
(:16-45), ``rce`` (:88-112) and ``js_divergance`` (:62-85) on the fused HIP loss kernels, hard-label and soft-label
(``soft=True``, the ``SOFT_LABELS`` setting) branches."""
from onda_amd import ops


def CXE(predicted, target):
    """-(target * log(predicted + 1e-6)).sum(1).mean() of two [n,c,h,w] tensors (reference :12-13) on the soft-loss kernels.
    `predicted` is used as it comes: over raw logits the value is NaN wherever predicted + 1e-6 < 0, whatever the target
    holds there, and the gradient -(target / n_pixels) / (predicted + 1e-6) stays finite."""
    return ops.soft_target_losses(predicted, target, 1.0, 0.0, 0.0, "none", ce_trunc=False)[0]


def cross_entropy_2d(predict, target, soft=False):
    """predict f32[n,c,h,w], target int[n,h,w]; mean CE over pixels with 0 <= target != 255
    (NaN when no pixel qualifies, like the reference)."""
    assert not target.requires_grad
    assert predict.dim() == 4
    assert target.dim() == 3 or target.dim() == 4
    assert predict.size(0) == target.size(0), f"{predict.size(0)} vs {target.size(0)}"
    assert predict.size(-2) == target.size(-2), f"{predict.size(-2)} vs {target.size(-2)}"
    assert predict.size(-1) == target.size(-1), f"{predict.size(-1)} vs {target.size(-1)}"
    if soft:  # the target as it is handed in: func.loss_calc has truncated it (`.long()`), a direct caller has not
        return CXE(predict, target)
    return ops.seg_losses(predict, target, 1.0, 0.0, 0.0)[0]


def rce(pred, labels, device, soft=False):
    if soft:  # -sum(softmax(pred) * log(labels + 1e-6)) / n_pixels over the real soft values (reference :95-99)
        return ops.soft_target_losses(pred, labels, 0.0, 1.0, 0.0, "none", ce_trunc=False)[0]
    return ops.seg_losses(pred, labels, 0.0, 1.0, 0.0)[0]


def js_divergance(pred, labels, device):
    """ProDA's Jensen-Shannon term (reference :62-85) on the fused HIP target-loss kernel: the one-hot of `labels` clamped
    to [1e-4, 1] against softmax(pred) masked to the kept pixels, divided by the kept-pixel count (+inf, with a NaN
    gradient, when every label is 255 -- as the reference)."""
    return ops.target_losses(pred, labels, 0.0, 0.0, 0.0, "none", 1.0)[0]
