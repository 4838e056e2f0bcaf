"""Drop-in for ``framework/domain_adaptation/eval_UDA.py``: ``evaluate_model`` (:21-74), the validation pass of source
pre-training (``segmentation.train``) -- mIoU at the training resolution, the mean entropy of the prediction and, with
``intrp_org``, mIoU against the labels at their native size.

The reference upsamples every batch to a [B,K,H,W] tensor, takes a softmax of the same size for the entropy, and brings every
image to the host for ``np.bincount``.  Here a batch is ONE launch of ``ops.upsample_eval`` on the low-resolution output
(class map, confusion matrix and entropy sum without the upsampled tensor; csrc/pointwise.hip), plus one
``ops.upsample_argmax_hist`` at the native size; the confusion matrices and the per-batch entropy rows stay on the device and
come back in one copy when the loader is exhausted.  A model on the CPU goes through ``ops.upsample_eval_composed``, the
reference's own statements.

Not mirrored: ``evaluate_domain_adaptation``, ``eval_single``, ``eval_best``, ``load_checkpoint_for_evaluation`` and
``display_stats`` -- ADVENT's offline sweep over checkpoint files; they stay with the reference.
"""
import numpy as np
import torch

from onda_amd import ops
from onda_amd.config import unset
from onda_amd.framework.utils.func import per_class_iu

_ROWS = 64  # entropy rows allocated at a time for a loader that does not tell its length


def _size(interp):
    """(H, W) of an nn.Upsample, a _Interp, or the pair itself."""
    size = getattr(interp, "size", interp)
    if isinstance(size, int):
        size = (size, size)
    return tuple(int(v) for v in size)


def _device(cfg):
    """The reference's `transfer` (:24-25): cfg.GPU_ID, else cfg.device; the drop-in's own configs carry OTHERS.DEVICE."""
    if "GPU_ID" in cfg:
        return torch.device("cuda", cfg.GPU_ID) if isinstance(cfg.GPU_ID, int) else torch.device(cfg.GPU_ID)
    if "device" in cfg and not unset(cfg.device):
        return torch.device(cfg.device)
    return torch.device(cfg.OTHERS.DEVICE)


def _labels_for(batch, key, size):
    label = batch[key]
    if tuple(label.shape[1:]) != size:
        raise RuntimeError(f"onda_amd: {key} of {tuple(label.shape[1:])} for an upsample to {size}")
    return label


def evaluate_model(model, val_loader, interp, cfg, return_entropy=False, intrp_org=None, prototype=None):
    """(IoU,) + (entropy,) if return_entropy + (IoU_org,) if intrp_org is not None, as the reference.  entropy = the plain mean
    over the batches of prob_2_entropy(softmax(interp(out), 1)).mean(): a short last batch weighs as much as a full one."""
    dev, n = _device(cfg), cfg.NUM_CLASSES
    size = _size(interp)
    size_org = None if intrp_org is None else _size(intrp_org)
    hists = torch.zeros(2, n, n, dtype=torch.int64, device=dev)
    try:
        capacity = max(len(val_loader), 1)
    except TypeError:
        capacity = _ROWS
    chunks, shapes = [torch.zeros(capacity, 2, dtype=torch.int64, device=dev)], []
    model.eval()
    with torch.no_grad():
        for batch in val_loader:
            out = model(batch["image"].to(dev))[1]
            shape = None
            if isinstance(out, dict):
                if prototype is not None:
                    b, _, h, w = out["out"].size()
                    prior = batch.get("soft_predictions")  # None: a prior of 1
                    shape = (b, h, w)
                    out = prototype.pseudo_labels(out["feat"], prior=None if prior is None else prior.to(dev), soft=True)
                else:
                    out = out["out"]
            B, K = (shape[0], out.shape[1]) if shape is not None else out.shape[:2]
            if len(shapes) == sum(c.shape[0] for c in chunks):
                chunks.append(torch.zeros(_ROWS, 2, dtype=torch.int64, device=dev))
            row = len(shapes) - sum(c.shape[0] for c in chunks[:-1])
            ops.upsample_eval(out, _labels_for(batch, "label", size), hists[0], n, chunks[-1][row], shape=shape)
            shapes.append(B * K * size[0] * size[1])
            if size_org is not None:
                nchw = out if shape is None else out.reshape(*shape, K).permute(0, 3, 1, 2)
                _hist(nchw, _labels_for(batch, "label_raw", size_org), hists[1], n)
    model.train()
    # the one read-back: both matrices and every batch's (entropy sum, non-finite pixels)
    packed = torch.cat([hists.reshape(-1)] + [c.reshape(-1) for c in chunks]).cpu().numpy()
    hist, hist_org = packed[:n * n].reshape(n, n), packed[n * n:2 * n * n].reshape(n, n)
    result = (per_class_iu(hist),)
    if return_entropy:
        ent = packed[2 * n * n:].reshape(-1, 2)[:len(shapes)]
        means = [float("nan") if bad else int(total) / ops.EVAL_FIX / count for (total, bad), count in zip(ent.tolist(), shapes)]
        result += (np.mean(means),)
    if size_org is not None:
        result += (per_class_iu(hist_org),)
    return result


def _hist(out, labels, hist, n):
    """hist += the confusion matrix of interp(out).argmax(1) at the labels' size: the fused kernel on the GPU, the composed
    route (whose entropy is not needed here) elsewhere."""
    if out.is_cuda:
        ops.upsample_argmax_hist(out, labels, hist, n)
    else:
        ops.upsample_eval_composed(out, labels, hist, n)
