"""The segmentation head's tail: class slices, fused CE / RCE / MRKLD (and, off the default path, MRENT and the JS term, and
the same loss against a soft target),
softmax statistics, bilinear upsampling (+ fused cross-entropy / argmax / confusion matrix / calibration table / ADVENT's
entropy map), the device-side prior select."""
import ctypes
import math
import os
from ctypes import byref

import torch

from .. import _lib
from .._lib import OndaConv, OndaLimbOut, call, query
from . import _state
from ._state import BN_EPS, GN_EPS, GN_GROUPS, HEAD_PAD, STEM_K
from .core import _p, _stream


class ClassSliceFn(torch.autograd.Function):
    """[B,h,w,32] padded head output -> the reference's NCHW `out` f32[B,K,h,w] (a view)."""

    @staticmethod
    def forward(ctx, out_pad, k):
        ctx.k, ctx.pad = k, out_pad.shape[3]
        return out_pad[..., :k].permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        B, K, H, W = dout.shape
        g = torch.zeros(B, H, W, ctx.pad, device=dout.device, dtype=torch.float32)
        g[..., :K].copy_(dout.permute(0, 2, 3, 1))
        return g, None


def logits_rows(out):
    """(tensor, ld, N, K) of an NCHW logits tensor laid out pixel-major (as this model
    returns it); copies into a padded pixel-major buffer otherwise."""
    B, K, H, W = out.shape
    ld = out.stride(3)
    if out.stride(1) == 1 and out.stride(2) == W * ld and (B == 1 or out.stride(0) == H * W * ld) and ld >= K:
        return out, ld, B * H * W, K
    buf = torch.zeros(B, H, W, HEAD_PAD, device=out.device, dtype=torch.float32)
    buf[..., :K].copy_(out.detach().permute(0, 2, 3, 1))
    return buf, HEAD_PAD, B * H * W, K


def _loss_setup(ctx, out, labels):
    """What the two fused losses' forward passes share: (rows, ld, N, K, labels i64[N], result f32[8], ws)."""
    rows, ld, N, K = logits_rows(out)
    labels = labels.reshape(-1).to(device=out.device, dtype=torch.int64).contiguous()
    result = torch.empty(8, device=out.device, dtype=torch.float32)
    ws = torch.empty(8 * (N // 256 + 1), device=out.device, dtype=torch.float32)
    ctx.save_for_backward(rows, labels, result)
    ctx.shape = tuple(out.shape)
    ctx.set_materialize_grads(False)
    return rows, ld, N, K, labels, result, ws


def _loss_backward_setup(ctx, gtotal):
    """What their backward passes share: (rows, labels, result, the upstream gradient as a device scalar, dl [B,H,W,ld])."""
    rows, labels, result = ctx.saved_tensors
    B, _, H, W = ctx.shape
    dl = torch.empty(B, H, W, ctx.meta[0], device=rows.device, dtype=torch.float32)
    return rows, labels, result, gtotal.reshape(1).to(torch.float32).contiguous(), dl


class SegLossFn(torch.autograd.Function):
    """w_ce*CE + w_rce*RCE + w_reg*MRKLD over hard labels, one pass; returns
    (total, ce, rce, mrkld) with gradients flowing through `total` only."""

    @staticmethod
    def forward(ctx, out, labels, w_ce, w_rce, w_reg):
        rows, ld, N, K, labels, result, ws = _loss_setup(ctx, out, labels)
        call("onda_seg_loss_fwd", _p(rows), ld, _p(labels), _p(result), _p(ws), N, K, _stream())
        ctx.meta = (ld, N, K, w_ce, w_rce, w_reg)
        ce, rce, reg = result[0], result[1], result[2]
        total = w_ce * ce + w_rce * rce + w_reg * reg
        ctx.mark_non_differentiable(ce, rce, reg)
        return total, ce, rce, reg

    @staticmethod
    def backward(ctx, gtotal, _a, _b, _c):
        if gtotal is None:
            return None, None, None, None, None
        rows, labels, result, g, dl = _loss_backward_setup(ctx, gtotal)
        ld, N, K, w_ce, w_rce, w_reg = ctx.meta
        call("onda_seg_loss_bwd", _p(rows), ld, _p(labels), _p(result), _p(g), w_ce, w_rce, w_reg, _p(dl), N, K,
             _stream())
        return dl[..., :K].permute(0, 3, 1, 2), None, None, None, None


def seg_losses(out, labels, w_ce=1.0, w_rce=0.0, w_reg=0.0):
    return SegLossFn.apply(out, labels, float(w_ce), float(w_rce), float(w_reg))


REGULARIZERS = {"MRKLD": 1, "MRENT": 2}  # any other name contributes 0, as in the reference's regular_loss


class TargetLossFn(torch.autograd.Function):
    """w_ce*CE + w_rce*RCE + w_reg*reg + w_js*JS over hard labels, one pass; reg is MRKLD, MRENT or nothing (selector
    0 / 1 / 2, REGULARIZERS) and JS the ProDA Jensen-Shannon term.  Returns (total, ce, rce, reg, js) with gradients
    flowing through `total` only; a term whose weight is 0 is left out of `total`.  Every label 255: js = +inf and, with
    w_js > 0, a NaN gradient, as in the reference."""

    @staticmethod
    def forward(ctx, out, labels, w_ce, w_rce, w_reg, regularizer, w_js):
        rows, ld, N, K, labels, result, ws = _loss_setup(ctx, out, labels)
        call("onda_target_loss_fwd", _p(rows), ld, _p(labels), regularizer, w_ce, w_rce, w_reg, w_js, _p(result), _p(ws),
             N, K, _stream())
        ctx.meta = (ld, N, K, w_ce, w_rce, w_reg, regularizer, w_js)
        ce, rce, reg, js, total = result[0], result[1], result[2], result[3], result[6].clone()
        ctx.mark_non_differentiable(ce, rce, reg, js)
        return total, ce, rce, reg, js

    @staticmethod
    def backward(ctx, gtotal, _a, _b, _c, _d):
        if gtotal is None:
            return None, None, None, None, None, None, None
        rows, labels, result, g, dl = _loss_backward_setup(ctx, gtotal)
        ld, N, K, w_ce, w_rce, w_reg, regularizer, w_js = ctx.meta
        call("onda_target_loss_bwd", _p(rows), ld, _p(labels), regularizer, w_ce, w_rce, w_reg, w_js, _p(result), _p(g),
             _p(dl), N, K, _stream())
        return dl[..., :K].permute(0, 3, 1, 2), None, None, None, None, None, None


def target_losses(out, labels, w_ce=1.0, w_rce=0.0, w_reg=0.0, regularizer="MRKLD", w_js=0.0):
    """The reference's whole hard-label target loss (prototypes.py:299-333): (total, ce, rce, reg, js)."""
    return TargetLossFn.apply(out, labels, float(w_ce), float(w_rce), float(w_reg), REGULARIZERS.get(regularizer, 0),
                              float(w_js))


def soft_rows_of(soft, N, K, device):
    """(tensor, ld) of a soft target as pixel-major float32 rows: the [N,K] map itself (no copy), or an NCHW tensor, float
    or integer, brought to rows (no copy either where it is a view of such a map)."""
    if soft.dim() == 4:
        soft = soft.permute(0, 2, 3, 1).reshape(-1, soft.shape[1])
    if soft.dim() != 2 or tuple(soft.shape) != (N, K):
        raise ValueError(f"soft_target_losses: a soft target of shape {tuple(soft.shape)} for {N} pixels of {K} classes")
    soft = soft.detach().to(device=device, dtype=torch.float32)
    if soft.stride(1) != 1 or soft.stride(0) < K:
        soft = soft.contiguous()
    return soft, soft.stride(0)


class SoftLossFn(torch.autograd.Function):
    """w_ce*CE + w_rce*RCE + w_reg*reg against a SOFT target (the reference's SOFT_LABELS branch), one pass each way; reg
    as in TargetLossFn.  CE reads the raw logits -- NaN over negative ones, with a finite gradient -- against trunc(target)
    (ce_trunc, func.loss_calc's `.long()`) or the target itself; RCE uses the real soft values (include/onda_hip.h).
    Returns (total, ce, rce, reg) with gradients flowing through `total` only; a term whose weight is 0 is left out of
    `total` and of the gradient."""

    @staticmethod
    def forward(ctx, out, soft, w_ce, w_rce, w_reg, regularizer, ce_trunc):
        rows, ld, N, K = logits_rows(out)
        soft, lds = soft_rows_of(soft, N, K, out.device)
        result = torch.empty(8, device=out.device, dtype=torch.float32)
        ws = torch.empty(8 * (N // 256 + 1), device=out.device, dtype=torch.float32)
        call("onda_soft_loss_fwd", _p(rows), ld, _p(soft), lds, ce_trunc, regularizer, w_ce, w_rce, w_reg, _p(result), _p(ws),
             N, K, _stream())
        ctx.save_for_backward(rows, soft)
        ctx.shape = tuple(out.shape)
        ctx.set_materialize_grads(False)
        ctx.meta = (ld, lds, N, K, w_ce, w_rce, w_reg, regularizer, ce_trunc)
        ce, rce, reg, total = result[0], result[1], result[2], result[3].clone()
        ctx.mark_non_differentiable(ce, rce, reg)
        return total, ce, rce, reg

    @staticmethod
    def backward(ctx, gtotal, _a, _b, _c):
        if gtotal is None:
            return None, None, None, None, None, None, None
        rows, soft = ctx.saved_tensors
        ld, lds, N, K, w_ce, w_rce, w_reg, regularizer, ce_trunc = ctx.meta
        B, _, H, W = ctx.shape
        g = gtotal.reshape(1).to(torch.float32).contiguous()
        dl = torch.empty(B, H, W, ld, device=rows.device, dtype=torch.float32)
        call("onda_soft_loss_bwd", _p(rows), ld, _p(soft), lds, ce_trunc, regularizer, w_ce, w_rce, w_reg, _p(g), _p(dl), N, K,
             _stream())
        return dl[..., :K].permute(0, 3, 1, 2), None, None, None, None, None, None


def soft_target_losses(out, soft_rows, w_ce=1.0, w_rce=0.0, w_reg=0.0, regularizer="MRKLD", ce_trunc=True):
    """The reference's soft-label target loss (prototypes.py:305-328 with SOFT_LABELS): (total, ce, rce, reg).  `soft_rows`:
    the [N,K] soft map in the pixel order of `out`, or an NCHW tensor (float or int64)."""
    return SoftLossFn.apply(out, soft_rows, float(w_ce), float(w_rce), float(w_reg), REGULARIZERS.get(regularizer, 0),
                            int(bool(ce_trunc)))


def softmax_stats(out, want_probs=False, want_argmax=False):
    """Per-pixel softmax of NCHW logits: (mean max-prob 0-dim tensor, probs [N,K] or None, argmax i32[N] or None)."""
    rows, ld, N, K = logits_rows(out)
    probs = torch.empty(N, K, device=out.device, dtype=torch.float32) if want_probs else None
    am = torch.empty(N, device=out.device, dtype=torch.int32) if want_argmax else None
    result = torch.empty(1, device=out.device, dtype=torch.float32)
    ws = torch.empty(N // 256 + 1, device=out.device, dtype=torch.float32)
    call("onda_softmax_stats", _p(rows), ld, _p(probs), K, _p(am), _p(result), _p(ws), N, K, _stream())
    return result[0], probs, am


class UpsampleFn(torch.autograd.Function):
    """nn.Upsample(size, bilinear, align_corners=True) on the pixel-major logits -> NCHW."""

    @staticmethod
    def forward(ctx, out, size):
        rows, ld, _, K = logits_rows(out)
        B, _, h, w = out.shape
        H, W = size
        up = torch.empty(B, K, H, W, device=out.device, dtype=torch.float32)
        call("onda_upsample_fwd", _p(rows), ld, _p(up), B, h, w, K, H, W, _stream())
        ctx.meta = (B, h, w, K, H, W)
        return up

    @staticmethod
    def backward(ctx, dup):
        B, h, w, K, H, W = ctx.meta
        dup = dup.contiguous()
        dl = torch.zeros(B, h, w, HEAD_PAD, device=dup.device, dtype=torch.float32)
        call("onda_upsample_bwd", _p(dup), _p(dl), HEAD_PAD, B, h, w, K, H, W, _stream())
        return dl[..., :K].permute(0, 3, 1, 2), None


class UpsampleCEFn(torch.autograd.Function):
    """loss_calc(interp(out), label): bilinear upsample (align_corners) to the label resolution -> cross-entropy over the
    pixels whose label is not 255, as ONE pass in each direction -- the upsampled logits (and their gradient) exist in
    registers only (csrc/pointwise.hip).
    Label contract: integer class maps with values in [0, K) or the ignore value 255; they travel as uint8, so any value >= K
    (a negative one wraps to >= 128) is IGNORED, as F.cross_entropy(ignore_index=255) ignores 255.  A batch without a single
    kept pixel returns NaN like the reference's mean over zero pixels (utils/loss.py:88-112), and its gradient is all zeros --
    what torch's own nll_loss backward produces for total_weight == 0 -- not NaN: the caller sees the NaN loss."""

    @staticmethod
    def forward(ctx, out, labels):
        rows, ld, _, K = logits_rows(out)
        B, _, h, w = out.shape
        labels = labels.to(device=out.device, dtype=torch.uint8).contiguous()
        H, W = labels.shape[1:]
        result = torch.empty(2, device=out.device, dtype=torch.float32)
        ws = torch.empty(query("onda_upsample_ce_ws", B, H, W), device=out.device, dtype=torch.float32)
        call("onda_upsample_ce_fwd", _p(rows), ld, _p(labels), _p(result), _p(ws), B, h, w, K, H, W, _stream())
        ctx.save_for_backward(rows, labels, result)
        ctx.meta = (ld, B, h, w, K, H, W)
        return result[0]

    @staticmethod
    def backward(ctx, g):
        rows, labels, result = ctx.saved_tensors
        ld, B, h, w, K, H, W = ctx.meta
        dl = torch.empty(B, h, w, ld, device=rows.device, dtype=torch.float32)
        ws = torch.empty(query("onda_upsample_ce_bwd_ws", B, w, K, H), device=rows.device, dtype=torch.float32)
        call("onda_upsample_ce_bwd", _p(rows), ld, _p(labels), _p(result), _p(g.reshape(1).float().contiguous()), 1.0, _p(dl),
             _p(ws), B, h, w, K, H, W, _stream())
        return dl[..., :K].permute(0, 3, 1, 2), None


_UCE_FUSED = {}  # (w, W) -> does the fused head's backward take the width pair


def upsample_ce(out, labels):
    """loss_calc(interp(out), label).  Fused (UpsampleCEFn) wherever its backward runs; past ~211x upsampling along x, where
    one low-resolution column's output span no longer fits the backward's row pass, UpsampleFn followed by torch's
    cross-entropy under the same label contract (values >= K ignored; no kept pixel: NaN, gradient zeros)."""
    key = (out.shape[3], labels.shape[2])
    if key not in _UCE_FUSED:
        _UCE_FUSED[key] = bool(query("onda_upsample_ce_fused", *key))
    if _UCE_FUSED[key]:
        return UpsampleCEFn.apply(out, labels)
    K = out.shape[1]
    labels = labels.to(device=out.device, dtype=torch.uint8).long()
    up = UpsampleFn.apply(out, tuple(labels.shape[1:]))
    return torch.nn.functional.cross_entropy(up, labels.masked_fill(labels >= K, -100), ignore_index=-100)


class UpsampleEntropyFn(torch.autograd.Function):
    """prob_2_entropy(softmax(interp(out), 1)) -> f32[B,K,H,W] (ADVENT's discriminator input, advent_da.py:94-128): ONE pass in
    each direction, the upsampled logits and the softmax in registers only (csrc/pointwise.hip).  2 <= K <= 32."""

    @staticmethod
    def forward(ctx, out, size):
        rows, ld, _, K = logits_rows(out)
        B, _, h, w = out.shape
        H, W = size
        ent = torch.empty(B, K, H, W, device=out.device, dtype=torch.float32)
        call("onda_upsample_entropy_fwd", _p(rows), ld, _p(ent), B, h, w, K, H, W, _stream())
        ctx.save_for_backward(rows)
        ctx.meta = (ld, B, h, w, K, H, W)
        ctx.set_materialize_grads(False)
        return ent

    @staticmethod
    def backward(ctx, dent):
        if dent is None:
            return None, None
        rows, = ctx.saved_tensors
        ld, B, h, w, K, H, W = ctx.meta
        dent = dent.to(torch.float32).contiguous()
        dl = torch.empty(B, h, w, ld, device=rows.device, dtype=torch.float32)
        ws = torch.empty(query("onda_upsample_entropy_bwd_ws", B, w, K, H, W), device=rows.device, dtype=torch.float32)
        call("onda_upsample_entropy_bwd", _p(rows), ld, _p(dent), _p(dl), _p(ws), B, h, w, K, H, W, _stream())
        return dl[..., :K].permute(0, 3, 1, 2), None


def upsample_entropy(out, size):
    """ADVENT's entropy map of the model's `out` at `size` = (H, W), differentiable with respect to `out`."""
    return UpsampleEntropyFn.apply(out, tuple(size))


def upsample_entropy_composed(out, size):
    """The same map the way the reference composes it -- UpsampleFn, torch.softmax, the entropy expression, autograd for the
    backward pass: three [B,K,H,W] tensors in memory.  The yardstick of tools/entropy_timing.py and of the step test."""
    p = torch.softmax(UpsampleFn.apply(out, tuple(size)), 1)
    return -torch.mul(p, torch.log2(p + 1e-30)) / math.log2(out.shape[1])


def upsample_argmax(out, size):
    """Fused evaluation tail: class map u8[B,H,W] of interp(out).softmax(1).argmax(1)."""
    rows, ld, _, K = logits_rows(out)
    B, _, h, w = out.shape
    H, W = size
    cls = torch.empty(B, H, W, device=out.device, dtype=torch.uint8)
    call("onda_upsample_argmax", _p(rows), ld, _p(cls), B, h, w, K, H, W, _stream())
    return cls


def upsample_argmax_hist(out, labels, hist, num_classes):
    """Evaluation tail on the GPU: hist[K,K] (int64, accumulated) += confusion matrix of the
    upsampled argmax of `out` against `labels` u8[B,H,W] (values >= K are ignored)."""
    rows, ld, _, K = logits_rows(out)
    B, _, h, w = out.shape
    labels = labels.to(device=out.device, dtype=torch.uint8).contiguous()
    H, W = labels.shape[1:]
    call("onda_upsample_argmax_hist", _p(rows), ld, _p(labels), _p(hist), None, B, h, w, num_classes, H, W, _stream())
    return hist


def upsample_ece(out_or_rows, labels, table, bins, probs=False, hist=None, num_classes=None, shape=None):
    """Calibration table of ECE.record(interp(out).softmax(1), label) (probs=False) or ECE.record(interp(out), label)
    (probs=True: `out` holds probabilities) without the upsampled tensor: table i64[bins + 1, 3] (accumulated) += per bin
    (sum of round(conf * 2^32), correct, pixels), non-finite confidences in row `bins` (include/onda_hip.h).
    `out_or_rows`: NCHW logits as upsample_argmax_hist takes them, or an [N,K] map with shape=(B, h, w).  With `hist`
    (i64[K,K], accumulated) the same launch also counts the confusion matrix of upsample_argmax_hist."""
    if out_or_rows.dim() == 2:
        if shape is None:
            raise ValueError("upsample_ece: an [N,K] map needs shape=(B, h, w)")
        B, h, w = shape
        N, K = out_or_rows.shape
        if N != B * h * w:
            raise ValueError(f"upsample_ece: {N} rows for shape {tuple(shape)}")
        out_or_rows = out_or_rows.reshape(B, h, w, K).permute(0, 3, 1, 2)
    rows, ld, _, K = logits_rows(out_or_rows)
    if rows.dtype != torch.float32:
        raise TypeError("upsample_ece: float32 only")
    B, _, h, w = out_or_rows.shape
    if num_classes is not None and num_classes != K:
        raise ValueError(f"upsample_ece: {K} classes in the map, num_classes = {num_classes}")
    labels = labels.to(device=rows.device, dtype=torch.uint8).contiguous()
    if labels.dim() != 3 or labels.shape[0] != B:
        raise ValueError(f"upsample_ece: labels of shape {tuple(labels.shape)} for a batch of {B}")
    H, W = labels.shape[1:]
    if table.dtype != torch.int64 or tuple(table.shape) != (bins + 1, 3) or not table.is_contiguous() or table.device != rows.device:
        raise ValueError(f"upsample_ece: table must be contiguous int64 [{bins + 1}, 3] on {rows.device}")
    if hist is not None and (hist.dtype != torch.int64 or hist.numel() != K * K or not hist.is_contiguous()
                             or hist.device != rows.device):
        raise ValueError(f"upsample_ece: hist must be contiguous int64 [{K}, {K}] on {rows.device}")
    call("onda_upsample_ece", _p(rows), ld, _p(labels), _p(table), int(bins), int(bool(probs)), _p(hist), B, h, w, K, H, W,
         _stream())
    return table


EVAL_FIX = 4294967296.0  # 2^32: the fixed point of ent[0] (ECE_FIX of csrc/pointwise.hip)
EVAL_KMIN, EVAL_KMAX = 2, 32  # classes onda_upsample_eval takes (the K-vector of a pixel stays in registers)
EVAL_FUSED = True  # False (the tests): upsample_eval takes the composed route on the GPU as well


def _eval_args(out_or_rows, labels, hist, num_classes, cls, shape):
    """What upsample_eval and upsample_eval_composed share: the checks of upsample_ece -> (NCHW view, labels u8 or None, (H, W))."""
    if out_or_rows.dim() == 2:
        if shape is None:
            raise ValueError("upsample_eval: an [N,K] map needs shape=(B, h, w)")
        B, h, w = shape
        N, K = out_or_rows.shape
        if N != B * h * w:
            raise ValueError(f"upsample_eval: {N} rows for shape {tuple(shape)}")
        out_or_rows = out_or_rows.reshape(B, h, w, K).permute(0, 3, 1, 2)
    if out_or_rows.dtype != torch.float32:
        raise TypeError("upsample_eval: float32 only")
    B, K = out_or_rows.shape[:2]
    dev = out_or_rows.device
    if num_classes is not None and num_classes != K:
        raise ValueError(f"upsample_eval: {K} classes in the map, num_classes = {num_classes}")
    if (labels is None) != (hist is None):
        raise ValueError("upsample_eval: labels and hist are given together or not at all")
    if labels is not None:
        labels = labels.to(device=dev, dtype=torch.uint8).contiguous()
        if labels.dim() != 3 or labels.shape[0] != B:
            raise ValueError(f"upsample_eval: labels of shape {tuple(labels.shape)} for a batch of {B}")
        size = tuple(labels.shape[1:])
        if hist.dtype != torch.int64 or hist.numel() != K * K or not hist.is_contiguous() or hist.device != dev:
            raise ValueError(f"upsample_eval: hist must be contiguous int64 [{K}, {K}] on {dev}")
    elif cls is None:
        raise ValueError("upsample_eval: without labels the size comes from cls u8[B,H,W]")
    else:
        size = tuple(cls.shape[1:])
    if cls is not None and (cls.dtype != torch.uint8 or tuple(cls.shape) != (B,) + size or not cls.is_contiguous() or cls.device != dev):
        raise ValueError(f"upsample_eval: cls must be contiguous uint8 {(B,) + size} on {dev}")
    return out_or_rows, labels, size


def upsample_eval_composed(out_or_rows, labels, hist, num_classes, cls=None, shape=None):
    """evaluate_model's per-batch tail the way the reference composes it (eval_UDA.py:47-57): interp (UpsampleFn on the GPU,
    F.interpolate elsewhere) -> torch softmax -> the entropy expression -> .mean(), three [B,K,H,W] tensors in memory, and the
    confusion matrix of the upsampled argmax (ops.upsample_argmax_hist on the GPU, fast_hist's bincount elsewhere) accumulated
    into `hist`.  Returns the batch's entropy mean, a float32 scalar on the input's device.  Arguments as upsample_eval; any K.
    The yardstick of tools/eval_timing.py and of the tests."""
    out, labels, size = _eval_args(out_or_rows, labels, hist, num_classes, cls, shape)
    K = out.shape[1]
    with torch.no_grad():
        if out.is_cuda:
            up = UpsampleFn.apply(out, size)
        else:
            up = torch.nn.functional.interpolate(out, size=size, mode="bilinear", align_corners=True)
        p = torch.softmax(up, 1)
        mean = (-torch.mul(p, torch.log2(p + 1e-30)) / math.log2(K)).mean()
        if labels is not None:
            if out.is_cuda and K <= 255:
                upsample_argmax_hist(out, labels, hist, K)
            else:
                a, b = labels.reshape(-1).long(), up.argmax(1).reshape(-1)
                keep = a < K  # fast_hist (func.py:77-79): rows = ground truth in [0, K), columns = prediction
                hist.view(-1).add_(torch.bincount(K * a[keep] + b[keep], minlength=K * K))
        if cls is not None:
            cls.copy_(upsample_argmax(out, size) if out.is_cuda and K <= 255 else up.argmax(1))
    return mean


def upsample_eval(out_or_rows, labels, hist, num_classes, ent, cls=None, shape=None):
    """evaluate_model's per-batch tail (eval_UDA.py:47-57) in one launch and one read of the low-resolution map, without the
    upsampled tensor: hist i64[K,K] (accumulated) += the confusion matrix of upsample_argmax_hist, `cls` (optional u8[B,H,W])
    = the class map, and ent i64[2] (accumulated) += (sum over the pixels of round(e * 2^32), pixels with a non-finite e),
    e = the sum over the classes of prob_2_entropy(softmax(interp(out), 1)) (include/onda_hip.h); entropy_mean turns `ent`
    into the reference's `.mean()`.  `out_or_rows`: NCHW logits, or an [N,K] map with shape=(B, h, w); labels u8[B,H,W] give
    the size (labels = hist = None: `cls` does).  Off the GPU, or with K outside [2, 32], upsample_eval_composed does the
    work and its mean is written into `ent` in the same fixed point."""
    out, labels, size = _eval_args(out_or_rows, labels, hist, num_classes, cls, shape)
    if ent.dtype != torch.int64 or tuple(ent.shape) != (2,) or not ent.is_contiguous() or ent.device != out.device:
        raise ValueError(f"upsample_eval: ent must be contiguous int64 [2] on {out.device}")
    B, K, h, w = out.shape
    if not out.is_cuda or not EVAL_KMIN <= K <= EVAL_KMAX or not EVAL_FUSED:
        mean = upsample_eval_composed(out, labels, hist, num_classes, cls=cls).double()
        ok = torch.isfinite(mean)
        total = torch.round(torch.where(ok, mean, torch.zeros_like(mean)) * (float(B * K * size[0] * size[1]) * EVAL_FIX))
        ent.add_(torch.stack([total.long(), (~ok).long()]))
        return ent
    rows, ld, _, _ = logits_rows(out)
    call("onda_upsample_eval", _p(rows), ld, _p(labels), _p(hist), _p(ent), _p(cls), B, h, w, K, size[0], size[1], _stream())
    return ent


def entropy_mean(ent, B, K, H, W):
    """prob_2_entropy(F.softmax(interp(x), 1)).mean() of a batch from upsample_eval's `ent`: ent[0] / 2^32 / (B*K*H*W) as a
    float64 scalar on ent's device; NaN when a pixel's entropy was not finite (ent[1] > 0)."""
    mean = ent[0].double() / EVAL_FIX / float(B * K * H * W)
    return torch.where(ent[1] > 0, torch.full_like(mean, float("nan")), mean)


# ------------------------------------------------------------------------------- device-side switch
def select_prior(flag, a, wa, b, wb):
    """flag ? wb * b : wa * a, elementwise, as a true select (`b` may be garbage when flag == 0).  `a` and `b` may be any
    views of one shape; the result is contiguous in that shape (empty_like would keep a dense permuted view's strides,
    which the kernel's flat order does not follow)."""
    out = torch.empty(a.shape, device=a.device, dtype=a.dtype)
    # the contiguous copies are held until the launch is enqueued: as temporaries, a's block would be freed at once and handed
    # to b's copy, and the kernel would read b through both pointers
    ac, bc = a.contiguous(), b.contiguous()
    call("onda_select_prior", _p(flag), _p(ac), float(wa), _p(bc), float(wb), _p(out), a.numel(), _stream())
    return out


def gate_scalar(flag, v):
    """flag ? v : NaN as a device scalar."""
    out = torch.empty(1, device=v.device, dtype=torch.float32)
    v32 = v.detach().reshape(1).float()  # (held until the launch is enqueued: a float64 scalar is a copy)
    call("onda_gate_scalar", _p(flag), _p(v32), _p(out), _stream())
    return out[0]


# ------------------------------------------------------------------------------- multi-tensor
