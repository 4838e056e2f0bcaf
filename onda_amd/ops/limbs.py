"""Limb-row tensors and their scales: packed-weight handles, the pools of zeroed max|x| buffers, activations that exist as limb
rows only (`limb_only`), the split pass for the rest."""
import ctypes
import os
from ctypes import byref

import torch

from .. import _lib
from .._lib import OndaConv, OndaLimbOut, call, query
from . import _state
from ._state import BN_EPS, GN_EPS, GN_GROUPS, HEAD_PAD, STEM_K
from .core import _p, _stream, nhwc_ld


class H2Weight:
    """Packed weight of the "f16x2" mode: two f16 limb planes of w * 2^e and the device float max|w| that
    defines e (include/onda_hip.h, f16x2 section)."""
    __slots__ = ("limbs", "amax")

    def __init__(self, limbs, amax):
        self.limbs, self.amax = limbs, amax


_AMAX_POOL = {}


AMAX_SLOTS = 2048  # ONDA_AMAX_FLOATS (include/onda_hip.h): 64 slots, one 128-byte line apart
AMAX_POOL_TENSORS = 16384  # tensors served by one zero-filled pool (128 MB)


WEIGHT_POOL_TENSORS = 256  # pools that serve LONG-LIVED scales (packed weights): 2 MB each


def _new_amax_pool(device, tensors=AMAX_POOL_TENSORS):
    buf = torch.zeros(tensors * AMAX_SLOTS, device=device, dtype=torch.float32)
    if buf.is_cuda:  # the zero-fill runs on the creating stream: any other stream that takes slices waits for it once
        done = torch.cuda.Event()
        done.record()
        return [buf, 0, done, {torch.cuda.current_stream().cuda_stream}]
    return [buf, 0, None, None]


def amax_slot(device, long_lived=False):
    """Zeroed device floats for a tensor's running max|x| (slices of a zero-filled pool: one fill kernel per
    16384 tensors instead of one per tensor; a slice is written by exactly one producer and never reused).
    long_lived: scales that outlive a step (the max|w| of packed weights: a frozen static / dynamic model keeps its slices
    for the whole run) come from small pools of their own -- a pool is freed only when every slice of it has died, and one
    long-lived slice used to pin a whole 128 MB activation pool (round-4 advisor)."""
    key = (str(device), bool(long_lived))
    pool = _AMAX_POOL.get(key)
    if pool is None or pool[1] + AMAX_SLOTS > pool[0].numel():
        pool = _AMAX_POOL[key] = _new_amax_pool(device, WEIGHT_POOL_TENSORS if long_lived else AMAX_POOL_TENSORS)
    if pool[2] is not None:
        cur = torch.cuda.current_stream()
        if cur.cuda_stream not in pool[3]:
            cur.wait_event(pool[2])
            pool[3].add(cur.cuda_stream)
    i = pool[1]
    pool[1] = i + AMAX_SLOTS
    return pool[0][i:i + AMAX_SLOTS]


def reserve_amax_slots(device, n):
    """Make sure the next `n` amax_slot() calls are served from a pool that already exists: call on the main stream before
    work is spread over side streams (a refill is safe on any stream -- the others wait for its zero-fill -- but it then
    costs them that wait)."""
    pool = _AMAX_POOL.get((str(device), False))
    if pool is None or pool[1] + n * AMAX_SLOTS > pool[0].numel():
        _AMAX_POOL[(str(device), False)] = _new_amax_pool(device)


def tag_amax(t, slot):
    """Remember that `slot` holds max|t| (valid while t is not modified in place)."""
    try:
        t._onda_scale = (t._version, slot)
    except AttributeError:
        pass
    return t


def known_amax(t):
    hit = getattr(t, "_onda_scale", None)
    return hit[1] if hit is not None and hit[0] == t._version else None


def activation_scale(x):
    """Device float max|x| of an NHWC fp32 activation ("f16x2" mode).  Usually the kernel that produced x
    already left it behind (BatchNorm apply / backward, folded-BN conv epilogue: tag_amax); otherwise one
    reduction pass, shared by every conv that reads the same tensor object."""
    slot = known_amax(x)
    if slot is not None:
        return slot
    B, H, W, C = x.shape
    slot = amax_slot(x.device)
    call("onda_absmax", _p(x), B * H * W, C, nhwc_ld(x), _p(slot), _stream())
    tag_amax(x, slot)
    return slot


class Limbs:
    """An activation as the two f16 limb planes of x * 2^e (include/onda_hip.h, pre-split section):
    planes f16[2, rows, ld], `amax` the device floats that define e."""
    __slots__ = ("planes", "amax", "ld", "plane", "true_amax")

    def __init__(self, planes, amax, ld, plane, true_amax=None):
        self.planes, self.amax, self.ld, self.plane = planes, amax, ld, plane
        # planes whose scale comes from an a-priori BOUND (eval-mode conv outputs) also carry their true max|x|: it is
        # what bounds the next layer's output, so that bounds do not compound
        self.true_amax = true_amax if true_amax is not None else amax


def activation_limbs(x):
    """Limb planes of an NHWC fp32 activation: left behind by its producer, or one split pass shared by
    every conv that reads the same tensor object."""
    hit = getattr(x, "_onda_limbs", None)
    if hit is not None and hit[0] == x._version:
        return hit[1]
    amax = activation_scale(x)
    B, H, W, C = x.shape
    rows = B * H * W
    planes = torch.empty(2, rows, C, device=x.device, dtype=torch.float16)
    call("onda_split_h2", _p(x), rows, C, nhwc_ld(x), _p(planes), C, rows * C, _p(amax), _stream())
    lb = Limbs(planes, amax, C, rows * C)
    try:
        x._onda_limbs = (x._version, lb)
    except AttributeError:
        pass
    return lb


def limb_only(shape, device, limbs):
    """A limb-only activation as autograd sees it: an fp32 [B,H,W,C]-SHAPED tensor without storage behind it (every
    stride 0) that carries the limb planes; gradients with respect to it are ordinary fp32 tensors of that shape."""
    t = torch.empty(1, device=device, dtype=torch.float32).as_strided(tuple(shape), (0,) * len(shape))
    t._onda_limbs = (t._version, limbs)
    return t


def is_limb_only(t):
    return t.dim() == 4 and t.stride() == (0, 0, 0, 0) and t.numel() > 1


def limbs_of(x):
    """Limb planes of an activation: carried by the tensor (its producer wrote them), or one split pass."""
    hit = getattr(x, "_onda_limbs", None)
    if hit is not None and hit[0] == x._version:
        return hit[1]
    if is_limb_only(x):
        raise RuntimeError("onda_amd: a limb-only activation lost its limb planes (it was copied or re-wrapped on the way "
                           "to its consumer); this is a bug in the caller, there is no fp32 copy to fall back to")
    return activation_limbs(x)


def _stat_tile_rows(stats):
    """GEMM rows one row of a conv's statistic partials covers (256 or 128: l2_plan's tile height, recorded by
    conv_forward).  Two row groups split their partials by it; there is no way to re-derive it from (M, C) alone -- short K
    loops run 128-row tiles (l2_plan) -- so a partial table that lost the attribute (detached, cloned, re-wrapped) is an
    error, not a guess (round-5 advisor)."""
    rows = getattr(stats, "_onda_tile_rows", None)
    if not rows:
        raise RuntimeError("onda_amd: BatchNorm with two row groups needs the statistic partials as conv_forward returned "
                           "them (the tensor lost its tile height: it was copied or re-wrapped on the way)")
    return rows


def limb_mode(channels):
    """Do the BatchNorm kernels write their output as limb planes only (no fp32 copy)?"""
    return _state.CONV_MODE == "f16x2" and channels % 32 == 0 and _state.LIMB_ONLY




def materialize(x):
    """fp32 NHWC copy of an activation (diagnostics and tests): limb-only tensors are rebuilt from their planes."""
    if not is_limb_only(x):
        return x
    lb = limbs_of(x)
    B, H, W, C = x.shape
    # limb rows [rows][ld / 32][2][32] -> the two limbs as [rows][ld]
    planes = lb.planes.reshape(B * H * W, lb.ld // 32, 2, 32).permute(2, 0, 1, 3).reshape(2, B * H * W, lb.ld)[:, :, :C].float()
    amax = lb.amax.max()
    e = torch.where((amax > 0) & (amax < 3e38), 15 - torch.frexp(amax)[1], torch.zeros((), dtype=torch.int32, device=x.device))
    return ((planes[0] + planes[1] / query("onda_limb2_scale")) * torch.ldexp(torch.ones((), device=x.device), -e)).reshape(B, H, W, C)


