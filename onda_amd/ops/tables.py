"""Multi-tensor launches over device tables (pinned staging buffers): duplicate-replaying SGD (plain and EWC-anchored), teacher
EMA, the EWC penalty's value, the swap of two tensor sets."""
import ctypes
import os
from ctypes import byref

import torch

from .. import _lib
from .._lib import OndaConv, OndaLimbOut, call, query
from . import _state
from ._state import BN_EPS, GN_EPS, GN_GROUPS, HEAD_PAD, STEM_K
from .core import _p, _stream


_TABLE_STAGES = {}


def _table(entries, struct, device):
    """The entry table of a multi-tensor launch on `device`.  A pageable host->device copy would stop the host until
    the stream has drained (measured: 39 ms behind the backward pass for the optimizer's table, 13 ms per weight
    repack): the bytes go through a small ring of pinned staging buffers with an asynchronous copy instead; a buffer is
    reused once the event recorded behind its copy has completed."""
    arr = (struct * len(entries))(*entries)
    raw = bytearray(bytes(arr))
    n = len(raw)
    host = torch.frombuffer(raw, dtype=torch.uint8)
    if torch.device(device).type != "cuda":
        return host.to(device)
    ring = _TABLE_STAGES.setdefault(str(device), [])
    slot = None
    for cand in ring:
        if cand[0].numel() >= n and cand[1].query():
            slot = cand
            break
    if slot is None:
        if len(ring) >= 16:  # (cannot happen with a few tables per step; bound the ring anyway)
            slot = max(ring, key=lambda c: c[0].numel())
            slot[1].synchronize()
            if slot[0].numel() < n:
                slot[0] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        else:
            slot = [torch.empty(max(n, 1 << 14), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
            ring.append(slot)
    slot[0][:n].copy_(host)
    dev = torch.empty(n, dtype=torch.uint8, device=device)
    dev.copy_(slot[0][:n], non_blocking=True)
    slot[1].record()
    return dev


def sgd_multi(items, momentum, weight_decay, grad_scale=1.0, anchors=None, half_lambda=0.0):
    """items: list of (param, grad, buf, lr, times, fresh).  One launch for all tensors; every gradient element is
    multiplied by `grad_scale` on the way in.  `anchors` (one tensor or None per item; the EWC penalty of the reference's
    ewc.py:47-54): the launch adds -2 * (half_lambda * (anchor - param)), rounded as autograd rounds it, to the gradient
    of the items that have one -- onda_sgd_anchor_multi; an item's grad may be None there (no loss reached it)."""
    blk, ents, first = query("onda_multi_tensor_block"), [], 0
    for i, (p, g, b, lr, times, fresh) in enumerate(items):
        head = (p.data_ptr(), g.data_ptr() if g is not None else None, b.data_ptr())
        tail = (p.numel(), float(lr), int(times), int(fresh), first)
        if anchors is None:
            ents.append(_lib.OndaSgdEntry(*head, *tail))
        else:
            ents.append(_lib.OndaSgdAnchorEntry(*head, anchors[i].data_ptr() if anchors[i] is not None else None, *tail))
        first += -(-p.numel() // blk)
    dev = items[0][0].device
    if anchors is None:
        table = _table(ents, _lib.OndaSgdEntry, dev)
        call("onda_sgd_multi", _p(table), len(ents), float(momentum), float(weight_decay), float(grad_scale), first, _stream())
    else:
        table = _table(ents, _lib.OndaSgdAnchorEntry, dev)
        call("onda_sgd_anchor_multi", _p(table), len(ents), float(momentum), float(weight_decay), float(grad_scale),
             float(half_lambda), first, _stream())
    for p, *_ in items:
        torch.autograd.graph.increment_version(p)


def sqdiff_multi(pairs, half_lambda, cache=None):
    """half_lambda * sum over the pairs (a, b) of sum((a - b)^2) as a 0-dim device tensor (float32 differences and
    squares, a fixed-order sum: onda_sqdiff_multi), one launch for all tensors and one to add its partials up.  `cache`
    (a dict the caller keeps next to a FIXED list of tensors): table and workspace are rebuilt only when an address
    changed, as in ema_multi."""
    key = [(a.data_ptr(), b.data_ptr()) for a, b in pairs]
    if cache is not None and cache.get("key") == key:
        table, n, first, ws = cache["table"], cache["n"], cache["blocks"], cache["ws"]
    else:
        blk, ents, first = query("onda_multi_tensor_block"), [], 0
        for a, b in pairs:
            assert a.numel() == b.numel() and a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
            ents.append(_lib.OndaSqdiffEntry(a.data_ptr(), b.data_ptr(), a.numel(), first))
            first += -(-a.numel() // blk)
        dev = pairs[0][0].device
        table, n = _table(ents, _lib.OndaSqdiffEntry, dev), len(ents)
        ws = torch.empty(query("onda_sqdiff_multi_ws", first), dtype=torch.float32, device=dev)
        if cache is not None:
            cache.update(key=key, table=table, n=n, blocks=first, ws=ws)
    result = torch.empty((), dtype=torch.float32, device=ws.device)
    call("onda_sqdiff_multi", _p(table), n, float(half_lambda), first, _p(ws), _p(result), _stream())
    return result


def ema_multi(items, cache=None):
    """items: list of (k, q, keep, blend): k = k*keep + q*blend, one launch.  `cache` (a dict the caller keeps next to a
    FIXED list of tensors): the device table is rebuilt only when an address or a factor changed -- at the end of a step
    nothing is queued behind the optimizer launch, so the ~1.5 ms of host work that 320 table entries cost were 1.5 ms of
    idle device per step (tools/trace_gaps.py)."""
    key = [(k.data_ptr(), q.data_ptr(), keep, blend) for k, q, keep, blend in items]
    if cache is not None and cache.get("key") == key:
        table, n, first = cache["table"], cache["n"], cache["blocks"]
    else:
        blk, ents, first = query("onda_multi_tensor_block"), [], 0
        for k, q, keep, blend in items:
            ents.append(_lib.OndaEmaEntry(k.data_ptr(), q.data_ptr(), k.numel(), float(keep), float(blend), first))
            first += -(-k.numel() // blk)
        table, n = _table(ents, _lib.OndaEmaEntry, items[0][0].device), len(ents)
        if cache is not None:
            cache.update(key=key, table=table, n=n, blocks=first)
    call("onda_ema_multi", _p(table), n, first, _stream())
    torch.autograd.graph.increment_version([k for k, *_ in items])


def swap_multi(pairs, cache=None):
    """pairs: list of (a, b): the contents of a and b change places, bit for bit, one launch for all tensors
    (onda_swap_multi; float32 and int64 alike -- the words move as integers).  `cache` (a dict the caller keeps next to a
    FIXED list of tensors): the device table is rebuilt only when an address, a size or a dtype changed.  The kernel's contract
    is checked whenever the table is built: per pair the same dtype, numel and device, contiguous, element size 4 or 8, and
    no address range twice in the table."""
    if not pairs:
        return
    # (size and dtype belong to the key: a tensor reallocated at a kept address goes through the checks again)
    key = [(a.data_ptr(), b.data_ptr(), a.numel(), b.numel(), a.dtype, b.dtype) for a, b in pairs]
    if cache is not None and cache.get("key") == key:
        table, n, first = cache["table"], cache["n"], cache["blocks"]
    else:
        found, spans = [], []
        dev = pairs[0][0].device
        for a, b in pairs:
            if a.dtype != b.dtype or a.numel() != b.numel():
                raise ValueError(f"swap_multi: a pair of {a.dtype}[{a.numel()}] and {b.dtype}[{b.numel()}]")
            if a.element_size() not in (4, 8) or not (a.is_contiguous() and b.is_contiguous()):
                raise ValueError("swap_multi: contiguous tensors of 4- or 8-byte elements only")
            if a.device != dev or b.device != dev:
                raise ValueError("swap_multi: every tensor of a table on one device")
            words = a.numel() * a.element_size() // 4
            if words == 0:
                continue
            spans += [(a.data_ptr(), a.data_ptr() + 4 * words), (b.data_ptr(), b.data_ptr() + 4 * words)]
            found.append((a.data_ptr(), b.data_ptr(), words))
        spans.sort()
        for (_, end), (start, _) in zip(spans, spans[1:]):
            if start < end:
                raise ValueError("swap_multi: an address range appears twice in the table")
        if dev.type != "cuda":
            raise ValueError("swap_multi: device tensors only (the library has no CPU path)")
        blk, ents, first = query("onda_multi_tensor_block"), [], 0
        for pa, pb, words in found:
            ents.append(_lib.OndaSwapEntry(pa, pb, words, first))
            first += -(-words // blk)
        table, n = (_table(ents, _lib.OndaSwapEntry, dev), len(ents)) if ents else (None, 0)
        if cache is not None:
            cache.update(key=key, table=table, n=n, blocks=first)
    if n:
        call("onda_swap_multi", _p(table), n, first, _stream())
    # HipBatchNorm2d.folded() and the bound caches key on _version
    torch.autograd.graph.increment_version([t for pair in pairs for t in pair])
