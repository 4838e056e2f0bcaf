"""Timing of the fused ECE entry (onda_upsample_ece) against onda_upsample_argmax_hist and a torch restatement of the
reference (interp -> softmax -> max -> index_add table) at the evaluation shape: 65x129 -> 1024x2048, K = 19, rows of 32
floats, 1 and 4 images, random logits and logits of a converged model (25 added to one class: the top bin takes all).

    python tools/ece_timing.py

Method: 5 warm-up calls, then 30 calls (10 for the slow ones) each between two events; median and minimum in microseconds."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from onda_amd import ops

DEV = "cuda:0"

def timed(fn, warm=5, iters=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1000)
    return statistics.median(ts), min(ts)

def torch_ece(out, labels, table, bins):
    up = F.interpolate(out, size=tuple(labels.shape[1:]), mode="bilinear", align_corners=True)
    conf, cls = up.softmax(1).max(1)
    conf, cls, lab = conf.reshape(-1), cls.reshape(-1), labels.reshape(-1).long()
    row = torch.floor_divide(conf, 1.0 / bins).clamp(0, bins - 1).long()
    fix = torch.round(conf.double() * 4294967296.0).long()
    table.index_add_(0, row, torch.stack([fix, (cls == lab).long(), torch.ones_like(row)], 1))

for B in (1, 4):
    for kind in ("random", "contention"):
        g = torch.Generator().manual_seed(5)
        x = torch.randn(B, 65, 129, 32, generator=g) * 3
        if kind == "contention":
            x[..., 7] += 25
        out = x.to(DEV)[..., :19].permute(0, 3, 1, 2)
        labels = torch.randint(0, 19, (B, 1024, 2048), generator=g).to(torch.uint8).to(DEV)
        table = torch.zeros(1001, 3, dtype=torch.int64, device=DEV)
        hist = torch.zeros(19, 19, dtype=torch.int64, device=DEV)
        big = torch.zeros(2049, 3, dtype=torch.int64, device=DEV)
        r = {}
        r["ece"] = timed(lambda: ops.upsample_ece(out, labels, table, 1000))
        r["ece+hist"] = timed(lambda: ops.upsample_ece(out, labels, table, 1000, hist=hist))
        r["ece probs"] = timed(lambda: ops.upsample_ece(out, labels, table, 1000, probs=True))
        r["ece global 2048"] = timed(lambda: ops.upsample_ece(out, labels, big, 2048), iters=10)
        r["argmax_hist"] = timed(lambda: ops.upsample_argmax_hist(out, labels, hist, 19))
        t2 = torch.zeros(1001, 3, dtype=torch.int64, device=DEV)
        r["torch"] = timed(lambda: torch_ece(out.contiguous(), labels, t2, 1000), iters=10)
        top = int(table[999, 2]) / max(int(table[:, 2].sum()), 1)
        print(f"B={B} {kind} top-bin share {top:.3f}: " + ", ".join(f"{k} {v[0]:.1f} us (min {v[1]:.1f})" for k, v in r.items()), flush=True)
