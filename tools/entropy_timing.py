"""Timing of the fused entropy-map entries (onda_upsample_entropy_fwd / _bwd through ops.upsample_entropy) against the composed
path on the same device -- the reference's formulation: UpsampleFn + torch.softmax + the entropy expression, autograd for the
backward pass (ops.upsample_entropy_composed) -- at ADVENT's training shape: 65x129 -> 512x1024, B = 4, K = 19, rows of 32 floats.

    python tools/entropy_timing.py

Method: 5 warm-up calls of each path, then 5 rounds that alternate the two paths, 20 calls each between two events; median and
minimum in microseconds over the 100 calls of a path.  "backward" is autograd's backward of the map under a fixed cotangent
(the forward pass that builds the graph runs outside the events)."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from onda_amd import ops

DEV = "cuda:0"
B, h, w, K, H, W = 4, 65, 129, 19, 512, 1024

def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1000

g = torch.Generator().manual_seed(5)
rows = (torch.randn(B, h, w, 32, generator=g) * 3).to(DEV).requires_grad_(True)
out = rows[..., :K].permute(0, 3, 1, 2)
cot = torch.randn(B, K, H, W, generator=g).to(DEV)
paths = {"fused": ops.upsample_entropy, "composed": ops.upsample_entropy_composed}

def forward(fn):
    with torch.no_grad():
        return event_time(lambda: fn(out, (H, W)))

def backward(fn):
    ent = fn(out, (H, W))
    rows.grad = None
    return event_time(lambda: ent.backward(cot))

for what, one in (("forward", forward), ("backward", backward)):
    ts = {k: [] for k in paths}
    for k, fn in paths.items():
        for _ in range(5):
            one(fn)
    torch.cuda.synchronize()
    for _ in range(5):
        for k, fn in paths.items():
            ts[k] += [one(fn) for _ in range(20)]
    med = {k: statistics.median(v) for k, v in ts.items()}
    print(f"{what}: " + ", ".join(f"{k} {med[k]:.1f} us (min {min(v):.1f})" for k, v in ts.items())
          + f", composed / fused {med['composed'] / med['fused']:.2f}", flush=True)
