"""Timing of the fused validation tail (onda_upsample_eval through ops.upsample_eval) against the composed path on the same
device -- the reference's formulation: UpsampleFn + torch.softmax + the entropy expression + .mean(), and the confusion matrix
from onda_upsample_argmax_hist (ops.upsample_eval_composed) -- for 8 frames, K = 19, rows of 32 floats, at 65x129 -> 512x1024
and at 129x257 -> 1024x2048.

    python tools/eval_timing.py

Method: 5 warm-up calls of each path, then 5 rounds that alternate the two paths, 10 calls each between two events; median and
minimum in microseconds over the 50 calls of a path.  Peak memory: torch's allocator peak over one call of a path above what was
allocated before it (the inputs, labels and counters).  The two paths' results are compared first: equal matrices, entropy
means within 4e-6 relative (twice the bound of tests/eval_fp64.py)."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from onda_amd import ops

DEV = "cuda:0"
B, K = 8, 19

def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1000

def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20

for h, w, H, W in ((65, 129, 512, 1024), (129, 257, 1024, 2048)):
    g = torch.Generator().manual_seed(5)
    out = (torch.randn(B, h, w, 32, generator=g) * 3).to(DEV)[..., :K].permute(0, 3, 1, 2)
    labels = torch.randint(0, K, (B, H, W), generator=g).to(torch.uint8).to(DEV)
    hist = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    ent = torch.zeros(2, dtype=torch.int64, device=DEV)

    def fused():
        ops.upsample_eval(out, labels, hist, K, ent)

    def composed():
        return ops.upsample_eval_composed(out, labels, hist, K)

    paths = {"fused": fused, "composed": composed}
    hist.zero_(); ent.zero_(); fused()
    mean_f, hist_f = float(ops.entropy_mean(ent, B, K, H, W)), hist.clone()
    hist.zero_()
    mean_c = float(composed())
    assert torch.equal(hist, hist_f) and abs(mean_f - mean_c) <= 4e-6 * abs(mean_c), (mean_f, mean_c)
    for fn in paths.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in paths}
    for _ in range(5):
        for k, fn in paths.items():
            ts[k] += [event_time(fn) for _ in range(10)]
    med = {k: statistics.median(v) for k, v in ts.items()}
    mem = {k: peak_mib(fn) for k, fn in paths.items()}
    print(f"{h}x{w} -> {H}x{W}, {B} frames: entropy mean fused {mean_f:.9f} composed {mean_c:.9f}; "
          + ", ".join(f"{k} {med[k]:.1f} us (min {min(v):.1f}), peak {mem[k]:.1f} MiB" for k, v in ts.items())
          + f", composed / fused {med['composed'] / med['fused']:.2f}", flush=True)
