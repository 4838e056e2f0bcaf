"""Timing of the soft-label target loss (onda_soft_loss_fwd / _bwd) next to the hard-label launches it stands in for
(onda_seg_loss_fwd / _bwd, onda_target_loss_fwd / _bwd) at the head size: 4 x 65 x 129 = 33 540 pixels, K = 19, logits in rows
of 32 floats, the soft map in rows of 19; the yml weights 0.1 / 1.0 / 0.1.

    python tools/soft_loss_timing.py

Method: the entry points are called directly on preallocated buffers (a forward entry is its pixel pass plus its one-thread
finalize).  5 warm-up rounds, then 20 rounds of 50 back-to-back calls each between two events; the median and the minimum of
a round's time / 50, in microseconds -- the launches queue up behind each other, so this is the device's time per call, not
the host's."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from onda_amd._lib import call  # noqa: E402
from onda_amd.ops.core import _p, _stream  # noqa: E402

DEV = "cuda:0"
N, K, LD = 4 * 65 * 129, 19, 32
W = (0.1, 1.0, 0.1)


def timed(fn, warm=5, rounds=20, per=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000 / per)
    return statistics.median(ts), min(ts)


def main():
    g = torch.Generator().manual_seed(7)
    logits = (3.0 * torch.randn(N, LD, generator=g)).to(DEV)
    soft = (2.0 * torch.randn(N, K, generator=g)).softmax(1).to(DEV)
    labels = torch.randint(0, K, (N,), generator=g)
    labels[torch.rand(N, generator=g) < 0.3] = 255
    labels = labels.to(DEV)
    result = torch.empty(8, device=DEV)
    ws = torch.empty(8 * (N // 256 + 1), device=DEV)
    one = torch.ones(1, device=DEV)
    dl = torch.empty(N, LD, device=DEV)
    s = _stream()
    runs = {
        "seg_loss_fwd": lambda: call("onda_seg_loss_fwd", _p(logits), LD, _p(labels), _p(result), _p(ws), N, K, s),
        "seg_loss_bwd": lambda: call("onda_seg_loss_bwd", _p(logits), LD, _p(labels), _p(result), _p(one), *W, _p(dl), N, K, s),
        "target_loss_fwd (MRENT)": lambda: call("onda_target_loss_fwd", _p(logits), LD, _p(labels), 2, *W, 0.0, _p(result), _p(ws),
                                                N, K, s),
        "target_loss_bwd (MRENT)": lambda: call("onda_target_loss_bwd", _p(logits), LD, _p(labels), 2, *W, 0.0, _p(result), _p(one),
                                                _p(dl), N, K, s),
    }
    for name, reg in (("MRKLD", 1), ("MRENT", 2)):
        runs[f"soft_loss_fwd ({name})"] = lambda reg=reg: call("onda_soft_loss_fwd", _p(logits), LD, _p(soft), K, 1, reg, *W,
                                                               _p(result), _p(ws), N, K, s)
        runs[f"soft_loss_bwd ({name})"] = lambda reg=reg: call("onda_soft_loss_bwd", _p(logits), LD, _p(soft), K, 1, reg, *W,
                                                               _p(one), _p(dl), N, K, s)
    runs["seg_loss_fwd"]()  # (the hard-label backward passes read the forward pass' normalisers)
    for name, fn in runs.items():
        if name.startswith("target_loss_bwd"):
            runs["target_loss_fwd (MRENT)"]()
        if name.startswith("seg_loss_bwd"):
            runs["seg_loss_fwd"]()
        med, lo = timed(fn)
        print(f"{name}: median {med:.2f} us (min {lo:.2f}) per call, N = {N}, K = {K}", flush=True)


if __name__ == "__main__":
    main()
