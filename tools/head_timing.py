"""Timing of the DeepLabV2 'normal' classifier head (ops.SumConvFn: four dilated 3x3 convolutions with bias, summed, to 19 classes
padded to 32) at the workload's feature size, 4 x 65 x 129, for layer6 (2048 input channels) and layer5 (1024), in "f16x2" mode:

  * the TAP-TABLE route (onda_conv2d_taps_fwd_l2: one launch each way over the 36 taps, one accumulator) against
  * the CHAIN route (four onda_conv2d_fwd_l2 launches of the unchanged kernels chained through the residual operand -- the
    baseline: what the head costs without the tap-table entry point),

forward, data gradient (plain, and adding into an existing buffer as ops.GradSink does for layer3's output), the packing of the
weights each route needs after an optimizer step, and forward + backward through ops.SumConvFn; the four weight-gradient launches
and the bias column sum, which both routes share, are timed once.  The limb rows of x and dy are made beforehand (in the model
the producer leaves them behind; either route would pay the same split pass).

    python tools/head_timing.py

Method: 5 warm-up calls of each variant, then 5 rounds that alternate the variants, each sample = 10 calls between two device
events; median, minimum and maximum over a variant's samples (the spread of one session).  Before timing, the two routes' results
are compared at the timed size (relative L2; they differ by rounding only: one weight scale and one accumulator against four)."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from onda_amd import ops

DEV = "cuda:0"
B, H, W, K, PAD = 4, 65, 129, 19, ops.HEAD_PAD
DILS = (6, 12, 18, 24)
GEOMS = tuple((3, d, d) for d in DILS)
CALLS = 10


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1000 / CALLS


def compare(title, variants):
    """variants: {name: callable}; prints microseconds per call"""
    ts = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(5):
        for k, fn in variants.items():
            ts[k].append(sample(fn))
    print(f"{title}: " + ", ".join(f"{k} {statistics.median(v):.1f} us (min {min(v):.1f}, max {max(v):.1f})" for k, v in ts.items()),
          flush=True)
    return {k: statistics.median(v) for k, v in ts.items()}


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def routed(tap, fn):
    def run():
        ops.TAP_CONV = tap
        return fn()
    return run


def level(name, cin):
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(B, H, W, cin, generator=g).to(DEV)
    ws = [(torch.randn(K, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(DEV).requires_grad_(True) for _ in DILS]
    bs = [(0.1 * torch.randn(K, generator=g)).to(DEV).requires_grad_(True) for _ in DILS]
    dy = torch.zeros(B, H, W, PAD, device=DEV)
    dy[..., :K] = torch.randn(B, H, W, K, generator=g).to(DEV)
    ops.limbs_of(x), ops.limbs_of(dy)
    taps, neg = ops.sum_taps(GEOMS), ops.sum_taps(GEOMS, negate=True)
    cache = ops._SumPack(4)
    cache.get(ws, PAD, True)
    shift = cache.bias_sum(bs, PAD)
    for i, w in enumerate(ws):
        cache.each[i].get_fwd(w, PAD), cache.each[i].get_dgrad(w, PAD)
    print(f"--- {name}: {B} x {H} x {W} x {cin} -> {K} classes ({PAD} columns), M = {B * H * W}", flush=True)

    def fwd_taps():
        return ops.conv_taps(x, cache.fwd, taps, PAD, shift=shift)

    def fwd_chain():
        y = None
        for i, (k, d, p) in enumerate(GEOMS):
            y, _, _ = ops.conv_forward(x, cache.each[i].fwd, k, 1, d, p, PAD, out=y, shift=shift if i == 0 else None, residual=y)
        return y

    def dgrad_taps(into=None):
        return ops.conv_taps(dy, cache.dgrad, neg, cin, out=into, residual=into, kind="dgrad")

    def dgrad_chain(into=None):
        for i, (k, d, p) in enumerate(GEOMS):
            got = ops.conv_dgrad(dy, cache.each[i].dgrad, k, 1, d, p, cin, (H, W), accumulate=into)
            into = got if into is None else into
        return into

    with torch.no_grad():
        print(f"agreement of the routes: forward {rel(fwd_taps(), fwd_chain()):.2e}, data gradient {rel(dgrad_taps(), dgrad_chain()):.2e}", flush=True)
        compare("forward", {"taps": fwd_taps, "chain": fwd_chain})
        compare("data gradient", {"taps": dgrad_taps, "chain": dgrad_chain})
        sink = torch.zeros(B, H, W, cin, device=DEV)
        compare("data gradient added into a buffer", {"taps": lambda: dgrad_taps(sink), "chain": lambda: dgrad_chain(sink)})
        del sink
        xl = ops.limbs_of(x)
        compare("weight gradients (4 launches) + bias column sum, either route",
                {"wgrad x4 + colsum": lambda: ([ops.conv_wgrad(x, dy, k, 1, d, p, K, cin, xlimbs=xl) for k, d, p in GEOMS], ops.colsum(dy))})

        def pack_taps():
            ops._SumPack(4).get(ws, PAD, True)

        def pack_chain():
            for w in ws:
                c = ops._PackCache()
                w._onda_scale = None  # (a new weight version: max|w| is taken again, as after an optimizer step)
                c.get_fwd(w, PAD), c.get_dgrad(w, PAD)
        compare("packing the weights, forward + data-gradient form", {"taps": pack_taps, "chain": pack_chain})

    xg = x.detach().requires_grad_(True)
    ops.limbs_of(xg)

    def step(pack):
        def run():
            xg.grad = None
            for t in ws + bs:
                t.grad = None
            ops.SumConvFn.apply(xg, pack, GEOMS, PAD, *ws, *bs).backward(dy)
        return run
    compare("SumConvFn forward + backward", {"taps": routed(True, step(ops._SumPack(4))), "chain": routed(False, step(ops._SumPack(4)))})


if __name__ == "__main__":
    assert ops.CONV_MODE == "f16x2", "the tap-table route exists in the default conv mode only"
    old = ops.TAP_CONV
    level("layer6", 2048)
    level("layer5", 1024)
    ops.TAP_CONV = old
