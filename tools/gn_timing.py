"""Timing of GroupNorm on a backbone convolution (ops.GNSiteFn: onda_gn_site_fwd / onda_gn_site_bwd) at the training shape,
512x1024 and batch 4, in the default conv mode:

  * the stem site (4 x 256 x 512 x 64 behind the real stem convolution) with its statistics from the conv epilogue's partials and
    from the reduction pass over the conv output (ops.GN_FUSED_STATS on / off), forward and backward;
  * one shortcut site (layer1.0.downsample: 4 x 129 x 257 x 256).  129 x 257 = 33153 rows per image is no multiple of a tile's
    rows, so only the reduction pass is legal there -- as at the other three shortcuts (65 x 129) at this resolution;
  * the ASPP head's GroupNorm (ops.GNConcatFn: onda_gn_fwd / onda_gn_bwd, the same kernels) at its feature size, 4 x 65 x 129:
    the five-branch concat (5 x 256 channels into one 1280-channel buffer, ReLU) and the bottleneck (256 channels, Dropout2d
    multiplier), forward and backward;
  * forward + backward of the DeepLabv2-Resnet50-GN model next to the DeepLabv2-Resnet50 (BatchNorm) model.

    python tools/gn_timing.py

Method: 5 warm-up calls of each variant, then 5 rounds that alternate the variants, 10 calls each between two events (3 per round
for the models); median and minimum over a variant's calls."""
import os, sys, statistics, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from onda_amd import ops
from onda_amd.framework.handlers import get_model
from onda_amd.synthetic import fill_state_dict, synth_batch

DEV = "cuda:0"
B, H, W = 4, 512, 1024


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1000


def compare(title, variants, calls=10, unit=("us", 1.0)):
    """variants: {name: callable returning microseconds}"""
    ts = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(5):
        for k, fn in variants.items():
            ts[k] += [fn() for _ in range(calls)]
    print(f"{title}: " + ", ".join(f"{k} {statistics.median(v) * unit[1]:.1f} {unit[0]} (min {min(v) * unit[1]:.1f})"
                                    for k, v in ts.items()), flush=True)


def site(y, stats, C, relu):
    g = torch.Generator().manual_seed(C)
    gamma, beta = (0.75 + 0.5 * torch.rand(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    dout = torch.randn(y.shape, generator=g).to(DEV)
    yl = y.detach().requires_grad_(True)

    def forward(fused):
        ops.GN_FUSED_STATS = fused
        with torch.no_grad():
            return event_time(lambda: ops.GNSiteFn.apply(y, stats, gamma, beta, relu))

    def backward():
        out = ops.GNSiteFn.apply(yl, stats, gamma, beta, relu)
        yl.grad = None
        return event_time(lambda: out.backward(dout))
    return forward, backward


g = torch.Generator().manual_seed(5)
img = torch.randn(B, 3, H, W, generator=g).to(DEV)
w = (torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5).to(DEV)
with torch.no_grad():
    y, stats = ops.StemConvFn.apply(img, w, ops._PackCache(), True)
assert ops.gn_site_stats(stats, B, y.shape[1] * y.shape[2]) is stats, "the stem's partials are not usable at this shape"
mb = y.numel() * 4 / 1e6
fwd, bwd = site(y, stats, 64, True)
compare(f"stem site forward ({mb:.0f} MB in, {mb:.0f} MB out)", {"epilogue partials": lambda: fwd(True), "reduction pass": lambda: fwd(False)})
compare("stem site backward", {"reduction + apply": bwd})
del y, stats

x = torch.randn(B, 129, 257, 64, generator=g).to(DEV)
w1 = (torch.randn(256, 64, 1, 1, generator=g) * (2.0 / 64) ** 0.5).to(DEV)
with torch.no_grad():
    y, stats = ops.Conv2dFn.apply(x, w1, None, ops._PackCache(), 1, 1, 0, True, None)
assert ops.gn_site_stats(stats, B, 129 * 257) is None
fwd, bwd = site(y, stats, 256, False)
compare(f"shortcut site (layer1, {y.numel() * 4 / 1e6:.0f} MB) forward", {"reduction pass": lambda: fwd(False)})
compare("shortcut site (layer1) backward", {"reduction + apply": bwd})
del y, stats, x
ops.GN_FUSED_STATS = True


def head(n, C, relu, drop):
    """ops.GNConcatFn on n conv outputs of the head's feature size (the input at 1/8: 65 x 129)."""
    g = torch.Generator().manual_seed(n)
    Hf, Wf = (H - 1) // 8 + 1, (W - 1) // 8 + 1
    ys = [torch.randn(B, Hf, Wf, C, generator=g).to(DEV).requires_grad_(True) for _ in range(n)]
    gammas = [(0.75 + 0.5 * torch.rand(C, generator=g)).to(DEV).requires_grad_(True) for _ in range(n)]
    betas = [(0.1 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True) for _ in range(n)]
    chmul = (torch.empty(B, C).bernoulli_(0.9, generator=g) / 0.9).to(DEV) if drop else None
    dcat = torch.randn(B, Hf, Wf, n * C, generator=g).to(DEV)

    def forward():
        with torch.no_grad():
            return event_time(lambda: ops.GNConcatFn.apply(relu, chmul, *ys, *gammas, *betas))

    def backward():
        cat = ops.GNConcatFn.apply(relu, chmul, *ys, *gammas, *betas)
        return event_time(lambda: torch.autograd.grad(cat, ys + gammas + betas, dcat))
    return forward, backward


fwd, bwd = head(5, 256, True, False)  # the ASPP concat: five branches side by side in one 1280-channel buffer
compare(f"head concat (5 x {B} x 65 x 129 x 256) GroupNorm", {"forward": fwd, "backward": bwd})
fwd, bwd = head(1, 256, False, True)  # the bottleneck: one tensor, the Dropout2d multiplier
compare(f"head bottleneck ({B} x 65 x 129 x 256, multiplier) GroupNorm", {"forward": fwd, "backward": bwd})


def model(name):
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NAME=name, CLASSIFIER="ProDA", LOAD=None, MULTI_LEVEL=False),
                                OTHERS=types.SimpleNamespace(DEVICE=DEV))
    m = get_model(cfg, 19)
    fill_state_dict(m, 1, 3.0)
    return m.train()


batch = synth_batch(B, H, W)
image, label = batch["image"].to(DEV), batch["label_res"].to(DEV)


def step(m):
    def run():
        m.zero_grad(set_to_none=True)
        _, o = m(image)
        ops.seg_losses(o["out"], label, 1.0, 0.0, 0.0)[0].backward()
    return lambda: event_time(run)


models = {"GN": model("DeepLabv2-Resnet50-GN"), "BatchNorm": model("DeepLabv2-Resnet50")}
compare("model forward + backward", {k: step(m) for k, m in models.items()}, calls=3, unit=("ms", 1e-3))
gn_step = step(models["GN"])


def routed(fused):
    def run():
        ops.GN_FUSED_STATS = fused
        return gn_step()
    return run


compare("GN model forward + backward by the stem's statistics route", {"epilogue partials": routed(True), "reduction pass": routed(False)},
        calls=3, unit=("ms", 1e-3))
