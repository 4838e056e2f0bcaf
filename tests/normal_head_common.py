"""What the 'normal'-head tests and the generator of fixture G25 share (a plain module, like g14_common.py): the seeded inputs of
the head-alone case, which gradient elements the fixture holds, and the float64 reference of a sum of dilated convolutions
built from conv_fp64 (one filter tap at a time, in float64 -- no tap table, no shared accumulation order with the kernels)."""
import torch

import conv_fp64 as R

DILATIONS = (6, 12, 18, 24)
CLASSES = 19
HEAD_CIN, HEAD_B, HEAD_H, HEAD_W = 64, 2, 27, 34  # fixture G25 (a)
MODEL = "DeepLabv2-Resnet50"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def head_input(B=HEAD_B, cin=HEAD_CIN, H=HEAD_H, W=HEAD_W, seed=2501):
    """NCHW float32."""
    return torch.randn(B, cin, H, W, generator=_gen(seed))


def head_params(cin=HEAD_CIN, classes=CLASSES, seed=2502, n=len(DILATIONS)):
    """([n weights [classes, cin, 3, 3]], [n biases [classes]]): N(0, 0.05) and N(0, 0.1), so that no branch and no bias is
    negligible in the sum."""
    g = _gen(seed + cin)
    ws = [0.05 * torch.randn(classes, cin, 3, 3, generator=g) for _ in range(n)]
    bs = [0.1 * torch.randn(classes, generator=g) for _ in range(n)]
    return ws, bs


def head_dout(B=HEAD_B, classes=CLASSES, H=HEAD_H, W=HEAD_W, seed=2503):
    """NCHW float32 upstream gradient."""
    return torch.randn(B, classes, H, W, generator=_gen(seed))


def sample_index(numel, n):
    return (torch.arange(n, dtype=torch.int64) * numel) // n


def sampled(t, n):
    """The fixture's strided sample of a tensor (whole when it has no more than n elements), flattened."""
    t = t.reshape(-1)
    return t if t.numel() <= n else t[sample_index(t.numel(), n)]


HEAD_SAMPLE = 8192  # fixture (a): dx, the float32 run's output
HEAD_W_SAMPLE = 4096  # ... each weight gradient


def grad_samples(name):
    """Elements of a model parameter's gradient fixture (b) holds.  Primes: the stride of the sample is then no multiple of the
    nine filter taps (with 256 or 1024 samples a 3 x 3 weight of 2^k channels is sampled at tap (0, 0) only -- which is dead,
    gradient exactly 0, for the dilations 12 to 24 at this feature size)."""
    if name == "conv1.weight":
        return 2039
    return 1021 if ".conv2d_list." in name and name.endswith(".weight") else 251


# ------------------------------------------------------------------------------------- float64 reference of the sum
def sum_fwd64(x, weights, biases=None, dilations=DILATIONS):
    """sum_i conv(x, w_i, dilation d_i, padding d_i) (+ sum_i b_i) in float64; x NHWC, weights OIHW.  [B,H,W,classes]."""
    y = None
    for i, (w, d) in enumerate(zip(weights, dilations)):
        t = R.conv_fwd(x, w, 1, d, d, bias=biases[i] if biases is not None else None)
        y = t if y is None else y + t
    return y


def sum_dgrad64(dy, weights, in_hw, dilations=DILATIONS):
    dx = None
    for w, d in zip(weights, dilations):
        t = R.conv_dgrad(dy, w, in_hw, 1, d, d)
        dx = t if dx is None else dx + t
    return dx


def sum_wgrads64(x, dy, dilations=DILATIONS):
    return [R.conv_wgrad(x, dy, 3, 1, d, d) for d in dilations]
