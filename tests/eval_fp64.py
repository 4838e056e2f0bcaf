"""fp64 restatement of evaluate_model's per-batch tail -- interp(x) -> argmax -> fast_hist, and
prob_2_entropy(softmax(interp(x), 1)).mean() (reference eval_UDA.py:47-57, func.py:71-79) -- with the comparator that holds the
fused kernel (onda_upsample_eval, csrc/pointwise.hip) and the composed route (ops.upsample_eval_composed) to it.  A plain module
like entropy_fp64.py, whose seeded logits, map restatement (`map64`) and `case_id` it imports, with the interpolation weights
of upsample_fp64.py (ATen's own float32 index arithmetic, widened to float64).

Restatement per (case, input set): up = einsum('Yy,bkyx,Xx->bkYX') on those weights; class map = its argmax over k; confusion
matrix = rows label in [0, K), columns class (labels >= K ignored); entropy mean = the mean over ALL B*K*H*W elements of
I_k = -p_k log2(p_k + 1e-30) / log2(K), p = float64 softmax over k: every pixel counts, whatever its label.

Criteria.  The entropy mean: |got - ref| <= BOUND * |ref|; a NaN reference (input set "nan") wants a NaN.  The confusion
matrix and the class map are integers: equal or not (the GPU tests take them from the parent's kernels, which evaluate the
same float32 expression, so no pixel is near a tie between the two).

BOUND is measured, not chosen: the reference's own expression in float32 on the CPU (F.interpolate(bilinear,
align_corners=True) -> softmax(1) -> prob_2_entropy -> .mean()) against this restatement over `runs()` (`floors()`;
tests/test_eval_reference.py asserts fp32 ATen stays inside), times 4, rounded to one digit, and not below 2^-23 = 1.19e-7,
the spacing of the float32 the reference returns:
                 CPU floor (worst relative error of the mean)   where                          4 x, one digit   BOUND
  entropy mean   4.17e-7                                        2x19x3x5 -> 17x33 "equal"      1.67e-6 -> 2e-6  2e-6
(the worst entries are the "equal" sets, where every element carries the same rounding of p = 1/K and of its logarithm and the
errors do not average out: 4.2e-7, 2.0e-7, 1.6e-7; the seeded sets sit at 1.3e-7 and below, the real geometry at 2.8e-8.)
Measured on the MI355X (tests/test_eval_parity.py): worst entry 3.58e-7 at 1x24x4x23 -> 9x701 "equal" (the other "equal" sets:
1.8e-7, 1.2e-7, 0 at K = 2 and 32), the seeded sets at 6.9e-8 and below, the real geometry at 2.7e-9: the per-pixel float32
errors average out in the exact integer sum, what stays is what every pixel has in common.
"""
import functools
import math

import torch
import torch.nn.functional as F

import entropy_fp64 as E
import upsample_fp64 as U
from entropy_fp64 import case_id, inputs as entropy_inputs, map64  # noqa: F401

BOUND = 2e-6
SPACING = 2.0 ** -23  # of the float32 the reference returns: BOUND does not go below it

EPS = E.EPS

# B, h, w, K, ldl, H, W
CASES = E.CASES[:5] + [
    (1, 3, 4, 2, 4, 7, 9),            # K = 2, the minimum
    (1, 65, 129, 19, 32, 512, 1024),  # the real geometry, once
]
REAL = CASES[6]
INPUT_SETS = ("normal", "gap", "equal", "nan")  # the real geometry runs "normal" only


def runs():
    """(case, input set) pairs of the table."""
    return [(c, kind) for c in CASES[:6] for kind in INPUT_SETS] + [(REAL, "normal")]


def run_id(v):
    return case_id(v) if isinstance(v, tuple) else v


# ------------------------------------------------------------------------------------------------- seeded inputs
@functools.lru_cache(maxsize=None)
def inputs(case, kind="normal"):
    """(x f32[B,K,h,w], labels u8[B,H,W]).  x: entropy_fp64.inputs for "normal", "gap" (low-resolution column 2 at +60 for
    class 0 and -60 for the others: exp(-120) underflows in float32, the 1e-30 decides) and "equal" (every logit 0.25: the
    mean is 1 / K); "nan": "normal" with one logit NaN, in the middle of image 0.  Labels: seeded, uniform in [0, K) with
    about one in eight set to 255 and five set to values in [K, 255), which count nowhere."""
    B, h, w, K, ldl, H, W = case
    x = entropy_inputs(case, "normal" if kind == "nan" else kind)[0].clone()
    if kind == "nan":
        x[0, K // 2, h // 2, w // 2] = float("nan")
    g = torch.Generator().manual_seed(31 + B * 7 + h * 1000003 + w * 10007 + H * 101 + W + K * 13 + ldl)
    labels = torch.randint(0, K, (B, H, W), generator=g)
    labels[torch.rand(B, H, W, generator=g) < 0.125] = 255
    flat = labels.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:5]
    flat[where] = torch.randint(K, 255, (5,), generator=g)
    return x, labels.to(torch.uint8)


# ------------------------------------------------------------------------------------------------- the restatement
def confusion(labels, cls, K):
    """int64 [K, K]: rows = label in [0, K), columns = class."""
    return U.confusion(labels, cls, K)


def restate(x, labels, mx=None, eps=EPS, divisor=None, per_pixel=False):
    """(class map i64[B,H,W], confusion matrix i64[K,K], entropy mean as a Python float) in float64.  `mx` overrides the
    X-axis weight matrix, `eps` the 1e-30, `divisor` the log2(K); `per_pixel` takes the mean over pixels instead of elements
    (the teeth tests)."""
    B, K = x.shape[:2]
    H, W = labels.shape[1:]
    x64 = x.detach().double().cpu()
    my = U.axis_matrix(x.shape[2], H)
    mx = U.axis_matrix(x.shape[3], W) if mx is None else mx
    up = torch.einsum("Yy,bkyx,Xx->bkYX", my, x64, mx)
    cls = up.argmax(1)
    ent = E.entropy_of(up.softmax(1), K, eps, divisor)
    mean = ent.sum(1).mean() if per_pixel else ent.mean()
    return cls, confusion(labels, cls, K), float(mean)


@functools.lru_cache(maxsize=None)
def reference(case, kind="normal"):
    """(class map, confusion matrix, entropy mean) of a table entry, computed once and shared."""
    return restate(*inputs(case, kind))


# ------------------------------------------------------------------------------------------------- the fp32 ATen leg
def aten(x, labels, eps=EPS, divisor=None):
    """The reference's statements in float32 on the CPU: (class map, confusion matrix, the float32 mean as a Python float)."""
    K = x.shape[1]
    up = F.interpolate(x.detach().float().cpu(), size=tuple(labels.shape[1:]), mode="bilinear", align_corners=True)
    cls = up.argmax(1)
    mean = E.entropy_of(up.softmax(1), K, eps, divisor).mean()
    assert mean.dtype == torch.float32
    return cls, confusion(labels, cls, K), float(mean)


def rel_err(got, ref):
    """|got - ref| / |ref|; 0 when both are NaN, inf when one is."""
    if math.isnan(ref) or math.isnan(got):
        return 0.0 if math.isnan(ref) and math.isnan(got) else float("inf")
    return abs(got - ref) / abs(ref)


def floors():
    """(worst relative error of fp32 ATen's mean over the table, where): what BOUND is 4 x of (and not below 2^-23)."""
    worst, where = 0.0, ""
    for case, kind in runs():
        r = rel_err(aten(*inputs(case, kind))[2], reference(case, kind)[2])
        print(f"{case_id(case)} {kind}: fp32 ATen mean, relative error {r:.3e}")
        if r > worst:
            worst, where = r, f"{case_id(case)} {kind}"
    return worst, where


# ------------------------------------------------------------------------------------------------- the comparator
def check_mean(got, ref, what, factor=1.0):
    """Assert the entropy mean `got` (anything float() takes) against `ref` within factor * BOUND.  Prints the figure first."""
    got, ref = float(got), float(ref)
    r = rel_err(got, ref)
    print(f"{what}: entropy mean {got:.12g}, reference {ref:.12g}, relative error {r:.3e} (bound {factor * BOUND:.2e})")
    assert r <= factor * BOUND, f"{what}: entropy mean {got!r} against {ref!r}: relative error {r:.3e} > {factor * BOUND:.2e}"
    return r


def check_counts(got, ref, what):
    """Integer tensors (confusion matrix, class map): equal everywhere."""
    got, ref = got.detach().cpu().long(), ref.detach().cpu().long()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} against {tuple(ref.shape)}"
    n = int((got != ref).sum())
    print(f"{what}: {n} of {ref.numel()} entries differ")
    assert n == 0, f"{what}: {n} entries differ"


def flagged(fn, *args, **kwargs):
    """True when the check `fn` fails (the teeth tests)."""
    try:
        fn(*args, **kwargs)
    except AssertionError:
        return True
    return False
