"""fp64 restatement of ADVENT's entropy map -- prob_2_entropy(softmax(interp(x), 1)), reference func.py:71-74 on
advent_da.py:94-128 -- and of its vector-Jacobian product, with the comparator that holds the HIP kernels
(onda_upsample_entropy_fwd / _bwd, csrc/pointwise.hip) to it.  A plain module like upsample_fp64.py, whose interpolation
weights (ATen's own float32 index arithmetic, widened to float64) and group comparator it imports.

Restatement.  up = einsum('Yy,bkyx,Xx->bkYX') on those weights; p = float64 softmax over k; I_k = -p_k log2(p_k + 1e-30) /
log2(K); the gradient with respect to x under a cotangent c[B,K,H,W] by float64 autograd through exactly that expression.

Criteria (upsample_fp64.measure): (a) relative L2 of the tensor; (b) relative L2 of the worst group -- a pixel's K-vector for
the map; a low-resolution pixel's K-vector, a low-resolution column and a low-resolution row for the gradient -- where a
group whose reference norm is below FLOOR = 0.1 x the tensor's RMS (x sqrt of the group's size) is compared against that floor
instead of its own norm; (c) exact zeros in the padding columns.  Every element is compared, nothing is masked.

BOUNDS are measured, not chosen: the reference's own expression in float32 on the CPU (F.interpolate(bilinear,
align_corners=True) -> softmax(1) -> prob_2_entropy, autograd for the gradient) against this restatement over CASES x
INPUT_SETS (`floors()`; tests/test_entropy_reference.py asserts fp32 ATen stays inside the bounds), times 4, rounded to one
digit -- the margin upsample_fp64.py and ece_fp64.py use: the kernels associate differently from ATen (two separable gather
passes instead of a per-pixel scatter) but have no business being more than a few times worse than float32 itself.
                 CPU floor, worst entry (a / b)      where                              bound (a / b)
  "map"          1.37e-7 / 9.60e-6                   2x3 -> 3x1001 / 3x5 -> 17x33 "gap"  5e-7 (5.5e-7 taken down) / 4e-5
  "grad"         6.53e-7 / 2.83e-6                   2x3 -> 3x1001, both                3e-6 / 1e-5 (1.13e-5 taken down)
(the map's worst group is a pixel whose K-vector of entropies is small against the tensor's RMS -- one class holds nearly all
the probability -- compared against the absolute floor; the real geometry's worst pixel sits at 6.7e-6.)
Measured on the MI355X (tests/test_entropy_parity.py, worst entry, a / b): map 1.50e-7 / 9.60e-6 (the same two entries as the
CPU floors), gradient 4.55e-7 / 2.36e-6 (2x3 -> 3x1001 / the real geometry): the kernels sit at the float32 floor itself.
"""
import functools
import math

import torch
import torch.nn.functional as F

import upsample_fp64 as U

BOUNDS = {"map": (5e-7, 4e-5), "grad": (3e-6, 1e-5)}

EPS = 1e-30

# B, h, w, K, ldl, H, W
CASES = [
    (2, 3, 5, 19, 32, 17, 33),        # integer ratio (8x), 16-byte class loads
    (1, 4, 7, 19, 32, 23, 50),        # non-integer on both axes
    (2, 2, 3, 5, 5, 3, 1001),         # odd ldl: scalar loads; 500x along x: past the two-pass backward, the fallback route
    (1, 5, 4, 32, 32, 33, 29),        # K = 32 = ldl, no padding column
    (1, 4, 23, 24, 24, 9, 701),       # the largest LDS demand of the row pass (68 384 bytes: the 64 KB opt-in), two blocks
    (1, 65, 129, 19, 32, 512, 1024),  # the real geometry, once
]
REAL = CASES[5]
INPUT_SETS = ("normal", "gap", "equal")  # "gap" and "equal" run on CASES[0] only
G19_CASES = [(1, 3, 5, 19, 32, 9, 17), (2, 4, 7, 5, 5, 11, 23)]


def case_id(c):
    return "B%d-%dx%d-K%d-ld%d-%dx%d" % c


def runs():
    """(case, input set) pairs of the table."""
    return [(c, "normal") for c in CASES] + [(CASES[0], "gap"), (CASES[0], "equal")]


# ------------------------------------------------------------------------------------------------- seeded inputs
@functools.lru_cache(maxsize=None)
def inputs(case, kind="normal"):
    """(x f32[B,K,h,w], cotangent f32[B,K,H,W]).  "normal": randn * 3.  "gap": the same with low-resolution column 2 set to
    +60 for class 0 and -60 for the others -- a gap of 120, exp(-120) underflows to 0 in float32 and the 1e-30 decides.
    "equal": every logit 0.25 -- p = 1 / K, every I_k = 1 / K."""
    B, h, w, K, ldl, H, W = case
    g = torch.Generator().manual_seed(19 + B * 7 + h * 1000003 + w * 10007 + H * 101 + W + K * 13 + ldl)
    x = torch.randn(B, K, h, w, generator=g) * 3
    cot = torch.randn(B, K, H, W, generator=g)
    if kind == "gap":
        x[:, :, :, 2] = -60.0
        x[:, 0, :, 2] = 60.0
    elif kind == "equal":
        x = torch.full_like(x, 0.25)
    return x, cot


# ------------------------------------------------------------------------------------------------- the restatement
def entropy_of(p, K, eps=EPS, divisor=None):
    return -(p * torch.log2(p + eps)) / (math.log2(K) if divisor is None else divisor)


def map64(x, H, W, mx=None):
    """float64 [B,K,H,W]; `mx` overrides the X-axis weight matrix [W, w] (the teeth tests drop a tap)."""
    x = x.detach().double().cpu()
    my = U.axis_matrix(x.shape[2], H)
    mx = U.axis_matrix(x.shape[3], W) if mx is None else mx
    return entropy_of(torch.einsum("Yy,bkyx,Xx->bkYX", my, x, mx).softmax(1), x.shape[1])


@functools.lru_cache(maxsize=None)
def reference(case, kind="normal"):
    """(map f64[B,K,H,W], gradient f64[B,K,h,w]) of a table entry, computed once and shared."""
    B, h, w, K, ldl, H, W = case
    x, cot = inputs(case, kind)
    return vjp64(x, cot)


def vjp64(x, cot):
    lo = x.detach().double().cpu().requires_grad_(True)
    ent = entropy_of(U.upsample_autograd(lo, *cot.shape[2:]).softmax(1), x.shape[1])
    ent.backward(cot.double().cpu())
    return ent.detach(), lo.grad


# ------------------------------------------------------------------------------------------------- the fp32 ATen leg
def aten(x, cot, eps=EPS, divisor=None):
    """The reference's expression in float32 on the CPU: (map, gradient)."""
    lo = x.detach().float().cpu().requires_grad_(True)
    p = F.interpolate(lo, size=tuple(cot.shape[2:]), mode="bilinear", align_corners=True).softmax(1)
    ent = entropy_of(p, x.shape[1], eps, divisor)
    ent.backward(cot.float().cpu())
    return ent.detach(), lo.grad


def floors():
    """{quantity: (worst tensor rel-L2, worst group rel-L2, where)} of fp32 ATen over the table: what BOUNDS are 4 x of."""
    worst = {"map": (0.0, 0.0, "", ""), "grad": (0.0, 0.0, "", "")}
    for case, kind in runs():
        x, cot = inputs(case, kind)
        got = aten(x, cot)
        for q, g_, r_ in zip(("map", "grad"), got, reference(case, kind)):
            t, g, _ = U.measure(g_, r_, "up" if q == "map" else "grad")
            a, b, wa, wb = worst[q]
            worst[q] = (max(a, t), max(b, g), f"{case_id(case)} {kind}" if t > a else wa, f"{case_id(case)} {kind}" if g > b else wb)
    return worst


# ------------------------------------------------------------------------------------------------- the comparator
def check(got, ref, quantity, what, exact=()):
    """Assert (a) and (b) against BOUNDS[quantity], finiteness, and every (c) in `exact`: triples (tensor, want, mask) as in
    upsample_fp64.check.  Prints the figures first; returns them."""
    bound_t, bound_g = BOUNDS[quantity]
    finite = bool(torch.isfinite(got).all())
    t, g, where = U.measure(got, ref, "up" if quantity == "map" else "grad")
    print(f"{what}: tensor rel-L2 {t:.3e} (bound {bound_t:.1e}), worst group {g:.3e} at {where} (bound {bound_g:.1e}), finite {finite}")
    assert finite, f"{what}: non-finite values"
    assert t <= bound_t, f"{what}: relative L2 {t:.3e} > {bound_t:.1e} (worst group {where}: {g:.3e})"
    assert g <= bound_g, f"{what}: worst group, {where}: relative L2 {g:.3e} > {bound_g:.1e}"
    for tensor, want, mask in exact:
        n = U.exact_violations(tensor, want, mask)
        assert n == 0, f"{what}: {n} elements differ where the result is exact by structure"
    return t, g


def flagged(got, ref, quantity):
    try:
        check(got, ref, quantity, "probe")
    except AssertionError:
        return True
    return False
