"""fp64 restatement of the EWC anchor penalty -- ``ewc_loss(lambda, static parameters, student parameters)`` with unit Fisher
weights, reference utils/ewc.py:47-54 on prototypes.py:81-91, :334-336 -- and of the SGD step that consumes its gradient, with
the comparators that hold the HIP kernels (onda_sqdiff_multi, onda_sgd_anchor_multi; csrc/loss_proto.hip) to them.  A plain
module like entropy_fp64.py.

Restatement.  pen = (lambda / 2) * sum_i sum((theta0_i - theta_i)^2) in float64 over the float32 inputs; its gradient with
respect to theta is lambda * (theta - theta0).  One anchored step: g' = g0 * grad_scale + lambda * (theta - theta0), formed
ONCE from the parameter the step finds, then `times` sequential torch-SGD updates with that g' (d = g' + wd * p;
b = d on a fresh buffer, else b * momentum + d; p -= lr * b), all in float64.

What float32 does (and the kernels must reproduce bit for bit, tests/test_ewc_reference.py pins it on fixture G20): autograd
leaves g0 + (-2 * (fl32(lambda / 2) * (theta0 - theta))) in .grad -- one rounding each for the difference, the product and
the sum; the factor -2 is exact.

Criteria.  "penalty": |got - ref| / ref of the scalar ("equal" inputs: exactly 0).  "step": relative L2 of the UPDATE
(p_after - p_before) over a case's tensors together, against the float64 update.

BOUNDS are measured, not chosen: the reference's own arithmetic in float32 on the CPU (the imported ``ewc_loss``, whose values
fixture G20 holds; torch's SGD loop on the .grad it leaves) against this restatement over CASES x INPUT_SETS x TIMES, times 4,
rounded to one digit -- the margin upsample_fp64.py, ece_fp64.py and entropy_fp64.py use for one more float32 re-association
(per-workgroup float32 partials and a float64 sum of them here, ATen's own blocked float32 sums per tensor there).
                 CPU floor, worst entry     where                                        bound
  "penalty"      4.60e-8                    3-tensor case (one unaligned), "far"         2e-7 (1.84e-7 rounded)
  "step"         3.13e-5                    3-tensor case, "equal", times 1, fresh       1e-4 (1.25e-4 taken down)
(most of the penalty's floor is the coefficient: fl32(0.15) is 4.0e-8 away from 0.15, for the reference and the kernel alike.
The step's floor is the rounding of p - lr * b at p's magnitude against an update of lr * |g|.)
Measured on the MI355X (tests/test_ewc_parity.py, worst entry): penalty 9.81e-8 (6-tensor case, "normal": one ulp of the float32
result), step 3.13e-5 (the same entry as the CPU floor; the anchored launch is bit-identical to onda_sgd_multi on the gradient
autograd leaves, so its distance from float64 is that kernel's).
"""
import functools
import warnings

import torch

BLK = 4096  # onda_multi_tensor_block(); tests/test_ewc_parity.py asserts the library agrees
LAMBDA = 0.3  # lambda / 2 = 0.15 is not a float32: the rounding of the coefficient is part of what is pinned
MOMENTUM, WD = 0.9, 5e-4
TIMES = (1, 3, 4)

# a case: [(elements, pointer offset in floats), ...] -- every size at which a multi-tensor kernel takes another path: below a
# vector, a ragged tail, exactly one full block (the f32x4 path), one element past it, two blocks and a tail; one entry whose
# tensors start 4 bytes past a 16-byte boundary (a FULL block, so that only the alignment keeps it off the vector path)
CASES = [
    [(1, 0), (3, 0), (BLK, 0), (BLK + 1, 0), (2 * BLK + 5, 0), (1024, 0)],
    [(3, 0), (BLK, 1), (2 * BLK + 5, 0)],
    [(1024, 0)],
]
INPUT_SETS = ("normal", "far", "equal")
BOUNDS = {"penalty": 2e-7, "step": 1e-4}


def case_id(i):
    return "case%d-%dt" % (i, len(CASES[i]))


def runs():
    return [(i, kind) for i in range(len(CASES)) for kind in INPUT_SETS]


# ------------------------------------------------------------------------------------------------- seeded inputs
@functools.lru_cache(maxsize=None)
def inputs(i, kind="normal"):
    """Per tensor of CASES[i]: (theta0, theta, g0, buf, lr) -- float32 CPU tensors, seeded.  "normal": theta0 = randn,
    theta = theta0 + 1e-2 * randn.  "far": theta = 50 + randn, theta0 = -50 + randn (large, nearly equal squares).
    "equal": theta = theta0 (penalty and contribution are exact zeros)."""
    out = []
    for j, (n, _) in enumerate(CASES[i]):
        g = torch.Generator().manual_seed(2000 + 97 * i + j)
        t0, t, g0, buf = (torch.randn(n, generator=g) for _ in range(4))
        if kind == "normal":
            t = t0 + 1e-2 * t
        elif kind == "far":
            t0, t = t0 - 50.0, t + 50.0
        else:
            t = t0.clone()
        out.append((t0, t, 0.1 * g0, 0.1 * buf, (1e-2, 1e-3)[j % 2]))
    return out


# ------------------------------------------------------------------------------------------------- the restatement
def penalty64(lam, pairs):
    """float64 scalar: (lam / 2) * sum over the pairs (theta0, theta) of sum((theta0 - theta)^2)."""
    return (lam / 2) * sum(((a.detach().double().cpu() - b.detach().double().cpu()) ** 2).sum() for a, b in pairs)


def contribution32(lam, theta0, theta):
    """What autograd leaves in .grad for the penalty, in ITS float32 arithmetic (IEEE elementwise ops, no re-association: the
    same bits on any device): -2 * (fl32(lam / 2) * (theta0 - theta))."""
    return -2.0 * (torch.tensor(lam / 2, dtype=torch.float32).to(theta.device) * (theta0 - theta))


def sgd_step64(lam, theta0, theta, g0, buf, lr, times, fresh, grad_scale=1.0):
    """(p, b) in float64 after one anchored step."""
    p, p0, b = theta.double(), theta0.double(), buf.double()
    g = g0.double() * grad_scale + lam * (p - p0)
    for r in range(times):
        d = g + WD * p
        b = d if fresh else b * MOMENTUM + d
        p = p - lr * b
    return p, b


def sgd_step32(g, theta, buf, lr, times, fresh):
    """torch's for-loop SGD in float32 on a gradient `g`, `times` occurrences of the parameter: (p, b)."""
    p = theta.clone().requires_grad_(True)
    p.grad = g.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "parameter group contains duplicate parameters"
        opt = torch.optim.SGD([{"params": [p] * times}], lr=lr, momentum=MOMENTUM, weight_decay=WD, foreach=False)
        if not fresh:
            opt.state[p]["momentum_buffer"] = buf.clone()
        opt.step()
    return p.detach(), opt.state[p]["momentum_buffer"]


@functools.lru_cache(maxsize=None)
def reference(i, kind="normal"):
    """The penalty of a table entry in float64, computed once and shared."""
    return float(penalty64(LAMBDA, [(t0, t) for t0, t, *_ in inputs(i, kind)]))


@functools.lru_cache(maxsize=None)
def step_reference(i, kind, times, fresh):
    """[(p, b) float64 per tensor] after one anchored step of a table entry, computed once and shared."""
    return [sgd_step64(LAMBDA, t0, t, g0, buf, lr, times, fresh) for t0, t, g0, buf, lr in inputs(i, kind)]


# ------------------------------------------------------------------------------------------------- the comparators
def penalty_error(got, ref):
    return abs(float(got) - ref) / ref if ref != 0 else abs(float(got))


def step_error(got_p, i, kind, times, fresh):
    """Relative L2 of the update over the case's tensors: got_p = [p after, ...]."""
    num = den = 0.0
    for gp, (t0, t, *_), (rp, _) in zip(got_p, inputs(i, kind), step_reference(i, kind, times, fresh)):
        num += float(((gp.detach().double().cpu() - t.double()) - (rp - t.double())).pow(2).sum())
        den += float((rp - t.double()).pow(2).sum())
    return (num / den) ** 0.5


def check_penalty(got, i, kind, what):
    err = penalty_error(got, reference(i, kind))
    print(f"{what} {case_id(i)} {kind}: penalty {float(got):.9g} ref {reference(i, kind):.9g} rel {err:.3e} (bound {BOUNDS['penalty']:.1e})")
    if kind == "equal":
        assert float(got) == 0.0, f"{what} {case_id(i)}: theta = theta0 must give exactly 0, got {float(got)}"
    assert err <= BOUNDS["penalty"], f"{what} {case_id(i)} {kind}: relative error {err:.3e} > {BOUNDS['penalty']:.1e}"
    return err


def check_step(got_p, i, kind, times, fresh, what):
    err = step_error(got_p, i, kind, times, fresh)
    print(f"{what} {case_id(i)} {kind} times {times} fresh {fresh}: update rel-L2 {err:.3e} (bound {BOUNDS['step']:.1e})")
    assert err <= BOUNDS["step"], f"{what} {case_id(i)} {kind} times {times} fresh {fresh}: {err:.3e} > {BOUNDS['step']:.1e}"
    return err
