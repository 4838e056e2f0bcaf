"""fp64 standard, inputs and comparator for softmax_stats_kernel (csrc/loss_proto.hip, ``ops.softmax_stats``): the per-pixel
softmax of the static prior's logits, its argmax and the mean max-probability -- the first link of the static / dynamic switch
chain (that mean is the sample ``DeviceSwitch.step`` is fed).  A plain module like entropy_fp64.py; used by
tests/test_softmax_stats_reference.py (CPU) and tests/test_softmax_stats_parity.py (GPU).

Standard.  probs = float64 softmax of the float32 logits; conf = float64 mean over the pixels of the row maximum of probs;
argmax = the FIRST index of the row's float32 maximum (exact).

Cases.  N in {1, 255, 256, 257, 33 540 = 131 * 256 + 4 = 4 * 65 * 129, the step's} at (K, ld) = (19, 32), and (K, ld) in {(2, 2),
(19, 19), (19, 24), (19, 32), (32, 32)} at N = 257 (not the full product) x INPUT_SETS: "normal" randn * 3; "gap" one class +60, the
rest -60 on a tenth of the rows; "equal" every logit 0.25; "ties" the row maximum repeated bitwise in two or three classes (first
index wins, conf = 1 / (ties + rest)); "huge" 1e4 + randn; "-inf" -inf in some non-maximal classes.

Criteria.  (a) per-element relative error of probs, an entry whose reference is below FLOOR = FLT_MIN * 2^24 compared absolutely
against FLOOR; (b) |sum_k p - 1| per row; (c) relative error of conf; (d) argmax exact.  Only engineered entries take the
absolute route: none in "normal", "equal", "ties", "huge"; the -60 classes of "gap" (exp(-120) = 8e-53) and the -inf entries (0)
in the other two (``absolute_route`` vs ``engineered``; asserted on the standard alone in the CPU file).

BOUNDS are measured, not chosen: float32 ATen on the CPU (``softmax(1)``, ``.max(1)[0].mean()``) against the standard over the same
table (``floors()``), times 4, rounded to one digit; the CPU file asserts float32 ATen stays inside.  The floor is taken on the same
inputs because the error of exp(x - m) grows with |x - m| for ATen as for the kernel (x - m is rounded to float32 first: half an
ulp of a difference of 25 is 1e-6 on the exponent, and both legs commit exactly that rounding).
                 CPU floor (worst entry)                        bound
  (a) probs      1.19e-6  N33540-K19-ld32 "-inf"              5e-6
  (b) row sum    2.30e-7  N33540-K19-ld32 "normal"            9e-7
  (c) conf       4.88e-7  N33540-K19-ld32 "equal"             2e-6
Measured on the MI355X (tests/test_softmax_stats_parity.py, worst entry): (a) 1.26e-6 at N33540-K19-ld32 "normal", (b) 4.74e-7 at
N33540-K19-ld32 "gap", (c) 8.08e-8 at N257-K19-ld32 "-inf"; argmax exact everywhere.  (a) sits at the float32 floor, (b) at twice
it, (c) well below it: the kernel adds its block partials in double.
"""
import functools

import torch

FLOOR = 1.1754943508222875e-38 * 2.0 ** 24  # FLT_MIN * 2^24: above it a float32 probability carries all its 24 bits

BOUNDS = {"a": 5e-6, "b": 9e-7, "c": 2e-6}

NS = (1, 255, 256, 257, 33540)
KLD = ((2, 2), (19, 19), (19, 24), (19, 32), (32, 32))
CASES = [(n, 19, 32) for n in NS] + [(257, k, ld) for k, ld in KLD if (k, ld) != (19, 32)]
STEP = (33540, 19, 32)
INPUT_SETS = ("normal", "gap", "equal", "ties", "huge", "-inf")
ENGINEERED_SETS = ("gap", "-inf")


def case_id(c):
    return "N%d-K%d-ld%d" % c


def runs():
    return [(c, kind) for c in CASES for kind in INPUT_SETS]


# ------------------------------------------------------------------------------------------------- seeded inputs
@functools.lru_cache(maxsize=None)
def _inputs(case, kind):
    N, K, ld = case
    g = torch.Generator().manual_seed(28 + N * 1009 + K * 31 + ld + 7919 * INPUT_SETS.index(kind))
    x = torch.randn(N, K, generator=g) * 3
    eng = torch.zeros(N, K, dtype=torch.bool)   # entries engineered to fall below FLOOR
    ties = torch.ones(N, dtype=torch.int64)     # how often the row maximum occurs
    if kind == "gap":
        rows = torch.arange(N) % 10 == 0
        hot = torch.randint(0, K, (N,), generator=g)
        gap = torch.full((N, K), -60.0)
        gap[torch.arange(N), hot] = 60.0
        x[rows] = gap[rows]
        eng[rows] = gap[rows] < 0
    elif kind == "equal":
        x = torch.full((N, K), 0.25)
        ties[:] = K
    elif kind == "ties":
        # the maximum (lifted clear of the rest) at two or three classes, bit for bit the same float
        top = x.max(1)[0] + 0.5
        for n in range(N):
            k = 2 if K == 2 else 2 + (n % 2)
            idx = torch.randperm(K, generator=g)[:k]
            x[n, idx] = top[n]
            ties[n] = k
    elif kind == "huge":
        x = 1e4 + torch.randn(N, K, generator=g)
    elif kind == "-inf":
        am = x.argmax(1)
        drop = torch.rand(N, K, generator=g) < 0.3
        drop[torch.arange(N), am] = False
        if K > 1:
            drop[0, (int(am[0]) + 1) % K] = True  # at least one, also at N = 1
        x[drop] = float("-inf")
        eng = drop
    return x, eng, ties


def inputs(case, kind="normal"):
    """float32 logits [N, K] (shared: do not write into them)."""
    return _inputs(case, kind)[0]


def engineered(case, kind):
    return _inputs(case, kind)[1]


def tie_counts(case, kind):
    return _inputs(case, kind)[2]


# ------------------------------------------------------------------------------------------------- the standard
def standard(x):
    """(probs f64 [N, K], conf float, argmax i64 [N]) of float32 logits."""
    x = x.detach().float().cpu()
    p = x.double().softmax(1)
    m = x.max(1, keepdim=True)[0]
    first = (x == m).double().argmax(1)  # argmax of a 0 / 1 map: the first 1
    return p, float(p.max(1)[0].mean()), first


@functools.lru_cache(maxsize=None)
def reference(case, kind="normal"):
    return standard(inputs(case, kind))


def absolute_route(ref_probs):
    return ref_probs < FLOOR


# ------------------------------------------------------------------------------------------------- the fp32 ATen leg
def aten(x):
    x = x.detach().float().cpu()
    p = x.softmax(1)
    return p, float(p.max(1)[0].mean()), x.argmax(1)


# ------------------------------------------------------------------------------------------------- the comparator
def measure(got, ref):
    """{a, b, c, d} of (probs or None, conf, argmax or None) against the standard's triple."""
    probs, conf, am = got
    rp, rc, ra = ref
    out = {"a": 0.0, "b": 0.0, "c": abs(float(conf) - rc) / rc if conf == conf else float("inf"), "d": 0}
    if probs is not None:
        p = probs.detach().double().cpu()
        err = (p - rp).abs() / rp.clamp_min(FLOOR)
        err = torch.where(torch.isfinite(p), err, torch.full_like(err, float("inf")))
        out["a"] = float(err.max())
        out["b"] = float((p.sum(1) - 1.0).abs().max())
    if am is not None:
        out["d"] = int((am.detach().cpu().long() != ra).sum())
    return out


def check(got, ref, what, bounds=None):
    bounds = BOUNDS if bounds is None else bounds
    m = measure(got, ref)
    print(f"{what}: probs rel {m['a']:.3e} (bound {bounds['a']:.0e}), row sum {m['b']:.3e} (bound {bounds['b']:.0e}), "
          f"conf rel {m['c']:.3e} (bound {bounds['c']:.0e}), argmax mismatches {m['d']}")
    assert m["a"] <= bounds["a"], f"{what}: (a) probs, relative error {m['a']:.3e} > {bounds['a']:.0e}"
    assert m["b"] <= bounds["b"], f"{what}: (b) |sum p - 1| {m['b']:.3e} > {bounds['b']:.0e}"
    assert m["c"] <= bounds["c"], f"{what}: (c) conf, relative error {m['c']:.3e} > {bounds['c']:.0e}"
    assert m["d"] == 0, f"{what}: (d) {m['d']} argmax entries differ"
    return m


def flagged(got, ref):
    try:
        check(got, ref, "probe")
    except AssertionError:
        return True
    return False


def floors():
    """{criterion: (worst figure of fp32 ATen over the table, where)}: what BOUNDS are 4 x of."""
    worst = {k: (0.0, "") for k in "abc"}
    for case, kind in runs():
        m = measure(aten(inputs(case, kind)), reference(case, kind))
        for k in "abc":
            if m[k] > worst[k][0]:
                worst[k] = (m[k], f"{case_id(case)} {kind}")
    return worst
