"""The standard, the inputs and the comparator that hold the device-side switch (csrc/switch.hip: switch_step_kernel behind
``DeviceSwitch.step``) to this repository's host path, bit for bit.  A plain module like entropy_fp64.py; used by
tests/test_switch_reference.py (CPU) and tests/test_switch_parity.py (GPU), and by tests/golden/make_golden_switch.py, which
records the reference's own Monitor + model_select on the same sequences (fixture G28).

Standard.  ``host_trajectory``: ``Monitor`` + ``model_select`` driven exactly as ``hybrid_proDA._prior_plan`` drives them --
``add``, then ``exp`` or ``avg`` as the confidence, ``dev_avg`` as the trend, ``evaluate`` -- i.e. the ``ONDA_DEVICE_SWITCH=0``
path.  Per step: exp, avg, dev, the confidence the machine looked at, current, current_dev (plus count and steps, which are
arithmetic).  float64 throughout; nothing here has a tolerance: exp / avg / dev must be ``np.array_equal``, the machine's
state equal.  With a NaN sample the three statistics compare with ``equal_nan`` (the host gives NaN while the NaN is in the
window: np.median, np.sum) and the machine's state still exactly.

Windows.  LIMITS; the trend's span is limit - 1, so they reach the serial branch of the kernel's restated numpy pairwise sum
(spans 1..7), the first blocked span (8), tails of 1 and 7 (spans 9, 15), the last single block (128), the first recursion (129 ->
64 + 65), the sort's 256-thread stride edge (256 / 257 elements), the first second-level recursion (257 -> 128 + 129 -> 64 + 65) and
MAX_WINDOW = 1024.  Limit 1 is left alone: the host's trend there is 0/0 = NaN (an empty np.hamming(0) / np.mean of nothing), the
device gives 0, and no configuration uses a one-sample window -- it is not pinned either way.

Sequences (``sequence``): a cosine through the gray area plus seeded noise, every fifth sample rounded to 3 decimals (exact
ties); exp_const = min(0.5, 4 / L), gray area (0.84, 0.89), threshold +-0.03 / L.  ``conditions`` states what makes a scenario
worth running -- both values of current and of current_dev, all three confidence zones, transitions -- and
test_switch_reference.py asserts it on the standard alone for every scenario the GPU file runs.

``pairwise_sum`` is the literal restatement of the kernel's np_pairwise_sum (numpy's @TYPE@_pairwise_sum on rounded products),
with one switchable defect at a time for the teeth tests.
"""
import functools
import math
import warnings
from fractions import Fraction

import numpy as np

LIMITS = [2, 3, 7, 8, 9, 10, 16, 17, 128, 129, 130, 200, 256, 257, 258, 513, 1023, 1024]
VARIED = [9, 130, 258]  # the limits that also run the variations
FUNCS = ["hamming", "mean", "median"]
GRAY = (0.84, 0.89)
FIELDS_F = ("exp", "avg", "dev", "confidence")
FIELDS_I = ("current", "current_dev", "count", "steps")


def n_steps(L):
    return (2 * L if L <= 258 else L) + L // 2 + 3


@functools.lru_cache(maxsize=None)
def sequence(L):
    n = n_steps(L)
    t = np.arange(n)
    s = 0.865 + 0.075 * np.cos(2 * np.pi * t / n) + 0.003 * np.random.RandomState(L).randn(n)
    s[::5] = np.round(s[::5], 3)
    s.setflags(write=False)
    return s


def exp_const(L):
    return min(0.5, 4.0 / L)


def threshold(L, sign=1):
    return sign * 0.03 / L


class Scenario:
    """One run: window, trend function and the settings of DeviceSwitch / Monitor / model_select."""

    def __init__(self, limit, dev_func, sign=1, use_exp=False, start=0, f32=False, tag="base"):
        self.limit, self.dev_func, self.sign, self.use_exp, self.start, self.f32, self.tag = limit, dev_func, sign, use_exp, start, f32, tag
        self.exp_const, self.gray, self.thr = exp_const(limit), GRAY, threshold(limit, sign)

    @property
    def id(self):
        return f"L{self.limit}-{self.dev_func}-{self.tag}"

    def samples(self):
        """The float64 values the standard is fed (float32 samples: widened back, as the kernel reads them)."""
        s = sequence(self.limit)
        return s.astype(np.float32).astype(np.float64) if self.f32 else s


def base_scenarios():
    return [Scenario(L, f) for L in LIMITS for f in FUNCS]


def varied_scenarios():
    out = []
    for L in VARIED:
        for f in FUNCS:
            out += [Scenario(L, f, use_exp=True, tag="exp"), Scenario(L, f, sign=-1, tag="thr-neg"), Scenario(L, f, sign=0, tag="thr-zero"),
                    Scenario(L, f, start=1, tag="start1"), Scenario(L, f, f32=True, tag="f32")]
    return out


# --------------------------------------------------------------------------------------------------- the standard
def host_trajectory(seq, limit, exp_const, dev_func, gray, thr, start=0, use_exp=False, writes=None, select=None):
    """{field: array over the steps} of this repository's Monitor + model_select, driven as _prior_plan drives them.
    `writes`: {step: (current, current_dev)} assigned to the machine before that step's sample (the write-through test).
    `select`: the model_select to use (the GPU test hands in one whose device_switch hook is set -- then its reads come from
    the device and this is no standard any more; default: a fresh host-side one)."""
    from onda_amd.framework.domain_adaptation.methods.prototypes_hybrid_switch import model_select
    from onda_amd.framework.utils.monitoring import Monitor
    mon = Monitor(limit, exp_const, dev_func)
    sel = model_select(start, list(gray), thr) if select is None else select
    n = len(seq)
    out = {k: np.zeros(n) for k in FIELDS_F}
    out.update({k: np.zeros(n, dtype=np.int64) for k in FIELDS_I})
    key = "prior static"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (np.median of a window that holds NaN)
        for i, v in enumerate(seq):
            if writes and i in writes:
                sel.current, sel.current_dev = writes[i]
            mon.add({key: float(v)})
            confidence = mon.exp(key) if use_exp else mon.avg(key)
            dev = mon.dev_avg(key)
            sel.evaluate(confidence, dev)
            out["exp"][i], out["avg"][i], out["dev"][i], out["confidence"][i] = mon.exp(key), mon.avg(key), dev, confidence
            out["current"][i], out["current_dev"][i] = sel.current, sel.current_dev
            out["count"][i], out["steps"][i] = min(i + 1, limit), i + 1
    return out


@functools.lru_cache(maxsize=None)
def _standard(limit, dev_func, sign, use_exp, start, f32):
    sc = Scenario(limit, dev_func, sign, use_exp, start, f32)
    return host_trajectory(sc.samples(), sc.limit, sc.exp_const, sc.dev_func, sc.gray, sc.thr, sc.start, sc.use_exp)


def standard(sc):
    """The scenario's host trajectory, computed once and shared (do not write into it)."""
    return _standard(sc.limit, sc.dev_func, sc.sign, sc.use_exp, sc.start, sc.f32)


def zones(confidence, gray=GRAY):
    """0 below the gray area, 1 inside (edges included: neither strict test fires), 2 above."""
    return np.where(confidence < gray[0], 0, np.where(confidence > gray[1], 2, 1))


def conditions(sc, tr):
    """What keeps a scenario from being vacuous, on the standard alone: (ok, what failed)."""
    failed = []
    if set(tr["current"].tolist()) != {0, 1}:
        failed.append("current takes one value only")
    if sc.limit >= 3 and set(tr["current_dev"].tolist()) != {0, 1}:
        failed.append("current_dev takes one value only")
    if set(zones(tr["confidence"], sc.gray).tolist()) != {0, 1, 2}:
        failed.append("the confidence misses a zone")
    transitions = int(np.count_nonzero(np.diff(tr["current"])))
    if transitions < (2 if sc.limit <= 258 else 1):
        failed.append(f"{transitions} transitions")
    return not failed, failed


# --------------------------------------------------------------------------------------------------- the comparator
def differing(got, want, nan=False):
    """Names of the fields in which two trajectories differ: floats by np.array_equal on float64 (equal_nan only where the
    scenario holds a NaN sample), the machine's state exactly."""
    bad = []
    for k in FIELDS_F:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        if g.shape != w.shape or not np.array_equal(g, w, equal_nan=nan):
            bad.append(k)
    for k in FIELDS_I:
        if k in got and k in want and not np.array_equal(np.asarray(got[k], dtype=np.int64), np.asarray(want[k], dtype=np.int64)):
            bad.append(k)
    return bad


def check(got, want, what, nan=False):
    bad = differing(got, want, nan)
    for k in bad:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        i = int(np.flatnonzero(~((g == w) | ((g != g) & (w != w) & nan)))[0]) if g.shape == w.shape else -1
        print(f"{what}: {k} first differs at step {i}: got {g[i]!r}, want {w[i]!r}")
    assert not bad, f"{what}: {bad} differ"


# --------------------------------------------------------------------------------------------------- the restated sum
def _fma(a, b, c):
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # exact, then one (correct) rounding


DEFECTS = ("serial", "block4", "n2", "fma")


def pairwise_sum(a, b, defect=None):
    """np.sum(a * b) as csrc/switch.hip's np_pairwise_sum forms it: products rounded one by one, fewer than 8 terms serially,
    up to 128 in 8 running partial sums (+ a serial tail), more by halving at a multiple of 8.  `defect`: "serial" (no
    blocking at all), "block4" (4 partial sums), "n2" (the split not rounded down to a multiple of 8), "fma" (the product
    fused into the add)."""
    a, b = [float(x) for x in a], [float(x) for x in b]
    acc = (lambda r, x, y: _fma(x, y, r)) if defect == "fma" else (lambda r, x, y: r + x * y)
    lanes = 4 if defect == "block4" else 8

    def go(lo, n):
        if n < 8 or defect == "serial":
            res = 0.0
            for i in range(lo, lo + n):
                res = acc(res, a[i], b[i])
            return res
        if n <= 128:
            r = [a[lo + j] * b[lo + j] for j in range(lanes)]
            i = lanes
            while i < n - (n % lanes):
                for j in range(lanes):
                    r[j] = acc(r[j], a[lo + i + j], b[lo + i + j])
                i += lanes
            if lanes == 8:
                res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            else:
                res = (r[0] + r[1]) + (r[2] + r[3])
            for k in range(i, n):
                res = acc(res, a[lo + k], b[lo + k])
            return res
        n2 = n // 2
        if defect != "n2":
            n2 -= n2 % 8
        return go(lo, n2) + go(lo + n2, n - n2)
    return go(0, len(a))


# --------------------------------------------------------------------------------------------------- scripted exact cases
# limit 3, "mean", exp_const 0.5, gray area (0.5, 0.75), threshold 0.25: every sample dyadic, so every statistic is exact and
# the expectations are written by hand.  dev = (w[2] - w[0]) / 2 once the window is full.  Columns: sample, exp, avg, dev,
# current, current_dev.
SCRIPT_CFG = dict(limit=3, exp_const=0.5, dev_func="mean", gray=(0.5, 0.75), thr=0.25)
SCRIPT_A = dict(start=0, rows=[
    (0.5, 0.5, 0.5, 0.0, 0, 0),            # avg == gray_lo exactly: `<` does not fire -> current_dev = 0 (a `<=` would say 1)
    (0.5, 0.5, 0.5, 0.0, 0, 0),
    (0.0, 0.25, 0.5, -0.25, 0, 0),         # dev == -thr exactly: no significant trend, current_dev stays 0; avg on the edge again
    (-0.5, -0.125, 0.0, -0.5, 1, 1),       # a real downward trend, confidence below the area
    (0.5, 0.1875, 0.0, 0.25, 1, 1),        # dev == +thr exactly: current_dev stays 1 (a `>=` would say 0)
    (0.5, 0.34375, 0.5, 0.5, 0, 0),        # upward trend -> current_dev 0; avg == gray_lo -> current = current_dev = 0
    (1.0, 0.671875, 0.5, 0.25, 0, 0),
    (1.0, 0.8359375, 1.0, 0.25, 0, 0),     # above the area
])
SCRIPT_B = dict(start=1, rows=[
    (0.75, 0.75, 0.75, 0.0, 1, 1),         # avg == gray_hi exactly: `>` does not fire -> current_dev = 1 (a `>=` would say 0)
    (0.75, 0.75, 0.75, 0.0, 1, 1),
    (1.25, 1.0, 0.75, 0.25, 1, 1),         # dev == +thr exactly with current_dev = 1: stays 1; avg on the upper edge
    (2.0, 1.5, 1.25, 0.625, 0, 0),
    (0.75, 1.125, 1.25, -0.25, 0, 0),      # dev == -thr exactly with current_dev = 0: stays 0
    (0.75, 0.9375, 0.75, -0.625, 1, 1),    # downward trend -> current_dev 1; avg == gray_hi -> current = current_dev = 1
])


def script_expectation(script):
    rows = np.array(script["rows"], dtype=np.float64)
    n = len(rows)
    return rows[:, 0].copy(), {"exp": rows[:, 1], "avg": rows[:, 2], "dev": rows[:, 3], "confidence": rows[:, 2],
                               "current": rows[:, 4].astype(np.int64), "current_dev": rows[:, 5].astype(np.int64),
                               "count": np.minimum(np.arange(n) + 1, 3), "steps": np.arange(n) + 1}


# --------------------------------------------------------------------------------------------------- NaN and write-through
NAN_LIMIT = 9
NAN_AT = (4, 20)  # one before the window of 9 is full, one after; the sequence goes on until both have left it


def nan_samples():
    s = sequence(NAN_LIMIT).copy()
    s = np.concatenate([s, s[:16]])  # 41 steps: 12 more after the second NaN has left the window
    for i in NAN_AT:
        s[i] = np.nan
    return s


WRITE_LIMIT = 9
# step -> (current, current_dev), assigned before that step's sample.  Both steps have an insignificant trend (3: the window
# is not full; 16: the turning point of the cosine), so the written current_dev survives them; `current` is recomputed by
# every step, so its write shows in the flag between the write and the step (the GPU test reads it there).
WRITES = {3: (1, 1), 16: (0, 0)}
