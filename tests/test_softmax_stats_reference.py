"""CPU: the float64 standard and the comparator of tests/softmax_stats_fp64.py -- the standard on rows whose answer is known in
closed form, the inputs against their conditions, float32 ATen inside the bounds that are 4 x its own error, and injected
faults."""
import math

import pytest
import torch

import softmax_stats_fp64 as F

IDS = [f"{F.case_id(c)}-{k}" for c, k in F.runs()]


# ------------------------------------------------------------------------------------------------ the standard
def test_the_table_is_the_stated_one():
    assert [c[0] for c in F.CASES if c[1:] == (19, 32)] == [1, 255, 256, 257, 33540] and 33540 == 131 * 256 + 4 == 4 * 65 * 129
    assert sorted(c[1:] for c in F.CASES if c[0] == 257) == [(2, 2), (19, 19), (19, 24), (19, 32), (32, 32)]
    assert len(F.CASES) == 9 and len(F.runs()) == 54 and F.FLOOR == 2.0 ** -126 * 2.0 ** 24


def test_standard_on_rows_with_a_closed_form():
    for case in ((257, 19, 32), (257, 2, 2), (257, 32, 32)):
        K = case[1]
        p, conf, am = F.reference(case, "equal")
        assert float((p - 1.0 / K).abs().max()) < 1e-16 and abs(conf - 1.0 / K) < 1e-16 and int(am.abs().sum()) == 0
        x = F.inputs(case, "ties")
        p, conf, am = F.reference(case, "ties")
        top = x.max(1, keepdim=True)[0]
        ties = F.tie_counts(case, "ties")
        assert torch.equal((x == top).sum(1), ties) and set(ties.tolist()) <= {2, 3} and int(ties.max()) == (2 if K == 2 else 3)
        rest = torch.where(x == top, torch.zeros(1, dtype=torch.float64), (x.double() - top.double()).exp()).sum(1)
        assert float((p.max(1)[0] - 1.0 / (ties + rest)).abs().max()) < 1e-15    # conf = 1 / (ties + rest)
        assert bool((x[torch.arange(len(x)), am] == top[:, 0]).all())
        assert bool(((x == top).long().cumsum(1)[torch.arange(len(x)), am] == 1).all())  # the FIRST of them
        last = K - 1 - (x == top).flip(1).long().argmax(1)
        assert bool((last != am).all())
    p, conf, _ = F.reference((257, 19, 32), "gap")
    rows = torch.arange(257) % 10 == 0
    assert float((p[rows].max(1)[0] - 1.0).abs().max()) < 1e-15 and float(p[rows].min()) == pytest.approx(math.exp(-120), rel=1e-12)


@pytest.mark.parametrize("case,kind", F.runs(), ids=IDS)
def test_inputs_meet_their_conditions(case, kind):
    N, K, ld = case
    x = F.inputs(case, kind)
    p, conf, am = F.reference(case, kind)
    assert x.dtype == torch.float32 and tuple(x.shape) == (N, K) and not torch.isnan(x).any()
    assert float((p.sum(1) - 1).abs().max()) < 1e-14 and 0 < conf <= 1
    route, eng = F.absolute_route(p), F.engineered(case, kind)
    if kind in F.ENGINEERED_SETS:
        assert bool((route <= eng).all()), "an entry that was not engineered takes the absolute route"
        assert bool(eng.any()) and bool((route & eng).any())
        assert not bool(eng[torch.arange(N), am].any())  # never the maximum
    else:
        assert not bool(route.any()) and not bool(eng.any())
    if kind == "gap":
        assert bool((route == eng).all()) and int(eng.any(1).sum()) == (N + 9) // 10
    if kind == "-inf":
        assert bool((torch.isinf(x) == eng).all()) and bool((p[eng] == 0).all())
    if kind == "huge":
        assert float(x.min()) > 9990
    if kind == "ties":
        assert bool((F.tie_counts(case, kind) >= 2).all())


# ------------------------------------------------------------------------------------------------ the basis of the bounds
@pytest.mark.parametrize("case,kind", F.runs(), ids=IDS)
def test_fp32_aten_stays_inside_the_bounds(case, kind):
    F.check(F.aten(F.inputs(case, kind)), F.reference(case, kind), f"{F.case_id(case)} {kind}")


def test_bounds_are_four_times_the_measured_floors():
    """One-digit rounding of 4 x floor moves a bound by at most 25 %: the band tests/test_entropy_reference.py keeps."""
    worst = F.floors()
    for k in "abc":
        ratio = F.BOUNDS[k] / worst[k][0]
        print(k, f"floor {worst[k][0]:.3e} at {worst[k][1]}, bound {F.BOUNDS[k]:.0e}, ratio {ratio:.2f}")
        assert 3.0 <= ratio <= 4.7


# ------------------------------------------------------------------------------------------------ teeth
def _exact(case, kind):
    p, conf, am = F.reference(case, kind)
    return p.clone(), conf, am.clone()


def test_last_index_on_a_tie_is_flagged():
    case = (257, 19, 24)
    x = F.inputs(case, "ties")
    p, conf, am = _exact(case, "ties")
    assert not F.flagged((p, conf, am), F.reference(case, "ties"))
    last = x.shape[1] - 1 - (x == x.max(1, keepdim=True)[0]).flip(1).long().argmax(1)
    assert F.flagged((p, conf, last), F.reference(case, "ties"))
    one = am.clone()
    one[256] = last[256]  # a single pixel, the last one
    assert F.flagged((p, conf, one), F.reference(case, "ties"))


def test_mean_that_drops_the_last_pixel_is_flagged():
    case = (257, 19, 32)
    for kind in ("normal", "equal"):
        p, conf, am = _exact(case, kind)
        dropped = float(p.max(1)[0][:256].sum() / 257)
        assert F.flagged((p, dropped, am), F.reference(case, kind))
        other_n = float(p.max(1)[0][:256].mean())  # ... and divides by what it summed: only data can tell
        assert F.flagged((p, other_n, am), F.reference(case, kind)) == (kind == "normal")


def test_sum_that_misses_a_class_is_flagged():
    case = (257, 19, 19)
    x = F.inputs(case, "normal").double()
    e = (x - x.max(1, keepdim=True)[0]).exp()
    p = e / e[:, :-1].sum(1, keepdim=True)
    _, conf, am = _exact(case, "normal")
    m = F.measure((p, conf, am), F.reference(case, "normal"))
    assert m["a"] > F.BOUNDS["a"] and m["b"] > F.BOUNDS["b"] and F.flagged((p, conf, am), F.reference(case, "normal"))
    # the same fault in the mean alone (probs not asked for)
    assert F.flagged((None, float(p.max(1)[0].mean()), am), F.reference(case, "normal"))


def test_non_finite_results_are_flagged():
    case = (255, 19, 32)
    p, conf, am = _exact(case, "-inf")
    q = p.clone()
    q[3, 5] = float("nan")
    assert F.flagged((q, conf, am), F.reference(case, "-inf")) and F.flagged((p, float("nan"), am), F.reference(case, "-inf"))
