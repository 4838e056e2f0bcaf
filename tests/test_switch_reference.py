"""CPU: the standard of tests/switch_np.py against the reference's own Monitor + model_select at four windows (fixture G28),
the conditions that keep every scenario of tests/test_switch_parity.py from being vacuous, the restated pairwise sum against
numpy, and the comparator's teeth."""
import numpy as np
import pytest

import switch_np as S

ALL = S.base_scenarios() + S.varied_scenarios()


# ------------------------------------------------------------------------------------------------ the standard vs G28
@pytest.mark.parametrize("func", S.FUNCS)
@pytest.mark.parametrize("limit", (2, 9, 130, 258))
def test_host_trajectory_is_the_reference_bit_for_bit(golden, limit, func):
    g = golden("g28_switch")
    seq = S.sequence(limit)
    assert np.array_equal(seq, g[f"L{limit}_seq"]) and not np.isnan(seq).any()  # the seeded sequence
    for sign, name in ((1, "pos"), (-1, "neg")):
        tr = S.standard(S.Scenario(limit, func, sign))
        want = {"exp": g[f"L{limit}_exp"], "avg": g[f"L{limit}_avg"], "dev": g[f"L{limit}_{func}_dev"], "confidence": g[f"L{limit}_avg"],
                "current": g[f"L{limit}_{func}_{name}_current"], "current_dev": g[f"L{limit}_{func}_{name}_current_dev"]}
        S.check(tr, want, f"G28 L{limit} {func} {name}")
    if limit >= 9:
        assert np.count_nonzero(g[f"L{limit}_{func}_dev"]) > limit  # the trend is live in what was recorded


def test_the_fixture_is_small():
    import os
    from conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "g28_switch.npz")) < 200 * 1024


# ------------------------------------------------------------------------------------------------ conditions
@pytest.mark.parametrize("sc", ALL, ids=lambda s: s.id)
def test_scenario_is_not_vacuous(sc):
    ok, failed = S.conditions(sc, S.standard(sc))
    assert ok, f"{sc.id}: {failed}"


@pytest.mark.parametrize("use_exp", (False, True))
@pytest.mark.parametrize("sign", (1, -1))
def test_conditions_hold_over_the_whole_grid(sign, use_exp):
    """18 limits x 3 functions x use_exp on / off x both signs of the threshold (a superset of what the GPU file runs)."""
    for L in S.LIMITS:
        for f in S.FUNCS:
            sc = S.Scenario(L, f, sign, use_exp)
            ok, failed = S.conditions(sc, S.standard(sc))
            assert ok, f"{sc.id} sign {sign} use_exp {use_exp}: {failed}"


def test_sequences_have_exact_ties_and_the_stated_length():
    for L in S.LIMITS:
        s = S.sequence(L)
        assert len(s) == S.n_steps(L) == (2 * L + L // 2 + 3 if L <= 258 else L + L // 2 + 3)
        assert np.array_equal(s[::5], np.round(s[::5], 3))
        if L >= 130:
            assert len(np.unique(s)) < len(s)  # at least one exact tie


def test_float32_samples_differ_from_float64_ones():
    sc = S.Scenario(130, "hamming", f32=True, tag="f32")
    assert not np.array_equal(sc.samples(), S.sequence(130))
    assert S.differing(S.standard(sc), S.standard(S.Scenario(130, "hamming")))


# ------------------------------------------------------------------------------------------------ scripted exact cases
@pytest.mark.parametrize("script", (S.SCRIPT_A, S.SCRIPT_B), ids=("A", "B"))
def test_scripted_expectations_are_what_the_host_computes(script):
    seq, want = S.script_expectation(script)
    c = S.SCRIPT_CFG
    S.check(S.host_trajectory(seq, c["limit"], c["exp_const"], c["dev_func"], c["gray"], c["thr"], script["start"]), want, "script")
    lo, hi = c["gray"]
    on_lo = (want["avg"] == lo) & (want["current"] == 0)
    on_hi = (want["avg"] == hi) & (want["current"] == 1)
    at_thr = (want["dev"] == c["thr"]) & (want["current_dev"] == 1)
    at_neg = (want["dev"] == -c["thr"]) & (want["current_dev"] == 0)
    if script is S.SCRIPT_A:  # each edge is met where the strict test's non-strict twin would decide otherwise
        assert on_lo.any() and at_neg.any() and at_thr.any()
    else:
        assert on_hi.any() and at_thr.any() and at_neg.any()
    assert set(want["current"].tolist()) == {0, 1}


# ------------------------------------------------------------------------------------------------ NaN and write-through
@pytest.mark.parametrize("func", S.FUNCS)
def test_nan_scenario_on_the_host(func):
    """The host path gives NaN while a NaN is in the window and recovers once it has left; the machine follows current_dev."""
    seq = S.nan_samples()
    L = S.NAN_LIMIT
    tr = S.host_trajectory(seq, L, S.exp_const(L), func, S.GRAY, S.threshold(L))
    held = np.zeros(len(seq), dtype=bool)
    for i in S.NAN_AT:
        held[i:i + L] = True
    assert S.NAN_AT[0] < L - 1 < S.NAN_AT[1] and np.array_equal(np.isnan(tr["avg"]), held)
    assert not held[-12:].any() and not np.isnan(tr["dev"][-12:]).any() and np.count_nonzero(tr["dev"][-12:]) >= 6
    assert np.array_equal(tr["current"][held], tr["current_dev"][held])
    assert np.isnan(tr["dev"][S.NAN_AT[1]]) and tr["dev"][S.NAN_AT[0]] == 0.0  # (window not full yet: no trend)
    if func == "median":  # the NaN as oldest sample: one level spans it, the other does not -> still NaN
        assert np.isnan(tr["dev"][S.NAN_AT[1] + L - 1])
    assert "avg" in S.differing(tr, tr) and not S.differing(tr, tr, nan=True)  # equal_nan is needed, and enough
    finite = dict(tr, avg=np.where(held, 0.86, tr["avg"]))                    # a device median that stays finite
    assert "avg" in S.differing(finite, tr, nan=True)


def test_writes_change_the_trajectory():
    L = S.WRITE_LIMIT
    args = (S.sequence(L), L, S.exp_const(L), "hamming", S.GRAY, S.threshold(L))
    plain, written = S.host_trajectory(*args), S.host_trajectory(*args, writes=S.WRITES)
    bad = S.differing(written, plain)
    assert bad == ["current_dev"]
    # each write is visible in the step it precedes: that step's trend is insignificant, so the written current_dev survives it
    for step, (cur, cur_dev) in S.WRITES.items():
        assert abs(plain["dev"][step]) <= S.threshold(L)
        assert written["current_dev"][step] == cur_dev != plain["current_dev"][step]


# ------------------------------------------------------------------------------------------------ the restated sum
def _data(n, seed=0):
    r = np.random.RandomState(1000 + seed)
    return 0.865 + 0.075 * r.rand(n + 1)


def test_restated_pairwise_sum_is_numpys_for_every_span():
    """np.sum(taps * w) and np.mean(w) for spans 1 .. 1023, Hamming taps and ones, on both sub-windows."""
    for n in range(1, 1024):
        w = _data(n, n)
        for taps in (np.hamming(n), np.ones(n)):
            for sub in (w[1:], w[:-1]):
                assert S.pairwise_sum(taps, sub) == np.sum(taps * sub), n
        assert S.pairwise_sum(np.ones(n), w[1:]) / n == np.mean(w[1:]), n


@pytest.mark.parametrize("defect", S.DEFECTS)
def test_a_defective_sum_is_flagged(defect):
    """Each defect changes np.sum(taps * w) for some span in 1 .. 1023, and a trajectory that carries the changed level is
    flagged by the comparator."""
    first = None
    for n in list(range(1, 1024)) if defect != "fma" else list(range(1, 200)):
        w = _data(n, n)
        taps = np.hamming(n)
        if S.pairwise_sum(taps, w[1:], defect) != np.sum(taps * w[1:]):
            first = n
            break
    assert first is not None, f"{defect}: equal to numpy on every span"
    print(f"{defect}: first differs at span {first}")
    if defect == "serial":
        assert first >= 8
    if defect == "n2":
        assert first > 128
    # the same defect inside a trajectory: limit = first + 1, "hamming"
    sc = next((s for s in S.base_scenarios() if s.dev_func == "hamming" and s.limit - 1 >= first), None)
    tr = S.standard(sc)
    seq, L = sc.samples(), sc.limit
    taps, total = np.hamming(L - 1), np.sum(np.hamming(L - 1))
    got = {k: v.copy() for k, v in tr.items()}
    changed = 0
    for i in range(L - 1, len(seq)):
        w = seq[i - L + 1:i + 1]
        dev = S.pairwise_sum(taps, w[1:], defect) / total - S.pairwise_sum(taps, w[:-1], defect) / total
        good = S.pairwise_sum(taps, w[1:]) / total - S.pairwise_sum(taps, w[:-1]) / total
        assert good == tr["dev"][i]  # the restatement is the host's trend at every step
        got["dev"][i] = dev
        changed += dev != good
        if changed and i > L + 8:
            break
    assert changed and S.differing(got, tr) == ["dev"]
    assert S.differing(tr, tr) == []


def test_comparator_flags_one_bit_and_one_state():
    sc = S.Scenario(9, "mean")
    tr = S.standard(sc)
    for k in S.FIELDS_F:
        got = {f: v.copy() for f, v in tr.items()}
        got[k][11] = np.nextafter(got[k][11], 1.0)
        assert S.differing(got, tr) == [k]
    for k in S.FIELDS_I:
        got = {f: v.copy() for f, v in tr.items()}
        got[k][-1] ^= 1
        assert S.differing(got, tr) == [k]
    with pytest.raises(AssertionError):
        S.check(got, tr, "probe")
