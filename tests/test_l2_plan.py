"""The pre-split conv's launch plan (csrc/conv_l2.hip l2_plan) pinned to a recorded table: kernel id, tile variant, statistic
rows (plain and with row groups) and live K-step fractions of every forward / data-gradient problem of the timed step, the
activation-stationary cases and the schedule edges, under each environment override.  The host queries need no device (the
library then plans for 256 compute units, the MI355X's count), so the table made by tests/golden/make_l2_plan.py must be
reproduced exactly -- the live fractions, doubles, included."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_l2_plan as plan  # noqa: E402


@pytest.fixture(scope="module")
def table():
    with open(plan.PATH) as fh:
        data = json.load(fh)
    assert data["fields"] == plan.FIELDS
    return data["problems"]


def test_the_table_covers_every_problem_and_setting(table):
    problems = plan.problems()
    assert set(table) == {name for name, _ in problems}
    for name, f in problems:
        want = {s for s, (_env, which, _plain) in plan.SETTINGS.items() if which is None or plan.splits(f)[which]}
        assert set(table[name]) == want, name
    ids = {rec[0] for recs in table.values() for rec in recs.values()}
    assert ids == {0, 1, 2, 3, 4}  # every device kernel is planned for somewhere


@pytest.mark.parametrize("setting", list(plan.SETTINGS))
def test_host_queries_reproduce_the_recorded_plan(table, setting, monkeypatch):
    env, which, plain = plan.SETTINGS[setting]
    for key in plan.OVERRIDES:
        monkeypatch.delenv(key, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    wrong = []
    for name, f in plan.problems():
        if setting not in table[name]:
            continue
        got = plan.record(f, plan.splits(f)[which], plain)
        if got != table[name][setting]:
            wrong.append((name, dict(zip(plan.FIELDS, got)), dict(zip(plan.FIELDS, table[name][setting]))))
    assert not wrong, "%d problems differ, the first: %r" % (len(wrong), wrong[0])
