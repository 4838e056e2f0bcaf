#!/usr/bin/env python3
"""Generate G28: the reference's ``Monitor`` (framework/utils/monitoring.py) and ``model_select``
(framework/domain_adaptation/methods/prototypes_hybrid_switch.py), IMPORTED and driven as the reference's ``_prior_plan``
drives them, at more windows than G5's one (run in the build container only):

    python tests/golden/make_golden_switch.py          # writes g28_switch.npz

Limits 2, 9, 130, 258 x the three trend functions x a threshold of either sign, on the sequences of tests/switch_np.py (no
NaN).  Per limit: the sequence, ``avg`` and ``exp`` (they do not depend on the trend function); per (limit, function): ``dev``;
per (limit, function, sign): ``current`` and ``current_dev`` (int8).  Inputs and outputs only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("ONDA_REFERENCE", "/root/reference")
sys.path[:0] = [REF, os.path.join(HERE, "_stubs"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from framework.domain_adaptation.methods.prototypes_hybrid_switch import model_select  # noqa: E402
from framework.utils.monitoring import Monitor  # noqa: E402

import switch_np as S  # noqa: E402

G28_LIMITS = (2, 9, 130, 258)


def main():
    out = {}
    for L in G28_LIMITS:
        seq = S.sequence(L)
        out[f"L{L}_seq"] = np.array(seq)
        for func in S.FUNCS:
            for sign, name in ((1, "pos"), (-1, "neg")):
                mon = Monitor(L, S.exp_const(L), func)
                sel = model_select(model_select.static, list(S.GRAY), S.threshold(L, sign))
                avg, exp, dev, cur, cur_dev = [], [], [], [], []
                for v in seq:
                    mon.add({"prior static": float(v)})
                    a, d = mon.avg("prior static"), mon.dev_avg("prior static")
                    sel.evaluate(a, d)
                    avg.append(a); exp.append(mon.exp("prior static")); dev.append(d)
                    cur.append(sel.current); cur_dev.append(sel.current_dev)
                avg, exp, dev = (np.array(x, dtype=np.float64) for x in (avg, exp, dev))
                for key, val in ((f"L{L}_avg", avg), (f"L{L}_exp", exp), (f"L{L}_{func}_dev", dev)):
                    assert key not in out or np.array_equal(out[key], val)
                    out[key] = val
                out[f"L{L}_{func}_{name}_current"] = np.array(cur, dtype=np.int8)
                out[f"L{L}_{func}_{name}_current_dev"] = np.array(cur_dev, dtype=np.int8)
                print(L, func, name, "transitions", int(np.count_nonzero(np.diff(cur))), "dev != 0 at", int(np.count_nonzero(dev)))
    assert not any(np.isnan(v).any() for v in out.values())
    path = os.path.join(HERE, "g28_switch.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
