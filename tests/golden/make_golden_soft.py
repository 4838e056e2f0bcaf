#!/usr/bin/env python3
"""Generate G29 / G30: the SOFT_LABELS branch of the target loss, by IMPORTING the reference on CPU (same shims and helpers
as make_golden.py; run in the build container only):

    python tests/golden/make_golden_soft.py          # writes g29_soft_losses.npz, g30_step_soft.npz

G29 holds, for the small cases of tests/soft_loss_fp64.py (stored; `pole` as the two positions that turn `positive` into it)
and one head-size case (seeded, gradients as digests), the value and gradient of `loss_calc(soft=True)` (the step's path: the
target truncated by `.long()`), `cross_entropy_2d(soft=True)` (not truncated), `rce(soft=True)`, and of the yml-weighted
total 0.1 * CE + 1.0 * RCE + 0.1 * MRKLD as prototypes.py:305-328 adds it up, with and without the CE term (RCE_ALPHA = 0:
the reference does not compute it).  G30 is G17's step recipe (G7's dynamic branch, same seeds, same mask draws) with
SOFT_LABELS: True and RCE_BETA = G30_RCE_BETA.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (sets up the reference's import path and shims)
import make_golden_regularisers as mr  # noqa: E402  (G17's step recipe and its update distance)
from make_golden import digest, save  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import soft_loss_fp64 as sl  # noqa: E402  (the cases, shared with the tests)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from framework.domain_adaptation.methods.prototypes import regular_loss  # noqa: E402
from framework.utils.func import loss_calc  # noqa: E402
from framework.utils.loss import cross_entropy_2d, rce  # noqa: E402

# RCE_BETA of G30.  At the yml weight (1) the step-0 update of the soft run is 0.0011 (relative L2 over the state digests)
# away from the hard-label run's: a soft path that silently ran the hard loss would pass the step test's 0.02.  The soft RCE's
# gradient grows with the weight: 100 gives 0.107, 300 gives G30_RATIO, >= 10x the bound.
G30_RCE_BETA = sl.G30_RCE_BETA
G30_RATIO = 0.3057  # printed by g30(); 0.3763 against G7-dynamic (the yml weights)
W_CE, W_RCE, W_REG = sl.W_CE, sl.W_RCE, sl.W_REG


def reference_terms(logits, soft):
    """Values and gradients of the reference's own functions."""
    def grad_of(fn):
        x = logits.clone().requires_grad_(True)
        v = fn(x)
        return v.detach(), torch.autograd.grad(v, x)[0]

    lc, g_lc = grad_of(lambda x: loss_calc(x, soft, "cpu", soft=True))
    ce, g_ce = grad_of(lambda x: cross_entropy_2d(x, soft, soft=True))
    rc, g_rc = grad_of(lambda x: rce(x, soft, "cpu", soft=True))
    # prototypes.py:305-328 with soft_labels, MRKLD; then the same with RCE_ALPHA = 0
    total, g_total = grad_of(lambda x: W_CE * loss_calc(x, soft, "cpu", soft=True) + W_RCE * rce(x, soft, "cpu", soft=True)
                             + W_REG * regular_loss("MRKLD", x))
    noce, g_noce = grad_of(lambda x: W_RCE * rce(x, soft, "cpu", soft=True) + W_REG * regular_loss("MRKLD", x))
    return dict(lc=lc, ce=ce, rce=rc, total=total, noce=noce, grad_lc=g_lc, grad_ce=g_ce, grad_rce=g_rc, grad_total=g_total,
                grad_noce=g_noce)


def nonzero_count(g):
    """Entries of a gradient that are not zero (a NaN or an inf is not zero)."""
    return int((g != 0).sum())


def g29():
    res = {"weights": np.array([W_CE, W_RCE, W_REG]), "head_seed": np.array(sl.HEAD_SEED), "head_shape": np.array(sl.HEAD_SHAPE)}
    cases = sl.small_cases()
    for case, (logits, soft, tc0_poles) in cases.items():
        r = reference_terms(logits, soft)
        if case == "pole":  # `positive` with two logits replaced: the positions, and the value they hold
            where = (logits != cases["positive"][0]).nonzero()
            assert where.shape[0] == 2 and torch.equal(soft, cases["positive"][1])
            res["pole_where"], res["pole_value"] = where, logits[tuple(where.t())]
        else:
            res[f"{case}_logits"], res[f"{case}_soft"] = logits, soft
        for k, v in r.items():
            res[f"{case}_{k}"] = v
        # the truncated target is 1 at the exact one-hots only: that many entries of the CE gradient are not zero
        n = nonzero_count(r["grad_lc"])
        assert n == int((soft == 1.0).sum()) + tc0_poles and n >= 1, (case, n)
        res[f"{case}_grad_lc_nonzero"] = np.array(n)
        print(case, {k: float(v) for k, v in r.items() if v.dim() == 0}, "CE gradient entries:", n,
              {k: float(v[torch.isfinite(v)].abs().max()) for k, v in r.items() if v.dim() > 0})
    # the branch as the reference has it
    assert torch.isnan(res["mixed_lc"]) and torch.isnan(res["mixed_total"])
    for k in ("grad_lc", "grad_ce", "grad_rce", "grad_total", "grad_noce"):
        assert torch.isfinite(res[f"mixed_{k}"]).all(), k
    assert torch.isfinite(res["positive_lc"]) and res["positive_lc"] != 0 and torch.isfinite(res["positive_total"])
    # the poles: -inf under tc = 1, NaN under tc = 0; CE itself NaN (0 * -inf) -- and nothing of it without the CE term
    g = res["pole_grad_lc"]
    hot, cold = (tuple(int(i) for i in w) for w in res["pole_where"])
    if cases["pole"][1][hot] != 1.0:
        hot, cold = cold, hot
    assert g[hot] == -float("inf") and torch.isnan(g[cold]) and torch.isnan(res["pole_lc"])
    assert torch.isinf(res["pole_ce"]) and not torch.isfinite(res["pole_grad_total"]).all()
    assert torch.isfinite(res["pole_noce"]) and torch.isfinite(res["pole_grad_noce"]).all()
    assert torch.isfinite(res["mixed_noce"]) and torch.isfinite(res["mixed_grad_noce"]).all()
    logits, soft = sl.head_case()
    r = reference_terms(logits, soft)
    for k, v in r.items():
        if v.dim() == 0:
            res[f"head_{k}"] = v
        else:
            res[f"head_{k}"] = digest(v, 4096)
            res[f"head_{k}_absmax"] = v.abs().max()
    n = nonzero_count(r["grad_lc"])
    assert n == int((soft == 1.0).sum()) and n >= 1, n
    res["head_grad_lc_nonzero"] = np.array(n)
    print("head", {k: float(v) for k, v in r.items() if v.dim() == 0}, "CE gradient entries:", n)
    save("g29_soft_losses", **res)


def _step_run(soft_labels, rce_beta):
    """G17's `_step_run` (G7's dynamic recipe) with SOFT_LABELS / RCE_BETA set on the spec."""
    real = mr.make_cfg

    def make_cfg(tmp):
        cfg, spec = real(tmp)
        if soft_labels is not None:
            spec.SOFT_LABELS = soft_labels
        if rce_beta is not None:
            spec.RCE_BETA = rce_beta
        return cfg, spec
    mr.make_cfg = make_cfg
    try:
        return mr._step_run(0, "MRKLD")
    finally:
        mr.make_cfg = real


def g30():
    base, before = _step_run(None, None)  # = G7-dynamic
    g7 = np.load(os.path.join(mg.HERE, "g7_step_dynamic.npz"))
    assert np.allclose(base["state_digest0"], g7["state_digest0"], rtol=1e-5, atol=1e-9), "G7-dynamic did not reproduce"
    hard, _ = _step_run(False, G30_RCE_BETA)  # hard labels, the same weights
    res, _ = _step_run(True, G30_RCE_BETA)
    ratio_hard = mr.update_distance(res, hard, before)
    ratio_g7 = mr.update_distance(res, base, before)
    log = json.loads(str(res["log0_json"]))
    print("g30: RCE_BETA", G30_RCE_BETA, "step-0 update, rel-L2 vs the hard-label run with the same weights", ratio_hard,
          "vs G7-dynamic", ratio_g7, "ce_loss", log["ce_loss"], "rce_loss", log["rce_loss"], "branches", res["branch0"],
          res["branch1"])
    assert ratio_hard >= 10 * 0.02 and ratio_g7 >= 10 * 0.02, (ratio_hard, ratio_g7)
    assert np.isnan(log["ce_loss"]) and np.isfinite(log["rce_loss"])
    res["ratio_vs_hard"] = np.array(ratio_hard)
    res["ratio_vs_g7"] = np.array(ratio_g7)
    save("g30_step_soft", **res)


if __name__ == "__main__":
    for w in sys.argv[1:] or ["g29", "g30"]:
        globals()[w]()
