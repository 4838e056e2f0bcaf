"""The SOFT_LABELS branch of the target loss, host leg: the float64 restatement of tests/soft_loss_fp64.py reproduces every
case of fixture G29 (tests/golden/make_golden_soft.py, the reference's own loss_calc / cross_entropy_2d / rce / regular_loss
with soft=True), and the C header and the ctypes table declare the two entry points alike.

Rules: values to 1e-5 relative with NaN / +-inf matched exactly; gradients to 1e-5 of their max-norm, non-finite entries
(the `pole` case) matched by position and kind; the CE gradient on its own element by element."""
import os
import re

import numpy as np
import pytest
import torch

import soft_loss_fp64 as sl
from conftest import ROOT, digest


def case_of(g, case):
    """(logits, soft) of a small case of G29; `pole` is `positive` with the stored positions overwritten."""
    if case != "pole":
        return torch.from_numpy(g[f"{case}_logits"]), torch.from_numpy(g[f"{case}_soft"])
    logits = torch.from_numpy(g["positive_logits"]).clone()
    for where, value in zip(g["pole_where"], g["pole_value"]):
        logits[tuple(int(i) for i in where)] = float(value)
    return logits, torch.from_numpy(g["positive_soft"])


# the reference's five (value, gradient) pairs as (key, w_ce, w_rce, w_reg, ce_trunc)
PAIRS = (("lc", 1.0, 0.0, 0.0, True), ("ce", 1.0, 0.0, 0.0, False), ("rce", 0.0, 1.0, 0.0, True),
         ("total", sl.W_CE, sl.W_RCE, sl.W_REG, True), ("noce", 0.0, sl.W_RCE, sl.W_REG, True))


def test_the_shared_cases_are_the_fixtures(golden):
    """tests/soft_loss_fp64.py re-creates what the generator stored (the head-size case exists only that way)."""
    g = golden("g29_soft_losses")
    for case, (logits, soft, _) in sl.small_cases().items():
        ref_logits, ref_soft = case_of(g, case)
        assert torch.equal(logits, ref_logits) and torch.equal(soft, ref_soft), case
        assert torch.allclose(soft.sum(1), torch.ones(()), atol=1e-5)
        assert int((soft == 1.0).sum()) == 6
    assert tuple(g["weights"]) == (sl.W_CE, sl.W_RCE, sl.W_REG)
    assert int(g["head_seed"]) == sl.HEAD_SEED and tuple(int(v) for v in g["head_shape"]) == sl.HEAD_SHAPE


@pytest.mark.parametrize("case", sl.SMALL)
def test_restatement_reproduces_the_reference(golden, case):
    g = golden("g29_soft_losses")
    logits, soft = case_of(g, case)
    for key, w_ce, w_rce, w_reg, trunc in PAIRS:
        total, grad, _ = sl.total_and_grad(logits, soft, w_ce, w_rce, w_reg, "MRKLD", trunc)
        print(case, key, float(total), float(g[f"{case}_{key}"]))
        assert sl.value_close(total, g[f"{case}_{key}"]), (case, key, float(total), float(g[f"{case}_{key}"]))
        ref = torch.from_numpy(g[f"{case}_grad_{key}"])
        if case != "pole":
            assert torch.isfinite(ref).all(), (case, key)
        sl.grad_close(grad, ref, 1e-5, f"{case} grad {key}")
    _, grad, _ = sl.total_and_grad(logits, soft, 1.0, 0.0, 0.0, "MRKLD", True)
    ref = torch.from_numpy(g[f"{case}_grad_lc"])
    sl.ce_grad_close(grad, ref, f"{case} CE gradient")
    assert int((ref != 0).sum()) == int(g[f"{case}_grad_lc_nonzero"]) >= 1


def test_the_three_properties_are_in_the_fixture(golden):
    """What a faithful mirror has to keep, as the reference's own numbers: CE is NaN over ordinary logits while every
    gradient is finite; the step's path truncates the target (as many CE-gradient entries as exact one-hots); the poles give
    -inf under tc = 1 and NaN under tc = 0, and nothing of either without the CE term."""
    g = golden("g29_soft_losses")
    assert np.isnan(g["mixed_lc"]) and np.isnan(g["mixed_total"]) and np.isfinite(g["mixed_rce"])
    assert all(np.isfinite(g[f"mixed_grad_{k}"]).all() for k in ("lc", "ce", "rce", "total", "noce"))
    assert np.isfinite(g["positive_lc"]) and g["positive_lc"] != 0
    assert int(g["mixed_grad_lc_nonzero"]) == 6 and int((g["mixed_grad_ce"] != 0).sum()) > 1000
    glc = g["pole_grad_lc"]
    assert int(np.isnan(glc).sum()) == 1 and int((glc == -np.inf).sum()) == 1 and np.isnan(g["pole_lc"])
    assert np.isfinite(g["pole_noce"]) and np.isfinite(g["pole_grad_noce"]).all()


def test_restatement_reproduces_the_reference_at_head_size(golden):
    g = golden("g29_soft_losses")
    logits, soft = sl.head_case(g["head_seed"], g["head_shape"])
    for key, w_ce, w_rce, w_reg, trunc in PAIRS:
        total, grad, _ = sl.total_and_grad(logits, soft, w_ce, w_rce, w_reg, "MRKLD", trunc)
        assert sl.value_close(total, g[f"head_{key}"]), (key, float(total), float(g[f"head_{key}"]))
        ref, mine = g[f"head_grad_{key}"], digest(grad, 4096)
        scale = float(g[f"head_grad_{key}_absmax"])
        assert abs(grad.abs().max().item() - scale) <= 1e-5 * scale, key
        np.testing.assert_allclose(mine[2:], ref[2:], rtol=0, atol=1e-5 * scale, err_msg=key)
        np.testing.assert_allclose(mine[:2], ref[:2], rtol=0, atol=1e-5 * ref[1], err_msg=key)  # sum, abs-sum
        if key == "lc":
            assert int((grad != 0).sum()) == int(g["head_grad_lc_nonzero"]) >= 1


def _c_arguments(decl):
    return [a for a in decl.split(",") if a.strip()]


def test_header_and_ctypes_table_declare_the_soft_loss_calls():
    from onda_amd import _lib
    header = open(os.path.join(ROOT, "include", "onda_hip.h")).read()
    for name in ("onda_soft_loss_fwd", "onda_soft_loss_bwd"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/onda_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes prototype"
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(_c_arguments(m.group(1))) == 14, name
    assert _lib.SIGNATURES["onda_soft_loss_fwd"][1][3:6] == [_lib.I] * 3  # lds, ce_trunc, regularizer
