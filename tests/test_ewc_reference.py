"""The EWC anchor penalty (MODEL_REGULARIZATION; reference utils/ewc.py:47-54 on prototypes.py:81-91, :334-336), host leg:
the fp64 restatement of tests/ewc_fp64.py against the reference's own values (fixture G20, made by
tests/golden/make_golden_ewc.py), the float32 rounding sequence of its gradient pinned bit for bit, and the plumbing that
needs no GPU."""
import numpy as np
import pytest
import torch

import ewc_fp64 as E


def _split(flat, i):
    return torch.split(flat, [n for n, _ in E.CASES[i]])


@pytest.mark.parametrize("i,kind", E.runs(), ids=lambda v: str(v))
def test_reference_penalty_is_within_bounds_of_the_restatement(golden, i, kind):
    """The imported ewc_loss (float32, as stored) and the same expression evaluated here: both inside BOUNDS -- the bounds are
    4 x the worst of these figures."""
    g = golden("g20_ewc")
    assert float(g["lambda_cases"]) == E.LAMBDA
    E.check_penalty(g[f"{E.case_id(i)}_{kind}_pen"], i, kind, "reference ewc_loss")
    pen = 0
    for t0, t, *_ in E.inputs(i, kind):
        pen = pen + E.LAMBDA / 2 * torch.sum(1 * (t0 - t) ** 2)
    E.check_penalty(pen, i, kind, "fp32 ATen")


@pytest.mark.parametrize("i,kind", [r for r in E.runs() if r[1] != "equal"], ids=lambda v: str(v))
def test_reference_gradient_rounding_sequence(golden, i, kind):
    """The .grad that ewc_loss(...).backward() left on top of g0 equals g0 + (-2 * (fl32(lambda / 2) * (theta0 - theta))) bit
    for bit: the sequence of float32 roundings that onda_sgd_anchor_multi reproduces (tests/test_ewc_parity.py)."""
    g = golden("g20_ewc")
    stored = _split(torch.from_numpy(g[f"{E.case_id(i)}_{kind}_grad"]), i)
    moved = 0
    for have, (t0, t, g0, _, _) in zip(stored, E.inputs(i, kind)):
        want = g0 + E.contribution32(E.LAMBDA, t0, t)
        assert torch.equal(have, want)
        moved += int((want != g0).sum())
        # and it is lambda * (theta - theta0), to float32 accuracy
        exact = g0.double() + E.LAMBDA * (t.double() - t0.double())
        assert float((have.double() - exact).abs().max()) <= 4e-7 * float(exact.abs().max())
    assert moved > 0


def test_equal_inputs_leave_the_gradient_alone():
    for t0, t, g0, _, _ in E.inputs(0, "equal"):
        c = E.contribution32(E.LAMBDA, t0, t)
        assert torch.equal(g0 + c, g0) and not bool(c.bool().any())


@pytest.mark.parametrize("i,kind", E.runs(), ids=lambda v: str(v))
def test_fp32_torch_sgd_is_within_bounds_of_the_restatement(i, kind):
    """torch's own for-loop SGD (float32, CPU) on g0 + contribution: what BOUNDS["step"] is 4 x of."""
    for times in E.TIMES:
        for fresh in (0, 1):
            got = [E.sgd_step32(g0 + E.contribution32(E.LAMBDA, t0, t), t, buf, lr, times, fresh)[0]
                   for t0, t, g0, buf, lr in E.inputs(i, kind)]
            E.check_step(got, i, kind, times, fresh, "torch SGD fp32")


def test_restatement_has_teeth():
    """A step that forgets the anchor term, or replays a gradient re-formed from the moved parameter, is flagged."""
    i, kind, times = 0, "normal", 3
    rows = E.inputs(i, kind)
    no_anchor = [E.sgd_step32(g0, t, buf, lr, times, 0)[0] for t0, t, g0, buf, lr in rows]
    assert E.step_error(no_anchor, i, kind, times, 0) > 10 * E.BOUNDS["step"]
    reformed = []
    for t0, t, g0, buf, lr in E.inputs(i, "far"):
        p, b = t, buf
        for _ in range(times):  # the gradient re-formed per occurrence: NOT what torch's loop does with one .grad
            p, b = E.sgd_step32(g0 + E.contribution32(E.LAMBDA, t0, p), p, b, lr, 1, 0)
        reformed.append(p)
    assert E.step_error(reformed, i, "far", times, 0) > 10 * E.BOUNDS["step"]
    assert E.penalty_error(E.reference(i, kind) * (1 + 1e-6), E.reference(i, kind)) > E.BOUNDS["penalty"]


def test_cases_cover_every_path_of_the_kernels():
    sizes = {n for case in E.CASES for n, _ in case}
    assert {1, 3, E.BLK, E.BLK + 1, 2 * E.BLK + 5, 1024} <= sizes
    assert any(off == 1 and n >= E.BLK for case in E.CASES for n, off in case)
    assert sum(n for case in E.CASES for n, _ in case) < 100_000


def _adapter(tmp_path, lam):
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_adapt_method, get_model
    cfg, spec = hybrid_switch_cfg(128, 64, "cpu", str(tmp_path), batch_size=2)
    if lam is not None:
        spec.MODEL_REGULARIZATION = lam
    return get_adapt_method(cfg)(get_model(cfg, 19), cfg, spec)


def test_constructor_accepts_model_regularization(tmp_path):
    """lambda > 0 no longer raises: the anchors are the static model's parameters, in the student's parameter order."""
    da = _adapter(tmp_path, 1e-4)
    assert callable(da.model_regularization)
    assert da.optimizer.half_lambda == 5e-5
    params, anchors = list(da.model.parameters()), list(da.static_model.parameters())
    assert len(da.optimizer.anchor_of) == len(params) == 217
    assert all(da.optimizer.anchor_of[id(p)] is a for p, a in zip(params, anchors))
    assert not any(a.requires_grad and a.grad is not None for a in anchors)


@pytest.mark.parametrize("lam", [None, 0, -1.0])
def test_unset_lambda_builds_no_anchor_map(tmp_path, lam):
    da = _adapter(tmp_path, lam)
    assert da.model_regularization is None
    assert da.optimizer.anchor_of is None and da.optimizer.half_lambda == 0.0


def test_several_ranks_still_raise(tmp_path, monkeypatch):
    from onda_amd import dist as odist
    monkeypatch.setattr(odist, "is_on", lambda: True)
    with pytest.raises(NotImplementedError, match="grad_scale"):
        _adapter(tmp_path, 1e-4)


def test_golden_step_has_a_visible_penalty(golden):
    """The fixture's lambda puts "model regularization" between 1 % and 100 % of "Total target loss" in step 0, and both
    aliases of the total carry it."""
    import json
    g = golden("g20_ewc")
    for s in (0, 1):
        log = json.loads(str(g[f"log{s}_json"]))
        assert log["sym_loss"] == log["Total target loss"]
        assert 0.01 <= log["model regularization"] / log["Total target loss"] <= 1.0
        parts = 0.1 * log["ce_loss"] + 1.0 * log["rce_loss"] + 0.1 * log["regularization_loss"] + log["model regularization"]
        assert log["Total target loss"] == pytest.approx(parts, rel=1e-5)
    assert float(g["lambda"]) > 0 and np.isfinite(g["state_digest0"]).all()
