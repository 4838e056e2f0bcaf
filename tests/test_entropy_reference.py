"""CPU: the float64 restatement and the comparator of tests/entropy_fp64.py against the reference's own numbers (fixture
G19), against float32 ATen on the whole shape table, and against injected faults; the torch-only parts of the ADVENT
mirror (func.prob_2_entropy, func.bce_loss, the discriminator, the handler, the drop-in aliases)."""
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import entropy_fp64 as E
import upsample_fp64 as U


# ------------------------------------------------------------------------------------------------ restatement vs G19
@pytest.mark.parametrize("case", E.G19_CASES, ids=E.case_id)
def test_restatement_agrees_with_the_reference(golden, case):
    g, key = golden("g19_entropy"), E.case_id(case)
    x, cot = E.inputs(case)
    assert np.array_equal(x.numpy(), g[key + "_x"]) and np.array_equal(cot.numpy(), g[key + "_c"])  # the seeded inputs
    ent, grad = E.vjp64(x, cot)
    E.check(torch.from_numpy(g[key + "_map"]), ent, "map", f"G19 {key} map")
    E.check(torch.from_numpy(g[key + "_grad"]), grad, "grad", f"G19 {key} gradient")


@pytest.mark.parametrize("case,kind", E.runs(), ids=lambda v: E.case_id(v) if isinstance(v, tuple) else v)
def test_fp32_aten_stays_inside_the_bounds(case, kind):
    """The basis of BOUNDS: the reference's expression in float32 sits at a quarter of them or below."""
    x, cot = E.inputs(case, kind)
    ent, grad = E.aten(x, cot)
    ref_map, ref_grad = E.reference(case, kind)
    E.check(ent, ref_map, "map", f"{E.case_id(case)} {kind} map")
    E.check(grad, ref_grad, "grad", f"{E.case_id(case)} {kind} gradient")


def test_bounds_are_four_times_the_measured_floors():
    """One-digit rounding of 4 x floor moves a bound by at most 25 % up (never taken: both are taken down) or down."""
    worst = E.floors()
    for q in ("map", "grad"):
        for i in range(2):
            ratio = E.BOUNDS[q][i] / worst[q][i]
            print(q, "ab"[i], f"floor {worst[q][i]:.3e} at {worst[q][2 + i]}, bound {E.BOUNDS[q][i]:.1e}, ratio {ratio:.2f}")
            assert 3.0 <= ratio <= 4.7


def test_equal_logits_give_one_over_k():
    case = E.CASES[0]
    ref_map, _ = E.reference(case, "equal")
    assert float((ref_map - 1.0 / case[3]).abs().max()) < 1e-15


# ------------------------------------------------------------------------------------------------ teeth
def test_missing_epsilon_is_flagged():
    """Without the 1e-30 a probability that underflows to 0 in float32 gives 0 * log2(0) = NaN."""
    case = E.CASES[0]
    x, cot = E.inputs(case, "gap")
    ent, grad = E.aten(x, cot, eps=0.0)
    ref_map, ref_grad = E.reference(case, "gap")
    assert E.flagged(ent, ref_map, "map") and E.flagged(grad, ref_grad, "grad")
    ok_map, ok_grad = E.aten(x, cot)
    assert not E.flagged(ok_map, ref_map, "map") and not E.flagged(ok_grad, ref_grad, "grad")


def test_natural_log_divisor_is_flagged():
    case = E.CASES[1]
    x, cot = E.inputs(case)
    ent, grad = E.aten(x, cot, divisor=float(np.log(case[3])))
    ref_map, ref_grad = E.reference(case)
    assert E.flagged(ent, ref_map, "map") and E.flagged(grad, ref_grad, "grad")


def test_jacobian_without_the_sum_term_is_flagged():
    case = E.CASES[1]
    B, h, w, K, ldl, H, W = case
    x, cot = E.inputs(case)
    p = U.upsample(x, H, W).softmax(1)
    q = p + E.EPS
    t = cot.double() * (-(torch.log2(q) + p / (q * np.log(2.0))) / np.log2(K))
    full = U.upsample_grad(p * (t - (p * t).sum(1, keepdim=True)), h, w)
    ref_grad = E.reference(case)[1]
    assert not E.flagged(full, ref_grad, "grad")  # the formula of the kernels, in float64, is the autograd gradient
    assert E.flagged(U.upsample_grad(p * t, h, w), ref_grad, "grad")


def test_dropped_tap_at_the_right_edge_is_flagged():
    """The last output column without its tap on the last low-resolution column: one pixel column of the map."""
    case = E.CASES[1]
    B, h, w, K, ldl, H, W = case
    x, _ = E.inputs(case)
    mx = U.axis_matrix(w, W).clone()
    assert mx[W - 1, w - 1] > 0.5
    mx[W - 1, w - 1] = 0.0
    ref_map = E.reference(case)[0]
    assert not E.flagged(E.map64(x, H, W), ref_map, "map")
    assert E.flagged(E.map64(x, H, W, mx), ref_map, "map")


# ------------------------------------------------------------------------------------------------ the torch-only mirror
def test_prob_2_entropy_is_the_reference_expression(golden):
    from onda_amd.framework.utils.func import prob_2_entropy
    case = E.G19_CASES[0]
    g, key = golden("g19_entropy"), E.case_id(case)
    x = torch.from_numpy(g[key + "_x"])
    p = F.interpolate(x, size=tuple(g[key + "_map"].shape[2:]), mode="bilinear", align_corners=True).softmax(1)
    mine = prob_2_entropy(p)
    assert mine.dtype == torch.float32
    assert torch.equal(mine, -torch.mul(p, torch.log2(p + 1e-30)) / np.log2(p.shape[1]))
    assert torch.allclose(mine, torch.from_numpy(g[key + "_map"]), rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("label", (0, 1))
def test_bce_loss_works_on_a_cpu_tensor(label):
    from onda_amd.framework.utils.func import bce_loss
    y = torch.randn(2, 1, 4, 8, generator=torch.Generator().manual_seed(3), requires_grad=True)
    loss = bce_loss(y, label)
    want = F.binary_cross_entropy_with_logits(y, torch.full((2, 1, 4, 8), float(label)))
    assert loss.device == y.device and torch.equal(loss, want)
    loss.backward()
    assert y.grad is not None and bool(torch.isfinite(y.grad).all())


def test_discriminator_has_the_reference_state_dict():
    from onda_amd.framework.model.discriminator import get_fc_discriminator
    d = get_fc_discriminator(19)
    shapes = {k: tuple(v.shape) for k, v in d.state_dict().items()}
    want = {}
    for i, (cin, cout) in enumerate(((19, 64), (64, 128), (128, 256), (256, 512), (512, 1))):
        want[f"{2 * i}.weight"], want[f"{2 * i}.bias"] = (cout, cin, 4, 4), (cout,)
    assert shapes == want and len(shapes) == 10
    y = d(torch.zeros(1, 19, 64, 128))
    assert tuple(y.shape) == (1, 1, 2, 4)
    acts = [m for m in d if isinstance(m, torch.nn.LeakyReLU)]
    assert len(acts) == 4 and all(m.negative_slope == 0.2 for m in acts)
    assert all(m.stride == (2, 2) and m.padding == (1, 1) for m in d if isinstance(m, torch.nn.Conv2d))


def test_handler_returns_advent():
    from onda_amd.config import Cfg
    from onda_amd.framework.handlers import get_adapt_method
    cls = get_adapt_method(Cfg.from_dict({"METHOD": {"ADAPTATION": {"NAME": "ADVENT"}}}))
    from onda_amd.framework.domain_adaptation.methods.advent_da import advent
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import da_model
    assert cls is advent and issubclass(advent, da_model)
    for name in ("save_model", "models_eval", "models_default_config", "discriminator_grad", "supervised_loss",
                 "adversarial_loss", "discriminator_loss", "step", "train"):
        assert callable(getattr(advent, name))
    assert (advent.source_label, advent.target_label) == (0, 1)
    with pytest.raises(AssertionError):
        get_adapt_method(Cfg.from_dict({"METHOD": {"ADAPTATION": {"NAME": "PROTO_ADVENT"}}}))


def test_dropin_aliases_the_advent_modules():
    import onda_amd.dropin as dropin
    saved = {k: v for k, v in sys.modules.items() if k == "framework" or k.startswith("framework.")}
    try:
        dropin.install()
        from framework.domain_adaptation.methods.advent_da import advent
        from framework.model.discriminator import get_fc_discriminator
        from framework.utils.func import bce_loss, prob_2_entropy  # noqa: F401
        import onda_amd.framework.domain_adaptation.methods.advent_da as mine
        import onda_amd.framework.model.discriminator as mine_d
        assert advent is mine.advent and get_fc_discriminator is mine_d.get_fc_discriminator
    finally:
        for k in [k for k in sys.modules if k == "framework" or k.startswith("framework.")]:
            del sys.modules[k]
        sys.modules.update(saved)
