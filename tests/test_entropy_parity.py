"""GPU: the fused entropy-map kernels (onda_upsample_entropy_fwd / _bwd, csrc/pointwise.hip) through ops.upsample_entropy
against the float64 restatement and the bounds of tests/entropy_fp64.py, and the ADVENT step that runs on them.  Every test
prints its figures before it asserts."""
import pytest
import torch

import entropy_fp64 as E

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _head_pad(x, ld):
    """CPU logits [B,K,h,w] as a device leaf in the model's pixel-major layout, rows of `ld` floats (padding: zeros)."""
    B, K, h, w = x.shape
    pad = torch.zeros(B, h, w, ld)
    pad[..., :K] = x.permute(0, 2, 3, 1)
    return pad.to(DEV).requires_grad_(True)


def _run(case, kind="normal", noncontiguous=False):
    """(map, gradient [B,K,h,w]) of ops.upsample_entropy and its backward under the case's cotangent."""
    from onda_amd import ops
    B, h, w, K, ldl, H, W = case
    x, cot = E.inputs(case, kind)
    pad = _head_pad(x, ldl)
    ent = ops.upsample_entropy(pad[..., :K].permute(0, 3, 1, 2), (H, W))
    assert ent.dtype == torch.float32 and tuple(ent.shape) == (B, K, H, W) and ent.is_contiguous()
    if noncontiguous:  # the gradient reaches backward as a transposed view
        ent.permute(0, 1, 3, 2).backward(cot.to(DEV).permute(0, 1, 3, 2).contiguous())
    else:
        ent.backward(cot.to(DEV))
    assert int((pad.grad[..., K:] != 0).sum()) == 0
    return ent.detach(), pad.grad[..., :K].permute(0, 3, 1, 2)


def _raw_backward(case, kind="normal"):
    """The entry point itself on rows filled with NaN: dlogits f32[B,h,w,ldl] as the kernels leave it."""
    from onda_amd._lib import call, query
    from onda_amd.ops.core import _p, _stream
    B, h, w, K, ldl, H, W = case
    x, cot = E.inputs(case, kind)
    rows = _head_pad(x, ldl).detach()
    dout = cot.to(DEV).contiguous()
    dl = torch.full((B, h, w, ldl), float("nan"), device=DEV)
    ws = torch.full((query("onda_upsample_entropy_bwd_ws", B, w, K, H, W),), float("nan"), device=DEV)
    call("onda_upsample_entropy_bwd", _p(rows), ldl, _p(dout), _p(dl), _p(ws), B, h, w, K, H, W, _stream())
    return dl


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_map_and_gradient_against_fp64(case):
    K = case[3]
    ent, grad = _run(case)
    ref_map, ref_grad = E.reference(case)
    E.check(ent.cpu(), ref_map, "map", f"{E.case_id(case)} map")
    E.check(grad.cpu(), ref_grad, "grad", f"{E.case_id(case)} gradient")
    if case is E.REAL:
        return
    # the entry point on NaN-filled rows: the same bits again (fixed summation order), zeros in the padding columns
    dl = _raw_backward(case)
    assert torch.equal(dl[..., :K].permute(0, 3, 1, 2), grad)
    assert int((dl[..., K:] != 0).sum()) == 0 and bool(torch.isfinite(dl).all())


@pytest.mark.parametrize("kind", ("gap", "equal"))
def test_underflow_and_equal_logits(kind):
    """"gap": a logit gap of 120 in one low-resolution column -- p underflows to 0, the 1e-30 keeps map and gradient finite.
    "equal": every I_k = 1 / K."""
    case = E.CASES[0]
    ent, grad = _run(case, kind)
    ref_map, ref_grad = E.reference(case, kind)
    assert bool(torch.isfinite(ent).all()) and bool(torch.isfinite(grad).all())
    E.check(ent.cpu(), ref_map, "map", f"{kind} map")
    E.check(grad.cpu(), ref_grad, "grad", f"{kind} gradient")
    if kind == "gap":
        assert float(ent[:, 1:, :, 16].abs().max()) == 0.0  # output column 16 = low-resolution column 2: p = 0 exactly
    else:
        print("max |I - 1/K|:", float((ent - 1.0 / case[3]).abs().max()))


def test_two_runs_are_bit_identical_and_a_transposed_gradient_is_taken():
    for case in (E.CASES[1], E.CASES[2]):  # the two-pass route and the fallback route
        a, b = _run(case), _run(case)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        c = _run(case, noncontiguous=True)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_no_gradient_requested_and_guards():
    from onda_amd import ops
    case = E.CASES[0]
    x, _ = E.inputs(case)
    pad = _head_pad(x, 32)
    with torch.no_grad():
        ent = ops.upsample_entropy(pad[..., :19].permute(0, 3, 1, 2), (17, 33))
    assert not ent.requires_grad
    for K in (1, 33):
        rows = torch.zeros(1, 3, 5, 40, device=DEV)
        with pytest.raises(RuntimeError, match="onda_upsample_entropy_fwd"):
            ops.upsample_entropy(rows[..., :K].permute(0, 3, 1, 2), (17, 33))
    from onda_amd._lib import call, query
    from onda_amd.ops.core import _p, _stream
    for K in (1, 33):
        rows, dout = torch.zeros(1, 3, 5, 40, device=DEV), torch.zeros(1, K, 17, 33, device=DEV)
        dl, ws = torch.zeros(1, 3, 5, 40, device=DEV), torch.zeros(max(query("onda_upsample_entropy_bwd_ws", 1, 5, K, 17, 33), 1), device=DEV)
        with pytest.raises(RuntimeError, match="onda_upsample_entropy_bwd"):
            call("onda_upsample_entropy_bwd", _p(rows), 40, _p(dout), _p(dl), _p(ws), 1, 3, 5, K, 17, 33, _stream())


def test_composed_route_is_the_same_function():
    """ops.upsample_entropy_composed (the yardstick of the step test and of tools/entropy_timing.py) against the same fp64."""
    from onda_amd import ops
    case = E.CASES[1]
    B, h, w, K, ldl, H, W = case
    x, cot = E.inputs(case)
    pad = _head_pad(x, ldl)
    ent = ops.upsample_entropy_composed(pad[..., :K].permute(0, 3, 1, 2), (H, W))
    ent.backward(cot.to(DEV))
    ref_map, ref_grad = E.reference(case)
    E.check(ent.detach().cpu(), ref_map, "map", "composed map")
    E.check(pad.grad[..., :K].permute(0, 3, 1, 2).cpu(), ref_grad, "grad", "composed gradient")


# ------------------------------------------------------------------------------------------------ the ADVENT step
@pytest.fixture(params=["f16x2", "f32"])
def conv_mode(request):
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, request.param
    yield request.param
    ops.CONV_MODE = old


def _advent_cfg(tmp_path):
    """hybrid_switch_cfg's model and schedule with the ADVENT block of configs/advent.yml; the adversarial weight is 1 (the
    yml: 0.001) so that the entropy path's gradient is not lost beside the supervised one in what the test compares."""
    from onda_amd.config import hybrid_switch_cfg
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, str(tmp_path), batch_size=2)
    cfg.METHOD.ADAPTATION.NAME = "ADVENT"
    for k, v in (("LAMBDA_SEG_MAIN", 1.0), ("LAMBDA_SEG_AUX", 0.1), ("LAMBDA_ADV_MAIN", 1.0), ("LAMBDA_ADV_AUX", 0.2)):
        spec[k] = v
    cfg.METHOD.ADAPTATION.ADVENT = spec
    return cfg, spec


def _one_step(tmp_path):
    """One advent.step on seeded weights, batches and dropout masks: (log, head-conv gradient before optimizer.step(),
    d_main's first-layer gradient, that weight before and after its Adam step, lr)."""
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.framework.model import deeplabv2
    from onda_amd.synthetic import fill_state_dict, synth_batch
    from oracle import model as omodel
    cfg, spec = _advent_cfg(tmp_path)
    model = get_model(cfg, 19)
    fill_state_dict(model, 1, 3.0)
    torch.manual_seed(77)  # the discriminators' initial weights
    da = get_adapt_method(cfg)(model, cfg, spec)
    torch.manual_seed(123)
    masks = iter([omodel.draw_drop_mask(2) for _ in range(4)])
    deeplabv2.drop_mask_fn = lambda B, C, p, dev: next(masks).to(dev)
    seen = {}
    head = model.layer6.head[1].weight
    first = da.d_main[0].weight
    real_step, real_d_step = da.optimizer.step, da.optimizer_d_main.step

    def step_spy(*a, **k):
        seen["head_grad"] = head.grad.detach().clone()
        return real_step(*a, **k)

    def d_step_spy(*a, **k):
        seen["d_grad"], seen["d_before"] = first.grad.detach().clone(), first.detach().clone()
        return real_d_step(*a, **k)
    da.optimizer.step, da.optimizer_d_main.step = step_spy, d_step_spy
    try:
        da.optimizer.zero_grad()
        da.adjust_learning_rate(0, 6)
        log = da.step(synth_batch(2, 64, 128, seed=100), synth_batch(2, 64, 128, seed=200))
    finally:
        deeplabv2.drop_mask_fn = deeplabv2._default_drop_mask
    torch.cuda.synchronize()
    assert not any(v.requires_grad or v.grad_fn is not None for v in log.values())
    assert all(p.grad is None or float(p.grad.abs().sum()) == 0.0 for p in da.d_main.parameters())  # zeroed after the step
    return ({k: v.item() for k, v in log.items()}, seen["head_grad"].cpu(), seen["d_grad"].cpu(), seen["d_before"].cpu(),
            first.detach().cpu().clone(), spec.LEARNING_RATE_D)


def _rel(a, b):
    return float(((a.double() - b.double()) ** 2).sum().sqrt() / (b.double() ** 2).sum().sqrt())


def test_advent_step_fused_against_composed(tmp_path, monkeypatch, conv_mode):
    """advent.step at 64x128, batch 2, on the fused kernels against the same step with ops.upsample_entropy replaced by the
    composed torch route (UpsampleFn + torch.softmax + the expression, autograd backward).  The class adds no arithmetic of
    its own around the two, so what separates the runs is the entropy path: each route is within BOUNDS of the float64
    restatement, the two of each other within twice that (triangle inequality).  Factor on top: 4 -- the project's margin
    for one more float32 re-association, here everything downstream of the maps that sums them in a data-dependent order or
    amplifies by a modest condition number (the discriminators' convolutions, the head's weight gradient, which contracts
    the map's gradient against features it is uncorrelated with).  So: 8 x BOUNDS["map"][0] = 4e-6 relative on the log
    values that see the maps, 8 x BOUNDS["grad"][0] = 2.4e-5 relative L2 on the head-conv gradient and on d_main's first-layer
    gradient.  Adam's first step is lr * g / (|g| + 1e-8): elements whose gradient is above 1e-3 of the tensor's RMS move by
    lr to within 1 % in both runs; no element can differ by more than two steps."""
    from onda_amd import ops
    fused = _one_step(tmp_path)
    calls = []

    def composed(out, size):
        calls.append(tuple(out.shape))
        return ops.upsample_entropy_composed(out, size)
    monkeypatch.setattr(ops, "upsample_entropy", composed)
    ref = _one_step(tmp_path)
    assert len(calls) == 2  # single-level model: the target map (reused, detached, by the discriminator pass) and the source map
    tol_log, tol_grad = 8 * E.BOUNDS["map"][0], 8 * E.BOUNDS["grad"][0]
    for k in ("Discriminator loss", "Segmentation loss", "Adversarial loss"):
        print(f"[{conv_mode}] {k}: fused {fused[0][k]:.9f}, composed {ref[0][k]:.9f}, rel {abs(fused[0][k] - ref[0][k]) / abs(ref[0][k]):.3e} (bound {tol_log:.1e})")
    print(f"[{conv_mode}] head-conv gradient rel-L2 {_rel(fused[1], ref[1]):.3e}, d_main.0 gradient rel-L2 {_rel(fused[2], ref[2]):.3e} (bound {tol_grad:.1e})")
    lr = fused[5]
    moved = (fused[4] - ref[4]).abs()
    big = ref[2].abs() > 1e-3 * ref[2].pow(2).mean().sqrt()
    ulp = 2.0 ** -23 * float(ref[4].abs().max())
    print(f"[{conv_mode}] d_main.0 weight after Adam: max |diff| {float(moved.max()):.3e} (lr {lr:.1e}), on the decided elements {float(moved[big].max()):.3e}")
    assert set(fused[0]) == {"Discriminator loss", "Segmentation loss", "Adversarial loss"}
    for k in fused[0]:
        assert abs(fused[0][k] - ref[0][k]) <= tol_log * abs(ref[0][k]), k
    assert _rel(fused[1], ref[1]) <= tol_grad
    assert _rel(fused[2], ref[2]) <= tol_grad
    assert torch.equal(fused[3], ref[3])  # the same initial discriminator
    assert float((fused[4] - fused[3]).abs().max()) > 0.5 * lr  # the step was taken
    assert float(moved[big].max()) <= 0.01 * lr + 2 * ulp
    assert float(moved.max()) <= 2 * lr + 2 * ulp


def test_default_step_never_calls_the_entropy_kernels(tmp_path, monkeypatch):
    """The shipped hybrid-switch settings launch what they launched before."""
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.ops import loss as oloss
    from onda_amd.synthetic import fill_state_dict, synth_batch
    seen = []
    real = oloss.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(oloss, "call", spy)
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, str(tmp_path), batch_size=2)
    model = get_model(cfg, 19)
    fill_state_dict(model, 1, 3.0)
    da = get_adapt_method(cfg)(model, cfg, spec)
    da.update_dynamic()
    loader = [synth_batch(2, 64, 128, seed=300)]
    switch_batch_statistics(da.model, False)
    da.calculate_prototypes(loader, save=False)
    switch_batch_statistics(da.model, True)
    da.optimizer.zero_grad()
    da.adjust_learning_rate(0, 6)
    da.step([synth_batch(2, 64, 128, seed=100)], synth_batch(2, 64, 128, seed=200))
    da.update_ema()
    torch.cuda.synchronize()
    assert seen and not [n for n in seen if n.startswith("onda_upsample_entropy")], sorted(set(seen))
