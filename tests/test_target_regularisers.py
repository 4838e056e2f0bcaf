"""The MRENT regulariser and the ProDA Jensen-Shannon term of the target loss (prototypes.py:29-39, :323-333;
loss.py:48-85): fixtures G16 (the terms on small and head-size logits) and G17 (two hybrid_proDA steps with
REGULARIZER: MRENT and JS_D > 0), both made by tests/golden/make_golden_regularisers.py from the reference.

The host leg pins an fp64 restatement of the formulas to the reference's values and gradients; the GPU legs hold the
fused kernels (onda_target_loss_fwd / _bwd) to the reference and to that restatement."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import digest

DEV = "cuda:0"
SMALL = ["mixed", "none_ignored", "all_ignored", "saturated"]


def restate(logits, target):
    """fp64 restatement: {js, mrent, mrkld} of logits [B,K,h,w] and labels [B,h,w] (255 = ignored), differentiable."""
    z = logits.double()
    B, K, h, w = z.shape
    lp = z.log_softmax(1)
    p = lp.exp()
    m = (target != 255).double().unsqueeze(1)
    onehot = F.one_hot(torch.where(target == 255, torch.full_like(target, K), target).long(), K + 1)[..., :K]
    y = onehot.permute(0, 3, 1, 2).double().clamp(1e-4, 1.0)
    mp = p * m
    a = (y + mp) / 2

    def xlog2x(v):
        return v * torch.log2(v + 1e-30)

    js = (-xlog2x(a) + (xlog2x(y) + xlog2x(mp)) / 2).sum() / (math.log2(K) * m.sum())
    return {"js": js, "mrent": (p * lp).sum() / (B * h * w), "mrkld": -lp.sum() / (B * K * h * w)}


def restate_grads(logits, target, weights, js_d):
    """(values, {grad_js, grad_mrent, grad_total}) of the restatement; total = yml-weighted CE + RCE + MRENT + js_d*JS."""
    x = logits.double().clone().requires_grad_(True)
    v = restate(x, target)
    keep = target != 255
    lp = x.log_softmax(1)
    pick = lp.gather(1, torch.where(keep, target, torch.zeros_like(target)).long().unsqueeze(1)).squeeze(1)
    ce = -(pick * keep).sum() / keep.sum()
    p = lp.exp()
    onehot = F.one_hot(torch.where(keep, target, torch.zeros_like(target)).long(), x.shape[1]).permute(0, 3, 1, 2)
    rce = -(math.log(1e-4) * (p * (1 - onehot)).sum(1) * keep).sum() / (keep.sum() + 1e-6)
    w_ce, w_rce, w_reg = weights
    grads = {}
    grads["grad_js"] = torch.autograd.grad(v["js"], x, retain_graph=True)[0]
    grads["grad_mrent"] = torch.autograd.grad(v["mrent"], x, retain_graph=True)[0]
    # ce's gradient is zero without a kept pixel (the reference's empty selection); leave its NaN value out of the graph
    total = w_rce * rce + w_reg * v["mrent"] + js_d * v["js"] + (w_ce * ce if keep.any() else 0.0)
    grads["grad_total"] = torch.autograd.grad(total, x)[0]
    return {k: t.detach() for k, t in v.items()}, grads


def _value_close(mine, ref, rtol):
    ref = float(ref)
    if math.isinf(ref):
        return mine == ref
    return mine == pytest.approx(ref, rel=rtol)


def _grad_close(mine, ref, rel, what):
    mine, ref = torch.as_tensor(mine).double().cpu(), torch.as_tensor(ref).double().cpu()
    if torch.isnan(ref).all():
        assert torch.isnan(mine).all(), what
        return
    scale = ref.abs().max().item()
    err = (mine - ref).abs().max().item()
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _head_case(g):
    gen = torch.Generator().manual_seed(int(g["head_seed"]))
    B, K, h, w = (int(v) for v in g["head_shape"])
    logits = 3.0 * torch.randn(B, K, h, w, generator=gen)
    target = torch.randint(0, K, (B, h, w), generator=gen)
    target[torch.rand(B, h, w, generator=gen) < 0.3] = 255
    return logits, target


# ------------------------------------------------------------------------------------------------ host leg
@pytest.mark.parametrize("case", SMALL)
def test_restatement_reproduces_the_reference(golden, case):
    g = golden("g16_regularisers")
    logits, target = torch.from_numpy(g[f"{case}_logits"]), torch.from_numpy(g[f"{case}_target"])
    vals, grads = restate_grads(logits, target, tuple(g["weights"]), float(g["js_d"]))
    for k in ("js", "mrent", "mrkld"):
        assert _value_close(vals[k].item(), g[f"{case}_{k}"], 1e-5), (case, k, vals[k].item(), g[f"{case}_{k}"])
    for k in ("grad_js", "grad_mrent", "grad_total"):
        _grad_close(grads[k], torch.from_numpy(g[f"{case}_{k}"]), 1e-5, f"{case} {k}")
    if case == "all_ignored":  # the reference's own results, reproduced: JS = +inf, NaN gradient, MRENT finite
        assert math.isinf(vals["js"].item()) and vals["js"].item() > 0
        assert torch.isnan(grads["grad_js"]).all() and torch.isfinite(grads["grad_mrent"]).all()


def test_restatement_reproduces_the_reference_at_head_size(golden):
    g = golden("g16_regularisers")
    logits, target = _head_case(g)
    vals, grads = restate_grads(logits, target, tuple(g["weights"]), float(g["js_d"]))
    for k in ("js", "mrent", "mrkld"):
        assert _value_close(vals[k].item(), g[f"head_{k}"], 1e-5), (k, vals[k].item(), g[f"head_{k}"])
    for k in ("grad_js", "grad_mrent", "grad_total"):
        ref, mine = g[f"head_{k}"], digest(grads[k], 4096)
        scale = float(g[f"head_{k}_absmax"])
        assert abs(grads[k].abs().max().item() - scale) <= 1e-5 * scale, k
        np.testing.assert_allclose(mine[2:], ref[2:], rtol=0, atol=1e-5 * scale, err_msg=k)
        np.testing.assert_allclose(mine[:2], ref[:2], rtol=0, atol=1e-5 * ref[1], err_msg=k)  # sum, abs-sum


# ------------------------------------------------------------------------------------------------ GPU legs
def _head_out(logits_nchw, ld=32):
    """CPU logits [B,K,h,w] on the device in the model's pixel-major layout, rows of `ld` floats."""
    B, K, h, w = logits_nchw.shape
    pad = torch.zeros(B, h, w, ld)
    pad[..., :K] = logits_nchw.permute(0, 2, 3, 1)
    return pad.to(DEV)[..., :K].permute(0, 3, 1, 2)


def _run(out, target, w_ce, w_rce, w_reg, reg, w_js):
    from onda_amd import ops
    out = out.detach().requires_grad_(True)
    total, ce, rce, r, js = ops.target_losses(out, target.to(DEV), w_ce, w_rce, w_reg, reg, w_js)
    total.backward()
    return {"total": total.item(), "ce": ce.item(), "rce": rce.item(), "reg": r.item(), "js": js.item(),
            "grad": out.grad.detach().cpu()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", SMALL)
def test_kernels_match_the_reference(golden, case):
    g = golden("g16_regularisers")
    logits, target = torch.from_numpy(g[f"{case}_logits"]), torch.from_numpy(g[f"{case}_target"])
    w_ce, w_rce, w_reg = (float(v) for v in g["weights"])
    js_d = float(g["js_d"])
    js = _run(_head_out(logits), target, 0.0, 0.0, 0.0, "MRKLD", 1.0)
    assert _value_close(js["js"], g[f"{case}_js"], 1e-5), (js["js"], g[f"{case}_js"])
    assert _value_close(js["total"], g[f"{case}_js"], 1e-5)
    _grad_close(js["grad"], torch.from_numpy(g[f"{case}_grad_js"]), 1e-5, f"{case} grad js")
    mrkld = _run(_head_out(logits), target, 0.0, 0.0, 1.0, "MRKLD", 0.0)
    assert _value_close(mrkld["reg"], g[f"{case}_mrkld"], 1e-5)
    mrent = _run(_head_out(logits), target, 0.0, 0.0, 1.0, "MRENT", 0.0)
    assert _value_close(mrent["reg"], g[f"{case}_mrent"], 1e-5), (mrent["reg"], g[f"{case}_mrent"])
    _grad_close(mrent["grad"], torch.from_numpy(g[f"{case}_grad_mrent"]), 1e-5, f"{case} grad mrent")
    full = _run(_head_out(logits), target, w_ce, w_rce, w_reg, "MRENT", js_d)
    _grad_close(full["grad"], torch.from_numpy(g[f"{case}_grad_total"]), 1e-5, f"{case} grad total")
    assert _value_close(full["js"], g[f"{case}_js"], 1e-5) and _value_close(full["reg"], g[f"{case}_mrent"], 1e-5)
    if case == "all_ignored":
        assert math.isinf(full["js"]) and full["js"] > 0
        assert torch.isnan(full["grad"]).all() and torch.isnan(js["grad"]).all()
        assert math.isfinite(mrent["reg"]) and torch.isfinite(mrent["grad"]).all()
    else:
        assert _value_close(full["total"], g[f"{case}_total"], 1e-5), (full["total"], g[f"{case}_total"])
        assert torch.isfinite(full["grad"]).all()


@pytest.mark.gpu
def test_kernels_match_the_restatement_at_head_size(golden):
    g = golden("g16_regularisers")
    logits, target = _head_case(g)
    w_ce, w_rce, w_reg = (float(v) for v in g["weights"])
    js_d = float(g["js_d"])
    vals, grads = restate_grads(logits, target, (w_ce, w_rce, w_reg), js_d)
    js = _run(_head_out(logits), target, 0.0, 0.0, 0.0, "MRENT", 1.0)
    mrent = _run(_head_out(logits), target, 0.0, 0.0, 1.0, "MRENT", 0.0)
    full = _run(_head_out(logits), target, w_ce, w_rce, w_reg, "MRENT", js_d)
    assert _value_close(js["js"], vals["js"], 1e-5) and _value_close(mrent["reg"], vals["mrent"], 1e-5)
    assert _value_close(js["js"], g["head_js"], 1e-5) and _value_close(mrent["reg"], g["head_mrent"], 1e-5)
    assert _value_close(full["total"], g["head_total"], 1e-5), (full["total"], float(g["head_total"]))
    _grad_close(js["grad"], grads["grad_js"], 1e-5, "head grad js")
    _grad_close(mrent["grad"], grads["grad_mrent"], 1e-5, "head grad mrent")
    _grad_close(full["grad"], grads["grad_total"], 1e-5, "head grad total")


@pytest.mark.gpu
def test_two_runs_are_bit_identical(golden):
    g = golden("g16_regularisers")
    logits, target = _head_case(g)
    a = _run(_head_out(logits), target, 0.1, 1.0, 0.1, "MRENT", 3.0)
    b = _run(_head_out(logits), target, 0.1, 1.0, 0.1, "MRENT", 3.0)
    assert all(a[k] == b[k] for k in ("total", "ce", "rce", "reg", "js"))
    assert torch.equal(a["grad"], b["grad"])


@pytest.mark.gpu
def test_strided_and_contiguous_logits_agree(golden):
    """Padded pixel-major rows (ld 32, 24, K) and a plain NCHW tensor (copied by logits_rows): same values, same gradient."""
    g = golden("g16_regularisers")
    logits, target = torch.from_numpy(g["mixed_logits"]), torch.from_numpy(g["mixed_target"])
    runs = [_run(_head_out(logits, ld), target, 0.1, 1.0, 0.1, "MRENT", 3.0) for ld in (32, 24, logits.shape[1])]
    runs.append(_run(logits.to(DEV).contiguous(), target, 0.1, 1.0, 0.1, "MRENT", 3.0))
    for r in runs[1:]:
        assert all(r[k] == runs[0][k] for k in ("total", "ce", "rce", "reg", "js"))
        assert torch.equal(r["grad"], runs[0]["grad"])


@pytest.mark.gpu
def test_framework_functions_run_on_the_kernels(golden):
    from onda_amd.framework.domain_adaptation.methods.prototypes import regular_loss
    from onda_amd.framework.utils.loss import js_divergance
    g = golden("g16_regularisers")
    logits, target = torch.from_numpy(g["mixed_logits"]), torch.from_numpy(g["mixed_target"])
    x = logits.to(DEV).requires_grad_(True)
    v = regular_loss("MRENT", x)
    v.backward()
    assert _value_close(v.item(), g["mixed_mrent"], 1e-5)
    _grad_close(x.grad, torch.from_numpy(g["mixed_grad_mrent"]), 1e-5, "regular_loss MRENT")
    assert regular_loss("KL", x) == 0
    x = logits.to(DEV).requires_grad_(True)
    v = js_divergance(x, target.to(DEV), DEV)
    v.backward()
    assert _value_close(v.item(), g["mixed_js"], 1e-5)
    _grad_close(x.grad, torch.from_numpy(g["mixed_grad_js"]), 1e-5, "js_divergance")


# ------------------------------------------------------------------------------------------------ GPU, full step
def _log_close(mine, ref, key, step, npix):
    """tests/test_hip_model.py's rule: 5e-3 relative; one pixel of count ratios in the second step."""
    if mine == pytest.approx(ref, rel=5e-3, abs=1e-5):
        return True
    if step >= 1 and ("agreement" in key or "percentage" in key or "pixel_num" in key):
        one = 1.0 if "pixel_num" in key else 1.0 / npix
        return abs(mine - ref) <= 1.01 * one
    return False


def _adapter(tmp_path, regularizer, js_d):
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.synthetic import fill_state_dict
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, str(tmp_path), batch_size=2)
    spec.REGULARIZER, spec.JS_D = regularizer, js_d
    model = get_model(cfg, 19)
    fill_state_dict(model, 1, 3.0)
    return get_adapt_method(cfg)(model, cfg, spec)


def _two_steps(da, check):
    """G7's recipe: same batches, same CPU mask draws; `check(s, log, soft)` after every step + update_ema."""
    from onda_amd.framework.model import deeplabv2
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.synthetic import synth_batch
    from oracle import model as omodel
    src = [synth_batch(2, 64, 128, seed=100 + i) for i in range(2)]
    trg = [synth_batch(2, 64, 128, seed=200 + i) for i in range(2)]
    torch.manual_seed(123)
    masks = [omodel.draw_drop_mask(2) for _ in range(8)]
    it = iter(masks)
    deeplabv2.drop_mask_fn = lambda B, C, p, dev: next(it).to(dev)
    try:
        da.update_dynamic()
        switch_batch_statistics(da.model, False)
        da.calculate_prototypes(src, save=False)
        switch_batch_statistics(da.model, True)
        check(-1, None, None)
        da.optimizer.zero_grad()
        for s in range(len(check.steps)):
            da.adjust_learning_rate(s, 6)
            log = da.step([src[s]], trg[s])
            da.update_ema()
            check(s, log, trg[s]["stored_predictions"])
    finally:
        deeplabv2.drop_mask_fn = deeplabv2._default_drop_mask


@pytest.mark.gpu
def test_full_step_with_mrent_and_js_golden(golden, tmp_path):
    """Two hybrid_proDA steps (+update_ema) at 128x64, B=2, dynamic branch, REGULARIZER: MRENT and JS_D = G17's:
    labels, soft predictions, log (both new keys included), prototypes and the weight updates against the reference."""
    g = golden("g17_step_regularisers")
    da = _adapter(tmp_path, "MRENT", float(g["js_d"]))
    prev = {}

    def check(s, log, soft):
        if s < 0:
            np.testing.assert_allclose(da.prototypes.prototypes.cpu().numpy(), g["proto0"], rtol=1e-3, atol=1e-4)
            for who, mod in (("student.", da.model), ("teacher.", da.ema_model)):
                for k, v in mod.state_dict().items():
                    prev[who + k] = digest(v.float(), 64)[2:]
            return
        assert not any(torch.is_tensor(v) and (v.requires_grad or v.grad_fn is not None) for v in log.values())
        assert int(g[f"branch{s}"]) == da.model_select.current
        assert (soft.cpu() - torch.from_numpy(g[f"soft{s}"])).abs().max() < 2e-3
        # pseudo-labels: equal wherever the reference's top two soft values are not within the soft tolerance of a tie
        top2 = torch.from_numpy(g[f"soft{s}"]).topk(2, dim=1).values
        decided = ((top2[:, 0] - top2[:, 1]) > 4e-3).numpy()
        mine_labels = soft.argmax(1).to(torch.uint8).cpu().numpy()
        assert np.array_equal(mine_labels[decided], g[f"labels{s}"][decided])
        ref = json.loads(str(g[f"log{s}_json"]))
        assert ref["JS Divergance loss"] > 0 and ref["regularization_loss"] < 0  # the two terms are in the fixture
        for k, v in ref.items():
            mine = log[k]
            mine = mine.item() if isinstance(mine, torch.Tensor) else float(mine)
            assert _log_close(mine, v, k, s, soft[0, 0].numel() * soft.shape[0]), (s, k, mine, v)
        np.testing.assert_allclose(da.prototypes.prototypes.cpu().numpy(), g[f"proto{s + 1}"], rtol=1e-3, atol=1e-4)
        names, dg = list(g[f"state_names{s}"]), g[f"state_digest{s}"]
        num = den = 0.0
        for who, mod in (("student.", da.model), ("teacher.", da.ema_model)):
            for k, v in mod.state_dict().items():
                if not v.is_floating_point() or v.dim() == 0:
                    continue
                row = dg[names.index(who + k)][2:]
                mine = digest(v.float(), 64)[2:]
                num += ((mine - row) ** 2).sum()
                den += ((row - prev[who + k]) ** 2).sum()
                prev[who + k] = row
        assert (num / den) ** 0.5 <= (0.02 if s == 0 else 0.6), (s, (num / den) ** 0.5)
    check.steps = (0, 1)
    _two_steps(da, check)


@pytest.mark.gpu
def test_default_step_keeps_the_seg_loss_kernels(tmp_path, monkeypatch):
    """The shipped settings (MRKLD, JS_D 0) launch exactly what they launched before: seg_loss, never target_loss."""
    from onda_amd.ops import loss as oloss
    seen = []
    real = oloss.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(oloss, "call", spy)
    da = _adapter(tmp_path, "MRKLD", 0)

    def check(s, log, soft):
        if s == 0:
            assert log["JS Divergance loss"] == 0
    check.steps = (0,)
    _two_steps(da, check)
    torch.cuda.synchronize()
    assert "onda_seg_loss_fwd" in seen and "onda_seg_loss_bwd" in seen
    assert not any(n.startswith("onda_target_loss") for n in seen), seen
