"""GPU: a DeepLabV2 with the 'normal' classifier head (MODEL.CLASSIFIER: 'normal', both levels) against fixture G25 (b) -- one
train-mode forward + backward of the reference in float64 and float32 with the loss of segmentation.py:70-80
(tests/golden/make_golden_normal_head.py) -- with the bars test_gn_model.py applies to the same quantities, and through
``SegmentationTrainer``: the reference's ``segmentation.train`` unit of work and its validation pass.  Every route of the head:
"f16x2" with the tap-table launches, "f16x2" with one launch per branch, exact fp32."""
import types

import numpy as np
import pytest
import torch

import normal_head_common as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(params=[("f16x2", True), ("f16x2", False), ("f32", False)], ids=["f16x2-taps", "f16x2-chain", "f32-chain"])
def route(request):
    from onda_amd import ops
    from onda_amd.framework.model import deeplabv2
    old = ops.CONV_MODE, ops.TAP_CONV
    ops.CONV_MODE, ops.TAP_CONV = request.param
    was = deeplabv2.enable_normal_classifier()
    yield "%s %s" % (request.param[0], "taps" if request.param[1] else "chain")
    deeplabv2.enable_normal_classifier(was)
    ops.CONV_MODE, ops.TAP_CONV = old


def build_model():
    from onda_amd.framework.handlers import get_model
    from onda_amd.framework.model import deeplabv2
    from onda_amd.synthetic import fill_state_dict
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NAME=C.MODEL, CLASSIFIER="normal", LOAD=None, MULTI_LEVEL=True),
                                OTHERS=types.SimpleNamespace(DEVICE=DEV))
    m = get_model(cfg, C.CLASSES)
    assert isinstance(m.layer5, deeplabv2.ClassifierModule) and not m.feat
    fill_state_dict(m, 1, 3.0)
    return m


def test_train_forward_backward_against_g25(golden, route):
    """Both logit maps within 1e-3 of the float64 run's maximum, the loss within 1e-4 relative, every gradient within 3 x the
    reference's own float32 distance from float64 + 1e-2 in relative L2 (on the fixture's strided samples)."""
    from onda_amd import ops
    from onda_amd.synthetic import synth_batch
    g = golden("g25_normal_head")
    m = build_model().train()
    batch = synth_batch(2, 64, 128)
    aux, main = m(batch["image"].to(DEV))
    assert torch.is_tensor(main) and torch.is_tensor(aux) and main.shape == (2, C.CLASSES, 9, 17) == aux.shape
    label = batch["label"].to(DEV)
    loss = ops.upsample_ce(main, label) + 0.1 * ops.upsample_ce(aux, label)
    for key, mine in (("main", main), ("aux", aux)):
        ref = g[f"b_{key}64"]
        err = np.abs(mine.detach().cpu().numpy() - ref).max() / np.abs(ref).max()
        print(f"{route} {key}: {err:.3e} of the maximum")
        assert err <= 1e-3, (key, err)
    rel = abs(loss.item() - float(g["b_loss64"])) / abs(float(g["b_loss64"]))
    print(f"{route} loss: {rel:.3e} relative")
    assert rel <= 1e-4
    loss.backward()
    params = dict(m.named_parameters())
    names = list(g["b_grad_names"])
    assert names == [n for n, p in m.named_parameters() if p.grad is not None]
    worst, failed = (0.0, ""), []
    for i, n in enumerate(names):
        mine = C.sampled(params[n].grad.detach().double().cpu(), C.grad_samples(n)).numpy()
        r64, r32 = g[f"b_g64_{i}"].astype(np.float64), g[f"b_g32_{i}"].astype(np.float64)
        assert mine.shape == r64.shape
        norm = np.linalg.norm(r64) + 1e-30
        e_mine, e_ref = np.linalg.norm(mine - r64) / norm, np.linalg.norm(r32 - r64) / norm
        ratio = e_mine / (3 * e_ref + 1e-2)
        worst = max(worst, (ratio, f"{n}: {e_mine:.3e} against e_ref {e_ref:.3e}"))
        if ".conv2d_list." in n and n.endswith(".weight"):
            print(f"{route} {n}: {e_mine:.3e} (e_ref {e_ref:.3e})")
        if ratio > 1.0:
            failed.append((n, e_mine, e_ref))
    print(f"{route} worst gradient, as a share of its bar: {worst[0]:.3f} ({worst[1]})")
    assert not failed, failed


def test_trainer_steps_and_evaluates(golden, route):
    """Two ``SegmentationTrainer.step`` calls and one ``evaluate`` on the model: finite losses, the first one the fixture's (the
    step's loss IS segmentation.py:70-80 on the fixture's batch), every parameter finite and the head moved."""
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.domain_adaptation.methods.segmentation import SegmentationTrainer
    from onda_amd.synthetic import synth_batch
    g = golden("g25_normal_head")
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, "NONE", batch_size=2)
    spec.LEARNING_RATE, spec.POWER, spec.WEIGHT_DECAY = 2.5e-4, 0.9, 5e-4
    m = build_model().train()
    tr = SegmentationTrainer(m, cfg, spec)
    batches = [synth_batch(2, 64, 128), synth_batch(2, 64, 128, seed=8)]
    before = m.layer6.conv2d_list[3].weight.detach().clone()
    losses = [tr.step(b, 10).item() for b in batches]
    assert all(np.isfinite(v) for v in losses)
    assert abs(losses[0] - float(g["b_loss64"])) <= 1e-4 * abs(float(g["b_loss64"])), losses
    assert float((m.layer6.conv2d_list[3].weight.detach() - before).abs().max()) > 0
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    iou = tr.evaluate([batches[0]])
    assert iou.shape == (C.CLASSES,) and np.isfinite(np.nanmean(iou)) and m.training


def test_eval_forward_is_deterministic(route):
    from onda_amd.synthetic import synth_batch
    m = build_model().eval()
    x = synth_batch(2, 64, 128)["image"].to(DEV)
    with torch.no_grad():
        a = m(x)
        b = m(x)
    for u, v in zip(a, b):
        assert torch.is_tensor(u) and u.shape == (2, C.CLASSES, 9, 17)
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v)
    assert float((a[0] - a[1]).abs().max()) > 0
