"""GPU: the DeepLabv2-Resnet101-ProDA model (opt-in on; all 104 BatchNorms train their affine parameters) against the reference's
runs of the same tree (fixtures G26, tests/golden/make_golden_proda101.py): one train-mode forward + backward of the seeded model on
a 2 x 3 x 65 x 129 batch against the reference's float64 run -- ``out``, ``feat``, all 208 BatchNorm gradient vectors, every other
gradient's norm and strided sample --, one ``online_proDA.step`` (static prior, replay buffer on) against the reference's, and
``freeze_bn=True``.

Tolerance, per tensor in relative L2: MARGIN = 4 x the distance of the reference's own float32 run from its float64 run (both in
the fixture), 4 x u where that is smaller (proda101_cases.tolerance).  The seeded N(0, 0.01) weights make a badly conditioned
network -- the reference's own float32 gradients are 2e-2 .. 7e-2 away from its float64 ones -- which is what the margin is relative to."""
import json
import os
import tempfile
import types
import warnings
from unittest import mock

import numpy as np
import pytest
import torch

from conftest import digest

import gn_site_fp64 as S
import proda101_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(params=["f32", "f16x2"])
def conv_mode(request):
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, request.param
    yield request.param
    ops.CONV_MODE = old


@pytest.fixture
def opt_in():
    from onda_amd.framework.handlers import model_handler as H
    old = H.enable_resnet101_proda()
    yield
    H.enable_resnet101_proda(old)


def build(**kw):
    """The handler's model, seeded: ``get_model`` with the opt-in on (or ``Deeplab`` with extra arguments)."""
    from onda_amd.framework.handlers import get_model
    from onda_amd.framework.model.deeplabv2_proda import Deeplab, ResNet101
    torch.manual_seed(P.SEED)
    # (an empty hub directory: the seeded init is what the fixture has, whatever the user's own cache holds)
    with warnings.catch_warnings(), tempfile.TemporaryDirectory() as home, mock.patch.dict(os.environ, {"TORCH_HOME": home}):
        warnings.simplefilter("ignore")
        if kw:
            m = Deeplab(torch.nn.BatchNorm2d, num_classes=19, **kw).to(DEV)
        else:
            cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NAME=P.PRODA_MODEL, CLASSIFIER="ProDA", LOAD=None, MULTI_LEVEL=True),
                                        OTHERS=types.SimpleNamespace(DEVICE=DEV))
            m = get_model(cfg, 19)
            assert cfg.MODEL.MULTI_LEVEL is False
    assert isinstance(m, ResNet101)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
    return m.train()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def test_train_forward_backward_against_g26(golden, opt_in, conv_mode):
    from onda_amd import ops
    from onda_amd.synthetic import synth_batch
    g, gb = golden("g26_proda101"), golden("g26_proda101_bn")
    m = build()
    none, o = m(synth_batch(2, P.H, P.W)["image"].to(DEV))
    assert none is None and set(o) == {"feat", "out"}
    assert np.array_equal(g["labels"], S.labels().numpy())
    loss = ops.seg_losses(o["out"], S.labels().to(DEV), 1.0, 0.0, 0.0)[0]
    failed, ratios = [], {}

    def hold(what, mine, r64, e_ref):
        e = rel(mine, r64)
        ratio = e / P.tolerance(e_ref)
        kind = what if what in ("out", "feat", "loss") else ("bn " + what.rsplit(".", 1)[1] if what in bn_set else "other")
        ratios[kind] = max(ratios.get(kind, (0.0, "")), (ratio, f"{what}: {e:.3e}, e_ref {e_ref:.3e}"))
        if ratio > 1.0:
            failed.append((what, e, e_ref))

    bn_names = list(gb["names"])
    bn_set = set(bn_names)
    hold("out", o["out"].detach().cpu().numpy(), g["out64"], rel(g["out32"], g["out64"]))
    f64 = g["feat64"].reshape(-1)
    idx = S.sample_index(f64.size, S.SAMPLE_DS).numpy()
    hold("feat", o["feat"].detach().cpu().numpy(), g["feat64"], rel(g["feat32_sample"], f64[idx]))
    hold("loss", [loss.item()], [float(g["loss64"])], abs(float(g["loss32"]) - float(g["loss64"])) / abs(float(g["loss64"])))
    loss.backward()
    params = dict(m.named_parameters())
    # ---- all 208 BatchNorm gradient vectors, whole
    assert bn_names == P.bn_param_names(m) and len(bn_names) == 208
    off = 0
    for n, size in zip(bn_names, gb["sizes"]):
        r64, r32 = gb["g64"][off:off + size], gb["g32"][off:off + size]
        off += int(size)
        assert params[n].grad is not None, f"{n} received no gradient"
        hold(n, params[n].grad.cpu().numpy(), r64, rel(r32, r64))
    # ---- every other gradient: its norm (against the whole-tensor distance of the reference's two runs) and a strided sample
    for i, n in enumerate(g["other_names"]):
        grad = params[str(n)].grad.detach().double().cpu().reshape(-1)
        e_ref = float(g["other_eref"][i])
        n64 = float(g["other_norm64"][i])
        e = abs(float(grad.norm()) - n64) / n64
        ratios["other norm"] = max(ratios.get("other norm", (0.0, "")), (e / P.tolerance(e_ref), f"{n}: {e:.3e}, e_ref {e_ref:.3e}"))
        if e > P.tolerance(e_ref):
            failed.append((str(n) + " norm", e, e_ref))
        sidx = S.sample_index(grad.numel(), S.SAMPLE)
        hold(str(n), grad[sidx].numpy(), g["other_sample64"][i], rel(g["other_sample32"][i], g["other_sample64"][i]))
    for kind in sorted(ratios):
        print(f"{conv_mode} worst ratio to the tolerance: {kind}: {ratios[kind][0]:.3f} ({ratios[kind][1]})")
    assert not failed, failed[:8]


def test_freeze_bn_leaves_no_batchnorm_gradient(opt_in, conv_mode):
    from onda_amd import ops
    from onda_amd.ops import norm
    from onda_amd.synthetic import synth_batch
    m = build(freeze_bn=True)
    calls = []
    real = norm.call
    norm.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        _, o = m(synth_batch(2, P.H, P.W)["image"].to(DEV))
        ops.seg_losses(o["out"], S.labels().to(DEV), 1.0, 0.0, 0.0)[0].backward()
    finally:
        norm.call = real
    bn = set(P.bn_param_names(m))
    for n, p in m.named_parameters():
        assert (p.grad is None) == (n in bn), n
    assert not [c for c in calls if "affine" in c], "a frozen model reached the affine entry points"
    assert any(c in ("onda_bn_bwd", "onda_bn_bwd_l2") for c in calls)


def _log_close(mine, ref, key):
    """test_hip_model.py's rule for the log scalars of a FIRST step: 5e-3 relative."""
    return mine == pytest.approx(ref, rel=5e-3, abs=1e-5)


def test_online_proda_step_against_g26(golden, opt_in, tmp_path, conv_mode):
    """One online_proDA.step (static prior, replay buffer on) + update_ema on the weights of fill_state_dict(model, 1, 40.0): the log
    keys of the reference, finite; log scalars, soft labels, prototypes and the post-step weights as updates with the comparisons and
    bars tests/test_gn_model.py::test_full_step_against_g22 applies to a first step; every BatchNorm gamma / beta moved."""
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.framework.model import deeplabv2
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.ops import norm
    from onda_amd.synthetic import fill_state_dict, synth_batch
    from oracle import model as omodel
    g = golden("g26_proda101_step")
    cfg, spec = hybrid_switch_cfg(P.W, P.H, DEV, str(tmp_path), batch_size=2)
    cfg.MODEL.NAME = P.PRODA_MODEL
    cfg.METHOD.ADAPTATION.NAME = "PROTO_ONLINE"
    spec.pop("GRAY_AREA", None)
    for k, v in P.STEP_SPEC.items():
        spec[k] = v
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = get_model(cfg, 19)
    fill_state_dict(model, 1, P.STEP_HEAD_SCALE)
    da = get_adapt_method(cfg)(model, cfg, spec)
    srcs = [synth_batch(2, P.H, P.W, seed=100 + i) for i in range(2)]
    trg = synth_batch(2, P.H, P.W, seed=200)
    torch.manual_seed(123)
    masks = iter([omodel.draw_drop_mask(2) for _ in range(8)])  # the same CPU draws as the reference run
    deeplabv2.drop_mask_fn = lambda B, C, p, dev: next(masks).to(dev)
    try:
        da.update_dynamic()
        switch_batch_statistics(da.model, False)
        da.calculate_prototypes(srcs, save=False)
        switch_batch_statistics(da.model, True)
        np.testing.assert_allclose(da.prototypes.prototypes.cpu().numpy(), g["proto0"], rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(da.prototypes.counter.cpu().numpy(), g["counter0"])
        da.optimizer.zero_grad()
        bn = P.bn_param_names(da.model)
        before = {n: p.detach().clone() for n, p in da.model.named_parameters() if n in set(bn)}
        assert len(before) == 208
        da.adjust_learning_rate(0, 6)
        calls, real = [], norm.call
        norm.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        try:
            log = da.step([srcs[0]], trg)
        finally:
            norm.call = real
        da.update_ema()
        # the student's BatchNorms went through the affine entry points -- in "f16x2" the paired student pass: both row groups
        # in one call, the shortcut blocks as pairs
        assert "onda_bn_bwd_affine" in calls and not [c for c in calls if c in ("onda_bn_bwd_l2", "onda_bn_pair_bwd_l2")]
        if conv_mode == "f16x2":
            assert calls.count("onda_bn_pair_bwd_affine_l2") == 4 and calls.count("onda_bn_bwd_affine_l2") == 104 - 1 - 8, \
                (calls.count("onda_bn_pair_bwd_affine_l2"), calls.count("onda_bn_bwd_affine_l2"))
        ref = json.loads(str(g["log_json"]))
        for k, v in ref.items():
            assert k in log, k
            mine = log[k]
            mine = mine.item() if isinstance(mine, torch.Tensor) else float(mine)
            assert np.isfinite(v) and np.isfinite(mine), (k, mine, v)
            print(f"{conv_mode} {k}: {mine:.6g} (reference {v:.6g})")
            assert _log_close(mine, v, k), (k, mine, v)
        soft = trg["stored_predictions"]
        assert (soft.cpu() - torch.from_numpy(g["soft"])).abs().max() < 2e-3
        np.testing.assert_allclose(da.prototypes.prototypes.cpu().numpy(), g["proto1"], rtol=1e-3, atol=1e-4)
        names, d0, d1 = list(g["state_names"]), g["state_before"], g["state_after"]
        num = den = 0.0
        for who, mod in (("student.", da.model), ("teacher.", da.ema_model)):
            for k, v in mod.state_dict().items():
                if not v.is_floating_point() or v.dim() == 0:
                    continue
                i = names.index(who + k)
                num += ((digest(v.float(), 64)[2:] - d1[i][2:]) ** 2).sum()
                den += ((d1[i][2:] - d0[i][2:]) ** 2).sum()
        rel_update = (num / den) ** 0.5
        print(f"{conv_mode} step: update rel-L2 against the reference {rel_update:.4f}")
        assert rel_update <= 0.02, rel_update
        moved = {n: bool((p.detach() != before[n]).any()) for n, p in da.model.named_parameters() if n in before}
        assert all(moved.values()), [n for n, v in moved.items() if not v][:8]
    finally:
        deeplabv2.drop_mask_fn = deeplabv2._default_drop_mask
