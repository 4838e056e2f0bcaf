"""GPU: the DeepLabv2-Resnet50-GN model (GroupNorm at the stem and at the four shortcuts, as the reference's handler builds it)
against G21 -- one train-mode forward + backward of the reference in float64 and float32 (tests/golden/make_golden_gn.py) -- with
the bars test_hip_model.py applies to the BatchNorm model for the same quantities, against G22 -- two hybrid_proDA steps of the
reference on that model, both switch branches -- and in the places the adaptation step puts a model: the paired student pass, the
predicated dynamic pass, an eval forward after a train step."""
import json
import types

import numpy as np
import pytest
import torch

from conftest import digest

import gn_site_fp64 as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(params=["f32", "f16x2"])
def conv_mode(request):
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, request.param
    yield request.param
    ops.CONV_MODE = old


@pytest.fixture
def f16x2():
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    yield
    ops.CONV_MODE = old


def build_model(seed=1, head_scale=3.0):
    from onda_amd.framework.handlers import get_model
    from onda_amd.synthetic import fill_state_dict
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NAME=S.GN_MODEL, CLASSIFIER="ProDA", LOAD=None, MULTI_LEVEL=False),
                                OTHERS=types.SimpleNamespace(DEVICE=DEV))
    m = get_model(cfg, 19)
    fill_state_dict(m, seed, head_scale)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
    return m


def test_train_forward_backward_against_g21(golden, conv_mode):
    """feat / out within 1e-3 of the float64 run's maximum, the loss within 1e-4 relative, every gradient within 3 x the
    reference's own float32 distance from float64 + 1e-2 in relative L2 (whole tensors for conv1.weight and
    layer1.0.downsample.0.weight, the fixture's strided sample for the rest)."""
    from onda_amd import ops
    from onda_amd.synthetic import synth_batch
    g = golden("g21_gn_model")
    m = build_model().train()
    _, o = m(synth_batch(2, 64, 128)["image"].to(DEV))
    assert np.array_equal(g["labels"], S.labels().numpy())
    loss = ops.seg_losses(o["out"], S.labels().to(DEV), 1.0, 0.0, 0.0)[0]
    for key in ("feat", "out"):
        ref = g[key + "64"]
        err = np.abs(o[key].detach().cpu().numpy() - ref).max() / np.abs(ref).max()
        print(f"{conv_mode} {key}: {err:.3e} of the maximum")
        assert err <= 1e-3, (key, err)
    rel = abs(loss.item() - float(g["loss64"])) / abs(float(g["loss64"]))
    print(f"{conv_mode} loss: {rel:.3e} relative")
    assert rel <= 1e-4
    loss.backward()
    params = dict(m.named_parameters())
    names = list(g["grad_names"])
    assert names == [n for n, p in m.named_parameters() if p.grad is not None]
    worst = (0.0, "")
    failed = []
    for i, n in enumerate(names):
        mine = params[n].grad.detach().double().cpu().reshape(-1)
        idx = S.grad_index(n, mine.numel())
        mine = (mine if idx is None else mine[idx]).numpy()
        r64, r32 = g[f"g64_{i}"].astype(np.float64), g[f"g32_{i}"].astype(np.float64)
        assert mine.shape == r64.shape
        norm = np.linalg.norm(r64) + 1e-30
        e_mine, e_ref = np.linalg.norm(mine - r64) / norm, np.linalg.norm(r32 - r64) / norm
        ratio = e_mine / (3 * e_ref + 1e-2)
        worst = max(worst, (ratio, f"{n}: {e_mine:.3e} against e_ref {e_ref:.3e}"))
        if n == "conv1.weight" or ".downsample.0." in n:
            print(f"{conv_mode} {n}: {e_mine:.3e} (e_ref {e_ref:.3e})")
        if ratio > 1.0:
            failed.append((n, e_mine, e_ref))
    print(f"{conv_mode} worst gradient, as a share of its bar: {worst[0]:.3f} ({worst[1]})")
    assert not failed, failed


def test_eval_forward_after_a_train_step_is_finite_and_deterministic(conv_mode):
    from onda_amd import ops
    from onda_amd.synthetic import synth_batch
    m = build_model().train()
    x = synth_batch(2, 64, 128)["image"].to(DEV)
    _, o = m(x)
    ops.seg_losses(o["out"], S.labels().to(DEV), 1.0, 0.0, 0.0)[0].backward()
    with torch.no_grad():
        for p in m.parameters():
            if p.grad is not None:
                p.add_(p.grad, alpha=-1e-3)
    m.eval()
    with torch.no_grad():
        a = m(x)[1]
        b = m(x)[1]
    for key in ("feat", "out"):
        assert bool(torch.isfinite(a[key]).all()) and torch.equal(a[key], b[key]), key
    assert a["out"].shape == (2, 19, 9, 17) and float((a["out"] - o["out"].detach()).abs().max()) > 0


def test_predicated_pass_obeys_the_flag(f16x2):
    """The dynamic model's pass under the device-side switch: with the flag at 0 nothing of it is computed and the selected prior
    is the static one bit for bit; with the flag at 1 it is the unpredicated pass bit for bit."""
    from onda_amd import ops
    from onda_amd.synthetic import synth_batch
    assert ops.predicates_supported()
    static, dynamic = build_model(1).eval(), build_model(2).eval()
    x = synth_batch(2, 64, 128)["image"].to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        prior = static(x)[1]["out"].contiguous()
        plain = dynamic(x)[1]["out"].contiguous()
        with ops.predicated(flag):
            skipped = dynamic(x)[1]["out"]
        assert torch.equal(ops.select_prior(flag, prior, 1.0, skipped, 0.5), prior)
        flag.fill_(1)
        with ops.predicated(flag):
            ran = dynamic(x)[1]["out"]
        assert torch.equal(ran.contiguous(), plain)
        assert torch.equal(ops.select_prior(flag, prior, 1.0, ran, 0.5), 0.5 * plain)
    assert ops.PREDICATE is None


def test_paired_student_pass_matches_the_two_passes(tmp_path, f16x2):
    """test_hip_model.py's comparison and bars on the GN model: GroupNorm is per image, so the five sites need no row groups --
    the one pass over both batches and the two passes agree as they do for the BatchNorm model."""
    from onda_amd import ops
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.domain_adaptation.methods import prototypes as pmod
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.framework.model import deeplabv2
    from onda_amd.synthetic import fill_state_dict, synth_batch
    from oracle import model as omodel
    assert ops.row_groups_supported()

    def run(paired):
        old, pmod.PAIR_STUDENT = pmod.PAIR_STUDENT, paired
        try:
            cfg, spec = hybrid_switch_cfg(256, 128, DEV, str(tmp_path), batch_size=2)
            cfg.MODEL.NAME = S.GN_MODEL
            model = get_model(cfg, 19)
            assert isinstance(model.bn1, torch.nn.GroupNorm)
            fill_state_dict(model, 1, 40.0)
            da = get_adapt_method(cfg)(model, cfg, spec)
            src = [synth_batch(2, 128, 256, seed=100 + i) for i in range(2)]
            trg = [synth_batch(3, 128, 256, seed=200 + i) for i in range(2)]
            torch.manual_seed(123)
            deeplabv2.drop_mask_fn = lambda B, C, p, dev: omodel.draw_drop_mask(B).to(dev)
            try:
                da.update_dynamic()
                switch_batch_statistics(da.model, False)
                da.calculate_prototypes(src, save=False)
                switch_batch_statistics(da.model, True)
                da.optimizer.zero_grad()
                states, logs = [{k: v.detach().double().cpu().clone() for k, v in da.model.state_dict().items()}], []
                for s_ in range(2):
                    da.adjust_learning_rate(s_, 6)
                    log = da.step([src[s_]], trg[s_])
                    da.update_ema()
                    logs.append({k: float(v) for k, v in log.items() if not isinstance(v, dict)})
                    states.append({k: v.detach().double().cpu().clone() for k, v in da.model.state_dict().items()})
                return states, logs, da.prototypes.prototypes.cpu().clone()
            finally:
                deeplabv2.drop_mask_fn = deeplabv2._default_drop_mask
        finally:
            pmod.PAIR_STUDENT = old

    sa, la, pa = run(True)
    sb, lb, pb = run(False)
    for s_ in range(2):
        assert la[s_].keys() == lb[s_].keys()
        for k in la[s_]:
            a, b = la[s_][k], lb[s_][k]
            assert a == b or (np.isnan(a) and np.isnan(b)) or abs(a - b) <= (2e-5 if s_ == 0 else 5e-3) * max(abs(b), 1e-3), (s_, k, a, b)
        num = den = 0.0
        for k in sa[0]:
            if sa[0][k].is_floating_point() and sa[0][k].dim() > 0:
                num += float(((sa[s_ + 1][k] - sb[s_ + 1][k]) ** 2).sum())
                den += float(((sb[s_ + 1][k] - sb[s_][k]) ** 2).sum())
        rel = (num / den) ** 0.5
        print("GN model, paired vs two passes, step", s_, "update rel-L2", rel)
        assert rel <= (3e-3 if s_ == 0 else 0.6), (s_, rel)
    assert (pa - pb).abs().max() <= 1e-4 * pb.abs().max()


def _log_close(mine, ref, key, step, npix):
    """test_hip_model.py's rule for log scalars: 5e-3 relative; pixel-count ratios of the SECOND step, behind one SGD step through
    train-mode BatchNorm, may move by one pixel (a tie of an argmax is within the reference's own noise there)."""
    if mine == pytest.approx(ref, rel=5e-3, abs=1e-5):
        return True
    if step >= 1 and ("agreement" in key or "percentage" in key or "pixel_num" in key):
        one = 1.0 if "pixel_num" in key else 1.0 / npix
        return abs(mine - ref) <= 1.01 * one
    return False


@pytest.mark.parametrize("tag,head_scale", [("static", 40.0), ("dynamic", 3.0)])
def test_full_step_against_g22(golden, tmp_path, conv_mode, tag, head_scale):
    """Two complete hybrid_proDA steps (+ update_ema) of the GN model at 128 x 64, B = 2 against the reference's log dict, soft
    labels, prototypes and post-step weights (fixture G22), both switch branches: the comparisons and bars of
    test_hip_model.py::test_full_step_golden."""
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.framework.model import deeplabv2
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.synthetic import fill_state_dict, synth_batch
    from oracle import model as omodel
    g = golden(f"g22_gn_step_{tag}")
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, str(tmp_path), batch_size=2)
    cfg.MODEL.NAME = S.GN_MODEL
    model = get_model(cfg, 19)
    fill_state_dict(model, 1, head_scale)
    da = get_adapt_method(cfg)(model, cfg, spec)
    assert isinstance(da.ema_model.bn1, torch.nn.GroupNorm) and isinstance(da.static_model.layer1[0].downsample[1], torch.nn.GroupNorm)
    src = [synth_batch(2, 64, 128, seed=100 + i) for i in range(2)]
    trg = [synth_batch(2, 64, 128, seed=200 + i) for i in range(2)]
    torch.manual_seed(123)
    masks = [omodel.draw_drop_mask(2) for _ in range(8)]  # same CPU draws as the reference run
    it = iter(masks)
    deeplabv2.drop_mask_fn = lambda B, C, p, dev: next(it).to(dev)
    try:
        da.update_dynamic()
        switch_batch_statistics(da.model, False)
        da.calculate_prototypes(src, save=False)
        switch_batch_statistics(da.model, True)
        np.testing.assert_allclose(da.prototypes.prototypes.cpu().numpy(), g["proto0"], rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(da.prototypes.counter.cpu().numpy(), g["counter0"])
        da.optimizer.zero_grad()
        prev_digest = {who + k: digest(v.float(), 64)[2:] for who, mod in (("student.", da.model), ("teacher.", da.ema_model))
                       for k, v in mod.state_dict().items()}
        for s in range(2):
            da.adjust_learning_rate(s, 6)
            log = da.step([src[s]], trg[s])
            da.update_ema()
            assert int(g[f"branch{s}"]) == da.model_select.current
            soft = trg[s]["stored_predictions"]
            assert (soft.cpu() - torch.from_numpy(g[f"soft{s}"])).abs().max() < 2e-3
            ref = json.loads(str(g[f"log{s}_json"]))
            for k, v in ref.items():
                mine = log[k]
                mine = mine.item() if isinstance(mine, torch.Tensor) else float(mine)
                assert _log_close(mine, v, k, s, soft[0, 0].numel() * soft.shape[0]), (s, k, mine, v)
            np.testing.assert_allclose(da.prototypes.prototypes.cpu().numpy(), g[f"proto{s + 1}"], rtol=1e-3, atol=1e-4)
            # post-step weights as UPDATES (w_after - w_before), student and teacher, on the fixture's strided digests
            names, dg = list(g[f"state_names{s}"]), g[f"state_digest{s}"]
            num = den = 0.0
            for who, mod in (("student.", da.model), ("teacher.", da.ema_model)):
                for k, v in mod.state_dict().items():
                    if not v.is_floating_point() or v.dim() == 0:
                        continue
                    row = dg[names.index(who + k)][2:]
                    mine = digest(v.float(), 64)[2:]
                    num += ((mine - row) ** 2).sum()
                    den += ((row - prev_digest[who + k]) ** 2).sum()
                    prev_digest[who + k] = row
            rel = (num / den) ** 0.5
            print(f"{conv_mode} {tag} step {s}: update rel-L2 against the reference {rel:.4f}")
            assert rel <= (0.02 if s == 0 else 0.6), (s, rel)
    finally:
        deeplabv2.drop_mask_fn = deeplabv2._default_drop_mask
