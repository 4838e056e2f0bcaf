"""CPU: the DeepLabV2 'normal' classifier head without a GPU -- fixture G25 (tests/golden/make_golden_normal_head.py: the
reference's ClassifierModule alone and inside its model, float64 and float32) against itself and against the float64 reference the
GPU parity test uses (normal_head_common: conv_fp64 summed over the four dilations); the module tree, keys, initialisation and
optimizer walk of the mirror against the reference's; the opt-in switch; the adaptation methods' refusal.

Bounds of the float32-against-float64 comparisons: a float32 sum of n products carries about u * sqrt(n) relative error in L2,
u = 2^-24 -- 36 taps x 64 channels = 2304 terms for the output and dx (2.9e-6), 2 x 27 x 34 = 1836 pixels for dW and db (2.6e-6);
the bound is 1e-5.  The fixture's float64 values are stored rounded to float32 (6e-8): conv_fp64's sum has to reproduce them to
5e-7."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import conv_fp64 as R
import normal_head_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


@pytest.fixture
def normal_head():
    from onda_amd.framework.model import deeplabv2
    old = deeplabv2.enable_normal_classifier()
    yield deeplabv2
    deeplabv2.enable_normal_classifier(old)


@pytest.fixture(scope="module")
def head64():
    """The float64 reference of fixture (a)'s case from conv_fp64: (out, dx, [dW], db), NHWC."""
    x = C.head_input().permute(0, 2, 3, 1).contiguous()
    dy = C.head_dout().permute(0, 2, 3, 1).contiguous()
    ws, bs = C.head_params()
    return (C.sum_fwd64(x, ws, bs), C.sum_dgrad64(dy, ws, (C.HEAD_H, C.HEAD_W)), C.sum_wgrads64(x, dy), R.bias_grad(dy)), (x, dy, ws, bs)


def test_fixture_a_float32_agrees_with_float64(golden):
    g = golden("g25_normal_head")
    assert g["a_out64"].shape == (C.HEAD_B, C.CLASSES, C.HEAD_H, C.HEAD_W)
    pairs = [("out", C.sampled(torch.from_numpy(g["a_out64"]), C.HEAD_SAMPLE).numpy(), g["a_out32_sample"]),
             ("dx", g["a_dx64_sample"], g["a_dx32_sample"])]
    for i in range(len(C.DILATIONS)):
        pairs.append((f"dW{i}", g[f"a_dw64_{i}_sample"], g[f"a_dw32_{i}_sample"]))
        pairs.append((f"db{i}", g[f"a_db64_{i}"], g[f"a_db32_{i}"]))
    for what, r64, r32 in pairs:
        e = rel_l2(r32, r64)
        print(f"{what}: float32 against float64 {e:.3e}")
        assert e <= 1e-5, (what, e)
    # the four biases see the same upstream gradient: one bias gradient
    for i in range(1, len(C.DILATIONS)):
        assert np.array_equal(g["a_db64_0"], g[f"a_db64_{i}"])


def test_fp64_sum_of_dilations_reproduces_fixture_a(golden, head64):
    """The GPU parity test's reference (conv_fp64, one tap at a time, summed over the dilations) IS the reference module's
    arithmetic: output, dx, the four dW and db of fixture (a); and leaving one dilation out is far outside the bound."""
    g = golden("g25_normal_head")
    (out, dx, dws, db), (x, dy, ws, bs) = head64
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    checks = [("out", nchw(out).numpy(), g["a_out64"]), ("dx", C.sampled(nchw(dx), C.HEAD_SAMPLE).numpy(), g["a_dx64_sample"]),
              ("db", db.numpy(), g["a_db64_0"])]
    checks += [(f"dW{i}", C.sampled(dws[i], C.HEAD_W_SAMPLE).numpy(), g[f"a_dw64_{i}_sample"]) for i in range(len(C.DILATIONS))]
    for what, mine, ref in checks:
        e = rel_l2(mine, ref)
        print(f"{what}: conv_fp64 sum against the reference module {e:.3e}")
        assert e <= 5e-7, (what, e)
    short = C.sum_fwd64(x, ws[:3], bs[:3], C.DILATIONS[:3])
    assert rel_l2(nchw(short).numpy(), g["a_out64"]) > 1e-2
    assert R.flagged(short, out, "f16x2") and not R.flagged(out.float(), out, "f16x2")


def _cfg(device="cpu", classifier="normal"):
    return types.SimpleNamespace(MODEL=types.SimpleNamespace(NAME=C.MODEL, CLASSIFIER=classifier, LOAD=None, MULTI_LEVEL=True),
                                 OTHERS=types.SimpleNamespace(DEVICE=device))


def test_tree_keys_init_and_optimizer_walk_match_fixture_b(golden, normal_head):
    from onda_amd.framework.handlers import get_model
    g = golden("g25_normal_head")
    torch.manual_seed(0)
    m = get_model(_cfg(), C.CLASSES)
    sd = m.state_dict()
    assert list(sd) == list(g["b_keys"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(g["b_shapes"])
    assert [str(v.dtype) for v in sd.values()] == list(g["b_dtypes"])
    assert [n for n, p in m.named_parameters() if p.requires_grad] == list(g["b_trainable"])
    assert m.feat is False and bool(g["b_feat_flag"]) is False
    for level in (m.layer5, m.layer6):
        assert isinstance(level, normal_head.ClassifierModule) and len(level.conv2d_list) == 4
        assert [(c.dilation[0], c.padding[0], c.kernel_size[0]) for c in level.conv2d_list] == [(d, d, 3) for d in C.DILATIONS]
    # same construction order and init recipe: one torch seed gives the reference's initial values (every conv N(0, 0.01))
    mean = np.array([float(v.double().mean()) for v in sd.values()])
    std = np.array([float(v.double().std()) if v.numel() > 1 else 0.0 for v in sd.values()])
    np.testing.assert_allclose(mean, g["b_init_mean"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(std, g["b_init_std"], rtol=1e-6, atol=1e-9)
    head_w = sd["layer6.conv2d_list.3.weight"]
    assert abs(float(head_w.std()) - 0.01) < 2e-4 and abs(float(head_w.mean())) < 2e-4
    name_of = {id(p): n for n, p in m.named_parameters()}
    groups = m.optim_parameters(2.5e-4)
    assert len(groups) == 2
    for gi, group in enumerate(groups):
        assert [name_of[id(p)] for p in group["params"]] == list(g[f"b_group{gi}"])
        assert group["lr"] == pytest.approx(float(g[f"b_group{gi}_lr"]))
    # the summed convolutions are packed by the head's own cache, never by the model's packer
    assert all(getattr(c, "_onda_sum_packed", False) for c in m.layer6.conv2d_list)
    import copy
    twin = copy.deepcopy(m.layer6)
    assert twin._pack is not m.layer6._pack and list(twin.state_dict()) == list(m.layer6.state_dict())


def test_rejection_stands_without_the_switch_and_lifts_with_it(capsys):
    from onda_amd.framework.model import deeplabv2
    was = deeplabv2.enable_normal_classifier(False)
    try:
        for name in ("normal", "something else"):
            with pytest.raises(NotImplementedError, match="enable_normal_classifier"):
                deeplabv2.get_deeplab_v2(19, True, [3, 4, 6, 3], name)
        assert deeplabv2.enable_normal_classifier(True) is False
        m = deeplabv2.get_deeplab_v2(19, True, [3, 4, 6, 3], "normal")
        assert isinstance(m.layer6, deeplabv2.ClassifierModule) and not m.feat
        assert "ADVENT CLF" not in capsys.readouterr().out
        m = deeplabv2.get_deeplab_v2(19, False, [3, 4, 6, 3], "anything")
        assert isinstance(m.layer6, deeplabv2.ClassifierModule) and not hasattr(m, "layer5")
        assert "Using default ADVENT CLF" in capsys.readouterr().out
        proda = deeplabv2.get_deeplab_v2(19, True, [3, 4, 6, 3], "ProDA")
        assert proda.feat and isinstance(proda.layer6, deeplabv2.Classifier_Module2)
        # the head refuses CPU tensors like every other op of the library
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.layer6(torch.zeros(1, 4, 4, 2048))
        assert deeplabv2.enable_normal_classifier(False) is True
        with pytest.raises(NotImplementedError):
            deeplabv2.get_deeplab_v2(19, True, [3, 4, 6, 3])  # "normal" is the default argument
    finally:
        deeplabv2.enable_normal_classifier(was)


def test_environment_switch():
    """ONDA_NORMAL_HEAD=1 at import switches the head on; unset, it is off (what this test is about is a fresh interpreter)."""
    code = ("from onda_amd.framework.model import deeplabv2 as d; import sys; "
            "sys.stdout.write(str(d.enable_normal_classifier(False)))")
    for value, want in (("1", "True"), (None, "False")):
        env = {k: v for k, v in os.environ.items() if k != "ONDA_NORMAL_HEAD"}
        if value is not None:
            env["ONDA_NORMAL_HEAD"] = value
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 0 and out.stdout.strip() == want, (value, out.stdout, out.stderr[-500:])


def test_adaptation_methods_refuse_a_model_without_features(tmp_path):
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import da_model, evaluation
    from onda_amd.framework.domain_adaptation.methods.advent_da import advent
    from onda_amd.framework.domain_adaptation.methods.prototypes import online_proDA
    from onda_amd.framework.domain_adaptation.methods.prototypes_hybrid_switch import hybrid_proDA
    cfg, spec = hybrid_switch_cfg(128, 64, "cpu", str(tmp_path), batch_size=2)
    featless = types.SimpleNamespace(feat=False)
    for cls in (da_model, evaluation, advent, online_proDA, hybrid_proDA):
        with pytest.raises(NotImplementedError, match="segmentation.train"):
            cls(featless, cfg, spec)


def test_tap_order_and_route_rules():
    """ops.sum_taps: convolution by convolution, filter taps row-major, (dh, dw) = ((r - 1) * d, (s - 1) * d) for the head; the data
    gradient's offsets are the negated ones in the same order.  ops.sum_conv_route: the table route needs the switch, "f16x2",
    32-channel blocks on both sides and no predicate."""
    from onda_amd import ops
    geoms = tuple((3, d, d) for d in C.DILATIONS)
    taps = ops.sum_taps(geoms)
    assert len(taps) == 36 and taps[0] == (-6, -6) and taps[4] == (0, 0) and taps[9 + 5] == (0, 12) and taps[35] == (24, 24)
    assert ops.sum_taps(geoms, negate=True) == [(-a, -b) for a, b in taps]
    old = ops.TAP_CONV, ops.CONV_MODE
    try:
        ops.TAP_CONV, ops.CONV_MODE = True, "f16x2"
        assert ops.sum_conv_route(2048, 32) == "taps" and ops.sum_conv_route(2048, 19) == "chain" and ops.sum_conv_route(48, 32) == "chain"
        ops.CONV_MODE = "f32"
        assert ops.sum_conv_route(2048, 32) == "chain"
        ops.TAP_CONV, ops.CONV_MODE = False, "f16x2"
        assert ops.sum_conv_route(2048, 32) == "chain"
    finally:
        ops.TAP_CONV, ops.CONV_MODE = old
