"""CPU: the DeepLabv2-Resnet101-ProDA mirror (onda_amd/framework/model/deeplabv2_proda.py) against the reference's tree (fixture
G26, tests/golden/make_golden_proda101.py): the same state_dict keys in the same order, shapes, ``requires_grad`` flags, seeded
initial weights and parameter-group multiplicities; the opt-in of the handler; ``freeze_bn`` / ``bn_clr``; that nothing is ever
fetched; the checkpoint formats; the drop-in alias; the one-GPU rule for trainable BatchNorm affine parameters; and the C ABI of
the affine BatchNorm entry points."""
import os
import re
import sys
import tempfile
import types
import warnings
from unittest import mock

import numpy as np
import pytest
import torch
from torch import nn

import proda101_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(**kw):
    from onda_amd.framework.model.deeplabv2_proda import Deeplab
    torch.manual_seed(P.SEED)
    # (an empty hub directory: a cached ImageNet file in the user's own must not reach the seeded model)
    with warnings.catch_warnings(), tempfile.TemporaryDirectory() as home, mock.patch.dict(os.environ, {"TORCH_HOME": home}):
        warnings.simplefilter("ignore")
        return Deeplab(nn.BatchNorm2d, num_classes=19, **kw)


@pytest.fixture(scope="module")
def model():
    return build()


@pytest.fixture
def empty_hub(tmp_path, monkeypatch):
    """TORCH_HOME at an empty directory, and every way torch has of downloading a checkpoint made to raise."""
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    calls = []

    def refuse(*a, **k):
        calls.append(a)
        raise AssertionError("a download was attempted")

    import torch.hub
    import torch.utils.model_zoo
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", refuse)
    monkeypatch.setattr(torch.hub, "download_url_to_file", refuse)
    monkeypatch.setattr(torch.utils.model_zoo, "load_url", refuse)
    assert torch.hub.get_dir() == os.path.join(str(tmp_path), "hub")
    return tmp_path, calls


def _digest(t, n=P.DIGEST):
    f = t.detach().double().cpu().reshape(-1)
    idx = (torch.arange(n, dtype=torch.int64) * f.numel()) // n
    return np.concatenate([[f.sum().item(), f.abs().sum().item()], f[idx].numpy()])


# ------------------------------------------------------------------------------------------------ the tree
def test_tree_is_the_references(golden, model):
    from onda_amd.framework.model.deeplabv2 import HipBatchNorm2d
    g = golden("g26_proda101")
    assert int(g["seed"]) == P.SEED
    sd = model.state_dict()
    assert list(sd) == list(g["keys"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(g["shapes"])
    assert [str(v.dtype) for v in sd.values()] == list(g["dtypes"])
    names = [n for n, _ in model.named_parameters()]
    assert names == list(g["param_names"])
    assert [p.requires_grad for _, p in model.named_parameters()] == list(g["requires_grad"]) and all(g["requires_grad"])
    counts = [len(sd), len(names), sum(isinstance(x, nn.BatchNorm2d) for x in model.modules()), sum(isinstance(x, nn.GroupNorm) for x in model.modules())]
    assert counts == list(g["counts"]) == [653, 341, 104, 6]
    assert all(isinstance(x, HipBatchNorm2d) for x in model.modules() if isinstance(x, nn.BatchNorm2d))
    assert not hasattr(model, "layer6") and model.multi_level is False and model.feat


def test_seeded_init_is_the_references(golden, model):
    """The construction order and the init recipe: the same seed gives the reference's initial weights, tensor by tensor."""
    g = golden("g26_proda101")
    for (k, v), ref in zip(model.state_dict().items(), g["digests"]):
        mine = _digest(v)
        assert np.array_equal(mine[2:], ref[2:]), k
        assert np.allclose(mine[:2], ref[:2], rtol=1e-12, atol=0), k
    # what the reference's init loops actually reach: every conv weight N(0, 0.01) -- the head's too --, BatchNorm at (1, 0)
    w = model.layer5.head[1].weight.detach()
    assert 0.005 < float(w.std()) < 0.02
    assert float(model.layer5.bottleneck[1].weight.detach().std()) < 0.02
    assert all(bool((m.weight == 1).all()) and bool((m.bias == 0).all()) for m in model.modules() if isinstance(m, nn.BatchNorm2d))


def test_parameter_groups_are_the_references(golden, model):
    g = golden("g26_proda101")
    by_id = {id(p): i for i, (_, p) in enumerate(model.named_parameters())}
    groups = model.optim_parameters(2.5e-4)
    assert [grp["lr"] for grp in groups] == [2.5e-4, 2.5e-3]
    for k, grp in enumerate(groups):
        count = np.zeros(len(by_id), dtype=np.int64)
        for p in grp["params"]:
            count[by_id[id(p)]] += 1
        assert np.array_equal(count, g[f"group{k}_count"]), k
    assert int(g["group0_count"].sum()) == 942 and int((g["group0_count"] > 0).sum()) == 312 and int(g["group1_count"].sum()) == 29
    assert len(list(model.get_1x_lr_params())) == 942 and len(list(model.get_10x_lr_params())) == 29
    # adjust_learning_rate: the reference's poly rule on both groups
    from onda_amd.optim import ReplaySGD
    opt = ReplaySGD(model.optim_parameters(1.0), lr=1.0)
    model.adjust_learning_rate(types.SimpleNamespace(learning_rate=1.0, num_steps=10, power=0.9), opt, 5)
    assert opt.param_groups[0]["lr"] == pytest.approx(0.5 ** 0.9) and opt.param_groups[1]["lr"] == pytest.approx(10 * 0.5 ** 0.9)


def test_freeze_bn_freezes_exactly_the_batchnorm_parameters():
    m = build(freeze_bn=True)
    bn = set(P.bn_param_names(m))
    assert len(bn) == 208
    for n, p in m.named_parameters():
        assert p.requires_grad == (n not in bn), n
    assert len({id(p) for p in m.get_1x_lr_params()}) == 312 - 208


def test_bn_clr_raises():
    from onda_amd.framework.model.deeplabv2_proda import Bottleneck, Deeplab, ResNet101
    with pytest.raises(NotImplementedError, match="bn_clr"):
        Deeplab(nn.BatchNorm2d, num_classes=19, bn_clr=True)
    with pytest.raises(NotImplementedError, match="bn_clr"):
        ResNet101(Bottleneck, [1, 1, 1, 1], 19, nn.BatchNorm2d, bn_clr=True)


# ------------------------------------------------------------------------------------------------ the handler
def _cfg(name):
    return types.SimpleNamespace(MODEL=types.SimpleNamespace(NAME=name, CLASSIFIER="ProDA", LOAD=None, MULTI_LEVEL=True),
                                 OTHERS=types.SimpleNamespace(DEVICE="cpu"))


def test_default_registry_rejects_the_fourth_name():
    from onda_amd.framework.handlers import model_handler as H
    assert H.MODEL_NAMES == ["DeepLabv2-Resnet50", "DeepLabv2-Resnet101", "DeepLabv2-Resnet50-GN"]
    with pytest.raises(AssertionError):
        H.get_model(_cfg(P.PRODA_MODEL), 19)


def test_opt_in_gives_the_references_names_and_builds_the_model(empty_hub):
    from onda_amd.framework import handlers
    from onda_amd.framework.handlers import model_handler as H
    from onda_amd.framework.model.deeplabv2_proda import ResNet101
    names = H.MODEL_NAMES
    before = list(names)
    assert H.enable_resnet101_proda() is False
    try:
        assert H.MODEL_NAMES is names and names == ["DeepLabv2-Resnet50", "DeepLabv2-Resnet101", P.PRODA_MODEL, "DeepLabv2-Resnet50-GN"]
        assert H.enable_resnet101_proda() is True
        cfg = _cfg(P.PRODA_MODEL)
        with pytest.warns(UserWarning, match="resnet101-5d3b4d8f.pth"):
            m = handlers.get_model(cfg, 19)
        assert isinstance(m, ResNet101) and cfg.MODEL.MULTI_LEVEL is False and m.multi_level is False
        assert m.layer5.head[1].out_channels == 19 and len(m.state_dict()) == 653
        assert all(p.requires_grad for p in m.parameters())
    finally:
        assert H.enable_resnet101_proda(False) is True
    assert H.MODEL_NAMES is names and names == before
    with pytest.raises(AssertionError):
        H.get_model(_cfg(P.PRODA_MODEL), 19)


def test_environment_switch_at_import():
    import subprocess
    code = ("from onda_amd.framework.handlers.model_handler import MODEL_NAMES; "
            "assert MODEL_NAMES == ['DeepLabv2-Resnet50', 'DeepLabv2-Resnet101', 'DeepLabv2-Resnet101-ProDA', 'DeepLabv2-Resnet50-GN'], MODEL_NAMES")
    env = dict(os.environ, ONDA_RESNET101_PRODA="1", PYTHONPATH=ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)


# ------------------------------------------------------------------------------------------------ no network, ever
def test_nothing_is_fetched_and_one_warning_names_the_file(empty_hub):
    from onda_amd.framework.model import deeplabv2_proda as M
    assert not hasattr(M, "model_zoo") and "model_zoo" not in open(M.__file__).read().split('"""', 2)[2]
    tmp, calls = empty_hub
    torch.manual_seed(P.SEED)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = M.Deeplab(nn.BatchNorm2d, num_classes=19)
    mine = [x for x in w if "resnet101-5d3b4d8f.pth" in str(x.message)]
    assert len(mine) == 1 and os.path.join(str(tmp), "hub", "checkpoints") in str(mine[0].message)
    assert not calls
    # the seeded init is kept
    torch.manual_seed(P.SEED)
    ref = M.ResNet101(M.Bottleneck, [3, 4, 23, 3], 19, nn.BatchNorm2d)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), ref.state_dict().values()))


def test_a_cached_file_is_loaded(empty_hub):
    from onda_amd.framework.model import deeplabv2_proda as M
    tmp, calls = empty_hub
    os.makedirs(os.path.join(str(tmp), "hub", "checkpoints"))
    g = torch.Generator().manual_seed(1)
    cached = {"conv1.weight": torch.randn(64, 3, 7, 7, generator=g), "bn1.running_var": torch.rand(64, generator=g) + 1,
              "layer3.22.bn2.weight": torch.randn(256, generator=g), "fc.weight": torch.randn(1000, 2048, generator=g)}
    torch.save(cached, M.pretrained_path())
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the file is there: no warning
        m = M.Deeplab(nn.BatchNorm2d, num_classes=19)
    sd = m.state_dict()
    for k in ("conv1.weight", "bn1.running_var", "layer3.22.bn2.weight"):
        assert torch.equal(sd[k], cached[k]), k
    assert "fc.weight" not in sd and not calls
    assert float(sd["layer5.head.1.weight"].std()) < 0.02  # what the file does not hold keeps its init


def test_initialization_and_restore_from_read_the_references_formats(empty_hub, tmp_path):
    from onda_amd.framework.model import deeplabv2_proda as M
    g = torch.Generator().manual_seed(2)
    init = {"state_dict": {"conv1.weight": torch.randn(64, 3, 7, 7, generator=g), "fc.bias": torch.randn(1000, generator=g)}}
    ipath = str(tmp_path / "init.pth")
    torch.save(init, ipath)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # with initialization= the hub directory is not even looked at
        m = M.Deeplab(nn.BatchNorm2d, num_classes=19, initialization=ipath)
    assert torch.equal(m.state_dict()["conv1.weight"], init["state_dict"]["conv1.weight"])
    # restore_from: the whole state, written by one model and read by another
    src = build()
    with torch.no_grad():
        for p in src.parameters():
            p.add_(0.25)
    rpath = str(tmp_path / "restore.pth")
    torch.save({"ResNet101": {"model_state": src.state_dict()}}, rpath)
    m = M.Deeplab(nn.BatchNorm2d, num_classes=19, initialization=ipath, restore_from=rpath)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), src.state_dict().values()))
    assert not empty_hub[1]


# ------------------------------------------------------------------------------------------------ drop-in, one GPU, C ABI
def test_dropin_aliases_the_module():
    import onda_amd.dropin as dropin
    saved = {k: v for k, v in sys.modules.items() if k == "framework" or k.startswith("framework.")}
    try:
        dropin.install()
        from framework.model.deeplabv2_proda import Deeplab, ResNet101
        import onda_amd.framework.model.deeplabv2_proda as mine
        assert Deeplab is mine.Deeplab and ResNet101 is mine.ResNet101
    finally:
        for k in [k for k in sys.modules if k == "framework" or k.startswith("framework.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_trainable_affine_is_refused_with_several_ranks(monkeypatch, tmp_path):
    from onda_amd import dist as odist
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import da_model
    from onda_amd.framework.domain_adaptation.methods.segmentation import SegmentationTrainer
    from onda_amd.framework.model import deeplabv2
    trainable = deeplabv2.get_deeplab_v2(19, False, [1, 1, 1, 1], "ProDA", norm_grad=True)
    frozen = deeplabv2.get_deeplab_v2(19, False, [1, 1, 1, 1], "ProDA")
    assert deeplabv2.trains_bn_affine(trainable) and not deeplabv2.trains_bn_affine(frozen)
    assert deeplabv2.trains_bn_affine(build()) and not deeplabv2.trains_bn_affine(build(freeze_bn=True))
    cfg, spec = hybrid_switch_cfg(128, 64, "cpu", str(tmp_path), batch_size=2)
    deeplabv2.require_single_gpu_affine(trainable, "a test")  # one rank: nothing to refuse
    monkeypatch.setattr(odist, "is_on", lambda: True)
    with pytest.raises(NotImplementedError, match="flat-buffer gradient exchange is untested"):
        da_model(trainable, cfg, spec)
    with pytest.raises(NotImplementedError, match="flat-buffer gradient exchange is untested"):
        SegmentationTrainer(trainable, cfg, spec)
    deeplabv2.require_single_gpu_affine(frozen, "a test")  # frozen models are unaffected
    # the exchange's name filter: the auxiliary head that never runs, never the ProDA model's main head
    frozen.multi_level = False
    skip = deeplabv2.unused_head_skip(frozen)
    assert skip("layer5.head.1.weight") and not skip("layer6.head.1.weight")
    assert deeplabv2.unused_head_skip(build(freeze_bn=True)) is None


def test_signatures_and_header_declare_the_affine_calls():
    from onda_amd import _lib
    header = open(os.path.join(ROOT, "include", "onda_hip.h")).read()
    new = (("onda_bn_bwd_affine", 18), ("onda_bn_bwd_affine_l2", 22), ("onda_bn_pair_bwd_affine_l2", 14))
    old = (("onda_bn_bwd", 14), ("onda_bn_bwd_l2", 20), ("onda_bn_pair_bwd_l2", 10), ("onda_bn_bwd_ws", 2), ("onda_bn_bwd_l2_ws", 2),
           ("onda_bn_pair_bwd_l2_ws", 2), ("onda_bn_train_l2", 25), ("onda_bn_pair_fwd_l2", 12))
    for name, nargs in new + old:
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\n(?:int|int64_t) %s\(([^;]*)\);" % name, header)  # (the declaration, not a mention in a comment)
        assert decl is not None, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == nargs, name
    # an affine call is its frozen call plus the gradient pointers (and, on the fp32 route, the previous group's workspace)
    for (a, na), (f, nf), extra in zip(new, old[:3], (4, 2, 4)):
        assert na == nf + extra
        assert _lib.SIGNATURES[a][1][:nf - 1] == _lib.SIGNATURES[f][1][:nf - 1]
