"""CPU: which blocks take the BatchNorm pair route (framework/model/deeplabv2.py pair_route / conv_bn_pair -> ops.BNPairLimbFn).
Every Bottleneck.forward of a model is called with conv_bn and conv_bn_pair replaced by recorders, so no kernel runs: the four
shortcut blocks layerN.0 of the BatchNorm model in train mode take the pair and nothing else does -- no identity block, no block
of the GroupNorm model, nothing in eval mode, in the exact-fp32 conv mode, with the switch off, or with the limb outputs off."""
import pytest
import torch

SHORTCUT_BLOCKS = ["layer1.0", "layer2.0", "layer3.0", "layer4.0"]


def _model(gn):
    from onda_amd.framework.model.deeplabv2 import get_deeplab_v2
    kw = {"norm_module": (lambda *k, **x: torch.nn.GroupNorm(32, *k, **x))} if gn else {}
    return get_deeplab_v2(num_classes=19, multi_level=True, layers=[3, 4, 6, 3], classifier="ProDA", **kw)


def _routes(model, monkeypatch):
    """(names of the blocks whose forward called conv_bn_pair, conv_bn calls with a residual) over all Bottleneck blocks."""
    from onda_amd.framework.model import deeplabv2
    paired, residual_sites = [], []
    current = [None]

    def fake_conv_bn(conv, bn, x, relu, residual=None):
        if residual is not None:
            residual_sites.append(current[0])
        return x

    def fake_pair(conv_a, bn_a, x_a, conv_b, bn_b, x_b, relu):
        block = dict(model.named_modules())[current[0]]
        assert conv_a is block.conv3 and bn_a is block.bn3 and conv_b is block.downsample[0] and bn_b is block.downsample[1] and relu is True
        paired.append(current[0])
        return x_a

    monkeypatch.setattr(deeplabv2, "conv_bn", fake_conv_bn)
    monkeypatch.setattr(deeplabv2, "conv_bn_pair", fake_pair)
    x = torch.zeros(1, 2, 2, 8)
    blocks = [(n, m) for n, m in model.named_modules() if isinstance(m, deeplabv2.Bottleneck)]
    assert len(blocks) == 16
    for name, block in blocks:
        current[0] = name
        block(x)
    return paired, residual_sites


@pytest.fixture
def flags():
    from onda_amd import ops
    old = ops.CONV_MODE, ops.BN_PAIR, ops.LIMB_ONLY
    ops.CONV_MODE, ops.BN_PAIR, ops.LIMB_ONLY = "f16x2", True, True
    yield ops
    ops.CONV_MODE, ops.BN_PAIR, ops.LIMB_ONLY = old


def test_batchnorm_model_pairs_exactly_its_four_shortcut_blocks(flags, monkeypatch):
    model = _model(gn=False).train()
    paired, residual_sites = _routes(model, monkeypatch)
    assert paired == SHORTCUT_BLOCKS
    assert len(residual_sites) == 12 and not set(residual_sites) & set(SHORTCUT_BLOCKS)  # the identity blocks, as before


def test_groupnorm_model_pairs_nothing(flags, monkeypatch):
    model = _model(gn=True).train()
    paired, residual_sites = _routes(model, monkeypatch)
    assert paired == [] and len(residual_sites) == 16


@pytest.mark.parametrize("what", ["eval", "f32", "switch-off", "fp32-outputs", "one-side-eval"])
def test_everything_else_keeps_the_two_calls(flags, monkeypatch, what):
    model = _model(gn=False).train()
    if what == "eval":
        model.eval()
    elif what == "f32":
        flags.CONV_MODE = "f32"
    elif what == "switch-off":
        flags.BN_PAIR = False
    elif what == "fp32-outputs":
        flags.LIMB_ONLY = False
    else:
        for name in SHORTCUT_BLOCKS:
            dict(model.named_modules())[name].downsample[1].eval()
    paired, residual_sites = _routes(model, monkeypatch)
    assert paired == [] and len(residual_sites) == 16


@pytest.mark.parametrize("value,want", [("0", False), ("1", True), (None, True)])
def test_switch_reads_the_environment(monkeypatch, value, want):
    """ONDA_BN_PAIR=0 turns the route off where ops/_state.py is first read; anything else leaves it on.  (The module's text is
    run in a namespace of its own: the live switches stay as they are.)"""
    import runpy
    from onda_amd.ops import _state
    if value is None:
        monkeypatch.delenv("ONDA_BN_PAIR", raising=False)
    else:
        monkeypatch.setenv("ONDA_BN_PAIR", value)
    assert runpy.run_path(_state.__file__)["BN_PAIR"] is want
