"""CPU: the DeepLabv2-Resnet50-GN model as the handler builds it (against the G21 fixture captured from the reference), the C ABI
of the two GroupNorm-site calls, and the float64 restatement with its comparators on the new cases (tests/gn_site_fp64.py):
double-precision torch equals the restatement, float32 torch passes the comparators, every injected fault is rejected."""
import os
import re
import types
from copy import deepcopy

import pytest
import torch
from torch import nn

import gn_site_fp64 as S
import norm_fp64 as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda c: c.id  # noqa: E731


def _cfg(name):
    return types.SimpleNamespace(MODEL=types.SimpleNamespace(NAME=name, CLASSIFIER="ProDA", LOAD=None, MULTI_LEVEL=False),
                                 OTHERS=types.SimpleNamespace(DEVICE="cpu"))


@pytest.fixture(scope="module")
def model():
    from onda_amd.framework.handlers.model_handler import get_model
    return get_model(_cfg(S.GN_MODEL), 19)


# ------------------------------------------------------------------------------------------------ the model
def test_handler_builds_the_reference_module_tree(model, golden):
    g = golden("g21_gn_model")
    sd = model.state_dict()
    assert list(sd) == list(g["keys"]) and len(sd) == 361
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(g["shapes"])
    assert [str(v.dtype) for v in sd.values()] == list(g["dtypes"])
    n_gn = sum(isinstance(m, nn.GroupNorm) for m in model.modules())
    n_bn = sum(isinstance(m, nn.BatchNorm2d) for m in model.modules())
    assert [n_gn, n_bn, len(list(model.parameters())), len(list(model.buffers()))] == list(g["counts"]) == [17, 48, 217, 144]
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert trainable == list(g["trainable"]) and len(trainable) == 111
    sites = [n for n, m in model.named_modules() if isinstance(m, nn.GroupNorm) and not n.startswith(("layer5.", "layer6."))]
    assert sites == ["bn1"] + [f"layer{i}.0.downsample.1" for i in (1, 2, 3, 4)]
    for n in sites:
        m = model.get_submodule(n)
        assert m.num_groups == 32 and not any(p.requires_grad for p in m.parameters())
    assert [model.get_submodule(n).num_channels // 32 for n in sites] == [2, 8, 16, 32, 64]
    assert model.multi_level is False and hasattr(model, "layer5")


def test_deepcopy_and_state_dict_round_trip(model):
    from onda_amd.framework.handlers.model_handler import get_model
    from onda_amd.synthetic import fill_state_dict
    a = deepcopy(model)
    fill_state_dict(a, 3, 2.0)
    b = get_model(_cfg(S.GN_MODEL), 19)
    b.load_state_dict(a.state_dict())
    c = deepcopy(a)
    for (ka, va), (kb, vb), (kc, vc) in zip(a.state_dict().items(), b.state_dict().items(), c.state_dict().items()):
        assert ka == kb == kc and torch.equal(va, vb) and torch.equal(va, vc) and va.data_ptr() != vc.data_ptr()
    assert [p.requires_grad for p in a.parameters()] == [p.requires_grad for p in c.parameters()]
    # optim_parameters walks the tree as the reference does: the frozen stem / shortcut GroupNorms contribute nothing
    sites = [a.bn1] + [getattr(a, f"layer{i}")[0].downsample[1] for i in (1, 2, 3, 4)]
    frozen = {id(p) for m in sites for p in m.parameters()}
    groups = a.optim_parameters(0.1)
    assert frozen and not frozen & {id(p) for p in groups[0]["params"]}
    assert groups[1]["lr"] == pytest.approx(1.0)


def test_the_other_names_are_unchanged():
    from onda_amd.framework.handlers.model_handler import MODEL_NAMES, get_model
    assert MODEL_NAMES == ["DeepLabv2-Resnet50", "DeepLabv2-Resnet101", S.GN_MODEL]
    m = get_model(_cfg("DeepLabv2-Resnet50"), 19)
    assert not any(isinstance(x, nn.GroupNorm) for n, x in m.named_modules() if not n.startswith(("layer5.", "layer6.")))
    with pytest.raises(AssertionError):
        get_model(_cfg("DeepLabv2-Resnet101-ProDA"), 19)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_signatures_and_header_declare_the_site_calls():
    from onda_amd import _lib
    header = open(os.path.join(ROOT, "include", "onda_hip.h")).read()
    for name, nargs in (("onda_gn_site_ws", 3), ("onda_gn_site_fwd", 20), ("onda_gn_site_bwd", 17)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert decl is not None, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == nargs, name
    # the ASPP head's calls keep their ABI
    assert len(_lib.SIGNATURES["onda_gn_fwd"][1]) == 18 and len(_lib.SIGNATURES["onda_gn_bwd"][1]) == 20


# ------------------------------------------------------------------------------------------------ restatement and comparators
def test_cases_reach_what_they_are_named_for():
    for c in S.SITE_CASES:
        chunks = N.col_plan(c.B, c.H * c.W, c.C).chunks
        assert (chunks >= 2) == ("chunks2" in c.id), c.id
    assert {c.C // S.GROUPS for c in S.SITE_CASES} == {2, 8, 64}


@pytest.mark.parametrize("case", S.SITE_CASES, ids=ids)
def test_restatement_equals_double_torch(case):
    """2^-53 times the cancellation of the one-pass variance (kappa <= 257 at mean / std 16) and sums of at most 4096 terms is
    below 2e-10; the restatement and torch agree to that relative to each unit's scale, or one of them is not GroupNorm."""
    x, gamma, beta, dout = S.site_inputs(case)
    out, mean, rstd, dx, dg, db = S.torch_site(x, gamma, beta, dout, case.relu, torch.float64)
    ref = N.gn64([x], [gamma], [beta], None, case.relu, S.GROUPS)
    bw = N.gn_bwd64(ref, dout, (out > 0) if case.relu else None, S.GROUPS)
    rel = 2.0 ** -53 * 257 * 4096
    for what, a, b in (("out", out, ref.cat), ("mean", mean, ref.mean[0].reshape(-1)), ("rstd", rstd, ref.rstd[0].reshape(-1)),
                       ("dx", dx, bw.dx[0]), ("dgamma", dg, bw.dgamma[0]), ("dbeta", db, bw.dbeta[0])):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"{case.id} {what}: {err:.2e}")
        assert err <= rel, (what, err)


@pytest.mark.parametrize("case", S.SITE_CASES, ids=ids)
def test_float32_torch_passes_the_comparators(case):
    x, gamma, beta, dout = S.site_inputs(case)
    got = S.torch_site(x, gamma, beta, dout, case.relu, torch.float32)
    exempt = S.hold(got, x, gamma, beta, dout, case.relu, S.geometry(case), f"torch {case.id}")
    assert exempt <= N.EXEMPT_SHARE
    for what in sorted(N.MEASURED):
        if what.startswith("gn"):
            print(f"{case.id}: worst ratio to its bound: {what}: {N.MEASURED[what][0]:.3f}")


@pytest.mark.parametrize("fault,cid", [("pairs", "c64-relu"), ("pairs", "c64-relu-off16"), ("batch", "c64-relu"), ("batch", "c256"),
                                       ("nomask", "c64-relu"), ("nomask", "c64-chunks2")])
def test_comparators_reject_the_injected_faults(fault, cid):
    case = S.SITE_BY_ID[cid]
    x, gamma, beta, dout = S.site_inputs(case)
    good = S.torch_site(x, gamma, beta, dout, case.relu, torch.float64)
    assert not N.flagged(S.hold, good, x, gamma, beta, dout, case.relu, S.geometry(case), cid)
    bad = S.torch_site(x, gamma, beta, dout, case.relu, torch.float64, fault)
    if fault == "nomask":  # a backward fault: the forward comparator has nothing to say, the backward one must
        ref = N.gn64([x], [gamma], [beta], None, case.relu, S.GROUPS)
        assert not N.flagged(N.check_gn_forward, bad[0], [bad[1]], [bad[2]], ref, S.geometry(case), cid)
    assert N.flagged(S.hold, bad, x, gamma, beta, dout, case.relu, S.geometry(case), f"{fault} {cid}")
