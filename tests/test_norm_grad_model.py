"""GPU: ``get_deeplab_v2(19, True, [1, 1, 1, 1], "ProDA", norm_grad=True)`` -- the public argument that makes ``bn1`` and the four
``layerN.0.downsample.1`` trainable, ten parameters in all -- on a 2 x 3 x 65 x 129 batch, against the reference's run of the same
seeded model (fixture G27, tests/golden/make_golden_proda101.py): the ten parameters receive gradients (on the frozen-affine
BatchNorm routes they stayed None and ReplaySGD skipped them in silence), the gradients are the reference's float64 ones, one
ReplaySGD step moves the parameters as torch's SGD moves them, the folded eval-mode BatchNorm sees the step, and the paired
student pass gives the gradients of the two passes run one after the other.

Tolerance, per tensor in relative L2: MARGIN = 4 x the distance of the reference's own float32 run from its float64 run (both in
the fixture), 4 x u where that is smaller (proda101_cases.tolerance)."""
import numpy as np
import pytest
import torch

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
def f16x2():
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    yield
    ops.CONV_MODE = old


def build(**kw):
    from onda_amd.framework.model.deeplabv2 import get_deeplab_v2
    torch.manual_seed(P.SEED)
    m = get_deeplab_v2(19, True, [1, 1, 1, 1], "ProDA", **kw)
    m.multi_level = False
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
    return m.to(DEV).train()


def image():
    from onda_amd.synthetic import synth_batch
    return synth_batch(2, P.H, P.W)["image"].to(DEV)


def backward(m, x=None):
    from onda_amd import ops
    _, o = m(image() if x is None else x)
    ops.seg_losses(o["out"], S.labels().to(DEV), 1.0, 0.0, 0.0)[0].backward()
    return o


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def test_the_ten_parameters_receive_the_references_gradients(golden, conv_mode):
    g = golden("g27_norm_grad")
    m = build(norm_grad=True)
    names = list(g["names"])
    assert names == [n for n in P.bn_param_names(m) if dict(m.named_parameters())[n].requires_grad] and len(names) == 10
    backward(m)
    params = dict(m.named_parameters())
    assert all(params[n].grad is not None for n in names), [n for n in names if params[n].grad is None]
    # the blocks' BatchNorms stay frozen, as in the reference (its _make_layer never hands norm_grad on)
    assert all(p.grad is None for n, p in params.items() if ".bn" in n and not n.startswith("bn1."))
    failed = []
    for i, n in enumerate(names):
        e_ref = rel(g[f"g32_{i}"], g[f"g64_{i}"])
        e = rel(params[n].grad.cpu().numpy(), g[f"g64_{i}"])
        print(f"{conv_mode} {n}: {e:.3e} from float64 (the reference's float32 run: {e_ref:.3e}; ratio to the tolerance {e / P.tolerance(e_ref):.3f})")
        if e > P.tolerance(e_ref):
            failed.append((n, e, e_ref))
    assert not failed, failed


def test_one_replay_sgd_step_moves_them_as_torch_moves_them(golden, conv_mode):
    from onda_amd.optim import ReplaySGD
    g = golden("g27_norm_grad")
    m = build(norm_grad=True)
    names = list(g["names"])
    params = dict(m.named_parameters())
    lr = float(g["lr"])
    opt = ReplaySGD(m.optim_parameters(lr), lr=lr, momentum=0.9, weight_decay=5e-4)
    backward(m)
    versions = {n: params[n]._version for n in names}
    opt.step()
    for i, n in enumerate(names):
        before, after = g[f"before_{i}"].astype(np.float64), g[f"after_{i}"].astype(np.float64)
        mine = params[n].detach().cpu().numpy().astype(np.float64)
        assert np.abs(after - before).max() > 0
        e_ref = rel(g[f"g32_{i}"], g[f"g64_{i}"])
        # the update is a multiple of (gradient + weight decay * value), applied to the value in float32: the gradient's
        # tolerance on the update, two roundings on the value
        bar = P.tolerance(e_ref) * np.linalg.norm(after - before) + 2 * P.U * np.linalg.norm(after)
        err = np.linalg.norm(mine - after)
        print(f"{conv_mode} {n}: update {np.linalg.norm(after - before):.3e}, off by {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (n, err, bar)
        assert params[n]._version > versions[n], f"{n}: the optimizer's launch did not bump the version"


def test_eval_forward_after_the_step_uses_the_new_affine_parameters(conv_mode):
    """Everything keyed on gamma / beta sees them move: the folded scale / shift of HipBatchNorm2d (and the bound cache behind it)
    follow the optimizer's raw-pointer writes.  The step is restricted to the ten BatchNorm parameters, so nothing else can explain
    a changed output."""
    from copy import deepcopy
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.optim import ReplaySGD
    m = build(norm_grad=True)
    x = image()
    m.eval()
    with torch.no_grad():
        before = m(x)[1]["out"].clone()
        folds = {n: mod.folded() for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)}
    m.train()
    switch_batch_statistics(m, False)  # (the train pass must not move the running statistics: only gamma / beta change)
    backward(m, x)
    ten = [p for n, p in m.named_parameters() if n in set(P.bn_param_names(m)) and p.requires_grad]
    assert len(ten) == 10
    ReplaySGD([{"params": ten}], lr=0.5, momentum=0.9, weight_decay=0.0).step()
    m.eval()
    with torch.no_grad():
        after = m(x)[1]["out"].clone()
        fresh = deepcopy(m)  # (HipBatchNorm2d.__deepcopy__ drops the fold and the bound cache: folded anew)
        for mod in fresh.modules():
            assert "_fold" not in mod.__dict__ and "_bound_cache" not in mod.__dict__
        again = fresh(x)[1]["out"]
    assert float((after - before).abs().max()) > 0, "the eval forward did not see the step"
    assert torch.equal(after, again), "the eval forward after the step is not that of a freshly folded copy"
    changed = [n for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) and mod.folded()[0] is not folds[n][0]]
    assert sorted(changed) == sorted(["bn1"] + [f"layer{i}.0.downsample.1" for i in range(1, 5)])


def test_paired_student_pass_gives_the_gradients_of_the_two_passes(golden, f16x2):
    """ops.row_groups over the concatenated batches against one pass per batch (gradients accumulated by autograd): the same ten
    gradients.  Both are float32 evaluations the first test holds to 4 x max(e_ref, u) of float64: their distance is held to twice
    that (triangle inequality)."""
    from onda_amd import ops
    from onda_amd.synthetic import synth_batch
    if not ops.row_groups_supported():
        pytest.skip("row groups exist in the f16x2 / dma configuration only")
    g = golden("g27_norm_grad")
    names = list(g["names"])
    xs = [synth_batch(2, P.H, P.W, seed=s)["image"].to(DEV) for s in (7, 8)]
    labels = S.labels().to(DEV)

    def run(paired):
        m = build(norm_grad=True)
        if paired:
            with ops.row_groups(2):
                out = m(torch.cat(xs, 0))[1]["out"]
            loss = ops.seg_losses(out[:2], labels, 1.0, 0.0, 0.0)[0] + ops.seg_losses(out[2:], labels, 1.0, 0.0, 0.0)[0]
            loss.backward()
        else:
            for x in xs:
                ops.seg_losses(m(x)[1]["out"], labels, 1.0, 0.0, 0.0)[0].backward()
        p = dict(m.named_parameters())
        return {n: p[n].grad.cpu().numpy() for n in names}

    a, b = run(True), run(False)
    for i, n in enumerate(names):
        e_ref = rel(g[f"g32_{i}"], g[f"g64_{i}"])
        e = rel(a[n], b[n])
        print(f"{n}: paired against two passes {e:.3e} (bar {2 * P.tolerance(e_ref):.3e})")
        assert e <= 2 * P.tolerance(e_ref), (n, e, e_ref)


def test_the_gn_model_keeps_giving_its_five_sites_gradients(conv_mode):
    """GroupNorm at the stem and the four shortcuts with norm_grad=True already trained through ops.GNSiteFn: it stays so."""
    m = build(norm_grad=True, norm_module=lambda *k, **x: torch.nn.GroupNorm(32, *k, **x))
    sites = ["bn1"] + [f"layer{i}.0.downsample.1" for i in range(1, 5)]
    assert all(isinstance(m.get_submodule(s), torch.nn.GroupNorm) for s in sites)
    backward(m)
    for s in sites:
        mod = m.get_submodule(s)
        for p in (mod.weight, mod.bias):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, s
