"""CPU: the float64 restatement of the discriminator layers (tests/disc_fp64.py) against torch autograd in float64, the
space-to-depth identity the HIP path rests on against the restatement, the comparator against injected faults and against a
float32 evaluation, and the module contract of get_fc_discriminator."""
import pytest
import torch
from torch import nn

import conv_fp64 as C64
import disc_fp64 as D

# ([B,C,H,W] of the issue, slope in front): the layer-0 shape, and an odd size -- Ho = floor((H - 2) / 2) + 1 = 8 for H = 17, one
# row fewer than the 2x2 conv over all ceil((H + 2) / 2) = 10 row pairs of the padded image gives
IDENTITY_CASES = ((0, 19, 64, 34, 38, 1.0, True), (2, 64, 128, 17, 19, D.SLOPE, False))
NAMES = ("forward", "data gradient", "weight gradient", "bias gradient")
TIGHT = 1e-12


def _inputs(case):
    return D.layer_inputs(case, batch=2 if case[1] == 19 else 1)


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=D.case_id)
def test_restatement_agrees_with_torch_autograd_in_float64(case):
    x, w, b, dy = _inputs(case)
    mine = (D.layer_fwd(x, w, b, case[5]),) + D.layer_bwd(x, w, dy, case[5])
    theirs = D.layer_torch(x, w, b, dy, case[5])
    assert tuple(mine[0].shape[1:3]) == ((case[3] - 2) // 2 + 1, (case[4] - 2) // 2 + 1)
    for name, a, t in zip(NAMES, mine, theirs):
        r = D.rel_l2(a, t)
        print(D.case_id(case), name, f"{r:.2e}")
        assert r <= TIGHT, name


@pytest.mark.parametrize("rows", ("kept", "all"))
@pytest.mark.parametrize("case", IDENTITY_CASES, ids=D.case_id)
def test_space_to_depth_identity(case, rows):
    """rows="all": S with every row pair of the padded image -- for the odd size the 2x2 conv then has one output row and
    column more than the layer, which are discarded, and the last row pair of S gets a gradient of exactly zero."""
    x, w, b, dy = _inputs(case)
    ref = (D.layer_fwd(x, w, b, case[5]),) + D.layer_bwd(x, w, dy, case[5])
    got = D.layer_s2d(x, w, b, dy, case[5], rows=rows)
    for name, a, t in zip(NAMES, got, ref):
        r = D.rel_l2(a, t)
        print(D.case_id(case), rows, name, f"{r:.2e}")
        assert a.shape == t.shape and r <= TIGHT, name
    H = case[3]
    S = D.s2d_input(D.lrelu(x.double(), case[5]), rows)
    assert S.shape[1] == (H // 2 + 1 if rows == "kept" else -(-(H + 2) // 2)) and S.shape[3] == D.up32(4 * case[1])
    assert float(S[..., 4 * case[1]:].abs().max() if S.shape[3] > 4 * case[1] else 0.0) == 0.0
    if rows == "all" and H % 2 == 1:
        assert float(S[:, -1].abs().max()) == 0.0  # the last row pair is border only: nothing of the image is discarded with it


def test_comparator_flags_each_injected_fault_and_passes_float32():
    """The faults of the HIP path's two rearrangement kernels, each far above BOUNDS["f16x2"]; torch in float32 far below."""
    bound = C64.BOUNDS["f16x2"][0]
    for case in IDENTITY_CASES:
        x, w, b, dy = _inputs(case)
        slope = case[5]
        ref = (D.layer_fwd(x, w, b, slope),) + D.layer_bwd(x, w, dy, slope)
        f32 = D.layer_torch(x, w, b, dy, slope, torch.float32)
        for name, a, t, kind in zip(NAMES, f32, ref, ("act", "act", "wgrad", "act")):
            t = t.reshape(1, -1) if name == "bias gradient" else t
            a = a.reshape(1, -1) if name == "bias gradient" else a
            m = C64.measure(a, t, kind)
            print(D.case_id(case), "float32", name, f"{m[0]:.2e} / {m[1]:.2e}")
            assert not C64.flagged(a, t, "f16x2", kind), name
        faults = {"swapped (py, px)": dict(order="xy"), "missing border": dict(border=False)}
        if 4 * case[1] % 32:
            faults["dropped padded-channel block"] = dict(drop_block=4 * case[1] // 32)
        else:
            faults["dropped last channel block"] = dict(drop_block=4 * case[1] // 32 - 1)
        for what, kw in faults.items():
            got = D.layer_s2d(x, w, b, dy, slope, **kw)
            for name, a, t, kind in zip(NAMES[:3], got, ref, ("act", "act", "wgrad")):
                r = D.rel_l2(a, t)
                print(D.case_id(case), what, name, f"{r:.2e}")
                assert r > 1000 * bound and C64.flagged(a, t, "f16x2", kind), (what, name)
        if slope != 1.0:
            got = D.layer_s2d(x, w, b, dy, slope, zero_rule=1.0)
            r = D.rel_l2(got[1], ref[1])
            print(D.case_id(case), "derivative 1 at x == 0", f"{r:.2e}")
            assert int((x == 0).sum()) > 0 and r > 1000 * bound and C64.flagged(got[1], ref[1], "f16x2")


def test_chained_reference_is_autograd_in_float64():
    """disc_reference (layer_fwd / layer_bwd chained, the BCE by hand) against autograd through the float64 modules."""
    from onda_amd.framework.model.discriminator import get_fc_discriminator
    from onda_amd.framework.utils.func import bce_loss
    state = D.disc_weights()
    x = D.disc_map(1, 34, 38)
    d = get_fc_discriminator(19)
    d.load_state_dict(state)
    d = d.double()
    xd = x.double().requires_grad_(True)
    loss = nn.BCEWithLogitsLoss()(d(xd), torch.zeros(1, 1, 1, 1, dtype=torch.float64))
    loss.backward()
    ref_loss, ref_dx, ref_grads = D.disc_reference(state, x)
    loss = loss.detach()
    assert abs(float(loss) - float(ref_loss)) <= TIGHT * abs(float(loss))
    assert D.rel_l2(ref_dx, xd.grad) <= TIGHT
    for k, p in d.named_parameters():
        assert D.rel_l2(ref_grads[k].reshape(p.shape), p.grad) <= TIGHT, k
    with torch.no_grad():
        assert float(bce_loss(d(xd).float(), 0)) == pytest.approx(float(loss), rel=1e-6)


# ------------------------------------------------------------------------------------------------ the module contract
def _plain(seed):
    torch.manual_seed(seed)
    widths, layers = D.WIDTHS, []
    for cin, cout in zip(widths, widths[1:]):
        if layers:
            layers.append(nn.LeakyReLU(negative_slope=0.2, inplace=True))
        layers.append(nn.Conv2d(cin, cout, kernel_size=4, stride=2, padding=1))
    return nn.Sequential(*layers)


def test_cpu_forward_is_the_module_chain_bit_for_bit(monkeypatch):
    from onda_amd.framework.model.discriminator import get_fc_discriminator
    monkeypatch.delenv("ONDA_DISC", raising=False)
    plain = _plain(77)
    torch.manual_seed(77)
    d = get_fc_discriminator(19)
    after = torch.rand(3)
    _plain(77)
    assert torch.equal(after, torch.rand(3))  # the same draws from the generator at construction
    assert isinstance(d, nn.Sequential) and [type(m) for m in d] == [type(m) for m in plain]
    for (k, a), (k2, b) in zip(d.state_dict().items(), plain.state_dict().items()):
        assert k == k2 and torch.equal(a, b)
    x = D.disc_map(2, 64, 128)
    assert not d.hip_path(x)
    assert torch.equal(d(x), plain(x))
    assert tuple(d[0].weight.shape) == (64, 19, 4, 4)


def test_onda_disc_torch_is_honoured(monkeypatch):
    """hip_path() is the decision `forward` takes; the conditions are probed with a stand-in for a GPU tensor's predicates."""
    from onda_amd import ops
    from onda_amd.framework.model.discriminator import get_fc_discriminator
    d = get_fc_discriminator(19)
    x = D.disc_map(1, 32, 32)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ops, "CONV_MODE", "f16x2")
    monkeypatch.delenv("ONDA_DISC", raising=False)
    assert not d.hip_path(x)  # the shipped default is the module chain (docs/experiments.md, "Discriminator convolutions")
    monkeypatch.setenv("ONDA_DISC", "hip")
    assert d.hip_path(x)
    monkeypatch.setenv("ONDA_DISC", "torch")
    assert not d.hip_path(x)
    monkeypatch.setenv("ONDA_DISC", "hip")
    assert not d.hip_path(x.double()) and not d.hip_path(x[0]) and not d.hip_path(x[:, :18]) and not d.hip_path(x[:, :, :31])
    monkeypatch.setattr(ops, "CONV_MODE", "f32")
    assert not d.hip_path(x)
