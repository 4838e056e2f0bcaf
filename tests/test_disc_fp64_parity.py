"""GPU, "f16x2" mode: ADVENT's discriminator on the HIP conv path (ops.disc_conv: onda_s2d_split_h2, the library's 2x2 stride-1
pre-split convolution in all three directions, onda_d2s_bwd) against the float64 restatement of tests/disc_fp64.py -- per layer,
the two rearrangement kernels on their own, the backward passes that must not be launched, the whole discriminator against the
float32 module chain, one advent.step, and the entry points' argument checks.  Every test prints its figures before it asserts."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import conv_fp64 as C64
import disc_fp64 as D

DEV = "cuda:0"
MODE = "f16x2"
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def f16x2_mode(monkeypatch):
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, MODE
    monkeypatch.setenv("ONDA_DISC", "hip")  # the route under test (the shipped default is the module chain)
    yield
    ops.CONV_MODE = old


@functools.lru_cache(maxsize=None)
def _layer_reference(case):
    return D.layer_reference(case)


def _wgrad_chain(M, cout, cin):
    """K-steps (32 pixels each) one weight-gradient workgroup accumulates at this shape: the pixel range of one split."""
    from onda_amd import ops
    sk = ops._wgrad_splitk(M, D.up32(cout), D.up32(4 * cin), 4, True)
    return -(-(-(-M // sk)) // 32), sk


# ------------------------------------------------------------------------------------------------ per layer
@pytest.mark.parametrize("case", D.LAYER_CASES, ids=D.case_id)
def test_layer_against_fp64(case):
    from onda_amd import ops
    layer, cin, cout, H, W, slope, nchw = case
    x, w, b, dy = D.layer_inputs(case)
    ref_y, ref_dx, ref_dw, ref_db = _layer_reference(case)
    xin = (x.permute(0, 3, 1, 2).contiguous() if nchw else x).to(DEV).requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = ops.disc_conv(xin, wd, bd, slope, nchw=nchw)
    assert tuple(y.shape) == (2, H // 2, W // 2, cout)  # (Cout = 1: the 31 padded output channels are not handed out)
    y.backward(dy.to(DEV))
    dx = xin.grad.permute(0, 2, 3, 1) if nchw else xin.grad
    assert tuple(wd.grad.shape) == (cout, cin, 4, 4) and tuple(bd.grad.shape) == (cout,)
    M = 2 * (H // 2) * (W // 2)
    chain, sk = _wgrad_chain(M, cout, cin)
    what = D.case_id(case)
    # an input pixel that no output reads has a data gradient of exactly 0 (4x4 / 2 / 1 reaches every pixel of these sizes but
    # the mask is applied all the same: it is what a leaked border would violate first)
    unreached = C64.dgrad_unreached((H, W), 4, 2, 1, 1, (H // 2, W // 2))[None, :, :, None]
    figs = [C64.check(y.detach().cpu(), ref_y, MODE, what + " forward"),
            C64.check(dx.cpu(), ref_dx, MODE, what + " data gradient", exact=[(0.0, unreached)]),
            C64.check(wd.grad.cpu(), ref_dw, MODE, what + " weight gradient", kind="wgrad", bounds=C64.chain_bounds(MODE, chain)),
            # the column sum adds M terms in float32: a chain of M (chain_bounds' rule), not of M / 32
            C64.check(bd.grad.cpu().reshape(1, -1), ref_db.reshape(1, -1), MODE, what + " bias gradient",
                      bounds=C64.chain_bounds(MODE, M))]
    print(what, f"M {M} split-K {sk} chain {chain}:", " | ".join(f"{n} {t:.2e}/{bl:.2e}" for n, (t, bl) in zip(
        ("fwd", "dgrad", "wgrad", "bias"), figs)))
    if slope != 1.0:  # where the planted input is exactly 0 the derivative is `slope`, not 1 (and not 0)
        zero = x == 0
        assert int(zero.sum()) > 100 and int((x < 0).sum()) > 100
        r = D.rel_l2(dx.cpu()[zero], ref_dx[zero])
        print(what, f"data gradient on the {int(zero.sum())} planted zeros: {r:.2e}")
        assert r <= C64.BOUNDS[MODE][0]
        assert float(ref_dx[zero].abs().max()) > 0


# ---------------------------------------------------------------------------------- the two rearrangement kernels alone
@pytest.mark.parametrize("case", D.LAYER_CASES[:2], ids=D.case_id)
def test_split_pass_writes_the_border_and_the_padded_channels_as_zeros(case):
    """S as onda_s2d_split_h2 leaves it (rebuilt from the limb rows) against the float64 S: the two-limb representation holds
    22 bits below the tensor's maximum; border positions and the channels 4C..Cp are exactly 0."""
    from onda_amd import ops
    from onda_amd.ops import disc as odisc
    layer, cin, cout, H, W, slope, nchw = case
    x = D.layer_inputs(case)[0]
    xin = (x.permute(0, 3, 1, 2).contiguous() if nchw else x).to(DEV)
    S = ops.materialize(odisc.s2d_split(xin, nchw, slope)[1]).cpu()
    want = D.s2d_input(D.lrelu(x.double(), slope))
    assert tuple(S.shape) == tuple(want.shape) == (2, H // 2 + 1, W // 2 + 1, D.up32(4 * cin))
    err = float((S.double() - want).abs().max())
    print(D.case_id(case), f"max |S - fp64| {err:.2e}, max |x| {float(x.abs().max()):.2f}")
    assert err <= 2.0 ** -21 * float(x.abs().max())
    assert int((S[want == 0] != 0).sum()) == 0  # border, padded channels (and the planted zeros)
    assert int((want[..., 4 * cin:] != 0).sum()) == 0 and int((want[:, 0, :, :2 * cin] != 0).sum()) == 0


@pytest.mark.parametrize("case", D.LAYER_CASES[:2], ids=D.case_id)
def test_way_back_drops_the_border_and_applies_the_derivative_exactly(case):
    """onda_d2s_bwd on a gradient of S whose border positions and padded channels hold 3.0: the fp32 output is a gather and at
    most one float32 product, so it equals torch's bit for bit; nothing of the border arrives.  The limb rows hold the same
    values to 22 bits below the bound max|gs|."""
    from onda_amd import ops
    from onda_amd.ops import disc as odisc
    layer, cin, cout, H, W, slope, nchw = case
    x = D.layer_inputs(case)[0]
    Hs, Ws, Cp = H // 2 + 1, W // 2 + 1, D.up32(4 * cin)
    g = torch.Generator().manual_seed(9)
    gs = torch.randn(2, Hs, Ws, Cp, generator=g)
    live = D.s2d_input(torch.ones(2, H, W, cin)) != 0
    gs[~live] = 3.0
    want = D.d2s_grad(gs.double(), torch.ones_like(x), 1.0).float()  # the gather alone
    if slope != 1.0:
        want = torch.where(x > 0, want, want * torch.tensor(slope, dtype=torch.float32))
    gsd = gs.to(DEV)
    gamax = ops.amax_slot(gsd.device)
    ops.call("onda_absmax", gsd.data_ptr(), 2 * Hs * Ws, Cp, Cp, gamax.data_ptr(), ops._stream())
    xin = (x.permute(0, 3, 1, 2).contiguous() if nchw else x).to(DEV)
    mask = xin if slope != 1.0 else None
    if nchw:
        dx = odisc.d2s_bwd(gsd, gamax, mask, True, (2, cin, H, W), slope, True).permute(0, 2, 3, 1)
        assert torch.equal(dx.cpu(), want)
        return
    dx = odisc.d2s_bwd(gsd, gamax, mask, False, (2, cin, H, W), slope, True)
    assert torch.equal(dx.cpu(), want)
    only = odisc.d2s_bwd(gsd, gamax, mask, False, (2, cin, H, W), slope, False)
    assert ops.is_limb_only(only)
    for t in (dx, only):
        lb = ops.limbs_of(t)
        rebuilt = ops.materialize(ops.limb_only((2, H, W, cin), gsd.device, lb)).cpu()
        err = float((rebuilt.double() - want.double()).abs().max())
        print(D.case_id(case), f"limb rows: max |dx - gather| {err:.2e}")
        assert err <= 2.0 ** -21 * 3.0


# ------------------------------------------------------------------------------------------------ needs_input_grad
def _spies(monkeypatch):
    from onda_amd.ops import conv as oconv
    seen = {"wgrad": 0, "dgrad": 0}
    real_w, real_d = oconv.conv_wgrad, oconv.conv_dgrad

    def wgrad(*a, **k):
        seen["wgrad"] += 1
        return real_w(*a, **k)

    def dgrad(*a, **k):
        seen["dgrad"] += 1
        return real_d(*a, **k)
    monkeypatch.setattr(oconv, "conv_wgrad", wgrad)
    monkeypatch.setattr(oconv, "conv_dgrad", dgrad)
    return seen


def _disc(state=None):
    from onda_amd.framework.model.discriminator import get_fc_discriminator
    d = get_fc_discriminator(19)
    d.load_state_dict(state or D.disc_weights())
    return d.train().to(DEV)


def test_backward_launches_only_what_is_asked_for(monkeypatch):
    from onda_amd.framework.utils.func import bce_loss
    seen = _spies(monkeypatch)
    d = _disc()
    x = D.disc_map(2, 64, 128).to(DEV)
    assert d.hip_path(x)
    for p in d.parameters():  # the adversarial pass: frozen parameters, the gradient goes into the map
        p.requires_grad = False
    xin = x.clone().requires_grad_(True)
    bce_loss(d(xin), 0).backward()
    print("frozen parameters:", seen)
    assert seen == {"wgrad": 0, "dgrad": 5} and xin.grad is not None and all(p.grad is None for p in d.parameters())
    seen.update(wgrad=0, dgrad=0)
    for p in d.parameters():  # the discriminator pass: a detached map, layer 0 has no data gradient to compute
        p.requires_grad = True
    bce_loss(d(x.detach()), 1).backward()
    print("detached map:", seen)
    assert seen == {"wgrad": 5, "dgrad": 4} and all(p.grad is not None for p in d.parameters())
    seen.update(wgrad=0, dgrad=0)
    with torch.no_grad():
        y = d(x)
    assert tuple(y.shape) == (2, 1, 2, 4) and not y.requires_grad


def test_forward_and_backward_never_reach_torch_conv2d(monkeypatch):
    """The discriminator's convolutions run on the library: with torch's conv2d taken away, forward and backward still work."""
    from onda_amd.framework.utils.func import bce_loss

    def no_conv(*a, **k):
        raise AssertionError("torch.nn.functional.conv2d was called")
    monkeypatch.setattr(F, "conv2d", no_conv)
    d = _disc()
    xin = D.disc_map(2, 64, 128).to(DEV).requires_grad_(True)
    y = d(xin)
    assert tuple(y.shape) == (2, 1, 2, 4)
    bce_loss(y, 0).backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xin.grad).all()) and float(xin.grad.abs().max()) > 0
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in d.parameters())


# ------------------------------------------------------------------------------------------------ the whole discriminator
def _disc_grads(state, x, monkeypatch, route, frozen=False):
    from onda_amd.framework.utils.func import bce_loss
    monkeypatch.setenv("ONDA_DISC", route)
    d = _disc(state)
    for p in d.parameters():
        p.requires_grad = not frozen
    xin = x.to(DEV).requires_grad_(True)
    assert d.hip_path(xin) == (route == "hip")
    loss = bce_loss(d(xin), 0)
    loss.backward()
    out = {"loss": loss.detach().cpu().reshape(1), "map": xin.grad.cpu()}
    out.update({k: p.grad.cpu() for k, p in d.named_parameters() if not frozen})
    return out


@pytest.mark.parametrize("shape", ((2, 64, 128), (1, 34, 38)), ids=("2x64x128", "1x34x38"))
def test_whole_discriminator_against_fp64_and_the_float32_chain(shape, monkeypatch):
    """bce_loss(D(map), 0): the gradients with respect to the map and the ten parameters against the chained float64
    restatement.  Five layers' errors compound and no per-layer bound says how, so the yardstick is the route the HIP chain
    replaces -- the float32 module chain on the same weights (ONDA_DISC=torch): per tensor the HIP chain's relative L2 must
    be at most max(2 x that chain's, 5 x BOUNDS' tensor bound) -- 2: two correct float32 evaluations with different summation
    orders differ by about that; 5: one per-layer bound per layer."""
    state = D.disc_weights()
    x = D.disc_map(*shape)
    ref_loss, ref_dx, ref_grads = D.disc_reference(state, x)
    ref = dict(ref_grads, loss=ref_loss.reshape(1), map=ref_dx)
    hip = _disc_grads(state, x, monkeypatch, "hip")
    eager = _disc_grads(state, x, monkeypatch, "torch")
    floor = 5 * C64.BOUNDS[MODE][0]
    bad = []
    for k in ("loss", "map") + tuple(state):
        fh, ft = D.rel_l2(hip[k].reshape(ref[k].shape), ref[k]), D.rel_l2(eager[k].reshape(ref[k].shape), ref[k])
        bound = max(2 * ft, floor)
        print(f"{shape} {k:9s} hip {fh:.3e}  torch-f32 {ft:.3e}  bound {bound:.3e}")
        if not fh <= bound:
            bad.append(k)
    # the adversarial pass: frozen parameters, the gradient travels between the layers as limb rows only
    fa = D.rel_l2(_disc_grads(state, x, monkeypatch, "hip", frozen=True)["map"], ref["map"])
    ft = D.rel_l2(eager["map"], ref["map"])
    print(f"{shape} map, frozen parameters: hip {fa:.3e}  torch-f32 {ft:.3e}")
    assert not bad, bad
    assert fa <= max(2 * ft, floor)


# ------------------------------------------------------------------------------------------------ one advent.step
def _advent_step(tmp_path):
    """One advent.step at 64x128, batch 2, on seeded weights, batches and dropout masks: (log, head-conv gradient before
    optimizer.step(), d_main's first-layer gradient, that weight before and after its Adam step, lr)."""
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.framework.model import deeplabv2
    from onda_amd.synthetic import fill_state_dict, synth_batch
    from oracle import model as omodel
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, str(tmp_path), batch_size=2)
    cfg.METHOD.ADAPTATION.NAME = "ADVENT"
    for k, v in (("LAMBDA_SEG_MAIN", 1.0), ("LAMBDA_SEG_AUX", 0.1), ("LAMBDA_ADV_MAIN", 1.0), ("LAMBDA_ADV_AUX", 0.2)):
        spec[k] = v
    cfg.METHOD.ADAPTATION.ADVENT = spec
    model = get_model(cfg, 19)
    fill_state_dict(model, 1, 3.0)
    torch.manual_seed(77)  # the discriminators' initial weights
    da = get_adapt_method(cfg)(model, cfg, spec)
    torch.manual_seed(123)
    masks = iter([omodel.draw_drop_mask(2) for _ in range(4)])
    deeplabv2.drop_mask_fn = lambda B, C, p, dev: next(masks).to(dev)
    seen = {}
    head, first = model.layer6.head[1].weight, da.d_main[0].weight
    real_step, real_d_step = da.optimizer.step, da.optimizer_d_main.step

    def step_spy(*a, **k):
        seen["head_grad"] = head.grad.detach().clone()
        return real_step(*a, **k)

    def d_step_spy(*a, **k):
        seen["d_grad"], seen["d_before"] = first.grad.detach().clone(), first.detach().clone()
        return real_d_step(*a, **k)
    da.optimizer.step, da.optimizer_d_main.step = step_spy, d_step_spy
    try:
        da.optimizer.zero_grad()
        da.adjust_learning_rate(0, 6)
        log = da.step(synth_batch(2, 64, 128, seed=100), synth_batch(2, 64, 128, seed=200))
    finally:
        deeplabv2.drop_mask_fn = deeplabv2._default_drop_mask
    torch.cuda.synchronize()
    return ({k: v.item() for k, v in log.items()}, seen["head_grad"].cpu(), seen["d_grad"].cpu(), seen["d_before"].cpu(),
            first.detach().cpu().clone(), spec.LEARNING_RATE_D)


def test_advent_step_hip_discriminators_against_the_module_chain(tmp_path, monkeypatch):
    """The same step twice: discriminators on the HIP chain, and on the float32 module chain (ONDA_DISC=torch).  Each chain is
    within 5 x BOUNDS' tensor bound of float64 (the test above), the two of each other within twice that (triangle
    inequality): 1e-5 relative on the three log values and relative L2 on the head-conv gradient.  d_main.0.weight after Adam
    follows test_entropy_parity's rule: the first step is lr * g / (|g| + 1e-8), so elements whose gradient is above 1e-3 of
    the tensor's RMS move by lr to within 1 % in both runs, and no element can differ by more than two steps."""
    from onda_amd.ops import disc as odisc
    launches = []
    real = odisc.call
    monkeypatch.setattr(odisc, "call", lambda name, *a: (launches.append(name), real(name, *a))[1])
    hip = _advent_step(tmp_path)
    n_hip = len(launches)
    monkeypatch.setenv("ONDA_DISC", "torch")
    ref = _advent_step(tmp_path)
    assert n_hip > 0 and len(launches) == n_hip  # the first run took the HIP chain, the second one did not
    tol = 2 * 5 * C64.BOUNDS[MODE][0]
    for k in ("Discriminator loss", "Segmentation loss", "Adversarial loss"):
        print(f"{k}: hip {hip[0][k]:.9f}, torch {ref[0][k]:.9f}, rel {abs(hip[0][k] - ref[0][k]) / abs(ref[0][k]):.3e} (bound {tol:.1e})")
    print(f"head-conv gradient rel-L2 {D.rel_l2(hip[1], ref[1]):.3e} (bound {tol:.1e}), d_main.0 gradient rel-L2 {D.rel_l2(hip[2], ref[2]):.3e}")
    lr = hip[5]
    moved = (hip[4] - ref[4]).abs()
    big = ref[2].abs() > 1e-3 * ref[2].pow(2).mean().sqrt()
    ulp = 2.0 ** -23 * float(ref[4].abs().max())
    print(f"d_main.0 weight after Adam: max |diff| {float(moved.max()):.3e} (lr {lr:.1e}), on the decided elements {float(moved[big].max()):.3e}")
    assert set(hip[0]) == {"Discriminator loss", "Segmentation loss", "Adversarial loss"}
    for k in hip[0]:
        assert abs(hip[0][k] - ref[0][k]) <= tol * abs(ref[0][k]), k
    assert D.rel_l2(hip[1], ref[1]) <= tol
    assert torch.equal(hip[3], ref[3])  # the same initial discriminator
    assert float((hip[4] - hip[3]).abs().max()) > 0.5 * lr  # the step was taken
    assert float(moved[big].max()) <= 0.01 * lr + 2 * ulp
    assert float(moved.max()) <= 2 * lr + 2 * ulp


# ------------------------------------------------------------------------------------------------ argument checks
def test_entry_points_refuse_bad_arguments_before_launching():
    from onda_amd import _lib
    lib = _lib.load()
    EINVAL, EALIGN = -1, -2
    x = torch.zeros(1, 8, 8, 32, device=DEV)
    amax = torch.zeros(2048, device=DEV)
    dst = torch.zeros(5 * 5 * 2 * 128 + 16, device=DEV, dtype=torch.float16)
    gs = torch.zeros(1, 5, 5, 128, device=DEV)
    out = torch.zeros(1, 8, 8, 32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def s2d(xp=x.data_ptr(), nchw=0, C=32, slope=0.2, dp=dst.data_ptr(), ldx=32):
        return lib.onda_s2d_split_h2(xp, nchw, 1, C, 8, 8, ldx, slope, amax.data_ptr(), dp, s)

    def d2s(gp=gs.data_ptr(), xp=x.data_ptr(), C=32, slope=0.2, lp=dst.data_ptr(), fp=out.data_ptr(), nchw=0, ap=amax.data_ptr()):
        return lib.onda_d2s_bwd(gp, ap, xp, nchw, 1, C, 8, 8, 32, slope, lp, fp, s)
    assert s2d() == 0 and d2s() == 0
    assert s2d(dp=dst.data_ptr() + 2) == EALIGN and s2d(xp=x.data_ptr() + 4) == EALIGN
    assert d2s(lp=dst.data_ptr() + 2) == EALIGN and d2s(gp=gs.data_ptr() + 4) == EALIGN and d2s(fp=out.data_ptr() + 4) == EALIGN
    for bad in (float("nan"), float("inf"), -float("inf"), 1.5):
        assert s2d(slope=bad) == EINVAL and d2s(slope=bad) == EINVAL
    assert s2d(C=0) == EINVAL and d2s(C=0) == EINVAL
    assert s2d(C=0, nchw=1) == EINVAL and d2s(C=0, nchw=1, lp=None) == EINVAL
    assert s2d(C=12) == EINVAL and s2d(ldx=16) == EINVAL  # NHWC: 8-channel pieces, rows at least C floats long
    assert s2d(xp=None) == EINVAL and s2d(dp=None) == EINVAL and d2s(gp=None) == EINVAL
    assert d2s(lp=None, fp=None) == EINVAL and d2s(ap=None) == EINVAL and d2s(nchw=1) == EINVAL  # NCHW writes no limb rows
    assert lib.onda_s2d_split_h2(x.data_ptr(), 0, 1 << 20, 32, 128, 128, 32, 0.2, amax.data_ptr(), dst.data_ptr(), s) == EINVAL  # B*Hs*Ws >= 2^31
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and math.isfinite(float(dst.float().abs().max()))
