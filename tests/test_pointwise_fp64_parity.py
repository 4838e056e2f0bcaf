"""GPU: the SE gate (colsum pooling, onda_se_fc_fwd, onda_chan_scale, onda_chan_scale_limbs, onda_se_fc_bwd) and the ceil-mode
max-pool, held to the float64 restatement of tests/pointwise_fp64.py stage by stage and unit by unit with the bounds derived
there.  Every stage's reference starts from what the device itself fed to that stage.  The wrappers (ops.SEScaleFn, ops.MaxPoolFn)
must then reproduce the checked sequence bit for bit.  The cases are the smallest that reach each code path
(tests/test_pointwise_fp64_reference.py asserts that they do)."""
import types

import pytest
import torch

import norm_fp64 as N
import pointwise_fp64 as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ids = lambda c: c.id  # noqa: E731
TABLE = {}  # (quantity, case and mode) -> worst ratio to its bound
OURS = ("se ", "pool ")


@pytest.fixture(params=["f32", "f16x2"])
def conv_mode(request):
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, request.param
    for k in [k for k in N.MEASURED if k.startswith(OURS)]:  # (what the CPU file's runs of the comparators left behind)
        del N.MEASURED[k]
    yield request.param
    ops.CONV_MODE = old
    for k in [k for k in N.MEASURED if k.startswith(OURS)]:
        TABLE[(k, request.node.callspec.id)] = N.MEASURED.pop(k)[0]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for what in sorted({k for k, _ in TABLE}):
        row = ", ".join(f"{label} {r:.3f}" for (k, label), r in sorted(TABLE.items()) if k == what)
        print(f"worst ratio to its bound: {what}: {row}")


# ------------------------------------------------------------------------------------------------ SE
def _nan(*shape, dtype=torch.float32):
    """An output buffer that shows what a kernel did not write."""
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _se_stages(inp, case):
    """The sequence ops.SEScaleFn issues, call by call; every stage's value on the CPU, x / dout as [B, HW, C]."""
    from onda_amd import ops
    from onda_amd._lib import call
    p, s = ops._p, ops._stream()
    B, C, R, H, W = case.B, case.C, case.R, case.H, case.W
    HW = H * W
    x, dout = inp.x.reshape(B, H, W, C).to(DEV), inp.dout.reshape(B, H, W, C).to(DEV)
    w1, b1, w2, b2 = (t.to(DEV) for t in (inp.w1, inp.b1, inp.w2, inp.b2))
    pooled = ops.colsum(x, alpha=1.0 / HW, per_image=True)
    hidden, gate = _nan(B, R), _nan(B, C)
    call("onda_se_fc_fwd", p(pooled), p(w1), p(b1), p(w2), p(b2), p(hidden), p(gate), B, C, R, s)
    out = _nan(B, H, W, C)
    call("onda_chan_scale", p(x), p(gate), None, p(out), B, HW, C, s)
    limb = bound = None
    if ops.limb_mode(C):
        slot = ops.activation_scale(x)
        planes = torch.zeros(2, B * HW, C, device=DEV, dtype=torch.float16)
        call("onda_chan_scale_limbs", p(x), p(gate), p(planes), B * HW * C, p(slot), B, HW, C, s)
        limb = ops.materialize(ops.limb_only((B, H, W, C), x.device, ops.Limbs(planes, slot, C, B * HW * C))).cpu().reshape(B, HW, C)
        bound = float(slot.max())
    dgate = ops.colsum(dout, x, per_image=True)
    dw1, db1, dw2, db2, dpooled, ws = _nan(R, C), _nan(R), _nan(C, R), _nan(C), _nan(B, C), _nan(B * R)
    call("onda_se_fc_bwd", p(dgate), p(pooled), p(hidden), p(gate), p(w1), p(w2), p(dw1), p(db1), p(dw2), p(db2), p(dpooled), p(ws),
         1.0 / HW, B, C, R, s)
    dx = _nan(B, H, W, C)
    call("onda_chan_scale", p(dout), p(gate), p(dpooled), p(dx), B, HW, C, s)
    torch.cuda.synchronize()
    v = types.SimpleNamespace(x=inp.x, w1=inp.w1, b1=inp.b1, w2=inp.w2, b2=inp.b2, dout=inp.dout, pooled=pooled.cpu(),
                              hidden=hidden.cpu(), gate=gate.cpu(), out=out.cpu().reshape(B, HW, C), dgate=dgate.cpu(), dw2=dw2.cpu(),
                              db2=db2.cpu(), dpre1=ws.cpu().reshape(B, R), dw1=dw1.cpu(), db1=db1.cpu(), dpooled=dpooled.cpu(),
                              dx=dx.cpu().reshape(B, HW, C))
    return v, limb, bound


def _se_wrapper(inp, case, known_scale):
    """ops.SEScaleFn forward and backward on the same tensors: (out materialised, dx, dw1, db1, dw2, db2, limb-only?)."""
    from onda_amd import ops
    B, C, H, W = case.B, case.C, case.H, case.W
    xd = inp.x.reshape(B, H, W, C).to(DEV).requires_grad_(True)
    ps = [t.to(DEV).requires_grad_(True) for t in (inp.w1, inp.b1, inp.w2, inp.b2)]
    if known_scale:  # the producer left max|x| behind (GroupNorm's apply pass does): the gated result exists as limb rows only
        ops.activation_scale(xd)
    out = ops.SEScaleFn.apply(xd, *ps)
    limb_only = ops.is_limb_only(out)
    mat = ops.materialize(out).detach().cpu().reshape(B, H * W, C)
    out.backward(inp.dout.reshape(B, H, W, C).to(DEV))
    torch.cuda.synchronize()
    return [mat, xd.grad.cpu().reshape(B, H * W, C)] + [t.grad.cpu() for t in ps], limb_only


@pytest.mark.parametrize("case", P.SE_CASES, ids=ids)
def test_se_block_stage_by_stage(case, conv_mode):
    from onda_amd import ops
    inp = P.se_case_inputs(case)
    where = f"{case.id} {conv_mode}"
    v, limb, bound = _se_stages(inp, case)
    assert (limb is not None) == (conv_mode == "f16x2")
    exempt, _ = P.check_se(v, where, inp.planted)
    assert exempt == 0, f"{where}: {exempt} hidden units exempt from the sign check"
    if limb is not None:
        P.check_limbs(limb, v.out, bound, where)
        assert bound == float(inp.x.abs().max())
    # what the structure of a case makes exact
    if case.id == "kink":
        for name in ("pooled", "hidden", "dpre1", "out", "dgate", "dpooled"):
            assert bool((getattr(v, name)[1] == 0).all()), f"{where}: {name} of the all-zero image is not exactly 0"
        assert limb is None or bool((limb[1] == 0).all())
        # dgate = 0 there, so nothing comes back through the pooling: dx is the rounded product alone
        assert torch.equal(v.dx[1], inp.dout[1] * v.gate[1][None, :]), f"{where}: dx of the all-zero image is not fl(dout * gate)"
        assert bool((v.dpooled[0] != 0).any())
    if case.id == "saturated":
        g = v.gate
        assert bool((g[:, 0] == 1).all()) and bool((g[:, 2] == 1).all()) and bool((g[:, 3] == 0).all())
        assert bool(((g[:, 1] > 0) & (g[:, 1] < 1e-10)).all())
        for ch in (0, 2, 3):  # gate * (1 - gate) = 0 in every image: nothing reaches b2 and w2 there
            assert float(v.db2[ch]) == 0 and bool((v.dw2[ch] == 0).all()), f"{where}: dpre2 of a saturated gate is not exactly 0"
    if case.id == "one-hot-dout":
        for b in range(case.B):
            others = torch.arange(case.H * case.W) != P.one_hot_pixel(b, case.H * case.W)
            assert torch.equal(v.dx[b][others], v.dpooled[b][None, :].expand(int(others.sum()), -1)), \
                f"{where}: dx away from the one pixel with a gradient is not the pooled-gradient term"
    # the wrapper issues that sequence: bit for bit, with and without the limb output
    for known_scale in ((False, True) if ops.limb_mode(case.C) else (False,)):
        got, limb_only = _se_wrapper(inp, case, known_scale)
        assert limb_only == known_scale
        want = [limb if limb_only else v.out, v.dx, v.dw1, v.db1, v.dw2, v.db2]
        for name, a, b in zip(("out", "dx", "dw1", "db1", "dw2", "db2"), got, want):
            assert torch.equal(a, b), f"{where}: SEScaleFn's {name} (limb output: {limb_only}) is not what the checked sequence gave"
    # and a second run gives the same bits
    v2, limb2, _ = _se_stages(inp, case)
    for name in P.STAGES:
        assert torch.equal(getattr(v, name), getattr(v2, name)), f"{where}: {name} differs between two runs"
    assert limb is None or torch.equal(limb, limb2)


# ------------------------------------------------------------------------------------------------ max-pool
def _pool(x, dy, limbs):
    from onda_amd import ops
    xd = x.to(DEV).requires_grad_(True)
    if limbs:
        ops.activation_scale(xd)  # max|x| known, as behind BatchNorm + ReLU
    y = ops.MaxPoolFn.apply(xd, limbs)
    assert ops.is_limb_only(y) == limbs
    (idx,) = y.grad_fn.saved_tensors
    mat = ops.materialize(y).detach().cpu()
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    return mat, idx.cpu(), xd.grad.cpu()


@pytest.mark.parametrize("nonfinite", [False, True], ids=["finite", "nonfinite"])
@pytest.mark.parametrize("case", P.POOL_CASES, ids=ids)
def test_maxpool_ceil_bit_for_bit(case, nonfinite, conv_mode):
    from onda_amd import ops
    x, dy = P.pool_case_inputs(case, nonfinite)
    ref = P.maxpool_scan(x, dy)
    where = f"{case.id} {conv_mode}"
    y, idx, dx = _pool(x, dy, False)
    P.check_pool(y, idx, dx, ref, where)
    y2, idx2, dx2 = _pool(x, dy, False)
    assert P.same_bits(y, y2) and torch.equal(idx, idx2) and P.same_bits(dx, dx2), f"{where}: two runs differ"
    if not nonfinite and case.C % 32 == 0 and ops.limb_mode(case.C):
        # the result as limb rows: the values to the format's floor, the same slots, so the same dx bit for bit
        yl, idxl, dxl = _pool(x, dy, True)
        P.check_limbs(yl, ref.y, float(x.abs().max()), where, "pool limbs")
        P.check_pool(ref.y, idxl, dxl, ref, where + " limbs")
