"""GPU: the BatchNorm pair of a shortcut block -- out = relu(BN_a(y_a) + BN_b(y_b)) in one pass each way (csrc/norm_l2.hip
bn_finalize_pair / bn_apply_pair / bn_bwd_reduce_pair / bn_bwd_sums_pair / bn_bwd_apply_pair, ops.BNPairLimbFn) -- held to the
float64 restatement of tests/norm_fp64.py with the populations, tolerances and exempt cap derived there.

Both conv outputs come out of real 1x1 convolutions with four stat rows, as in test_norm_fp64_parity.py.  Restatement: side b is
``bn64`` without residual or ReLU; side a is ``bn64`` with ``res=`` side b's float64 output and the ReLU.  TOLERANCE of the output:
``bn_out_tol`` of side a (its ``res_amax`` term carries the roundings of the add on side b's magnitude, plus the limb floor of
the one tensor that is written) PLUS ``bn_out_tol`` of side b without a limb floor: side a's bound takes its residual as given,
but here the residual is itself a BatchNorm whose statistics carry their own error (e_xhat of side b, amplified off-centre); the
two-function route meets the same sum, and a limb floor for the shortcut tensor on top.  Gradients: each side against
``bn_bwd64`` with the kernel's own mask and ``bn_dx_tol`` of that side.

Shapes: the smallest at which a pair kernel takes another path -- fewer items than a wave (the partial-wave `whole = false`
stores), more channel columns than one workgroup of the reduction, two row groups with the boundary on and off a conv tile row
and with group 0 inside the one straddling tile row (no partial row of its own), and one tensor of more than two grid strides
(the element-wise grids are capped at 4096 workgroups: only there does the two-items-per-trip loop run, with a tail, and the walk
get cut at the group boundary mid-way)."""
import numpy as np
import pytest
import torch

import norm_fp64 as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class PairCase:
    def __init__(self, id, C, shape, first=0, track=True, on_tile=None):
        self.id, self.C, self.shape, self.first, self.track, self.on_tile = id, C, shape, first, track, on_tile


CASES = [
    PairCase("c32-m70", 32, (2, 5, 7)),                                   # 280 items: the last wave is not whole
    PairCase("c256-m70", 256, (2, 5, 7), track=False),
    PairCase("c64-m1683", 64, (3, 33, 17)),                               # several conv tile rows, 13464 items = 210.4 waves
    PairCase("c2048-m260", 2048, (1, 13, 20)),                            # 8 workgroup columns in the reduction
    PairCase("c64-rg-on-tile", 64, (3, 16, 16), first=1, on_tile=True),   # split = 256 rows: between two partial rows
    PairCase("c256-rg-straddle", 256, (4, 9, 17), first=1, on_tile=False),
    PairCase("c64-rg-short-chunk", 64, (5, 33, 41), first=2, on_tile=False, track=False),   # group 0's last chunk: 18 of 128 rows
    PairCase("c32-rg-one-tile", 32, (3, 5, 7), first=2, on_tile=False),   # group 0 lies inside the one (straddling) tile row
    PairCase("c64-rg-two-trips", 64, (2, 513, 257), first=1, on_tile=False),   # > 2 grid strides of items, cut at the boundary
]


def _supported():
    from onda_amd import ops
    return ops.CONV_MODE == "f16x2" and ops.H2_PATH == "dma" and ops.LIMB_ONLY


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for what in sorted(N.MEASURED):
        print(f"worst ratio to its bound: {what}: {N.MEASURED[what][0]:.3f} at {N.MEASURED[what][1]}")


def _side(M, C, seed, split):
    """Input, affine parameters, mixing weight and running buffers of one side, seeded."""
    x, gamma, beta = N.bn_input(M, C, seed, shift_rows=split)
    g = torch.Generator().manual_seed(seed + 2)
    w = torch.eye(C) + 1e-3 * torch.randn(C, C, generator=g) / C ** 0.5
    w[C - 2] = 0
    w[C - 2, C - 2] = 1  # the constant channel stays constant
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    return x, gamma, beta, w, rm, rv


def _run(case, sides, dout):
    """One forward + backward of ops.BNPairLimbFn behind two 1x1 convolutions; everything the checks take, on the CPU."""
    from onda_amd import ops
    from onda_amd.ops.limbs import _stat_tile_rows
    B, H, W = case.shape
    C, M = case.C, B * H * W
    ys, stats, running = [], [], []
    with ops.row_groups(case.first):
        for x, gamma, beta, w, rm, rv in sides:
            xd = x.reshape(B, H, W, C).to(DEV).requires_grad_(True)
            yd, st = ops.Conv2dFn.apply(xd, w.reshape(C, C, 1, 1).to(DEV), None, ops._PackCache(), 1, 1, 0, 4, None)
            assert st.shape[1] == 4
            ys.append(yd)
            stats.append(st)
            running.append((rm.to(DEV), rv.to(DEV), torch.zeros((), dtype=torch.int64, device=DEV)))
        assert ops.bn_pair_ok(ys[0], stats[0], ys[1], stats[1])
        args = []
        for i, (x, gamma, beta, w, rm, rv) in enumerate(sides):
            args += [ys[i], stats[i], gamma.to(DEV), beta.to(DEV), running[i] if case.track else None, N.MOMENTUM]
        zd = ops.BNPairLimbFn.apply(*args, True)
        assert ops.is_limb_only(zd)
        lb = ops.limbs_of(zd)
        node = zd.grad_fn
        stat, relu_mask = list(node.saved_tensors[4:]), node.relu_mask
        grads = torch.autograd.grad(zd, ys, dout.reshape(B, H, W, C).to(DEV))
        torch.cuda.synchronize()
    got = dict(out=ops.materialize(zd).cpu().reshape(M, C), out_planes=lb.planes.cpu(), bound=float(lb.amax.max()),
               mask=relu_mask.cpu(), y=[y.detach().cpu().reshape(M, C) for y in ys],
               stat=[t.cpu() for t in stat], tiles=[s.shape[0] for s in stats], bm=[_stat_tile_rows(s) for s in stats],
               dx=[ops.materialize(g).cpu().reshape(M, C) for g in grads], dx_planes=[ops.limbs_of(g).planes.cpu() for g in grads],
               dx_bound=[float(ops.limbs_of(g).amax.max()) for g in grads], running=[tuple(t.cpu() for t in r) for r in running])
    return got


def _geometry(case, got, i, M, split):
    tiles, bm = got["tiles"][i], got["bm"][i]
    if not split:
        return [(N.EPILOGUE_CHAIN, tiles)]
    assert (split % bm == 0) == case.on_tile, f"{case.id}: split {split}, statistic tiles of {bm} rows: not the case it is there for"
    return [(N.EPILOGUE_CHAIN, max(1, split // bm)), (N.EPILOGUE_CHAIN, tiles - split // bm)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_batchnorm_pair(case):
    if not _supported():
        pytest.skip("limb rows exist in the f16x2 / dma configuration only")
    B, H, W = case.shape
    C, M, split = case.C, B * H * W, case.first * H * W
    total8 = M * C // 8
    if case.id == "c64-rg-two-trips":
        assert 2 * 4096 * 256 < total8 < 3 * 4096 * 256 and 4096 * 256 < split * C // 8 < 2 * 4096 * 256
    else:
        assert N.ew_trips(total8, 4096) == 1
    seed = N.case_seed(case.id)
    sides = [_side(M, C, seed, split), _side(M, C, seed + 1000, split)]
    dout = torch.randn(M, C, generator=torch.Generator().manual_seed(seed + 7))
    got = _run(case, sides, dout)
    again = _run(case, sides, dout)
    groups = [(0, split), (split, M - split)] if split else None
    G = 2 if split else 1
    where = case.id

    # ---- fixed order: a second run gives the same bits everywhere
    assert torch.equal(got["out_planes"], again["out_planes"]) and got["bound"] == again["bound"] and torch.equal(got["mask"], again["mask"])
    for i in range(2):
        assert torch.equal(got["dx_planes"][i], again["dx_planes"][i]) and got["dx_bound"][i] == again["dx_bound"][i], f"{where}: side {i} dx"
        assert all(torch.equal(a, b) for a, b in zip(got["stat"], again["stat"]))

    # ---- forward
    (xa, gamma_a, beta_a, _, rm_a, rv_a), (xb, gamma_b, beta_b, _, rm_b, rv_b) = sides
    ya, yb = got["y"]
    assert bool((ya[:, C - 2] == ya[0, C - 2]).all()) and bool((yb[:, C - 2] == yb[0, C - 2]).all())
    ref_b = N.bn64(yb, gamma_b, beta_b, None, False, groups, (rm_b, rv_b, 0) if case.track else None)
    ref_a = N.bn64(ya, gamma_a, beta_a, ref_b.out, True, groups, (rm_a, rv_a, 0) if case.track else None)
    geo = [_geometry(case, got, i, M, split) for i in range(2)]
    refs = (ref_a, ref_b)
    for i in range(2):
        mean, invstd, xhat_amax = (t.reshape(G, C) for t in got["stat"][3 * i:3 * i + 3])
        N.check_bn_stats(mean, invstd, refs[i], geo[i], f"{where} side {'ab'[i]}", xhat_amax=xhat_amax)
    out, bound = got["out"], got["bound"]
    assert float(ref_a.out.abs().max()) <= bound * (1 + 1e-6), f"{where}: the limb bound {bound:.6e} is below the true maximum {float(ref_a.out.abs().max()):.6e}"
    assert float(out.abs().max()) <= bound * (1 + 1e-6), f"{where}: the limb bound {bound:.6e} is below the kernel's own maximum"
    tol = N.bn_out_tol(ref_a, geo[0], bound)[0] + N.bn_out_tol(ref_b, geo[1])[0]
    err = (out.double() - ref_a.out).abs()
    N._hold("bn pair out", torch.stack([err[r0:r0 + n].amax(0) for r0, n in ref_a.groups]), tol, where)
    t = N._rows(ref_a.groups, tol)
    clear = ref_a.pre.abs() > t
    wrong = clear & ((out > 0) != (ref_a.pre > 0))
    assert not bool(wrong.any()), f"{where}: {int(wrong.sum())} ReLU mask bits wrong away from the kink, first at {wrong.nonzero()[0].tolist()}"
    assert bool((out[ref_a.pre < -t] == 0).all()), f"{where}: non-zero output behind the ReLU"
    exempt = 1.0 - float(clear.double().mean())
    print(f"{where}: {100 * exempt:.4f} % of the elements within the tolerance of the kink")
    assert exempt <= N.EXEMPT_SHARE, f"{where}: {100 * exempt:.3f} % exempt from the mask check"
    bits = torch.from_numpy(np.unpackbits(got["mask"].numpy(), bitorder="little").reshape(M, C)).bool()
    mask = out > 0
    assert bool((bits == mask).all()), f"{where}: the saved bit mask is not [out > 0]"

    # ---- running buffers: moved by group 1's statistics (the last group of the restatement) or not at all
    for i, (rm, rv) in enumerate(((rm_a, rv_a), (rm_b, rv_b))):
        new = got["running"][i]
        if case.track:
            N.check_bn_running((new[0], new[1], int(new[2])), (rm, rv), refs[i], geo[i], f"{where} side {'ab'[i]}")
        else:
            assert torch.equal(new[0], rm) and torch.equal(new[1], rv) and int(new[2]) == 0, f"{where}: untracked running buffers moved"

    # ---- backward: the same masked gradient into both BatchNorms
    bgeo = [N.bn_geometry(n, C) for _, n in (groups or [(0, M)])]
    for i in range(2):
        side = f"{where} side {'ab'[i]}"
        bw = N.bn_bwd64(refs[i], dout, mask)
        dx, dx_bound = got["dx"][i], got["dx_bound"][i]
        N.check_bn_backward(dx, bw, refs[i], geo[i], bgeo, side, limb_bound=dx_bound)
        tol_dx = N.bn_dx_tol(refs[i], bw, geo[i], bgeo)
        assert float(dx.abs().max()) <= dx_bound * (1 + 1e-6), f"{side}: the dx bound {dx_bound:.6e} is below max|dx| {float(dx.abs().max()):.6e}"
        ref_max = torch.stack([bw.dx[r0:r0 + n].abs().amax(0) for r0, n in refs[i].groups])
        assert float((ref_max - tol_dx).max()) <= dx_bound * (1 + 1e-6), f"{side}: the dx bound {dx_bound:.6e} is below the reference's max|dx|"
        assert dx_bound <= 2.0 * float((bw.scale + tol_dx).max()), f"{side}: the dx bound {dx_bound:.6e} is more than twice its formula {float(bw.scale.max()):.6e}"


def test_pair_entry_points_refuse_what_their_kernels_cannot_run():
    """The ONDA_REQUIREs of the pair entry points: a channel count that is no multiple of 32, a split outside the rows, a ReLU
    without its mask, a side without its buffers."""
    from ctypes import byref
    from onda_amd import ops
    from onda_amd._lib import OndaBnSide, call
    p, s = ops._p, ops._stream()
    buf = [torch.zeros(8192, device=DEV) for _ in range(10)]

    def side(dx=True, partials=True):
        return OndaBnSide(p(buf[0]), p(buf[1]) if partials else None, 1, 128, p(buf[2]), p(buf[3]), p(buf[4]), None, None, None, 0.1,
                          p(buf[5]), p(buf[6]), p(buf[7]) if dx else None, p(buf[8]) if dx else None)

    bad = pytest.raises(RuntimeError, match="ONDA_EINVAL")
    a, b = side(), side()
    with bad:
        call("onda_bn_pair_fwd_l2", byref(a), byref(b), 1e-5, 1, p(buf[7]), p(buf[8]), 8, 48, None, 0, 1, s)      # C % 32
    with bad:
        call("onda_bn_pair_fwd_l2", byref(a), byref(b), 1e-5, 1, p(buf[7]), p(buf[8]), 8, 64, None, 8, 1, s)      # split == M
    with bad:
        nop = side(partials=False)
        call("onda_bn_pair_fwd_l2", byref(a), byref(nop), 1e-5, 1, p(buf[7]), p(buf[8]), 8, 64, None, 0, 1, s)    # no statistics
    with bad:
        call("onda_bn_pair_bwd_l2", p(buf[9]), None, byref(a), byref(b), p(buf[1]), 8, 64, 1, 0, s)               # ReLU without mask
    with bad:
        nodx = side(dx=False)
        call("onda_bn_pair_bwd_l2", p(buf[9]), None, byref(a), byref(nodx), p(buf[1]), 8, 64, 0, 0, s)            # nowhere to write
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the whole model, both routes
_oracle = {}


@pytest.mark.parametrize("pair", [True, False], ids=["pair", "two-functions"])
def test_train_pass_holds_the_g2_bars_on_both_routes(golden, monkeypatch, pair):
    """One train-mode forward + backward of the whole model at 64 x 128 with the pair route on (the default) and off
    (ONDA_BN_PAIR=0): each must hold every bar of test_hip_model.test_train_forward_backward_golden (G2) -- that test's own body
    runs here.  The routes need not agree bit for bit.  The pair route must really be taken: four launches each way, or none."""
    import test_hip_model as T
    from onda_amd import ops
    from onda_amd.ops import norm
    if not _supported():
        pytest.skip("limb rows exist in the f16x2 / dma configuration only")
    launches = []
    real_call = norm.call

    def counting(name, *args):
        launches.append(name)
        return real_call(name, *args)

    def oracle_once(g, b, mask, names):  # (the float64 oracle on the CPU does not depend on the route)
        if "grads" not in _oracle:
            _oracle["grads"] = real_oracle(g, b, mask, names)
        return _oracle["grads"]

    real_oracle = T._fp64_oracle_grads
    monkeypatch.setattr(norm, "call", counting)
    monkeypatch.setattr(T, "_fp64_oracle_grads", oracle_once)
    old = ops.BN_PAIR
    ops.BN_PAIR = pair
    try:
        T.test_train_forward_backward_golden(golden, True)
    finally:
        ops.BN_PAIR = old
    want = 4 if pair else 0
    assert launches.count("onda_bn_pair_fwd_l2") == want and launches.count("onda_bn_pair_bwd_l2") == want
