"""GPU: the normalisation kernels of csrc/norm.hip and csrc/norm_l2.hip, driven through ops/norm.py (BNTrainFn, BNTrainLimbFn,
GNConcatFn), held to the float64 restatement of tests/norm_fp64.py per channel / per (image, group) with the bounds derived
there.  The cases are the smallest at which a kernel can still go wrong (tests/test_norm_fp64_reference.py asserts that they
reach the paths they are named for); the input of every restatement is what the device normalised."""
import ctypes

import numpy as np
import pytest
import torch

import norm_fp64 as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ids = lambda c: c.id  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for what in sorted(N.MEASURED):
        print(f"worst ratio to its bound: {what}: {N.MEASURED[what][0]:.3f} at {N.MEASURED[what][1]}")


def _stats(xd, M, C):
    """onda_bn_stats over M dense rows: partials [tiles, 2, C]."""
    from onda_amd import ops
    from onda_amd._lib import call, query
    parts = torch.empty(query("onda_bn_bwd_ws", M, C), device=DEV)
    tiles = ctypes.c_int(0)
    call("onda_bn_stats", xd.data_ptr(), M, C, C, parts.data_ptr(), ctypes.byref(tiles), ops._stream())
    assert tiles.value == N.col_plan(1, M, C).chunks
    return parts[: tiles.value * 2 * C].reshape(tiles.value, 2, C)


def _bn_fp32(x, gamma, beta, res, dout, rm, rv, shape, relu, track, first=0, tile_rows=0):
    """BNTrainFn on the device; returns what the comparators take."""
    from onda_amd import ops
    B, H, W, C = shape
    M = B * H * W
    xd = x.reshape(shape).to(DEV).requires_grad_(True)
    rd = res.reshape(shape).to(DEV).requires_grad_(True) if res is not None else None
    stats = _stats(xd, M, C)
    if tile_rows:
        stats._onda_tile_rows = tile_rows
    rm_d, rv_d, nbt = rm.to(DEV), rv.to(DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    with ops.row_groups(first):
        out = ops.BNTrainFn.apply(xd, stats, gamma.to(DEV), beta.to(DEV), rd, relu, (rm_d, rv_d, nbt) if track else None, N.MOMENTUM)
        saved = out.grad_fn.saved_tensors
        out.backward(dout.reshape(shape).to(DEV))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu().reshape(M, C), mean=saved[2].cpu(), invstd=saved[3].cpu(), dx=xd.grad.cpu().reshape(M, C),
                dres=rd.grad.cpu().reshape(M, C) if rd is not None else None, rm=rm_d.cpu(), rv=rv_d.cpu(), nbt=int(nbt))


def _hold_bn(got, ref, x, dout, res, rm, rv, relu, track, geometry, bwd_geometry, where):
    N.check_bn_stats(got["mean"], got["invstd"], ref, geometry, where)
    exempt = N.check_bn_forward(got["out"], ref, geometry, where)
    assert exempt <= N.EXEMPT_SHARE, f"{where}: {100 * exempt:.3f} % exempt from the mask check"
    bw = N.bn_bwd64(ref, dout, (got["out"] > 0) if relu else None)
    N.check_bn_backward(got["dx"], bw, ref, geometry, bwd_geometry, where)
    if res is not None:
        assert torch.equal(got["dres"].double(), bw.g), f"{where}: dres is not dout * [out > 0] bit for bit"
    if track:
        N.check_bn_running((got["rm"], got["rv"], got["nbt"]), (rm, rv), ref, geometry, where)
    else:
        assert torch.equal(got["rm"], rm) and torch.equal(got["rv"], rv) and got["nbt"] == 0, f"{where}: untracked running buffers moved"


# ------------------------------------------------------------------------------------------------ fp32 path
@pytest.mark.parametrize("case", N.BN_CASES, ids=ids)
def test_batchnorm_fp32_path(case):
    x, gamma, beta, res, dout, rm, rv = N.bn_case_inputs(case)
    got = _bn_fp32(x, gamma, beta, res, dout, rm, rv, (1, case.M, 1, case.C), case.relu, case.track)
    ref = N.bn64(x, gamma, beta, res, case.relu, None, (rm, rv, 0) if case.track else None)
    geo = [N.bn_geometry(case.M, case.C)]
    _hold_bn(got, ref, x, dout, res, rm, rv, case.relu, case.track, geo, geo, case.id)


@pytest.mark.parametrize("case", N.RG_CASES, ids=ids)
def test_batchnorm_fp32_path_row_groups(case):
    """Two row groups through ops.row_groups: on a partial-row boundary each group takes its own rows of the partial table, off it
    one onda_bn_stats pass per group; group 0 leaves the running buffers alone (they move by group 1's statistics only)."""
    M, C, split = case.B * case.H * case.W, case.C, case.first * case.H * case.W
    seed = N.case_seed(case.id)
    x, gamma, beta = N.bn_input(M, C, seed, shift_rows=split)
    g = torch.Generator().manual_seed(seed + 2)
    res = torch.randn(M, C, generator=g) * 3 if case.res else None
    dout = torch.randn(M, C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    p = N.col_plan(1, M, C)
    got = _bn_fp32(x, gamma, beta, res, dout, rm, rv, (case.B, case.H, case.W, C), case.relu, True, case.first, p.rows_per_chunk)
    groups = [(0, split), (split, M - split)]
    ref = N.bn64(x, gamma, beta, res, case.relu, groups, (rm, rv, 0))
    if split % p.rows_per_chunk == 0:
        L = -(-p.rows_per_chunk // p.ry) + p.ry - 1
        geo = [(L, split // p.rows_per_chunk), (L, -(-(M - split) // p.rows_per_chunk))]
    else:
        geo = [N.bn_geometry(n, C) for _, n in groups]
    _hold_bn(got, ref, x, dout, res, rm, rv, case.relu, True, geo, [N.bn_geometry(n, C) for _, n in groups], case.id)


def test_one_pass_kernels_against_fp32_torch_off_centre():
    """Measured, not held: the per-channel xhat error (max|xhat| * d invstd / invstd + invstd * d mean, worst ordinary channel)
    of onda_bn_stats + onda_bn_finalize and of fp32 torch on the CPU at mean / std 4, 4.45 (the network's worst) and 16.  The
    figures go to docs/experiments.md; the statistics themselves are held by test_batchnorm_fp32_path."""
    from onda_amd import ops
    from onda_amd._lib import call
    for cid in ("c24-m306", "c64-m306", "c2048-m306", "c64-chunks66"):
        case = N.BN_BY_ID[cid]
        for ratio in (4.0, 4.45, 16.0):
            x, gamma, beta = N.bn_case_inputs(case, ratio)[:3]
            ref = N.bn64(x, gamma, beta)
            xd = x.to(DEV)
            stats = _stats(xd, case.M, case.C)
            mean, invstd = torch.empty(case.C, device=DEV), torch.empty(case.C, device=DEV)
            call("onda_bn_finalize", ops._p(stats), stats.shape[0], case.C, case.M, N.BN_EPS, ops._p(mean), ops._p(invstd), None, None, None,
                 N.MOMENTUM, ops._stream())
            _, tm, ts = torch.native_batch_norm(x.t()[None, :, :, None].contiguous(), gamma, beta, None, None, True, N.MOMENTUM, N.BN_EPS)
            live = slice(0, case.C - 2)
            err = [float((ref.xhat_amax[0] * (i.cpu().double() - ref.invstd[0]).abs() / ref.invstd[0]
                          + ref.invstd[0] * (m.cpu().double() - ref.mean[0]).abs())[live].max()) for m, i in ((mean, invstd), (tm, ts))]
            print(f"one-pass kernel vs fp32 torch, {cid} mean/std {ratio}: kernel {err[0]:.2e}, torch {err[1]:.2e}, ratio {err[0] / err[1]:.1f}")
            assert err[0] > 0 and err[1] > 0


# ------------------------------------------------------------------------------------------------ limb path
class LimbCase:
    def __init__(self, id, C, shape, relu, res=None, track=True, grad=True, first=0, fuse=None, bm=None, balanced=False):
        self.id, self.C, self.shape, self.relu, self.res, self.track, self.grad, self.first, self.fuse = id, C, shape, relu, res, track, grad, first, fuse
        self.bm, self.balanced = bm, balanced  # the tile height the case is there for; a hybrid stream-K statistics table


LIMB_CASES = [
    LimbCase("c32-one-tile", 32, (1, 7, 9), True, res=1.0, fuse=False),           # 252 items: the last wave is not whole
    LimbCase("c64-tiles-res100", 64, (2, 17, 33), True, res=100.0, fuse=True),    # several tiles, 8976 items = 140.25 waves
    LimbCase("c256-res0.01", 256, (2, 9, 17), False, res=0.01),
    LimbCase("c2048-nomask", 2048, (1, 9, 17), True, track=False, grad=False, balanced=True),    # ReLU without the bit mask: forward alone
    # the same conv (64 K-steps: hybrid stream-K, the last tile row's extrema spread over sub-block rows) without the ReLU
    LimbCase("c2048-balanced", 2048, (1, 9, 17), False, track=False, grad=False, balanced=True),
    LimbCase("c64-stride-tail", 64, (1, 513, 513), True, res=None, track=True, grad=False),  # two items in the loop + the tail item
    LimbCase("c256-rg", 256, (4, 9, 17), True, res=1.0, first=1, bm=128),         # two row groups, a straddling partial row
    LimbCase("c64-rg", 64, (5, 33, 41), True, first=2, bm=256),
]


def _limb_supported():
    from onda_amd import ops
    return ops.CONV_MODE == "f16x2" and ops.H2_PATH == "dma"


@pytest.mark.parametrize("case", LIMB_CASES, ids=ids)
def test_batchnorm_limb_path(case):
    """BNTrainLimbFn behind a 1x1 Conv2dFn with four stat rows.  The conv is the identity plus a little mixing, so that y carries
    the channel population; the restatement starts from the fp32 conv output the device returned."""
    from onda_amd import ops
    if not _limb_supported():
        pytest.skip("limb planes exist in the f16x2 / dma configuration only")
    B, H, W = case.shape
    C, M, split = case.C, B * H * W, case.first * H * W
    total8 = M * C // 8
    if case.id == "c64-stride-tail":
        stride = 4096 * 256
        assert 2 * stride < total8 < 3 * stride
    elif case.first == 0:
        assert N.ew_trips(total8, 4096) == 1 and (total8 % 64 != 0) == (case.id in ("c32-one-tile", "c64-tiles-res100"))
    seed = N.case_seed(case.id)
    x, gamma, beta = N.bn_input(M, C, seed, shift_rows=split)
    g = torch.Generator().manual_seed(seed + 2)
    w = torch.eye(C) + 1e-3 * torch.randn(C, C, generator=g) / C ** 0.5
    w[C - 2] = 0
    w[C - 2, C - 2] = 1  # the constant channel stays constant
    dout = torch.randn(M, C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    xd = x.reshape(B, H, W, C).to(DEV).requires_grad_(case.grad)
    wd = w.reshape(C, C, 1, 1).to(DEV)
    rm_d, rv_d, nbt = rm.to(DEV), rv.to(DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    old_fuse = ops.FUSE_BN_FINALIZE
    if case.fuse is not None:
        ops.FUSE_BN_FINALIZE = case.fuse
    try:
        with ops.row_groups(case.first):
            yd, stats = ops.Conv2dFn.apply(xd, wd, None, ops._PackCache(), 1, 1, 0, 4, None)
            assert stats.shape[1] == 4
            y = yd.detach().cpu().reshape(M, C)
            assert bool((y[:, C - 2] == y[0, C - 2]).all())
            # the residual's size relative to the normalised branch, whose maximum the restatement knows
            res = None
            if case.res is not None:
                branch = N.bn64(y, gamma, beta, None, False, [(0, split), (split, M - split)] if split else None)
                res = torch.randn(M, C, generator=g)
                res = res * (case.res * float(branch.out.abs().max()) / float(res.abs().max()))
            rd = res.reshape(B, H, W, C).to(DEV).requires_grad_(case.grad) if res is not None else None
            zd = ops.BNTrainLimbFn.apply(yd, stats, gamma.to(DEV), beta.to(DEV), rd, case.relu, (rm_d, rv_d, nbt) if case.track else None, N.MOMENTUM)
            assert ops.is_limb_only(zd)
            lb = ops.limbs_of(zd)
            out = ops.materialize(zd).cpu().reshape(M, C)
            bound = float(lb.amax.max())
            groups = [(0, split), (split, M - split)] if split else None
            ref = N.bn64(y, gamma, beta, res, case.relu, groups, (rm, rv, 0) if case.track else None)
            from onda_amd.ops.limbs import _stat_tile_rows
            tiles, bm = stats.shape[0], _stat_tile_rows(stats)
            assert case.bm is None or bm == case.bm, f"{case.id}: statistic tiles of {bm} rows, the case is there for {case.bm}"
            assert (tiles > -(-M // bm)) == case.balanced, f"{case.id}: {tiles} statistic rows for {-(-M // bm)} tile rows"
            if split:
                assert split % bm != 0, "the case is there for the straddling partial row"
                geo = [(N.EPILOGUE_CHAIN, max(1, split // bm)), (N.EPILOGUE_CHAIN, tiles - split // bm)]
            else:
                geo = [(N.EPILOGUE_CHAIN, tiles)]
            where = case.id
            if split:  # group 1 keeps the whole straddling row's extrema: an upper bound only (as test_batchnorm_row_groups holds it)
                assert float(ref.out.abs().max()) <= bound * (1 + 1e-6), f"{where}: the limb bound {bound:.6e} is below the true maximum"
            else:
                N.check_limb_bound(bound, float(ref.out.abs().max()), float(ref.res_amax.max()), where)
            exempt = N.check_bn_forward(out, ref, geo, where, limb_bound=bound)
            assert exempt <= N.EXEMPT_SHARE, f"{where}: {100 * exempt:.3f} % exempt from the mask check"
            if case.track:
                N.check_bn_running((rm_d.cpu(), rv_d.cpu(), int(nbt)), (rm, rv), ref, geo, where)
            else:
                assert torch.equal(rm_d.cpu(), rm) and torch.equal(rv_d.cpu(), rv) and int(nbt) == 0
            if not case.grad:
                assert zd.grad_fn is None
                return
            node = zd.grad_fn
            _, mean, invstd, _, xhat_amax = node.saved_tensors
            G = 2 if split else 1
            N.check_bn_stats(mean.cpu().reshape(G, C), invstd.cpu().reshape(G, C), ref, geo, where, xhat_amax=xhat_amax.cpu().reshape(G, C))
            mask = None
            if case.relu:
                assert node.relu_mask is not None
                bits = np.unpackbits(node.relu_mask.cpu().numpy(), bitorder="little").reshape(M, C)
                mask = out > 0
                assert bool((torch.from_numpy(bits).bool() == mask).all()), f"{where}: the saved bit mask is not [out > 0]"
            grads = torch.autograd.grad(zd, [yd] + ([rd] if rd is not None else []), dout.reshape(B, H, W, C).to(DEV))
            dxl = ops.limbs_of(grads[0])
            dx = ops.materialize(grads[0]).cpu().reshape(M, C)
            dx_bound = float(dxl.amax.max())
            torch.cuda.synchronize()
        bw = N.bn_bwd64(ref, dout, mask)
        bgeo = [N.bn_geometry(n, C) for _, n in (groups or [(0, M)])]
        N.check_bn_backward(dx, bw, ref, geo, bgeo, where, limb_bound=dx_bound)
        tol = N.bn_dx_tol(ref, bw, geo, bgeo)
        # an upper bound of what the device wrote, and of the reference up to the reference's own tolerance
        assert float(dx.abs().max()) <= dx_bound * (1 + 1e-6), f"{where}: the dx bound {dx_bound:.6e} is below max|dx| {float(dx.abs().max()):.6e}"
        ref_max = torch.stack([bw.dx[r0:r0 + n].abs().amax(0) for r0, n in ref.groups])
        assert float((ref_max - tol).max()) <= dx_bound * (1 + 1e-6), f"{where}: the dx bound {dx_bound:.6e} is below the reference's max|dx|"
        assert dx_bound <= 2.0 * float((bw.scale + tol).max()), f"{where}: the dx bound {dx_bound:.6e} is more than twice its formula {float(bw.scale.max()):.6e}"
        if rd is not None:
            assert torch.equal(grads[1].cpu().reshape(M, C).double(), bw.g), f"{where}: dres is not dout * [out > 0] bit for bit"
    finally:
        ops.FUSE_BN_FINALIZE = old_fuse


# ------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("case", N.GN_CASES, ids=ids)
def test_groupnorm_concat(case):
    from onda_amd import ops
    xs, gammas, betas, chmul, dcat = N.gn_case_inputs(case)
    B, HW, C, n = case.B, case.HW, case.C, case.n
    xd = [x.reshape(B, HW, 1, C).to(DEV).requires_grad_(True) for x in xs]
    gd = [t.to(DEV).requires_grad_(True) for t in gammas]
    bd = [t.to(DEV).requires_grad_(True) for t in betas]
    cat = ops.GNConcatFn.apply(case.relu, chmul.to(DEV) if chmul is not None else None, *xd, *gd, *bd)
    saved = cat.grad_fn.saved_tensors
    means, rstds = saved[2 + 2 * n:2 + 3 * n], saved[2 + 3 * n:2 + 4 * n]
    cat.backward(dcat.reshape(B, HW, 1, C * n).to(DEV))
    torch.cuda.synchronize()
    got = cat.detach().cpu().reshape(B, HW, C * n)
    ref = N.gn64(xs, gammas, betas, chmul, case.relu)
    geo = N.gn_geometry(case)
    exempt = N.check_gn_forward(got, [m.cpu() for m in means], [r.cpu() for r in rstds], ref, geo, case.id)
    assert exempt <= N.EXEMPT_SHARE, f"{case.id}: {100 * exempt:.3f} % exempt from the mask check"
    bw = N.gn_bwd64(ref, dcat, (got > 0) if case.relu else None)
    N.check_gn_backward([t.grad.cpu().reshape(B, HW, C) for t in xd], [t.grad.cpu() for t in gd], [t.grad.cpu() for t in bd], bw, ref, geo, geo, case.id)


# ------------------------------------------------------------------------------------------------ guards
def test_norm_entry_points_refuse_what_their_kernels_cannot_run():
    """Every ONDA_REQUIRE of the norm entry points beyond test_bad_arguments_raise: a channel count, a row stride or a group width
    that is no multiple of 4 (the kernels move 16-byte quads), and a ReLU mask without the forward output to take it from."""
    from onda_amd import ops
    from onda_amd._lib import call
    p, s = ops._p, ops._stream()
    buf = [torch.zeros(4096, device=DEV) for _ in range(8)]
    a, b, c, d, e, f, g, h = buf
    tiles = ctypes.c_int(0)
    bad = pytest.raises(RuntimeError, match="ONDA_EINVAL")
    with bad:
        call("onda_bn_stats", p(a), 8, 6, 8, p(b), ctypes.byref(tiles), s)            # C % 4
    with bad:
        call("onda_bn_stats", p(a), 8, 8, 10, p(b), ctypes.byref(tiles), s)           # ldx % 4
    with bad:
        call("onda_bn_apply", p(a), p(b), p(c), p(d), p(e), None, p(f), 8, 6, 0, None, s)   # C % 4
    with bad:
        call("onda_bn_bwd", p(a), p(b), p(c), p(d), p(e), p(f), p(g), None, p(h), 8, 6, 0, None, s)     # C % 4
    with bad:
        call("onda_bn_bwd", p(a), None, p(c), p(d), p(e), p(f), p(g), None, p(h), 8, 8, 1, None, s)     # ReLU without out
    with bad:
        call("onda_gn_fwd", p(a), 64, p(b), p(c), None, p(d), 64, p(e), p(f), p(g), 1, 4, 64, 32, 1e-5, 0, None, s)   # (C / groups) % 4
    with bad:
        call("onda_gn_fwd", p(a), 130, p(b), p(c), None, p(d), 128, p(e), p(f), p(g), 1, 4, 128, 32, 1e-5, 0, None, s)  # ldx % 4
    with bad:
        call("onda_gn_bwd", p(a), 128, None, 128, p(b), 128, p(c), None, p(d), p(e), p(f), p(g), p(h), p(buf[0]), 1, 4, 128, 32, 1, s)  # ReLU without out
    with bad:
        call("onda_gn_bwd", p(a), 64, p(b), 64, p(c), 64, p(d), None, p(e), p(f), p(g), p(h), p(a), p(b), 1, 4, 64, 32, 0, s)  # (C / groups) % 4
    torch.cuda.synchronize()
