"""GPU: GroupNorm on a backbone convolution (csrc/norm.hip onda_gn_site_fwd / onda_gn_site_bwd, ops.GNSiteFn) held to the float64
restatement of tests/norm_fp64.py per (image, group), with that module's bounds and comparators; both conv modes.  The
statistics tolerance takes the geometry of the route that produced the partials: colreduce_geometry for the reduction pass,
bn_geometry for the conv epilogue's.  The input of every restatement is what the device normalised."""
import pytest
import torch

import gn_site_fp64 as S
import norm_fp64 as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ids = lambda c: c.id  # noqa: E731


@pytest.fixture(autouse=True, params=["f32", "f16x2"])
def conv_mode(request):
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, request.param
    yield request.param
    ops.CONV_MODE = old


def _report(where):
    """Print (and forget) what the comparators measured since the last report: a test's own worst ratios."""
    for what in sorted(N.MEASURED):
        if what.startswith("gn"):
            print(f"{where}: worst ratio to its bound: {what}: {N.MEASURED[what][0]:.3f} at {N.MEASURED[what][1]}")
            del N.MEASURED[what]


def _site(y, stats, gamma, beta, dout, relu, affine):
    """ops.GNSiteFn on the device, forward and backward; y [B, H, W, C] on the device.  Returns what gn_site_fp64.hold takes."""
    from onda_amd import ops
    B, H, W, C = y.shape
    yd = y.detach().requires_grad_(True)
    gd, bd = gamma.to(DEV).requires_grad_(affine), beta.to(DEV).requires_grad_(affine)
    out = ops.GNSiteFn.apply(yd, stats, gd, bd, relu)
    _, _, mean, rstd, _ = out.grad_fn.saved_tensors
    if ops.CONV_MODE == "f16x2":  # the convolution above reads max|out| from the tag
        assert float(ops.known_amax(out).max()) == float(out.detach().abs().max())
    else:
        assert ops.known_amax(out) is None
    out.backward(dout.reshape(B, H, W, C).to(DEV))
    torch.cuda.synchronize()
    assert (gd.grad is not None) == affine and (bd.grad is not None) == affine
    r = lambda t: t.detach().cpu().reshape(B, H * W, C)  # noqa: E731
    return (r(out), mean.cpu(), rstd.cpu(), r(yd.grad), gd.grad.cpu() if affine else None, bd.grad.cpu() if affine else None)


@pytest.mark.parametrize("case", S.SITE_CASES, ids=ids)
def test_site_kernels_against_fp64(case):
    """The reduction route at every group width; dgamma / dbeta asked for at the stem's width, NULL (frozen) elsewhere."""
    x, gamma, beta, dout = S.site_inputs(case)
    affine = case.id == "c64-relu"
    got = _site(x.reshape(case.B, case.H, case.W, case.C).to(DEV), None, gamma, beta, dout, case.relu, affine)
    try:
        exempt = S.hold(got, x, gamma, beta, dout, case.relu, S.geometry(case), case.id, affine=affine)
    finally:
        _report(case.id)
    assert exempt <= N.EXEMPT_SHARE, f"{case.id}: {100 * exempt:.3f} % exempt from the mask check"


def _stem_output(B, H, W):
    """The real stem convolution (7 x 7, stride 2, 3 -> 64) with its epilogue's statistic partials."""
    from onda_amd import ops
    g = torch.Generator().manual_seed(1000 * B + H + W)
    img = torch.randn(B, 3, H, W, generator=g).to(DEV)
    w = (torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5).to(DEV)
    with torch.no_grad():
        y, stats = ops.StemConvFn.apply(img, w, ops._PackCache(), True)
    return y, stats


@pytest.mark.parametrize("B,H,W,fused", [(2, 32, 32, True), (2, 64, 128, True), (2, 33, 65, False)], ids=["hw256", "hw2048", "hw561"])
def test_stem_site_behind_the_real_conv(conv_mode, B, H, W, fused):
    """C = 64 behind the stem convolution: the statistics come from its epilogue's partials where no tile lies across two images
    (HW a multiple of the 256-row tile: the pre-split kernels record their tile height, the exact-fp32 kernels do not and always
    take the reduction pass), from the reduction pass otherwise."""
    from onda_amd import ops
    y, stats = _stem_output(B, H, W)
    _, Ho, Wo, C = y.shape
    HW = Ho * Wo
    assert (C, HW) == (64, {32: 256, 64: 2048, 33: 561}[H])
    route = ops.gn_site_stats(stats, B, HW)
    takes_partials = fused and conv_mode == "f16x2"
    assert (route is stats) if takes_partials else (route is None)
    seed = N.case_seed(f"stem-{H}x{W}")
    gamma, beta, _, _ = N.population(C, seed)
    dout = torch.randn(B, HW, C, generator=torch.Generator().manual_seed(seed + 1))
    got = _site(y, stats, gamma, beta, dout, True, False)
    x = y.cpu().reshape(B, HW, C)
    geo = N.bn_geometry(HW, C) if takes_partials else N.colreduce_geometry(B, HW, C)
    try:
        exempt = S.hold(got, x, gamma, beta, dout, True, geo, f"stem {H}x{W}", bwd_geo=N.colreduce_geometry(B, HW, C), affine=False)
    finally:
        _report(f"stem {H}x{W} ({'epilogue partials' if takes_partials else 'reduction pass'})")
    assert exempt <= N.EXEMPT_SHARE
    if takes_partials:  # the two routes see the same tensor: their statistics agree within the sum of their bounds
        old, ops.GN_FUSED_STATS = ops.GN_FUSED_STATS, False
        try:
            assert ops.gn_site_stats(stats, B, HW) is None
            other = _site(y, stats, gamma, beta, dout, True, False)
        finally:
            ops.GN_FUSED_STATS = old
        S.hold(other, x, gamma, beta, dout, True, N.colreduce_geometry(B, HW, C), f"stem {H}x{W} reduction", affine=False)


# ------------------------------------------------------------------------------------------------ the C ABI directly
class _Direct:
    """One (B, HW, C) problem on the device, driven through the C ABI."""

    def __init__(self, case, tile_rows=0):
        from onda_amd._lib import query
        x, gamma, beta, dout = S.site_inputs(case)
        self.B, self.HW, self.C, self.relu = case.B, case.H * case.W, case.C, case.relu
        self.x, self.gamma, self.beta, self.dout = x.to(DEV), gamma.to(DEV), beta.to(DEV), dout.to(DEV)
        self.ws = torch.empty(query("onda_gn_site_ws", self.B, self.HW, self.C), device=DEV)
        self.stats, self.tile_rows = None, tile_rows
        if tile_rows:  # a partial table as a conv epilogue leaves it: [tiles][2][C], `tile_rows` rows each
            t = self.x.reshape(self.B * self.HW // tile_rows, tile_rows, self.C)
            self.stats = torch.stack([t.sum(1), (t * t).sum(1)], 1).contiguous()

    def fwd(self, out=None, mean=None, rstd=None, amax=None, flag=None, groups=S.GROUPS, stats="own", tile_rows=None, C=None):
        from onda_amd import ops
        from onda_amd._lib import call
        p = ops._p
        out = torch.empty_like(self.x) if out is None else out
        mean = torch.empty(self.B * groups, device=DEV) if mean is None else mean
        rstd = torch.empty(self.B * groups, device=DEV) if rstd is None else rstd
        st = self.stats if stats == "own" else stats
        call("onda_gn_site_fwd", p(self.x), p(st), st.shape[0] if st is not None else 0, 2 if st is not None else 0,
             (self.tile_rows if tile_rows is None else tile_rows) if st is not None else 0, p(self.gamma), p(self.beta), p(out),
             p(mean), p(rstd), p(self.ws), self.B, self.HW, C or self.C, groups, N.GN_EPS, int(self.relu), p(amax), p(flag), ops._stream())
        return out, mean, rstd

    def bwd(self, out, mean, rstd, amax=None, affine=True):
        from onda_amd import ops
        from onda_amd._lib import call
        p = ops._p
        dx = torch.empty_like(self.x)
        dg, db = (torch.empty(self.C, device=DEV), torch.empty(self.C, device=DEV)) if affine else (None, None)
        call("onda_gn_site_bwd", p(self.dout), p(out), p(self.x), p(self.gamma), p(mean), p(rstd), p(dx), p(dg), p(db), p(self.ws),
             self.B, self.HW, self.C, S.GROUPS, int(self.relu), p(amax), ops._stream())
        return dx, dg, db


@pytest.mark.parametrize("tile_rows", [0, 35], ids=["reduction", "partials"])
def test_run_if_gates_every_launch(tile_rows):
    """run_if reading 0: a sentinel-filled output, statistics and max slot are untouched, on both statistics routes; reading 1:
    the bits of the call with run_if == NULL."""
    from onda_amd import ops
    d = _Direct(S.SITE_BY_ID["c64-relu"], tile_rows)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, mean, rstd = torch.full_like(d.x, 7.0), torch.full((d.B * S.GROUPS,), 7.0, device=DEV), torch.full((d.B * S.GROUPS,), 7.0, device=DEV)
    amax = ops.amax_slot(DEV)
    d.ws.fill_(7.0)
    d.fwd(out, mean, rstd, amax, flag)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((mean == 7.0).all()) and bool((rstd == 7.0).all()) and bool((d.ws == 7.0).all())
    assert float(amax.max()) == 0.0
    ref = d.fwd()
    flag.fill_(1)
    got = d.fwd(out, mean, rstd, amax, flag)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert float(amax.max()) == float(ref[0].abs().max()) > 0


def test_partials_route_matches_the_restatement():
    """The finalize kernel on a hand-made partial table (one 35-row tile per image), without a convolution in front."""
    case = S.SITE_BY_ID["c64-relu"]
    d = _Direct(case, 35)
    out, mean, rstd = d.fwd()
    dx, dg, db = d.bwd(out, mean, rstd)
    torch.cuda.synchronize()
    x, gamma, beta, dout = S.site_inputs(case)
    r = lambda t: t.cpu().reshape(d.B, d.HW, d.C)  # noqa: E731
    # torch's sums over 35 rows: a chain no longer than colreduce_kernel's for this shape, one partial per image
    try:
        S.hold((r(out), mean.cpu(), rstd.cpu(), r(dx), dg.cpu(), db.cpu()), x, gamma, beta, dout, case.relu, S.geometry(case), "partials c64-relu")
    finally:
        _report("partials c64-relu")


def test_argument_checks():
    from onda_amd._lib import query
    d = _Direct(S.SITE_BY_ID["c64-relu"], 35)
    bad = pytest.raises(RuntimeError, match="ONDA_EINVAL")
    with bad:
        d.fwd(groups=16, C=48)                      # 3 channels per group
    with bad:
        d.fwd(groups=64, C=64)                      # 1 channel per group
    with bad:
        d.fwd(tile_rows=4)                          # HW % tile_rows != 0
    with bad:
        d.fwd(stats=d.stats[:1].contiguous())       # fewer partial rows than tile rows
    with bad:
        d.fwd(stats=torch.cat([d.stats, d.stats]))  # more: a stream-K remainder's extra rows
    torch.cuda.synchronize()
    assert query("onda_gn_site_ws", 2, 35, 64) >= 2 * 2 * 64 + 2 * 2 * 64 + 2 * 32 * 2


@pytest.mark.parametrize("cid", ["c64-chunks2", "c2048"])
def test_two_runs_give_the_same_bits(cid):
    from onda_amd import ops
    d = _Direct(S.SITE_BY_ID[cid])
    runs = []
    for _ in range(2):
        a_out, a_dx = ops.amax_slot(DEV), ops.amax_slot(DEV)
        out, mean, rstd = d.fwd(amax=a_out)
        dx, dg, db = d.bwd(out, mean, rstd, amax=a_dx)
        torch.cuda.synchronize()
        assert float(a_out.max()) == float(out.abs().max()) and float(a_dx.max()) == float(dx.abs().max()) > 0
        runs.append((out, mean, rstd, dx, dg, db))
        dx2, dg2, db2 = d.bwd(out, mean, rstd, affine=False)  # the frozen case: the same dx without dgamma / dbeta
        assert dg2 is None and db2 is None and torch.equal(dx2, dx)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
