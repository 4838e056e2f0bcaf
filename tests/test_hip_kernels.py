"""GPU parity of every HIP kernel family, called through the C ABI (ctypes), against plain
fp32 torch on the CPU / the oracle on the same seeded inputs.  Integer outputs (labels,
argmax maps, pool indices) must match exactly; floating point within the stated tolerance."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def close(a, b, rel=1e-4, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(b.abs().max().item(), 1e-20)
    err = (a - b).abs().max().item()
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


CONV_CASES = [
    # cin, cout, k, stride, dil, pad, H, W, bias
    (64, 64, 1, 1, 1, 0, 17, 33, False),
    (64, 256, 1, 1, 1, 0, 17, 33, False),
    (256, 64, 1, 1, 1, 0, 9, 17, False),
    (256, 128, 1, 2, 1, 0, 17, 33, False),
    (256, 512, 1, 2, 1, 0, 17, 33, False),
    (64, 64, 3, 1, 1, 1, 17, 33, False),
    (128, 128, 3, 1, 1, 1, 9, 17, False),
    (128, 128, 3, 1, 1, 1, 8, 8, False),   # ONE 128 x 128 tile cut over all 512 resident workgroups: 512 candidate pieces, 36 live
    (256, 256, 3, 1, 2, 2, 9, 17, False),
    (512, 512, 3, 1, 4, 4, 9, 17, False),
    (2048, 256, 3, 1, 6, 6, 9, 17, True),
    (2048, 256, 3, 1, 24, 24, 9, 17, True),
    (2048, 256, 1, 1, 1, 0, 9, 17, True),
    (1280, 256, 3, 1, 1, 1, 9, 17, True),
]


@pytest.fixture(params=["f32", "f16x2"])
def conv_mode(request):
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, request.param
    yield request.param
    ops.CONV_MODE = old


# the dominant shapes at the BASELINE size (4 x 65 x 129 pixels; layer1 at 4 x 129 x 257): what only full-size problems
# reach -- whole rounds of 256 x 128 tiles + a stream-K remainder, split-K weight gradients, offsets past 2^31 / 4
FULL_SIZE_CASES = [
    # cin, cout, k, dil, H, W
    (2048, 256, 3, 6, 65, 129),
    (2048, 256, 3, 24, 65, 129),
    (512, 512, 3, 4, 65, 129),
    (1024, 256, 1, 1, 65, 129),
    (64, 256, 1, 1, 129, 257),
]


@pytest.mark.parametrize("mode", ["default", "f32"])
@pytest.mark.parametrize("case", FULL_SIZE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_full_size_against_torch_cpu(case, mode):
    """Forward, data gradient and weight gradient of the default conv path at the BASELINE problem size against
    fp32 torch on the CPU (max-norm, relative to the largest reference value).  "f32": the exact-fp32 kernels on three of the
    shapes -- only full-size problems reach their 256 x 128 tiles (round 6), with statistics and a stream-K remainder."""
    from onda_amd import ops
    if mode == "f32" and case[0] == 2048:
        pytest.skip("exact-fp32 mode: the other three shapes cover the tile, its statistics rows and the remainder")
    old_mode = ops.CONV_MODE
    if mode == "f32":
        ops.CONV_MODE = "f32"
    try:
        _conv_full_size(ops, case)
    finally:
        ops.CONV_MODE = old_mode


def _conv_full_size(ops, case):
    cin, cout, k, dil, H, W = case
    g = torch.Generator().manual_seed(sum(case))
    B, pad = 4, dil * (k - 1) // 2
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, 1, pad, dil)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    xd = nhwc(x).to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    y, stats = ops.Conv2dFn.apply(xd, wd, None, ops._PackCache(), 1, dil, pad, True, None)
    close(nchw(y), yr, 2e-5, "conv fwd")
    s = stats.sum(0).cpu()
    close(s[0], yr.sum((0, 2, 3)), 1e-4, "stats sum")
    close(s[1], (yr ** 2).sum((0, 2, 3)), 1e-4, "stats sumsq")
    y.backward(nhwc(gy).to(DEV))
    close(nchw(xd.grad), xr.grad, 2e-5, "dgrad")
    close(wd.grad, wr.grad, 1e-4, "wgrad")


def test_weight_gradient_pixel_table_across_batch_sizes():
    """The 256-output-channel weight-gradient kernel reads its input pixels from a per-geometry table that the CALLER owns
    (onda_conv2d_wgrad_l2_table; ops.conv._wgrad_pixel_table keeps one per geometry): the same geometry at batch 1, then 3 (a
    larger table replaces it), then 2 (served by the larger one), dilated 3 x 3 and a stride-2 1 x 1, each against fp32
    torch on the CPU -- and once with no table at all (the kernel then works the pixels out in its K loop: same result)."""
    from onda_amd import ops
    from onda_amd._lib import query
    import ctypes
    for (cin, cout, k, stride, dil, pad, H, W) in [(256, 256, 3, 1, 2, 2, 11, 19), (256, 512, 1, 2, 1, 0, 11, 19)]:
        Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
        d = ops._desc(3, H, W, cin, Ho, Wo, cout, k, stride, dil, pad, cin, cout)
        assert query("onda_conv2d_wgrad_l2_table_stride", ctypes.byref(d)) == (3 * Ho * Wo + 31) // 32 * 32 + 64
        d1 = ops._desc(3, H, W, cin, H, W, cout, 1, 1, 1, 0, cin, cout)
        assert query("onda_conv2d_wgrad_l2_table_stride", ctypes.byref(d1)) == 0  # 1 x 1 stride 1: x pixel = output pixel
        for B in (1, 3, 2, 0):
            no_table = B == 0
            B = B or 2
            real = ops.conv._wgrad_pixel_table
            if no_table:
                ops.conv._wgrad_pixel_table = lambda d, device: None
            try:
                _wgrad_case(ops, cin, cout, k, stride, dil, pad, H, W, B)
            finally:
                ops.conv._wgrad_pixel_table = real
        key = [kk for kk in ops._PIX_TABLES if kk[1:] == (H, W, Ho, Wo, k, k, stride, dil, pad)]
        assert len(key) == 1 and ops._PIX_TABLES[key[0]][1] == 3  # one table per geometry, the largest batch's


def _wgrad_case(ops, cin, cout, k, stride, dil, pad, H, W, B):
    g = torch.Generator().manual_seed(100 * B + k)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    wr = w.clone().requires_grad_(True)
    yr = F.conv2d(x, wr, None, stride, pad, dil)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    xd = nhwc(x).to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    y, _ = ops.Conv2dFn.apply(xd, wd, None, ops._PackCache(), stride, dil, pad, True, None)
    y.backward(nhwc(gy).to(DEV))
    close(wd.grad, wr.grad, 5e-5, f"wgrad k={k} stride={stride} B={B}")


STATIONARY_CASES = [
    # cin, cout, stride, B, H, W       (1 x 1 convolutions the activation-stationary kernel takes: Cin 64 / 128 / 256, Cout >= 128)
    (256, 1024, 1, 2, 33, 65),   # 4290 rows: 34 panels of 128 (the last one 66 rows), 8 column tiles, 8 K-steps (second limbs in LDS)
    (256, 320, 1, 1, 19, 23),    # Cout not a multiple of 128
    (256, 512, 2, 2, 17, 33),    # stride 2 (layer2's downsample): GEMM row m reads pixel (2 ho, 2 wo)
    (128, 512, 1, 2, 33, 65),    # 4 K-steps, both limbs in registers
    (128, 256, 1, 1, 9, 17),     # two column tiles, two panels
    (64, 256, 1, 2, 65, 129),    # 2 K-steps
    (64, 448, 1, 3, 7, 11),      # Cout not a multiple of 128, the last tile half empty
]


@pytest.mark.parametrize("case", STATIONARY_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("epilogue", ["stats", "accumulate", "affine_res_relu", "limbs"])
def test_activation_stationary_conv_is_the_tile_kernel_bit_for_bit(case, epilogue):
    """conv_l2a_kernel (round 6: a workgroup's rows in registers, weight rows streamed; deeplabv2.py:22-24,44,351-357; off by
    default, switched on here) against the 128 x 128 tile kernel it replaces (ONDA_L2_VARIANT=1 forces it): the same products in
    the same order per accumulator, so the output must be IDENTICAL (the statistic partials: equal up to the association of the
    row sums) in the epilogue the kernel takes -- plain output with train-mode statistics -- and close to an fp64 reference.
    The other epilogues (add into a gradient sink; folded BatchNorm + residual + ReLU; eval-mode limb rows) stay on the tile
    kernel whatever the switch says: checked to run and agree."""
    import os
    from onda_amd import ops
    from onda_amd._lib import query
    cin, cout, stride, B, H, W = case
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    try:
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        M = B * Ho * Wo
        os.environ["ONDA_L2_STATIONARY"] = "1"  # (off by default since its step-level A/B; the library reads the switch per call)
        assert query("onda_conv_l2_kernel_id", M, cout, 1, cin) == 4
        g = torch.Generator().manual_seed(cin + cout + stride)
        x = torch.randn(B, H, W, cin, generator=g).to(DEV)
        w = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(DEV)
        wp = ops.pack_weight_fwd(w)
        scale = (0.5 + torch.rand(cout, generator=g)).to(DEV)
        shift = torch.randn(cout, generator=g).to(DEV)
        res = torch.randn(B, Ho, Wo, cout, generator=g).to(DEV)

        def run():
            if epilogue == "stats":
                y, st, _ = ops.conv_forward(x, wp, 1, stride, 1, 0, cout, want_stats=4)
                return y, st
            if epilogue == "accumulate":  # a data gradient that joins a gradient sink: residual == output (ops.GradSink)
                buf = res.clone()
                y, _, _ = ops.conv_forward(x, wp, 1, stride, 1, 0, cout, out=buf, residual=buf)
                return y, y.abs().max()
            if epilogue == "affine_res_relu":
                y, _, _ = ops.conv_forward(x, wp, 1, stride, 1, 0, cout, scale=scale, shift=shift, residual=res, relu=True)
                return y, ops.known_amax(y)
            if cout % 32:
                pytest.skip("limb rows need whole 32-channel blocks")
            y, _, _ = ops.conv_forward(x, wp, 1, stride, 1, 0, cout, scale=scale, shift=shift, relu=True,
                                       limb_out=ops.fold_bounds(w, scale, shift))
            lb = ops.limbs_of(y)
            return lb.planes, lb.true_amax

        got = run()
        del os.environ["ONDA_L2_STATIONARY"]
        os.environ["ONDA_L2_VARIANT"] = "1"
        os.environ["ONDA_CONV_SCHED"] = "1"  # (no stream-K remainder: the same statistic rows)
        try:
            assert query("onda_conv_l2_kernel_id", M, cout, 1, cin) == 1
            want = run()
        finally:
            del os.environ["ONDA_L2_VARIANT"], os.environ["ONDA_CONV_SCHED"]
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]), (got[0].float() - want[0].float()).abs().max().item()
        if epilogue != "stats":
            assert torch.equal(got[1].max(), want[1].max())  # max|y| as the kernel left it
        else:  # the statistic partials: the same sums over a tile's 128 rows, associated by four waves of 32 rows instead of two of 64
            assert torch.equal(got[1][:, 2:], want[1][:, 2:])  # (minima and maxima do not depend on the order)
            np.testing.assert_allclose(got[1][:, :2].cpu().numpy(), want[1][:, :2].cpu().numpy(), rtol=2e-5, atol=1e-4)
        if epilogue == "stats":
            ref = torch.einsum("bhwc,oc->bhwo", x[:, ::stride, ::stride].double().cpu(), w[:, :, 0, 0].double().cpu())
            close(got[0], ref.float(), 2e-6, "stationary conv vs fp64")
            np.testing.assert_allclose(got[1][:, 0].sum(0).cpu().numpy(), ref.reshape(-1, cout).sum(0).numpy(), rtol=1e-4, atol=1e-2)
    finally:
        ops.CONV_MODE = old
        os.environ.pop("ONDA_L2_STATIONARY", None)


L2_PLAN_CASES = [
    # kernel id, cin, cout, B, H, W   (1 x 1 convolutions, the smallest that select each device kernel: tests/golden/l2_plan.json)
    (0, 1056, 256, 2, 99, 130),   # 101 x 2 tiles of 256 x 128 (the last tile row 140 rows), 33 K-steps: past the stream kernel's 32
    (1, 128, 160, 2, 9, 17),      # 128 x 128 tiles, the second column tile a quarter full
    (2, 64, 64, 2, 9, 17),        # 256 x 64 tiles
    (3, 512, 256, 2, 105, 170),   # 16 K-steps: the continuous stream; 280 tiles = one round + a stream-K remainder (512 statistic rows)
    (4, 128, 256, 1, 9, 17),      # activation-stationary (switched on for the case)
]


@pytest.mark.parametrize("case", L2_PLAN_CASES, ids=lambda c: "id%d" % c[0])
def test_l2_launch_follows_its_plan(case, monkeypatch):
    """One problem per device kernel of the pre-split conv (csrc/conv_l2.hip l2_plan), in each epilogue the launch tells apart:
    plain + statistics, folded BatchNorm + residual + ReLU, limb-row output, and the scattered stride-2 data gradient (dy and the
    transposed weight chosen so that it is the SAME (M, Cout, K) problem).  The launch is recorded under the kernel the host
    query names, the statistics have the rows the query promises and sum to the reference's, and every output meets the
    file's conv bound against F.conv2d."""
    import ctypes
    from onda_amd import ops
    from onda_amd._lib import query
    kid, cin, cout, B, H, W = case
    M = B * H * W
    if kid == 4:
        monkeypatch.setenv("ONDA_L2_STATIONARY", "1")
    monkeypatch.setattr(ops._state, "CONV_MODE", "f16x2")
    monkeypatch.setattr(ops._state, "PROFILE", [])
    assert query("onda_conv_l2_kernel_id", M, cout, 1, cin) == kid
    name = ops.core._L2_KERNELS[kid]
    g = torch.Generator().manual_seed(kid)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    res = torch.randn(B, cout, H, W, generator=g)
    ref = F.conv2d(x, w)
    affine = ref * sc[None, :, None, None] + sh[None, :, None, None]
    xd, wd, scd, shd = nhwc(x).to(DEV), w.to(DEV), sc.to(DEV), sh.to(DEV)
    wp = ops.pack_weight_fwd(wd)

    def launched(kind):
        torch.cuda.synchronize()
        got = [(e[0], e[4][:4]) for e in ops._state.PROFILE if e[4] and e[4][0] in ("fwd", "dgrad")]
        del ops._state.PROFILE[:]
        assert got == [(name, (kind, M, cout, cin))], got

    y, stats, tiles = ops.conv_forward(xd, wp, 1, 1, 1, 0, cout, want_stats=4)
    launched("fwd")
    rows = ctypes.c_int(0)
    assert stats.shape[0] == tiles == query("onda_conv_l2_tiles_m_split", M, cout, 1, cin, 0, 0, ctypes.byref(rows))
    assert stats._onda_tile_rows == rows.value == (128 if kid in (1, 4) else 256)
    close(nchw(y), ref, 2e-5, "plain")
    close(stats[:, 0].sum(0), ref.sum((0, 2, 3)), 1e-4, "stats sum")
    close(stats[:, 1].sum(0), (ref ** 2).sum((0, 2, 3)), 1e-4, "stats sumsq")

    y, _, _ = ops.conv_forward(xd, wp, 1, 1, 1, 0, cout, scale=scd, shift=shd, residual=nhwc(res).to(DEV), relu=True)
    launched("fwd")
    close(nchw(y), F.relu(affine + res), 2e-5, "affine + residual + ReLU")

    y, _, _ = ops.conv_forward(xd, wp, 1, 1, 1, 0, cout, scale=scd, shift=shd, relu=True, limb_out=ops.fold_bounds(wd, scd, shd))
    launched("fwd")
    close(nchw(ops.materialize(y)), F.relu(affine), 2e-5, "limb rows")

    # the data gradient of a stride-2 1 x 1 conv with cout -> cin channels swapped: dx[2h, 2w] = dy[h, w] . W, zero elsewhere
    wpd = ops.pack_weight_dgrad(wd.permute(1, 0, 2, 3).contiguous())
    dx = ops.conv_dgrad(xd, wpd, 1, 2, 1, 0, cout, (2 * H - 1, 2 * W - 1))
    launched("dgrad")
    close(nchw(dx[:, ::2, ::2]), ref, 2e-5, "scattered data gradient")
    assert dx[:, 1::2].abs().max().item() == 0 and dx[:, :, 1::2].abs().max().item() == 0


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c[:6])))
def test_conv_fwd_bwd(case, conv_mode):
    from onda_amd import ops
    cin, cout, k, stride, dil, pad, H, W, bias = case
    g = torch.Generator().manual_seed(hash(case) & 0xFFFF)
    B = 2
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g) if bias else None
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    yr = F.conv2d(xr, wr, br, stride, pad, dil)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)

    xd = nhwc(x).to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True) if bias else None
    cache = ops._PackCache()
    y, stats = ops.Conv2dFn.apply(xd, wd, bd, cache, stride, dil, pad, not bias, None)
    close(nchw(y), yr, 2e-5, "conv fwd")
    if stats is not None:
        s = stats.sum(0).cpu()
        close(s[0], yr.sum((0, 2, 3)), 1e-4, "stats sum")
        close(s[1], (yr ** 2).sum((0, 2, 3)), 1e-4, "stats sumsq")
    y.backward(nhwc(gy).to(DEV))
    close(nchw(xd.grad), xr.grad, 2e-5, "dgrad")
    close(wd.grad, wr.grad, 5e-5, "wgrad")
    if bias:
        close(bd.grad, br.grad, 5e-5, "bias grad")


def test_conv_fused_epilogue_and_slice(conv_mode):
    """eval-mode fold: scale/shift + residual + ReLU in the epilogue, written into a channel slice."""
    from onda_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 128, 9, 17, generator=g)
    w = torch.randn(256, 128, 3, 3, generator=g) / 34.0
    sc, sh = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g)
    res = torch.randn(2, 256, 9, 17, generator=g)
    ref = F.relu(F.conv2d(x, w, None, 1, 2, 2) * sc[None, :, None, None] + sh[None, :, None, None] + res)
    buf = torch.zeros(2, 9, 17, 512, device=DEV)
    out = buf[..., 256:]
    ops.conv_forward(nhwc(x).to(DEV), ops.pack_weight_fwd(w.to(DEV)), 3, 1, 2, 2, 256, out=out, scale=sc.to(DEV),
                     shift=sh.to(DEV), residual=nhwc(res).to(DEV), relu=True)
    close(nchw(out), ref, 2e-5, "fused epilogue")
    assert buf[..., :256].abs().max().item() == 0


def test_head_and_stem(conv_mode):
    from onda_amd import ops
    g = torch.Generator().manual_seed(6)
    # 19-class head through the padded 32-wide GEMM
    feat = torch.randn(2, 256, 9, 17, generator=g)
    w = torch.randn(19, 256, 1, 1, generator=g) / 16
    fr, wr = feat.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = F.conv2d(fr, wr)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    fd, wd = nhwc(feat).to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    out_pad, _ = ops.Conv2dFn.apply(fd, wd, None, ops._PackCache(), 1, 1, 0, False, ops.HEAD_PAD)
    out = ops.ClassSliceFn.apply(out_pad, 19)
    close(out, yr, 2e-5, "head fwd")
    assert out_pad[..., 19:].abs().max().item() == 0
    out.backward(gy.to(DEV))
    close(nchw(fd.grad), fr.grad, 2e-5, "head dgrad")
    close(wd.grad, wr.grad, 5e-5, "head wgrad")
    # stem 7x7 s2 p3 from the NCHW image
    x = torch.randn(2, 3, 64, 128, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / 12
    wr = w.clone().requires_grad_(True)
    yr = F.conv2d(x, wr, None, 2, 3)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    wd = w.to(DEV).requires_grad_(True)
    y, stats = ops.StemConvFn.apply(x.to(DEV), wd, ops._PackCache(), True)
    close(nchw(y), yr, 2e-5, "stem fwd")
    y.backward(nhwc(gy).to(DEV))
    close(wd.grad, wr.grad, 5e-5, "stem wgrad")


@pytest.mark.parametrize("cin,cout,k,dil,H,W,res", [(64, 256, 1, 1, 33, 65, True), (256, 64, 1, 1, 33, 65, False),
                                                     (128, 128, 3, 2, 19, 37, False), (512, 2048, 1, 1, 65, 129, True),
                                                     (512, 512, 3, 4, 65, 129, False)])
def test_eval_conv_writes_limb_planes(cin, cout, k, dil, H, W, res):
    """Eval-mode conv + folded BatchNorm [+ residual limbs] + ReLU with the result written as limb planes by the conv
    epilogue itself (a-priori bound as the scale): values against fp32 torch on the CPU, the bound really bounds, the
    true maximum is reported exactly, and a second such conv on top (bounds must not compound) is as accurate as the
    first; small and full-size grids, every tile variant, stream-K remainders."""
    from onda_amd import ops
    g = torch.Generator().manual_seed(cin + cout + k)
    B, pad = 2, dil * (k - 1) // 2
    x = torch.relu(torch.randn(B, cin, H, W, generator=g)) * 3.0
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    r = torch.randn(B, cout, H, W, generator=g) if res else None
    ref = F.conv2d(x, w, None, 1, pad, dil) * sc[None, :, None, None] + sh[None, :, None, None]
    if res:
        ref = ref + r
    ref = F.relu(ref)
    xd = nhwc(x).to(DEV)
    ops.activation_limbs(xd)
    rd = nhwc(r).to(DEV) if res else None
    kb = ops.fold_bounds(w.to(DEV), sc.to(DEV), sh.to(DEV))
    y, _, _ = ops.conv_forward(xd, ops.pack_weight_fwd(w.to(DEV)), k, 1, dil, pad, cout, scale=sc.to(DEV), shift=sh.to(DEV),
                               residual=rd, relu=True, limb_out=kb)
    assert ops.is_limb_only(y)
    lb = ops.limbs_of(y)
    close(nchw(ops.materialize(y)), ref, 2e-5, "limb-plane conv output")
    true_max, bound = lb.true_amax.max().item(), lb.amax.max().item()
    assert true_max == pytest.approx(ref.max().item(), rel=2e-5) and true_max <= bound <= true_max * 2.0 ** 13, (true_max, bound)
    # a second conv of the same kind on top, the first one's output as its residual too
    w2 = torch.randn(cout, cout, 1, 1, generator=g) / cout ** 0.5
    ref2 = F.relu(F.conv2d(ref, w2) * sc[None, :, None, None] + sh[None, :, None, None] + ref)
    kb2 = ops.fold_bounds(w2.to(DEV), sc.to(DEV), sh.to(DEV))
    y2, _, _ = ops.conv_forward(y, ops.pack_weight_fwd(w2.to(DEV)), 1, 1, 1, 0, cout, scale=sc.to(DEV), shift=sh.to(DEV),
                                residual=y, relu=True, limb_out=kb2)
    close(nchw(ops.materialize(y2)), ref2, 3e-5, "second limb-plane conv")
    lb2 = ops.limbs_of(y2)
    assert lb2.true_amax.max().item() <= lb2.amax.max().item() <= lb2.true_amax.max().item() * 2.0 ** 13


def test_model_packer_matches_the_single_weight_packer():
    """All conv weights of a model packed in two launches (LDS-blocked transposition) against the one-weight packer:
    bit-identical limb planes in the forward and the data-gradient layout, same max|w|; 1 x 1 and 3 x 3 filters, channel
    counts that are and are not multiples of the 32-channel block (the latter take the element-per-thread path)."""
    from onda_amd import ops
    from onda_amd.framework.model.deeplabv2 import HipConv2d
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    try:
        g = torch.Generator().manual_seed(21)
        shapes = [(64, 256, 1), (256, 64, 3), (128, 128, 3), (2048, 512, 1), (96, 160, 3), (32, 1280, 3)]  # (multiples of 32: limb rows)
        convs = []
        for cin, cout, k in shapes:
            c = HipConv2d(cin, cout, kernel_size=k, padding=k // 2, bias=False).to(DEV)
            c.weight.data = (torch.randn(cout, cin, k, k, generator=g) * 10.0 ** float(torch.randn((), generator=g))).to(DEV)
            convs.append(c)
        ops.ModelPacker(convs).refresh(need_dgrad=True)
        for c in convs:
            f, d = c._pack.get_fwd(c.weight), c._pack.get_dgrad(c.weight)
            rf, rd = ops.pack_weight_fwd(c.weight.detach().clone()), ops.pack_weight_dgrad(c.weight.detach().clone())
            assert f.amax.max().item() == rf.amax.max().item() == c.weight.abs().max().item()
            assert torch.equal(f.limbs.reshape(-1), rf.limbs.reshape(-1)), tuple(c.weight.shape)
            assert torch.equal(d.limbs.reshape(-1), rd.limbs.reshape(-1)), tuple(c.weight.shape)
    finally:
        ops.CONV_MODE = old


def test_host_never_waits_for_tables_or_monitor_scalars():
    """Multi-tensor entry tables and the monitor's device scalars reach their destination through pinned staging
    buffers (asynchronous copies): same values as the direct path, staging buffers reused only after their copy's event
    has completed, and neither call waits for work queued in front of it."""
    import time
    from onda_amd import ops, _lib
    from onda_amd.framework.utils.monitoring import Monitor
    # tables: round trip of the bytes, ring reuse
    ents = [_lib.OndaEmaEntry(1000 + i, 2000 + i, 10 + i, 0.5, 0.5, i) for i in range(300)]
    want = bytes((_lib.OndaEmaEntry * len(ents))(*ents))
    for _ in range(6):
        dev = ops._table(ents, _lib.OndaEmaEntry, torch.device(DEV))
        assert bytes(dev.cpu().numpy().tobytes()) == want
    assert 1 <= len(ops._TABLE_STAGES[DEV]) <= 16
    # neither path blocks behind a long-running queue (steady state: the pinned buffers exist -- allocating page-locked
    # memory is slow and may synchronise, it happens once)
    mon = Monitor(5, 0.1, "hamming")
    big = torch.randn(8192, 8192, device=DEV)
    for rep in range(2):  # (the first round loads the kernels of the torch ops used here and sets hipBLASLt up)
        mon.reset()
        torch.cuda.synchronize()
        for _ in range(6):
            big = big @ big * 1e-4
        t0 = time.perf_counter()
        dev = ops._table(ents, _lib.OndaEmaEntry, torch.device(DEV))
        mon.add_device(["a", "b"], torch.stack([big[0, 0] * 0 + 0.25, big[0, 0] * 0 + 0.75]))
        issued = time.perf_counter() - t0
        torch.cuda.synchronize()
        drained = time.perf_counter() - t0
    assert issued < 0.25 * drained, (issued, drained)
    assert bytes(dev.cpu().numpy().tobytes()) == want
    assert mon.avg("a") == 0.25 and mon.avg("b") == 0.75


def test_stem_patches_as_limb_planes():
    """Pre-split "f16x2": the stem's patch kernel writes limb planes directly (scale from max|image|); rebuilt, they are
    the fp32 patch matrix to 2^-22 of each value, ragged image size, and the matrix is shared by every pass that reads
    the same image tensor (teacher / static / student) until the image changes."""
    from onda_amd import ops
    g = torch.Generator().manual_seed(16)
    x = (torch.randn(2, 3, 75, 141, generator=g) * 3.0).to(DEV)
    Ho, Wo = ops.conv_out_size(75, 7, 2, 1, 3), ops.conv_out_size(141, 7, 2, 1, 3)
    ref = ops.stem_patches(x, Ho, Wo, False)
    assert not ops.is_limb_only(ref) and ref[..., 147:].abs().max().item() == 0
    col = ops.stem_patches(x, Ho, Wo, True)
    assert ops.is_limb_only(col) and ops.stem_patches(x, Ho, Wo, True) is col
    got = ops.materialize(col)
    assert (got - ref).abs().max().item() <= 2.0 ** -21 * ref.abs().max().item()
    rel = ((got - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
    assert rel <= 2.0 ** -20, rel
    x.mul_(0.5)  # in-place change of the image: the remembered matrix is stale
    again = ops.stem_patches(x, Ho, Wo, True)
    assert again is not col
    assert (ops.materialize(again) - 0.5 * ref).abs().max().item() <= 2.0 ** -21 * ref.abs().max().item()


@pytest.mark.parametrize("C,H,W,relu,res,track", [(64, 17, 33, True, False, True), (256, 9, 17, True, True, False),
                                                    (512, 9, 17, False, False, True), (2048, 5, 9, True, True, True)])
def test_batchnorm_train(C, H, W, relu, res, track):
    from onda_amd import ops
    g = torch.Generator().manual_seed(C + H)
    B = 2
    x = torch.randn(B, C, H, W, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    r = torch.randn(B, C, H, W, generator=g) if res else None
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    xr = x.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True) if res else None
    rm_r, rv_r = rm.clone(), rv.clone()
    y = F.batch_norm(xr, rm_r if track else None, rv_r if track else None, gamma, beta, True, 0.1, 1e-5)
    if res:
        y = y + rr
    if relu:
        y = F.relu(y)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)

    xd = nhwc(x).to(DEV).requires_grad_(True)
    rd = nhwc(r).to(DEV).requires_grad_(True) if res else None
    parts = torch.empty(64 * 2 * C, device=DEV)
    import ctypes
    from onda_amd._lib import call
    tiles = ctypes.c_int(0)
    call("onda_bn_stats", xd.data_ptr(), B * H * W, C, C, parts.data_ptr(), ctypes.byref(tiles), ops._stream())
    stats = parts[: tiles.value * 2 * C].reshape(tiles.value, 2, C)
    rm_d, rv_d, nbt = rm.to(DEV), rv.to(DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    out = ops.BNTrainFn.apply(xd, stats, gamma.to(DEV), beta.to(DEV), rd, relu, (rm_d, rv_d, nbt) if track else None, 0.1)
    close(nchw(out), y, 2e-5, "bn fwd")
    out.backward(nhwc(gy).to(DEV))
    close(nchw(xd.grad), xr.grad, 1e-4, "bn dx")
    if res:
        close(nchw(rd.grad), rr.grad, 1e-5, "bn dres")
    if track:
        close(rm_d, rm_r, 1e-5, "running mean")
        close(rv_d, rv_r, 1e-5, "running var")
        assert int(nbt) == 1
    else:
        assert torch.equal(rm_d.cpu(), rm)


@pytest.mark.parametrize("C,H,W,relu,res,track", [(64, 17, 33, True, False, True), (256, 9, 17, True, True, False),
                                                    (512, 9, 17, False, False, True), (256, 33, 65, True, True, True)])
def test_batchnorm_train_limb_planes(C, H, W, relu, res, track):
    """The limb-writing BatchNorm of the pre-split path (csrc/norm_l2.hip): conv(1x1) -> BN (+residual, +ReLU) -> conv(3x3),
    the BN output existing as limb planes only.  Forward values (rebuilt from the planes), the scale bound, the second
    conv's output, and every gradient (input, residual, both weights) against fp32 torch on the CPU."""
    from onda_amd import ops
    if not (ops.CONV_MODE == "f16x2" and ops.H2_PATH == "dma"):
        pytest.skip("limb planes exist in the f16x2 / dma configuration only")
    g = torch.Generator().manual_seed(C + H + relu)
    B, Cin = 2, 64
    x = torch.randn(B, Cin, H, W, generator=g)
    w1 = torch.randn(C, Cin, 1, 1, generator=g) / Cin ** 0.5
    w2 = torch.randn(64, C, 3, 3, generator=g) / (9 * C) ** 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    r = torch.randn(B, C, H, W, generator=g) * 3 if res else None
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    xr, w1r, w2r = (t.clone().requires_grad_(True) for t in (x, w1, w2))
    rr = r.clone().requires_grad_(True) if res else None
    rm_r, rv_r = rm.clone(), rv.clone()
    y1 = F.conv2d(xr, w1r)
    z = F.batch_norm(y1, rm_r if track else None, rv_r if track else None, gamma, beta, True, 0.1, 1e-5)
    if res:
        z = z + rr
    if relu:
        z = F.relu(z)
    y2 = F.conv2d(z, w2r, None, 1, 2, 2)
    gy = torch.randn(y2.shape, generator=g)
    y2.backward(gy)

    xd = nhwc(x).to(DEV).requires_grad_(True)
    w1d, w2d = w1.to(DEV).requires_grad_(True), w2.to(DEV).requires_grad_(True)
    rd = nhwc(r).to(DEV).requires_grad_(True) if res else None
    rm_d, rv_d, nbt = rm.to(DEV), rv.to(DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    yd, stats = ops.Conv2dFn.apply(xd, w1d, None, ops._PackCache(), 1, 1, 0, 4, None)
    assert stats.shape[1] == 4
    ext = stats.cpu()
    assert torch.all(ext[:, 2].min(0).values <= y1.detach().amin((0, 2, 3)) + 1e-5)
    assert torch.all(ext[:, 3].max(0).values >= y1.detach().amax((0, 2, 3)) - 1e-5)
    zd = ops.BNTrainLimbFn.apply(yd, stats, gamma.to(DEV), beta.to(DEV), rd, relu, (rm_d, rv_d, nbt) if track else None, 0.1)
    assert ops.is_limb_only(zd) and zd.shape == (B, H, W, C)
    lb = ops.limbs_of(zd)
    bound, true_max = float(lb.amax.max()), float(z.detach().abs().max())
    assert true_max <= bound * (1 + 1e-6) and bound <= (2.0 if res else 1.0 + 1e-4) * true_max + 1e-6, (bound, true_max)
    close(nchw(ops.materialize(zd)), z, 2e-5, "bn fwd (limb planes)")
    y2d, _ = ops.Conv2dFn.apply(zd, w2d, None, ops._PackCache(), 1, 2, 2, False, None)
    close(nchw(y2d), y2, 3e-5, "conv on limb planes")
    y2d.backward(nhwc(gy).to(DEV))
    close(nchw(xd.grad), xr.grad, 2e-4, "dx through BN")
    close(w2d.grad, w2r.grad, 1e-4, "wgrad from limb-only x")
    close(w1d.grad, w1r.grad, 2e-4, "wgrad from limb-only dy")
    if res:
        close(nchw(rd.grad), rr.grad, 1e-4, "bn dres")
    if track:
        close(rm_d, rm_r, 1e-5, "running mean")
        close(rv_d, rv_r, 1e-5, "running var")
        assert int(nbt) == 1


@pytest.mark.parametrize("C,H,W,B,first,relu,res", [(256, 33, 65, 4, 0, True, True), (64, 17, 33, 3, 0, False, False),
                                                    (128, 33, 41, 5, 2, True, True), (2048, 9, 17, 2, 0, True, False)])
def test_batchnorm_statistics_inside_the_apply_launches(C, H, W, B, first, relu, res):
    """onda_bn_train_l2 / onda_bn_bwd_l2(fuse_sums) (round 6: the small statistics passes run by the first workgroups of the apply
    launches, everybody waiting for an atomic count; off by default since its step-level A/B, ops.FUSE_BN_FINALIZE) against the
    separate launches: the same arithmetic in the same order, so limb rows, statistics, running buffers and gradients must be
    IDENTICAL -- one row group, two row groups with a straddling statistics row, more finalizing workgroups than apply work."""
    from onda_amd import ops
    if not (ops.CONV_MODE == "f16x2" and ops.H2_PATH == "dma"):
        pytest.skip("limb planes exist in the f16x2 / dma configuration only")
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, H, W, 64, generator=g).to(DEV)
    w1 = (torch.randn(C, 64, 1, 1, generator=g) / 8).to(DEV)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), torch.randn(C, generator=g).to(DEV)
    r = (torch.randn(B, H, W, C, generator=g) * 3).to(DEV) if res else None
    gy = torch.randn(B, H, W, C, generator=g).to(DEV)

    def run(fused):
        old, ops.FUSE_BN_FINALIZE = ops.FUSE_BN_FINALIZE, fused
        try:
            rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
            xd, wd = x.clone().requires_grad_(True), w1.clone().requires_grad_(True)
            rd = r.clone().requires_grad_(True) if res else None
            with ops.row_groups(first):
                yd, stats = ops.Conv2dFn.apply(xd, wd, None, ops._PackCache(), 1, 1, 0, 4, None)
                zd = ops.BNTrainLimbFn.apply(yd, stats, gamma, beta, rd, relu, (rm, rv, nbt), 0.1)
                lb = ops.limbs_of(zd)
                zd.backward(gy)  # BatchNorm backward (dx as limb rows) -> the conv's data and weight gradients
            torch.cuda.synchronize()
            # (the scale of a limb tensor = the maximum over its buffer's 64 slots, every 32nd float; floats 1..3 carry the fused
            #  launch's hand-over counter and its "gave up" flag)
            return (lb.planes.clone(), lb.amax[::32].max(), rm, rv, xd.grad.clone(), wd.grad.clone(),
                    rd.grad.clone() if res else torch.zeros(1), lb.amax.view(torch.int32)[1:3].clone())
        finally:
            ops.FUSE_BN_FINALIZE = old

    a, b = run(True), run(False)
    for name, u, v in zip(("out limbs", "out scale", "running mean", "running var", "dx through the conv", "dw", "dres"), a, b):
        assert torch.equal(u, v), name
    assert int(a[7][0]) == (C + 15) // 16 * (2 if first else 1) and int(b[7][0]) == 0  # (the fused launch ran: its finalizers counted)
    assert int(a[7][1]) == 0, "the hand-over's bounded wait gave up"


@pytest.mark.parametrize("C,H,W,B,first,relu,res", [(256, 65, 129, 4, 2, True, True), (64, 33, 41, 5, 2, True, False),
                                                    (128, 16, 16, 4, 2, False, True), (256, 9, 17, 4, 1, True, False)])
def test_batchnorm_row_groups(C, H, W, B, first, relu, res):
    """Two micro-batches through conv -> BatchNorm (+residual, +ReLU) -> conv as ONE launch train (ops.row_groups: the
    student's source-replay and target batches, prototypes.py:418-450): each row group is normalised with its own batch
    statistics, only the second one moves the running statistics -- against fp32 torch on the CPU running the two batches
    one after the other (frozen / tracked), forward, all gradients and the running buffers.  Sizes: group boundaries inside
    a 256-row and inside a 128-row tile (the statistics row finalize has to split), tile-aligned ones, whole rounds of tiles
    with a stream-K remainder (4 x 65 x 129)."""
    from onda_amd import ops
    if not ops.row_groups_supported():
        pytest.skip("row groups exist in the f16x2 / dma configuration only")
    g = torch.Generator().manual_seed(C + H + B)
    Cin = 64
    x = torch.randn(B, Cin, H, W, generator=g)
    x[first:] = x[first:] * 1.7 + 0.4  # the two groups have visibly different statistics
    w1 = torch.randn(C, Cin, 1, 1, generator=g) / Cin ** 0.5
    w2 = torch.randn(64, C, 3, 3, generator=g) / (9 * C) ** 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    r = torch.randn(B, C, H, W, generator=g) * 3 if res else None
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    xr, w1r, w2r = (t.clone().requires_grad_(True) for t in (x, w1, w2))
    rr = r.clone().requires_grad_(True) if res else None
    rm_r, rv_r = rm.clone(), rv.clone()
    y1 = F.conv2d(xr, w1r)
    z = torch.cat([F.batch_norm(y1[:first], None, None, gamma, beta, True, 0.1, 1e-5),
                   F.batch_norm(y1[first:], rm_r, rv_r, gamma, beta, True, 0.1, 1e-5)], 0)
    if res:
        z = z + rr
    if relu:
        z = F.relu(z)
    y2 = F.conv2d(z, w2r, None, 1, 2, 2)
    gy = torch.randn(y2.shape, generator=g)
    y2.backward(gy)

    xd = nhwc(x).to(DEV).requires_grad_(True)
    w1d, w2d = w1.to(DEV).requires_grad_(True), w2.to(DEV).requires_grad_(True)
    rd = nhwc(r).to(DEV).requires_grad_(True) if res else None
    rm_d, rv_d, nbt = rm.to(DEV), rv.to(DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    with ops.row_groups(first):
        yd, stats = ops.Conv2dFn.apply(xd, w1d, None, ops._PackCache(), 1, 1, 0, 4, None)
        zd = ops.BNTrainLimbFn.apply(yd, stats, gamma.to(DEV), beta.to(DEV), rd, relu, (rm_d, rv_d, nbt), 0.1)
    assert ops.is_limb_only(zd) and zd.shape == (B, H, W, C)
    lb = ops.limbs_of(zd)
    bound, true_max = float(lb.amax.max()), float(z.detach().abs().max())
    assert true_max <= bound * (1 + 1e-6), (bound, true_max)
    close(nchw(ops.materialize(zd)), z, 2e-5, "bn fwd (two row groups)")
    y2d, _ = ops.Conv2dFn.apply(zd, w2d, None, ops._PackCache(), 1, 2, 2, False, None)
    close(nchw(y2d), y2, 3e-5, "conv on limb planes")
    y2d.backward(nhwc(gy).to(DEV))
    close(nchw(xd.grad), xr.grad, 2e-4, "dx through the grouped BN")
    close(w2d.grad, w2r.grad, 1e-4, "wgrad (second conv)")
    close(w1d.grad, w1r.grad, 2e-4, "wgrad through the grouped BN")
    if res:
        close(nchw(rd.grad), rr.grad, 1e-4, "bn dres")
    close(rm_d, rm_r, 1e-5, "running mean: moved by the second group only")
    close(rv_d, rv_r, 1e-5, "running var: moved by the second group only")
    assert int(nbt) == 1


def test_bn_fold_matches_eval_batchnorm():
    from onda_amd import ops
    g = torch.Generator().manual_seed(9)
    C = 256
    x = torch.randn(2, C, 9, 17, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    ref = F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, 1e-5)
    sc, sh = ops.bn_eval_fold(gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV))
    got = x * sc.cpu()[None, :, None, None] + sh.cpu()[None, :, None, None]
    close(got, ref, 1e-6, "bn fold")


@pytest.mark.parametrize("n,relu,drop", [(5, True, False), (1, False, True), (1, False, False)])
def test_groupnorm_concat(n, relu, drop):
    from onda_amd import ops
    g = torch.Generator().manual_seed(n * 7 + relu)
    B, C, H, W = 2, 256, 9, 17
    xs = [torch.randn(B, C, H, W, generator=g) * (i + 1) + 0.3 for i in range(n)]
    gs = [torch.rand(C, generator=g) + 0.5 for _ in range(n)]
    bs = [torch.randn(C, generator=g) for _ in range(n)]
    mask = (torch.empty(B, C, 1, 1).bernoulli_(0.9, generator=g) / 0.9) if drop else None
    xr = [x.clone().requires_grad_(True) for x in xs]
    gr = [t.clone().requires_grad_(True) for t in gs]
    br = [t.clone().requires_grad_(True) for t in bs]
    outs = []
    for i in range(n):
        y = F.group_norm(xr[i], 32, gr[i], br[i], 1e-5)
        y = F.relu(y) if relu else y
        outs.append(y * mask if drop else y)
    ref = torch.cat(outs, 1)
    gy = torch.randn(ref.shape, generator=g)
    ref.backward(gy)
    xd = [nhwc(x).to(DEV).requires_grad_(True) for x in xs]
    gd = [t.to(DEV).requires_grad_(True) for t in gs]
    bd = [t.to(DEV).requires_grad_(True) for t in bs]
    chmul = mask.reshape(B, C).to(DEV) if drop else None
    cat = ops.GNConcatFn.apply(relu, chmul, *xd, *gd, *bd)
    close(nchw(cat), ref, 2e-5, "gn fwd")
    cat.backward(nhwc(gy).to(DEV))
    for i in range(n):
        close(nchw(xd[i].grad), xr[i].grad, 2e-4, f"gn dx{i}")
        close(gd[i].grad, gr[i].grad, 1e-4, f"gn dgamma{i}")
        close(bd[i].grad, br[i].grad, 1e-4, f"gn dbeta{i}")


@pytest.mark.parametrize("H,W", [(64, 128), (33, 65), (8, 9)])
def test_maxpool_ceil(H, W):
    from onda_amd import ops
    g = torch.Generator().manual_seed(H)
    x = F.relu(torch.randn(2, 64, H, W, generator=g))  # many exact ties at 0, like the post-ReLU stem
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1, ceil_mode=True)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    xd = nhwc(x).to(DEV).requires_grad_(True)
    y = ops.MaxPoolFn.apply(xd)
    assert torch.equal(nchw(y).cpu(), yr.detach())
    y.backward(nhwc(gy).to(DEV))
    assert torch.equal(nchw(xd.grad).cpu(), xr.grad)
    # the same pool with its result written as limb rows (what the model uses behind the stem): values to the format's 22 bits,
    # the same window choice (identical gradient)
    if ops.limb_mode(64):
        xl = nhwc(x).to(DEV).requires_grad_(True)
        ops.activation_scale(xl)  # max|x| known, as behind BatchNorm + ReLU
        yl = ops.MaxPoolFn.apply(xl, True)
        assert ops.is_limb_only(yl)
        close(nchw(ops.materialize(yl)), yr.detach(), 5e-7, "pool output as limb rows")
        yl.backward(nhwc(gy).to(DEV))
        assert torch.equal(nchw(xl.grad).cpu(), xr.grad)


@pytest.mark.parametrize("known_scale", [False, True])
def test_se_block(known_scale):
    from onda_amd import ops
    g = torch.Generator().manual_seed(3)
    B, C, R, H, W = 2, 1280, 80, 9, 17
    x = torch.randn(B, C, H, W, generator=g)
    w1, b1 = torch.randn(R, C, generator=g) / 30, torch.randn(R, generator=g) * 0.1
    w2, b2 = torch.randn(C, R, generator=g) / 9, torch.randn(C, generator=g) * 0.1
    ps = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    z = torch.sigmoid(F.linear(F.relu(F.linear(ps[0].mean((2, 3)), ps[1], ps[2])), ps[3], ps[4]))
    ref = ps[0] * z[:, :, None, None]
    gy = torch.randn(ref.shape, generator=g)
    ref.backward(gy)
    ds = [nhwc(x).to(DEV).requires_grad_(True)] + [t.to(DEV).requires_grad_(True) for t in (w1, b1, w2, b2)]
    if known_scale:  # the producer left max|x| behind (GroupNorm apply does): the gated result exists as limb planes only
        ops.activation_scale(ds[0])
    out = ops.SEScaleFn.apply(*ds)
    assert ops.is_limb_only(out) == (known_scale and ops.limb_mode(C))
    close(nchw(ops.materialize(out)), ref, 2e-5, "se fwd")
    out.backward(nhwc(gy).to(DEV))
    close(nchw(ds[0].grad), ps[0].grad, 1e-4, "se dx")
    for i, name in enumerate(("dw1", "db1", "dw2", "db2"), 1):
        close(ds[i].grad, ps[i].grad, 2e-4, "se " + name)


def _head_out(logits_nchw):
    """Bring CPU logits [B,K,h,w] to the device in the model's own output layout."""
    B, K, h, w = logits_nchw.shape
    pad = torch.zeros(B, h, w, 32)
    pad[..., :K] = logits_nchw.permute(0, 2, 3, 1)
    return pad.to(DEV)[..., :K].permute(0, 3, 1, 2)


@pytest.mark.parametrize("h,w,H,W", [(9, 17, 64, 128), (65, 129, 512, 1024), (5, 7, 11, 13)])
def test_upsample_align_corners(h, w, H, W):
    from onda_amd import ops
    g = torch.Generator().manual_seed(h)
    lo = torch.randn(2, 19, h, w, generator=g) * 3
    lr = lo.clone().requires_grad_(True)
    up = F.interpolate(lr, size=(H, W), mode="bilinear", align_corners=True)
    gy = torch.randn(up.shape, generator=g)
    up.backward(gy)
    ld = _head_out(lo).detach().requires_grad_(True)
    got = ops.UpsampleFn.apply(ld, (H, W))
    close(got, up, 2e-6, "upsample fwd")
    got.backward(gy.to(DEV))
    close(ld.grad, lr.grad, 2e-5, "upsample bwd")
    cls = ops.upsample_argmax(_head_out(lo), (H, W)).cpu()
    ref_cls = up.softmax(1).argmax(1)
    top2 = up.detach().topk(2, dim=1)[0]
    decided = (top2[:, 0] - top2[:, 1]) > 1e-5  # exclude numerical ties of the reference itself
    assert torch.equal(cls.long()[decided], ref_cls[decided])
    assert (cls.long() != ref_cls).float().mean().item() < 1e-4


@pytest.mark.parametrize("K,ld,hw,HW", [(19, 32, (9, 17), (64, 128)), (19, 19, (9, 17), (64, 128)), (19, 20, (5, 7), (11, 13)),
                                        (40, 40, (5, 7), (33, 47)), (19, 32, (65, 129), (512, 1024))])
def test_upsample_argmax_confusion_matrix(K, ld, hw, HW):
    """The evaluation tail (adaptation_model.py:127-166, func.py:77-79 fast_hist): hist += confusion matrix of the upsampled
    argmax against the labels, labels >= K ignored; counted per workgroup in LDS for K <= 32, per pixel in memory above;
    16-byte and 4-byte class loads (row stride 32 / 20 / 19 floats) give the same class map."""
    from onda_amd import ops
    from onda_amd.framework.utils.func import fast_hist
    (h, w), (H, W) = hw, HW
    B = 8 if H == 512 else 2
    g = torch.Generator().manual_seed(K * 1000 + ld)
    rows = (torch.randn(B, h, w, ld, generator=g) * 3).to(DEV)
    out = rows[..., :K].permute(0, 3, 1, 2)
    assert ops.logits_rows(out)[1] == ld  # read in place, with this row stride
    labels = torch.randint(0, K + 3, (B, H, W), generator=g).to(torch.uint8)
    labels[labels >= K] = 255
    labels[0, : H // 2] = 3  # a block of one class: many pixels of a workgroup in one cell
    hist = torch.arange(K * K, dtype=torch.int64).reshape(K, K).to(DEV)  # accumulated INTO, not overwritten
    before = hist.cpu().numpy().copy()
    ops.upsample_argmax_hist(out, labels.to(DEV), hist, K)
    cls = ops.upsample_argmax(out, (H, W)).cpu().numpy()
    ref = F.interpolate(out.cpu().contiguous(), size=(H, W), mode="bilinear", align_corners=True)
    top2 = ref.topk(2, dim=1)[0]
    decided = ((top2[:, 0] - top2[:, 1]) > 1e-5).numpy()
    assert np.array_equal(cls[decided], ref.argmax(1).numpy()[decided])
    want = fast_hist(labels.numpy().flatten().astype(np.int64), cls.flatten().astype(np.int64), K)
    assert np.array_equal(hist.cpu().numpy() - before, want.astype(np.int64))
    assert int(want.sum()) == int((labels != 255).sum())


def test_upsample_argmax_confusion_matrix_all_ignored():
    """Every label outside [0, K): the matrix is left exactly as it was (fast_hist keeps nothing, func.py:77-79)."""
    from onda_amd import ops
    rows = torch.randn(1, 9, 17, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    out = rows[..., :19].permute(0, 3, 1, 2)
    hist = torch.arange(361, dtype=torch.int64).reshape(19, 19).to(DEV)
    ops.upsample_argmax_hist(out, torch.full((1, 64, 128), 255, dtype=torch.uint8, device=DEV), hist, 19)
    assert torch.equal(hist.cpu(), torch.arange(361, dtype=torch.int64).reshape(19, 19))


@pytest.mark.parametrize("case", ["mixed", "none_ignored", "all_ignored"])
def test_losses_golden(golden, case):
    """Fused CE/RCE/MRKLD kernel against the reference's own numbers (fixture G3)."""
    from onda_amd import ops
    g = golden("g3_losses")
    logits = torch.from_numpy(g[f"{case}_logits"])
    target = torch.from_numpy(g[f"{case}_target"])
    out = _head_out(logits).detach().requires_grad_(True)
    total, ce, rce, reg = ops.seg_losses(out, target.to(DEV), 0.1, 1.0, 0.1)
    np.testing.assert_allclose(rce.item(), g[f"{case}_rce"], rtol=2e-6)
    np.testing.assert_allclose(reg.item(), g[f"{case}_mrkld"], rtol=2e-6)
    if case == "all_ignored":
        # the reference's value is NaN and its GRADIENT is finite: autograd scatters an empty gradient back through
        # predict[mask] (loss.py:36-44), so CE contributes exact zeros and the total's gradient is RCE + MRKLD (G3 holds both)
        assert torch.isnan(ce).item() and torch.isnan(total).item()
        assert not g["all_ignored_grad_ce"].any()
    else:
        np.testing.assert_allclose(ce.item(), g[f"{case}_ce"], rtol=2e-6)
    total.backward()
    assert torch.isfinite(out.grad).all()
    close(out.grad, torch.from_numpy(g[f"{case}_grad"]), 2e-5, "loss grad")
    if case == "all_ignored":  # CE alone: exact zeros, as the reference
        out1 = _head_out(logits).detach().requires_grad_(True)
        ops.seg_losses(out1, target.to(DEV), 1.0, 0.0, 0.0)[0].backward()
        assert not out1.grad.any()


def test_losses_full_size_property():
    """At 4x65x129 pixels: kernel vs oracle, and the gradient sums to zero over classes for CE."""
    from onda_amd import ops
    from oracle import losses
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(4, 19, 65, 129, generator=g) * 4
    target = torch.randint(0, 19, (4, 65, 129), generator=g)
    target[torch.rand(4, 65, 129, generator=g) < 0.4] = 255
    lr = logits.clone().requires_grad_(True)
    ref = losses.target_loss(lr, target)
    ref["Total target loss"].backward()
    out = _head_out(logits).detach().requires_grad_(True)
    total, ce, rce, reg = ops.seg_losses(out, target.to(DEV), 0.1, 1.0, 0.1)
    np.testing.assert_allclose(total.item(), ref["Total target loss"].item(), rtol=1e-5)
    total.backward()
    close(out.grad, lr.grad, 1e-4, "loss grad full")
    out2 = _head_out(logits).detach().requires_grad_(True)
    ops.seg_losses(out2, target.to(DEV), 1.0, 0.0, 0.0)[0].backward()
    assert out2.grad.sum(1).abs().max().item() < 1e-9


def test_softmax_stats():
    from onda_amd import ops
    g = torch.Generator().manual_seed(8)
    logits = torch.randn(2, 19, 9, 17, generator=g) * 3
    conf, probs, am = ops.softmax_stats(_head_out(logits), True, True)
    p = logits.softmax(1)
    np.testing.assert_allclose(conf.item(), p.max(1)[0].mean().item(), rtol=1e-6)
    close(probs, p.permute(0, 2, 3, 1).reshape(-1, 19), 1e-6, "softmax probs")
    assert torch.equal(am.cpu().long(), logits.permute(0, 2, 3, 1).reshape(-1, 19).argmax(1))


@pytest.mark.parametrize("regime", ["far", "near"])
def test_prototypes_golden(golden, regime):
    """Pseudo-labels bit-exact, soft map / EMA / append / sigma close, against the reference's
    own outputs (fixture G4)."""
    from onda_amd.framework.domain_adaptation.methods.prototype_handler import prototype_handler
    g = golden("g4_prototypes")
    t = lambda k: torch.from_numpy(g[f"{regime}_{k}"])
    feat = nhwc(t("feat")).to(DEV).permute(0, 3, 1, 2)  # the model's own layout
    prior, out = t("prior").to(DEV), t("out").to(DEV)
    for metric in ("mahalanobis", "euclidean"):
        for tau in (1, 2):
            for th in (0, 0.3):
                h = prototype_handler(0.9995, tau, th, metric)
                h.prototypes, h.squared_mean, h.counter = t("proto").to(DEV), t("sqmean").to(DEV), t("counter").to(DEV)
                tag = f"{regime}_{metric}_t{tau}_th{th}"
                labels = h.pseudo_labels(feat, prior)
                soft = h.pseudo_labels(feat, prior, soft=True)
                assert labels.shape == (306, 1) and labels.dtype == torch.int64
                assert np.array_equal(labels.cpu().numpy(), g[tag + "_labels"]), tag
                close(soft, torch.from_numpy(g[tag + "_soft"]), 2e-5, tag)
    h = prototype_handler(0.9995, 1, 0.3, "mahalanobis")
    h.prototypes, h.squared_mean, h.counter = t("proto").to(DEV), t("sqmean").to(DEV), t("counter").to(DEV)
    close(h.global_var(), t("global_var"), 1e-5, "sigma")
    h.ma(feat, out)
    close(h.prototypes, t("ma_proto"), 1e-6, "ma proto")
    close(h.squared_mean, t("ma_sqmean"), 1e-6, "ma sqmean")
    h2 = prototype_handler(0.9995, 1, 0.3, "mahalanobis")
    h2.append(feat, out)
    h2.append(feat * 0.5 + 0.1, out.flip(0))
    close(h2.prototypes, t("append_proto"), 1e-5, "append proto")
    close(h2.squared_mean, t("append_sqmean"), 1e-5, "append sqmean")
    assert torch.equal(h2.counter.cpu(), t("append_counter"))
    with pytest.raises(ValueError):
        prototype_handler(distance_metric="cosine")


def test_prototypes_full_size():
    """BASELINE size (N = 4*65*129 = 33 540 pixels): labels identical to the oracle except at
    numerical ties of the threshold / argmax, which are counted and bounded."""
    from onda_amd.framework.domain_adaptation.methods.prototype_handler import prototype_handler
    from onda_amd.synthetic import synth_prototypes
    from oracle import prototypes as op
    g = torch.Generator().manual_seed(99)
    proto, sq, cnt = synth_prototypes()
    N = 4 * 65 * 129
    cls = torch.randint(0, 19, (N,), generator=g)
    mix = torch.rand(N, 1, generator=g) * 0.5
    other = proto[torch.randint(0, 19, (N,), generator=g)]
    rows = proto[cls] * (1 - mix) + other * mix + 0.8 * torch.randn(N, 256, generator=g)
    feat = rows.reshape(4, 65, 129, 256)
    prior = (2 * torch.randn(4, 19, 65, 129, generator=g)).softmax(1)
    ref_labels, ref_soft, ref_conf = op.assign(feat.permute(0, 3, 1, 2), prior, (proto, sq, cnt), 1.0, 0.3)
    h = prototype_handler(0.9995, 1, 0.3, "mahalanobis")
    h.prototypes, h.squared_mean, h.counter = proto.to(DEV), sq.to(DEV), cnt.to(DEV)
    fd = feat.to(DEV).permute(0, 3, 1, 2)
    labels, soft, stats = h.assign_stats(fd, prior.to(DEV))
    mism = (labels.cpu() != ref_labels).reshape(-1)
    if mism.any():
        top2 = ref_soft.topk(2, dim=1)[0][mism]
        near_tie = ((top2[:, 0] - top2[:, 1]).abs() < 1e-5) | ((top2[:, 0] - 0.3).abs() < 1e-5)
        assert near_tie.all(), "label mismatch away from a numerical tie"
    assert mism.sum().item() <= 3
    close(soft, ref_soft, 5e-5, "soft full")
    np.testing.assert_allclose(stats[0], ref_conf.item(), rtol=1e-5)
    np.testing.assert_allclose(stats[1], ref_soft.max(1)[0].mean().item(), rtol=1e-5)
    np.testing.assert_allclose(stats[2], prior.max(1)[0].mean().item(), rtol=1e-5)
    assert (labels != 255).float().mean().item() > 0.2 and (labels == 255).any().item()
    # class sums: linearity / counts
    out = torch.randn(4, 19, 65, 129, generator=g)
    flat, K, C = h.class_statistics(fd, out.to(DEV))
    s, n = op.class_sums(feat.permute(0, 3, 1, 2), out)
    close(flat[: K * C].reshape(K, C), s, 1e-5, "class sums")
    assert torch.equal(flat[2 * K * C:].cpu(), n) and n.sum().item() == N


def test_replay_sgd_golden(golden):
    """Duplicate-aware SGD against torch's for-loop SGD run on the reference's group layout (G6)."""
    from onda_amd.optim import ReplaySGD
    g = golden("g6_optimizer")
    ps = {n: torch.nn.Parameter(torch.from_numpy(g[n + "_init"]).to(DEV)) for n in ("w3", "w4", "w1", "h1")}
    w3, w4, w1, h1 = ps["w3"], ps["w4"], ps["w1"], ps["h1"]
    opt = ReplaySGD([{"params": [w3, w4, w1, w3, w4, w3, w4, w4], "lr": 8e-4}, {"params": [h1], "lr": 1e-4}],
                    lr=1e-5, momentum=0.9, weight_decay=1e-4)
    for s in range(3):
        for n, p in ps.items():
            p.grad = torch.from_numpy(g[f"{n}_grad{s}"]).to(DEV)
        v = w3._version
        opt.step()
        assert w3._version > v
        for n, p in ps.items():
            close(p, torch.from_numpy(g[f"{n}_after{s}"]), 2e-6, f"{n} step {s}")
    # grad_scale (rank sums left by the gradient exchange): sums x 1/world give the same trajectory, for one step() only
    qs = {n: torch.nn.Parameter(torch.from_numpy(g[n + "_init"]).to(DEV)) for n in ("w3", "w4", "w1", "h1")}
    opt2 = ReplaySGD([{"params": [qs[k] for k in ("w3", "w4", "w1", "w3", "w4", "w3", "w4", "w4")], "lr": 8e-4},
                      {"params": [qs["h1"]], "lr": 1e-4}], lr=1e-5, momentum=0.9, weight_decay=1e-4)
    for s in range(2):
        for n, p in qs.items():
            p.grad = torch.from_numpy(g[f"{n}_grad{s}"]).to(DEV) * 4.0
        opt2.grad_scale = 0.25
        opt2.step()
        assert opt2.grad_scale == 1.0
        for n, p in qs.items():
            close(p, torch.from_numpy(g[f"{n}_after{s}"]), 2e-6, f"scaled {n} step {s}")


def test_ema_multi():
    from onda_amd import ops
    g = torch.Generator().manual_seed(4)
    ks = [torch.randn(n, generator=g) for n in (7, 1000, 33333)]
    qs = [torch.randn(n, generator=g) for n in (7, 1000, 33333)]
    kd, qd = [t.to(DEV) for t in ks], [t.to(DEV) for t in qs]
    ops.ema_multi([(k, q, 0.999, 1.0 - 0.999) for k, q in zip(kd[:2], qd[:2])] + [(kd[2], qd[2], 0.0, 1.0)])
    for i in range(2):
        close(kd[i], ks[i] * 0.999 + qs[i] * (1.0 - 0.999), 1e-6, "ema")
    assert torch.equal(kd[2].cpu(), qs[2])


@pytest.mark.parametrize("metric", ["mahalanobis", "euclidean"])
def test_prototype_distance_matrices(metric):
    """prototype_handler.distance / mahalanobis_distance / distance_measure, onehot and get_proto_array (reference
    prototype_handler.py:76-86, :111-138) against the oracle; N not a multiple of the pixels per workgroup."""
    from onda_amd.framework.domain_adaptation.methods.prototype_handler import prototype_handler
    from onda_amd.synthetic import synth_prototypes
    from oracle import prototypes as op
    g = torch.Generator().manual_seed(17)
    proto, sq, cnt = synth_prototypes()
    feat = proto[torch.randint(0, 19, (2 * 9 * 13,), generator=g)].reshape(2, 9, 13, 256) + 0.7 * torch.randn(2, 9, 13, 256, generator=g)
    feat = feat.permute(0, 3, 1, 2).contiguous()
    h = prototype_handler(0.9995, 1, 0.3, metric)
    h.prototypes, h.squared_mean, h.counter = proto.to(DEV), sq.to(DEV), cnt.to(DEV)
    ref = op.distances(feat, (proto, sq, cnt), metric)
    got = h.distance_measure(feat.to(DEV))
    assert got.shape == ref.shape and got.min(dim=1)[0].abs().max().item() == 0.0
    close(got, ref, 2e-6, f"{metric} distances")
    close(h.mahalanobis_distance(feat.to(DEV)) if metric == "mahalanobis" else h.distance(feat.to(DEV)), ref, 2e-6, "named")
    out = torch.randn(2, 19, 9, 13, generator=g)
    rows = op.to_rows(out)
    oh = h.onehot(rows.to(DEV)).cpu()
    assert torch.equal(oh.argmax(1), rows.argmax(1)) and torch.equal(oh.sum(1), torch.ones(rows.shape[0]))
    sums, counts = h.get_proto_array(feat.to(DEV), out.to(DEV))
    s_ref, n_ref = op.class_sums(feat, out)
    close(sums, s_ref, 1e-5, "proto array")
    assert torch.equal(counts.cpu(), n_ref)


@pytest.mark.parametrize("sk,Co,taps,Cin,co_real,ci_real,flat_k", [
    (128, 64, 1, 64, 64, 64, 0),      # 16 slab groups per element, vector store
    (32, 256, 1, 1024, 256, 1024, 0),  # 4 slab groups
    (3, 128, 1, 256, 100, 250, 0),     # one group; padded rows / columns dropped, scalar store (250 % 4 != 0)
    (14, 256, 9, 256, 256, 256, 0),    # taps: workgroup per 128 channels x 9 taps, transposed through LDS
    (7, 64, 9, 128, 64, 128, 0),       # taps kernel, one slab batch with a zero-padded tail
    (56, 64, 9, 64, 64, 64, 0),        # taps with Cin < 128: generic kernel, strided stores
    (128, 64, 1, 160, 64, 3, 49),      # stem: packed K = tap7 * 3 + c3 -> OIHW [n][c3][7 x 7]
])
def test_slab_reduction_variants(sk, Co, taps, Cin, co_real, ci_real, flat_k):
    """onda_wgrad_reduce (split-K slabs [sk][Cout][taps][Cin] -> OIHW gradient): every launch variant against a float64
    sum; overwrite and accumulate; bit-reproducible (fixed order inside and across the slab groups)."""
    from onda_amd import ops
    from onda_amd._lib import call
    g = torch.Generator().manual_seed(sk * 31 + Cin)
    slabs = torch.randn(sk, Co, taps, Cin, generator=g)
    ref = slabs.double().sum(0)  # [Co][taps][Cin]
    if flat_k:
        kk = flat_k * ci_real
        want = ref[:co_real, 0, :kk].reshape(co_real, flat_k, ci_real).permute(0, 2, 1)  # [n][c3][tap7]
        shape = (co_real, ci_real, flat_k)
    else:
        want = ref[:co_real, :, :ci_real].permute(0, 2, 1)  # [n][c][tap]
        shape = (co_real, ci_real, taps)
    sd = slabs.to(DEV)
    prev = torch.randn(shape, generator=g)
    outs = []
    for acc in (0, 1, 1):
        dw = prev.to(DEV).contiguous()
        call("onda_wgrad_reduce", ops._p(sd), ops._p(dw), sk, Co, taps, Cin, co_real, ci_real, flat_k, acc, ops._stream())
        outs.append(dw.cpu())
        close(dw.reshape(shape), want + (prev.double() if acc else 0.0), 2e-6, f"slab sum acc={acc}")
    assert torch.equal(outs[1], outs[2])


def test_bad_arguments_raise():
    from onda_amd import ops
    with pytest.raises(RuntimeError):
        ops.conv_forward(torch.zeros(1, 4, 4, 32), torch.zeros(32, 32), 1, 1, 1, 0, 32)  # CPU tensor
    x = torch.zeros(1, 4, 4, 48, device=DEV)  # Cin not a multiple of 32
    with pytest.raises(RuntimeError, match="ONDA_EINVAL"):
        ops.conv_forward(x, torch.zeros(32, 48, device=DEV), 1, 1, 1, 0, 32)


def test_limb_row_strides_must_be_whole_32_channel_blocks():
    """Limb rows hold [32 x l1][32 x l2] per block of 32 channels (limbs.h limb_at): a row stride of 40 would put channels
    32..39 into the next row (and past the buffer on the last one).  The two public producers of limb rows refuse it
    (round-5 advisor: they still validated the two-plane contract, % 8)."""
    from onda_amd import ops
    from onda_amd._lib import call
    rows = 64
    x = torch.randn(rows, 40, device=DEV)
    amax = ops.amax_slot(torch.device(DEV))
    dst = torch.empty(2 * rows * 64, device=DEV, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="ONDA_EINVAL"):
        call("onda_split_h2", ops._p(x), rows, 40, 40, ops._p(dst), 40, 0, ops._p(amax), ops._stream())
    with pytest.raises(RuntimeError, match="ONDA_EINVAL"):  # C = 32 of a 40-wide row: still a 40-channel stride
        call("onda_split_h2", ops._p(x), rows, 32, 40, ops._p(dst), 40, 0, ops._p(amax), ops._stream())
    call("onda_split_h2", ops._p(x), rows, 32, 40, ops._p(dst), 64, 0, ops._p(amax), ops._stream())  # 64: fine
    img = torch.randn(1, 3, 16, 16, device=DEV)
    col = torch.empty(2 * 64 * 160, device=DEV, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="ONDA_EINVAL"):
        call("onda_stem_im2col_l2", ops._p(img), ops._p(amax), ops._p(col), 0, 1, 16, 16, 8, 8, 152, ops._stream())
    call("onda_stem_im2col_l2", ops._p(img), ops._p(amax), ops._p(col), 0, 1, 16, 16, 8, 8, 160, ops._stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- f16x2 specifics
def test_amax_producers():
    """max|x| as the f16x2 kernels see it: the standalone pass (channel slices, zeros) and the fused producers
    (BatchNorm apply / backward, folded-BN conv epilogue incl. stream-K fix-up tiles) all leave exactly
    tensor.abs().max() behind, on the device."""
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    try:
        g = torch.Generator().manual_seed(11)
        for mag in (1e-30, 3e-7, 0.37, 8192.0, 1e30):
            x = torch.randn(2, 5, 7, 64, generator=g)
            x = (x / x.abs().max() * mag).to(DEV)
            assert ops.activation_scale(x).max().item() == x.abs().max().item()
        assert ops.activation_scale(torch.zeros(1, 3, 3, 32, device=DEV)).max().item() == 0.0
        buf = torch.randn(2, 4, 4, 96, generator=g).to(DEV)
        buf[..., 64:] *= 1e6  # outside the slice: must not be seen
        sl = buf[..., :64]
        assert ops.activation_scale(sl).max().item() == sl.abs().max().item()
        # BatchNorm apply (+residual, ReLU) and its backward
        y = torch.randn(2, 9, 17, 64, generator=g).to(DEV).requires_grad_(True)
        stats = torch.stack([y.detach().sum((0, 1, 2)), (y.detach() ** 2).sum((0, 1, 2))])[None].contiguous()
        res = torch.randn(2, 9, 17, 64, generator=g).to(DEV)
        out = ops.BNTrainFn.apply(y, stats, torch.rand(64, device=DEV) + 0.5, torch.randn(64, device=DEV), res, True, None, 0.1)
        assert ops.known_amax(out) is not None and ops.known_amax(out).max().item() == out.abs().max().item()
        seen = {}

        class Probe(torch.autograd.Function):
            @staticmethod
            def forward(ctx, t):
                return t.view_as(t)

            @staticmethod
            def backward(ctx, gr):
                seen["amax"], seen["true"] = ops.known_amax(gr), gr.abs().max().item()
                return gr

        y2 = torch.randn(2, 9, 17, 64, generator=g).to(DEV).requires_grad_(True)
        out2 = ops.BNTrainFn.apply(Probe.apply(y2), stats, torch.rand(64, device=DEV) + 0.5, torch.randn(64, device=DEV), None, True,
                                   None, 0.1)
        out2.backward(torch.randn(out2.shape, generator=g).to(DEV))
        assert seen["amax"] is not None and seen["amax"].max().item() == seen["true"]
        # folded-BN conv epilogue, one tile per workgroup and stream-K (fix-up kernel) schedules
        x = torch.randn(4, 33, 65, 128, generator=g).to(DEV)
        wp = ops.pack_weight_fwd((torch.randn(256, 128, 3, 3, generator=g) / 34).to(DEV))
        sc, sh = (torch.rand(256, generator=g) + 0.5).to(DEV), torch.randn(256, generator=g).to(DEV)
        yy = ops.conv_forward(x, wp, 3, 1, 2, 2, 256, scale=sc, shift=sh, relu=True)[0]
        assert ops.known_amax(yy).max().item() == yy.abs().max().item()
    finally:
        ops.CONV_MODE = old


@pytest.mark.parametrize("regime", ["wide-range", "tiny", "huge", "outlier", "mixed-sign-cancel"])
def test_f16x2_accuracy_against_fp64(regime):
    """The two-limb f16 evaluation against fp64, next to what a plain fp32 conv (torch CPU) achieves on the
    same data: forward, data gradient and weight gradient stay within 2x of fp32's own error (and below
    1e-6 relative L2) over dynamic ranges that a single f16 could not hold."""
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    try:
        g = torch.Generator().manual_seed(hash(regime) & 0xFFF)
        B, C, K, H, W = 2, 128, 128, 17, 23
        x = torch.randn(B, C, H, W, generator=g)
        w = torch.randn(K, C, 3, 3, generator=g) * 0.03
        if regime == "wide-range":
            x = torch.relu(x) * torch.exp(torch.randn(x.shape, generator=g) * 3)
        elif regime == "tiny":
            x, w = x * 1e-20, w * 1e-12
        elif regime == "huge":
            x, w = x * 1e15, w * 1e10
        elif regime == "outlier":
            x[0, 0, 0, 0] = 4000.0
        else:
            x = x + 100.0
            w = w - w.mean(dim=(1, 2, 3), keepdim=True)
        gy = torch.randn(B, K, H, W, generator=g) * (1e-7 if regime == "tiny" else 1.0)
        x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
        y64 = F.conv2d(x64, w64, None, 1, 2, 2)
        y64.backward(gy.double())
        x32, w32 = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y32 = F.conv2d(x32, w32, None, 1, 2, 2)
        y32.backward(gy)
        xd, wd = nhwc(x).to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        y, _ = ops.Conv2dFn.apply(xd, wd, None, ops._PackCache(), 1, 2, 2, False, None)
        y.backward(nhwc(gy).to(DEV))

        def rel(a, ref):
            return ((a.double() - ref).norm() / ref.norm()).item()

        for name, mine, f32, ref in (("fwd", nchw(y).detach().cpu(), y32.detach(), y64.detach()),
                                     ("dgrad", nchw(xd.grad).cpu(), x32.grad, x64.grad),
                                     ("wgrad", wd.grad.cpu(), w32.grad, w64.grad)):
            e_mine, e_f32 = rel(mine, ref), rel(f32, ref)
            assert e_mine <= max(2.0 * e_f32, 4e-7) and e_mine < 1e-6, (regime, name, e_mine, e_f32)
    finally:
        ops.CONV_MODE = old


def test_f16x2_zero_and_nonfinite():
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    try:
        w = torch.randn(128, 64, 1, 1).to(DEV)
        wp = ops.pack_weight_fwd(w)
        z = ops.conv_forward(torch.zeros(1, 5, 5, 64, device=DEV), wp, 1, 1, 1, 0, 128)[0]
        assert z.abs().max().item() == 0.0
        x = torch.randn(1, 5, 5, 64, device=DEV)
        x[0, 2, 2, 3] = float("nan")
        y = ops.conv_forward(x, wp, 1, 1, 1, 0, 128)[0]
        assert torch.isnan(y[0, 2, 2]).all() and not torch.isnan(y[0, 0, 0]).any()
    finally:
        ops.CONV_MODE = old


def test_f16x2_interpixel_range():
    """The one place where two scaled f16 limbs differ from fp32: outputs that depend ONLY on elements far
    below the tensor's maximum (here: half of the pixels scaled down, through a 1x1 conv).  Full accuracy down
    to 2^-24 of the maximum (the second limb is stored times 2^11), graceful below."""
    from onda_amd import ops
    old = ops.CONV_MODE
    try:
        g = torch.Generator().manual_seed(1)
        w = torch.randn(256, 256, 1, 1, generator=g) * 0.05
        bounds = {"f16x2": {0: 4e-7, 16: 4e-7, 24: 4e-7, 28: 2e-6, 32: 5e-5}}
        for mode, table in bounds.items():
            ops.CONV_MODE = mode
            wp = ops.pack_weight_fwd(w.to(DEV))
            for shift, bound in table.items():
                x = torch.randn(1, 16, 64, 256, generator=g)
                x[:, 8:] *= 2.0 ** -shift
                y = ops.conv_forward(x.to(DEV), wp, 1, 1, 1, 0, 256)[0].cpu().double()
                ref = torch.einsum("bhwc,kc->bhwk", x.double(), w[:, :, 0, 0].double())
                for part in (slice(0, 8), slice(8, 16)):
                    err = ((y[:, part] - ref[:, part]).norm() / ref[:, part].norm()).item()
                    assert err <= bound, (mode, shift, part, err)
    finally:
        ops.CONV_MODE = old


def test_f16x2_bitwise_reproducible():
    """Same inputs -> bit-identical conv outputs, gradients and fused max|x| on every run: the only atomics on
    the path are order-independent maxima, every sum has a fixed order."""
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    try:
        g = torch.Generator().manual_seed(21)
        x0 = torch.randn(4, 33, 65, 256, generator=g).to(DEV)
        w0 = (torch.randn(256, 256, 3, 3, generator=g) / 48).to(DEV)
        gy = torch.randn(4, 33, 65, 256, generator=g).to(DEV)
        gamma, beta = torch.rand(256, device=DEV) + 0.5, torch.randn(256, device=DEV)
        runs = []
        for _ in range(3):
            x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
            y, stats = ops.Conv2dFn.apply(x, w, None, ops._PackCache(), 1, 2, 2, True, None)
            out = ops.BNTrainFn.apply(y, stats, gamma, beta, None, True, None, 0.1)
            out.backward(gy)
            runs.append((out.detach().clone(), x.grad.clone(), w.grad.clone(), ops.known_amax(out).max().clone()))
        for r in runs[1:]:
            for a, b in zip(runs[0], r):
                assert torch.equal(a, b)
    finally:
        ops.CONV_MODE = old


def test_f16x2_scale_equivariance_full_size():
    """Size-independent property at the BASELINE layer size (33 540 pixels, 2048 -> 256 channels, dilated 3x3):
    the per-tensor power-of-two scale makes the evaluation EXACTLY equivariant -- conv(2^a x, 2^b w) is
    bit-for-bit 2^(a+b) conv(x, w), for forward, data gradient and weight gradient."""
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    try:
        g = torch.Generator(device=DEV).manual_seed(5)
        x = torch.randn(4, 65, 129, 2048, device=DEV, generator=g)
        w = torch.randn(256, 2048, 3, 3, device=DEV, generator=g) * 0.01
        gy = torch.randn(4, 65, 129, 256, device=DEV, generator=g)

        def run(xs, ws, gs):
            xd, wd = (x * xs).requires_grad_(True), (w * ws).requires_grad_(True)
            y, _ = ops.Conv2dFn.apply(xd, wd, None, ops._PackCache(), 1, 12, 12, False, None)
            y.backward(gy * gs)
            return y.detach(), xd.grad, wd.grad

        y0, dx0, dw0 = run(1.0, 1.0, 1.0)
        y1, dx1, dw1 = run(2.0 ** 9, 2.0 ** -21, 2.0 ** 5)
        assert torch.equal(y1, y0 * 2.0 ** (9 - 21))
        assert torch.equal(dx1, dx0 * 2.0 ** (5 - 21))
        assert torch.equal(dw1, dw0 * 2.0 ** (5 + 9))
        assert torch.isfinite(y0).all() and y0.abs().max() > 0
    finally:
        ops.CONV_MODE = old


@pytest.mark.parametrize("dev_func", ["hamming", "mean", "median"])
def test_device_switch_reproduces_the_reference_trajectories(golden, dev_func):
    """csrc/switch.hip against the reference's Monitor + model_select (fixture G5, captured from the imported reference
    with the "hamming" trend; the other two trend functions against this repo's host-side Monitor, which G5 pins on the
    CPU): median, exponential average and trend of every one of the 520 steps BIT FOR BIT in float64, the switch state
    identical at every step -- including the 199 steps before the window is full and the two transitions."""
    from onda_amd.framework.domain_adaptation.methods.prototypes_hybrid_switch import model_select
    from onda_amd.framework.utils.monitoring import DeviceSwitch, Monitor
    g = golden("g5_switch")
    seq = g["seq"]
    sw = DeviceSwitch(DEV, 200, 0.003, dev_func, (0.83, 0.9), 0.0002, model_select.static)
    mon, sel = Monitor(200, 0.003, dev_func), model_select(model_select.static, [0.83, 0.9], 0.0002)
    samples = torch.from_numpy(seq).to(DEV)
    got = np.zeros((len(seq), 4))
    cur = np.zeros(len(seq), dtype=np.int64)
    trace_s = torch.zeros(len(seq), 4, dtype=torch.float64, device=DEV)
    trace_i = torch.zeros(len(seq), dtype=torch.int32, device=DEV)
    for i in range(len(seq)):
        sw.step(samples[i])
        trace_s[i] = sw.state[:4]          # (device-side copies: no read-back inside the loop)
        trace_i[i] = sw.istate[2]
        mon.add({"prior static": float(seq[i])})
        a, d = mon.avg("prior static"), mon.dev_avg("prior static")
        sel.evaluate(a, d)
        got[i] = (mon.exp("prior static"), a, d, a)
        cur[i] = sel.current
    dev_s, dev_i = trace_s.cpu().numpy(), trace_i.cpu().numpy()
    assert np.array_equal(dev_s[:, 0], got[:, 0]), "exponential average"
    assert np.array_equal(dev_s[:, 1], got[:, 1]), "median"
    assert np.array_equal(dev_s[:, 2], got[:, 2]), "trend"
    assert np.array_equal(dev_i, cur)
    if dev_func == "hamming":  # ... and the host monitor is the reference's (G5)
        assert np.array_equal(dev_s[:, 1], g["avg"]) and np.array_equal(dev_s[:, 0], g["exp"]) and np.array_equal(dev_s[:, 2], g["dev"])
        assert np.array_equal(dev_i, g["current"]) and len(set(g["current"].tolist())) == 2
    assert sw.read()["steps"] == len(seq) and sw.read()["count"] == 200
    # float32 samples (what a step feeds) take the same path
    sw32 = DeviceSwitch(DEV, 4, 0.1, "mean", (0.3, 0.6), 0.01, 0)
    for v in (0.25, 0.5, 0.75, 1.0, 0.125):
        sw32.step(torch.tensor(v, device=DEV))
    r = sw32.read()
    assert r["avg"] == 0.625 and r["count"] == 4 and r["current"] == 0 and r["dev"] == pytest.approx((0.75 + 1.0 + 0.125) / 3 - (0.5 + 0.75 + 1.0) / 3)


def test_predicated_convolutions_and_select():
    """OndaConv::run_if: a conv launched under a device flag of 0 writes nothing (whole tiles, stream-K pieces and their
    fix-up included), under 1 it is the plain conv; select_prior / gate_scalar pick by the same flag and never read the
    side that was not computed."""
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    try:
        g = torch.Generator().manual_seed(5)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        # 4 x 65 x 129 pixels, 256 -> 256: 264 tiles of 256 x 128 on the stream kernel + a stream-K remainder with its fix-up;
        # 2 x 33 x 65, 256 -> 128: the four-wave 128 x 128 tiles
        for (B, H, W, cout) in ((4, 65, 129, 256), (2, 33, 65, 128)):
            x = torch.randn(B, H, W, 256, generator=g).to(DEV)
            w = (torch.randn(cout, 256, 1, 1, generator=g) * 0.05).to(DEV)
            wp = ops.pack_weight_fwd(w)
            ref, _, _ = ops.conv_forward(x, wp, 1, 1, 1, 0, cout)
            out = torch.full_like(ref, 7.0)
            flag.fill_(0)
            with ops.predicated(flag):
                ops.conv_forward(x, wp, 1, 1, 1, 0, cout, out=out)
            assert ops.PREDICATE is None and bool((out == 7.0).all())
            flag.fill_(1)
            with ops.predicated(flag):
                ops.conv_forward(x, wp, 1, 1, 1, 0, cout, out=out)
            assert torch.equal(out, ref)
        a, b = torch.randn(1000, 19, device=DEV), torch.full((1000, 19), float("nan"), device=DEV)
        flag.fill_(0)
        assert torch.equal(ops.select_prior(flag, a, 1.0, b, 2.0), a) and torch.isnan(ops.gate_scalar(flag, a[0, 0]))
        flag.fill_(1)
        assert torch.equal(ops.select_prior(flag, b, 1.0, a, 2.0), 2.0 * a) and ops.gate_scalar(flag, a[0, 0]).item() == a[0, 0].item()
    finally:
        ops.CONV_MODE = old


def test_upsample_ce_all_ignored_batch_matches_the_reference_gradient():
    """config 2's loss head on a batch whose labels are all 255: the reference's loss_calc(interp(logits), label) is NaN and
    its gradient exact ZEROS (func.py:88-96 -> loss.py:36-44: the gradient of an empty selection scattered back), so the SGD
    step that follows moves on weight decay and momentum only.  The fused head does the same -- value NaN, gradient zeros, not
    NaN -- checked against torch's autograd on the reference's formulation."""
    from onda_amd import ops
    g = torch.Generator().manual_seed(5)
    B, K, h, w, H, W = 2, 19, 9, 17, 33, 65
    logits = torch.randn(B, K, h, w, generator=g) * 2
    labels = torch.full((B, H, W), 255, dtype=torch.long)
    lr = logits.clone().requires_grad_(True)
    up = F.interpolate(lr, size=(H, W), mode="bilinear", align_corners=True)
    mask = labels != 255  # the reference's own selection (loss.py:34-42)
    sel = up.permute(0, 2, 3, 1)[mask.view(B, H, W, 1).repeat(1, 1, 1, K)].view(-1, K)
    ref = F.cross_entropy(sel, labels[mask])
    ref.backward()
    assert torch.isnan(ref) and not lr.grad.any()
    ld = torch.zeros(B, h, w, ops.HEAD_PAD, device=DEV)
    ld[..., :K] = logits.permute(0, 2, 3, 1).to(DEV)
    out = ld[..., :K].permute(0, 3, 1, 2).requires_grad_(True)
    loss = ops.upsample_ce(out, labels.to(DEV))
    loss.backward()
    assert torch.isnan(loss).item()
    assert not out.grad.any()


@pytest.mark.parametrize("K", [19, 22, 32])
def test_upsample_ce_for_every_class_count_the_library_accepts(K):
    """loss_calc(interp(logits), label) fused (onda_upsample_ce_fwd / _bwd) against torch: value and gradient, for the
    19 classes of the network, and for 22 and 32 -- the backward's row pass needs more than the default 64 KB of dynamic LDS from
    22 classes on (round-4 advisor: such a model trained forward and died in backward)."""
    from onda_amd import ops
    g = torch.Generator().manual_seed(K)
    B, h, w, H, W = 2, 17, 33, 65, 129
    logits = torch.randn(B, K, h, w, generator=g) * 2
    labels = torch.randint(0, K, (B, H, W), generator=g)
    labels[0, :5] = 255
    lr = logits.clone().requires_grad_(True)
    up = F.interpolate(lr, size=(H, W), mode="bilinear", align_corners=True)
    ref = F.cross_entropy(up, labels, ignore_index=255)
    ref.backward()
    ld = torch.zeros(B, h, w, ops.HEAD_PAD, device=DEV)
    ld[..., :K] = logits.permute(0, 2, 3, 1).to(DEV)
    out = ld[..., :K].permute(0, 3, 1, 2).requires_grad_(True)  # pixel-major NCHW view, as the model returns its logits
    loss = ops.upsample_ce(out, labels.to(DEV))
    loss.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach()))
    close(out.grad, lr.grad, 2e-4, f"d loss / d logits, K = {K}")
