"""The fp64 conv reference and the comparator of tests/conv_fp64.py, proven on the CPU before the GPU parity tests
(test_conv_fp64_parity.py) lean on them: the reference equals F.conv2d's float64 autograd, and the comparator flags each
fault a kernel could make quietly -- while the reference rounded to fp32 passes."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_fp64 as ref  # noqa: E402


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


REF_CASES = [
    # B, cin, cout, k, stride, dil, pad, H, W, bias
    (2, 8, 6, 1, 1, 1, 0, 9, 17, False),
    (2, 8, 6, 1, 2, 1, 0, 9, 17, False),
    (2, 8, 6, 1, 2, 1, 0, 10, 18, False),
    (2, 5, 7, 3, 1, 2, 2, 9, 17, False),
    (2, 5, 7, 3, 1, 24, 24, 9, 17, True),   # dilation past the image: only the centre tap is live
    (2, 3, 8, 7, 2, 1, 3, 20, 26, False),   # the stem
    (1, 4, 3, 3, 1, 1, 1, 6, 5, True),
]


@pytest.mark.parametrize("case", REF_CASES, ids=lambda c: "x".join(map(str, c)))
def test_reference_matches_float64_conv2d(case):
    B, cin, cout, k, stride, dil, pad, H, W, bias = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(cout, generator=g, dtype=torch.float64, requires_grad=True) if bias else None
    y = F.conv2d(x, w, b, stride, pad, dil)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    yr = ref.conv_fwd(nhwc(x.detach()), w.detach(), stride, dil, pad, b.detach() if bias else None)
    torch.testing.assert_close(yr, nhwc(y.detach()), rtol=1e-12, atol=1e-12)
    dx = ref.conv_dgrad(nhwc(gy), w.detach(), (H, W), stride, dil, pad)
    torch.testing.assert_close(dx, nhwc(x.grad), rtol=1e-12, atol=1e-12)
    dw = ref.conv_wgrad(nhwc(x.detach()), nhwc(gy), k, stride, dil, pad)
    torch.testing.assert_close(dw, w.grad, rtol=1e-12, atol=1e-12)
    if bias:
        torch.testing.assert_close(ref.bias_grad(nhwc(gy)), b.grad, rtol=1e-12, atol=1e-12)
    st = ref.channel_stats(yr)
    torch.testing.assert_close(st[0], y.detach().sum((0, 2, 3)), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(st[1], (y.detach() ** 2).sum((0, 2, 3)), rtol=1e-12, atol=1e-12)
    # the structural zeros the comparator checks exactly are zeros of F.conv2d's own gradients
    Ho, Wo = y.shape[2:]
    unreached = ref.dgrad_unreached((H, W), k, stride, dil, pad, (Ho, Wo))
    assert (x.grad.permute(0, 2, 3, 1)[:, unreached] == 0).all()
    dead = ref.dead_taps((H, W), k, stride, dil, pad)
    assert (w.grad[:, :, dead] == 0).all()
    if stride == 2 and k == 1:
        assert unreached[1::2].all() and unreached[:, 1::2].all() and not unreached[::2, ::2].any()
    if dil == 24:
        assert dead.sum() == 8 and not dead[1, 1]


# ------------------------------------------------------------------------------------------- the comparator's teeth
def _fwd_case(M_rows_hw=(4, 65), cin=128, cout=128, seed=5):
    """A 1 x 1 forward problem as a GEMM: x [B,H,W,cin] (M = B*H*W rows), w [cout, cin, 1, 1], y in fp64."""
    g = torch.Generator().manual_seed(seed)
    B, HW = M_rows_hw
    x = torch.randn(B, 1, HW, cin, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    return x, w, ref.conv_fwd(x, w)


@pytest.mark.parametrize("mode", ["f16x2", "f32"])
def test_fp32_rounding_of_the_reference_passes(mode):
    x, w, y = _fwd_case()
    assert not ref.flagged(y.float(), y, mode)
    t, b, _ = ref.measure(y.float(), y)
    assert t < 1e-7 and b < 1e-7, (t, b)


@pytest.mark.parametrize("mode", ["f16x2", "f32"])
def test_a_dropped_k_step_in_one_block_is_flagged(mode):
    x, w, y = _fwd_case()
    got = y.clone()
    rows, cols, ks = slice(64, 128), slice(64, 128), slice(32, 64)  # one 64 x 64 block, one 32-channel K-step
    xf = x.double().reshape(-1, x.shape[-1])
    got.view(-1, got.shape[-1])[rows, cols] -= xf[rows, ks] @ w[cols, ks, 0, 0].double().t()
    assert ref.flagged(got.float(), y, mode)
    assert ref.measure(got, y)[2] == (1, 0, 1)


def _lo_hi_product(x, w, rows, cols):
    """x_lo . w_hi of the given GEMM rows / output channels, with the library's limb split."""
    xf = x.double().reshape(-1, x.shape[-1])
    _, x_lo = ref.limb_split(xf)
    w_hi, _ = ref.limb_split(w[:, :, 0, 0].double())
    return x_lo[rows] @ w_hi[cols].t()


@pytest.mark.parametrize("mode", ["f16x2", "f32"])
def test_a_missing_limb_product_in_one_block_is_flagged(mode):
    x, w, y = _fwd_case()
    hi, lo = ref.limb_split(x)
    assert (hi + lo - x.double()).abs().max() <= 2.0 ** -21 * x.abs().max()  # two f16 limbs: 22 of fp32's 24 bits
    got = y.clone().reshape(-1, y.shape[-1])
    got[128:192, 0:64] -= _lo_hi_product(x, w, slice(128, 192), slice(0, 64))
    t, b, where = ref.measure(got, y.reshape(-1, y.shape[-1]))
    assert where == (2, 0, 0) and b > 1e-4, (t, b, where)  # ~5e-4 for a full-range operand
    assert ref.flagged(got.float(), y.reshape(-1, y.shape[-1]), mode)


@pytest.mark.parametrize("mode", ["f16x2", "f32"])
@pytest.mark.parametrize("fault", ["zeroed", "limb"])
def test_the_last_partial_tile_rows_are_held(mode, fault):
    """M = 260 = 4 * 65: the last 4 GEMM rows form a partial block of their own."""
    x, w, y = _fwd_case()
    yf = y.reshape(-1, y.shape[-1])
    assert yf.shape[0] == 260
    got = yf.clone()
    if fault == "zeroed":
        got[256:] = 0
    else:
        got[256:] -= _lo_hi_product(x, w, slice(256, 260), slice(0, 128))
    assert ref.flagged(got.float(), yf, mode)
    assert ref.measure(got, yf)[2][0] == 4


@pytest.mark.parametrize("mode", ["f16x2", "f32"])
def test_one_missing_split_k_slab_of_248_is_flagged(mode):
    g = torch.Generator().manual_seed(7)
    M, cin, cout = 248 * 32, 64, 64
    x = torch.randn(1, 1, M, cin, generator=g)
    dy = torch.randn(1, 1, M, cout, generator=g)
    dw = ref.conv_wgrad(x, dy, 1)
    piece = slice(100 * 32, 101 * 32)  # slab 100 of 248
    got = dw.clone()
    got[:, :, 0, 0] -= dy[0, 0, piece].double().t() @ x[0, 0, piece].double()
    assert ref.flagged(got.float(), dw, mode, kind="wgrad")


@pytest.mark.parametrize("mode", ["f16x2", "f32"])
def test_a_skipped_live_border_tap_is_flagged(mode):
    """A dead-tap skip that wrongly drops tap (0, 0) of a 3 x 3 pad-1 conv for the tile of the first 64 rows."""
    g = torch.Generator().manual_seed(9)
    B, H, W, cin, cout = 2, 9, 17, 64, 64
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    y = ref.conv_fwd(x, w, 1, 1, 1)
    w0 = torch.zeros_like(w)
    w0[:, :, 0, 0] = w[:, :, 0, 0]
    tap = ref.conv_fwd(x, w0, 1, 1, 1).reshape(-1, cout)
    got = y.clone().reshape(-1, cout)
    got[:64] -= tap[:64]
    assert tap[:64].abs().max() > 0  # the tap is live in that tile (row 0 of the image sits in padding for it, row 1 does not)
    assert ref.flagged(got.float(), y.reshape(-1, cout), mode)


@pytest.mark.parametrize("mode", ["f16x2", "f32"])
def test_a_structural_zero_set_to_1e_30_is_flagged(mode):
    g = torch.Generator().manual_seed(3)
    B, H, W, cin, cout = 2, 10, 18, 64, 64
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    dy = torch.randn(B, 5, 9, cout, generator=g)
    dx = ref.conv_dgrad(dy, w, (H, W), 2)
    unreached = ref.dgrad_unreached((H, W), 1, 2, 1, 0, (5, 9))
    exact = [(0.0, unreached[None, :, :, None])]
    good = dx.float()
    assert not ref.flagged(good, dx, mode, exact=exact)
    bad = good.clone()
    bad[1, 3, 5, 17] = 1e-30  # an odd row and column: no tap of the 1 x 1 stride-2 conv reaches it
    assert unreached[3, 5]
    assert ref.measure(bad, dx)[0] < 1e-7  # invisible to the L2 measures ...
    assert ref.flagged(bad, dx, mode, exact=exact)  # ... not to the exact check


def test_the_comparator_is_the_same_over_row_chunks(monkeypatch):
    """The comparator works through a tensor in row chunks: chunk edges, the partial last block and the tensor figure equal a
    one-piece computation."""
    g = torch.Generator().manual_seed(4)
    r = torch.randn(1000, 96, generator=g, dtype=torch.float64)
    got = (r + 1e-6 * torch.randn(r.shape, generator=g, dtype=torch.float64)).float()
    got[999, 95] += 1e-3  # the partial last block, partial last channel block
    whole = ref.measure(got, r)
    monkeypatch.setattr(ref, "CHUNK_ROWS", 128)
    chunked = ref.measure(got, r)
    assert chunked[2] == whole[2] == (15, 0, 1)
    assert abs(chunked[0] - whole[0]) <= 1e-12 * whole[0] and abs(chunked[1] - whole[1]) <= 1e-12 * whole[1]
    assert abs(whole[0] - ((got.double() - r).norm() / r.norm()).item()) <= 1e-12
    st = ref.channel_stats(r, with_abs=True)
    assert torch.allclose(st, torch.stack([r.sum(0), (r * r).sum(0), r.abs().sum(0)]), rtol=1e-12, atol=1e-12)
