"""GPU, "f16x2" mode: every fused producer of limb rows writes the BITS of the one definition of the format (csrc/limbs.h).

Each case holds two sets of limb rows against each other: the rows a fused producer wrote, and the rows onda_split_h2 writes for
the same fp32 values with the SAME amax slot (the slot defines the power-of-two scale, so it has to be shared: a fused producer
scales by a bound -- max|source| -- not by the maximum of what it writes).  The scaling is exact and both sides round through
the same two conversions, so the bar is equality of the raw f16 words, not a tolerance: a producer that derived the scale, the
rounding, the factor of the second limb or the place of a limb differently would differ in some word.

Inputs keep to magnitudes of 1e-2 .. 1e2 (nothing the scaling pushes into f16 subnormals in the first limb).  BatchNorm apply and
the conv limb epilogue are not here: their fp32 twins are other kernels whose arithmetic may contract differently; their
tolerance tests hold them (test_hip_kernels.py, test_conv_fp64_parity.py, test_norm_fp64_parity.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def f16x2_mode():
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    yield
    ops.CONV_MODE = old


def values(*shape, seed):
    """sign * 10^u, u uniform in [-2, 2)"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(10.0, torch.rand(*shape, generator=g) * 4.0 - 2.0)
    sign = torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).to(DEV)


def absmax_slot(x, rows, C, ld):
    """A fresh amax slot with max|x| of x[rows][ld] (C valid channels; rows == 1: a flat tensor of C floats)."""
    from onda_amd import ops
    from onda_amd._lib import call
    slot = ops.amax_slot(torch.device(DEV))
    call("onda_absmax", x.data_ptr(), rows, C, ld, ops._p(slot), ops._stream())
    return slot


def split(x, rows, C, ldx, slot):
    """onda_split_h2 of x[rows][ldx] (C valid channels) with the scale of `slot`: limb rows [rows][C / 32][2][32] f16."""
    from onda_amd import ops
    from onda_amd._lib import call
    dst = torch.full((rows, 2 * C), float("nan"), device=DEV, dtype=torch.float16)
    call("onda_split_h2", x.data_ptr(), rows, C, ldx, ops._p(dst), C, rows * C, ops._p(slot), ops._stream())
    return dst


def new_rows(rows, C):
    return torch.full((rows, 2 * C), float("nan"), device=DEV, dtype=torch.float16)


def same_bits(fused, ref, what):
    torch.cuda.synchronize()
    a, b = fused.reshape(-1).view(torch.int16), ref.reshape(-1).view(torch.int16)
    assert a.numel() == b.numel(), what
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} f16 words differ"
    assert not torch.isnan(ref).any(), f"{what}: words left unwritten"


def test_stem_patches_write_the_split_of_the_patch_matrix():
    """Ragged 19 x 23 image: border taps out of range, K padded from 147 to 160."""
    from onda_amd import ops
    x = values(2, 3, 19, 23, seed=1)
    Ho, Wo = ops.conv_out_size(19, 7, 2, 1, 3), ops.conv_out_size(23, 7, 2, 1, 3)
    col = ops.stem_patches(x, Ho, Wo, True)
    lb = ops.limbs_of(col)
    ref = ops.stem_patches(x, Ho, Wo, False)
    assert ref.shape == (2, Ho, Wo, 160) and lb.ld == 160
    rows = 2 * Ho * Wo
    same_bits(lb.planes, split(ref, rows, 160, 160, lb.amax), "stem patches")


def test_maxpool_limb_rows_are_the_split_of_the_fp32_pool():
    """9 x 11 post-ReLU input: ceil-mode windows clipped on both edges; 64 channels = two 32-channel blocks."""
    from onda_amd import ops
    B, Hi, Wi, C = 2, 9, 11, 64
    x = values(B, Hi, Wi, C, seed=2).clamp_min(0.0).contiguous()
    slot = absmax_slot(x, B * Hi * Wi, C, C)
    ops.tag_amax(x, slot)
    yl = ops.MaxPoolFn.apply(x, True)
    assert ops.is_limb_only(yl)
    y = ops.MaxPoolFn.apply(x)  # fp32; carries the same slot
    assert ops.known_amax(y) is slot and ops.limbs_of(yl).amax is slot
    _, Ho, Wo, _ = y.shape
    assert (Ho, Wo) == (5, 6)
    same_bits(ops.limbs_of(yl).planes, split(y, B * Ho * Wo, C, C, slot), "max-pool")


def test_se_gate_limb_rows_are_the_split_of_the_fp32_gate():
    from onda_amd import ops
    from onda_amd._lib import call
    B, H, W, C = 2, 3, 5, 64
    x = values(B, H, W, C, seed=3)
    gate = torch.sigmoid(torch.randn(B, C, generator=torch.Generator().manual_seed(4))).to(DEV)
    slot = absmax_slot(x, B * H * W, C, C)
    fused = new_rows(B * H * W, C)
    call("onda_chan_scale_limbs", ops._p(x), ops._p(gate), ops._p(fused), B * H * W * C, ops._p(slot), B, H * W, C, ops._stream())
    out = torch.empty_like(x)
    call("onda_chan_scale", ops._p(x), ops._p(gate), None, ops._p(out), B, H * W, C, ops._stream())
    same_bits(fused, split(out, B * H * W, C, C, slot), "SE gate")


def s2d_reference(x_nchw, slope):
    """LeakyReLU -> one-pixel zero border -> space-to-depth, fp32 [B, Hs, Ws, Cp] (zeros above 4C), in torch."""
    B, C, H, W = x_nchw.shape
    Hs, Ws, Cp = H // 2 + 1, W // 2 + 1, -(-4 * C // 32) * 32
    a = torch.where(x_nchw > 0, x_nchw, x_nchw * torch.tensor(slope, dtype=torch.float32, device=x_nchw.device))
    xp = torch.zeros(B, C, 2 * Hs, 2 * Ws, device=x_nchw.device)
    xp[:, :, 1:H + 1, 1:W + 1] = a  # (odd H or W: the far border row / column would be row 2 * Hs / column 2 * Ws, which nothing reads)
    S = torch.zeros(B, Hs, Ws, Cp, device=x_nchw.device)
    # S[b, i, j, (py*2 + px)*C + c] = xp[b, c, 2i + py, 2j + px]
    S[..., :4 * C] = xp.reshape(B, C, Hs, 2, Ws, 2).permute(0, 2, 4, 3, 5, 1).reshape(B, Hs, Ws, 4 * C)
    return S.contiguous()


@pytest.mark.parametrize("H,W", [(11, 13), (10, 14)])
def test_disc_split_from_an_nchw_map_is_the_split_of_the_rearrangement(H, W):
    """19 channels (4C = 76 padded to 96); odd H: the padded image has a row pair that holds the bottom border only."""
    from onda_amd import ops
    from onda_amd._lib import call
    B, C, slope = 2, 19, 0.2
    x = values(B, C, H, W, seed=5 + H)
    slot = absmax_slot(x, 1, x.numel(), x.numel())
    S = s2d_reference(x, slope)
    _, Hs, Ws, Cp = S.shape
    assert Cp == 96
    fused = new_rows(B * Hs * Ws, Cp)
    call("onda_s2d_split_h2", ops._p(x), 1, B, C, H, W, 0, slope, ops._p(slot), ops._p(fused), ops._stream())
    same_bits(fused, split(S, B * Hs * Ws, Cp, Cp, slot), f"s2d split, NCHW {H} x {W}")


def test_disc_split_from_an_nhwc_conv_output_is_the_split_of_the_rearrangement():
    from onda_amd import ops
    from onda_amd._lib import call
    B, H, W, C, slope = 2, 7, 9, 64, 0.2
    x = values(B, H, W, C, seed=6)
    slot = absmax_slot(x, B * H * W, C, C)
    S = s2d_reference(x.permute(0, 3, 1, 2), slope)
    _, Hs, Ws, Cp = S.shape
    assert Cp == 256
    fused = new_rows(B * Hs * Ws, Cp)
    call("onda_s2d_split_h2", ops._p(x), 0, B, C, H, W, C, slope, ops._p(slot), ops._p(fused), ops._stream())
    same_bits(fused, split(S, B * Hs * Ws, Cp, Cp, slot), "s2d split, NHWC")


def test_split_h2_of_a_channel_slice_is_the_split_of_its_copy():
    """ldx 96, C 64: the row stride of the source is not its channel count."""
    rows, C, ld = 37, 64, 96
    buf = values(rows, ld, seed=7)
    view = buf[:, 32:]  # 128 bytes in: still 16-byte aligned
    slot = absmax_slot(view, rows, C, ld)
    same_bits(split(view, rows, C, ld, slot), split(view.contiguous(), rows, C, C, slot), "split_h2 of a slice")
