"""The fp64 reference of the eval-mode conv epilogue that writes limb planes (tests/conv_fp64.py eval_conv_ref) and the
comparator's `scale_ref`, proven on the CPU before tests/test_eval_conv_fp64_parity.py leans on them:

  (a) an emulation of the epilogue in torch -- fp32 conv -> folded scale / shift -> residual joined from limb planes that
      carry a loose bound -> ReLU -> split into limbs at an a-priori bound -> rejoined -- stays inside BOUNDS["f16x2"] relative
      to `mag`, with the bound 2^8 and 2^13 above the true maximum, and the output's representation alone (the fp64 reference
      rounded to limbs at that scale) uses less than a quarter of each bound: the reference and the format leave the kernel
      three quarters of the condition;
  (b) each fault the epilogue could make quietly, confined to one tile / block / tile row, is flagged;
  (c) ops.fold_bounds and the bound formula restated in fp64, which the GPU leg holds the library's scalars to."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_fp64 as ref  # noqa: E402

MODE = "f16x2"
B, H, W, CIN, COUT, K, DIL = 2, 17, 33, 64, 256, 3, 2  # M = 1122: four 256-row tile rows and a partial one of 98; two column tiles
RES_LOOSE = 2.0 ** 9  # the residual's planes carry a bound this far above its true maximum


class _Case:
    pass


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(11)
    c = _Case()
    x = torch.randn(B, H, W, CIN, generator=g)
    c.x = sum(ref.limb_split(x))  # the operand as the conv reads it: two limbs at the true scale
    c.w = torch.randn(COUT, CIN, K, K, generator=g) / (CIN * K * K) ** 0.5
    sign = torch.where(torch.rand(COUT, generator=g) < 0.25, -1.0, 1.0)
    c.sc = (torch.rand(COUT, generator=g) + 0.5) * sign
    c.sh = torch.randn(COUT, generator=g)
    r = torch.randn(B, H, W, COUT, generator=g)
    c.res_true = r.abs().max().item()
    c.res = sum(ref.limb_split(r, amax=RES_LOOSE * c.res_true))  # what the planes under the loose bound hold
    c.conv32 = F.conv2d(c.x.float().permute(0, 3, 1, 2), c.w, None, 1, DIL, DIL).permute(0, 2, 3, 1).contiguous()
    c.y, c.mag = ref.eval_conv_ref(c.x, c.w, c.sc, c.sh, c.res, True, 1, DIL, DIL)
    c.true_max = c.y.abs().max().item()
    return c


def _emulate(c, bound, sc=None, sh=None, res=True, res_factor=1.0, relu=True, second_limb=True):
    """The epilogue in fp32 torch; the keyword arguments are the faults of (b)."""
    v = c.conv32 * (c.sc if sc is None else sc) + (c.sh if sh is None else sh)
    if res:
        v = v + c.res.float() * res_factor
    if relu:
        v = torch.relu(v)
    hi, lo = ref.limb_split(v, amax=bound)
    return (hi + lo if second_limb else hi).reshape(-1, COUT)


def _flagged(got, c):
    return ref.flagged(got.reshape(c.y.shape), c.y, MODE, scale_ref=c.mag)


@pytest.mark.parametrize("loose", [8, 13])
def test_the_emulated_epilogue_stays_inside_the_bounds(case, loose):
    c = case
    bound = c.true_max * 2.0 ** loose
    got = _emulate(c, bound).reshape(c.y.shape)
    t, b = ref.check(got, c.y, MODE, f"emulation, bound 2^{loose} above the maximum", scale_ref=c.mag)
    # the output's representation alone: the reference itself rounded to two limbs at the bound's scale
    rt, rb, _ = ref.measure(sum(ref.limb_split(c.y, amax=bound)), c.y, scale_ref=c.mag)
    print(f"bound 2^{loose}: emulation rel {t:.2e} block {b:.2e}; representation floor rel {rt:.2e} block {rb:.2e}")
    assert rt <= ref.BOUNDS[MODE][0] / 4 and rb <= ref.BOUNDS[MODE][1] / 4, (rt, rb)
    # limbs.h: the element error of the two limbs is at most 2^-22 of the element, down to 2^-28 of the scale
    live = c.y > 2.0 ** -24 * bound
    err = ((sum(ref.limb_split(c.y, amax=bound)) - c.y).abs() / c.y.abs().clamp_min(1e-300))[live].max().item()
    assert err <= 2.0 ** -22, err


TILE = (slice(256, 512), slice(128, 256))  # one 256 x 128 tile


def _paste(c, region, **fault):
    bound = c.true_max * 2.0 ** 8
    got = _emulate(c, bound)
    bad = _emulate(c, bound, **fault)
    assert not torch.equal(got[region], bad[region])
    got[region] = bad[region]
    return got


def test_the_clean_emulation_is_not_flagged(case):
    assert not _flagged(_emulate(case, case.true_max * 2.0 ** 8), case)


def test_a_residual_left_out_in_one_tile_is_flagged(case):
    assert _flagged(_paste(case, TILE, res=False), case)


def test_a_residual_joined_with_the_scale_of_its_true_maximum_is_flagged(case):
    """The planes carry a bound 2^9 above the residual's maximum; a join by the true maximum's scale is off by that factor."""
    assert _flagged(_paste(case, TILE, res_factor=1.0 / RES_LOOSE), case)


def test_a_zeroed_second_output_limb_in_one_block_is_flagged(case):
    got = _paste(case, (slice(64, 128), slice(64, 128)), second_limb=False)
    assert _flagged(got, case)
    assert ref.measure(got.reshape(case.y.shape), case.y, scale_ref=case.mag)[2] == (1, 0, 1)


def test_a_stale_last_partial_tile_row_is_flagged(case):
    got = _emulate(case, case.true_max * 2.0 ** 8)
    assert got.shape[0] == 1122
    got[1024:] = 0
    assert _flagged(got, case)


def test_scale_and_shift_of_channel_n_plus_4_in_one_column_tile_are_flagged(case):
    c = case
    assert _flagged(_paste(c, (slice(None), slice(128, 256)), sc=c.sc.roll(-4), sh=c.sh.roll(-4)), c)


def test_a_skipped_relu_in_one_tile_is_flagged(case):
    assert _flagged(_paste(case, TILE, relu=False), case)


def test_scale_ref_replaces_the_denominators_and_nothing_else(monkeypatch):
    g = torch.Generator().manual_seed(8)
    r = torch.randn(300, 96, generator=g, dtype=torch.float64)
    got = (r + 1e-6 * torch.randn(r.shape, generator=g, dtype=torch.float64)).float()
    s = r.abs() + 1.0
    t, b, where = ref.measure(got, r, scale_ref=s)
    d = got.double() - r
    assert abs(t - (d.norm() / s.norm()).item()) <= 1e-12 * t
    blocks = [(i, j) for i in range(5) for j in range(2)]
    by_hand = {(i, j): (d[64 * i:64 * i + 64, 64 * j:64 * j + 64].norm() / s[64 * i:64 * i + 64, 64 * j:64 * j + 64].norm()).item()
               for i, j in blocks}
    worst = max(by_hand, key=by_hand.get)
    assert where == (worst[0], 0, worst[1]) and abs(b - by_hand[worst]) <= 1e-12 * b
    monkeypatch.setattr(ref, "CHUNK_ROWS", 128)  # (chunk edges and the partial last block)
    t2, b2, where2 = ref.measure(got, r, scale_ref=s)
    assert where2 == where and abs(t2 - t) <= 1e-12 * t and abs(b2 - b) <= 1e-12 * b
    assert ref.measure(got, r) == ref.measure(got, r, scale_ref=r)  # None: the reference itself, as before


# ------------------------------------------------------------------------------------------------ restatements
def test_fold_bounds_restated_in_fp64(case):
    from onda_amd import ops
    c = case
    kb = ops.fold_bounds(c.w, c.sc, c.sh)
    want = ref.fold_bounds_ref(c.w, c.sc, c.sh)
    assert kb.dtype == torch.float32 and kb.shape == (2,)
    assert kb[0].item() == pytest.approx(want[0], rel=1e-6) and kb[1].item() == pytest.approx(want[1], rel=1e-6)
    # from the definition, channel by channel
    rows = [abs(c.sc[n].item()) * c.w[n].double().abs().sum().item() for n in range(COUT)]
    assert want[0] == pytest.approx(max(rows), rel=1e-12) and want[1] == c.sh.abs().max().item()
    # it bounds: |conv * scale| <= max|x| * kb0, |y| <= bound
    assert (c.mag - c.sh.double().abs() - c.res.abs()).max().item() <= c.x.abs().max().item() * want[0]
    assert c.true_max <= ref.limb_out_bound_ref(c.x.abs().max().item(), want, c.res_true)


def test_the_bound_formula_restated_in_fp64():
    assert ref.limb_out_bound_ref(2.0, (3.0, 1.0), 0.5) == 7.5 * 1.0001
    assert ref.limb_out_bound_ref(2.0, (3.0, 1.0)) == 7.0 * 1.0001
    g = torch.Generator().manual_seed(3)
    for _ in range(64):  # the epilogue's own fp32 evaluation (three roundings) stays within 1e-6 of it
        xt, k0, k1, rt = (torch.rand(4, generator=g) * 10.0 ** torch.randint(-3, 4, (4,), generator=g).float()).unbind()
        b = ((xt * k0 + k1) + rt) * torch.tensor(1.0001)
        assert b.item() == pytest.approx(ref.limb_out_bound_ref(xt.item(), (k0.item(), k1.item()), rt.item()), rel=1e-6)
