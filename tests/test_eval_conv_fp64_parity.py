"""The eval-mode conv epilogue that writes limb planes (onda_conv2d_fwd_l2_limbs: conv + folded BatchNorm [+ residual read as
limb planes] [+ ReLU], scaled by an a-priori bound) held to fp64 per 64 x 64 block -- what tests/test_conv_fp64_parity.py does for
the train-mode launches.  Every no-grad pass of the adaptation step (static and dynamic model, evaluation, pseudo-labels) runs its
backbone through this entry point; its code sits in three places of csrc/conv_l2.hip (l2_epilogue_limbs of the tile kernels, of
the continuous-stream kernel, and a copy inside conv_l2_fixup_kernel), and each case here confirms through the library's dispatch
queries which of them it runs before it is held to the reference.

The reference (tests/conv_fp64.py eval_conv_ref) is fed with the operands the kernel received -- the materialized limb planes of
the input and of the residual -- and the fp32 weight, scale and shift; the error scale is `mag`, the size of the terms of the
sum, because the result cancels and is then clipped (tests/test_eval_conv_fp64_reference.py proves the reference, the format's
own share of the bounds and the comparator's teeth on the CPU).  The residual is always limb-only planes under a loose bound,
produced by a preceding limb-writing 1 x 1 conv, as a block's input is in the model."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_fp64 as ref  # noqa: E402
from conv_fp64 import _G, _edge_geometries, _schedule  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODE = "f16x2"
LOOSEST = 2.0 ** 13  # how far above the true maximum a bound may sit (limbs.h: full accuracy down to 2^-24 of the scale)


@pytest.fixture(autouse=True)
def _f16x2():
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, MODE
    yield
    ops.CONV_MODE = old
    torch.cuda.empty_cache()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, device=DEV, generator=g) * scale


def _affine(cout, g):
    """scale in [0.5, 1.5) with a random sign on a quarter of the channels, shift ~ N(0, 1)."""
    sign = torch.where(torch.rand(cout, device=DEV, generator=g) < 0.25, -1.0, 1.0)
    return (torch.rand(cout, device=DEV, generator=g) + 0.5) * sign, _randn((cout,), g)


def _operand(t):
    """float64 copy of an activation AS A CONV READS IT: its limb planes, materialized."""
    from onda_amd import ops
    if ops.is_limb_only(t):
        return ops.materialize(t).double()
    return ops.materialize(ops.limb_only(tuple(t.shape), t.device, ops.activation_limbs(t))).double()


def _scalar(slots):
    return slots.max().item()


def _limb_conv(x, w, sc, sh, k, stride, dil, pad, residual=None, relu=False):
    from onda_amd import ops
    y, _, _ = ops.conv_forward(x, ops.pack_weight_fwd(w), k, stride, dil, pad, w.shape[0], scale=sc, shift=sh, residual=residual,
                               relu=relu, limb_out=ops.fold_bounds(w, sc, sh))
    assert ops.is_limb_only(y)
    return y


def loose_planes(shape, g, cin=64):
    """A limb-only activation whose planes carry a bound, not their true maximum: the output of a limb-writing 1 x 1 conv
    (no ReLU: both signs), as a block's input is in the model."""
    from onda_amd import ops
    B, H, W, C = shape
    src = _randn((B, H, W, cin), g)
    ops.activation_limbs(src)
    sc, sh = _affine(C, g)
    t = _limb_conv(src, _randn((C, cin, 1, 1), g, 1.0 / math.sqrt(cin)), sc, sh, 1, 1, 1, 0)
    lb = ops.limbs_of(t)
    assert _scalar(lb.amax) > 2.0 * _scalar(lb.true_amax) > 0  # (the construction: a scale that is not the true maximum's)
    return t


def expected_plan(M, cout, taps, cin):
    """(kernel id, balanced) of an (M, Cout, K) problem, restated from the rules of l2_plan (csrc/conv_l2.hip) over the
    resident-workgroup count the library reports: what a case asserts the dispatch queries against."""
    KT = taps * (cin // 32)
    variant = 2 if cout <= 64 else (0 if -(-M // 256) * -(-cout // 128) >= 200 else 1)
    if variant == 0 and (KT <= 8 or (KT <= 16 and cout >= 512) or (KT <= 32 and cout >= 2048)):
        variant = 1  # short K loops: 128 x 128 tiles, two workgroups per CU
    BM, BN = (128 if variant == 1 else 256), (64 if variant == 2 else 128)
    G = _G() // 2 if variant == 0 else _G()
    tiles = -(-M // BM) * -(-cout // BN)
    rem = tiles % G
    t_tile_us = 2.0 * BM * BN * taps * cin / 1.4e6
    fix_us = 6.0 + (G + 2.0 * rem) * (BM * BN / 16384.0) * 0.02
    balanced = rem != 0 and KT >= 4 and t_tile_us * (1.0 - rem / G) > fix_us
    return (3 if variant == 0 and KT <= 32 else variant), balanced


PLAN = "plan"


def confirm_plan(label, M, cout, taps, cin, kid=PLAN, balanced=PLAN, rem=None):
    """Assert kernel and schedule through the dispatch queries (the limb entry point follows the same plan: l2_plan only
    diverts it from the stationary kernel, which is off) and print them.  kid / balanced: what the case names; PLAN = what
    expected_plan says; balanced None = left open (the stream kernel's remainder row of the edge table)."""
    want_kid, want_bal = expected_plan(M, cout, taps, cin)
    kid_got, bal_got, rem_got, G = _schedule(M, cout, taps, cin)
    assert kid_got == want_kid and (kid == PLAN or kid_got == kid), (label, kid_got, want_kid)
    if balanced is not None:
        assert bal_got == (want_bal if balanced == PLAN else balanced), (label, bal_got)
    if rem is not None:
        assert rem_got == rem, (label, rem_got, G)
    print(f"plan: {label}: G={G} kernel {kid_got} balanced {bal_got} remainder {rem_got}")
    return kid_got, bal_got


def run_eval_geometry(name, B, Hi, Wi, Cin, Cout, k, stride, dil, pad, res, relu, seed=1, x=None, x_scale=None, shift_zero=False,
                      shared=None):
    """One launch through ops.conv_forward(..., limb_out=ops.fold_bounds(...)) held to fp64.  x: the input (default: random,
    dense, read through ops.activation_limbs; x_scale multiplies it elementwise first); res: False, True (limb-only planes
    under a loose bound, made here) or the limb-only residual itself.  shared: a dict that carries the operands and the fp64
    convolution from one epilogue of a geometry to the next (same seed).  Returns a dict: y (limb-only), its Limbs, the
    reference and the figures.  A failure is re-raised with its message only (a traceback would keep the device tensors alive)."""
    try:
        return _run_eval_geometry(name, B, Hi, Wi, Cin, Cout, k, stride, dil, pad, res, relu, seed, x, x_scale, shift_zero,
                                  shared if shared is not None else {})
    except AssertionError as e:
        msg = str(e)
    raise AssertionError(msg)


def _run_eval_geometry(name, B, Hi, Wi, Cin, Cout, k, stride, dil, pad, res, relu, seed, x, x_scale, shift_zero, shared):
    from onda_amd import ops
    Ho, Wo = ref.out_size(Hi, k, stride, dil, pad), ref.out_size(Wi, k, stride, dil, pad)
    M = B * Ho * Wo
    if "w" not in shared:
        g = _gen(seed)
        if x is None:
            x = _randn((B, Hi, Wi, Cin), g)
            if x_scale is not None:
                x = x * x_scale
            ops.activation_limbs(x)
        assert tuple(x.shape) == (B, Hi, Wi, Cin)
        shared["x"], shared["w"] = x, _randn((Cout, Cin, k, k), g, 1.0 / math.sqrt(Cin * k * k))
        shared["sc"], shared["sh"] = _affine(Cout, g)
        shared["x64"] = _operand(x)
        shared["conv"] = ref.conv_fwd(shared["x64"], shared["w"], stride, dil, pad)
    x, w, sc, sh, x64, conv = (shared[n] for n in ("x", "w", "sc", "sh", "x64", "conv"))
    if shift_zero:
        sh = torch.zeros_like(sh)
    if res is True:
        if "res" not in shared:
            shared["res"] = loose_planes((B, Ho, Wo, Cout), _gen(seed + 1000))
        res = shared["res"]
    residual = res if res is not False else None
    kid, bal = _schedule(M, Cout, k * k, Cin)[:2]

    y = _limb_conv(x, w, sc, sh, k, stride, dil, pad, residual, relu)
    lb, xl = ops.limbs_of(y), ops.limbs_of(x)
    got = ops.materialize(y)
    assert tuple(got.shape) == (B, Ho, Wo, Cout)

    # the reference, from the operands the kernel received (pre: before the ReLU)
    res64 = _operand(residual) if residual is not None else None
    pre, mag = ref.eval_conv_ref(x64, w, sc, sh, res64, False, stride, dil, pad, conv=conv)
    y_ref = pre.clamp_min(0) if relu else pre
    what = f"{name} {'+res' if residual is not None else ''}{'+relu' if relu else ''}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    if float(mag.max()) > 0:
        t, b = ref.check(got, y_ref, MODE, what, scale_ref=mag)
    else:  # (all terms zero: the result is exact by structure)
        assert ref.exact_violations(got, 0.0) == 0, f"{what}: not zero"
        t = b = 0.0
    if relu:
        n = ref.exact_violations(got, 0.0, pre < -1e-4 * mag)
        assert n == 0, f"{what}: {n} elements the ReLU clips are not exactly 0"

    # the scalars that travel with the planes
    kb = ref.fold_bounds_ref(w, sc, sh)
    res_true = _scalar(ops.limbs_of(residual).true_amax) if residual is not None else None
    bound_ref = ref.limb_out_bound_ref(_scalar(xl.true_amax), kb, res_true)
    bound, true = _scalar(lb.amax), _scalar(lb.true_amax)
    assert abs(bound - bound_ref) <= 1e-6 * bound_ref, f"{what}: bound {bound!r}, formula {bound_ref!r}"
    assert float(y_ref.abs().max()) <= bound, f"{what}: max|y| {float(y_ref.abs().max())!r} above the bound {bound!r}"
    gmax = float(got.abs().max())
    assert abs(true - gmax) <= 2.0 ** -21 * true, f"{what}: recorded maximum {true!r}, of the planes {gmax!r}"
    assert bound <= LOOSEST * true, f"{what}: bound {bound!r} more than 2^13 above the true maximum {true!r}"
    loose = math.log2(bound / true) if true > 0 else 0.0
    print(f"[eval] {name} B={B} {Hi}x{Wi} {Cin}->{Cout} k{k} s{stride} d{dil}{' +res' if residual is not None else ''}"
          f"{' +relu' if relu else ''}: {ops.core._L2_KERNELS[kid]}{' stream-K + fixup' if bal else ''}  rel {t:.2e} block {b:.2e}"
          f"  bound 2^{loose:.1f} above the maximum")
    return {"y": y, "limbs": lb, "got": got, "y_ref": y_ref, "mag": mag, "rel": t, "block": b, "bound": bound, "true": true}


# ---------------------------------------------------------------------------------------------------- 1. every path
EPILOGUES = [("affine+relu", False, True), ("affine+res+relu", True, True), ("affine", False, False)]


@pytest.mark.parametrize("i", range(7))
def test_every_kernel_path_writes_limb_planes_against_fp64(i):
    """The seven schedule edges (256 x 128 tiles with whole rounds, remainder + fixup, long K; 128 x 128 and 256 x 64
    balanced; the continuous stream with whole rounds and with a remainder), three epilogues each.  The balanced rows put
    the fixup kernel's own limb output under test."""
    label, geo, kid, balanced, rem = _edge_geometries()[i]
    name, H, W, cin, cout, k, stride, dil, pad = geo[:9]
    confirm_plan(label, H * W, cout, k * k, cin, kid, balanced, rem)
    shared = {}
    for _ename, res, relu in EPILOGUES:
        run_eval_geometry(name, 1, H, W, cin, cout, k, stride, dil, pad, res, relu, seed=200 + i, shared=shared)


# ---------------------------------------------------------------------------- 2. the model's geometries, small
def _sites():
    """(name, Cin, Cout, k, stride, dil, pad, residual, relu) of every backbone site of the eval-mode forward: the layer1..4
    rows of test_conv_fp64_parity.STEP_CONVS, each with its own epilogue -- conv3: residual + ReLU, downsample: neither, the
    others: ReLU (layer1's conv3 and downsample share a geometry and differ in the epilogue)."""
    from test_conv_fp64_parity import STEP_CONVS
    out = []
    for name, _Hi, _Wi, cin, cout, k, stride, dil, pad, *_ in STEP_CONVS:
        if not name.startswith("layer"):
            continue
        kinds = {"layer1.conv3+ds": ["conv3", "ds"]}.get(name, [name.rsplit(".", 1)[1]])
        for kind in kinds:
            res, relu = {"conv3": (True, True), "ds": (False, False)}.get(kind, (False, True))
            out.append((name.replace("conv3+ds", kind), cin, cout, k, stride, dil, pad, res, relu))
    return out


SITES = _sites()


@pytest.mark.parametrize("site", SITES, ids=lambda s: s[0])
def test_backbone_site_writes_limb_planes_against_fp64(site):
    """Two images, input grid 33 x 65 for the layer1 rows and the two stride-2 rows, 17 x 33 for the rest: M = 4290 and 1122 --
    a partial last tile row and an image boundary inside a tile."""
    name, cin, cout, k, stride, dil, pad, res, relu = site
    Hi, Wi = (33, 65) if name.startswith("layer1") or stride == 2 else (17, 33)
    M = 2 * ref.out_size(Hi, k, stride, dil, pad) * ref.out_size(Wi, k, stride, dil, pad)
    assert M == (4290 if name.startswith("layer1") else 1122)
    confirm_plan(name, M, cout, k * k, cin)
    run_eval_geometry(name, 2, Hi, Wi, cin, cout, k, stride, dil, pad, res, relu, seed=300 + SITES.index(site))


# --------------------------------------------------------------------------------------- 3., 4. short K, partial columns
def test_short_k_128x128_unbalanced_writes_limb_planes_against_fp64():
    """64 -> 256 1 x 1: two K-steps (KT < 4), 128 x 128 tiles one per workgroup, never stream-K."""
    confirm_plan("short K", 4290, 256, 1, 64, kid=1, balanced=False)
    run_eval_geometry("shortk.128x128", 2, 33, 65, 64, 256, 1, 1, 1, 0, True, True, seed=31)


@pytest.mark.parametrize("cout", [160, 96])
def test_partial_column_tiles_write_limb_planes_against_fp64(cout):
    """Cout = 160: a whole column tile and one of 32 channels; Cout = 96: one partial tile.  One image 19 x 37 (M = 703)."""
    confirm_plan(f"partial column tile, Cout {cout}", 703, cout, 9, 128, kid=1)
    run_eval_geometry(f"cols.{cout}", 1, 19, 37, 128, cout, 3, 1, 1, 1, True, True, seed=40 + cout)


# ------------------------------------------------------------------------------------------------- 5. a loose bound
def test_a_bound_far_above_the_maximum_keeps_the_small_elements():
    """256 -> 256 3 x 3 on one image 24 x 40 with ONE input pixel scaled by 2^12: the bound follows the outlier, everything
    away from it is 2^-16 ... 2^-24 of the planes' scale -- limbs.h promises full accuracy there -- and the comparator's own
    denominators per block hold those blocks as they hold the rest.  Then a second limb-writing 1 x 1 conv reads the loosely
    scaled planes, held the same way against a reference fed with the first launch's materialized output."""
    H, W, C, h0, w0 = 24, 40, 256, 12, 20
    confirm_plan("loose bound, first conv", H * W, C, 9, C)
    x_scale = torch.ones(1, H, W, 1, device=DEV)
    x_scale[0, h0, w0, 0] = 2.0 ** 12
    r = run_eval_geometry("loose.3x3", 1, H, W, C, C, 3, 1, 1, 1, False, True, seed=51, x_scale=x_scale)
    # the construction, from the reference: the 64-row blocks all of whose pixels are at least 8 pixels from the outlier
    hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    near = (torch.maximum((hh - h0).abs(), (ww - w0).abs()) < 8).reshape(-1)
    far = [rb for rb in range(-(-H * W // ref.BLOCK)) if not bool(near[rb * ref.BLOCK:(rb + 1) * ref.BLOCK].any())]
    assert len(far) >= 4, far
    rows = torch.cat([torch.arange(rb * ref.BLOCK, min(H * W, (rb + 1) * ref.BLOCK)) for rb in far]).to(DEV)
    rms = float(r["y_ref"].reshape(-1, C)[rows].pow(2).mean().sqrt())
    assert 2.0 ** -24 * r["bound"] <= rms <= 2.0 ** -16 * r["bound"], (rms, r["bound"])
    num, den = ref._block_sums(r["got"], r["y_ref"], "act", r["mag"])
    worst = float(ref._ratio(num, den)[far].max())
    print(f"loose bound: rms away from the outlier 2^{math.log2(rms / r['bound']):.1f} of the bound; worst such block {worst:.2e}")
    assert worst <= ref.BOUNDS[MODE][1], worst
    confirm_plan("loose bound, second conv", H * W, C, 1, C)
    run_eval_geometry("loose.1x1.on.top", 1, H, W, C, C, 1, 1, 1, 0, False, True, seed=52, x=r["y"])


# -------------------------------------------------------------------------------------------- 6. degenerate scales
def test_a_zero_input_leaves_shift_plus_residual():
    """x == 0 with a residual: y = relu(shift + res), held to the same bounds (the planes' scale comes from the shift and
    the residual alone)."""
    x = torch.zeros(2, 17, 33, 128, device=DEV)
    confirm_plan("zero input", 1122, 256, 1, 128)
    r = run_eval_geometry("zero.x", 2, 17, 33, 128, 256, 1, 1, 1, 0, True, True, seed=61, x=x)
    assert r["true"] > 0


def test_all_zero_terms_store_exact_zero_limbs():
    """x == 0, shift == 0, no residual: every stored limb is exactly zero, bound and true maximum are 0, nothing is NaN."""
    x = torch.zeros(2, 17, 33, 128, device=DEV)
    for relu in (True, False):
        r = run_eval_geometry("zero.all", 2, 17, 33, 128, 256, 1, 1, 1, 0, False, relu, seed=62, x=x, shift_zero=True)
        planes = r["limbs"].planes
        assert int((planes.view(torch.int16) & 0x7FFF).ne(0).sum()) == 0  # (+-0 bit patterns only: no NaN, no value)
        assert r["bound"] == 0.0 and r["true"] == 0.0
        assert not bool(torch.isnan(r["limbs"].amax).any()) and not bool(torch.isnan(r["limbs"].true_amax).any())


# --------------------------------------------------------------------------------------------------------- 7. census
def test_the_sites_are_the_eval_forward(tmp_path):
    """One eval-mode forward of the model in "f16x2": the (Cin, Cout, k, stride, dil, residual?, relu?) that reach
    onda_conv2d_fwd_l2_limbs are exactly the sites the table above tests."""
    from onda_amd import ops
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_model
    from onda_amd.synthetic import fill_state_dict, synth_batch
    cfg, _spec = hybrid_switch_cfg(128, 64, DEV, str(tmp_path), batch_size=2)
    model = get_model(cfg, 19)
    fill_state_dict(model, 1, 1.0)
    model.eval()
    image = synth_batch(2, 64, 128, seed=5)["image"].to(DEV)
    real, seen = ops.conv._launch, set()

    def spy(name, flops, fn_name, *args, **kw):
        if fn_name == "onda_conv2d_fwd_l2_limbs":
            lo, d = args[7]._obj, args[9]._obj
            assert kw["tag"][2:] == (d.Cout, d.Cin, d.kh, d.stride, d.dil)
            seen.add((d.Cin, d.Cout, d.kh, d.stride, d.dil, bool(lo.res), bool(d.relu)))
        return real(name, flops, fn_name, *args, **kw)

    ops.conv._launch = spy
    try:
        with torch.no_grad():
            model(image)
        torch.cuda.synchronize()
    finally:
        ops.conv._launch = real
    want = {(cin, cout, k, stride, dil, res, relu) for _n, cin, cout, k, stride, dil, _pad, res, relu in SITES}
    assert seen == want, f"in the forward, not the table: {sorted(seen - want)}; in the table, not the forward: {sorted(want - seen)}"


# ------------------------------------------------------------------------------------------ 8. teacher-forced chain
def test_a_chain_of_bottlenecks_holds_launch_by_launch():
    """Three bottlenecks (1024 -> 256, 256 -> 256 dilation 2, 256 -> 1024 + residual) at 2 x 17 x 33, every intermediate
    limb-only.  Each of the nine launches is held to the per-launch bounds against a reference fed with THAT launch's own
    materialized inputs (no tolerance that grows with depth), and no bound sits more than 2^13 above its true maximum at any
    stage: bounds do not compound."""
    B, H, W = 2, 17, 33
    x = loose_planes((B, H, W, 1024), _gen(80))
    ratios = []
    for blk in range(3):
        a = run_eval_geometry(f"chain.{blk}.conv1", B, H, W, 1024, 256, 1, 1, 1, 0, False, True, seed=81 + 3 * blk, x=x)
        b = run_eval_geometry(f"chain.{blk}.conv2", B, H, W, 256, 256, 3, 1, 2, 2, False, True, seed=82 + 3 * blk, x=a["y"])
        c = run_eval_geometry(f"chain.{blk}.conv3", B, H, W, 256, 1024, 1, 1, 1, 0, x, True, seed=83 + 3 * blk, x=b["y"])
        ratios += [r["bound"] / r["true"] for r in (a, b, c)]
        x = c["y"]
    print("chain: bound / true maximum per launch: " + " ".join(f"2^{math.log2(q):.1f}" for q in ratios))
    assert max(ratios) <= LOOSEST
