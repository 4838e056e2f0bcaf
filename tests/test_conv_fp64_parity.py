"""The conv launches of the timed step held to fp64 at their real shapes (tests/conv_fp64.py: the reference, the comparator
and its bounds), in both conv modes; a census proving the table IS the step; and schedule edges the step does not reach, each
asserting through the library's dispatch queries that it takes the kernel and schedule it names.

Which launches: every geometry of the table, forward (+ statistics), data gradient (plain and accumulating) and weight
gradient, at the batch the student trains with (8 paired images in "f16x2", 4 in exact fp32), and in "f16x2" also at the
step's other batch, 4 images -- the M of the teacher / static / dynamic no-grad passes -- at 512x1024 and at bench.py's config
5, 1024x2048.  The no-grad passes themselves run the eval-mode epilogue that writes limb planes (BatchNorm folded,
onda_conv2d_fwd_l2_limbs); that epilogue is held to fp64 on every kernel path and at every backbone geometry by
tests/test_eval_conv_fp64_parity.py: here their geometries run through the train-mode entry points, same kernel choice and schedule."""
import ctypes
import gc
import math
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_fp64 as ref  # noqa: E402
from conv_fp64 import _edge_geometries, _schedule  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# Every conv geometry of the step bench.py times: get_model(hybrid_switch_cfg(1024, 512)) = DeepLabv2-ResNet50 with the ProDA
# ASPP head (deeplabv2.py), images 512 x 1024, batch 4.  Feature grids: stem 512x1024 -> 256x512, max-pool (ceil) -> 129x257
# (layer1), layer2's stride-2 1x1 -> 65x129 (layer2..4, ASPP).  Columns:
#   Hi, Wi, Cin, Cout, k, stride, dil, pad -- of the conv as the model declares it (the stem: on the image);
#   bias; stats = statistic rows the model asks for (4: BatchNorm convs, whose limb-writing BatchNorm also wants the per-channel
#   min / max -- 2 where ops.limb_mode is off, i.e. exact-fp32 mode; 2: the stem; 0: none); head = HEAD_PAD (the 19-class
#   head runs as a 32-wide GEMM); stem = through StemConvFn; acc = the data gradient is ADDED into a shared buffer
#   (ops.share_grad / GradSink: a bottleneck's input feeds conv1 and the shortcut -- the identity's BatchNorm residual or the
#   downsample conv runs backward first, conv1 adds; the ASPP input feeds five convs -- the last created, d24, runs first).
# (layer1's conv3 and its downsample share one geometry; so do the conv1 / conv2 / conv3 of all non-first blocks of a layer.)
BATCH = 4
STEP_CONVS = [
    # name              Hi    Wi    Cin  Cout  k  s  dil pad  bias  stats head stem  acc
    ("stem",            512, 1024,    3,   64, 7, 2, 1,  3,  False, 2,  0,   True,  False),
    ("layer1.0.conv1",  129,  257,   64,   64, 1, 1, 1,  0,  False, 4,  0,   False, True),
    ("layer1.conv2",    129,  257,   64,   64, 3, 1, 1,  1,  False, 4,  0,   False, False),
    ("layer1.conv3+ds", 129,  257,   64,  256, 1, 1, 1,  0,  False, 4,  0,   False, False),
    ("layer1.conv1",    129,  257,  256,   64, 1, 1, 1,  0,  False, 4,  0,   False, True),
    ("layer2.0.conv1",  129,  257,  256,  128, 1, 2, 1,  0,  False, 4,  0,   False, True),
    ("layer2.0.ds",     129,  257,  256,  512, 1, 2, 1,  0,  False, 4,  0,   False, False),
    ("layer2.conv2",     65,  129,  128,  128, 3, 1, 1,  1,  False, 4,  0,   False, False),
    ("layer2.conv3",     65,  129,  128,  512, 1, 1, 1,  0,  False, 4,  0,   False, False),
    ("layer2.conv1",     65,  129,  512,  128, 1, 1, 1,  0,  False, 4,  0,   False, True),
    ("layer3.0.conv1",   65,  129,  512,  256, 1, 1, 1,  0,  False, 4,  0,   False, True),
    ("layer3.0.ds",      65,  129,  512, 1024, 1, 1, 1,  0,  False, 4,  0,   False, False),
    ("layer3.conv2",     65,  129,  256,  256, 3, 1, 2,  2,  False, 4,  0,   False, False),
    ("layer3.conv3",     65,  129,  256, 1024, 1, 1, 1,  0,  False, 4,  0,   False, False),
    ("layer3.conv1",     65,  129, 1024,  256, 1, 1, 1,  0,  False, 4,  0,   False, True),
    ("layer4.0.conv1",   65,  129, 1024,  512, 1, 1, 1,  0,  False, 4,  0,   False, True),
    ("layer4.0.ds",      65,  129, 1024, 2048, 1, 1, 1,  0,  False, 4,  0,   False, False),
    ("layer4.conv2",     65,  129,  512,  512, 3, 1, 4,  4,  False, 4,  0,   False, False),
    ("layer4.conv3",     65,  129,  512, 2048, 1, 1, 1,  0,  False, 4,  0,   False, False),
    ("layer4.conv1",     65,  129, 2048,  512, 1, 1, 1,  0,  False, 4,  0,   False, True),
    ("aspp.1x1",         65,  129, 2048,  256, 1, 1, 1,  0,  True,  0,  0,   False, True),
    ("aspp.d6",          65,  129, 2048,  256, 3, 1, 6,  6,  True,  0,  0,   False, True),
    ("aspp.d12",         65,  129, 2048,  256, 3, 1, 12, 12, True,  0,  0,   False, True),
    ("aspp.d18",         65,  129, 2048,  256, 3, 1, 18, 18, True,  0,  0,   False, True),
    ("aspp.d24",         65,  129, 2048,  256, 3, 1, 24, 24, True,  0,  0,   False, False),
    ("aspp.bottleneck",  65,  129, 1280,  256, 3, 1, 1,  1,  True,  0,  0,   False, False),
    ("head",             65,  129,  256,   19, 1, 1, 1,  0,  False, 0,  32,  False, False),
]
# bench.py's config 5 (1024 x 2048): the same network one size up
SIZE_2X = {(512, 1024): (1024, 2048), (129, 257): (257, 513), (65, 129): (129, 257)}


def _at(geo, size):
    if size == 1:
        return geo
    name, Hi, Wi, *rest = geo
    return (name, *SIZE_2X[(Hi, Wi)], *rest)


@pytest.fixture(params=["f16x2", "f32"])
def mode(request):
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, request.param
    yield request.param
    ops.CONV_MODE = old


def _train_batch(ops):
    """Images per student pass: the step runs its source-replay and target passes as ONE pass over both batches (row groups
    of BATCH images) where the library supports it (prototypes.py _pairable), else one after the other."""
    return 2 * BATCH if ops.row_groups_supported() else BATCH


# ------------------------------------------------------------------------------------------ launch tags and kernel names
def _l2_kernel(M, cout, taps, cin):
    from onda_amd import ops
    from onda_amd._lib import query
    return ops.core._L2_KERNELS[query("onda_conv_l2_kernel_id", M, cout, taps, cin)]


def _launches(geo, B, mode, kinds=("fwd", "dgrad", "wgrad")):
    """{kind: (profile tag, kernel name)} of one table row at batch B, as ops.conv tags and names its launches."""
    from onda_amd import ops
    from onda_amd._lib import query
    _, Hi, Wi, Cin, Cout, k, stride, dil, pad, _bias, _stats, head, stem, _acc = geo
    Ho, Wo = ref.out_size(Hi, k, stride, dil, pad), ref.out_size(Wi, k, stride, dil, pad)
    M = B * Ho * Wo
    co = head or Cout
    if stem:  # the patch matrix: a 1 x 1 conv over STEM_K packed values
        Cin, k, stride, dil = ops.STEM_K, 1, 1, 1
    h2 = mode == "f16x2"
    out = {}
    if "fwd" in kinds:
        name = _l2_kernel(M, co, k * k, Cin) if h2 and Cin % 32 == 0 else "conv_fwd_kernel<128,%d>" % (128 if co > 64 else 64)
        out["fwd"] = (("fwd", M, co, Cin, k, stride, dil), name)
    if "dgrad" in kinds and not stem:
        Mo = M if stride != 1 else B * Hi * Wi
        name = _l2_kernel(Mo, Cin, k * k, co) if h2 and co % 32 == 0 else "conv_fwd_kernel<128,%d>" % (128 if Cin > 64 else 64)
        out["dgrad"] = (("dgrad", Mo, Cin, co, k, stride, dil), name)
    if "wgrad" in kinds:
        l2 = h2 and Cin % 32 == 0 and co % 32 == 0
        sk = ops.conv._wgrad_splitk(M, co, Cin, k * k, l2)
        name = ("conv_wgrad_l2_kernel<%d>" % query("onda_conv_wgrad_l2_variant", co, Cin) if l2
                else "conv_wgrad_kernel<%s>" % ("128,128" if (co > 64 and Cin > 64) else "64,64"))
        out["wgrad"] = (("wgrad", M, co, Cin, k, stride, dil, sk), name)
    return out


# --------------------------------------------------------------------------------------------------- one geometry
def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, device=DEV, generator=g) * scale


MEMORY_LIMIT = 12 << 30  # device bytes one item may hold at its peak: 16 processes share the card


def run_geometry(geo, B, mode, groups=0, accumulate=None, seed=1):
    """Forward (+ statistics), data gradient (plain, and added into a prefilled buffer where the model does that) and weight
    gradient of one geometry through the model's entry points, each held to fp64.  Returns the report dict.  A failure is
    re-raised with its message only: a traceback would keep this item's device tensors alive for the rest of the session."""
    try:
        return _run_geometry(geo, B, mode, groups, accumulate, seed)
    except AssertionError as e:
        msg = str(e)
    raise AssertionError(msg)


def _run_geometry(geo, B, mode, groups, accumulate, seed):
    from onda_amd import ops
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    name, Hi, Wi, Cin, Cout, k, stride, dil, pad, bias, stats, head, stem, acc = geo
    acc = acc if accumulate is None else accumulate
    Ho, Wo = ref.out_size(Hi, k, stride, dil, pad), ref.out_size(Wi, k, stride, dil, pad)
    co = head or Cout
    g = _gen(seed)
    w = _randn((Cout, Cin, k, k), g, 1.0 / math.sqrt(Cin * k * k))
    b = _randn((Cout,), g) if bias else None
    wd = w.clone().requires_grad_(True)
    bd = b.clone().requires_grad_(True) if bias else None
    want = (4 if ops.limb_mode(Cout) else True) if stats == 4 else bool(stats)
    report = {"geometry": f"{name} B={B} {Hi}x{Wi} {Cin}->{Cout} k{k} s{stride} d{dil}", "mode": mode}
    with ops.row_groups(groups):
        if stem:
            img = _randn((B, 3, Hi, Wi), g)
            x = img.permute(0, 2, 3, 1)
            y, st = ops.StemConvFn.apply(img, wd, ops._PackCache(), want)
        else:
            x = _randn((B, Hi, Wi, Cin), g).requires_grad_(True)
            y, st = ops.Conv2dFn.apply(x, wd, bd, ops._PackCache(), stride, dil, pad, want, head or None)
    dy = _randn((B, Ho, Wo, co), g)
    if head:
        dy[..., Cout:] = 0  # ClassSliceFn's gradient: nothing flows into the padded columns
    launches = _launches(geo, B, mode)
    res = report["passes"] = {}

    # forward
    yr = ref.conv_fwd(x.detach(), w, stride, dil, pad, b)
    exact = [(0.0, torch.arange(co, device=DEV) >= Cout)] if head else []
    res["fwd"] = ref.check(y[..., :Cout] if head else y, yr, mode, f"{name} fwd", exact=[])
    for want_v, mask in exact:
        assert ref.exact_violations(y, want_v, mask) == 0, f"{name}: padded head columns are not 0"
    if stats:
        assert st is not None and st.shape[1] == (4 if want == 4 else 2)
        s = st.double().sum(0)
        sr = ref.channel_stats(yr, with_abs=True)
        # a per-channel SUM of M fp32 values: its error scale is sum|y| (no relative bound holds for a sum that cancels)
        err = ((s[:2] - sr[:2]) / sr[[2, 1]]).abs().max().item()
        assert err <= ref.BOUNDS[mode][0], f"{name}: statistics sum / sumsq error {err:.3e} of sum|y|"
        if st.shape[1] == 4:  # per-channel min / max of the raw output: exactly the kernel's own y
            yk = y.detach().reshape(-1, Cout)
            assert torch.equal(st[:, 2].min(0)[0], yk.min(0)[0]) and torch.equal(st[:, 3].max(0)[0], yk.max(0)[0]), name
    del yr

    # data gradient and weight gradient (autograd through the Function, as the model runs them)
    with ops.row_groups(groups):
        y.backward(dy)
    if not stem:
        dxr = ref.conv_dgrad(dy[..., :Cout], w, (Hi, Wi), stride, dil, pad)
        unreached = ref.dgrad_unreached((Hi, Wi), k, stride, dil, pad, (Ho, Wo), DEV)[None, :, :, None]
        res["dgrad"] = ref.check(x.grad, dxr, mode, f"{name} dgrad", exact=[(0.0, unreached)])
        if acc:  # the GradSink path: the gradient ADDED into a prefilled dense buffer
            buf = _randn((B, Hi, Wi, Cin), g)
            prefill = buf.clone()
            wpd = ops.pack_weight_dgrad(w, head or None)
            out = ops.conv_dgrad(dy, wpd, k, stride, dil, pad, Cin, (Hi, Wi), accumulate=buf)
            assert out is buf
            dxr += prefill
            res["dgrad+acc"] = ref.check(buf, dxr, mode, f"{name} dgrad accumulate", exact=[(prefill, unreached)])
            del buf, prefill
        del dxr
    dwr = ref.conv_wgrad(x.detach(), dy[..., :Cout], k, stride, dil, pad)
    sk = launches["wgrad"][0][-1]
    chain = -(-(-(-launches["wgrad"][0][1] // sk)) // 32)  # K-steps of 32 pixels one workgroup accumulates in fp32
    dead = ref.dead_taps((Hi, Wi), k, stride, dil, pad).reshape(1, 1, k, k).to(DEV)
    res["wgrad"] = ref.check(wd.grad, dwr, mode, f"{name} wgrad", kind="wgrad", exact=[(0.0, dead)],
                             bounds=ref.chain_bounds(mode, chain))
    if bias:
        sd = ref.channel_stats(dy[..., :Cout], with_abs=True)
        err = ((bd.grad.double() - sd[0]) / sd[2]).abs().max().item()
        assert err <= ref.BOUNDS[mode][0], f"{name}: bias gradient error {err:.3e} of sum|dy|"
    report["launches"] = {kind: (tag, kname) for kind, (tag, kname) in launches.items()}
    line = "  ".join(f"{p} {launches.get(p.split('+')[0], (None, '?'))[1]}"
                     f"{' sk=%d chain=%d' % (sk, chain) if p == 'wgrad' else ''} rel {t:.2e} block {bb:.2e}"
                     for p, (t, bb) in res.items())
    torch.cuda.synchronize()
    report["peak_bytes"] = peak = torch.cuda.max_memory_allocated()
    print(f"[{mode}] {report['geometry']}: {line}  peak {peak / 2**30:.2f} GiB")
    assert peak < MEMORY_LIMIT, f"{name}: {peak / 2**30:.2f} GiB of device memory at the peak"
    return report


@pytest.mark.parametrize("size", [1, 2], ids=["512x1024", "1024x2048"])
@pytest.mark.parametrize("geo", STEP_CONVS, ids=lambda g: g[0])
def test_step_conv_at_batch4_against_fp64(geo, size):
    """"f16x2": one table row at BATCH images, at the step's size (the no-grad passes' M: 33540 = 131 * 256 + 4 at layer2..4,
    the partial last tile row) and at 1024x2048, bench config 5 (M = 132612 / 527364 / 2097152, the largest splits)."""
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    geo = _at(geo, size)
    try:
        run_geometry(geo, BATCH, "f16x2", seed=zlib.crc32(geo[0].encode()) & 0xFFFF ^ size)
    finally:
        ops.CONV_MODE = old
        torch.cuda.empty_cache()


@pytest.mark.parametrize("geo", STEP_CONVS, ids=lambda g: g[0])
def test_step_conv_against_fp64(geo, mode):
    """One table row at the step's size, in both conv modes, at the batch the student trains with (row groups as the step)."""
    from onda_amd import ops
    B = _train_batch(ops)
    try:
        run_geometry(geo, B, mode, groups=BATCH if B > BATCH else 0, seed=zlib.crc32(geo[0].encode()) & 0xFFFF)
    finally:
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ census
def _step_launches(tmp_path, width, height):
    """Distinct (tag, kernel) of one adaptation step as _full_size_step_against runs it, and the data-gradient launches
    that were added into a shared buffer."""
    from onda_amd import ops
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.framework.model import deeplabv2
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.synthetic import fill_state_dict, synth_batch
    from oracle import model as omodel
    cfg, spec = hybrid_switch_cfg(width, height, DEV, str(tmp_path), batch_size=BATCH)
    model = get_model(cfg, 19)
    fill_state_dict(model, 1, 1.0)
    da = get_adapt_method(cfg)(model, cfg, spec)
    src = [synth_batch(BATCH, height, width, seed=1000 + i) for i in range(2)]
    trg = synth_batch(BATCH, height, width, seed=2000)
    torch.manual_seed(123)
    masks = iter([omodel.draw_drop_mask(BATCH) for _ in range(6)])
    deeplabv2.drop_mask_fn = lambda B, C, p, dev: next(masks).to(dev)
    real_dgrad, seen, depth = ops.conv.conv_dgrad, set(), [0]

    def dgrad(dy, wpd, k, stride, dil, pad, cin, in_hw, accumulate=None):
        if depth[0] == 0:
            B, Ho, Wo, Co = dy.shape
            Mo = B * Ho * Wo if stride != 1 else B * in_hw[0] * in_hw[1]
            seen.add((("dgrad", Mo, cin, Co, k, stride, dil), accumulate is not None))
        depth[0] += 1
        try:
            return real_dgrad(dy, wpd, k, stride, dil, pad, cin, in_hw, accumulate=accumulate)
        finally:
            depth[0] -= 1
    try:
        da.update_dynamic()
        switch_batch_statistics(da.model, False)
        da.calculate_prototypes(src, save=False)
        switch_batch_statistics(da.model, True)
        da.optimizer.zero_grad()
        da.adjust_learning_rate(0, 6)
        ops.PROFILE = []
        ops.conv.conv_dgrad = dgrad
        da.step([src[0]], trg)
        torch.cuda.synchronize()
        entries = ops.profile_entries(ops.PROFILE)
    finally:
        ops.PROFILE = None
        ops.conv.conv_dgrad = real_dgrad
        deeplabv2.drop_mask_fn = deeplabv2._default_drop_mask
    return {(e[4], e[0]) for e in entries if e[4] is not None and e[4][0] in ("fwd", "dgrad", "wgrad")}, seen


def _table_launches(size, mode):
    from onda_amd import ops
    Bt = _train_batch(ops)
    want, acc = set(), set()
    for geo in STEP_CONVS:
        geo = _at(geo, size)
        for kind, launch in _launches(geo, Bt, mode).items():
            want.add(launch)
            if kind == "dgrad":
                acc.add((launch[0], geo[-1]))
        want.add(_launches(geo, BATCH, mode, ("fwd",))["fwd"])  # teacher / static / dynamic: no-grad passes of BATCH images
    return want, acc


@pytest.mark.parametrize("size", [1, 2], ids=["512x1024", "1024x2048"])
def test_the_table_is_the_step(tmp_path, mode, size):
    if size == 2 and mode != "f16x2":
        pytest.skip("config 5 runs the default conv mode")
    seen, seen_acc = _step_launches(tmp_path, 1024 * size, 512 * size)
    want, want_acc = _table_launches(size, mode)
    assert seen == want, f"in the step, not the table: {sorted(seen - want)}; in the table, not the step: {sorted(want - seen)}"
    assert seen_acc == want_acc, (f"accumulated data gradients, step only: {sorted(seen_acc - want_acc)}; "
                                  f"table only: {sorted(want_acc - seen_acc)}")


# ------------------------------------------------------------------------------------------------ schedule edges
@pytest.mark.parametrize("i", range(7))
def test_conv_schedule_edges_against_fp64(i):
    """A schedule branch the step does not reach: the library's dispatch queries confirm the kernel and the (un)balanced
    schedule before the launches are held to fp64."""
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    try:
        label, geo, kid, balanced, rem = _edge_geometries()[i]
        _, H, W, cin, cout, k = geo[:6]
        kid_got, bal_got, rem_got, G = _schedule(H * W, cout, k * k, cin)
        assert kid_got == kid, (label, kid_got)
        if balanced is not None:
            assert bal_got == balanced, (label, bal_got)
        if rem is not None:  # (construction: the tile count this geometry was built for)
            assert rem_got == rem, (label, rem_got, G)
        print(f"edge: {label}: G={G} kernel {kid_got} balanced {bal_got} remainder {rem_got}")
        run_geometry(geo, 1, "f16x2", seed=100 + i)
    finally:
        ops.CONV_MODE = old
        torch.cuda.empty_cache()


@pytest.mark.parametrize("which", ["linear", "pixel-table", "128-wide"])
def test_weight_gradient_at_the_split_floor_against_fp64(which):
    """The weight-gradient kernels at the smallest split the library allows: ceil(M / 65536), a workgroup's K range at the
    2048 listed K-steps of 32 pixels."""
    from onda_amd import ops
    from onda_amd._lib import query
    cout, k = {"linear": (256, 1), "pixel-table": (256, 3), "128-wide": (128, 3)}[which]
    H, W, cin = 256, 767, 128  # M = 196352: floor 3, 2046 K-steps per split
    geo = (f"wgrad.{which}", H, W, cin, cout, k, 1, 1, k // 2, False, 0, 0, False, False)
    d = ops._desc(1, H, W, cin, H, W, cout, k, 1, 1, k // 2, cin, cout)
    assert query("onda_conv_wgrad_l2_variant", cout, cin) == (1 if which == "128-wide" else 0)
    assert (query("onda_conv2d_wgrad_l2_table_stride", ctypes.byref(d)) > 0) == (which == "pixel-table")
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    real = ops.conv._wgrad_splitk
    floor = -(-H * W // 65536)
    assert floor == 3 and -(-H * W // floor) <= 2048 * 32
    ops.conv._wgrad_splitk = lambda M, co, ci, taps, l2=False: -(-M // 65536)
    try:  # (run_geometry holds the weight gradient to ref.chain_bounds of its 2046 K-steps per workgroup)
        run_geometry(geo, 1, "f16x2", seed=7)
    finally:
        ops.conv._wgrad_splitk = real
        ops.CONV_MODE = old
        torch.cuda.empty_cache()


def test_dilation_past_the_image_is_the_centre_tap_alone():
    """3 x 3, dilation 24 on a 9 x 17 image: the eight outer taps see padding only -- their weight gradient is exactly 0 and
    the forward pass is the centre tap's 1 x 1 conv."""
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    try:
        geo = ("dil24.9x17", 9, 17, 256, 256, 3, 1, 24, 24, True, 0, 0, False, False)
        assert ref.dead_taps((9, 17), 3, 1, 24, 24).sum() == 8
        run_geometry(geo, 2, "f16x2", seed=24)
        g = _gen(5)
        x = _randn((2, 9, 17, 256), g)
        w = _randn((256, 256, 3, 3), g, 1 / 48)
        y, _ = ops.Conv2dFn.apply(x, w, None, ops._PackCache(), 1, 24, 24, False, None)
        centre = ref.conv_fwd(x, w[:, :, 1:2, 1:2])
        ref.check(y, centre, "f16x2", "dilation 24 forward = centre tap")
    finally:
        ops.CONV_MODE = old


# ------------------------------------------------------------------------------------- weight gradient: bad tables
def test_weight_gradient_refuses_a_bad_pixel_table(monkeypatch, capfd):
    """onda_conv2d_wgrad_l2 with a caller's pixel table that is misaligned, has a row stride that is not whole 16-byte groups,
    or belongs to a geometry of 2^31 or more input pixels (its int32 entries would wrap): refused before any launch.  The
    library names the failed requirement on stderr under ONDA_DEBUG_REQUIRE: the refusal must come from the table checks.
    (The 2^31 case is a stride-2 geometry, M = 2^29 < 2^31 <= B * Hi * Wi, so the M < 2^31 requirement passes; at split 1
    its pixel range would still fail the K-step limit further down -- a second refusal, so that the case can never launch.)"""
    from onda_amd import ops
    from onda_amd._lib import call
    B, H, W, cin, cout, k = 1, 8, 8, 256, 256, 3
    xl = torch.zeros(2 * B * H * W * cin, device=DEV, dtype=torch.float16)
    dyl = torch.zeros(2 * B * H * W * cout, device=DEV, dtype=torch.float16)
    amax = torch.zeros(64, device=DEV)
    slabs = torch.zeros(cout * 9 * cin, device=DEV)
    M = B * H * W
    stride = (M + 31) // 32 * 32 + 64
    table = torch.full((9 * stride + 8,), -1, device=DEV, dtype=torch.int32)
    monkeypatch.setenv("ONDA_DEBUG_REQUIRE", "1")

    def launch(d):
        capfd.readouterr()
        call("onda_conv2d_wgrad_l2", ops._p(xl), 0, ops._p(amax), ops._p(dyl), 0, ops._p(amax), ops._p(slabs), cout, 1,
             ctypes.byref(d), ops._stream())

    def refused_by(text):
        err = capfd.readouterr().err
        assert err.count("requirement failed") == 1 and text in err, err

    def desc(ptr, pstride, b=B, h=H, w=W, cstride=1):
        ho = (h + 2 - 2 - 1) // cstride + 1
        d = ops._desc(b, h, w, cin, ho, ho, cout, k, cstride, 1, 1, cin, cout)
        d.pix_table, d.pix_stride = ptr, pstride
        return d

    with pytest.raises(RuntimeError, match="ONDA_EALIGN"):
        launch(desc(table.data_ptr() + 4, stride))  # 4-byte aligned only
    assert "requirement failed" not in capfd.readouterr().err  # (the alignment return is not an ONDA_REQUIRE)
    with pytest.raises(RuntimeError, match="ONDA_EINVAL"):
        launch(desc(table.data_ptr(), stride + 2))  # rows of whole int4 groups
    refused_by("c->pix_stride % 4 == 0")
    d = desc(table.data_ptr(), 1 << 40, b=1 << 25, cstride=2)
    assert d.B * d.Ho * d.Wo < (1 << 31) <= d.B * d.Hi * d.Wi
    with pytest.raises(RuntimeError, match="ONDA_EINVAL"):
        launch(d)
    refused_by("c->B * c->Hi * c->Wi < (1ll << 31)")
    torch.cuda.synchronize()
