"""GPU: the tap-table convolution (onda_conv2d_taps_fwd_l2, onda_pack_sum_h2) and ops.SumConvFn -- the DeepLabV2 'normal' head's
sum of four dilated 3 x 3 convolutions -- against float64: conv_fp64.conv_fwd / conv_dgrad / conv_wgrad summed over the dilations
(normal_head_common; tests/test_normal_head_reference.py ties that sum to the reference's module), held by conv_fp64.check with
conv_fp64.BOUNDS.  Every case stays under 280 K-steps (36 taps x Cin / 32 <= 108; weight gradients <= 1836 / 32 pixels steps), so
chain_bounds does not come into play; the bias gradient -- one column sum over M <= 1875 rows -- is held to BOUNDS as well.

Shapes: the smallest at which this kernel can still go wrong --
  B=2, 27x34, Cin 64 and 96: every dilation has live taps; M = 1836 is seven 256-row tiles and a partial one, one tile lies
     across the two images (a tap's offset must not reach into the neighbouring image); Cin 96 gives the data gradient a second
     tile shape (96 output columns: 128 x 128 tiles) and three K-steps per tap;
  B=1, 9x17, Cin 64: less than one tile; only the centre taps and a part of dilation 6 are live (every other tap is dead by its
     row or its column offset);
  B=3, 25x25, Cin 32: the dilation-24 taps reach exactly one row / column; one K-step per tap.
The kernel-level tests run each case on both schedules (ONDA_CONV_SCHED 1: one tile per workgroup, where whole tiles skip their
dead taps through the 64-bit mask; 2: stream-K pieces and the fix-up launch, the schedule these shapes get by default) and, forced
by ONDA_L2_VARIANT=0, on the 256 x 128 eight-wave tile the workload's data gradient runs on."""
import ctypes
import os

import pytest
import torch

import conv_fp64 as R
import normal_head_common as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, PAD = C.CLASSES, 32
GEOMS = tuple((3, d, d) for d in C.DILATIONS)
CASES = [("b2-27x34-c64", 2, 27, 34, 64), ("b2-27x34-c96", 2, 27, 34, 96), ("b1-9x17-c64", 1, 9, 17, 64), ("b3-25x25-c32", 3, 25, 25, 32)]
ROUTES = [("f16x2", True), ("f16x2", False), ("f32", False)]  # (conv mode, ops.TAP_CONV): the table route exists in "f16x2" only
SCHEDULES = [("1", None), ("2", None), ("1", "0"), ("2", "0")]  # (ONDA_CONV_SCHED, ONDA_L2_VARIANT)

_DATA = {}


def data(case):
    """Inputs and float64 references of a case, computed once (on the GPU, in float64) and left unchanged."""
    if case[0] in _DATA:
        return _DATA[case[0]]
    _, B, H, W, cin = case
    x = C.head_input(B, cin, H, W).permute(0, 2, 3, 1).contiguous().to(DEV)
    ws, bs = C.head_params(cin)
    ws, bs = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    dy = torch.zeros(B, H, W, PAD, device=DEV)
    dy[..., :K] = C.head_dout(B, K, H, W).permute(0, 2, 3, 1).to(DEV)
    d = types_ns(x=x, ws=ws, bs=bs, dy=dy, y=C.sum_fwd64(x, ws), yb=C.sum_fwd64(x, ws, bs), dx=C.sum_dgrad64(dy[..., :K], ws, (H, W)),
                 dws=C.sum_wgrads64(x, dy[..., :K]), db=R.bias_grad(dy[..., :K]))
    _DATA[case[0]] = d
    return d


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


class switches:
    def __init__(self, mode, tap_conv, **env):
        self.mode, self.tap, self.env = mode, tap_conv, env

    def __enter__(self):
        from onda_amd import ops
        self.old = ops.CONV_MODE, ops.TAP_CONV
        ops.CONV_MODE, ops.TAP_CONV = self.mode, self.tap
        self.old_env = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        from onda_amd import ops
        ops.CONV_MODE, ops.TAP_CONV = self.old
        for k, v in self.old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def pad_is_zero(t, what):
    assert R.exact_violations(t[..., K:], 0.0) == 0, f"{what}: padded columns {K}..{PAD - 1} are not exactly zero"


def shift_of(bs):
    s = torch.zeros(PAD, device=DEV)
    s[:K] = torch.stack(bs).sum(0)
    return s


# ------------------------------------------------------------------------------------------------ the kernel and the packer
@pytest.mark.parametrize("sched,variant", SCHEDULES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_tap_kernel_against_fp64(case, sched, variant):
    from onda_amd import ops
    d = data(case)
    _, B, H, W, cin = case
    taps, neg = ops.sum_taps(GEOMS), ops.sum_taps(GEOMS, negate=True)
    with switches("f16x2", True, ONDA_CONV_SCHED=sched, ONDA_L2_VARIANT=variant):
        pack = ops._SumPack(4).get(d.ws, PAD, True)
        y = ops.conv_taps(d.x, pack.fwd, taps, PAD)
        yb = ops.conv_taps(d.x, pack.fwd, taps, PAD, shift=shift_of(d.bs))
        dx = ops.conv_taps(d.dy, pack.dgrad, neg, cin, kind="dgrad")
        prefill = torch.randn(B, H, W, cin, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
        acc = prefill.clone()
        assert ops.conv_taps(d.dy, pack.dgrad, neg, cin, out=acc, residual=acc, kind="dgrad") is acc
        # teeth: one tap of the table pointed far outside the image (= dropped), one dilation's weights zeroed
        lame = list(taps)
        lame[4] = (16000, 16000)
        y_tap = ops.conv_taps(d.x, pack.fwd, lame, PAD)
        y_dil = ops.conv_taps(d.x, ops._SumPack(4).get(d.ws[:3] + [torch.zeros_like(d.ws[3])], PAD, False).fwd, taps, PAD)
        torch.cuda.synchronize()
    what = f"{case[0]} sched {sched} variant {variant}"
    figs = [R.check(y[..., :K], d.y, "f16x2", what + " forward"), R.check(yb[..., :K], d.yb, "f16x2", what + " forward + bias"),
            R.check(dx, d.dx, "f16x2", what + " data gradient"),
            R.check(acc, prefill.double() + d.dx, "f16x2", what + " data gradient, accumulated")]
    print(what, " | ".join(f"{n} {t:.2e}/{b:.2e}" for n, (t, b) in zip(("fwd", "fwd+bias", "dgrad", "dgrad+="), figs)))
    pad_is_zero(y, what + " forward")
    pad_is_zero(yb, what + " forward + bias")
    assert R.flagged(y_tap[..., :K], d.y, "f16x2") and R.flagged(y_dil[..., :K], d.y, "f16x2")


def test_rejections_launch_nothing():
    """ONDA_EINVAL (-1) / ONDA_EALIGN (-2) before anything is launched: the output, prefilled with NaN, stays NaN."""
    from onda_amd import _lib, ops
    from onda_amd.ops.core import _conv_ws, _desc, _p, _stream
    d = data(CASES[0])
    _, B, H, W, cin = CASES[0]
    with switches("f16x2", True):
        pack = ops._SumPack(4).get(d.ws, PAD, False)
        xl = ops.limbs_of(d.x)
        y = torch.full((B, H, W, PAD), float("nan"), device=DEV)
        stats = torch.zeros(64, 2, PAD, device=DEV)
        flag = torch.ones(1, dtype=torch.int32, device=DEV)
        table = (ctypes.c_int * 72)(*([0, 0] * 36))
        fn = _lib.load().onda_conv2d_taps_fwd_l2

        def run(desc, ntaps=36, out=None, stat=None, lo=None, x_planes=None, ldy=None):
            c = _desc(B, H, W, cin, H, W, PAD, 1, 1, 1, 0, xl.ld, PAD if ldy is None else ldy)
            for k_, v in desc.items():
                setattr(c, k_, v)
            return fn(_p(xl.planes) if x_planes is None else x_planes, _p(xl.amax), _p(pack.fwd.limbs), _p(pack.fwd.amax),
                      y.data_ptr() if out is None else out, None, None, stat, lo, _p(_conv_ws(d.x.device)), None, ctypes.byref(c),
                      table, ntaps, _stream())

        lo = _lib.OndaLimbOut()
        assert run({"Cin": 48}) == -1 and run({"Cin": 0}) == -1
        assert run({}, ntaps=0) == -1 and run({}, ntaps=65) == -1
        assert run({"stride": 2}) == -1 and run({"Ho": H - 1}) == -1
        assert run({}, stat=stats.data_ptr()) == -1
        assert run({}, lo=ctypes.addressof(lo)) == -1
        assert run({"run_if": flag.data_ptr()}) == -1
        table[0] = 20000
        assert run({}) == -1
        table[0] = 0
        assert run({}, out=y.data_ptr() + 4) == -2
        assert run({}, x_planes=_p(xl.planes) + 2) == -2
        assert run({}, ldy=PAD + 2) == -2
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all())
        # ... and the same call with nothing wrong runs: 36 taps at offset (0, 0) = one 1 x 1 convolution with the summed taps
        assert run({}) == 0
        torch.cuda.synchronize()
        w_sum = torch.stack([w.double().sum((2, 3)) for w in d.ws]).sum(0)  # [K, cin]
        R.check(y[..., :K], d.x.double() @ w_sum.t(), "f16x2", "36 coincident taps")
        pad_is_zero(y, "36 coincident taps")


# ------------------------------------------------------------------------------------------------ ops.SumConvFn, every route
def _run_sum_fn(d, cin, with_bias=True, consumers=1):
    """(y of the first consumer, x.grad, [dW], [db]) of `consumers` SumConvFn readers of one x (the second one's upstream gradient
    is half the first one's: GradSink then holds 1.5 x the data gradient)."""
    from onda_amd import ops
    x = d.x.clone().requires_grad_(True)
    ws = [w.clone().requires_grad_(True) for w in d.ws]
    bs = [b.clone().requires_grad_(True) for b in d.bs] if with_bias else []
    if consumers > 1:
        ops.share_grad(x)
        assert getattr(x, "_onda_sink", None) is not None
    ys = [ops.SumConvFn.apply(x, ops._SumPack(4), GEOMS, PAD, *ws, *bs) for _ in range(consumers)]
    torch.autograd.backward(ys, [d.dy * (0.5 ** i) for i in range(consumers)])
    torch.cuda.synchronize()
    return ys[0].detach(), x.grad, [w.grad for w in ws], [b.grad for b in bs]


@pytest.mark.parametrize("mode,tap_conv", ROUTES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_sum_conv_fn_against_fp64(case, mode, tap_conv):
    from onda_amd import ops
    d = data(case)
    cin = case[4]
    what = f"{case[0]} {mode} {'taps' if tap_conv else 'chain'}"
    with switches(mode, tap_conv):
        assert ops.sum_conv_route(cin, PAD) == ("taps" if tap_conv else "chain")
        y, dx, dws, dbs = _run_sum_fn(d, cin)
        with torch.no_grad():
            y0 = ops.SumConvFn.apply(d.x, ops._SumPack(4), GEOMS, PAD, *d.ws)
        _, dx2, dws2, _ = _run_sum_fn(d, cin, consumers=2)
    assert tuple(y.shape) == tuple(d.dy.shape) and all(tuple(g.shape) == (K, cin, 3, 3) for g in dws) and all(tuple(g.shape) == (K,) for g in dbs)
    figs = [R.check(y[..., :K], d.yb, mode, what + " forward + bias"), R.check(y0[..., :K], d.y, mode, what + " forward"),
            R.check(dx, d.dx, mode, what + " data gradient"), R.check(dx2, 1.5 * d.dx, mode, what + " data gradient, two consumers")]
    pad_is_zero(y, what + " forward + bias")
    pad_is_zero(y0, what + " forward")
    for i, (dw, db) in enumerate(zip(dws, dbs)):
        figs.append(R.check(dw, d.dws[i], mode, what + f" dW dilation {C.DILATIONS[i]}", kind="wgrad"))
        figs.append(R.check(dws2[i], 1.5 * d.dws[i], mode, what + f" dW dilation {C.DILATIONS[i]}, two consumers", kind="wgrad"))
        R.check(db.reshape(1, -1), d.db.reshape(1, -1), mode, what + f" db {i}")
    print(what, " | ".join(f"{t:.2e}/{b:.2e}" for t, b in figs))
    # teeth, on the result of the route itself: without one dilation's branch the comparator fails
    short = y0[..., :K].double() - R.conv_fwd(d.x, d.ws[3], 1, 24, 24)
    assert R.flagged(short, d.y, mode)


@pytest.mark.parametrize("case", CASES[:2], ids=lambda c: c[0])
def test_the_two_routes_agree(case):
    """Each route is within BOUNDS of float64, so they are within twice that of each other (the triangle inequality; their
    roundings differ: one shared weight scale and one accumulator against four scales and four rounded partial sums)."""
    d = data(case)
    cin = case[4]
    with switches("f16x2", True):
        a = _run_sum_fn(d, cin)
    with switches("f16x2", False):
        b = _run_sum_fn(d, cin)
    twice = tuple(2 * v for v in R.BOUNDS["f16x2"])
    R.check(a[0][..., :K], b[0][..., :K].double(), "f16x2", "forward, taps against chain", bounds=twice)
    R.check(a[1], b[1].double(), "f16x2", "data gradient, taps against chain", bounds=twice)
    for i in range(4):  # the weight and bias gradients do not depend on the route: the same launches on the same operands
        assert torch.equal(a[2][i], b[2][i]) and torch.equal(a[3][i], b[3][i])


def test_pack_cache_follows_the_weight_versions():
    from onda_amd import ops
    d = data(CASES[3])
    with switches("f16x2", True):
        ws = [w.clone() for w in d.ws]
        cache = ops._SumPack(4)
        first = cache.get(ws, PAD, False).fwd
        assert cache.get(ws, PAD, False).fwd is first and cache.dgrad is None
        assert cache.get(ws, PAD, True).dgrad is not None
        again = cache.fwd
        ws[2].mul_(2.0)
        assert cache.get(ws, PAD, True).fwd is not again
        y = ops.conv_taps(d.x, cache.fwd, ops.sum_taps(GEOMS), PAD)
        torch.cuda.synchronize()
    R.check(y[..., :K], C.sum_fwd64(d.x, ws), "f16x2", "after an in-place weight update")
