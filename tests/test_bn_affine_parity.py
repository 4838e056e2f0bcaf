"""GPU: dgamma / dbeta of the three train-mode BatchNorm Functions (ops.BNTrainLimbFn, ops.BNPairLimbFn, ops.BNTrainFn; csrc/norm_l2.hip
onda_bn_bwd_affine_l2 / onda_bn_pair_bwd_affine_l2, csrc/norm.hip onda_bn_bwd_affine) held to the float64 restatement of
tests/bn_affine_fp64.py, per channel, with the bounds derived there.  The conv outputs and their statistic partials come out of a
real HipConv2d (1x1, the identity plus a little mixing, so that y carries norm_fp64's channel population); the restatement starts
from the fp32 conv output the device returned and takes the device's own ReLU mask.

Shapes: the smallest that reach every branch of the backward plan (col_plan3: C = 32 -> 256 rows a chunk, C = 64 -> 128,
C = 2048 -> 32 and the (C / 8) % 256 == 0 branch of the apply pass): one chunk, three chunks, a split that gives 2 + 2 chunks (one
chunk row more than the plan of all rows), each with ReLU + residual and without.  Every case also runs frozen, gamma only and
beta only: the frozen run must make the calls the Functions always made, dx / dres must not depend on who asks for what, and a
second run must give the same bits."""
import numpy as np
import pytest
import torch

import bn_affine_fp64 as A
import norm_fp64 as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ids = lambda c: c.id  # noqa: E731


class Case:
    def __init__(self, kind, C, shape, first=0, relu=True, res=False, fuse=None):
        self.kind, self.C, self.shape, self.first, self.relu, self.res, self.fuse = kind, C, shape, first, relu, res, fuse
        B, H, W = shape
        self.M, self.split = B * H * W, first * H * W
        self.id = f"{kind}-c{C}-m{self.M}" + (f"-split{self.split}" if first else "") + ("-relu-res" if relu and res else "-plain" if not relu else "-relu") \
            + ("" if fuse is None else "-fused" if fuse else "-unfused")


def _both(kind, C, shape, first=0, fuse=None):
    return [Case(kind, C, shape, first, True, True, fuse), Case(kind, C, shape, first, False, False, fuse)]


LIMB_CASES = (_both("limb", 32, (2, 9, 13)) + _both("limb", 32, (2, 9, 13), 1) + _both("limb", 32, (2, 17, 19)) + _both("limb", 32, (2, 17, 19), 1)
              + _both("limb", 64, (2, 9, 13)) + _both("limb", 2048, (1, 5, 7))
              # both ways of running the sums pass: its own launch, and the first workgroups of the apply launch
              + [Case("limb", 32, (2, 17, 19), 1, True, True, fuse=False), Case("limb", 32, (2, 17, 19), 1, True, True, fuse=True),
                 Case("limb", 64, (2, 9, 13), 0, True, False, fuse=False), Case("limb", 64, (2, 9, 13), 0, True, False, fuse=True)])
PAIR_CASES = [Case("pair", C, (2, 9, 13), first) for C in (32, 256) for first in (0, 1)]
FP32_CASES = [Case("fp32", 64, (2, 17, 33), 0, True, True), Case("fp32", 64, (2, 17, 33), 1, True, True)]


@pytest.fixture
def f16x2():
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, "f16x2"
    yield
    ops.CONV_MODE = old


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for what in sorted(N.MEASURED):
        if "dgamma" in what or "dbeta" in what:
            print(f"worst ratio to its bound: {what}: {N.MEASURED[what][0]:.3f} at {N.MEASURED[what][1]}")


def _limb_supported():
    from onda_amd import ops
    return ops.H2_PATH == "dma" and ops.LIMB_ONLY


def _side(case, k):
    """Input, affine parameters and the conv of one BatchNorm, seeded by the case."""
    from onda_amd.framework.model.deeplabv2 import HipConv2d
    C, M = case.C, case.M
    seed = N.case_seed(case.id) + 1000 * k
    x, gamma, beta = N.bn_input(M, C, seed, shift_rows=case.split)
    g = torch.Generator().manual_seed(seed + 2)
    w = torch.eye(C) + 1e-3 * torch.randn(C, C, generator=g) / C ** 0.5
    w[C - 2] = 0
    w[C - 2, C - 2] = 1  # the constant channel stays constant
    conv = HipConv2d(C, C, kernel_size=1, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w.reshape(C, C, 1, 1))
    conv.weight.requires_grad_(False)
    return x, gamma, beta, conv


def _inputs(case):
    g = torch.Generator().manual_seed(N.case_seed(case.id) + 7)
    dout = torch.randn(case.M, case.C, generator=g)
    res = torch.randn(case.M, case.C, generator=g) * 2 if case.res else None
    return [_side(case, k) for k in range(2 if case.kind == "pair" else 1)], dout, res


def _run(case, sides, dout, res, train, log):
    """One forward + backward of the case's Function with gamma / beta trainable as `train` = (gamma?, beta?) says.  Everything
    on the CPU: conv outputs, device statistics, the mask, dx (bits), dres, the affine gradients."""
    from onda_amd import ops
    from onda_amd.ops import norm
    from onda_amd.ops.limbs import _stat_tile_rows
    B, H, W = case.shape
    C, M = case.C, case.M
    real = norm.call

    def spy(name, *args):
        log.append((name, args))
        return real(name, *args)

    old_fuse = ops.FUSE_BN_FINALIZE
    if case.fuse is not None:
        ops.FUSE_BN_FINALIZE = case.fuse
    norm.call = spy
    try:
        with ops.row_groups(case.first):
            ys, stats, affine = [], [], []
            for x, gamma, beta, conv in sides:
                xd = x.reshape(B, H, W, C).to(DEV).requires_grad_(True)
                y, st = conv(xd, want_stats=True if case.kind == "fp32" else 4)
                assert st.shape[1] == (2 if case.kind == "fp32" else 4)
                ys.append(y)
                stats.append(st)
                affine += [gamma.to(DEV).requires_grad_(train[0]), beta.to(DEV).requires_grad_(train[1])]
            rd = res.reshape(B, H, W, C).to(DEV).requires_grad_(True) if res is not None else None
            del log[:]
            if case.kind == "pair":
                assert ops.bn_pair_ok(ys[0], stats[0], ys[1], stats[1])
                z = ops.BNPairLimbFn.apply(ys[0], stats[0], affine[0], affine[1], None, N.MOMENTUM,
                                           ys[1], stats[1], affine[2], affine[3], None, N.MOMENTUM, case.relu)
            else:
                fn = ops.BNTrainFn if case.kind == "fp32" else ops.BNTrainLimbFn
                z = fn.apply(ys[0], stats[0], affine[0], affine[1], rd, case.relu, None, N.MOMENTUM)
            node = z.grad_fn
            wanted = ys + ([rd] if rd is not None else []) + [t for t in affine if t.requires_grad]
            grads = list(torch.autograd.grad(z, wanted, dout.reshape(B, H, W, C).to(DEV)))
            torch.cuda.synchronize()
        got = dict(y=[y.detach().cpu().reshape(M, C) for y in ys], tiles=[s.shape[0] for s in stats], log=[n for n, _ in log], args=list(log))
        got["bm"] = [_stat_tile_rows(s) for s in stats] if case.kind != "fp32" or case.first else None
        if case.kind == "fp32":
            out = z.detach().cpu().reshape(M, C)
            got["mask"] = (out > 0) if case.relu else None
            got["dx"] = [grads[0].cpu()]
        else:
            out = ops.materialize(z).cpu().reshape(M, C)
            got["mask"] = None
            if case.relu:
                bits = np.unpackbits(node.relu_mask.cpu().numpy(), bitorder="little").reshape(M, C)
                got["mask"] = torch.from_numpy(bits).bool()
            got["dx"] = [ops.limbs_of(g).planes.cpu() for g in grads[:len(ys)]]
            got["dx_amax"] = [float(ops.limbs_of(g).amax.max()) for g in grads[:len(ys)]]
        rest = grads[len(ys):]
        got["dres"] = rest.pop(0).cpu() if rd is not None else None
        got["affine"] = [rest.pop(0).cpu() if t.requires_grad else None for t in affine]
        assert not rest
        return got
    finally:
        norm.call = real
        ops.FUSE_BN_FINALIZE = old_fuse


def _expected_log(case, train):
    """The C-ABI calls of the Function, forward then backward: what the frozen Functions always made, with the backward call(s)
    that write a gradient under their affine names -- the same number of calls either way."""
    from onda_amd import ops
    aff = train[0] or train[1]
    if case.kind == "pair":
        return ["onda_bn_pair_fwd_l2", "onda_bn_pair_bwd_affine_l2" if aff else "onda_bn_pair_bwd_l2"]
    if case.kind == "limb":
        fuse = ops.FUSE_BN_FINALIZE if case.fuse is None else case.fuse
        fwd = ["onda_bn_train_l2"] if fuse else ["onda_bn_finalize_l2", "onda_bn_apply_l2"]
        return fwd + ["onda_bn_bwd_affine_l2" if aff else "onda_bn_bwd_l2"]
    if not case.first:
        return ["onda_bn_finalize", "onda_bn_apply", "onda_bn_bwd_affine" if aff else "onda_bn_bwd"]
    # two groups, the boundary inside a partial row: a statistics pass per group; the LAST group's backward call writes the sums
    return ["onda_bn_stats", "onda_bn_finalize", "onda_bn_apply"] * 2 + ["onda_bn_bwd", "onda_bn_bwd_affine" if aff else "onda_bn_bwd"]


def _check(case):
    from onda_amd import ops
    if case.kind != "fp32" and not _limb_supported():
        pytest.skip("limb rows exist in the f16x2 / dma configuration only")
    C, M, split = case.C, case.M, case.split
    sides, dout, res = _inputs(case)
    runs = {}
    for train in ((True, True), (False, False), (True, False), (False, True)):
        log = []
        runs[train] = _run(case, sides, dout, res, train, log)
        assert runs[train]["log"] == _expected_log(case, train), f"{case.id} {train}: {runs[train]['log']}"
    again = _run(case, sides, dout, res, (True, True), [])
    full, frozen = runs[(True, True)], runs[(False, False)]
    nb = len(sides)

    # ---- who asks for what changes nothing else: dx, dres bit for bit the frozen route's; a second run gives the same bits
    for train, got in list(runs.items()) + [("again", again)]:
        for i in range(nb):
            assert torch.equal(got["dx"][i], frozen["dx"][i]), f"{case.id} {train}: dx of side {i} differs from the frozen route's"
            if "dx_amax" in got:
                assert got["dx_amax"][i] == frozen["dx_amax"][i]
        if res is not None:
            assert torch.equal(got["dres"], frozen["dres"]), f"{case.id} {train}: dres differs from the frozen route's"
    assert all(t is None for t in frozen["affine"])
    for i, t in enumerate(full["affine"]):
        assert t is not None and t.shape == (C,) and torch.equal(t, again["affine"][i]), f"{case.id}: gradient {i} is not reproducible"
    # gamma only / beta only: just that one, the same bits; the pointer of the other is NULL in the call
    for train in ((True, False), (False, True)):
        got = runs[train]
        for i, t in enumerate(got["affine"]):
            if train[i % 2]:
                assert torch.equal(t, full["affine"][i]), f"{case.id} {train}: gradient {i} differs from the run that asked for both"
            else:
                assert t is None
        name, args = [(n, a) for n, a in got["args"] if "affine" in n][-1]
        ptrs = args[-5:-1] if case.kind == "pair" else args[-3:-1]
        assert [p is not None for p in ptrs] == [train[i % 2] for i in range(len(ptrs))], f"{case.id} {train}: {name} got {ptrs}"

    # ---- the restatement, from the conv outputs the device normalised and the device's own mask
    groups = [(0, split), (split, M - split)] if split else None
    mask = full["mask"]
    if case.relu:
        assert torch.equal(mask, frozen["mask"])
    if case.kind == "fp32":
        if split:
            assert split % full["bm"][0] != 0, "the case is there for the statistics pass per group"
            fwd = [N.bn_geometry(n, C) for _, n in groups]
        else:
            fwd = [(N.EPILOGUE_CHAIN, full["tiles"][0])]
        bwd = A.fp32_geometry(M, C, split)
    else:
        bwd = A.limb_geometry(M, C, split)
    refs = []
    for i, (x, gamma, beta, conv) in enumerate(sides):
        y = full["y"][i]
        assert bool((y[:, C - 2] == y[0, C - 2]).all())
        if case.kind == "pair":
            refs.append(N.bn64(y, gamma, beta, None, False, groups))
        else:
            refs.append(N.bn64(y, gamma, beta, res, case.relu, groups))
    if case.kind == "pair":
        arefs = A.pair_affine64(refs[0], refs[1], dout, mask)
    else:
        arefs = [A.affine64(refs[0], dout, mask)]
    for i in range(nb):
        if case.kind != "fp32":
            tiles, bm = full["tiles"][i], full["bm"][i]
            fwd = [(N.EPILOGUE_CHAIN, max(1, split // bm)), (N.EPILOGUE_CHAIN, tiles - split // bm)] if split else [(N.EPILOGUE_CHAIN, tiles)]
        dg, db = full["affine"][2 * i], full["affine"][2 * i + 1]
        A.check_affine(dg, db, arefs[i], refs[i], fwd, bwd, case.id, f" side {'ab'[i]}" if nb > 1 else f" {case.kind}")
    if nb > 1:
        assert torch.equal(full["affine"][1], full["affine"][3]), f"{case.id}: the pair's two dbeta differ"
    return ops


@pytest.mark.parametrize("case", LIMB_CASES, ids=ids)
def test_limb_batchnorm_affine_gradients(case, f16x2):
    p = N.col_plan(1, case.M, case.C)
    want = {32: 256, 64: 128, 2048: 32}[case.C]
    assert p.rows_per_chunk == want
    if case.M == 646:
        assert p.chunks == 3 and (not case.split or [P for _, P in A.limb_geometry(case.M, case.C, case.split)] == [2, 2])
    _check(case)


@pytest.mark.parametrize("case", PAIR_CASES, ids=ids)
def test_pair_batchnorm_affine_gradients(case, f16x2):
    _check(case)


# (row groups need the pre-split conv path: two groups exist in the "f16x2" mode only)
@pytest.mark.parametrize("case,mode", [(FP32_CASES[0], "f32"), (FP32_CASES[0], "f16x2"), (FP32_CASES[1], "f16x2")],
                         ids=lambda v: v if isinstance(v, str) else v.id)
def test_fp32_batchnorm_affine_gradients(case, mode):
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, mode
    try:
        _check(case)
    finally:
        ops.CONV_MODE = old


def test_affine_entry_points_refuse_before_they_launch(f16x2):
    """ONDA_EINVAL before anything is launched: what the frozen entry points refuse, and a previous workspace without a gradient
    to add it into."""
    from ctypes import byref
    from onda_amd import ops
    from onda_amd._lib import OndaBnSide, call
    p, s = ops._p, ops._stream()
    buf = [torch.zeros(8192, device=DEV) for _ in range(12)]
    bad = pytest.raises(RuntimeError, match="ONDA_EINVAL")
    with bad:   # C % 32
        call("onda_bn_bwd_affine_l2", p(buf[0]), None, 0, p(buf[1]), p(buf[2]), p(buf[3]), p(buf[4]), p(buf[5]), p(buf[6]), 0, p(buf[7]), None,
             p(buf[8]), 8, 48, 0, None, 0, 0, p(buf[9]), p(buf[10]), s)
    with bad:   # split == M
        call("onda_bn_bwd_affine_l2", p(buf[0]), None, 0, p(buf[1]), p(buf[2]), p(buf[3]), p(buf[4]), p(buf[5]), p(buf[6]), 0, p(buf[7]), None,
             p(buf[8]), 8, 64, 0, None, 8, 0, p(buf[9]), p(buf[10]), s)
    side = OndaBnSide(p(buf[0]), None, 0, 0, p(buf[2]), p(buf[3]), p(buf[4]), None, None, None, 0.0, p(buf[5]), None, p(buf[6]), p(buf[7]))
    with bad:   # ReLU without its mask
        call("onda_bn_pair_bwd_affine_l2", p(buf[9]), None, byref(side), byref(side), p(buf[8]), 8, 64, 1, 0, p(buf[10]), None, None, None, s)
    with bad:   # a previous group's workspace, but nowhere to write the sum
        call("onda_bn_bwd_affine", p(buf[0]), None, p(buf[1]), p(buf[2]), p(buf[3]), p(buf[4]), p(buf[6]), None, p(buf[8]), 8, 64, 0, None,
             p(buf[9]), 8, None, None, s)
    with bad:   # C % 4
        call("onda_bn_bwd_affine", p(buf[0]), None, p(buf[1]), p(buf[2]), p(buf[3]), p(buf[4]), p(buf[6]), None, p(buf[8]), 8, 6, 0, None,
             None, 0, p(buf[9]), p(buf[10]), s)
    torch.cuda.synchronize()
