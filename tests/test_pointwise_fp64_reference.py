"""CPU: the float64 restatement and the comparators of tests/pointwise_fp64.py, validated without a GPU: the restatement equals
double-precision torch (autograd on the composed SE block, F.max_pool2d); fp32 torch passes every comparator on every case and
its error is what FLOOR records; an fp32 torch emulation of the stages with one defect at a time is rejected by the comparator of
the defect's stage and by no other; the case tables reach the paths they are named for, and no hidden unit of any case comes
near the kink unless it was planted there.  The emulation is arithmetic in torch, test scaffolding; it shares no text with the
kernels."""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import norm_fp64 as N
import pointwise_fp64 as P

ids = lambda c: c.id  # noqa: E731


@functools.lru_cache(maxsize=None)
def inputs(case):
    return P.se_case_inputs(case)


# ------------------------------------------------------------------------------------------------ torch, fp32 / fp64
def torch_se(inp, dtype):
    """The composed block under autograd in `dtype`, the pixels of a channel contiguous ([B, C, HW]: the layout torch reduces
    best); every stage's value, the intermediate gradients through retain_grad."""
    chw = lambda t: t.to(dtype).permute(0, 2, 1).contiguous()  # noqa: E731
    back = lambda t: t.detach().permute(0, 2, 1).contiguous()  # noqa: E731
    x = chw(inp.x).requires_grad_(True)
    w1, b1, w2, b2 = (t.to(dtype).clone().requires_grad_(True) for t in (inp.w1, inp.b1, inp.w2, inp.b2))
    pooled = x.mean(2)
    pre1 = F.linear(pooled, w1, b1)
    hidden = F.relu(pre1)
    s = F.linear(hidden, w2, b2)
    gate = torch.sigmoid(s)
    out = x * gate[:, :, None]
    for t in (pooled, pre1, s, gate):
        t.retain_grad()
    out.backward(chw(inp.dout))
    return types.SimpleNamespace(
        x=inp.x, w1=inp.w1, b1=inp.b1, w2=inp.w2, b2=inp.b2, dout=inp.dout, pooled=pooled.detach(), pre1=pre1.detach(),
        hidden=hidden.detach(), s=s.detach(), gate=gate.detach(), out=back(out), dgate=gate.grad, dw2=w2.grad, db2=b2.grad,
        dpre1=pre1.grad, dw1=w1.grad, db1=b1.grad, dpooled=pooled.grad / x.shape[2], dx=back(x.grad))


def torch_pool(x, dy, channels_last=False):
    """F.max_pool2d(3, 2, 1, ceil_mode=True) in x's dtype: (y, slot, dx) in NHWC."""
    B, Hi, Wi, C = x.shape
    xr = x.permute(0, 3, 1, 2)
    xr = (xr.contiguous(memory_format=torch.channels_last) if channels_last else xr.contiguous()).requires_grad_(True)
    y, idx = F.max_pool2d(xr, 3, 2, 1, ceil_mode=True, return_indices=True)
    y.backward(dy.to(x.dtype).permute(0, 3, 1, 2))
    Ho, Wo = y.shape[2:]
    hi, wi = idx // Wi, idx % Wi
    slot = (hi - (torch.arange(Ho)[:, None] * 2 - 1)) * 3 + (wi - (torch.arange(Wo)[None, :] * 2 - 1))
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()  # noqa: E731
    return P.PoolRef(nhwc(y), nhwc(slot), nhwc(xr.grad))


@pytest.mark.parametrize("case", P.SE_CASES, ids=ids)
def test_se_restatement_is_double_precision_torch(case):
    inp = inputs(case)
    ref, t = P.se_chain64(inp), torch_se(inp, torch.float64)
    for name in P.STAGES + ("pre1", "s"):
        a, b = getattr(ref, name), getattr(t, name)
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
    assert torch.equal(ref.hidden > 0, t.hidden > 0)


@pytest.mark.parametrize("nonfinite", [False, True], ids=["finite", "nonfinite"])
@pytest.mark.parametrize("case", P.POOL_CASES, ids=ids)
def test_pool_restatement_is_torch(case, nonfinite):
    """In double and in float, NCHW and channels_last: y bit for bit, the slots and dx exact."""
    x, dy = P.pool_case_inputs(case, nonfinite)
    for dtype in (torch.float64, torch.float32):
        ref = P.maxpool_scan(x.to(dtype), dy.to(dtype))
        for channels_last in (False, True):
            t = torch_pool(x.to(dtype), dy, channels_last)
            P.check_pool(t.y, t.slot, t.dx, ref, f"torch {case.id} {dtype} channels_last={channels_last}")


# ------------------------------------------------------------------------------------------------ fp32 torch, FLOOR
@pytest.mark.parametrize("case", P.SE_CASES, ids=ids)
def test_fp32_torch_passes_every_se_comparator(case):
    inp = inputs(case)
    exempt, clearance = P.check_se(torch_se(inp, torch.float32), f"torch {case.id}", inp.planted)
    assert exempt == 0, f"{case.id}: {exempt} hidden units exempt from the sign check"


@pytest.mark.parametrize("case", P.SE_CASES, ids=ids)
def test_no_unit_is_exempt_from_the_sign_check(case):
    """The reference alone: pre1 of the fp64 pooled values, rounded as the device receives them, keeps every unit that was not
    planted at least CLEARANCE bounds from the kink -- so a device whose pooled values differ by a bound or two exempts none."""
    inp = inputs(case)
    v = P.se_chain64(inp)
    v.pooled, v.hidden = v.pooled.float(), v.hidden.float()
    exempt, clearance = P.check_hidden(v, f"reference {case.id}", inp.planted)
    print(f"{case.id}: the smallest |pre1| that was not planted is {clearance:.1f} x its bound")
    assert exempt == 0 and clearance >= P.CLEARANCE, f"{case.id}: seed {case.seed} leaves |pre1| at {clearance:.1f} bounds"


def test_floor_is_what_bounds_record():
    """FLOOR = fp32 torch's own error against the restatement of each stage, fed torch's own fp32 upstream values, in units of
    u * the unit's sum of magnitudes, the worst unit of the worst case."""
    worst = {k: (0.0, "") for k in P.FLOOR}

    def note(k, err, scale, where):
        r = torch.where(scale > 0, err / scale.clamp(min=1e-300), torch.zeros_like(err))
        worst[k] = max(worst[k], (float(r.max()), where))

    for case in P.SE_CASES:
        t = torch_se(inputs(case), torch.float32)
        for name in P.STAGES:
            ref, mag, _ = P.stage64(name, t)
            if name == "hidden":
                ref = ref.clamp(min=0)
            if name == "gate":
                note("s", (t.s.double() - ref).abs(), N.U * mag, case.id)
                g = P.se_gate64(t.s)
                note("sigmoid", (t.gate.double() - g).abs(), N.U * torch.where(g >= P.TINY, g, torch.zeros_like(g)), case.id)
                continue
            note(name, (getattr(t, name).double() - ref).abs(), N.U * mag, case.id)
    for k, (v, where) in worst.items():
        print(f"FLOOR[{k}]: measured {v:.4f} at {where}, recorded {P.FLOOR[k]}")
    for k, (v, where) in worst.items():
        assert 0.75 * P.FLOOR[k] <= v <= 1.25 * P.FLOOR[k], f"FLOOR[{k}]: measured {v:.4f} at {where}, recorded {P.FLOOR[k]}"


@pytest.mark.parametrize("case", P.POOL_CASES, ids=ids)
def test_limb_comparator_takes_a_value_rounded_to_the_format(case):
    """What the limb path may do to y -- a rounding to 2^-22 of max|x| -- passes check_limbs; twice that does not."""
    x, _ = P.pool_case_inputs(case)
    y = P.maxpool_scan(x).y
    bound = float(x.abs().max())
    step = bound * N.LIMB_FLOOR
    P.check_limbs(torch.round(y / step) * step, y, bound, case.id, "pool limbs")
    assert N.flagged(P.check_limbs, y + 2 * step, y, bound, case.id, "pool limbs")


# ------------------------------------------------------------------------------------------------ teeth
def emulate_se(inp, mutant=None, dgate=None):
    """The stages in fp32 torch, each fed the stage before it, with one defect.  dgate: fed in place of the computed one."""
    f32 = torch.float32
    x, w1, b1, w2, b2, dout = inp.x, inp.w1, inp.b1, inp.w2, inp.b2, inp.dout
    B, HW, C = x.shape
    R = w1.shape[0]
    v = types.SimpleNamespace(x=x, w1=w1, b1=b1, w2=w2, b2=b2, dout=dout)
    v.pooled = (x[:, :-1] if mutant == "pooled-without-the-last-row" else x).sum(1) / HW
    bias = b1.clone()
    if mutant == "fc1-tail-without-bias":
        assert R % 4
        bias[R - R % 4:] = 0.0
    pre1 = v.pooled @ w1.t() + bias
    v.hidden = pre1.clamp(min=0)
    s = v.hidden @ w2.t() + b2
    if mutant == "s-in-fp16":
        s = s.half().float()
    v.gate = torch.sigmoid(s)
    v.out = x * v.gate[:, None, :]
    prod = dout * x
    if mutant == "dgate-from-fp16-products":
        prod = prod.half().float()
    if mutant == "dgate-first-64-chunks":
        p = N.col_plan(B, HW, C)
        assert p.chunks > 64
        prod = prod[:, :64 * p.rows_per_chunk]
    v.dgate = prod.sum(1) if dgate is None else dgate
    g = v.gate
    dpre2 = v.dgate * g * (1 - g)
    v.dw2 = dpre2.t() @ v.hidden
    v.db2 = dpre2[0].clone() if mutant == "db2-from-image-0" else dpre2.sum(0)
    mask = (pre1 >= 0) if mutant == "mask-ge" else (v.hidden > 0)
    v.dpre1 = (dpre2 @ w2) * mask
    v.dw1 = v.dpre1.t() @ v.pooled
    v.db1 = v.dpre1.sum(0)
    dp = v.dpre1 @ w1
    if mutant != "dpooled-without-1/HW":
        dp = dp * torch.tensor(1.0 / HW, dtype=f32)
    if mutant == "dpooled-of-image-0":
        dp = dp[:1].expand(B, -1).clone()
    if mutant == "dpooled-first-R*C":
        assert R * C < B * C
        dp = dp.reshape(-1).clone()
        dp[R * C:] = 0.0
        dp = dp.reshape(B, C)
    v.dpooled = dp
    v.dx = dout * g[:, None, :]
    if mutant != "dx-without-add":
        v.dx = v.dx + dp[:, None, :]
    return v


SE_MUTANTS = [
    # mutant, case, the stage whose comparator must reject it
    ("pooled-without-the-last-row", "head", "pooled"),
    ("dgate-first-64-chunks", "chunks68", "dgate"),
    ("fc1-tail-without-bias", "ragged", "hidden"),
    ("s-in-fp16", "head", "gate"),
    ("dpooled-without-1/HW", "head", "dpooled"),
    ("dpooled-of-image-0", "head", "dpooled"),
    ("dpooled-first-R*C", "wide-batch", "dpooled"),
    ("db2-from-image-0", "head", "db2"),
    ("dgate-from-fp16-products", "head", "dgate"),
    ("dx-without-add", "one-hot-dout", "dx"),
    ("dx-without-add", "kink", "dx"),
]


@pytest.mark.parametrize("case", P.SE_CASES, ids=ids)
def test_emulation_passes_every_se_comparator(case):
    inp = inputs(case)
    assert P.se_flagged(emulate_se(inp), f"emulation {case.id}", inp.planted) == set()


@pytest.mark.parametrize("mutant,cid,stage", SE_MUTANTS, ids=[f"{m}@{c}" for m, c, _ in SE_MUTANTS])
def test_comparators_see_the_mutants(mutant, cid, stage):
    """Rejected by the comparator of its stage, and by no other stage's when that stage is fed the mutant's output."""
    inp = inputs(P.SE_BY_ID[cid])
    assert P.se_flagged(emulate_se(inp, mutant), mutant, inp.planted) == {stage}


def test_comparators_see_a_mask_that_lets_the_planted_zeros_through():
    """[pre1 >= 0] for [hidden > 0].  In the kink case the image whose pre1 is planted has dgate = 0 (its x is zero), which hides
    any mask; the stage is therefore FED the other image's dgate (the comparators are stage-wise: any input will do).  The
    replaced dgate is no sum of dout * x, so its own comparator is left out; every other stage passes."""
    inp = inputs(P.SE_BY_ID["kink"])
    fed = emulate_se(inp).dgate.flip(0)
    assert bool((inp.b1 == 0).any()) and bool((fed[1] != 0).all())
    assert P.se_flagged(emulate_se(inp, None, fed), "fed", inp.planted) == {"dgate"}
    assert P.se_flagged(emulate_se(inp, "mask-ge", fed), "mask-ge", inp.planted) == {"dgate", "dpre1"}


def last_maximum(v, best):
    return (v >= best) | (v != v)


def nan_gives_way(v, best):
    return (v > best) | (v != v) | ((best != best) & (v == v))


def test_pool_comparator_sees_the_mutants():
    case = P.POOL_BY_ID["9x11"]
    for nonfinite, take in ((False, last_maximum), (True, nan_gives_way)):
        x, dy = P.pool_case_inputs(case, nonfinite)
        ref, bad = P.maxpool_scan(x, dy), P.maxpool_scan(x, dy, take=take)
        P.check_pool(ref.y, ref.slot, ref.dx, ref, "itself")
        assert N.flagged(P.check_pool, bad.y, bad.slot, bad.dx, ref, take.__name__)
        if take is last_maximum:  # another element of the tie: y differs by a sign of zero at the most, the slots and dx see it
            assert torch.equal(bad.y, ref.y) and N.flagged(P.check_pool, ref.y, None, bad.dx, ref, "dx alone")
    # a full window at the clipped edge: Ho without ceil_mode, seen by the shape
    x, dy = P.pool_case_inputs(P.POOL_BY_ID["8x9"])
    bad = P.maxpool_scan(x, None, ceil_mode=False)
    assert bad.y.shape[1] == 4 and N.flagged(P.check_pool, bad.y, None, None, P.maxpool_scan(x), "floor mode")
    # and a sign of zero
    ref = P.maxpool_scan(x, dy)
    y = ref.y.clone()
    y[ref.y == 0] = -ref.y[ref.y == 0]
    assert bool((ref.y == 0).any()) and N.flagged(P.check_pool, y, ref.slot, ref.dx, ref, "sign of zero")


def test_todays_global_max_norm_lets_a_wrong_pooled_gradient_through():
    """close() of tests/test_hip_kernels.py -- max|a - b| <= rel * max|b| over the tensor -- at test_se_block's shape, recipe and
    tolerance passes a dx whose pooled-gradient term is off by 0.4 %; the per-(image, channel) comparator of dpooled does not."""
    g = torch.Generator().manual_seed(3)
    B, C, R, H, W = 2, 1280, 80, 9, 17
    x = torch.randn(B, C, H, W, generator=g)
    w1, b1 = torch.randn(R, C, generator=g) / 30, torch.randn(R, generator=g) * 0.1
    w2, b2 = torch.randn(C, R, generator=g) / 9, torch.randn(C, generator=g) * 0.1
    gy = torch.randn(B, C, H, W, generator=g)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous()  # noqa: E731
    inp = P.SEIn(rows(x), w1, b1, w2, b2, rows(gy), None)
    ref, bad = P.se_chain64(inp), emulate_se(inp)
    assert P.se_flagged(bad, "today's recipe") == set()
    share = float((ref.dpooled.abs().max() / ref.dx.abs().max()))
    print(f"the pooled-gradient term is at most {share:.2e} of max|dx|")
    bad.dpooled = bad.dpooled * 1.004
    bad.dx = inp.dout * bad.gate[:, None, :] + bad.dpooled[:, None, :]
    assert float((bad.dx.double() - ref.dx).abs().max()) <= 1e-4 * float(ref.dx.abs().max())
    assert P.se_flagged(bad, "probe") == {"dpooled"}


# ------------------------------------------------------------------------------------------------ the case tables
def test_cases_reach_the_paths_they_are_named_for():
    by = P.SE_BY_ID
    plan = lambda c: N.col_plan(c.B, c.H * c.W, c.C)  # noqa: E731
    last = lambda c: c.H * c.W - (plan(c).chunks - 1) * plan(c).rows_per_chunk  # noqa: E731
    head = by["head"]
    assert (head.C, head.R) == (1280, 80) and (plan(head).chunks, plan(head).rows_per_chunk, last(head)) == (5, 32, 25)
    big = by["chunks68"]
    assert plan(big).chunks == 68 > 64 and last(big) == 1  # colsum_finalize_kernel: lanes 0 .. 3 take a second partial
    assert max(plan(c).chunks for c in P.SE_CASES if c is not big) <= 5
    rag = by["ragged"]
    p = plan(rag)
    assert rag.C // 4 == 72 and (p.cx, p.gridx) == (64, 2) and rag.C // 4 - p.cx == 8           # colreduce_kernel: col < C
    assert -(-rag.C // 256) == 2 and rag.C % 256 == 32                                       # se_fc2_kernel: ch >= C
    assert rag.R % 4 == 2 and -(-rag.R // 4) == 5                                            # se_fc1_kernel: r >= R
    assert (p.chunks, last(rag)) == (2, 3)
    wide = by["wide-batch"]
    p = plan(wide)
    assert wide.B > wide.R and max(wide.R, wide.B) * wide.C == wide.B * wide.C > wide.R * wide.C  # onda_se_fc_bwd's launch size
    assert wide.H * wide.W == 3 < p.ry == 32 and p.cx == 8 and p.chunks == 1
    assert all(c.B <= c.R for c in P.SE_CASES if c is not wide)
    kink = inputs(by["kink"])
    assert bool((kink.x[1] == 0).all()) and bool((kink.x[0] > 0).any()) and bool((kink.b1 <= 0).all())
    assert bool((kink.b1 == 0).any()) and bool((kink.b1 < 0).any()) and bool(kink.planted[1].all()) and not bool(kink.planted[0].any())
    t = torch_se(kink, torch.float32)
    assert bool((t.hidden[0] > 0).any())  # (image 0 is an ordinary image)
    sat = inputs(by["saturated"])
    assert tuple(sat.b2[:4].tolist()) == P.SATURATED_B2
    ones, zeros = P.check_gate(torch_se(sat, torch.float32), "saturated")
    assert ones == 2 * by["saturated"].B and zeros == by["saturated"].B  # +30 and +100 must give 1; -100 must give 0; -30 a normal number
    hot = inputs(by["one-hot-dout"])
    assert bool(((hot.dout != 0).any(2).sum(1) == 1).all())
    assert all((inputs(c).x >= 0).all() and float(inputs(c).x.mean()) > 0.3 for c in P.SE_CASES if c.id != "kink")
    # the limb kernel (C % 32 == 0) runs every case
    assert all(c.C % 32 == 0 for c in P.SE_CASES)
    # max-pool
    shapes = [(c.B, c.Hi, c.Wi, c.C) for c in P.POOL_CASES]
    assert shapes == [(3, 1, 1, 4), (2, 2, 3, 4), (2, 3, 4, 68), (2, 9, 11, 64), (1, 8, 9, 64)]
    assert 68 // 4 == 17 and [c.id for c in P.POOL_CASES if c.C % 32 == 0] == ["9x11", "8x9"]
    assert [P.pool_out_size(n) for n in (1, 2, 3, 4, 8, 9, 11)] == [1, 2, 2, 3, 5, 5, 6]
    for case in P.POOL_CASES:
        x, dy = P.pool_case_inputs(case)
        assert bool(torch.isfinite(x).all()) and bool((x < 0).any())
        assert x.numel() < 1000 or 0.2 < float((x * 2 == torch.round(x * 2)).double().mean()) < 0.3
        assert bool((dy * 4 == torch.round(dy * 4)).all()) and float(dy.abs().max()) <= 2
        xn, _ = P.pool_case_inputs(case, True)
        ref = P.maxpool_scan(xn)
        # the window of -inf keeps its first in-range element: the centre of the window, the image's first pixel
        assert float(ref.y[0, 0, 0, 0]) == float("-inf") and int(ref.slot[0, 0, 0, 0]) == 4
        assert float(ref.y[0, 0, 0, 1]) == float("inf") and bool(torch.isnan(ref.y[0, 0, 0, 2]))
        assert bool((xn[..., 1] == float("-inf")).any())
    x, _ = P.pool_case_inputs(P.POOL_BY_ID["9x11"])
    ref, lastmax = P.maxpool_scan(x), P.maxpool_scan(x, take=last_maximum)
    ties = ref.slot != lastmax.slot
    assert int(ties.sum()) >= 8 and bool(torch.signbit(ref.y[ties]).any())  # windows whose maximum is a tie, below +0.0 too
