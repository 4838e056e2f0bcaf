"""CPU: the float64 restatement and the comparators of tests/bn_affine_fp64.py (dgamma / dbeta of a train-mode BatchNorm, one or
two row groups, and of the pair), validated without a GPU: fp32 torch (F.batch_norm under autograd) passes every comparator and
its error is what FLOOR records; a torch emulation of the kernels' chunked one-pass sums (fp32 chunk partials with the kernels' row
geometry, combined in double, the groups added, one rounding) passes too; and each comparator sees the fault it was built for.
The emulation is arithmetic in torch, test scaffolding; it shares no text with the kernels."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

import bn_affine_fp64 as A
import norm_fp64 as N
from test_norm_fp64_reference import chunk_partials, combine

ids = lambda c: c.id  # noqa: E731

Case = collections.namedtuple("Case", "id C M split relu res")
# every case of norm_fp64.BN_CASES (one group), norm_fp64.RG_CASES (two), and the GPU file's row-group shapes
CASES = [Case(c.id, c.C, c.M, 0, c.relu, c.res) for c in N.BN_CASES] + \
        [Case(c.id, c.C, c.B * c.H * c.W, c.first * c.H * c.W, c.relu, c.res) for c in N.RG_CASES] + \
        [Case("c32-m234-rg", 32, 234, 117, True, True), Case("c32-m646-rg", 32, 646, 323, True, False)]
BY_ID = {c.id: c for c in CASES}


def groups_of(case):
    return [(0, case.split), (case.split, case.M - case.split)] if case.split else [(0, case.M)]


@functools.lru_cache(maxsize=None)
def inputs(case, side=0):
    """(x, gamma, beta, res, dout) f32, seeded by the case id; `side` 1: the other BatchNorm of a pair (same dout)."""
    seed = N.case_seed(case.id)
    x, gamma, beta = N.bn_input(case.M, case.C, seed + 1000 * side, shift_rows=case.split)
    g = torch.Generator().manual_seed(seed + 2)
    res = torch.randn(case.M, case.C, generator=g) * 3 if case.res else None
    dout = torch.randn(case.M, case.C, generator=g)
    return x, gamma, beta, res, dout


def reference(case, side=0):
    x, gamma, beta, res, dout = inputs(case, side)
    return N.bn64(x, gamma, beta, res, case.relu, groups_of(case))


def torch_affine(case, dtype):
    """F.batch_norm (+res, +ReLU) under autograd in `dtype`, one call per row group with the SAME gamma / beta leaves, NCHW
    [1, C, rows, 1]: (out, dgamma, dbeta)."""
    x, gamma, beta, res, dout = (t.to(dtype) if t is not None else None for t in inputs(case))
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    outs = []
    for r0, n in groups_of(case):
        nchw = x[r0:r0 + n].t()[None, :, :, None].contiguous()
        outs.append(torch.batch_norm(nchw, gr, br, None, None, True, N.MOMENTUM, N.BN_EPS, False)[0, :, :, 0].t())
    y = torch.cat(outs, 0)
    if res is not None:
        y = y + res
    if case.relu:
        y = F.relu(y)
    y.backward(dout)
    return y.detach(), gr.grad, br.grad


def emulate(case, geometry_rule="limb", side=0, mutant=None):
    """The kernels' scheme in torch: one-pass fp32 statistics (chunk partials, double finalize), fp32 forward, then per row group
    fp32 chunk partials of g and g * xhat in the route's row geometry, combined in double, the groups' doubles added in order and
    rounded to fp32 once.  Returns (out, dgamma, dbeta, mean, invstd)."""
    x, gamma, beta, res, dout = inputs(case, side)
    f32 = torch.float32
    groups = groups_of(case)
    mean, invstd = torch.empty(len(groups), case.C), torch.empty(len(groups), case.C)
    out = torch.empty_like(x)
    for k, (r0, n) in enumerate(groups):
        p = N.col_plan(1, n, case.C)
        xs = x[r0:r0 + n]
        s1, s2 = chunk_partials(xs, xs * xs, p.rows_per_chunk, p.ry)
        mu = combine(s1) / n
        var = (combine(s2) / n - mu * mu).clamp(min=0)
        mean[k], invstd[k] = mu.to(f32), (1.0 / torch.sqrt(var + N.BN_EPS)).to(f32)
        v = (xs - mean[k]) * (invstd[k] * gamma) + beta
        if res is not None:
            v = v + res[r0:r0 + n]
        out[r0:r0 + n] = v.clamp(min=0) if case.relu else v
    return (out,) + emulate_sums(case, out, mean, invstd, x, dout, geometry_rule, mutant) + (mean, invstd)


def emulate_sums(case, out, mean, invstd, x, dout, geometry_rule="limb", mutant=None, xhat_from=None):
    g = dout * (out > 0) if case.relu and mutant != "unmasked" else dout
    plan_all = N.col_plan(1, case.M, case.C)
    tot = [torch.zeros(case.C, dtype=torch.float64), torch.zeros(case.C, dtype=torch.float64)]
    for k, (r0, n) in enumerate(groups_of(case)):
        if mutant == "group1-left-out" and k == 1:
            continue
        p = plan_all if geometry_rule == "limb" else N.col_plan(1, n, case.C)
        mk, ik, xs = (mean[k], invstd[k], x[r0:r0 + n]) if xhat_from is None else (xhat_from[0][k], xhat_from[1][k], xhat_from[2][r0:r0 + n])
        xh = (xs - mk) * ik
        gs = g[r0:r0 + n]
        s1, s2 = chunk_partials(gs, gs * xh, p.rows_per_chunk, p.ry)
        tot[0] = tot[0] + combine(s1)
        tot[1] = tot[1] + combine(s2)
    return tot[1].to(torch.float32), tot[0].to(torch.float32)


def geometries(case, rule):
    fwd = [N.bn_geometry(n, case.C) for _, n in groups_of(case)]
    return fwd, (A.limb_geometry if rule == "limb" else A.fp32_geometry)(case.M, case.C, case.split)


# ------------------------------------------------------------------------------------------------ restatement and torch
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_restatement_is_double_precision_torch(case):
    out, dg, db = torch_affine(case, torch.float64)
    ref = reference(case)
    a = A.affine64(ref, inputs(case)[4], (out > 0) if case.relu else None)
    close = lambda u, v, s: float((u - v).abs().max()) <= 1e-11 * max(1.0, float(s.max()))  # noqa: E731
    assert close(a.dbeta, db, a.a_g.sum(0))
    if min(n for _, n in ref.groups) > 1:   # (one row: torch's xhat is 0 / sqrt(eps) as well, but through another expression)
        assert close(a.dgamma, dg, a.a_gx.sum(0) + a.a_g.sum(0) * 1e-3)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_fp32_torch_passes_the_comparators(case):
    out, dg, db = torch_affine(case, torch.float32)
    ref = reference(case)
    a = A.affine64(ref, inputs(case)[4], (out > 0) if case.relu else None)
    fwd, bwd = geometries(case, "fp32")
    A.check_affine(dg, db, a, ref, fwd, bwd, f"torch {case.id}")


@pytest.mark.parametrize("rule", ["limb", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_chunked_one_pass_emulation_passes_the_comparators(case, rule):
    out, dg, db, mean, invstd = emulate(case, rule)
    ref = reference(case)
    a = A.affine64(ref, inputs(case)[4], (out > 0) if case.relu else None)
    fwd, bwd = geometries(case, rule)
    A.check_affine(dg, db, a, ref, fwd, bwd, f"emulation {rule} {case.id}")


def pair_emulation(case, mutant=None):
    """out = relu(BN_a(x_a) + BN_b(x_b)): side b without ReLU or residual, side a takes it as its residual."""
    xa, ga, ba, _, dout = inputs(case, 0)
    xb, gb, bb, _, _ = inputs(case, 1)
    cb = case._replace(relu=False, res=False)
    out_b, _, _, mean_b, invstd_b = emulate(cb, "limb", side=1)
    groups = groups_of(case)
    ref_b = N.bn64(xb, gb, bb, None, False, groups)
    ref_a = N.bn64(xa, ga, ba, ref_b.out, True, groups)
    # side a with the emulated side b as its residual
    out_a0, _, _, mean_a, invstd_a = emulate(case._replace(relu=False, res=False), "limb", side=0)
    out = (out_a0 + out_b).clamp(min=0)
    ca = case._replace(relu=True)
    dg_a, db_a = emulate_sums(ca, out, mean_a, invstd_a, xa, dout)
    wrong = (mean_a, invstd_a, xa) if mutant == "dgamma_b-from-xhat_a" else None
    dg_b, db_b = emulate_sums(ca, out, mean_b, invstd_b, xb, dout, xhat_from=wrong)
    return ref_a, ref_b, out, (dg_a, db_a), (dg_b, db_b), dout


@pytest.mark.parametrize("cid", ["c64-m306", "c2048-m33", "rg-off", "c32-m646-rg"])
def test_pair_emulation_passes_the_comparators(cid):
    case = BY_ID[cid]
    ref_a, ref_b, out, got_a, got_b, dout = pair_emulation(case)
    a, b = A.pair_affine64(ref_a, ref_b, dout, out > 0)
    assert a.dbeta is not None and torch.equal(a.dbeta, b.dbeta)
    fwd, bwd = geometries(case, "limb")
    A.check_affine(got_a[0], got_a[1], a, ref_a, fwd, bwd, f"pair {cid}", " a")
    A.check_affine(got_b[0], got_b[1], b, ref_b, fwd, bwd, f"pair {cid}", " b")
    assert torch.equal(got_a[1], got_b[1])


# ------------------------------------------------------------------------------------------------ FLOOR
def test_floor_is_what_torch_is_off_by():
    """FLOOR = fp32 torch's own error against the restatement in units of u * sum|g| / u * sum|g xhat|, the worst centred channel
    (kappa <= FLOOR_KAPPA) of the worst one-group case with more than one row."""
    worst = {"dbeta": (0.0, ""), "dgamma": (0.0, "")}
    for case in CASES:
        if case.split or case.M == 1:
            continue
        out, dg, db = torch_affine(case, torch.float32)
        ref = reference(case)
        a = A.affine64(ref, inputs(case)[4], (out > 0) if case.relu else None)
        kap = (1.0 + ref.mean ** 2 / (ref.var + ref.eps))[0]
        for k, err, scale in (("dbeta", (db.double() - a.dbeta).abs(), a.a_g[0]), ("dgamma", (dg.double() - a.dgamma).abs(), a.a_gx[0])):
            r = torch.where((scale > 0) & (kap <= N.FLOOR_KAPPA), err / (A.U * scale).clamp(min=1e-300), torch.zeros_like(err))
            worst[k] = max(worst[k], (float(r.max()), case.id))
    for k, (v, where) in worst.items():
        print(f"FLOOR[{k}]: measured {v:.4f} at {where}, recorded {A.FLOOR[k]}")
    for k, (v, where) in worst.items():
        assert 0.75 * A.FLOOR[k] <= v <= 1.25 * A.FLOOR[k], f"FLOOR[{k}]: measured {v:.4f} at {where}, recorded {A.FLOOR[k]}"


# ------------------------------------------------------------------------------------------------ teeth
def test_comparator_sees_an_unmasked_gradient():
    case = BY_ID["c64-m306"]
    assert case.relu
    out, dg, db, _, _ = emulate(case, "limb", mutant="unmasked")
    ref = reference(case)
    a = A.affine64(ref, inputs(case)[4], out > 0)
    fwd, bwd = geometries(case, "limb")
    assert N.flagged(A.check_affine, None, db, a, ref, fwd, bwd, "unmasked")
    assert N.flagged(A.check_affine, dg, None, a, ref, fwd, bwd, "unmasked")


@pytest.mark.parametrize("cid", ["rg-off", "c32-m234-rg"])
def test_comparator_sees_group_1_left_out(cid):
    case = BY_ID[cid]
    out, dg, db, _, _ = emulate(case, "limb", mutant="group1-left-out")
    ref = reference(case)
    a = A.affine64(ref, inputs(case)[4], (out > 0) if case.relu else None)
    fwd, bwd = geometries(case, "limb")
    assert N.flagged(A.check_affine, None, db, a, ref, fwd, bwd, "group 1 left out")
    assert N.flagged(A.check_affine, dg, None, a, ref, fwd, bwd, "group 1 left out")


def test_comparator_sees_the_pairs_dgamma_b_taken_from_xhat_a():
    case = BY_ID["c64-m306"]
    ref_a, ref_b, out, got_a, got_b, dout = pair_emulation(case, mutant="dgamma_b-from-xhat_a")
    a, b = A.pair_affine64(ref_a, ref_b, dout, out > 0)
    fwd, bwd = geometries(case, "limb")
    A.check_affine(got_a[0], got_a[1], a, ref_a, fwd, bwd, "pair mutant", " a")   # side a is untouched
    A.check_affine(None, got_b[1], b, ref_b, fwd, bwd, "pair mutant", " b")       # dbeta does not know about xhat
    assert N.flagged(A.check_affine, got_b[0], None, b, ref_b, fwd, bwd, "pair mutant", " b")


def test_geometries_are_the_plans_of_the_code():
    """col_plan3 at the GPU file's shapes: C = 32 -> 256 rows a chunk, C = 64 -> 128, C = 2048 -> 32; a split that rounds each
    group up separately gives one chunk row more than the plan of all rows (the workspace's '+ 1 chunk row')."""
    assert N.col_plan(1, 234, 32).rows_per_chunk == 256 and A.limb_geometry(234, 32) == [(32 + 7, 1)]
    assert A.limb_geometry(234, 32, 117) == [(-(-117 // 32) + 31, 1)] * 2
    p = N.col_plan(1, 646, 32)
    assert (p.rows_per_chunk, p.chunks) == (256, 3) and [P for _, P in A.limb_geometry(646, 32, 323)] == [2, 2]
    assert N.col_plan(1, 234, 64).rows_per_chunk == 128 and N.col_plan(1, 35, 2048).rows_per_chunk == 32
