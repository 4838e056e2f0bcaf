"""CPU: the float64 restatement and the comparators of tests/norm_fp64.py, validated without a GPU: the restatement equals
double-precision F.batch_norm / F.group_norm under autograd; fp32 torch passes every comparator on every case and its error is
what FLOOR records; a torch emulation of the kernels' ONE-PASS statistics (fp32 partial sums with the kernels' row geometry, a
sequential chain inside a partial, a double finalize, fp32 apply arithmetic) passes too; each comparator sees the fault it was
built for; the case tables reach the paths they are named for; and the off-centre cases cover the mean^2 / var the network's
own normalisation inputs have.  The emulation is arithmetic in torch, test scaffolding; it shares no text with the kernels."""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import norm_fp64 as N

ids = lambda c: c.id  # noqa: E731
MOM = float(torch.tensor(N.MOMENTUM, dtype=torch.float32))  # the momentum as the kernels hold it


@functools.lru_cache(maxsize=None)
def bn_inputs(case, ratio=None):
    return N.bn_case_inputs(case, ratio)


def bn_reference(case, groups=None, ratio=None):
    x, gamma, beta, res, dout, rm, rv = bn_inputs(case, ratio)
    running = (rm, rv, torch.zeros((), dtype=torch.int64)) if case.track else None
    return N.bn64(x, gamma, beta, res, case.relu, groups, running)


# ------------------------------------------------------------------------------------------------ fp32 / fp64 torch
def torch_bn(case, dtype, groups=None, ratio=None):
    """torch's batch_norm (+res, +ReLU) under autograd in `dtype`, one call per row group, on the NCHW layout torch reduces
    best ([1, C, rows, 1]: a contiguous run per channel); statistics from native_batch_norm."""
    x, gamma, beta, res, dout, rm, rv = (t.to(dtype) if t is not None else None for t in bn_inputs(case, ratio))
    groups = groups or [(0, case.M)]
    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if res is not None else None
    rm, rv = rm.clone(), rv.clone()
    outs, mean, invstd = [], [], []
    for k, (r0, n) in enumerate(groups):
        track = case.track and k == len(groups) - 1
        # (torch.batch_norm: F.batch_norm refuses one value per channel, and torch's unbiased variance of one value is 0 / 0 --
        #  there the running buffers move by the kernels' rule, the biased value)
        hand = track and n == 1
        nchw = lambda t: t.t()[None, :, :, None].contiguous()  # noqa: E731
        outs.append(torch.batch_norm(nchw(xr[r0:r0 + n]), gamma, beta, rm if track and not hand else None, rv if track and not hand else None,
                                     True, MOM, N.BN_EPS, False)[0, :, :, 0].t())
        _, m, s = torch.native_batch_norm(nchw(x[r0:r0 + n]), gamma, beta, None, None, True, N.MOMENTUM, N.BN_EPS)
        if hand:
            mom = torch.tensor(N.MOMENTUM, dtype=torch.float32).to(dtype)
            rm, rv = (1 - mom) * rm + mom * m, (1 - mom) * rv + mom * (1 / s ** 2 - N.BN_EPS)
        mean.append(m)
        invstd.append(s)
    y = torch.cat(outs, 0)
    if rr is not None:
        y = y + rr
    if case.relu:
        y = F.relu(y)
    y.backward(dout)
    return types.SimpleNamespace(out=y.detach(), dx=xr.grad, dres=rr.grad if rr is not None else None, mean=torch.stack(mean),
                                 invstd=torch.stack(invstd), rm=rm, rv=rv)


def torch_gn(case, dtype):
    xs, gammas, betas, chmul, dcat = N.gn_case_inputs(case)
    cv = lambda t: t.to(dtype).clone().requires_grad_(True)  # noqa: E731
    xr, gr, br = [cv(t.permute(0, 2, 1)) for t in xs], [cv(t) for t in gammas], [cv(t) for t in betas]  # [B, C, HW]
    outs = []
    for i in range(case.n):
        y = F.group_norm(xr[i], N.GN_GROUPS, gr[i], br[i], N.GN_EPS)
        y = F.relu(y) if case.relu else y
        outs.append(y * chmul.to(dtype)[:, :, None] if chmul is not None else y)
    cat = torch.cat(outs, 1)
    cat.backward(dcat.to(dtype).permute(0, 2, 1))
    stats = [torch.native_group_norm(t.detach().permute(0, 2, 1).contiguous().to(dtype), None, None, case.B, case.C, case.HW, N.GN_GROUPS, N.GN_EPS)[1:]
             for t in xs]
    return types.SimpleNamespace(cat=cat.detach().permute(0, 2, 1), dx=[t.grad.permute(0, 2, 1) for t in xr], dgamma=[t.grad for t in gr],
                                 dbeta=[t.grad for t in br], mean=[s[0] for s in stats], rstd=[s[1] for s in stats])


@pytest.mark.parametrize("case", N.BN_CASES, ids=ids)
def test_bn_restatement_is_double_precision_torch(case):
    t = torch_bn(case, torch.float64)
    ref = bn_reference(case)
    bw = N.bn_bwd64(ref, bn_inputs(case)[4], (t.out > 0) if case.relu else None)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))  # noqa: E731
    assert close(ref.out, t.out) and close(bw.dx, t.dx) and close(ref.mean[0], t.mean[0])
    assert float(((ref.invstd[0] - t.invstd[0]) / t.invstd[0]).abs().max()) <= 1e-12
    if case.res:
        assert torch.equal(bw.g, t.dres)
    if case.track:
        assert close(ref.rm, t.rm) and close(ref.rv, t.rv)


@pytest.mark.parametrize("case", N.GN_CASES, ids=ids)
def test_gn_restatement_is_double_precision_torch(case):
    xs, gammas, betas, chmul, dcat = N.gn_case_inputs(case)
    t = torch_gn(case, torch.float64)
    ref = N.gn64(xs, gammas, betas, chmul, case.relu)
    bw = N.gn_bwd64(ref, dcat, (t.cat > 0) if case.relu else None)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))  # noqa: E731
    assert close(ref.cat, t.cat)
    for i in range(case.n):
        assert close(bw.dx[i], t.dx[i]) and close(bw.dgamma[i], t.dgamma[i]) and close(bw.dbeta[i], t.dbeta[i])
        assert close(ref.mean[i].reshape(-1), t.mean[i].reshape(-1))


def check_bn_all(case, got, ref, geometry, bwd_geometry, where, old=None):
    """Every BatchNorm comparator on one set of results (a namespace: out, dx, dres, mean, invstd, rm, rv [, nbt])."""
    x, gamma, beta, res, dout, rm, rv = bn_inputs(case)
    N.check_bn_stats(got.mean, got.invstd, ref, geometry, where)
    exempt = N.check_bn_forward(got.out, ref, geometry, where)
    assert exempt <= N.EXEMPT_SHARE, f"{where}: {100 * exempt:.3f} % of the elements exempt from the mask check"
    bw = N.bn_bwd64(ref, dout, (got.out > 0) if case.relu else None)
    N.check_bn_backward(got.dx, bw, ref, geometry, bwd_geometry, where)
    if case.res:
        assert torch.equal(got.dres.double(), bw.g), f"{where}: dres is not g"
    if case.track:
        N.check_bn_running((got.rm, got.rv, getattr(got, "nbt", 1)), (rm, rv), ref, geometry, where)
    else:
        assert torch.equal(got.rm, rm) and torch.equal(got.rv, rv)
    return exempt


@pytest.mark.parametrize("case", N.BN_CASES, ids=ids)
def test_fp32_torch_passes_every_bn_comparator(case):
    ref = bn_reference(case)
    check_bn_all(case, torch_bn(case, torch.float32), ref, [N.bn_geometry(case.M, case.C)], [N.bn_geometry(case.M, case.C)], f"torch {case.id}")


@pytest.mark.parametrize("case", N.GN_CASES, ids=ids)
def test_fp32_torch_passes_every_gn_comparator(case):
    xs, gammas, betas, chmul, dcat = N.gn_case_inputs(case)
    t = torch_gn(case, torch.float32)
    ref = N.gn64(xs, gammas, betas, chmul, case.relu)
    geo = N.gn_geometry(case)
    exempt = N.check_gn_forward(t.cat, t.mean, t.rstd, ref, geo, f"torch {case.id}")
    assert exempt <= N.EXEMPT_SHARE
    bw = N.gn_bwd64(ref, dcat, (t.cat > 0) if case.relu else None)
    N.check_gn_backward(t.dx, t.dgamma, t.dbeta, bw, ref, geo, geo, f"torch {case.id}")


def _unit_max(err, scale, kappa):
    """The worst unit among those with kappa <= FLOOR_KAPPA (0 when there is none)."""
    r = torch.where((scale > 0) & (kappa <= N.FLOOR_KAPPA), err / scale.clamp(min=1e-300), torch.zeros_like(err))
    return float(r.max())


def test_floor_is_what_bounds_record():
    """FLOOR = fp32 torch's own error against the restatement, in units of u * the unit's scale, the worst unit of the worst case."""
    worst = {k: (0.0, "") for k in N.FLOOR}

    def note(k, v, where):
        worst[k] = max(worst[k], (v, where))

    for case in N.BN_CASES:
        x, gamma, beta, res, dout, rm, rv = bn_inputs(case)
        ref, t = bn_reference(case), torch_bn(case, torch.float32)
        bw = N.bn_bwd64(ref, dout, (t.out > 0) if case.relu else None)
        std = torch.sqrt(ref.var)
        kap = 1.0 + ref.mean ** 2 / (ref.var + ref.eps)
        note("bn_mean", _unit_max((t.mean.double() - ref.mean).abs(), N.U * (ref.mean.abs() + std), kap), case.id)
        note("bn_invstd", _unit_max((t.invstd.double() - ref.invstd).abs(), N.U * ref.invstd, kap), case.id)
        _, scale = N.bn_out_tol(ref, [(1, 1)])
        note("bn_out", _unit_max((t.out.double() - ref.out).abs().amax(0, keepdim=True), N.U * scale, kap), case.id)
        note("bn_dx", _unit_max((t.dx.double() - bw.dx).abs().amax(0, keepdim=True), N.U * bw.scale, kap), case.id)
    for case in N.GN_CASES:
        xs, gammas, betas, chmul, dcat = N.gn_case_inputs(case)
        t = torch_gn(case, torch.float32)
        ref = N.gn64(xs, gammas, betas, chmul, case.relu)
        bw = N.gn_bwd64(ref, dcat, (t.cat > 0) if case.relu else None)
        G = N.GN_GROUPS
        for i in range(case.n):
            B, HW, C = ref.xhat[i].shape
            xmax = ref.xhat[i].reshape(B, HW, G, C // G).abs().amax((1, 3))
            cm = ref.chmul.abs() if ref.chmul is not None else torch.ones(B, C, dtype=torch.float64)
            scale = (ref.gammas[i].abs() * xmax.repeat_interleave(C // G, 1) + ref.betas[i].abs()) * cm
            err = (t.cat.double()[:, :, i * C:(i + 1) * C] - ref.cat[:, :, i * C:(i + 1) * C]).abs().amax(1)
            kap = 1.0 + ref.mean[i] ** 2 / (ref.var[i] + N.GN_EPS)  # [B, G]
            kap_c = kap.repeat_interleave(C // G, 1)                # [B, C]
            note("gn_out", _unit_max(err, N.U * scale, kap_c), case.id)
            note("gn_dx", _unit_max(N._per_group((t.dx[i].double() - bw.dx[i]).abs(), G), N.U * bw.scale[i], kap), case.id)
            if case.HW == 1:  # one term per channel: torch's sum dy * x - mean * sum dy cancels by |x| / |x - mean| of that one pixel
                continue
            note("gn_dgamma", _unit_max((t.dgamma[i].double() - bw.dgamma[i]).abs(), N.U * bw.a_gx[i], kap_c.amax(0)), case.id)
            note("gn_dbeta", _unit_max((t.dbeta[i].double() - bw.dbeta[i]).abs(), N.U * bw.a_g[i], kap_c.amax(0)), case.id)
    for k, (v, where) in worst.items():
        print(f"FLOOR[{k}]: measured {v:.4f} at {where}, recorded {N.FLOOR[k]}")
    for k, (v, where) in worst.items():
        assert 0.75 * N.FLOOR[k] <= v <= 1.25 * N.FLOOR[k], f"FLOOR[{k}]: measured {v:.4f} at {where}, recorded {N.FLOOR[k]}"


# ------------------------------------------------------------------------------------------------ the one-pass emulation
def chunk_partials(a, b, rows_per_chunk, ry, drop_last=False):
    """fp32 partial sums [chunks, C] of a and b over chunks of rows: ry row lanes walk a chunk (lane t adds the rows t, t + ry, ...
    one after the other), lane 0 then adds the other lanes' sums one after the other."""
    M, C = a.shape
    chunks = -(-M // rows_per_chunk)
    steps = -(-rows_per_chunk // ry)
    out = []
    for t in (a, b):
        pad = torch.zeros(chunks * steps * ry, C, dtype=torch.float32)  # (adding a zero row is exact)
        for k in range(chunks):
            blk = t[k * rows_per_chunk:(k + 1) * rows_per_chunk]
            pad[k * steps * ry:k * steps * ry + blk.shape[0]] = blk
        pad = pad.reshape(chunks, steps, ry, C)
        lane = torch.zeros(chunks, ry, C, dtype=torch.float32)
        for s in range(steps):
            lane = lane + pad[:, s]
        acc = lane[:, 0].clone()
        for y in range(1, ry):
            acc = acc + lane[:, y]
        out.append(acc[:-1] if drop_last and chunks > 1 else acc)
    return out


def combine(parts, fp32=False):
    if not fp32:
        return parts.double().sum(0)
    acc = torch.zeros(parts.shape[1], dtype=torch.float32)
    for k in range(parts.shape[0]):
        acc = acc + parts[k]
    return acc.double()


def emulate_bn(case, groups=None, ratio=None, mutant=None):
    """The kernels' scheme in torch fp32: one-pass statistics from chunk partials, fp32 apply and backward arithmetic."""
    x, gamma, beta, res, dout, rm, rv = bn_inputs(case, ratio)
    groups = groups or [(0, case.M)]
    f32 = torch.float32
    mean, invstd = torch.empty(len(groups), case.C), torch.empty(len(groups), case.C)
    rm, rv = rm.clone(), rv.clone()
    out, dx = torch.empty_like(x), torch.empty_like(x)
    m = torch.tensor(N.MOMENTUM, dtype=f32)
    for k, (r0, n) in enumerate(groups):
        p = N.col_plan(1, n, case.C)
        xs = x[r0:r0 + n]
        s1, s2 = chunk_partials(xs, xs * xs, p.rows_per_chunk, p.ry, drop_last=mutant == "drop-last-partial")
        mu = combine(s1, mutant == "fp32-combine") / n
        var = (combine(s2, mutant == "fp32-combine") / n - mu * mu).clamp(min=0)
        mean[k], invstd[k] = mu.to(f32), (1.0 / torch.sqrt(var + N.BN_EPS)).to(f32)
        if case.track and k == len(groups) - 1:
            unb = var * n / (n - 1) if n > 1 and mutant != "biased-running-var" else var
            rm = (1 - m) * rm + m * mu.to(f32)
            rv = (1 - m) * rv + m * unb.to(f32)
    if mutant == "invstd-1e-4":
        invstd[0, low_gamma_channel(case)] *= 1 + 1e-4
    if mutant == "group0-statistics":
        mean[1], invstd[1] = mean[0], invstd[0]
    for k, (r0, n) in enumerate(groups):
        xs = x[r0:r0 + n]
        v = (xs - mean[k]) * (invstd[k] * gamma) + beta
        if res is not None and mutant != "residual-after-relu":
            v = v + res[r0:r0 + n]
        if case.relu:
            v = v.clamp(min=0)
        if res is not None and mutant == "residual-after-relu":
            v = v + res[r0:r0 + n]
        out[r0:r0 + n] = v
    g = dout * (out > 0) if case.relu else dout
    for k, (r0, n) in enumerate(groups):
        p = N.col_plan(1, n, case.C)
        xh = (x[r0:r0 + n] - mean[k]) * invstd[k]
        gs = g[r0:r0 + n]
        s1, s2 = chunk_partials(gs, gs * xh, p.rows_per_chunk, p.ry)
        inv_m = torch.tensor(1.0 / n, dtype=f32)
        a, b = combine(s1).to(f32), combine(s2).to(f32)
        dx[r0:r0 + n] = gamma * invstd[k] * (gs - a * inv_m - xh * (b * inv_m))
    return types.SimpleNamespace(out=out, dx=dx, dres=g if res is not None else None, mean=mean, invstd=invstd, rm=rm, rv=rv)


def low_gamma_channel(case):
    """The centred channel (mean / std 0) of the last 16-channel block with the smallest |gamma| (constant and small-std channels
    aside): off-centre its own bound, which grows with kappa, is above 1e-4 by design."""
    gamma, ratio = bn_inputs(case)[1], N.population(case.C, N.case_seed(case.id))[2]
    lo = max(0, case.C - 16)
    g = torch.where(ratio[lo:case.C - 2] == 0, gamma[lo:case.C - 2].abs().double(), torch.full((case.C - 2 - lo,), 1e9, dtype=torch.float64))
    assert float(g.min()) < 1e9
    return lo + int(g.argmin())


def geometries(case, groups=None):
    return [N.bn_geometry(n, case.C) for _, n in (groups or [(0, case.M)])]


@pytest.mark.parametrize("case", N.BN_CASES, ids=ids)
def test_one_pass_emulation_passes_every_bn_comparator(case):
    geo = geometries(case)
    check_bn_all(case, emulate_bn(case), bn_reference(case), geo, geo, f"emulation {case.id}")


OFF_CENTRE = [N.BN_BY_ID[i] for i in ("c64-m306", "c64-chunks66", "c2048-m306", "c24-m306")]


def test_one_pass_falls_behind_torch_off_centre():
    """The per-channel xhat error (max|xhat| * d invstd / invstd + invstd * d mean) of the one-pass emulation and of fp32 torch at
    every mean / std: what docs/experiments.md records, and the statistics bound's constants confirmed -- the emulation stays
    inside A_INVSTD * u * kappa and A_MEAN * u * (|mean| + std) WITHOUT the 4 x."""
    worst_is = worst_mu = 0.0
    for case in OFF_CENTRE:
        for ratio in (0.25, 4.0, 16.0, 64.0):
            ref = bn_reference(case, ratio=ratio)
            L, P = N.bn_geometry(case.M, case.C)
            kappa = 1.0 + ref.mean ** 2 / (ref.var + ref.eps)
            row = []
            for got in (emulate_bn(case, ratio=ratio), torch_bn(case, torch.float32, ratio=ratio)):
                d_is = (got.invstd.double() - ref.invstd).abs() / ref.invstd
                d_mu = (got.mean.double() - ref.mean).abs()
                live = slice(0, case.C - 2)  # (the constant and the small-std channel keep their own kappa)
                row.append(float((ref.xhat_amax * d_is + ref.invstd * d_mu)[0, live].max()))
                if got.out is not None and len(row) == 1:
                    worst_is = max(worst_is, float((d_is / (N.A_INVSTD(L, P) * N.U * kappa))[0, live].max()))
                    worst_mu = max(worst_mu, float((d_mu / (N.A_MEAN(L, P) * N.U * (ref.mean.abs() + torch.sqrt(ref.var))))[0, live].max()))
            print(f"{case.id} mean/std {ratio}: one-pass {row[0]:.2e}, fp32 torch {row[1]:.2e}, ratio {row[0] / row[1]:.1f}")
    print(f"emulation / (A_INVSTD u kappa) <= {worst_is:.3f}, emulation / (A_MEAN u (|mean| + std)) <= {worst_mu:.3f}")
    assert worst_is <= 1.0 and worst_mu <= 1.0


# ------------------------------------------------------------------------------------------------ teeth
def test_comparators_see_the_mutants_of_the_bn_emulation():
    tracked = N.BN_BY_ID["c2048-m306"]  # relu + residual + tracked
    geo = geometries(tracked)
    ref = bn_reference(tracked)
    for mutant in ("invstd-1e-4", "biased-running-var", "residual-after-relu"):
        assert N.flagged(check_bn_all, tracked, emulate_bn(tracked, mutant=mutant), ref, geo, geo, mutant), mutant
    # the last partial row dropped: a case with several chunks, the last one short
    many = N.BN_BY_ID["c64-chunks66"]
    assert N.col_plan(1, many.M, many.C).chunks == 66 and many.M % N.col_plan(1, many.M, many.C).rows_per_chunk == 3
    geo = geometries(many)
    assert N.flagged(check_bn_all, many, emulate_bn(many, mutant="drop-last-partial"), bn_reference(many), geo, geo, "drop")
    # the statistics of group 0 applied to group 1
    case, groups = N.BN_BY_ID["c64-m306"], [(0, 153), (153, 153)]
    x = bn_inputs(case)[0]
    ref = N.bn64(x, *bn_inputs(case)[1:4], case.relu, groups, (bn_inputs(case)[5], bn_inputs(case)[6], 0))
    geo = geometries(case, groups)
    check_bn_all(case, emulate_bn(case, groups), ref, geo, geo, "two groups")
    assert N.flagged(check_bn_all, case, emulate_bn(case, groups, mutant="group0-statistics"), ref, geo, geo, "group0")


def test_fp32_combination_of_the_partials_is_seen_at_the_largest_count():
    """The partials added in fp32 one after the other instead of in double: at the largest count (1025 partials) and the largest
    kappa of the table (mean / std 16) the statistics comparator rejects it; combined in double the same partials pass."""
    case = N.BN_BY_ID["c64-grid2"]
    x = bn_inputs(case, 16.0)[0]
    p = N.col_plan(1, case.M, case.C)
    assert p.chunks == max(N.col_plan(1, c.M, c.C).chunks for c in N.BN_CASES)
    ref = N.bn64(x, *bn_inputs(case, 16.0)[1:3])
    s1, s2 = chunk_partials(x, x * x, p.rows_per_chunk, p.ry)
    got = {}
    for fp32 in (False, True):
        mu = combine(s1, fp32) / case.M
        var = (combine(s2, fp32) / case.M - mu * mu).clamp(min=0)
        got[fp32] = (mu.float()[None], (1.0 / torch.sqrt(var + N.BN_EPS)).float()[None])
    N.check_bn_stats(*got[False], ref, geometries(case), "double combination")
    assert N.flagged(N.check_bn_stats, *got[True], ref, geometries(case), "fp32 combination")


def test_todays_global_max_norm_lets_the_low_gamma_channel_through():
    """close() of tests/test_hip_kernels.py -- max|a - b| <= rel * max|b| over the tensor -- passes the emulation whose invstd is
    off by 1e-4 in one low-gamma channel, at the tolerances test_batchnorm_train uses; the per-channel comparator does not."""
    case = N.BN_BY_ID["c2048-m306"]
    ref = bn_reference(case)
    bad = emulate_bn(case, mutant="invstd-1e-4")
    bw = N.bn_bwd64(ref, bn_inputs(case)[4], bad.out > 0)
    live = slice(0, case.C - 2)  # (today's inputs have no constant and no small-std channel: left out of the max-norm)
    for got, want, rel in ((bad.out, ref.out, 2e-5), (bad.dx, bw.dx, 1e-4)):
        assert float((got.double() - want)[:, live].abs().max()) <= rel * float(want[:, live].abs().max())
    geo = geometries(case)
    assert N.flagged(N.check_bn_stats, bad.mean, bad.invstd, ref, geo, "probe")
    assert N.flagged(N.check_bn_forward, bad.out, ref, geo, "probe") or N.flagged(N.check_bn_backward, bad.dx, bw, ref, geo, geo, "probe")


def test_gn_comparator_sees_dgamma_without_the_multiplier():
    case = N.GN_BY_ID["c256-n1-drop"]
    xs, gammas, betas, chmul, dcat = N.gn_case_inputs(case)
    t = torch_gn(case, torch.float32)
    ref = N.gn64(xs, gammas, betas, chmul, case.relu)
    bw = N.gn_bwd64(ref, dcat, None)
    geo = N.gn_geometry(case)
    N.check_gn_backward(t.dx, t.dgamma, t.dbeta, bw, ref, geo, geo, "torch")
    plain = N.gn_bwd64(N.gn64(xs, gammas, betas, None, case.relu), dcat, None)  # g without chmul
    assert N.flagged(N.check_gn_backward, t.dx, [plain.dgamma[0].float()], t.dbeta, bw, ref, geo, geo, "probe")
    # and a group normalised with its neighbour's statistics
    cat = t.cat.clone()
    cpg = case.C // N.GN_GROUPS
    cat[:, :, 3 * cpg:4 * cpg] = ((xs[0][:, :, 3 * cpg:4 * cpg].double() - ref.mean[0][:, 4][:, None, None]) * ref.rstd[0][:, 4][:, None, None]
                                  * ref.gammas[0][3 * cpg:4 * cpg] + ref.betas[0][3 * cpg:4 * cpg]).float() * chmul[:, None, 3 * cpg:4 * cpg]
    assert N.flagged(N.check_gn_forward, cat, t.mean, t.rstd, ref, geo, "probe")


def test_limb_bound_check_sees_a_bound_computed_from_the_magnitude_of_gamma():
    """The limb path bounds max|out| from the channel extrema through the per-channel MONOTONE map x -> gamma * xhat + beta.  With
    |gamma| in its place the map is wrong where gamma < 0: with a large beta of the sign that gamma * xhat reinforces at the far
    extremum, the result is no upper bound.  The correct map gives the exact maximum."""
    case = N.BN_BY_ID["c2048-m306"]
    x, gamma, beta = bn_inputs(case)[:3]
    ref = N.bn64(x, gamma, beta)
    lo, hi = ref.xhat.amin(0), ref.xhat.amax(0)
    true_max = float(ref.out.abs().max())

    def bound(gm):
        return float(torch.maximum((gm * lo + ref.beta).abs(), (gm * hi + ref.beta).abs()).max())

    N.check_limb_bound(bound(ref.gamma), true_max, 0.0, "monotone map")
    assert bound(ref.gamma) <= true_max * (1 + 1e-12)
    assert N.flagged(N.check_limb_bound, bound(ref.gamma.abs()), true_max, 0.0, "|gamma|")


# ------------------------------------------------------------------------------------------------ the case tables
def test_cases_reach_the_paths_they_are_named_for():
    by = N.BN_BY_ID
    for C, ry8 in ((4, 2048), (24, 256), (64, 128), (2048, 32)):
        p = N.col_plan(1, 306, C)
        assert p.ry * 8 == ry8 and p.cx * p.ry == 256
        ms = {c.M for c in N.BN_CASES if c.C == C}
        assert {ry8 - 1, ry8, ry8 + 1} <= ms, (C, ms)
        assert (N.col_plan(1, ry8, C).chunks, N.col_plan(1, ry8 + 1, C).chunks) == (1, 2)
    assert {c.C for c in N.BN_CASES} == {4, 24, 64, 2048} and {1, 7, 306} <= {c.M for c in N.BN_CASES}
    assert N.col_plan(1, 306, 24).cx == 8 and 24 // 4 == 6  # a quad count that is no power of two: two idle column lanes
    for cid in ("c64-chunks66", "c2048-chunks66"):
        assert N.col_plan(1, by[cid].M, by[cid].C).chunks > 64  # the finalize lanes' second trip
    big = by["c64-grid2"]
    assert big.M * big.C // 4 > 8192 * 256 and N.ew_trips(big.M * big.C // 4) == 2
    assert all(N.ew_trips(c.M * c.C // 4) == 1 for c in N.BN_CASES if c is not big)
    # option axes: every value at least twice, and all three together
    for axis in ("relu", "res", "track"):
        vals = [getattr(c, axis) for c in N.BN_CASES]
        assert vals.count(True) >= 2 and vals.count(False) >= 2
    assert any(c.relu and c.res and c.track for c in N.BN_CASES)
    # row groups: at C = 64 one onda_bn_stats partial row covers 128 rows
    on, off = N.RG_CASES[0], N.RG_CASES[1]
    assert N.col_plan(1, on.B * on.H * on.W, on.C).rows_per_chunk == 128 and (on.first * on.H * on.W) % 128 == 0
    assert (off.first * off.H * off.W) % N.col_plan(1, off.B * off.H * off.W, off.C).rows_per_chunk != 0
    # GroupNorm
    g = N.GN_CASES
    assert {c.C for c in g} == {128, 256} and {c.n for c in g} == {1, 5} and {c.B for c in g} == {1, 3}
    assert {c.HW for c in g} == {1, 153, 9 * 17 + 1} and {c.relu for c in g} == {True, False} and any(c.drop for c in g)
    assert 128 // N.GN_GROUPS == 4
    chm = N.gn_case_inputs(N.GN_BY_ID["c256-n1-drop"])[3]
    assert bool((chm == 0).any()) and bool((chm > 0).any())


def test_population_is_what_the_issue_asks_for():
    for C in (4, 24, 64, 2048):
        gamma, beta, ratio, std = N.population(C, 5)
        assert 1e-3 <= float(gamma.abs().min()) and float(gamma.abs().max()) <= 10
        assert abs(float((gamma < 0).double().mean()) - 0.25) <= 0.1
        assert set(ratio.tolist()) == set(N.RATIOS) and float(std[C - 2]) == 0 and float(std[C - 1]) == 1e-3
        assert bool((beta.abs() > 20 * gamma.abs()).any())
        x = N.bn_input(64, C, 5)[0]
        assert bool((x[:, C - 2] == x[0, C - 2]).all())


# ------------------------------------------------------------------------------------------------ kappa of the network
def network_kappa():
    """The largest mean^2 / var over the inputs of every BatchNorm (per channel) and GroupNorm (per (image, group)) of one
    train-mode forward of the CPU oracle on the synthetic pretrained-like state, at the step tests' smallest size (2 x 64 x 128):
    the source batch (student) and the target batch (teacher: the same weights at the start of adaptation)."""
    from onda_amd.synthetic import synth_batch, synth_tensor
    from oracle import model as omodel
    worst = {"bn": (0.0, ""), "gn": (0.0, "")}
    count = [0]

    class Shim:
        def __getattr__(self, name):
            return getattr(F, name)

        @staticmethod
        def batch_norm(x, *a, **k):
            xd = x.double()
            r = (xd.mean((0, 2, 3)) ** 2 / (xd.var((0, 2, 3), unbiased=False) + N.BN_EPS)).max()
            worst["bn"] = max(worst["bn"], (float(r), f"BatchNorm #{count[0]} C={x.shape[1]}"))
            count[0] += 1
            return F.batch_norm(x, *a, **k)

        @staticmethod
        def group_norm(x, groups, *a, **k):
            xd = x.double().reshape(x.shape[0], groups, -1)
            r = (xd.mean(2) ** 2 / (xd.var(2, unbiased=False) + N.GN_EPS)).max()
            worst["gn"] = max(worst["gn"], (float(r), f"GroupNorm #{count[0]}"))
            count[0] += 1
            return F.group_norm(x, groups, *a, **k)

    old, omodel.F = omodel.F, Shim()
    try:
        for seed in (100, 200):
            sd = {k: synth_tensor(k, torch.empty(shape, dtype=dt), 1, 40.0).to(dt) for k, shape, dt in omodel.state_spec()}
            with torch.no_grad():
                omodel.forward(synth_batch(2, 64, 128, seed=seed)["image"], sd, omodel.BNMode(training=True, track=False))
    finally:
        omodel.F = old
    return worst, count[0]


def test_off_centre_cases_cover_the_network():
    worst, layers = network_kappa()
    # ResNet-50: the stem, 16 bottlenecks of three and four downsample BatchNorms; the head: five ASPP GroupNorms and the
    # bottleneck's -- per forward, two forwards
    assert layers == 2 * (1 + 16 * 3 + 4 + 6) and min(v for v, _ in worst.values()) > 0, (layers, worst)
    for k, (v, where) in worst.items():
        print(f"largest mean^2 / var of a {k} input: {v:.2f} ({where}): mean / std {v ** 0.5:.2f}")
    assert max(v for v, _ in worst.values()) <= max(N.RATIOS) ** 2
