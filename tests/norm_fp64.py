"""fp64 restatement of the normalisation kernels -- train-mode BatchNorm (+residual, +ReLU, one or two row groups, running
buffers), its frozen-affine backward, and the ASPP head's GroupNorm + concat (+ per-(image, channel) multiplier, +ReLU) with its
backward -- and the comparators that hold csrc/norm.hip, csrc/norm_l2.hip and ops/norm.py to it.  A plain module like
conv_fp64.py / proto_fp64.py: tests/test_norm_fp64_reference.py runs fp32 torch and a torch emulation of the kernels' one-pass
statistics through every comparator on the CPU and measures what BOUNDS record; tests/test_norm_fp64_parity.py runs the kernels
through the same comparators on the GPU.

Restatement (all float64, plain arithmetic; no F.batch_norm / F.group_norm -- those are the independent check of the CPU file).
BatchNorm, per row group of n rows: mean, biased var, invstd = 1 / sqrt(var + eps), xhat = (x - mean) * invstd,
pre = gamma * xhat + beta (+ res), out = relu(pre) or pre; the running mean moves towards mean, the running variance towards
var * n / (n - 1) (var itself when n = 1, as bn_finalize_kernel does), by the LAST group only; num_batches_tracked + 1.
Backward (frozen affine): g = dout * mask, dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)), dres = g.  The mask is
an ARGUMENT: the tests pass [out_dev > 0] of the code under test, and `check_bn_forward` separately holds that mask to the sign
of `pre` wherever |pre| exceeds its own bound -- so a flip at the kink is neither noise in the backward check nor hidden by it.
GroupNorm: per (image, group) over HW * (C / groups) values; v = gamma * xhat + beta, out = relu(v) * chmul; backward with
g = dcat * mask * chmul: dgamma = sum g * xhat, dbeta = sum g, dx = rstd * (gamma * g - (ds + xhat * dq) / n), ds = sum gamma * g,
dq = sum gamma * g * xhat over the group.

Comparators: never one max-norm over a tensor.  Statistics per channel (per (image, group)); activations and gradients per
channel (per (image, group)): the unit's largest error against the unit's OWN bound, the worst unit reported with its index.
What the structure makes exact must be exact (zeros behind a ReLU where pre < -bound, dres == g, untouched running buffers, nbt).

BOUNDS.  u = 2^-24.  Every statistics path of the kernels is ONE pass: per-channel sums of x and x * x in fp32 partials, the
partials combined in double, var = E[x^2] - mean^2 in double.  The error of var is the error of the two sums, amplified by the
cancellation: with kappa = 1 + mean^2 / (var + eps),

    |d var| <= rho * u * (E[x^2] + 2 |mean| E|x|) <= 3 * rho * u * (var + mean^2),  so  |d invstd| / invstd <= 1.5 * rho * u * kappa,
    |d mean| <= rho * u * E|x| <= rho * u * (|mean| + std),

rho * u being the relative error of a sum against the sum of its terms' magnitudes.  rho from the summation geometry, as
conv_fp64.chain_bounds counts a chain: one partial is an fp32 chain of L dependent additions (+ 1 rounding for x * x) and its
rounding grows as sqrt(L + 1) * u at most (u * sqrt(L / 6) .. u * sqrt(L / 3) typically); P partials of about equal weight,
added exactly, average independent errors: rho = sqrt((L + 1) / P) -- except in an exactly constant channel, where every
partial repeats the same roundings and nothing averages (P = 1 there).  L read from the code:
  colreduce_kernel (onda_bn_stats, GroupNorm, both backward reductions): a thread walks rows_per_chunk / ry rows, thread ty = 0
      then adds the other ry - 1 threads' sums one after the other: L = ceil(rows_per_chunk / ry) + ry - 1, P = chunks (col_plan);
  conv epilogues (conv_common.h conv_epilogue, conv_l2.hip l2_epilogue): a lane adds its TM * E = 16 accumulators, a shuffle tree
      of 2 levels folds the lanes that hold other rows, at most 4 waves are added through LDS: L = 16 + 2 + 4 = 22, P = tile rows.
A_INVSTD(L, P) = 1.5 * rho + 1 and A_MEAN(L, P) = rho + 1 (+ 1: the result's own rounding to fp32).  On the CPU the emulation
of that scheme in test_norm_fp64_reference.py (sequential chains, the kernels' row geometry, double finalize) measured at most
0.49 of A_INVSTD * u * kappa and 0.72 of A_MEAN * u * (|mean| + std) at mean / std 0.25 .. 64 (docs/experiments.md) -- WITHOUT
the 4 x, which test_one_pass_falls_behind_torch_off_centre asserts.
The apply passes add their own arithmetic: (x - mean) * (invstd * gamma) + beta (+ res) is 4 roundings on terms bounded by the
unit's scale |gamma| * max|xhat| + |beta| (+ max|res|): C_APPLY = 4; the backward apply pass computes
gamma * invstd * (g - m1 - xhat * m2) with 3 more for xhat: C_BWD = 7, on the scale |gamma * invstd| * (max|g| + |mean g| +
max|xhat| * |mean g * xhat|), the quantity norm_l2.hip itself bounds.  The statistics terms propagate through gamma * xhat:
e_xhat = max|xhat| * t_invstd + invstd * t_mean.
FLOOR: what fp32 torch on the CPU (native_batch_norm / F.group_norm under autograd, NCHW) is off by against the restatement,
in the same units (u * the unit's scale), measured by test_floor_is_what_bounds_record over the units with kappa <= FLOOR_KAPPA
= 2 of every case of the tables below and recorded rounded up.  (Centred units only: torch applies x * a + (beta - mean * a),
which cancels by sqrt(kappa) off-centre -- everything that grows with kappa is the derived terms' business, and torch passes
the comparators there through them.)  A tolerance is 4 x the larger of FLOOR and the derived constant (the margin
conv_fp64.BOUNDS gives a block over the tensor), plus the propagated statistics terms -- never tuned to what a kernel achieves.
Limb outputs (norm_l2.hip) add the format's absolute floor, tensor-wide: 2^-22 of the tensor's scale bound (the figure
test_maxpool_ceil relies on); a channel far below the tensor's maximum is not held to a relative figure it cannot meet by design.
"""
import collections
import math

import torch

U = 2.0 ** -24
BN_EPS = 1e-5
GN_EPS = 1e-5
GN_GROUPS = 32
MOMENTUM = 0.1
LIMB_FLOOR = 2.0 ** -22
EXEMPT_SHARE = 1e-3
MARGIN = 4.0
C_APPLY = 4.0
C_BWD = 7.0
EPILOGUE_CHAIN = 16 + 2 + 4
FLOOR_KAPPA = 2.0

# fp32 torch on the CPU against the restatement, in units of u * the unit's scale (see the module docstring), the worst unit of
# the worst case; measured by tests/test_norm_fp64_reference.py::test_floor_is_what_bounds_record, which holds
# measured / recorded to [0.75, 1.25].  Recorded: the measured figure rounded up.
FLOOR = {
    "bn_mean": 0.42,      # |d mean| / (u * (|mean| + std))
    "bn_invstd": 1.6,    # |d invstd| / (u * invstd)          (torch's statistics are two-pass: no kappa in its error)
    "bn_out": 2.6,        # per channel, / (u * (|gamma| max|xhat| + |beta| + max|res|))
    "bn_dx": 3.4,         # per channel, / (u * |gamma invstd| (max|g| + |mean g| + max|xhat| |mean g xhat|))
    "gn_out": 2.9,        # per (image, group)
    "gn_dx": 2.8,         # per (image, group)
    "gn_dgamma": 29.0,    # per channel, / (u * sum |g xhat|); HW > 1 (torch forms sum dy * x - mean * sum dy, which cancels)
    "gn_dbeta": 1.4,      # per channel, / (u * sum |g|)
}

MEASURED = {}  # what -> (worst ratio to its bound, where): filled by the comparators, printed by the tests


def _note(what, ratio, where):
    if ratio >= MEASURED.get(what, (-1.0, ""))[0]:
        MEASURED[what] = (ratio, where)


def flagged(check, *args, **kw):
    """Does the comparator reject these values?"""
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------ the plans, restated
Plan = collections.namedtuple("Plan", "cx ry gridx chunks rows_per_chunk")


def col_plan(B, HW, C):
    """csrc/norm.hip col_plan (csrc/norm_l2.hip col_plan3 is the same rule with B = 1): a 256-thread workgroup covers cx column
    quads x ry row lanes, cx the power of two >= C / 4 capped at 64; about 2048 workgroups in all, at least 8 rows a thread."""
    c4 = C // 4
    cx = 1
    while cx < c4 and cx < 64:
        cx *= 2
    ry = 256 // cx
    gridx = -(-c4 // cx)
    target = max(1, 2048 // (B * gridx))
    rpc = max(-(-HW // target), ry * 8)
    return Plan(cx, ry, gridx, -(-HW // rpc), rpc)


def colreduce_geometry(B, HW, C):
    """(L, P) of colreduce_kernel for one image's HW rows."""
    p = col_plan(B, HW, C)
    return -(-min(p.rows_per_chunk, HW) // p.ry) + p.ry - 1, p.chunks


def ew_trips(total, cap=8192):
    """Trips of an element-wise kernel's grid-stride loop over `total` 16- (norm.hip, cap 8192) or 32-byte (norm_l2.hip, cap
    4096) items."""
    grid = min(max(-(-total // 256), 1), cap)
    return -(-total // (grid * 256))


def A_INVSTD(L, P):
    return 1.5 * math.sqrt((L + 1) / P) + 1.0


def A_MEAN(L, P):
    return math.sqrt((L + 1) / P) + 1.0


# ------------------------------------------------------------------------------------------------ BatchNorm: restatement
BNRef = collections.namedtuple("BNRef", "groups mean var invstd xhat xhat_amax pre out rm rv nbt gamma beta res_amax relu eps")


def bn64(x, gamma, beta, res=None, relu=False, groups=None, running=None, momentum=MOMENTUM, eps=BN_EPS):
    """x [M, C] (any float dtype; widened).  groups: [(first row, rows)], default one group.  running = (rm, rv, nbt) or None."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    M, C = x.shape
    groups = groups or [(0, M)]
    mean, var = torch.empty(len(groups), C, dtype=torch.float64), torch.empty(len(groups), C, dtype=torch.float64)
    xhat = torch.empty_like(x)
    for g, (r0, n) in enumerate(groups):
        xs = x[r0:r0 + n]
        mean[g] = xs.sum(0) / n
        var[g] = ((xs - mean[g]) ** 2).sum(0) / n
        xhat[r0:r0 + n] = (xs - mean[g]) / torch.sqrt(var[g] + eps)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat_amax = torch.stack([xhat[r0:r0 + n].abs().amax(0) for r0, n in groups])
    pre = gamma * xhat + beta
    res_amax = torch.zeros(C, dtype=torch.float64)
    if res is not None:
        pre = pre + res.double()
        res_amax = res.double().abs().amax(0)
    out = pre.clamp(min=0) if relu else pre
    rm = rv = nbt = None
    if running is not None:
        m = float(torch.tensor(momentum, dtype=torch.float32))  # the kernels hold the momentum as a float
        n = groups[-1][1]
        rm = (1.0 - m) * running[0].double() + m * mean[-1]
        rv = (1.0 - m) * running[1].double() + m * (var[-1] * n / (n - 1) if n > 1 else var[-1])
        nbt = int(running[2]) + 1
    return BNRef(groups, mean, var, invstd, xhat, xhat_amax, pre, out, rm, rv, nbt, gamma, beta, res_amax, relu, eps)


BNBwdRef = collections.namedtuple("BNBwdRef", "g dx gmax m1 m2 a1 a2 scale")


def bn_bwd64(ref, dout, mask=None):
    """mask: [out > 0] of the code under test ([M, C] bool), or None without a ReLU."""
    g = dout.double() * (mask.double() if mask is not None else 1.0)
    dx = torch.empty_like(g)
    G, C = ref.mean.shape
    gmax, m1, m2, a1, a2 = (torch.empty(G, C, dtype=torch.float64) for _ in range(5))
    for k, (r0, n) in enumerate(ref.groups):
        gs, xh = g[r0:r0 + n], ref.xhat[r0:r0 + n]
        m1[k], m2[k] = gs.sum(0) / n, (gs * xh).sum(0) / n
        a1[k], a2[k] = gs.abs().sum(0) / n, (gs * xh).abs().sum(0) / n
        gmax[k] = gs.abs().amax(0)
        dx[r0:r0 + n] = ref.gamma * ref.invstd[k] * (gs - m1[k] - xh * m2[k])
    scale = (ref.gamma * ref.invstd).abs() * (gmax + m1.abs() + ref.xhat_amax * m2.abs())
    return BNBwdRef(g, dx, gmax, m1, m2, a1, a2, scale)


# ------------------------------------------------------------------------------------------------ BatchNorm: tolerances
def bn_stat_tol(ref, geometry):
    """(t_invstd relative, t_mean absolute, e_xhat absolute), each [G, C].  geometry: [(L, P)] per row group."""
    kappa = 1.0 + ref.mean ** 2 / (ref.var + ref.eps)
    std = torch.sqrt(ref.var)
    t_is, t_mu = torch.empty_like(kappa), torch.empty_like(kappa)
    for g, (L, P) in enumerate(geometry):
        # an exactly constant channel repeats the same roundings in every partial: nothing averages, P = 1
        a_is = torch.where(ref.var[g] > 0, A_INVSTD(L, P), A_INVSTD(L, 1))
        a_mu = torch.where(ref.var[g] > 0, A_MEAN(L, P), A_MEAN(L, 1))
        t_is[g] = MARGIN * torch.clamp(a_is * kappa[g], min=FLOOR["bn_invstd"]) * U
        t_mu[g] = MARGIN * torch.clamp(a_mu, min=FLOOR["bn_mean"]) * U * (ref.mean[g].abs() + std[g])
    return t_is, t_mu, ref.xhat_amax * t_is + ref.invstd * t_mu


def _rows(groups, per_group):
    """[G, C] -> [M, C]: every row takes its group's values."""
    return torch.cat([per_group[g].expand(n, -1) for g, (r0, n) in enumerate(groups)], 0)


def bn_out_tol(ref, geometry, limb_bound=None):
    """[G, C]: the bound of |out - ref| for a channel's elements in a row group."""
    _, _, e_xhat = bn_stat_tol(ref, geometry)
    scale = ref.gamma.abs() * ref.xhat_amax + ref.beta.abs() + ref.res_amax
    tol = MARGIN * max(C_APPLY, FLOOR["bn_out"]) * U * scale + ref.gamma.abs() * e_xhat
    if limb_bound is not None:
        tol = tol + LIMB_FLOOR * limb_bound
    return tol, scale


def _hold(what, err, tol, where):
    """err, tol [units...]: every unit's error within its bound (a unit whose bound is 0 must be exact); notes the worst ratio."""
    err, tol = err.double(), tol.double().expand_as(err)
    ratio = torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ratio.shape)) if ratio.dim() else ()
    r = float(ratio.reshape(-1)[worst])
    _note(what, r, f"{where} unit {idx}")
    assert r <= 1.0, f"{where}: {what} unit {idx}: error {float(err.reshape(-1)[worst]):.3e} is {r:.2f} x its bound {float(tol.reshape(-1)[worst]):.3e}"
    return r


def check_bn_stats(mean, invstd, ref, geometry, where, xhat_amax=None):
    """mean, invstd (and the limb path's xhat_amax) [G, C] of the code under test, per channel."""
    t_is, t_mu, e_xhat = bn_stat_tol(ref, geometry)
    G, C = ref.mean.shape
    _hold("bn mean", (mean.double().reshape(G, C) - ref.mean).abs(), t_mu, where)
    _hold("bn invstd", (invstd.double().reshape(G, C) - ref.invstd).abs() / ref.invstd, t_is, where)
    if xhat_amax is not None:
        # The device takes it from the conv epilogue's tile extrema (the last tile's from its live rows of y: a tile's rows
        # past M count as zeros in the table).  One group: max|xhat| itself.  Two groups: the straddling tile is counted whole
        # with group 1, so there it is an upper bound only.
        d = xhat_amax.double().reshape(G, C) - ref.xhat_amax
        tol = e_xhat + MARGIN * U * ref.xhat_amax
        _hold("bn xhat_amax", (-d).clamp(min=0) if G > 1 else d.abs(), tol, where)


def check_bn_running(new, old, ref, geometry, where, momentum=MOMENTUM):
    """The running buffers as the change they make: (new - (1 - m) * old) / m against mean and the unbiased variance of the last
    row group, per channel; nbt exact.  old = the buffers before the call."""
    m = float(torch.tensor(momentum, dtype=torch.float32))
    t_is, t_mu, _ = bn_stat_tol(ref, geometry)
    n = ref.groups[-1][1]
    unb = ref.var[-1] * n / (n - 1) if n > 1 else ref.var[-1]
    fac = n / (n - 1) if n > 1 else 1.0
    for what, k, target, tol in (("running mean", 0, ref.mean[-1], t_mu[-1]), ("running var", 1, unb, 2.0 * t_is[-1] * (ref.var[-1] + ref.eps) * fac)):
        change = (new[k].double().cpu() - (1.0 - m) * old[k].double()) / m
        # the update itself: (1 - m) * old + m * v in fp32 is 3 roundings on |(1 - m) old| + |m v|, and (float)v one more
        upd = MARGIN * U * ((1.0 - m) * old[k].double().abs() + m * target.abs()) / m + U * target.abs()
        _hold(what, (change - target).abs(), tol + upd, where)
    assert int(new[2]) == ref.nbt, f"{where}: num_batches_tracked {int(new[2])}, expected {ref.nbt}"


def check_bn_forward(out, ref, geometry, where, limb_bound=None):
    """out [M, C] of the code under test (limb outputs materialised).  Per (group, channel): the largest error against the unit's
    bound; behind a ReLU, exact zeros where pre < -bound and the mask [out > 0] equal to [pre > 0] wherever |pre| > bound.
    Returns the share of elements exempt from the mask check."""
    out = out.double()
    tol, _ = bn_out_tol(ref, geometry, limb_bound)
    err = (out - ref.out).abs()
    _hold("bn out", torch.stack([err[r0:r0 + n].amax(0) for r0, n in ref.groups]), tol, where)
    if not ref.relu:
        return 0.0
    t = _rows(ref.groups, tol)
    clear = ref.pre.abs() > t
    wrong = clear & ((out > 0) != (ref.pre > 0))
    assert not bool(wrong.any()), f"{where}: {int(wrong.sum())} ReLU mask bits wrong away from the kink, first at {wrong.nonzero()[0].tolist()}"
    below = ref.pre < -t
    assert bool((out[below] == 0).all()), f"{where}: non-zero output behind the ReLU"
    return 1.0 - float(clear.double().mean())


def bn_dx_tol(ref, bw, geometry, bwd_geometry, limb_bound=None):
    t_is, _, e_xhat = bn_stat_tol(ref, geometry)
    gi = (ref.gamma * ref.invstd).abs()
    tol = MARGIN * max(C_BWD, FLOOR["bn_dx"]) * U * bw.scale + bw.scale * t_is + 2.0 * gi * e_xhat * ref.xhat_amax * bw.gmax
    for g, (L, P) in enumerate(bwd_geometry):
        tol[g] = tol[g] + MARGIN * A_MEAN(L, P) * U * gi[g] * (bw.a1[g] + ref.xhat_amax[g] * bw.a2[g])
    if limb_bound is not None:
        tol = tol + LIMB_FLOOR * limb_bound
    return tol


def check_bn_backward(dx, bw, ref, geometry, bwd_geometry, where, limb_bound=None):
    err = (dx.double() - bw.dx).abs()
    tol = bn_dx_tol(ref, bw, geometry, bwd_geometry, limb_bound)
    _hold("bn dx", torch.stack([err[r0:r0 + n].amax(0) for r0, n in ref.groups]), tol, where)


def check_limb_bound(bound, true_max, res_max, where):
    """The limb scale bound, two-sided: an upper bound, and at most 2 x (the true maximum + max|res|)."""
    assert true_max <= bound * (1 + 1e-6), f"{where}: the limb bound {bound:.6e} is below the true maximum {true_max:.6e}"
    assert bound <= 2.0 * (true_max + res_max) + 1e-30, f"{where}: the limb bound {bound:.6e} is more than twice {true_max:.6e} + {res_max:.6e}"


# ------------------------------------------------------------------------------------------------ BatchNorm: cases
def population(C, seed):
    """Per-channel (gamma, beta, mean/std ratio, std, constant channel, small-std channel).  gamma log-uniform in [1e-3, 10], every
    fourth channel negative; beta N(0, 1), every 16th channel (from channel 1) |beta| = 50 (>> |gamma| for most); mean / std from
    {0, 4, 16}; the last but one channel exactly constant, the last with std 1e-3."""
    g = torch.Generator().manual_seed(seed)
    gamma = 10.0 ** (torch.rand(C, generator=g, dtype=torch.float64) * 4 - 3)
    gamma[1::4] *= -1
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    beta[1::16] = 50.0 * torch.sign(beta[1::16])
    ratio = torch.tensor(RATIOS, dtype=torch.float64)[torch.randint(0, len(RATIOS), (C,), generator=g)]
    ratio[:len(RATIOS)] = torch.tensor(RATIOS, dtype=torch.float64)[:C]  # every ratio occurs, at any C
    std = 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
    std[C - 1] = 1e-3
    std[C - 2] = 0.0
    return gamma.float(), beta.float(), ratio, std


RATIOS = (0.0, 4.0, 16.0)
CONSTANT = 3.3


def bn_input(M, C, seed, ratio=None, shift_rows=0):
    """x [M, C] f32: channel c is std_c * (randn + ratio_c); the constant channel is CONSTANT.  shift_rows: the rows from there on
    are scaled by 1.7 and moved by 0.4 std (the second row group has visibly different statistics)."""
    gamma, beta, r, std = population(C, seed)
    if ratio is not None:
        r = torch.full_like(r, ratio)
    g = torch.Generator().manual_seed(seed + 1)
    z = torch.randn(M, C, generator=g)
    if shift_rows:
        z[shift_rows:] = z[shift_rows:] * 1.7 + 0.4
    x = (z.double() + r) * std
    x[:, C - 2] = CONSTANT
    return x.float(), gamma, beta


BNCase = collections.namedtuple("BNCase", "id C M relu res track")

_b = BNCase
# C = 4 / 24 / 64 / 2048: ry * 8 = 2048 / 256 / 128 / 32 rows a chunk at the least (col_plan)
BN_CASES = [
    _b("c4-m1", 4, 1, False, False, True), _b("c4-m7", 4, 7, True, True, True),
    _b("c4-m2047", 4, 2047, True, False, False), _b("c4-m2048", 4, 2048, False, True, False), _b("c4-m2049", 4, 2049, True, True, True),
    _b("c24-m255", 24, 255, False, False, True), _b("c24-m256", 24, 256, True, True, False), _b("c24-m257", 24, 257, True, False, True),
    _b("c24-m306", 24, 306, False, True, True),
    _b("c64-m1", 64, 1, True, False, True), _b("c64-m127", 64, 127, True, True, True), _b("c64-m128", 64, 128, False, False, False),
    _b("c64-m129", 64, 129, True, False, True), _b("c64-m306", 64, 306, True, True, True),
    _b("c64-chunks66", 64, 128 * 65 + 3, False, True, False),        # finalize lanes take a second trip over the chunks
    _b("c64-grid2", 64, 131075, True, False, True),                  # > 8192 x 256 quads: second trip of the element-wise grids
    _b("c2048-m1", 2048, 1, False, True, False), _b("c2048-m7", 2048, 7, True, False, True),
    _b("c2048-m31", 2048, 31, True, True, False), _b("c2048-m32", 2048, 32, False, False, True), _b("c2048-m33", 2048, 33, True, True, True),
    _b("c2048-m306", 2048, 306, True, True, True), _b("c2048-chunks66", 2048, 32 * 65 + 1, True, False, True),
]
BN_BY_ID = {c.id: c for c in BN_CASES}
# row groups on the fp32 path (ops.row_groups around BNTrainFn): B images of H x W pixels, the first `first` are group 0.
# "on": the boundary falls between two partial rows (128 rows each at C = 64), "off": inside one -- a reduction pass per group
RGCase = collections.namedtuple("RGCase", "id C B H W first relu res")
RG_CASES = [RGCase("rg-on", 64, 3, 8, 16, 1, True, True), RGCase("rg-off", 64, 3, 9, 17, 1, True, False),
            RGCase("rg-off-c24", 24, 4, 9, 17, 2, False, True)]


def case_seed(cid):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(cid)) % 100003


def bn_case_inputs(case, ratio=None):
    """(x, gamma, beta, res, dout, rm, rv) f32 of a BN case, seeded by its id."""
    seed = case_seed(case.id)
    x, gamma, beta = bn_input(case.M, case.C, seed, ratio)
    g = torch.Generator().manual_seed(seed + 2)
    res = torch.randn(case.M, case.C, generator=g) * 3 if case.res else None
    dout = torch.randn(case.M, case.C, generator=g)
    rm, rv = torch.randn(case.C, generator=g) * 0.1, torch.rand(case.C, generator=g) + 0.5
    return x, gamma, beta, res, dout, rm, rv


def bn_geometry(rows, C):
    """(L, P) of onda_bn_stats / the backward reduction over `rows` rows."""
    return colreduce_geometry(1, rows, C)


# ------------------------------------------------------------------------------------------------ GroupNorm
GNRef = collections.namedtuple("GNRef", "cat mean var rstd xhat v gammas betas chmul relu n")


def gn64(xs, gammas, betas, chmul=None, relu=False, groups=GN_GROUPS, eps=GN_EPS):
    """xs: n tensors [B, HW, C]; chmul [B, C] or None.  cat [B, HW, n * C]; mean / var / rstd [n, B, groups]."""
    n = len(xs)
    B, HW, C = xs[0].shape
    cpg = C // groups
    mean, var = torch.empty(n, B, groups, dtype=torch.float64), torch.empty(n, B, groups, dtype=torch.float64)
    xhat, v = [], []
    for i in range(n):
        x = xs[i].double().reshape(B, HW, groups, cpg)
        mean[i] = x.sum((1, 3)) / (HW * cpg)
        var[i] = ((x - mean[i][:, None, :, None]) ** 2).sum((1, 3)) / (HW * cpg)
        xh = ((x - mean[i][:, None, :, None]) / torch.sqrt(var[i] + eps)[:, None, :, None]).reshape(B, HW, C)
        xhat.append(xh)
        v.append(xh * gammas[i].double() + betas[i].double())
    rstd = 1.0 / torch.sqrt(var + eps)
    outs = [(t.clamp(min=0) if relu else t) * (chmul.double()[:, None, :] if chmul is not None else 1.0) for t in v]
    return GNRef(torch.cat(outs, 2), mean, var, rstd, xhat, v, [t.double() for t in gammas], [t.double() for t in betas],
                 chmul.double() if chmul is not None else None, relu, n)


GNBwdRef = collections.namedtuple("GNBwdRef", "g dx dgamma dbeta scale a_gx a_g")


def gn_bwd64(ref, dcat, mask=None, groups=GN_GROUPS):
    """mask: [cat > 0] of the code under test [B, HW, n * C], or None without a ReLU."""
    B, HW, C = ref.xhat[0].shape
    cpg = C // groups
    cnt = HW * cpg
    gs, dxs, dgs, dbs, scales, agx, ag = [], [], [], [], [], [], []
    for i in range(ref.n):
        g = dcat.double()[:, :, i * C:(i + 1) * C]
        if mask is not None:
            g = g * mask[:, :, i * C:(i + 1) * C].double()
        if ref.chmul is not None:
            g = g * ref.chmul[:, None, :]
        xh, gam = ref.xhat[i], ref.gammas[i]
        dgs.append((g * xh).sum((0, 1)))
        dbs.append(g.sum((0, 1)))
        agx.append((g * xh).abs().sum((0, 1)))
        ag.append(g.abs().sum((0, 1)))
        gg = (gam * g).reshape(B, HW, groups, cpg)
        ds, dq = gg.sum((1, 3)), (gg * xh.reshape(B, HW, groups, cpg)).sum((1, 3))
        ads, adq = gg.abs().sum((1, 3)), (gg * xh.reshape(B, HW, groups, cpg)).abs().sum((1, 3))
        rs = ref.rstd[i]
        dx = rs[:, None, :, None] * (gg - (ds[:, None, :, None] + xh.reshape(B, HW, groups, cpg) * dq[:, None, :, None]) / cnt)
        xmax = xh.reshape(B, HW, groups, cpg).abs().amax((1, 3))
        scales.append(rs * (gg.abs().amax((1, 3)) + ads / cnt + xmax * adq / cnt))
        gs.append(g)
        dxs.append(dx.reshape(B, HW, C))
    return GNBwdRef(gs, dxs, dgs, dbs, scales, agx, ag)


def gn_stat_tol(ref, i, geometry, eps=GN_EPS):
    """(t_rstd relative, t_mean, e_xhat) [B, groups] of tensor i.  geometry (L, P): P counts the chunk partials of ONE channel;
    a group's sums average cpg channels' partials on top, which the bound does not claim."""
    L, P = geometry
    kappa = 1.0 + ref.mean[i] ** 2 / (ref.var[i] + eps)
    t_rs = MARGIN * torch.clamp(A_INVSTD(L, P) * kappa, min=FLOOR["bn_invstd"]) * U
    t_mu = MARGIN * max(A_MEAN(L, P), FLOOR["bn_mean"]) * U * (ref.mean[i].abs() + torch.sqrt(ref.var[i]))
    B, HW, C = ref.xhat[i].shape
    G = ref.mean.shape[2]
    xmax = ref.xhat[i].reshape(B, HW, G, C // G).abs().amax((1, 3))
    return t_rs, t_mu, xmax * t_rs + ref.rstd[i] * t_mu, xmax


def _per_group(t, G):
    """[B, HW, C] -> [B, G]: the largest value of each (image, group)."""
    B, HW, C = t.shape
    return t.reshape(B, HW, G, C // G).amax((1, 3))


def check_gn_forward(cat, mean, rstd, ref, geometry, where):
    """cat [B, HW, n * C], mean / rstd: n tensors [B * groups] of the code under test."""
    cat = cat.double()
    G = ref.mean.shape[2]
    exempt = 0.0
    for i in range(ref.n):
        B, HW, C = ref.xhat[i].shape
        t_rs, t_mu, e_xhat, xmax = gn_stat_tol(ref, i, geometry)
        _hold("gn mean", (mean[i].double().reshape(B, G) - ref.mean[i]).abs(), t_mu, f"{where}[{i}]")
        _hold("gn rstd", (rstd[i].double().reshape(B, G) - ref.rstd[i]).abs() / ref.rstd[i], t_rs, f"{where}[{i}]")
        gam, bet = ref.gammas[i].abs().reshape(G, C // G), ref.betas[i].abs().reshape(G, C // G)
        cm = ref.chmul.abs().reshape(B, G, C // G) if ref.chmul is not None else torch.ones(B, G, C // G, dtype=torch.float64)
        # per (image, group, channel) bound; the unit reported is the (image, group)
        scale = (gam[None] * xmax[:, :, None] + bet[None]) * cm
        tol_c = (MARGIN * max(C_APPLY + 1, FLOOR["gn_out"]) * U * scale + gam[None] * e_xhat[:, :, None] * cm).reshape(B, C)
        err = (cat[:, :, i * C:(i + 1) * C] - ref.cat[:, :, i * C:(i + 1) * C]).abs()
        emax = err.amax(1)
        ratio_c = torch.where(tol_c > 0, emax / tol_c.clamp(min=1e-300), torch.where(emax > 0, torch.full_like(emax, float("inf")), torch.zeros_like(emax)))
        _hold("gn out", ratio_c.reshape(B, G, C // G).amax(2), torch.ones(B, G, dtype=torch.float64), f"{where}[{i}]")
        if ref.relu:
            t = tol_c[:, None, :] / cm.reshape(B, 1, C).clamp(min=1e-300)
            live = (cm.reshape(B, 1, C) > 0).expand(B, HW, C)
            clear = (ref.v[i].abs() > t) & live
            got = cat[:, :, i * C:(i + 1) * C] > 0
            wrong = clear & (got != (ref.v[i] > 0))
            assert not bool(wrong.any()), f"{where}[{i}]: {int(wrong.sum())} ReLU mask bits wrong away from the kink"
            assert bool((cat[:, :, i * C:(i + 1) * C][(ref.v[i] < -t) | ~live] == 0).all()), f"{where}[{i}]: non-zero output behind the ReLU / a zero multiplier"
            exempt = max(exempt, 1.0 - float((clear | ~live).double().mean()))
    return exempt


def check_gn_backward(dxs, dgammas, dbetas, bw, ref, geometry, bwd_geometry, where):
    G = ref.mean.shape[2]
    Lb, Pb = bwd_geometry
    for i in range(ref.n):
        B, HW, C = ref.xhat[i].shape
        cpg = C // G
        t_rs, t_mu, e_xhat, xmax = gn_stat_tol(ref, i, geometry)
        gam = ref.gammas[i].abs()
        gmax = _per_group((gam * bw.g[i]).abs(), G)
        # the group sums ds / dq are fp32 chains over cpg channel sums (gn_bwd_group_kernel), each an fp32 figure itself
        tol = (MARGIN * max(C_BWD + cpg, FLOOR["gn_dx"]) * U * bw.scale[i] + bw.scale[i] * t_rs
               + 2.0 * ref.rstd[i] * e_xhat * xmax * gmax + MARGIN * A_MEAN(Lb, Pb) * U * bw.scale[i])
        _hold("gn dx", _per_group((dxs[i].double() - bw.dx[i]).abs(), G), tol, f"{where}[{i}]")
        # dgamma / dbeta per channel: B image sums added in fp32 (B roundings), each a chain of the backward geometry
        e_c = e_xhat.amax(0).repeat_interleave(cpg)  # the worst image's statistics error of the channel's group
        tol_g = MARGIN * max(A_MEAN(Lb, Pb) + B, FLOOR["gn_dgamma"]) * U * bw.a_gx[i] + bw.a_g[i] * e_c
        tol_b = MARGIN * max(A_MEAN(Lb, Pb) + B, FLOOR["gn_dbeta"]) * U * bw.a_g[i]
        _hold("gn dgamma", (dgammas[i].double() - bw.dgamma[i]).abs(), tol_g, f"{where}[{i}]")
        _hold("gn dbeta", (dbetas[i].double() - bw.dbeta[i]).abs(), tol_b, f"{where}[{i}]")


GNCase = collections.namedtuple("GNCase", "id C n B HW relu drop")
GN_CASES = [
    GNCase("c256-n5-b3", 256, 5, 3, 153, True, False),
    GNCase("c256-n1-drop", 256, 1, 1, 154, False, True),
    GNCase("c128-n1-hw1", 128, 1, 3, 1, True, True),
    GNCase("c128-n5-b1", 128, 5, 1, 153, False, False),
    GNCase("c256-n1-hw1", 256, 1, 1, 1, False, False),
    GNCase("c128-n1-relu", 128, 1, 3, 154, True, False),
]
GN_BY_ID = {c.id: c for c in GN_CASES}


def gn_case_inputs(case):
    """(xs [B, HW, C], gammas, betas, chmul or None, dcat) f32.  Channels carry the BatchNorm population's gamma / beta and
    mean / std; group 1 has all its channels at mean / std 16 with one common std, group 2 a single live channel (the others
    constant zero)."""
    seed = case_seed(case.id)
    cpg = case.C // GN_GROUPS
    xs, gammas, betas = [], [], []
    for i in range(case.n):
        gamma, beta, ratio, std = population(case.C, seed + 10 * i)
        std[case.C - 2] = 1.0  # (the constant channel of the BatchNorm population is no special case of a group)
        ratio[cpg:2 * cpg], std[cpg:2 * cpg] = 16.0, 0.7
        g = torch.Generator().manual_seed(seed + 10 * i + 1)
        x = (torch.randn(case.B, case.HW, case.C, generator=g).double() + ratio) * std
        x[:, :, 2 * cpg + 1:3 * cpg] = 0.0
        xs.append(x.float())
        gammas.append(gamma)
        betas.append(beta)
    g = torch.Generator().manual_seed(seed + 5)
    chmul = None
    if case.drop:
        chmul = torch.empty(case.B, case.C).bernoulli_(0.8, generator=g) / 0.8
        chmul[:, 0], chmul[:, 1] = 0.0, 1.25
    dcat = torch.randn(case.B, case.HW, case.C * case.n, generator=g)
    return xs, gammas, betas, chmul, dcat


def gn_geometry(case):
    return colreduce_geometry(case.B, case.HW, case.C)
