"""fp64 restatement of the pointwise kernels of csrc/pointwise.hip that are not upsampling -- the ASPP head's SE gate (colsum
pooling of csrc/norm.hip, se_fc1 / se_fc2, chan_scale, chan_scale_limbs of csrc/norm_l2.hip, the kernels behind onda_se_fc_bwd)
and the stem's 3x3 / s2 / p1 ceil-mode max-pool -- and the comparators that hold them and ops/norm.py (SEScaleFn, MaxPoolFn) to
it.  A plain module like norm_fp64.py, whose plan restatement, u, margin, limb floor and report it imports:
tests/test_pointwise_fp64_reference.py runs fp32 torch and seeded defects through every comparator on the CPU and measures what
FLOOR records; tests/test_pointwise_fp64_parity.py runs the kernels through the same comparators on the GPU.

Restatement, float64 and plain arithmetic, every stage a function of its own inputs (x, dout [B, HW, C]; w1 [R, C]; w2 [C, R]):
    pooled = sum_px x / HW                 pre1 = W1 pooled + b1, hidden = relu(pre1)
    s = W2 hidden + b2, gate = 1 / (1 + exp(-s))                  out = x * gate
    dgate = sum_px dout * x                dpre2 = dgate * gate * (1 - gate)
    dw2 = dpre2^T hidden, db2 = sum_b dpre2                       dpre1 = (dpre2 W2) * mask      (the mask an ARGUMENT)
    dw1 = dpre1^T pooled, db1 = sum_b dpre1                       dpooled = (dpre1 W1) / HW      dx = dout * gate + dpooled

STAGE-WISE.  The reference of a stage is computed in fp64 from the fp32 values the code under test FED to that stage -- its own
pooled, hidden, gate, dgate, dpre1 (a namespace `v` carries them) -- so a stage's bound is that stage's arithmetic alone and
nothing is propagated.  [hidden > 0] of the code under test is the mask; check_hidden separately holds hidden to the sign of pre1
wherever |pre1| exceeds its bound and to exactly 0 where pre1 is exactly 0 or negative by construction (`planted`), and counts
the units it had to exempt.  dpre2 never leaves the kernels (se_bwd_w2_kernel and se_bwd_hidden_kernel form it in registers), so
the stages dw2, db2 and dpre1 start from (dgate, gate) and carry its three roundings.

Units: never one max-norm over a tensor.  pooled, dgate, gate, dpooled per (image, channel); hidden, dpre1 per (image, unit);
dw1, dw2 per element; db1, db2 per unit; out, dx per element.  Each unit is held to u * (the sum of the magnitudes of the terms
of its OWN contraction) * its constant; a unit whose terms are all zero must be exact.  The worst unit is reported with its index.

Constants, counted in the code (as conv_fp64.chain_bounds and the norm_fp64 header count a chain): the number of roundings a
term of the contraction can pass through.
  colreduce_kernel + colsum_finalize_kernel (pooled, dgate): rho = sqrt((L + 1) / P), L = ceil(rows_per_chunk / ry) + ry - 1,
      P = chunks (norm_fp64.colreduce_geometry; the partials are combined in double); + 1 for the product dout * x (dgate) or
      for alpha, which crosses the ABI as an fp32 1 / HW while the restatement divides exactly (pooled); + 1 for the result.
  se_fc1_kernel (hidden) / se_bwd_hidden_kernel (dpre1): a lane's chain of ceil(C / 64) terms, each a rounded product (+ 1), the 6
      levels of wave_sum, the bias (fc1: + 1) or dpre2's own three roundings (bwd_hidden: + 3).
  se_fc2_kernel (s): a sequential chain of R terms from b2, products rounded: R + 1.
  se_bwd_w2_kernel (dw2, db2): chains of B terms; the product with hidden (dw2: + 1); dpre2: + 3.
  se_bwd_w1_kernel (dw1, db1, dpooled): chains of B, B and R terms; products (+ 1); dpooled: * scale, and the scale itself an
      fp32 1 / HW (+ 2).
  chan_scale_kernel: out = fl(x * gate): 1; dx = fl(fl(dout * gate) + dpooled): 2 on |dout * gate| + |dpooled|.
The gate's own arithmetic (expf, add, divide) is NOT derived: its constant is FLOOR["sigmoid"], relative to the gate; the error
of s reaches the gate through the slope gate * (1 - gate).  Below fp32's smallest normal (2^-126) a gate is held absolutely:
the format promises nothing there.  Where fp32 MUST saturate the gate has to be exactly 1 (exp(-s) < 2^-25: 1 + e rounds to 1)
or exactly 0 (-s > 89: expf overflows); it is finite and in [0, 1] everywhere.

FLOOR: what fp32 torch on the CPU (mean, F.linear, sigmoid, autograd; pixels contiguous per channel) is off by against the
restatement, in the same units (u * the unit's sum of magnitudes), stage-wise too, the worst unit of the worst case of SE_CASES;
measured by test_floor_is_what_bounds_record and recorded rounded up.  A tolerance is MARGIN (4) x the larger of FLOOR and the
derived constant -- never tuned to what a kernel achieves.
Limb output (chan_scale_limbs, the max-pool's limb rows): the materialised value within LIMB_FLOOR (2^-22) of the tensor's scale
bound of the fp32 result, the figure test_maxpool_ceil and norm_fp64 use.

Max-pool: the window scan restated in plain code -- rows then columns of the 3x3 window clipped to the image, strict '>' keeps
the first maximum, NaN always wins, a window of -inf keeps its first in-range element -- with the slot per output and dx by
routing dy to the slot.  Comparators: bit equality of y (NaN positions equal) and of dx.  dy is drawn from small integers over
a power of two, so the at most four contributions of an input pixel sum exactly in any order.
"""
import collections
import math
import types

import torch

from norm_fp64 import LIMB_FLOOR, MARGIN, U, _hold, case_seed, col_plan, colreduce_geometry, flagged  # noqa: F401

TINY = 2.0 ** -126          # fp32's smallest normal
ONE_BELOW = 2.0 ** -25      # exp(-s) below this: 1 + e is 1 in fp32 whatever expf's last bits
ZERO_ABOVE = 89.0           # -s above this: expf(-s) is +inf in fp32 (log(FLT_MAX) = 88.72)
C_DPRE2 = 3.0               # fl(fl(dgate * g) * fl(1 - g))
C_OUT = 1.0
C_DX = 2.0
CLEARANCE = 16.0            # every non-planted |pre1| of a case is at least this many bounds away from the kink

# fp32 torch on the CPU against the restatement, stage by stage, in units of u * the unit's sum of magnitudes (u * the gate for
# "sigmoid"), the worst unit of the worst case; measured by tests/test_pointwise_fp64_reference.py::
# test_floor_is_what_bounds_record, which holds measured / recorded to [0.75, 1.25].  Recorded: the measured figure rounded up.
FLOOR = {
    "pooled": 3.5,    # / (u * sum_px |x| / HW), per (image, channel)
    "hidden": 1.1,    # / (u * (|W1| |pooled| + |b1|)), per (image, unit)
    "s": 1.9,         # / (u * (|W2| |hidden| + |b2|)), per (image, channel)
    "sigmoid": 2.0,   # / (u * gate): sigmoid(s) of torch's own fp32 s
    "out": 1.0,       # per element, / (u * |x gate|)
    "dgate": 2.7,     # / (u * sum_px |dout x|)
    "dw2": 3.8,       # per element, / (u * sum_b |dpre2 hidden|)
    "db2": 2.9,       # / (u * sum_b |dpre2|)
    "dpre1": 1.7,     # / (u * |dpre2| |W2|), per (image, unit)
    "dw1": 1.9,       # per element, / (u * sum_b |dpre1 pooled|)
    "db1": 1.0,       # / (u * sum_b |dpre1|)
    "dpooled": 3.8,   # / (u * |dpre1| |W1| / HW)
    "dx": 2.0,        # per element, / (u * (|dout gate| + |dpooled|))
}

STAGES = ("pooled", "hidden", "gate", "out", "dgate", "dw2", "db2", "dpre1", "dw1", "db1", "dpooled", "dx")


# ------------------------------------------------------------------------------------------------ SE: the restatement
def _d(*ts):
    return [t.double() for t in ts]


def _contract(a, b):
    """(a b^T, |a| |b|^T): a contraction and the sum of the magnitudes of its terms."""
    return a @ b.t(), a.abs() @ b.abs().t()


def se_pooled64(x):
    (x,) = _d(x)
    return x.sum(1) / x.shape[1], x.abs().sum(1) / x.shape[1]


def se_pre1_64(pooled, w1, b1):
    p, w, b = _d(pooled, w1, b1)
    v, m = _contract(p, w)
    return v + b, m + b.abs()


def se_s64(hidden, w2, b2):
    h, w, b = _d(hidden, w2, b2)
    v, m = _contract(h, w)
    return v + b, m + b.abs()


def se_gate64(s):
    return 1.0 / (1.0 + torch.exp(-s.double()))


def se_out64(x, gate):
    x, g = _d(x, gate)
    v = x * g[:, None, :]
    return v, v.abs()


def se_dgate64(dout, x):
    d, x = _d(dout, x)
    t = d * x
    return t.sum(1), t.abs().sum(1)


def se_dpre2_64(dgate, gate):
    d, g = _d(dgate, gate)
    return d * g * (1.0 - g)


def se_dw2_64(dpre2, hidden):
    (h,) = _d(hidden)
    return _contract(dpre2.t(), h.t())


def se_db2_64(dpre2):
    return dpre2.sum(0), dpre2.abs().sum(0)


def se_dpre1_64(dpre2, w2, mask):
    (w,) = _d(w2)
    v, m = _contract(dpre2, w.t())
    return v * mask.double(), m * mask.double()


def se_dw1_64(dpre1, pooled):
    d, p = _d(dpre1, pooled)
    return _contract(d.t(), p.t())


def se_db1_64(dpre1):
    (d,) = _d(dpre1)
    return d.sum(0), d.abs().sum(0)


def se_dpooled64(dpre1, w1, HW):
    d, w = _d(dpre1, w1)
    v, m = _contract(d, w.t())
    return v / HW, m / HW


def se_dx64(dout, gate, dpooled):
    d, g, p = _d(dout, gate, dpooled)
    t = d * g[:, None, :]
    return t + p[:, None, :], t.abs() + p.abs()[:, None, :]


def rho(B, HW, C):
    L, P = colreduce_geometry(B, HW, C)
    return math.sqrt((L + 1) / P)


def stage64(name, v):
    """(reference, sum of magnitudes, derived constant) of a stage from what `v` -- the inputs and the code under test's own
    upstream values -- fed to it.  For "hidden" the reference is pre1, for "gate" it is s: their comparators go on from there."""
    B, HW, C = v.x.shape
    R = v.w1.shape[0]
    lanes = -(-C // 64)
    if name == "pooled":
        return (*se_pooled64(v.x), rho(B, HW, C) + 2.0)
    if name == "hidden":
        return (*se_pre1_64(v.pooled, v.w1, v.b1), lanes + 1.0 + 6.0 + 1.0)
    if name == "gate":
        return (*se_s64(v.hidden, v.w2, v.b2), R + 1.0)
    if name == "out":
        return (*se_out64(v.x, v.gate), C_OUT)
    if name == "dgate":
        return (*se_dgate64(v.dout, v.x), rho(B, HW, C) + 2.0)
    if name == "dw2":
        return (*se_dw2_64(se_dpre2_64(v.dgate, v.gate), v.hidden), B + 1.0 + C_DPRE2)
    if name == "db2":
        return (*se_db2_64(se_dpre2_64(v.dgate, v.gate)), B + C_DPRE2)
    if name == "dpre1":
        return (*se_dpre1_64(se_dpre2_64(v.dgate, v.gate), v.w2, v.hidden > 0), lanes + 1.0 + 6.0 + C_DPRE2)
    if name == "dw1":
        return (*se_dw1_64(v.dpre1, v.pooled), B + 1.0)
    if name == "db1":
        return (*se_db1_64(v.dpre1), float(B))
    if name == "dpooled":
        return (*se_dpooled64(v.dpre1, v.w1, HW), R + 1.0 + 2.0)
    if name == "dx":
        return (*se_dx64(v.dout, v.gate, v.dpooled), C_DX)
    raise KeyError(name)


def se_chain64(inp):
    """The whole block in fp64, every stage fed the stage before it: what double-precision torch computes."""
    v = types.SimpleNamespace(x=inp.x, w1=inp.w1, b1=inp.b1, w2=inp.w2, b2=inp.b2, dout=inp.dout)
    for name in STAGES:
        ref = stage64(name, v)[0]
        if name == "hidden":
            v.pre1, ref = ref, ref.clamp(min=0)
        if name == "gate":
            v.s, ref = ref, se_gate64(ref)
        setattr(v, name, ref)
    return v


# ------------------------------------------------------------------------------------------------ SE: comparators
def stage_tol(name, v):
    """(reference, bound) of a plain stage: MARGIN x the larger of FLOOR and the derived constant, on the unit's own terms."""
    ref, mag, c = stage64(name, v)
    return ref, MARGIN * max(FLOOR[name], c) * U * mag


def check_hidden(v, where, planted=None):
    """hidden [B, R] of the code under test against relu(pre1) of its own pooled.  planted [B, R] bool: units whose pre1 is
    exactly 0 or negative by construction -- hidden exactly 0.  Returns (units exempt from the sign check, the smallest
    |pre1| / bound of the units that are not planted)."""
    pre, tol = stage_tol("hidden", v)
    got = v.hidden.double()
    _hold("se hidden", (got - pre.clamp(min=0)).abs(), tol, where)
    clear = pre.abs() > tol
    wrong = clear & ((got > 0) != (pre > 0))
    assert not bool(wrong.any()), f"{where}: {int(wrong.sum())} hidden units on the wrong side of the kink, first at {wrong.nonzero()[0].tolist()}"
    free = torch.ones_like(clear)
    if planted is not None:
        assert bool((got[planted] == 0).all()), f"{where}: a hidden unit whose pre1 is <= 0 by construction is not exactly 0"
        free = ~planted
    ratio = torch.where(free, pre.abs() / tol.clamp(min=1e-300), torch.full_like(pre, float("inf")))
    return int((free & ~clear).sum()), float(ratio.min())


def check_gate(v, where):
    """gate [B, C] against sigmoid(s) of the code under test's own hidden: the chain's error of s through the slope, the
    sigmoid's own arithmetic relative to the gate; absolute below fp32's normals; exact where fp32 must saturate."""
    s, mag, c = stage64("gate", v)
    got = v.gate.double()
    assert bool(torch.isfinite(got).all()) and bool(((got >= 0) & (got <= 1)).all()), f"{where}: a gate outside [0, 1]"
    ds = MARGIN * max(FLOOR["s"], c) * U * mag
    g = se_gate64(s)
    slope = g / (1.0 + torch.exp(s))  # gate * (1 - gate) without the cancellation
    tol = ds * slope * torch.exp(ds) + MARGIN * FLOOR["sigmoid"] * U * g
    tol = torch.where(g < TINY, torch.full_like(tol, TINY), tol)
    _hold("se gate", (got - g).abs(), tol, where)
    one = torch.exp(-(s - ds)) < ONE_BELOW
    zero = -(s + ds) > ZERO_ABOVE
    assert bool((got[one] == 1).all()), f"{where}: a gate that fp32 must round to 1 is not 1"
    assert bool((got[zero] == 0).all()), f"{where}: a gate whose exponential overflows fp32 is not 0"
    return int(one.sum()), int(zero.sum())


def check_stage(name, v, where, planted=None):
    """The comparator of a stage on getattr(v, name), fed what v holds upstream."""
    if name == "hidden":
        return check_hidden(v, where, planted)
    if name == "gate":
        return check_gate(v, where)
    ref, tol = stage_tol(name, v)
    got = getattr(v, name).double()
    assert got.shape == ref.shape, f"{where}: {name} has shape {tuple(got.shape)}, expected {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{where}: {name} is not finite"
    return _hold("se " + name, (got - ref).abs(), tol, where)


def check_se(v, where, planted=None):
    """Every stage; returns check_hidden's (exempt, clearance)."""
    kink = None
    for name in STAGES:
        r = check_stage(name, v, where, planted)
        if name == "hidden":
            kink = r
    return kink


def se_flagged(v, where, planted=None):
    """The stages whose comparator rejects what v holds."""
    return {name for name in STAGES if flagged(check_stage, name, v, where, planted)}


def check_limbs(mat, fp32, bound, where, what="se out limbs"):
    """A limb output materialised against the fp32 result: within LIMB_FLOOR of the tensor's scale bound, which bounds it."""
    assert float(fp32.abs().max()) <= bound * (1 + 1e-6), f"{where}: the scale bound {bound:.6e} is below max|value|"
    err = (mat.double() - fp32.double()).abs().max().reshape(1)
    _hold(what, err, torch.full((1,), LIMB_FLOOR * bound, dtype=torch.float64), where)


# ------------------------------------------------------------------------------------------------ SE: cases
SECase = collections.namedtuple("SECase", "id B C R H W seed")
SEIn = collections.namedtuple("SEIn", "x w1 b1 w2 b2 dout planted")

# the smallest shapes that reach each path (test_cases_reach_the_paths_they_are_named_for); the seeds are chosen so that no
# non-planted |pre1| comes within CLEARANCE bounds of the kink (test_no_unit_is_exempt_from_the_sign_check)
SE_CASES = [
    SECase("head", 2, 1280, 80, 9, 17, 4),          # the model's C and R; 5 chunks, the last of 25 of 32 rows
    SECase("chunks68", 2, 1280, 80, 33, 65, 5),     # 68 chunks: colsum_finalize_kernel's second round; the last chunk has 1 row
    SECase("ragged", 3, 288, 18, 5, 7, 1),          # c4 = 72 on cx = 64; C % 256 = 32; R % 4 = 2; 2 chunks, the last of 3 rows
    SECase("wide-batch", 5, 32, 2, 1, 3, 2),        # B > R: the max(R, B) * C launch; 3 rows under 32 row lanes; cx = 8
    SECase("kink", 2, 1280, 80, 3, 5, 2),           # image 1 all zeros, b1 <= 0 with exact zeros: pre1 = b1 in any arithmetic
    SECase("saturated", 2, 64, 4, 3, 5, 1),         # b2 planted at +-30 and +-100
    SECase("one-hot-dout", 2, 1280, 80, 9, 17, 8),  # dout zero outside one pixel per image: dx elsewhere is dpooled alone
]
SE_BY_ID = {c.id: c for c in SE_CASES}
SATURATED_B2 = (30.0, -30.0, 100.0, -100.0)  # channels 0 .. 3


def one_hot_pixel(b, HW):
    return (7 * b + 3) % HW


def se_case_inputs(case):
    """x post-ReLU and off-centre, as behind GroupNorm + ReLU; W1 ~ randn / sqrt(C), W2 ~ randn / sqrt(R), small biases;
    dout ~ randn; the plants of the case."""
    g = torch.Generator().manual_seed(case.seed)
    B, C, R, HW = case.B, case.C, case.R, case.H * case.W
    x = (torch.randn(B, HW, C, generator=g) + 0.3).clamp(min=0)
    w1, b1 = torch.randn(R, C, generator=g) / C ** 0.5, torch.randn(R, generator=g) * 0.1
    w2, b2 = torch.randn(C, R, generator=g) / R ** 0.5, torch.randn(C, generator=g) * 0.1
    dout = torch.randn(B, HW, C, generator=g)
    planted = None
    if case.id == "kink":
        x[1] = 0.0
        b1 = -b1.abs()
        b1[::4] = 0.0
        planted = torch.zeros(B, R, dtype=torch.bool)
        planted[1] = True
    if case.id == "saturated":
        b2[:4] = torch.tensor(SATURATED_B2)
    if case.id == "one-hot-dout":
        keep = torch.zeros(B, HW, 1)
        for b in range(B):
            keep[b, one_hot_pixel(b, HW)] = 1.0
        dout = dout * keep
    return SEIn(x, w1, b1, w2, b2, dout, planted)


# ------------------------------------------------------------------------------------------------ max-pool
def pool_out_size(n, ceil_mode=True):
    """Outputs of a 3 / s2 / p1 pool along an axis of n: the last window must start inside the image or its left padding."""
    if not ceil_mode:
        return (n - 1) // 2 + 1
    o = -(-(n - 1) // 2) + 1
    return o - 1 if (o - 1) * 2 >= n + 1 else o


def first_maximum(v, best):
    """Does v replace best?  Strict '>' keeps the first maximum; NaN always wins (and then stays: nothing is > NaN)."""
    return (v > best) | (v != v)


PoolRef = collections.namedtuple("PoolRef", "y slot dx")


def maxpool_scan(x, dy=None, take=first_maximum, ceil_mode=True):
    """x [B, Hi, Wi, C] in its own dtype (comparisons only: no arithmetic on x).  slot = r * 3 + s of the window element kept;
    dx: dy routed to the slot (dy's dtype; exact for dy on a small power-of-two grid)."""
    B, Hi, Wi, C = x.shape
    Ho, Wo = pool_out_size(Hi, ceil_mode), pool_out_size(Wi, ceil_mode)
    y = x.new_empty(B, Ho, Wo, C)
    slot = torch.zeros(B, Ho, Wo, C, dtype=torch.int64)
    dx = torch.zeros(B, Hi, Wi, C, dtype=dy.dtype) if dy is not None else None
    for ho in range(Ho):
        for wo in range(Wo):
            window = [(r, s, ho * 2 - 1 + r, wo * 2 - 1 + s) for r in range(3) for s in range(3)
                      if 0 <= ho * 2 - 1 + r < Hi and 0 <= wo * 2 - 1 + s < Wi]
            best = sl = None
            for r, s, hi, wi in window:
                v = x[:, hi, wi]
                if best is None:
                    best, sl = v.clone(), torch.full((B, C), r * 3 + s, dtype=torch.int64)
                else:
                    t = take(v, best)
                    best, sl = torch.where(t, v, best), torch.where(t, torch.full_like(sl, r * 3 + s), sl)
            y[:, ho, wo], slot[:, ho, wo] = best, sl
            if dy is not None:
                for r, s, hi, wi in window:
                    dx[:, hi, wi] += torch.where(sl == r * 3 + s, dy[:, ho, wo], torch.zeros_like(dy[:, ho, wo]))
    return PoolRef(y, slot, dx)


def same_bits(a, b):
    """Bit equality (so -0.0 is not 0.0), NaN positions equal whatever the payload."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = a != a
    if not torch.equal(nan, b != b):
        return False
    as_int = torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(a.contiguous().view(as_int)[~nan], b.contiguous().view(as_int)[~nan])


def check_pool(y, slot, dx, ref, where):
    """y, dx (and the slots, when the code under test exposes them) bit for bit."""
    assert y.shape == ref.y.shape, f"{where}: the pooled tensor has shape {tuple(y.shape)}, expected {tuple(ref.y.shape)}"
    assert same_bits(y, ref.y), f"{where}: y differs in {int(((y != ref.y) & ~((y != y) & (ref.y != ref.y))).sum())} places (or in a sign of zero / a NaN position)"
    if slot is not None:
        assert torch.equal(slot.long(), ref.slot), f"{where}: {int((slot.long() != ref.slot).sum())} slots differ"
    if dx is not None:
        assert same_bits(dx, ref.dx), f"{where}: dx differs in {int((dx != ref.dx).sum())} places"


PoolCase = collections.namedtuple("PoolCase", "id B Hi Wi C")
POOL_CASES = [
    PoolCase("1x1", 3, 1, 1, 4),          # one window, one element
    PoolCase("2x3", 2, 2, 3, 4),          # every window clipped
    PoolCase("3x4-c68", 2, 3, 4, 68),     # c4 = 17: no power of two
    PoolCase("9x11", 2, 9, 11, 64),
    PoolCase("8x9", 1, 8, 9, 64),         # even height: the last window row is clipped below
]
POOL_BY_ID = {c.id: c for c in POOL_CASES}


def pool_case_inputs(case, nonfinite=False):
    """(x, dy) f32.  x signed, about a quarter of it on the 1/2 grid (ties between negatives, zeros of both signs); dy small
    integers over 4.  nonfinite: channel 0 has the window of output (0, 0) of image 0 all -inf, channel 1 a +inf and a -inf,
    the channels from 2 on a few NaN (one of them the first element of a window)."""
    g = torch.Generator().manual_seed(case_seed("pool-" + case.id))
    B, Hi, Wi, C = case.B, case.Hi, case.Wi, case.C
    x = torch.randn(B, Hi, Wi, C, generator=g)
    on_grid = torch.rand(B, Hi, Wi, C, generator=g) < 0.25
    x = torch.where(on_grid, torch.round(x * 2) / 2, x)
    nan = torch.rand(B, Hi, Wi, C, generator=g) < 0.03
    if nonfinite:
        nan[..., :2] = False
        nan[0, 0, 0, 2] = True
        x[nan] = float("nan")
        x[0, :2, :2, 0] = float("-inf")
        x[0, 0, 0, 1] = float("inf")
        x[B - 1, Hi - 1, Wi - 1, 1] = float("-inf")
    dy = torch.randint(-8, 9, (B, pool_out_size(Hi), pool_out_size(Wi), C), generator=g).float() / 4
    return x, dy
