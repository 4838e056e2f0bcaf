"""fp64 restatement of the prototype pipeline -- reference prototype_handler.py:53-166: sigma, the distance matrix, the
posterior / pseudo-label / soft map, the three monitor means, the class sums, the EMA and the running append -- with the
comparators that hold the HIP kernels of csrc/loss_proto.hip (onda_proto_sigma / _assign / _distances / _class_sums / _ema /
_append, driven by prototype_handler.py) to it.  A plain module like entropy_fp64.py; tests/test_proto_fp64_reference.py runs
the fp32 torch oracle (oracle/prototypes.py) through every comparator on the CPU and measures what BOUNDS record,
tests/test_proto_fp64_parity.py runs the kernels through the same comparators on the GPU.

Restatement (all float64, written plainly).  w = counter / sum counter; g_sq = sum_k w_k sqmean_k, g_m = sum_k w_k proto_k;
sigma = sqrt(g_sq - g_m^2).  D[n,k] = |(f_n - p_k) / sigma| (sigma = 1: Euclidean), minus its row minimum -- the DIRECT form,
what the reference computes.  L = softmax(-D / tau); P = L * prior / sum (prior optional); label = first argmax P, 255 where
max P < thresh; means = (mean max L, mean max P, mean max prior or 0).  Class sums S[k] = sum of f over the rows of class k,
S2[k] of f^2, n[k] the count; a class outside [0, K) drops the row.  EMA: classes with n > 0 move to lam * old + (1 - lam) * S / n,
the others stay.  Append: counter += n; proto += (S - proto * n) / max(counter, 1) with the new counter.

sigma as an argument.  `assign64` and `distances64` take sigma; the tests pass the fp32 sigma that the code under test produced
itself, widened, so that sigma's own cancellation (g_sq - g_m^2, held by `check_sigma`) stays out of the assignment contract.
Likewise `ema64` / `append64` take the fp32 class sums of the code under test (held by `check_class_sums`).

Inputs (`inputs(case)`, seeded, float32).  State: synth_prototypes(256, K) with `offset` added to every prototype channel (post-
ReLU features have a common offset; the zero-mean state is the only one the older tests use) and squared_mean recomputed as
proto^2 + spread^2.  Features: the mixture of test_prototypes_full_size -- proto[cls] (1 - m) + proto[other] m + 0.8 randn, m in
[0, 0.5).  Class logits `out`: randn.  Prior: softmax(SHARP * z), z = randn -- and on a seeded CONTESTED = 35 % of the pixels the
prior also carries the reciprocal of the likelihood, + min((D - min D) / tau, 60) on its logits (D in float64), so that the
posterior there is softmax(SHARP * z) up to rounding.  Why: with these features the likelihood is peaked (the nearest prototype
leads by ~15 in D for Mahalanobis, ~34 for Euclidean) and NO sharpness of an independent prior moves pixels under thresh = 0.3:
measured at N = 2 053 over SHARP in {2, 6, 10, 14, 20, 30}, at most 0.4 % of the pixels get 255 at tau = 1 and none at
tau = 0.25 or with the Euclidean metric.  With the contested pixels every thresholded case that CAN be two-sided is
(`two_sided(case)`: a prior, thresh > 0, K * thresh > 1 -- max P >= 1 / K otherwise -- and N >= 20 so that 5 % is a pixel):
>= 20 % labelled, >= 5 % sent to 255, asserted by the reference test.  The contested pixels are also the ones whose posterior
depends on EVERY distance, not on the nearest two.

BOUNDS, each with its derivation (u = 2^-24, the unit roundoff of float32):

  E_REF[tau]   the largest soft-map error of the fp32 direct-form oracle (oracle.prototypes.assign) against `assign64` over all
               cases with that tau (CASES and LIST_CASE), measured by test_oracle_floor_is_what_bounds_record and recorded
               here rounded up to two digits (the larger of two hosts' figures, see below).
  S(tau)       = 4 * E_REF[tau] + 0.5 * 1e-5 / tau: the soft map's absolute bound.  4 x is the project's margin for one more
               fp32 re-association (entropy_fp64.py, upsample_fp64.py, ece_fp64.py); the second term is the MFMA kernel's
               documented design allowance, a distance error of ~1e-5 (the comment above proto_assign_mfma_kernel) through a
               softmax whose slope is at most 0.5 / tau: |dP_k| <= P_k sum_j |[j = k] - P_j| |dD_j| / tau <= 2 P_k (1 - P_k) dD /
               tau <= 0.5 dD / tau.  S does not depend on the offset: distances are translation-invariant.
  labels       equal to fp64 wherever gap = min(best - second, |best - thresh|) > 2 S(tau): two posteriors each off by S swap
               no further apart.  The exempt pixels are at most EXEMPT_SHARE = 0.5 % of a case and carry a candidate: the
               winner or 255 where |best - thresh| <= 2 S; the runner-up where best - second <= 2 S, unless the pixel lies
               clearly below the threshold, where only 255 will do.
  means        absolute S(tau): a mean of values each within S.
  sigma        relative, per channel, R_SIGMA(K) * u * (g_sq + g_m^2) / (g_sq - g_m^2) with R_SIGMA = K + 3.  Count: each of g_sq
               and g_m is a sum of K terms w_k x_k: two roundings per term (the weight, the product; the kernel's x * counter /
               total likewise) and K - 1 additions: K + 1 on sum |terms|.  g_m^2: 2 (K + 1) through the square, and |g_m| sum |w p|
               <= (g_m^2 + g_sq) / 2 bounds the mixed-sign case, + 1 for the product.  The variance: <= (2 K + 3) u (g_sq + g_m^2)
               + 1 for the subtraction; the root halves it and rounds once: (K + 1.5) ratio + 1.5 <= (K + 3) ratio as ratio >= 1.
               Also: at most 4 x SIGMA_REF, the oracle global_std's measured error in the same unit (u * ratio).
  class sums   per element (rows_per_block + 256) * u * sum |v| over the class and channel, rows_per_block = ceil(N / 256):
               the two-level sequential summation the kernel performs -- a block adds its rows in order (rows_per_block - 1
               roundings, + 1 for v * v in the second moment), the finalize kernel adds the 256 block partials (255).  Counts
               exact (integers below 2^24).
  EMA          R_EMA = 4, times u * (|old * keep| + |(1 - keep) * S / n|) per element: old * keep rounds once and passes the
               final addition (2); S / n, 1 - keep (exact for keep in [0.5, 1], counted all the same), their product and the
               addition (4).  Absent class: bit-identical.
  append       R_APPEND = 4, times u * (|old| + |S / c| + |old * n / c|), c the new counter: old * n (1), the subtraction (1),
               the division (1) and the addition (1) on that term: |old n / c| carries 4, |S / c| 3, |old| 1.  Counter exact.
  distances    the entry point is the direct form: absolute, 4 x DIST_REF[metric], the oracle's measured error; row minimum 0.
"""
import collections
import functools
import math

import torch

from onda_amd.synthetic import synth_prototypes
from oracle import prototypes as op

U32 = 2.0 ** -24
C = 256
SHARP = 2.0
CONTESTED = 0.35
EXEMPT_SHARE = 0.005
R_EMA = 4
R_APPEND = 4

# measured on the CPU by tests/test_proto_fp64_reference.py, which asserts 0.75 <= measured / recorded <= 1.25: torch's fp32 sums
# depend on the host's vector width, and two hosts gave 2.7136e-6 / 2.4351e-6, 1.6045e-6 (both), 2.0756e-7 / 2.0898e-7 for E_REF,
# 2.1667 / 2.4104 for SIGMA_REF, 4.3883e-6 / 4.3624e-6 and 7.9254e-6 (both) for DIST_REF.  Recorded: the larger, rounded up.
E_REF = {0.25: 2.8e-6, 1.0: 1.7e-6, 4.0: 2.1e-7}  # at tau0.25, off8-eucl, tau4
SIGMA_REF = 2.5  # (K32): oracle.global_std, worst channel over the states, in units of u * ratio
DIST_REF = {"mahalanobis": 4.4e-6, "euclidean": 8.0e-6}  # at K2, off8-eucl: oracle.distances, absolute


def S(tau):
    return 4.0 * E_REF[float(tau)] + 0.5 * 1e-5 / tau


def R_SIGMA(K):
    return K + 3


Case = collections.namedtuple("Case", "id N K metric tau thresh prior offset layout twin")


def _case(id, N, K=19, metric="mahalanobis", tau=1.0, thresh=0.3, prior=True, offset=0.0, layout="2d", twin=False):
    return Case(id, N, K, metric, float(tau), thresh, prior, float(offset), layout, twin)


# 32 pixels make an MFMA block, 6 waves x 256 workgroups = 1 536 of them one trip of its grid-stride loop
CASES = [
    _case("tail", 33),                                          # one full block and a block of one pixel
    _case("one", 1),
    _case("short", 31, metric="euclidean", prior=False),        # less than a block
    _case("second-trip", 49189),                                # 1 538 blocks: two waves take a second block
    _case("off8-maha", 2053, offset=8), _case("off8-eucl", 2053, metric="euclidean", offset=8),
    _case("off32-maha", 2053, offset=32), _case("off32-eucl", 2053, metric="euclidean", offset=32),
    _case("tau0.25", 2053, tau=0.25, offset=8), _case("tau4", 2053, tau=4, offset=8),
    _case("nothresh", 2053, thresh=0.0, prior=False),
    _case("K1", 2053, K=1), _case("K2", 2053, K=2), _case("K32", 2053, K=32),
    _case("padded", 2 * 9 * 13, offset=8, layout="padded"),     # NCHW view of NHWC rows of 288 floats; prior rows of 32
    _case("copied", 2 * 9 * 13, metric="euclidean", layout="nchw"),  # NCHW-contiguous: the copy of _rows
]
# classes 3 and 7 are the same prototype and every feature lies around it: every pixel is a tie, three trips of the list pass
LIST_CASE = _case("list", 2085, prior=False, twin=True)
BY_ID = {c.id: c for c in CASES + [LIST_CASE]}
SHAPE = (2, 9, 13)  # B, H, W of the two 4-D layouts


def two_sided(case):
    """Whether a case can both label and reject pixels (see the module docstring)."""
    return case.prior and case.thresh > 0 and case.K * case.thresh > 1 and case.N >= 20


# ------------------------------------------------------------------------------------------------------ seeded inputs
def state(K, offset, twin=False):
    """(proto, squared_mean, counter) f32: synth_prototypes with `offset` on every prototype channel."""
    proto0, sq0, counter = synth_prototypes(C, K)
    spread2 = sq0.double() - proto0.double() ** 2
    proto = proto0 + offset
    if twin:
        proto[7] = proto[3]
        spread2[7] = spread2[3]
    return proto, (proto.double() ** 2 + spread2).float(), counter


def mixture(proto, N, g):
    K = proto.shape[0]
    cls = torch.randint(0, K, (N,), generator=g)
    mix = torch.rand(N, 1, generator=g) * 0.5
    other = proto[torch.randint(0, K, (N,), generator=g)]
    return proto[cls] * (1 - mix) + other * mix + 0.8 * torch.randn(N, C, generator=g)


Inputs = collections.namedtuple("Inputs", "state rows prior out")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Inputs(state, rows f32[N,256], prior f32[N,K] or None, out f32[N,K]) of a case; shared, never written to."""
    st = state(case.K, case.offset, case.twin)
    g = torch.Generator().manual_seed(4100 + [c.id for c in CASES + [LIST_CASE]].index(case.id))
    if case.twin:
        rows = st[0][3] + 0.8 * torch.randn(case.N, C, generator=g)
    else:
        rows = mixture(st[0], case.N, g)
    out = torch.randn(case.N, case.K, generator=g)
    prior = None
    if case.prior:
        logits = SHARP * torch.randn(case.N, case.K, generator=g).double()
        contested = torch.rand(case.N, generator=g) < CONTESTED
        d = distances64(rows, st[0], sigma64(st) if case.metric == "mahalanobis" else None)
        logits += contested[:, None] * (d / case.tau).clamp(max=60.0)
        prior = logits.softmax(1).float()
    return Inputs(st, rows, prior, out)


def nchw(case, m, device, pitch=None):
    """[N, ch] rows as the tensor the handler is given in the case's layout: the matrix itself, an NCHW view of an NHWC buffer
    whose rows are `pitch` floats long, or a contiguous NCHW tensor."""
    if m is None:
        return None
    if case.layout == "2d":
        return m.to(device)
    B, H, W = SHAPE
    if case.layout == "nchw":
        return m.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous().to(device)
    buf = torch.full((B, H, W, pitch), float("nan"))  # the padding is never to be read
    buf[..., : m.shape[1]] = m.reshape(B, H, W, -1)
    return buf.to(device)[..., : m.shape[1]].permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------ the restatement
def sigma_terms(st):
    proto, sq, counter = (t.double() for t in st)
    w = counter / counter.sum()
    return (sq * w[:, None]).sum(0), (proto * w[:, None]).sum(0)


def sigma64(st):
    g_sq, g_m = sigma_terms(st)
    return (g_sq - g_m ** 2).sqrt()


def distances64(rows, proto, sigma=None):
    """f64[N,K], the direct form minus its row minimum; sigma None: Euclidean.  One class at a time (N x 256 doubles)."""
    f, p = rows.double(), proto.double()
    s = torch.ones(C, dtype=torch.float64) if sigma is None else sigma.double().cpu()
    d = torch.stack([(((f - p[k]) / s) ** 2).sum(1).sqrt() for k in range(p.shape[0])], 1)
    return d - d.min(1, keepdim=True)[0]


Assigned = collections.namedtuple("Assigned", "labels soft means best arg second arg2 gap thresh")


def assign64(rows, prior, proto, sigma, tau, thresh):
    d = distances64(rows, proto, sigma)
    lik = (-d / tau).softmax(1)
    post = lik if prior is None else lik * prior.double()
    post = post / post.sum(1, keepdim=True)
    best, arg = post.max(1)  # the first maximum
    if post.shape[1] > 1:
        rest = post.clone()
        rest[torch.arange(post.shape[0]), arg] = -math.inf
        second, arg2 = rest.max(1)
    else:
        second, arg2 = torch.full_like(best, -math.inf), arg
    labels = torch.where(best < thresh, torch.full_like(arg, 255), arg)
    means = torch.stack([lik.max(1)[0].mean(), best.mean(),
                         prior.double().max(1)[0].mean() if prior is not None else torch.zeros((), dtype=torch.float64)])
    gap = torch.minimum(best - second, (best - thresh).abs())
    return Assigned(labels, post, means, best, arg, second, arg2, gap, thresh)


def class_sums64(rows, cls, K):
    """(S f64[K,256], S2, n, A = sum |f|, A2 = sum f^2 -- the bounds' weights) over the rows whose class is in [0, K)."""
    f = rows.double()
    keep = (cls >= 0) & (cls < K)
    onehot = torch.zeros(rows.shape[0], K, dtype=torch.float64)
    onehot[keep, cls[keep].long()] = 1.0
    return onehot.T @ f, onehot.T @ f ** 2, onehot.sum(0), onehot.T @ f.abs(), onehot.T @ f ** 2


def ema64(st, sums, sums2, counts, lam):
    """(proto, squared_mean, weights of the bound) from fp32 class sums; `lam` is the float32 the kernel receives."""
    lam = float(torch.tensor(lam, dtype=torch.float32))
    n = counts.double()
    keep = torch.where(n > 0, torch.full_like(n, lam), torch.ones_like(n))[:, None]
    den = torch.where(n > 0, n, torch.ones_like(n))[:, None]
    res, wts = [], []
    for old, s in ((st[0], sums), (st[1], sums2)):
        a, b = old.double() * keep, (1 - keep) * (s.double() / den)
        res.append(a + b)
        wts.append(a.abs() + b.abs())
    return res[0], res[1], wts[0], wts[1]


def append64(st, sums, sums2, counts):
    """(proto, squared_mean, counter, weights) of the running append; st None: the empty state."""
    n = counts.double()
    if st is None:
        st = (torch.zeros_like(sums), torch.zeros_like(sums2), torch.zeros_like(counts))
    counter = st[2].double() + n
    den = torch.where(counter > 0, counter, torch.ones_like(counter))[:, None]
    res, wts = [], []
    for old, s in ((st[0], sums), (st[1], sums2)):
        o = old.double()
        res.append(o + (s.double() - o * n[:, None]) / den)
        wts.append(o.abs() + (s.double() / den).abs() + (o * n[:, None] / den).abs())
    return res[0], res[1], counter, wts[0], wts[1]


# ------------------------------------------------------------------------------------------------------ the comparators
def _cpu64(t):
    return t.detach().double().cpu()


def soft_error(soft, ref):
    return float((_cpu64(soft) - ref.soft).abs().max())


def check_assign(labels, soft, means, ref, tau, what, soft_only=False):
    """Labels i64[N,1] or [N], soft [N,K], means (3) against `ref` (Assigned) under S(tau).  Prints the figures first; returns
    (soft-map error, means error, exempt share, label mismatches outside the exempt pixels)."""
    s = S(tau)
    finite = bool(torch.isfinite(soft).all())
    e_soft = soft_error(soft, ref)
    e_means = float((torch.as_tensor(means, dtype=torch.float64).cpu() - ref.means).abs().max())
    lab = labels.detach().cpu().reshape(-1).long()
    exempt = ref.gap <= 2 * s
    wrong = lab != ref.labels
    hard = int((wrong & ~exempt).sum())
    # an exempt pixel carries a candidate: the reference label; at a close threshold the winner or 255; at a close race the
    # runner-up -- but only on the side of the threshold the pixel is on: clearly below it nothing but 255 will do
    cand = lab == ref.labels
    close_race, close_thr = (ref.best - ref.second) <= 2 * s, (ref.best - ref.thresh).abs() <= 2 * s
    clearly_below = ~close_thr & (ref.best < ref.thresh)
    cand |= close_thr & ((lab == ref.arg) | (lab == 255))
    cand |= close_race & ~clearly_below & (lab == ref.arg2)
    stray = int((exempt & ~cand).sum())
    share = float(exempt.double().mean())
    print(f"{what}: soft map {e_soft:.3e} (S = {s:.3e}), means {e_means:.3e}, exempt {int(exempt.sum())} of {lab.numel()} "
          f"({100 * share:.3f} %), labels off {int(wrong.sum())} ({hard} outside the exempt pixels, {stray} not a candidate), finite {finite}")
    assert finite, f"{what}: non-finite soft map"
    assert e_soft <= s, f"{what}: soft map off by {e_soft:.3e} > S = {s:.3e}"
    if soft_only:
        return e_soft, e_means, share, hard
    assert e_means <= s, f"{what}: a monitor mean off by {e_means:.3e} > S = {s:.3e}"
    assert share <= EXEMPT_SHARE, f"{what}: {100 * share:.3f} % of the pixels lie within 2 S of a tie: the inputs do not test the labels"
    assert hard == 0, f"{what}: {hard} labels differ from fp64 at a gap above 2 S = {2 * s:.3e}"
    assert stray == 0, f"{what}: {stray} pixels near a tie carry a label that is no candidate"
    return e_soft, e_means, share, hard


def sigma_error(sigma, st):
    """Worst channel of |sigma - sigma64| / sigma64 in units of u * (g_sq + g_m^2) / (g_sq - g_m^2)."""
    g_sq, g_m = sigma_terms(st)
    ref = (g_sq - g_m ** 2).sqrt()
    ratio = (g_sq + g_m ** 2) / (g_sq - g_m ** 2)
    return float((((_cpu64(sigma) - ref).abs() / ref) / (U32 * ratio)).max()), float(ratio.max())


def check_sigma(sigma, st, what):
    K = st[0].shape[0]
    e, ratio = sigma_error(sigma, st)
    bound = min(R_SIGMA(K), 4 * SIGMA_REF)
    print(f"{what}: sigma off by {e:.3f} u x ratio (worst ratio {ratio:.1f}); derived {R_SIGMA(K)}, 4 x oracle {4 * SIGMA_REF:.3f}")
    assert bool(torch.isfinite(sigma).all()) and e <= bound, f"{what}: sigma off by {e:.3f} u x ratio > {bound:.3f}"
    return e


def check_class_sums(sums, sums2, counts, rows, cls, K, what):
    N = rows.shape[0]
    s, s2, n, a, a2 = class_sums64(rows, cls, K)
    r = (N + 255) // 256 + 256
    worst = 0.0
    for got, ref, wt, name in ((sums, s, a, "sum f"), (sums2, s2, a2, "sum f^2")):
        err = (_cpu64(got) - ref).abs()
        assert bool((err[wt == 0] == 0).all()), f"{what}: {name} of an empty class is not 0"
        worst = max(worst, float((err / (r * U32 * wt).clamp(min=1e-300)).max()))
    exact = bool(torch.equal(_cpu64(counts), n))
    print(f"{what}: class sums at {worst:.4f} of ({r} u sum |v|), counts exact {exact}, {int((n == 0).sum())} empty classes, "
          f"{int(n.sum())} of {N} rows counted")
    assert exact, f"{what}: counts differ"
    assert worst <= 1.0, f"{what}: a class sum is off by {worst:.3f} x its bound"
    return worst


def check_weighted(got, ref, wts, r, what):
    e = float(((_cpu64(got) - ref).abs() / (r * U32 * wts).clamp(min=1e-300)).max())
    print(f"{what}: at {e:.4f} of ({r} u sum |operands|)")
    assert bool(torch.isfinite(got).all()) and e <= 1.0, f"{what}: off by {e:.3f} x its bound"
    return e


def check_distances(got, rows, proto, sigma, metric, what):
    ref = distances64(rows, proto, sigma)
    g = _cpu64(got)
    e, rowmin = float((g - ref).abs().max()), float(g.min(1)[0].abs().max())
    print(f"{what}: distances off by {e:.3e} (4 x oracle = {4 * DIST_REF[metric]:.3e}), largest row minimum {rowmin}")
    assert g.shape == ref.shape and rowmin == 0.0, f"{what}: a row minimum is not exactly 0"
    assert e <= 4 * DIST_REF[metric], f"{what}: distances off by {e:.3e} > {4 * DIST_REF[metric]:.3e}"
    return e


def flagged(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------ the fp32 oracle leg
def oracle_assign(case):
    """(labels, soft, means, sigma or None) of oracle.prototypes.assign on a case, and the sigma it used."""
    x = inputs(case)
    labels, soft, conf = op.assign(x.rows, x.prior, x.state, case.tau, case.thresh, case.metric)
    means = torch.stack([conf.double(), soft.max(1)[0].double().mean(),
                         x.prior.max(1)[0].double().mean() if x.prior is not None else torch.zeros((), dtype=torch.float64)])
    return labels, soft, means, (op.global_std(x.state) if case.metric == "mahalanobis" else None)


@functools.lru_cache(maxsize=None)
def reference(case):
    """assign64 of a case under the fp64 sigma -- what the population and the exempt share are asserted on."""
    x = inputs(case)
    sg = sigma64(x.state) if case.metric == "mahalanobis" else None
    return assign64(x.rows, x.prior, x.state[0], sg, case.tau, case.thresh)


def reference_with(case, sigma):
    """assign64 of a case under a given fp32 sigma (None: Euclidean)."""
    x = inputs(case)
    return assign64(x.rows, x.prior, x.state[0], sigma, case.tau, case.thresh)


def check_twin(labels, soft, means, ref, tau, what, first=3, twin=7):
    """LIST_CASE: classes `first` and `twin` are one prototype, so every pixel is an exact tie between them and the generic
    label rule exempts it.  Here: the soft map and the means within S, and the FIRST of the two wherever the fp64 gap to every
    other class and to the threshold exceeds 2 S."""
    s = S(tau)
    e_soft = soft_error(soft, ref)
    e_means = float((torch.as_tensor(means, dtype=torch.float64).cpu() - ref.means).abs().max())
    lab = labels.detach().cpu().reshape(-1).long()
    tie = float((ref.soft[:, first] - ref.soft[:, twin]).abs().max())
    rest = ref.soft.clone()
    rest[:, [first, twin]] = -math.inf
    clear = torch.minimum(ref.soft[:, first] - rest.max(1)[0], (ref.soft[:, first] - ref.thresh).abs()) > 2 * s
    off = int(((lab != first) & clear).sum())
    print(f"{what}: soft map {e_soft:.3e} (S = {s:.3e}), means {e_means:.3e}, fp64 tie {tie}, {int(clear.sum())} of {lab.numel()} "
          f"pixels clear of the other classes and the threshold, {off} of them not labelled {first}")
    assert tie == 0.0 and bool(clear.double().mean() > 0.9), f"{what}: the inputs are not the tie they are meant to be"
    assert e_soft <= s and e_means <= s, f"{what}: soft map {e_soft:.3e} / means {e_means:.3e} > S = {s:.3e}"
    assert off == 0, f"{what}: {off} pixels of an exact tie do not carry the first maximum"
    return e_soft, e_means


# ------------------------------------------------------------------------------------------------------ class sums, EMA, append
SumsCase = collections.namedtuple("SumsCase", "id N offset layout classes")
SUMS_CASES = [
    SumsCase("few", 37, 0.0, "2d", False),           # fewer pixels than the 256 blocks: most blocks are empty
    SumsCase("classes", 2053, 0.0, "2d", True),      # `classes` given: 30 % of the rows 255, one -1, class 6 never occurs
    SumsCase("large", 33540, 8.0, "2d", False),      # 132 rows per block, sums of f^2 of ~1e5
    SumsCase("padded", 2 * 9 * 13, 8.0, "padded", False),
]
SUMS_K = 19


@functools.lru_cache(maxsize=None)
def sums_inputs(sc):
    """(rows f32[N,256], out f32[N,K], cls i32[N]): cls is argmax(out), or the list handed over as `classes`."""
    g = torch.Generator().manual_seed(5200 + SUMS_CASES.index(sc))
    rows = mixture(state(SUMS_K, sc.offset)[0], sc.N, g)
    out = torch.randn(sc.N, SUMS_K, generator=g)
    cls = out.argmax(1).to(torch.int32)
    if sc.classes:
        cls[cls == 6] = 5
        cls[torch.rand(sc.N, generator=g) < 0.3] = 255
        cls[11] = -1
    return rows, out, cls


@functools.lru_cache(maxsize=None)
def update_inputs():
    """(state, batch A: rows, out without classes 4 and 11; batch B: rows, out without class 5; batch C: rows, out with all)."""
    g = torch.Generator().manual_seed(6300)
    st = state(SUMS_K, 0.0)
    batches = []
    for N, absent in ((2053, (4, 11)), (307, (5,)), (2053, ())):
        rows, out = mixture(st[0], N, g), torch.randn(N, SUMS_K, generator=g)
        out[:, list(absent)] = -1e9
        batches.append((rows, out))
    return st, batches
