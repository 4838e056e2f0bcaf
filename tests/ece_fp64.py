"""fp64 restatement of the expected calibration error of an evaluation (reference monitoring.py:99-136 on
adaptation_model.py:145-149 / prototypes.py:191-200) and the comparator that holds a HIP table to it (imported by the
ECE tests; a plain module, like upsample_fp64.py, whose interpolation helpers it reuses).

Restatement.  Per output pixel: the K values of the align_corners bilinear upsample on ATen's float32 weights, widened to
float64 (upsample_fp64.upsample); mode "logits" takes their float64 softmax, mode "probs" leaves them; confidence = the
maximum, class = its index.  Row of the table = floor(conf / gap) with gap = float32(1.0 / bins) -- exactly what ATen's
fmod-based float32 floor division yields for a float32 conf (`rows_exact` does it in rationals; the CPU tests hold it to
torch.floor_divide) -- clamped to [0, bins - 1]; a non-finite conf counts (0, 0, 1) into row `bins`.  Table int64
[bins + 1, 3]: (sum of round(conf * 2^32), correct, pixels), every pixel counted, a label of 255 never correct.
ECE = sum_b |table[b, 0] / 2^32 - table[b, 1]| / sum_b table[b, 2]; NaN when row `bins` is not empty.

Comparator for interpolated inputs, where float32 confidences sit near bin edges.  A pixel is NEAR when its float64
confidence is within DELTA of an edge j * gap (0 < j < bins), or its two largest values are within DELTA of each other.
DELTA = 4 x the worst |conf(fp32 ATen on the CPU: F.interpolate, softmax, max) - conf(fp64)| over CASES + CONTENTION in
both modes -- the project's usual 4 x fp32 floor.  Measured: 3.67e-7 (5x7 -> 64x128, mode logits; mode probs: 9.5e-8;
the contention inputs: 2.2e-7), so DELTA = 1.5e-6.  Held:
  * every pixel is counted: sum of the pixel column == B * H * W, row `bins` empty (finite inputs);
  * the correct total differs from the float64 one by at most the number of near-tie pixels;
  * per bin, pixels and correct lie between the count of the bin's certain pixels and that plus its slack: the near pixels
    that may land in it (one near edge j: bins j - 1 and j; a near-tie pixel away from an edge: its bin and both neighbours);
  * per bin, |sum of conf - certain sum| <= slack * 1 + pixels * DELTA (a confidence is at most 1);
  * |ECE - ECE(fp64)| <= (3 * near + N * DELTA) / N: a near pixel that changes bin moves two terms |S_b - C_b| by at most
    1 each and a flipped class one more; every pixel's conf is off by at most DELTA.
Near pixels may be at most NEAR_CAP = 1 % of a case: a condition on the seeds, asserted with fp32 ATen on the CPU.
"""
import functools
from fractions import Fraction

import torch
import torch.nn.functional as F

import upsample_fp64 as U

FIX = 1 << 32
DELTA = 1.5e-6
NEAR_CAP = 0.01
BATCH = 2

# h, w, H, W, K, ld
CASES = [
    (3, 5, 7, 11, 5, 5),        # ld = K = 5: scalar class loads
    (4, 23, 9, 701, 19, 32),    # several workgroups, non-integer ratios
    (5, 7, 64, 128, 19, 32),    # the evaluation's own ratio range at test size
]
CONTENTION = (5, 7, 64, 128, 19, 32)  # with `contention_inputs`: > 95 % of the pixels in the top bin
EXACT_CASE = (8, 16, 8, 16, 19, 32)   # the identity size: l1 = 0, values pass through unchanged
EXACT_BINS = (1000, 10, 4, 1)


def case_id(c):
    return "%dx%d-%dx%d-K%d-ld%d" % c


def gap32(bins):
    return float(torch.tensor(1.0 / bins, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(case, mode, B=BATCH):
    """(x f32[B,K,h,w], labels u8[B,H,W]); mode "logits": randn * 3, mode "probs": their softmax.  Labels: random in
    [0, K), ~10 % 255, and 30 % set to the float64 class of the logits so that the correct column is not nearly empty (the
    same labels in both modes)."""
    h, w, H, W, K, ld = case
    g = torch.Generator().manual_seed(18 + h * 1000003 + w * 10007 + H * 101 + W + K * 7 + ld)
    x = torch.randn(B, K, h, w, generator=g) * 3
    labels = torch.randint(0, K, (B, H, W), generator=g).to(torch.uint8)
    cls = pixels(x, H, W, "logits")[1]
    take = torch.rand(B, H, W, generator=g) < 0.3
    labels[take] = cls[take].to(torch.uint8)
    labels[torch.rand(B, H, W, generator=g) < 0.1] = 255
    return (x.softmax(1) if mode == "probs" else x), labels


@functools.lru_cache(maxsize=None)
def contention_inputs(B=BATCH):
    """Logits of a converged model: randn * 3 with 25 added to class 7 everywhere (conf = 1 - ~18 e^-25)."""
    h, w, H, W, K, ld = CONTENTION
    g = torch.Generator().manual_seed(1807)
    x = torch.randn(B, K, h, w, generator=g) * 3
    x[:, 7] += 25.0
    labels = torch.randint(0, K, (B, H, W), generator=g).to(torch.uint8)
    labels[torch.rand(B, H, W, generator=g) < 0.6] = 7
    labels[torch.rand(B, H, W, generator=g) < 0.1] = 255
    return x, labels


def exact_inputs(bins, safe=False):
    """(conf f32[B,8,16], cls i64[B,8,16], labels u8[B,8,16]) placed by hand: inside bins, exactly on edges (j / bins
    rounded to float32), one float below and above an edge, 1.0, and one NaN and one +inf pixel (each at (0, 0) of an
    image: at the identity size a pixel is read, with weight 0, by its left / upper neighbours only).  safe=True leaves
    out what the reference cannot take: the non-finite pixels, and confidences whose bin is >= bins."""
    h, w, K = EXACT_CASE[0], EXACT_CASE[1], EXACT_CASE[4]
    g = torch.Generator().manual_seed(4242 + bins)
    n = BATCH * h * w
    conf = torch.rand(n, generator=g) * 0.9 + 0.06          # inside bins
    js = torch.arange(0, bins + 1)
    if len(js) > 40:
        js = torch.cat([js[:14], js[(bins // 2) - 6:(bins // 2) + 6], js[-14:]])
    edges = (js.double() / bins).float()                     # j / bins rounded to float32
    up, down = torch.nextafter(edges, torch.tensor(2.0)), torch.nextafter(edges, torch.tensor(-1.0))
    special = torch.cat([edges, up, down, torch.tensor([1.0, 1.0, 0.3, 0.7, 0.6])]).clamp(0.0, 1.0)
    free = torch.arange(n)
    free = free[(free >= w) & (free != h * w)]  # (not in row 0 of image 0, the NaN pixel's row, nor at the +inf pixel)
    pos = free[torch.randperm(len(free), generator=g)[: len(special)]]
    conf[pos] = special
    conf = conf.reshape(BATCH, h, w)
    if safe:
        g32 = torch.tensor(gap32(bins))
        conf = torch.where(torch.floor_divide(conf, g32) >= bins, conf * 0.5, conf)
    else:
        conf[0, 0, 0] = float("nan")
        conf[1, 0, 0] = float("inf")
    cls = torch.randint(0, K, (BATCH, h, w), generator=g)
    labels = torch.where(torch.rand(BATCH, h, w, generator=g) < 0.5, cls, torch.randint(0, K, (BATCH, h, w), generator=g))
    labels[torch.rand(BATCH, h, w, generator=g) < 0.15] = 255
    return conf, cls, labels.to(torch.uint8)


def exact_map(conf, cls, K):
    """f32[B,K,h,w] whose maximum over K is `conf` at class `cls` (the others: conf - 1, or 0 beside a non-finite one)."""
    rest = torch.where(torch.isfinite(conf), conf - 1.0, torch.zeros_like(conf))
    x = rest.unsqueeze(1).repeat(1, K, 1, 1)
    x.scatter_(1, cls.unsqueeze(1), conf.unsqueeze(1))
    return x


# ------------------------------------------------------------------------------------------------- the restatement
def pixels(x, H, W, mode):
    """(conf f64[B,H,W], class i64[B,H,W], margin f64[B,H,W] between the two largest values) of x f32[B,K,h,w]."""
    up = U.upsample(x, H, W)
    if mode == "logits":
        up = up.softmax(1)
    top2 = up.topk(2, dim=1)
    return top2.values[:, 0], top2.indices[:, 0], top2.values[:, 0] - top2.values[:, 1]


def rows_exact(conf32, bins):
    """Row per float32 confidence, in rationals: floor(conf / float32(1 / bins)) clamped; non-finite -> bins."""
    gap = Fraction(gap32(bins))
    out = []
    for c in conf32.reshape(-1).tolist():
        if c != c or c in (float("inf"), float("-inf")):
            out.append(bins)
        else:
            out.append(min(max(Fraction(c) // gap, 0), bins - 1))
    return torch.tensor(out, dtype=torch.int64).reshape(conf32.shape)


def rows_fp64(conf64, bins):
    finite = torch.isfinite(conf64)
    row = torch.floor(torch.where(finite, conf64, torch.zeros_like(conf64)) / gap32(bins)).clamp(0, bins - 1).long()
    return torch.where(finite, row, torch.full_like(row, bins))


def table_of(conf, cls, labels, bins, rows=None):
    """int64 [bins + 1, 3] of per-pixel (conf, class) against labels; `rows` overrides the float64 rule."""
    conf, cls, labels = conf.reshape(-1).double(), cls.reshape(-1).long(), labels.reshape(-1).long()
    rows = (rows_fp64(conf, bins) if rows is None else rows).reshape(-1)
    ok = rows < bins
    fix = torch.where(ok, torch.round(torch.where(ok, conf, torch.zeros_like(conf)).clamp(-2.0 ** 30, 2.0 ** 30) * FIX), torch.zeros_like(conf)).long()
    hit = ((cls == labels) & ok).long()
    t = torch.zeros(bins + 1, 3, dtype=torch.int64)
    t.index_add_(0, rows, torch.stack([fix, hit, torch.ones_like(hit)], 1))
    return t


def ece_of(table):
    table = torch.as_tensor(table).cpu()
    bins = table.shape[0] - 1
    if int(table[bins, 2]) > 0:
        return float("nan")
    m = table[:bins].double()
    return ((m[:, 0] / FIX - m[:, 1]).abs().sum() / m[:, 2].sum()).item()


# ------------------------------------------------------------------------------------------------- the fp32 ATen leg
def aten_pixels(x, H, W, mode):
    """fp32 ATen on the CPU: (conf f32, class) of interp(x).softmax(1) ("logits") or interp(x) ("probs")."""
    up = F.interpolate(x.float(), size=(H, W), mode="bilinear", align_corners=True)
    if mode == "logits":
        up = up.softmax(1)
    return up.max(1)


def aten_table(x, labels, bins, mode):
    conf, cls = aten_pixels(x, *labels.shape[1:], mode)
    finite = torch.isfinite(conf)
    rows = torch.where(finite, torch.floor_divide(torch.where(finite, conf, torch.zeros_like(conf)), 1.0 / bins).clamp(0, bins - 1).long(),
                       torch.full_like(cls, bins))
    return table_of(conf, cls, labels, bins, rows)


# ------------------------------------------------------------------------------------------------- the comparator
class Split:
    """The certain / near split of a case at `bins`: what a table may hold."""

    def __init__(self, x, labels, bins, mode, delta=DELTA):
        B, H, W = labels.shape
        conf, cls, margin = pixels(x, H, W, mode)
        conf, cls, margin, lab = conf.reshape(-1), cls.reshape(-1), margin.reshape(-1), labels.reshape(-1).long()
        self.bins, self.n, self.delta = bins, conf.numel(), delta
        gap = gap32(bins)
        row = rows_fp64(conf, bins)
        j = torch.round(conf / gap).clamp(1, max(bins - 1, 1))          # the nearest inner edge
        edge = ((conf - j * gap).abs() <= delta) & (bins > 1)
        tie = margin <= delta
        near = edge | tie
        self.near, self.ties = int(near.sum()), int(tie.sum())
        certain = ~near
        self.certain = table_of(conf[certain], cls[certain], lab[certain], bins)
        self.full = table_of(conf, cls, lab, bins)
        slack = torch.zeros(bins + 1, dtype=torch.int64)
        je = j[edge].long()
        slack.index_add_(0, je - 1, torch.ones_like(je))
        slack.index_add_(0, je, torch.ones_like(je))
        rt = row[tie & ~edge]
        for d in (-1, 0, 1):
            slack.index_add_(0, (rt + d).clamp(0, bins - 1), torch.ones_like(rt) * ((rt + d >= 0) & (rt + d < bins)).long())
        self.slack = slack
        self.ece = ece_of(self.full)
        self.ece_bound = (3.0 * self.near + self.n * delta) / self.n
        self.top_share = float((row == bins - 1).double().mean())

    def check(self, table, what="table", extra_sum=None):
        """`extra_sum`: a further allowance per bin on the conf sums (a float32-accumulated reference table)."""
        t = torch.as_tensor(table).cpu().long()
        b = self.bins
        assert tuple(t.shape) == (b + 1, 3), t.shape
        print(f"{what}: {self.n} pixels, {self.near} near ({self.ties} ties), ECE {ece_of(t):.9f} vs fp64 {self.ece:.9f} "
              f"(bound {self.ece_bound:.2e})")
        assert self.near <= NEAR_CAP * self.n, f"{what}: {self.near} near pixels of {self.n}: choose another seed"
        assert int(t[:b, 2].sum()) + int(t[b, 2]) == self.n, f"{what}: {int(t[:, 2].sum())} pixels counted, {self.n} expected"
        assert int(t[b, 2]) == 0 and int(t[b, 0]) == 0 and int(t[b, 1]) == 0, f"{what}: overflow row {t[b].tolist()}"
        assert abs(int(t[:b, 1].sum()) - int(self.full[:b, 1].sum())) <= self.ties, \
            f"{what}: {int(t[:b, 1].sum())} correct, fp64 {int(self.full[:b, 1].sum())}, {self.ties} near ties"
        lo, hi = self.certain[:b], self.certain[:b] + self.slack[:b, None]
        for col, name in ((2, "pixels"), (1, "correct")):
            bad = (t[:b, col] < lo[:, col]) | (t[:b, col] > hi[:, col])
            assert not bad.any(), f"{what}: {name} of bin {int(bad.nonzero()[0])}: {int(t[:b, col][bad][0])}, " \
                                  f"certain {int(lo[:, col][bad][0])} + slack {int(self.slack[:b][bad][0])}"
        err = (t[:b, 0] - self.certain[:b, 0]).double().abs() / FIX
        allow = self.slack[:b].double() + t[:b, 2].double() * self.delta + (0.0 if extra_sum is None else extra_sum)
        bad = err > allow
        assert not bad.any(), f"{what}: conf sum of bin {int(bad.nonzero()[0])} off by {float(err[bad][0]):.3e} > {float(allow[bad][0]):.3e}"
        assert abs(ece_of(t) - self.ece) <= self.ece_bound, f"{what}: ECE {ece_of(t)} vs {self.ece} (bound {self.ece_bound})"

    def flagged(self, table):
        try:
            self.check(table, "probe")
        except AssertionError:
            return True
        return False


@functools.lru_cache(maxsize=None)
def split(case, mode, bins, contention=False):
    x, labels = contention_inputs() if contention else inputs(case, mode)
    return Split(x, labels, bins, mode)
