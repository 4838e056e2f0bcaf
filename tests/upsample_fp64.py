"""fp64 reference of the bilinear (align_corners) upsample / fused cross-entropy head and the comparator that holds a HIP
result to it (imported by the upsample tests; a plain module, like conv_fp64.py).

Reference: the kernels reproduce ATen's fp32 index arithmetic on purpose (scale = float32(n_in - 1) / float32(n_out - 1),
src = scale * dst rounded to fp32, i0 = int(src), i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1), so the reference
takes exactly these weights -- `axis_matrix`, two non-zeros per row -- widens them to float64 and is exact after that:
upsample = einsum('Yy,bkyx,Xx->bkYX'), its gradient the transposed einsum, the fused head upsample -> float64 log-softmax ->
mean of -logp[label] over the labels < K (labels travel as uint8: every value >= K is ignored), gradient by float64 autograd.

Comparator, three ways:
  (a) relative L2 of the whole tensor;
  (b) relative L2 of the worst group.  kind "up" (an upsampled [B,K,H,W] tensor): one pixel's K-vector.  kind "grad" (a
      gradient with respect to the low-resolution logits, [B,K,h,w]): one low-resolution pixel's K-vector, and each
      low-resolution column and each low-resolution row taken over everything else (batch, classes, the other axis) -- a fault
      confined to a seam column of the backward's column blocks or to an edge row cannot be diluted by the rest of the tensor.
      A group whose reference norm is below FLOOR times the tensor's RMS (times sqrt of the group's size) is compared
      absolutely, against that floor: a K-vector that happens to cancel to almost nothing has no meaningful relative error;
  (c) exact equality wherever the reference is exact by structure (padded class columns, sentinel columns the launch must
      not touch, all-ignored batches, the identity size).

BOUNDS, (tensor rel-L2, worst-group rel-L2) per quantity.  Basis: fp32 ATen on the CPU (F.interpolate + F.cross_entropy and
their autograd) run through this comparator against this reference at every entry of CASES with the inputs of `inputs` --
that is the fp32-rounding floor of one legitimate evaluation order (ATen scatters the gradient pixel by pixel; the kernels
gather in two separable passes, a different but equally legitimate fp32 summation order, which is what the margin is for).
                  CPU floor, worst entry of CASES (a / b)    multiple                       bound (a / b)
  "fwd"           4.0e-8 / 1.2e-7                            4, rounded to one digit        2e-7 / 5e-7
  "grad"          6.7e-7 / 1.1e-6   (UpsampleFn backward)    4, rounded to one digit        3e-6 / 4e-6
  "ce_grad"       5.8e-7 / 1.4e-6   (d 2.5 * loss / d logits)  4, rounded to one digit      2e-6 / 5e-6  (5.5e-6 taken down)
  CE value        1.3e-7  (|value - ref| / |ref|)            4, rounded to one digit        5e-7
(the gradient floors are those of the long fp32 chains: ~ 2 W / w output columns times ~ 2 H / h rows scattered into one
low-resolution pixel one after another, 3x5 -> 7x801 and 4x5 -> 9x802 being the longest; the identity entry's forward and gradient are exact.)
Measured on the MI355X: not yet -- no GPU run of test_upsample_fp64_parity.py stands behind these bounds so far; every test
there prints its figures before it asserts, and the worst of them belong here beside the floors.  A figure that needs more
than the margin is a finding to explain, not a reason to widen a bound.
For scale: a gather range that misses its outermost output column at 3x17 -> 7x1021 changes that low-resolution column by
1e-4 .. 1e-3 relative L2 (tests/test_upsample_fp64_reference.py), a normaliser off by one pixel (n / (n + 1)) the whole
tensor by 1 / n.
"""
import functools

import torch
import torch.nn.functional as F

FLOOR = 0.1  # groups whose reference norm is below FLOOR * tensor RMS * sqrt(group size) are compared against that floor

BOUNDS = {"fwd": (2e-7, 5e-7), "grad": (3e-6, 4e-6), "ce_grad": (2e-6, 5e-6)}
CE_VALUE_BOUND = 5e-7

# h, w, H, W, K, ldl.  Pass A of the fused backward cuts the w low-resolution columns into blocks of
# CW = min(64, int(634 * sx) - 2) columns, sx = float32(w - 1) / float32(W - 1) (documentation: the tests read no CW from
# the library, but plant one run of ignored labels over the output span of block 1, or block 0 where there is one block).
CASES = [
    # shape                     CW  blocks          what it reaches
    (3, 17, 7, 1021, 19, 32),   # 7   3 (7, 7, 3)     an interior block with both neighbours, ratio 1020 / 16
    (3, 129, 5, 1024, 19, 32),  # 64  3 (64, 64, 1)   the workload's own sx = 128 / 1023, a last block of one column
    (3, 5, 7, 801, 19, 32),     # 1   5               one column per block, the widest span per column
    (4, 23, 9, 701, 22, 32),    # 17  2 (17, 6)       22 classes together with a seam (63 112 bytes of LDS at this CW: the
                                #                     64 KB opt-in is reached by the K = 24 and K = 32 entries below)
    (9, 65, 6, 34, 19, 32),     # 64  2 (64, 1)       downsampling in both axes (sx, sy > 1)
    (5, 7, 5, 7, 19, 20),       # 64  1               the identity: bit-exact forward
    (5, 7, 11, 13, 32, 32),     # 64  1               K = KMAX = ldl, no padding column; 95 488 bytes of LDS
    (4, 23, 9, 701, 19, 19),    # 17  2 (17, 6)       ldl not a multiple of 4: scalar class loads in upsample_kernel
    (4, 23, 9, 701, 24, 32),    # 17  2 (17, 6)       LDS above 64 KB (68 384 bytes) together with a seam
    (4, 5, 9, 802, 19, 32),     # 1   5               one column per block at non-integer ratios: 3x5 -> 7x801 above is 200x
                                #                     along x and 3x along y, the one entry with integer ratios on both axes
]
INTEGER_RATIO = [(3, 5, 7, 801, 19, 32)]
CW = {(3, 17, 7, 1021): 7, (3, 129, 5, 1024): 64, (3, 5, 7, 801): 1, (4, 23, 9, 701): 17, (9, 65, 6, 34): 64, (5, 7, 5, 7): 64,
      (5, 7, 11, 13): 64, (4, 5, 9, 802): 1}
HIST_GLOBAL_CASE = (5, 7, 33, 47, 40, 40)  # K * K > 1024: the confusion matrix is counted by global atomics per pixel
PAST_FUSED_CASE = (2, 3, 3, 1001, 19, 32)  # 500x along x, batch 1: past what the fused head's backward takes (~211x)
BATCH = 2


def case_id(c):
    return "%dx%d-%dx%d-K%d-ld%d" % c


# ------------------------------------------------------------------------------------------------- the reference
@functools.lru_cache(maxsize=None)
def _axis(n_in, n_out):
    one = torch.ones((), dtype=torch.float32)
    scale = (one * (n_in - 1)) / (one * (n_out - 1)) if n_out > 1 else one * 0
    src = scale * torch.arange(n_out, dtype=torch.float32)  # (one fp32 rounding per product, as in ATen)
    i0 = src.to(torch.int64)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = src - i0.to(torch.float32)
    l0 = 1.0 - l1
    return src, i0, i1, l0, l1


def axis_taps(n_in, n_out):
    """(src, i0, i1, l0, l1) of ATen's align_corners rule for every destination index, in float32 / int64."""
    return _axis(n_in, n_out)


def axis_matrix(n_in, n_out):
    """float64 [n_out, n_in]: row dst holds l0 at i0 and l1 at i1 (added where i1 == i0, the last source index)."""
    _, i0, i1, l0, l1 = _axis(n_in, n_out)
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    rows = torch.arange(n_out)
    m.index_put_((rows, i0), l0.double(), accumulate=True)
    m.index_put_((rows, i1), l1.double(), accumulate=True)
    return m


def upsample(x, H, W):
    """[B,K,H,W] float64 of the bilinear align_corners upsample of x[B,K,h,w]."""
    return torch.einsum("Yy,bkyx,Xx->bkYX", axis_matrix(x.shape[2], H), x.double().cpu(), axis_matrix(x.shape[3], W))


def upsample_grad(gy, h, w):
    """[B,K,h,w] float64: the gradient of `upsample` under the upstream gradient gy[B,K,H,W]."""
    return torch.einsum("Yy,bkYX,Xx->bkyx", axis_matrix(h, gy.shape[2]), gy.double().cpu(), axis_matrix(w, gy.shape[3]))


def head_ce(x, labels, upstream=1.0):
    """(value, gradient [B,K,h,w], kept labels) of the fused head in float64: upsample to the labels' size, log-softmax,
    mean of -logp[label] over the labels < K; the gradient is that of upstream * value.  No kept label: NaN and zeros."""
    K = x.shape[1]
    labels = labels.cpu().to(torch.uint8)
    keep = labels < K
    n = int(keep.sum())
    if n == 0:
        return float("nan"), torch.zeros(x.shape, dtype=torch.float64), 0
    lo = x.detach().double().cpu().requires_grad_(True)
    logp = torch.log_softmax(upsample_autograd(lo, *labels.shape[1:]), 1)
    picked = logp.gather(1, labels.long().clamp(max=K - 1)[:, None])[:, 0]
    value = -(picked * keep).sum() / n
    (value * upstream).backward()
    return value.item(), lo.grad, n


def upsample_autograd(x64, H, W):
    return torch.einsum("Yy,bkyx,Xx->bkYX", axis_matrix(x64.shape[2], H), x64, axis_matrix(x64.shape[3], W))


def class_map(up64):
    """(class map int64 [B,H,W], top-2 margin float64 [B,H,W], K-vector norm [B,H,W]) of float64 upsampled logits."""
    top2 = up64.topk(2, dim=1)
    return top2[1][:, 0], top2[0][:, 0] - top2[0][:, 1], up64.norm(dim=1)


def confusion(labels, cls, K, keep=None):
    """int64 [K, K]: rows = label in [0, K), columns = class, over the pixels under `keep` (None: all)."""
    labels, cls = labels.reshape(-1).long().cpu(), cls.reshape(-1).long().cpu()
    ok = labels < K
    if keep is not None:
        ok = ok & keep.reshape(-1).cpu()
    return torch.bincount(labels[ok] * K + cls[ok], minlength=K * K).reshape(K, K)


def decided(margin, norm):
    """Pixels whose class a result within BOUNDS["fwd"] cannot change.  Derivation: criterion (b) bounds the L2 error of a
    pixel's K-vector by e = BOUNDS["fwd"][1] * max(|v|, FLOOR * rms * sqrt(K)); the errors e1, e2 of its two largest logits
    then satisfy |e1| + |e2| <= sqrt(2) * e, so an order of the two that differs from the reference's needs a margin of at
    most sqrt(2) * e.  The logits are randn * 3 (|v| ~ 3 * sqrt(K) ~ 13 at K = 19), so the margin is ~ 2e-5 * bound / 1e-6."""
    rms = (norm.double() ** 2).mean().sqrt()  # = tensor RMS * sqrt(K)
    return margin > 2.0 ** 0.5 * BOUNDS["fwd"][1] * torch.maximum(norm, FLOOR * rms)


UNDECIDED_CAP = 1e-3  # share of pixels `decided` may leave out (a condition on the seeds, checked on the CPU)


# ------------------------------------------------------------------------------------------------- the fp32 ATen leg
def aten_upsample(x, H, W):
    return F.interpolate(x.float(), size=(H, W), mode="bilinear", align_corners=True)


def aten_head_ce(x, labels, upstream=1.0):
    """fp32 ATen on the CPU: (value, gradient, the gradient with respect to the upsampled logits)."""
    K = x.shape[1]
    lab = labels.long().clone()
    lab[lab >= K] = 255
    lo = x.detach().float().cpu().requires_grad_(True)
    up = aten_upsample(lo, *labels.shape[1:])
    up.retain_grad()
    value = F.cross_entropy(up, lab, ignore_index=255)
    (value * upstream).backward()
    return value.item(), lo.grad, up.grad


# ------------------------------------------------------------------------------------------------- seeded inputs
def block_span(w, W, cw, block):
    """(X0, X1): the output columns whose interpolation reads a column of pass-A block `block` (cw columns a block), one of
    slack on either side, clamped to the image."""
    xb, xe = block * cw, min(w, block * cw + cw)
    inv = (W - 1) / (w - 1)
    return max(int((xb - 1) * inv) - 1, 0), min(int(-(-xe * inv // 1)) + 1, W - 1)


@functools.lru_cache(maxsize=None)
def inputs(case, B=BATCH):
    """(logits f32[B,K,h,w] = randn * 3, labels u8[B,H,W]) of a case, seeded by the case.  Labels are random in [0, K) with
    about 10 % set to 255, five set to values in [K, 255), one full output row of 255 (image 0, row H // 2) and, in image
    B - 1, row 1, a run of 255 over the whole output span of one pass-A block (block 1, or the only block)."""
    h, w, H, W, K, ldl = case
    g = torch.Generator().manual_seed(h * 1000003 + w * 10007 + H * 101 + W + K * 7 + ldl)
    logits = torch.randn(B, K, h, w, generator=g) * 3
    labels = torch.randint(0, K, (B, H, W), generator=g).to(torch.uint8)
    labels[torch.rand(B, H, W, generator=g) < 0.1] = 255
    flat = labels.view(-1)
    pos = torch.randint(0, flat.numel(), (5,), generator=g)
    flat[pos] = torch.randint(K, 255, (5,), generator=g).to(torch.uint8)
    labels[0, H // 2] = 255
    cw = CW.get((h, w, H, W), 64)
    X0, X1 = block_span(w, W, cw, 1 if w > cw else 0)
    labels[B - 1, 1, X0:X1 + 1] = 255
    return logits, labels


def upstream_gradient(case, B=BATCH):
    h, w, H, W, K, ldl = case
    return torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(H * 7919 + W))


# ------------------------------------------------------------------------------------------------- the comparator
def _ratio(num, den):
    rel = torch.sqrt(num / den)
    return torch.where(den > 0, rel, torch.where(num > 0, torch.full_like(rel, float("inf")), torch.zeros_like(rel)))


def measure(got, ref, kind):
    """(tensor rel-L2, worst group rel-L2, name of the worst group).  got, ref: [B,K,n,m]."""
    ref = ref.detach().double().cpu()
    d2 = (got.detach().double().cpu() - ref) ** 2
    r2 = ref ** 2
    tensor = _ratio(d2.sum(), r2.sum()).item()
    ms = r2.mean() * FLOOR ** 2  # (FLOOR * rms)^2: a group's floor is this times its size
    sets = [("pixel (b, y, x)", (1,))]
    if kind == "grad":
        sets += [("column x", (0, 1, 2)), ("row y", (0, 1, 3))]
    worst, where = 0.0, "none"
    for name, dims in sets:
        size = 1
        for a in dims:
            size *= ref.shape[a]
        rel = _ratio(d2.sum(dims), torch.clamp(r2.sum(dims), min=float(ms) * size))
        flat = int(rel.reshape(-1).argmax())
        if rel.reshape(-1)[flat].item() >= worst:
            worst = rel.reshape(-1)[flat].item()
            where = name + " = " + str(tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), rel.shape)))
    return tensor, worst, where


def exact_violations(got, want, mask=None):
    """Elements under `mask` (broadcast against got; None = all) where got != want bit for bit (-0.0 == 0.0)."""
    got = got.detach().cpu()
    bad = got != (want.detach().cpu() if torch.is_tensor(want) else want)
    if mask is not None:
        bad = bad & mask
    return int(bad.sum())


def check(got, ref, quantity, what, exact=()):
    """Assert (a) and (b) against BOUNDS[quantity] and every (c) in `exact`: triples (tensor, want, mask) -- `tensor` must
    equal `want` (a tensor or a number) wherever `mask` is True (None: everywhere).  Returns the two figures."""
    kind = "up" if quantity == "fwd" else "grad"
    bound_t, bound_g = BOUNDS[quantity]
    t, g, where = measure(got, ref, kind)
    print(f"{what}: tensor rel-L2 {t:.3e} (bound {bound_t:.1e}), worst group {g:.3e} at {where} (bound {bound_g:.1e})")
    assert t <= bound_t, f"{what}: relative L2 {t:.3e} > {bound_t:.1e} (worst group {where}: {g:.3e})"
    assert g <= bound_g, f"{what}: worst group, {where}: relative L2 {g:.3e} > {bound_g:.1e}"
    for tensor, want, mask in exact:
        n = exact_violations(tensor, want, mask)
        assert n == 0, f"{what}: {n} elements differ where the result is exact by structure"
    return t, g


def flagged(got, ref, quantity, exact=()):
    """True when `check` would fail (the teeth tests)."""
    try:
        check(got, ref, quantity, "probe", exact)
    except AssertionError:
        return True
    return False


def old_close(a, b, rel):
    """The tensor-max criterion of test_hip_kernels.close: max|err| <= rel * max|ref|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return (a - b).abs().max().item() <= rel * max(b.abs().max().item(), 1e-20)
