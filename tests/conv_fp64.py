"""fp64 reference of the convolutions and the comparator that holds a HIP result to it (imported by the conv tests; a plain
module, like g14_common.py).

Reference: one filter tap at a time over the tap's live window of the NHWC input (the rows and columns it reads outside the
padding), one image at a time, accumulated in float64 with torch.matmul on whatever device the operands live on -- forward `window @ W_tap.T`, data gradient scatter-add of `dy @ W_tap` into the tap's window,
weight gradient `dy.T @ window`; bias gradient and the per-channel sum / sum of squares of y for the statistics partials.

Comparator, three ways:
  (a) relative L2 of the whole tensor;
  (b) relative L2 of the worst block: 64 rows x 64 channels of the [M, C] GEMM view of an activation (M in NHWC row order),
      64 Cout x 1 tap x 64 Cin of a weight gradient; partial edge blocks are blocks.  A fault confined to one tile, one
      stream-K piece, one tap or the last partial tile row cannot be diluted by the rest of the tensor;
  (c) exact equality wherever the reference is exact by structure (pixels no tap reaches, taps that only see padding,
      padded head columns, prefilled buffer regions the launch must not touch).
(a) and (b) take another tensor for their denominators (`scale_ref`) where the result is a sum that cancels: the eval-mode
epilogue that writes limb planes (eval_conv_ref and its bound, at the end, with the schedule helpers both parity files share).
"""
import ctypes
import math

import torch
import torch.nn.functional as F

BLOCK = 64
CHUNK_ROWS = 64 * 256  # rows of a [rows, taps, channels] view turned into fp64 at a time (no fp64 copy of a whole tensor)

# (tensor rel-L2, worst-block rel-L2) per conv mode.  Basis:
#  - f16x2: 1e-6 is the bound test_f16x2_accuracy_against_fp64 applies; the line's measured figure is 1.4e-7.  The
#    block bound leaves 4x for a 64 x 64 block's own spread around the tensor figure.
#  - f32 (exact-fp32 kernels): 3e-6 is what test_f16x2_per_layer_against_exact_f32_on_a_pretrained_like_state allows
#    between the two modes; block bound 4x as above.
#  For scale: one missing limb product (x_lo * w_hi) is ~5e-4 relative L2, one dropped 32-channel K-step >= 1e-2.
BOUNDS = {"f16x2": (1e-6, 4e-6), "f32": (3e-6, 1.2e-5)}


def chain_bounds(mode, chain):
    """BOUNDS for a launch whose fp32 accumulators run `chain` dependent K-steps (a weight-gradient workgroup's pixel range,
    32 pixels a step): the rounding of a chain of random-sign partial sums grows as sqrt(chain) -- about u * sqrt(chain / 6)
    to u * sqrt(chain / 3), u = 2^-24, relative to the result -- so the bound is u * sqrt(chain) where that exceeds BOUNDS
    (chains past ~280 K-steps); blocks 4x as above.  Measured on the MI355X, "f16x2" weight gradients follow
    0.6 * u * sqrt(chain) to 2 %: 524 steps (layer4 downsample, 8 images) 8.25e-7, 1036 steps (the same at 1024x2048, 4
    images) 1.17e-6, 2046 steps (the split floor) 1.66e-6.  A missing slab, limb product or K-step is >= 5e-4."""
    t = max(BOUNDS[mode][0], 2.0 ** -24 * math.sqrt(chain))
    return t, max(BOUNDS[mode][1], 4.0 * t)


def out_size(n, k, stride, dil, pad):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _tap_slices(Ho, Wo, r, s, stride, dil):
    """The window of tap (r, s) in the zero-padded input (used for the coverage masks)."""
    return (slice(r * dil, r * dil + stride * (Ho - 1) + 1, stride), slice(s * dil, s * dil + stride * (Wo - 1) + 1, stride))


def _live(n_in, n_out, t, stride, dil, pad):
    """(output slice, input slice) of tap offset t along one axis: the output positions whose input position
    o * stride + t * dil - pad lies inside [0, n_in), or None when there is none (the tap sees padding only)."""
    off = t * dil - pad
    lo = max(0, -(-(-off) // stride))            # first o with o * stride + off >= 0
    hi = min(n_out, (n_in - 1 - off) // stride + 1) if n_in - 1 - off >= 0 else 0
    if lo >= hi:
        return None
    first = lo * stride + off
    return slice(lo, hi), slice(first, first + stride * (hi - lo - 1) + 1, stride)


def _live_range(n_in, n_out, t, stride, dil, pad):
    """Does tap offset t (rows or columns) reach any input position?"""
    return _live(n_in, n_out, t, stride, dil, pad) is not None


def _taps(Hi, Wi, Ho, Wo, kh, kw, stride, dil, pad):
    """(r, s, output rows, output columns, input rows, input columns) of every tap that sees at least one input pixel.
    No padded copy of any operand is made: each tap reads and writes only its live window, one image at a time."""
    for r in range(kh):
        hr = _live(Hi, Ho, r, stride, dil, pad)
        for s in range(kw):
            wr = _live(Wi, Wo, s, stride, dil, pad)
            if hr is not None and wr is not None:
                yield r, s, hr[0], wr[0], hr[1], wr[1]


def conv_fwd(x, w, stride=1, dil=1, pad=0, bias=None):
    """y[B,Ho,Wo,Cout] in float64.  x NHWC, w OIHW (any float dtype, any device)."""
    B, Hi, Wi, Cin = x.shape
    Cout, _, kh, kw = w.shape
    Ho, Wo = out_size(Hi, kh, stride, dil, pad), out_size(Wi, kw, stride, dil, pad)
    w = w.double()
    y = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float64, device=x.device)
    for b in range(B):
        for r, s, oh, ow, ih, iw in _taps(Hi, Wi, Ho, Wo, kh, kw, stride, dil, pad):
            y[b, oh, ow] += torch.matmul(x[b, ih, iw].double(), w[:, :, r, s].t())
    if bias is not None:
        y += bias.double()
    return y


def conv_dgrad(dy, w, in_hw, stride=1, dil=1, pad=0):
    """dx[B,Hi,Wi,Cin] in float64 of the conv that maps in_hw -> dy's grid."""
    B, Ho, Wo, Cout = dy.shape
    _, Cin, kh, kw = w.shape
    Hi, Wi = in_hw
    w = w.double()
    dx = torch.zeros(B, Hi, Wi, Cin, dtype=torch.float64, device=dy.device)
    for b in range(B):
        for r, s, oh, ow, ih, iw in _taps(Hi, Wi, Ho, Wo, kh, kw, stride, dil, pad):
            dx[b, ih, iw] += torch.matmul(dy[b, oh, ow].double(), w[:, :, r, s])
    return dx


def conv_wgrad(x, dy, k, stride=1, dil=1, pad=0):
    """dw[Cout,Cin,k,k] in float64."""
    B, Hi, Wi, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    dw = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, device=x.device)
    for b in range(B):
        for r, s, oh, ow, ih, iw in _taps(Hi, Wi, Ho, Wo, k, k, stride, dil, pad):
            dw[:, :, r, s] += torch.matmul(dy[b, oh, ow].double().reshape(-1, Cout).t(), x[b, ih, iw].double().reshape(-1, Cin))
    return dw


def bias_grad(dy):
    return dy.double().reshape(-1, dy.shape[-1]).sum(0)


def channel_stats(y, with_abs=False):
    """[2, C]: per-channel sum and sum of squares of y (what the statistics partials add up to); with_abs: a third row,
    sum |y| (the error scale of a sum).  In float64, over row chunks."""
    yf = y.reshape(-1, y.shape[-1])
    out = torch.zeros(3 if with_abs else 2, y.shape[-1], dtype=torch.float64, device=y.device)
    for r0 in range(0, yf.shape[0], CHUNK_ROWS):
        c = yf[r0:r0 + CHUNK_ROWS].double()
        out[0] += c.sum(0)
        out[1] += (c * c).sum(0)
        if with_abs:
            out[2] += c.abs().sum(0)
    return out


# ----------------------------------------------------------------------------------- structure of the exact zeros
def dgrad_unreached(in_hw, k, stride, dil, pad, out_hw, device=None):
    """[Hi, Wi] bool: input pixels no tap of any output pixel reads (their data gradient is exactly 0)."""
    Hi, Wi = in_hw
    Ho, Wo = out_hw
    cov = torch.zeros(Hi + 2 * pad, Wi + 2 * pad, dtype=torch.bool, device=device)
    for r in range(k):
        for s in range(k):
            hs, ws = _tap_slices(Ho, Wo, r, s, stride, dil)
            cov[hs, ws] = True
    return ~cov[pad:pad + Hi, pad:pad + Wi]


def dead_taps(in_hw, k, stride, dil, pad):
    """[k, k] bool: taps whose window holds padding only (their weight gradient is exactly 0)."""
    Hi, Wi = in_hw
    Ho, Wo = out_size(Hi, k, stride, dil, pad), out_size(Wi, k, stride, dil, pad)
    rows = torch.tensor([_live_range(Hi, Ho, r, stride, dil, pad) for r in range(k)])
    cols = torch.tensor([_live_range(Wi, Wo, s, stride, dil, pad) for s in range(k)])
    return ~(rows[:, None] & cols[None, :])


# ----------------------------------------------------------------------------------------------- the comparator
def _as_rtc(t, kind):
    """[rows, taps, channels] view: activations [..., C] -> [M, 1, C]; weight gradients OIHW -> [Cout, taps, Cin]."""
    if kind == "wgrad":
        co, ci, kh, kw = t.shape
        return t.reshape(co, ci, kh * kw).permute(0, 2, 1)
    return t.reshape(-1, 1, t.shape[-1])  # (a view for a dense tensor; a channel slice is copied in its own dtype)


def _block_sums(got, ref, kind, scale_ref=None):
    """Per block [row blocks, taps, channel blocks]: sum of (got - ref)^2 and of ref^2, in float64, computed over row chunks
    so that no fp64 copy of a whole tensor is made.  scale_ref: a tensor of ref's shape whose squares take the place of ref's
    in the denominators -- the error scale of a result that is a cancelling sum (eval_conv_ref's `mag`)."""
    g3, r3 = _as_rtc(got, kind), _as_rtc(ref, kind)
    s3 = _as_rtc(scale_ref, kind) if scale_ref is not None else None
    R, T, C = r3.shape
    nr, nc = -(-R // BLOCK), -(-C // BLOCK)
    num = torch.zeros(nr, T, nc, dtype=torch.float64, device=ref.device)
    den = torch.zeros_like(num)
    pc = -C % BLOCK
    for r0 in range(0, R, CHUNK_ROWS):
        r1 = min(R, r0 + CHUNK_ROWS)
        rc = r3[r0:r1].to(torch.float64)
        d = g3[r0:r1].to(device=ref.device, dtype=torch.float64) - rc
        pr = -(r1 - r0) % BLOCK  # (only the last chunk has a partial block)

        def sums(t):
            t = F.pad(t * t, (0, pc, 0, 0, 0, pr))
            return t.reshape(t.shape[0] // BLOCK, BLOCK, T, (C + pc) // BLOCK, BLOCK).sum((1, 4))

        num[r0 // BLOCK:r0 // BLOCK + (r1 - r0 + pr) // BLOCK] = sums(d)
        dc = rc if s3 is None else s3[r0:r1].to(device=ref.device, dtype=torch.float64)
        den[r0 // BLOCK:r0 // BLOCK + (r1 - r0 + pr) // BLOCK] = sums(dc)
    return num, den


def block_rel_l2(got, ref, kind="act"):
    """Relative L2 per block: [row blocks, taps, channel blocks] (a block whose reference is exactly 0 scores 0 if it is
    0 as well, inf otherwise)."""
    num, den = _block_sums(got, ref, kind)
    return _ratio(num, den)


def _ratio(num, den):
    rel = torch.sqrt(num / den)
    return torch.where(den > 0, rel, torch.where(num > 0, torch.full_like(rel, float("inf")), torch.zeros_like(rel)))


def measure(got, ref, kind="act", scale_ref=None):
    """(tensor rel-L2, worst block rel-L2, (row block, tap, channel block) of the worst block); relative to `scale_ref`
    instead of `ref` where one is given (_block_sums)."""
    num, den = _block_sums(got, ref, kind, scale_ref)
    tensor = _ratio(num.sum(), den.sum()).item()  # (the tensor's squared norms are the sums of its blocks')
    blocks = _ratio(num, den)
    flat = int(blocks.reshape(-1).argmax())
    where = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), blocks.shape))
    return tensor, blocks.reshape(-1)[flat].item(), where


def exact_violations(got, want, mask=None):
    """Elements under `mask` (broadcast against got; None = all) where got != want bit for bit (-0.0 == 0.0)."""
    g = got.to(want.device) if torch.is_tensor(want) else got
    bad = g != want
    if mask is not None:
        bad = bad & mask.to(bad.device)
    return int(bad.sum())


def check(got, ref, mode, what, kind="act", exact=(), bounds=None, scale_ref=None):
    """Assert (a) and (b) against BOUNDS[mode] (or `bounds`, from chain_bounds) and every (c) in `exact`: pairs (want, mask)
    -- `got` must equal `want` (a tensor or a number) wherever `mask` is True.  Returns (tensor rel-L2, worst block rel-L2)
    for the report line.  scale_ref: the denominators' tensor where the error scale is not |ref| (_block_sums)."""
    bound_t, bound_b = bounds or BOUNDS[mode]
    t, b, where = measure(got, ref, kind, scale_ref)
    assert t <= bound_t, f"{what}: relative L2 {t:.3e} > {bound_t:.0e} (worst block {where}: {b:.3e})"
    assert b <= bound_b, f"{what}: worst block (row block, tap, channel block) {where} relative L2 {b:.3e} > {bound_b:.0e}"
    for want, mask in exact:
        n = exact_violations(got, want, mask)
        assert n == 0, f"{what}: {n} elements differ where the result is exact by structure"
    return t, b


def flagged(got, ref, mode, kind="act", exact=(), scale_ref=None):
    """True when `check` would fail (the teeth tests)."""
    try:
        check(got, ref, mode, "probe", kind, exact, scale_ref=scale_ref)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------- "f16x2" limb split
def limb_split(t, limb2_scale=2048.0, amax=None):
    """(hi, lo) with t == hi + lo as the library splits a tensor into two f16 limbs of t * 2^e, e = 15 - exponent of
    max|t| (ops.limbs.materialize undoes the same split; the second limb is stored times limb2_scale).  amax: the split
    uses the scale of that bound instead of max|t| -- planes written under an a-priori bound (the eval-mode conv epilogue)."""
    t = t.double()
    amax = t.abs().max() if amax is None else torch.as_tensor(amax, dtype=torch.float64)
    e = 15 - int(torch.frexp(amax.float())[1]) if 0 < amax < 3e38 else 0
    xs = t * 2.0 ** e
    hi = xs.half().double()
    lo = ((xs - hi) * limb2_scale).half().double() / limb2_scale
    return hi * 2.0 ** -e, lo * 2.0 ** -e


# ------------------------------------------------------------------ the eval-mode epilogue that writes limb planes
def eval_conv_ref(x, w, scale, shift, res=None, relu=False, stride=1, dil=1, pad=0, conv=None):
    """(y, mag) in float64 of conv + folded BatchNorm [+ residual] [+ ReLU] (onda_conv2d_fwd_l2_limbs):
    y = relu?(conv_fwd(x, w) * scale + shift [+ res]) and, per element and before the ReLU,
    mag = |conv * scale| + |shift| [+ |res|] -- y is a sum that cancels and is then clipped, so no bound relative to |y|
    holds; the error scale is the size of its terms (check(..., scale_ref=mag)).  x and res are the operands the kernel
    received (the materialized limb planes), w / scale / shift the fp32 originals.  conv: conv_fwd(x, w, stride, dil, pad)
    where the caller has it already (several epilogues of one geometry); it is left unchanged."""
    y = (conv_fwd(x, w, stride, dil, pad) if conv is None else conv) * scale.double()
    mag = y.abs() + shift.double().abs()
    y += shift.double()
    if res is not None:
        y += res.double()
        mag += res.double().abs()
    return (y.clamp_min(0) if relu else y), mag


def fold_bounds_ref(w, scale, shift):
    """ops.fold_bounds from its definition, as two python floats from float64: max_c |scale_c| * sum_k |w_ck|, max_c |shift_c|."""
    l1 = w.double().abs().sum(dim=(1, 2, 3))
    return (scale.double().abs() * l1).max().item(), shift.double().abs().max().item()


def limb_out_bound_ref(xtrue, kb, res_true=None):
    """The a-priori bound the limb-writing epilogue scales its planes by (conv_l2.hip limb_out_bound), in float64:
    (max|x| * kb[0] + kb[1] [+ max|res|]) * 1.0001."""
    return (float(xtrue) * kb[0] + kb[1] + (float(res_true) if res_true is not None else 0.0)) * 1.0001


# ------------------------------------------------------------------------------------------------ schedule edges
def _G():
    """Resident workgroups of the conv kernels (what the schedules count rounds in: onda_conv_ws_floats = 3 tiles each)."""
    from onda_amd._lib import query
    return query("onda_conv_ws_floats") // (3 * 128 * 128)


def _schedule(M, cout, taps, cin):
    """(kernel id, balanced, tiles mod G, G).  The kernel id, its tile height and whether the schedule is balanced (statistic
    rows past ceil(M / BM): stream-K pieces) come from the library's queries; the remainder is this test's own arithmetic
    over the tile shape the library reported -- it checks that a case was BUILT with the remainder its label names, it does
    not come from the library."""
    from onda_amd._lib import query
    rows = ctypes.c_int(0)
    total = query("onda_conv_l2_tiles_m_split", M, cout, taps, cin, 0, 0, ctypes.byref(rows))
    kid = query("onda_conv_l2_kernel_id", M, cout, taps, cin)
    BM, BN = {0: (256, 128), 1: (128, 128), 2: (256, 64), 3: (256, 128)}[kid]
    assert rows.value == BM
    tiles = -(-M // BM) * -(-cout // BN)
    G = _G() // 2 if BM * BN == 256 * 128 else _G()
    return kid, total > -(-M // BM), tiles % G, G


def _edge_geometries():
    """(label, geometry row, expected kernel id [library], expected balanced [library], remainder the case is built with
    [construction check, see _schedule] or None), built from G."""
    R = _G()
    G0 = R // 2  # 256 x 128 tiles: one workgroup per CU
    mk = lambda name, H, W, cin, cout, k, dil=1: (name, H, W, cin, cout, k, 1, dil, dil * (k // 2), False, 0, 0, False, False)
    return [
        ("256x128, whole rounds (tiles = G)", mk("e.256x128.exact", 64, 4 * G0, 128, 128, 3), 0, False, 0),
        ("256x128, remainder 1 (tiles = G + 1), stream-K", mk("e.256x128.rem1", 64, 4 * G0 + 4, 128, 128, 3), 0, True, 1),
        ("128x128 balanced (stream-K)", mk("e.128x128.sk", 50, 256, 256, 128, 3), 1, True, None),
        ("256x64 balanced (stream-K)", mk("e.256x64.sk", 100, 256, 256, 64, 3), 2, True, None),
        ("256x128 long K, not balanced (remainder G - 1)", mk("e.256x128.longk", 2 * G0 - 1, 256, 512, 128, 3), 0, False, G0 - 1),
        ("continuous stream, whole rounds", mk("e.l2x.exact", G0 // 2, 256, 512, 256, 1), 3, False, 0),
        ("continuous stream, remainder", mk("e.l2x.rem", G0 // 2 + 1, 256, 512, 256, 1), 3, None, 2),
    ]
