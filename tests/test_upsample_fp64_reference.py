"""The fp64 upsample / fused-CE reference and the comparator of tests/upsample_fp64.py, proven on the CPU before the GPU
parity tests (test_upsample_fp64_parity.py) lean on them: fp32 ATen passes the comparator at every entry of the shape table
within the floor-derived bounds, and the comparator flags each fault a kernel could make quietly -- most of which the
tensor-max criterion of test_hip_kernels.close lets through at its current tolerances (2e-4 for the CE gradient, 2e-5 for
the upsample gradient, 2e-6 for the forward)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upsample_fp64 as ref  # noqa: E402

CASES = ref.CASES
NON_IDENTITY = [c for c in CASES if c[:2] != c[2:4]]
SEAM_CASES = [c for c in CASES if c[1] > ref.CW[c[:4]] and c[3] > c[1]]  # more than one pass-A block, upsampling
ids = ref.case_id
_cache = {}


def aten(case):
    """fp32 ATen on the CPU and the fp64 reference of a case, computed once: the upsample and its gradient under a random
    upstream gradient, the head's value and the gradient of 2.5 * value."""
    if case not in _cache:
        h, w, H, W, K, ldl = case
        x, lab = ref.inputs(case)
        gy = ref.upstream_gradient(case)
        lo = x.clone().requires_grad_(True)
        up = ref.aten_upsample(lo, H, W)
        up.backward(gy)
        v32, g32, gup32 = ref.aten_head_ce(x, lab, 2.5)
        v64, g64, n = ref.head_ce(x, lab, 2.5)
        _cache[case] = dict(x=x, lab=lab, gy=gy, up32=up.detach(), up64=ref.upsample(x, H, W), dx32=lo.grad,
                            dx64=ref.upsample_grad(gy, h, w), v32=v32, v64=v64, g32=g32, g64=g64, gup32=gup32, n=n)
    return _cache[case]


def padded(grad, ldl):
    """A [B,K,h,w] gradient as the [B,h,w,ldl] buffer the backward kernels write (padding columns zero)."""
    B, K, h, w = grad.shape
    buf = torch.zeros(B, h, w, ldl)
    buf[..., :K] = grad.permute(0, 2, 3, 1)
    return buf


def pad_mask(K, ldl):
    return (torch.arange(ldl) >= K).expand(1, 1, 1, ldl)


# ----------------------------------------------------------------------------------------------- reference vs ATen
def test_axis_matrix_is_atens_rule():
    for n_in, n_out in ((17, 1021), (129, 1024), (65, 34), (7, 7), (3, 1001)):
        m = ref.axis_matrix(n_in, n_out)
        assert m.dtype == torch.float64 and m.shape == (n_out, n_in)
        assert int((m != 0).sum(1).max()) <= 2 and float((m.sum(1) - 1).abs().max()) <= 2.0 ** -23
        assert m[0, 0] == 1.0
        # a ramp is reproduced to fp32 rounding of the source coordinate: the matrix interpolates where ATen does
        ramp = m @ torch.arange(n_in, dtype=torch.float64)
        exact = torch.arange(n_out, dtype=torch.float64) * (n_in - 1) / (n_out - 1)
        assert float((ramp - exact).abs().max()) <= 2.0 ** -23 * n_in
    assert torch.equal(ref.axis_matrix(7, 7), torch.eye(7, dtype=torch.float64))


@pytest.mark.parametrize("case", CASES + [ref.HIST_GLOBAL_CASE], ids=ids)
def test_fp32_aten_passes_the_comparator(case):
    """Values and gradients of fp32 ATen against the reference at every entry of the table, within BOUNDS (the CPU floor
    in upsample_fp64's docstring is the worst figure this test prints)."""
    h, w, H, W, K, ldl = case
    if K > 32:  # the confusion-matrix entry: the fused head does not take it
        x = ref.inputs(case)[0]
        ref.check(ref.aten_upsample(x, H, W), ref.upsample(x, H, W), "fwd", ids(case) + " fwd")
        return
    a = aten(case)
    ref.check(a["up32"], a["up64"], "fwd", ids(case) + " fwd")
    ref.check(a["dx32"], a["dx64"], "grad", ids(case) + " upsample gradient")
    ref.check(a["g32"], a["g64"], "ce_grad", ids(case) + " CE gradient",
              exact=[(padded(a["g32"], ldl), 0.0, pad_mask(K, ldl))])
    rel = abs(a["v32"] - a["v64"]) / abs(a["v64"])
    print(f"{ids(case)} CE value: {a['v32']!r} vs {a['v64']!r}, relative {rel:.3e} (bound {ref.CE_VALUE_BOUND:.1e})")
    assert rel <= ref.CE_VALUE_BOUND
    assert a["n"] == int((a["lab"] < K).sum()) and 0 < a["n"] < a["lab"].numel()
    if (h, w) == (H, W):  # the identity is exact by structure
        assert torch.equal(a["up64"], a["x"].double()) and torch.equal(a["up32"], a["x"])
        assert torch.equal(a["dx64"], a["gy"].double())


def test_fp32_aten_passes_the_comparator_past_the_fused_backward():
    """The 500x shape ops.upsample_ce routes around the fused head (batch 1) keeps to the same bounds."""
    case = ref.PAST_FUSED_CASE
    x, lab = ref.inputs(case, 1)
    v32, g32, _ = ref.aten_head_ce(x, lab, 2.5)
    v64, g64, n = ref.head_ce(x, lab, 2.5)
    ref.check(g32, g64, "ce_grad", ids(case) + " CE gradient")
    assert abs(v32 - v64) <= ref.CE_VALUE_BOUND * abs(v64) and 0 < n < lab.numel()


def test_all_ignored_is_nan_and_exact_zeros():
    x, lab = ref.inputs(CASES[0])
    for fill in (255, 19, 200):
        v, g, n = ref.head_ce(x, torch.full_like(lab, fill), 2.5)
        assert v != v and n == 0 and g.dtype == torch.float64 and not g.any()
    v32, g32, _ = ref.aten_head_ce(x, torch.full_like(lab, 255), 2.5)
    assert v32 != v32 and not g32.any()  # (torch's own nll_loss backward gives zeros, not NaN)


def test_labels_at_or_above_K_are_ignored():
    case = CASES[0]
    x, lab = ref.inputs(case)
    assert int(((lab >= case[4]) & (lab < 255)).sum()) >= 1 and bool((lab[0, case[2] // 2] == 255).all())
    folded = lab.clone()
    folded[folded >= case[4]] = 255
    a, b = ref.head_ce(x, lab), ref.head_ce(x, folded)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("case", CASES + [ref.HIST_GLOBAL_CASE], ids=ids)
def test_seeds_keep_the_undecided_share_within_the_cap(case):
    """upsample_argmax is compared where the fp64 top-2 margin exceeds the derived margin (upsample_fp64.decided); the
    seeds must leave at most UNDECIDED_CAP of the pixels out -- a condition on the seed, not on the kernel."""
    h, w, H, W, K, ldl = case
    x, lab = ref.inputs(case)
    cls, margin, norm = ref.class_map(ref.upsample(x, H, W))
    ok = ref.decided(margin, norm)
    assert 1.0 - ok.double().mean().item() <= ref.UNDECIDED_CAP
    assert torch.equal(ref.aten_upsample(x, H, W).argmax(1)[ok], cls[ok])
    # the fp64 confusion matrix counts every kept label once
    assert torch.equal(ref.confusion(lab, cls, K).sum(1), torch.bincount(lab.reshape(-1).long(), minlength=256)[:K])


# ----------------------------------------------------------------------------------------------- the shape table
def _contributors(n_in, n_out):
    """Per source index: (lowest, highest) destination index with a non-zero weight on it, or None."""
    m = ref.axis_matrix(n_in, n_out)
    out = []
    for x in range(n_in):
        nz = torch.nonzero(m[:, x])[:, 0]
        out.append((int(nz[0]), int(nz[-1])) if len(nz) else None)
    return m, out


def _fractional(n_in, n_out):
    return (n_out - 1) % (n_in - 1) != 0 and (n_in - 1) % (n_out - 1) != 0


@pytest.mark.parametrize("case", NON_IDENTITY, ids=ids)
def test_no_integer_ratio_in_the_table(case):
    """At an integer ratio every gather range of the backward kernels ends on a destination pixel whose source fraction is
    exactly 0 (floor((x - 1) / s) and ceil((x + 1) / s) are hit exactly).  One entry is such a shape, 3x5 -> 7x801 (200x
    and 3x: upsample_fp64.INTEGER_RATIO); it stays for its one-column blocks, and 4x5 -> 9x802 repeats it at non-integer
    ratios.  Every other entry has a non-integer ratio along x, the axis of pass A's A0 / A1 and X0 / X1, except
    5x7 -> 11x13 (one block), which has it along y; the entries with h = 3 (H = 5, 7) are integer along y, so Y0 / Y1 of
    pass B rest on 4 -> 9, 5 -> 11 and 9 -> 6 (test_the_table_covers_both_axes).  Along every non-integer axis: the destination pixel at floor((x - 1) / s) has a
    fraction strictly between 0 and 1 for some x, and so has the one at ceil((x + 1) / s); and the outermost destination
    pixel that contributes to a source index carries a weight strictly between 0 and 1 at every end that is not the image
    border itself -- dropping it changes the result."""
    h, w, H, W = case[:4]
    if case in ref.INTEGER_RATIO:
        assert not _fractional(h, H) and not _fractional(w, W)
        return
    assert _fractional(h, H) or _fractional(w, W)
    assert _fractional(w, W) or ref.CW[case[:4]] >= w  # (an integer ratio along x only where pass A has one block)
    for n_in, n_out in ((h, H), (w, W)):
        if not _fractional(n_in, n_out):
            continue
        src = ref.axis_taps(n_in, n_out)[0].double()
        frac = src - src.floor()
        inv = (n_out - 1) / (n_in - 1)
        lo_ends = [int((x - 1) * inv) for x in range(1, n_in)]
        hi_ends = [min(n_out - 1, -int(-(x + 1) * inv // 1)) for x in range(n_in - 1)]
        assert any(0 < frac[e] < 1 for e in lo_ends) and any(0 < frac[e] < 1 for e in hi_ends)
        m, ends = _contributors(n_in, n_out)
        for x, e in enumerate(ends):
            for X in (e or ()):
                if X not in (0, n_out - 1):
                    assert 0 < m[X, x] < 1


def test_the_table_covers_both_axes():
    """A non-integer ratio along y both ways (up and down), and along x at every entry with more than one pass-A block."""
    assert any(_fractional(c[0], c[2]) and c[2] > c[0] for c in CASES) and any(_fractional(c[0], c[2]) and c[2] < c[0] for c in CASES)
    assert len(SEAM_CASES) >= 4 and all(_fractional(c[1], c[3]) for c in CASES if c[1] > ref.CW[c[:4]] and c not in ref.INTEGER_RATIO)
    for c in CASES:  # the documented block width is the host formula's
        sx = (torch.ones((), dtype=torch.float32) * (c[1] - 1)) / (torch.ones((), dtype=torch.float32) * (c[3] - 1))
        assert ref.CW[c[:4]] == min(64, int(torch.ones((), dtype=torch.float32) * 634 * sx) - 2)


# ----------------------------------------------------------------------------------------------- injected faults
def _drop_column(a, case, x, side):
    """The CE gradient of fp32 ATen with low-resolution column x computed without its outermost (side 0: lowest,
    1: highest) contributing output column."""
    h, w, H, W, K, ldl = case
    my = ref.axis_matrix(h, H)
    mx, ends = _contributors(w, W)
    X = ends[x][side]
    bad = a["g32"].clone()
    bad[:, :, :, x] -= (torch.einsum("Yy,bkY->bky", my, a["gup32"][:, :, :, X].double()) * mx[X, x]).float()
    return bad


def _drop_row(a, case, y, side):
    h, w, H, W, K, ldl = case
    mx = ref.axis_matrix(w, W)
    my, ends = _contributors(h, H)
    Y = ends[y][side]
    bad = a["g32"].clone()
    bad[:, :, y, :] -= (torch.einsum("bkX,Xx->bkx", a["gup32"][:, :, Y, :].double(), mx) * my[Y, y]).float()
    return bad


def _seam_columns(case):
    cw, w = ref.CW[case[:4]], case[1]
    out = []
    for xb in range(cw, w, cw):
        out += [(xb, 0), (xb - 1, 1)]  # the first column of a block misses its lowest tap, the last of the one before its highest
    return out[:2] + out[-2:] if len(out) > 4 else out


@pytest.mark.parametrize("case", SEAM_CASES, ids=ids)
def test_fault_i_seam_column_without_its_outermost_tap(case):
    """(i) Flagged by criterion (b) at every seam, 1e-4 .. 2e-2 against a bound of 5e-6.  The old close(..., 2e-4) passes it
    at the large ratios (3x17 -> 7x1021, 3x5 -> 7x801, 4x5 -> 9x802: the dropped tap is one of >= 128 of the column); at
    3x129 -> 5x1024 and 4x23 -> 9x701 (16 and 64 taps a column) the old criterion sees it as well: not asserted there."""
    a = aten(case)
    for x, side in _seam_columns(case):
        bad = _drop_column(a, case, x, side)
        t, g, where = ref.measure(bad, a["g64"], "grad")
        print(f"{ids(case)} column {x} side {side}: tensor {t:.2e}, worst group {g:.2e} at {where}, "
              f"old close passes: {ref.old_close(bad, a['g32'], 2e-4)}")
        assert g > ref.BOUNDS["ce_grad"][1] and ref.flagged(bad, a["g64"], "ce_grad")
        if case[3] > 60 * case[1]:
            assert ref.old_close(bad, a["g32"], 2e-4)


@pytest.mark.parametrize("case", NON_IDENTITY, ids=ids)
def test_fault_ii_edge_row_without_its_outermost_tap(case):
    """(ii) The first low-resolution row without its highest contributing output row, the last without its lowest: flagged
    at every shape.  The rows of the table are short (H / h <= 3: the dropped row is one of two or three that reach the edge
    row), so this fault is 6e-2 .. 5e-1 of the tensor and the old close(..., 2e-4) sees it as well: not asserted."""
    h, w, H, W, K, ldl = case
    a = aten(case)
    for y, side in ((0, 1), (h - 1, 0)):
        bad = _drop_row(a, case, y, side)
        t, g, where = ref.measure(bad, a["g64"], "grad")
        print(f"{ids(case)} row {y}: tensor {t:.2e}, worst group {g:.2e} at {where}, "
              f"old close passes: {ref.old_close(bad, a['g32'], 2e-4)}")
        assert ref.flagged(bad, a["g64"], "ce_grad")


@pytest.mark.parametrize("case", NON_IDENTITY, ids=ids)
def test_fault_iii_one_pixel_interpolated_without_its_right_neighbour(case):
    """(iii) One output pixel's K-vector with i1 = i0 away from the edge: flagged by criterion (b), the pixel group.  One
    pixel out of thousands moves the tensor's relative L2 by little, but its own K-vector by a fraction of itself -- which
    the old close(..., 2e-6) sees as well (the error is a fraction of a logit against a maximum of ~ 10): not asserted."""
    h, w, H, W, K, ldl = case
    a = aten(case)
    _, i0, i1, l0, l1 = ref.axis_taps(w, W)
    X = int(torch.nonzero((i1 > i0) & (l1 > 0.25) & (l1 < 0.75))[0, 0])
    Y, b = H // 2, ref.BATCH - 1
    bad = a["up32"].clone()
    bad[b, :, Y, X] = (ref.axis_matrix(h, H)[Y] @ a["x"][b, :, :, int(i0[X])].double().T).float()
    t, g, where = ref.measure(bad, a["up64"], "up")
    print(f"{ids(case)} pixel ({b}, {Y}, {X}): tensor {t:.2e}, worst group {g:.2e} at {where}")
    assert where == f"pixel (b, y, x) = ({b}, {Y}, {X})" and ref.flagged(bad, a["up64"], "fwd")


@pytest.mark.parametrize("case", [c for c in CASES if c[5] > c[4]], ids=ids)
def test_fault_iv_a_padded_column_that_is_not_zero(case):
    """(iv) 1e-30 in one padded class column: only the exact check (c) can see it; the old criterion passes."""
    h, w, H, W, K, ldl = case
    a = aten(case)
    buf = padded(a["g32"], ldl)
    exact = [(buf, 0.0, pad_mask(K, ldl))]
    assert not ref.flagged(a["g32"], a["g64"], "ce_grad", exact)
    bad = buf.clone()
    bad[ref.BATCH - 1, h - 1, w // 2, ldl - 1] = 1e-30
    assert ref.flagged(a["g32"], a["g64"], "ce_grad", [(bad, 0.0, pad_mask(K, ldl))])
    assert ref.old_close(bad, buf, 2e-4)


@pytest.mark.parametrize("case", [c for c in CASES if c[4] <= 32], ids=ids)
def test_fault_v_normaliser_off_by_one_pixel(case):
    """(v) The gradient scaled by n / (n + 1): flagged by criterion (a) at every shape.  The old close(..., 2e-4) passes
    it where 1 / (n + 1) < 2e-4, the shapes of more than 5000 kept labels; at the small shapes (n of 44 .. 327) it sees
    the fault too: not asserted there."""
    a = aten(case)
    bad = a["g32"] * (a["n"] / (a["n"] + 1.0))
    assert ref.flagged(bad, a["g64"], "ce_grad")
    if a["n"] > 5000:
        assert ref.old_close(bad, a["g32"], 2e-4)
