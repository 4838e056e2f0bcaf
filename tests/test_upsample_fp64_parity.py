"""The bilinear upsample and the fused upsample / cross-entropy head (csrc/pointwise.hip: onda_upsample_fwd / _bwd,
onda_upsample_argmax / _argmax_hist, onda_upsample_ce_fwd / _bwd) held to the fp64 reference of tests/upsample_fp64.py at
non-integer ratios, through the entry points the model uses (ops.UpsampleFn, upsample_ce, upsample_argmax,
upsample_argmax_hist), with the comparator that cannot dilute a fault at a block seam or an image edge.  The shape table,
the bounds and their basis are in upsample_fp64; test_upsample_fp64_reference.py proves reference and comparator on the
CPU."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upsample_fp64 as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ref.CASES
FUSED = [c for c in CASES if c[4] <= 32]
ids = ref.case_id
SENTINEL = 7.0


def head_out(logits_nchw, ldl):
    """CPU logits [B,K,h,w] on the device in the model's own output layout: a [B,K,h,w] view of pixel-major rows of ldl
    floats (the padding columns hold zeros, as the head's padded GEMM leaves them)."""
    B, K, h, w = logits_nchw.shape
    pad = torch.zeros(B, h, w, ldl)
    pad[..., :K] = logits_nchw.permute(0, 2, 3, 1)
    return pad.to(DEV)[..., :K].permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def expected(case):
    """The fp64 reference of a case, computed once and left unchanged."""
    h, w, H, W, K, ldl = case
    x, lab = ref.inputs(case)
    gy = ref.upstream_gradient(case)
    up64 = ref.upsample(x, H, W)
    e = dict(x=x, lab=lab, gy=gy, up64=up64, dx64=ref.upsample_grad(gy, h, w))
    e["cls"], margin, norm = ref.class_map(up64)
    e["decided"] = ref.decided(margin, norm)
    if K <= 32:
        e["v64"], e["g64"], e["n"] = ref.head_ce(x, lab, 2.5)
    return e


def pad_mask(K, ldl):
    return (torch.arange(ldl) >= K).expand(1, 1, 1, ldl)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_upsample_fn_forward_and_backward(case):
    from onda_amd import _lib, ops
    from onda_amd.ops.core import _p, _stream
    h, w, H, W, K, ldl = case
    e = expected(case)
    out = head_out(e["x"], ldl).detach().requires_grad_(True)
    assert ops.logits_rows(out)[1] == ldl  # read in place, with this row stride
    up = ops.UpsampleFn.apply(out, (H, W))
    exact = [(up, e["x"], None)] if (h, w) == (H, W) else []  # the identity reproduces its input bit for bit
    ref.check(up, e["up64"], "fwd", ids(case) + " UpsampleFn forward", exact)
    up.backward(e["gy"].to(DEV))
    # onda_upsample_bwd writes the K class columns only: the rest of a prefilled buffer keeps its sentinel
    dup = e["gy"].to(DEV).contiguous()
    dl = torch.full((ref.BATCH, h, w, ldl), SENTINEL, device=DEV)
    _lib.call("onda_upsample_bwd", _p(dup), _p(dl), ldl, ref.BATCH, h, w, K, H, W, _stream())
    exact = [(dl, SENTINEL, pad_mask(K, ldl))]
    if (h, w) == (H, W):
        exact.append((out.grad, e["gy"], None))
    ref.check(out.grad, e["dx64"], "grad", ids(case) + " UpsampleFn backward", exact)
    assert torch.equal(dl[..., :K].permute(0, 3, 1, 2), out.grad)


@pytest.mark.parametrize("case", FUSED, ids=ids)
def test_upsample_ce_value_and_gradient(case):
    from onda_amd import _lib, ops
    from onda_amd.ops.core import _p, _stream
    h, w, H, W, K, ldl = case
    e = expected(case)
    lab = e["lab"].to(DEV)
    runs = []
    for _ in range(2):
        out = head_out(e["x"], ldl).detach().requires_grad_(True)
        loss = ops.upsample_ce(out, lab)
        (2.5 * loss).backward()
        runs.append((loss.detach().cpu(), out.grad.cpu()))
    value = float(runs[0][0])
    rel = abs(value - e["v64"]) / abs(e["v64"])
    print(f"{ids(case)} CE value {value!r} vs {e['v64']!r}: relative {rel:.3e} (bound {ref.CE_VALUE_BOUND:.1e})")
    assert rel <= ref.CE_VALUE_BOUND
    # the padded columns of the kernel's own output buffer are exact zeros, over a sentinel
    rows = ops.logits_rows(out.detach())[0]
    result = torch.empty(2, device=DEV)
    ws = torch.empty(_lib.query("onda_upsample_ce_ws", ref.BATCH, H, W), device=DEV)
    _lib.call("onda_upsample_ce_fwd", _p(rows), ldl, _p(lab), _p(result), _p(ws), ref.BATCH, h, w, K, H, W, _stream())
    assert result[1].item() == e["n"] == int((e["lab"] < K).sum())
    assert result[0].item() == value
    dl = torch.full((ref.BATCH, h, w, ldl), SENTINEL, device=DEV)
    ws = torch.empty(_lib.query("onda_upsample_ce_bwd_ws", ref.BATCH, w, K, H), device=DEV)
    gscale = torch.full((1,), 2.5, device=DEV)
    _lib.call("onda_upsample_ce_bwd", _p(rows), ldl, _p(lab), _p(result), _p(gscale), 1.0, _p(dl), _p(ws), ref.BATCH, h, w, K,
              H, W, _stream())
    ref.check(runs[0][1], e["g64"], "ce_grad", ids(case) + " d 2.5 * loss / d logits", [(dl, 0.0, pad_mask(K, ldl))])
    assert torch.equal(dl[..., :K].permute(0, 3, 1, 2).cpu(), runs[0][1])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"


def test_upsample_ce_everything_ignored():
    """No kept label (255, or any value >= K): the value is NaN, not an error, and the gradient exact zeros."""
    from onda_amd import ops
    case = CASES[0]
    h, w, H, W, K, ldl = case
    e = expected(case)
    for fill in (255, K):
        out = head_out(e["x"], ldl).detach().requires_grad_(True)
        loss = ops.upsample_ce(out, torch.full_like(e["lab"], fill).to(DEV))
        (2.5 * loss).backward()
        assert torch.isnan(loss).item()
        assert ref.exact_violations(out.grad, 0.0) == 0


@pytest.mark.parametrize("case", CASES + [ref.HIST_GLOBAL_CASE], ids=ids)
def test_upsample_argmax_and_confusion_matrix(case):
    """The class map equals the fp64 one wherever the fp64 top-2 margin exceeds what a forward within its bound can turn
    (upsample_fp64.decided, at most 1e-3 of the pixels left out); the confusion matrix is accumulated INTO `hist`, equals
    fast_hist of the kernel's own class map, equals the fp64 confusion matrix over the decided pixels, and its row sums
    are the per-class counts of the kept labels.  K <= 32 counts in LDS, K = 40 by global atomics."""
    from onda_amd import ops
    from onda_amd.framework.utils.func import fast_hist
    h, w, H, W, K, ldl = case
    e = expected(case)
    ok = e["decided"]
    assert 1.0 - ok.double().mean().item() <= ref.UNDECIDED_CAP
    out = head_out(e["x"], ldl)
    cls = ops.upsample_argmax(out, (H, W)).cpu().long()
    wrong = int((cls != e["cls"])[ok].sum())
    assert wrong == 0, f"{wrong} decided pixels differ from the fp64 class map"
    hist = torch.arange(K * K, dtype=torch.int64).reshape(K, K).to(DEV)
    before = hist.cpu().clone()
    ops.upsample_argmax_hist(out, e["lab"].to(DEV), hist, K)
    got = hist.cpu() - before
    lab = e["lab"].numpy().astype(np.int64)
    want = fast_hist(lab.flatten(), cls.numpy().flatten(), K)
    assert np.array_equal(got.numpy(), want.astype(np.int64))
    keep = ok.numpy()
    assert np.array_equal(fast_hist(lab[keep], cls.numpy()[keep], K).astype(np.int64), ref.confusion(e["lab"], e["cls"], K, ok).numpy())
    assert torch.equal(got.sum(1), torch.bincount(e["lab"].reshape(-1).long(), minlength=256)[:K])


def test_upsample_ce_past_the_fused_backward():
    """2x3 -> 3x1001 (500x along x): one low-resolution column's output span does not fit the fused backward's row pass
    (it takes up to ~211x).  ops.upsample_ce takes the unfused route there -- UpsampleFn, then torch's cross-entropy --
    so the shape trains: value and gradient against the reference, same label contract."""
    from onda_amd import _lib, ops
    case = ref.PAST_FUSED_CASE
    h, w, H, W, K, ldl = case
    assert not _lib.query("onda_upsample_ce_fused", w, W) and _lib.query("onda_upsample_ce_fused", 129, 1024)
    x, lab = ref.inputs(case, 1)
    v64, g64, n = ref.head_ce(x, lab, 2.5)
    out = head_out(x, ldl).detach().requires_grad_(True)
    loss = ops.upsample_ce(out, lab.to(DEV))
    (2.5 * loss).backward()
    rel = abs(float(loss) - v64) / abs(v64)
    print(f"{ids(case)} CE value {float(loss)!r} vs {v64!r}: relative {rel:.3e}")
    assert rel <= ref.CE_VALUE_BOUND and 0 < n < lab.numel()
    ref.check(out.grad, g64, "ce_grad", ids(case) + " d 2.5 * loss / d logits")
    out = head_out(x, ldl).detach().requires_grad_(True)
    loss = ops.upsample_ce(out, torch.full_like(lab, 255).to(DEV))
    loss.backward()
    assert torch.isnan(loss).item() and ref.exact_violations(out.grad, 0.0) == 0
