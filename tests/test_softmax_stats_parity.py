"""GPU: softmax_stats_kernel (csrc/loss_proto.hip) through ops.softmax_stats against the float64 standard and the bounds of
tests/softmax_stats_fp64.py -- block edges, K = 2 and 32, odd row strides, argmax ties, saturated rows, -inf logits, the
null-pointer variants and NaN in the padding columns.  Every test prints its figures before it asserts."""
import itertools

import pytest
import torch

import softmax_stats_fp64 as F

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _rows(x, ld, pad=0.0):
    """CPU logits [N, K] as the model lays them out: pixel-major rows of `ld` floats (padding columns: `pad`), seen as the
    NCHW view [1, K, 1, N] ops.softmax_stats is given.  The wrapper must take the rows as they are, not copy them."""
    from onda_amd.ops.loss import logits_rows
    N, K = x.shape
    buf = torch.full((1, 1, N, ld), pad)
    buf[0, 0, :, :K] = x
    buf = buf.to(DEV)
    out = buf[..., :K].permute(0, 3, 1, 2)
    rows, got_ld, n, k = logits_rows(out)
    assert rows.data_ptr() == buf.data_ptr() and (got_ld, n, k) == (ld, N, K)
    return out


def _run(case, kind, want_probs=True, want_argmax=True, pad=0.0):
    from onda_amd import ops
    N, K, ld = case
    conf, probs, am = ops.softmax_stats(_rows(F.inputs(case, kind), ld, pad), want_probs, want_argmax)
    assert conf.dtype == torch.float32 and conf.dim() == 0
    assert (probs is None) == (not want_probs) and (am is None) == (not want_argmax)
    if probs is not None:
        assert probs.dtype == torch.float32 and tuple(probs.shape) == (N, K) and probs.is_contiguous()
    if am is not None:
        assert am.dtype == torch.int32 and tuple(am.shape) == (N,)
    return probs, conf, am


@pytest.mark.parametrize("case,kind", F.runs(), ids=[f"{F.case_id(c)}-{k}" for c, k in F.runs()])
def test_against_fp64(case, kind):
    probs, conf, am = _run(case, kind)
    F.check((probs.cpu(), conf.item(), am.cpu()), F.reference(case, kind), f"{F.case_id(case)} {kind}")
    if kind == "ties":  # conf = 1 / (ties + rest) on every row, the first index wins
        x = F.inputs(case, kind)
        assert bool(((x == x.max(1, keepdim=True)[0]).long().cumsum(1)[torch.arange(len(x)), am.cpu().long()] == 1).all())
    if kind == "equal":
        print("max |p - 1/K|:", float((probs.cpu().double() - 1.0 / case[1]).abs().max()))
    if kind == "gap":
        assert float(probs.cpu()[F.engineered(case, kind)].abs().max()) == 0.0  # exp(-120) underflows to 0 in float32
    if kind == "-inf":
        assert float(probs.cpu()[F.engineered(case, kind)].abs().max()) == 0.0 and bool(torch.isfinite(probs).all())


@pytest.mark.parametrize("case", [(257, 19, 32), (257, 19, 24), (257, 2, 2), (33540, 19, 32)], ids=F.case_id)
def test_null_pointer_variants_and_nan_padding(case):
    """want_probs / want_argmax off in every combination: conf has the bits of the run where both are on, and what is still
    asked for too.  NaN in the padding columns ld > K: everything has the bits of the clean run."""
    for kind in ("normal", "ties"):
        probs, conf, am = _run(case, kind)
        for wp, wa in itertools.product((False, True), repeat=2):
            p2, c2, a2 = _run(case, kind, wp, wa)
            assert torch.equal(c2, conf), (kind, wp, wa)
            assert (p2 is None or torch.equal(p2, probs)) and (a2 is None or torch.equal(a2, am))
        if case[2] > case[1]:
            p3, c3, a3 = _run(case, kind, pad=float("nan"))
            assert torch.equal(c3, conf) and torch.equal(p3, probs) and torch.equal(a3, am)
            c4 = _run(case, kind, False, False, pad=float("nan"))[1]
            assert torch.equal(c4, conf)


def test_a_copied_layout_gives_the_same_bits():
    """An NCHW-contiguous tensor takes logits_rows' padded copy: same function, same bits as the pixel-major rows."""
    from onda_amd import ops
    case = (257, 19, 19)
    x = F.inputs(case, "normal")
    probs, conf, am = _run(case, "normal")
    nchw = x.t().reshape(1, 19, 1, 257).contiguous().to(DEV)
    c2, p2, a2 = ops.softmax_stats(nchw, True, True)
    assert torch.equal(c2, conf) and torch.equal(p2, probs) and torch.equal(a2, am)
