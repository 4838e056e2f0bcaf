"""GPU: the fused validation kernel (onda_upsample_eval, csrc/pointwise.hip) through ops.upsample_eval: confusion matrix and
class map bit-equal to the parent's kernels (ops.upsample_argmax_hist / ops.upsample_argmax: the same float32 expression, so
no tolerance), the entropy mean within eval_fp64.BOUND of the float64 restatement.  Every test prints its figures before it
asserts."""
import math

import pytest
import torch

import eval_fp64 as V

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _rows(x, ld, fill=0.0):
    """CPU logits [B,K,h,w] in the model's pixel-major layout on the device, rows of `ld` floats (padding: `fill`), as the
    NCHW view the ops take."""
    B, K, h, w = x.shape
    pad = torch.full((B, h, w, ld), fill)
    pad[..., :K] = x.permute(0, 2, 3, 1)
    return pad.to(DEV)[..., :K].permute(0, 3, 1, 2)


def _run(out, labels, want_cls=True):
    """(hist i64[K,K], ent i64[2], cls u8[B,H,W]) of one ops.upsample_eval launch into zeroed buffers."""
    from onda_amd import ops
    B, K = out.shape[:2]
    hist = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    ent = torch.zeros(2, dtype=torch.int64, device=DEV)
    cls = torch.full((B,) + tuple(labels.shape[1:]), 255, dtype=torch.uint8, device=DEV) if want_cls else None
    assert ops.upsample_eval(out, labels, hist, K, ent, cls=cls) is ent
    return hist, ent, cls


def _parent(out, labels):
    """The parent's kernels on the same inputs: (hist, cls)."""
    from onda_amd import ops
    K = out.shape[1]
    hist = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    ops.upsample_argmax_hist(out, labels, hist, K)
    return hist, ops.upsample_argmax(out, tuple(labels.shape[1:]))


@pytest.mark.parametrize("case,kind", V.runs(), ids=V.run_id)
def test_against_the_parent_kernels_and_fp64(case, kind):
    from onda_amd import ops
    B, h, w, K, ldl, H, W = case
    x, labels = V.inputs(case, kind)
    out = _rows(x, ldl)
    hist, ent, cls = _run(out, labels)
    want_hist, want_cls = _parent(out, labels)
    mean = ops.entropy_mean(ent, B, K, H, W)
    assert mean.dtype == torch.float64 and mean.is_cuda
    ref = V.reference(case, kind)[2]
    print(f"{V.case_id(case)} {kind}: ent {ent.tolist()}, counted pixels {int(hist.sum())} of {B * H * W}")
    assert torch.equal(hist, want_hist) and int(hist.sum()) == int((labels < K).sum())
    assert torch.equal(cls, want_cls)
    if kind == "nan":
        assert int(ent[1]) >= 1 and math.isnan(float(mean)) and math.isnan(ref)
        return
    assert int(ent[1]) == 0
    V.check_mean(mean, ref, f"{V.case_id(case)} {kind}")
    if kind == "equal":
        V.check_mean(mean, 1.0 / K, f"{V.case_id(case)} equal, against 1 / K")
    if kind == "normal" and case is not V.REAL:
        # the restatement's own classes: pixels apart, where float32 and float64 order two near-equal logits differently
        n = int((cls.cpu().long() != V.reference(case, kind)[0]).sum())
        print(f"class map against the float64 restatement: {n} of {B * H * W} pixels differ")
        assert n <= max(1, B * H * W // 1000)


def test_two_runs_and_split_batches_give_the_same_integers():
    from onda_amd import ops
    for case in (V.CASES[0], V.CASES[2]):  # 16-byte class loads; scalar loads
        B, h, w, K, ldl, H, W = case
        assert B == 2
        x, labels = V.inputs(case)
        out = _rows(x, ldl)
        a, b = _run(out, labels), _run(out, labels)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        hist = torch.zeros(K, K, dtype=torch.int64, device=DEV)
        ent = torch.zeros(2, dtype=torch.int64, device=DEV)
        for i in range(B):  # one image at a time, accumulated into the same buffers
            ops.upsample_eval(_rows(x[i:i + 1], ldl), labels[i:i + 1], hist, K, ent)
        print(f"{V.case_id(case)}: one launch {a[1].tolist()}, two launches {ent.tolist()}")
        assert torch.equal(hist, a[0]) and torch.equal(ent, a[1])
        # without a class map, and without labels: the same entropy sum
        assert torch.equal(_run(out, labels, want_cls=False)[1], a[1])
        ent2, cls2 = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)
        ops.upsample_eval(out, None, None, K, ent2, cls=cls2)
        assert torch.equal(ent2, a[1]) and torch.equal(cls2, a[2])


def test_padding_columns_are_never_read_as_classes():
    case = V.CASES[0]  # K = 19 in rows of 32: the last 16-byte group holds one padding column
    B, h, w, K, ldl, H, W = case
    x, labels = V.inputs(case)
    clean = _run(_rows(x, ldl), labels)
    dirty = _run(_rows(x, ldl, fill=float("nan")), labels)
    print(f"zero padding {clean[1].tolist()}, NaN padding {dirty[1].tolist()}")
    assert int(dirty[1][1]) == 0 and all(torch.equal(u, v) for u, v in zip(clean, dirty))


def test_rows_form_and_a_copied_layout():
    """The [N,K] map with shape=(B, h, w) (the prototype route): the launch its NCHW view gets, held to the parent's kernel and
    to float64 like every other (rows of 19 floats take the scalar loads, whose interpolation the compiler contracts its own
    way: the sum agrees with the 16-byte route's to 3e-9, not to the bit).  NCHW-contiguous logits are copied into zero-padded
    rows of 32: the same bits as rows laid out that way."""
    from onda_amd import ops
    case = V.CASES[1]
    B, h, w, K, ldl, H, W = case
    x, labels = V.inputs(case)
    rows = x.permute(0, 2, 3, 1).reshape(-1, K).contiguous().to(DEV)  # ld = 19
    hist, ent = torch.zeros(K, K, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    ops.upsample_eval(rows, labels, hist, K, ent, shape=(B, h, w))
    view = rows.reshape(B, h, w, K).permute(0, 3, 1, 2)
    same = _run(view, labels)
    print(f"[N,K] form {ent.tolist()}, its NCHW view {same[1].tolist()}")
    assert torch.equal(hist, same[0]) and torch.equal(ent, same[1])
    assert torch.equal(hist, _parent(view, labels)[0])
    V.check_mean(ops.entropy_mean(ent, B, K, H, W), V.reference(case)[2], f"{V.case_id(case)} as [N,K] rows")
    want = _run(_rows(x, ldl), labels)
    got = _run(x.to(DEV), labels)
    print(f"rows of 32 {want[1].tolist()}, copied from NCHW {got[1].tolist()}")
    assert ldl == 32 and all(torch.equal(u, v) for u, v in zip(got, want))


@pytest.mark.parametrize("K", (1, 33))
def test_class_counts_outside_the_kernel_take_the_composed_route(K, monkeypatch):
    from onda_amd import ops
    from onda_amd._lib import call
    from onda_amd.ops import loss as oloss
    from onda_amd.ops.core import _p, _stream
    B, h, w, H, W = 2, 3, 5, 17, 33
    g = torch.Generator().manual_seed(K)
    rows = torch.zeros(B, h, w, 40)
    rows[..., :K] = torch.randn(B, h, w, K, generator=g) * 3
    rows = rows.to(DEV)
    out = rows[..., :K].permute(0, 3, 1, 2)
    labels = torch.randint(0, K, (B, H, W), generator=g).to(torch.uint8)
    seen = []
    real = oloss.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(oloss, "call", spy)
    hist, ent, cls = _run(out, labels)
    assert "onda_upsample_eval" not in seen and "onda_upsample_fwd" in seen
    want_hist = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    want_cls = torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)
    want = ops.upsample_eval_composed(out, labels, want_hist, K, cls=want_cls)
    mean = ops.entropy_mean(ent, B, K, H, W)
    print(f"K = {K}: composed mean {float(want)!r}, through upsample_eval {float(mean)!r}, ent {ent.tolist()}")
    assert torch.equal(hist, want_hist) and torch.equal(cls, want_cls) and int(hist.sum()) == B * H * W
    if K == 1:  # log2(1) = 0 divides: the reference's mean is NaN
        assert math.isnan(float(want)) and math.isnan(float(mean)) and ent.tolist() == [0, 1]
    else:
        assert abs(float(mean) - float(want)) <= 1.0 / (B * K * H * W * 2.0 ** 32) + 2.0 ** -50 * float(want)
    ent_raw = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="onda_upsample_eval failed: ONDA_EINVAL"):
        call("onda_upsample_eval", _p(rows), 40, _p(labels.to(DEV)), _p(want_hist), _p(ent_raw), None, B, h, w, K, H, W, _stream())
    assert ent_raw.tolist() == [0, 0]


def test_the_c_entry_refuses_half_a_label_pair():
    from onda_amd._lib import call
    from onda_amd.ops.core import _p, _stream
    rows = torch.zeros(1, 3, 5, 32, device=DEV)
    labels = torch.zeros(1, 17, 33, dtype=torch.uint8, device=DEV)
    hist = torch.zeros(19, 19, dtype=torch.int64, device=DEV)
    ent = torch.zeros(2, dtype=torch.int64, device=DEV)
    for lab, hh in ((labels, None), (None, hist)):
        with pytest.raises(RuntimeError, match="ONDA_EINVAL"):
            call("onda_upsample_eval", _p(rows), 32, _p(lab), _p(hh), _p(ent), None, 1, 3, 5, 19, 17, 33, _stream())
    with pytest.raises(RuntimeError, match="ONDA_EINVAL"):
        call("onda_upsample_eval", _p(rows), 32, _p(labels), _p(hist), None, None, 1, 3, 5, 19, 17, 33, _stream())
