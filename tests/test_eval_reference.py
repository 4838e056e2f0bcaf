"""CPU: the float64 restatement and the comparator of tests/eval_fp64.py against float32 ATen on the whole table and against
injected faults; the composed route of ops.upsample_eval off the GPU; the identity tables `label_raw` is made with; the surface
the validation pass adds (C prototype, drop-in alias, Segmentation_db's `original_label`)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import eval_fp64 as V
import upsample_fp64 as U
from conftest import ROOT


# ------------------------------------------------------------------------------------------------ floors
@pytest.mark.parametrize("case,kind", V.runs(), ids=V.run_id)
def test_fp32_aten_stays_inside_the_bound(case, kind):
    """The basis of BOUND: the reference's statements in float32 sit at a quarter of it or below."""
    x, labels = V.inputs(case, kind)
    _, _, mean = V.aten(x, labels)
    V.check_mean(mean, V.reference(case, kind)[2], f"{V.case_id(case)} {kind} fp32 ATen")


def test_bound_is_four_times_the_measured_floor():
    """4 x floor rounded to one digit lies within a third of 4 x floor (1.5 -> 2, 1.49 -> 1), and not below 2^-23."""
    worst, where = V.floors()
    ratio = V.BOUND / worst
    print(f"floor {worst:.3e} at {where}, bound {V.BOUND:.1e}, ratio {ratio:.2f}")
    assert V.BOUND >= V.SPACING
    assert 2.6 <= ratio <= 5.4 or (V.BOUND == V.SPACING and ratio > 4.0)


def test_equal_logits_give_one_over_k():
    for case in V.CASES[:6]:
        assert abs(V.reference(case, "equal")[2] - 1.0 / case[3]) < 1e-15


def test_nan_input_gives_a_nan_mean():
    case = V.CASES[0]
    assert np.isnan(V.reference(case, "nan")[2]) and np.isnan(V.aten(*V.inputs(case, "nan"))[2])
    assert V.flagged(V.check_mean, 0.5, float("nan"), "probe") and V.flagged(V.check_mean, float("nan"), 0.5, "probe")


def test_labels_carry_ignored_values():
    for case in V.CASES[:6]:
        K = case[3]
        labels = V.inputs(case)[1]
        assert int((labels == 255).sum()) > 0 and int(((labels >= K) & (labels < 255)).sum()) >= 1
        assert int(V.reference(case)[1].sum()) == int((labels < K).sum())


# ------------------------------------------------------------------------------------------------ teeth
def test_dropped_tap_at_the_right_edge_is_flagged():
    """The last output column without its tap on the last low-resolution column: one pixel column of the map."""
    case = V.CASES[1]
    B, h, w, K, ldl, H, W = case
    x, labels = V.inputs(case)
    mx = U.axis_matrix(w, W).clone()
    assert mx[W - 1, w - 1] > 0.5
    mx[W - 1, w - 1] = 0.0
    cls, hist, mean = V.reference(case)
    bad_cls, bad_hist, bad_mean = V.restate(x, labels, mx=mx)
    assert not V.flagged(V.check_mean, V.restate(x, labels)[2], mean, "probe")
    assert V.flagged(V.check_mean, bad_mean, mean, "probe")
    assert V.flagged(V.check_counts, bad_cls, cls, "probe") and V.flagged(V.check_counts, bad_hist, hist, "probe")


def test_missing_epsilon_is_flagged():
    """Without the 1e-30 a probability that underflows to 0 in float32 gives 0 * log2(0) = NaN."""
    case = V.CASES[0]
    x, labels = V.inputs(case, "gap")
    mean = V.reference(case, "gap")[2]
    assert V.flagged(V.check_mean, V.aten(x, labels, eps=0.0)[2], mean, "probe")
    assert not V.flagged(V.check_mean, V.aten(x, labels)[2], mean, "probe")


def test_natural_log_in_place_of_log2_is_flagged():
    case = V.CASES[1]
    x, labels = V.inputs(case)
    mean = V.reference(case)[2]
    assert V.flagged(V.check_mean, V.aten(x, labels, divisor=float(np.log(case[3])))[2], mean, "probe")
    # K = 2: the divisor log2(K) is 1, and the fault to catch is a natural logarithm in the numerator, ln p = log2 p / log2 e
    k2 = V.CASES[5]
    x2, labels2 = V.inputs(k2)
    assert V.flagged(V.check_mean, V.aten(x2, labels2, divisor=1.0 / float(np.log(2.0)))[2], V.reference(k2)[2], "probe")


def test_mean_over_pixels_instead_of_elements_is_flagged():
    case = V.CASES[0]
    x, labels = V.inputs(case)
    assert V.flagged(V.check_mean, V.restate(x, labels, per_pixel=True)[2], V.reference(case)[2], "probe")


def test_transposed_confusion_matrix_is_flagged():
    for case in (V.CASES[0], V.CASES[5]):
        hist = V.reference(case)[1]
        assert V.flagged(V.check_counts, hist.t().contiguous(), hist, "probe")
        assert not V.flagged(V.check_counts, hist.clone(), hist, "probe")


# ------------------------------------------------------------------------------------------------ the composed route, off the GPU
@pytest.mark.parametrize("case", V.CASES[:6], ids=V.case_id)
def test_composed_route_on_the_cpu_is_the_reference_statement_for_statement(case):
    """ops.upsample_eval on CPU tensors takes ops.upsample_eval_composed: the same statements as the fp32 ATen leg, so the
    same class map, matrix and float32 mean bit for bit; `ent` holds that mean in the kernel's fixed point."""
    from onda_amd import ops
    B, h, w, K, ldl, H, W = case
    x, labels = V.inputs(case)
    cls, hist, mean = V.aten(x, labels)
    got_hist, got_cls = torch.zeros(K, K, dtype=torch.int64), torch.zeros(B, H, W, dtype=torch.uint8)
    got = ops.upsample_eval_composed(x, labels, got_hist, K, cls=got_cls)
    assert got.dtype == torch.float32 and float(got) == mean
    V.check_counts(got_hist, hist, "composed matrix")
    V.check_counts(got_cls, cls, "composed class map")
    ent, again = torch.zeros(2, dtype=torch.int64), torch.zeros(K, K, dtype=torch.int64)
    ops.upsample_eval(x, labels, again, K, ent)
    assert torch.equal(again, got_hist) and int(ent[1]) == 0
    back = ops.entropy_mean(ent, B, K, H, W)
    # (one rounding to a multiple of 2^-32 of the batch's sum, two roundings in float64)
    assert back.dtype == torch.float64 and abs(float(back) - mean) <= 1.0 / (B * K * H * W * 2.0 ** 32) + 2.0 ** -50 * mean
    V.check_mean(back, V.reference(case)[2], f"{V.case_id(case)} composed")
    rows = x.permute(0, 2, 3, 1).reshape(-1, K)  # the [N,K] form
    ent2, hist2 = torch.zeros(2, dtype=torch.int64), torch.zeros(K, K, dtype=torch.int64)
    ops.upsample_eval(rows, labels, hist2, K, ent2, shape=(B, h, w))
    assert torch.equal(ent2, ent) and torch.equal(hist2, got_hist)


def test_composed_route_counts_a_nan_batch_and_checks_its_arguments():
    from onda_amd import ops
    case = V.CASES[0]
    B, h, w, K, ldl, H, W = case
    x, labels = V.inputs(case, "nan")
    ent, hist = torch.zeros(2, dtype=torch.int64), torch.zeros(K, K, dtype=torch.int64)
    ops.upsample_eval(x, labels, hist, K, ent)
    assert ent.tolist() == [0, 1] and np.isnan(float(ops.entropy_mean(ent, B, K, H, W)))
    good = V.inputs(case)[0]
    with pytest.raises(ValueError):
        ops.upsample_eval(good, labels, hist, K + 1, ent)
    with pytest.raises(ValueError):
        ops.upsample_eval(good, labels, hist, K, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.upsample_eval(good, labels, None, K, ent)
    with pytest.raises(ValueError):
        ops.upsample_eval(good.permute(0, 2, 3, 1).reshape(-1, K), labels, hist, K, ent)
    with pytest.raises(TypeError):
        ops.upsample_eval(good.double(), labels, hist, K, ent)


# ------------------------------------------------------------------------------------------------ identity tables
def test_nearest_table_of_equal_sizes_is_the_identity():
    """`label_raw` is the nearest-resize kernel under nearest_table(n, n): the id map alone."""
    from onda_amd.pipeline import nearest_table
    for n in list(range(1, 2049)):
        t = nearest_table(n, n)
        assert t.dtype == np.int32 and np.array_equal(t, np.arange(n)), n


# ------------------------------------------------------------------------------------------------ surface
def test_header_and_signatures_name_the_kernel():
    from onda_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "onda_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+onda_upsample_eval\s*\(([^)]*)\)", text)
    assert m is not None
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 13 and args[0].startswith("const float*") and args[3].startswith("int64_t*") and args[4].startswith("int64_t*")
    res, argtypes = _lib.SIGNATURES["onda_upsample_eval"]
    assert res is _lib.I and len(argtypes) == 13
    assert argtypes == [_lib.P, _lib.I, _lib.P, _lib.P, _lib.P, _lib.P] + [_lib.I] * 6 + [_lib.P]


def test_dropin_aliases_eval_uda():
    import onda_amd.dropin as dropin
    assert "framework.domain_adaptation.eval_UDA" in dropin._MODULES
    saved = {k: v for k, v in sys.modules.items() if k == "framework" or k.startswith("framework.")}
    try:
        dropin.install()
        from framework.domain_adaptation.eval_UDA import evaluate_model
        import onda_amd.framework.domain_adaptation.eval_UDA as mine
        assert evaluate_model is mine.evaluate_model
    finally:
        for k in [k for k in sys.modules if k == "framework" or k.startswith("framework.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_segmentation_db_takes_original_label():
    import pandas as pd
    from onda_amd.framework.dataset.segmentation_db import Segmentation_db
    meta = pd.DataFrame([{"image_path": "a.png", "label_path": "b.png"}])
    ds = Segmentation_db("root", meta, {0: 0, 1: 255}, (64, 32), original_label=True)
    assert ds.original_label is True and len(ds) == 1
    assert Segmentation_db("root", meta, {0: 0, 1: 255}, (64, 32)).original_label is False


def test_trainer_reads_original_res():
    """SCHEME.ORIGINAL_RES unset ({} or None) or equal to RESOLUTION: no full-image pass (reference segmentation.py:49-54)."""
    from onda_amd.config import Cfg
    from onda_amd.framework.domain_adaptation.methods.segmentation import SegmentationTrainer
    t = SegmentationTrainer.__new__(SegmentationTrainer)
    for res, want in (({}, None), (None, None), ([128, 64], None), ([256, 128], (128, 256))):
        t.cfg = Cfg.from_dict({"SCHEME": {"RESOLUTION": [128, 64]}})
        if res != {}:
            t.cfg.SCHEME.ORIGINAL_RES = res
        assert t.original_size == want, (res, t.original_size)
