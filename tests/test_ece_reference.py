"""CPU: the expected calibration error (reference monitoring.py:99-136) -- fixture G18 (tests/golden/make_golden_ece.py:
the reference's own ECE behind nn.Upsample) against the float64 restatement of tests/ece_fp64.py and the torch path
``ECE.record``; the comparator's teeth; the wiring of OTHERS.ECE_SKIP: False through the adapters.

G18_ECE_FLOOR: the reference accumulates its table in float32 (a sparse matmul); the worst |ECE(reference) - ECE(exact
table of the same pixels)| over G18 is 8.9e-8 (exact case, bins = 1; interpolated cases: <= 2.3e-8).  Held to 4 x that."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ece_fp64 as E

G18_ECE_FLOOR = 8.9e-8
ECE_TOL = 4 * G18_ECE_FLOOR
MODES = ("logits", "probs")


def _ece_class():
    from onda_amd.framework.utils.monitoring import ECE
    return ECE


def _label_digest(labels):
    """As tests/golden/make_golden_ece.py: per-value counts and a position-weighted sum of the seeded labels."""
    flat = labels.reshape(-1).long()
    return np.concatenate([np.bincount(flat.numpy(), minlength=256), [int((flat * (torch.arange(flat.numel()) % 8191 + 1)).sum())]])


def _stored_table(g, key, bins):
    """The reference's float32 [bins, 3] table from its non-empty rows."""
    t = torch.zeros(bins, 3, dtype=torch.float32)
    t[torch.from_numpy(g[key + "_rows"]).long()] = torch.from_numpy(g[key + "_table"])
    return t


def _f32_sum_allowance(table):
    """What a float32 accumulation of n values <= 1 may be off by: n * 2^-24 * sum <= n^2 * 2^-24."""
    n = table[:, 2].double()
    return n * n * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ G18, exact cases
@pytest.mark.parametrize("bins", E.EXACT_BINS)
def test_exact_cases_reproduce_the_reference(golden, bins):
    g = golden("g18_ece")
    conf, cls, labels = E.exact_inputs(bins, safe=True)
    assert np.array_equal(conf.numpy(), g[f"exact{bins}_conf"]) and np.array_equal(cls.numpy(), g[f"exact{bins}_cls"])
    assert np.array_equal(labels.numpy(), g[f"exact{bins}_labels"])
    rows = E.rows_exact(conf, bins)
    assert torch.equal(rows, torch.floor_divide(conf, 1.0 / bins).long())  # ATen's float32 floor division, unclamped here
    mine = E.table_of(conf, cls, labels, bins, rows)
    ref = torch.from_numpy(g[f"exact{bins}_table"])
    assert torch.equal(ref[:, 1:].long(), mine[:bins, 1:]) and int(mine[bins, 2]) == 0
    assert ((ref[:, 0].double() - mine[:bins, 0].double() / E.FIX).abs() <= _f32_sum_allowance(mine[:bins])).all()
    assert abs(E.ece_of(mine) - float(g[f"exact{bins}_ece"])) <= ECE_TOL
    ece = _ece_class()(bins)
    ece.record(E.exact_map(conf, cls, E.EXACT_CASE[4]), labels, axis=1)
    assert torch.equal(ece.table, mine)
    assert ece().dtype == torch.float32 and abs(ece().item() - float(g[f"exact{bins}_ece"])) <= ECE_TOL
    assert torch.allclose(ece.calc_matrix, ref, rtol=0, atol=float(_f32_sum_allowance(mine[:bins]).max()) + 1e-7)


@pytest.mark.parametrize("bins", E.EXACT_BINS)
def test_where_the_reference_breaks(bins):
    """conf = 1.0 at bins = 4 (bin 4 of 4) goes to the last bin; NaN / +inf go to the extra row and make ECE() NaN."""
    conf, cls, labels = E.exact_inputs(bins)
    rows = E.rows_exact(conf, bins)
    assert int((rows == bins).sum()) == 2 and int(rows.max()) == bins
    if bins in (4, 1):
        assert int((torch.floor_divide(conf[torch.isfinite(conf)], 1.0 / bins) >= bins).sum()) >= 2  # the reference raises here
    mine = E.table_of(conf, cls, labels, bins, rows)
    ece = _ece_class()(bins)
    ece.record(E.exact_map(conf, cls, E.EXACT_CASE[4]), labels, axis=1)
    assert torch.equal(ece.table, mine) and mine[bins].tolist() == [0, 0, 2]
    assert int(mine[:, 2].sum()) == conf.numel()
    assert np.isnan(ece().item()) and np.isnan(E.ece_of(mine))
    finite = _ece_class()(bins)
    finite.record(torch.tensor([-0.5, 0.0, 1.0e-30, 1.0, 3.0e38]).reshape(5, 1), torch.zeros(5), axis=1)  # finite: inside the table
    assert int(finite.table[bins, 2]) == 0 and int(finite.table[0, 2]) >= 3 and int(finite.table[bins - 1, 2]) >= 2
    assert int(finite.table[:bins, 2].sum()) == 5


# ------------------------------------------------------------------------------------------------ G18, interpolated
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_interpolated_cases_reproduce_the_reference(golden, case, mode):
    g = golden("g18_ece")
    bins = int(g["bins"])
    x, labels = E.inputs(case, mode)
    key = f"{E.case_id(case)}_{mode}"
    assert np.array_equal(E.inputs(case, "logits")[0].numpy(), g[E.case_id(case) + "_x"])
    assert np.array_equal(_label_digest(labels), g[E.case_id(case) + "_labels_digest"])
    sp = E.split(case, mode, bins)
    ref = _stored_table(g, key, bins).double()
    ref_int = torch.zeros(bins + 1, 3, dtype=torch.int64)
    ref_int[:bins, 0] = torch.round(ref[:, 0] * E.FIX).long()
    ref_int[:bins, 1:] = ref[:, 1:].long()
    sp.check(ref_int, f"reference {key}", extra_sum=_f32_sum_allowance(ref_int[:bins]))
    assert abs(float(g[key + "_ece"]) - sp.ece) <= sp.ece_bound + ECE_TOL
    # fp32 ATen on this machine, binned by the torch path of the product
    H, W = labels.shape[1:]
    up = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True)
    ece = _ece_class()(bins)
    ece.record(up.softmax(1) if mode == "logits" else up, labels, axis=1)
    sp.check(ece.table, f"ECE.record {key}")
    assert torch.equal(ece.table, E.aten_table(x, labels, bins, mode))
    assert abs(ece().item() - float(g[key + "_ece"])) <= 2 * sp.ece_bound + ECE_TOL


def test_contention_case_reproduces_the_reference(golden):
    g = golden("g18_ece")
    x, labels = E.contention_inputs()
    assert np.array_equal(x.numpy(), g["contention_x"]) and np.array_equal(_label_digest(labels), g["contention_labels_digest"])
    sp = E.split(E.CONTENTION, "logits", 1000, True)
    assert sp.top_share > 0.95
    ref = _stored_table(g, "contention", 1000).double()
    ref_int = torch.zeros(1001, 3, dtype=torch.int64)
    ref_int[:1000, 0] = torch.round(ref[:, 0] * E.FIX).long()
    ref_int[:1000, 1:] = ref[:, 1:].long()
    sp.check(ref_int, "reference, contention", extra_sum=_f32_sum_allowance(ref_int[:1000]))
    sp.check(E.aten_table(x, labels, 1000, "logits"), "ATen, contention")
    assert abs(float(g["contention_ece"]) - sp.ece) <= sp.ece_bound + ECE_TOL


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bins", (1000, 2048))
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_seeds_keep_near_pixels_rare(case, mode, bins):
    """The condition the comparator stands on: fp32 ATen on the CPU passes it and at most 1 % of the pixels are near."""
    x, labels = E.inputs(case, mode)
    sp = E.split(case, mode, bins)
    assert sp.near <= E.NEAR_CAP * sp.n
    conf32, conf64 = E.aten_pixels(x, *labels.shape[1:], mode)[0], E.pixels(x, *labels.shape[1:], mode)[0]
    assert 4 * (conf32.double() - conf64).abs().max().item() <= E.DELTA
    sp.check(E.aten_table(x, labels, bins, mode), "ATen")


# ------------------------------------------------------------------------------------------------ teeth
def _case():
    case, mode, bins = E.CASES[2], "logits", 1000
    x, labels = E.inputs(case, mode)
    return x, labels, bins, E.split(case, mode, bins)


def test_comparator_flags_dropped_ignore_pixels():
    x, labels, bins, sp = _case()
    conf, cls = E.aten_pixels(x, *labels.shape[1:], "logits")
    keep = labels != 255
    rows = torch.floor_divide(conf, 1.0 / bins).clamp(0, bins - 1).long()
    assert not sp.flagged(E.table_of(conf, cls, labels, bins, rows))
    assert sp.flagged(E.table_of(conf[keep], cls[keep], labels[keep], bins, rows[keep]))


def test_comparator_flags_softmax_before_interpolation():
    x, labels, bins, sp = _case()
    assert not sp.flagged(E.aten_table(x, labels, bins, "logits"))
    assert sp.flagged(E.aten_table(x.softmax(1), labels, bins, "probs"))


def test_comparator_flags_a_lost_flush():
    x, labels, bins, sp = _case()
    t = E.aten_table(x, labels, bins, "logits")
    row = int(t[:bins, 2].argmax())
    lost = t.clone()
    lost[row] = 0
    assert not sp.flagged(t) and sp.flagged(lost)
    one = t.clone()
    one[int((t[:bins, 2] == 1).nonzero()[0]), :] = 0  # a bin with a single pixel
    assert sp.flagged(one)


def test_comparator_flags_ceil_instead_of_floor():
    x, labels, bins, sp = _case()
    conf, cls = E.aten_pixels(x, *labels.shape[1:], "logits")
    rows = torch.ceil(conf / E.gap32(bins)).clamp(0, bins - 1).long()
    assert sp.flagged(E.table_of(conf, cls, labels, bins, rows))


def test_exact_cases_tell_the_division_rules_apart():
    """bins = 10: floorf(a / b) rounds 0.7f / 0.1f = 6.9999998 up to 7 and ceil moves every confidence inside a bin; the
    fmod-based floor division (and the restatement in rationals) keeps bin 6."""
    bins = 10
    conf, cls, labels = E.exact_inputs(bins)
    fin = torch.isfinite(conf)
    rows = E.rows_exact(conf, bins)
    good = E.table_of(conf, cls, labels, bins, rows)
    gap = torch.tensor(E.gap32(bins))
    naive = torch.where(fin, torch.floor(conf / gap).clamp(0, bins - 1), torch.full_like(conf, bins)).long()
    assert int(E.rows_exact(torch.tensor([0.7]), bins)) == 6 and int(torch.floor(torch.tensor(0.7) / gap)) == 7
    assert int((naive != rows).sum()) >= 1 and not torch.equal(E.table_of(conf, cls, labels, bins, naive), good)
    up = torch.where(fin, torch.ceil(conf / gap).clamp(0, bins - 1), torch.full_like(conf, bins)).long()
    assert not torch.equal(E.table_of(conf, cls, labels, bins, up), good)


def test_exact_cases_tell_a_missing_top_clamp():
    bins = 4
    conf, cls, labels = E.exact_inputs(bins)
    rows = E.rows_exact(conf, bins)
    good = E.table_of(conf, cls, labels, bins, rows)
    raw = torch.where(torch.isfinite(conf), torch.floor_divide(torch.nan_to_num(conf, 0.0, 0.0, 0.0), 1.0 / bins), torch.tensor(float(bins))).long()
    assert int((raw[torch.isfinite(conf)] >= bins).sum()) >= 2  # conf = 1.0: bin 4 of 4, outside the table
    unclamped = raw.clamp(max=bins)  # (a kernel without the clamp would index past the table; here: the extra row)
    assert not torch.equal(E.table_of(conf, cls, labels, bins, unclamped), good)


# ------------------------------------------------------------------------------------------------ wiring
def _cfg(skip, device="cpu"):
    from onda_amd.config import hybrid_switch_cfg
    cfg, spec = hybrid_switch_cfg(128, 64, device, "NONE", batch_size=2)
    cfg.OTHERS.ECE_SKIP = skip
    return cfg, spec


@pytest.fixture(scope="module")
def cpu_model():
    from onda_amd.framework.handlers import get_model
    return get_model(_cfg(True)[0], 19)


def test_adapters_construct_with_ece_on(cpu_model):
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import evaluation
    from onda_amd.framework.handlers import get_adapt_method
    cfg, spec = _cfg(False)
    ev = evaluation(cpu_model, cfg, spec)
    assert ev.ece_record is True and ev.ece_bins() == 1000 and ev.eval_metric_list == []
    cfg.OTHERS.BINS = 15
    assert ev.ece_bins() == 15
    da = get_adapt_method(cfg)(cpu_model, cfg, spec)
    assert da.ece_record is True and da.ece_save == {}
    for skip in (True, "yes", {}):  # the reference's rule: anything but the boolean True records
        cfg, spec = _cfg(skip)
        assert evaluation(cpu_model, cfg, spec).ece_record is (skip is not True)


def test_default_config_leaves_the_attributes_as_they_were(cpu_model):
    from onda_amd.config import hybrid_switch_cfg, unset
    from onda_amd.framework.handlers import get_adapt_method
    cfg, spec = hybrid_switch_cfg(128, 64, "cpu", "NONE", batch_size=2)
    assert cfg.OTHERS.ECE_SKIP is True and unset(cfg.OTHERS.BINS)
    da = get_adapt_method(cfg)(cpu_model, cfg, spec)
    assert da.ece_record is False and da.eval_metric_list == [] and da.ece_save == {}
    da.intensity_ma.eval()
    da.record_ece("ema", None, None)  # off: nothing is touched, nothing recorded
    da.register_ece()
    assert da.ece_save == {} and da.eval_metric_list == []


def test_recorders_reach_eval_metric_list_under_the_reference_keys(cpu_model, monkeypatch):
    """register_ece / evaluate_all with the launches replaced by the torch path: the keys and the reset."""
    from onda_amd.framework.handlers import get_adapt_method
    from onda_amd.framework.utils import monitoring
    cfg, spec = _cfg(False)
    da = get_adapt_method(cfg)(cpu_model, cfg, spec)
    seen = []

    def fake(self, rows_or_out, label, size, probs, hist=None, num_classes=None):
        seen.append((probs, tuple(size)))
        self.record(torch.full((1, 2, 2, 2), 0.5), torch.zeros(1, 2, 2), 1)
    monkeypatch.setattr(monitoring.ECE, "record_lowres", fake)
    label = torch.zeros(2, 64, 128, dtype=torch.uint8)
    da.record_ece("ema", torch.zeros(4, 19), label, shape=(2, 1, 2))
    assert da.ece_save == {}  # the monitor is not frozen: a training step records nothing
    da.intensity_ma.eval()
    for name in ("ema", "static", "pure prototypes"):
        da.record_ece(name, torch.zeros(4, 19), label, shape=(2, 1, 2))
    assert seen == [(True, (64, 128))] * 3 and set(da.ece_save) == {"ece ema", "ece static", "ece pure prototypes"}
    da.register_ece()
    assert [k for k, _ in da.eval_metric_list] == ["ece ema", "ece static", "ece pure prototypes"] and da.ece_save == {}
    assert all(v == pytest.approx(0.5) for _, v in da.eval_metric_list)
    da.intensity_ma.train()


def test_label_size_is_checked():
    ece = _ece_class()(10)
    with pytest.raises(RuntimeError, match="labels of"):
        ece.record_lowres(torch.zeros(1, 19, 4, 4), torch.zeros(1, 32, 64), (64, 128), probs=False)
