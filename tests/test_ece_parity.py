"""GPU: the fused calibration kernel (onda_upsample_ece, csrc/pointwise.hip) against the float64 restatement and the
comparator of tests/ece_fp64.py, and the evaluation paths that use it.  B = 2 throughout; every test prints its figures
before it asserts."""
import pytest
import torch

import ece_fp64 as E

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
MODES = ("logits", "probs")


def _head_out(x, ld):
    """CPU map [B,K,h,w] on the device in the model's pixel-major layout, rows of `ld` floats."""
    B, K, h, w = x.shape
    pad = torch.zeros(B, h, w, ld)
    pad[..., :K] = x.permute(0, 2, 3, 1)
    return pad.to(DEV)[..., :K].permute(0, 3, 1, 2)


def _table(x, labels, bins, mode, ld, hist=None):
    from onda_amd import ops
    table = torch.zeros(bins + 1, 3, dtype=torch.int64, device=DEV)
    ops.upsample_ece(_head_out(x, ld), labels.to(DEV), table, bins, probs=(mode == "probs"), hist=hist)
    return table


def _bins_global():
    from onda_amd._lib import query
    return query("onda_ece_bins_local") + 1


@pytest.mark.parametrize("bins", E.EXACT_BINS)
def test_exact_cases(bins):
    """The identity size in probs mode: hand-placed confidences (inside bins, on edges, 1.0, NaN, +inf), labels with 255;
    the table equals the restatement exactly, the extra row included."""
    conf, cls, labels = E.exact_inputs(bins)
    K, ld = E.EXACT_CASE[4], E.EXACT_CASE[5]
    want = E.table_of(conf, cls, labels, bins, E.rows_exact(conf, bins))
    got = _table(E.exact_map(conf, cls, K), labels, bins, "probs", ld).cpu()
    print(f"bins {bins}: overflow row {got[bins].tolist()}, rows that differ: {int((got != want).any(1).sum())}")
    assert int((labels == 255).sum()) > 0 and want[bins].tolist() == [0, 0, 2]
    assert torch.equal(got, want)
    from onda_amd.framework.utils.monitoring import ECE
    ece = ECE(bins)
    ece.record_lowres(_head_out(E.exact_map(conf, cls, K), ld), labels, (8, 16), probs=True)
    assert torch.equal(ece.table.cpu(), want) and torch.isnan(ece())


def test_exact_case_without_the_non_finite_pixels_has_the_restated_value():
    bins = 10
    conf, cls, labels = E.exact_inputs(bins, safe=True)
    want = E.table_of(conf, cls, labels, bins, E.rows_exact(conf, bins))
    rows = E.exact_map(conf, cls, 19).permute(0, 2, 3, 1).reshape(-1, 19).contiguous().to(DEV)  # an [N,K] map, ld = 19
    from onda_amd import ops
    from onda_amd.framework.utils.monitoring import ECE
    table = torch.zeros(bins + 1, 3, dtype=torch.int64, device=DEV)
    ops.upsample_ece(rows, labels.to(DEV), table, bins, probs=True, shape=(2, 8, 16))
    assert torch.equal(table.cpu(), want)
    ece = ECE(bins)
    ece.record_lowres((rows, (2, 8, 16)), labels, (8, 16), probs=True)
    assert ece().item() == pytest.approx(E.ece_of(want), abs=1e-7)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("where", ("lds", "global"))
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_interpolated_cases(case, where, mode):
    bins = 1000 if where == "lds" else _bins_global()
    x, labels = E.inputs(case, mode)
    got = _table(x, labels, bins, mode, case[5])
    E.split(case, mode, bins).check(got, f"{E.case_id(case)} {mode} bins {bins}")


def test_contention_case():
    """> 95 % of the pixels in the top bin: every lane of a wave adds to the same LDS row."""
    sp = E.split(E.CONTENTION, "logits", 1000, True)
    assert sp.top_share > 0.95
    x, labels = E.contention_inputs()
    got = _table(x, labels, 1000, "logits", E.CONTENTION[5])
    sp.check(got, "contention")
    print("top bin:", got[999].tolist(), "certain:", sp.certain[999].tolist(), "near:", sp.near)
    if sp.near == 0:  # no pixel near an edge or a tie: counts are held exactly
        assert torch.equal(got[:, 1:].cpu(), sp.full[:, 1:])


def test_two_runs_are_bit_identical_and_tables_accumulate():
    case, mode = E.CASES[1], "logits"
    x, labels = E.inputs(case, mode)
    a, b = _table(x, labels, 1000, mode, case[5]), _table(x, labels, 1000, mode, case[5])
    assert torch.equal(a, b)
    x2, labels2 = E.inputs(E.CASES[2], mode)
    from onda_amd import ops
    ops.upsample_ece(_head_out(x2, 32), labels2.to(DEV), b, 1000)  # a second record into the same table
    assert torch.equal(b, a + _table(x2, labels2, 1000, mode, 32))
    g = _bins_global()
    assert torch.equal(_table(x, labels, g, mode, case[5]), _table(x, labels, g, mode, case[5]))


@pytest.mark.parametrize("case", E.CASES[1:], ids=E.case_id)
def test_hist_argument(case):
    from onda_amd import ops
    x, labels = E.inputs(case, "logits")
    K = case[4]
    hist = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    with_hist = _table(x, labels, 1000, "logits", case[5], hist=hist)
    want = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    ops.upsample_argmax_hist(_head_out(x, case[5]), labels.to(DEV), want, K)
    assert int(want.sum()) == int((labels < K).sum())
    assert torch.equal(hist, want)
    assert torch.equal(with_hist, _table(x, labels, 1000, "logits", case[5]))


def test_guards():
    from onda_amd import ops
    x, labels = E.inputs(E.CASES[0], "logits")
    out = _head_out(x, 5)
    with pytest.raises(ValueError):
        ops.upsample_ece(out, labels.to(DEV), torch.zeros(10, 3, dtype=torch.int64, device=DEV), 10)
    with pytest.raises(RuntimeError, match="onda_upsample_ece"):
        ops.upsample_ece(out, labels.to(DEV), torch.zeros(1, 3, dtype=torch.int64, device=DEV), 0)


# ------------------------------------------------------------------------------------------------ evaluation paths
def _cfg(tmp_path, skip, snapshot=None):
    from onda_amd.config import hybrid_switch_cfg
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, snapshot or str(tmp_path), batch_size=2)
    cfg.OTHERS.ECE_SKIP = skip
    return cfg, spec


@pytest.fixture(scope="module")
def model():
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_model
    from onda_amd.synthetic import fill_state_dict
    m = get_model(hybrid_switch_cfg(128, 64, DEV, "NONE", batch_size=2)[0], 19)
    fill_state_dict(m, 1, 3.0)
    return m


@pytest.fixture(scope="module")
def loader():
    from onda_amd.synthetic import synth_batch
    return [synth_batch(2, 64, 128, seed=300 + i) for i in range(2)]


def test_evaluation_end_to_end(tmp_path, model, loader):
    """`evaluation` with ECE on: "ece model" is the restatement's value on the logits of the same forward passes, within
    the comparator's bound; the IoU arrays equal those of an ECE_SKIP: True run bit for bit."""
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import evaluation
    cfg, spec = _cfg(tmp_path, False, "NONE")
    ev = evaluation(model, cfg, spec)
    seen = []
    hook = model.register_forward_hook(lambda m, a, out: seen.append(out[1]["out"].detach().float().cpu().clone()))
    try:
        iou = ev.evaluate(loader)
    finally:
        hook.remove()
    assert [k for k, _ in ev.eval_metric_list] == ["ece model"] and len(seen) == 2
    report_value = ev.eval_metric_list[0][1]
    tables, near, n = [], 0, 0
    for logits, batch in zip(seen, loader):
        sp = E.Split(logits, batch["label"], 1000, "logits")
        tables.append(sp.full)
        near, n = near + sp.near, n + sp.n
    want = E.ece_of(sum(tables))
    bound = (3.0 * near + n * E.DELTA) / n
    print(f"ece model {report_value:.9f}, restated {want:.9f}, {near} near pixels of {n}, bound {bound:.2e}")
    assert near <= E.NEAR_CAP * n and abs(report_value - want) <= bound + 1e-7  # (+ the float32 return value)
    cfg_off, spec_off = _cfg(tmp_path, True, "NONE")
    off = evaluation(model, cfg_off, spec_off)
    iou_off = off.evaluate(loader)
    assert off.eval_metric_list == [] and set(iou) == set(iou_off) == {"model"}
    assert (iou["model"].tobytes() == iou_off["model"].tobytes())
    report = ev.evaluate_all({"val": loader})
    assert "ece model val" in report and ev.eval_metric_list == []


@pytest.mark.parametrize("dynamic", (False, True))
def test_hybrid_adapter_reports_every_recorder(tmp_path, model, loader, dynamic):
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.framework.handlers import get_adapt_method
    cfg, spec = _cfg(tmp_path, False)
    spec.SKIP_PROTO_EVAL = False
    spec.EMA_LAMBDA = 0.5
    da = get_adapt_method(cfg)(model, cfg, spec)
    da.update_dynamic()
    switch_batch_statistics(da.model, False)
    da.calculate_prototypes(loader, save=False)
    switch_batch_statistics(da.model, True)
    da.model_select.current = da.model_select.dynamic if dynamic else da.model_select.static
    iou = da.evaluate(loader[:1])
    keys = [k for k, _ in da.eval_metric_list]
    print(keys, [round(v, 6) for _, v in da.eval_metric_list])
    want = {"ece model", "ece proto", "ece ema", "ece static", "ece pure prototypes"} | ({"ece dynamic"} if dynamic else set())
    assert set(keys) == want and len(keys) == len(want) and set(iou) == {"model", "proto"}
    assert all(0.0 <= v <= 1.0 for _, v in da.eval_metric_list)
    assert da.ece_save == {}
    report = da.evaluate_all({"val": loader[:1]})
    assert {k + " val" for k in want} <= set(report)


def test_default_step_and_evaluation_never_call_the_ece_kernel(tmp_path, model, loader, monkeypatch):
    """The shipped settings (ECE_SKIP: True): a step and an evaluation launch what they launched before."""
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.framework.handlers import get_adapt_method
    from onda_amd.ops import loss as oloss
    seen = []
    real = oloss.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(oloss, "call", spy)
    cfg, spec = _cfg(tmp_path, True)
    spec.SKIP_PROTO_EVAL = False
    da = get_adapt_method(cfg)(model, cfg, spec)
    da.update_dynamic()
    switch_batch_statistics(da.model, False)
    da.calculate_prototypes(loader, save=False)
    switch_batch_statistics(da.model, True)
    da.optimizer.zero_grad()
    da.adjust_learning_rate(0, 6)
    from onda_amd.synthetic import synth_batch
    da.step([synth_batch(2, 64, 128, seed=100)], synth_batch(2, 64, 128, seed=200))
    da.update_ema()
    iou = da.evaluate(loader[:1])
    torch.cuda.synchronize()
    assert set(iou) == {"model", "proto"} and da.eval_metric_list == []
    assert "onda_upsample_argmax_hist" in seen and "onda_upsample_ece" not in seen, sorted(set(seen))
