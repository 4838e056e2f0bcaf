"""The SOFT_LABELS branch of the target loss on the GPU: the fused kernels onda_soft_loss_fwd / _bwd against fixture G29 (the
reference's own functions) and against the float64 restatement of tests/soft_loss_fp64.py, the framework functions on top of
them, two hybrid_proDA steps against fixture G30, one adv_proDA step, and the default path left alone.

Tolerances are the ones tests/test_target_regularisers.py holds the sibling kernels to: 1e-5 for values and gradients (of the
gradient's max-norm; NaN / +-inf matched exactly, by position and kind), 5e-3 for log entries, 0.02 / 0.6 for the weight update
of step 0 / step 1 (relative L2 over the state digests).

G30 runs at RCE_BETA = 300: at the yml weight the soft run's step-0 update is 0.0011 from the hard-label run's, inside the 0.02
bound; at 300 it is 0.306 (0.376 from G7's), so a soft path that ran the hard loss fails."""
import json
import math

import numpy as np
import pytest
import torch

import soft_loss_fp64 as sl
from conftest import digest
from test_soft_labels_reference import PAIRS, case_of
from test_target_regularisers import _head_out, _log_close, _two_steps

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _run(out, soft, w_ce, w_rce, w_reg, reg="MRKLD", trunc=True):
    from onda_amd import ops
    out = out.detach().requires_grad_(True)
    total, ce, rce, r = ops.soft_target_losses(out, soft, w_ce, w_rce, w_reg, reg, ce_trunc=trunc)
    total.backward()
    return {"total": total.item(), "ce": ce.item(), "rce": rce.item(), "reg": r.item(), "grad": out.grad.detach().cpu()}


def _rows(soft_nchw):
    """The [N,K] soft map of an NCHW target, on the device."""
    return soft_nchw.permute(0, 2, 3, 1).reshape(-1, soft_nchw.shape[1]).contiguous().to(DEV)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("case", sl.SMALL)
def test_kernels_match_the_reference(golden, case):
    """Each term alone, the weighted total and the total without CE against the reference's values and gradients."""
    g = golden("g29_soft_losses")
    logits, soft = case_of(g, case)
    out, rows = _head_out(logits), _rows(soft)
    for key, w_ce, w_rce, w_reg, trunc in PAIRS:
        r = _run(out, rows, w_ce, w_rce, w_reg, "MRKLD", trunc)
        print(case, key, r["total"], float(g[f"{case}_{key}"]))
        assert sl.value_close(r["total"], g[f"{case}_{key}"]), (case, key, r["total"], float(g[f"{case}_{key}"]))
        sl.grad_close(r["grad"], torch.from_numpy(g[f"{case}_grad_{key}"]), 1e-5, f"{case} grad {key}")
        if key in ("lc", "ce"):  # the term's own value, and the CE gradient element by element
            assert sl.value_close(r["ce"], g[f"{case}_{key}"])
            sl.ce_grad_close(r["grad"], torch.from_numpy(g[f"{case}_grad_{key}"]), f"{case} CE gradient ({key})")
        if key == "lc":
            assert int((r["grad"] != 0).sum()) == int(g[f"{case}_grad_lc_nonzero"]) >= 1
        if key == "rce":
            assert sl.value_close(r["rce"], g[f"{case}_rce"]) and math.isfinite(r["rce"])
        if key == "noce":  # a term without a weight enters neither the total nor the gradient: finite over negative logits
            assert math.isfinite(r["total"]) and torch.isfinite(r["grad"]).all(), case  # and at a pole
    if case in ("mixed", "pole"):
        full = _run(out, rows, sl.W_CE, sl.W_RCE, sl.W_REG, "MRKLD", True)
        assert math.isnan(full["total"]) and math.isnan(full["ce"]) and math.isfinite(full["rce"])
        assert bool(torch.isfinite(full["grad"]).all()) == (case == "mixed")


@pytest.mark.parametrize("case", sl.SMALL)
@pytest.mark.parametrize("reg", ["MRKLD", "MRENT", "none"])
@pytest.mark.parametrize("trunc", [True, False])
def test_kernels_match_the_restatement(golden, case, reg, trunc):
    """Every regulariser selector, ce_trunc on and off: the regulariser alone, the weighted total, the total without CE."""
    g = golden("g29_soft_losses")
    logits, soft = case_of(g, case)
    out, rows = _head_out(logits), _rows(soft)
    for w_ce, w_rce, w_reg in ((0.0, 0.0, 1.0), (sl.W_CE, sl.W_RCE, sl.W_REG), (0.0, sl.W_RCE, sl.W_REG)):
        if reg == "none" and w_ce == w_rce == 0.0:
            continue  # (no term at all: the total has no graph)
        total, grad, v = sl.total_and_grad(logits, soft, w_ce, w_rce, w_reg, reg, trunc)
        r = _run(out, rows, w_ce, w_rce, w_reg, reg, trunc)
        what = f"{case} {reg} trunc={trunc} weights {(w_ce, w_rce, w_reg)}"
        print(what, r["total"], float(total))
        assert sl.value_close(r["total"], total), (what, r["total"], float(total))
        assert sl.value_close(r["ce"], v["ce"]) and sl.value_close(r["rce"], v["rce"]), what
        assert sl.value_close(r["reg"], v[reg.lower()] if reg != "none" else 0.0), what
        sl.grad_close(r["grad"], grad, 1e-5, what)


def test_kernels_at_head_size(golden):
    g = golden("g29_soft_losses")
    logits, soft = sl.head_case(g["head_seed"], g["head_shape"])
    out, rows = _head_out(logits), _rows(soft)
    for key, w_ce, w_rce, w_reg, trunc in PAIRS:
        r = _run(out, rows, w_ce, w_rce, w_reg, "MRKLD", trunc)
        total, grad, _ = sl.total_and_grad(logits, soft, w_ce, w_rce, w_reg, "MRKLD", trunc)
        print("head", key, r["total"], float(total), float(g[f"head_{key}"]))
        assert sl.value_close(r["total"], g[f"head_{key}"]) and sl.value_close(r["total"], total), key
        sl.grad_close(r["grad"], grad, 1e-5, f"head grad {key}")
        ref, mine = g[f"head_grad_{key}"], digest(r["grad"], 4096)
        scale = float(g[f"head_grad_{key}_absmax"])
        np.testing.assert_allclose(mine[2:], ref[2:], rtol=0, atol=1e-5 * scale, err_msg=key)
        np.testing.assert_allclose(mine[:2], ref[:2], rtol=0, atol=1e-5 * ref[1], err_msg=key)
        if key == "lc":
            sl.ce_grad_close(r["grad"], grad, "head CE gradient")
            assert int((r["grad"] != 0).sum()) == int(g["head_grad_lc_nonzero"]) >= 1


def test_two_runs_are_bit_identical(golden):
    g = golden("g29_soft_losses")
    logits, soft = sl.head_case(g["head_seed"], g["head_shape"])
    logits = logits.abs() + 0.1  # (finite values: NaN != NaN)
    a = _run(_head_out(logits), _rows(soft), 0.1, 1.0, 0.1, "MRENT", False)
    b = _run(_head_out(logits), _rows(soft), 0.1, 1.0, 0.1, "MRENT", False)
    assert all(math.isfinite(a[k]) and a[k] == b[k] for k in ("total", "ce", "rce", "reg"))
    assert torch.equal(a["grad"], b["grad"])


def test_layouts_agree(golden):
    """Padded pixel-major logits (ld 32, 24, K) and a plain NCHW tensor; the soft target as the [N,K] map (taken as it is), a
    view of it, a plain NCHW tensor and padded rows: same values, same gradient, bit for bit."""
    g = golden("g29_soft_losses")
    logits, soft = case_of(g, "positive")
    K = logits.shape[1]
    rows = _rows(soft)
    runs = [_run(_head_out(logits, ld), rows, 0.1, 1.0, 0.1, "MRENT", False) for ld in (32, 24, K)]
    runs.append(_run(logits.to(DEV).contiguous(), rows, 0.1, 1.0, 0.1, "MRENT", False))
    B, _, h, w = logits.shape
    padded = torch.zeros(rows.shape[0], 32, device=DEV)
    padded[:, :K] = rows
    for target in (rows.reshape(B, h, w, K).permute(0, 3, 1, 2), soft.to(DEV).contiguous(), padded[:, :K]):
        runs.append(_run(_head_out(logits), target, 0.1, 1.0, 0.1, "MRENT", False))
    for r in runs[1:]:
        assert all(r[k] == runs[0][k] for k in ("total", "ce", "rce", "reg"))
        assert torch.equal(r["grad"], runs[0]["grad"])
    # the [N,K] map and padded rows are read in place
    from onda_amd.ops.loss import soft_rows_of
    assert soft_rows_of(rows, rows.shape[0], K, rows.device)[0].data_ptr() == rows.data_ptr()
    view, ld = soft_rows_of(padded[:, :K], rows.shape[0], K, rows.device)
    assert view.data_ptr() == padded.data_ptr() and ld == 32
    # an integer target (what loss_calc's .long() hands on) is its float value
    a = _run(_head_out(logits), soft.long().to(DEV), 1.0, 0.0, 0.0, "none", False)
    b = _run(_head_out(logits), rows, 1.0, 0.0, 0.0, "none", True)
    assert a["total"] == b["total"] and torch.equal(a["grad"], b["grad"])


def test_argument_checks():
    from onda_amd import _lib
    from onda_amd.ops.core import _p, _stream
    lib = _lib.load()
    x, t = torch.zeros(256, 32, device=DEV), torch.zeros(256, 19, device=DEV)
    res, ws, dl = torch.zeros(8, device=DEV), torch.zeros(16, device=DEV), torch.zeros(256, 32, device=DEV)
    fwd = lambda **k: lib.onda_soft_loss_fwd(_p(k.get("x", x)), k.get("ldl", 32), _p(k.get("t", t)), k.get("lds", 19), 1,  # noqa: E731
                                             k.get("reg", 1), 0.1, 1.0, 0.1, _p(res), _p(ws), 256, k.get("K", 19), _stream())
    bwd = lambda **k: lib.onda_soft_loss_bwd(_p(x), k.get("ldl", 32), _p(k.get("t", t)), k.get("lds", 19), 1, k.get("reg", 1),  # noqa: E731
                                             0.1, 1.0, 0.1, None, _p(dl), 256, k.get("K", 19), _stream())
    for f in (fwd, bwd):
        assert f() == 0
        assert f(K=33) == -1 and f(lds=18) == -1 and f(ldl=18) == -1 and f(reg=3) == -1 and f(t=None) == -1
    assert bwd(ldl=33) == -1
    assert lib.onda_soft_loss_fwd(x.data_ptr() + 2, 32, _p(t), 19, 1, 1, 0.1, 1.0, 0.1, _p(res), _p(ws), 256, 19, _stream()) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ framework functions
def test_framework_functions_run_on_the_kernels(golden, monkeypatch):
    from onda_amd.framework.utils.func import loss_calc
    from onda_amd.framework.utils.loss import CXE, cross_entropy_2d, rce
    from onda_amd.ops import loss as oloss
    seen, real = [], oloss.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(oloss, "call", spy)
    g = golden("g29_soft_losses")
    for case in ("mixed", "positive"):
        logits, soft = case_of(g, case)
        target = soft.to(DEV)
        for key, fn in (("lc", lambda x: loss_calc(x, target, DEV, soft=True)), ("ce", lambda x: cross_entropy_2d(x, target, soft=True)),
                        ("ce", lambda x: CXE(x, target)), ("rce", lambda x: rce(x, target, DEV, soft=True))):
            x = logits.to(DEV).requires_grad_(True)
            v = fn(x)
            v.backward()
            assert sl.value_close(v.item(), g[f"{case}_{key}"]), (case, key, v.item())
            sl.grad_close(x.grad, torch.from_numpy(g[f"{case}_grad_{key}"]), 1e-5, f"{case} {key}")
    assert set(seen) == {"onda_soft_loss_fwd", "onda_soft_loss_bwd"}, set(seen)


# ------------------------------------------------------------------------------------------------ full steps
def _adapter(tmp_path, **over):
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.synthetic import fill_state_dict
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, str(tmp_path), batch_size=2)
    for k, v in over.items():
        spec[k] = v
    model = get_model(cfg, 19)
    fill_state_dict(model, 1, 3.0)
    return get_adapt_method(cfg)(model, cfg, spec)


def _spy_on_loss_calls(monkeypatch):
    from onda_amd.ops import loss as oloss
    seen, real = [], oloss.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(oloss, "call", spy)
    return seen


def test_full_step_with_soft_labels_golden(golden, tmp_path, monkeypatch):
    """Two hybrid_proDA steps (+update_ema) at 128x64, B=2, dynamic branch, SOFT_LABELS: True and RCE_BETA = 300 (G30), by the
    rules of test_full_step_with_mrent_and_js_golden: soft map, labels off the ties, log (a NaN of the reference is a NaN here,
    rce_loss finite), prototypes and the weight updates."""
    g = golden("g30_step_soft")
    assert float(g["ratio_vs_hard"]) >= 0.2 and float(g["ratio_vs_g7"]) >= 0.2  # what makes the 0.02 below mean something
    seen = _spy_on_loss_calls(monkeypatch)
    da = _adapter(tmp_path, SOFT_LABELS=True, RCE_BETA=sl.G30_RCE_BETA)
    prev = {}

    def check(s, log, soft):
        if s < 0:
            np.testing.assert_allclose(da.prototypes.prototypes.cpu().numpy(), g["proto0"], rtol=1e-3, atol=1e-4)
            for who, mod in (("student.", da.model), ("teacher.", da.ema_model)):
                for k, v in mod.state_dict().items():
                    prev[who + k] = digest(v.float(), 64)[2:]
            return
        assert not any(torch.is_tensor(v) and (v.requires_grad or v.grad_fn is not None) for v in log.values())
        assert int(g[f"branch{s}"]) == da.model_select.current
        assert (soft.cpu() - torch.from_numpy(g[f"soft{s}"])).abs().max() < 2e-3
        top2 = torch.from_numpy(g[f"soft{s}"]).topk(2, dim=1).values
        decided = ((top2[:, 0] - top2[:, 1]) > 4e-3).numpy()
        mine_labels = soft.argmax(1).to(torch.uint8).cpu().numpy()
        assert np.array_equal(mine_labels[decided], g[f"labels{s}"][decided])
        ref = json.loads(str(g[f"log{s}_json"]))
        assert math.isnan(ref["ce_loss"]) and math.isnan(ref["sym_loss"]) and math.isnan(ref["Total target loss"])
        for k, v in ref.items():
            mine = log[k]
            mine = mine.item() if isinstance(mine, torch.Tensor) else float(mine)
            print(f"step {s}: {k}: {mine!r} / {v!r}")
            if math.isnan(v):
                assert math.isnan(mine), (s, k, mine)
            else:
                assert _log_close(mine, v, k, s, soft[0, 0].numel() * soft.shape[0]), (s, k, mine, v)
        rce_loss = log["rce_loss"]
        assert math.isfinite(rce_loss.item() if torch.is_tensor(rce_loss) else rce_loss)
        np.testing.assert_allclose(da.prototypes.prototypes.cpu().numpy(), g[f"proto{s + 1}"], rtol=1e-3, atol=1e-4)
        names, dg = list(g[f"state_names{s}"]), g[f"state_digest{s}"]
        num = den = 0.0
        for who, mod in (("student.", da.model), ("teacher.", da.ema_model)):
            for k, v in mod.state_dict().items():
                if not v.is_floating_point() or v.dim() == 0:
                    continue
                row = dg[names.index(who + k)][2:]
                mine = digest(v.float(), 64)[2:]
                num += ((mine - row) ** 2).sum()
                den += ((row - prev[who + k]) ** 2).sum()
                prev[who + k] = row
        print(f"step {s}: weight update, relative L2 {(num / den) ** 0.5:.4e}")
        assert (num / den) ** 0.5 <= (0.02 if s == 0 else 0.6), (s, (num / den) ** 0.5)
    check.steps = (0, 1)
    _two_steps(da, check)
    assert seen.count("onda_soft_loss_fwd") == 2 and seen.count("onda_soft_loss_bwd") == 2  # one launch each way a step
    # the hard-label kernels see the source-replay pass alone (one seg_loss a step: its labels are hard), never the target
    assert seen.count("onda_seg_loss_fwd") == 2 and not any(n.startswith("onda_target_loss") for n in seen), seen
    assert all(torch.isfinite(p).all() for p in da.model.parameters())


def test_proto_advent_step_with_soft_labels(tmp_path, monkeypatch):
    """One adv_proDA step with SOFT_LABELS: True: the target loss goes through the soft-loss kernels alone; rce_loss is finite,
    sym_loss NaN (CE over raw logits), every parameter finite."""
    from onda_amd.framework.model import deeplabv2
    from test_proto_advent_golden import _build, _cfg, _prepare
    cfg, spec = _cfg(tmp_path, "PROTO_ADVENT", False, SOFT_LABELS=True)
    model, da = _build(cfg, spec)
    try:
        src, trg, _ = _prepare(da.proto_model, 8)
        seen = _spy_on_loss_calls(monkeypatch)
        da.advent.optimizer.zero_grad()
        da.advent.optimizer_d_main.zero_grad()
        da.advent.optimizer_d_aux.zero_grad()
        da.advent.adjust_learning_rate(0, 6)
        log = da.step(src[0], trg[0])
        da.proto_model.update_ema()
    finally:
        deeplabv2.drop_mask_fn = deeplabv2._default_drop_mask
    torch.cuda.synchronize()
    assert seen.count("onda_soft_loss_fwd") == 1 and seen.count("onda_soft_loss_bwd") == 1, seen
    assert not any(n.startswith(("onda_seg_loss", "onda_target_loss")) for n in seen), seen
    assert math.isfinite(float(log["rce_loss"])) and float(log["rce_loss"]) > 0
    assert math.isnan(float(log["sym_loss"])) and math.isnan(float(log["Total target loss"]))
    assert tuple(trg[0]["stored_predictions"].shape) == (2, 19, 9, 17)
    for module in (model, da.proto_model.ema_model, da.advent.d_main):
        assert all(torch.isfinite(p).all() for p in module.parameters())


def test_soft_labels_with_js_raises_before_any_launch(tmp_path, monkeypatch):
    from onda_amd.ops import conv, core, disc, limbs, loss, norm, tables
    from onda_amd.synthetic import synth_batch
    da = _adapter(tmp_path, SOFT_LABELS=True, JS_D=1.0)
    src, trg = synth_batch(2, 64, 128, seed=100), synth_batch(2, 64, 128, seed=200)
    launched = []
    for mod in (conv, core, disc, limbs, loss, norm, tables):  # (each imports `call` under its own name)
        if hasattr(mod, "call"):
            monkeypatch.setattr(mod, "call", lambda name, *a, _real=mod.call: launched.append(name) or _real(name, *a))
    with pytest.raises(RuntimeError, match=r"SOFT_LABELS.*JS_D.*loss\.py:62-85"):
        da.step([src], trg)
    with pytest.raises(RuntimeError, match=r"SOFT_LABELS.*JS_D.*loss\.py:62-85"):
        da.pseudolabel_loss(trg)
    assert not launched and "stored_predictions" not in trg


@pytest.mark.parametrize("setting", ["unset", False, None])
def test_default_step_keeps_the_seg_loss_kernels(tmp_path, monkeypatch, setting):
    """SOFT_LABELS unset, False or None: the step launches what it launched before -- seg_loss, never soft_loss."""
    seen = _spy_on_loss_calls(monkeypatch)
    da = _adapter(tmp_path, **({} if setting == "unset" else {"SOFT_LABELS": setting}))

    def check(s, log, soft):
        if s == 0:
            assert math.isfinite(float(log["ce_loss"])) and math.isfinite(float(log["sym_loss"]))
    check.steps = (0,)
    _two_steps(da, check)
    torch.cuda.synchronize()
    assert "onda_seg_loss_fwd" in seen and "onda_seg_loss_bwd" in seen
    assert not any(n.startswith("onda_soft_loss") for n in seen), seen
