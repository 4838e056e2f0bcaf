"""GPU: the EWC anchor penalty on the device -- onda_sqdiff_multi (the value) and onda_sgd_anchor_multi (the gradient, formed
inside the optimizer's launch) through ops.sqdiff_multi / ops.sgd_multi -- against the float64 restatement and the bounds of
tests/ewc_fp64.py, bit for bit against onda_sgd_multi fed the gradient autograd would have left, and the adaptation step that
runs on them against the reference's (fixture G20).  Every test prints its figures before it asserts."""
import json

import numpy as np
import pytest
import torch

import ewc_fp64 as E
from conftest import digest

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
HALF = E.LAMBDA / 2


def _dev(t, off=0):
    """A CPU tensor on the device, starting `off` floats past an allocation's (16-byte aligned) start."""
    flat = torch.empty(t.numel() + off + 4, device=DEV)
    view = flat[off:off + t.numel()]
    view.copy_(t)
    assert (view.data_ptr() % 16 == 0) == (off % 4 == 0)
    return view


def _columns(i, kind):
    """theta0, theta, g0, buf (lists of device tensors at the case's pointer offsets) and the learning rates."""
    rows, offs = E.inputs(i, kind), [off for _, off in E.CASES[i]]
    cols = [[_dev(r[c], off) for r, off in zip(rows, offs)] for c in range(4)]
    return (*cols, [r[4] for r in rows])


def test_block_size_is_the_librarys():
    from onda_amd._lib import query
    assert query("onda_multi_tensor_block") == E.BLK


# ------------------------------------------------------------------------------------------------ the penalty's value
@pytest.mark.parametrize("i,kind", E.runs(), ids=lambda v: str(v))
def test_penalty_value(i, kind):
    from onda_amd import ops
    t0, t, _, _, _ = _columns(i, kind)
    pairs = list(zip(t0, t))
    got = ops.sqdiff_multi(pairs, HALF)
    assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
    E.check_penalty(got.item(), i, kind, "onda_sqdiff_multi")
    cache = {}
    again = [ops.sqdiff_multi(pairs, HALF, cache) for _ in range(2)]  # the second call reuses table and workspace
    assert all(torch.equal(a, got) for a in again), [got.item()] + [a.item() for a in again]
    swapped = ops.sqdiff_multi([(b, a) for a, b in pairs], HALF)  # (a - b)^2: symmetric, bit for bit
    assert torch.equal(swapped, got)


def test_penalty_of_all_cases_in_one_launch():
    """Every tensor of every case as ONE table (10 entries, 13 workgroups): the sum of the cases' values."""
    from onda_amd import ops
    pairs, ref = [], 0.0
    for i in range(len(E.CASES)):
        t0, t, _, _, _ = _columns(i, "far")
        pairs += list(zip(t0, t))
        ref += E.reference(i, "far")
    got = ops.sqdiff_multi(pairs, HALF).item()
    err = E.penalty_error(got, ref)
    print(f"all cases, far: {got:.9g} ref {ref:.9g} rel {err:.3e} (bound {E.BOUNDS['penalty']:.1e})")
    assert err <= E.BOUNDS["penalty"]


# ------------------------------------------------------------------------------------------------ the anchored optimizer launch
def _items(p, g, b, lrs, times, fresh):
    return [(pj, gj, bj, lr, times, fresh) for pj, gj, bj, lr in zip(p, g, b, lrs)]


@pytest.mark.parametrize("i,kind", E.runs(), ids=lambda v: str(v))
def test_anchored_sgd_is_plain_sgd_on_the_gradient_autograd_leaves(i, kind):
    """Parameters and momentum buffers after onda_sgd_anchor_multi equal, bit for bit, what onda_sgd_multi makes of
    g0 + contribution -- the contribution formed by torch's float32 elementwise kernels on the device (IEEE, no
    re-association: a reference, not the code under test).  And the update is the float64 restatement's within BOUNDS."""
    from onda_amd import ops
    offs = [off for _, off in E.CASES[i]]
    for times in E.TIMES:
        for fresh in (0, 1):
            t0, p, g0, b, lrs = _columns(i, kind)
            _, p_ref, _, b_ref, _ = _columns(i, kind)
            g_ref = [_dev(g + E.contribution32(E.LAMBDA, a, q), off) for g, a, q, off in zip(g0, t0, p_ref, offs)]
            ops.sgd_multi(_items(p, g0, b, lrs, times, fresh), E.MOMENTUM, E.WD, 1.0, t0, HALF)
            ops.sgd_multi(_items(p_ref, g_ref, b_ref, lrs, times, fresh), E.MOMENTUM, E.WD, 1.0)
            for j, (a, r, ba, br) in enumerate(zip(p, p_ref, b, b_ref)):
                assert torch.equal(a, r), (times, fresh, j, int((a != r).sum()))
                assert torch.equal(ba, br), (times, fresh, j, int((ba != br).sum()))
            E.check_step(p, i, kind, times, fresh, "onda_sgd_anchor_multi")
            for a, src in zip(t0, E.inputs(i, kind)):  # the anchors are read, never written
                assert torch.equal(a.cpu(), src[0])


@pytest.mark.parametrize("times,fresh", [(1, 0), (3, 1), (4, 0)])
def test_entries_without_an_anchor_are_plain_sgd(times, fresh):
    """anchor = NULL on every entry, and on every other entry, under a grad_scale that is not 1."""
    from onda_amd import ops
    i, kind, scale = 0, "normal", 0.5
    offs = [off for _, off in E.CASES[i]]
    for mixed in (False, True):
        t0, p, g0, b, lrs = _columns(i, kind)
        _, p_ref, _, b_ref, _ = _columns(i, kind)
        anchors = [a if mixed and j % 2 else None for j, a in enumerate(t0)]
        ops.sgd_multi(_items(p, g0, b, lrs, times, fresh), E.MOMENTUM, E.WD, scale, anchors, HALF)
        if mixed:
            # the reference takes the scaled gradients at scale 1: g0 * 0.5 is exact, and with an anchor the sum is rounded
            # once, as in the launch
            g_ref = [_dev(g * scale + (E.contribution32(E.LAMBDA, a, q) if a is not None else 0), off)
                     for g, a, q, off in zip(g0, anchors, p_ref, offs)]
            ops.sgd_multi(_items(p_ref, g_ref, b_ref, lrs, times, fresh), E.MOMENTUM, E.WD, 1.0)
        else:
            ops.sgd_multi(_items(p_ref, g0, b_ref, lrs, times, fresh), E.MOMENTUM, E.WD, scale)
        for a, r, ba, br in zip(p, p_ref, b, b_ref):
            assert torch.equal(a, r) and torch.equal(ba, br), (mixed, int((a != r).sum()))


def test_a_parameter_no_loss_reached_gets_the_penalty_alone():
    """grad = None with an anchor: the reference's backward() leaves the penalty's term alone in .grad."""
    from onda_amd import ops
    i, kind, times = 1, "normal", 3
    offs = [off for _, off in E.CASES[i]]
    t0, p, _, b, lrs = _columns(i, kind)
    _, p_ref, _, b_ref, _ = _columns(i, kind)
    g_ref = [_dev(torch.zeros_like(q) + E.contribution32(E.LAMBDA, a, q), off) for a, q, off in zip(t0, p_ref, offs)]
    ops.sgd_multi(_items(p, [None] * len(p), b, lrs, times, 1), E.MOMENTUM, E.WD, 1.0, t0, HALF)
    ops.sgd_multi(_items(p_ref, g_ref, b_ref, lrs, times, 1), E.MOMENTUM, E.WD, 1.0)
    for a, r, ba, br in zip(p, p_ref, b, b_ref):
        assert torch.equal(a, r) and torch.equal(ba, br)


def test_replay_sgd_hands_the_anchors_over():
    """ReplaySGD with anchor_of: duplicates replayed on ONE anchored gradient, against torch's loop on g0 + contribution."""
    from onda_amd.optim import ReplaySGD
    rows = E.inputs(1, "normal")
    params = [torch.nn.Parameter(r[1].to(DEV)) for r in rows]
    anchors = [r[0].to(DEV) for r in rows]
    for p, r in zip(params, rows):
        p.grad = r[2].to(DEV)
    opt = ReplaySGD([{"params": [params[0], params[1], params[0], params[2], params[0]]}], lr=1e-2, momentum=E.MOMENTUM,
                    weight_decay=E.WD, anchor_of={id(p): a for p, a in zip(params, anchors)}, half_lambda=HALF)
    opt.step()
    for p, r, times in zip(params, rows, (3, 1, 1)):
        want = E.sgd_step64(E.LAMBDA, r[0], r[1], r[2], r[3], 1e-2, times, 1)[0]
        err = float((p.detach().double().cpu() - want).norm() / (want - r[1].double()).norm())
        print(f"ReplaySGD times {times}: update rel-L2 {err:.3e} (bound {E.BOUNDS['step']:.1e})")
        assert err <= E.BOUNDS["step"]


# ------------------------------------------------------------------------------------------------ the guards
def test_argument_errors_come_before_any_launch():
    from onda_amd import _lib
    from onda_amd.ops import tables
    lib = _lib.load()
    t0, t, g0, b, lrs = _columns(2, "normal")
    n = t[0].numel()
    stream = torch.cuda.current_stream().cuda_stream
    table = tables._table([_lib.OndaSqdiffEntry(t0[0].data_ptr(), t[0].data_ptr(), n, 0)], _lib.OndaSqdiffEntry, DEV)
    ws, result = torch.full((4,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
    bad = [(None, 1, 1, ws, result), (table, 0, 1, ws, result), (table, -1, 1, ws, result), (table, 1, 0, ws, result),
           (table, 1, -1, ws, result), (table, 1, 1, None, result), (table, 1, 1, ws, None)]
    for tb, cnt, blocks, w, r in bad:
        rc = lib.onda_sqdiff_multi(tb.data_ptr() if tb is not None else None, cnt, HALF, blocks,
                                   w.data_ptr() if w is not None else None, r.data_ptr() if r is not None else None, stream)
        assert rc == -1, (cnt, blocks, rc)
    assert lib.onda_sqdiff_multi_ws(-3) == 0 and lib.onda_sqdiff_multi_ws(5) >= 5
    torch.cuda.synchronize()
    assert bool((ws == 7.0).all()) and result.item() == 7.0
    before_p, before_b = t[0].clone(), b[0].clone()
    table = tables._table([_lib.OndaSgdAnchorEntry(t[0].data_ptr(), g0[0].data_ptr(), b[0].data_ptr(), t0[0].data_ptr(), n, 1e-2, 1,
                                                  0, 0)], _lib.OndaSgdAnchorEntry, DEV)
    for tb, cnt, blocks in ((None, 1, 1), (table, 0, 1), (table, -1, 1), (table, 1, 0), (table, 1, -1), (table, 1, 1 << 31)):
        rc = lib.onda_sgd_anchor_multi(tb.data_ptr() if tb is not None else None, cnt, E.MOMENTUM, E.WD, 1.0, HALF, blocks, stream)
        assert rc == -1, (cnt, blocks, rc)
    torch.cuda.synchronize()
    assert torch.equal(t[0], before_p) and torch.equal(b[0], before_b)


# ------------------------------------------------------------------------------------------------ the step
@pytest.fixture(params=["f16x2", "f32"])
def conv_mode(request):
    from onda_amd import ops
    old, ops.CONV_MODE = ops.CONV_MODE, request.param
    yield request.param
    ops.CONV_MODE = old


def _log_close(mine, ref, key, step, npix):
    """The project's rule for log scalars (tests/test_hip_model.py): 5e-3 relative; one pixel on the count keys of the SECOND
    step, which sits behind one SGD step through train-mode BatchNorm."""
    if mine == pytest.approx(ref, rel=5e-3, abs=1e-5):
        return True
    if step >= 1 and ("agreement" in key or "percentage" in key or "pixel_num" in key):
        one = 1.0 if "pixel_num" in key else 1.0 / npix
        return abs(mine - ref) <= 1.01 * one
    return False


def _adapter(tmp_path, lam):
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.synthetic import fill_state_dict
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, str(tmp_path), batch_size=2)
    if lam is not None:
        spec.MODEL_REGULARIZATION = lam
    model = get_model(cfg, 19)
    fill_state_dict(model, 1, 3.0)
    return get_adapt_method(cfg)(model, cfg, spec)


def _perturb(model, seed):
    """tests/golden/make_golden_ewc.py's draws, on the CPU generator, copied."""
    with torch.no_grad():
        for i, p in enumerate(model.parameters()):
            g = torch.Generator().manual_seed(seed + i)
            p += (1e-2 * torch.randn(p.shape, generator=g)).to(p.device)


def _steps(da, n, after):
    """G7's recipe: same batches, same CPU mask draws; after(s, log, soft) behind every step + update_ema."""
    from onda_amd.framework.model import deeplabv2
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.synthetic import synth_batch
    from oracle import model as omodel
    src = [synth_batch(2, 64, 128, seed=100 + i) for i in range(2)]
    trg = [synth_batch(2, 64, 128, seed=200 + i) for i in range(2)]
    torch.manual_seed(123)
    masks = [omodel.draw_drop_mask(2) for _ in range(8)]
    it = iter(masks)
    deeplabv2.drop_mask_fn = lambda B, C, p, dev: next(it).to(dev)
    try:
        da.update_dynamic()
        switch_batch_statistics(da.model, False)
        da.calculate_prototypes(src, save=False)
        switch_batch_statistics(da.model, True)
        after(-1, None, None)
        da.optimizer.zero_grad()
        for s in range(n):
            da.adjust_learning_rate(s, 6)
            log = da.step([src[s]], trg[s])
            da.update_ema()
            after(s, log, trg[s]["stored_predictions"])
    finally:
        deeplabv2.drop_mask_fn = deeplabv2._default_drop_mask


def test_full_step_with_model_regularization_golden(golden, tmp_path, conv_mode):
    """Two hybrid_proDA steps (+update_ema) at 128x64, B=2 with MODEL_REGULARIZATION = G20's lambda, the student moved off
    the static model first: log scalars under the project's rule, the weight updates under test_full_step_golden's bars,
    and "model regularization" itself within BOUNDS of the reference's where both sides read the same bits (step 0; in
    step 1 each side's penalty is that of its own updated weights, and the log rule holds it)."""
    g = golden("g20_ewc")
    lam = float(g["lambda"])
    da = _adapter(tmp_path, lam)
    _perturb(da.model, int(g["perturb_seed"]))
    prev = {}

    def after(s, log, soft):
        if s < 0:
            np.testing.assert_allclose(da.prototypes.prototypes.cpu().numpy(), g["proto0"], rtol=1e-3, atol=1e-4)
            np.testing.assert_allclose(da.prototypes.counter.cpu().numpy(), g["counter0"])
            for who, mod in (("student.", da.model), ("teacher.", da.ema_model)):
                for k, v in mod.state_dict().items():
                    prev[who + k] = digest(v.float(), 64)[2:]
            return
        assert not any(torch.is_tensor(v) and (v.requires_grad or v.grad_fn is not None) for v in log.values())
        assert int(g[f"branch{s}"]) == da.model_select.current
        assert (soft.cpu() - torch.from_numpy(g[f"soft{s}"])).abs().max() < 2e-3
        ref = json.loads(str(g[f"log{s}_json"]))
        mine_pen, ref_pen = float(log["model regularization"]), ref["model regularization"]
        rel = abs(mine_pen - ref_pen) / ref_pen
        print(f"[{conv_mode}] step {s}: model regularization {mine_pen:.9g}, reference {ref_pen:.9g}, rel {rel:.3e} "
              f"(bound {E.BOUNDS['penalty']:.1e} in step 0); Total target loss {float(log['Total target loss']):.7g}, "
              f"reference {ref['Total target loss']:.7g}")
        assert mine_pen > 0 and ref_pen > 0
        if s == 0:
            assert rel <= E.BOUNDS["penalty"], (mine_pen, ref_pen, rel)
        assert float(log["sym_loss"]) == float(log["Total target loss"])
        for k, v in ref.items():
            mine = log[k]
            mine = mine.item() if isinstance(mine, torch.Tensor) else float(mine)
            assert _log_close(mine, v, k, s, soft[0, 0].numel() * soft.shape[0]), (s, k, mine, v)
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
        dist = (num / den) ** 0.5
        print(f"[{conv_mode}] step {s}: weight update against the reference's, rel-L2 over the digests {dist:.4f} "
              f"(bound {0.02 if s == 0 else 0.6})")
        assert dist <= (0.02 if s == 0 else 0.6), (s, dist)
    _steps(da, 2, after)


def test_penalty_in_the_step_is_the_restatement_of_its_own_weights(tmp_path):
    """"model regularization" of a step against the float64 restatement on the weights that step started from."""
    lam = 1e-4
    da = _adapter(tmp_path, lam)
    _perturb(da.model, 7)
    want = {}

    def after(s, log, soft):
        if s >= 0:
            got = float(log["model regularization"])
            err = E.penalty_error(got, want[s])
            print(f"step {s}: model regularization {got:.9g}, float64 {want[s]:.9g}, rel {err:.3e} (bound {E.BOUNDS['penalty']:.1e})")
            assert err <= E.BOUNDS["penalty"]
        want[s + 1] = float(E.penalty64(lam, list(zip(da.static_model.parameters(), da.model.parameters()))))
    _steps(da, 2, after)
    assert want[1] != want[0]


def test_default_step_never_calls_the_new_entry_points(tmp_path, monkeypatch):
    """MODEL_REGULARIZATION unset: the same launches, the same OndaSgdEntry path."""
    from onda_amd.ops import tables
    seen = []
    real = tables.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(tables, "call", spy)
    da = _adapter(tmp_path, None)
    logs = []
    _steps(da, 1, lambda s, log, soft: logs.append(log))
    torch.cuda.synchronize()
    assert logs[-1]["model regularization"] == 0
    assert "onda_sgd_multi" in seen and "onda_ema_multi" in seen
    assert "onda_sgd_anchor_multi" not in seen and "onda_sqdiff_multi" not in seen, sorted(set(seen))


def test_regularized_step_calls_each_new_entry_point_once_per_step(tmp_path, monkeypatch):
    """lambda > 0: one penalty launch and one anchored optimizer launch per step, two micro-batches or one."""
    from onda_amd.ops import tables
    from onda_amd.synthetic import synth_batch
    seen = []
    real = tables.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(tables, "call", spy)
    da = _adapter(tmp_path, 1e-4)
    _perturb(da.model, 7)
    _steps(da, 1, lambda s, log, soft: None)
    assert seen.count("onda_sqdiff_multi") == 1 and "onda_sgd_multi" not in seen
    n_opt = seen.count("onda_sgd_anchor_multi")
    assert n_opt >= 1
    del seen[:]
    shards = [([synth_batch(2, 64, 128, seed=110 + i)], synth_batch(2, 64, 128, seed=210 + i)) for i in range(2)]
    log = da.step_sharded(shards)
    torch.cuda.synchronize()
    assert seen.count("onda_sqdiff_multi") == 1 and seen.count("onda_sgd_anchor_multi") == n_opt and "onda_sgd_multi" not in seen
    assert float(log["model regularization"]) > 0
