"""GPU: the device side of the static / dynamic switch -- switch_step_kernel behind DeviceSwitch.step, select_prior_kernel,
gate_scalar_kernel (csrc/switch.hip) -- against this repository's host path, bit for bit (tests/switch_np.py holds the
standard, the scenarios and the comparator; tests/test_switch_reference.py pins the standard to the reference and shows that
no scenario is vacuous).  The device state is copied device-side into a preallocated trace after every step and compared once
at the end: no read-back inside a run."""
import ctypes

import numpy as np
import pytest
import torch

import switch_np as S

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the device leg
def _switch(limit, exp_const, dev_func, gray, thr, start=0, use_exp=False):
    from onda_amd.framework.utils.monitoring import DeviceSwitch
    return DeviceSwitch(DEV, limit, exp_const, dev_func, gray, thr, start, use_exp)


def _device_trajectory(sw, samples, writes=None, select=None, after_step=None):
    """{field: array over the steps} of DeviceSwitch.step on the device tensor `samples` (float64 or float32), plus "flag".
    `writes` go through `select` (a model_select whose device_switch is `sw`) before the step they are keyed by; what the
    device holds right after each write is returned under "written" (current, current_dev, flag per write)."""
    n = len(samples)
    trace_s = torch.zeros(n, 4, dtype=torch.float64, device=DEV)
    trace_i = torch.zeros(n, 5, dtype=torch.int32, device=DEV)
    trace_f = torch.zeros(n, dtype=torch.int32, device=DEV)
    written = torch.zeros(max(len(writes or ()), 1), 3, dtype=torch.int32, device=DEV)
    for i in range(n):
        if writes and i in writes:
            select.current, select.current_dev = writes[i]
            j = sorted(writes).index(i)
            written[j, :2] = sw.istate[2:4]
            written[j, 2] = sw.flag[0]
        flag = sw.step(samples[i])
        assert flag is sw.flag
        trace_s[i] = sw.state[:4]
        trace_i[i] = sw.istate[:5]
        trace_f[i] = sw.flag[0]
        if after_step is not None:
            after_step(i)
    s, it = trace_s.cpu().numpy(), trace_i.cpu().numpy().astype(np.int64)
    return {"exp": s[:, 0], "avg": s[:, 1], "dev": s[:, 2], "confidence": s[:, 3], "count": it[:, 0], "current": it[:, 2],
            "current_dev": it[:, 3], "steps": it[:, 4], "flag": trace_f.cpu().numpy().astype(np.int64),
            "written": written.cpu().numpy().astype(np.int64)}


def _run(sc):
    sw = _switch(sc.limit, sc.exp_const, sc.dev_func, sc.gray, sc.thr, sc.start, sc.use_exp)
    seq = S.sequence(sc.limit)
    samples = torch.from_numpy(seq.astype(np.float32) if sc.f32 else np.array(seq)).to(DEV)
    got = _device_trajectory(sw, samples)
    assert np.array_equal(got["flag"], got["current"])
    r = sw.read()
    assert r["steps"] == len(seq) and r["count"] == sc.limit and r["current"] == got["current"][-1]
    return got


# ------------------------------------------------------------------------------------------------ the windows
@pytest.mark.parametrize("sc", S.base_scenarios(), ids=lambda s: s.id)
def test_every_window_and_trend_function(sc):
    """18 limits x 3 trend functions, thr > 0, use_exp off, start 0, float64 samples."""
    S.check(_run(sc), S.standard(sc), sc.id)


@pytest.mark.parametrize("sc", S.varied_scenarios(), ids=lambda s: s.id)
def test_one_variation_at_a_time(sc):
    """Limits 9, 130, 258: use_exp, a negative threshold (the two one-sided tests are not |dev| > thr), a zero threshold,
    start = 1, float32 samples (the standard is fed the widened values)."""
    S.check(_run(sc), S.standard(sc), sc.id)


# ------------------------------------------------------------------------------------------------ write-through
def test_model_select_setters_write_through():
    """model_select.current / .current_dev assigned at two fixed steps on both legs: on the device leg through the
    device_switch hook, which writes istate and the flag.  The device holds the written values right after each write, and
    trajectories and flag stay equal to the host's afterwards."""
    from onda_amd.framework.domain_adaptation.methods.prototypes_hybrid_switch import model_select
    L = S.WRITE_LIMIT
    for func in S.FUNCS:
        cfg = (L, S.exp_const(L), func, S.GRAY, S.threshold(L))
        want = S.host_trajectory(S.sequence(L), *cfg, writes=S.WRITES)
        sw = _switch(*cfg)
        sel = model_select(0, list(S.GRAY), S.threshold(L))
        sel.device_switch = sw
        got = _device_trajectory(sw, torch.from_numpy(np.array(S.sequence(L))).to(DEV), writes=S.WRITES, select=sel)
        S.check(got, want, f"write-through {func}")
        assert np.array_equal(got["flag"], want["current"])
        for j, step in enumerate(sorted(S.WRITES)):
            cur, cur_dev = S.WRITES[step]
            assert got["written"][j].tolist() == [cur, cur_dev, cur]
        assert sel.current == int(want["current"][-1]) and sel.current_dev == int(want["current_dev"][-1])  # reads come from the device


# ------------------------------------------------------------------------------------------------ scripted exact cases
def _script(script, dtype=torch.float64):
    seq, want = S.script_expectation(script)
    c = S.SCRIPT_CFG
    sw = _switch(c["limit"], c["exp_const"], c["dev_func"], c["gray"], c["thr"], script["start"])
    return sw, seq, want, (lambda hook=None: _device_trajectory(sw, torch.from_numpy(seq).to(DEV).to(dtype), after_step=hook))


@pytest.mark.parametrize("script", (S.SCRIPT_A, S.SCRIPT_B), ids=("A", "B"))
@pytest.mark.parametrize("dtype", (torch.float64, torch.float32), ids=("f64", "f32"))
def test_scripted_edges_against_hand_written_expectations(script, dtype):
    """Limit 3, "mean", dyadic samples: a confidence exactly on gray_lo and exactly on gray_hi (neither strict test fires ->
    current_dev), a trend exactly thr and exactly -thr (not significant) -- tests/switch_np.py, SCRIPT_A / SCRIPT_B."""
    sw, seq, want, run = _script(script, dtype)
    got = run()
    S.check(got, want, "script")
    assert np.array_equal(got["flag"], want["current"])


# ------------------------------------------------------------------------------------------------ NaN
@pytest.mark.parametrize("func", S.FUNCS)
def test_a_nan_sample_is_nan_for_limit_steps_as_on_the_host(func):
    """One NaN before the window of 9 is full and one after: median, trend and the machine's decisions are the host's at
    every step -- NaN while the sample is in the window (np.median, np.sum), finite again once it has left."""
    L = S.NAN_LIMIT
    seq = S.nan_samples()
    cfg = (L, S.exp_const(L), func, S.GRAY, S.threshold(L))
    want = S.host_trajectory(seq, *cfg)
    got = _device_trajectory(_switch(*cfg), torch.from_numpy(seq).to(DEV))
    for k in ("avg", "dev"):
        print(func, k, "NaN at steps", np.flatnonzero(np.isnan(got[k])).tolist(), "host", np.flatnonzero(np.isnan(want[k])).tolist())
    S.check(got, want, f"NaN {func}", nan=True)
    assert np.array_equal(got["flag"], want["current"]) and not np.isnan(got["avg"][-12:]).any()


# ------------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_are_refused_before_any_launch(monkeypatch, capfd):
    from onda_amd._lib import call
    monkeypatch.setenv("ONDA_DEBUG_REQUIRE", "1")
    sw = _switch(1025, 0.01, "hamming", S.GRAY, 0.001)
    before = (sw.state.clone(), sw.istate.clone(), sw.flag.clone())
    capfd.readouterr()
    with pytest.raises(RuntimeError, match="ONDA_EINVAL"):
        sw.step(torch.tensor(0.5, device=DEV))
    err = capfd.readouterr().err
    assert err.count("requirement failed") == 1 and "cfg->limit <= MAX_WINDOW" in err, err
    ok = _switch(9, 0.1, "hamming", S.GRAY, 0.001)
    sample = torch.tensor([0.5], device=DEV)
    with pytest.raises(RuntimeError, match="ONDA_EINVAL"):  # a weighted trend function without its taps
        call("onda_switch_step", ok.state.data_ptr(), ok.istate.data_ptr(), sample.data_ptr(), 0, None, ctypes.byref(ok.cfg),
             ok.flag.data_ptr(), torch.cuda.current_stream().cuda_stream)
    err = capfd.readouterr().err
    assert err.count("requirement failed") == 1 and "taps != nullptr" in err, err
    torch.cuda.synchronize()
    assert torch.equal(sw.state, before[0]) and torch.equal(sw.istate, before[1]) and torch.equal(sw.flag, before[2])
    assert ok.read()["steps"] == 0


# ------------------------------------------------------------------------------------------------ the selects
SELECT_SIZES = (1, 1023, 1024, 1025, 637260, 1047552, 1048577, 2549040)  # 1 047 552 = 1023 * 1024: exactly 1024 blocks; above it the grid is capped


@pytest.fixture(scope="module")
def select_data():
    g = torch.Generator().manual_seed(28)
    n = max(SELECT_SIZES) + 128
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


@pytest.mark.parametrize("n", SELECT_SIZES)
def test_select_prior_is_one_rounding_at_every_grid_shape(select_data, n):
    """out = flag ? 0.3 * b : 1.0 * a: torch.equal with the float32 product, the side that is not picked full of NaN.
    637 260 = 4 * 65 * 129 * 19 is the step's own prior (623 blocks); at 2 549 040, four times that, the grid is capped at
    1024 blocks and every thread loops past its first four elements."""
    from onda_amd import ops
    assert 637260 == 4 * 65 * 129 * 19 and 2549040 == 4 * 637260
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    carve = n == 1047552
    a_cpu, b_cpu = select_data[0][:n + 128], select_data[1][:n + 128]
    big_a, big_b = a_cpu.to(DEV), b_cpu.to(DEV)
    a, b = big_a[64:64 + n], big_b[64:64 + n]
    nan = torch.full((n + 128,), float("nan"), device=DEV)[64:64 + n]
    assert a.is_contiguous() and a.data_ptr() == big_a.data_ptr() + 256
    flag.fill_(0)
    out0 = ops.select_prior(flag, a, 1.0, nan, 0.3)
    flag.fill_(1)
    out1 = ops.select_prior(flag, nan, 1.0, b, 0.3)
    assert out0.shape == a.shape and out0.dtype == torch.float32
    assert torch.equal(out0.cpu(), a_cpu[64:64 + n] * 1.0)
    assert torch.equal(out1.cpu(), b_cpu[64:64 + n] * 0.3)
    if carve:  # a and b sit inside larger buffers: the 64 floats on either side of them are what they were
        for big, cpu in ((big_a, a_cpu), (big_b, b_cpu)):
            assert torch.equal(big[:64].cpu(), cpu[:64]) and torch.equal(big[64 + n:].cpu(), cpu[64 + n:])
            assert torch.equal(big[64:64 + n].cpu(), cpu[64:64 + n])


def test_select_prior_takes_non_contiguous_operands():
    """A dense permuted view (the NCHW view of pixel-major rows) and a [:, :19] slice of 32-wide rows, as `a` and as `b`: the
    result is logically the expectation, in the operands' shape."""
    from onda_amd import ops
    g = torch.Generator().manual_seed(29)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    rows_a, rows_b = torch.randn(2, 3, 4, 5, generator=g), torch.randn(2, 3, 4, 5, generator=g)
    wide_a, wide_b = torch.randn(37, 32, generator=g), torch.randn(37, 32, generator=g)
    views = {"permuted": lambda t: t.permute(0, 3, 1, 2), "sliced": lambda t: t[:, :19]}
    for name, (ta, tb) in (("permuted", (rows_a, rows_b)), ("sliced", (wide_a, wide_b))):
        a, b = views[name](ta.to(DEV)), views[name](tb.to(DEV))
        assert not a.is_contiguous()
        for f, want in ((0, views[name](ta) * 1.0), (1, views[name](tb) * 0.3)):
            flag.fill_(f)
            for aa, bb in ((a, b), (a.contiguous(), b), (a, b.contiguous())):
                out = ops.select_prior(flag, aa, 1.0, bb, 0.3)
                assert out.shape == want.shape, name
                assert torch.equal(out.cpu(), want), f"{name}, flag {f}: the result is not the operands' logical order"


def test_gate_scalar_both_flags_both_dtypes():
    from onda_amd import ops
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    vec = torch.tensor([0.25, 0.8671875, 3.0], device=DEV)
    view = vec[1]                                                  # a 0-dim float32 view at an offset
    dbl = torch.tensor(0.1, dtype=torch.float64, device=DEV)      # a float64 scalar: rounded to float32 once
    assert view.dim() == 0 and view.data_ptr() == vec.data_ptr() + 4
    for v, want in ((view, 0.8671875), (dbl, float(np.float32(0.1)))):
        flag.fill_(0)
        off = ops.gate_scalar(flag, v)
        flag.fill_(1)
        on = ops.gate_scalar(flag, v)
        assert off.dim() == 0 and off.dtype == torch.float32 and on.dtype == torch.float32
        assert np.isnan(off.item()) and on.item() == want
    assert vec.tolist() == [0.25, 0.8671875, 3.0]


# ------------------------------------------------------------------------------------------------ one chain item
def test_step_then_select_on_one_stream_without_synchronisation():
    """The scripted limit-3 sequence; after every step select_prior(sw.flag, ...) on the same stream, nothing waited for: each
    result is the prior the host's decision for that step picks."""
    from onda_amd import ops
    g = torch.Generator().manual_seed(30)
    a_cpu, b_cpu = torch.randn(4, 19, generator=g), torch.randn(4, 19, generator=g)
    a, b = a_cpu.to(DEV), b_cpu.to(DEV)
    for script in (S.SCRIPT_A, S.SCRIPT_B):
        sw, seq, want, run = _script(script)
        picked = []
        got = run(lambda i: picked.append(ops.select_prior(sw.flag, a, 1.0, b, 0.3)))
        S.check(got, want, "chain")
        assert len(picked) == len(seq) and set(want["current"].tolist()) == {0, 1}
        for i, out in enumerate(picked):
            assert torch.equal(out.cpu(), b_cpu * 0.3 if want["current"][i] else a_cpu * 1.0), f"step {i}"
