"""GPU: the multi-tensor swap (onda_swap_multi, csrc/loss_proto.hip) through ops.swap_multi, bit for bit, and
``batchnorm_stats.exchange()`` on the HIP model: one launch, the bits of the copying route (``ONDA_BN_SWAP=0``), no stale BatchNorm
fold behind a swap."""
from copy import deepcopy

import numpy as np
import pytest
import torch
from torch import nn

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA75EA7
# float32 patterns a float move could damage: NaNs with payloads (quiet, signalling, negative), +-inf, -0.0, denormals
SPECIAL = [0x7FC12345, 0x7F800001, 0xFFC00001, 0xFFA5A5A5, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000]
KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _i32(v):
    return v - (1 << 32) if v >= (1 << 31) else v


def _layout(specs, seed):
    """One int32 arena full of sentinel words with the tensors of `specs` = [(words, a_mod, b_mod, dtype)] carved out of it: every
    tensor starts `mod` words past a 16-byte boundary and has at least three sentinel words on either side.  Returns (arena,
    pairs, the arena's expected words after one swap)."""
    spans, cursor = [], 8
    for words, a_mod, b_mod, dtype in specs:
        row = []
        for mod in (a_mod, b_mod):
            start = -(-(cursor + 3) // 4) * 4 + mod
            row.append(start)
            cursor = start + words
        spans.append(row)
    total = cursor + 8
    g = torch.Generator().manual_seed(seed)
    host = torch.full((total,), _i32(SENTINEL), dtype=torch.int32)
    for (words, _, _, dtype), row in zip(specs, spans):
        for start in row:
            if dtype == torch.int64:  # counters of 2^33 and more: the high word is never zero
                vals = (1 << 33) + torch.randint(0, 1 << 40, (words // 2,), generator=g, dtype=torch.int64)
                host[start:start + words] = vals.view(torch.int32)
            else:
                host[start:start + words] = torch.randint(-(1 << 31), (1 << 31) - 1, (words,), generator=g, dtype=torch.int64).to(torch.int32)
                for i in range(min(words, len(SPECIAL))):
                    host[start + i] = _i32(SPECIAL[(i + start) % len(SPECIAL)])
    expected = host.clone()
    for (words, _, _, _), (sa, sb) in zip(specs, spans):
        expected[sa:sa + words], expected[sb:sb + words] = host[sb:sb + words], host[sa:sa + words]
    arena = host.to(DEV)
    assert arena.data_ptr() % 16 == 0
    pairs = []
    for (words, a_mod, b_mod, dtype), row in zip(specs, spans):
        pair = []
        for start, mod in zip(row, (a_mod, b_mod)):
            t = arena[start:start + words].view(dtype)
            assert t.data_ptr() % 16 == 4 * mod
            pair.append(t[0] if dtype == torch.int64 and words == 2 else t)  # (a 0-dim view, as a BatchNorm counter is)
        pairs.append(tuple(pair))
    return arena, pairs, expected


def _check_swap(specs, seed):
    from onda_amd import ops
    arena, pairs, expected = _layout(specs, seed)
    original = arena.cpu()
    clones = [(a.clone(), b.clone()) for a, b in pairs]
    versions = [(a._version, b._version) for a, b in pairs]
    cache = {}
    ops.swap_multi(pairs, cache)
    torch.cuda.synchronize()
    got = arena.cpu()
    bad = (got != expected).nonzero().reshape(-1)
    print(f"{len(pairs)} entries, {arena.numel()} words: {bad.numel()} words differ after one swap")
    assert bad.numel() == 0, bad[:8].tolist()
    # a, b = b.clone(), a.clone(), as bit patterns
    for (a, b), (a0, b0) in zip(pairs, clones):
        kind = torch.int64 if a.element_size() == 8 else torch.int32
        assert torch.equal(a.view(kind), b0.view(kind)) and torch.equal(b.view(kind), a0.view(kind))
    assert all(a._version > va and b._version > vb for (a, b), (va, vb) in zip(pairs, versions))
    table = cache["table"]
    ops.swap_multi(pairs, cache)
    torch.cuda.synchronize()
    assert cache["table"] is table  # (no address changed: the device table is the first call's)
    assert torch.equal(arena.cpu(), original)
    return arena, pairs, original


F, L = torch.float32, torch.int64
TABLE = [(n, 0, 0, F) for n in (1, 2, 3, 64, 4095, 4096, 4097, 8197)] + [
    (4096, 1, 1, F),   # both tensors [1:] views: a full block that must move word by word
    (4096, 0, 1, F),   # only b is such a view
    (4096, 0, 0, F),   # the vector path
    (4097, 3, 2, F),
    (2, 0, 2, L), (2, 2, 2, L), (10, 2, 0, L), (8192, 0, 0, L), (8194, 2, 2, L)]


def test_swap_table_bit_for_bit():
    """Every size class of the kernel in one table (word path, vector path, full blocks that are not 16-byte aligned, tails,
    several blocks per entry, int64 at 8-byte offsets), inside sentinel words; a second launch restores the original."""
    _check_swap(TABLE, 11)


def test_swap_table_past_the_lds_bisection():
    """1 030 entries of one to five words: past 1 024 entries mt_entry_of bisects in global memory."""
    specs = [(1 + i % 5, i % 4, (i * 3) % 4, F) for i in range(1024)] + [(2, 2 * (i % 2), 0, L) for i in range(6)]
    assert len(specs) == 1030
    _check_swap(specs, 12)


def test_swap_bad_arguments_launch_nothing():
    from onda_amd import _lib, ops
    from onda_amd.ops.core import _p, _stream
    arena, pairs, expected = _layout(TABLE[:4], 13)
    original = arena.cpu()
    blk = _lib.query("onda_multi_tensor_block")
    ents, first = [], 0
    for a, b in pairs:
        ents.append(_lib.OndaSwapEntry(a.data_ptr(), b.data_ptr(), a.numel(), first))
        first += -(-a.numel() // blk)
    table = ops._table(ents, _lib.OndaSwapEntry, arena.device)
    fn = _lib.load().onda_swap_multi
    assert fn(None, len(ents), first, _stream()) == -1
    assert fn(_p(table), 0, first, _stream()) == -1
    assert fn(_p(table), -3, first, _stream()) == -1
    assert fn(_p(table), len(ents), 0, _stream()) == -1
    assert fn(_p(table), len(ents), -1, _stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(arena.cpu(), original)
    assert fn(_p(table), len(ents), first, _stream()) == 0  # (the same table is a good one)
    torch.cuda.synchronize()
    assert torch.equal(arena.cpu(), expected)


def test_swap_multi_rejects_a_tensor_named_twice():
    from onda_amd import ops
    arena, pairs, _ = _layout(TABLE[:4], 14)
    original = arena.cpu()
    (a0, b0), (a1, b1) = pairs[2], pairs[3]
    with pytest.raises(ValueError, match="twice"):
        ops.swap_multi([(a0, b0), (a1, b1), (b0, a0)])
    with pytest.raises(ValueError, match="twice"):
        ops.swap_multi([(a1, a1)])
    with pytest.raises(ValueError, match="twice"):
        ops.swap_multi([(a1[:32], b1[:32]), (b1[16:48], a1[32:])])  # overlapping views
    with pytest.raises(ValueError):
        ops.swap_multi([(a1, b1[:32])])
    with pytest.raises(ValueError):
        ops.swap_multi([(a1, b1.cpu())])
    with pytest.raises(ValueError):
        ops.swap_multi([(a1[::2], b1[::2])])
    torch.cuda.synchronize()
    assert torch.equal(arena.cpu(), original)


# ------------------------------------------------------------------------------------------- exchange() on the HIP model
def _model_and_sets(seed=21):
    """The ResNet-50 model with a kept set (the filled state) and a live set perturbed in all five keys of every BatchNorm."""
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import batchnorm_stats
    from onda_amd.framework.model.deeplabv2 import get_deeplab_v2
    from onda_amd.synthetic import fill_state_dict
    m = get_deeplab_v2(num_classes=19, multi_level=True, layers=[3, 4, 6, 3], classifier="ProDA")
    m.multi_level = False
    fill_state_dict(m, 1, 3.0)
    m = m.to(DEV)
    bn = batchnorm_stats(m)
    g = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for i, b in enumerate(x for x in m.modules() if isinstance(x, nn.BatchNorm2d)):
            c = b.num_features
            b.running_mean.add_(0.1 * torch.randn(c, device=DEV, generator=g))
            b.running_var.mul_(1 + 0.5 * torch.rand(c, device=DEV, generator=g))
            b.weight.mul_(1 + 0.1 * torch.randn(c, device=DEV, generator=g))
            b.bias.add_(0.1 * torch.randn(c, device=DEV, generator=g))
            b.num_batches_tracked.fill_((1 << 33) + i)
    return m, bn


def _bits(t):
    return t.detach().clone().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _sets(m, bn):
    live = {name: {k: _bits(getattr(b, k)) for k in KEYS} for name, b in m.named_modules() if isinstance(b, nn.BatchNorm2d)}
    kept = {name: {k: _bits(v[k]) for k in KEYS} for name, v in bn.memory.items()}
    assert live.keys() == kept.keys() and len(live) >= 48
    return live, kept


def _same(a, b):
    return all(torch.equal(a[n][k], b[n][k]) for n in a for k in KEYS)


class _CallSpy:
    def __init__(self, monkeypatch):
        from onda_amd.ops import tables
        self.names, real = [], tables.call

        def spy(name, *args):
            self.names.append(name)
            return real(name, *args)
        monkeypatch.setattr(tables, "call", spy)

    def swaps(self):
        return self.names.count("onda_swap_multi")


def test_exchange_is_one_launch_with_the_copying_routes_bits(monkeypatch):
    """exchange() on the HIP model: exactly one onda_swap_multi and no state_dict per call, both sets bit-identical to the
    ONDA_BN_SWAP=0 route's -- also after update_ema's _flat_int_buffers has rebound the counters -- and twice is the identity."""
    from onda_amd.framework.domain_adaptation.methods.prototypes import _flat_int_buffers
    m1, bn1 = _model_and_sets()
    m0, bn0 = _model_and_sets()
    live_a, kept_a = _sets(m1, bn1)
    assert not _same(live_a, kept_a) and _same(_sets(m0, bn0)[0], live_a)
    spy = _CallSpy(monkeypatch)

    def launch_route(bn):
        def boom(*a, **k):
            raise AssertionError("state_dict called on the one-launch route")
        before = spy.swaps()
        with monkeypatch.context() as mp:
            mp.setattr(nn.Module, "state_dict", boom)
            mp.setattr(nn.Module, "load_state_dict", boom)
            bn.exchange()
        assert spy.swaps() == before + 1

    def copy_route(bn):
        before = spy.swaps()
        with monkeypatch.context() as mp:
            mp.setenv("ONDA_BN_SWAP", "0")
            bn.exchange()
        assert spy.swaps() == before

    launch_route(bn1)
    copy_route(bn0)
    live1, kept1 = _sets(m1, bn1)
    live0, kept0 = _sets(m0, bn0)
    assert _same(live1, kept_a) and _same(kept1, live_a)
    assert _same(live1, live0) and _same(kept1, kept0)
    # the 53 counters become views of one flat tensor: new addresses, a new table, the same one launch
    table = bn1._swap_cache["table"]
    for m in (m1, m0):
        assert _flat_int_buffers(m) is not None
    launch_route(bn1)
    copy_route(bn0)
    assert bn1._swap_cache["table"] is not table
    live1, kept1 = _sets(m1, bn1)
    live0, kept0 = _sets(m0, bn0)
    assert _same(live1, live_a) and _same(kept1, kept_a)
    assert _same(live1, live0) and _same(kept1, kept0)
    table = bn1._swap_cache["table"]
    launch_route(bn1)
    assert bn1._swap_cache["table"] is table
    # the routes mix: a set the copying route left behind is swapped by the launch
    launch_route(bn0)
    assert _same(_sets(m0, bn0)[0], _sets(m1, bn1)[0]) and _same(_sets(m0, bn0)[1], _sets(m1, bn1)[1])


def test_eval_forward_after_exchange_uses_the_swapped_set():
    """An eval-mode forward folds BatchNorm into the conv epilogue and caches the fold: after exchange() the forward must be,
    bit for bit, the forward of a fresh copy whose BatchNorms were given the kept set by load_state_dict."""
    from onda_amd.framework.model.deeplabv2 import get_deeplab_v2
    from onda_amd.synthetic import fill_state_dict, synth_batch
    m, bn = _model_and_sets()
    m.eval()
    x = synth_batch(1, 64, 128, seed=7)["image"].to(DEV)
    kept = deepcopy(bn.memory)
    with torch.no_grad():
        stale = {k: v.clone() for k, v in m(x)[1].items()}  # (fills the fold caches with the perturbed set)
        bn.exchange()
        got = m(x)[1]
    fresh = get_deeplab_v2(num_classes=19, multi_level=True, layers=[3, 4, 6, 3], classifier="ProDA")
    fresh.multi_level = False
    fill_state_dict(fresh, 1, 3.0)
    fresh = fresh.to(DEV).eval()
    for name, b in fresh.named_modules():
        if isinstance(b, nn.BatchNorm2d):
            b.load_state_dict(kept[name])
    with torch.no_grad():
        want = fresh(x)[1]
    for key in ("feat", "out"):
        print(key, "max |after exchange - fresh|", float((got[key] - want[key]).abs().max()),
              "max |before exchange - fresh|", float((stale[key] - want[key]).abs().max()))
        assert torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), key
        assert not torch.equal(stale[key], want[key])


def test_default_hybrid_step_never_swaps(monkeypatch, tmp_path):
    """BN_POLICY "freeze" (the shipped configs): the step calls no onda_swap_multi."""
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
    from onda_amd.framework.handlers import get_adapt_method, get_model
    from onda_amd.synthetic import fill_state_dict, synth_batch
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, str(tmp_path), batch_size=1)
    model = get_model(cfg, 19)
    fill_state_dict(model, 1, 3.0)
    da = get_adapt_method(cfg)(model, cfg, spec)
    src, trg = synth_batch(1, 64, 128, seed=100), synth_batch(1, 64, 128, seed=200)
    torch.manual_seed(123)
    da.update_dynamic()
    switch_batch_statistics(da.model, False)
    da.calculate_prototypes([src], save=False)
    switch_batch_statistics(da.model, True)
    da.optimizer.zero_grad()
    spy = _CallSpy(monkeypatch)
    da.adjust_learning_rate(0, 6)
    log = da.step([src], trg)
    da.update_ema()
    assert np.isfinite(float(log["Total target loss"]))
    assert "onda_sgd_multi" in spy.names and "onda_ema_multi" in spy.names  # (the spy sees this module's launches)
    assert spy.swaps() == 0
