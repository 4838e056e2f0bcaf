"""CPU: what PROTO_ADVENT and the two BatchNorm state sets need without a GPU -- the drop-in alias, the class's surface, and the
semantics of ``batchnorm_stats`` (reference adaptation_model.py:39-72) on a small torch model, bit for bit."""
import sys

import pytest
import torch
from torch import nn

KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


# the reference's registry, framework/handlers/adaptation_method_handler.py:1-8
REFERENCE_NAMES = ["PROTO_ONLINE", "ADVENT", "PROTO_ONLINE_VSWITCH", "PROTO_ONLINE_HSWITCH", "PROTO_ADVENT", "PROTO_ONLINE_HYBRIDSWITCH"]


def test_handler_returns_adv_proDA_once_enabled():
    """PROTO_ADVENT is an opt-in of the registry: enabled, the names are the reference's six in its order and the handler
    returns adv_proDA; taken out again, the registry is what it was."""
    from onda_amd.config import Cfg
    from onda_amd.framework import handlers
    from onda_amd.framework.handlers import adaptation_method_handler as H
    from onda_amd.framework.domain_adaptation.methods.prototype_advent import adv_proDA
    cfg = Cfg.from_dict({"METHOD": {"ADAPTATION": {"NAME": "PROTO_ADVENT"}}})
    names, before = H.ADAPTATION_METHOD_NAMES, list(H.ADAPTATION_METHOD_NAMES)
    try:
        handlers.enable_proto_advent()
        assert H.ADAPTATION_METHOD_NAMES is names and names == REFERENCE_NAMES
        assert handlers.get_adapt_method(cfg) is adv_proDA
        for name in REFERENCE_NAMES:
            assert isinstance(handlers.get_adapt_method(Cfg.from_dict({"METHOD": {"ADAPTATION": {"NAME": name}}})), type)
    finally:
        handlers.enable_proto_advent("PROTO_ADVENT" in before)
    assert names == before


def test_dropin_registers_prototype_advent():
    import onda_amd.dropin as dropin
    saved = {k: v for k, v in sys.modules.items() if k == "framework" or k.startswith("framework.")}
    try:
        dropin.install()
        from framework.domain_adaptation.methods.prototype_advent import adv_proDA
        import onda_amd.framework.domain_adaptation.methods.prototype_advent as mine
        assert adv_proDA is mine.adv_proDA
        for name in ("update_cfg_spec", "step", "train"):
            assert callable(getattr(adv_proDA, name))
    finally:
        for k in [k for k in sys.modules if k == "framework" or k.startswith("framework.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def _model(seed):
    """Three BatchNorm2d of different widths with every one of the five state entries perturbed."""
    g = torch.Generator().manual_seed(seed)
    m = nn.Sequential(nn.Conv2d(3, 5, 1), nn.BatchNorm2d(5), nn.Conv2d(5, 64, 1), nn.BatchNorm2d(64), nn.Conv2d(64, 7, 1),
                      nn.BatchNorm2d(7))
    for i, bn in enumerate(b for b in m if isinstance(b, nn.BatchNorm2d)):
        with torch.no_grad():
            for key in KEYS[:4]:
                getattr(bn, key).copy_(torch.randn(bn.num_features, generator=g))
            bn.num_batches_tracked.fill_((1 << 33) + seed * 10 + i)
    return m


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in (b for b in m if isinstance(b, nn.BatchNorm2d)):
            for key in KEYS[:4]:
                getattr(bn, key).add_(torch.randn(bn.num_features, generator=g))
            bn.num_batches_tracked.add_(17)
            bn.running_var[0] = float("nan")
            bn.running_mean[1] = -0.0


def _bits(t):
    return t.detach().clone().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _live(m):
    return {name: {k: _bits(getattr(b, k)) for k in KEYS} for name, b in m.named_modules() if isinstance(b, nn.BatchNorm2d)}


def _kept(bn):
    assert all(set(v) == set(KEYS) for v in bn.memory.values())
    return {name: {k: _bits(v[k]) for k in KEYS} for name, v in bn.memory.items()}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[n][k], b[n][k]) for n in a for k in KEYS)


def test_batchnorm_stats_exchange_swaps_both_sets_bit_for_bit():
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import batchnorm_stats
    m = _model(1)
    bn = batchnorm_stats(m)
    assert sorted(bn.memory) == ["1", "3", "5"]
    first = _live(m)
    assert _same(_kept(bn), first)
    _perturb(m, 2)
    second = _live(m)
    assert not _same(first, second)
    bn.exchange()
    assert _same(_live(m), first) and _same(_kept(bn), second)
    bn.exchange()
    assert _same(_live(m), second) and _same(_kept(bn), first)
    # the kept set is a copy, not a view of the live one
    _perturb(m, 3)
    assert _same(_kept(bn), first)


def test_batchnorm_stats_save_exchange_load():
    """save() overwrites the kept set with the live one; after exchange() both sets hold what the other held; load() copies the
    kept set over the live one and leaves the kept set alone (reference :57-72)."""
    from onda_amd.framework.domain_adaptation.methods.adaptation_model import batchnorm_stats
    m = _model(4)
    bn = batchnorm_stats(m)
    _perturb(m, 5)
    a = _live(m)
    bn.save()
    assert _same(_kept(bn), a)
    _perturb(m, 6)
    b = _live(m)
    bn.exchange()
    assert _same(_live(m), a) and _same(_kept(bn), b)
    _perturb(m, 7)
    bn.load()
    assert _same(_live(m), b) and _same(_kept(bn), b)
    bn.compare()


def test_swap_multi_checks_its_contract_before_any_launch():
    """The contract is checked on the host, before the table is built: nothing here reaches a launch (CPU tensors would not)."""
    from onda_amd import ops
    a, b, c = torch.zeros(8), torch.ones(8), torch.ones(4)
    with pytest.raises(ValueError, match="twice"):
        ops.swap_multi([(a, b), (c, a[2:6])])
    with pytest.raises(ValueError):
        ops.swap_multi([(a, c)])
    with pytest.raises(ValueError):
        ops.swap_multi([(a, b.to(torch.int64))])
    with pytest.raises(ValueError):
        ops.swap_multi([(a.half(), b.half())])
    with pytest.raises(ValueError):
        ops.swap_multi([(torch.zeros(4, 4).t(), torch.zeros(4, 4))])
