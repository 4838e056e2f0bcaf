"""Drop-in for ``framework/handlers/adaptation_method_handler.py`` (:1-40): the prototype methods, the ADVENT baseline and
PROTO_ADVENT, the combination of the two (``prototype_advent.adv_proDA``).

PROTO_ADVENT is an opt-in: ``enable_proto_advent()`` -- or ``ONDA_PROTO_ADVENT=1`` in the environment at import -- makes
``ADAPTATION_METHOD_NAMES`` the reference's six names in the reference's order and ``get_adapt_method`` hand ``adv_proDA`` out.  Left
alone the registry holds the five names it held before and rejects the sixth, which ``tests/test_entropy_reference.py::
test_handler_returns_advent`` pins."""
import os

REFERENCE_METHOD_NAMES = ("PROTO_ONLINE", "ADVENT", "PROTO_ONLINE_VSWITCH", "PROTO_ONLINE_HSWITCH", "PROTO_ADVENT",
                          "PROTO_ONLINE_HYBRIDSWITCH")
ADAPTATION_METHOD_NAMES = ["ADVENT", "PROTO_ONLINE", "PROTO_ONLINE_VSWITCH", "PROTO_ONLINE_HSWITCH", "PROTO_ONLINE_HYBRIDSWITCH"]
_DEFAULT_NAMES = tuple(ADAPTATION_METHOD_NAMES)


def enable_proto_advent(on=True):
    """Put PROTO_ADVENT into the registry (the list object stays the same, so earlier imports of it see the change) or take it
    out again."""
    ADAPTATION_METHOD_NAMES[:] = REFERENCE_METHOD_NAMES if on else _DEFAULT_NAMES


if os.environ.get("ONDA_PROTO_ADVENT", "0") == "1":
    enable_proto_advent()


def get_adapt_method(cfg):
    name = cfg.METHOD.ADAPTATION.NAME
    assert name in ADAPTATION_METHOD_NAMES, f"cfg.METHOD.ADAPTATION.NAME not in {ADAPTATION_METHOD_NAMES}"
    if name == "ADVENT":
        from onda_amd.framework.domain_adaptation.methods.advent_da import advent
        return advent
    if name == "PROTO_ONLINE":
        from onda_amd.framework.domain_adaptation.methods.prototypes import online_proDA
        return online_proDA
    if name == "PROTO_ONLINE_VSWITCH":
        from onda_amd.framework.domain_adaptation.methods.prototypes_vswitch import vswitch_proDA
        return vswitch_proDA
    if name == "PROTO_ONLINE_HSWITCH":
        from onda_amd.framework.domain_adaptation.methods.prototypes_hswitch import hswitch_proDA
        return hswitch_proDA
    if name == "PROTO_ADVENT":
        from onda_amd.framework.domain_adaptation.methods.prototype_advent import adv_proDA
        return adv_proDA
    from onda_amd.framework.domain_adaptation.methods.prototypes_hybrid_switch import hybrid_proDA
    return hybrid_proDA
