"""Drop-in for ``framework/handlers/model_handler.py``: ``get_model(cfg, n_classes)`` (:14-60).

``DeepLabv2-Resnet101-ProDA`` (``framework/model/deeplabv2_proda.py``) is an opt-in: ``enable_resnet101_proda()`` -- or
``ONDA_RESNET101_PRODA=1`` in the environment at import -- makes ``MODEL_NAMES`` the reference's four names in the reference's order.
Left alone the registry holds the three names it held before and rejects the fourth, which
``tests/test_gn_site_reference.py::test_the_other_names_are_unchanged`` pins."""
import os
import types

import torch

from onda_amd.framework.model.deeplabv2 import get_deeplab_v2

PRODA_MODEL = "DeepLabv2-Resnet101-ProDA"
REFERENCE_MODEL_NAMES = ("DeepLabv2-Resnet50", "DeepLabv2-Resnet101", PRODA_MODEL, "DeepLabv2-Resnet50-GN")
MODEL_NAMES = ["DeepLabv2-Resnet50", "DeepLabv2-Resnet101", "DeepLabv2-Resnet50-GN"]
_DEFAULT_NAMES = tuple(MODEL_NAMES)
_LAYERS = {"DeepLabv2-Resnet50": [3, 4, 6, 3], "DeepLabv2-Resnet101": [3, 4, 23, 3], "DeepLabv2-Resnet50-GN": [3, 4, 6, 3]}


def enable_resnet101_proda(on=True):
    """Put DeepLabv2-Resnet101-ProDA into the registry (the list object stays the same, so earlier imports of it see the
    change) or take it out again.  Returns the previous setting."""
    old = PRODA_MODEL in MODEL_NAMES
    MODEL_NAMES[:] = REFERENCE_MODEL_NAMES if on else _DEFAULT_NAMES
    return old


if os.environ.get("ONDA_RESNET101_PRODA", "0") == "1":
    enable_resnet101_proda()


def get_model(cfg, n_classes):
    assert cfg.MODEL.NAME in MODEL_NAMES, f"cfg.MODEL.NAME should be in {MODEL_NAMES} (the HIP path covers the DeepLabV2 ResNets)"
    if cfg.MODEL.NAME == PRODA_MODEL:
        from onda_amd.framework.model.deeplabv2_proda import Deeplab
        cfg.MODEL.MULTI_LEVEL = False
        return _finish(Deeplab(torch.nn.BatchNorm2d, num_classes=n_classes), cfg)
    kw = {}
    if cfg.MODEL.NAME == "DeepLabv2-Resnet50-GN":
        # the reference's lambda (:33); its _make_layer never hands it to the blocks, so it reaches the stem's bn1 and the
        # four layerN.0.downsample.1 only -- the blocks keep their BatchNorms
        kw["norm_module"] = lambda *k, **x: torch.nn.GroupNorm(32, *k, **x)
    # built multi_level=True like the reference, so the (never executed) layer5 head is part of the state_dict
    model = get_deeplab_v2(num_classes=n_classes, layers=_LAYERS[cfg.MODEL.NAME], multi_level=True,
                           classifier=cfg.MODEL.CLASSIFIER, **kw)
    return _finish(model, cfg)


def _finish(model, cfg):
    """MODEL.LOAD, ``multi_level`` and the device: what follows the construction for every name (reference :41-60)."""
    load = cfg.MODEL.LOAD
    if load is not None and load != "None" and not (isinstance(load, dict) and not load):
        state = torch.load(load, map_location="cpu")
        if isinstance(state, types.MethodType):
            state = state()
        if "imagenet" in load.lower():
            merged = model.state_dict().copy()
            for key in state:
                parts = key.split(".")
                start = 1 if parts[0] in ("Scale", "module") else 0
                if parts[start] not in ("layer5", "fc"):
                    merged[".".join(parts[start:])] = state[key]
            model.load_state_dict(merged)
        else:
            model.load_state_dict(state)
    model.multi_level = cfg.MODEL.MULTI_LEVEL
    model.to(cfg.OTHERS.DEVICE)
    return model
