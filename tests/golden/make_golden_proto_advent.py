#!/usr/bin/env python3
"""Generate G23 and G24 by IMPORTING the reference on the CPU (run in the build container only):

    python tests/golden/make_golden_proto_advent.py    # writes g23_proto_advent.npz, g23_proto_advent_aux.npz, g24_bn_double.npz

G23: two steps of the reference's ``adv_proDA`` (``PROTO_ADVENT``, prototype_advent.py:14-152) at 128 x 64, batch 2, without and
with the auxiliary head.  G24: two steps of its ``hswitch_proDA`` with ``BN_POLICY: "double"``.  Both keep two BatchNorm state sets
and swap them around the source pass (``batchnorm_stats.exchange``, adaptation_model.py:39-72).

Set-up, the same for all three: ``make_golden.make_cfg``'s cfg; as spec the ``PROTO_ONLINE_HSWITCH`` block of
configs/confidence_switch.yml plus the five ADVENT keys of configs/advent.yml (LAMBDA_ADV_AUX, LAMBDA_SEG_AUX, EPOCHS,
LAMBDA_ADV_MAIN, LAMBDA_SEG_MAIN), with LAMBDA_ADV_MAIN = 1.0 so that the adversarial gradient is visible beside the supervised
one, SWITCH_PRIOR_THRESH = 0.86, SOFT_TRANS = True, LOAD_PROTO = None; ``ref_model(1, 9.0)``; ``torch.manual_seed(77)`` before
construction (the discriminators' initial weights); batches ``synth_batch(2, 64, 128, seed=100+i / 200+i)``;
``torch.manual_seed(123)``, ``update_dynamic``, prototypes from the source batches under frozen statistics; two steps with
``adjust_learning_rate(s, 6)`` and ``update_ema`` after each.

The shims are make_golden.py's, and one more: ``advent_da.bce_loss`` builds its target with ``y_pred.get_device()``, which is -1
on the CPU; it is replaced with ``BCEWithLogitsLoss()(y, full_like(y, label))``, the same value.

Per step the files hold the scalar log as JSON, ``stored_predictions``, the prototypes and ``num_batches_tracked`` of ``bn1`` in
both state sets; after step 0 also ``running_mean`` / ``running_var`` of the five BatchNorms G2 samples, from both sets, and (G23)
the gradients of ``layer6.head.1.weight``, ``layer6.bottleneck.2.weight`` and of the first and last conv weight of each working
discriminator, taken in front of the first optimizer step.  Seeds and outputs only.

Two measuring modes write the same files into ``ONDA_GOLDEN_OUT`` instead (the reference's own spread, from which
tests/test_proto_advent_golden.py takes the bars of the discriminators' first-conv gradients): ``ONDA_GOLDEN_THREADS=<n>`` runs with
another thread count, ``ONDA_GOLDEN_LOGIT_NOISE=<eps>:<seed>`` adds noise to the student's logits (``noisy_heads``)."""
import json
import os
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (the shims, make_cfg, ref_model, tolog, save)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402
from addict import Dict  # noqa: E402  (stub)
from framework.domain_adaptation.methods import advent_da  # noqa: E402
from framework.domain_adaptation.methods.prototype_advent import adv_proDA  # noqa: E402
from framework.domain_adaptation.methods.prototypes_hswitch import hswitch_proDA  # noqa: E402

from onda_amd.synthetic import synth_batch  # noqa: E402

if "ONDA_GOLDEN_THREADS" in os.environ:  # (the spread of the reference's own results under another thread count)
    torch.set_num_threads(int(os.environ["ONDA_GOLDEN_THREADS"]))

LOGIT_NOISE = os.environ.get("ONDA_GOLDEN_LOGIT_NOISE")
if LOGIT_NOISE:
    assert os.environ.get("ONDA_GOLDEN_OUT"), "a noise run writes to ONDA_GOLDEN_OUT, never over the fixtures"

advent_da.bce_loss = lambda y, label: torch.nn.BCEWithLogitsLoss()(y, torch.full_like(y, label))

SAMPLED_BN = ("bn1", "layer1.0.bn1", "layer2.0.downsample.1", "layer3.2.bn2", "layer4.2.bn3")
ADVENT_KEYS = ("LAMBDA_ADV_AUX", "LAMBDA_SEG_AUX", "EPOCHS", "LAMBDA_ADV_MAIN", "LAMBDA_SEG_MAIN")


def make_spec():
    cwd = os.getcwd()
    os.chdir(G.REF)
    try:
        spec = Dict(yaml.load(open("configs/confidence_switch.yml"))).METHOD.ADAPTATION.PROTO_ONLINE_HSWITCH
        adv = Dict(yaml.load(open("configs/advent.yml"))).METHOD.ADAPTATION.ADVENT
    finally:
        os.chdir(cwd)
    for k in ADVENT_KEYS:
        spec[k] = adv[k]
    spec.LAMBDA_ADV_MAIN = 1.0
    spec.SWITCH_PRIOR_THRESH, spec.SOFT_TRANS, spec.LOAD_PROTO = 0.86, True, None
    spec.set_ = (25,)
    return spec


def conv_ends(d):
    convs = [m for m in d if isinstance(m, torch.nn.Conv2d)]
    return convs[0].weight, convs[-1].weight


def bn_sets(res, s, model, memory, sampled):
    sd = model.state_dict()
    res[f"nbt{s}_model"], res[f"nbt{s}_memory"] = sd["bn1.num_batches_tracked"].clone(), memory["bn1"]["num_batches_tracked"].clone()
    if sampled:
        for k in SAMPLED_BN:
            for stat in ("running_mean", "running_var"):
                res[f"model_{k}.{stat}"], res[f"memory_{k}.{stat}"] = sd[f"{k}.{stat}"].clone(), memory[k][stat].clone()


def noisy_heads(model, multi_level):
    """ONDA_GOLDEN_LOGIT_NOISE="<eps>:<seed>": every forward of the student adds eps * max|out| * N(0, 1) to the logits of its
    head(s), from a generator of its own (the Dropout2d draws stay the fixture's).  Not for fixtures: it measures how far the
    reference's own outputs move when its logits move by what a float32 forward of another order of operations differs by."""
    eps, seed = LOGIT_NOISE.split(":")
    gen = torch.Generator().manual_seed(int(seed))

    def hook(mod, inp, out):
        o = out["out"]
        return dict(out, out=o + float(eps) * o.detach().abs().max() * torch.randn(o.shape, generator=gen))
    for head in (model.layer6,) + ((model.layer5,) if multi_level else ()):
        head.register_forward_hook(hook)


def prepare(proto):
    src = [synth_batch(2, 64, 128, seed=100 + i) for i in range(2)]
    trg = [synth_batch(2, 64, 128, seed=200 + i) for i in range(2)]
    torch.manual_seed(123)
    proto.update_dynamic()
    G.switch_batch_statistics(proto.model, False)
    proto.calculate_prototypes(src)
    G.switch_batch_statistics(proto.model, True)
    return src, trg


def record(res, s, log, trg, prototypes):
    lg = G.tolog(log)
    res[f"log{s}_json"] = np.array(json.dumps({k: v for k, v in lg.items() if np.isscalar(v)}))
    res[f"soft{s}"] = trg["stored_predictions"].to(torch.float32)
    res[f"proto{s + 1}"] = prototypes.prototypes.clone()


def g23(name, multi_level):
    with tempfile.TemporaryDirectory() as tmp:
        cfg, _ = G.make_cfg(tmp)
        cfg.MODEL.MULTI_LEVEL = multi_level
        model = G.ref_model(1, 9.0)
        model.multi_level = multi_level
        torch.manual_seed(77)
        da = adv_proDA(model, cfg, make_spec())
        src, trg = prepare(da.proto_model)
        if LOGIT_NOISE:
            noisy_heads(model, multi_level)
        res, params = {}, dict(model.named_parameters())
        real_step = da.advent.optimizer.step

        def step_spy(*a, **k):  # the first of the three optimizers: nothing has moved yet
            if "grad_layer6.head.1.weight" not in res:
                for key in ("layer6.head.1.weight", "layer6.bottleneck.2.weight"):
                    res["grad_" + key] = params[key].grad.detach().clone()
                for tag, d in (("d_main", da.advent.d_main),) + ((("d_aux", da.advent.d_aux),) if multi_level else ()):
                    first, last = conv_ends(d)
                    res[f"grad_{tag}_first"], res[f"grad_{tag}_last"] = first.grad.detach().clone(), last.grad.detach().clone()
            return real_step(*a, **k)
        da.advent.optimizer.step = step_spy
        da.advent.optimizer.zero_grad()
        da.advent.optimizer_d_main.zero_grad()
        da.advent.optimizer_d_aux.zero_grad()
        for s in range(2):
            da.advent.adjust_learning_rate(s, 6)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                log = da.step(src[s], trg[s])
            da.proto_model.update_ema()
            record(res, s, log, trg[s], da.proto_model.prototypes)
            bn_sets(res, s, model, da.advent.bn.memory, sampled=s == 0)
        G.save(name, **res)
        print(name, {k: round(v, 5) for k, v in json.loads(str(res["log1_json"])).items()})


def g24():
    with tempfile.TemporaryDirectory() as tmp:
        cfg, _ = G.make_cfg(tmp)
        spec = make_spec()
        spec.BN_POLICY = "double"
        torch.manual_seed(77)
        da = hswitch_proDA(G.ref_model(1, 9.0), cfg, spec)
        src, trg = prepare(da)
        res = {}
        da.optimizer.zero_grad()
        for s in range(2):
            da.adjust_learning_rate(s, 6)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                log = da.step([src[s]], trg[s])
            da.update_ema()
            record(res, s, log, trg[s], da.prototypes)
            bn_sets(res, s, da.model, da.bn.memory, sampled=s == 0)
        G.save("g24_bn_double", **res)
        print("g24", {k: round(v, 5) for k, v in json.loads(str(res["log1_json"])).items()})


if __name__ == "__main__":
    out = os.environ.get("ONDA_GOLDEN_OUT")  # (another directory: a spread measurement must not touch the committed files)
    if out:
        G.HERE = out
    g23("g23_proto_advent", False)
    g23("g23_proto_advent_aux", True)
    g24()
