#!/usr/bin/env python3
"""Generate G26 / G27 by IMPORTING the reference (run in the build container only; nothing is fetched -- the reference's
``Deeplab()`` would download ImageNet weights, so ``ResNet101(Bottleneck, [3, 4, 23, 3], 19, nn.BatchNorm2d)`` is built directly):

    python tests/golden/make_golden_proda101.py [g26] [g27] [step]

g26_proda101.npz -- the tree of the reference's DeepLabv2-Resnet101-ProDA built under ``torch.manual_seed(SEED)``: state_dict keys,
    shapes, dtypes, the parameters' ``requires_grad`` flags, a digest of every seeded tensor, how often each parameter occurs in
    the 1x and the 10x group of ``optim_parameters``; and one train-mode forward + backward of that seeded model (Dropout2d.p = 0)
    on ``synth_batch(2, 65, 129)`` with the labels of ``gn_site_fp64.labels()`` in float64 and in float32: ``out`` of both, ``feat``
    of the float64 run (rounded to float32) and a strided sample of the float32 run's, the loss, and for every conv / linear weight
    and every GroupNorm parameter the gradient's norm in both runs, the relative L2 distance of the two runs over the whole
    tensor, and a strided sample of 256 values from both.
g26_proda101_bn.npz -- the gradients of all 208 BatchNorm weight / bias vectors from both runs, whole (float64 rounded to float32).
g26_proda101_step.npz -- one ``online_proDA.step`` (static prior, replay buffer on, + ``update_ema``) of the reference on that tree
    with the weights of ``fill_state_dict(model, 1, 40.0)`` at 129 x 65, B = 2 (prototypes from two source batches): the log dict, the soft labels, the prototypes before
    and after, digests of the student's and the teacher's state before and after.
g27_norm_grad.npz -- the reference's ``get_deeplab_v2(19, True, [1, 1, 1, 1], "ProDA", norm_grad=True)`` under the same seed and
    batch, run with ``multi_level`` off: the names of the BatchNorm parameters that train (ten), their gradients in float64 and
    float32, and their values after one ``torch.optim.SGD(optim_parameters(LR), LR, momentum 0.9, weight_decay 5e-4)`` step of the
    float32 run.  Inputs and outputs only."""
import json
import os
import sys
import tempfile
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("ONDA_REFERENCE", "/root/reference")
sys.path[:0] = [REF, os.path.join(HERE, "_stubs"), ROOT, os.path.join(ROOT, "tests"), HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

from framework.model.deeplabv2_proda import Bottleneck, ResNet101  # noqa: E402
from framework.model.deeplabv2 import get_deeplab_v2  # noqa: E402
from framework.utils.func import loss_calc  # noqa: E402

from onda_amd.synthetic import fill_state_dict, synth_batch  # noqa: E402

import gn_site_fp64 as S  # noqa: E402
import proda101_cases as P  # noqa: E402

torch.set_num_threads(8)


def digest(t, n=P.DIGEST):
    f = t.detach().double().cpu().reshape(-1)
    idx = (torch.arange(n, dtype=torch.int64) * f.numel()) // n
    return np.concatenate([[f.sum().item(), f.abs().sum().item()], f[idx].numpy()])


def seeded(build):
    torch.manual_seed(P.SEED)
    m = build()
    for mod in m.modules():
        if isinstance(mod, nn.Dropout2d):
            mod.p = 0.0
    return m.train()


def proda():
    return seeded(lambda: ResNet101(Bottleneck, [3, 4, 23, 3], 19, nn.BatchNorm2d))


def train_pass(m, dtype):
    m = m.to(dtype)
    _, o = m(synth_batch(2, P.H, P.W)["image"].to(dtype))
    loss = loss_calc(o["out"], S.labels(), "cpu")
    loss.backward()
    return m, o, loss


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def g26():
    t0 = time.time()
    m = proda()
    sd = m.state_dict()
    res = {"seed": np.array(P.SEED), "keys": np.array(list(sd)), "shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()]),
           "dtypes": np.array([str(v.dtype) for v in sd.values()]), "digests": np.stack([digest(v) for v in sd.values()])}
    names = [n for n, _ in m.named_parameters()]
    res["param_names"] = np.array(names)
    res["requires_grad"] = np.array([p.requires_grad for _, p in m.named_parameters()])
    by_id = {id(p): i for i, (_, p) in enumerate(m.named_parameters())}
    groups = m.optim_parameters(1.0)
    for k, grp in enumerate(groups):
        count = np.zeros(len(names), dtype=np.int64)
        for p in grp["params"]:
            count[by_id[id(p)]] += 1
        res[f"group{k}_count"] = count
    res["counts"] = np.array([len(sd), len(names), sum(isinstance(x, nn.BatchNorm2d) for x in m.modules()),
                              sum(isinstance(x, nn.GroupNorm) for x in m.modules())])
    print("tree:", res["counts"], "1x entries", int(res["group0_count"].sum()), "over", int((res["group0_count"] > 0).sum()),
          "10x", int(res["group1_count"].sum()))
    m64, o64, l64 = train_pass(proda(), torch.float64)
    m32, o32, l32 = train_pass(proda(), torch.float32)
    res["labels"] = S.labels().numpy().astype(np.uint8)
    res["out64"], res["out32"] = o64["out"].detach().float().numpy(), o32["out"].detach().numpy()
    res["feat64"] = o64["feat"].detach().float().numpy()
    f32 = o32["feat"].detach().reshape(-1)
    res["feat32_sample"] = f32[S.sample_index(f32.numel(), S.SAMPLE_DS)].numpy()
    res["loss64"], res["loss32"] = np.array(l64.item()), np.array(l32.item())
    p64, p32 = dict(m64.named_parameters()), dict(m32.named_parameters())
    bn = P.bn_param_names(m32)
    assert len(bn) == 208
    other = [n for n in names if n not in set(bn)]
    res["other_names"] = np.array(other)
    res["other_norm64"] = np.array([float(p64[n].grad.norm()) for n in other])
    res["other_norm32"] = np.array([float(p32[n].grad.double().norm()) for n in other])
    res["other_eref"] = np.array([rel(p32[n].grad, p64[n].grad) for n in other])
    s64, s32 = [], []
    for n in other:
        g64, g32 = p64[n].grad.reshape(-1), p32[n].grad.reshape(-1)
        idx = S.sample_index(g64.numel(), S.SAMPLE)
        s64.append(g64[idx].float().numpy())
        s32.append(g32[idx].numpy())
    res["other_sample64"], res["other_sample32"] = np.stack(s64), np.stack(s32)
    print(f"out32 vs out64 {rel(o32['out'], o64['out']):.3e}; feat {rel(o32['feat'], o64['feat']):.3e}; worst other e_ref {res['other_eref'].max():.3e}")
    save("g26_proda101", res)
    res = {"names": np.array(bn), "sizes": np.array([p64[n].numel() for n in bn])}
    res["g64"] = torch.cat([p64[n].grad.reshape(-1) for n in bn]).float().numpy()
    res["g32"] = torch.cat([p32[n].grad.reshape(-1) for n in bn]).numpy()
    eref = [rel(p32[n].grad, p64[n].grad) for n in bn]
    print(f"BatchNorm gradients: e_ref median {np.median(eref):.3e}, worst {max(eref):.3e} ({bn[int(np.argmax(eref))]}); {time.time() - t0:.1f} s")
    save("g26_proda101_bn", res)


def save(name, res):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()})
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


def g26_step():
    import make_golden as G  # the reference's make_cfg, tolog, switch_batch_statistics
    from framework.domain_adaptation.methods.prototypes import online_proDA
    with tempfile.TemporaryDirectory() as tmp:
        cfg, spec = G.make_cfg(tmp)
        cfg.SCHEME.RESOLUTION = [P.W, P.H]
        spec.pop("GRAY_AREA", None)
        for k, v in P.STEP_SPEC.items():
            spec[k] = v
        torch.manual_seed(P.SEED)
        model = ResNet101(Bottleneck, [3, 4, 23, 3], 19, nn.BatchNorm2d)
        fill_state_dict(model, 1, P.STEP_HEAD_SCALE)
        model.multi_level = False
        da = online_proDA(model, cfg, spec)
        srcs, trg = [synth_batch(2, P.H, P.W, seed=100 + i) for i in range(2)], synth_batch(2, P.H, P.W, seed=200)
        src = srcs[0]
        torch.manual_seed(123)
        da.update_dynamic()
        G.switch_batch_statistics(da.model, False)
        da.calculate_prototypes(srcs)
        G.switch_batch_statistics(da.model, True)
        res = {"proto0": da.prototypes.prototypes.clone(), "counter0": da.prototypes.counter.clone()}
        da.optimizer.zero_grad()
        names, before = [], []
        for who, mod in (("student.", da.model), ("teacher.", da.ema_model)):
            for n, p in mod.state_dict().items():
                names.append(who + n)
                before.append(digest(p.float(), 64))
        da.adjust_learning_rate(0, 6)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            log = da.step([src], trg)
        da.update_ema()
        lg = G.tolog(log)
        res["log_json"] = np.array(json.dumps({k: v for k, v in lg.items() if np.isscalar(v)}))
        res["soft"] = trg["stored_predictions"].to(torch.float32)
        res["proto1"] = da.prototypes.prototypes.clone()
        after = [digest(p.float(), 64) for mod in (da.model, da.ema_model) for p in mod.state_dict().values()]
        res["state_names"], res["state_before"], res["state_after"] = np.array(names), np.stack(before), np.stack(after)
        print("step log:", {k: round(v, 5) for k, v in json.loads(str(res["log_json"])).items()})
        save("g26_proda101_step", res)


def g27():
    def build():
        m = get_deeplab_v2(19, True, [1, 1, 1, 1], "ProDA", norm_grad=True)
        m.multi_level = False
        return m
    runs = {}
    for dtype in (torch.float64, torch.float32):
        m = seeded(build).to(dtype)
        _, o = m(synth_batch(2, P.H, P.W)["image"].to(dtype))
        loss_calc(o["out"], S.labels(), "cpu").backward()
        runs[dtype] = m
    m64, m32 = runs[torch.float64], runs[torch.float32]
    bn = [n for n in P.bn_param_names(m32) if dict(m32.named_parameters())[n].requires_grad]
    assert len(bn) == 10, bn
    p64, p32 = dict(m64.named_parameters()), dict(m32.named_parameters())
    res = {"names": np.array(bn), "lr": np.array(P.SGD_LR)}
    for i, n in enumerate(bn):
        res[f"g64_{i}"], res[f"g32_{i}"] = p64[n].grad.numpy(), p32[n].grad.numpy()
        res[f"before_{i}"] = p32[n].detach().clone().numpy()
        print(f"{n}: e_ref {rel(p32[n].grad, p64[n].grad):.3e}")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = torch.optim.SGD(m32.optim_parameters(P.SGD_LR), lr=P.SGD_LR, momentum=0.9, weight_decay=5e-4)
    opt.step()
    for i, n in enumerate(bn):
        res[f"after_{i}"] = p32[n].detach().numpy()
    save("g27_norm_grad", res)


if __name__ == "__main__":
    parts = sys.argv[1:] or ["g26", "g27", "step"]
    if "g26" in parts:
        g26()
    if "g27" in parts:
        g27()
    if "step" in parts:
        g26_step()
