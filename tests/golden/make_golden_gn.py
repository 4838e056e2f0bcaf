#!/usr/bin/env python3
"""Generate G21: one train-mode forward + backward of the reference's ``DeepLabv2-Resnet50-GN`` on the CPU, in float64 and in
float32, by IMPORTING the reference's ``get_model`` (framework/handlers/model_handler.py; run in the build container only):

    python tests/golden/make_golden_gn.py          # writes g21_gn_model.npz, g22_gn_step_static.npz, g22_gn_step_dynamic.npz

Both sides use: the handler's GN model (built ``multi_level=True``, run with it False), every state_dict entry from
``onda_amd.synthetic.synth_tensor(key, ..., 1, 3.0)``, ``Dropout2d.p = 0``, the image of ``synth_batch(2, 64, 128)`` and the
labels of ``labels()`` below ([2, 9, 17], one row of 255).

The file holds the key / shape / dtype list of the state_dict, the names of the trainable parameters, ``feat`` / ``out`` / the CE
loss of both runs, and the gradient of every trainable parameter from both runs: whole for ``conv1.weight`` and
``layer1.0.downsample.0.weight``, the fixed strided sample of ``sample_index`` for the rest (``SAMPLE_DS`` values for the three
larger shortcut weights, ``SAMPLE`` for everything else).  To stay within the size a committed file may have, the float64 run's
tensors are stored rounded to float32 (6e-8 relative, four orders below every bar they are used for; the loss stays a double)
and the float32 run's ``feat`` as a strided sample.  Inputs and outputs only."""
import os
import sys
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("ONDA_REFERENCE", "/root/reference")
sys.path[:0] = [REF, os.path.join(HERE, "_stubs"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from framework.handlers.model_handler import get_model  # noqa: E402
from framework.utils.func import loss_calc  # noqa: E402

from onda_amd.synthetic import fill_state_dict, synth_batch  # noqa: E402

import gn_site_fp64 as S  # noqa: E402

torch.set_num_threads(8)


def ref_model(head_scale=3.0, dropout=False):
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NAME=S.GN_MODEL, CLASSIFIER="ProDA", LOAD=None, MULTI_LEVEL=False),
                                OTHERS=types.SimpleNamespace(DEVICE="cpu"))
    m = get_model(cfg, 19)
    fill_state_dict(m, 1, head_scale)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout2d) and not dropout:
            mod.p = 0.0
    return m.train()


def run(dtype):
    m = ref_model().to(dtype)
    _, o = m(synth_batch(2, 64, 128)["image"].to(dtype))
    loss = loss_calc(o["out"], S.labels(), "cpu")
    loss.backward()
    return m, o, loss


def main():
    t0 = time.time()
    res = {}
    m64, o64, l64 = run(torch.float64)
    m32, o32, l32 = run(torch.float32)
    sd = m32.state_dict()
    res["keys"] = np.array(list(sd))
    res["shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    res["dtypes"] = np.array([str(v.dtype) for v in sd.values()])
    names = [n for n, p in m32.named_parameters() if p.requires_grad]
    assert names == [n for n, p in m64.named_parameters() if p.requires_grad]
    res["trainable"] = np.array(names)
    res["counts"] = np.array([sum(isinstance(x, torch.nn.GroupNorm) for x in m32.modules()),
                              sum(isinstance(x, torch.nn.BatchNorm2d) for x in m32.modules()),
                              len(list(m32.parameters())), len(list(m32.buffers()))])
    res["labels"] = S.labels().numpy().astype(np.uint8)
    res["feat64"], res["out64"], res["loss64"] = o64["feat"].detach().float().numpy(), o64["out"].detach().float().numpy(), l64.item()
    f32 = o32["feat"].detach().reshape(-1)
    res["feat32_sample"], res["out32"], res["loss32"] = f32[S.sample_index(f32.numel(), S.SAMPLE_DS)].numpy(), o32["out"].detach().numpy(), l32.item()
    p64, p32 = dict(m64.named_parameters()), dict(m32.named_parameters())
    worst = 0.0
    # (the layer5 head is built and never run: its 30 trainable parameters have no gradient)
    graded = [n for n in names if p32[n].grad is not None]
    assert graded == [n for n in names if p64[n].grad is not None]
    res["grad_names"] = np.array(graded)
    for i, n in enumerate(graded):
        g64, g32 = p64[n].grad.reshape(-1), p32[n].grad.reshape(-1)
        idx = S.grad_index(n, g64.numel())
        if idx is not None:
            g64, g32 = g64[idx], g32[idx]
        res[f"g64_{i}"], res[f"g32_{i}"] = g64.float().numpy(), g32.numpy()
        e = float((g32.double() - g64).norm() / (g64.norm() + 1e-30))
        worst = max(worst, e)
        if n == "conv1.weight" or ".downsample.0." in n:
            print(f"e_ref {n}: {e:.3e}")
    print(f"e_ref worst {worst:.3e}; out32 vs out64 {float((o32['out'].detach().double() - o64['out'].detach()).abs().max() / o64['out'].detach().abs().max()):.3e}; "
          f"{time.time() - t0:.1f} s")
    path = os.path.join(HERE, "g21_gn_model.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


def g22():
    """Two hybrid_proDA steps (+ update_ema) of the reference on its GN model at 128 x 64, B = 2, both switch branches: what g7()
    of make_golden.py captures for the BatchNorm model, with the same configuration, batches, seed and fields."""
    import json
    import tempfile
    import warnings
    import make_golden as G  # the reference's hybrid_proDA, make_cfg, tolog, digest, save
    for tag, head_scale in (("static", 40.0), ("dynamic", 3.0)):
        with tempfile.TemporaryDirectory() as tmp:
            cfg, spec = G.make_cfg(tmp)
            da = G.hybrid_proDA(ref_model(head_scale, dropout=True), cfg, spec)
            src = [synth_batch(2, 64, 128, seed=100 + i) for i in range(2)]
            trg = [synth_batch(2, 64, 128, seed=200 + i) for i in range(2)]
            torch.manual_seed(123)
            da.update_dynamic()
            G.switch_batch_statistics(da.model, False)
            da.calculate_prototypes(src)
            G.switch_batch_statistics(da.model, True)
            res = {"proto0": da.prototypes.prototypes.clone(), "sqmean0": da.prototypes.squared_mean.clone(),
                   "counter0": da.prototypes.counter.clone()}
            da.optimizer.zero_grad()
            for s in range(2):
                da.adjust_learning_rate(s, 6)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    log = da.step([src[s]], trg[s])
                da.update_ema()
                lg = G.tolog(log)
                res[f"log{s}_json"] = np.array(json.dumps({k: v for k, v in lg.items() if np.isscalar(v)}))
                res[f"soft{s}"] = trg[s]["stored_predictions"].to(torch.float32)
                res[f"proto{s + 1}"] = da.prototypes.prototypes.clone()
                res[f"branch{s}"] = np.array(da.model_select.current)
                names, dig = [], []
                for who, mod in (("student.", da.model), ("teacher.", da.ema_model)):
                    for n, p in mod.state_dict().items():
                        names.append(who + n)
                        dig.append(G.digest(p.float(), 64))
                res[f"state_names{s}"] = np.array(names)
                res[f"state_digest{s}"] = np.stack(dig)
            G.save(f"g22_gn_step_{tag}", **res)
            print(tag, "branch", res["branch0"], res["branch1"])


if __name__ == "__main__":
    main()
    g22()
