#!/usr/bin/env python3
"""Generate G25: the reference's 'normal' classifier head (``ClassifierModule``, framework/model/deeplabv2.py:71-95) on the CPU,
in float64 and in float32, by IMPORTING the reference (run in the build container only):

    python tests/golden/make_golden_normal_head.py          # writes g25_normal_head.npz

(a) ``a_*`` -- the head alone: ``ClassifierModule(64, [6,12,18,24], [6,12,18,24], 19)`` with the weights and biases of
``normal_head_common.head_params()`` on ``head_input()`` ([2,64,27,34]), backward from ``head_dout()``: the output, dx, the four
dW and the four db of both runs.  The float64 output is stored whole (rounded to float32: 6e-8 relative), everything else as the
strided samples of ``normal_head_common.sampled`` (HEAD_SAMPLE / HEAD_W_SAMPLE elements; the db whole), to stay within the size a
committed file may have.

(b) ``b_*`` -- the model: the reference's ``get_model`` with ``NAME: DeepLabv2-Resnet50, CLASSIFIER: 'normal', MULTI_LEVEL: True``.
First, under ``torch.manual_seed(0)``, the freshly constructed model: its state_dict key / shape / dtype list, the trainable
names, per-key mean and standard deviation of the initial values, and the ``optim_parameters`` walk (parameter names per group,
in order, duplicates included).  Then the WEIGHT-FILL RECIPE both sides use: every state_dict entry from
``onda_amd.synthetic.synth_tensor(key, ..., seed 1, head_scale 3.0)`` (He-style conv weights -- the eight head convolutions
included --, N(0, 0.1) biases, BatchNorm gamma in [0.75, 1.25) with ``.bn3.`` scaled by 0.4, running_mean 0.1 N(0,1), running_var
0.5 + U[0,1)), train mode, the image and the full-resolution label of ``synth_batch(2, 64, 128)``, and the loss of
segmentation.py:70-80: ``loss_calc(interp(main), label) + 0.1 * loss_calc(interp(aux), label)`` with ``interp`` the bilinear
``align_corners=True`` upsampling to 64 x 128.  Stored: both logit maps and the loss of both runs, and of every trainable
parameter's gradient the strided sample of ``normal_head_common.grad_samples`` from both runs (the float64 run's tensors rounded to
float32; the loss stays a double).  Inputs and outputs only."""
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
from framework.model.deeplabv2 import ClassifierModule  # noqa: E402
from framework.utils.func import loss_calc  # noqa: E402

from onda_amd.synthetic import fill_state_dict, synth_batch  # noqa: E402

import normal_head_common as C  # noqa: E402

torch.set_num_threads(8)


def head_run(dtype):
    m = ClassifierModule(C.HEAD_CIN, list(C.DILATIONS), list(C.DILATIONS), C.CLASSES)
    ws, bs = C.head_params()
    with torch.no_grad():
        for conv, w, b in zip(m.conv2d_list, ws, bs):
            conv.weight.copy_(w)
            conv.bias.copy_(b)
    m = m.to(dtype)
    x = C.head_input().to(dtype).requires_grad_(True)
    out = m(x)
    out.backward(C.head_dout().to(dtype))
    return out.detach(), x.grad, [c.weight.grad for c in m.conv2d_list], [c.bias.grad for c in m.conv2d_list]


def part_a(res):
    (o64, dx64, dw64, db64), (o32, dx32, dw32, db32) = head_run(torch.float64), head_run(torch.float32)
    res["a_out64"] = o64.float().numpy()
    res["a_out32_sample"] = C.sampled(o32, C.HEAD_SAMPLE).numpy()
    res["a_dx64_sample"], res["a_dx32_sample"] = C.sampled(dx64, C.HEAD_SAMPLE).float().numpy(), C.sampled(dx32, C.HEAD_SAMPLE).numpy()
    for i in range(len(C.DILATIONS)):
        res[f"a_dw64_{i}_sample"] = C.sampled(dw64[i], C.HEAD_W_SAMPLE).float().numpy()
        res[f"a_dw32_{i}_sample"] = C.sampled(dw32[i], C.HEAD_W_SAMPLE).numpy()
        res[f"a_db64_{i}"], res[f"a_db32_{i}"] = db64[i].float().numpy(), db32[i].numpy()
    print("(a) out32 vs out64: %.3e of the maximum" % float((o32.double() - o64).abs().max() / o64.abs().max()))


def ref_model():
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NAME=C.MODEL, CLASSIFIER="normal", LOAD=None, MULTI_LEVEL=True),
                                OTHERS=types.SimpleNamespace(DEVICE="cpu"))
    return get_model(cfg, C.CLASSES)


def model_run(dtype):
    m = ref_model()
    fill_state_dict(m, 1, 3.0)
    m = m.train().to(dtype)
    batch = synth_batch(2, 64, 128)
    aux, main = m(batch["image"].to(dtype))
    assert torch.is_tensor(main) and torch.is_tensor(aux)
    interp = torch.nn.Upsample(size=(64, 128), mode="bilinear", align_corners=True)
    loss = loss_calc(interp(main), batch["label"], "cpu") + 0.1 * loss_calc(interp(aux), batch["label"], "cpu")
    loss.backward()
    return m, main.detach(), aux.detach(), loss


def part_b(res):
    torch.manual_seed(0)
    fresh = ref_model()
    sd = fresh.state_dict()
    res["b_keys"] = np.array(list(sd))
    res["b_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    res["b_dtypes"] = np.array([str(v.dtype) for v in sd.values()])
    res["b_trainable"] = np.array([n for n, p in fresh.named_parameters() if p.requires_grad])
    res["b_init_mean"] = np.array([float(v.double().mean()) for v in sd.values()])
    res["b_init_std"] = np.array([float(v.double().std()) if v.numel() > 1 else 0.0 for v in sd.values()])
    name_of = {id(p): n for n, p in fresh.named_parameters()}
    for gi, group in enumerate(fresh.optim_parameters(2.5e-4)):
        res[f"b_group{gi}"] = np.array([name_of[id(p)] for p in group["params"]])
        res[f"b_group{gi}_lr"] = float(group["lr"])
    res["b_feat_flag"] = bool(fresh.feat)

    m64, main64, aux64, l64 = model_run(torch.float64)
    m32, main32, aux32, l32 = model_run(torch.float32)
    res["b_main64"], res["b_aux64"], res["b_loss64"] = main64.float().numpy(), aux64.float().numpy(), l64.item()
    res["b_main32"], res["b_aux32"], res["b_loss32"] = main32.numpy(), aux32.numpy(), l32.item()
    p64, p32 = dict(m64.named_parameters()), dict(m32.named_parameters())
    graded = [n for n, p in m32.named_parameters() if p.requires_grad and p.grad is not None]
    assert graded == [n for n, p in m64.named_parameters() if p.requires_grad and p.grad is not None]
    res["b_grad_names"] = np.array(graded)
    worst = 0.0
    for i, n in enumerate(graded):
        g64, g32 = C.sampled(p64[n].grad, C.grad_samples(n)), C.sampled(p32[n].grad, C.grad_samples(n))
        res[f"b_g64_{i}"], res[f"b_g32_{i}"] = g64.float().numpy(), g32.numpy()
        worst = max(worst, float((g32.double() - g64).norm() / (g64.norm() + 1e-30)))
    print("(b) loss %.6f / %.6f; e_ref worst %.3e; main32 vs main64 %.3e of the maximum" % (
        l64.item(), l32.item(), worst, float((main32.double() - main64).abs().max() / main64.abs().max())))


def main():
    t0 = time.time()
    res = {}
    part_a(res)
    part_b(res)
    path = os.path.join(HERE, "g25_normal_head.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes, %.1f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
