#!/usr/bin/env python3
"""Generate G31: the reference's validation pass, by IMPORTING its ``evaluate_model``
(framework/domain_adaptation/eval_UDA.py) and running it on the CPU (run in the build container only):

    python tests/golden/make_golden_eval.py          # writes g31_evaluate_model.npz

The model is a stand-in that returns its input as ``(None, {"out": x, "feat": x})``, so a batch's "image" IS the [B,19,5,9]
logits; the loader is three batches of 2, 2 and 1 frames -- the short last one pins the reference's unweighted mean over the
batches.  interp: 33x65, intrp_org: 41x77.  Three calls: with return_entropy, with intrp_org, with neither.  Stored: the
logits, `label` and `label_raw` per batch, the IoU vectors of every call, the reference's entropy (a mean of float32 values)
and the float64 entropy of tests/eval_fp64.py's restatement.

Condition on the inputs: no pixel is excluded from the comparison, so the seed is advanced until every pixel's top-2 margin of
the float64 upsampled logits, at both sizes, is at least MARGIN = 1e-4 (a float32 ulp at |x| = 8 is 1e-6), and fp32 ATen's
argmax is asserted to equal the float64 one."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("ONDA_REFERENCE", "/root/reference")
sys.path[:0] = [REF, os.path.join(HERE, "_stubs"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from framework.domain_adaptation.eval_UDA import evaluate_model  # noqa: E402

import eval_fp64 as V  # noqa: E402
import upsample_fp64 as U  # noqa: E402

K, LOW, SIZE, SIZE_ORG, BATCHES = 19, (5, 9), (33, 65), (41, 77), (2, 2, 1)
MARGIN = 1e-4


class Cfg(dict):
    __getattr__ = dict.__getitem__


class StandIn(nn.Module):
    def forward(self, x):
        return None, {"out": x, "feat": x}


def labels_of(g, b, size):
    lab = torch.randint(0, K + 2, (b,) + size, generator=g).to(torch.uint8)
    lab[lab >= K] = 255
    return lab


def draw(seed):
    g = torch.Generator().manual_seed(seed)
    return [{"image": torch.randn(b, K, *LOW, generator=g) * 3, "label": labels_of(g, b, SIZE), "label_raw": labels_of(g, b, SIZE_ORG)}
            for b in BATCHES]


def margin(batches):
    """(the smallest top-2 margin of the float64 upsampled logits over every pixel, batch and size, whether fp32 ATen's
    classes equal the float64 ones everywhere)."""
    worst, agree = float("inf"), True
    for batch in batches:
        for size in (SIZE, SIZE_ORG):
            cls, m, _ = U.class_map(U.upsample(batch["image"], *size))
            worst = min(worst, float(m.min()))
            agree = agree and torch.equal(cls, F.interpolate(batch["image"], size=size, mode="bilinear", align_corners=True).argmax(1))
    return worst, agree


def main():
    seed = 31
    while True:
        batches = draw(seed)
        m, agree = margin(batches)
        print("seed", seed, "smallest top-2 margin", m)
        if m >= MARGIN:
            assert agree, "fp32 ATen's argmax differs from the float64 one at a margin of 1e-4"
            break
        seed += 1
    cfg = Cfg(device="cpu", NUM_CLASSES=K)
    interp = nn.Upsample(size=SIZE, mode="bilinear", align_corners=True)
    interp_org = nn.Upsample(size=SIZE_ORG, mode="bilinear", align_corners=True)
    iou_a, entropy = evaluate_model(StandIn(), batches, interp, cfg, return_entropy=True)
    iou_b, iou_org = evaluate_model(StandIn(), batches, interp, cfg, intrp_org=interp_org)
    iou_c, = evaluate_model(StandIn(), batches, interp, cfg)
    assert np.array_equal(iou_a, iou_b) and np.array_equal(iou_a, iou_c)
    entropy64 = float(np.mean([V.restate(b["image"], b["label"])[2] for b in batches]))
    print("mIoU", np.nanmean(iou_a), "full image", np.nanmean(iou_org), "entropy", entropy, "float64", entropy64,
          "relative error of the reference", abs(entropy - entropy64) / entropy64)
    out = {"seed": np.int64(seed), "margin": np.float64(m), "size": np.asarray(SIZE, np.int64), "size_org": np.asarray(SIZE_ORG, np.int64),
           "iou": np.asarray(iou_a, np.float64), "iou_org": np.asarray(iou_org, np.float64), "entropy": np.float64(entropy),
           "entropy64": np.float64(entropy64)}
    for i, b in enumerate(batches):
        out[f"x{i}"], out[f"label{i}"], out[f"label_raw{i}"] = b["image"].numpy(), b["label"].numpy(), b["label_raw"].numpy()
    path = os.path.join(HERE, "g31_evaluate_model.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
