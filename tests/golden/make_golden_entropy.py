#!/usr/bin/env python3
"""Generate G19: ADVENT's entropy map and its gradient, by IMPORTING the reference's ``prob_2_entropy``
(framework/utils/func.py) and running the expression of advent_da.py:94-128 on the CPU (run in the build container only):

    python tests/golden/make_golden_entropy.py          # writes g19_entropy.npz

Per case of tests/entropy_fp64.G19_CASES: the low-resolution logits ``x``, a cotangent ``c``, the reference's
``prob_2_entropy(F.softmax(interp(x)))`` (``F.softmax`` without ``dim``, as the reference calls it: torch picks dim=1 for a
4-D input) and the gradient of ``(map * c).sum()`` with respect to ``x``.  Inputs and outputs only."""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("ONDA_REFERENCE", "/root/reference")
sys.path[:0] = [REF, os.path.join(HERE, "_stubs"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402
from torch.functional import F  # noqa: E402

from framework.utils.func import prob_2_entropy  # noqa: E402

import entropy_fp64 as E  # noqa: E402


def main():
    out = {}
    for case in E.G19_CASES:
        x, cot = E.inputs(case)
        interp = nn.Upsample(size=tuple(cot.shape[2:]), mode="bilinear", align_corners=True)
        lo = x.clone().requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "Implicit dimension choice for softmax"
            ent = prob_2_entropy(F.softmax(interp(lo)))
        ent.backward(cot)
        key = E.case_id(case)
        out[key + "_x"], out[key + "_c"] = x.numpy(), cot.numpy()
        out[key + "_map"], out[key + "_grad"] = ent.detach().numpy(), lo.grad.numpy()
        print(key, float(ent.detach().sum()), float(lo.grad.abs().sum()))
    path = os.path.join(HERE, "g19_entropy.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
