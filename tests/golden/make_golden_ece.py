#!/usr/bin/env python3
"""Generate G18: the reference's expected calibration error, by IMPORTING its ``ECE`` (framework/utils/monitoring.py)
and running it behind ``nn.Upsample(bilinear, align_corners=True)`` on the CPU (run in the build container only):

    python tests/golden/make_golden_ece.py          # writes g18_ece.npz

Per case the low-resolution logits (the "probs" input is their softmax), a digest of the seeded labels, the
non-empty rows of the reference's float32 table ``calc_matrix`` [bins, 3] and its ECE
value, in both modes: "logits" = record(interp(x).softmax(1), label) (adaptation_model.py:145-149) and "probs" =
record(interp(x), label) (prototypes.py:200).  The inputs are those of tests/ece_fp64.py (which imports nothing of the
reference); the exact cases are its `safe` variants: the reference raises on a non-finite confidence and on one whose
bin is >= bins."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("ONDA_REFERENCE", "/root/reference")
sys.path[:0] = [REF, os.path.join(HERE, "_stubs"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

from framework.utils.monitoring import ECE  # noqa: E402

import ece_fp64 as E  # noqa: E402

BINS = 1000


def reference(x, labels, bins, mode):
    interp = nn.Upsample(size=tuple(labels.shape[1:]), mode="bilinear", align_corners=True)
    ece = ECE(bins)
    pred = interp(x)
    ece.record(pred.softmax(1) if mode == "logits" else pred, labels, axis=1)
    return ece.calc_matrix.clone(), ece().item()


def label_digest(labels):
    """The labels are seeded (ece_fp64.inputs); the fixture keeps their per-value counts and a position-weighted sum."""
    flat = labels.reshape(-1).long()
    return np.concatenate([np.bincount(flat.numpy(), minlength=256), [int((flat * (torch.arange(flat.numel()) % 8191 + 1)).sum())]])


def put_table(out, key, table, value):
    rows = (table[:, 2] != 0).nonzero()[:, 0]
    out[key + "_rows"], out[key + "_table"], out[key + "_ece"] = rows.numpy().astype(np.int32), table[rows].numpy(), np.float64(value)


def main():
    out = {"bins": np.int64(BINS)}
    for case in E.CASES:
        for mode in ("logits", "probs"):
            x, labels = E.inputs(case, mode)
            key = f"{E.case_id(case)}_{mode}"
            table, value = reference(x, labels, BINS, mode)
            if mode == "logits":
                out[E.case_id(case) + "_x"], out[E.case_id(case) + "_labels_digest"] = x.numpy(), label_digest(labels)
            put_table(out, key, table, value)
            print(key, value)
    x, labels = E.contention_inputs()
    table, value = reference(x, labels, BINS, "logits")
    out["contention_x"], out["contention_labels_digest"] = x.numpy(), label_digest(labels)
    put_table(out, "contention", table, value)
    K = E.EXACT_CASE[4]
    for bins in E.EXACT_BINS:
        conf, cls, labels = E.exact_inputs(bins, safe=True)
        table, value = reference(E.exact_map(conf, cls, K), labels, bins, "probs")
        key = f"exact{bins}"
        out[key + "_conf"], out[key + "_cls"], out[key + "_labels"] = conf.numpy(), cls.numpy(), labels.numpy()
        out[key + "_table"], out[key + "_ece"] = table.numpy(), np.float64(value)
        print(key, value)
    path = os.path.join(HERE, "g18_ece.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
