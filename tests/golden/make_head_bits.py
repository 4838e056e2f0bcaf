"""Digests of everything the bilinear (align_corners) head kernels of csrc/pointwise.hip put out, through the public
onda_amd.ops functions only -- so this file runs unchanged in a checkout of any commit that has those functions.

    python tests/golden/make_head_bits.py [--out tests/golden/head_bits.json]      (on the MI355X)

writes {"torch": ..., "hip": ..., "digests": {name: sha256 of the output's raw bytes}}.  tests/test_head_bits.py recomputes
`digests()` and compares.  Sound because every one of these kernels sums in a fixed order or counts integers; the fused
cross-entropy's partial sums follow the launch grid, so the digests pin the host launches as well.  The fixture is recorded
at a commit whose kernels are trusted (the parent of the change under test), never from the code under test.

Inputs: the CPU-seeded generators of tests/upsample_fp64.py, entropy_fp64.py and ece_fp64.py, no shapes of its own.
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)
import ece_fp64 as C  # noqa: E402
import entropy_fp64 as E  # noqa: E402
import upsample_fp64 as U  # noqa: E402

DEV = "cuda:0"
FIXTURE = os.path.join(HERE, "head_bits.json")
ECE_BINS = (1000, 2048)  # at or below / above the 2047 bins a workgroup counts in LDS
# B, h, w, K, ldl, H, W: PAST_FUSED_CASE's shape on the entropy route (per-pixel gradient + plain gather, 16-byte loads)
ENTROPY_PAST_FUSED = (1,) + U.PAST_FUSED_CASE[:2] + U.PAST_FUSED_CASE[4:] + U.PAST_FUSED_CASE[2:4]
ECE_CASES = C.CASES + ([] if any(c[4] > 32 for c in C.CASES) else [U.HIST_GLOBAL_CASE])  # K > 32: classes not kept in registers


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def toolchain():
    return {"torch": str(torch.__version__), "hip": str(torch.version.hip)}


def head_out(x, ld):
    """CPU [B,K,h,w] on the device in the model's output layout: a [B,K,h,w] view of pixel-major rows of `ld` floats."""
    B, K, h, w = x.shape
    pad = torch.zeros(B, h, w, ld)
    pad[..., :K] = x.permute(0, 2, 3, 1)
    return pad.to(DEV)[..., :K].permute(0, 3, 1, 2)


def digests():
    from onda_amd import ops
    d = {}
    for case in U.CASES + [U.HIST_GLOBAL_CASE, U.PAST_FUSED_CASE]:
        h, w, H, W, K, ldl = case
        B = 1 if case == U.PAST_FUSED_CASE else U.BATCH
        x, lab = U.inputs(case, B)
        name = U.case_id(case)
        if case in U.CASES:
            out = head_out(x, ldl).detach().requires_grad_(True)
            up = ops.UpsampleFn.apply(out, (H, W))
            up.backward(U.upstream_gradient(case).to(DEV))
            d[f"upsample fwd {name}"], d[f"upsample bwd {name}"] = sha(up), sha(out.grad)
        if K <= 32:
            out = head_out(x, ldl).detach().requires_grad_(True)
            loss = ops.upsample_ce(out, lab.to(DEV))
            (2.5 * loss).backward()
            d[f"ce value {name}"], d[f"ce grad {name}"] = sha(loss), sha(out.grad)
        if case != U.PAST_FUSED_CASE:
            d[f"argmax {name}"] = sha(ops.upsample_argmax(head_out(x, ldl), (H, W)))
            hist = torch.zeros(K, K, dtype=torch.int64, device=DEV)
            ops.upsample_argmax_hist(head_out(x, ldl), lab.to(DEV), hist, K)
            d[f"argmax hist {name}"] = sha(hist)
    for case in ECE_CASES:
        K, ld = case[4], case[5]
        for mode in ("logits", "probs"):
            x, lab = C.inputs(case, mode)
            for bins in ECE_BINS:
                for with_hist in (False, True):
                    table = torch.zeros(bins + 1, 3, dtype=torch.int64, device=DEV)
                    hist = torch.zeros(K, K, dtype=torch.int64, device=DEV) if with_hist else None
                    ops.upsample_ece(head_out(x, ld), lab.to(DEV), table, bins, probs=(mode == "probs"), hist=hist)
                    name = f"{C.case_id(case)} {mode} bins {bins}"
                    if with_hist:
                        d[f"ece+hist table {name}"], d[f"ece+hist hist {name}"] = sha(table), sha(hist)
                    else:
                        d[f"ece table {name}"] = sha(table)
    for case in E.CASES + [ENTROPY_PAST_FUSED]:
        B, h, w, K, ldl, H, W = case
        x, cot = E.inputs(case)
        out = head_out(x, ldl).detach().requires_grad_(True)
        ent = ops.upsample_entropy(out, (H, W))
        ent.backward(cot.to(DEV))
        d[f"entropy map {E.case_id(case)}"], d[f"entropy grad {E.case_id(case)}"] = sha(ent), sha(out.grad)
    torch.cuda.synchronize()
    return d


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    rec = dict(toolchain(), digests=digests())
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec['digests'])} digests -> {path} (torch {rec['torch']}, hip {rec['hip']})")
