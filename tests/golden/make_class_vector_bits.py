"""Digests of everything the per-pixel class-vector kernels of csrc/loss_proto.hip put out -- the two loss families and their
gradients, softmax statistics, the prototype kernels, the multi-tensor SGD and EMA -- through public Python entry points only
(onda_amd.ops and prototype_handler), so this file runs unchanged in a checkout of any commit that has them.

    python tests/golden/make_class_vector_bits.py --out first.json                      (on the MI355X)
    python tests/golden/make_class_vector_bits.py --second-of first.json [--out tests/golden/class_vector_bits.json]

The first call writes {"torch": ..., "hip": ..., "digests": {name: sha256 of the output's raw bytes}}.  The second, a new
process, records again and writes the fixture: the first record plus "unstable", the keys whose two digests differ.  Only the
three monitor means of onda_proto_assign ("proto means ...") may be unstable: the pixels whose decision the MFMA kernel does
not trust are handed to the direct kernel through a list whose slots an atomic counter gives out, so the order of that
kernel's partial sums changes from run to run; those means stay held by the tolerance tests test_prototypes_golden and
test_prototypes_full_size.  Any other unstable key stops the recording.  tests/test_class_vector_bits.py recomputes `digests()`
and compares every stable key.  Sound because every other kernel here sums in a fixed order; the block partials follow the
launch grid, so the digests pin the host launches as well.  The fixture is recorded at a commit whose kernels are trusted
(the parent of the change under test), never from the code under test.  One exception so far, the change that made
proto_assign_mfma_kernel centre features and prototypes on the mean prototype and accumulate each 128-channel half from zero: it
changes the arithmetic of the soft map on purpose, so the 48 "proto soft" keys (and the 20 "proto means" keys that moved with
them) were recorded from it, twice in separate processes, after every other key -- the 48 "proto labels" among them -- had been
found equal to the parent's record; the new soft maps are held to float64 by tests/test_proto_fp64_parity.py.

Inputs: CPU-seeded generators below, fixtures G4 (prototypes) and G16 (label patterns of test_target_regularisers.SMALL).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
FIXTURE = os.path.join(HERE, "class_vector_bits.json")
PIXELS = (37, 256, 700)  # of a 256-pixel workgroup: below one, exactly one, a ragged third
CLASSES = (2, 19, 32)
SMALL = ("mixed", "none_ignored", "all_ignored", "saturated")  # test_target_regularisers.SMALL
WEIGHTS = (0.1, 1.0, 0.1)  # w_ce, w_rce, w_reg
GSCALE = 2.5  # upstream gradient of `total`
UNSTABLE_PREFIX = "proto means "


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def toolchain():
    return {"torch": str(torch.__version__), "hip": str(torch.version.hip)}


def head_out(x, ld):
    """CPU [B,K,h,w] on the device in the model's output layout: a [B,K,h,w] view of pixel-major rows of `ld` floats."""
    B, K, h, w = x.shape
    pad = torch.zeros(B, h, w, ld)
    pad[..., :K] = x.permute(0, 2, 3, 1)
    return pad.to(DEV)[..., :K].permute(0, 3, 1, 2)


def row_inputs(N, K):
    """logits [1,K,1,N] and labels [1,1,N]: classes, ~20 % 255, one negative and one >= K."""
    gen = torch.Generator().manual_seed(1000 * K + N)
    logits = 3.0 * torch.randn(1, K, 1, N, generator=gen)
    labels = torch.randint(0, K, (1, 1, N), generator=gen)
    labels[torch.rand(1, 1, N, generator=gen) < 0.2] = 255
    labels[0, 0, 3], labels[0, 0, N - 2], labels[0, 0, 5], labels[0, 0, 7] = -1, K, 255, K - 1
    return logits, labels


def loss_digests(d, name, logits, labels, ld):
    from onda_amd import ops
    lab = labels.to(DEV)
    w_ce, w_rce, w_reg = WEIGHTS
    out = head_out(logits, ld).detach().requires_grad_(True)
    vals = ops.seg_losses(out, lab, w_ce, w_rce, w_reg)
    (GSCALE * vals[0]).backward()
    d[f"seg_loss values {name}"], d[f"seg_loss grad {name}"] = sha(*vals), sha(out.grad)
    for reg in ("MRKLD", "MRENT", "none"):
        for w_js in (0.0, 3.0):
            out = head_out(logits, ld).detach().requires_grad_(True)
            vals = ops.target_losses(out, lab, w_ce, w_rce, w_reg, reg, w_js)
            (GSCALE * vals[0]).backward()
            d[f"target_loss values {reg} js {w_js} {name}"] = sha(*vals)
            d[f"target_loss grad {reg} js {w_js} {name}"] = sha(out.grad)
    conf, probs, am = ops.softmax_stats(head_out(logits, ld), True, True)
    d[f"softmax_stats {name}"] = sha(conf, probs, am)
    d[f"softmax_stats mean only {name}"] = sha(ops.softmax_stats(head_out(logits, ld))[0])


def golden(name):
    z = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
    return {k: torch.from_numpy(z[k]) for k in z.files if z[k].dtype.kind in "fiu"}


def handler(state, metric, tau=1, thresh=0.3):
    from onda_amd.framework.domain_adaptation.methods.prototype_handler import prototype_handler
    h = prototype_handler(0.9995, tau, thresh, metric)
    if state is not None:
        h.prototypes, h.squared_mean, h.counter = (t.clone().to(DEV) for t in state)
    return h


def assign_digests(d, name, state, feat, prior):
    for metric in ("mahalanobis", "euclidean"):
        for with_prior in (False, True):
            for tau in (1, 2):
                for thresh in (0, 0.3):
                    labels, soft, means = handler(state, metric, tau, thresh).assign_stats(feat, prior if with_prior else None)
                    tag = f"{name} {metric} prior {int(with_prior)} tau {tau} thresh {thresh}"
                    d[f"proto labels {tag}"], d[f"proto soft {tag}"] = sha(labels), sha(soft)
                    d[f"{UNSTABLE_PREFIX}{tag}"] = sha(torch.tensor(means, dtype=torch.float64))
    d[f"proto distance {name}"] = sha(handler(state, "euclidean").distance(feat))
    d[f"proto mahalanobis_distance {name}"] = sha(handler(state, "mahalanobis").mahalanobis_distance(feat))
    d[f"proto global_var {name}"] = sha(handler(state, "mahalanobis").global_var())


def prototype_digests(d):
    g = golden("g4_prototypes")
    for regime in ("far", "near"):
        t = lambda k: g[f"{regime}_{k}"]
        state = (t("proto"), t("sqmean"), t("counter"))
        feat = t("feat").permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)  # the model's own layout
        prior, out = t("prior").to(DEV), t("out").to(DEV)
        assign_digests(d, regime, state, feat, prior)
        K = state[0].shape[0]
        h = handler(state, "mahalanobis")
        d[f"proto class_statistics {regime}"] = sha(h.class_statistics(feat, out)[0])
        cls = torch.randint(-2, K + 2, (feat.shape[0] * feat.shape[2] * feat.shape[3],), generator=torch.Generator().manual_seed(5))
        d[f"proto class_statistics classes= {regime}"] = sha(h.class_statistics(feat, K, classes=cls)[0])
        h.ma(feat, out)
        d[f"proto ma {regime}"] = sha(h.prototypes, h.squared_mean)
        h2 = handler(None, "mahalanobis")
        h2.append(feat, out)
        d[f"proto append 1 {regime}"] = sha(h2.prototypes, h2.squared_mean, h2.counter)
        h2.append(feat * 0.5 + 0.1, out.flip(0))
        d[f"proto append 2 {regime}"] = sha(h2.prototypes, h2.squared_mean, h2.counter)
        d[f"proto append global_var {regime}"] = sha(h2.global_var())
    # K = 32, the class-vector limit: 231 pixels, neither a multiple of 32 nor of 4
    gen = torch.Generator().manual_seed(32)
    proto = torch.randn(32, 256, generator=gen)
    state = (proto, proto ** 2 + (0.5 + torch.rand(32, 256, generator=gen)) ** 2, torch.randint(1, 500, (32,), generator=gen).float())
    rows = proto[torch.randint(0, 32, (231,), generator=gen)] + 0.7 * torch.randn(231, 256, generator=gen)
    feat = rows.reshape(1, 7, 33, 256).to(DEV).permute(0, 3, 1, 2)
    prior = (2 * torch.randn(1, 32, 7, 33, generator=gen)).softmax(1).to(DEV)
    assign_digests(d, "K32", state, feat, prior)


def offset_tensor(values):
    """`values` on the device in a view one float past a 16-byte boundary: the multi-tensor kernels' scalar path."""
    base = torch.zeros(values.numel() + 1, device=DEV)
    assert base.data_ptr() % 16 == 0
    view = base[1:]
    view.copy_(values)
    return view


def multi_tensor_digests(d):
    from onda_amd import ops
    gen = torch.Generator().manual_seed(77)
    sizes = (7, 4096, 33333)  # a tail alone, one full block (off the 16-byte boundary), full blocks + a tail
    put = lambda i, v: offset_tensor(v) if i == 1 else v.to(DEV)
    ps, gs = ([put(i, torch.randn(n, generator=gen)) for i, n in enumerate(sizes)] for _ in range(2))
    bs = [put(i, torch.full((n,), float("nan"))) for i, n in enumerate(sizes)]  # fresh: never read
    lrs = (8e-4, 1e-4, 2.5e-3)
    ops.sgd_multi([(p, g, b, lr, times, 1) for p, g, b, lr, times in zip(ps, gs, bs, lrs, (1, 3, 1))], 0.9, 1e-4, 0.25)
    d["sgd_multi fresh"] = sha(*ps, *bs)
    ops.sgd_multi([(p, g, b, lr, times, 0) for p, g, b, lr, times in zip(ps, gs, bs, lrs, (3, 1, 3))], 0.9, 1e-4, 0.25)
    d["sgd_multi momentum"] = sha(*ps, *bs)
    ks, qs = ([put(i, torch.randn(n, generator=gen)) for i, n in enumerate(sizes)] for _ in range(2))
    ops.ema_multi([(k, q, keep, 1.0 - keep) for k, q, keep in zip(ks, qs, (0.999, 0.0, 0.999))])
    d["ema_multi 1"] = sha(*ks)
    ops.ema_multi([(k, q, keep, 1.0 - keep) for k, q, keep in zip(ks, gs, (0.0, 0.999, 0.0))])
    d["ema_multi 2"] = sha(*ks)


def digests():
    d = {}
    for N in PIXELS:
        for K in CLASSES:
            logits, labels = row_inputs(N, K)
            for ld in sorted({K, 32}):
                loss_digests(d, f"N {N} K {K} ld {ld}", logits, labels, ld)
    g = golden("g16_regularisers")
    for case in SMALL:
        loss_digests(d, case, g[f"{case}_logits"], g[f"{case}_target"], 32)
    prototype_digests(d)
    multi_tensor_digests(d)
    torch.cuda.synchronize()
    return d


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    rec = dict(toolchain(), digests=digests())
    if "--second-of" in sys.argv:
        with open(sys.argv[sys.argv.index("--second-of") + 1]) as f:
            first = json.load(f)
        assert sorted(first["digests"]) == sorted(rec["digests"]) and toolchain() == {k: first[k] for k in ("torch", "hip")}
        rec["unstable"] = sorted(k for k in rec["digests"] if rec["digests"][k] != first["digests"][k])
        bad = [k for k in rec["unstable"] if not k.startswith(UNSTABLE_PREFIX)]
        assert not bad, f"outputs other than the monitor means differ between two runs of one library: {bad}"
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec['digests'])} digests, {len(rec.get('unstable', []))} unstable -> {path} (torch {rec['torch']}, hip {rec['hip']})")
