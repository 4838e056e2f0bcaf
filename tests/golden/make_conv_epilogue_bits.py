"""Digests of what the convolutions' OUTPUT side puts out -- the tile epilogues of csrc/conv_l2.hip (fp32 and limb-plane
output), conv_l2_fixup_kernel, the activation-stationary kernel's epilogue slices, and the exact-fp32 kernels' conv_epilogue
and conv_fixup_kernel (csrc/conv_common.h, csrc/conv.hip) -- through onda_amd.ops, so this file runs unchanged in a checkout
of any commit that has them.

    ONDA_LIB_PATH=<library> python tests/golden/make_conv_epilogue_bits.py --out first.json             (on the MI355X)
    ONDA_LIB_PATH=<library> python tests/golden/make_conv_epilogue_bits.py --second-of first.json [--out <fixture>]

The first call writes {"torch": ..., "hip": ..., "digests": {name: sha256 of the output's raw bytes}}.  The second, a new
process, records again and writes the fixture: the first record plus "unstable", the keys whose two digests differ.  That list
has to come out EMPTY, and tests/test_conv_epilogue_bits.py asserts that it is: a tile's K-steps, a remainder tile's pieces
(ascending workgroups) and the statistic partials all have a fixed order, and a maximum does not depend on the order.  The
fixture is recorded at a commit whose kernels are trusted (the parent of the change under test, `ONDA_LIB_PATH` selecting a
library built there), never from the code under test.

A max|.| slot buffer is digested as the maximum over all its floats, never as the raw slots (make_norm_bits.py).

Inputs: no shapes of their own.  The schedule edges of tests/conv_fp64.py (_edge_geometries: whole rounds, remainder +
fix-up, 128 x 128 and 256 x 64 balanced, long K, the continuous stream with whole rounds and with a remainder) and the short-K,
partial-column and stride-2 site shapes of tests/test_eval_conv_fp64_parity.py, with seeded inputs.  Every case asserts the
kernel and the schedule it runs on through the library's dispatch queries before it launches (confirm_plan / _schedule of those
files); where an environment switch picks the path (ONDA_L2_STATIONARY, ONDA_CONV_SCHED) the queries are asked under it.  The
exact-fp32 entry point has no dispatch query: its two schedules are chosen by ONDA_CONV_SCHED (1: one tile per workgroup, 2:
hybrid), on shapes whose tile count is no multiple of the resident workgroups, so the hybrid launch has remainder tiles.
"""
import contextlib
import hashlib
import json
import math
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_fp64 as ref  # noqa: E402
import test_eval_conv_fp64_parity as E  # noqa: E402

DEV = "cuda:0"
FIXTURE = os.path.join(HERE, "conv_epilogue_bits.json")
# fp32-output epilogues: (name, statistic rows, scale + shift, residual, ReLU)
FP32_EPILOGUES = [("plain stats2", True, False, False, False), ("plain stats4", 4, False, False, False),
                  ("affine", 0, True, False, False), ("affine+res+relu", 0, True, True, True), ("res alone", 0, False, True, False)]
SHORT_K = ("shortk", 2, 33, 65, 64, 256, 1, 0)            # B, H, W, Cin, Cout, k, pad: M = 4290, a partial last tile row
PARTIAL = [("cols.%d" % c, 1, 19, 37, 128, c, 3, 1) for c in (160, 96)]  # M = 703
STRIDE2 = (2, 33, 65, 256, 512)                           # layer2.0.ds at the sites' size: B, Hi, Wi, Cin, Cout; M = 1122


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def toolchain():
    return {"torch": str(torch.__version__), "hip": str(torch.version.hip)}


def amax_sha(slot):
    return "none" if slot is None else sha(slot.max())


@contextlib.contextmanager
def switches(**env):
    """Environment switches the library reads per call, for the launches (and the dispatch queries) inside."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def operands(seed, B, H, W, cin, cout, k):
    g = E._gen(seed)
    x = E._randn((B, H, W, cin), g)
    w = E._randn((cout, cin, k, k), g, 1.0 / math.sqrt(cin * k * k))
    sc, sh = E._affine(cout, g)
    res = E._randn((B, H, W, cout), g, 3.0)
    return x, w, sc, sh, res


def fp32_out_digests(d, name, ops_in, k, dil, pad, epilogues=FP32_EPILOGUES):
    """ops.conv_forward with fp32 output, one launch per epilogue: y, the statistic partials (every row the launch wrote,
    the fix-up's extra rows and their identities included) and the maximum it left."""
    from onda_amd import ops
    x, w, sc, sh, res = ops_in
    cout = w.shape[0]
    wp = ops.pack_weight_fwd(w)
    for ename, stats, affine, with_res, relu in epilogues:
        out = residual = None
        if with_res and not affine:  # the gradient sink: the running sum is the residual and is stored over
            out = residual = res.clone()
        elif with_res:
            residual = res
        y, st, _ = ops.conv_forward(x, wp, k, 1, dil, pad, cout, out=out, scale=sc if affine else None,
                                    shift=sh if affine else None, residual=residual, relu=relu, want_stats=stats)
        d[f"{name} | {ename} | y"] = sha(y)
        d[f"{name} | {ename} | amax"] = amax_sha(ops.known_amax(y))
        if stats:
            assert st is not None and st.shape[1] == (4 if stats == 4 else 2)
            d[f"{name} | {ename} | stats"] = sha(st)


def edges_fp32(d):
    for i, (label, geo, kid, balanced, rem) in enumerate(ref._edge_geometries()):
        name, H, W, cin, cout, k, _stride, dil, pad = geo[:9]
        E.confirm_plan(label, H * W, cout, k * k, cin, kid, balanced, rem)
        bal = ref._schedule(H * W, cout, k * k, cin)[1]
        fp32_out_digests(d, f"f16x2 {name} kernel {kid}{' fixup' if bal else ''}", operands(400 + i, 1, H, W, cin, cout, k), k, dil, pad)


def short_k_and_partial_fp32(d):
    name, B, H, W, cin, cout, k, pad = SHORT_K
    E.confirm_plan(name, B * H * W, cout, 1, cin, kid=1, balanced=False)
    ops_in = operands(410, B, H, W, cin, cout, k)
    fp32_out_digests(d, f"f16x2 {name} kernel 1", ops_in, k, 1, pad)
    with switches(ONDA_L2_STATIONARY=1):  # the activation-stationary kernel takes the plain epilogue only
        from onda_amd._lib import query
        kid, rows = query("onda_conv_l2_kernel_id", B * H * W, cout, 1, cin), query("onda_conv_l2_tiles_m", B * H * W, cout, 1, cin)
        assert kid == 4 and rows == -(-B * H * W // 128), (kid, rows)  # (128-row statistic tiles, no stream-K remainder)
        fp32_out_digests(d, f"f16x2 {name} kernel 4", ops_in, k, 1, pad, FP32_EPILOGUES[:2])
    for name, B, H, W, cin, cout, k, pad in PARTIAL:
        E.confirm_plan(name, B * H * W, cout, k * k, cin, kid=1)
        bal = ref._schedule(B * H * W, cout, k * k, cin)[1]
        fp32_out_digests(d, f"f16x2 {name} kernel 1{' fixup' if bal else ''}", operands(420 + cout, B, H, W, cin, cout, k), k, 1, pad)


def stride2_dgrad(d):
    """The scattered store (out_os = 2): the data gradient of a stride-2 1 x 1 conv, a GEMM of M = B * Ho * Wo rows, Cin
    columns and K = Cout, through a tile epilogue (ONDA_CONV_SCHED=1) and through the fix-up (2)."""
    from onda_amd import ops
    B, Hi, Wi, cin, cout = STRIDE2
    Ho, Wo = ref.out_size(Hi, 1, 2, 1, 0), ref.out_size(Wi, 1, 2, 1, 0)
    g = E._gen(430)
    dy = E._randn((B, Ho, Wo, cout), g)
    wpd = ops.pack_weight_dgrad(E._randn((cout, cin, 1, 1), g, 1.0 / math.sqrt(cin)))
    for sched, want_bal in ((1, False), (2, True)):
        with switches(ONDA_CONV_SCHED=sched):
            kid, bal = ref._schedule(B * Ho * Wo, cin, 1, cout)[:2]
            assert kid == 1 and bal == want_bal, (sched, kid, bal)
            amax = ops.amax_slot(DEV)
            dx = ops.conv_dgrad(dy, wpd, 1, 2, 1, 0, cin, (Hi, Wi), yamax=amax)
        tag = f"f16x2 stride-2 dgrad kernel 1{' fixup' if bal else ''}"
        d[f"{tag} | dx"], d[f"{tag} | amax"] = sha(dx), amax_sha(amax)


def edges_limbs(d):
    """test_every_kernel_path_writes_limb_planes_against_fp64's launches: both planes, `ybound` and the true maximum."""
    from onda_amd import ops
    for i, (label, geo, kid, balanced, rem) in enumerate(ref._edge_geometries()):
        name, H, W, cin, cout, k, stride, dil, pad = geo[:9]
        E.confirm_plan(label, H * W, cout, k * k, cin, kid, balanced, rem)
        bal = ref._schedule(H * W, cout, k * k, cin)[1]
        x, w, sc, sh, _ = operands(440 + i, 1, H, W, cin, cout, k)
        ops.activation_limbs(x)
        res = E.loose_planes((1, H, W, cout), E._gen(1440 + i))
        for ename, with_res, relu in E.EPILOGUES:
            y = E._limb_conv(x, w, sc, sh, k, stride, dil, pad, res if with_res else None, relu)
            lb = ops.limbs_of(y)
            tag = f"limbs {name} kernel {kid}{' fixup' if bal else ''} | {ename}"
            d[f"{tag} | planes"], d[f"{tag} | ybound"], d[f"{tag} | true max"] = sha(lb.planes), amax_sha(lb.amax), amax_sha(lb.true_amax)


def f32_mode(d):
    """conv_epilogue and conv_fixup_kernel (ONDA_CONV_MODE f32): 128 x 128 tiles with the piece-sum launch in front of the
    fix-up (few remainder tiles) and 128 x 64 tiles without it."""
    G = ref._G()
    cases = [PARTIAL[0], ("e.256x64.sk", 1, 100, 256, 256, 64, 3, 1)]
    for name, B, H, W, cin, cout, k, pad in cases:
        tiles = -(-B * H * W // 128) * -(-cout // (128 if cout > 64 else 64))
        assert tiles % G != 0 and (tiles * 4 < G) == (name == PARTIAL[0][0]), (name, tiles, G)
        ops_in = operands(450 + cout, B, H, W, cin, cout, k)
        for sched in (1, 2):
            with switches(ONDA_CONV_SCHED=sched):
                fp32_out_digests(d, f"f32 {name}{' fixup' if sched == 2 else ''}", ops_in, k, 1, pad,
                                 [FP32_EPILOGUES[0], FP32_EPILOGUES[3]])
        # no query names the path here: a remainder tile is the sum of its pieces, rounded piece by piece, so the hybrid launch's
        # output differs in its last bits from the whole tile's -- equal digests would mean the switch did not take
        for ename in (FP32_EPILOGUES[0][0], FP32_EPILOGUES[3][0]):
            assert d[f"f32 {name} | {ename} | y"] != d[f"f32 {name} fixup | {ename} | y"], (name, ename)


def digests():
    from onda_amd import ops
    d = {}
    old = ops.CONV_MODE
    try:
        with torch.no_grad():
            ops.CONV_MODE = "f16x2"
            edges_fp32(d)
            short_k_and_partial_fp32(d)
            stride2_dgrad(d)
            edges_limbs(d)
            ops.CONV_MODE = "f32"
            f32_mode(d)
    finally:
        ops.CONV_MODE = old
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return d


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    t0 = time.time()
    rec = dict(toolchain(), digests=digests())
    seconds = time.time() - t0
    if "--second-of" in sys.argv:
        with open(sys.argv[sys.argv.index("--second-of") + 1]) as f:
            first = json.load(f)
        assert sorted(first["digests"]) == sorted(rec["digests"]) and toolchain() == {k: first[k] for k in ("torch", "hip")}
        rec["unstable"] = sorted(k for k in rec["digests"] if rec["digests"][k] != first["digests"][k])
        assert not rec["unstable"], f"outputs differ between two runs of one library: {rec['unstable']}"
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec['digests'])} digests in {seconds:.1f} s, {len(rec.get('unstable', []))} unstable -> {path} "
          f"(torch {rec['torch']}, hip {rec['hip']})")
