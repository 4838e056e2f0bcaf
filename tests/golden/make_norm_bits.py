"""Digests of everything the kernels of csrc/norm.hip put out -- fp32 BatchNorm (statistics partials, finalize with the running
buffers, apply, backward), the folded eval BatchNorm, the ASPP head's GroupNorm + concat, GroupNorm on a backbone convolution and
the column sums -- through onda_amd.ops and, for the backbone sites, the C ABI as tests/test_gn_site_parity.py drives it, so this
file runs unchanged in a checkout of any commit that has them.

    ONDA_LIB_PATH=<library> python tests/golden/make_norm_bits.py --out first.json                      (on the MI355X)
    ONDA_LIB_PATH=<library> python tests/golden/make_norm_bits.py --second-of first.json [--out tests/golden/norm_bits.json]

The first call writes {"torch": ..., "hip": ..., "digests": {name: sha256 of the output's raw bytes}}.  The second, a new
process, records again and writes the fixture: the first record plus "unstable", the keys whose two digests differ.  That list
has to come out EMPTY, and tests/test_norm_bits.py asserts that it is: every reduction of the file has a fixed order (block
partials by the launch grid, the partials combined in double by a fixed lane stride and a fixed order of the wave sums), and a
maximum does not depend on the order.  The fixture is recorded at a commit whose kernels are trusted (the parent of the change
under test, `ONDA_LIB_PATH` selecting a library built there), never from the code under test.

What a max|.| slot buffer holds is digested as the maximum over all its ONDA_AMAX_FLOATS floats, never as the raw slots: which
slot a workgroup or a wave folds its maximum into is the kernels' own business.  A tensor whose producer left no maximum where
the mode asks for one is recorded as "untagged" (none at the time of recording).

Inputs: no shapes of their own.  The case tables of tests/norm_fp64.py (BN_CASES, RG_CASES, GN_CASES) and tests/gn_site_fp64.py
(SITE_CASES) with their seeded inputs, each in ONDA_CONV_MODE "f32" (no maxima) and "f16x2" (maxima left behind): ragged chunks,
second trips of the finalize lanes and of the element-wise grid, 2 / 4 / 8 / 64 channels per group, HW = 1, several images, the
per-(image, channel) multiplier, strided `out` / `dout`.  The backbone sites take their statistics from the reduction pass and
from hand-made [tile][2][C] and [tile][4][C] partial tables (tiles of one row, and of seven where HW allows), with and without
dgamma / dbeta, and with the launch predicate off over pre-filled outputs.
"""
import ctypes
import hashlib
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import gn_site_fp64 as S  # noqa: E402
import norm_fp64 as N  # noqa: E402

DEV = "cuda:0"
FIXTURE = os.path.join(HERE, "norm_bits.json")
MODES = ("f32", "f16x2")
COLSUM_CASES = ("c256-n5-b3", "c128-n1-relu")
FOLD_CASE = "c24-m306"
SENTINEL = 7.0
UNTAGGED = [0]


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def toolchain():
    return {"torch": str(torch.__version__), "hip": str(torch.version.hip)}


def amax_sha(slot, mode):
    """The maximum a producer left for `mode`: over the whole slot buffer."""
    if mode != "f16x2":
        assert slot is None
        return sha(torch.zeros(0))
    if slot is None:
        UNTAGGED[0] += 1
        return "untagged"
    return sha(slot.max())


# ------------------------------------------------------------------------------------------------ BatchNorm
def bn_stats(xd, M, C):
    from onda_amd import ops
    from onda_amd._lib import call, query
    parts = torch.empty(query("onda_bn_bwd_ws", M, C), device=DEV)
    tiles = ctypes.c_int(0)
    call("onda_bn_stats", xd.data_ptr(), M, C, C, parts.data_ptr(), ctypes.byref(tiles), ops._stream())
    return parts[: tiles.value * 2 * C].reshape(tiles.value, 2, C)


def bn_digests(d, name, mode, inputs, shape, relu, track, first=0, tile_rows=0):
    """ops.BNTrainFn as tests/test_norm_fp64_parity.py drives it."""
    from onda_amd import ops
    x, gamma, beta, res, dout, rm, rv = inputs
    xd = x.reshape(shape).to(DEV).requires_grad_(True)
    rd = res.reshape(shape).to(DEV).requires_grad_(True) if res is not None else None
    stats = bn_stats(xd, xd.numel() // shape[3], shape[3])
    d[f"bn partials {name}"] = sha(stats)
    if tile_rows:
        stats._onda_tile_rows = tile_rows
    rm_d, rv_d, nbt = rm.to(DEV), rv.to(DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    with ops.row_groups(first):
        out = ops.BNTrainFn.apply(xd, stats, gamma.to(DEV), beta.to(DEV), rd, relu, (rm_d, rv_d, nbt) if track else None, N.MOMENTUM)
        saved = out.grad_fn.saved_tensors
        grads = torch.autograd.grad(out, [xd] + ([rd] if rd is not None else []), dout.reshape(shape).to(DEV))
    d[f"bn out {name}"], d[f"bn stats {name}"] = sha(out), sha(saved[2], saved[3])
    d[f"bn running {name}"] = sha(rm_d, rv_d, nbt)
    d[f"bn dx {name}"] = sha(grads[0])
    d[f"bn amax out {name}"], d[f"bn amax dx {name}"] = amax_sha(ops.known_amax(out), mode), amax_sha(ops.known_amax(grads[0]), mode)
    if rd is not None:
        d[f"bn dres {name}"] = sha(grads[1])


def rg_inputs(case):
    """The inputs of test_batchnorm_fp32_path_row_groups."""
    M, C, split = case.B * case.H * case.W, case.C, case.first * case.H * case.W
    seed = N.case_seed(case.id)
    x, gamma, beta = N.bn_input(M, C, seed, shift_rows=split)
    g = torch.Generator().manual_seed(seed + 2)
    res = torch.randn(M, C, generator=g) * 3 if case.res else None
    dout = torch.randn(M, C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    return x, gamma, beta, res, dout, rm, rv


def fold_digests(d):
    from onda_amd import ops
    case = N.BN_BY_ID[FOLD_CASE]
    _, gamma, beta, _, _, rm, rv = N.bn_case_inputs(case)
    d[f"bn fold {case.id}"] = sha(*ops.bn_eval_fold(gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)))


# ------------------------------------------------------------------------------------------------ the head's GroupNorm, colsum
def gn_digests(d, name, mode, case, inputs):
    """ops.GNConcatFn as test_groupnorm_concat drives it."""
    from onda_amd import ops
    xs, gammas, betas, chmul, dcat = inputs
    B, HW, C, n = case.B, case.HW, case.C, case.n
    xd = [x.reshape(B, HW, 1, C).to(DEV).requires_grad_(True) for x in xs]
    gd = [t.to(DEV).requires_grad_(True) for t in gammas]
    bd = [t.to(DEV).requires_grad_(True) for t in betas]
    cat = ops.GNConcatFn.apply(case.relu, chmul.to(DEV) if chmul is not None else None, *xd, *gd, *bd)
    saved = cat.grad_fn.saved_tensors
    grads = torch.autograd.grad(cat, xd + gd + bd, dcat.reshape(B, HW, 1, C * n).to(DEV))
    d[f"gn cat {name}"], d[f"gn amax cat {name}"] = sha(cat), amax_sha(ops.known_amax(cat), mode)
    d[f"gn stats {name}"] = sha(*saved[2 + 2 * n:2 + 4 * n])
    d[f"gn dx {name}"], d[f"gn dgamma {name}"], d[f"gn dbeta {name}"] = sha(*grads[:n]), sha(*grads[n:2 * n]), sha(*grads[2 * n:])


def colsum_digests(d, name, case, inputs):
    from onda_amd import ops
    xs, _, _, _, dcat = inputs
    x = xs[0].reshape(case.B, case.HW, 1, case.C).to(DEV)
    y = dcat.reshape(case.B, case.HW, 1, case.C * case.n).to(DEV)[..., :case.C]  # a strided second operand where n > 1
    for per_image in (False, True):
        d[f"colsum x per_image {int(per_image)} {name}"] = sha(ops.colsum(x, alpha=1.0 / case.HW, per_image=per_image))
        d[f"colsum x*y per_image {int(per_image)} {name}"] = sha(ops.colsum(x, y, per_image=per_image))


# ------------------------------------------------------------------------------------------------ GroupNorm on a backbone conv
def site_tables(x, tile_rows):
    """[tile][2][C] and [tile][4][C] partial tables as a conv epilogue leaves them (sum, sum of squares, min, max)."""
    B, HW, C = x.shape
    t = x.reshape(B * HW // tile_rows, tile_rows, C)
    two = torch.stack([t.sum(1), (t * t).sum(1)], 1).contiguous()
    four = torch.stack([t.sum(1), (t * t).sum(1), t.amin(1), t.amax(1)], 1).contiguous()
    return two, four


def site_fwd(x, stats, tile_rows, gamma, beta, relu, mode, flag=None, fill=None):
    from onda_amd import ops
    from onda_amd._lib import call, query
    p = ops._p
    B, HW, C = x.shape
    new = (lambda *s: torch.full(s, fill, device=DEV)) if fill is not None else (lambda *s: torch.empty(*s, device=DEV))
    out, mean, rstd = new(B, HW, C), new(B * S.GROUPS), new(B * S.GROUPS)
    ws = torch.empty(query("onda_gn_site_ws", B, HW, C), device=DEV)
    amax = ops.amax_slot(DEV) if mode == "f16x2" else None
    call("onda_gn_site_fwd", p(x), p(stats), stats.shape[0] if stats is not None else 0, stats.shape[1] if stats is not None else 0,
         tile_rows if stats is not None else 0, p(gamma), p(beta), p(out), p(mean), p(rstd), p(ws), B, HW, C, S.GROUPS, N.GN_EPS,
         int(relu), p(amax), p(flag), ops._stream())
    return out, mean, rstd, amax


def site_bwd(x, dout, out, mean, rstd, gamma, relu, mode, affine):
    from onda_amd import ops
    from onda_amd._lib import call, query
    p = ops._p
    B, HW, C = x.shape
    dx = torch.empty_like(x)
    dg, db = (torch.empty(C, device=DEV), torch.empty(C, device=DEV)) if affine else (None, None)
    ws = torch.empty(query("onda_gn_site_ws", B, HW, C), device=DEV)
    amax = ops.amax_slot(DEV) if mode == "f16x2" else None
    call("onda_gn_site_bwd", p(dout), p(out), p(x), p(gamma), p(mean), p(rstd), p(dx), p(dg), p(db), p(ws), B, HW, C, S.GROUPS,
         int(relu), p(amax), ops._stream())
    return dx, dg, db, amax


def site_digests(d, name, mode, case, inputs):
    x, gamma, beta, dout = (t.to(DEV) for t in inputs)
    HW = case.H * case.W
    routes = {"reduction": (None, 0)}
    for rows in (1, 7):
        if HW % rows == 0:
            two, four = site_tables(x, rows)
            routes[f"partials2 rows {rows}"], routes[f"partials4 rows {rows}"] = (two, rows), (four, rows)
    for route, (stats, rows) in routes.items():
        out, mean, rstd, amax = site_fwd(x, stats, rows, gamma, beta, case.relu, mode)
        d[f"site out {route} {name}"], d[f"site stats {route} {name}"] = sha(out), sha(mean, rstd)
        d[f"site amax out {route} {name}"] = amax_sha(amax, mode)
        if route not in ("reduction", "partials2 rows 1"):
            continue
        for affine in (True, False):
            dx, dg, db, amax = site_bwd(x, dout, out, mean, rstd, gamma, case.relu, mode, affine)
            tag = f"{route} affine {int(affine)} {name}"
            d[f"site dx {tag}"], d[f"site amax dx {tag}"] = sha(dx), amax_sha(amax, mode)
            if affine:
                d[f"site dgamma dbeta {tag}"] = sha(dg, db)
        for on in (0, 1):  # the launch predicate: off leaves the pre-filled outputs and the maximum alone
            flag = torch.full((1,), on, dtype=torch.int32, device=DEV)
            out, mean, rstd, amax = site_fwd(x, stats, rows, gamma, beta, case.relu, mode, flag, SENTINEL)
            d[f"site predicate {on} {route} {name}"] = sha(out, mean, rstd)
            d[f"site predicate {on} amax {route} {name}"] = amax_sha(amax, mode)


# ------------------------------------------------------------------------------------------------ all of it
def digests():
    from onda_amd import ops
    bn_in = {c.id: N.bn_case_inputs(c) for c in N.BN_CASES}
    rg_in = {c.id: rg_inputs(c) for c in N.RG_CASES}
    gn_in = {c.id: N.gn_case_inputs(c) for c in N.GN_CASES}
    site_in = {c.id: S.site_inputs(c) for c in S.SITE_CASES}
    d = {}
    old = ops.CONV_MODE
    try:
        for mode in MODES:
            ops.CONV_MODE = mode
            for c in N.BN_CASES:
                bn_digests(d, f"{c.id} {mode}", mode, bn_in[c.id], (1, c.M, 1, c.C), c.relu, c.track)
            for c in N.RG_CASES:
                rpc = N.col_plan(1, c.B * c.H * c.W, c.C).rows_per_chunk
                bn_digests(d, f"{c.id} {mode}", mode, rg_in[c.id], (c.B, c.H, c.W, c.C), c.relu, True, c.first, rpc)
            for c in N.GN_CASES:
                gn_digests(d, f"{c.id} {mode}", mode, c, gn_in[c.id])
            for c in S.SITE_CASES:
                site_digests(d, f"{c.id} {mode}", mode, c, site_in[c.id])
    finally:
        ops.CONV_MODE = old
    fold_digests(d)
    for cid in COLSUM_CASES:
        colsum_digests(d, cid, N.GN_BY_ID[cid], gn_in[cid])
    torch.cuda.synchronize()
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
    print(f"{len(rec['digests'])} digests in {seconds:.1f} s, {len(rec.get('unstable', []))} unstable, {UNTAGGED[0]} untagged -> {path} "
          f"(torch {rec['torch']}, hip {rec['hip']})")
