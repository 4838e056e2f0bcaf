"""Planning table of the pre-split conv (csrc/conv_l2.hip l2_plan): what the library's host queries answer for every forward
and data-gradient problem of the timed step, the activation-stationary cases and a handful of schedule edges, under each
environment override.  Without a device the library plans for 256 compute units, the MI355X's own count, so the table is the
same wherever it is made.

    python tests/golden/make_l2_plan.py      (rewrites tests/golden/l2_plan.json; tests/test_l2_plan.py holds the library to it)
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(HERE, "l2_plan.json")

OVERRIDES = ("ONDA_L2_VARIANT", "ONDA_L2_STATIONARY", "ONDA_CONV_SCHED")
# name -> (environment, which stat_split of the problem: None / "image" / "row", plain_schedule)
SETTINGS = {
    "default": ({}, None, 0),
    "variant1_sched1": ({"ONDA_L2_VARIANT": "1", "ONDA_CONV_SCHED": "1"}, None, 0),
    "stationary": ({"ONDA_L2_STATIONARY": "1"}, None, 0),
    "sched2": ({"ONDA_CONV_SCHED": "2"}, None, 0),
    "split_image": ({}, "image", 0),
    "split_row": ({}, "row", 0),
    "plain_schedule": ({}, None, 1),
}
FIELDS = ["kernel_id", "variant", "tiles_m", "tiles_m_split", "tile_rows", "live", "live_stats"]


def _out(n, k, stride, dil, pad):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _fwd(name, B, Hi, Wi, Cin, Cout, k, stride, dil, pad):
    """A forward problem as ops.conv_forward describes it: (name, OndaConv fields)."""
    Ho, Wo = _out(Hi, k, stride, dil, pad), _out(Wi, k, stride, dil, pad)
    return name, dict(B=B, Hi=Hi, Wi=Wi, Cin=Cin, Ho=Ho, Wo=Wo, Cout=Cout, kh=k, kw=k, stride=stride, dil=dil, pad=pad,
                      out_os=1, Hf=Ho, Wf=Wo)


def _dgrad(name, B, Hi, Wi, Cin, Cout, k, stride, dil, pad):
    """The data gradient of that conv as ops.conv_dgrad describes it: a conv of dy (stride 1), or a scattered 1 x 1 (stride 2)."""
    Ho, Wo = _out(Hi, k, stride, dil, pad), _out(Wi, k, stride, dil, pad)
    if stride == 1:
        return name, dict(B=B, Hi=Ho, Wi=Wo, Cin=Cout, Ho=Hi, Wo=Wi, Cout=Cin, kh=k, kw=k, stride=1, dil=dil,
                          pad=dil * (k - 1) - pad, out_os=1, Hf=Hi, Wf=Wi)
    return name, dict(B=B, Hi=Ho, Wi=Wo, Cin=Cout, Ho=Ho, Wo=Wo, Cout=Cin, kh=1, kw=1, stride=1, dil=1, pad=0,
                      out_os=stride, Hf=Hi, Wf=Wi)


def problems():
    """[(name, OndaConv fields)], names unique."""
    from test_conv_fp64_parity import BATCH, STEP_CONVS, _at
    from test_hip_kernels import STATIONARY_CASES
    from onda_amd.ops._state import STEM_K
    out = []
    for size in (1, 2):
        for geo in STEP_CONVS:
            name, Hi, Wi, Cin, Cout, k, stride, dil, pad, _bias, _stats, head, stem, _acc = _at(geo, size)
            for B in (BATCH, 2 * BATCH):
                tag = "%s@%dx%d/b%d" % (name, Hi, Wi, B)
                if stem:  # the patch matrix: a 1 x 1 conv over STEM_K packed values, no data gradient
                    out.append(_fwd("fwd:" + tag, B, _out(Hi, k, stride, dil, pad), _out(Wi, k, stride, dil, pad), STEM_K, Cout, 1, 1, 1, 0))
                    continue
                out.append(_fwd("fwd:" + tag, B, Hi, Wi, Cin, head or Cout, k, stride, dil, pad))
                out.append(_dgrad("dgrad:" + tag, B, Hi, Wi, Cin, head or Cout, k, stride, dil, pad))
    for cin, cout, stride, B, H, W in STATIONARY_CASES:
        out.append(_fwd("stationary:%dx%d/s%d/b%d@%dx%d" % (cin, cout, stride, B, H, W), B, H, W, cin, cout, 1, stride, 1, 0))
    # edges: M = 1, either side of one 256-row tile, and the step's 4 x 65 x 129 rows, at the four tile-column cases
    for H, W in ((1, 1), (15, 17), (16, 16), (1, 257), (65, 129)):
        for cout in (64, 96, 128, 160):
            B = 4 if H == 65 else 1
            out.append(_fwd("edge:M%d/co%d" % (B * H * W, cout), B, H, W, 64, cout, 3, 1, 1, 1))
    # ... and K-steps per tile (taps * Cin / 32) either side of the short-K rule's and the stream kernel's thresholds
    for ksteps, k, cin in ((8, 1, 256), (9, 3, 32), (16, 1, 512), (17, 1, 544), (32, 1, 1024), (33, 1, 1056)):
        for cout in (256, 512, 2048):
            out.append(_fwd("edge:k%d/co%d" % (ksteps, cout), 4, 65, 129, cin, cout, k, 1, 1, k // 2))
    assert len({n for n, _ in out}) == len(out)
    return out


def splits(f):
    """{"image": first row of the second half of the images, "row": a row inside a tile}; 0 = the problem has no such row."""
    M, per_image = f["B"] * f["Ho"] * f["Wo"], f["Ho"] * f["Wo"]
    row = M // 3 + (1 if (M // 3) % 128 == 0 else 0)
    return {None: 0, "image": (f["B"] // 2) * per_image if f["B"] > 1 else 0, "row": row if 0 < row < M else 0}


def record(f, split, plain):
    """What the five host queries answer for one problem under the current environment, in the order of FIELDS."""
    from onda_amd._lib import OndaConv, query
    M, taps = f["B"] * f["Ho"] * f["Wo"], f["kh"] * f["kw"]
    d = OndaConv(**f, stat_split=split, plain_schedule=plain)
    rows = ctypes.c_int(0)
    tiles_split = query("onda_conv_l2_tiles_m_split", M, f["Cout"], taps, f["Cin"], split, plain, ctypes.byref(rows))
    return [query("onda_conv_l2_kernel_id", M, f["Cout"], taps, f["Cin"]), query("onda_conv_l2_variant", M, f["Cout"]),
            query("onda_conv_l2_tiles_m", M, f["Cout"], taps, f["Cin"]), tiles_split, rows.value,
            query("onda_conv_l2_live_fraction", ctypes.byref(d), 0), query("onda_conv_l2_live_fraction", ctypes.byref(d), 1)]


def main():
    table = {}
    saved = {k: os.environ.pop(k, None) for k in OVERRIDES}
    try:
        for setting, (env, which, plain) in SETTINGS.items():
            os.environ.update(env)
            for name, f in problems():
                split = splits(f)[which]
                if which is None or split:
                    table.setdefault(name, {})[setting] = record(f, split, plain)
            for k in env:
                del os.environ[k]
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    with open(PATH, "w") as fh:  # one problem per line, a record as the values of FIELDS
        rows = ",\n".join(json.dumps(n) + ": " + json.dumps(r, separators=(",", ":")) for n, r in table.items())
        fh.write('{"fields": %s, "problems": {\n%s\n}}\n' % (json.dumps(FIELDS), rows))
    print(PATH, len(table), "problems,", sum(len(r) for r in table.values()), "records,", os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
