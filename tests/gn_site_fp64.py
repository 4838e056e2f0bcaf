"""Cases, inputs and injected faults for GroupNorm on a backbone convolution (onda_gn_site_fwd / onda_gn_site_bwd, ops.GNSiteFn:
the stem and the four shortcuts of DeepLabv2-Resnet50-GN), and what the G21 fixture and its tests share.  A plain module like
norm_fp64.py, whose restatement (gn64 / gn_bwd64 with one branch, n = 1) and comparators (check_gn_forward / check_gn_backward,
MARGIN) these tests use unchanged: no constants of their own.

tests/test_gn_site_reference.py runs torch (float64: equality with the restatement; float32: passes the comparators) and the
injected faults on the CPU; tests/test_gn_site_parity.py runs the kernels through the same comparators on the GPU."""
import collections

import torch

import norm_fp64 as N

GROUPS = 32
GN_MODEL = "DeepLabv2-Resnet50-GN"

# ------------------------------------------------------------------------------------------------ G21
SAMPLE = 256      # strided gradient sample of an ordinary parameter
SAMPLE_DS = 4096  # ... of the three larger shortcut weights (and of the float32 run's feat)
FULL = ("conv1.weight", "layer1.0.downsample.0.weight")


def sample_index(numel, n):
    return (torch.arange(n, dtype=torch.int64) * numel) // n


def grad_index(name, numel):
    """Which elements of a parameter's flattened gradient G21 holds: None = all of them."""
    if name in FULL:
        return None
    return sample_index(numel, SAMPLE_DS if name.endswith(".downsample.0.weight") else SAMPLE)


def labels():
    """[2, 9, 17] class labels, one row of 255."""
    g = torch.Generator().manual_seed(21)
    lab = torch.randint(0, 19, (2, 9, 17), generator=g, dtype=torch.int64)
    lab[1, 4, :] = 255
    return lab


# ------------------------------------------------------------------------------------------------ kernel cases
# The smallest at which each thing can break: two channels per group (one 16-byte access spans two groups) with the ReLU,
# centred and at mean / std 16; 8 and 64 channels per group; two chunks of colreduce_kernel per image (col_plan: at least
# ry * 8 = 128 rows a chunk at C = 64, 32 at C >= 256); more than one image everywhere but at C = 2048.
SiteCase = collections.namedtuple("SiteCase", "id C B H W relu ratio")
SITE_CASES = [
    SiteCase("c64-relu", 64, 2, 5, 7, True, None),
    SiteCase("c64-relu-off16", 64, 2, 5, 7, True, N.RATIOS[2]),
    SiteCase("c256", 256, 3, 3, 3, False, None),
    SiteCase("c2048", 2048, 1, 2, 2, False, None),
    SiteCase("c64-chunks2", 64, 2, 3, 43, True, None),
    SiteCase("c256-chunks2", 256, 2, 5, 7, False, None),
]
SITE_BY_ID = {c.id: c for c in SITE_CASES}


def site_inputs(case):
    """(x [B, HW, C], gamma, beta, dout [B, HW, C]) f32, seeded by the case id: the BatchNorm population's gamma / beta and
    per-channel mean / std (norm_fp64.population), so neighbouring channels -- the two of a stem group -- differ in both."""
    seed = N.case_seed(case.id)
    gamma, beta, ratio, std = N.population(case.C, seed)
    std[case.C - 2] = 1.0  # (the constant channel of the BatchNorm population is no special case of a group)
    if case.ratio is not None:
        ratio = torch.full_like(ratio, case.ratio)
    g = torch.Generator().manual_seed(seed + 1)
    HW = case.H * case.W
    x = (torch.randn(case.B, HW, case.C, generator=g).double() + ratio) * std
    x = x * (1.0 + 0.5 * torch.arange(case.B, dtype=torch.float64))[:, None, None]  # every image its own statistics
    dout = torch.randn(case.B, HW, case.C, generator=g)
    return x.float(), gamma, beta, dout


def geometry(case):
    return N.colreduce_geometry(case.B, case.H * case.W, case.C)


# ------------------------------------------------------------------------------------------------ torch, and the faults
def torch_site(x, gamma, beta, dout, relu, dtype, fault=None, groups=GROUPS):
    """torch.native_group_norm under autograd in `dtype`; returns (out, mean, rstd, dx, dgamma, dbeta), [B, HW, C] / [B * groups].
    fault: "pairs" -- groups (1,2),(3,4).. instead of (0,1),(2,3)..; "batch" -- statistics over the batch instead of per
    image; "nomask" -- the backward pass without the ReLU mask."""
    B, HW, C = x.shape
    xt = x.to(dtype).clone().requires_grad_(True)
    gt, bt = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    xin, nb, hw = xt, B, HW
    if fault == "pairs":
        xin = torch.roll(xin, -1, 2)
    if fault == "batch":
        xin, nb, hw = xin.reshape(1, B * HW, C), 1, B * HW
    nchw = xin.permute(0, 2, 1).reshape(nb, C, hw, 1).contiguous()
    xhat, mean, rstd = torch.native_group_norm(nchw, None, None, nb, C, hw, groups, N.GN_EPS)
    xhat = xhat.reshape(nb, C, hw).permute(0, 2, 1).reshape(B, HW, C)
    if fault == "pairs":
        xhat = torch.roll(xhat, 1, 2)
    if fault == "batch":
        mean, rstd = mean.expand(B, groups), rstd.expand(B, groups)
    v = xhat * gt + bt
    out = v.clamp(min=0) if relu else v
    (v if fault == "nomask" else out).backward(dout.to(dtype))
    return (out.detach(), mean.detach().reshape(-1), rstd.detach().reshape(-1), xt.grad, gt.grad, bt.grad)


def hold(got, x, gamma, beta, dout, relu, geo, where, bwd_geo=None, affine=True, groups=GROUPS):
    """(out, mean, rstd, dx, dgamma, dbeta) of the code under test through norm_fp64's comparators; returns the share of elements
    exempt from the ReLU mask check.  affine False: dgamma / dbeta were not asked for (the restatement's own stand in)."""
    out, mean, rstd, dx, dg, db = got
    ref = N.gn64([x], [gamma], [beta], None, relu, groups)
    exempt = N.check_gn_forward(out, [mean], [rstd], ref, geo, where)
    bw = N.gn_bwd64(ref, dout, (out > 0) if relu else None, groups)
    N.check_gn_backward([dx], [dg if affine else bw.dgamma[0]], [db if affine else bw.dbeta[0]], bw, ref, geo, bwd_geo or geo, where)
    return exempt
