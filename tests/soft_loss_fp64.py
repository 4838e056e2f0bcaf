"""float64 restatement of the reference's SOFT_LABELS target loss (loss.py:12-13 CXE, :95-99 soft RCE, func.py:35-42,
prototypes.py:29-39, :305-328) and the cases the fixtures G29 / G30 and their tests share.

    CE  = -sum_k tc_k log(x_k + 1e-6) / N     over the RAW logits x; tc = trunc(t) on the step's path (loss_calc's .long())
    RCE = -sum_k softmax(x)_k log(t_k + 1e-6) / N

`x + 1e-6` and `t + 1e-6` are formed in float32 first, as the reference forms them: the sign of the logarithm's argument and
the pole x + 1e-6 == 0 are then the reference's (in float64 -1e-6f + 1e-6 is 2.5e-14, not 0).  A term whose weight is zero
stays out of the graph, as the reference does not compute it: 0 * NaN would poison the total and the gradient."""
import math

import torch

W_CE, W_RCE, W_REG = 0.1, 1.0, 0.1  # hybrid_switch.yml RCE_ALPHA, RCE_BETA, REGULARIZER_WEIGHT
SMALL = ("mixed", "positive", "saturated", "pole")
SMALL_SHAPE = (2, 19, 9, 17)
HEAD_SEED = 2901
HEAD_SHAPE = (4, 19, 65, 129)
G30_RCE_BETA = 300  # the RCE weight of fixture G30's two steps (tests/golden/make_golden_soft.py says why)


def soft_target(gen, shape, n_onehot, zero_frac=0.0):
    """A distribution per pixel [B,K,h,w]; `n_onehot` pixels hold an exact one-hot (1.0 / 0.0); with `zero_frac`, that share
    of the other entries is exactly 0 (rows renormalised, the largest entry kept)."""
    B, K, h, w = shape
    z = 2.0 * torch.randn(B, K, h, w, generator=gen)
    if zero_frac > 0:
        drop = torch.rand(B, K, h, w, generator=gen) < zero_frac
        drop &= z < z.max(1, keepdim=True).values
        z = z.masked_fill(drop, -math.inf)
    t = z.softmax(1)
    pix = torch.randperm(B * h * w, generator=gen)[:n_onehot]
    cls = torch.randint(0, K, (n_onehot,), generator=gen)
    rows = t.permute(0, 2, 3, 1).reshape(-1, K).clone()
    rows[pix] = 0.0
    rows[pix, cls] = 1.0
    return rows.reshape(B, h, w, K).permute(0, 3, 1, 2).contiguous(), pix, cls


def small_cases():
    """{name: (logits, soft, n_tc0_poles)} of the four small cases.
    mixed: 3*randn logits -- CE is NaN, every gradient finite.  positive: |3*randn| + 0.1 -- CE finite and non-zero.
    saturated: logits at scale 40 against rows with exact zeros.  pole: `positive` with two logits at -1e-6f (x + 1e-6f == 0),
    one under tc = 1 (the hot class of a one-hot pixel) and one under tc = 0 (a pixel that is no one-hot)."""
    gen = torch.Generator().manual_seed(2900)
    out = {}
    for name, scale, zero_frac in (("mixed", 3.0, 0.0), ("positive", 3.0, 0.0), ("saturated", 40.0, 0.3)):
        logits = scale * torch.randn(*SMALL_SHAPE, generator=gen)
        if name == "positive":
            logits = logits.abs() + 0.1
        soft, pix, cls = soft_target(gen, SMALL_SHAPE, 6, zero_frac)
        out[name] = (logits, soft, 0)
        if name == "positive":
            B, K, h, w = SMALL_SHAPE
            rows = logits.permute(0, 2, 3, 1).reshape(-1, K).clone()
            rows[pix[0], cls[0]] = -1e-6                       # under tc = 1
            other = int((pix.max() + 1) % (B * h * w))
            while (pix == other).any():
                other = (other + 1) % (B * h * w)
            rows[other, 3] = -1e-6                             # under tc = 0 (soft value strictly inside (0, 1))
            out["pole"] = (rows.reshape(B, h, w, K).permute(0, 3, 1, 2).contiguous(), soft, 1)
    return {k: out[k] for k in SMALL}


def head_case(seed=HEAD_SEED, shape=HEAD_SHAPE):
    """The head-size case, re-created from its seed: 3*randn logits, 40 one-hot pixels."""
    gen = torch.Generator().manual_seed(int(seed))
    logits = 3.0 * torch.randn(*[int(v) for v in shape], generator=gen)
    soft, _, _ = soft_target(gen, tuple(int(v) for v in shape), 40)
    return logits, soft


def terms(x, soft, ce_trunc):
    """{ce, rce, mrkld, mrent} in float64 of logits x f64[B,K,h,w] (may require grad) and the soft target."""
    B, K, h, w = x.shape
    n = B * h * w
    x32 = x.detach().float()
    u = x + ((x32 + 1e-6).double() - x.detach())  # the float32 value of x + 1e-6, exactly; du/dx = 1
    t = soft.float()
    tc = (t.trunc() if ce_trunc else t).double()
    c = torch.log((t + 1e-6).double())  # (t + 1e-6 in float32, its logarithm in float64)
    lp = x.log_softmax(1)
    p = lp.exp()
    return {"ce": -(tc * torch.log(u)).sum(1).sum() / n, "rce": -(p * c).sum() / n,
            "mrkld": -lp.sum() / (n * K), "mrent": (p * lp).sum() / n}


def total_and_grad(logits, soft, w_ce, w_rce, w_reg, regularizer="MRKLD", ce_trunc=True):
    """(total, d total / d logits, terms) of the weighted sum; a zero weight keeps its term out of the graph."""
    x = logits.double().clone().requires_grad_(True)
    v = terms(x, soft, ce_trunc)
    total = x.sum() * 0.0
    if w_ce != 0:
        total = total + w_ce * v["ce"]
    if w_rce != 0:
        total = total + w_rce * v["rce"]
    if w_reg != 0 and regularizer in ("MRKLD", "MRENT"):
        total = total + w_reg * v[regularizer.lower()]
    grad = torch.autograd.grad(total, x)[0]
    return total.detach(), grad, {k: t.detach() for k, t in v.items()}


# ---- the comparison rules of the G29 tests ---------------------------------------------------------------------------------
def value_close(mine, ref, rtol=1e-5):
    """1e-5 relative; NaN / +inf / -inf matched exactly."""
    mine, ref = float(mine), float(ref)
    if math.isnan(ref):
        return math.isnan(mine)
    if math.isinf(ref):
        return mine == ref
    return math.isfinite(mine) and abs(mine - ref) <= rtol * abs(ref)


def grad_close(mine, ref, rel, what):
    """`rel` of the max-norm over the reference's finite entries; its non-finite ones matched by position and kind."""
    mine, ref = torch.as_tensor(mine).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert mine.shape == ref.shape, what
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(mine), torch.isnan(ref)), f"{what}: NaN positions differ"
    assert torch.equal(mine == math.inf, ref == math.inf) and torch.equal(mine == -math.inf, ref == -math.inf), \
        f"{what}: inf positions differ"
    scale = ref[fin].abs().max().item()
    err = (mine[fin] - ref[fin]).abs().max().item()
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def ce_grad_close(mine, ref, what):
    """The CE gradient on its own, element-wise: rtol 1e-5 where the reference is non-zero, exactly zero elsewhere."""
    mine, ref = torch.as_tensor(mine).double().cpu(), torch.as_tensor(ref).double().cpu()
    zero = ref == 0
    assert (mine[zero] == 0).all(), f"{what}: {int((mine[zero] != 0).sum())} entries where the reference has none"
    fin = torch.isfinite(ref) & ~zero
    assert torch.equal(torch.isnan(mine), torch.isnan(ref)), f"{what}: NaN positions differ"
    assert torch.equal(mine == math.inf, ref == math.inf) and torch.equal(mine == -math.inf, ref == -math.inf), \
        f"{what}: inf positions differ"
    assert ((mine[fin] - ref[fin]).abs() <= 1e-5 * ref[fin].abs()).all(), \
        f"{what}: max rel err {((mine[fin] - ref[fin]).abs() / ref[fin].abs()).max().item():.3e}"
