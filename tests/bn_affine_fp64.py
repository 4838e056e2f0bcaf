"""fp64 restatement of the AFFINE gradients of a train-mode BatchNorm -- dgamma / dbeta of one BatchNorm over one or two row
groups, and of the pair of a shortcut block -- with the comparators that hold csrc/norm.hip (onda_bn_bwd_affine), csrc/norm_l2.hip
(onda_bn_bwd_affine_l2, onda_bn_pair_bwd_affine_l2) and ops/norm.py to it.  A plain module in the style of norm_fp64.py, whose
forward restatement (``bn64``), statistics bounds (``bn_stat_tol``) and ``_hold`` it uses: tests/test_bn_affine_reference.py
validates it on the CPU, tests/test_bn_affine_parity.py runs the kernels through it on the GPU.

Restatement (float64, plain sums).  g = dout * mask -- the mask is an ARGUMENT, [out > 0] of the code under test, as in
``norm_fp64.bn_bwd64``.  One BatchNorm:  dbeta[c] = sum over ALL rows of g,  dgamma[c] = sum of g * xhat, xhat taken from the
statistics of the row's OWN group (``ref.xhat``); two row groups contribute group 0's sum plus group 1's.  The pair
out = relu(BN_a + BN_b) hands the same g to both: dbeta_a = dbeta_b = sum g, dgamma_a = sum g * xhat_a, dgamma_b = sum g * xhat_b.

Comparators: per channel, a channel's error against that channel's OWN bound (``norm_fp64._hold``), never one max-norm.

BOUNDS.  u = 2^-24.  The kernels form both sums as the data gradient's: fp32 chunk partials (one chain of L dependent additions
per partial, P partials per row group), the partials combined in double, the groups' doubles added, ONE rounding to fp32.
With rho_k = sqrt((L_k + 1) / P_k) of row group k (norm_fp64's count of a chain: L additions + the rounding of the product
g * xhat; P partials of about equal weight average independent errors) and S_k(.) the group's sum of magnitudes:

    |d dbeta|  <= u * (sum_k rho_k * S_k|g|      +     S|g|)          (+ 1: the final rounding, on |dbeta| <= S|g|)
    |d dgamma| <= u * (sum_k (rho_k + C_XHAT) * S_k|g xhat| + S|g xhat|)   +   sum_k e_xhat[k] * S_k|g|

C_XHAT = 2: xhat = (x - mean) * invstd is two fp32 roundings per element before the product (they do not average: the bound
takes them in full).  e_xhat[k] is the propagated STATISTICS term norm_fp64.bn_stat_tol already derives (max|xhat| * t_invstd +
invstd * t_mean, its own 4 x inside): the device's xhat is built from the device's mean / invstd.  The geometry (L, P) is read
from the code: csrc/norm_l2.hip col_plan3 -- the same rule as norm.hip's col_plan with B = 1, planned over ALL M rows, a chunk never
across the group boundary: L = ceil(min(rows_per_chunk, n) / ry) + ry - 1, P = ceil(n / rows_per_chunk) for a group of n rows
(``limb_geometry``) -- and csrc/norm.hip col_plan over each group's own rows for the fp32 route (``norm_fp64.bn_geometry``).
A tolerance is MARGIN = 4 x the larger of the derived constant and FLOOR, plus the statistics term.
FLOOR: what fp32 torch on the CPU (F.batch_norm under autograd) is off by against the restatement, in units of u * S|g| (dbeta)
and u * S|g xhat| (dgamma), over the channels with kappa = 1 + mean^2 / (var + eps) <= norm_fp64.FLOOR_KAPPA of every case of
norm_fp64.BN_CASES with more than one row; measured by test_bn_affine_reference.py::test_floor_is_what_torch_is_off_by and
recorded rounded up.  No tolerance is tuned to what the kernels reach.
"""
import collections

import torch

import norm_fp64 as N

U = N.U
MARGIN = 4.0
C_XHAT = 2.0

# fp32 torch on the CPU against the restatement (see above); measured / recorded is held to [0.75, 1.25]
FLOOR = {
    "dbeta": 1.8,     # per channel, / (u * sum |g|)
    "dgamma": 3.1,    # per channel, / (u * sum |g xhat|); more than one row
}

AffineRef = collections.namedtuple("AffineRef", "g dgamma dbeta a_g a_gx")


def affine64(ref, dout, mask=None, g=None):
    """ref: norm_fp64.BNRef (its groups and xhat).  mask [M, C] bool or None.  dgamma, dbeta [C]; a_g, a_gx [G, C]: each row
    group's sum of |g| and of |g * xhat|.  `g`: the masked gradient itself, when the caller already has it (the pair)."""
    if g is None:
        g = dout.double() * (mask.double() if mask is not None else 1.0)
    gx = g * ref.xhat
    a_g = torch.stack([g[r0:r0 + n].abs().sum(0) for r0, n in ref.groups])
    a_gx = torch.stack([gx[r0:r0 + n].abs().sum(0) for r0, n in ref.groups])
    # group 0's sum plus group 1's, as the kernels add them (in double the order is far below every bound here)
    dbeta = sum(g[r0:r0 + n].sum(0) for r0, n in ref.groups)
    dgamma = sum(gx[r0:r0 + n].sum(0) for r0, n in ref.groups)
    return AffineRef(g, dgamma, dbeta, a_g, a_gx)


def pair_affine64(ref_a, ref_b, dout, mask=None):
    """The pair: one g for both sides.  Returns (AffineRef of side a, AffineRef of side b); their dbeta are the same tensor."""
    a = affine64(ref_a, dout, mask)
    return a, affine64(ref_b, dout, mask, g=a.g)


def limb_geometry(M, C, split=0):
    """[(L, P)] per row group of bn_bwd_reduce_l2_kernel / bn_bwd_reduce_pair_l2_kernel: col_plan3 over all M rows, the chunks of
    a group counted from its own first row."""
    p = N.col_plan(1, M, C)
    return [(-(-min(p.rows_per_chunk, n) // p.ry) + p.ry - 1, -(-n // p.rows_per_chunk)) for n in ((split, M - split) if split else (M,))]


def fp32_geometry(M, C, split=0):
    """[(L, P)] per row group of onda_bn_bwd_affine: one colreduce per group, planned over that group's rows."""
    return [N.bn_geometry(n, C) for n in ((split, M - split) if split else (M,))]


def affine_tol(ref, aref, geometry, bwd_geometry):
    """(tol_dgamma, tol_dbeta), each [C].  geometry: the (L, P) of the forward statistics per row group (norm_fp64.bn_stat_tol),
    bwd_geometry: those of the backward reduction."""
    _, _, e_xhat = N.bn_stat_tol(ref, geometry)
    tol_db, tol_dg = torch.zeros_like(aref.dbeta), torch.zeros_like(aref.dgamma)
    for k, (L, P) in enumerate(bwd_geometry):
        rho = ((L + 1) / P) ** 0.5  # (+ 1.0 below: the final rounding, each group's share of S|.|)
        tol_db = tol_db + MARGIN * max(rho + 1.0, FLOOR["dbeta"]) * U * aref.a_g[k]
        tol_dg = tol_dg + MARGIN * max(rho + 1.0 + C_XHAT, FLOOR["dgamma"]) * U * aref.a_gx[k] + e_xhat[k] * aref.a_g[k]
    return tol_dg, tol_db


def check_affine(dgamma, dbeta, aref, ref, geometry, bwd_geometry, where, what=""):
    """dgamma / dbeta [C] of the code under test (either may be None: not asked for), per channel against its own bound."""
    tol_dg, tol_db = affine_tol(ref, aref, geometry, bwd_geometry)
    if dbeta is not None:
        N._hold(f"bn dbeta{what}", (dbeta.double() - aref.dbeta).abs(), tol_db, where)
    if dgamma is not None:
        N._hold(f"bn dgamma{what}", (dgamma.double() - aref.dgamma).abs(), tol_dg, where)
