"""GPU: the prototype kernels of csrc/loss_proto.hip, through prototype_handler, against the float64 restatement of
tests/proto_fp64.py under the bounds derived there -- sigma, the one-pass assignment (labels, soft map, monitor means) with the
MFMA kernel and its list pass, the distance-matrix entry point, the class sums, the EMA and the running append -- on the case
table of that module: N below one 32-pixel block, a second trip of the MFMA kernel's grid-stride loop, three trips of the list
pass, prototypes and features with a common channel offset, tau off 1, no prior, K in {1, 2, 32}, padded and copied layouts.
tests/test_proto_fp64_reference.py validates the same comparators on the CPU.  Every test prints its figures before it asserts."""
import pytest
import torch

import proto_fp64 as P
from onda_amd import ops
from onda_amd._lib import call, query
from onda_amd.framework.domain_adaptation.methods import prototype_handler as PH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAM = 0.9995
ids = lambda c: c.id  # noqa: E731


def handler(st, case=None):
    h = PH.prototype_handler(LAM, *((case.tau, case.thresh, case.metric) if case else (1, 0.3, "mahalanobis")))
    if st is not None:
        h.prototypes, h.squared_mean, h.counter = (t.clone().to(DEV) for t in st)
    return h


def on_device(case):
    x = P.inputs(case)
    return x, P.nchw(case, x.rows, DEV, 288), P.nchw(case, x.prior, DEV, 32)


def assign(case):
    """(labels, soft, means, sigma f32 on the CPU or None, shapes and one-pass service as expected) of one pass, from a fresh
    handler.  Asserts nothing: the callers print their figures first."""
    x, feat, prior = on_device(case)
    h = handler(x.state, case)
    sigma = h.global_var().cpu() if case.metric == "mahalanobis" else None
    labels, soft, means = h.assign_stats(feat, prior)
    shaped = labels.shape == (case.N, 1) and labels.dtype == torch.int64 and soft.shape == (case.N, case.K)
    # pseudo_labels is served from the same pass
    served = h.pseudo_labels(feat, prior) is labels and h.pseudo_labels(feat, prior, soft=True) is soft
    return labels, soft, means, sigma, shaped and served


@pytest.mark.parametrize("case", P.CASES, ids=ids)
def test_assign_against_fp64(case):
    x, feat, prior = on_device(case)
    rows, pitch = PH._rows(feat)[:2]
    in_place, prior_pitch = rows is feat, PH._rows(prior)[1] if prior is not None else 0
    labels, soft, means, sigma, as_expected = assign(case)
    print(f"{case.id}: layout {case.layout}, features read in place {in_place} at a pitch of {pitch}, prior at {prior_pitch}")
    if sigma is not None:
        P.check_sigma(sigma, x.state, case.id)
    P.check_assign(labels, soft, means, P.reference_with(case, sigma), case.tau, case.id)
    h = handler(x.state, case)
    dist = h.distance_measure(feat)
    P.check_distances(dist, x.rows, x.state[0], sigma, case.metric, case.id)
    named = h.mahalanobis_distance(feat) if case.metric == "mahalanobis" else h.distance(feat)
    assert as_expected and torch.equal(named, dist)
    if case.layout == "padded":  # read in place, at the buffer's pitch
        assert in_place and pitch == 288 and prior_pitch == 32
    elif case.layout == "nchw":
        assert not in_place and pitch == P.C
    else:
        assert in_place and pitch == P.C


# onda_proto_assign's workspace (the comment above PA_GRID in csrc/loss_proto.hip): 3 floats for each of the 256 + 256 workgroups
# of the MFMA and the list pass, the list of flagged pixels (N ints), its length (one int)
WS_PARTIALS = 3 * 512


def raw_assign(case, x, sigma):
    """onda_proto_assign itself on 2-D inputs: (labels, soft, number of pixels the MFMA kernel put on the list)."""
    N, K = case.N, case.K
    feat, proto = x.rows.to(DEV), x.state[0].to(DEV)
    prior = x.prior.to(DEV) if x.prior is not None else None
    sg = sigma.to(DEV) if sigma is not None else None
    labels = torch.empty(N, 1, device=DEV, dtype=torch.int64)
    soft = torch.empty(N, K, device=DEV)
    result = torch.empty(3, device=DEV)
    ws = torch.zeros(3 * query("onda_proto_assign_blocks", N), device=DEV)
    p = ops._p
    call("onda_proto_assign", p(feat), P.C, p(prior), K if prior is not None else 0, p(proto), p(sg), int(sigma is not None),
         float(case.tau), float(case.thresh), p(labels), p(soft), p(result), p(ws), N, P.C, K, ops._stream())
    torch.cuda.synchronize()
    return labels, soft, int(ws.view(torch.int32)[WS_PARTIALS + N]) if ws.numel() > WS_PARTIALS + N else -1


def test_every_pixel_on_the_list():
    """Classes 3 and 7 are one prototype: the two largest posteriors of every pixel are bit-equal, so the MFMA kernel flags all
    2 085 pixels and the list pass takes three trips of its 1 024-pixel grid; the first maximum decides.  The list's length is
    read from the workspace of a direct call, for this case and for one whose list is short."""
    case = P.LIST_CASE
    labels, soft, means, sigma, as_expected = assign(case)
    ref = P.reference_with(case, sigma)
    P.check_twin(labels, soft, means, ref, case.tau, case.id)
    raw_labels, raw_soft, listed = raw_assign(case, P.inputs(case), sigma)
    other = P.BY_ID["off8-maha"]
    o_labels, o_soft, o_means, o_sigma, _ = assign(other)
    _, o_raw_soft, o_listed = raw_assign(other, P.inputs(other), o_sigma)
    print(f"list: {listed} of {case.N} pixels on the list ({-(-listed // 1024)} trips of the list pass), class 3 and 7 bit-equal "
          f"{torch.equal(soft[:, 3], soft[:, 7])}; {other.id}: {o_listed} of {other.N} on the list")
    assert as_expected and torch.equal(soft[:, 3], soft[:, 7])
    assert listed == case.N and torch.equal(raw_labels, labels) and torch.equal(raw_soft, soft)
    assert 0 < o_listed < other.N // 20 and torch.equal(o_raw_soft, o_soft)


def test_labels_and_soft_map_repeat_bit_for_bit():
    """Two passes over `second-trip`: labels and the soft map are decided per pixel and are bit-identical.  The three monitor
    means are NOT required to be: the list pass adds its pixels in list order, and atomicAdd fills the list in arrival order;
    each run's means are held to S against float64 instead."""
    case = P.BY_ID["second-trip"]
    a, b = assign(case), assign(case)
    ref = P.reference_with(case, a[3])
    errs = [float((torch.tensor(r[2], dtype=torch.float64) - ref.means).abs().max()) for r in (a, b)]
    same = [torch.equal(a[i], b[i]) for i in (0, 1)]
    print(f"labels equal {same[0]}, soft map equal {same[1]}, means {a[2]} / {b[2]}, off fp64 by {errs[0]:.3e} / {errs[1]:.3e} "
          f"(S = {P.S(case.tau):.3e})")
    assert all(same) and torch.equal(a[3], b[3])
    assert max(errs) <= P.S(case.tau)


def test_assign_guards():
    """Shapes the kernels do not take are refused before any launch; so is a sigma off the 16-byte boundary both assign kernels
    load it across."""
    N, K = 33, 19
    feat = torch.zeros(N, 260, device=DEV)
    proto = torch.zeros(33, P.C, device=DEV)
    base = torch.ones(P.C + 4, device=DEV)
    labels = torch.full((N, 1), -7, device=DEV, dtype=torch.int64)
    soft = torch.full((N, 33), -7.0, device=DEV)
    result = torch.zeros(3, device=DEV)
    ws = torch.zeros(3 * query("onda_proto_assign_blocks", N), device=DEV)
    p = ops._p

    def run(K=K, C=P.C, ldf=260, sigma=base[:P.C]):
        try:
            call("onda_proto_assign", p(feat), ldf, None, 0, p(proto), p(sigma), 1, 1.0, 0.3, p(labels), p(soft), p(result), p(ws), N, C,
                 K, ops._stream())
        except RuntimeError as e:
            return str(e)
        return "accepted"

    aligned = (base.data_ptr() % 16, base[1:].data_ptr() % 16)
    refused = {name: run(**kw) for name, kw in (("K = 0", dict(K=0)), ("K = 33", dict(K=33)), ("C = 128", dict(C=128)),
                                                ("ldf = 258", dict(ldf=258)), ("sigma + 4 bytes", dict(sigma=base[1:P.C + 1])))}
    torch.cuda.synchronize()
    untouched = bool((labels == -7).all()) and bool((soft == -7.0).all())
    accepted = run()  # the same buffers, aligned
    torch.cuda.synchronize()
    print(f"guards: {refused}; outputs untouched by the refused calls {untouched}; aligned call: {accepted}; sigma offsets {aligned}")
    assert aligned == (0, 4) and untouched
    assert all("ONDA_EINVAL" in refused[k] for k in ("K = 0", "K = 33", "C = 128", "ldf = 258"))
    assert "ONDA_EALIGN" in refused["sigma + 4 bytes"]
    assert accepted == "accepted" and bool((labels != -7).all())


# ------------------------------------------------------------------------------------------------ class sums, EMA, append
def split(flat, K):
    return flat[: K * P.C].reshape(K, P.C), flat[K * P.C: 2 * K * P.C].reshape(K, P.C), flat[2 * K * P.C:]


@pytest.mark.parametrize("sc", P.SUMS_CASES, ids=ids)
def test_class_sums_against_fp64(sc):
    rows, out, cls = P.sums_inputs(sc)
    K = P.SUMS_K
    feat = P.nchw(sc, rows, DEV, 288)
    h = handler(None)
    if sc.classes:
        flat, k_, c_ = h.class_statistics(feat, K, classes=cls.to(DEV))
    elif sc.layout == "padded":  # NCHW logits: the argmax comes from the softmax-statistics kernel
        assert PH._rows(feat)[1] == 288
        flat, k_, c_ = h.class_statistics(feat, out.reshape(*P.SHAPE, K).permute(0, 3, 1, 2).contiguous().to(DEV))
    else:
        flat, k_, c_ = h.class_statistics(feat, out.to(DEV))
    assert (k_, c_) == (K, P.C) and flat.shape == (2 * K * P.C + K,)
    P.check_class_sums(*split(flat, K), rows, cls, K, sc.id)


def test_ema_and_append_against_fp64():
    """`ma` on a batch without classes 4 and 11 (their rows stay bit-identical), `append` from the empty state on a batch without
    class 5, then a batch in which it first appears; the references start from the fp32 class sums of the kernels themselves."""
    st, ((ra, oa), (rb, ob), (rc, oc)) = P.update_inputs()
    K = P.SUMS_K
    h = handler(st)
    s, s2, n = (t.cpu() for t in split(h.class_statistics(ra.to(DEV), oa.to(DEV))[0], K))
    P.check_class_sums(s, s2, n, ra, oa.argmax(1), K, "ema batch")
    assert n[4] == 0 and n[11] == 0
    h.ma(ra.to(DEV), oa.to(DEV))
    r_proto, r_sq, w_proto, w_sq = P.ema64(st, s, s2, n, LAM)
    P.check_weighted(h.prototypes, r_proto, w_proto, P.R_EMA, "ema proto")
    P.check_weighted(h.squared_mean, r_sq, w_sq, P.R_EMA, "ema sqmean")
    for k in (4, 11):
        assert torch.equal(h.prototypes[k].cpu(), st[0][k]) and torch.equal(h.squared_mean[k].cpu(), st[1][k])
    assert torch.equal(h.counter.cpu(), st[2])
    h2, before = handler(None), None
    for name, rows, out in (("append 1", rb, ob), ("append 2", rc, oc)):
        s, s2, n = (t.cpu() for t in split(h2.class_statistics(rows.to(DEV), out.to(DEV))[0], K))
        P.check_class_sums(s, s2, n, rows, out.argmax(1), K, name)
        assert (n[5] == 0) == (before is None)
        h2.append(rows.to(DEV), out.to(DEV))
        r = P.append64(before, s, s2, n)
        P.check_weighted(h2.prototypes, r[0], r[3], P.R_APPEND, name + " proto")
        P.check_weighted(h2.squared_mean, r[1], r[4], P.R_APPEND, name + " sqmean")
        assert torch.equal(h2.counter.cpu().double(), r[2])
        if before is None:
            assert bool((h2.prototypes[5] == 0).all()) and bool((h2.squared_mean[5] == 0).all())
        before = tuple(t.cpu().clone() for t in (h2.prototypes, h2.squared_mean, h2.counter))
