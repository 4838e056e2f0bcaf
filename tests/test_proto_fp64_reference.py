"""CPU: the float64 restatement and the comparators of tests/proto_fp64.py, validated on the fp32 torch oracle
(oracle/prototypes.py): the oracle passes every check on every case, the floors that BOUNDS record are the ones measured here,
the seeded inputs are two-sided at the threshold and keep clear of ties, and the comparator sees the fault it was built for --
an fp32 restatement of the UNCENTRED expanded distance |g|^2 - 2 g.q + |q|^2 (with the 1e-3 flag rule of the MFMA kernel) fails
the soft-map bound once the channels carry a common offset, the CENTRED one passes everywhere.  The restatements here are
arithmetic in torch, test scaffolding; they share no text with the kernels."""
import functools

import pytest
import torch

import proto_fp64 as P
from oracle import prototypes as op

ALL = P.CASES + [P.LIST_CASE]
ids = lambda c: c.id  # noqa: E731


@functools.lru_cache(maxsize=None)
def oracle(case):
    return P.oracle_assign(case)


# ------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("case", P.CASES, ids=ids)
def test_inputs_are_two_sided_and_clear_of_ties(case):
    ref = P.reference(case)
    labelled, rejected = float((ref.labels != 255).double().mean()), float((ref.labels == 255).double().mean())
    exempt = float((ref.gap <= 2 * P.S(case.tau)).double().mean())
    print(f"{case.id}: labelled {100 * labelled:.1f} %, 255 {100 * rejected:.1f} %, within 2 S of a tie {100 * exempt:.3f} %, "
          f"two-sided {P.two_sided(case)}")
    assert exempt <= P.EXEMPT_SHARE
    if P.two_sided(case):
        assert labelled >= 0.20 and rejected >= 0.05
    elif case.thresh > 0:  # K * thresh <= 1 or no prior to contest the likelihood: nothing can fall under the threshold
        assert case.N < 20 or rejected == 0.0


def test_cases_reach_the_paths_they_are_named_for():
    c = P.BY_ID
    assert (c["second-trip"].N + 31) // 32 > 6 * 256 and (c["tail"].N, c["one"].N, c["short"].N) == (33, 1, 31)
    assert P.LIST_CASE.N > 2 * 1024 and sorted(x.K for x in P.CASES if x.id.startswith("K")) == [1, 2, 32]
    assert {x.tau for x in P.CASES} == set(P.E_REF)


# ------------------------------------------------------------------------------------------------ the oracle under every check
@pytest.mark.parametrize("case", P.CASES, ids=ids)
def test_oracle_assign_passes(case):
    labels, soft, means, sigma = oracle(case)
    P.check_assign(labels, soft, means, P.reference_with(case, sigma), case.tau, f"oracle {case.id}")
    x = P.inputs(case)
    P.check_distances(op.distances(x.rows, x.state, case.metric), x.rows, x.state[0], sigma, case.metric, f"oracle {case.id}")
    if sigma is not None:
        P.check_sigma(sigma, x.state, f"oracle {case.id}")


def test_oracle_decides_the_exact_tie_for_the_first_class():
    case = P.LIST_CASE
    labels, soft, means, sigma = oracle(case)
    assert torch.equal(soft[:, 3], soft[:, 7])
    P.check_twin(labels, soft, means, P.reference_with(case, sigma), case.tau, "oracle list")


def test_oracle_floor_is_what_bounds_record():
    """E_REF, SIGMA_REF and DIST_REF are the oracle's own errors, recorded rounded up.  The oracle is fp32 torch on the CPU and
    its sums follow the host's vector width (sigma: 2.17 on one host, 2.41 on another), so measured / recorded is held to
    [0.75, 1.25], the band tests/test_entropy_reference.py keeps around its floors."""
    e_ref = {tau: (0.0, "") for tau in P.E_REF}
    dist = {m: (0.0, "") for m in P.DIST_REF}
    sig = (0.0, "")
    for case in ALL:
        labels, soft, means, sigma = oracle(case)
        x = P.inputs(case)
        e = P.soft_error(soft, P.reference_with(case, sigma))
        e_ref[case.tau] = max(e_ref[case.tau], (e, case.id))
        d = float((op.distances(x.rows, x.state, case.metric).double() - P.distances64(x.rows, x.state[0], sigma)).abs().max())
        dist[case.metric] = max(dist[case.metric], (d, case.id))
        if sigma is not None:
            sig = max(sig, (P.sigma_error(sigma, x.state)[0], case.id))
    figures = [(f"E_REF[{tau}]", e_ref[tau], P.E_REF[tau]) for tau in sorted(e_ref)]
    figures += [(f"DIST_REF[{m}]", dist[m], P.DIST_REF[m]) for m in sorted(dist)] + [("SIGMA_REF", sig, P.SIGMA_REF)]
    for name, (got, where), recorded in figures:
        print(f"{name}: measured {got:.4e} at {where}, recorded {recorded:.4e}")
    for tau in sorted(e_ref):
        print(f"S({tau}) = {P.S(tau):.4e}")
    for name, (got, where), recorded in figures:
        assert 0.75 * recorded <= got <= 1.25 * recorded, f"{name}: measured {got:.4e}, recorded {recorded:.4e}"


# ------------------------------------------------------------------------------------------------ class sums, EMA, append
@pytest.mark.parametrize("sc", P.SUMS_CASES, ids=ids)
def test_oracle_class_sums_pass(sc):
    rows, out, cls = P.sums_inputs(sc)
    if sc.classes:  # the oracle knows no dropped rows: it is given the kept ones
        keep = (cls >= 0) & (cls < P.SUMS_K)
        o = torch.nn.functional.one_hot(cls[keep].long(), P.SUMS_K).float()
        s, n = op.class_sums(rows[keep], o)
        s2, _ = op.class_sums(rows[keep] ** 2, o)
        assert 0.25 < float((~keep).double().mean()) < 0.35 and int((cls == 6).sum()) == 0 and int(cls[11]) == -1
    else:
        s, n = op.class_sums(rows, out)
        s2, _ = op.class_sums(rows ** 2, out)
    P.check_class_sums(s, s2, n, rows, cls, P.SUMS_K, f"oracle {sc.id}")


def test_class_sum_check_sees_a_dropped_row_and_a_lost_bit():
    sc = P.SUMS_CASES[0]
    rows, out, cls = P.sums_inputs(sc)
    s, n = op.class_sums(rows, out)
    s2, _ = op.class_sums(rows ** 2, out)
    k = int(cls[0])
    assert P.flagged(P.check_class_sums, s - rows[0] * (torch.arange(P.SUMS_K) == k)[:, None], s2, n, rows, cls, P.SUMS_K, "probe")
    assert P.flagged(P.check_class_sums, s, s2 * (1 + 2e-5), n, rows, cls, P.SUMS_K, "probe")
    assert P.flagged(P.check_class_sums, s, s2, n + (torch.arange(P.SUMS_K) == k), rows, cls, P.SUMS_K, "probe")


def test_oracle_ema_and_append_pass():
    st, ((ra, oa), (rb, ob), (rc, oc)) = P.update_inputs()
    sums = lambda r, o: (op.class_sums(r, o)[0], op.class_sums(r ** 2, o)[0], op.class_sums(r, o)[1])  # noqa: E731
    # EMA on a batch without classes 4 and 11
    s, s2, n = sums(ra, oa)
    assert n[4] == 0 and n[11] == 0 and int((n == 0).sum()) == 2
    proto, sq, counter = op.ema_update(st, ra, oa, torch.tensor(0.9995))
    r_proto, r_sq, w_proto, w_sq = P.ema64(st, s, s2, n, 0.9995)
    P.check_weighted(proto, r_proto, w_proto, P.R_EMA, "oracle ema proto")
    P.check_weighted(sq, r_sq, w_sq, P.R_EMA, "oracle ema sqmean")
    for k in (4, 11):
        assert torch.equal(proto[k], st[0][k]) and torch.equal(sq[k], st[1][k])
    assert torch.equal(counter, st[2])
    assert P.flagged(P.check_weighted, proto * (1 + 1e-6), r_proto, w_proto, P.R_EMA, "probe")
    # append from the empty state (class 5 absent), then a batch in which it first appears
    s, s2, n = sums(rb, ob)
    assert n[5] == 0
    st1 = op.running_append(None, rb, ob)
    r = P.append64(None, s, s2, n)
    P.check_weighted(st1[0], r[0], r[3], P.R_APPEND, "oracle append 1 proto")
    P.check_weighted(st1[1], r[1], r[4], P.R_APPEND, "oracle append 1 sqmean")
    assert torch.equal(st1[2].double(), r[2]) and bool((st1[0][5] == 0).all())
    s, s2, n = sums(rc, oc)
    assert n[5] > 0
    st2 = op.running_append(st1, rc, oc)
    r = P.append64(st1, s, s2, n)
    P.check_weighted(st2[0], r[0], r[3], P.R_APPEND, "oracle append 2 proto")
    P.check_weighted(st2[1], r[1], r[4], P.R_APPEND, "oracle append 2 sqmean")
    assert torch.equal(st2[2].double(), r[2])


# ------------------------------------------------------------------------------------------------ teeth: the expanded form
def expanded_fp32(case, centred):
    """The soft map of the expanded form in float32: D^2 = |g|^2 - 2 g.q + |q|^2 with g = (f - c) / sigma, q = (p - c) / sigma,
    c = the mean prototype (centred) or 0; pixels whose two largest posteriors, or whose largest posterior and the threshold,
    lie within 1e-3 take the direct form's (the oracle's) values instead."""
    x = P.inputs(case)
    proto = x.state[0]
    inv = 1.0 / op.global_std(x.state) if case.metric == "mahalanobis" else torch.ones(P.C)
    c = proto.mean(0) if centred else torch.zeros(P.C)
    g, q = (x.rows - c) * inv, (proto - c) * inv
    d = ((g * g).sum(1, keepdim=True) - 2.0 * (g @ q.T) + (q * q).sum(1)[None]).clamp(min=0).sqrt()
    post = (-(d - d.min(1, keepdim=True)[0]) / case.tau).softmax(1)
    if x.prior is not None:
        post = post * x.prior
    post = post / post.sum(1, keepdim=True)
    top = post.topk(min(2, case.K), dim=1)[0]
    best, second = top[:, 0], (top[:, 1] if case.K > 1 else torch.full_like(top[:, 0], -float("inf")))
    redo = (best - second < 1e-3) | ((best - case.thresh).abs() < 1e-3)
    return torch.where(redo[:, None], oracle(case)[1], post), float(redo.double().mean())


@pytest.mark.parametrize("case", [c for c in P.CASES if c.id.startswith("off")], ids=ids)
def test_uncentred_expanded_form_fails_the_soft_map_bound(case):
    soft, redone = expanded_fp32(case, centred=False)
    ref = P.reference_with(case, oracle(case)[3])
    e = P.soft_error(soft, ref)
    print(f"{case.id}: uncentred expanded form off by {e:.3e} (S = {P.S(case.tau):.3e}), {100 * redone:.1f} % redone directly")
    assert e > P.S(case.tau)
    assert P.flagged(P.check_assign, ref.labels, soft, ref.means, ref, case.tau, "probe")


@pytest.mark.parametrize("case", ALL, ids=ids)
def test_centred_expanded_form_passes(case):
    soft, redone = expanded_fp32(case, centred=True)
    ref = P.reference_with(case, oracle(case)[3])
    print(f"{case.id}: {100 * redone:.1f} % redone directly")
    P.check_assign(ref.labels, soft, ref.means, ref, case.tau, f"centred {case.id}", soft_only=True)


def test_label_check_sees_a_swapped_and_a_rejected_label():
    case = P.BY_ID["off8-maha"]
    labels, soft, means, sigma = oracle(case)
    ref = P.reference_with(case, sigma)
    clear = int((ref.gap > 0.05).nonzero()[0])
    for wrong in (int(ref.arg2[clear]), 255 if int(ref.labels[clear]) != 255 else int(ref.arg[clear])):
        bad = labels.clone()
        bad[clear] = wrong
        assert P.flagged(P.check_assign, bad, soft, means, ref, case.tau, "probe")
    assert P.flagged(P.check_assign, labels, soft, means + 1e-4, ref, case.tau, "probe")


def test_runner_up_is_no_candidate_clearly_below_the_threshold():
    """A close race between two classes that both lie clearly under the threshold: 255 is the only label."""
    case = P.BY_ID["off8-maha"]
    ref = P.reference(case)
    i = int((ref.labels != 255).nonzero()[0])
    best, second, gap, labels = ref.best.clone(), ref.second.clone(), ref.gap.clone(), ref.labels.clone()
    best[i], second[i], gap[i], labels[i] = 0.2, 0.2 - 1e-7, 1e-7, 255
    ref = ref._replace(best=best, second=second, gap=gap, labels=labels)
    P.check_assign(labels, ref.soft, ref.means, ref, case.tau, "rejected")
    for wrong in (int(ref.arg2[i]), int(ref.arg[i])):
        bad = labels.clone()
        bad[i] = wrong
        assert P.flagged(P.check_assign, bad, ref.soft, ref.means, ref, case.tau, "probe")
    best[i], second[i] = 0.6, 0.6 - 1e-7  # the same race clearly above it: either class, not 255
    ref = ref._replace(best=best, second=second, labels=ref.labels.clone().index_fill_(0, torch.tensor([i]), int(ref.arg[i])))
    for label, ok in ((int(ref.arg[i]), True), (int(ref.arg2[i]), True), (255, False)):
        lab = ref.labels.clone()
        lab[i] = label
        assert P.flagged(P.check_assign, lab, ref.soft, ref.means, ref, case.tau, "probe") != ok
