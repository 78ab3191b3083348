"""numpy.longdouble reference of the outlier-robust chain placement (include/cora_hip.h, cora_place_chains_robust_dev) -- TEST
INFRASTRUCTURE ONLY.  Built on tests/placement_ref.py and tests/placement_levels_ref.py: the stages and their lists (greedy or
levels), the linear stage, the Gauss-Newton steps and the refit are their functions; new here are the samples, the hypotheses
with their polish, the scores, the vote with its intervals and the election.

Per stage list of L >= m = unknowns + 1 entries: the hypothesis of entry h is placement_ref.solve_stage with HYP_STEPS
Gauss-Newton steps over the sample (h + k s) mod L, k = 0 .. m - 1, s = max(1, L // m), about the LIST's origin (the list's
first entry is put in front of the sample with precision 0: it adds nothing to any sum and gives the coordinates), in
longdouble with plain sums: its last visited point.  r(h, j) = omega_j (|R_h q'_j + t'_h - a'_j| - r_j)^2.

Bound on r(h, j) (derived, its constant measured).  The hypothesis is a stage of the plain placement, so placement_ref's bound
holds for it: t'_h moves by at most C a_h and R_h by C a_h / L_h, with a_h = eps max(kappa(M_h) (|t'| + L)^2 / L, kappa(H_h)
(|t'| + L), |t'| + L).  The residual e = |R q' + t' - a'| - r then moves by at most de = C a_h (1 + |q'| / L_h) + 4 eps (|q'| +
|t'| + |a'| + |p| + r) (the products, the fma chains, the root, the difference) and omega e^2 by at most omega (2 |e| de +
de^2) + 4 eps omega e^2.  C_BOUND: measured as placement_ref's was -- the host mirror of the plain placement with HYP_STEPS
Gauss-Newton steps (pl_linear_terms, pl_pair_sum, pl_linear_solve, pl_gn_terms, pl_gn_step: the functions pl_hypothesis calls;
the robust call does not return g_h) on samples of the lists of tests/test_chain_consensus_cpu.py's cases, each as the list of
a chain of its own, against placement_ref on the same entries about the same origin: measure_constant() below.

A pair (h, j) whose reference residual lies within its bound of barc2 is IN THE BAND.  A hypothesis with a pivot of the linear
stage within its band of 1e-8 (pivot_band) may be valid on one side and not on the other: its vote interval starts at 0 and ends
at the votes it has where it is held valid.  Votes become intervals [certain, certain + in band]; check() asserts that the
election is unambiguous under the intervals, then that the elected entry, the consensus, the statuses and the inlier bytes are
exactly the reference's, then transforms, rows, costs and `chosen` within placement_ref.check's bound computed over I (the
refit is placement_ref.solve_stage with the precisions outside I set to zero: an entry outside I adds nothing to any sum, and
the origin stays the list's)."""
import numpy as np

import placement_levels_ref as plr
import placement_ref as pl

LD = pl.LD
EPS = pl.EPS
HYP_STEPS = 3   # kPlHypSteps
GREEDY, LEVELS = plr.GREEDY, plr.LEVELS
# A pivot of the scaled normal matrix is a diagonal entry minus at most N - 1 = 15 squares of factor entries; every operand
# carries about 6 roundings of a value <= 16 (an entry of the scaled matrix: a mean of products of terms 2 q' / L, 2 a' / L <=
# 4) divided by (the least pivot before it, where that is below 1: the factor's entries are divided by its root twice):
# 16 x 6 x 16 eps; 4 x that as the band.
PIVOT_BAND = 4 * 16 * 6 * 16 * EPS
# 4 x the worst ratio error / (a + b) of the mirror's polished hypotheses over the samples test_the_constant_of_the_score_bound
# measures (6.45, on a sample with lengthened ranges whose three steps have not converged; 0.60 at d = 3: profiles/chain_consensus.md)
C_BOUND = 26.0


def terms(d):
    return pl.unknowns(d) + 1


def sample(h, L, d):
    m = terms(d)
    s = max(1, L // m)
    return [(h + k * s) % L for k in range(m)]


def _stage(d, q, a, rng, w, steps, min_pivot):
    keep = pl.MIN_PIVOT
    pl.MIN_PIVOT = min_pivot
    try:
        return pl.solve_stage(d, q, a, rng, w, steps)
    finally:
        pl.MIN_PIVOT = keep


def pivot_near(piv):
    """(near, band): whether a pivot lies within its band of the refusal rule, and the widest band seen."""
    near, widest = False, 0.0
    for j, p in enumerate(piv):
        band = PIVOT_BAND / min([1.0] + [max(x, pl.MIN_PIVOT) for x in piv[:j]])
        widest = max(widest, band)
        near = near or abs(p - pl.MIN_PIVOT) <= band
    return near, widest


def hypothesis(d, q, a, rng, w, idx):
    """The hypothesis of the sample idx of the list q, a [L][d], rng, w (longdouble) about the list's origin.  dict valid, R, t
    (t'), L, a (the bound's unit, without C), near (a pivot in its band of the rule), alt (near only: the hypothesis with the
    rule lowered by the band, or None where it is refused there too), unknown (refused there too, but not surely)."""
    sel = np.concatenate([[0], np.asarray(idx)])
    ws = np.concatenate([[LD(0)], w[idx]])

    def run(min_pivot):
        one = _stage(d, q[sel], a[sel], rng[sel], ws, HYP_STEPS, min_pivot)
        R, t = one["visited"][-1]
        tp, L = float(pl._norm(t)), one["L"]
        unit = EPS * max(one["kappa_lin"] * (tp + L) ** 2 / L, one["kappa_gn"] * (tp + L), tp + L)
        return dict(valid=one["status"] == 0, R=R, t=t, L=L, a=unit, pivots=one["pivots"])

    out = run(pl.MIN_PIVOT)
    out["near"], band = pivot_near(out["pivots"])
    out["alt"], out["unknown"] = None, False
    if out["near"] and not out["valid"]:
        alt = run(max(pl.MIN_PIVOT - band, 0.0))
        out["alt"] = alt if alt["valid"] else None
        # (refused there too, at a pivot that is still within its band of the rule: nothing is known of its votes)
        out["unknown"] = not alt["valid"] and pivot_near(alt["pivots"])[0] and alt["pivots"][-1] > pl.MIN_PIVOT - pivot_near(alt["pivots"])[1]
    return out


def scores(hyp, qq, aa, rng, w):
    """(r, e, |p|) of every entry under the hypothesis, longdouble."""
    p = qq @ hyp["R"].T + hyp["t"][None, :] - aa
    nrm = np.sqrt(np.sum(p * p, axis=1))
    e = nrm - rng
    return w * e * e, e, nrm


def score_bound(hyp, qq, aa, rng, w, r, e, nrm, C):
    nq, na = np.sqrt(np.sum(qq * qq, axis=1)), np.sqrt(np.sum(aa * aa, axis=1))
    de = C * hyp["a"] * (1 + nq / hyp["L"]) + 4 * EPS * (nq + float(pl._norm(hyp["t"])) + na + nrm + rng)
    return w * (2 * np.abs(e) * de + de * de) + 4 * EPS * r


def vote_list(d, q, a, rng, w, barc2, C=C_BOUND):
    """The vote over one list.  dict hyp (per entry), lo, hi (the vote intervals), elected, consensus, ambiguous (a list of
    reasons, empty where the election is the reference's alone), inlier (bool per entry), band (entries whose residual under the
    elected hypothesis lies within its bound of barc2), r (the residuals under the elected hypothesis), valid (how many)."""
    L = len(q)
    qq, aa = q - q[0], a - a[0]
    lo, hi, hyps = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64), []

    def interval(hyp):
        r, e, nrm = scores(hyp, qq, aa, rng, w)
        bound = score_bound(hyp, qq, aa, rng, w, r, e, nrm, C)
        sure = r <= barc2 - bound
        maybe = (np.abs(r - barc2) <= bound) & ~sure
        return r, np.flatnonzero(np.abs(r - barc2) <= bound), int(np.sum(sure)), int(np.sum(sure)) + int(np.sum(maybe))

    for h in range(L):
        hyp = hypothesis(d, q, a, rng, w, sample(h, L, d))
        hyps.append(hyp)
        if hyp["valid"]:
            hyp["r"], hyp["in_band"], lo[h], hi[h] = interval(hyp)
            if hyp["near"]:
                lo[h] = 0
        elif hyp["alt"] is not None:
            hi[h] = interval(hyp["alt"])[3]
        elif hyp["unknown"]:
            hi[h] = L
    best = 0
    for h in range(1, L):
        if lo[h] > lo[best]:
            best = h
    ambiguous = []
    for h in range(L):
        if h != best and (hi[h] > lo[best] or (hi[h] == lo[best] and h < best)):
            ambiguous.append(("entry %d could beat the elected %d" % (h, best), int(lo[best]), int(hi[h])))
    if hi[best] != lo[best]:
        ambiguous.append(("the consensus of the elected %d is an interval" % best, int(lo[best]), int(hi[best])))
    hyp = hyps[best]
    inlier, band, r = np.zeros(L, dtype=bool), [], None
    if hyp["valid"] and lo[best] > 0:
        r = hyp["r"]
        inlier = np.asarray(r <= barc2)
        band = [int(j) for j in hyp["in_band"]]
    return dict(hyp=hyps, lo=lo, hi=hi, elected=best, consensus=int(lo[best]), ambiguous=ambiguous, inlier=inlier, band=band, r=r,
                valid=sum(1 for x in hyps if x["valid"]))


def structure(order, d, n, r, nt, table, chains, chain_fixed=None, min_ranges=None):
    return (pl if order == GREEDY else plr).structure(d, n, r, nt, table, chains, chain_fixed, min_ranges)


def reference(d, n, r, nt, table, chains, X, gn_steps, barc2, min_consensus=None, order=LEVELS, chain_fixed=None, min_ranges=None, votes=None,
              C=C_BOUND):
    """placement_ref.reference's dict for the robust call over the stages of `order` (status 5: no consensus; such a chain is in
    none of struct's stages, so that placement_ref.check treats it as a chain that keeps its rows) plus elected, consensus,
    list_len (per chain), inlier (per range measurement: 1 | 0 | 2), no_consensus, excluded, ambiguous and band (lists of
    (chain, ..) that must be empty on a committed case), margin (the largest inlier and the least outlier residual under the
    elected hypotheses, over barc2), votes (per stage the dict of vote_list: pass it back in to share the vote between two
    gn_steps), n_stages."""
    min_consensus = 2 * terms(d) if min_consensus is None else min_consensus
    rr, rd = np.asarray(table[2]), np.asarray(table[3], dtype=np.float64)
    X = np.array(X, dtype=LD)
    S = structure(order, d, n, r, nt, table, chains, chain_fixed, min_ranges)
    nch = len(chains)
    res = dict(status=np.array(S["init"], dtype=np.uint8), chosen=np.full(nch, -1, dtype=np.int32),
               cost_start=np.zeros(nch, dtype=LD), cost_linear=np.zeros(nch, dtype=LD), cost_final=np.zeros(nch, dtype=LD), steps=0,
               transforms=np.tile(np.concatenate([np.eye(d).reshape(-1), np.zeros(d)]), (nch, 1)).astype(LD), stage=[], row_a={}, row_b={},
               elected=np.full(nch, -1, dtype=np.int32), consensus=np.zeros(nch, dtype=np.int32), list_len=np.zeros(nch, dtype=np.int32),
               inlier=np.full(len(rr), 2, dtype=np.uint8), ambiguous=[], band=[], votes=[], margin=[0.0, np.inf], n_stages=len(S["stages"]))
    kept = []
    for k, st in enumerate(S["stages"]):
        qi, ai, ms = np.array(st["q"]), np.array(st["a"]), np.array(st["m"])
        q, a = X[qi], X[ai]
        rng, w = rd[ms, 0].astype(LD), rd[ms, 1].astype(LD)
        c = st["chain"]
        vote = votes[k] if votes is not None else vote_list(d, q, a, rng, w, barc2, C)
        res["votes"].append(vote)
        res["elected"][c], res["consensus"][c], res["list_len"][c] = vote["elected"], vote["consensus"], len(ms)
        res["inlier"][ms] = vote["inlier"].astype(np.uint8)
        res["ambiguous"] += [(c,) + x for x in vote["ambiguous"]]
        res["band"] += [(c, j) for j in vote["band"]]
        if vote["r"] is not None:
            rin, rout = vote["r"][vote["inlier"]], vote["r"][~vote["inlier"]]
            res["margin"][0] = max(res["margin"][0], float(rin.max()) / barc2 if len(rin) else 0.0)
            res["margin"][1] = min(res["margin"][1], float(rout.min()) / barc2 if len(rout) else np.inf)
        if vote["consensus"] < min_consensus:
            res["status"][c] = 5
            continue
        kept.append(st)
        one = pl.solve_stage(d, q, a, rng, w * vote["inlier"], gn_steps)
        res["status"][c], res["chosen"][c], res["steps"] = one["status"], one["chosen"], res["steps"] + one["steps"]
        res["cost_start"][c], res["cost_linear"][c], res["cost_final"][c] = one["costs"][0], one["costs"][1], one["costs"][one["chosen"]]
        R, t = pl.full_transform(one, q[0], a[0], one["chosen"])
        res["transforms"][c] = np.concatenate([R.reshape(-1), t])
        L, tp = one["L"], float(pl._norm(one["visited"][one["chosen"]][1]))
        kap = max(one["kappa_lin"], one["kappa_gn"], 1.0)
        delta = max([res["row_a"].get(int(x), 0.0) for x in ai] + [0.0])
        one.update(q0=q[0].copy(), a0=a[0].copy(), rows_before={},
                   a=EPS * max(one["kappa_lin"] * (tp + L) ** 2 / L, one["kappa_gn"] * (tp + L), tp + L) + kap * delta)
        for rot, trn in S["positions"][c]:
            x = X[trn].copy()
            one["rows_before"][trn] = (x, X[rot:rot + d].copy())
            xn = R @ x + t
            X[rot:rot + d] = X[rot:rot + d] @ R.T
            X[trn] = xn
            res["row_a"][trn] = one["a"] * (1 + float(pl._norm(x - q[0])) / L)
            res["row_b"][trn] = EPS * float(pl._norm(q[0]) + pl._norm(a[0]) + pl._norm(t) + pl._norm(x) + pl._norm(xn))
        res["stage"].append(one)
    deg, norm = np.zeros(len(rr), dtype=bool), np.zeros(len(rr), dtype=LD)
    for m in range(len(rr)):
        diff = X[rr[m, 2]] - X[rr[m, 1]]
        nrm = norm[m] = np.sqrt(np.sum(diff * diff))
        deg[m] = nrm < 1e-5
        X[rr[m, 0]] = 0 if deg[m] else -diff / nrm
    res.update(X=X, degenerate=deg, norm=norm, struct=dict(S, stages=kept), no_consensus=int(np.sum(res["status"] == 5)),
               excluded=int(np.sum(res["inlier"] == 0)))
    return res


def committed(ref):
    """Whether a case may be committed, BY THE REFERENCE ALONE: an unambiguous election, an empty band about barc2 under the
    elected hypotheses, inliers <= barc2 / 2 and outliers >= 2 barc2."""
    return ref["ambiguous"] == [] and ref["band"] == [] and ref["margin"][0] <= 0.5 and ref["margin"][1] >= 2.0


def check(got, d, n, r, nt, table, ref, C=pl.C_BOUND):
    """Asserts that the case may be committed, then elected, consensus, list lengths, inlier bytes and counts exactly, then
    everything placement_ref.check asserts, over I (a chain of status 5 as a chain that is no stage: its rows keep the caller's
    bits); returns its worst error / (a + b)."""
    assert ref["ambiguous"] == [], ref["ambiguous"][:5]
    assert ref["band"] == [], ref["band"][:5]
    assert ref["margin"][0] <= 0.5 and ref["margin"][1] >= 2.0, ref["margin"]
    for key in ("elected", "consensus", "list_len", "inlier"):
        assert np.array_equal(got[key], ref[key]), (key, got[key], ref[key])
    assert got["no_consensus"] == ref["no_consensus"] and got["excluded"] == ref["excluded"]
    assert got["stages"] == ref["n_stages"] and got["placed"] == ref["n_stages"] - ref["no_consensus"]   # (no consensus: a stage, not placed)
    assert got["not_placed"] == ref["no_consensus"] + sum(1 for s in ref["struct"]["init"] if s in (1, 3))
    kept = len(ref["struct"]["stages"])
    assert got["placed"] == kept
    plain = dict(got, stages=kept, not_placed=got["not_placed"] - got["no_consensus"])
    return pl.check(plain, d, n, r, nt, table, ref, C)


def measure_constant(ctx_of, d, q, a, rng, w, stride=1):
    """The worst error / (a + b) of the mirror's polished hypotheses over the samples h = 0, stride, .. of one list (q, a [L][d]
    as the vector holds them, rng, w: float64): each sample becomes the list of a chain of its own against one fixed chain of
    all the anchors, in a graph the plain mirror places with HYP_STEPS Gauss-Newton steps (ctx_of(dims): a fresh plan-only
    handle); the origin is the sample's first entry on both sides.  A sample with a pivot in its band of the rule is left out.
    Returns (worst ratio, samples measured)."""
    m, L = terms(d), len(q)
    picks = []
    for h in range(0, L, stride):
        idx = sample(h, L, d)
        one = _stage(d, np.asarray(q[idx], dtype=LD), np.asarray(a[idx], dtype=LD), np.asarray(rng[idx], dtype=LD), np.asarray(w[idx], dtype=LD),
                     0, pl.MIN_PIVOT)
        if not pivot_near(one["pivots"])[0]:
            picks.append(idx)
    k = len(picks)
    if k == 0:
        return 0.0, 0
    world = np.concatenate([np.concatenate([a[idx] for idx in picks]), np.concatenate([q[idx] for idx in picks])])
    ranges = [(s * m + j, k * m + s * m + j) for s in range(k) for j in range(m)]
    dims, table, Y, chains, _ = pl.scene(d, [k * m] + [m] * k, ranges, seed=1, world=world, moved=False)
    table[3][:, 0] = np.concatenate([rng[idx] for idx in picks])
    table[3][:, 1] = np.concatenate([w[idx] for idx in picks])
    ctx = ctx_of(dims)
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_chain_placement(min_ranges=m)
    got = ctx.debug_place_chains_host(Y, HYP_STEPS)
    got["X_in"] = Y
    ref = pl.reference(*dims, table, chains, Y, HYP_STEPS, min_ranges=m)
    return pl.check(got, *dims, table, ref, C=1e6), k
