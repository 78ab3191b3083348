"""numpy.longdouble reference of the outlier-robust multilateration (include/cora_hip.h, cora_multilaterate_robust_dev) -- TEST
INFRASTRUCTURE ONLY.  Built on tests/multilat_ref.py: the lists, the linear stage and the Gauss-Newton refit are its functions;
new here are the samples, the hypotheses, the scores, the vote with its intervals and the election.

Per list that is voted on (L >= d + 1 entries, the landmark on): the hypothesis of entry h is the linear stage over the sample
(h + k s) mod L, k = 0 .. d, s = max(1, L // (d + 1)), about the LIST's origin t_0, in longdouble with plain sums; with it come
the condition number of the scaled normal matrix and its smallest pivot.  r(h, j) = omega_j (|y_h - u_j| - r_j)^2.

Bound on r(h, j) (derived, its constant measured).  The hypothesis is a linear stage, so multilat_ref's bound holds for it: y_h
moves by at most C a_h with a_h = eps kappa(M_h) (|y_h| + L_h)^2 / L_h.  The residual e = |y - u| - r then moves by at most
de = C a_h + 4 eps (|y| + |u| + |y - u| + r) (the subtractions, the fma chain, the root, the difference), and omega e^2 by at most
omega (2 |e| de + de^2) + 4 eps omega e^2.  C_BOUND: measured as multilat_ref's was -- the host mirror's linear stage
(cora_debug_multilaterate_host with no Gauss-Newton step: ml_linear_terms and ml_linear_solve, the two functions ml_hypothesis
calls; the robust call does not return y_h) on every sample of every list of tests/test_range_consensus_cpu.py's cases as a list
of its own, against this module's hypothesis of the same d + 1 entries about the same origin: measure_constant() below.

A pair (h, j) whose reference residual lies within its bound of barc2 is IN THE BAND; a hypothesis whose smallest pivot lies
within PIVOT_BAND (below) of 1e-8 is in the band too, with all its pairs.  Votes
become intervals [certain, certain + in band]; check() asserts that the election is unambiguous under the intervals, then that
the elected entry, the consensus, the statuses and the flags are exactly the reference's, then rows, costs and `chosen` within
multilat_ref.check's bound computed over I (the refit is multilat_ref.solve_landmark with the precisions outside I set to zero:
an entry outside I adds nothing to any sum, and the origin stays the list's)."""
import numpy as np

import multilat_ref as ml

LD = ml.LD
EPS = ml.EPS
# A pivot of the scaled normal matrix (entries <= 4, trace of its leading block 4) is a diagonal entry minus at most d squares
# of factor entries: each of the d + 1 <= 4 operands carries about 6 roundings of a value <= 4 / (the least pivot before it, where
# that is below 1: the factor's entries are divided by its root twice), so 4 x 4 x 6 eps ~ 100 eps; 4 x that as the band.
PIVOT_BAND = 400 * EPS
C_BOUND = 1.4   # 4 x the worst ratio |y_mirror - y_ref| / a_h over the samples of the CPU cases (0.33, profiles/range_consensus.md)


def sample(h, L, d):
    s = max(1, L // (d + 1))
    return [(h + k * s) % L for k in range(d + 1)]


def hypothesis(d, u, rng, w):
    """The linear stage over the entries u [m][d] (relative to the origin), rng, w (longdouble), plain sums.  dict valid, y,
    kappa, L, pivot (the smallest), a (the bound's unit, without C)."""
    out = dict(valid=False, y=np.zeros(d, dtype=LD), kappa=np.inf, L=0.0, pivot=0.0, a=np.inf, near_pivot=False)
    n2 = np.sum(u * u, axis=1)
    b = rng * rng - n2
    sw, tr = ml._lsum(w), ml._lsum(w * n2)
    if not sw > 0 or not tr > 0:
        return out
    L = np.sqrt(tr / sw)
    M = np.zeros((d + 1, d + 1), dtype=LD)
    q = np.zeros(d + 1, dtype=LD)
    M[:d, :d] = 4 * ml._lsum(w[:, None, None] * u[:, :, None] * u[:, None, :]) / tr
    M[:d, d] = M[d, :d] = -2 * ml._lsum(w[:, None] * u) / (L * sw)
    M[d, d] = 1
    q[:d] = -2 * ml._lsum((w * b)[:, None] * u) / (L * tr)
    q[d] = ml._lsum(w * b) / tr
    z, piv = ml._chol_solve(M, q, ml.MIN_PIVOT)
    out["L"], out["pivot"] = float(L), float(min(piv))
    out["near_pivot"] = any(abs(p - ml.MIN_PIVOT) <= PIVOT_BAND / min([1.0] + [max(x, ml.MIN_PIVOT) for x in piv[:j]]) for j, p in enumerate(piv))
    if z is None:
        # (a refused factorisation stopped at its first small pivot: the band rule below reads that pivot)
        return out
    y = L * z[:d]
    if not np.all(np.isfinite(np.asarray(y, dtype=np.float64))):
        return out
    ny = float(np.sqrt(np.sum(y * y)))
    kappa = ml._cond(M)
    out.update(valid=True, y=y, kappa=kappa, a=EPS * kappa * (ny + float(L)) ** 2 / float(L))
    return out


def scores(y, u, rng, w):
    """(r, e, |y - u|) of every entry under the point y, longdouble."""
    D = y[None, :] - u
    nrm = np.sqrt(np.sum(D * D, axis=1))
    e = nrm - rng
    return w * e * e, e, nrm


def score_bound(hyp, u, rng, w, r, e, nrm, C):
    ny = float(np.sqrt(np.sum(hyp["y"] * hyp["y"])))
    de = C * hyp["a"] + 4 * EPS * (ny + np.sqrt(np.sum(u * u, axis=1)) + nrm + rng)
    return w * (2 * np.abs(e) * de + de * de) + 4 * EPS * r


def vote_list(d, t, rng, w, barc2, C=C_BOUND):
    """The vote over one list: t [L][d] anchors, rng, w (longdouble).  dict hyp (per entry), lo, hi (the vote intervals), elected,
    consensus, ambiguous (a list of reasons, empty where the election is the reference's alone), inlier (bool per entry), band
    (entries whose residual under the elected hypothesis lies within its bound of barc2)."""
    L = len(t)
    u = t - t[0]
    lo, hi, hyps = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64), []
    for h in range(L):
        idx = sample(h, L, d)
        hyp = hypothesis(d, u[idx], rng[idx], w[idx])
        near_pivot = hyp["near_pivot"]
        hyps.append(hyp)
        if not hyp["valid"]:
            if near_pivot:   # the device may hold it valid: its votes are unknown
                hi[h] = L
            continue
        r, e, nrm = scores(hyp["y"], u, rng, w)
        bound = score_bound(hyp, u, rng, w, r, e, nrm, C)
        sure = r <= barc2 - bound
        maybe = (np.abs(r - barc2) <= bound) & ~sure
        hyp["r"], hyp["in_band"] = r, np.flatnonzero(np.abs(r - barc2) <= bound)
        lo[h] = 0 if near_pivot else int(np.sum(sure))
        hi[h] = int(np.sum(sure)) + int(np.sum(maybe))
    best = 0
    for h in range(1, L):
        if lo[h] > lo[best]:
            best = h
    ambiguous = []
    for h in range(L):
        if h == best:
            continue
        if hi[h] > lo[best] or (hi[h] == lo[best] and h < best):
            ambiguous.append(("entry %d could beat the elected %d" % (h, best), int(lo[best]), int(hi[h])))
    if hi[best] != lo[best]:
        ambiguous.append(("the consensus of the elected %d is an interval" % best, int(lo[best]), int(hi[best])))
    hyp = hyps[best]
    inlier = np.zeros(L, dtype=bool)
    band = []
    if hyp["valid"] and lo[best] > 0:
        inlier = np.asarray(hyp["r"] <= barc2)
        band = [int(j) for j in hyp["in_band"]]
    return dict(hyp=hyps, lo=lo, hi=hi, elected=best, consensus=int(lo[best]), ambiguous=ambiguous, inlier=inlier, band=band)


def reference(d, n, r, nt, table, X, gn_steps, barc2, min_consensus=None, pose_ok=None, landmark_on=None, votes=None, C=C_BOUND):
    """multilat_ref.reference's dict for the robust call (status 5: no consensus) plus elected, consensus, list_len (per landmark),
    inlier (per range measurement: 1 | 0 | 2), no_consensus, excluded, ambiguous and band (lists of (landmark, ..) that must be
    empty on a committed case), votes (per landmark the dict of vote_list, or None: pass it back in to share the vote between
    two gn_steps)."""
    min_consensus = d + 2 if min_consensus is None else min_consensus
    rr, rd = np.asarray(table[2]), np.asarray(table[3], dtype=np.float64)
    X = np.array(X, dtype=LD)
    nl, t0 = nt - n, d * n + r
    lists, usable, skipped = ml.lists_of(d, n, r, nt, rr, pose_ok, landmark_on)
    res = dict(status=np.zeros(nl, dtype=np.uint8), chosen=np.full(nl, -1, dtype=np.int32), cost_linear=np.zeros(nl, dtype=LD),
               cost_final=np.zeros(nl, dtype=LD), steps=0, lm=[], bound=[], elected=np.full(nl, -1, dtype=np.int32),
               consensus=np.zeros(nl, dtype=np.int32), list_len=np.array([len(lst) for lst in lists], dtype=np.int32),
               inlier=np.full(len(rr), 2, dtype=np.uint8), ambiguous=[], band=[], votes=[])
    for l, lst in enumerate(lists):
        rows = np.array([a for a, _ in lst], dtype=np.int64)
        ms = np.array([m for _, m in lst], dtype=np.int64)
        on = landmark_on is None or landmark_on[l]
        vote = None
        if on and len(lst) >= d + 1:
            rng, w = rd[ms, 0].astype(LD), rd[ms, 1].astype(LD)
            vote = votes[l] if votes is not None else vote_list(d, X[rows], rng, w, barc2, C)
            res["elected"][l], res["consensus"][l] = vote["elected"], vote["consensus"]
            res["inlier"][ms] = vote["inlier"].astype(np.uint8)
            res["ambiguous"] += [(l,) + a for a in vote["ambiguous"]]
            res["band"] += [(l, j) for j in vote["band"]]
            if vote["consensus"] < min_consensus:
                one = dict(status=5, y=None, chosen=-1, costs=[], steps=0, kappa_lin=0.0, kappa_gn=0.0, L=0.0, pivots=[])
            else:
                one = ml.solve_landmark(d, X[rows], rng, w * vote["inlier"], gn_steps)
        else:   # not voted on: masked or empty (3), too short (1)
            one = dict(status=3 if not on or len(lst) == 0 else 1, y=None, chosen=-1, costs=[], steps=0, kappa_lin=0.0, kappa_gn=0.0, L=0.0,
                       pivots=[])
        res["votes"].append(vote)
        res["lm"].append(one)
        res["status"][l] = one["status"]
        a = b = 0.0
        if one["status"] == 0:
            y, L = one["y"], one["L"]
            x = X[rows[0]] + y
            X[t0 + n + l] = x
            res["chosen"][l] = one["chosen"]
            res["cost_linear"][l], res["cost_final"][l] = one["costs"][0], one["costs"][one["chosen"]]
            res["steps"] += one["steps"]
            ny, nx = float(np.sqrt(np.sum(y * y))), float(np.sqrt(np.sum(x * x)))
            a = EPS * max(one["kappa_lin"] * (ny + L) ** 2 / L, one["kappa_gn"] * (ny + L))
            b = EPS * nx
        res["bound"].append((a, b))
    deg, norm = np.zeros(len(rr), dtype=bool), np.zeros(len(rr), dtype=LD)
    for m in range(len(rr)):
        diff = X[rr[m, 2]] - X[rr[m, 1]]
        nrm = norm[m] = np.sqrt(np.sum(diff * diff))
        deg[m] = nrm < 1e-5
        X[rr[m, 0]] = 0 if deg[m] else -diff / nrm
    chunks = sum((len(lst) + ml.CHUNK - 1) // ml.CHUNK for lst in lists)
    res.update(X=X, degenerate=deg, norm=norm, counts=(sum(1 for lst in lists if lst), usable, skipped, chunks),
               no_consensus=int(np.sum(res["status"] == 5)), excluded=int(np.sum(res["inlier"] == 0)))
    return res


def check(got, d, n, r, nt, table, ref, C=ml.C_BOUND):
    """Asserts that the election is the reference's alone (no interval overlaps, nothing in the band under the elected
    hypotheses), then elected, consensus, list lengths, flags and counts exactly, then everything multilat_ref.check asserts, over
    I; returns its worst error / (a + b)."""
    assert ref["ambiguous"] == [], ref["ambiguous"][:5]
    assert ref["band"] == [], ref["band"][:5]
    for key in ("elected", "consensus", "list_len", "inlier"):
        assert np.array_equal(got[key], ref[key]), (key, got[key], ref[key])
    assert got["no_consensus"] == ref["no_consensus"] and got["excluded"] == ref["excluded"]
    return ml.check(got, d, n, r, nt, table, ref, C)


def measure_constant(ctx_of, d, n, r, nt, table, X, pose_ok=None, landmark_on=None):
    """The worst |y_mirror - y_ref| / a_h over every sample of every voted list of a graph: each sample becomes the list of a
    landmark of its own in a graph the plain mirror solves without a Gauss-Newton step (ctx_of(dims): a fresh plan-only handle);
    the origin is the sample's first entry on both sides."""
    rr, rd = np.asarray(table[2]), np.asarray(table[3], dtype=np.float64)
    t0 = d * n + r
    lists, _, _ = ml.lists_of(d, n, r, nt, rr, pose_ok, landmark_on)
    poses, rngs, oms = [], [], []
    for lst in lists:
        if len(lst) < d + 1:
            continue
        for h in range(len(lst)):
            idx = sample(h, len(lst), d)
            poses.append([X[lst[k][0]] for k in idx])
            rngs.append([rd[lst[k][1], 0] for k in idx])
            oms.append([rd[lst[k][1], 1] for k in idx])
    if not poses:
        return 0.0
    P = np.array(poses).reshape(-1, d)
    k = len(poses)
    ranges = [(h * (d + 1) + j, len(P) + h) for h in range(k) for j in range(d + 1)]
    dims, tab, Y = ml.graph(d, P, np.zeros((k, d)), ranges)
    tab[3][:, 0], tab[3][:, 1] = np.array(rngs).ravel(), np.array(oms).ravel()
    ctx = ctx_of(dims)
    ctx.set_measurements(*tab)
    ctx.set_multilateration()
    got = ctx.debug_multilaterate_host(Y, 0)
    tt = dims[0] * dims[1] + dims[2]
    worst = 0.0
    for h in range(k):
        t = np.array(poses[h], dtype=LD)
        hyp = hypothesis(d, t - t[0], np.array(rngs[h], dtype=LD), np.array(oms[h], dtype=LD))
        if not hyp["valid"] or got["status"][h] != 0 or abs(hyp["pivot"] - ml.MIN_PIVOT) < 1e-3 * ml.MIN_PIVOT:
            continue
        y = np.asarray(got["X"][tt + dims[1] + h], dtype=LD) - t[0]
        err = float(np.sqrt(np.sum((y - hyp["y"]) ** 2)))
        rounding = EPS * float(np.sqrt(np.sum((t[0] + hyp["y"]) ** 2)))   # (the row t_0 + y is rounded once more)
        worst = max(worst, max(err - rounding, 0.0) / hyp["a"])
    return worst
