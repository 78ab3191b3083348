"""numpy.longdouble / mpmath reference of the outlier-robust placement from sightings (include/cora_hip.h,
cora_place_by_sightings_robust_dev) -- TEST INFRASTRUCTURE ONLY.  The structure is sighting_ref.structure's.  Per
list: every r(h, j) in longdouble, the votes, the election (largest vote, lowest entry) and the inliers I; then sighting_ref's
exact minimisers (the weighted mean; the weighted Kabsch alignment in mpmath) over the sub-list I, with the origin terms of
the list's actual first entry.  The chain HYPOTHESES (one alignment of d entries per entry of a list, up to 513 per list) are
not worth mpmath: their sums are longdouble, their rotation numpy's float64 singular value decomposition, batched.  They
are only ever thresholded, and the band below is what makes that fair.

The counts are integers and are compared exactly.  That is fair only where no residual sits on the threshold and no
hypothesis sits on the refusal rule: the reference reports in `band` every (h, j) whose r lies in [barc2 / 2, 2 barc2], over all
h and j of every list of every stage, and every hypothesis whose refusal quantity lies within a factor 4 of its threshold; every
test case asserts that `band` is empty.  This is a condition on the inputs, not a measurement.  `classes` is (the largest r
below barc2, the smallest r above it) over everything scored: barc2 is chosen per case as their geometric middle (middle_barc2).

The result has the layout of sighting_ref.reference's, so sighting_ref.check applies: the bound is sighting_ref's, over I."""
import numpy as np

import sighting_ref as sg

LD, EPS = sg.LD, sg.EPS
_lsum, _norm = sg._lsum, sg._norm
# 4 x the worst ratio error / (a + b) of the mirror over the cases of tests/test_sighting_consensus_cpu.py stays below
# sighting_ref.C_BOUND (profiles/sighting_consensus.md), so the constant is sighting_ref's
C_BOUND = sg.C_BOUND
NO_SPREAD = 1e-20    # a centred spread below this share of the uncentred one is none (longdouble rounding is 1e-38 of it)


def default_min_chain_consensus(d):
    return d + 1


def sample(L, d):
    """idx[h, k]: entry k of the sample of entry h in a list of L entries."""
    s = max(1, L // d)
    return (np.arange(L)[:, None] + s * np.arange(d)[None]) % L


def hypotheses(d, pp, ll, tau):
    """(valid [L], R [L, d, d], t' [L, d], margin [L]) of the chain hypotheses of a list in relative coordinates pp, ll
    (longdouble).  margin: the refusal rule's quantity over its threshold (inf: no rule applies, 0: no spread)."""
    L = len(tau)
    idx = sample(L, d)
    P, M, T = pp[idx], ll[idx], tau[idx]
    W = np.sum(T, axis=1)
    valid = W > 0
    Ws = np.where(valid, W, 1)
    cp, cl = np.sum(T[:, :, None] * P, axis=1) / Ws[:, None], np.sum(T[:, :, None] * M, axis=1) / Ws[:, None]
    pc, lc = P - cp[:, None], M - cl[:, None]
    H = np.einsum("hk,hka,hkb->hab", T, lc, pc)
    sp, sl = np.sum(T * np.sum(pc * pc, axis=2), axis=1), np.sum(T * np.sum(lc * lc, axis=2), axis=1)
    up, ul = np.sum(T * np.sum(P * P, axis=2), axis=1), np.sum(T * np.sum(M * M, axis=2), axis=1)
    spread = (sp > NO_SPREAD * up) & (sl > NO_SPREAD * ul) & (sp > 0) & (sl > 0)
    k2 = LD(sg.MIN_SPREAD) ** 2
    with np.errstate(all="ignore"):
        if d == 2:
            margin = np.sum(H * H, axis=(1, 2)) / (k2 * sp * sl)
        else:
            cof = np.stack([np.cross(H[:, 1], H[:, 2]), np.cross(H[:, 2], H[:, 0]), np.cross(H[:, 0], H[:, 1])], axis=1)
            margin = np.sqrt(np.sum(cof * cof, axis=(1, 2))) / (k2 * sp * sl)
    margin = np.where(valid & spread, margin, 0).astype(np.float64)
    valid = valid & spread & (margin > 1)
    U, _, Vt = np.linalg.svd(np.where(valid[:, None, None], H, np.eye(d)).astype(np.float64))
    D = np.tile(np.eye(d), (L, 1, 1))
    D[:, d - 1, d - 1] = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    R = (U @ D @ Vt).astype(LD)
    tr = cl - np.einsum("hab,hb->ha", R, cp)
    return valid, R, tr, margin


def landmark_scores(pp, tau):
    """r[h, j] = tau_j |p'_h - p'_j|^2 (longdouble)."""
    return tau[None] * np.sum((pp[:, None] - pp[None]) ** 2, axis=2)


def chain_scores(R, tr, pp, ll, tau):
    """r[h, j] = tau_j |R_h p'_j + t'_h - l'_j|^2 (longdouble)."""
    pred = np.einsum("hab,jb->hja", R, pp) + tr[:, None] - ll[None]
    return tau[None] * np.sum(pred ** 2, axis=2)


def reference(d, n, r, nt, table, chains, X, barc2, min_chain_consensus=None, min_landmark_consensus=1, chain_fixed=None,
              landmark_fixed=None, min_sightings=None):
    """sighting_ref.reference's dict for the robust call, plus chain_consensus, chain_list_len (per chain), landmark_consensus,
    landmark_list_len (per landmark, the REFIT's), inlier_chain, inlier_landmark (per edge: 1 | 0 | 2), elected (per list: (stage,
    item) -> entry), votes ((stage, item) -> array), the four counts, band and classes."""
    rr = np.asarray(table[2])
    X = np.array(X, dtype=LD)
    S = sg.structure(d, n, r, nt, table, chains, chain_fixed, landmark_fixed, min_sightings)
    nch, nl, t0, ne = len(chains), nt - n, d * n + r, len(table[0])
    mcc = default_min_chain_consensus(d) if not min_chain_consensus or min_chain_consensus <= 0 else min_chain_consensus
    res = dict(struct=S, status=np.array(S["chain_init"], dtype=np.uint8), chosen=np.full(nch, -1, dtype=np.int32),
               cost_start=np.zeros(nch, dtype=LD), cost_final=np.zeros(nch, dtype=LD),
               transforms=np.tile(np.concatenate([np.eye(d).reshape(-1), np.zeros(d)]), (nch, 1)).astype(LD),
               landmark_status=np.array(S["lm_init"], dtype=np.uint8), landmark_cost=np.zeros(nl, dtype=LD), chain={},
               level={}, rot_level={}, round={}, X_before_refit=None,
               chain_consensus=np.zeros(nch, dtype=np.int32), chain_list_len=np.zeros(nch, dtype=np.int32),
               landmark_consensus=np.zeros(nl, dtype=np.int32), landmark_list_len=np.zeros(nl, dtype=np.int32),
               inlier_chain=np.full(ne, 2, dtype=np.uint8), inlier_landmark=np.full(ne, 2, dtype=np.uint8), elected={}, votes={},
               band=[], classes=[0.0, np.inf], landmark_I={})
    level, rot_level = res["level"], res["rot_level"]

    def inherited(rot, trn, tn, Xv):
        return np.array([level.get(int(b), 0.0) + rot_level.get(int(a), 0.0) * float(k) + EPS * (float(_norm(Xv[b])) + float(k))
                         for a, b, k in zip(rot, trn, tn)])

    def vote(key, Rs, valid):
        """The election over the scores Rs[h, j]: (entry, consensus, I); band and classes grow."""
        with np.errstate(invalid="ignore"):
            near = (Rs >= barc2 / 2) & (Rs <= 2 * barc2) & valid[:, None]
            agree = (Rs <= barc2) & valid[:, None]
        res["band"] += [(key, int(h), int(j), float(Rs[h, j])) for h, j in zip(*np.nonzero(near))]
        used = Rs[valid]
        if np.any(used <= barc2):
            res["classes"][0] = max(res["classes"][0], float(used[used <= barc2].max()))
        if np.any(used > barc2):
            res["classes"][1] = min(res["classes"][1], float(used[used > barc2].min()))
        votes = np.sum(agree, axis=1)
        h = int(np.argmax(votes))    # (the first of the largest)
        res["elected"][key], res["votes"][key] = h, votes
        return h, int(votes[h])

    for si, st in enumerate(S["stages"]):
        if st["kind"] == "REFIT":
            res["X_before_refit"] = X.copy()
        if st["kind"] != "C":
            new = {}
            for l, es in st["lists"]:
                p, _, tau, rot, trn, lm, tn = sg.predictions(d, n, r, table, X, es)
                pp = p - p[0]
                Rs = landmark_scores(pp, tau)
                h, cons = vote((si, l), Rs, np.ones(len(es), dtype=bool))
                I = np.nonzero(Rs[h] <= barc2)[0]
                row = t0 + n + l
                if st["kind"] == "REFIT":
                    res["landmark_consensus"][l], res["landmark_list_len"][l] = cons, len(es)
                    res["inlier_landmark"][list(es)] = 0
                    res["inlier_landmark"][[es[j] for j in I]] = 1
                    res["landmark_I"][l] = [es[j] for j in I]
                if cons < min_landmark_consensus:
                    res["landmark_status"][l] = 5
                    continue
                p, tau, rot, trn, tn = (v[I] for v in (p, tau, rot, trn, tn))
                W = _lsum(tau)
                if not W > 0:
                    res["landmark_status"][l] = 2
                    continue
                res["landmark_status"][l] = 0
                new[row] = _lsum(tau[:, None] * p) / W
                dp = inherited(rot, trn, tn, X)
                level[row] = float(dp.max())
                res["round"][row] = EPS * (float(_norm(new[row])) + float(np.sqrt(np.max(np.sum(pp[I] ** 2, axis=1)))))
            for row, x in new.items():
                X[row] = x
            if st["kind"] == "REFIT":
                for l, es in st["lists"]:
                    res["landmark_cost"][l] = sg.sighting_cost(d, n, r, table, X, res["landmark_I"][l])
            continue
        moves = []
        for c, es in st["lists"]:
            p, l, tau, rot, trn, lm, tn = sg.predictions(d, n, r, table, X, es)
            pp, ll = p - p[0], l - l[0]
            valid, Rh, trh, margin = hypotheses(d, pp, ll, tau)
            res["band"] += [((si, c), int(h), -1, float(margin[h])) for h in np.nonzero((margin > 0.25) & (margin < 4))[0]]
            Rs = chain_scores(Rh, trh, pp, ll, tau)
            h, cons = vote((si, c), Rs, valid)
            # an elected hypothesis that is not valid (no valid one in the list) is the refused solve's: the identity
            I = np.nonzero((Rs[h] if valid[h] else tau * np.sum((l - p) ** 2, axis=1)) <= barc2)[0]
            res["chain_consensus"][c], res["chain_list_len"][c] = cons, len(es)
            res["inlier_chain"][list(es)] = 0
            res["inlier_chain"][[es[j] for j in I]] = 1
            start = _lsum(tau[I] * np.sum((l[I] - p[I]) ** 2, axis=1)) if len(I) else LD(0)
            one = dict(es=es, I=I, rows_before={}, R=np.eye(d, dtype=LD), t=np.zeros(d, dtype=LD), a_R=0.0, a_t=0.0, b_t=0.0, sv=None,
                       margin=None, costs=(float(start), float(start)), chosen=False)
            res["chain"][c] = one
            res["cost_start"][c] = res["cost_final"][c] = start
            res["chosen"][c] = 0
            if cons < mcc:
                res["status"][c] = 5
                continue
            p0, l0 = p[0], l[0]     # the origin: the list's first entry, an inlier or not
            p, l, tau, rot, trn, lm, tn = (v[I] for v in (p, l, tau, rot, trn, lm, tn))
            W = _lsum(tau)
            ok = bool(W > 0)
            if ok:
                cp, cl = _lsum(tau[:, None] * p) / W, _lsum(tau[:, None] * l) / W
                pc, lc = p - cp, l - cl
                H = _lsum(tau[:, None, None] * lc[:, :, None] * pc[:, None, :])
                sp, sl = _lsum(tau * np.sum(pc * pc, axis=1)), _lsum(tau * np.sum(lc * lc, axis=1))
                up, ul = _lsum(tau * np.sum((p - p0) ** 2, axis=1)), _lsum(tau * np.sum((l - l0) ** 2, axis=1))
                ok = bool(sp > NO_SPREAD * up and sl > NO_SPREAD * ul) and not sg.refused(d, H, W, sp, sl)
                if ok:
                    R, sv = sg.kabsch(H)
                    one["sv"] = sv
            if not ok:
                res["status"][c] = 2
                continue
            res["status"][c] = 0
            t = cl - R @ cp
            final = _lsum(tau * np.sum((l - (p @ R.T + t)) ** 2, axis=1))
            Lp, Ll = float(np.sqrt(up / W)), float(np.sqrt(ul / W))
            delta = float((inherited(rot, trn, tn, X) + np.array([level.get(int(b), 0.0) for b in lm])).max())
            gap = (sv[0] + sv[1]) if d == 2 else (sv[1] + sv[2])
            dH = EPS * float(W) * Lp * Ll + float(W) * (Lp + Ll) * delta
            one.update(R=R, t=t, cp=cp, cl=cl, a_R=dH / gap, a_t=2 * delta + EPS * (Lp + Ll), kappa=float(W) * Lp * Ll / gap,
                       b_t=EPS * float(_norm(p0) + _norm(l0) + _norm(t) + _norm(cp) + _norm(cl)), chosen=bool(final < start),
                       costs=(float(start), float(final)))
            res["chosen"][c] = 1 if final < start else 0
            if final < start:
                res["cost_final"][c] = final
                res["transforms"][c] = np.concatenate([R.reshape(-1), t])
                moves.append((c, R, t))
        for c, R, t in moves:
            one = res["chain"][c]
            for rot, trn in S["positions"][c]:
                x = X[trn].copy()
                one["rows_before"][trn] = (x, X[rot:rot + d].copy())
                xn = R @ x + t
                X[rot:rot + d] = X[rot:rot + d] @ R.T
                X[trn] = xn
                level[trn] = level.get(trn, 0.0) + one["a_R"] * float(_norm(x - one["cp"])) + one["a_t"]
                rot_level[rot] = rot_level.get(rot, 0.0) + one["a_R"] + 4 * EPS
                res["round"][trn] = one["b_t"] + EPS * float(_norm(x) + _norm(xn))
    if res["X_before_refit"] is None:
        res["X_before_refit"] = X.copy()
    deg, norm = np.zeros(len(rr), dtype=bool), np.zeros(len(rr), dtype=LD)
    for m in range(len(rr)):
        diff = X[rr[m, 2]] - X[rr[m, 1]]
        nrm = norm[m] = np.sqrt(np.sum(diff * diff))
        deg[m] = nrm < 1e-5
        X[rr[m, 0]] = 0 if deg[m] else -diff / nrm   # towards a: the direction of least residual
    res.update(X=X, degenerate=deg, norm=norm, chains_no_consensus=int(np.sum(res["status"] == 5)),
               landmarks_no_consensus=int(np.sum(res["landmark_status"] == 5)), chain_excluded=int(np.sum(res["inlier_chain"] == 0)),
               landmark_excluded=int(np.sum(res["inlier_landmark"] == 0)))
    return res


def middle_barc2(classes):
    """The geometric middle of the two residual classes; the lower one is at least the square of the rounding of a metre."""
    lo, hi = max(classes[0], EPS * EPS), classes[1]
    assert np.isfinite(hi) and hi > 1e6 * lo, classes
    return float(np.sqrt(lo * hi))


INTEGERS = ("chain_consensus", "chain_list_len", "landmark_consensus", "landmark_list_len", "inlier_chain", "inlier_landmark")
COUNTS = ("chains_no_consensus", "landmarks_no_consensus", "chain_excluded", "landmark_excluded")


def check(got, d, n, r, nt, table, ref):
    """The band is empty; the integer results equal the reference's exactly; then sighting_ref.check (statuses, counts, chosen,
    the transforms and every written row within the bound over I).  Returns the worst error / (a + b)."""
    assert ref["band"] == [], ref["band"][:8]
    for key in INTEGERS:
        assert np.array_equal(got[key], ref[key]), (key, got[key], ref[key])
    for key in COUNTS:
        assert got[key] == ref[key], (key, got[key], ref[key])
    # the landmarks' cost is a sum over I at the row as it stands, written or not (status 5, 2: sighting_ref.check wants 0 there)
    lc = np.asarray(got["landmark_cost"])
    for l in range(nt - n):
        want = float(ref["landmark_cost"][l])
        if ref["landmark_status"][l] != 0:
            assert abs(lc[l] - want) <= 1e-9 * want + 1e-300, (l, lc[l], want)
    return sg.check(dict(got, landmark_cost=np.where(ref["landmark_status"] == 0, lc, 0.0)), d, n, r, nt, table, ref, C=C_BOUND)


def spoil(d, table, edges, rng, relabel=True, rows=None):
    """The sightings `edges` of the table made wrong, in place: re-labelled (relabel) to another landmark row among `rows`
    (None: the rows the table's sightings name), or their t moved by 2 .. 8 m per axis, either sign."""
    er, ed = table[0], table[1]
    rows = np.unique(er[er[:, 1] < 0, 3]) if rows is None else np.asarray(rows)
    for e in edges:
        if relabel:
            others = rows[rows != er[e, 3]]
            er[e, 3] = int(others[int(rng.integers(len(others)))])
        else:
            ed[e, d * d:d * d + d] += rng.uniform(2, 8, d) * rng.choice([-1.0, 1.0], d)


def start_world(d=2, seed=11, robots=(("A", 30), ("B", 30), ("C", 30), ("D", 30)), n_lm=12, per_robot=36, contaminated=True):
    """A topologies.World of four robots and 12 landmarks with EXACT odometry and exact sightings (so that the residuals under
    a clean hypothesis are rounding, and the two residual classes are far apart): every robot sights every landmark three times
    (36 sightings, from distinct (pose, landmark) pairs); then, per robot, one wrong-id sighting per five true ones is APPENDED
    (contaminated): a pose sees landmark a and the measurement is credited to landmark b.  The wrong sightings are the last
    entries of every list they enter.  Returns (world, true sightings, wrong sightings)."""
    import topologies as tp
    w = tp.World(d, seed)
    idxs = [w.robot(c, n) for c, n in robots]
    lms = w.landmarks(n_lm)
    for idx in idxs:
        for i, j in zip(idx[:-1], idx[1:]):
            w.g.rpms.append((w.names[i], w.names[j], w.R[i].T @ w.R[j], w.R[i].T @ (w.T[j] - w.T[i]), w.cov))
    used, true, wrong = set(), [], []
    for idx in idxs:
        for k in range(per_robot):
            lm = lms[k % n_lm]
            i = int(w.rng.choice(idx))
            while (i, lm) in used:
                i = int(w.rng.choice(idx))
            used.add((i, lm))
            true.append((i, lm, lm))
    for idx in idxs:
        for k in range(per_robot // 5):
            while True:
                i = int(w.rng.choice(idx))
                a, b = (lms[int(x)] for x in w.rng.choice(n_lm, 2, replace=False))
                if (i, a) not in used and (i, b) not in used:
                    break
            used.update([(i, a), (i, b)])
            wrong.append((i, a, b))
    for i, seen, credited in true + (wrong if contaminated else []):
        w.g.rplms.append((w.names[i], credited, w.R[i].T @ (w.pos[seen] - w.T[i]), w.covt))
    return w, len(true), len(wrong)


def standin_start(w, robots=4, per=30, seed=3):
    """A stand-in for the odometry start of start_world's graph: the truth with every chain after the first in a random frame
    of its own and the landmarks at random places (exact odometry composes to exactly this, up to rounding and the draws)."""
    rng = np.random.default_rng(seed)
    d, n = w.d, len(w.names)
    X = w.truth()
    t0 = d * n + len(w.g.ranges)
    for c in range(1, robots):
        Rc, tc = sg.pl._rot(d, rng, 2.5), 10 * rng.uniform(-1, 1, d)
        for i in range(per * c, per * (c + 1)):
            X[d * i:d * i + d] = X[d * i:d * i + d] @ Rc
            X[t0 + i] = Rc.T @ (X[t0 + i] - tc)
    X[t0 + n:] = 10 * rng.uniform(-1, 1, (len(w.L), d))
    return X


def built_flags(w, table, chains, n_true):
    """(inlier_chain, inlier_landmark) as start_world built them: a sighting by chain 0 is in no C list; the true sightings are
    inliers, the appended ones are not; every other edge is in no list."""
    er = np.asarray(table[0])
    first = len(er) - len(w.g.rplms)
    d, n = w.d, len(w.names)
    t0 = d * n + len(w.g.ranges)
    chain0 = {int(er[e, 3]) for e in chains[0]} | {int(er[chains[0][0], 2])}
    ic, il = np.full(len(er), 2, dtype=np.uint8), np.full(len(er), 2, dtype=np.uint8)
    for e in range(first, len(er)):
        il[e] = 1 if e - first < n_true else 0
        if int(er[e, 2]) not in chain0:
            ic[e] = il[e]
    return ic, il


def write_pyfg(w, path):
    """A d = 2 World of poses, landmarks, relative poses and sightings as PyFG text, the vertices at the truth."""
    g = w.g
    assert g.dim == 2 and not g.pose_priors and not g.ranges
    with open(path, "w") as f:
        for i, s in enumerate(w.names):
            f.write("VERTEX_SE2 %d.0 %s %.17g %.17g %.17g\n" % (i, s, w.T[i][0], w.T[i][1], np.arctan2(w.R[i][1, 0], w.R[i][0, 0])))
        for s, l in sorted(g.landmarks.items(), key=lambda kv: kv[1]):
            f.write("VERTEX_XY %s %.17g %.17g\n" % (s, w.L[l][0], w.L[l][1]))
        for i, (a, b, R, t, cov) in enumerate(g.rpms):
            up = " ".join("%.17g" % cov[r, c] for r in range(3) for c in range(r, 3))
            f.write("EDGE_SE2 %d.0 %s %s %.17g %.17g %.17g %s\n" % (i, a, b, t[0], t[1], np.arctan2(R[1, 0], R[0, 0]), up))
        for i, (a, b, t, cov) in enumerate(g.rplms):
            f.write("EDGE_SE2_XY %d.0 %s %s %.17g %.17g %.17g %.17g %.17g\n" % (i, a, b, t[0], t[1], cov[0, 0], cov[0, 1], cov[1, 1]))


__all__ = ["reference", "check", "spoil", "middle_barc2", "hypotheses", "sample", "start_world", "standin_start", "built_flags", "write_pyfg", "C_BOUND", "sg"]
