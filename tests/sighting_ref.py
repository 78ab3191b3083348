"""numpy.longdouble / mpmath reference of the placement from pose-landmark sightings (include/cora_hip.h,
cora_place_by_sightings_dev) -- TEST INFRASTRUCTURE ONLY.  The same structural decisions in plain Python (the sightings, the
alternating L- and C-stages, the REFIT, the lists in table order) and the exact minimisers: the weighted mean of the
predictions for a landmark, the weighted Kabsch alignment (singular value decomposition in mpmath, the determinant's sign on
the least singular value) for a chain, plain left-to-right sums, then the unit range rows of all range measurements.

Bound (derived, its constant measured: profiles/sighting_placement.md).  Every translation row carries an error level, every
pose block a rotation error level; the caller's rows carry none.  A prediction p = x_t(a) + R_a t inherits
dp = level(x_t(a)) + rot_level(a) |t| + eps (|x_t(a)| + |t|).
  landmark   the weighted mean is a convex combination: level = max dp + eps (|x| + max |p - p_0|).
  chain      with W = sum tau, L_p^2 = sum tau |p - p_0|^2 / W, L_l likewise and delta = max (dp + level(l)), the matrix H
             (size W L_p L_l) is perturbed by dH = eps W L_p L_l + W (L_p + L_l) delta.  The rotation of the alignment moves by
             dH / g with the gap g = s_1 + s_2' (d = 2), s_2 + s_3' (d = 3) of H's singular values (the last one signed by the
             determinant): the CONDITION of the alignment is W L_p L_l / g.  a_R = dH / g; the translation about the centroid
             moves by a_t = 2 delta + eps (L_p + L_l); a row R (x - c_p) + c_l by a_R |x - c_p| + a_t, and is rounded:
             b = eps (|p_0| + |l_0| + |t| + |x| + |x_new|).
error <= C a + b with C = C_BOUND for every written row and transform."""
import mpmath
import numpy as np

import multilat_ref as ml
import placement_ref as pl

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
CHUNK = 256          # kSgChunk
MIN_SPREAD = 1e-6    # kSgMinSpread
C_BOUND = 1.34       # 4 x the worst ratio error / (a + b) of the mirror over the cases of tests/test_sighting_cpu.py (0.3345, profiles/sighting_placement.md)

bits, diagonal_q = ml.bits, ml.diagonal_q
_lsum, _norm = ml._lsum, pl._norm


def default_min_sightings(d):
    return 4 * d


def structure(d, n, r, nt, table, chains, chain_fixed=None, landmark_fixed=None, min_sightings=None):
    """dict stages (list of dict kind "L" | "C" | "REFIT", lists: [(item, [edges in table order])]), chain_init (0 taken | 1 |
    3 | 4 fixed), lm_init (0 in the REFIT | 1 | 3 fixed), skipped, positions (per chain: (first rotation row, translation
    row)), counts (stages, entries, chunks, skipped), order."""
    er = np.asarray(table[0])
    ms = default_min_sightings(d) if min_sightings is None else min_sightings
    nch, nl, t0 = len(chains), nt - n, d * n + r
    positions, chain_of = [], {}
    for c, ch in enumerate(chains):
        pos = [(int(er[ch[0], 0]), int(er[ch[0], 2]))] + [(int(er[e, 1]), int(er[e, 3])) for e in ch]
        positions.append(pos)
        for _, trn in pos:
            chain_of[trn] = c
    placed = [c == 0 for c in range(nch)] if chain_fixed is None else [bool(f) for f in chain_fixed]
    fixed_c = list(placed)
    lm_fixed = [False] * nl if landmark_fixed is None else [bool(f) for f in landmark_fixed]
    lm_placed = list(lm_fixed)
    sights, skipped = [], 0
    for e in range(len(er)):
        if er[e, 1] >= 0:
            continue
        c, l = chain_of.get(int(er[e, 2]), -1), int(er[e, 3]) - t0 - n
        if c < 0 or l < 0:
            skipped += 1
            continue
        sights.append((e, c, l))
    stages, taken_c = [], set()

    def landmark_stage(kind, want):
        lists = [(l, [e for e, c, ll in sights if ll == l and placed[c]]) for l in range(nl) if want[l]]
        lists = [(l, es) for l, es in lists if es]
        if lists:
            stages.append(dict(kind=kind, lists=lists))
        return [l for l, _ in lists]

    while sights:
        lms = landmark_stage("L", [not p for p in lm_placed])
        for l in lms:
            lm_placed[l] = True
        lists = []
        for c in range(nch):
            if placed[c]:
                continue
            es = [(e, l) for e, cc, l in sights if cc == c and lm_placed[l]]
            if len(es) >= ms and len({l for _, l in es}) >= d:
                lists.append((c, [e for e, _ in es]))
        if lists:
            stages.append(dict(kind="C", lists=lists))
        for c, _ in lists:
            placed[c] = True
            taken_c.add(c)
        if not lms and not lists:
            break
    refit = landmark_stage("REFIT", [not f for f in lm_fixed])
    sees = {c for _, c, _ in sights}
    chain_init = [0 if c in taken_c else (4 if fixed_c[c] else (1 if c in sees else 3)) for c in range(nch)]
    lm_init = [3 if lm_fixed[l] else (0 if l in refit else 1) for l in range(nl)]
    entries = sum(len(es) for st in stages for _, es in st["lists"])
    chunks = sum((len(es) + CHUNK - 1) // CHUNK for st in stages for _, es in st["lists"])
    return dict(stages=stages, chain_init=chain_init, lm_init=lm_init, skipped=skipped, positions=positions, placed=placed,
                counts=(len(stages), entries, chunks, skipped), order=[(st["kind"], [i for i, _ in st["lists"]]) for st in stages])


def _mp(x):
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def kabsch(H):
    """(R, singular values with the last one signed by the determinant) of the d x d longdouble H: the rotation that
    maximises tr(R^T H), by mpmath's singular value decomposition at 50 digits."""
    d = H.shape[0]
    with mpmath.workdps(50):
        U, S, V = mpmath.svd_r(mpmath.matrix([[_mp(H[i, j]) for j in range(d)] for i in range(d)]))
        sign = 1 if mpmath.det(U) * mpmath.det(V) >= 0 else -1
        D = mpmath.eye(d)
        D[d - 1, d - 1] = sign
        R = U * D * V
        Rn = np.array([[LD(float(R[i, j])) + LD(float(R[i, j] - mpmath.mpf(float(R[i, j])))) for j in range(d)] for i in range(d)], dtype=LD)
        sv = [float(S[i]) for i in range(d)]
    sv[-1] *= sign
    return Rn, sv


def predictions(d, n, r, table, X, es):
    """(p, l, tau, rot rows, trn rows, lm rows, |t|) of the edges es at the vector X (longdouble)."""
    er, ed = np.asarray(table[0]), np.asarray(table[1], dtype=np.float64)
    es = np.asarray(es, dtype=np.int64)
    t = ed[es, d * d:d * d + d].astype(LD)
    rot, trn, lm = er[es, 0], er[es, 2], er[es, 3]
    p = X[trn].copy()
    for c in range(d):
        p = p + t[:, c:c + 1] * X[rot + c]
    return p, X[lm], ed[es, d * d + d + 1].astype(LD), rot, trn, lm, np.sqrt(np.sum(t * t, axis=1))


def sighting_cost(d, n, r, table, X, es):
    """sum tau |x_t(l) - p|^2 over the edges es, longdouble, left to right."""
    if len(es) == 0:
        return LD(0)
    p, l, tau, *_ = predictions(d, n, r, table, np.asarray(X, dtype=LD), es)
    return _lsum(tau * np.sum((l - p) ** 2, axis=1))


def refused(d, H, W, sp, sl):
    """The refusal rule of the header, on the exact sums."""
    if not W > 0 or not sp > 0 or not sl > 0:
        return True
    k2 = LD(MIN_SPREAD) ** 2
    if d == 2:
        return not np.sum(H * H) > k2 * sp * sl
    cof = np.array([np.cross(H[1], H[2]), np.cross(H[2], H[0]), np.cross(H[0], H[1])], dtype=LD)
    return not np.sum(cof * cof) > (k2 * sp * sl) ** 2


def reference(d, n, r, nt, table, chains, X, chain_fixed=None, landmark_fixed=None, min_sightings=None):
    """dict X (N x d longdouble), struct, status, chosen, cost_start, cost_final, transforms (per chain), landmark_status,
    landmark_cost, chain (per taken chain: dict with R, t, a_R, a_t, b_t, sv, margin, rows_before), level / rot_level (per
    row: the bound's a without C), round (per row: b), X_before_refit, degenerate, norm."""
    rr = np.asarray(table[2])
    X = np.array(X, dtype=LD)
    S = structure(d, n, r, nt, table, chains, chain_fixed, landmark_fixed, min_sightings)
    nch, nl, G, t0 = len(chains), nt - n, d * d + d, d * n + r
    res = dict(struct=S, status=np.array(S["chain_init"], dtype=np.uint8), chosen=np.full(nch, -1, dtype=np.int32),
               cost_start=np.zeros(nch, dtype=LD), cost_final=np.zeros(nch, dtype=LD),
               transforms=np.tile(np.concatenate([np.eye(d).reshape(-1), np.zeros(d)]), (nch, 1)).astype(LD),
               landmark_status=np.array(S["lm_init"], dtype=np.uint8), landmark_cost=np.zeros(nl, dtype=LD), chain={},
               level={}, rot_level={}, round={}, X_before_refit=None)
    level, rot_level = res["level"], res["rot_level"]

    def inherited(rot, trn, tn, Xv):
        return np.array([level.get(int(b), 0.0) + rot_level.get(int(a), 0.0) * float(k) + EPS * (float(_norm(Xv[b])) + float(k))
                         for a, b, k in zip(rot, trn, tn)])

    for st in S["stages"]:
        if st["kind"] == "REFIT":
            res["X_before_refit"] = X.copy()
        if st["kind"] != "C":
            new = {}
            for l, es in st["lists"]:
                p, _, tau, rot, trn, lm, tn = predictions(d, n, r, table, X, es)
                W = _lsum(tau)
                row = t0 + n + l
                if not W > 0:
                    res["landmark_status"][l] = 2
                    continue
                res["landmark_status"][l] = 0
                new[row] = _lsum(tau[:, None] * p) / W
                dp = inherited(rot, trn, tn, X)
                level[row] = float(dp.max())
                res["round"][row] = EPS * (float(_norm(new[row])) + float(np.sqrt(np.max(np.sum((p - p[0]) ** 2, axis=1)))))
            for row, x in new.items():
                X[row] = x
            if st["kind"] == "REFIT":
                for l, es in st["lists"]:
                    res["landmark_cost"][l] = sighting_cost(d, n, r, table, X, es)
            continue
        moves = []
        for c, es in st["lists"]:
            p, l, tau, rot, trn, lm, tn = predictions(d, n, r, table, X, es)
            W = _lsum(tau)
            one = dict(es=es, rows_before={}, R=np.eye(d, dtype=LD), t=np.zeros(d, dtype=LD), a_R=0.0, a_t=0.0, b_t=0.0, sv=None, margin=None)
            res["chain"][c] = one
            start = _lsum(tau * np.sum((l - p) ** 2, axis=1))
            res["cost_start"][c] = res["cost_final"][c] = start
            res["chosen"][c] = 0
            ok = bool(W > 0)
            if ok:
                cp, cl = _lsum(tau[:, None] * p) / W, _lsum(tau[:, None] * l) / W
                pc, lc = p - cp, l - cl
                H = _lsum(tau[:, None, None] * lc[:, :, None] * pc[:, None, :])
                sp, sl = _lsum(tau * np.sum(pc * pc, axis=1)), _lsum(tau * np.sum(lc * lc, axis=1))
                ok = not refused(d, H, W, sp, sl)
                if sp > 0 and sl > 0:
                    R, sv = kabsch(H)
                    one["sv"] = sv
                    # the rule's quantity over its threshold, from the singular values
                    if d == 2:
                        one["margin"] = float((sv[0] ** 2 + sv[1] ** 2) / (LD(MIN_SPREAD) ** 2 * sp * sl))
                    else:
                        e2 = sv[0] ** 2 * sv[1] ** 2 + sv[0] ** 2 * sv[2] ** 2 + sv[1] ** 2 * sv[2] ** 2
                        one["margin"] = float(np.sqrt(LD(e2)) / (LD(MIN_SPREAD) ** 2 * sp * sl))
            if not ok:
                res["status"][c] = 2
                continue
            res["status"][c] = 0
            t = cl - R @ cp
            final = _lsum(tau * np.sum((l - (p @ R.T + t)) ** 2, axis=1))
            res["cost_final"][c] = final
            Lp, Ll = float(np.sqrt(_lsum(tau * np.sum((p - p[0]) ** 2, axis=1)) / W)), float(np.sqrt(_lsum(tau * np.sum((l - l[0]) ** 2, axis=1)) / W))
            delta = float((inherited(rot, trn, tn, X) + np.array([level.get(int(b), 0.0) for b in lm])).max())
            gap = (sv[0] + sv[1]) if d == 2 else (sv[1] + sv[2])
            dH = EPS * float(W) * Lp * Ll + float(W) * (Lp + Ll) * delta
            one.update(R=R, t=t, cp=cp, cl=cl, a_R=dH / gap, a_t=2 * delta + EPS * (Lp + Ll), kappa=float(W) * Lp * Ll / gap,
                       b_t=EPS * float(_norm(p[0]) + _norm(l[0]) + _norm(t) + _norm(cp) + _norm(cl)), chosen=bool(final < start),
                       costs=(float(start), float(final)))
            res["chosen"][c] = 1 if final < start else 0
            if final < start:
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
    res.update(X=X, degenerate=deg, norm=norm)
    return res


def check(got, d, n, r, nt, table, ref, C=C_BOUND):
    """Asserts the statuses, the counts, chosen (where the reference's costs decide it), the degenerate flags, never-worse,
    and the transforms and every written row within the bound; untouched rows keep the caller's bits.  Returns the worst
    error / (a + b) seen (0 where nothing was written)."""
    rr = np.asarray(table[2])
    S = ref["struct"]
    t0 = d * n + r
    assert np.array_equal(got["status"], ref["status"]), (got["status"], ref["status"])
    assert np.array_equal(got["landmark_status"], ref["landmark_status"]), (got["landmark_status"], ref["landmark_status"])
    assert got["stages"] == len(S["stages"])
    assert got["placed"] == int(np.sum(ref["status"] == 0)) and got["not_placed"] == int(np.sum(np.isin(ref["status"], (1, 2, 3))))
    assert got["landmarks_placed"] == int(np.sum(ref["landmark_status"] == 0))
    assert got["landmarks_not_placed"] == int(np.sum(np.isin(ref["landmark_status"], (1, 2))))
    worst = 0.0
    ident = np.concatenate([np.eye(d).reshape(-1), np.zeros(d)])
    Xg = np.asarray(got["X"], dtype=LD)
    moved = set()
    for c in range(len(S["chain_init"])):
        one = ref["chain"].get(c)
        if one is None:
            assert got["chosen"][c] == -1 and got["cost_start"][c] == 0 and got["cost_final"][c] == 0
        else:
            assert got["cost_final"][c] <= got["cost_start"][c], (c, got["cost_final"][c], got["cost_start"][c])   # never worse, as doubles
        if one is None or ref["status"][c] == 2:
            if one is not None:
                assert got["chosen"][c] == 0 and got["cost_final"][c] == got["cost_start"][c]
            pick = 0
        else:
            start, final = one["costs"]
            # the order of the two costs is the algorithm's only where they differ by more than their rounding
            floor = 1e-9 * max(start, final) + 1e-300
            pick = int(got["chosen"][c])
            if abs(start - final) > floor:
                assert pick == int(one["chosen"]), (c, pick, one["costs"])
            if not pick:
                assert got["cost_final"][c] == got["cost_start"][c]
        if not pick:
            assert np.array_equal(got["transforms"][c], ident)
            for rot, trn in S["positions"][c]:   # a chain that is not moved keeps the caller's bits
                assert np.array_equal(bits(got["X"][trn]), bits(got["X_in"][trn])) and np.array_equal(bits(got["X"][rot:rot + d]), bits(got["X_in"][rot:rot + d]))
            continue
        R, t = one["R"], one["t"]
        gR, gt = np.asarray(got["transforms"][c][:d * d], dtype=LD).reshape(d, d), np.asarray(got["transforms"][c][d * d:], dtype=LD)
        err_R, err_t = float(_norm(gR - R)), float(_norm(gt - t))
        a_T = one["a_R"] * float(_norm(one["cp"])) + one["a_t"]
        assert err_R <= C * one["a_R"] + 4 * EPS, ("rotation of chain %d" % c, err_R, C * one["a_R"])
        assert err_t <= C * a_T + one["b_t"], ("translation of chain %d" % c, err_t, C * a_T, one["b_t"])
        worst = max(worst, err_R / (one["a_R"] + 4 * EPS), err_t / (a_T + one["b_t"]))
        if not one["chosen"]:
            continue   # (a tie the reference broke the other way: its rows are the caller's)
        for rot, trn in S["positions"][c]:
            moved.add(trn)
            a, b = ref["level"][trn], ref["round"][trn]
            err = float(_norm(Xg[trn] - ref["X"][trn]))
            assert err <= C * a + b, ("translation row %d of chain %d" % (trn, c), err, C * a + b)
            worst = max(worst, err / (a + b))
            err = float(_norm(Xg[rot:rot + d] - ref["X"][rot:rot + d]))
            assert err <= C * ref["rot_level"][rot] + 8 * EPS, ("rotation block %d of chain %d" % (rot, c), err)
    for l in range(nt - n):
        row = t0 + n + l
        if ref["landmark_status"][l] != 0:
            assert np.array_equal(bits(got["X"][row]), bits(got["X_in"][row])) and got["landmark_cost"][l] == 0
            continue
        moved.add(row)
        a, b = ref["level"][row], ref["round"][row]
        err = float(_norm(Xg[row] - ref["X"][row]))
        assert err <= C * a + b, ("landmark %d" % l, err, C * a + b)
        worst = max(worst, err / (a + b))
    assert np.array_equal(got["degenerate"], ref["degenerate"]) and got["n_degenerate"] == int(ref["degenerate"].sum())
    for m in range(len(rr)):
        row = Xg[rr[m, 0]]
        if ref["degenerate"][m]:
            assert not row.any()
            continue
        bound = 0.0
        for k in (1, 2):
            if int(rr[m, k]) in moved:
                bound += C * ref["level"][int(rr[m, k])] + ref["round"][int(rr[m, k])]
        assert float(_norm(row - ref["X"][rr[m, 0]])) <= bound / float(ref["norm"][m]) + 4 * EPS, ("range row of measurement %d" % m)
    return worst


def scene(d, lens, sights, seed, n_free=0, n_lm=0, noise=0.0, ranges=(), lm_world=None, moved=True, tau=None, offset=0.0, world=None,
          known=(), pose_sights=()):
    """The scene of placement_ref.scene (chains of lens[c] poses, every chain after the first in a frame of its own, n_free
    free poses, n_lm landmarks) plus one edge without a second rotation per (pose, landmark) of `sights`, in that order after
    the odometry edges: the landmark's world position in the pose's frame, plus `noise` (a free pose may sight too: a
    landmark prior is such an edge from the origin pose); then one such edge per (pose, pose) of `pose_sights`.  The
    landmarks' rows of X are random except those of `known`, which hold the truth.  Returns (dims, table, X, chains, truth,
    landmarks' true positions)."""
    rng = np.random.default_rng(1000 + seed)
    dims, table, X, chains, truth = pl.scene(d, lens, list(ranges), seed, n_free=n_free, n_lm=n_lm, moved=moved, offset=offset, world=world)
    _, n, r, nt = dims
    t0 = d * n + r
    first = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    if lm_world is not None:
        X[t0 + n:] = np.asarray(lm_world) + offset
    lm_true = X[t0 + n:].copy()
    Rw, Tw = np.zeros((n, d, d)), np.zeros((n, d))
    for i in range(n):
        c = int(np.searchsorted(first, i, side="right")) - 1
        Rc, tc = truth[c] if c < len(lens) else (np.eye(d), np.zeros(d))
        Rw[i], Tw[i] = Rc @ X[d * i:d * i + d].T, Rc @ X[t0 + i] + tc
    er, ed = [list(row) for row in table[0]], [list(row) for row in table[1]]
    for k, (i, j) in enumerate(sights):
        t = Rw[i].T @ (lm_true[j] - Tw[i]) + noise * rng.normal(0, 1, d)
        er.append([d * i, -1, t0 + i, t0 + n + j])
        ed.append(list(np.concatenate([np.zeros(d * d), t, [0.0, 1.0 if tau is None else tau[k]]])))
    for i, k in pose_sights:
        er.append([d * i, -1, t0 + i, t0 + k])
        ed.append(list(np.concatenate([np.zeros(d * d), Rw[i].T @ (Tw[k] - Tw[i]), [0.0, 1.0]])))
    for l in range(n_lm):
        if l not in known:
            X[t0 + n + l] = 10 * rng.uniform(-1, 1, d) + offset
    table = (np.array(er, dtype=np.int32).reshape(-1, 4), np.array(ed).reshape(-1, d * d + d + 2), table[2], table[3])
    return dims, table, X, chains, truth, lm_true
