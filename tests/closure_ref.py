"""numpy.longdouble / mpmath reference of the placement from inter-chain relative-pose edges (include/cora_hip.h,
cora_place_by_closures_dev) -- TEST INFRASTRUCTURE ONLY.  The same structural decisions in plain Python (the closures, the
breadth-first stages, the lists in table order) and the exact minimiser of a list's closure cost J(G, s) = sum kappa |G - P|^2
+ sum tau |G q + s - l|^2: H = sum kappa P + sum tau (l - c_l)(q - c_q)^T about the weighted centroids, G by the weighted
Kabsch alignment (singular value decomposition in mpmath, the determinant's sign on the least singular value), s = c_l - G c_q
(W = 0: s = l_0 - G q_0), plain left-to-right sums, then the unit range rows of all range measurements.

Bound (derived, its constant measured: profiles/closure_placement.md).  Every translation row carries an error level, every
pose block a rotation error level; the caller's rows carry none.  Of an entry, x_t(a) + R_a t inherits
dp = level(x_t(a)) + rot_level(a) |t| + eps (|x_t(a)| + |t|), x_t(b) inherits level(x_t(b)), and P inherits
dP = rot_level(a) + rot_level(b) + 4 eps sqrt(d).  With W = sum tau, K = sum kappa, L_q^2 = sum tau |q - q_0|^2 / W, L_l
likewise and delta = max (dp + level(x_t(b))), the matrix H (size S = K sqrt(d) + W L_q L_l) is perturbed by
dH = eps S + K max dP + W (L_q + L_l) delta.  The rotation moves by dH / g with the gap g = s_1 + s_2' (d = 2), s_2 + s_3'
(d = 3) of H's singular values (the last one signed by the determinant): the CONDITION of the alignment is S / g.
a_R = dH / g; the translation about the centroid moves by a_t = 2 delta + eps (L_q + L_l); a row G (x - c_q) + c_l by
a_R |x - c_q| + a_t, and is rounded: b = eps (|q_0| + |l_0| + |s| + |x| + |x_new|).
error <= C a + b with C = C_BOUND for every written row and transform."""
import mpmath
import numpy as np

import multilat_ref as ml
import placement_ref as pl

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
CHUNK = 256        # kClChunk
MIN_RANK = 1e-6    # kClMinRank
C_BOUND = 1.10     # 4 x the worst ratio error / (a + b) of the mirror over the cases of tests/test_closure_cpu.py (0.2738, profiles/closure_placement.md)

bits, diagonal_q = ml.bits, ml.diagonal_q
_lsum, _norm = ml._lsum, pl._norm


def structure(d, n, r, nt, table, chains, chain_fixed=None, min_closures=1):
    """dict stages (list of lists [(chain, [(edge, dir)] in table order)]), chain_init (0 taken | 1 | 3 | 4 fixed), skipped,
    unused, positions (per chain: (first rotation row, translation row)), counts (stages, entries, chunks, skipped + unused),
    order."""
    er = np.asarray(table[0])
    nch = len(chains)
    positions, chain_of, chain_edge = [], {}, set()
    for c, ch in enumerate(chains):
        pos = [(int(er[ch[0], 0]), int(er[ch[0], 2]))] + [(int(er[e, 1]), int(er[e, 3])) for e in ch]
        positions.append(pos)
        chain_edge.update(int(e) for e in ch)
        for _, trn in pos:
            chain_of[trn] = c
    placed = [c == 0 for c in range(nch)] if chain_fixed is None else [bool(f) for f in chain_fixed]
    fixed = list(placed)
    closures, skipped = [], 0
    for e in range(len(er)):
        if er[e, 1] < 0 or e in chain_edge:
            continue
        a, b = chain_of.get(int(er[e, 2]), -1), chain_of.get(int(er[e, 3]), -1)
        if a < 0 or b < 0 or a == b:
            skipped += 1
            continue
        closures.append((e, a, b))
    stages, taken, used = [], set(), 0
    while True:
        lists = []
        for c in range(nch):
            if placed[c]:
                continue
            es = [(e, 1 if a == c else 0) for e, a, b in closures if (a == c and placed[b]) or (b == c and placed[a])]
            if es and len(es) >= min_closures:
                lists.append((c, es))
        if not lists:
            break
        stages.append(lists)
        for c, es in lists:
            placed[c] = True
            taken.add(c)
            used += len(es)
    has = {a for _, a, _ in closures} | {b for _, _, b in closures}
    chain_init = [4 if fixed[c] else (0 if c in taken else (1 if c in has else 3)) for c in range(nch)]
    chunks = sum((len(es) + CHUNK - 1) // CHUNK for st in stages for _, es in st)
    unused = len(closures) - used
    return dict(stages=stages, chain_init=chain_init, skipped=skipped, unused=unused, positions=positions,
                counts=(len(stages), used, chunks, skipped + unused), order=[[c for c, _ in st] for st in stages])


def _mp(x):
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def kabsch(H):
    """(G, singular values with the last one signed by the determinant) of the d x d longdouble H: the rotation that
    maximises tr(G^T H), by mpmath's singular value decomposition at 50 digits."""
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


def entries(d, table, X, es):
    """(P, q, l, kappa, tau, residual, rows ra, rb, ta, tb, |t|) of the entries es = [(edge, dir)] at the vector X (longdouble):
    the header's table, and the table's own rot + trans residual of each edge."""
    er, ed = np.asarray(table[0]), np.asarray(table[1], dtype=np.float64)
    m = len(es)
    P, q, l, res = np.zeros((m, d, d), dtype=LD), np.zeros((m, d), dtype=LD), np.zeros((m, d), dtype=LD), np.zeros(m, dtype=LD)
    e = np.array([k for k, _ in es], dtype=np.int64)
    kappa, tau = ed[e, d * d + d].astype(LD), ed[e, d * d + d + 1].astype(LD)
    tn = np.sqrt(np.sum(ed[e, d * d:d * d + d] ** 2, axis=1))
    for i, (k, dr) in enumerate(es):
        ra, rb, ta, tb = (int(v) for v in er[k])
        R, t = ed[k, :d * d].astype(LD).reshape(d, d), ed[k, d * d:d * d + d].astype(LD)
        Xa, Xb = X[ra:ra + d], X[rb:rb + d]
        pa = X[ta] + t @ Xa          # x_t(a) + R_a t with R_a = X_a^T
        P0 = Xa.T @ R @ Xb
        P[i], q[i], l[i] = (P0.T, pa, X[tb]) if dr else (P0, X[tb], pa)
        res[i] = kappa[i] * np.sum((Xb - R.T @ Xa) ** 2) + tau[i] * np.sum((X[tb] - pa) ** 2)
    return P, q, l, kappa, tau, res, er[e, 0], er[e, 1], er[e, 2], er[e, 3], tn


def closure_cost(d, table, X, es):
    """The sum of the table's own rot + trans residuals over the entries es, longdouble, left to right."""
    if len(es) == 0:
        return LD(0)
    return _lsum(entries(d, table, np.asarray(X, dtype=LD), es)[5])


def rule(d, H, K, W, sq, sl):
    """(refused, the rule's quantity over its threshold or None) by the header's refusal rule, on the exact sums."""
    if not K > 0 and not W > 0:
        return True, None
    if not K > 0 and (not sq > 0 or not sl > 0):
        return True, None
    S = (K if K > 0 else LD(0)) * np.sqrt(LD(d)) + np.sqrt(max(sq, LD(0)) * max(sl, LD(0)))
    k = LD(MIN_RANK)
    if d == 2:
        quantity, threshold = np.sum(H * H), (k * S) ** 2
    else:
        cof = np.array([np.cross(H[1], H[2]), np.cross(H[2], H[0]), np.cross(H[0], H[1])], dtype=LD)
        quantity, threshold = np.sum(cof * cof), (k * S) ** 4
    return (not quantity > threshold), (float(quantity / threshold) if threshold > 0 else None)


def reference(d, n, r, nt, table, chains, X, chain_fixed=None, min_closures=1):
    """dict X (N x d longdouble), struct, status, chosen, cost_start, cost_final, transforms (per chain), chain (per taken
    chain: dict with G, s, a_R, a_t, b_t, sv, margin, kappa, costs, chosen), level / rot_level (per row: the bound's a without
    C), round (per row: b), degenerate, norm."""
    rr = np.asarray(table[2])
    X = np.array(X, dtype=LD)
    S = structure(d, n, r, nt, table, chains, chain_fixed, min_closures)
    nch = len(chains)
    res = dict(struct=S, status=np.array(S["chain_init"], dtype=np.uint8), chosen=np.full(nch, -1, dtype=np.int32),
               cost_start=np.zeros(nch, dtype=LD), cost_final=np.zeros(nch, dtype=LD),
               transforms=np.tile(np.concatenate([np.eye(d).reshape(-1), np.zeros(d)]), (nch, 1)).astype(LD), chain={},
               level={}, rot_level={}, round={})
    level, rot_level = res["level"], res["rot_level"]
    for st in S["stages"]:
        moves = []
        for c, es in st:
            P, q, l, kappa, tau, resid, ra, rb, ta, tb, tn = entries(d, table, X, es)
            W, K = _lsum(tau), _lsum(kappa)
            one = dict(es=es, G=np.eye(d, dtype=LD), s=np.zeros(d, dtype=LD), a_R=0.0, a_t=0.0, b_t=0.0, sv=None, margin=None)
            res["chain"][c] = one
            start = _lsum(resid)
            res["cost_start"][c] = res["cost_final"][c] = start
            res["chosen"][c] = 0
            H = _lsum(kappa[:, None, None] * P)
            sq = sl = LD(0)
            if W > 0:
                cq, cl = _lsum(tau[:, None] * q) / W, _lsum(tau[:, None] * l) / W
                qc, lc = q - cq, l - cl
                H = H + _lsum(tau[:, None, None] * lc[:, :, None] * qc[:, None, :])
                sq, sl = _lsum(tau * np.sum(qc * qc, axis=1)), _lsum(tau * np.sum(lc * lc, axis=1))
            else:
                cq, cl = q[0], l[0]
            no, one["margin"] = rule(d, H, K, W, sq, sl)
            if no:
                res["status"][c] = 2
                continue
            res["status"][c] = 0
            G, sv = kabsch(H)
            s = cl - G @ cq
            final = _lsum(kappa * np.sum((G - P) ** 2, axis=(1, 2)) + tau * np.sum((q @ G.T + s - l) ** 2, axis=1))
            res["cost_final"][c] = final
            Wf, Kf = float(W), float(K)
            Lq = float(np.sqrt(_lsum(tau * np.sum((q - q[0]) ** 2, axis=1)) / W)) if W > 0 else 0.0
            Ll = float(np.sqrt(_lsum(tau * np.sum((l - l[0]) ** 2, axis=1)) / W)) if W > 0 else 0.0
            dp = np.array([level.get(int(b), 0.0) + rot_level.get(int(a), 0.0) * float(k) + EPS * (float(_norm(X[b])) + float(k))
                           for a, b, k in zip(ra, ta, tn)])
            delta = float((dp + np.array([level.get(int(b), 0.0) for b in tb])).max())
            dP = max(rot_level.get(int(a), 0.0) + rot_level.get(int(b), 0.0) for a, b in zip(ra, rb)) + 4 * EPS * np.sqrt(d)
            size = Kf * np.sqrt(d) + Wf * Lq * Ll
            gap = (sv[0] + sv[1]) if d == 2 else (sv[1] + sv[2])
            dH = EPS * size + Kf * dP + Wf * (Lq + Ll) * delta
            one.update(G=G, s=s, cq=cq, cl=cl, sv=sv, a_R=dH / gap, a_t=2 * delta + EPS * (Lq + Ll), kappa=size / gap,
                       b_t=EPS * float(_norm(q[0]) + _norm(l[0]) + _norm(s) + _norm(cq) + _norm(cl)), chosen=bool(final < start),
                       costs=(float(start), float(final)),
                       # a cost of this size is the rounding of the written numbers (64 eps per rotation entry and per length, squared)
                       cost_floor=(64 * EPS) ** 2 * float(_lsum(kappa * d + tau * (np.sum(q * q, axis=1) + np.sum(l * l, axis=1)))))
            res["chosen"][c] = 1 if final < start else 0
            if final < start:
                res["transforms"][c] = np.concatenate([G.reshape(-1), s])
                moves.append((c, G, s))
            else:
                res["cost_final"][c] = start
        for c, G, s in moves:
            one = res["chain"][c]
            for rot, trn in S["positions"][c]:
                x = X[trn].copy()
                xn = G @ x + s
                X[rot:rot + d] = X[rot:rot + d] @ G.T
                X[trn] = xn
                level[trn] = level.get(trn, 0.0) + one["a_R"] * float(_norm(x - one["cq"])) + one["a_t"]
                rot_level[rot] = rot_level.get(rot, 0.0) + one["a_R"] + 4 * EPS
                res["round"][trn] = one["b_t"] + EPS * float(_norm(x) + _norm(xn))
    deg, norm = np.zeros(len(rr), dtype=bool), np.zeros(len(rr), dtype=LD)
    for m in range(len(rr)):
        diff = X[rr[m, 2]] - X[rr[m, 1]]
        nrm = norm[m] = np.sqrt(np.sum(diff * diff))
        deg[m] = nrm < 1e-5
        X[rr[m, 0]] = 0 if deg[m] else -diff / nrm   # towards a: the direction of least residual
    res.update(X=X, degenerate=deg, norm=norm)
    return res


def check(got, d, n, r, nt, table, ref, C=None):
    """Asserts the statuses, the counts, chosen (where the reference's costs decide it), the degenerate flags, never-worse,
    cost_start against the reference's, and the transforms and every written row within the bound; untouched rows keep the
    caller's bits.  Returns the worst error / (a + b) seen (0 where nothing was written)."""
    C = C_BOUND if C is None else C
    rr = np.asarray(table[2])
    S = ref["struct"]
    assert np.array_equal(got["status"], ref["status"]), (got["status"], ref["status"])
    assert got["stages"] == len(S["stages"])
    assert got["placed"] == int(np.sum(ref["status"] == 0)) and got["not_placed"] == int(np.sum(np.isin(ref["status"], (1, 2, 3))))
    assert got["refused"] == int(np.sum(ref["status"] == 2))
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
            floor = 1e-9 * max(start, final) + one["cost_floor"] + 1e-300
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
        G, s = one["G"], one["s"]
        gG, gs = np.asarray(got["transforms"][c][:d * d], dtype=LD).reshape(d, d), np.asarray(got["transforms"][c][d * d:], dtype=LD)
        err_R, err_t = float(_norm(gG - G)), float(_norm(gs - s))
        a_T = one["a_R"] * float(_norm(one["cq"])) + one["a_t"]
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
            worst = max(worst, err / (ref["rot_level"][rot] + 8 * EPS))
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


def path_world(d=2, seed=77):
    """A topologies.World of four robots A, B, C, D of 40 .. 60 poses with odometry, no ranges and no landmarks, and 3 rel_pose
    edges per neighbouring pair of the path A - B - C - D, in both directions: every chain after A's hangs on closures alone."""
    import topologies as tp
    w = tp.World(d, seed)
    robots = [w.robot(c, n) for c, n in (("A", 40), ("B", 60), ("C", 47), ("D", 53))]
    for idx in robots:
        w.odometry(idx)
    for k in range(3):
        for a, b in zip(robots[:-1], robots[1:]):
            i, j = int(w.rng.choice(a)), int(w.rng.choice(b))
            w.rel_pose(*((i, j) if k % 2 == 0 else (j, i)))
    return w


def world_problem(w, rank=None):
    """The graph of a World fed into the C++ host through its programmatic API, updated (topologies.to_problem for a graph
    outside the catalogue)."""
    from cora_amd import capi, host
    g = w.g
    P = host.Problem.new(g.dim, rank=rank or g.dim, precond=capi.PRECOND_JACOBI)
    for sym, _ in sorted(g.poses.items(), key=lambda kv: kv[1]):
        P.add_pose(sym)
    for a, b, R, t, cov in g.rpms:
        P.add_rel_pose(a, b, R, t, cov)
    P.update()
    return P


def write_pyfg(w, path):
    """A d = 2 World of poses and relative poses as PyFG text, the vertices at the truth."""
    g = w.g
    assert g.dim == 2 and not g.rplms and not g.pose_priors and not g.ranges and not g.landmarks
    with open(path, "w") as f:
        for i, s in enumerate(w.names):
            f.write("VERTEX_SE2 %d.0 %s %.17g %.17g %.17g\n" % (i, s, w.T[i][0], w.T[i][1], np.arctan2(w.R[i][1, 0], w.R[i][0, 0])))
        for i, (a, b, R, t, cov) in enumerate(g.rpms):
            up = " ".join("%.17g" % cov[r, c] for r in range(3) for c in range(r, 3))
            f.write("EDGE_SE2 %d.0 %s %s %.17g %.17g %.17g %s\n" % (i, a, b, t[0], t[1], np.arctan2(R[1, 0], R[0, 0]), up))


def scene(d, lens, closures, seed, n_free=0, n_lm=0, noise=0.0, ranges=(), moved=True, kappa=None, tau=None, offset=0.0, world=None,
          sights=(), shuffle=False):
    """The scene of placement_ref.scene (chains of lens[c] poses, every chain after the first in a frame of its own, n_free
    free poses, n_lm landmarks) plus one relative-pose edge per (i, j) of `closures` (pose indices; a = i, b = j, so both
    directions occur as the caller orders the pairs), in that order after the odometry edges: the true relative pose in the
    world frame, perturbed by a rotation of about `noise` radians and `noise` in the translation; weights kappa[k], tau[k]
    (None: 1).  A pair inside one chain or with a free pose gives an edge the placement skips.  Then one edge without a second
    rotation per (pose, landmark) of `sights`.  shuffle: the non-chain edges in a random order.  Returns (dims, table, X,
    chains, truth)."""
    rng = np.random.default_rng(2000 + seed)
    dims, table, X, chains, truth = pl.scene(d, lens, list(ranges), seed, n_free=n_free, n_lm=n_lm, moved=moved, offset=offset, world=world)
    _, n, r, nt = dims
    t0 = d * n + r
    first = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    Rw, Tw = np.zeros((n, d, d)), np.zeros((n, d))
    for i in range(n):
        c = int(np.searchsorted(first, i, side="right")) - 1
        Rc, tc = truth[c] if c < len(lens) else (np.eye(d), np.zeros(d))
        Rw[i], Tw[i] = Rc @ X[d * i:d * i + d].T, Rc @ X[t0 + i] + tc
    er, ed = [], []
    for k, (i, j) in enumerate(closures):
        R, t = Rw[i].T @ Rw[j], Rw[i].T @ (Tw[j] - Tw[i])
        if noise:
            R, t = R @ pl._rot(d, rng, noise), t + noise * rng.normal(0, 1, d)
        er.append([d * i, d * j, t0 + i, t0 + j])
        ed.append(list(np.concatenate([R.reshape(-1), t, [1.0 if kappa is None else kappa[k], 1.0 if tau is None else tau[k]]])))
    for i, j in sights:
        er.append([d * i, -1, t0 + i, t0 + n + j])
        ed.append(list(np.concatenate([np.zeros(d * d), Rw[i].T @ (X[t0 + n + j] - Tw[i]), [0.0, 1.0]])))
    if shuffle:
        order = rng.permutation(len(er))
        er, ed = [er[i] for i in order], [ed[i] for i in order]
    er, ed = [list(row) for row in table[0]] + er, [list(row) for row in table[1]] + ed
    table = (np.array(er, dtype=np.int32).reshape(-1, 4), np.array(ed).reshape(-1, d * d + d + 2), table[2], table[3])
    return dims, table, X, chains, truth
