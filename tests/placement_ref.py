"""numpy.longdouble reference of the chain placement from inter-robot ranges (include/cora_hip.h, cora_place_chains_dev) --
TEST INFRASTRUCTURE ONLY.  The same definitions with plain left-to-right sums, independent of the library: the entries
between chains, the greedy order of the stages, per stage the identity, the linear stage in the squared ranges (scaled by L,
divided by sum w, Cholesky without pivoting, M projected to SO(d)), Gauss-Newton steps with the Cayley retraction, the
visited point of least cost (the earliest on ties), the rigid motion of the chain's rows, then the unit range rows of all
range measurements, (x_t(a) - x_t(b)) / |x_t(a) - x_t(b)|.

Bound (derived, its constant measured: profiles/chain_placement.md).  A stage's point is (R, t') in coordinates relative to
the first entry.  As for the multilateration a relative rounding eps of the terms moves the linear stage's t' by about
eps kappa(M) (|t'| + L)^2 / L and a converged Gauss-Newton step moves it by eps kappa(H) (|t'| + L); call the larger a.  R
moves by a / L (the rotation's degrees of freedom are in units of L).  Anchors that an earlier stage wrote carry that
stage's row error delta, which enters like a perturbation of the ranges: a += max(kappa(M), kappa(H)) delta.  A row
R (x - q_0) + t' + a_0 of the chain is then within C a (1 + |x - q_0| / L) + b, with b = eps (|q_0| + |a_0| + |t| + |x| +
|x_new|) for the roundings of the written translation and of the row itself."""
import numpy as np

import multilat_ref as ml

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
CHUNK = 256           # kPlChunk
MIN_PIVOT = 1e-8      # kPlMinPivot
GN_MIN_PIVOT = 1e-12  # kPlGnMinPivot
C_BOUND = 3.2         # 4 x the worst ratio error / (a + b) over the cases of tests/test_placement_cpu.py (0.80, profiles/chain_placement.md)

bits, diagonal_q = ml.bits, ml.diagonal_q


def unknowns(d):
    return 7 if d == 2 else 16


def default_min_ranges(d):
    return 4 * unknowns(d)


def _norm(v):
    return np.sqrt(np.sum(np.asarray(v, dtype=LD) ** 2))


def so_polish(M):
    """The rotation nearest M (3 x 3 longdouble, det > 0) by the scaled Newton iteration X <- (X + X^-T) / 2; the float64
    singular value decomposition with the determinant's sign on the least singular value where det <= 0."""
    M = np.asarray(M, dtype=LD)

    def cof(X):
        return np.array([np.cross(X[1], X[2]), np.cross(X[2], X[0]), np.cross(X[0], X[1])], dtype=LD)

    det = np.sum(M[0] * cof(M)[0])
    if not det > 0:
        U, _, Vt = np.linalg.svd(np.asarray(M, dtype=np.float64))
        D = np.eye(3)
        D[2, 2] = np.sign(np.linalg.det(U @ Vt)) or 1.0
        return np.asarray(U @ D @ Vt, dtype=LD)
    X = M / np.cbrt(det)
    for _ in range(60):
        Cf = cof(X)
        Xn = (X + Cf / np.sum(X[0] * Cf[0])) / 2
        done = float(np.max(np.abs(Xn - X))) < 1e-19
        X = Xn
        if done:
            break
    return X


def cayley(d, om):
    """The Cayley map of the rotation step om (d = 2: an angle, d = 3: a rotation vector), first order I + [om]x."""
    if d == 2:
        b = om[0] / 2
        c, s = (1 - b * b) / (1 + b * b), 2 * b / (1 + b * b)
        return np.array([[c, -s], [s, c]], dtype=LD)
    b = np.asarray(om, dtype=LD) / 2
    B = np.array([[0, -b[2], b[1]], [b[2], 0, -b[0]], [-b[1], b[0], 0]], dtype=LD)
    bb = np.sum(b * b)
    return ((1 - bb) * np.eye(3, dtype=LD) + 2 * np.outer(b, b) + 2 * B) / (1 + bb)


def structure(d, n, r, nt, table, chains, chain_fixed=None, min_ranges=None):
    """dict stages (list of dict chain, q, a, m: API translation rows and measurements in table order), init (per chain: 0 a
    stage | 1 | 3 | 4 fixed), skipped, positions (per chain: list of (first rotation row, translation row)), counts (stages,
    entries, chunks, skipped)."""
    er, rr = np.asarray(table[0]), np.asarray(table[2])
    min_ranges = default_min_ranges(d) if min_ranges is None else min_ranges
    nch = len(chains)
    positions, chain_of = [], {}
    for c, ch in enumerate(chains):
        pos = [(int(er[ch[0], 0]), int(er[ch[0], 2]))] + [(int(er[e, 1]), int(er[e, 3])) for e in ch]
        positions.append(pos)
        for _, trn in pos:
            chain_of[trn] = c
    placed = [c == 0 for c in range(nch)] if chain_fixed is None else [bool(f) for f in chain_fixed]
    init = [4 if p else 0 for p in placed]
    use, skipped = [], 0
    cnt = np.zeros((nch, nch), dtype=np.int64)
    for m in range(len(rr)):
        ca, cb = chain_of.get(int(rr[m, 1]), -1), chain_of.get(int(rr[m, 2]), -1)
        if ca < 0 or cb < 0 or ca == cb:
            skipped += 1
            continue
        use.append((m, ca, cb))
        cnt[ca, cb] += 1
        cnt[cb, ca] += 1
    stages = []
    while True:
        best, most = -1, -1
        for c in range(nch):
            if placed[c]:
                continue
            k = int(sum(cnt[c, o] for o in range(nch) if placed[o]))
            if k > most:
                best, most = c, k
        if best < 0 or most < min_ranges:
            break
        st = dict(chain=best, q=[], a=[], m=[])
        for m, ca, cb in use:
            if ca == best and placed[cb]:
                st["q"].append(int(rr[m, 1])), st["a"].append(int(rr[m, 2])), st["m"].append(m)
            elif cb == best and placed[ca]:
                st["q"].append(int(rr[m, 2])), st["a"].append(int(rr[m, 1])), st["m"].append(m)
        stages.append(st)
        placed[best] = True
    for c in range(nch):
        if not placed[c]:
            init[c] = 1 if cnt[c].sum() > 0 else 3
    entries = sum(len(s["m"]) for s in stages)
    chunks = sum((len(s["m"]) + CHUNK - 1) // CHUNK for s in stages)
    return dict(stages=stages, init=init, skipped=skipped, positions=positions, counts=(len(stages), entries, chunks, skipped))


def _terms(d, qq, aa, rng):
    m = len(qq)
    cols = [np.ones(m, dtype=LD)] + [2 * qq[:, k] for k in range(d)]
    if d == 2:
        cols += [-2 * (aa[:, 0] * qq[:, 0] + aa[:, 1] * qq[:, 1]), -2 * (aa[:, 1] * qq[:, 0] - aa[:, 0] * qq[:, 1])]
    else:
        cols += [-2 * aa[:, i] * qq[:, j] for i in range(d) for j in range(d)]
    cols += [-2 * aa[:, k] for k in range(d)]
    cols.append(rng * rng - np.sum(qq * qq, axis=1) - np.sum(aa * aa, axis=1))
    return np.stack(cols, axis=1)


def _degrees(d):
    mm = 2 if d == 2 else 9
    return np.array([0] + [1] * d + [2] * mm + [1] * d + [2])


def _cost(R, t, qq, aa, rng, w):
    p = qq @ R.T + t[None, :] - aa
    nrm = np.sqrt(np.sum(p * p, axis=1))
    e = nrm - rng
    return p, nrm, e, ml._lsum(w * e * e)


def solve_stage(d, q, a, rng, w, gn_steps):
    """One stage: q, a [m][d], rng, w [m] (longdouble).  dict status (0 | 2), visited (list of (R, t') per visited point),
    costs, chosen, steps, L, kappa_lin, kappa_gn, pivots (of the linear stage), gn_pivots (the least of every step)."""
    N = unknowns(d)
    qq, aa = q - q[0], a - a[0]
    out = dict(status=0, steps=0, L=1.0, kappa_lin=0.0, kappa_gn=0.0, pivots=[], gn_pivots=[])
    ident = (np.eye(d, dtype=LD), q[0] - a[0])
    sw = ml._lsum(w)
    tr = ml._lsum(w * (np.sum(qq * qq, axis=1) + np.sum(aa * aa, axis=1)))
    L = LD(1)
    lin = None
    if sw > 0 and tr > 0:
        L = np.sqrt(tr / (2 * sw))
        Cm = _terms(d, qq, aa, rng)
        deg = _degrees(d)
        S = ml._lsum(w[:, None, None] * Cm[:, :, None] * Cm[:, None, :])
        scale = L ** (deg[:, None] + deg[None, :]).astype(LD) * sw
        Sn = S / scale
        M, rhs = Sn[:N, :N], Sn[:N, N]
        z, piv = ml._chol_solve(M, rhs, MIN_PIVOT)
        out["pivots"] = piv
        if z is not None:
            out["kappa_lin"] = ml._cond(M)
            if d == 2:
                c, s = z[3], z[4]
                nrm = np.sqrt(c * c + s * s)
                if nrm > 0:
                    lin = (np.array([[c, -s], [s, c]], dtype=LD) / nrm, L * z[5:7])
            else:
                lin = (so_polish(z[4:13].reshape(3, 3)), L * z[13:16])
    out["L"] = float(L)
    if lin is None:
        out["status"] = 2
        lin = ident
    visited, costs = [ident], [_cost(*ident, qq, aa, rng, w)[3]]
    R, t = lin
    stepping = True
    F = d * (d + 1) // 2
    for step in range(1, gn_steps + 2):
        p, nrm, e, cost = _cost(R, t, qq, aa, rng, w)
        visited.append((R.copy(), t.copy()))
        costs.append(cost)
        if step == gn_steps + 1 or not stepping:
            continue
        u = qq @ R.T
        nv = np.where(nrm[:, None] == 0, 0, p / np.where(nrm == 0, 1, nrm)[:, None])
        if d == 2:
            Jr = (u[:, 0] * nv[:, 1] - u[:, 1] * nv[:, 0])[:, None] / L
        else:
            Jr = np.cross(u, nv) / L
        J = np.concatenate([Jr, nv], axis=1)
        H = ml._lsum(w[:, None, None] * J[:, :, None] * J[:, None, :]) / sw
        g = ml._lsum((w * e)[:, None] * J) / sw
        dl, piv = ml._chol_solve(H, g, GN_MIN_PIVOT)
        out["gn_pivots"].append(min(piv))
        if dl is None or not np.all(np.isfinite(np.asarray(dl, dtype=np.float64))):
            stepping = False
            continue
        out["kappa_gn"] = max(out["kappa_gn"], ml._cond(H))
        Rn = cayley(d, -dl[:F - d] / L) @ R
        if d == 3:
            Rn = so_polish(Rn)
        else:
            Rn = Rn / np.sqrt(Rn[0, 0] ** 2 + Rn[1, 0] ** 2)
        R, t = Rn, t - dl[F - d:]
        out["steps"] += 1
    best = 0
    for j in range(1, len(costs)):
        if costs[j] < costs[best]:
            best = j
    out.update(visited=visited, costs=costs, chosen=best)
    return out


def full_transform(one, q0, a0, pick):
    """(R, t) as written for visited point `pick` of a stage: the identity exactly for point 0."""
    d = len(q0)
    if pick == 0:
        return np.eye(d, dtype=LD), np.zeros(d, dtype=LD)
    R, t = one["visited"][pick]
    return R, t + a0 - R @ q0


def reference(d, n, r, nt, table, chains, X, gn_steps, chain_fixed=None, min_ranges=None):
    """dict X (N x d longdouble), struct (structure()), status, chosen, cost_start, cost_linear, cost_final (per chain),
    steps, transforms (per chain [d * d + d]), stage (per stage the dict of solve_stage plus q0, a0, a: the bound's a of the
    module docstring without C), row_a / row_b (per API translation row of a placed chain), degenerate, norm."""
    rr, rd = np.asarray(table[2]), np.asarray(table[3], dtype=np.float64)
    X = np.array(X, dtype=LD)
    S = structure(d, n, r, nt, table, chains, chain_fixed, min_ranges)
    nch, G = len(chains), d * d + d
    res = dict(struct=S, status=np.array(S["init"], dtype=np.uint8), chosen=np.full(nch, -1, dtype=np.int32),
               cost_start=np.zeros(nch, dtype=LD), cost_linear=np.zeros(nch, dtype=LD), cost_final=np.zeros(nch, dtype=LD), steps=0,
               transforms=np.tile(np.concatenate([np.eye(d).reshape(-1), np.zeros(d)]), (nch, 1)).astype(LD), stage=[], row_a={}, row_b={})
    t0 = d * n + r
    for st in S["stages"]:
        qi, ai, ms = np.array(st["q"]), np.array(st["a"]), np.array(st["m"])
        q, a = X[qi], X[ai]
        one = solve_stage(d, q, a, rd[ms, 0].astype(LD), rd[ms, 1].astype(LD), gn_steps)
        c = st["chain"]
        res["status"][c], res["chosen"][c], res["steps"] = one["status"], one["chosen"], res["steps"] + one["steps"]
        res["cost_start"][c], res["cost_linear"][c], res["cost_final"][c] = one["costs"][0], one["costs"][1], one["costs"][one["chosen"]]
        R, t = full_transform(one, q[0], a[0], one["chosen"])
        res["transforms"][c] = np.concatenate([R.reshape(-1), t])
        L, tp = one["L"], float(_norm(one["visited"][one["chosen"]][1]))
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
            res["row_a"][trn] = one["a"] * (1 + float(_norm(x - q[0])) / L)
            res["row_b"][trn] = EPS * float(_norm(q[0]) + _norm(a[0]) + _norm(t) + _norm(x) + _norm(xn))
        res["stage"].append(one)
    deg, norm = np.zeros(len(rr), dtype=bool), np.zeros(len(rr), dtype=LD)
    for m in range(len(rr)):
        diff = X[rr[m, 2]] - X[rr[m, 1]]
        nrm = norm[m] = np.sqrt(np.sum(diff * diff))
        deg[m] = nrm < 1e-5
        X[rr[m, 0]] = 0 if deg[m] else -diff / nrm   # towards a: the direction of least residual
    res.update(X=X, degenerate=deg, norm=norm)
    return res


def check(got, d, n, r, nt, table, ref, C=C_BOUND):
    """Asserts statuses, counts, chosen (where the reference's costs decide it), the degenerate flags, never-worse, and the
    written transforms and rows within the bound; returns the worst error / (a + b) seen (0 without a stage)."""
    rd, rr = np.asarray(table[3], dtype=np.float64), np.asarray(table[2])
    S = ref["struct"]
    t0 = d * n + r
    assert np.array_equal(got["status"], ref["status"]), (got["status"], ref["status"])
    assert got["placed"] == len(S["stages"]) == got["stages"]
    assert got["not_placed"] == sum(1 for s in S["init"] if s in (1, 3))
    worst = 0.0
    row_bound = {}
    stage_of = {st["chain"]: k for k, st in enumerate(S["stages"])}
    for c in range(len(S["init"])):
        if c not in stage_of:
            assert got["chosen"][c] == -1 and got["cost_start"][c] == 0 and got["cost_linear"][c] == 0 and got["cost_final"][c] == 0
            assert np.array_equal(got["transforms"][c], np.asarray(ref["transforms"][c], dtype=np.float64))
            for rot, trn in S["positions"][c]:   # a chain that is no stage keeps the caller's bits
                assert np.array_equal(bits(got["X"][trn]), bits(got["X_in"][trn])) and np.array_equal(bits(got["X"][rot:rot + d]), bits(got["X_in"][rot:rot + d]))
            continue
        one = ref["stage"][stage_of[c]]
        # never worse, as doubles
        assert got["cost_final"][c] <= got["cost_start"][c], (c, got["cost_final"][c], got["cost_start"][c])
        # the order of two visited costs is the algorithm's only where they differ by more than their rounding (the rule of
        # multilat_ref.check): below that the point taken must be one that ties, and it is compared with THAT visited point
        costs = np.array([float(v) for v in one["costs"]])
        order = np.sort(costs)
        floor = 1e-9 * costs.max() + 1e-20 * float(np.sum(rd[:, 1] * rd[:, 0] ** 2))
        pick = int(got["chosen"][c])
        if order[1] - order[0] > floor:
            assert pick == one["chosen"], (c, pick, one["chosen"], costs)
        assert 0 <= pick < len(costs) and costs[pick] - order[0] <= floor, (c, pick, costs)
        R, t = full_transform(one, one["q0"], one["a0"], pick)
        gR, gt = np.asarray(got["transforms"][c][:d * d], dtype=LD).reshape(d, d), np.asarray(got["transforms"][c][d * d:], dtype=LD)
        a, L = one["a"], one["L"]
        if pick == 0:
            assert np.array_equal(got["transforms"][c], np.concatenate([np.eye(d).reshape(-1), np.zeros(d)]))
        bt = EPS * float(_norm(one["q0"]) + _norm(one["a0"]) + _norm(t))
        err_R, err_t = float(_norm(gR - R)), float(_norm(gt - t))
        assert err_R <= C * a / L + 4 * EPS, ("rotation of chain %d" % c, err_R, C * a / L)
        assert err_t <= C * a * (1 + float(_norm(one["q0"])) / L) + bt, ("translation of chain %d" % c, err_t, C * a, bt)
        worst = max(worst, err_R / (a / L + 4 * EPS), err_t / (a * (1 + float(_norm(one["q0"])) / L) + bt))
        for rot, trn in S["positions"][c]:
            x, blk = one["rows_before"][trn]
            ra, rb = ref["row_a"][trn], ref["row_b"][trn]
            err = float(_norm(np.asarray(got["X"][trn], dtype=LD) - (R @ x + t)))
            assert err <= C * ra + rb, ("translation row %d of chain %d" % (trn, c), err, C * ra + rb)
            worst = max(worst, err / (ra + rb))
            err = float(_norm(np.asarray(got["X"][rot:rot + d], dtype=LD) - blk @ R.T))
            assert err <= C * a / L + 8 * EPS, ("rotation block %d of chain %d" % (rot, c), err)
            row_bound[trn] = (C * ra + rb) if pick == one["chosen"] else np.inf
    assert np.array_equal(got["degenerate"], ref["degenerate"]) and got["n_degenerate"] == int(ref["degenerate"].sum())
    for m in range(len(rr)):
        row = np.asarray(got["X"][rr[m, 0]], dtype=LD)
        if ref["degenerate"][m]:
            assert not row.any()
            continue
        bound = (row_bound.get(int(rr[m, 1]), 0.0) + row_bound.get(int(rr[m, 2]), 0.0)) / float(ref["norm"][m]) + 4 * EPS
        assert float(_norm(row - ref["X"][rr[m, 0]])) <= bound, ("range row of measurement %d" % m, bound)
    return worst


def _rot(d, rng, angle):
    """A rotation by about `angle` radians about a random axis (d = 3) / by a random angle in [-angle, angle] (d = 2)."""
    th = rng.uniform(-angle, angle)
    if d == 2:
        return np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    ax = rng.normal(0, 1, 3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def scene(d, lens, ranges, seed, noise=0.0, offset=0.0, n_free=0, n_lm=0, omega=None, world=None, moved=True):
    """Chains of lens[c] poses over consecutive pose indices, then n_free poses in no chain, then n_lm landmarks.  The truth
    lives in one world frame (a random walk per chain around a common area, or `world`: [poses][d] positions); the vector X
    holds chain 0 as it is and every other chain in a frame of its own: pose_own = g_c^-1 o pose_world with a random g_c
    (`moved` False, or False at c in a list: g_c = identity).  ranges: (a, b) translation indices in table order, measured in the world frame.
    Returns (dims, table, X, chains, truth) with truth = per chain (R_c, t_c)."""
    rng = np.random.default_rng(seed)
    n, nch = int(sum(lens)) + n_free, len(lens)
    r, nt = len(ranges), n + n_lm
    t0 = d * n + r
    Tw = np.zeros((nt, d))
    Rw = np.zeros((n, d, d))
    first = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    for c in range(nch):
        Tw[first[c]:first[c + 1]] = 10 * rng.uniform(-1, 1, d) + np.cumsum(rng.normal(0, 1, (lens[c], d)), axis=0)
    Tw[first[nch]:] = 10 * rng.uniform(-1, 1, (nt - first[nch], d))
    if world is not None:
        Tw[:len(world)] = world
    Tw += offset
    for i in range(n):
        Rw[i] = _rot(d, rng, np.pi)
    truth = [(np.eye(d), np.zeros(d))]
    mv = list(moved) if isinstance(moved, (list, tuple)) else [moved] * nch
    for c in range(1, nch):
        truth.append((_rot(d, rng, 2.5), 10 * rng.uniform(-1, 1, d)) if mv[c] else (np.eye(d), np.zeros(d)))
    X = np.zeros((d * n + r + nt, d))
    To, Ro = Tw.copy(), Rw.copy()
    for c in range(nch):
        Rc, tc = truth[c]
        for i in range(first[c], first[c + 1]):
            To[i] = Rc.T @ (Tw[i] - tc)
            Ro[i] = Rc.T @ Rw[i]
    for i in range(n):
        X[d * i:d * i + d] = Ro[i].T
    X[t0:] = To
    chains, er, ed = [], [], []
    for c in range(nch):
        chains.append(list(range(len(er), len(er) + lens[c] - 1)))
        for i in range(first[c], first[c + 1] - 1):
            er.append([d * i, d * (i + 1), t0 + i, t0 + i + 1])
            ed.append(np.concatenate([(Ro[i].T @ Ro[i + 1]).reshape(-1), Ro[i].T @ (To[i + 1] - To[i]), [1.0, 1.0]]))
    rr = np.zeros((r, 3), dtype=np.int32)
    rd = np.ones((r, 2))
    for m, (a, b) in enumerate(ranges):
        rr[m] = [d * n + m, t0 + a, t0 + b]
        rd[m, 0] = abs(np.linalg.norm(Tw[a] - Tw[b]) + noise * rng.normal())
        rd[m, 1] = 1.0 if omega is None else omega[m]
    table = (np.array(er, dtype=np.int32).reshape(-1, 4), np.array(ed).reshape(-1, d * d + d + 2), rr, rd)
    return (d, n, r, nt), table, X, chains, truth
