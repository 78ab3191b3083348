"""numpy.longdouble reference of the landmark initialisation from ranges (include/cora_hip.h, cora_multilaterate_dev) --
TEST INFRASTRUCTURE ONLY.  The same definitions with plain left-to-right sums: per landmark the usable ranges in table
order after the masks, the origin t_0 = the first anchor, the linear stage in (y, s) scaled by L and divided by sum w, a
Cholesky without pivoting, Gauss-Newton steps on the range cost, the visited point of least cost (the earliest on ties),
then the unit range rows of all range measurements, (x_t(a) - x_t(b)) / |x_t(a) - x_t(b)|.

Bound (derived, its constant measured: profiles/multilateration.md).  The linear stage solves M z = q whose right-hand side
carries b = r^2 - |u|^2 of size (|y| + L)^2 in a solution of size |y| / L, so a relative rounding eps of the terms moves y
by about eps kappa(M) (|y| + L)^2 / L; a converged Gauss-Newton step moves it by eps kappa(H) (|y| + L); the row t_0 + y is
rounded once more, eps |x|.  error <= C eps max(kappa(M) (|y| + L)^2 / L, kappa(H) (|y| + L)) + eps |x|."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
CHUNK = 256          # kMlChunk
MIN_PIVOT = 1e-8     # kMlMinPivot
GN_MIN_PIVOT = 1e-12
C_BOUND = 0.3        # 4 x the worst ratio error / (a + b) over the cases of tests/test_multilat_cpu.py (0.074, profiles/multilateration.md)


def lists_of(d, n, r, nt, rr, pose_ok=None, landmark_on=None):
    """(lists, usable, skipped): per landmark the (API translation row of the anchor, range measurement) pairs."""
    t0 = d * n + r
    lists = [[] for _ in range(nt - n)]
    usable = skipped = 0
    for m in range(len(rr)):
        ia, ib = int(rr[m, 1]) - t0, int(rr[m, 2]) - t0
        if (ia >= n) == (ib >= n):
            skipped += 1
            continue
        usable += 1
        l, pose = (ia - n, ib) if ia >= n else (ib - n, ia)
        if landmark_on is not None and not landmark_on[l]:
            continue
        if pose_ok is not None and not pose_ok[pose]:
            continue
        lists[l].append((t0 + pose, m))
    return lists, usable, skipped


def _lsum(a):
    """Plain left-to-right sum over the first axis."""
    return np.cumsum(np.asarray(a, dtype=LD), axis=0)[-1]


def _chol_solve(M, q, min_pivot):
    """(z or None, pivots): Cholesky without pivoting in longdouble, refused at the first pivot <= min_pivot."""
    k = len(q)
    G = np.zeros((k, k), dtype=LD)
    piv = []
    for j in range(k):
        p = M[j, j] - np.sum(G[j, :j] ** 2)
        piv.append(float(p))
        if not p > min_pivot:
            return None, piv
        G[j, j] = np.sqrt(p)
        for i in range(j + 1, k):
            G[i, j] = (M[i, j] - np.sum(G[i, :j] * G[j, :j])) / G[j, j]
    z = np.array(q, dtype=LD)
    for i in range(k):
        z[i] = (z[i] - np.sum(G[i, :i] * z[:i])) / G[i, i]
    for i in range(k - 1, -1, -1):
        z[i] = (z[i] - np.sum(G[i + 1:, i] * z[i + 1:])) / G[i, i]
    return z, piv


def _cond(M):
    M = np.asarray(M, dtype=np.float64)
    return float(np.linalg.cond(M)) if np.all(np.isfinite(M)) else float("inf")


def _cost(y, u, rng, w):
    D = y[None, :] - u
    nrm = np.sqrt(np.sum(D * D, axis=1))
    e = nrm - rng
    return D, nrm, e, _lsum(w * e * e)


def solve_landmark(d, t, rng, w, gn_steps):
    """One list: t [m][d] anchors, rng [m], w [m] (longdouble).  dict status, y (chosen, relative to t[0]), chosen, costs
    (per visited point), steps, kappa_lin, kappa_gn, L, pivots (of the linear stage)."""
    m = len(t)
    out = dict(status=0, y=None, chosen=-1, costs=[], steps=0, kappa_lin=0.0, kappa_gn=0.0, L=0.0, pivots=[])
    if m == 0:
        out["status"] = 3
        return out
    if m < d + 1:
        out["status"] = 1
        return out
    u = t - t[0]
    n2 = np.sum(u * u, axis=1)
    b = rng * rng - n2
    sw = _lsum(w)
    tr = _lsum(w * n2)
    if not sw > 0 or not tr > 0:
        out["status"] = 2
        return out
    L = np.sqrt(tr / sw)
    out["L"] = float(L)
    M = np.zeros((d + 1, d + 1), dtype=LD)
    q = np.zeros(d + 1, dtype=LD)
    M[:d, :d] = 4 * _lsum(w[:, None, None] * u[:, :, None] * u[:, None, :]) / tr
    M[:d, d] = M[d, :d] = -2 * _lsum(w[:, None] * u) / (L * sw)
    M[d, d] = 1
    q[:d] = -2 * _lsum((w * b)[:, None] * u) / (L * tr)
    q[d] = _lsum(w * b) / tr
    z, piv = _chol_solve(M, q, MIN_PIVOT)
    out["pivots"] = piv
    if z is None:
        out["status"] = 2
        return out
    out["kappa_lin"] = _cond(M)
    y = L * z[:d]
    visited, stepping = [y.copy()], True
    for j in range(gn_steps + 1):
        D, nrm, e, cost = _cost(y, u, rng, w)
        out["costs"].append(cost)
        if j == gn_steps or not stepping:
            if j < gn_steps:
                visited.append(y.copy())
            continue
        J = np.where(nrm[:, None] == 0, 0, D / np.where(nrm == 0, 1, nrm)[:, None])
        H = _lsum(w[:, None, None] * J[:, :, None] * J[:, None, :]) / sw
        g = _lsum((w * e)[:, None] * J) / sw
        step, _ = _chol_solve(H, g, GN_MIN_PIVOT)
        if step is None or not np.all(np.isfinite(np.asarray(y - step, dtype=np.float64))):
            stepping = False
        else:
            out["kappa_gn"] = max(out["kappa_gn"], _cond(H))
            y = y - step
            out["steps"] += 1
        visited.append(y.copy())
    costs = out["costs"]
    best = 0
    for j in range(1, len(costs)):
        if costs[j] < costs[best]:
            best = j
    out["chosen"], out["y"], out["visited"] = best, visited[best], visited
    return out


def reference(d, n, r, nt, table, X, gn_steps, pose_ok=None, landmark_on=None):
    """dict X (N x d longdouble: landmark rows of the solved landmarks and every range row of the table rewritten), status,
    chosen, cost_linear, cost_final, steps, counts (landmarks with a list, usable, skipped, chunks), degenerate, per
    landmark the dicts of solve_landmark (lm), bound (per landmark, the module docstring's without C: (a, b) with
    error <= C a + b)."""
    rr, rd = np.asarray(table[2]), np.asarray(table[3], dtype=np.float64)
    X = np.array(X, dtype=LD)
    nl, t0 = nt - n, d * n + r
    lists, usable, skipped = lists_of(d, n, r, nt, rr, pose_ok, landmark_on)
    res = dict(status=np.zeros(nl, dtype=np.uint8), chosen=np.full(nl, -1, dtype=np.int32), cost_linear=np.zeros(nl, dtype=LD),
               cost_final=np.zeros(nl, dtype=LD), steps=0, lm=[], bound=[])
    for l, lst in enumerate(lists):
        rows = np.array([a for a, _ in lst], dtype=np.int64)
        ms = np.array([m for _, m in lst], dtype=np.int64)
        one = solve_landmark(d, X[rows], rd[ms, 0].astype(LD), rd[ms, 1].astype(LD), gn_steps)
        if landmark_on is not None and not landmark_on[l]:
            one["status"] = 3
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
        X[rr[m, 0]] = 0 if deg[m] else -diff / nrm   # towards a: the direction of least residual
    chunks = sum((len(lst) + CHUNK - 1) // CHUNK for lst in lists)
    res.update(X=X, degenerate=deg, norm=norm, counts=(sum(1 for lst in lists if lst), usable, skipped, chunks))
    return res


def check(got, d, n, r, nt, table, ref, C=C_BOUND):
    """Asserts statuses, counts of solved landmarks, degenerate flags, chosen (where the reference's costs decide it) and
    the rows of the solved landmarks within the bound; returns the worst error / (a + b) seen (0 without a solved landmark)."""
    rd = np.asarray(table[3], dtype=np.float64)
    t0 = d * n + r
    assert np.array_equal(got["status"], ref["status"]), (got["status"], ref["status"])
    assert got["solved"] == int(np.sum(ref["status"] == 0)) and got["not_solved"] == nt - n - got["solved"]
    worst = 0.0
    row_bound = np.zeros(nt)   # per translation row: the landmarks' bounds, the poses are the caller's
    for l, one in enumerate(ref["lm"]):
        if one["status"] != 0:
            assert got["chosen"][l] == -1 and got["cost_linear"][l] == 0 and got["cost_final"][l] == 0
            continue
        # The order of two visited costs is the algorithm's only where they differ by more than their rounding: the cost
        # is a sum of len terms each within a few eps of w (|D| + r)^2-sized squares -- below 1e-9 of the largest visited
        # cost plus 1e-20 sum w r^2 the comparison belongs to the rounding, and `chosen` is not compared.
        costs = np.array([float(c) for c in one["costs"]])
        order = np.sort(costs)
        floor = 1e-9 * costs.max() + 1e-20 * float(np.sum(rd[:, 1] * rd[:, 0] ** 2))
        pick = int(got["chosen"][l])
        if len(order) == 1 or order[1] - order[0] > floor:
            assert pick == one["chosen"], (l, pick, one["chosen"], costs)
        # (otherwise the point taken is one whose reference cost ties with the least, and the row is compared with THAT
        # visited point of the reference)
        assert 0 <= pick < len(costs) and costs[pick] - order[0] <= floor, (l, pick, costs)
        assert got["cost_final"][l] <= got["cost_linear"][l]
        a, b = ref["bound"][l]
        origin = ref["X"][t0 + n + l] - one["y"]
        err = float(np.sqrt(np.sum((np.asarray(got["X"][t0 + n + l], dtype=LD) - (origin + one["visited"][pick])) ** 2)))
        assert err <= C * a + b, ("landmark %d" % l, err, C * a + b)
        row_bound[n + l] = (C * a + b) if pick == one["chosen"] else np.inf   # (another visited point: the row is not the reference's)
        worst = max(worst, err / (a + b))
    assert np.array_equal(got["degenerate"], ref["degenerate"]) and got["n_degenerate"] == int(ref["degenerate"].sum())
    # a range row is the difference of two translation rows divided by its norm: their bounds over the norm, plus 4 eps
    # for the subtraction, the norm and the division; a degenerate row is exactly zero
    rr = np.asarray(table[2])
    for m in range(len(rr)):
        row = np.asarray(got["X"][rr[m, 0]], dtype=LD)
        if ref["degenerate"][m]:
            assert not row.any()
            continue
        bound = (row_bound[rr[m, 1] - t0] + row_bound[rr[m, 2] - t0]) / float(ref["norm"][m]) + 4 * EPS
        assert float(np.sqrt(np.sum((row - ref["X"][rr[m, 0]]) ** 2))) <= bound, ("range row of measurement %d" % m, bound)
    return worst


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def diagonal_q(d, n, r, nt):
    """A CSR a handle of a synthetic table is created with: the identity (the multilateration reads the measurement table
    and the row maps, never Q)."""
    N = d * n + r + nt
    return np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32), np.ones(N)


def graph(d, poses, landmarks, ranges, noise=0.0, seed=0, omega=None):
    """A table of ranges only over given positions: poses [n][d], landmarks [nl][d] (the truth), ranges a list of
    (a, b) translation indices (poses 0 .. n - 1, landmarks n ..) in table order.  Returns (dims, table, X) with X (N x d)
    holding identity rotation blocks, the poses' rows, and the landmarks' rows set to a marker the solve must replace."""
    rng = np.random.default_rng(seed)
    poses, landmarks = np.asarray(poses, dtype=np.float64).reshape(-1, d), np.asarray(landmarks, dtype=np.float64).reshape(-1, d)
    n, nl, r = len(poses), len(landmarks), len(ranges)
    nt, t0 = n + nl, d * n + r
    T = np.concatenate([poses, landmarks])
    rr = np.zeros((r, 3), dtype=np.int32)
    rd = np.ones((r, 2))
    for m, (a, b) in enumerate(ranges):
        rr[m] = [d * n + m, t0 + a, t0 + b]
        rd[m, 0] = abs(np.linalg.norm(T[a] - T[b]) + noise * rng.normal())
        rd[m, 1] = 1.0 if omega is None else omega[m]
    X = np.zeros((d * n + r + nt, d))
    for i in range(n):
        X[d * i:d * i + d] = np.eye(d)
    X[t0:t0 + n] = poses
    X[t0 + n:] = 123.5 + np.arange(nl * d).reshape(nl, d)
    table = (np.zeros((0, 4), dtype=np.int32), np.zeros((0, d * d + d + 2)), rr, rd)
    return (d, n, r, nt), table, X
