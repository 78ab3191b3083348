"""numpy.longdouble reference of the odometry initialisation (include/cora_hip.h, cora_odometry_init_dev) -- TEST
INFRASTRUCTURE ONLY.  The same definitions composed sequentially: a chain is a list of relative-pose edges of the
measurement table (tests/residuals_ref.table), its head gets (I, s), pose b of edge k gets T_k = T_{k-1} o (R_k, t_k); the
rotation block of a pose holds R^T, its translation row t; poses in no chain are (I, 0); a range row is the direction of
x_t(b) - x_t(a), zero and reported where the norm is below 1e-5.

Bounds (derived, not tuned): a product of k factors of spectral norm 1, bracketed in any order, is within k d^2 eps in
Frobenius norm to first order, so at chain position k -- with the running scale S_k = |s| + sum_{m <= k} |t_m| -- the
rotation block is within max(k, 1) d^2 eps (Frobenius) and the translation row within max(k, 1) d^2 eps S_k; a range row
inherits the bounds of its two translations divided by the norm of their difference, plus 4 eps."""
import numpy as np

from synth import _rot

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def chains_of(g):
    """The chain rule of getOdomInitialization restated on a PyFG: per robot character the edges (c, k) -> (c, k + 1) in
    index order, the last duplicate wins, a gap starts a new chain.  Lists of indices into g.rpms, robots by character."""
    by = {}
    for e, m in enumerate(g.rpms):
        a, b = m[0], m[1]
        if a[0] == b[0] and int(b[1:]) == int(a[1:]) + 1:
            by.setdefault(a[0], {})[int(a[1:])] = e
    chains = []
    for c in sorted(by):
        expect = None
        for i in sorted(by[c]):
            if expect is None or i != expect:
                chains.append([])
            chains[-1].append(by[c][i])
            expect = i + 1
    return chains


def draw_inputs(d, n_chains, n_landmarks, seed):
    """starts [chains][d] (the first chain starts at zero, as the host function's) and landmarks [l][d]."""
    rng = np.random.default_rng(seed)
    starts = 10.0 * rng.uniform(-1, 1, (n_chains, d))
    if n_chains:
        starts[0] = 0.0
    return starts, 10.0 * rng.uniform(-1, 1, (n_landmarks, d))


def reference(d, n, r, nt, table, chains, starts, landmarks=None):
    """dict X (N x d longdouble), k and S (per translation row of poses and landmarks: chain position, running scale),
    degenerate (bool per range measurement), norm (of the difference, per range measurement), written."""
    er, ed, rr, rd = table
    N, t0 = d * n + r + nt, d * n + r
    X = np.zeros((N, d), dtype=LD)
    k_of, S_of = np.zeros(nt, dtype=np.int64), np.zeros(nt, dtype=LD)
    for i in range(n):
        X[d * i:d * i + d] = np.eye(d, dtype=LD)
    written = 0

    def put(rot, trn, R, t, k, S):
        X[rot:rot + d] = R.T
        X[trn] = t
        k_of[trn - t0], S_of[trn - t0] = k, S

    for c, ch in enumerate(chains):
        R, t = np.eye(d, dtype=LD), np.asarray(starts[c], dtype=LD)
        S = np.sqrt(np.sum(t * t))
        put(er[ch[0], 0], er[ch[0], 2], R, t, 0, S)
        for k, e in enumerate(ch, 1):
            Re, te = ed[e, :d * d].reshape(d, d).astype(LD), ed[e, d * d:d * d + d].astype(LD)
            t = t + R @ te
            R = R @ Re
            S = S + np.sqrt(np.sum(te * te))
            put(er[e, 1], er[e, 3], R, t, k, S)
        written += len(ch) + 1
    if landmarks is not None and nt > n:
        X[t0 + n:] = np.asarray(landmarks, dtype=LD).reshape(nt - n, d)
    deg, norm = np.zeros(len(rr), dtype=bool), np.zeros(len(rr), dtype=LD)
    for m in range(len(rr)):
        diff = X[rr[m, 2]] - X[rr[m, 1]]
        norm[m] = np.sqrt(np.sum(diff * diff))
        deg[m] = norm[m] < 1e-5
        X[rr[m, 0]] = 0 if deg[m] else diff / norm[m]
    return dict(X=X, k=k_of, S=S_of, degenerate=deg, norm=norm, written=written)


def row_bounds(d, n, r, nt, table, ref):
    """(rotation bound per pose, translation bound per translation row, bound per range measurement): the bounds of the
    module docstring.  A degenerate range row has bound 0 (it is exactly zero)."""
    kk = np.maximum(ref["k"], 1).astype(LD)
    t0 = d * n + r
    rot = kk[:n] * d * d * EPS
    trn = kk * d * d * EPS * ref["S"]
    trn[n:] = 0   # landmarks are copied
    rr = table[2]
    rng = np.zeros(len(rr), dtype=LD)
    for m in range(len(rr)):
        if not ref["degenerate"][m]:
            rng[m] = (trn[rr[m, 1] - t0] + trn[rr[m, 2] - t0]) / ref["norm"][m] + 4 * EPS
    return rot, trn, rng


def check(X, d, n, r, nt, table, ref):
    """Asserts X (N x d float64) within the bounds of the reference; returns the worst ratio error / bound seen
    (rotation, translation, range)."""
    rot_b, trn_b, rng_b = row_bounds(d, n, r, nt, table, ref)
    E = np.asarray(X, dtype=LD) - ref["X"]
    t0 = d * n + r
    worst = [0.0, 0.0, 0.0]

    def one(kind, what, err, bound):
        assert err <= bound, (what, float(err), float(bound))
        if bound > 0:
            worst[kind] = max(worst[kind], float(err / bound))

    for i in range(n):
        one(0, "rotation block of pose %d (position %d)" % (i, ref["k"][i]), np.sqrt(np.sum(E[d * i:d * i + d] ** 2)), rot_b[i])
    for i in range(nt):
        one(1, "translation row %d (position %d)" % (i, ref["k"][i]), np.sqrt(np.sum(E[t0 + i] ** 2)), trn_b[i])
    rr = table[2]
    for m in range(len(rr)):
        one(2, "range row of measurement %d" % m, np.sqrt(np.sum(E[rr[m, 0]] ** 2)), rng_b[m])
    return worst


# ---- synthetic chains on a handle of its own: n poses, edge i from pose i to pose i + 1, cut into chains by length
def synthetic_table(d, n, n_ranges, seed, step=1.0, sigma=0.3):
    """The measurement table of one string of n poses (API rows, no landmarks): n - 1 relative-pose edges with random
    rotations and steps of length about `step`, n_ranges ranges between random poses."""
    rng = np.random.default_rng(seed)
    m = max(n - 1, 0)
    er = np.zeros((m, 4), dtype=np.int32)
    ed = np.zeros((m, d * d + d + 2))
    t0 = d * n + n_ranges
    for e in range(m):
        er[e] = [d * e, d * (e + 1), t0 + e, t0 + e + 1]
        ed[e, :d * d] = _rot(d, rng, sigma).reshape(-1)
        ed[e, d * d:d * d + d] = step * rng.normal(0, 1, d)
        ed[e, d * d + d:] = 1.0
    rr = np.zeros((n_ranges, 3), dtype=np.int32)
    for k in range(n_ranges):
        a, b = rng.choice(n, size=2, replace=False) if n > 1 else (0, 0)
        rr[k] = [d * n + k, t0 + a, t0 + b]
    return er, ed, rr, np.ones((n_ranges, 2))


def synthetic_chains(lengths, first=0):
    """Chains of the given numbers of edges over consecutive poses from pose `first`: chain c takes the edges
    [o_c, o_c + lengths[c]) and writes the poses o_c .. o_c + lengths[c]; o_{c+1} = o_c + lengths[c] + 1."""
    chains, o = [], first
    for m in lengths:
        chains.append(list(range(o, o + m)))
        o += m + 1
    return chains


def boundary_lengths(tile, sweep, second_sweep):
    """Chain lengths (edges) that sit on every boundary of the scan's shape: 1, 2, 63, 64, 65 edges; tile - 1, tile,
    tile + 1; 2 tile + 3; a head on the last and on the first position of a tile; with second_sweep a chain that runs from
    the first sweep of the middle pass into the second.  Returns (lengths, positions of the heads)."""
    lengths = [1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3]

    def at():
        return sum(m + 1 for m in lengths)

    while at() % tile != tile - 1:          # pad with the shortest chains (2 or 3 positions) up to the last position of a tile
        lengths.append(2 if ((tile - 1 - at()) % tile) % 2 else 1)
    lengths.append(tile - 1)                # a head on the last position of a tile; the next head is on one again
    lengths.append(tile)                    # tile + 1 positions: the next head is on the first position of a tile
    lengths.append(3)
    if second_sweep:
        lengths.append(tile * sweep - at() + 10)  # crosses position tile * sweep: the carry out of the first sweep
        lengths += [tile + 7, 1, 1, 2 * tile]
        assert at() > tile * sweep + 3 * tile
    heads = np.cumsum([0] + [m + 1 for m in lengths])[:-1]
    assert any(h % tile == tile - 1 for h in heads) and any(h > 0 and h % tile == 0 for h in heads)
    return lengths, heads


def diagonal_q(d, n, r, nt):
    """A CSR the handle of a synthetic table is created with: the identity (the initialisation reads the measurement table
    and the row maps, never Q)."""
    N = d * n + r + nt
    return np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32), np.ones(N)
