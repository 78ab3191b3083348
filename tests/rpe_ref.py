"""The relative pose error of include/cora_hip.h (cora_rpe_dev) restated in numpy: every sum in longdouble, the two
rounding bounds the header states, the pair builders of Problem::posePairsByStep / posePairsByDistance restated
independently, and the inputs the tests use (gauge copies, known perturbations).  API row order: d n rotation rows, r
range rows, n + l translation rows (poses, then landmarks)."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


def RANKS(d):
    """(k, kr): both stride parities for each vector, k above and below kr."""
    return ((d, d), (d + 1, d), (5, 5), (24, d), (d, 24), (24, 24))


def rows(d, n, r, nt):
    """(rotation rows [n, d], translation rows [nt]) in API order."""
    return np.arange(d * n).reshape(n, d), d * n + r + np.arange(nt)


def _motion(V, d, n, r, nt, pairs):
    """E [m, d, d] and u [m, d] of every pair in longdouble, plus the norms the bounds are made of (float64)."""
    rot, trn = rows(d, n, r, nt)
    V = np.asarray(V, dtype=LD)
    i, j = pairs[:, 0], pairs[:, 1]
    Vi, Vj = V[rot[i]], V[rot[j]]  # [m, d, k]
    dx = V[trn[j]] - V[trn[i]]     # [m, k]
    E = np.einsum("mak,mbk->mab", Vi, Vj)
    u = np.einsum("mak,mk->ma", Vi, dx)
    ni = np.sqrt((Vi * Vi).sum((1, 2))).astype(np.float64)
    nj = np.sqrt((Vj * Vj).sum((1, 2))).astype(np.float64)
    return E, u, ni * np.sqrt((dx * dx).sum(1)).astype(np.float64), ni * nj


def rpe(X, Ref, d, n, r, nt, pairs):
    """(et [m], er [m]) in longdouble; both 0 where i == j (the identity motion in both vectors, by definition)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    E, u, _, _ = _motion(X, d, n, r, nt, pairs)
    S, v, _, _ = _motion(Ref, d, n, r, nt, pairs)
    other = pairs[:, 0] != pairs[:, 1]
    et = np.sqrt(((u - v) ** 2).sum(1)) * other
    er = np.sqrt(((E - S) ** 2).sum((1, 2))) * other
    return et, er


def bounds(X, Ref, d, n, r, nt, pairs):
    """2 (k + kr + d + 8) eps (a + b) for et and 2 (k + kr + d + 8) eps (A + B) for er, per pair (float64)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    _, _, a, A = _motion(X, d, n, r, nt, pairs)
    _, _, b, B = _motion(Ref, d, n, r, nt, pairs)
    c = 2 * (X.shape[1] + Ref.shape[1] + d + 8) * EPS
    return c * (a + b), c * (A + B)


def check(res, X, Ref, d, n, r, nt, pairs, what=""):
    """A result of Context.rpe / rpe_dev / debug_rpe_host against the longdouble reference within the bounds, and its
    statistics against its own arrays; returns the worst ratios to the bounds."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    et, er = rpe(X, Ref, d, n, r, nt, pairs)
    bt, br = bounds(X, Ref, d, n, r, nt, pairs)
    worst = []
    for key, want, b in (("trans_err", et, bt), ("rot_err", er, br)):
        err = np.abs(res[key] - want).astype(np.float64)
        ratio = float((err / np.maximum(b, 1e-300)).max(initial=0.0))
        print("%s: %s worst |error| / bound = %.3f" % (what, key, ratio))
        assert np.all(err <= b), (what, key, ratio)
        worst.append(ratio)
    check_statistics(res, len(pairs), what)
    return worst


def check_statistics(res, m, what=""):
    """The maxima and the first maximum are exact functions of the arrays; the sums within m eps sum."""
    et, er = res["trans_err"], res["rot_err"]
    assert res["m"] == m and len(et) == m and len(er) == m, what
    assert res["max_et"] == et.max(initial=0.0) and res["max_er"] == er.max(initial=0.0), what
    assert res["argmax_et"] == (int(np.argmax(et)) if m else 0), what
    for key, v in (("sum_et2", et), ("sum_er2", er)):
        want = float((v.astype(LD) ** 2).sum())
        assert abs(res[key] - want) <= max(m, 1) * EPS * want, (what, key, res[key], want)


# ---- pair builders, independent of the C++ ones: `chains` is a list of lists of pose indices, one per robot
def chains_of(symbols):
    """symbols: the pose symbols ('A12') in pose order.  One chain per character (characters ascending), the poses of a
    chain by ascending number."""
    by = {}
    for idx, s in enumerate(symbols):
        by.setdefault(s[0], []).append((int(s[1:]), idx))
    return [[idx for _, idx in sorted(by[c])] for c in sorted(by)]


def pairs_by_step(chains, step):
    pairs = [(c[a], c[a + step]) for c in chains for a in range(len(c) - step)]
    return np.array(pairs, dtype=np.int32).reshape(-1, 2), np.full(len(pairs), float(step))


def pairs_by_distance(chains, positions, L):
    """positions [n, kr]: the reference's position of every pose.  For each start, by plain search, the first later pose
    of the chain at least L away along the path."""
    pairs, length = [], []
    for c in chains:
        seg = [float(np.linalg.norm(positions[c[a + 1]] - positions[c[a]])) for a in range(len(c) - 1)]
        s = np.concatenate([[0.0], np.cumsum(seg)]) if c else np.zeros(0)
        for a in range(len(c)):
            for b in range(a + 1, len(c)):
                if s[b] - s[a] >= L:
                    pairs.append((c[a], c[b]))
                    length.append(s[b] - s[a])
                    break
    return np.array(pairs, dtype=np.int32).reshape(-1, 2), np.array(length)


# ---- inputs
def reference_of_rank(truth, kr, rng):
    """The ground truth (N x d) in a random orthonormal frame of R^kr (kr >= d), or its first kr columns' worth: for
    kr < d the truth times a d x kr matrix with orthonormal columns (off the manifold, still a valid input)."""
    d = truth.shape[1]
    if kr == d:
        return truth.copy()
    Q = np.linalg.qr(rng.standard_normal((max(kr, d), max(kr, d))))[0]
    return truth @ Q[:d, :kr]


def gauge_copy(Ref, d, n, r, nt, k, rng):
    """X = Ref B + shift on the translation rows, B random kr x k with orthonormal rows (k >= kr): every relative motion
    of X is that of Ref."""
    kr = Ref.shape[1]
    B = np.linalg.qr(rng.standard_normal((k, kr)))[0].T
    X = Ref @ B
    X[rows(d, n, r, nt)[1]] += rng.standard_normal(k) * 3.0
    return X


def rotation(d, theta, axis=None):
    if d == 2:
        return np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * K @ K


def rotate_pose(X, d, j, Q):
    """The rotation block of pose j multiplied by Q from the left: E_ij becomes E_ij Q^T."""
    out = X.copy()
    out[d * j:d * j + d] = Q @ X[d * j:d * j + d]
    return out


def shift_pose(X, d, n, r, i, j, delta):
    """Pose j moved by delta (d numbers) in pose i's frame: x_j += delta X_i."""
    out = X.copy()
    out[d * n + r + j] += np.asarray(delta) @ X[d * i:d * i + d]
    return out
