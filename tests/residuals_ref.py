"""numpy reference of the per-measurement residuals over oracle.assemble.PyFG -- TEST INFRASTRUCTURE ONLY.

With X_a the d x k block of pose a's rotation rows, x_t(s) the translation row of symbol s and x_rho(m) the unit row of
range m (X in the API row order: d*n rotation rows, r range rows, n + l translation rows):
  edge  (a, b, R, t, kappa, tau):  rot = kappa |X_b - R^T X_a|_F^2,  trans = tau |x_t(b) - x_t(a) - sum_c t_c X_a[c, :]|^2
  range (a, b, r, omega):          res = omega |x_t(b) - x_t(a) + r x_rho(m)|^2
Edges come in the row order of fillRelPoseSubmatrices (oracle/assemble.py: pose-pose, pose priors, pose-landmark, landmark
priors); pose-landmark edges and landmark priors have no rotation part.  No 1/2 in the values: 1/2 of all of them is the
cost 1/2 <X, Q X>."""
import numpy as np

from oracle import assemble as asm

KINDS = ("rel_pose", "pose_prior", "pose_landmark", "landmark_prior")


def edges(g):
    """[(kind, a, b, R or None, t, kappa, tau)] in table order."""
    d = g.dim
    out = [("rel_pose", a, b, R, t, asm._rot_precision(cov), asm._trans_precision(cov, d)) for a, b, R, t, cov in g.rpms]
    out += [("pose_prior", "O0", s, R, t, asm._rot_precision(cov), asm._trans_precision(cov, d))
            for s, R, t, cov in g.pose_priors]
    out += [("pose_landmark", a, b, None, t, 0.0, asm._trans_precision(cov, d)) for a, b, t, cov in g.rplms]
    out += [("landmark_prior", "O0", s, None, p, 0.0, asm._trans_precision(cov, d)) for s, p, cov in g.landmark_priors]
    return out


def _rows(g):
    d, n, r = g.dim, len(g.poses), len(g.ranges)

    def trow(s):
        return d * n + r + (g.poses[s] if s in g.poses else n + g.landmarks[s])

    return d, n, trow


def table(g):
    """(edge_rows [m][4] int32, edge_data [m][d*d + d + 2], range_rows [r][3] int32, range_data [r][2]) in API rows: the
    arguments of cora_set_measurements."""
    d, n, trow = _rows(g)
    E = edges(g)
    er = np.zeros((len(E), 4), dtype=np.int32)
    ed = np.zeros((len(E), d * d + d + 2))
    for i, (_, a, b, R, t, kappa, tau) in enumerate(E):
        er[i] = [d * g.poses[a], d * g.poses[b] if R is not None else -1, trow(a), trow(b)]
        if R is not None:
            ed[i, :d * d] = np.asarray(R).reshape(-1)
        ed[i, d * d:d * d + d] = t
        ed[i, d * d + d:] = [kappa, tau]
    rr = np.zeros((len(g.ranges), 3), dtype=np.int32)
    rd = np.zeros((len(g.ranges), 2))
    for m, (a, b, dist, cov) in enumerate(g.ranges):
        rr[m] = [d * n + m, trow(a), trow(b)]
        rd[m] = [dist, 1.0 / cov]
    return er, ed, rr, rd


def reference(g, X):
    """dict edge_rot, edge_trans, range (table order), sums = [sum rot, sum trans, sum range], kind = edge kinds."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    d, n, trow = _rows(g)
    E = edges(g)
    rot, trn = np.zeros(len(E)), np.zeros(len(E))
    for i, (_, a, b, R, t, kappa, tau) in enumerate(E):
        Xa = X[d * g.poses[a]:d * g.poses[a] + d]
        trn[i] = tau * np.sum((X[trow(b)] - X[trow(a)] - np.asarray(t) @ Xa) ** 2)
        if R is not None:
            Xb = X[d * g.poses[b]:d * g.poses[b] + d]
            rot[i] = kappa * np.sum((Xb - np.asarray(R).T @ Xa) ** 2)
    rng = np.zeros(len(g.ranges))
    for m, (a, b, dist, cov) in enumerate(g.ranges):
        rng[m] = np.sum((X[trow(b)] - X[trow(a)] + dist * X[d * n + m]) ** 2) / cov
    return dict(edge_rot=rot, edge_trans=trn, range=rng, sums=np.array([rot.sum(), trn.sum(), rng.sum()]),
                kind=[e[0] for e in E])


def by_kind(ref):
    """The reference split as CORA::MeasurementResiduals names it."""
    kind = np.array(ref["kind"]) if len(ref["kind"]) else np.zeros(0, dtype=str)
    pick = lambda arr, k: arr[kind == k] if len(arr) else arr
    return dict(rel_pose_rot=pick(ref["edge_rot"], "rel_pose"), rel_pose_trans=pick(ref["edge_trans"], "rel_pose"),
                pose_prior_rot=pick(ref["edge_rot"], "pose_prior"), pose_prior_trans=pick(ref["edge_trans"], "pose_prior"),
                pose_landmark=pick(ref["edge_trans"], "pose_landmark"),
                landmark_prior=pick(ref["edge_trans"], "landmark_prior"), range=ref["range"],
                rot_sum=ref["sums"][0], trans_sum=ref["sums"][1], range_sum=ref["sums"][2])
