"""numpy reference of Q(w) as a sum of per-measurement terms over oracle.assemble.PyFG -- TEST INFRASTRUCTURE ONLY.

Q is linear in the measurement weights.  With the table of residuals_ref.table (API rows), rows (ra, rb, ta, tb) and data
(R, t, kappa, tau) of an edge, rows (q, ta, tb) and data (r, omega) of a range, the terms are
  rotation of edge e (rb >= 0), weight e:     kappa at (ra+k, ra+k) and (rb+k, rb+k), k < d;
                                              -kappa R[a, c] at (ra+a, rb+c) and (rb+c, ra+a)
  translation of edge e, weight n_edges + e:  tau v_i v_j over all pairs of rows (ra .. ra+d-1, ta, tb), v = (-t, -1, +1)
  range m, weight 2 n_edges + m:              omega v_i v_j over all pairs of rows (q, ta, tb), v = (r, -1, +1)
-- the operators of oracle/assemble.py:160-230 written out entry by entry.  The sums are formed in np.longdouble.

TOLERANCE of a double-precision assembly against this reference, per entry:
    |got - ref| <= (n_terms + 3) eps sum |coef w|
the forward error bound of an n-term sum (n - 1 additions), two roundings of the coefficient (the precision times the
product v_i v_j) and one for the weight.  Derived, not measured."""
import numpy as np

import residuals_ref as rr

EPS = np.finfo(np.float64).eps


def n_weights(g):
    return 2 * len(rr.edges(g)) + len(g.ranges)


def terms(g):
    """(rows, cols, weight index, coefficient as longdouble) of every term, arrays."""
    d = g.dim
    er, ed, rg, rd = rr.table(g)
    ne = len(er)
    L = np.longdouble
    I, J, W, Cf = [], [], [], []

    def emit(i, j, w, c):
        I.append(int(i)); J.append(int(j)); W.append(int(w)); Cf.append(c)

    for e in range(ne):
        ra, rb, ta, tb = (int(x) for x in er[e])
        R = ed[e, :d * d].reshape(d, d)
        t = ed[e, d * d:d * d + d]
        kappa, tau = L(ed[e, d * d + d]), L(ed[e, d * d + d + 1])
        if rb >= 0:
            for k in range(d):
                emit(ra + k, ra + k, e, kappa)
                emit(rb + k, rb + k, e, kappa)
            for a in range(d):
                for c in range(d):
                    emit(ra + a, rb + c, e, -kappa * L(R[a, c]))
                    emit(rb + c, ra + a, e, -kappa * L(R[a, c]))
        u = [ra + k for k in range(d)] + [ta, tb]
        v = [-L(x) for x in t] + [L(-1.0), L(1.0)]
        for i in range(d + 2):
            for j in range(d + 2):
                emit(u[i], u[j], ne + e, tau * v[i] * v[j])
    for m in range(len(rg)):
        u = [int(x) for x in rg[m]]
        v = [L(rd[m, 0]), L(-1.0), L(1.0)]
        for i in range(3):
            for j in range(3):
                emit(u[i], u[j], 2 * ne + m, L(rd[m, 1]) * v[i] * v[j])
    return (np.array(I, dtype=np.int64), np.array(J, dtype=np.int64), np.array(W, dtype=np.int64),
            np.array(Cf, dtype=np.longdouble))


def positions(rowptr, col, N, I, J):
    """CSR position of every (I, J), -1 where the pattern does not hold it (rows may be unsorted)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    key = rows * N + col
    order = np.argsort(key, kind="stable")
    skey = key[order]
    want = I * N + J
    at = np.searchsorted(skey, want)
    at[at >= len(skey)] = 0
    hit = skey[at] == want if len(skey) else np.zeros(len(want), dtype=bool)
    return np.where(hit, order[at] if len(skey) else -1, -1)


class Reference:
    """The terms of a graph over a CSR pattern, computed once; evaluate(w) is cheap."""

    def __init__(self, g, rowptr, col, N):
        I, J, W, Cf = terms(g)
        pos = positions(rowptr, col, N, I, J)
        outside = pos < 0
        assert np.all(Cf[outside] == 0), "a nonzero term falls outside the pattern"
        keep = ~outside
        self.nnz = int(np.asarray(rowptr)[-1])
        self.pos, self.w, self.coef = pos[keep], W[keep], Cf[keep]
        self.n_terms = np.bincount(self.pos, minlength=self.nnz)
        self.n_weights = n_weights(g)

    def evaluate(self, w):
        """(sum of coef w per entry as longdouble, sum |coef w| per entry as float64)."""
        w = np.asarray(w, dtype=np.float64)
        assert len(w) == self.n_weights
        prod = self.coef * w[self.w].astype(np.longdouble)
        ref = np.zeros(self.nnz, dtype=np.longdouble)
        np.add.at(ref, self.pos, prod)
        mag = np.zeros(self.nnz, dtype=np.longdouble)
        np.add.at(mag, self.pos, np.abs(prod))
        return ref, mag.astype(np.float64)

    def check(self, got, w, what=""):
        """Asserts the bound on every entry; returns the worst ratio |got - ref| / bound."""
        ref, mag = self.evaluate(w)
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == (self.nnz,)
        err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        bound = (self.n_terms + 3) * EPS * mag
        bad = np.nonzero(err > bound)[0]
        assert len(bad) == 0, (what, int(bad[0]), float(got[bad[0]]), float(ref[bad[0]]), float(bound[bad[0]]), len(bad))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, 0.0)
        return float(ratio.max()) if len(ratio) else 0.0


# ---- the graphs the assembly tests share ------------------------------------------------------------------------------
K_LONG_ENTRY = 128   # cora_internal.h kLongEntry: entries with more terms are summed by a wavefront
STAR_SIZES = (K_LONG_ENTRY - 1, K_LONG_ENTRY, K_LONG_ENTRY + 1, 2 * K_LONG_ENTRY + 1, 64 * 3 + 5)
TOPOLOGIES = ("pp_only", "hub-d2", "hub-d3", "fat_landmark", "dups", "rplm_priors", "priors_wide", "lm_lm", "n1", "n2")


def star(K, d=2):
    """Nine poses and ONE landmark with K ranges to it: the landmark's diagonal entry is a sum of exactly K terms, the
    longest entry of the graph (a pose's diagonal has K / 9 + a few)."""
    import topologies as tp
    w = tp.World(d, 300 + K)
    idx = w.robot("A", 9)
    w.odometry(idx)
    lm = w.landmarks(1)[0]
    for k in range(K):
        w.range(w.names[idx[k % 9]], lm)
    return w.g


def random_weights(n, seed):
    """n weights in [0.25, 2), about a fifth of them exactly 0."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.25, 2.0, n) * (rng.uniform(size=n) > 0.2)


_GRAPHS = {}


def graph(name):
    """(g, Q, dm, Reference) of a named graph, built once per process: a golden case, "plaza2", a topologies entry or
    "star<K>[-d3]"."""
    import os
    from oracle import assemble as asm
    from oracle import oracle as orc
    if name not in _GRAPHS:
        golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        if name.startswith("star"):
            K, _, dd = name[4:].partition("-d")
            g = star(int(K), int(dd or 2))
        elif name == "plaza2":
            g = asm.parse_pyfg(os.path.join(golden, "datasets", "plaza2.pyfg"))
        elif os.path.isdir(os.path.join(golden, name)):
            g = asm.parse_pyfg(os.path.join(golden, name, "factor_graph.pyfg"))
        else:
            import topologies as tp
            g = tp.build(name)[3]
        A = asm.assemble(g)
        Q = orc.CSR.from_scipy(A["Q"])
        dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
        _GRAPHS[name] = (g, Q, dm, Reference(g, Q.rowptr, Q.col, dm.N))
    return _GRAPHS[name]
