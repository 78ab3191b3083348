"""Integer data on which every product of this project is EXACT in fp64, and the exact reference in integer arithmetic.

The format (cora_amd/csrc/format_build.cpp) asks of Q only that it equals its transpose bit for bit, so the values of any
catalogue matrix can be replaced on the unchanged pattern.  With Q, the point Y and the vectors X, V all integers, Q X,
the Lambda blocks sym((QY)_i Y_i^T) and <y_j, (QY)_j>, S X = Q X - Lambda X, the tangent projection and the Hessian-vector
product (oracle/cora_oracle.c, orc_tangent_proj .. orc_hvp) use only +, -, x and x0.5: every intermediate value is an
integer multiple of 2^-SHIFT.  While the SAME expression evaluated with absolute values throughout (the majorant), counted
in units of 2^-SHIFT, stays below 2^52, every partial sum of every summation order, with or without FMA, is such a
multiple below 2^53 and therefore a double: fp64 arithmetic commits no rounding at all and a correct implementation
returns the integer result bit for bit.  That is a theorem about the data, not a measurement; `Exact` returns the
majorant beside every result and the tests assert it.

The reference works in int64 row by row over the CSR (scipy's csr product on integer arrays); the majorant below 2^52
also rules out a wrap of int64.  The majorants are evaluated in float64: all terms are non-negative, so their relative
error is below 1e-10, and the exactness argument holds up to 2^53.

numpy and scipy only; nothing here needs a GPU or calls the library under test."""
import numpy as np
import scipy.sparse as sp

from oracle import oracle as orc

LIMIT = 2.0 ** 52
# (grade of Q, row grade of X / V0) per operator; tests/test_spmm_exact_cpu.py asserts the certificates they give on every
# catalogue entry and stride, profiles/spmm_exact.md lists the largest.  Q X: products of 7 * 2^30 by 4 * 2^7 summed
# over a row of at most 2^14 entries.  The operators at a point pass through Lambda V (Lambda itself a row sum of Q)
# and carry SHIFT = 2 (Hvp) more bits; the scalar <g, H g> of the STPCG case sums N p such entries times g, and sets the
# grades of every operator at a point.
GRADES = {"qx": (30, 7), "point": (16, 4)}


def integer_matrix(Q, rng, grade):
    """The pattern of Q with one value per unordered index pair {i, j}: mantissa in +-{1..7} times 2^e, e in 0..grade.
    Symmetric bit for bit (the pattern of Q is symmetric: asserted)."""
    N = Q.N
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(Q.rowptr))
    cols = Q.col.astype(np.int64)
    keys = np.minimum(rows, cols) * N + np.maximum(rows, cols)
    uniq, inv, counts = np.unique(keys, return_inverse=True, return_counts=True)
    lo, hi = uniq // N, uniq % N
    assert np.all(counts == np.where(lo == hi, 1, 2)), "the pattern of Q is not symmetric"
    mant = rng.integers(1, 8, len(uniq)) * rng.choice([-1, 1], len(uniq))
    vals = (mant * 2 ** rng.integers(0, grade + 1, len(uniq))).astype(np.float64)
    return orc.CSR(Q.rowptr, Q.col, vals[inv], N)


def integer_block(N, k, rng, row_grade):
    """N x k integers: entries -4..4 times a per-row 2^e, e in 0..row_grade (int64)."""
    scale = 2 ** rng.integers(0, row_grade + 1, (N, 1))
    return (rng.integers(-4, 5, (N, k)) * scale).astype(np.int64)


def frame_point(dm, p, rng):
    """A point exactly on the manifold at rank p (int64, N x p): the d rotation rows of each pose are +- distinct
    coordinate vectors of R^p, each range row is one +- coordinate vector, translation and landmark rows are integers in
    -3..3.  The oracle's projection onto the manifold leaves its rotation and range rows unchanged (asserted)."""
    Y = np.zeros((dm.N, p), dtype=np.int64)
    for i in range(dm.n):
        axes = rng.choice(p, size=dm.d, replace=False)
        Y[dm.d * i + np.arange(dm.d), axes] = rng.choice([-1, 1], dm.d)
    if dm.r:
        Y[dm.dn + np.arange(dm.r), rng.integers(0, p, dm.r)] = rng.choice([-1, 1], dm.r)
    tb = dm.dn + dm.r
    Y[tb:] = rng.integers(-3, 4, (dm.N - tb, p))
    back = orc.project_manifold(dm, Y.astype(np.float64))
    assert np.array_equal(back[:tb], Y[:tb].astype(np.float64)), "the frame point is not a fixed point of the projection"
    return Y


def f64(a, shift=0):
    """The double an integer array stands for: a / 2^shift, column-major.  Exact below 2^53."""
    return np.asfortranarray(np.asarray(a, dtype=np.float64) / float(2 ** shift))


def _blocks(dm, A):
    return A[:dm.dn].reshape(dm.n, dm.d, A.shape[1])


def _sym2(P, s):
    """2 sym(P) per block (s = -1) or its majorant |P| + |P|^T (s = +1): the same sum either way."""
    return P + P.transpose(0, 2, 1)


class _Algebra:
    """The operators once, for the integers (s = -1: a - b) and for the majorant (s = +1: |a| + |b|)."""

    def __init__(self, M, dm, s):
        self.M, self.dm, self.s = M, dm, s

    def spmm(self, X):
        return self.M @ X

    def lambda2(self, Y, G):
        """2 sym(G_i Y_i^T) as n x d x d, and <y_j, g_j> over the range rows."""
        dm = self.dm
        P = np.einsum("nap,nbp->nab", _blocks(dm, G), _blocks(dm, Y))
        return _sym2(P, self.s), np.sum(Y[dm.dn:dm.dn + dm.r] * G[dm.dn:dm.dn + dm.r], axis=1)

    def minus_lambda2(self, H, L2, ob, X):
        """2 (H - Lambda X): rotation rows 2 H_i - L2_i X_i, range rows 2 h_j - 2 ob_j x_j, the others 2 H."""
        dm, s = self.dm, self.s
        out = 2 * H
        out[:dm.dn] += s * np.einsum("nab,nbp->nap", L2, _blocks(dm, X)).reshape(dm.dn, -1)
        out[dm.dn:dm.dn + dm.r] += s * 2 * ob[:, None] * X[dm.dn:dm.dn + dm.r]
        return out

    def proj2(self, Y, W):
        """2 Proj_Y(W): rotation rows 2 W_i - 2 sym(Y_i W_i^T) Y_i, range rows 2 w_j - 2 <y_j, w_j> y_j, the others 2 W."""
        dm, s = self.dm, self.s
        out = 2 * W
        P = np.einsum("nap,nbp->nab", _blocks(dm, Y), _blocks(dm, W))
        out[:dm.dn] += s * np.einsum("nab,nbp->nap", _sym2(P, s), _blocks(dm, Y)).reshape(dm.dn, -1)
        rg = slice(dm.dn, dm.dn + dm.r)
        out[rg] += s * 2 * np.sum(Y[rg] * W[rg], axis=1)[:, None] * Y[rg]
        return out

    def hvp4(self, Y, V):
        """4 Hess(V) as orc_hvp restates src/CORA_problem.cpp:822-867, with G = Q Y."""
        G = self.spmm(Y)
        L2, ob = self.lambda2(Y, G)
        return self.proj2(Y, self.minus_lambda2(self.spmm(V), L2, ob, V))


class Exact:
    """The exact operators of one integer matrix.  Every method returns (result, certificate): the result as int64
    in units of 2^-shift (the shift is in the method's name and docstring), the certificate the largest entry of the same
    expression evaluated with absolute values, in the same units.  Below LIMIT = 2^52 the result is what fp64 gives."""

    def __init__(self, Q, dm):
        assert np.all(Q.val == np.rint(Q.val)) and np.abs(Q.val).max() < 2.0 ** 40
        self.Q, self.dm = Q, dm
        Mi = sp.csr_matrix((Q.val.astype(np.int64), Q.col, Q.rowptr), shape=(Q.N, Q.N))
        Ma = sp.csr_matrix((np.abs(Q.val), Q.col, Q.rowptr), shape=(Q.N, Q.N))
        self.ex, self.mj = _Algebra(Mi, dm, -1), _Algebra(Ma, dm, +1)

    @staticmethod
    def _both(X):
        X = np.asarray(X)
        assert X.dtype == np.int64
        return X, np.abs(X).astype(np.float64)

    @staticmethod
    def _cert(*arrays):
        return float(max([np.abs(a).max(initial=0.0) for a in arrays]))

    def spmm(self, X):
        """Q X (shift 0)."""
        X, Xa = self._both(X)
        return self.ex.spmm(X), self._cert(self.mj.spmm(Xa))

    def lambda_blocks2(self, Y):
        """(2 Lst as d x dn in the oracle's layout, lob): shift 1 for the Stiefel blocks, 0 for the oblique entries."""
        Y, Ya = self._both(Y)
        dm = self.dm
        L2, ob = self.ex.lambda2(Y, self.ex.spmm(Y))
        L2a, oba = self.mj.lambda2(Ya, self.mj.spmm(Ya))
        st2 = L2.transpose(1, 0, 2).reshape(dm.d, dm.dn)   # st2[a, d i + b] = L2[i, a, b]
        return (st2, ob), self._cert(L2a, oba)

    def S_apply2(self, Y, X):
        """2 (Q - Lambda(Y)) X (shift 1)."""
        Y, Ya = self._both(Y)
        X, Xa = self._both(X)
        out = []
        for alg, y, x in ((self.ex, Y, X), (self.mj, Ya, Xa)):
            L2, ob = alg.lambda2(y, alg.spmm(y))
            out.append(alg.minus_lambda2(alg.spmm(x), L2, ob, x))
        return out[0], self._cert(out[1])

    def tangent_proj2(self, Y, W):
        """2 Proj_Y(W) (shift 1)."""
        Y, Ya = self._both(Y)
        W, Wa = self._both(W)
        return self.ex.proj2(Y, W), self._cert(self.mj.proj2(Ya, Wa))

    def hvp4(self, Y, V):
        """4 Hess_Y(V) (shift 2)."""
        Y, Ya = self._both(Y)
        V, Va = self._both(V)
        return self.ex.hvp4(Y, V), self._cert(self.mj.hvp4(Ya, Va))

    def cost2(self, Y):
        """2 f = <Y, Q Y> (shift 1): a Python int."""
        Y, Ya = self._both(Y)
        return int(np.sum(Y * self.ex.spmm(Y))), float(np.sum(Ya * self.mj.spmm(Ya)))

    def curvature4(self, Y, V):
        """4 <V, Hess_Y(V)> (shift 2): a Python int."""
        Y, Ya = self._both(Y)
        V, Va = self._both(V)
        return int(np.sum(V * self.ex.hvp4(Y, V))), float(np.sum(Va * self.mj.hvp4(Ya, Va)))


_CASES = {}


def case(Q, dm, key, p, k=None, op="point", sign=1):
    """The shared data of one (graph, stride): built once per process from `key` (any hashable naming the graph) and left
    unchanged.  Qi the integer matrix, Y a frame point, X an integer block of k columns (default p), V = 2 Proj_Y(V0) an
    integer tangent vector, and the exact results as doubles with their certificates in `cert`.  sign = -1: the same case
    with -Qi (as symmetric and as integral as Qi)."""
    k = p if k is None else k
    ck = (key, p, k, op, sign)
    if ck in _CASES:
        return _CASES[ck]
    grade, row_grade = GRADES[op]
    base = sum(ord(c) for c in str(key)) * 1009 + 31 * p   # (no hash(): the same data in every process)
    Qi = integer_matrix(Q, np.random.default_rng(base + 7 * sorted(GRADES).index(op)), grade)   # one matrix for every k
    Qi.val *= sign
    rng = np.random.default_rng(base + 1000003 * k)
    E = Exact(Qi, dm)
    R = dict(Qi=Qi, E=E, cert={})
    X = integer_block(dm.N, k, rng, row_grade)
    qx, R["cert"]["qx"] = E.spmm(X)
    R.update(X=f64(X), qx=f64(qx))
    if op != "qx":
        Y = frame_point(dm, p, rng)
        Xp = integer_block(dm.N, p, rng, row_grade)
        V, c0 = E.tangent_proj2(Y, integer_block(dm.N, p, rng, row_grade))
        (st2, ob), R["cert"]["lambda"] = E.lambda_blocks2(Y)
        sx2, R["cert"]["sx"] = E.S_apply2(Y, Xp)
        hv4, R["cert"]["hvp"] = E.hvp4(Y, V)
        f2, R["cert"]["f"] = E.cost2(Y)
        G, R["cert"]["g"] = E.spmm(Y)
        R["cert"]["v"] = c0
        R.update(Yi=Y, Vi=V, Y=f64(Y), V=f64(V), Xp=f64(Xp), G=f64(G), st=f64(st2, 1), ob=f64(ob).ravel(), sx=f64(sx2, 1),
                 hv=f64(hv4, 2), f=f2 / 2.0)
    _CASES[ck] = R
    return R


def gradient_case(Q, dm, key, p):
    """One interior STPCG iteration without a preconditioner on the point's grades: an integer tangent gradient g with
    exact positive curvature <g, H g>, the exact H g, <g, g> and <g, H g>, every certificate in `cert`.  A random
    symmetric integer matrix is indefinite, and the Hessian is linear in Q: where the draw of g has negative curvature
    the case is the one of -Qi."""
    ck = (key, p, "gradient")
    if ck in _CASES:
        return _CASES[ck]
    R = case(Q, dm, key, p, op="point")
    rng = np.random.default_rng(77 + p)
    g, cg = R["E"].tangent_proj2(R["Yi"], integer_block(dm.N, p, rng, GRADES["point"][1]))
    k4, ck4 = R["E"].curvature4(R["Yi"], g)
    assert k4 != 0
    if k4 < 0:
        R = case(Q, dm, key, p, op="point", sign=-1)
        k4, ck4 = R["E"].curvature4(R["Yi"], g)
    assert k4 > 0
    R = dict(R)
    hg4, ch = R["E"].hvp4(R["Yi"], g)
    rr = int(np.sum(g * g))
    R["cert"] = dict(R["cert"], grad=cg, hg=ch, rr=float(rr), kappa=ck4)
    R.update(g=f64(g), hg=f64(hg4, 2), rr=float(rr), kappa=k4 / 4.0)
    _CASES[ck] = R
    return R

KAPPA_MAX_P = 12   # topologies_worker.KAPPA_MAX_P: the strides at which the device STPCG is run


def point_case(Q, dm, key, p):
    """The operators at a point of (graph, stride): with the STPCG iteration's data where the device test runs one."""
    return gradient_case(Q, dm, key, p) if p <= KAPPA_MAX_P else case(Q, dm, key, p, op="point")


# ---- the cases of tests/test_gpu_spmm_exact.py, listed here so that tests/test_spmm_exact_cpu.py certifies the same ones
QX_SUBSET = ("fat_landmark", "priors_wide", "hub-d3", "robots-d2", "n65")   # long rows, the plain slice, two slices
QX_COLS = (1, 2, 10)
LONG_QX_COLS = (2, 5, 10)
LONG_HVP_P = (3, 5)
REPEATED = ("robots-d3", "fat_landmark")        # once more under the forced stagger and after update_values
PARTITIONED = ("robots-d3", "hub-d3", "fat_landmark")
PARTITION_P = 5


def device_cases():
    """(key, Q, dm, p, k, op) of every case the device test runs; op in qx | point | gradient."""
    import long_rows_graphs as lrg
    import topologies as topo
    import topologies_worker as W
    assert KAPPA_MAX_P == W.KAPPA_MAX_P
    for name in topo.NAMES:
        A, Q, dm, g = topo.build(name)
        for p in W.strides(dm.d):
            yield name, Q, dm, p, p, "qx"
            yield name, Q, dm, p, p, "gradient" if p <= KAPPA_MAX_P else "point"
        if name in QX_SUBSET:
            for k in QX_COLS:
                yield name, Q, dm, dm.d, k, "qx"
        if name in REPEATED:   # the second matrix of the update
            yield name + "#2", Q, dm, 5, 5, "qx"
            yield name + "#2", Q, dm, 5, 5, "point"
    for name in lrg.NAMES:
        A, Q, dm = lrg.build(name)
        for k in LONG_QX_COLS:
            yield "long-" + name, Q, dm, 5, k, "qx"
        for p in LONG_HVP_P:
            yield "long-" + name, Q, dm, p, p, "point"
