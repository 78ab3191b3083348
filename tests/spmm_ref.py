"""Graded floating-point data for the product kernels and a PER-ENTRY bound against a high-precision reference.

tests/spmm_exact.py holds the products to the exact result on integer data; integers cannot contain a value that rounds.
This is the second family: ordinary doubles whose magnitudes differ as real data's do, every entry of every result held
to a forward-error bound of its own -- not to 1e-10 of the largest entry of the whole result, under which a small row
can lose everything.

DATA.  A catalogue graph (tests/topologies.py), assembled by tests/assembly_ref.py with one weight per measurement
spread log-uniformly over 1e-6 .. 1e6 (the longdouble sums, rounded once to double: symmetric bit for bit, asserted).
X: standard normals times a row scale by the role of the row (rotation and range rows 1, translation rows 1e3, landmark
rows 1e-3) times a column scale log-uniform over 1e-3 .. 1e3.  The point: topologies.near_truth.

REFERENCE.  The operators of spmm_exact._Algebra -- the oracle's formulas (oracle/cora_oracle.c) -- evaluated in
np.longdouble (64-bit significand here, asserted: its own error is 2^-11 of the bounds below) and once more with absolute
values throughout: the majorant B, the sum of the magnitudes of every term that enters an entry.

BOUND.  |got - ref|_i <= c_i EPS B_i, EPS = 2^-52 = 2u.  A sum of n products of doubles, evaluated in fp64 in ANY order,
with or without FMA, differs from the exact sum by at most gamma_n sum |terms|, gamma_n = n u / (1 - n u) < n EPS / 2
(Higham, Accuracy and Stability of Numerical Algorithms, 3.1 and 3.5); an operand that carries a relative error e against
its own majorant adds e.  Counting in units of EPS gives every count below a factor 2 in hand, which covers the
(1 + gamma) cross terms and the reference's own rounding.  With nnz_i the stored entries of row i, nnzb the largest nnz
over the d rows of a pose's block (over the one row, for a range row):

  Q X             c_i = nnz_i                                  one product and one addition per stored entry
  Lambda blocks   c   = nnzb + p + d^2                         G = Q Y (nnzb), p products per entry of G_i Y_i^T, the sum
                                                               of sym (x0.5 is exact); d^2 is the issue's allowance for
                                                               the block product, above the 1 the sum needs
  (Q - Lambda) X  c_i = nnz_i + c_Lambda + d^2 + S_ROUND       the row's products, Lambda's error against its majorant,
                                                               d more products Lambda_i X_i, and S_ROUND = 2 for a STORED
                                                               S block: Q_ii - Lambda_i is rounded when the fold writes it
                                                               (cora_amd/csrc/kernels/spmm.inc, the folded S blocks)
                        translation and landmark rows: nnz_i   (Lambda has no entry there)
  Proj_Y W        c   = p + d^2 + 2                            p products per entry of Y_i W_i^T, sym, d products, the
                                                               subtraction
  Hvp             c_i = max over the block's rows of c_(Q - Lambda)V  +  p + d^2 + 2
                                                               the projection is linear and its majorant is monotone: an
                                                               error of c EPS H'maj in H' = (Q - Lambda) V comes out below
                                                               c EPS B; then the projection's own roundings.
                        translation and landmark rows: nnz_i
  f = <Y, Q Y>/2  c   = max_i nnz_i + N p                      G's error, then a sum of N p products

None of these figures comes from a run of the code under test.  Nothing is filtered: `check` asserts every entry.
numpy only (plus the oracle for near_truth); no GPU."""
import numpy as np

import assembly_ref as aref
import topologies as topo
from oracle import oracle as orc
from spmm_exact import _Algebra

EPS = 2.0 ** -52
S_ROUND = 2
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no wider than double here: no reference"

ENTRIES = ("robots-d2", "robots-d3", "hub-d3", "near_hub", "fat_landmark", "priors_wide", "dups", "n1", "n65")
WIDE = (5, 9, 24)


def ranks(d):
    return (d,) + WIDE


class _RowSums:
    """A CSR matrix of any dtype with the one operation the algebra needs: M @ X, row by row over the stored entries."""

    def __init__(self, rowptr, col, val):
        assert np.all(np.diff(rowptr) > 0)   # (every row holds its diagonal: reduceat needs no empty row)
        self.start, self.col, self.val = np.asarray(rowptr[:-1], dtype=np.int64), np.asarray(col, dtype=np.int64), val

    def __matmul__(self, X):
        return np.add.reduceat(self.val[:, None] * X[self.col], self.start, axis=0)


def weighted_matrix(name, seed=0):
    """(Q with the weighted values, dm): weights 10^U(-6, 6) per measurement, assembled in longdouble, rounded once."""
    g, Q, dm, ref = aref.graph(name)
    w = 10.0 ** np.random.default_rng(4000 + seed).uniform(-6.0, 6.0, ref.n_weights)
    vals = ref.evaluate(w)[0].astype(np.float64)
    Qw = orc.CSR(Q.rowptr, Q.col, vals, dm.N)
    M = Qw.to_scipy()
    assert abs(M - M.T).max() == 0.0
    return Qw, dm


def graded_block(dm, k, rng):
    """N x k doubles: N(0, 1) times the row's scale (rotation, range 1; translation 1e3; landmark 1e-3) times a column scale
    10^U(-3, 3)."""
    row = np.ones(dm.N)
    tb = dm.dn + dm.r
    row[tb:tb + dm.n] = 1e3
    row[tb + dm.n:] = 1e-3
    colscale = 10.0 ** rng.uniform(-3.0, 3.0, k)
    return np.asfortranarray(rng.standard_normal((dm.N, k)) * row[:, None] * colscale[None, :])


class Counts:
    """The c_i of the module's docstring for one matrix and rank."""

    def __init__(self, Q, dm, p):
        d = dm.d
        nnz = np.diff(Q.rowptr).astype(np.float64)
        nnzb = nnz.copy()
        nnzb[:dm.dn] = np.repeat(nnz[:dm.dn].reshape(dm.n, d).max(axis=1), d)
        curved = np.arange(dm.N) < dm.dn + dm.r
        self.qx = nnz
        self.lam_st = nnzb[:dm.dn:d] + p + d * d                 # per pose block
        self.lam_ob = nnz[dm.dn:dm.dn + dm.r] + p + d * d
        lam = nnzb + p + d * d
        self.sx = np.where(curved, nnz + lam + d * d + S_ROUND, nnz)
        sxb = self.sx.copy()
        sxb[:dm.dn] = np.repeat(self.sx[:dm.dn].reshape(dm.n, d).max(axis=1), d)
        self.proj = np.where(curved, p + d * d + 2.0, 0.0)
        self.hvp = np.where(curved, sxb + p + d * d + 2, nnz)
        self.f = nnz.max() + dm.N * p


def check(what, got, ref, B, c):
    """Asserts |got - ref| <= c EPS B on EVERY entry (c per row, or a scalar); returns the worst err / bound."""
    got = np.asarray(got, dtype=np.float64)
    ref, B = np.asarray(ref), np.asarray(B, dtype=np.float64)
    assert got.shape == ref.shape == B.shape, (what, got.shape, ref.shape, B.shape)
    c = np.asarray(c, dtype=np.float64)
    if c.ndim == 1 and got.ndim == 2:
        c = c[:, None]
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    bound = c * EPS * B
    assert np.all(np.isfinite(got)), what
    bad = np.argwhere(err > bound)
    assert len(bad) == 0, "%s: %d of %d entries outside their bound, first at %s: got %r, reference %r, bound %g" % (
        what, len(bad), err.size, tuple(bad[0]), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]),
        float(np.broadcast_to(bound, err.shape)[tuple(bad[0])]))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    return float(ratio.max(initial=0.0))


def _layout(dm, L2):
    """n x d x d blocks -> d x dn as the oracle and the library lay Lambda's Stiefel blocks out."""
    return L2.transpose(1, 0, 2).reshape(dm.d, dm.dn)


_CASES = {}


def case(name, p):
    """The data, the longdouble references and their majorants of one (entry, rank), built once per process and left
    unchanged.  Keys: Q dm Y X V G (doubles; G = the reference Q Y rounded once, what the host-pointer Hvp is given) and,
    each as (reference, majorant, c): qx lam_st lam_ob sx hv f proj (of the raw V0)."""
    if (name, p) in _CASES:
        return _CASES[name, p]
    Q, dm = weighted_matrix(name)
    rng = np.random.default_rng(5000 + p)
    L = np.longdouble
    Y = np.asfortranarray(topo.near_truth(name, p))
    X = graded_block(dm, p, rng)
    V0 = graded_block(dm, p, rng)
    ex = _Algebra(_RowSums(Q.rowptr, Q.col, Q.val.astype(L)), dm, -1)
    mj = _Algebra(_RowSums(Q.rowptr, Q.col, np.abs(Q.val)), dm, +1)
    V = np.asfortranarray(orc.tangent_proj(dm, Y, V0))   # a double tangent vector (its own rounding is the INPUT's)
    c = Counts(Q, dm, p)
    R = dict(Q=Q, dm=dm, Y=Y, X=X, V=V, V0=V0, counts=c)
    out = {}
    for alg, cast in ((ex, lambda a: a.astype(L)), (mj, np.abs)):
        y, x, v, v0 = cast(Y), cast(X), cast(V), cast(V0)
        G = alg.spmm(y)
        L2, ob = alg.lambda2(y, G)
        out[alg.s] = dict(qx=alg.spmm(x), G=G, lam_st=_layout(dm, L2) / 2, lam_ob=ob,
                          sx=alg.minus_lambda2(alg.spmm(x), L2, ob, x) / 2, hv=alg.hvp4(y, v) / 4,
                          proj=alg.proj2(y, v0) / 2, f=np.sum(y * G) / 2)
    for key, cc in (("qx", c.qx), ("lam_st", np.repeat(c.lam_st, dm.d)[None, :]), ("lam_ob", c.lam_ob), ("sx", c.sx),
                    ("hv", c.hvp), ("proj", c.proj), ("f", c.f)):
        R[key] = (out[-1][key], np.asarray(out[+1][key], dtype=np.float64), cc)
    R["G"] = np.asfortranarray(out[-1]["G"].astype(np.float64))
    _CASES[name, p] = R
    return R
