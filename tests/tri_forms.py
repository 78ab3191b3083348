"""Fixtures and reference of the staged Cholesky solve's tests (tests/test_tri_forms_cpu.py, tests/test_gpu_tri_forms.py
through tests/tri_forms_worker.py): seeded SPD matrices of a given order whose factors take every form of the solve
plan (cora_amd/csrc/trisolve.h), the factor in the layout the library takes (CSC, diagonal first), and a reference
solve that nothing of the library takes part in.  numpy / scipy only, no GPU.

Every matrix is strictly diagonally dominant (diagonal = sum of the row's magnitudes + U(0.1, 1)), so its condition
number is small and the reference's own error stays orders below the bounds the solves are held to."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spl


# ---------------------------------------------------------------- matrices
def _dominant(A, rng):
    """off-diagonal pattern (upper or full) -> symmetric, strictly diagonally dominant CSR"""
    A = sp.triu(sp.csr_matrix(A), 1)
    A = (A + A.T).tocsr()
    n = A.shape[0]
    d = np.asarray(abs(A).sum(axis=1)).ravel() + rng.uniform(0.1, 1.0, n)
    return (A + sp.diags(d)).tocsr()


def spd(n, kind, rng):
    """The structures of tests/test_trisolve_cpu.py: chain (block tridiagonal, like an odometry chain), arrow (chain + a
    few dense trailing rows: landmarks), anything else a random sparse graph Laplacian (no chain structure at all)."""
    if kind == "chain":
        A = sp.diags([np.full(n - k, -1.0 / (k + 1)) for k in range(1, 5)], list(range(1, 5)), shape=(n, n))
    elif kind == "arrow":
        A = sp.diags([np.full(n - 1, -1.0)], [1], shape=(n, n)).tolil()
        for r in range(n - 6, n):
            A[r, rng.choice(n - 6, size=(n - 6) // 2, replace=False)] = -0.01
        A = sp.triu(A.tocsr().T + A.tocsr(), 1)
    else:
        nz = 3 * n
        A = sp.coo_matrix((-rng.uniform(0.1, 1.0, nz), (rng.integers(0, n, nz), rng.integers(0, n, nz))), shape=(n, n))
        A = sp.triu(A.tocsr(), 1)
    A = (A + A.T).tocsr()
    d = np.asarray(abs(A).sum(axis=1)).ravel() + rng.uniform(0.1, 1.0, n)
    return (A + sp.diags(d)).tocsr()


def bisection_order(lo, hi, leaf, sep):
    """Nested-dissection order of the rows lo..hi-1 of a band of half-width `sep`: halves first, `sep` middle rows last;
    pieces of up to `leaf` rows stay in their own order."""
    if hi - lo <= leaf:
        return list(range(lo, hi))
    mid = (lo + hi - sep) // 2
    return bisection_order(lo, mid, leaf, sep) + bisection_order(mid + sep, hi, leaf, sep) + list(range(mid, mid + sep))


def nd_chain(n, rng, band=4, trailing=6, loops=5, leaf=16):
    """A banded chain of n - trailing rows (half-width `band`) in nested-dissection order with leaves of `leaf` rows,
    `loops` entries between far-apart rows of the chain (fill across separators, as loop closures cause), and `trailing`
    rows at the end that are coupled to half of the chain each (landmarks)."""
    nc = n - trailing
    A = sp.diags([rng.uniform(-1.0, -0.2, nc - k) for k in range(1, band + 1)], list(range(1, band + 1)), shape=(nc, nc)).tolil()
    for _ in range(loops):
        i, j = sorted(rng.choice(nc, size=2, replace=False))
        if j - i > band:
            A[i, j] = -0.5
    A = sp.bmat([[A.tocsr(), None], [None, sp.csr_matrix((trailing, trailing))]]).tolil()
    for r in range(nc, n):
        A[rng.choice(nc, size=nc // 2, replace=False), r] = -0.01
    order = np.array(bisection_order(0, nc, leaf, band) + list(range(nc, n)))
    A = _dominant(A.tocsr(), rng)
    return A[order][:, order].tocsr()


def tree(n, rng, window=40, extra=30):
    """A branching structure without any chain in it: row i < n - 1 is coupled to one random row among the `window`
    after it (its parent: a random tree, eliminated leaves first), and `extra` rows also to an ancestor further up
    (fill along the path between them)."""
    parent = np.minimum(np.arange(n - 1) + rng.integers(1, window + 1, n - 1), n - 1)
    rows, cols = list(range(n - 1)), list(parent)
    for i in rng.choice(n - 1, size=extra, replace=False):
        a = int(i)
        for _ in range(int(rng.integers(2, 6))):
            a = int(parent[a]) if a < n - 1 else a
        if a != i and a != parent[i]:
            rows.append(int(i))
            cols.append(a)
    A = sp.coo_matrix((rng.uniform(-1.0, -0.2, len(rows)), (rows, cols)), shape=(n, n))
    return _dominant(A.tocsr(), rng)


# ---------------------------------------------------------------- factors
def factor_csc(A):
    """dense Cholesky -> CSC of L with the diagonal first (structural zeros stay exact zeros)."""
    L = np.linalg.cholesky(A.toarray())
    Ls = sp.csc_matrix(np.where(np.abs(L) > 0, L, 0.0))
    Ls.sort_indices()
    return Ls


def drop_entries(Ls, rng, keep_above=0.02, keep_share=0.3):
    """An INCOMPLETE factor: every diagonal entry, every entry above keep_above and a random share of the others."""
    L = Ls.tocoo()
    keep = (L.row == L.col) | (np.abs(L.data) > keep_above) | (rng.uniform(size=L.nnz) < keep_share)
    Li = sp.csc_matrix((L.data[keep], (L.row[keep], L.col[keep])), shape=Ls.shape)
    Li.sort_indices()
    return Li


# ---------------------------------------------------------------- reference
def _ld_apply(M, X):
    """M X for a CSR matrix without an empty row, every product and sum in np.longdouble"""
    prod = M.data.astype(np.longdouble)[:, None] * np.asarray(X, dtype=np.longdouble)[M.indices]
    return np.add.reduceat(prod, M.indptr[:-1], axis=0)


class Reference:
    """(L L^T)^-1 B in float64 + one step of iterative refinement with the residual in np.longdouble (the scheme of
    tests/stpcg_ref.py).  A complete factor is built from A and the residual is B - A X: a dense Cholesky solve of the
    matrix itself.  An incomplete one (A is None) is all there is: two triangular solves with it, the residual
    B - L (L^T X).  plain(): the unrefined solve -- what the reference differs from itself by."""

    def __init__(self, Ls, A=None):
        self.Lcsr = Ls.tocsr()
        self.Ltcsr = Ls.T.tocsr()
        self.Lcsr.sort_indices()
        self.Ltcsr.sort_indices()
        self.A = None
        if A is not None:
            self.A = A.tocsr()
            self.A.sort_indices()
            self.Ld = Ls.toarray()

    def plain(self, B):
        B = np.asarray(B, dtype=np.float64)
        if self.A is not None:
            return sla.solve_triangular(self.Ld, sla.solve_triangular(self.Ld, B, lower=True), lower=True, trans="T")
        Y = spl.spsolve_triangular(self.Lcsr, B, lower=True)
        return spl.spsolve_triangular(self.Ltcsr, Y, lower=False)

    def residual(self, X, B):
        AX = _ld_apply(self.A, X) if self.A is not None else _ld_apply(self.Lcsr, _ld_apply(self.Ltcsr, X))
        return (np.asarray(B, dtype=np.longdouble) - AX).astype(np.float64)

    def solve(self, B):
        X = self.plain(B)
        return X + self.plain(self.residual(X, B))


def rel_err(got, ref):
    """max |got - ref| relative to the largest entry of the reference"""
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------- fixtures by name
# name -> (generator, order, seed).  What plan each takes under which switches is the business of tri_forms_worker.py.
FIXTURES = {
    "ndchain-1700": ("ndchain", 1700, 11),
    "ndchain-2600": ("ndchain", 2600, 12),
    "ndchain-4300": ("ndchain", 4300, 13),
    "random-1600": ("random", 1600, 1600),
    "random-2600": ("random", 2600, 2600),
    "arrow-2500": ("arrow", 2500, 2500),
    "incomplete-2600": ("incomplete", 2600, 8),
    "tree-2000": ("tree", 2000, 15),
}
RHS_COLUMNS = 24
_cache = {}


def fixture(name):
    """dict: A (CSR, None for the incomplete factor), L (CSC, diagonal first), ref (Reference), B (order x 24 right-hand
    sides), X (the reference solution).  Built once per process."""
    if name not in _cache:
        kind, n, seed = FIXTURES[name]
        rng = np.random.default_rng(seed)
        if kind == "ndchain":
            A = nd_chain(n, rng)
        elif kind == "tree":
            A = tree(n, rng)
        elif kind == "incomplete":
            A = spd(n, "random", rng)
        else:
            A = spd(n, kind, rng)
        L = factor_csc(A)
        if kind == "incomplete":
            L = drop_entries(L, rng)
            A = None
        ref = Reference(L, A)
        B = np.asfortranarray(np.random.default_rng(seed + 1).uniform(-1, 1, (n, RHS_COLUMNS)))
        _cache[name] = dict(name=name, n=n, A=A, L=L, ref=ref, B=B, X=np.asfortranarray(ref.solve(B)))
    return _cache[name]
