"""The row-unit, reduction, block and mover kernels of cora_amd/csrc/kernels/rows.inc at their edges, against the plain
high-precision references of tests/rowops_ref.py.

Tolerances.  Polar factor: 2 x the worst error of the reference's own float64 SVD route on the same blocks, in units of
eps * kappa_polar, and 2 x its worst |U U^T - I| (rowops_ref.POLAR_BOUND / ORTH_BOUND, calibrated by
tests/test_rowops_ref_cpu.py, figures in profiles/rowops.md).  Sums of products: the forward-error bound of the
summation tree the kernel's code fixes, (depth) * eps * sum |a_i b_i|, stated beside each case.  eps = 2^-52.  Nothing
is filtered: every block, row and entry is asserted; the only inputs with weaker assertions are the rank-deficient ones
of test_degenerate_blocks."""
import functools

import numpy as np
import pytest

import rowops_ref as rr
import topologies as topo
from cora_amd import capi
from oracle import oracle as orc
from synth import make_problem

pytestmark = pytest.mark.gpu
EPS = rr.EPS
NPOSE = 28            # >= the longest catalogue (26 blocks at p == d)
STRIDES = [(d, p) for d in (2, 3) for p in rr.strides(d)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def problem(d, n, lm, nr, seed=1):
    if n == 1:
        A, Q, dm, _ = topo.build("n1")
        assert dm.d == d
        return A, Q, dm
    return make_problem(d=d, n=n, n_landmarks=lm, n_ranges=nr, seed=seed)


class Pool:
    """One handle per (graph, partition), shared by the module."""

    def __init__(self):
        self.ctx = {}

    def get(self, d, n, lm, nr, p=None, **kw):
        key = (d, n, lm, nr, tuple(sorted(kw.items())))
        if key not in self.ctx:
            _, Q, dm = problem(d, n, lm, nr)
            self.ctx[key] = (capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, **kw), Q, dm)
        c, Q, dm = self.ctx[key]
        if p is not None and c.p != p:
            c.set_rank(p)
        return c, Q, dm

    def close(self):
        for c, _, _ in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def pool():
    P = Pool()
    yield P
    P.close()


class Vecs:
    """Resident vectors of one test, freed at its end."""

    def __init__(self, c):
        self.c, self.ptrs = c, []

    def new(self, k, host=None, nan=False):
        ptr = self.c.dev_alloc(k)
        self.ptrs.append(ptr)
        if nan:
            poison(self.c, ptr, k)
        if host is not None:
            self.c.upload(host, ptr)
        return ptr

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for ptr in self.ptrs:
            self.c.dev_free(ptr)


def poison(c, ptr, k):
    """NaN in every API row and every column of the row stride (k = 1 has a padding column: written as k = 2)."""
    c.upload(np.full((c.N, max(k, 2) if k == 1 else k), np.nan), ptr)


GRAPH = {2: (2, NPOSE, 3, 30), 3: (3, NPOSE, 3, 30)}     # the polar / projection graph per d: one handle, every rank


# ----------------------------------------------------------------------------------------------------------------------
# polar factor, retraction, projection to the manifold
# ----------------------------------------------------------------------------------------------------------------------
RANGE_SCALES = (1e-160, 1e-100, 1e100, 1e160, 1e-60, 1e60)


@functools.lru_cache(maxsize=None)
def polar_case(d, p):
    """(A, pose entries, exact-unit range rows): the N x p input of the polar test at (d, p).  Pose i holds the block of
    catalogue entry `entries[i]` -- the families shuffled, so that neighbouring threads take different sweep counts --;
    range rows cycle through exact unit rows, ordinary rows, rows of scale 1e+-3 and rows of the six extreme scales;
    translation rows are ordinary or huge / tiny."""
    _, _, dm = problem(*GRAPH[d])
    rng = np.random.default_rng([7, d, p])
    cat = rr.catalogue(d, p)
    order = rng.permutation(len(cat))
    entries = [cat[order[i % len(cat)]] for i in range(dm.n)]
    A = rng.uniform(-1, 1, (dm.N, p))
    for i, (name, k, seed) in enumerate(entries):
        A[d * i:d * i + d] = rr.block(name, k, d, p, seed)
    unit = []
    for j in range(dm.r):
        row = dm.dn + j
        if j % 4 == 0:
            A[row] = 0.0
            A[row, rng.integers(p)] = rng.choice([-1.0, 1.0])
            unit.append(row)
        elif j % 4 == 2:
            A[row] *= 10.0 ** rng.uniform(-3, 3)
        elif j % 4 == 3:
            A[row] *= RANGE_SCALES[(j // 4) % len(RANGE_SCALES)]
    tb = dm.dn + dm.r
    A[tb + 1] *= 1e200
    A[tb + 2] *= 1e-200
    A.setflags(write=False)
    return A, entries, unit


def split_for_retract(A):
    """(Y, V) with fma(1, V, Y) == A bit for bit and V != 0: Y = A rounded to float32 (0 where that leaves its range),
    V = A - Y, which is exact."""
    with np.errstate(over="ignore"):
        Y = A.astype(np.float32).astype(np.float64)
    Y[~np.isfinite(Y) | (np.abs(A) < 1e-30)] = 0.0
    V = A - Y
    assert same_bits(Y + V, A)
    return Y, V


def five_entry_points(c, A):
    """projectToManifold(A) through the host-pointer call, the resident call out of place and in place, retract_dev at
    the point Y with (V, 1) and the host retract(Y, V), Y + V == A."""
    p = c.p
    Y, V = split_for_retract(A)
    out = {"host": c.projectToManifold(A)}
    with Vecs(c) as v:
        a, o = v.new(p, A), v.new(p, nan=True)
        c.project_to_manifold_dev(a, o)
        out["dev"] = c.download(o, p)
        c.project_to_manifold_dev(a, a)
        out["dev_inplace"] = c.download(a, p)
        c.set_point(Y)
        poison(c, o, p)
        c.upload(V, a)
        c.retract_dev(a, 1.0, o)
        out["retract_dev"] = c.download(o, p)
    out["retract_host"] = c.retract(Y, V)
    return out


def check_projection(d, dm, A, got, blocks, unit_rows=(), skip_poses=(), skip_ranges=()):
    """Every pose block of `got` against its polar factor (blocks[i] = (P, sigma)), every range row, every translation
    row.  Returns (worst polar error in eps * kappa, worst |UU^T - I|); raises with EVERY miss listed."""
    bad, worst, worst_o = [], 0.0, 0.0
    for i in range(dm.n):
        if i in skip_poses:
            continue
        P, sig = blocks[i]
        U = got[d * i:d * i + d]
        e, o = (rr.polar_error(U, P, sig), rr.orth_error(U)) if np.isfinite(U).all() else (np.inf, np.inf)
        worst, worst_o = max(worst, e), max(worst_o, o)
        if not (e <= rr.POLAR_BOUND and o <= rr.ORTH_BOUND):
            bad.append(("pose", i, "%.3g eps*kappa" % e, "orth %.3g" % o))
    rows = slice(dm.dn, dm.dn + dm.r)
    ref = rr.unit_rows(A[rows])
    nrm = np.sqrt((got[rows].astype(rr.LD) ** 2).sum(axis=1))
    for j in range(dm.r):
        if j in skip_ranges:
            continue
        if not (abs(nrm[j] - 1) <= 4 * EPS and np.abs(got[dm.dn + j] - ref[j]).max() <= 4 * EPS):
            bad.append(("range", j, "norm - 1 = %.3g" % float(nrm[j] - 1), "dir %.3g" % np.abs(got[dm.dn + j] - ref[j]).max()))
    for row in unit_rows:
        if not same_bits(got[row], A[row]):
            bad.append(("unit range row changed", row))
    if not same_bits(got[dm.dn + dm.r:], A[dm.dn + dm.r:]):
        bad.append(("translation rows changed",))
    assert not bad, bad
    return worst, worst_o


@pytest.mark.parametrize("d,p", STRIDES)
def test_polar_every_stride_every_family(d, p, pool):
    """k_project_manifold<LD, D> at every compiled stride on every block family, through all five entry points: per
    block the calibrated error and orthonormality bounds, identical bits from the five, range rows unit to 4 eps (and
    unchanged where already unit), translation rows passed through."""
    c, _, dm = pool.get(*GRAPH[d], p=p)
    A, entries, unit = polar_case(d, p)
    out = five_entry_points(c, A)
    for name, got in out.items():
        assert same_bits(got, out["host"]), name
    blocks = [rr.block_polar(name, k, d, p, seed) for name, k, seed in entries]
    worst, worst_o = check_projection(d, dm, A, out["dev"], blocks, unit)
    print("d=%d p=%d: worst polar error %.3f eps*kappa (bound %.1f), worst |UU^T - I| %.3e (bound %.2e)"
          % (d, p, worst, rr.POLAR_BOUND, worst_o, rr.ORTH_BOUND))


@pytest.mark.parametrize("k", range(len(rr.FAMILIES["scaled"])))
@pytest.mark.parametrize("d,p", [(2, 2), (3, 5)])
def test_scales(d, p, k, pool):
    """A kappa = 10 block times s and range rows times s, s = 1e-160 ... 1e160, meet the bounds of ordinary input: the
    polar factor and the unit row are scale-invariant.  (Without the scale guard of polar_rows sqrt(alpha * beta)
    under- or overflows at |s| = 1e+-100 and 1e+-160 -- profiles/rowops.md.)"""
    s = rr.FAMILIES["scaled"][k]
    c, _, dm = pool.get(*GRAPH[d], p=p)
    rng = np.random.default_rng([11, d, p])
    A = rng.uniform(-1, 1, (dm.N, p))
    for i in range(dm.n):
        A[d * i:d * i + d] = rr.block("scaled", k, d, p, i % 4)
    A[dm.dn:dm.dn + dm.r] *= s
    with Vecs(c) as v:
        a, o = v.new(p, A), v.new(p, nan=True)
        c.project_to_manifold_dev(a, o)
        got = c.download(o, p)
    blocks = [rr.block_polar("scaled", k, d, p, i % 4) for i in range(dm.n)]
    worst, worst_o = check_projection(d, dm, A, got, blocks)
    print("d=%d p=%d s=%g: worst polar error %.3f eps*kappa, worst |UU^T - I| %.3e" % (d, p, s, worst, worst_o))


@pytest.mark.parametrize("d,p", [(2, 2), (3, 3), (3, 5), (2, 24)])
def test_degenerate_blocks(d, p, pool):
    """Rank-deficient input, pinned as documented above polar_rows and in include/cora_hip.h: a zero block returns zero,
    a zero row stays zero beside orthonormal others, two identical rows and a zero range row give finite output; every
    OTHER block and row of the launch meets its bound."""
    c, _, dm = pool.get(*GRAPH[d], p=p)
    A0, entries, unit = polar_case(d, p)
    A = A0.copy()
    zero_blk, zero_row, twin = 3, 9, 20
    A[d * zero_blk:d * zero_blk + d] = 0.0
    A[d * zero_row + 1] = 0.0
    A[d * twin + 1] = A[d * twin]
    zr = 5
    A[dm.dn + zr] = 0.0
    with Vecs(c) as v:
        a, o = v.new(p, A), v.new(p, nan=True)
        c.project_to_manifold_dev(a, o)
        got = c.download(o, p)
    assert np.isfinite(got).all()
    assert not got[d * zero_blk:d * zero_blk + d].any()
    blk = got[d * zero_row:d * zero_row + d]
    assert not blk[1].any()
    rest = np.delete(blk, 1, axis=0)
    assert np.abs(rest @ rest.T - np.eye(d - 1)).max() <= rr.ORTH_BOUND
    assert not got[dm.dn + zr].any()
    blocks = [rr.block_polar(name, k, d, p, seed) for name, k, seed in entries]
    check_projection(d, dm, A, got, blocks, [r for r in unit if r != dm.dn + zr], skip_poses=(zero_blk, zero_row, twin),
                     skip_ranges=(zr,))


@pytest.mark.parametrize("d,p", [(2, 2), (3, 5), (3, 24)])
def test_retract_general_alpha(d, p, pool):
    """retract_dev(V, alpha) == projectToManifold(fma(alpha, V, Y)) bit for bit (the sum formed with one rounding on
    the host, exactly), translation rows == fma(alpha, v, y), and alpha = 0 returns Y to 4 eps."""
    c, _, dm = pool.get(*GRAPH[d], p=p)
    rng = np.random.default_rng([13, d, p])
    Y = orc.project_manifold(dm, rng.uniform(-1, 1, (dm.N, p)))
    V = rng.standard_normal((dm.N, p))
    c.set_point(Y)
    with Vecs(c) as v:
        dv, o, a = v.new(p, V), v.new(p, nan=True), v.new(p)
        for alpha in (0.0, 0.3, -2.5e3, 1e-9):
            S = rr.fma(alpha, V, Y)
            poison(c, o, p)
            c.retract_dev(dv, alpha, o)
            got = c.download(o, p)
            c.upload(S, a)
            c.project_to_manifold_dev(a, a)
            assert same_bits(got, c.download(a, p)), alpha
            assert same_bits(got[dm.dn + dm.r:], S[dm.dn + dm.r:]), alpha
            if alpha == 0.0:
                assert np.abs(got - Y).max() <= 4 * EPS


@pytest.mark.parametrize("p", [3, 5])
@pytest.mark.parametrize("n,lm,nr", [(1, 0, 0), (100, 5, 50), (100, 5, 51), (100, 5, 52), (200, 3, 110)])
def test_unit_count_edges(n, lm, nr, p, pool):
    """The row-unit kernels launch ceil(units / 256) blocks of one thread per unit, units = n + r + (n + l): 255, 256, 257
    and 513 units and a single pose.  Every output is poisoned with NaN first and must come back finite and right
    (k_project_manifold, k_tangent_project with and without the Jacobi scale, k_point_finish)."""
    d = 3
    c, Q, dm = pool.get(d, n, lm, nr, p=p)
    units = dm.n + dm.r + dm.n_trans
    assert units == {1: 7}.get(n, 2 * n + lm + nr) and (n == 1 or units in (255, 256, 257, 513))
    rng = np.random.default_rng([17, n, nr, p])
    A = rng.uniform(-1, 1, (dm.N, p))
    V = rng.standard_normal((dm.N, p))
    Y = orc.project_manifold(dm, A)
    with Vecs(c) as v:
        a, dv, o = v.new(p, A), v.new(p, V), v.new(p, nan=True)
        c.project_to_manifold_dev(a, o)
        got = c.download(o, p)
        assert np.isfinite(got).all() and np.abs(got - Y).max() < 1e-12
        c.set_point_dev(o)
        Yd = got
        rg = c.download(c.point_ptrs()[2], p)
        ref = orc.rgrad(Q, dm, Yd)
        assert np.isfinite(rg).all() and np.abs(rg - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1e-300)
        assert abs(c.point_cost() - orc.cost(Q, Yd)) <= 1e-11 * abs(orc.cost(Q, Yd))
        o2 = v.new(p, nan=True)
        c.tangent_space_projection_dev(dv, o2)
        T = c.download(o2, p)
        assert np.isfinite(T).all() and np.abs(T - rr.tangent_proj(Yd, V, d, dm.n, dm.r, dm.n_trans)).max() <= 8 * EPS * np.abs(V).max()
        poison(c, o2, p)
        c.retract_dev(dv, 0.25, o2)
        R = c.download(o2, p)
        assert np.isfinite(R).all() and np.abs(R - orc.retract(dm, Yd, 0.25 * V)).max() < 1e-12
        c.precond_setup(capi.PRECOND_JACOBI)
        poison(c, o2, p)
        c.precondition_projected_dev(dv, o2)
        J = c.download(o2, p)
        SV = V * (1.0 / Q.to_scipy().diagonal())[:, None]     # the device multiplies by 1 / diag
        assert np.isfinite(J).all() and np.abs(J - rr.tangent_proj(Yd, SV, d, dm.n, dm.r, dm.n_trans)).max() <= 8 * EPS * np.abs(SV).max()
        c.precond_setup(capi.PRECOND_NONE)


# ----------------------------------------------------------------------------------------------------------------------
# tangent projection
# ----------------------------------------------------------------------------------------------------------------------
def row_classes(dm):
    return {"pose": slice(0, dm.dn), "range": slice(dm.dn, dm.dn + dm.r), "translation": slice(dm.dn + dm.r, dm.N)}


def check_tangent(d, dm, Y, V, T, what):
    """T = Proj_Y(V) from the device: error <= 8 eps max|V| and tangency <= 16 eps max|V|, per row class."""
    ref = rr.tangent_proj(Y, V, d, dm.n, dm.r, dm.n_trans)
    Yl, Tl = Y.astype(rr.LD), T.astype(rr.LD)
    for name, rows in row_classes(dm).items():
        vmax = np.abs(V[rows]).max()
        err = np.abs(T[rows] - ref[rows]).max()
        assert err <= 8 * EPS * vmax, (what, name, err / (EPS * vmax))
    tang = 0.0
    for i in range(dm.n):
        m = Yl[d * i:d * i + d] @ Tl[d * i:d * i + d].T
        tang = max(tang, float(np.abs(m + m.T).max()) / 2)
    assert tang <= 16 * EPS * np.abs(V[:dm.dn]).max(), (what, "sym(Y^T T)", tang)
    if dm.r:
        rows = row_classes(dm)["range"]
        ip = float(np.abs((Yl[rows] * Tl[rows]).sum(axis=1)).max())
        assert ip <= 16 * EPS * np.abs(V[rows]).max(), (what, "<y, t>", ip)
    assert same_bits(T[dm.dn + dm.r:], V[dm.dn + dm.r:]), what
    return ref


@pytest.mark.parametrize("d,p", STRIDES)
def test_tangent_projection_every_stride(d, p, pool):
    """k_tangent_project<LD, D> against longdouble: the resident and the host-pointer call (same bits), tangency of the
    result, idempotence, and the Jacobi form Proj_Y(D^-1 V) of precondition_projected_dev."""
    c, Q, dm = pool.get(*GRAPH[d], p=p)
    rng = np.random.default_rng([19, d, p])
    Y = orc.project_manifold(dm, rng.uniform(-1, 1, (dm.N, p)))
    V = rng.uniform(-1, 1, (dm.N, p))
    c.set_point(Y)
    with Vecs(c) as v:
        dv, o, o2 = v.new(p, V), v.new(p, nan=True), v.new(p, nan=True)
        c.tangent_space_projection_dev(dv, o)
        T = c.download(o, p)
        check_tangent(d, dm, Y, V, T, "dev")
        c.tangent_space_projection_dev(o, o2)
        T2 = c.download(o2, p)
        for name, rows in row_classes(dm).items():
            assert np.abs(T2[rows] - T[rows]).max() <= 8 * EPS * np.abs(V[rows]).max(), ("second projection", name)
        c.precond_setup(capi.PRECOND_JACOBI)
        poison(c, o2, p)
        c.precondition_projected_dev(dv, o2)
        J = c.download(o2, p)
        c.precond_setup(capi.PRECOND_NONE)
    SV = V * (1.0 / Q.to_scipy().diagonal())[:, None]     # the device multiplies by 1 / diag
    check_tangent(d, dm, Y, SV, J, "jacobi")
    assert same_bits(c.tangent_space_projection(Y, V), T)


def test_partitioned_row_units_match_single(pool):
    """Row-partitioned handles without communication (world = 3, long rows kept whole): projection, Jacobi projection,
    retraction and project_to_manifold_dev write the single handle's bits on the shard's rows and leave every other row
    of a NaN-poisoned output alone -- the rot_base / rng_base / trn_base offsets and the scale[row - base] indexing."""
    d, n, lm, nr, p, world = 3, 90, 3, 70, 5, 3
    c1, Q, dm = pool.get(d, n, lm, nr, p=p)
    rng = np.random.default_rng(23)
    A = rng.uniform(-1, 1, (dm.N, p))
    Y = orc.project_manifold(dm, A)
    V = rng.standard_normal((dm.N, p))

    def run(c):
        res = {}
        c.set_point(Y)
        c.precond_setup(capi.PRECOND_JACOBI)
        with Vecs(c) as v:
            a, dv, o = v.new(p, A), v.new(p, V), v.new(p)
            for name, call in (("tangent", lambda: c.tangent_space_projection_dev(dv, o)),
                               ("jacobi", lambda: c.precondition_projected_dev(dv, o)),
                               ("retract", lambda: c.retract_dev(dv, 0.5, o)),
                               ("project", lambda: c.project_to_manifold_dev(a, o))):
                poison(c, o, p)
                call()
                res[name] = c.download(o, p)
        c.precond_setup(capi.PRECOND_NONE)
        return res

    single = run(c1)
    assert all(np.isfinite(x).all() for x in single.values())
    seen = np.zeros(dm.N, dtype=int)
    for rank in range(world):
        c, _, _ = pool.get(d, n, lm, nr, p=p, rank=rank, world=world, whole_long_rows=True)
        m = c.row_map()
        mine = (m >= c.shard_begin) & (m < c.shard_begin + c.shard_rows)
        seen += mine
        assert mine.any()
        for name, got in run(c).items():
            assert same_bits(got[mine], single[name][mine]), (rank, name)
            assert np.isnan(got[~mine]).all(), (rank, name)
    assert np.all(seen == 1)


# ----------------------------------------------------------------------------------------------------------------------
# inner products
# ----------------------------------------------------------------------------------------------------------------------
SMALL_ODD = (3, 1, 0, 0)       # N = 9
SMALL_EVEN = (3, 3, 1, 3)      # N = 16
LARGE = (3, 1400, 3, 100)      # N = 5703: N * 24 / 2 > 65 536 (all 256 blocks), N * 23 odd and > 65 536


def dot_bound(N, ld, mag):
    """(terms per thread + 18) eps sum|a b|: k_dots / k_dots1 add sequentially per thread (double2 elements where the
    length is even: two terms each), then an 8-level tree over the block's 256 threads, then the last block adds <= 256
    partials -- one per thread -- through the same tree: terms + 8 + 1 + 8, and one for the products' own rounding."""
    n = N * ld
    per_el = 2 if n % 2 == 0 else 1
    n2 = n // per_el
    grid = min(max((n2 + 255) // 256, 1), 256)
    terms = per_el * ((n2 + grid * 256 - 1) // (grid * 256))
    return (terms + 18) * EPS * mag


def dot_inputs(N, k, kind, seed):
    rng = np.random.default_rng([29, N, k, seed])
    a = rng.uniform(-1, 1, (N, k))
    if kind == "uniform":
        b = rng.uniform(-1, 1, (N, k))
    elif kind == "cancel":
        sign = np.where(np.arange(N * k).reshape(N, k) % 2 == 0, 1.0, -1.0)
        b = sign * a + 1e-8 * rng.standard_normal((N, k))
    else:  # columns of scale 1e8 next to columns of scale 1
        sc = np.where(np.arange(k) % 2 == 0, 1e8, 1.0)
        a, b = a * sc, rng.uniform(-1, 1, (N, k)) * sc
    return a, b


@pytest.mark.parametrize("kind", ["uniform", "cancel", "scales"])
@pytest.mark.parametrize("k", [1, 2, 5, 24, 23])
@pytest.mark.parametrize("graph", [SMALL_ODD, SMALL_EVEN, LARGE], ids=["N9", "N16", "N5703"])
def test_dot_dev(graph, k, kind, pool):
    """dot_dev on one partly filled block (N ld / 2 < 256) and on all 256 blocks, double2 kernel (N ld even) and scalar
    kernel (N ld odd: N odd and k in {5, 23}), against longdouble at the bound of dot_bound()."""
    c, _, dm = pool.get(*graph)
    a, b = dot_inputs(dm.N, k, kind, 0)
    ld = 2 if k == 1 else k
    with Vecs(c) as v:
        da, db = v.new(k, a), v.new(k, b)
        got = c.dot_dev(da, db, k)
        again = [c.dot_dev(da, db, k) for _ in range(3)]
    ref, mag = rr.dot(a, b)
    bound = dot_bound(dm.N, ld, mag)
    print("N=%d k=%d %s: |got - ref| = %.3g, bound %.3g" % (dm.N, k, kind, abs(got - ref), bound))
    assert abs(got - ref) <= bound
    assert all(x == got for x in again)


@pytest.mark.parametrize("p", [5, 24])
@pytest.mark.parametrize("graph", [SMALL_ODD, SMALL_EVEN, LARGE], ids=["N9", "N16", "N5703"])
def test_dots_dev(graph, p, pool):
    """dots_dev with 1 to 4 pairs, the two-pair form [(r, r), (r, v)] of k_dots_rr_rv against the bound and against two
    separate dot_dev calls, and fifty back-to-back calls with identical bits (the ticket is reset by the last block)."""
    c, _, dm = pool.get(*graph, p=p)
    kinds = ("uniform", "cancel", "scales", "uniform")
    with Vecs(c) as v:
        host = [dot_inputs(dm.N, p, kinds[j], j + 1) for j in range(4)]
        dev = [(v.new(p, a), v.new(p, b)) for a, b in host]
        refs = [rr.dot(a, b) for a, b in host]
        for count in (1, 2, 3, 4):
            got = c.dots_dev(dev[:count])
            for j in range(count):
                assert abs(got[j] - refs[j][0]) <= dot_bound(dm.N, p, refs[j][1]), (count, j)
        r, w = host[0][0], host[2][1]
        dr, dw = dev[0][0], dev[2][1]
        got = c.dots_dev([(dr, dr), (dr, dw)])
        (rr_ref, rr_mag), (rv_ref, rv_mag) = rr.dot(r, r), rr.dot(r, w)
        assert abs(got[0] - rr_ref) <= dot_bound(dm.N, p, rr_mag)
        assert abs(got[1] - rv_ref) <= dot_bound(dm.N, p, rv_mag)
        assert abs(got[0] - c.dot_dev(dr, dr, p)) <= dot_bound(dm.N, p, rr_mag)
        assert abs(got[1] - c.dot_dev(dr, dw, p)) <= dot_bound(dm.N, p, rv_mag)
        first = c.dots_dev(dev[:3])
        for _ in range(50):
            assert c.dots_dev(dev[:3]) == first
            assert c.dots_dev([(dr, dr), (dr, dw)]) == got


@pytest.mark.parametrize("graph", [SMALL_ODD, LARGE], ids=["N9", "N5703"])
def test_single_column_padding_stays_zero(graph, pool):
    """k = 1 lives in a row stride of 2: no operation that writes a one-column vector may leave anything in the padding
    column, which dot_dev(x, x, 1) reads.  Every output starts with NaN in BOTH columns."""
    c, Q, dm = pool.get(*graph, p=5)
    rng = np.random.default_rng(31)
    x = rng.uniform(-1, 1, (dm.N, 1))

    def sumsq_is(ptr, col):
        ref, mag = rr.dot(col, col)
        got = c.dot_dev(ptr, ptr, 1)
        assert abs(got - ref) <= dot_bound(dm.N, 2, mag), (got, ref)

    with Vecs(c) as v:
        dx, o = v.new(1, nan=True), v.new(1, nan=True)
        c.upload(x, dx)
        sumsq_is(dx, x)
        c.spmm_dev(dx, 1, o)
        sumsq_is(o, c.download(o, 1))
        assert not c.download(o, 2)[:, 1].any()
        poison(c, o, 1)
        c.combine_dev([dx], [1], [np.array([[2.0]])], 1, o)
        sumsq_is(o, 2.0 * x)
        poison(c, o, 1)
        c.fill_random_dev(1, 5, o)
        sumsq_is(o, c.download(o, 1))
        assert not c.download(o, 2)[:, 1].any()


# ----------------------------------------------------------------------------------------------------------------------
# Gram products and combinations (the LOBPCG block kernels on the fp64 matrix cores)
# ----------------------------------------------------------------------------------------------------------------------
ROW_GRAPHS = {"N9": SMALL_ODD, "N14": (2, 3, 2, 3), "N16": SMALL_EVEN, "N35": (3, 7, 2, 5), "N5703": LARGE}
WIDTHS = (1, 15, 16, 17, 24)


def gram_bound(N, mag):
    """(rows per wavefront + 12) eps sum_r |a_ri b_rj|: gram_block gives each of 1 024 wavefronts per = roundup4(ceil(rows
    / 1024)) rows, added in sequence on the matrix core; 4 wavefronts are added in order (3) and k_gram_reduce adds the
    256 blocks, one per thread, through the 8-level tree (8), and one for the products' rounding."""
    per = (-(-N // 1024) + 3) // 4 * 4
    return (per + 12) * EPS * mag


@functools.lru_cache(maxsize=None)
def block_of(N, k, seed):
    B = np.random.default_rng([37, N, k, seed]).uniform(-1, 1, (N, k))
    B[:, ::3] *= 1e3
    B.setflags(write=False)
    return B


@pytest.mark.parametrize("graph", list(ROW_GRAPHS), ids=list(ROW_GRAPHS))
def test_gram_dev(graph, pool):
    """G = A^T B at N % 4 in {0, 1, 2, 3}, N < 16, 17 <= N <= 63 and N ~ 5 000 (wavefronts with no row, a ragged last
    group of four, `per` > 4), widths over {1, 15, 16, 17, 24}^2 (one and two 16-column tiles, the padded k = 1), and
    A = B; gram_batch_dev on 16 pairs of mixed widths gives the single calls' bits."""
    c, _, dm = pool.get(*ROW_GRAPHS[graph])
    assert dm.N == int(graph[1:])
    with Vecs(c) as v:
        dev = {(k, s): v.new(k, block_of(dm.N, k, s)) for k in WIDTHS for s in (0, 1)}
        single = {}
        for ka in WIDTHS:
            for kb in WIDTHS:
                A, B = block_of(dm.N, ka, 0), block_of(dm.N, kb, 1)
                G = c.gram_dev(dev[ka, 0], ka, dev[kb, 1], kb)
                single[ka, kb] = G
                ref, mag = rr.gram(A, B)
                assert np.all(np.abs(G - ref) <= gram_bound(dm.N, mag)), (ka, kb, (np.abs(G - ref) / (EPS * mag)).max())
            A = block_of(dm.N, ka, 0)
            G = c.gram_dev(dev[ka, 0], ka, dev[ka, 0], ka)
            ref, mag = rr.gram(A, A)
            assert np.all(np.abs(G - ref) <= gram_bound(dm.N, mag)), ka
        if graph in ("N14", "N5703"):
            pairs = [(WIDTHS[i % 5], WIDTHS[(2 * i + i // 5) % 5]) for i in range(16)]
            Gs = c.gram_batch_dev([(dev[ka, 0], ka, dev[kb, 1], kb) for ka, kb in pairs])
            for (ka, kb), G in zip(pairs, Gs):
                assert same_bits(G, single[ka, kb]), (ka, kb)


def combine_bound(ks, mag):
    """(sum k_i + 2) eps sum |x| |c|: one accumulator per output element takes the sum k_i products in sequence."""
    return (sum(ks) + 2) * EPS * mag


@pytest.mark.parametrize("graph", list(ROW_GRAPHS), ids=list(ROW_GRAPHS))
def test_combine_dev(graph, pool):
    """Out = sum_i X_i C_i with 1 to 4 input blocks and kout in {1, 5, 16, 17, 24} over a NaN-poisoned output: every row
    written (ragged 16-row groups, N < 16), padding columns exactly 0, values against longdouble."""
    c, _, dm = pool.get(*ROW_GRAPHS[graph])
    rng = np.random.default_rng(41)
    ins = (24, 1, 17, 16, 15, 5)
    with Vecs(c) as v:
        dev = {k: v.new(k, block_of(dm.N, k, 0)) for k in ins}
        for kout in (1, 5, 16, 17, 24):
            o = v.new(kout)
            for nb in (1, 2, 3, 4):
                ks = [ins[(kout + nb + i) % len(ins)] for i in range(nb)]
                Cs = [rng.standard_normal((k, kout)) for k in ks]
                poison(c, o, kout)
                c.combine_dev([dev[k] for k in ks], ks, Cs, kout, o)
                got = c.download(o, max(kout, 2))
                if kout == 1:
                    assert not got[:, 1].any()
                    got = got[:, :1]
                ref, mag = rr.combine([block_of(dm.N, k, 0) for k in ks], Cs)
                assert np.isfinite(got).all(), (kout, ks)
                assert np.all(np.abs(got - ref) <= combine_bound(ks, mag)), (kout, ks)


@pytest.mark.parametrize("graph", ["N35", "N5703"])
def test_combine_coefficient_paths_agree(graph, pool):
    """Up to 400 coefficients travel in the kernel's arguments, more through a device buffer: 16 x 24 = 384 on the first
    path, and the same product with an all-zero one-column block and 24 finite coefficients appended (408) on the second,
    give identical bits.  An output that is one of the inputs is refused."""
    c, _, dm = pool.get(*ROW_GRAPHS[graph])
    rng = np.random.default_rng(43)
    X, C16 = block_of(dm.N, 16, 0), rng.standard_normal((16, 24))
    with Vecs(c) as v:
        dx, dz, o1, o2 = v.new(16, X), v.new(1, np.zeros((dm.N, 1))), v.new(24, nan=True), v.new(24, nan=True)
        c.combine_dev([dx], [16], [C16], 24, o1)
        c.combine_dev([dx, dz], [16, 1], [C16, rng.standard_normal((1, 24))], 24, o2)
        a, b = c.download(o1, 24), c.download(o2, 24)
        assert np.isfinite(a).all() and same_bits(a, b)
        ref, mag = rr.combine([X], [C16])
        assert np.all(np.abs(a - ref) <= combine_bound([16], mag))
        d16 = v.new(16, X)
        with pytest.raises(capi.CoraError) as e:
            c.combine_dev([dx, d16], [16, 16], [np.eye(16), np.eye(16)], 16, d16)
        assert e.value.code == 5


# ----------------------------------------------------------------------------------------------------------------------
# movers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5, 24])
@pytest.mark.parametrize("graph", ["N9", "N5703"])
def test_upload_download_round_trip(graph, k, pool):
    """Host column-major with a leading dimension larger than N, both ways; the host's padding rows come back untouched."""
    c, _, dm = pool.get(*ROW_GRAPHS[graph])
    rng = np.random.default_rng(47)
    src = np.asfortranarray(rng.standard_normal((dm.N + 7, k)))
    with Vecs(c) as v:
        x = v.new(k, nan=True)
        c.upload(src, x)                      # leading dimension N + 7: only the first N rows travel
        dst = np.full((dm.N + 5, k), -7.25, order="F")
        c.download(x, k, out=dst)
        assert same_bits(dst[:dm.N], src[:dm.N]) and np.all(dst[dm.N:] == -7.25)
        assert same_bits(c.download(x, k), src[:dm.N])
        if k == 1:
            assert not c.download(x, 2)[:, 1].any()
        y = v.new(k, nan=True)
        c.copy_dev(x, k, y)                   # k columns, whatever the handle's rank
        assert same_bits(c.download(y, k), src[:dm.N])


def test_row_moves(pool):
    """pack / scatter / copy of rows against numpy fancy indexing: n = 0, a few rows, a permutation of all rows."""
    import torch
    c, _, dm = pool.get(*ROW_GRAPHS["N35"])
    rng = np.random.default_rng(53)
    rows_all = int(c.rows)
    for ld in (2, 5, 24):
        X = rng.standard_normal((rows_all, ld))
        for rows in (np.zeros(0, dtype=np.int32), np.array([4, 0, 17], dtype=np.int32),
                     rng.permutation(rows_all).astype(np.int32)):
            n = len(rows)
            dX = torch.from_numpy(X).cuda()
            dR = torch.from_numpy(np.concatenate([rows, np.zeros(1, dtype=np.int32)])).cuda()
            packed = torch.full((n + 1, ld), -1.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            c.pack_rows_dev(dX.data_ptr(), ld, dR.data_ptr(), n, packed.data_ptr())
            c.sync()
            got = packed.cpu().numpy()
            assert same_bits(got[:n], X[rows]) and np.all(got[n:] == -1.0)
            fresh = rng.standard_normal((n + 1, ld))
            dF = torch.from_numpy(fresh).cuda()
            torch.cuda.synchronize()
            c.scatter_rows_dev(dF.data_ptr(), ld, dR.data_ptr(), n, dX.data_ptr())
            c.sync()
            want = X.copy()
            want[rows] = fresh[:n]
            assert same_bits(dX.cpu().numpy(), want)
            dst = torch.full((rows_all, ld), -2.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            c.copy_rows_dev(dX.data_ptr(), ld, dR.data_ptr(), n, dst.data_ptr())
            c.sync()
            want2 = np.full((rows_all, ld), -2.0)
            want2[rows] = want[rows]
            assert same_bits(dst.cpu().numpy(), want2)


def test_fill_random(pool):
    """cora_fill_random_dev's documented contract: numbers in (-1, 1) that depend on (seed, variable, column) only -- the
    same bits on a second call and on every partition of the problem --, zeros beyond column k, different seeds and
    columns differ, and mean and variance of uniform(-1, 1) within 5 sigma."""
    d, n, lm, nr = 3, 90, 3, 70
    c, _, dm = pool.get(d, n, lm, nr)
    with Vecs(c) as v:
        got = {}
        for k in (1, 5, 24):
            x = v.new(k, nan=True)
            c.fill_random_dev(k, 12345, x)
            got[k] = c.download(x, k)
            c.fill_random_dev(k, 12345, x)
            assert same_bits(c.download(x, k), got[k])
            assert np.all(np.abs(got[k]) < 1.0)
            if k == 1:
                assert not c.download(x, 2)[:, 1].any()
        assert same_bits(got[5], got[24][:, :5]) and same_bits(got[1], got[24][:, :1])    # (seed, variable, column) only
        x = v.new(24)
        c.fill_random_dev(24, 12346, x)
        other = c.download(x, 24)
        assert not np.any(other == got[24])
        cols = got[24]
        assert all(not np.any(cols[:, i] == cols[:, j]) for i in range(24) for j in range(i))
        for sample in (cols, other):
            m = sample.size
            assert abs(sample.mean()) <= 5 * np.sqrt(1.0 / 3 / m)
            assert abs((sample ** 2).mean() - 1.0 / 3) <= 5 * np.sqrt(4.0 / 45 / m)
    for rank in range(3):
        cr, _, _ = pool.get(d, n, lm, nr, rank=rank, world=3, whole_long_rows=True)
        with Vecs(cr) as v:
            x = v.new(24, nan=True)
            cr.fill_random_dev(24, 12345, x)
            assert same_bits(cr.download(x, 24), got[24]), rank


@pytest.mark.parametrize("graph", ["N9", "N16", "N5703"])
def test_axpby_axpy2(graph, pool):
    """y = a x + b y as fma(a, x, b y) bit for bit (odd and even lengths: the scalar and the double2 kernel), b = 0 over a
    NaN-filled y gives a x exactly, the k-column form at k != p, and axpy2_dev as two fused multiply-adds -- the host
    side forms each with ONE rounding in exact rational arithmetic (rowops_ref.fma)."""
    p = 5
    c, _, dm = pool.get(*ROW_GRAPHS[graph], p=p)
    rng = np.random.default_rng(59)
    N = min(dm.N, 40)       # rows compared through the exact host fma (all rows run on the device)

    def fma_rows(a, X, Y):
        return rr.fma(a, X[:N], Y[:N])

    with Vecs(c) as v:
        for k, call in ((p, lambda a, x, b, y: c.axpby_dev(a, x, b, y)), (24, lambda a, x, b, y: c.axpby_cols_dev(24, a, x, b, y)),
                        (1, lambda a, x, b, y: c.axpby_cols_dev(1, a, x, b, y))):
            X, Y = rng.standard_normal((dm.N, k)), rng.standard_normal((dm.N, k))
            dx, dy = v.new(k, X), v.new(k, Y)
            call(1.7, dx, -0.3, dy)
            got = c.download(dy, k)
            assert same_bits(got[:N], fma_rows(1.7, X, -0.3 * Y)), k
            assert np.abs(got - (1.7 * X - 0.3 * Y)).max() <= 2 * EPS * (np.abs(1.7 * X) + np.abs(0.3 * Y)).max()
            poison(c, dy, k)
            call(1.7, dx, 0.0, dy)
            assert same_bits(c.download(dy, k), 1.7 * X), k
        X1, Y1, X2, Y2 = (rng.standard_normal((dm.N, p)) for _ in range(4))
        x1, y1, x2, y2 = (v.new(p, M) for M in (X1, Y1, X2, Y2))
        c.axpy2_dev(0.37, x1, y1, -1.9e3, x2, y2)
        g1, g2 = c.download(y1, p), c.download(y2, p)
        assert same_bits(g1[:N], fma_rows(0.37, X1, Y1)) and same_bits(g2[:N], fma_rows(-1.9e3, X2, Y2))
        assert np.abs(g1 - (0.37 * X1 + Y1)).max() <= 2 * EPS * (np.abs(X1) + np.abs(Y1)).max()
        assert np.abs(g2 - (-1.9e3 * X2 + Y2)).max() <= 2 * EPS * (np.abs(1.9e3 * X2) + np.abs(Y2)).max()
