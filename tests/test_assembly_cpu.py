"""Q(w) assembled from per-measurement weights, without a GPU: the term map (cora_assembly_build) executed on the host in
the device's order (cora_debug_assemble_values_host, cora_assemble_values on plan-only handles) against the longdouble
reference of tests/assembly_ref.py, within its derived bound (n_terms + 3) eps sum |coef w| per entry."""
import os

import numpy as np
import pytest

import assembly_ref as ar
import residuals_ref as rr
from conftest import CASES, GOLDEN
from cora_amd import capi

ERR_ARG, ERR_NOT_READY = 5, 2
KS = (1, 3, 8)
GRAPHS = tuple(CASES) + ar.TOPOLOGIES + tuple("star%d" % k for k in ar.STAR_SIZES)


def plan(Q, dm, vals=None, **kw):
    return capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val if vals is None else vals, device=-1, **kw)


def built(name):
    """A plan-only handle of a named graph with its table and term map."""
    g, Q, dm, ref = ar.graph(name)
    ctx = plan(Q, dm)
    ctx.set_measurements(*rr.table(g))
    ctx.assembly_build(Q.rowptr, Q.col)
    return ctx, g, Q, dm, ref


def products(ctx, dm):
    rng = np.random.default_rng(5)
    return [ctx.debug_format_spmm_host(rng.standard_normal((dm.N, k))) for k in KS]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", tuple(CASES) + ("plaza2",))
def test_reference_is_pinned_to_the_oracle(name):
    """Unit weights: the sum of the terms is oracle.assemble's Q within the bound (observed ratio at most 0.23)."""
    g, Q, dm, ref = ar.graph(name)
    ratio = ref.check(np.asarray(Q.val, dtype=np.float64), np.ones(ref.n_weights), name)
    print("%s: worst |Q - ref| / bound = %.3f" % (name, ratio))


@pytest.mark.parametrize("name", GRAPHS + ("plaza2",))
def test_host_mirror_within_the_bound(name):
    ctx, g, Q, dm, ref = built(name)
    info = ctx.assembly_info()
    assert info["n_weights"] == ref.n_weights and info["n_terms"] == int(ref.n_terms.sum())
    assert info["max_terms"] == int(ref.n_terms.max()) and info["long_entries"] == int(np.sum(ref.n_terms > ar.K_LONG_ENTRY))
    for seed, w in ((0, np.ones(ref.n_weights)), (1, ar.random_weights(ref.n_weights, 11)), (2, ar.random_weights(ref.n_weights, 12))):
        assert seed == 0 or ref.n_weights < 8 or np.any(w == 0.0)
        got = ctx.debug_assemble_values_host(w)
        ratio = ref.check(got, w, name)
        print("%s weights %d: worst ratio %.3f" % (name, seed, ratio))
        assert np.array_equal(got, ctx.debug_assemble_values_host(w))
        assert not np.any(np.signbit(got) & (got == 0.0))  # zeros are +0.0
    ctx.close()


@pytest.mark.parametrize("K", ar.STAR_SIZES)
def test_star_takes_the_declared_path(K):
    """The landmark's diagonal has exactly K terms: the long path iff K > kLongEntry, so no case silently misses its path."""
    ctx, g, Q, dm, ref = built("star%d" % K)
    info = ctx.assembly_info()
    assert info["max_terms"] == K
    assert info["long_entries"] == (1 if K > ar.K_LONG_ENTRY else 0)
    diag = int(np.argmax(ref.n_terms))
    w = ar.random_weights(ref.n_weights, K)
    got = ctx.debug_assemble_values_host(w)
    refv, mag = ref.evaluate(w)
    assert abs(float(got[diag] - refv[diag])) <= (K + 3) * ar.EPS * mag[diag]
    ctx.close()


def test_star_d3_and_edgeless_and_rangeless():
    for name in ("star129-d3", "single_range", "pp_only", "single_rpm"):
        ctx, g, Q, dm, ref = built(name)
        w = ar.random_weights(ref.n_weights, 3)
        ref.check(ctx.debug_assemble_values_host(w), w, name)
        ctx.close()
    assert len(rr.edges(ar.graph("single_range")[0])) == 0 and len(ar.graph("single_rpm")[0].ranges) == 0


def _with_zero_pair(Q, N, i, j):
    """The CSR with explicit zeros added at (i, j) and (j, i) (neither is in the pattern)."""
    import scipy.sparse as sp
    A = sp.csr_matrix((np.asarray(Q.val, dtype=np.float64), np.asarray(Q.col), np.asarray(Q.rowptr)), shape=(N, N)).tocoo()
    assert A.tocsr()[i, j] == 0 and i != j
    rows, cols = np.append(A.row, [i, j]), np.append(A.col, [j, i])
    vals = np.append(A.data, [0.0, 0.0])
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    rowptr = np.zeros(N + 1, dtype=np.int32)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), cols.astype(np.int32), vals


def test_entry_no_term_reaches_is_plus_zero():
    """The assembled patterns hold no such entry (asserted), so: a CSR with a symmetric pair of explicit zeros between the
    translation rows of two poses no measurement joins."""
    g, Q, dm, ref = ar.graph("lm_lm")
    assert np.all(ref.n_terms > 0)
    t0 = dm.d * dm.n + dm.r
    rowptr, col, vals = _with_zero_pair(Q, dm.N, t0 + 3, t0 + 40)
    ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, rowptr, col, vals, device=-1)
    ctx.set_measurements(*rr.table(g))
    ctx.assembly_build(rowptr, col)
    ref2 = ar.Reference(g, rowptr, col, dm.N)
    untouched = np.nonzero(ref2.n_terms == 0)[0]
    assert len(untouched) == 2
    w = ar.random_weights(ref2.n_weights, 4)
    for got in (ctx.debug_assemble_values_host(w), ctx.assemble_values(w)):
        assert np.all(got[untouched] == 0.0) and not np.any(np.signbit(got[untouched]))
        ref2.check(got, w)
    ctx.close()


@pytest.mark.parametrize("name", ("small_ra_slam_problem", "hub-d3", "priors_wide", "star257", "fat_landmark"))
def test_round_trip_equals_a_fresh_handle(name):
    ctx, g, Q, dm, ref = built(name)
    first = products(ctx, dm)
    w = ar.random_weights(ref.n_weights, 21)
    vals = ctx.assemble_values(w)
    assert np.array_equal(vals, ctx.debug_assemble_values_host(w))
    fresh = plan(Q, dm, vals)
    after = products(ctx, dm)
    assert same(after, products(fresh, dm)) and not same(after, first)
    # the host table follows the weights: the residuals of a table set with kappa w, tau w, omega w, bit for bit
    er, ed, rg, rd = rr.table(g)
    ne, d = len(er), dm.d
    ed2, rd2 = ed.copy(), rd.copy()
    ed2[:, d * d + d] *= w[:ne]
    ed2[:, d * d + d + 1] *= w[ne:2 * ne]
    rd2[:, 1] *= w[2 * ne:]
    fresh.set_measurements(er, ed2, rg, rd2)
    X = np.random.default_rng(2).standard_normal((dm.N, 3))
    a, b = ctx.debug_measurement_residuals_host(X), fresh.debug_measurement_residuals_host(X)
    for key in ("edge_rot", "edge_trans", "range", "sums"):
        assert np.array_equal(a[key], b[key]), key
    # ones again: the first assembly's bits again, and weights multiply the BASE precisions, not the current ones
    ones = ctx.assemble_values(np.ones(ref.n_weights))
    ref.check(ones, np.ones(ref.n_weights))
    assert np.array_equal(ctx.assemble_values(w), vals)
    ctx.close()
    fresh.close()


def test_refusals_leave_the_handle_alone():
    g, Q, dm, ref = ar.graph("rplm_priors")
    ctx = plan(Q, dm)
    with pytest.raises(capi.CoraError) as e:
        ctx.assembly_build(Q.rowptr, Q.col)  # before a table
    assert e.value.code == ERR_NOT_READY
    ctx.set_measurements(*rr.table(g))
    with pytest.raises(capi.CoraError) as e:
        ctx.assemble_values(np.ones(ref.n_weights))  # before a build
    assert e.value.code == ERR_NOT_READY
    with pytest.raises(capi.CoraError) as e:
        ctx.assembly_info()
    assert e.value.code == ERR_NOT_READY
    ctx.assembly_build(Q.rowptr, Q.col)
    w = ar.random_weights(ref.n_weights, 8)
    ctx.assemble_values(w)
    before = products(ctx, dm)
    X = np.random.default_rng(3).standard_normal((dm.N, 2))
    res = ctx.debug_measurement_residuals_host(X)
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        for at in (0, ref.n_weights // 2, ref.n_weights - 1):
            wb = np.ones(ref.n_weights)
            wb[at] = bad
            for call in (ctx.assemble_values, ctx.debug_assemble_values_host):
                with pytest.raises(capi.CoraError) as e:
                    call(wb)
                assert e.value.code == ERR_ARG
    for n in (ref.n_weights - 1, ref.n_weights + 1, 0):
        with pytest.raises(capi.CoraError):
            ctx.assemble_values(np.ones(n))
    assert same(products(ctx, dm), before)
    again = ctx.debug_measurement_residuals_host(X)
    assert all(np.array_equal(res[k], again[k]) for k in res)
    # a new table drops the map
    ctx.set_measurements(*rr.table(g))
    with pytest.raises(capi.CoraError) as e:
        ctx.assemble_values(w)
    assert e.value.code == ERR_NOT_READY
    ctx.close()


def test_term_outside_the_pattern_is_refused():
    """A range's coupling (t_a, t_b) and its mirror dropped from the CSR: the range has a nonzero term there."""
    import scipy.sparse as sp
    g, Q, dm, ref = ar.graph("lm_lm")
    _, _, rg, _ = rr.table(g)
    i, j = int(rg[0][1]), int(rg[0][2])
    A = sp.csr_matrix((np.asarray(Q.val, dtype=np.float64), np.asarray(Q.col), np.asarray(Q.rowptr)), shape=(dm.N, dm.N)).tocoo()
    keep = ~(((A.row == i) & (A.col == j)) | ((A.row == j) & (A.col == i)))
    assert np.count_nonzero(~keep) == 2
    B = sp.csr_matrix((A.data[keep], (A.row[keep], A.col[keep])), shape=(dm.N, dm.N))
    B.sort_indices()
    ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, B.indptr.astype(np.int32), B.indices.astype(np.int32), B.data, device=-1)
    ctx.set_measurements(*rr.table(g))
    with pytest.raises(capi.CoraError) as e:
        ctx.assembly_build(B.indptr.astype(np.int32), B.indices.astype(np.int32))
    assert e.value.code == ERR_ARG and "range 0" in str(e.value), str(e.value)
    ctx.close()


def test_another_pattern_duplicates_and_partitions_are_refused():
    g, Q, dm, ref = ar.graph("n2")
    rowptr, col = np.array(Q.rowptr, dtype=np.int32), np.array(Q.col, dtype=np.int32)
    vals = np.asarray(Q.val, dtype=np.float64)
    at = int(rowptr[1])  # row 0 repeats its last column
    rp = rowptr.copy()
    rp[1:] += 1
    ci, v = np.insert(col, at, col[at - 1]), np.insert(vals, at, 0.25)
    a = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, rp, ci, v, device=-1)
    a.set_measurements(*rr.table(g))
    with pytest.raises(capi.CoraError) as e:
        a.assembly_build(rp, ci)
    assert e.value.code == ERR_ARG
    b = plan(Q, dm)
    b.set_measurements(*rr.table(g))
    moved = col.copy()
    row0 = set(col[rowptr[0]:rowptr[1]].tolist())
    moved[rowptr[1] - 1] = next(c for c in range(dm.N - 1, 0, -1) if c not in row0)
    with pytest.raises(capi.CoraError) as e:
        b.assembly_build(rowptr, moved)
    assert e.value.code == ERR_ARG
    g2, Q2, dm2, _ = ar.graph("hub-d2")
    p = plan(Q2, dm2, rank=0, world=2)
    with pytest.raises(capi.CoraError) as e:
        p.assembly_build(Q2.rowptr, Q2.col)
    assert e.value.code == ERR_ARG
    for c in (a, b, p):
        c.close()


# ---- CORA::Problem without a GPU: reweight on a plan-only handle ---------------------------------------------------------

def _problem(case, live):
    from cora_amd import host
    P = host.Problem.from_pyfg(os.path.join(GOLDEN, case, "factor_graph.pyfg"))
    P.update()
    if live:
        P.set_device(-1)  # a plan-only handle: the term map is executed on the host
        P.context_ptr()
    return P


def _weights(P, seed):
    rng = np.random.default_rng(seed)
    return {kind: rng.uniform(0.25, 2.0, len(ones)) * (rng.uniform(size=len(ones)) > 0.2)
            for kind, ones in P.get_measurement_weights().items() if len(ones)}


@pytest.mark.parametrize("live", [False, True])
def test_problem_reweight(case, live):
    """DataMatrix of reweight(w) within the bound of set_measurement_weights(w)'s, on the same pattern; without a handle
    reweight IS set_measurement_weights."""
    P, S = _problem(case, live), _problem(case, False)
    g = ar.graph(case)[0]
    unit = P.matrix("DataMatrix")
    w = _weights(P, 17)
    P.reweight(w)
    S.set_measurement_weights(w)
    for kind, v in w.items():
        assert np.array_equal(P.get_measurement_weights()[kind], v)
    got, want = P.matrix("DataMatrix"), S.matrix("DataMatrix")
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.array_equal(got[2], unit[2]) and np.array_equal(got[3], unit[3])
    if not live:
        assert np.array_equal(got[4], want[4])
    ref = ar.Reference(g, got[2], got[3], len(got[2]) - 1)
    kinds = P.WEIGHT_KINDS
    full = {k: w.get(k, P.get_measurement_weights()[k]) for k in kinds}
    flat = np.concatenate([full["rel_pose_rot"], full["pose_prior_rot"], np.ones(len(full["pose_landmark"]) + len(full["landmark_prior"])),
                           full["rel_pose_trans"], full["pose_prior_trans"], full["pose_landmark"], full["landmark_prior"],
                           full["range"]])
    ref.check(got[4], flat, "reweight")
    ref.check(want[4], flat, "set_measurement_weights")
    # back to ones: the bits of a first reweight({})
    P.reweight({})
    back = P.matrix("DataMatrix")[4].copy()
    F = _problem(case, live)
    F.reweight({})
    assert np.array_equal(back.view(np.int64), F.matrix("DataMatrix")[4].view(np.int64))
    ref.check(back, np.ones(ref.n_weights), "ones")


def test_problem_reweight_bad_weights_raise():
    from cora_amd import host
    P = _problem("small_ra_slam_problem", True)
    P.reweight(_weights(P, 3))
    before = P.matrix("DataMatrix")[4].copy()
    n = len(P.get_measurement_weights()["range"])
    for bad in ({"range": np.ones(n + 1)}, {"range": -np.ones(n)}, {"range": np.full(n, np.nan)}, {"ranges": np.ones(n)}):
        with pytest.raises(host.HostError):
            P.reweight(bad)
    assert np.array_equal(P.matrix("DataMatrix")[4], before)
