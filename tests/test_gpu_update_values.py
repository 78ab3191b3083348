"""New values of Q on a live handle (cora_update_values, cora_update_values_dev): a handle updated in place against a
handle freshly created from the same values.  The same values land in the same slots and every kernel adds in a fixed
order, so every comparison is bit for bit; the yardstick is always the fresh handle.  What survives an update and what it
invalidates; rejected updates; CORA::Problem::setMeasurementWeights on a golden data set with the Cholesky preconditioner,
in both formulations; one partitioned case."""
import os
import threading

import numpy as np
import pytest

from conftest import GOLDEN
from cora_amd import capi, host
from cora_amd.dist import NativeLocalComm, NativeLocalGroup
from oracle import oracle as orc
from test_update_values_cpu import _mirror_entry, graph

pytestmark = pytest.mark.gpu
ERR_NOT_READY, ERR_ARG = 2, 5
P_RANK = 5
KS = (1, 2, 3, 5, 8, 13, 24)
FORMS = (("window", 0), ("gather", 1 << 30))  # cora_debug_spmm_window_min_slices: LDS windows always / never


@pytest.fixture
def restore_form():
    L = capi.load()
    old = L.cora_debug_spmm_window_min_slices(0)
    L.cora_debug_spmm_window_min_slices(old)
    yield L
    L.cora_debug_spmm_window_min_slices(old)


@pytest.fixture(scope="module", params=[2, 3])
def problem(request):
    """(Q, dm, vals1, vals2, point Y, tangent V, operands by column count): computed once, never written."""
    Q, dm, vals1, vals2 = graph(request.param)
    rng = np.random.default_rng(40 + request.param)
    Y = orc.project_manifold(dm, rng.uniform(-1, 1, (dm.N, P_RANK)))
    V = orc.tangent_proj(dm, Y, rng.uniform(-1, 1, (dm.N, P_RANK)))
    X = {k: rng.standard_normal((dm.N, k)) for k in KS}
    for a in (Y, V, *X.values()):
        a.setflags(write=False)
    return Q, dm, vals1, vals2, Y, V, X


def handle(Q, dm, vals, **kw):
    c = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, vals, **kw)
    c.set_rank(P_RANK)
    return c


def everything(c, Y, V, X):
    """Every product and the point state of a handle, as host arrays (name -> array)."""
    out = {}
    for k, Xk in X.items():
        x, o = c.dev_alloc(k), c.dev_alloc(k)
        c.upload(Xk, x)
        c.spmm_dev(x, k, o)
        out["spmm%d" % k] = c.download(o, k)
        c.dev_free(x)
        c.dev_free(o)
    y, v, o = c.dev_alloc(P_RANK), c.dev_alloc(P_RANK), c.dev_alloc(P_RANK)
    c.upload(Y, y)
    c.set_point_dev(y)
    out["f"] = np.array([c.point_cost()])
    _, g, rg = c.point_ptrs()
    out["egrad"], out["rgrad"] = c.download(g, P_RANK), c.download(rg, P_RANK)
    c.upload(V, v)
    c.hvp_dev(v, o)
    out["hvp"] = c.download(o, P_RANK)
    for k in (3, 8):
        x, s = c.dev_alloc(k), c.dev_alloc(k)
        c.upload(X[k], x)
        c.certificate_product_dev(x, k, s)
        out["cert%d" % k] = c.download(s, k)
        c.dev_free(x)
        c.dev_free(s)
    c.precond_setup(capi.PRECOND_JACOBI)
    out["jacobi"] = c.precondition(V)
    for p in (y, v, o):
        c.dev_free(p)
    return out


def assert_same(got, ref, what=""):
    assert got.keys() == ref.keys()
    for name in ref:
        assert np.array_equal(got[name], ref[name]), (what, name)


def device_copy(vals):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(vals)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def test_update_matches_fresh_handle(problem, restore_form):
    Q, dm, vals1, vals2, Y, V, X = problem
    for form, win in FORMS:
        restore_form.cora_debug_spmm_window_min_slices(win)
        b = handle(Q, dm, vals2)
        fresh = everything(b, Y, V, X)
        b.close()
        b = handle(Q, dm, vals1)
        first = everything(b, Y, V, X)
        b.close()
        assert not np.array_equal(first["hvp"], fresh["hvp"])
        a = handle(Q, dm, vals1)
        everything(a, Y, V, X)  # a point, Lambda and a preconditioner of the old values are in place
        a.update_values(Q.rowptr, Q.col, vals2)
        assert_same(everything(a, Y, V, X), fresh, form + ": host values")
        a.update_values(Q.rowptr, Q.col, vals1)
        assert_same(everything(a, Y, V, X), first, form + ": back")
        t = device_copy(vals2)
        a.update_values_dev(t.data_ptr())
        assert_same(everything(a, Y, V, X), fresh, form + ": device values")
        with pytest.raises(capi.CoraError) as e:  # the host copy of the format is stale now: refused, not old numbers
            a.debug_format_spmm_host(X[3])
        assert e.value.code == ERR_NOT_READY
        a.update_values(Q.rowptr, Q.col, vals2)
        plan = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, vals2, device=-1)
        assert np.array_equal(a.debug_format_spmm_host(X[3]), plan.debug_format_spmm_host(X[3]))
        a.close()


def test_device_update_needs_the_map(problem):
    Q, dm, vals1, vals2, Y, V, X = problem
    a = handle(Q, dm, vals1)
    t = device_copy(vals2)
    with pytest.raises(capi.CoraError) as e:
        a.update_values_dev(t.data_ptr())
    assert e.value.code == ERR_NOT_READY
    a.values_map_build(Q.rowptr, Q.col)
    a.update_values_dev(t.data_ptr())
    b = handle(Q, dm, vals2)
    x, o = a.dev_alloc(8), a.dev_alloc(8)
    a.upload(X[8], x)
    a.spmm_dev(x, 8, o)
    xb, ob = b.dev_alloc(8), b.dev_alloc(8)
    b.upload(X[8], xb)
    b.spmm_dev(xb, 8, ob)
    assert np.array_equal(a.download(o, 8), b.download(ob, 8))
    a.close()
    b.close()


def test_survival_invalidation_and_rejection(problem):
    Q, dm, vals1, vals2, Y, V, X = problem
    a = handle(Q, dm, vals1)
    y, v, o, keep = (a.dev_alloc(P_RANK) for _ in range(4))
    a.upload(Y, y)
    a.upload(V, v)
    a.upload(X[5], keep)
    kept = a.download(keep, P_RANK)
    a.set_point_dev(y)
    a.hvp_dev(v, o)
    hvp1 = a.download(o, P_RANK)
    x8, o8 = a.dev_alloc(8), a.dev_alloc(8)
    a.upload(X[8], x8)
    a.spmm_dev(x8, 8, o8)
    spmm1 = a.download(o8, 8)

    broken = vals2.copy()  # one of a mirror pair moved by an ulp: refused by the check kernel, nothing written
    q = _mirror_entry(Q, dm)
    broken[q] = np.nextafter(broken[q], np.inf)
    nan = vals2.copy()
    nan[7] = np.nan
    a.values_map_build(Q.rowptr, Q.col)
    for bad in (broken, nan):
        for call in (lambda: a.update_values(Q.rowptr, Q.col, bad), lambda: a.update_values_dev(device_copy(bad).data_ptr())):
            with pytest.raises(capi.CoraError) as e:
                call()
            assert e.value.code == ERR_ARG
            a.hvp_dev(v, o)  # the point is still there, and so are the values
            assert np.array_equal(a.download(o, P_RANK), hvp1)
            a.spmm_dev(x8, 8, o8)
            assert np.array_equal(a.download(o8, 8), spmm1)

    a.update_values(Q.rowptr, Q.col, vals2)
    assert np.array_equal(a.download(keep, P_RANK), kept)  # a caller's vector survives with its contents
    assert np.array_equal(a.download(y, P_RANK), Y)
    with pytest.raises(capi.CoraError) as e:  # no current point until the next set_point
        a.hvp_dev(v, o)
    assert e.value.code == ERR_NOT_READY
    a.set_point_dev(y)
    a.hvp_dev(v, o)
    assert not np.array_equal(a.download(o, P_RANK), hvp1)
    a.close()


def _golden_problem(implicit, weights=None):
    P = host.Problem.from_pyfg(os.path.join(GOLDEN, "small_ra_slam_problem", "factor_graph.pyfg"))
    P.set_formulation(implicit)
    P.update()
    P.set_rank(P.dims()["d"] + 2)  # (above d: at rank d the completion of an implicit point insists on det R = +1)
    if weights is not None:
        P.set_measurement_weights(weights)
    return P


@pytest.mark.parametrize("implicit", [False, True])
def test_problem_weights_keep_the_handle(implicit):
    """Cholesky preconditioner (the default of a parsed problem): weights set on a problem that has already solved give
    what a new problem with the same weights gives, on the SAME handle."""
    P1 = _golden_problem(implicit)
    rank = P1.dims()["rank"]
    rng = np.random.default_rng(3)
    x0 = P1.op("projectToManifold", rng.standard_normal((P1.variable_size(), rank)))
    first = P1.tnt(x0, max_iterations=20)
    P1.measurement_residuals(first["x"])  # (a table of the unit weights is installed)
    ptr = P1.context_ptr()
    weights = {}
    for kind, ones in P1.get_measurement_weights().items():
        if len(ones):
            weights[kind] = rng.uniform(0.25, 2.0, len(ones)) * (rng.uniform(size=len(ones)) > 0.15)
    P1.set_measurement_weights(weights)
    assert P1.context_ptr() == ptr
    P2 = _golden_problem(implicit, weights)
    r1, r2 = P1.tnt(x0, max_iterations=20), P2.tnt(x0, max_iterations=20)
    assert P1.context_ptr() == ptr
    assert r1["f"] != first["f"]
    assert np.array_equal(r1["x"], r2["x"]) and r1["f"] == r2["f"]
    assert (r1["iterations"], r1["hvps"]) == (r2["iterations"], r2["hvps"])
    m1, m2 = P1.measurement_residuals(r1["x"]), P2.measurement_residuals(r2["x"])
    for name in m2:
        assert np.array_equal(m1[name], m2[name]), name
    half = 0.5 * (m1["rot_sum"] + m1["trans_sum"] + m1["range_sum"])
    print("f = %.15g, half the weighted residuals = %.15g" % (r1["f"], half))
    assert abs(half - r1["f"]) <= 1e-8 * abs(r1["f"])


def test_partitioned_handles(problem):
    """Four ranks as threads on one GPU: every rank updates its own handle (the call is not collective); products that
    exchange rows afterwards equal those of freshly created partitioned handles."""
    Q, dm, vals1, vals2, Y, V, X = problem
    world = 4
    groups = (NativeLocalGroup(world), NativeLocalGroup(world))
    out, err = [None] * world, [None] * world

    def products(c):
        y, v, o, x7, o7 = c.dev_alloc(P_RANK), c.dev_alloc(P_RANK), c.dev_alloc(P_RANK), c.dev_alloc(8), c.dev_alloc(8)
        c.upload(Y, y)
        c.set_point_dev(y)
        c.upload(V, v)
        c.hvp_dev(v, o)
        c.upload(X[8], x7)
        c.spmm_dev(x7, 8, o7)
        return c.download(o, P_RANK), c.download(o7, 8)

    def body(r):
        a = handle(Q, dm, vals1, rank=r, world=world)
        comm_a = NativeLocalComm(a, groups[0])
        before = products(a)
        a.update_values(Q.rowptr, Q.col, vals2)
        got = products(a)
        b = handle(Q, dm, vals2, rank=r, world=world)
        comm_b = NativeLocalComm(b, groups[1])
        ref = products(b)
        del comm_a, comm_b
        return before, got, ref

    def run(r):
        try:
            out[r] = body(r)
        except BaseException as e:  # noqa: BLE001
            err[r] = e
            for g in groups:
                g.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    for e in err:
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise e
    for e in err:
        if e is not None:
            raise e
    for before, got, ref in out:
        assert not np.array_equal(before[0], ref[0])
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
