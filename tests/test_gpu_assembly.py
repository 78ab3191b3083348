"""Q(w) assembled on the device from per-measurement weights (k_assemble_short / k_assemble_long behind
cora_assemble_values*): the device against the host mirror of the same term map and a handle assembled in place against a
handle freshly created from the assembled values -- every comparison bit for bit, since every sum has a fixed order.  What
an assembly keeps and what it invalidates, refused weights, determinism, and CORA::Problem::reweight against
setMeasurementWeights."""
import os

import numpy as np
import pytest

import assembly_ref as ar
import residuals_ref as rr
from conftest import GOLDEN
from cora_amd import capi, host
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
ERR_NOT_READY, ERR_ARG = 2, 5
P_RANK = 5
KS = (1, 5, 24)
FORMS = (("window", 0), ("gather", 1 << 30))  # cora_debug_spmm_window_min_slices: LDS windows always / never
STARS = tuple("star%d" % k for k in ar.STAR_SIZES)
GRAPHS = ("small_ra_slam_problem", "single_rpm", "single_range") + ar.TOPOLOGIES + STARS + ("star129-d3", "plaza2")


@pytest.fixture
def restore_form():
    L = capi.load()
    old = L.cora_debug_spmm_window_min_slices(0)
    L.cora_debug_spmm_window_min_slices(old)
    yield L
    L.cora_debug_spmm_window_min_slices(old)


def handle(name, vals=None, table=None, build=True):
    g, Q, dm, ref = ar.graph(name)
    c = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val if vals is None else vals)
    c.set_rank(P_RANK)
    c.set_measurements(*(table or rr.table(g)))
    if build:
        c.assembly_build(Q.rowptr, Q.col)
    return c


def on_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def positive(w):
    """The same weights with the zeros replaced: no zero on the diagonal of Q(w) (the Jacobi preconditioner needs one)."""
    return np.where(w == 0.0, 0.375, w)


def scaled_table(g, d, w):
    er, ed, rg, rd = rr.table(g)
    ne = len(er)
    ed, rd = ed.copy(), rd.copy()
    ed[:, d * d + d] *= w[:ne]
    ed[:, d * d + d + 1] *= w[ne:2 * ne]
    rd[:, 1] *= w[2 * ne:]
    return er, ed, rg, rd


def operands(dm, seed=40):
    rng = np.random.default_rng(seed)
    Y = orc.project_manifold(dm, rng.uniform(-1, 1, (dm.N, P_RANK)))
    V = orc.tangent_proj(dm, Y, rng.uniform(-1, 1, (dm.N, P_RANK)))
    X = {k: rng.standard_normal((dm.N, k)) for k in KS + (3,)}
    return Y, V, X


def everything(c, Y, V, X):
    """Every product and the point state of a handle, as host arrays (the idea of tests/test_gpu_update_values.py)."""
    out = {}
    for k in KS:
        x, o = c.dev_alloc(k), c.dev_alloc(k)
        c.upload(X[k], x)
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
    x, s = c.dev_alloc(3), c.dev_alloc(3)
    c.upload(X[3], x)
    c.certificate_product_dev(x, 3, s)
    out["cert3"] = c.download(s, 3)
    c.precond_setup(capi.PRECOND_JACOBI)
    out["jacobi"] = c.precondition(V)
    for p in (y, v, o, x, s):
        c.dev_free(p)
    return out


def assert_same(got, ref, what=""):
    assert got.keys() == ref.keys()
    for name in ref:
        assert np.array_equal(got[name], ref[name]), (what, name)


@pytest.mark.parametrize("name", GRAPHS)
def test_device_equals_the_host_mirror(name):
    """Both forms, weights with zeros: the bits of cora_debug_assemble_values_host, which are within the derived bound of
    the longdouble reference.  star* cover both sides of kLongEntry, fat_landmark an entry of 8190 terms, single_range
    nnz = 9 (odd: the last entry is stored alone)."""
    import torch
    g, Q, dm, ref = ar.graph(name)
    c = handle(name)
    info = c.assembly_info()
    if name in STARS:
        K = int(name[4:])
        assert info["max_terms"] == K and info["long_entries"] == (1 if K > ar.K_LONG_ENTRY else 0)
    if name == "single_range":
        assert ref.nnz == 9
    for seed in (31, 32):
        w = ar.random_weights(ref.n_weights, seed)
        mirror = c.debug_assemble_values_host(w)
        ref.check(mirror, w, name)
        got = c.assemble_values(w)
        assert np.array_equal(got.view(np.int64), mirror.view(np.int64)), (name, "host-pointer form")
        out = torch.full((ref.nnz + 1,), -7.0, dtype=torch.float64, device="cuda:0")
        c.assemble_values_dev(on_device(np.ones(ref.n_weights)).data_ptr())  # (other values in between, no output asked)
        c.assemble_values_dev(on_device(w).data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        back = out.cpu().numpy()
        assert back[-1] == -7.0  # nothing written past nnz
        assert np.array_equal(back[:-1].view(np.int64), mirror.view(np.int64)), (name, "device form")
    c.close()


def test_some_graph_has_odd_and_even_nnz():
    nnz = [ar.graph(n)[3].nnz for n in GRAPHS]
    assert any(n % 2 for n in nnz) and any(n % 2 == 0 for n in nnz)


@pytest.mark.parametrize("name", ("hub-d2", "priors_wide", "fat_landmark", "star257"))
def test_assembled_handle_equals_a_fresh_handle(name, restore_form):
    g, Q, dm, ref = ar.graph(name)
    Y, V, X = operands(dm)
    w = positive(ar.random_weights(ref.n_weights, 33))
    for form, win in FORMS:
        restore_form.cora_debug_spmm_window_min_slices(win)
        a = handle(name)
        first = everything(a, Y, V, X)  # a point, Lambda and a preconditioner of the old values are in place
        vals = a.assemble_values(w)
        fresh_h = handle(name, vals=vals, build=False)
        fresh = everything(fresh_h, Y, V, X)
        fresh_h.close()
        assert not np.array_equal(first["hvp"], fresh["hvp"])
        assert_same(everything(a, Y, V, X), fresh, form + ": host weights")
        a.assemble_values(np.ones(ref.n_weights))
        a.assemble_values_dev(on_device(w).data_ptr())
        assert_same(everything(a, Y, V, X), fresh, form + ": device weights")
        a.close()


@pytest.mark.parametrize("name", ("small_ra_slam_problem", "rplm_priors", "star197", "single_range", "single_rpm"))
def test_residuals_follow_the_weights(name):
    g, Q, dm, ref = ar.graph(name)
    w = ar.random_weights(ref.n_weights, 34)
    X = np.random.default_rng(6).standard_normal((dm.N, 4))
    a = handle(name)
    b = handle(name, table=scaled_table(g, dm.d, w), build=False)
    want = b.measurement_residuals(X)
    unit = a.measurement_residuals(X)
    for form in ("host", "device"):
        if form == "host":
            a.assemble_values(w)
        else:
            a.assemble_values(np.ones(ref.n_weights))
            assert all(np.array_equal(a.measurement_residuals(X)[k], unit[k]) for k in unit)
            a.assemble_values_dev(on_device(w).data_ptr())
        got = a.measurement_residuals(X)
        for key in ("edge_rot", "edge_trans", "range", "sums"):
            assert np.array_equal(got[key], want[key]), (form, key)
    with pytest.raises(capi.CoraError) as e:  # the host table is stale after the device form
        a.debug_measurement_residuals_host(X)
    assert e.value.code == ERR_NOT_READY
    a.assemble_values(w)
    host_side = a.debug_measurement_residuals_host(X)
    hb = b.debug_measurement_residuals_host(X)
    assert all(np.array_equal(host_side[k], hb[k]) for k in hb)
    a.close()
    b.close()


def _diagonal_factor(Q, dm, vals):
    """A Cholesky factor of the right size (diagonal: the solve it gives is not the point of the test)."""
    N = dm.N
    return np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32), np.ones(N), np.arange(N, dtype=np.int32)


def test_state_contract():
    name = "hub-d3"
    g, Q, dm, ref = ar.graph(name)
    Y, V, X = operands(dm)
    a = handle(name)
    y, v, o, keep = (a.dev_alloc(P_RANK) for _ in range(4))
    a.upload(Y, y)
    a.upload(V, v)
    a.upload(X[5], keep)
    kept = a.download(keep, P_RANK)
    a.set_point_dev(y)
    a.hvp_dev(v, o)
    hvp1 = a.download(o, P_RANK)
    a.precond_set_cholesky(*_diagonal_factor(Q, dm, None))
    a.precond_setup(capi.PRECOND_REGULARIZED_CHOLESKY)
    w = positive(ar.random_weights(ref.n_weights, 35))
    for form in ("host", "device"):
        if form == "host":
            a.assemble_values(w)
        else:
            a.assemble_values_dev(on_device(w).data_ptr())
        assert np.array_equal(a.download(keep, P_RANK), kept)  # a caller's vectors survive with their contents
        assert np.array_equal(a.download(y, P_RANK), Y)
        with pytest.raises(capi.CoraError) as e:  # no current point until the next set_point
            a.hvp_dev(v, o)
        assert e.value.code == ERR_NOT_READY
        with pytest.raises(capi.CoraError) as e:  # the factor belonged to the old values
            a.precond_setup(capi.PRECOND_REGULARIZED_CHOLESKY)
        assert e.value.code == ERR_NOT_READY
        if form == "device":
            with pytest.raises(capi.CoraError) as e:  # the host copy of the format is stale: refused, not old numbers
                a.debug_format_spmm_host(X[3])
            assert e.value.code == ERR_NOT_READY
        else:
            plan = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, a.debug_assemble_values_host(w), device=-1)
            assert np.array_equal(a.debug_format_spmm_host(X[3]), plan.debug_format_spmm_host(X[3]))
            plan.close()
        a.set_point_dev(y)
        a.hvp_dev(v, o)
        assert not np.array_equal(a.download(o, P_RANK), hvp1)
        a.precond_set_cholesky(*_diagonal_factor(Q, dm, None))
        a.precond_setup(capi.PRECOND_REGULARIZED_CHOLESKY)
    a.close()


def test_refused_weights_change_nothing():
    name = "dups"
    g, Q, dm, ref = ar.graph(name)
    Y, V, X = operands(dm)
    a = handle(name, build=False)
    with pytest.raises(capi.CoraError) as e:
        a.assemble_values_dev(on_device(np.ones(ref.n_weights)).data_ptr())  # before a build
    assert e.value.code == ERR_NOT_READY
    a.assembly_build(Q.rowptr, Q.col)
    a.assemble_values(positive(ar.random_weights(ref.n_weights, 36)))
    y, v, o, x8, o8 = a.dev_alloc(P_RANK), a.dev_alloc(P_RANK), a.dev_alloc(P_RANK), a.dev_alloc(5), a.dev_alloc(5)
    a.upload(Y, y)
    a.upload(V, v)
    a.upload(X[5], x8)
    a.set_point_dev(y)
    a.hvp_dev(v, o)
    hvp1 = a.download(o, P_RANK)
    a.spmm_dev(x8, 5, o8)
    spmm1 = a.download(o8, 5)
    Xr = np.random.default_rng(9).standard_normal((dm.N, 3))
    res1 = a.measurement_residuals(Xr)
    for bad in (np.nan, -0.5, np.inf):
        for at in (0, ref.n_weights - 1):
            wb = np.ones(ref.n_weights)
            wb[at] = bad
            for call in (lambda: a.assemble_values(wb), lambda: a.assemble_values_dev(on_device(wb).data_ptr())):
                with pytest.raises(capi.CoraError) as e:
                    call()
                assert e.value.code == ERR_ARG
                a.hvp_dev(v, o)  # the point is still there, and so are the values and the table
                assert np.array_equal(a.download(o, P_RANK), hvp1)
                a.spmm_dev(x8, 5, o8)
                assert np.array_equal(a.download(o8, 5), spmm1)
                again = a.measurement_residuals(Xr)
                assert all(np.array_equal(res1[k], again[k]) for k in res1)
    a.close()


@pytest.mark.parametrize("name", ("fat_landmark", "star129"))
def test_determinism(name):
    import torch
    g, Q, dm, ref = ar.graph(name)
    a = handle(name)
    w = ar.random_weights(ref.n_weights, 37)
    dw, ones = on_device(w), on_device(np.ones(ref.n_weights))
    outs = [torch.zeros(ref.nnz, dtype=torch.float64, device="cuda:0") for _ in range(3)]
    a.assemble_values_dev(dw.data_ptr(), outs[0].data_ptr())
    a.assemble_values_dev(dw.data_ptr(), outs[1].data_ptr())
    a.assemble_values_dev(ones.data_ptr())
    a.assemble_values_dev(dw.data_ptr(), outs[2].data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    b = handle(name)  # another handle, another map build: the same bits
    assert np.array_equal(b.assemble_values(w), outs[0].cpu().numpy())
    a.close()
    b.close()


# ---- CORA::Problem::reweight ---------------------------------------------------------------------------------------------

def _problem(path, implicit):
    P = host.Problem.from_pyfg(path)
    P.set_formulation(implicit)
    P.update()
    P.set_rank(P.dims()["d"] + 2)
    return P


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("data", ["small_ra_slam_problem", "plaza2"])
def test_problem_reweight(data, implicit):
    """Cholesky preconditioner (the default of a parsed problem).  reweight on a live handle against setMeasurementWeights
    on another problem: the cost at a fixed Y to 1e-9 relative, the same certification decision after a solve from the same
    start, and a host DataMatrix that holds the device's bits."""
    path = os.path.join(GOLDEN, "datasets", "plaza2.pyfg") if data == "plaza2" else os.path.join(GOLDEN, data, "factor_graph.pyfg")
    P1, P2 = _problem(path, implicit), _problem(path, implicit)
    rank = P1.dims()["rank"]
    rng = np.random.default_rng(3)
    x0 = P1.op("projectToManifold", rng.standard_normal((P1.variable_size(), rank)))
    f_unit = P1.op("evaluateObjective", x0)  # (the handle is live)
    ptr = P1.context_ptr()
    weights = {kind: rng.uniform(0.5, 2.0, len(ones)) for kind, ones in P1.get_measurement_weights().items() if len(ones)}
    P1.reweight(weights)
    P2.set_measurement_weights(weights)
    assert P1.context_ptr() == ptr
    f1, f2 = P1.op("evaluateObjective", x0), P2.op("evaluateObjective", x0)
    print("%s: f(reweight) = %.15g, f(setMeasurementWeights) = %.15g, unit %.15g" % (data, f1, f2, f_unit))
    assert f1 != f_unit and abs(f1 - f2) <= 1e-9 * abs(f2)
    # the host matrix holds what the device assembled: the same weights assembled again, straight into a device buffer
    import torch
    C, L = capi.C, capi.load()
    m1, m2 = P1.matrix("DataMatrix"), P2.matrix("DataMatrix")
    assert np.array_equal(m1[2], m2[2]) and np.array_equal(m1[3], m2[3])
    full = {k: weights.get(k, v) for k, v in P1.get_measurement_weights().items()}
    flat = np.concatenate([full["rel_pose_rot"], full["pose_prior_rot"],   # table order: rot | trans of every edge, ranges
                           np.ones(len(full["pose_landmark"]) + len(full["landmark_prior"])), full["rel_pose_trans"],
                           full["pose_prior_trans"], full["pose_landmark"], full["landmark_prior"], full["range"]])
    info = (C.c_int64 * 4)()
    assert L.cora_assembly_info(C.c_void_p(ptr), info) == 0 and info[0] == len(flat)
    out = torch.zeros(len(m1[4]), dtype=torch.float64, device="cuda:0")
    assert L.cora_assemble_values_dev(C.c_void_p(ptr), C.c_void_p(on_device(flat).data_ptr()), C.c_void_p(out.data_ptr())) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int64), m1[4].view(np.int64))
    P1.reweight(weights)  # (the raw call reset the handle behind the Problem's back: the Problem's own call resets both)
    assert np.array_equal(P1.matrix("DataMatrix")[4].view(np.int64), m1[4].view(np.int64))
    r1 = P1.solve(x0, max_rank=rank + 3)
    r2 = P2.solve(x0, max_rank=rank + 3)
    print("%s: certified %s / %s, f %.12g / %.12g" % (data, r1["certified"], r2["certified"], r1["f"], r2["f"]))
    assert r1["certified"] == r2["certified"] and r1["relaxation_certified"] == r2["relaxation_certified"]
