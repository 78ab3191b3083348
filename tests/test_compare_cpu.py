"""The trajectory comparison without a GPU: cora_debug_compare_host (the operations of cora_compare_dev on the host) on
plan-only handles against the longdouble reference of tests/compare_ref.py within that file's rounding bounds, the
ground-truth parser (parsePyfgGroundTruth) on the fixtures and the data sets, and every refusal."""
import ctypes as C
import os

import numpy as np
import pytest

import compare_ref as cr
from conftest import GOLDEN
from cora_amd import capi, host
from mmio import read_dense
from oracle import assemble as asm
from oracle import oracle as orc
from synth import ground_truth, make_graph

ERR_SHAPE, ERR_NAN, ERR_HIP, ERR_ARG = 1, 3, 4, 5
FIXTURES = ("small_ra_slam_problem", "single_range", "single_rpm")
DATASETS = ("mrclam3b", "mrclam5a", "mrclam6", "plaza1", "plaza2", "single_drone", "tiers")

_BUILT = {}


def built(d, n, landmarks=3):
    """(ctx, dims tuple, ground truth) of a synthetic graph on a plan-only handle, once per process."""
    key = (d, n, landmarks)
    if key not in _BUILT:
        g = make_graph(d=d, n=n, n_landmarks=landmarks, n_ranges=min(20, n * landmarks), n_loops=0)
        A = asm.assemble(g)
        Q = orc.CSR.from_scipy(A["Q"])
        dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
        ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1)
        _BUILT[key] = (ctx, (dm.d, dm.n, dm.r, dm.n_trans), ground_truth(g))
    return _BUILT[key]


def ranks(d):
    return ((d, d), (d + 1, d), (5, 5), (24, d), (24, 24))


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", [30, 64, 65, 300])
def test_host_form_against_the_reference(d, n):
    ctx, dims, truth = built(d, n)
    rng = np.random.default_rng(100 * d + n)
    for k, kr in ranks(d):
        Ref = cr.reference_of_rank(truth, *dims, kr, rng)
        X, B, c = cr.gauge_copy(Ref, *dims, k, rng)
        what = "d=%d n=%d k=%d kr=%d" % (d, n, k, kr)
        res = ctx.debug_compare_host(X, Ref)
        _, _, xc, gc, _ = cr.centred(X, Ref, *dims)
        cr.check_gauge(res, B, c, Ref, *dims, xc, gc, what=what + " gauge")
        Xn = X + 1e-2 * rng.standard_normal(X.shape)
        res = ctx.debug_compare_host(Xn, Ref, aligned=True)
        assert res["sigma"][-1] / res["sigma"][0] >= 1e-4
        cr.check_noisy(res, ctx.debug_compare_H(k, kr), Xn, Ref, *dims, what=what + " noisy")
        cr.check_aligned(res["aligned"], res, Xn, Ref, *dims, Xn.shape[0], what=what)
        # the alignment itself against the reference's, at the bound the header states for either form
        _, _, xc, gc, H = cr.centred(Xn, Ref, *dims)
        assert np.linalg.norm(res["A"] - cr.kabsch(H, False)[0]) <= cr.alignment_bound(xc, gc, k) + 64 * k * cr.EPS, what


@pytest.mark.parametrize("d", [2, 3])
def test_selection_reflection_and_degenerate_cases(d):
    ctx, dims, truth = built(d, 65)
    _, n, r, nt = dims
    rng = np.random.default_rng(7 + d)
    # a mask that selects nothing in the first 64 poses and one landmark
    sel = np.zeros(nt, dtype=np.uint8)
    sel[64:n] = 1
    sel[n + 1] = 1
    X, B, c = cr.gauge_copy(truth, *dims, d + 1, rng)
    one = ctx.debug_compare_host(X, truth, select=sel)
    cr.check_degenerate(one, d + 1, "one selected pose")
    assert one["m"] == 1 and one["n_landmarks"] == 1 and np.all(one["sigma"] == 0.0)
    sel[::3] = 1
    Xn = X + 1e-2 * rng.standard_normal(X.shape)
    res = ctx.debug_compare_host(Xn, truth, select=sel)
    cr.check_noisy(res, ctx.debug_compare_H(d + 1, d), Xn, truth, *dims, select=sel, what="d=%d selection" % d)
    Xo = Xn.copy()
    off = np.flatnonzero(sel == 0)
    Xo[cr.rows(*dims)[2][off]] = 1e6
    Xo[cr.rows(*dims)[0][off[off < n]].ravel()] = 1e6
    again = ctx.debug_compare_host(Xo, truth, select=sel)
    assert all(np.array_equal(res[key], again[key]) for key in ("raw", "pose_trans_err", "pose_rot_err", "landmark_err"))
    # a mirrored copy: matched by a reflection unless a proper rotation is asked for
    M, Bm, cm = cr.gauge_copy(truth, *dims, d, rng, mirror=True)
    free = ctx.debug_compare_host(M, truth)
    assert np.linalg.det(free["A"]) < 0
    _, _, xc, gc, H = cr.centred(M, truth, *dims)
    cr.check_gauge(free, Bm, cm, truth, *dims, xc, gc, what="d=%d mirrored" % d)
    prop = ctx.debug_compare_host(M, truth, proper=True)
    assert abs(np.linalg.det(prop["A"]) - 1.0) <= 64 * d * cr.EPS
    opt = cr.optimum(xc, gc, H, True)[0]
    assert opt > 1.0 and abs(prop["sum_et2"] - opt) <= 1e-12 * opt
    # n = 1 and a straight line in 3-D: finite, A^T A = I, nothing else
    ctx1, dims1, truth1 = built(d, 1)
    for k in (d, 5):
        X1 = cr.gauge_copy(truth1, *dims1, k, rng)[0]
        cr.check_degenerate(ctx1.debug_compare_host(X1, truth1, proper=(k == d)), k, "n = 1")
    if d == 3:
        line = truth.copy()
        trn = cr.rows(*dims)[2]
        line[trn] = np.outer(np.arange(nt, dtype=float), [1.0, 2.0, -0.5])
        for k in (3, 4):
            Xl = cr.gauge_copy(line, *dims, k, rng)[0]
            cr.check_degenerate(ctx.debug_compare_host(Xl, line, proper=(k == 3)), k, "straight line")


@pytest.mark.parametrize("case", FIXTURES)
def test_ground_truth_of_the_fixtures(case):
    path = os.path.join(GOLDEN, case, "factor_graph.pyfg")
    P = host.Problem.from_pyfg(path)
    P.update()
    X = P.ground_truth(path)
    want = read_dense(os.path.join(GOLDEN, case, "X_gt.mm"))
    assert X.shape == want.shape
    print("%s: max |X - X_gt| = %.3e" % (case, np.abs(X - want).max()))
    assert np.abs(X - want).max() <= 1e-6  # the files print 7 to 9 decimals
    if case == "small_ra_slam_problem":
        # VERTEX_SE2 .. A5 4 1 1.5707963: R^T of a quarter turn in rows 11-12, (2.68e-8, 1) and (-1, 2.68e-8)
        assert np.abs(X[10:12] - [[0.0, 1.0], [-1.0, 0.0]]).max() <= 1e-6 and 0 < X[10, 0] < 1e-7
        dm = P.dims()
        assert abs(X[dm["d"] * dm["n"], 0] + 0.4657) <= 1e-4  # the first range row: (x_A1 - x_L0) / |.|


@pytest.mark.parametrize("name", DATASETS)
def test_ground_truth_of_the_data_sets_is_a_valid_point(name):
    path = os.path.join(GOLDEN, "datasets", name + ".pyfg")
    P = host.Problem.from_pyfg(path)
    P.update()
    X = P.ground_truth(path)
    dm = P.dims()
    d, n, r = dm["d"], dm["n"], dm["r"]
    assert X.shape == (dm["N"], d) and np.all(np.isfinite(X))
    P.op("alignEstimateToOrigin", X)  # runs Problem::checkVariablesAreValid on its argument (throws otherwise)
    R = X[:d * n].reshape(n, d, d)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(d)).max() <= 1e-12 and np.abs(np.linalg.det(R) - 1).max() <= 1e-12
    assert np.abs(np.linalg.norm(X[d * n:d * n + r], axis=1) - 1).max(initial=0.0) <= 1e-12


def test_ground_truth_needs_every_vertex(tmp_path):
    path = os.path.join(GOLDEN, "small_ra_slam_problem", "factor_graph.pyfg")
    P = host.Problem.from_pyfg(path)
    P.update()
    short = tmp_path / "short.pyfg"
    short.write_text("".join(line for line in open(path) if " A3 " not in line or not line.startswith("VERTEX")))
    with pytest.raises(host.HostError, match="no VERTEX record"):
        P.ground_truth(str(short))


def _raw(ctx, X, Ref, flags=0, x=True, ref=True, out=True, select=None, aligned=None, fn="cora_debug_compare_host"):
    X, Ref = np.asfortranarray(X), np.asfortranarray(Ref)
    dp = C.POINTER(C.c_double)
    o = np.zeros(8 + 2 * Ref.shape[1] + X.shape[1] + X.shape[1] * Ref.shape[1] + 1)
    return getattr(ctx.L, fn)(ctx.h, X.ctypes.data_as(dp) if x else None, X.shape[0], X.shape[1],
                              Ref.ctypes.data_as(dp) if ref else None, Ref.shape[0], Ref.shape[1],
                              select.ctypes.data_as(C.c_void_p) if select is not None else None, int(flags), None, None, None,
                              aligned.ctypes.data_as(dp) if aligned is not None else None, X.shape[0], o.ctypes.data_as(dp) if out else None)


def test_refusals():
    ctx, dims, truth = built(2, 30)
    d, n, r, nt = dims
    N = truth.shape[0]
    X = np.random.default_rng(3).standard_normal((N, 3))
    good = ctx.debug_compare_host(X, truth)
    assert _raw(ctx, np.zeros((N, 25)), truth) == ERR_SHAPE
    assert _raw(ctx, np.zeros((N, 0)), truth) == ERR_SHAPE
    assert _raw(ctx, X, np.zeros((N, 0))) == ERR_SHAPE
    assert _raw(ctx, X[:, :2], np.zeros((N, 3))) == ERR_SHAPE  # kr > k
    for missing in ("x", "ref", "out"):
        assert _raw(ctx, X, truth, **{missing: False}) == ERR_ARG
    assert _raw(ctx, X, truth, flags=2) == ERR_ARG  # unknown flag
    assert _raw(ctx, X, truth, flags=1) == ERR_ARG  # PROPER with k != kr
    assert _raw(ctx, X[:, :2], truth, flags=1) == 0
    nobody = np.zeros(nt, dtype=np.uint8)
    nobody[n:] = 1  # landmarks only: m = 0
    assert _raw(ctx, X, truth, select=nobody) == ERR_ARG
    Xf = np.asfortranarray(X)
    assert _raw(ctx, Xf, truth, aligned=Xf) == ERR_ARG  # aliased
    for bad in (float("inf"), float("nan")):
        Xb = X.copy()
        Xb[N - nt, 0] = bad  # the first pose's position
        assert _raw(ctx, Xb, truth) == ERR_NAN
    with pytest.raises(capi.CoraError) as e:
        ctx.compare(X, truth)  # plan-only: no device, no fall-back
    assert e.value.code == ERR_HIP
    after = ctx.debug_compare_host(X, truth)
    assert np.array_equal(good["raw"], after["raw"])
    g = make_graph(d=2, n=70, n_landmarks=3, n_ranges=20)
    A = asm.assemble(g)
    Q = orc.CSR.from_scipy(A["Q"])
    p = capi.Context(2, A["n"], A["r"], A["N"] - 2 * A["n"] - A["r"], Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=2)
    T = ground_truth(g)
    assert _raw(p, T, T) == ERR_ARG and "partitioned" in p.L.cora_last_error(p.h).decode()
    p.close()


def test_problem_compare_checks_its_shapes():
    path = os.path.join(GOLDEN, "small_ra_slam_problem", "factor_graph.pyfg")
    P = host.Problem.from_pyfg(path)
    P.update()
    T = P.ground_truth(path)
    with pytest.raises(host.HostError):
        P.compare(T[:-1], T)
    with pytest.raises(host.HostError):
        P.compare(T, T, select=[1, 0])
