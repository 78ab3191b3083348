"""Per-measurement residuals on the device (k_edge_residuals / k_range_residuals behind cora_measurement_residuals*)
against the numpy reference of tests/residuals_ref.py: through capi.Context on the golden cases and on small synthetic
graphs at every column count, through host.Problem for every measurement kind and both formulations, and at the point
a full solve returns."""
import os

import numpy as np
import pytest

import residuals_ref as rr
from conftest import EXPECTED_COST, GOLDEN
from cora_amd import capi, host
from mmio import read_dense
from oracle import assemble as asm
from oracle import oracle as orc
from synth import make_graph

pytestmark = pytest.mark.gpu
REL = 1e-10  # the project's oracle tolerance, relative to the largest value: only the summation order differs


def _ctx(g):
    A = asm.assemble(g)
    Q = orc.CSR.from_scipy(A["Q"])
    dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
    ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val)
    ctx.set_measurements(*rr.table(g))
    return ctx, dm


def _close(got, ref, keys=("edge_rot", "edge_trans", "range")):
    largest = max(max(np.abs(ref[k]).max(initial=0.0) for k in keys), 1e-300)
    for k in keys:
        assert got[k].shape == ref[k].shape, k
        err = np.abs(got[k] - ref[k]).max(initial=0.0)
        print("%s: max error %.3e of largest value %.3e" % (k, err, largest))
        assert err <= REL * largest, k


_GRAPHS = {}


def _graph(d):
    """The n = 70 graph with 10 loop closures drawn and 100 ranges -- 79 edges at d = 3, 78 at d = 2 (one drawn pair is no
    loop), neither count a multiple of a lane group's 8 or of a block's 32 measurements --, its handle and table: one per d."""
    if d not in _GRAPHS:
        g = make_graph(d=d, n=70, n_landmarks=3, n_ranges=100, n_loops=10)
        assert len(rr.edges(g)) == (79 if d == 3 else 78) and len(g.ranges) == 100
        _GRAPHS[d] = (g,) + _ctx(g) + (rr.table(g),)
    return _GRAPHS[d]


def test_golden_cases(case):
    """single_range is the zero-edge launch, single_rpm the zero-range launch."""
    g = asm.parse_pyfg(os.path.join(GOLDEN, case, "factor_graph.pyfg"))
    ctx, dm = _ctx(g)
    assert ctx.measurement_counts() == (len(rr.edges(g)), len(g.ranges))
    X = read_dense(os.path.join(GOLDEN, case, "X_rand_dim2.mm"))
    got = ctx.measurement_residuals(X)
    ref = rr.reference(g, X)
    _close(got, ref)
    cost = EXPECTED_COST[case]
    assert abs(0.5 * got["sums"].sum() - cost) < 1e-9 * max(1.0, abs(cost))
    for j in range(3):  # the totals are the sums of the values
        assert abs(got["sums"][j] - ref["sums"][j]) <= REL * max(ref["sums"].max(), 1e-300)


@pytest.mark.parametrize("d", [2, 3])
def test_every_column_count(d):
    """k = 1 (row stride 2, padding column), odd strides (8-byte pieces), even strides (16-byte pieces), more pieces
    than lanes of a group (k > 16 even, k > 8 odd), a last partially filled group and block."""
    g, ctx, dm, _ = _graph(d)
    rng = np.random.default_rng(100 + d)
    for k in range(1, 25):
        X = rng.standard_normal((dm.N, k))
        got = ctx.measurement_residuals(X)
        _close(got, rr.reference(g, X))
        half = 0.5 * got["sums"].sum()
        if k >= d:
            ctx.set_rank(k)
            f = ctx.evaluateObjective(X)
        else:  # no relaxation rank below d: the same handle's product instead, f = 1/2 <X, Q X>
            f = 0.5 * np.sum(X * ctx.dataMatrixProduct(X))
        assert abs(half - f) <= 1e-9 * abs(f), (k, half, f)


@pytest.mark.parametrize("d", [2, 3])
def test_position_independence_and_determinism(d):
    """A measurement has the same bits as the only entry of a table and as entry 17 / 41 of a longer one, and two calls
    on the same table give the same bits, totals included."""
    g, ctx, dm, (er, ed, rg, rd) = _graph(d)
    rng = np.random.default_rng(7 + d)
    try:
        for k in (1, d, 5, 8, 17, 24):
            X = rng.standard_normal((dm.N, k))
            x = ctx.dev_alloc(k)
            ctx.upload(X, x)
            ctx.set_measurements(er, ed, rg, rd)
            a1 = ctx.measurement_residuals_dev(x, k)
            a2 = ctx.measurement_residuals_dev(x, k)
            for key in ("edge_rot", "edge_trans", "range", "sums"):
                assert np.array_equal(a1[key], a2[key]), key
            ctx.set_measurements(er[17:18], ed[17:18], rg[41:42], rd[41:42])
            b = ctx.measurement_residuals_dev(x, k)
            assert b["edge_rot"][0] == a1["edge_rot"][17] and b["edge_trans"][0] == a1["edge_trans"][17]
            assert b["range"][0] == a1["range"][41]
            assert np.array_equal(b["sums"], [b["edge_rot"][0], b["edge_trans"][0], b["range"][0]])
            ctx.dev_free(x)
    finally:
        ctx.set_measurements(er, ed, rg, rd)


def _rot(d, rng, s):
    if d == 2:
        return asm._from_angle(rng.normal(0, s))
    w = rng.normal(0, s, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _all_kinds(d, implicit, rank):
    """5 poses, 2 landmarks, odometry, a reversed loop closure, a pose prior, a landmark prior, a pose-landmark edge and a
    pose-pose, a pose-landmark and a landmark-landmark range: the host's Problem and the same graph for the reference."""
    rng = np.random.default_rng(31 + d)
    P = host.Problem.new(d, rank=rank, implicit=implicit)
    g = asm.PyFG()
    g.dim = d
    cov = np.diag([0.05 ** 2] * d + [0.01 ** 2] * (3 if d == 3 else 1))
    covt = np.eye(d) * 0.07 ** 2
    for i in range(5):
        P.add_pose("A%d" % i)
        g._add_pose("A%d" % i)
    for k in range(2):
        P.add_landmark("L%d" % k)
        g.landmarks["L%d" % k] = k

    def rel_pose(a, b):
        R, t = _rot(d, rng, 0.3), rng.normal(0, 1.0, d)
        P.add_rel_pose(a, b, R, t, cov)
        g.rpms.append((a, b, R, t, cov))

    for i in range(4):
        rel_pose("A%d" % i, "A%d" % (i + 1))
    rel_pose("A4", "A1")  # reversed: b before a
    R, t = _rot(d, rng, 0.3), rng.normal(0, 1.0, d)
    P.add_pose_prior("A0", R, t, cov)
    g.pose_priors.append(("A0", R, t, cov))
    g._origin()
    pos = rng.normal(0, 3.0, d)
    P.add_landmark_prior("L0", pos, covt)
    g.landmark_priors.append(("L0", pos, covt))
    t = rng.normal(0, 2.0, d)
    P.add_rel_pose_landmark("A2", "L1", t, covt)
    g.rplms.append(("A2", "L1", t, covt))
    for a, b in (("A0", "A3"), ("A4", "L0"), ("L0", "L1")):
        dist = float(rng.uniform(1.0, 5.0))
        P.add_range(a, b, dist, 0.01)
        g.ranges.append((a, b, dist, 0.01))
    P.update()
    dm = P.dims()
    assert (dm["n"], dm["l"], dm["r"]) == (6, 2, 3)
    return P, g, orc.Dims(dm["d"], dm["n"], dm["r"], dm["N"])


def _same(got, ref):
    names = ("rel_pose_rot", "rel_pose_trans", "pose_prior_rot", "pose_prior_trans", "pose_landmark", "landmark_prior",
             "range")
    _close(got, ref, names)
    for s in ("rot_sum", "trans_sum", "range_sum"):
        assert abs(got[s] - ref[s]) <= REL * max(ref["rot_sum"], ref["trans_sum"], ref["range_sum"]), s


@pytest.mark.parametrize("d", [2, 3])
def test_all_measurement_kinds_and_the_implicit_formulation(d):
    p = d + 2
    P, g, dims = _all_kinds(d, False, p)
    rng = np.random.default_rng(d)
    Y = orc.project_manifold(dims, rng.uniform(-1, 1, (dims.N, p)))
    got = P.measurement_residuals(Y)
    assert [len(got[k]) for k in ("rel_pose_rot", "pose_prior_trans", "pose_landmark", "landmark_prior", "range")] == [5, 1, 1, 1, 3]
    _same(got, rr.by_kind(rr.reference(g, Y)))
    f = P.op("evaluateObjective", Y)
    assert abs(0.5 * (got["rot_sum"] + got["trans_sum"] + got["range_sum"]) - f) <= 1e-9 * abs(f)
    Xd = rng.standard_normal((dims.N, d))  # any column count, on the manifold or not
    _same(P.measurement_residuals(Xd), rr.by_kind(rr.reference(g, Xd)))
    with pytest.raises(host.HostError):
        P.measurement_residuals(Y[:-1])
    # implicit formulation: the residuals at Y are the explicit problem's at the completed point
    PI, gi, _ = _all_kinds(d, True, p)
    Yi = Y[:dims.dn + dims.r]
    X = PI.op("getTranslationExplicitSolution", Yi)
    assert X.shape == (dims.N, p) and np.array_equal(X[:dims.dn + dims.r], Yi)
    gi_res = PI.measurement_residuals(Yi)
    _same(gi_res, P.measurement_residuals(X))
    _same(gi_res, rr.by_kind(rr.reference(g, X)))


def test_after_a_solve_half_the_total_is_the_cost():
    P = host.Problem.from_pyfg(os.path.join(GOLDEN, "datasets", "plaza2.pyfg"))
    P.update()
    res = P.solve(P.op("getRandomInitialGuess"), max_rank=10, max_seconds=60)
    got = P.measurement_residuals(res["x"])
    half = 0.5 * (got["rot_sum"] + got["trans_sum"] + got["range_sum"])
    print("plaza2: f = %.12g, half the residuals = %.12g" % (res["f"], half))
    assert abs(half - res["f"]) <= 1e-8 * abs(res["f"])
    dm = P.dims()
    assert len(got["rel_pose_rot"]) == dm["rpm"] and len(got["range"]) == dm["r"]
    assert min(v.min(initial=0.0) for v in got.values() if isinstance(v, np.ndarray)) >= 0.0
