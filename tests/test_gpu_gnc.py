"""The GNC weight step on the device (k_gnc_edges / k_gnc_ranges behind cora_gnc_weights*) against its host mirror and the
longdouble reference of tests/gnc_ref.py, what the step must leave alone, the device round trip into the assembly of
Q(w), and the robust solve (Problem.solve_robust, the command-line driver) against a loop written out by hand."""
import os
import subprocess

import numpy as np
import pytest

import gnc_ref as gr
import residuals_ref as rr
from conftest import GOLDEN
from cora_amd import capi, host
from oracle import assemble as asm
from oracle import oracle as orc
from synth import ground_truth, make_graph

pytestmark = pytest.mark.gpu
INF = float("inf")
KS = lambda d: (1, d, 5, 8, 17, 24)  # noqa: E731
COSTS = (gr.NONE, gr.TLS, gr.GM)


def on_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _ctx(g, table=None):
    A = asm.assemble(g)
    Q = orc.CSR.from_scipy(A["Q"])
    dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
    ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val)
    ctx.set_measurements(*(table or rr.table(g)))
    ctx.assembly_build(Q.rowptr, Q.col)
    return ctx, dm, Q


_GRAPHS = {}


def _graph(d):
    """The n = 70, 10-loop, 100-range graph of tests/test_gpu_residuals.py: 79 edges at d = 3, 78 at d = 2."""
    if d not in _GRAPHS:
        g = make_graph(d=d, n=70, n_landmarks=3, n_ranges=100, n_loops=10)
        assert len(rr.edges(g)) == (79 if d == 3 else 78) and len(g.ranges) == 100
        _GRAPHS[d] = (g,) + _ctx(g)
    return _GRAPHS[d]


def _thresholds(nw, rng, scale):
    c = rng.choice([0.3, 1.0, 7.8, 40.0], nw) * scale
    c[rng.uniform(size=nw) < 0.1] = INF
    return c


def _against_mirror(ctx, ne, X, c, cost, mu, couple, what):
    got = ctx.gnc_weights(X, c, cost, mu, couple)
    ref = ctx.debug_gnc_weights_host(X, c, cost, mu, couple)
    assert np.array_equal(got["r2"], ref["r2"]), what  # bit for bit
    worst = gr.check_weights(got["w"], got["r2"], c, ne, cost, mu, couple, what)
    print("%s: weights bit-equal to the mirror's: %s" % (what, np.array_equal(got["w"], ref["w"])))
    assert np.abs(got["w"] - ref["w"]).max(initial=0.0) <= 2 * gr.weight_bound(cost, mu)
    gr.check_statistics(got["stats_raw"], got["r2"], c, got["w"], ne, couple, what)  # counts and maxima exact, sums bounded
    gr.check_statistics(ref["stats_raw"], ref["r2"], c, ref["w"], ne, couple, what + " (mirror)")
    return got, worst


@pytest.mark.parametrize("d", [2, 3])
def test_device_against_mirror(d):
    g, ctx, dm, Q = _graph(d)
    ne, nw = len(rr.edges(g)), 2 * len(rr.edges(g)) + len(g.ranges)
    rng = np.random.default_rng(40 + d)
    mid = 0
    for k, mu in zip(KS(d), (0.3, 1.0, 1.4, 1e2, 1e-8, 1e8)):
        X = rng.standard_normal((dm.N, k)) * 0.2
        scale = np.median(ctx.debug_gnc_weights_host(X, np.full(nw, INF), gr.NONE)["r2"])
        c = _thresholds(nw, rng, scale)
        for cost in COSTS:
            for couple in (False, True):
                got, _ = _against_mirror(ctx, ne, X, c, cost, mu, couple, "d=%d k=%d" % (d, k))
                mid += int(got["stats_raw"][2::4].sum()) if cost != gr.NONE else 0
    assert mid > 0


@pytest.mark.parametrize("case", ["single_range", "single_rpm"])
def test_golden_cases_without_edges_and_without_ranges(case):
    g = asm.parse_pyfg(os.path.join(GOLDEN, case, "factor_graph.pyfg"))
    ctx, dm, Q = _ctx(g)
    ne, nw = len(rr.edges(g)), 2 * len(rr.edges(g)) + len(g.ranges)
    assert (ne == 0) if case == "single_range" else (len(g.ranges) == 0)
    X = np.random.default_rng(2).standard_normal((dm.N, 3))
    for cost in COSTS:
        for couple in (False, True):
            _against_mirror(ctx, ne, X, np.full(nw, 0.7), cost, 1.4, couple, case)
    ctx.close()


def test_grid_stride_path():
    """65 600 ranges = 2 050 groups of 32 on a grid capped at 2 048 blocks: blocks 0 and 1 take a second trip.  The rows
    repeat with period 64, so measurement j and measurement j + 65 536 hold equal records."""
    g = make_graph(d=2, n=70, n_landmarks=3, n_ranges=100, n_loops=10)
    er, ed, rg, rd = rr.table(g)
    reps = 1025
    ctx, dm, Q = _ctx(g, (er, ed, np.tile(rg[:64], (reps, 1)), np.tile(rd[:64], (reps, 1))))
    ne, nr = len(er), 64 * reps
    assert nr > 65536 and ctx.measurement_counts() == (ne, nr)
    rng = np.random.default_rng(8)
    c = np.full(2 * ne + nr, INF)
    c[2 * ne:] = np.tile(rng.choice([0.5, 3.0, 20.0], 64), reps)
    for k in (3, 4):
        X = rng.standard_normal((dm.N, k)) * 0.2
        for cost in (gr.TLS, gr.GM):
            got, _ = _against_mirror(ctx, ne, X, c, cost, 1.4, False, "grid-stride k=%d" % k)
            r2, w = got["r2"][2 * ne:], got["w"][2 * ne:]
            assert np.array_equal(r2[:64], r2[65536:65600]) and np.array_equal(w[:64], w[65536:65600])
            assert np.array_equal(r2, np.tile(r2[:64], reps)) and np.array_equal(w, np.tile(w[:64], reps))
            assert got["stats"]["range"]["n_out"] == reps * np.sum(w[:64] < 0.5)
    ctx.close()


def _dev_step(ctx, x, k, c, cost, mu, couple, nw):
    import torch
    dc = on_device(c)
    dw = torch.full((nw,), -7.0, dtype=torch.float64, device="cuda:0")
    dr = torch.full((nw,), -7.0, dtype=torch.float64, device="cuda:0")
    st = ctx.gnc_weights_dev(x, k, dc.data_ptr(), cost, mu, couple, dw.data_ptr(), dr.data_ptr())
    torch.cuda.synchronize()
    return dw, dr.cpu().numpy(), st["raw"].copy()


@pytest.mark.parametrize("d", [2, 3])
def test_independent_of_the_current_weights_and_device_round_trip(d):
    import torch
    import assembly_ref as ar
    g = make_graph(d=d, n=70, n_landmarks=3, n_ranges=100, n_loops=10)
    ctx, dm, Q = _ctx(g)
    ne, nw = len(rr.edges(g)), 2 * len(rr.edges(g)) + len(g.ranges)
    rng = np.random.default_rng(60 + d)
    k = 5
    X = rng.standard_normal((dm.N, k)) * 0.2
    x = ctx.dev_alloc(k)
    ctx.upload(X, x)
    c = _thresholds(nw, rng, np.median(ctx.debug_gnc_weights_host(X, np.full(nw, INF), gr.NONE)["r2"]))
    res0 = ctx.measurement_residuals_dev(x, k)
    dw0, r0, st0 = _dev_step(ctx, x, k, c, gr.TLS, 1.4, True, nw)
    assert np.array_equal(r0, np.concatenate([res0["edge_rot"], res0["edge_trans"], res0["range"]]))  # the residual kernels' bits
    wr = ar.random_weights(nw, 5)
    assert np.any(wr == 0.0)
    ctx.assemble_values_dev(on_device(wr).data_ptr())
    dw1, r1, st1 = _dev_step(ctx, x, k, c, gr.TLS, 1.4, True, nw)
    assert torch.equal(dw0, dw1) and np.array_equal(r0, r1) and np.array_equal(st0, st1)
    res1 = ctx.measurement_residuals_dev(x, k)
    assert not np.array_equal(res1["range"], res0["range"])  # (the residuals do follow the weights)
    # round trip: the step's device weights straight into the device assembly = the assembly of the downloaded weights
    out = torch.zeros(len(Q.val), dtype=torch.float64, device="cuda:0")
    ctx.assemble_values_dev(dw1.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ctx.assemble_values(dw1.cpu().numpy()))
    # all thresholds +inf: all ones, whatever the cost
    for cost in (gr.TLS, gr.GM):
        dw, _, st = _dev_step(ctx, x, k, np.full(nw, INF), cost, 0.3, False, nw)
        assert torch.all(dw == 1.0) and np.all(st[1::4] == 0.0) and np.all(st[2::4] == 0.0)
    ctx.dev_free(x)
    ctx.close()


@pytest.mark.parametrize("d", [2, 3])
def test_reproducible_position_independent_and_the_handle_untouched(d):
    g = make_graph(d=d, n=70, n_landmarks=3, n_ranges=100, n_loops=10)
    er, ed, rg, rd = rr.table(g)
    ctx, dm, Q = _ctx(g)
    ne, nw = len(er), 2 * len(er) + len(rg)
    rng = np.random.default_rng(80 + d)
    p = d + 1
    Y = orc.project_manifold(dm, rng.standard_normal((dm.N, p)))
    V = rng.standard_normal((dm.N, p))
    ctx.set_rank(p)
    ctx.precond_setup(capi.PRECOND_JACOBI)
    y, v, o1, o2 = (ctx.dev_alloc(p) for _ in range(4))
    ctx.upload(Y, y)
    ctx.upload(V, v)
    ctx.set_point_dev(y)

    def state():
        ctx.hvp_dev(v, o1)
        ctx.precondition_projected_dev(v, o2)
        return ctx.download(o1, p).copy(), ctx.download(o2, p).copy(), ctx.point_cost()

    before = state()
    runs = {}
    for k in KS(d):
        X = rng.standard_normal((dm.N, k)) * 0.2
        c = _thresholds(nw, rng, 0.05 * k)
        for cost in (gr.TLS, gr.GM):
            for couple in (False, True):
                a = ctx.gnc_weights(X, c, cost, 1.4, couple)
                b = ctx.gnc_weights(X, c, cost, 1.4, couple)
                for key in ("w", "r2", "stats_raw"):
                    assert np.array_equal(a[key], b[key]), (k, cost, couple, key)
                runs[(k, cost, couple)] = (X, c, a)
    after = state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    # edge 17 and range 41 alone in a table: the bits they have as entries 17 and 41
    ctx.set_measurements(er[17:18], ed[17:18], rg[41:42], rd[41:42])
    ctx.assembly_build(Q.rowptr, Q.col)
    for (k, cost, couple), (X, c, a) in runs.items():
        pick = [17, ne + 17, 2 * ne + 41]
        one = ctx.gnc_weights(X, c[pick], cost, 1.4, couple)
        assert np.array_equal(one["w"], a["w"][pick]) and np.array_equal(one["r2"], a["r2"][pick]), (k, cost, couple)
    for ptr in (y, v, o1, o2):
        ctx.dev_free(ptr)
    ctx.close()


# ---- the robust solve -------------------------------------------------------------------------------------------------
BAD = (3, 11, 19, 27, 42, 55)  # the ranges replaced by grossly wrong distances
SHIFT = 10.0                   # added to the measured distance: 100 sigma at sigma = 0.1
BARC2 = 25.0                   # 5 sigma on one degree of freedom


def _corrupted(d, shift=SHIFT):
    g = make_graph(d=d, n=30, n_landmarks=3, n_ranges=60, n_loops=5)
    for i in BAD:
        a, b, r, cov = g.ranges[i]
        g.ranges[i] = (a, b, r + shift, cov)
    return g


def _problem(g):
    P = host.Problem.new(g.dim)
    for s in g.poses:
        P.add_pose(s)
    for s in g.landmarks:
        P.add_landmark(s)
    for a, b, R, t, cov in g.rpms:
        P.add_rel_pose(a, b, R, t, cov)
    for a, b, r, cov in g.ranges:
        P.add_range(a, b, r, cov)
    P.update()
    return P


def _by_hand(g, cost, mu_factor=1.4, max_outer=100):
    """solveRobustCORA's loop from calls that exist without it: solve, the UNWEIGHTED residuals from a second Problem that
    is never re-weighted, the numpy formulas of gnc_ref, reweight."""
    P, P2 = _problem(g), _problem(g)
    nr = len(g.ranges)
    c = np.full(nr, BARC2)
    res = P.solve(ground_truth(g), max_rank=10)
    r2 = P2.measurement_residuals(res["x"])["range"]
    rho_max = float((r2 / c).max())
    w = np.ones(nr)
    if rho_max <= 1:
        return res, w, 0
    mu = 1 / (2 * rho_max - 1) if cost == gr.TLS else 2 * rho_max
    prev, rounds = None, 0
    while True:
        w_new = gr.weights_float64(P2.measurement_residuals(res["x"])["range"], c, 0, cost, mu, True)
        if cost == gr.TLS and prev is not None and not np.any((w_new > 0) & (w_new < 1)) and np.array_equal(w_new, prev):
            break
        if rounds >= max_outer:
            break
        w = w_new
        P.reweight({"range": w})
        res = P.solve(res["x"], max_rank=10)
        rounds += 1
        if cost == gr.GM and mu == 1.0:
            break
        mu = mu * mu_factor if cost == gr.TLS else max(1.0, mu / mu_factor)
        prev = w
    return res, w, rounds


def _flagged(w):
    return tuple(int(i) for i in np.flatnonzero(np.asarray(w) < 0.5))


@pytest.mark.parametrize("cost", [gr.TLS, gr.GM])
@pytest.mark.parametrize("d", [2, 3])
def test_robust_solve_recovers_the_injected_outliers(d, cost):
    g = _corrupted(d)
    hand, w_hand, rounds = _by_hand(g, cost)
    print("by hand, d=%d %s: %d rounds, f = %.9g, flagged %s" % (d, cost, rounds, hand["f"], _flagged(w_hand)))
    assert _flagged(w_hand) == BAD  # a condition on the inputs: corruption size and seed are chosen so that it holds
    if cost == gr.TLS:
        assert np.all(w_hand[list(BAD)] == 0.0) and np.all(np.delete(w_hand, BAD) == 1.0)
    P = _problem(g)
    res = P.solve_robust(ground_truth(g), {"range": np.full(len(g.ranges), BARC2)}, cost=cost)
    w = res["weights"]["range"]
    print("solve_robust: %d rounds, converged %s, f = %.9g, flagged %s" % (res["outer_iterations"], res["converged"], res["f"], _flagged(w)))
    assert res["converged"] and _flagged(w) == BAD
    assert all(np.all(res["weights"][k] == 1.0) for k in res["weights"] if k != "range")  # the edges are trusted
    assert abs(res["f"] - hand["f"]) <= 1e-6 * abs(hand["f"])
    assert len(res["mu_history"]) == len(res["sum_wr2_history"]) >= res["outer_iterations"] > 0
    assert np.array_equal(P.get_measurement_weights()["range"], w)  # the Problem is left weighted with the final weights


@pytest.mark.parametrize("d", [2, 3])
def test_robust_solve_without_corruption_is_one_solve(d):
    g = _corrupted(d, shift=0.0)
    P = _problem(g)
    plain = _problem(g).solve(ground_truth(g), max_rank=10)
    res = P.solve_robust(ground_truth(g), {"range": np.full(len(g.ranges), BARC2)}, cost=gr.TLS)
    assert res["converged"] and res["outer_iterations"] == 0 and len(res["mu_history"]) == 0
    assert all(np.all(v == 1.0) for v in res["weights"].values())
    assert float(res["f"]).hex() == float(plain["f"]).hex()


def _write_pyfg(g, path):
    """A d = 2 graph of make_graph as text (poses at the origin: the driver starts from the odometry)."""
    assert g.dim == 2 and not g.rplms and not g.pose_priors and not g.landmark_priors
    with open(path, "w") as f:
        for i, s in enumerate(g.poses):
            f.write("VERTEX_SE2 %d.0 %s 0 0 0\n" % (i, s))
        for s in g.landmarks:
            f.write("VERTEX_XY %s 0 0\n" % s)
        for i, (a, b, R, t, cov) in enumerate(g.rpms):
            up = " ".join("%.17g" % cov[r, c] for r in range(3) for c in range(r, 3))
            f.write("EDGE_SE2 %d.0 %s %s %.17g %.17g %.17g %s\n" % (i, a, b, t[0], t[1], np.arctan2(R[1, 0], R[0, 0]), up))
        for i, (a, b, r, cov) in enumerate(g.ranges):
            f.write("EDGE_RANGE %d.0 %s %s %.17g %.17g\n" % (i, a, b, r, cov))


def test_command_line_driver_reproduces_the_set(tmp_path):
    from cora_amd import build as _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = _build.build()
    exe = str(tmp_path / "cora_main")
    subprocess.run([_build.HIPCC, "-O1", "-std=c++17", "-I" + os.path.join(root, "include"),
                    "-I" + os.path.join(root, "cora_amd", "csrc", "host"), os.path.join(root, "examples", "main.cpp"),
                    "-L" + os.path.dirname(lib), "-lcora_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe],
                   check=True, timeout=600)
    pyfg, out = str(tmp_path / "corrupted.pyfg"), str(tmp_path / "w.csv")
    _write_pyfg(_corrupted(2), pyfg)
    r = subprocess.run([exe, pyfg, "--odom-init", "--robust", "tls", "--barc2", "range=%g" % BARC2, "--weights-out", out],
                       stdout=subprocess.PIPE, text=True, timeout=300, check=True)
    assert "robust solve (tls)" in r.stdout and "converged" in r.stdout, r.stdout[-2000:]
    rows = [line.split(",") for line in open(out).read().split()]
    w = np.array([float(v) for kind, i, v in rows if kind == "range"])
    assert len(w) == 60 and [int(i) for kind, i, v in rows if kind == "range"] == list(range(60))
    assert _flagged(w) == BAD and np.all(w[list(BAD)] == 0.0) and np.all(np.delete(w, BAD) == 1.0)
    assert all(float(v) == 1.0 for kind, i, v in rows if kind != "range")
