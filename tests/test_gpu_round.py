"""The rounding to SE(d) on the device (k_round_count, k_round_finish, k_round_apply behind cora_round*) against the
mpmath / longdouble reference of tests/round_ref.py within the calibrated bound, bit for bit against the host mirror given
the device's basis, at the launch edges, what the call must leave alone, the catalogue and degenerate blocks of the CPU
file, Problem.round_solution against Problem.project_solution, end to end through solveCORA, and chained with the
trajectory comparison and the relative pose error on the rounded resident vector."""
import os

import numpy as np
import pytest

import round_ref as rf
import rowops_ref as ro
import rpe_ref as rp
from conftest import GOLDEN
from cora_amd import capi, host
from oracle import assemble as asm
from oracle import oracle as orc
from synth import ground_truth, make_graph

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, "datasets")

_BUILT = {}


def graph_ctx(g):
    A = asm.assemble(g)
    Q = orc.CSR.from_scipy(A["Q"])
    dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
    return capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val), (dm.d, dm.n, dm.r, dm.n_trans), ground_truth(g)


def built(d, n):
    """(ctx, (d, n, r, nt), ground truth) of a graph of make_graph at its default seed, once per process."""
    key = (d, n)
    if key not in _BUILT:
        _BUILT[key] = graph_ctx(make_graph(d=d, n=n, n_landmarks=3, n_ranges=min(20, n * 3), n_loops=0))
    return _BUILT[key]


def against_host_mirror(ctx, dev, Y, what):
    mir = ctx.debug_round_host(Y, basis=dev["Vd"])
    assert np.array_equal(dev["X"], mir["X"]), (what, float(np.abs(dev["X"] - mir["X"]).max()))
    assert dev["count"] == mir["count"] and dev["flipped"] == mir["flipped"], what


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", [1, 2, 30, 64, 65, 300])
def test_device_against_the_reference_and_the_host_mirror(d, n):
    ctx, dims, truth = built(d, n)
    rng = np.random.default_rng(100 * d + n)
    for k in rf.KS(d):
        what = "d=%d n=%d k=%d" % (d, n, k)
        Y = rf.relaxed_point(truth, *dims, k, rng)
        dev = ctx.round(Y)
        rf.check(dev, Y, *dims, what=what)
        rf.basis_checks(dev, Y, what=what)
        against_host_mirror(ctx, dev, Y, what)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("units", [255, 256, 257, 513])
def test_launch_edges_of_the_apply_pass(d, units):
    """poses + ranges + translations = units: the last block of the apply pass full, one short, one over, two over."""
    n_landmarks, n_ranges = 3, 20
    n = (units - n_landmarks - n_ranges) // 2
    g = make_graph(d=d, n=n, n_landmarks=n_landmarks + (units - n_landmarks - n_ranges) % 2, n_ranges=n_ranges, n_loops=0)
    ctx, dims, truth = graph_ctx(g)
    assert dims[1] + dims[2] + dims[3] == units
    rng = np.random.default_rng(units + d)
    Y = rf.relaxed_point(truth, *dims, d + 2, rng)
    dev = ctx.round(Y)
    rf.check(dev, Y, *dims, what="units=%d d=%d" % (units, d))
    against_host_mirror(ctx, dev, Y, "units=%d" % units)
    ctx.close()


def test_more_than_one_round_of_the_finish():
    """5 000 poses are 79 partials of the count pass: the one-wavefront finish goes round twice.  Fewer than half the
    blocks are proper, so the flip is taken too."""
    g = make_graph(d=2, n=5000, n_landmarks=3, n_ranges=40, n_loops=0)
    ctx, dims, truth = graph_ctx(g)
    d, n = dims[0], dims[1]
    rng = np.random.default_rng(5000)
    k = 4
    Vd = rf.basis(d, k)
    Y = rf.in_span(truth, dims, Vd, rng)
    rot = rf.rows(*dims)[0]
    mirrored = rng.permutation(n)[:n - 2400]
    for i in mirrored:
        M = Y[rot[i]] @ Vd
        M[:, -1] = -M[:, -1]
        Y[rot[i]] = M @ Vd.T
    dev = ctx.round(Y)
    mir = ctx.debug_round_host(Y, basis=dev["Vd"])
    assert dev["count"] == mir["count"] and dev["flipped"] == mir["flipped"]
    assert dev["count"] in (2400, n - 2400), dev["count"]   # (the device's basis may itself be a reflection of Vd)
    assert dev["flipped"] == (dev["count"] < n // 2)
    assert np.array_equal(dev["X"], mir["X"])
    sample = rng.permutation(n)[:40]
    for i in sample:
        err, kap, _ = rf.block_error(dev["X"][rot[i]], Y[rot[i]], dev["Vd"], dev["flipped"])
        assert err <= rf.ROUND_BOUND and ro.orth_error(dev["X"][rot[i]]) <= rf.ORTH_BOUND, (i, err)
    ctx.close()


@pytest.mark.parametrize("d", [2, 3])
def test_resident_form_leaves_the_input_and_the_handle_alone(d):
    g = make_graph(d=d, n=70, n_landmarks=3, n_ranges=100, n_loops=10)
    ctx, dims, truth = graph_ctx(g)
    N = truth.shape[0]
    dm = orc.Dims(dims[0], dims[1], dims[2], N)
    rng = np.random.default_rng(80 + d)
    p = d + 1
    P0 = orc.project_manifold(dm, rng.standard_normal((N, p)))
    ctx.set_rank(p)
    pt = ctx.dev_alloc(p)
    ctx.upload(P0, pt)
    ctx.set_point_dev(pt)
    f0 = ctx.point_cost()
    g0 = ctx.download(ctx.point_ptrs()[2], p).copy()
    k = 5
    Y = rf.relaxed_point(truth, *dims, k, rng)
    y, out = ctx.dev_alloc(k), ctx.dev_alloc(d)
    ctx.upload(Y, y)
    before = ctx.download(y, k).copy()
    dev = ctx.round_dev(y, k, out)
    X = ctx.download(out, d).copy()
    assert np.array_equal(ctx.download(y, k), before), "the input vector is unchanged"
    assert ctx.point_cost() == f0 and np.array_equal(ctx.download(ctx.point_ptrs()[2], p), g0), "cost and gradient"
    again = ctx.round_dev(y, k, out)
    assert np.array_equal(ctx.download(out, d), X) and np.array_equal(again["raw"], dev["raw"]), "a second call gives the same bits"
    hostform = ctx.round(Y)
    assert np.array_equal(hostform["X"], X) and np.array_equal(hostform["raw"], dev["raw"]), "cora_round equals cora_round_dev"
    dev["X"] = X
    rf.check(dev, Y, *dims, what="resident d=%d" % d)
    with pytest.raises(capi.CoraError) as e:   # the output must not alias the input
        ctx.round_dev(y, k, y)
    assert e.value.code == 5
    for ptr in (pt, y, out):
        ctx.dev_free(ptr)
    ctx.close()


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("large", [False, True])
def test_catalogue_blocks_on_the_device(d, large):
    """Every row of the input lies in the span of one basis, so the device's own basis spans the same space and Y_i Vd is
    the catalogue block times an orthogonal d x d matrix: the same singular values, the same Gram matrix of its rows."""
    ctx, dims, truth = built(d, 30)
    rng = np.random.default_rng(300 + d)
    blocks = [ro.block(name, kk, d, d, seed) for name, kk, seed in rf.catalogue(d, large)]
    for k in rf.KS(d):
        what = "catalogue d=%d k=%d large=%s" % (d, k, large)
        Vd = rf.basis(d, k)
        Y = rf.with_blocks(rf.in_span(truth, dims, Vd, rng), d, blocks, Vd)
        dev = ctx.round(Y)
        rf.check(dev, Y, *dims, what=what)
        against_host_mirror(ctx, dev, Y, what)


@pytest.mark.parametrize("d", [2, 3])
def test_degenerate_blocks_on_the_device(d):
    ctx, dims, truth = built(d, 30)
    rng = np.random.default_rng(500 + d)
    rot, rng_rows, _ = rf.rows(*dims)
    for k in rf.KS(d):
        Vd = rf.basis(d, k)
        u = rng.standard_normal(d)
        blocks = [np.zeros((d, d)), np.outer(rng.standard_normal(d), u), np.outer(np.eye(d)[0], u)]
        if d == 3:
            B = rng.standard_normal((3, 3))
            B[2] = 0.5 * B[0] - 2.0 * B[1]
            C = rng.standard_normal((3, 3))
            C[1] = 0.0
            blocks += [B, C]
        Y = rf.with_blocks(rf.in_span(truth, dims, Vd, rng), d, blocks, Vd, first=3)
        Y[rng_rows[2]] = 0.0
        dev = ctx.round(Y)
        rf.check(dev, Y, *dims, what="degenerate d=%d k=%d" % (d, k), blocks=False)
        against_host_mirror(ctx, dev, Y, "degenerate d=%d k=%d" % (d, k))
        assert np.array_equal(dev["X"][rot[3]], np.eye(d)), "a zero block gives exactly the identity"
        assert np.all(dev["X"][rng_rows[2]] == 0.0), "a zero range row stays zero"
    for bad in (np.nan, np.inf):
        Y = rf.relaxed_point(truth, *dims, 5, rng)
        Y[11, 2] = bad
        with pytest.raises(capi.CoraError) as e:
            ctx.round(Y)
        assert e.value.code == 3, bad
    for e2 in (600, -600, 1000, -1040):   # squares that overflow or vanish altogether, the last with every entry subnormal
        Y = rf.relaxed_point(truth, *dims, 5, rng)
        base, res = ctx.round(Y), ctx.round(np.ldexp(Y, e2))
        assert res["count"] == base["count"] and res["flipped"] == base["flipped"]
        lost = 2.0 ** max(0, -e2 - 1022 + 8)   # (a subnormal input is itself a rounded copy)
        assert np.abs(res["X"][rot.ravel()] - base["X"][rot.ravel()]).max() <= 1e-9 * lost
        against_host_mirror(ctx, res, np.ldexp(Y, e2), "scaled by 2^%d" % e2)


# ---- Problem.round_solution
def problems():
    """plaza2 and one synthetic graph as host Problems (name, Problem, Q, dims), once per process."""
    if "problems" not in _BUILT:
        out = []
        P = host.Problem.from_pyfg(os.path.join(DATA, "plaza2.pyfg"))
        P.update()
        out.append(("plaza2", P))
        g = make_graph(d=3, n=60, n_landmarks=3, n_ranges=40, n_loops=6)
        S = host.Problem.new(g.dim)   # the programmatic API, as tests/test_gpu_rpe.py feeds it
        for sym in g.poses:
            S.add_pose(sym)
        for sym in g.landmarks:
            S.add_landmark(sym)
        for a, b, R, t, cov in g.rpms:
            S.add_rel_pose(a, b, R, t, cov)
        for a, b, r, cov in g.ranges:
            S.add_range(a, b, r, cov)
        S.update()
        out.append(("synth", S))
        res = []
        for name, P in out:
            dm = P.dims()
            _, _, rowptr, colidx, vals = P.matrix("DataMatrix")
            res.append((name, P, orc.CSR(rowptr, colidx, vals, dm["N"]), orc.Dims(dm["d"], dm["n"], dm["r"], dm["N"])))
        _BUILT["problems"] = res
    return _BUILT["problems"]


@pytest.mark.parametrize("which", [0, 1])
def test_round_solution_against_project_solution(which):
    name, P, Q, dims = problems()[which]
    d = dims.d
    rng = np.random.default_rng(40 + which)
    P.set_formulation(False)
    for k in (d + 1, 5):
        P.set_rank(k)
        Y = P.op("projectToManifold", rng.uniform(-1, 1, (dims.N, k)))
        Y[:, d:] *= 0.05    # close to rank d, as a certified point is
        Y = P.op("projectToManifold", Y)
        Xh = P.project_solution(Y)
        Xd, info = P.round_solution(Y, info=True)
        fh, fd = orc.cost(Q, Xh), orc.cost(Q, Xd)
        assert abs(fh - fd) <= 1e-9 * abs(fh), (name, k, fh, fd)
        R = np.linalg.lstsq(Xd, Xh, rcond=None)[0]   # equal up to one rotation on the right
        assert np.abs(R.T @ R - np.eye(d)).max() < 1e-6 and np.linalg.det(R) > 0
        assert np.abs(Xd @ R - Xh).max() < 1e-6
        assert len(info["sigma"]) == k and np.all(np.diff(info["sigma"]) <= 0)
    P.set_rank(d)


def test_round_solution_refuses_bad_column_counts():
    name, P, Q, dims = problems()[1]
    P.set_formulation(False)
    for k in (dims.d - 1, 25):
        with pytest.raises(host.HostError, match="column count must lie in"):
            P.round_solution(np.zeros((dims.N, k)))


def test_round_solution_in_the_implicit_formulation():
    name, P, Q, dims = problems()[0]
    d = dims.d
    rng = np.random.default_rng(77)
    k = d + 2
    P.set_rank(k)
    Yfull = P.op("projectToManifold", rng.uniform(-1, 1, (dims.N, k)))
    explicit = P.round_solution(Yfull)
    P.set_formulation(True)
    try:
        rows = d * dims.n + dims.r
        Xi = P.round_solution(Yfull[:rows])
        assert Xi.shape == (rows, d)
        lifted = np.zeros_like(Yfull)
        lifted[:rows] = Yfull[:rows]
        P.set_formulation(False)
        want = P.round_solution(lifted)[:rows]   # the same call on [Y; 0]
        assert np.array_equal(Xi, want)
        assert explicit.shape == (dims.N, d)
    finally:
        P.set_formulation(False)
        P.set_rank(d)


# ---- end to end
@pytest.mark.parametrize("which", [0, 1])
def test_solve_with_device_rounding(which):
    name, P, Q, dims = problems()[which]
    P.set_formulation(False)
    P.set_preconditioner(capi.PRECOND_REGULARIZED_CHOLESKY)

    # from rank d + 1, so that the certified point has more than d columns and the rounding step runs whatever the
    # staircase does
    def solve(**kw):
        P.set_rank(dims.d + 1)
        return P.solve(x0, max_rank=10, max_seconds=60, **kw)
    P.set_rank(dims.d + 1)
    x0 = P.op("getRandomInitialGuess")
    assert x0.shape[1] == dims.d + 1
    plain, plain2, dev = solve(), solve(), solve(device_rounding=True)
    assert np.array_equal(plain["x"], plain2["x"]) and plain["f"] == plain2["f"], "the default path is deterministic"
    X = dev["x"]
    assert X.shape[1] == dims.d and dev["final_rank"] == dims.d and plain["final_rank"] == dims.d
    assert np.abs(X - orc.project_manifold(dims, X)).max() < 1e-9      # checkVariablesAreValid accepted it
    P.op("alignEstimateToOrigin", X)                                     # (which calls checkVariablesAreValid itself)
    assert abs(orc.cost(Q, X) - dev["f"]) < 1e-9 * max(1.0, abs(dev["f"]))
    if name == "plaza2":
        assert abs(dev["f"] - 734.328) < 2e-3 and abs(plain["f"] - 734.328) < 2e-3
    assert abs(dev["f"] - plain["f"]) <= 2e-3
    assert dev["certified"] == plain["certified"] and dev["relaxation_certified"] == plain["relaxation_certified"]
    print("\n%s: f %.6f (default %.6f) certified %s" % (name, dev["f"], plain["f"], dev["certified"]))


# ---- chaining on resident vectors
@pytest.mark.parametrize("d", [2, 3])
def test_round_then_evaluate_on_the_device(d):
    """Round on the device, evaluate the rounded resident vector there; the same evaluations of the HOST-rounded point
    (the mirror on its own basis, uploaded).  The two rounded points differ by delta = max |entry| (the two Gram matrices
    are summed in different orders); the results may differ by the calls' own rounding bounds plus what delta does to
    exact arithmetic:
      rpe      u = X_i (x_j - x_i)^T moves by |dX_i|_F |x_j - x_i| + |X_i|_F |d(x_j - x_i)| <= d delta (|x_j - x_i| + 2),
               E = X_i X_j^T by 2 d sqrt(d) delta;
      compare  with the alignment fixed a row's error moves by the row's change; the alignment, a polar factor of
               H = Xc^T Gc, moves by at most 2 |dH|_F / (sigma_{d-1} + sigma_d) <= 4 sqrt(n d) delta |Gc|_F / (..).
    Second-order terms are covered by a factor 2 on these."""
    ctx, dims, truth = built(d, 65)
    n = dims[1]
    rng = np.random.default_rng(900 + d)
    k = 5
    Y = rf.relaxed_point(truth, *dims, k, rng)
    pairs = np.concatenate([rp.pairs_by_step([list(range(n))], 1)[0], rp.pairs_by_step([list(range(n))], 5)[0]]).astype(np.int32)
    ctx.set_pose_pairs(pairs)
    y, out, ref, up = ctx.dev_alloc(k), ctx.dev_alloc(d), ctx.dev_alloc(d), ctx.dev_alloc(d)
    ctx.upload(Y, y)
    ctx.upload(truth, ref)
    ctx.round_dev(y, k, out)
    Xd = ctx.download(out, d).copy()
    cmp_dev = ctx.compare_dev(out, d, ref, d, proper=True)
    rpe_dev = ctx.rpe_dev(out, d, ref, d)
    Xh = ctx.debug_round_host(Y)["X"]
    ctx.upload(Xh, up)
    cmp_up = ctx.compare_dev(up, d, ref, d, proper=True)
    rpe_up = ctx.rpe_dev(up, d, ref, d)
    delta = float(np.abs(Xd - Xh).max())
    print("d=%d: device-rounded against host-rounded point: max |difference| %.3e" % (d, delta))
    assert delta <= 1e-10
    rot, trn = rp.rows(*dims)
    i, j = pairs[:, 0], pairs[:, 1]
    bt_a, br_a = rp.bounds(Xd, truth, *dims, pairs)
    bt_b, br_b = rp.bounds(Xh, truth, *dims, pairs)
    dx = np.linalg.norm(Xd[trn[j]] - Xd[trn[i]], axis=1)
    assert np.all(np.abs(rpe_dev["trans_err"] - rpe_up["trans_err"]) <= bt_a + bt_b + 2 * d * delta * (dx + 2))
    assert np.all(np.abs(rpe_dev["rot_err"] - rpe_up["rot_err"]) <= br_a + br_b + 2 * 2 * d * np.sqrt(d) * delta)
    rp.check(rpe_dev, Xd, truth, *dims, pairs, what="rpe of the rounded point d=%d" % d)
    Gc = truth[trn[:n]] - truth[trn[:n]].mean(axis=0)
    Xc = Xd[trn[:n]] - Xd[trn[:n]].mean(axis=0)
    sig = np.sort(cmp_dev["sigma"])[::-1]
    dA = 4 * np.sqrt(n * d) * delta * np.linalg.norm(Gc) / (sig[d - 2] + sig[d - 1])
    own = 64 * (k + d) * rf.EPS * (1 + np.abs(Xd).max()) ** 2   # (the call's own rounding, far below the rest)
    lim_t = 2 * (2 * np.sqrt(d) * delta + np.linalg.norm(Xc, axis=1) * dA) + own
    lim_r = 2 * (d * delta + np.sqrt(d) * dA) + own
    assert np.all(np.abs(cmp_dev["pose_trans_err"] - cmp_up["pose_trans_err"]) <= lim_t)
    assert np.all(np.abs(cmp_dev["pose_rot_err"] - cmp_up["pose_rot_err"]) <= lim_r)
    assert rpe_dev["max_er"] < 0.2 and cmp_dev["raw"][4] < 0.2   # a rounded noisy gauge copy is close to the truth
    for ptr in (y, out, ref, up):
        ctx.dev_free(ptr)
    ctx.set_pose_pairs(None)


def test_command_line_driver_with_device_rounding(tmp_path):
    """cora_main --device-rounding on plaza2: from the driver's random start the staircase leaves rank d (the plain run of
    tests/test_gpu_datasets.py does), so the rounding step runs and prints its line; the final cost is the recorded one."""
    import re
    import subprocess
    from cora_amd import build as _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = _build.build()
    exe = str(tmp_path / "cora_main")
    subprocess.run([_build.HIPCC, "-O1", "-std=c++17", "-I" + os.path.join(root, "include"),
                    "-I" + os.path.join(root, "cora_amd", "csrc", "host"), os.path.join(root, "examples", "main.cpp"),
                    "-L" + os.path.dirname(lib), "-lcora_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe],
                   check=True, timeout=600)
    r = subprocess.run([exe, os.path.join(DATA, "plaza2.pyfg"), "--device-rounding"], stdout=subprocess.PIPE, text=True,
                       timeout=300, check=True)
    m = re.search(r"final cost ([0-9.eE+-]+)", r.stdout)
    assert m, r.stdout[-2000:]
    assert abs(float(m.group(1)) - 734.328) < 2e-3
    assert "Projecting solution to rank" in r.stdout and "(device rounding)" in r.stdout, r.stdout[-2000:]
    bad = subprocess.run([exe, os.path.join(DATA, "plaza2.pyfg"), "--device-rounding", "--robust", "tls"], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert bad.returncode != 0 and "--device-rounding applies to the plain solve" in bad.stdout
