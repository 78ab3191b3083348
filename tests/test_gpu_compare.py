"""The trajectory comparison on the device (k_compare_sums / k_compare_centre / k_compare_errors and the Gram kernel behind
cora_compare*) against the longdouble reference of tests/compare_ref.py within that file's rounding bounds, against the
host form, what the call must leave alone, and end to end: the error of a solve and of a robust solve against ground
truth."""
import os

import numpy as np
import pytest

import compare_ref as cr
import topologies as tp
from conftest import GOLDEN
from cora_amd import capi, host
from mmio import read_dense
from oracle import assemble as asm
from oracle import oracle as orc
from synth import ground_truth, make_graph

pytestmark = pytest.mark.gpu
ERR_ARG = 5

_BUILT = {}


def built(d, n, landmarks=3):
    """(ctx, (d, n, r, nt), ground truth) of a graph of make_graph at its default seed, once per process."""
    key = (d, n, landmarks)
    if key not in _BUILT:
        g = make_graph(d=d, n=n, n_landmarks=landmarks, n_ranges=min(20, n * landmarks), n_loops=0)
        A = asm.assemble(g)
        Q = orc.CSR.from_scipy(A["Q"])
        dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
        _BUILT[key] = (capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val), (dm.d, dm.n, dm.r, dm.n_trans),
                       ground_truth(g))
    return _BUILT[key]


def catalogue(name):
    key = ("tp", name)
    if key not in _BUILT:
        A, Q, dm, g = tp.build(name)
        _BUILT[key] = (capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val), (dm.d, dm.n, dm.r, dm.n_trans),
                       A["truth"], g)
    return _BUILT[key]


def ranks(d):
    return ((d, d), (d + 1, d), (5, 5), (24, d), (24, 24))


OUTPUTS = ("raw", "pose_trans_err", "pose_rot_err", "landmark_err")


def against_host_form(ctx, dev, X, Ref, dims, select=None, proper=False, what=""):
    """The host form does not mirror the lane order: its sums, its H and its A have other last bits.  Every bound here is
    fixed by the inputs (include/cora_hip.h): each form's A is within dA = cr.alignment_bound of the exact polar factor
    (the cases are well conditioned and need no determinant correction: D = I), so the two differ by at most 2 dA and
    each is within dA + 64 k eps of the reference's A; each form's means are within cr.mean_bound; and an entry of the
    two differs by at most twice the per-entry bound plus what 2 dA and the means' difference can move it."""
    d, n, r, nt = dims
    k = X.shape[1]
    ref = ctx.debug_compare_host(X, Ref, select=select, proper=proper)
    sel = cr.selection(select, nt)
    xbar, gbar, xc, gc, H = cr.centred(X, Ref, d, n, r, nt, select)
    A_exact, s, D = cr.kabsch(H, proper)
    assert np.all(D == 1.0) and s[-1] / s[0] >= 1e-4, what
    dA = cr.alignment_bound(xc, gc, k)
    between = np.linalg.norm(dev["A"] - ref["A"])
    print("%s: device and host form: |A_dev - A_host|_F = %.3e, bound %.3e; per-entry errors bit-equal: %s" % (
        what, between, 2 * dA, all(np.array_equal(dev[key], ref[key]) for key in OUTPUTS[1:])))
    assert between <= 2 * dA, (what, between, 2 * dA)
    for form in (dev, ref):
        assert np.linalg.norm(form["A"] - A_exact) <= dA + 64 * k * cr.EPS, what
    bx, bg = cr.mean_bound(X, Ref, d, n, r, nt, select)
    assert np.all(np.abs(dev["xbar"] - ref["xbar"]) <= 2 * bx) and np.all(np.abs(dev["gbar"] - ref["gbar"]) <= 2 * bg), what
    dm = 2 * (np.linalg.norm(bx) + np.linalg.norm(bg))
    b = 2 * cr.entry_bound(X, Ref, d, n, r, nt, np.asarray(xbar, dtype=np.float64), np.asarray(gbar, dtype=np.float64))
    move = np.linalg.norm(X[cr.rows(d, n, r, nt)[2]] - np.asarray(xbar, dtype=np.float64), axis=1) * 2 * dA + dm
    assert np.all(np.abs(dev["pose_trans_err"] - ref["pose_trans_err"]) <= (b + move)[:n] * sel[:n]), what
    assert np.all(np.abs(dev["landmark_err"] - ref["landmark_err"]) <= (b + move)[n:] * sel[n:]), what
    assert np.all(np.abs(dev["pose_rot_err"] - ref["pose_rot_err"]) <= (b[:n] + np.sqrt(d) * 2 * dA) * sel[:n]), what


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", [30, 64, 65, 300])
def test_gauge_copy_and_noisy_estimate(d, n):
    ctx, dims, truth = built(d, n)
    rng = np.random.default_rng(100 * d + n)
    for k, kr in ranks(d):
        Ref = cr.reference_of_rank(truth, *dims, kr, rng)
        X, B, c = cr.gauge_copy(Ref, *dims, k, rng)
        what = "d=%d n=%d k=%d kr=%d" % (d, n, k, kr)
        res = ctx.compare(X, Ref)
        _, _, xc, gc, _ = cr.centred(X, Ref, *dims)
        cr.check_gauge(res, B, c, Ref, *dims, xc, gc, what=what + " gauge")
        Xn = X + 1e-2 * rng.standard_normal(X.shape)
        res = ctx.compare(Xn, Ref, aligned=True)
        assert res["sigma"][-1] / res["sigma"][0] >= 1e-4
        cr.check_noisy(res, ctx.debug_compare_H(k, kr), Xn, Ref, *dims, what=what + " noisy")
        cr.check_aligned(res["aligned"], res, Xn, Ref, *dims, Xn.shape[0], what=what)
        against_host_form(ctx, res, Xn, Ref, dims, what=what)


@pytest.mark.parametrize("d", [2, 3])
def test_no_landmarks_priors_and_several_robots(d):
    rng = np.random.default_rng(20 + d)
    ctx, dims, truth = built(d, 64, landmarks=0)
    assert dims[3] == dims[1] and dims[2] == 0
    Xn = cr.gauge_copy(truth, *dims, d + 1, rng)[0] + 1e-2 * rng.standard_normal((len(truth), d + 1))
    res = ctx.compare(Xn, truth)
    cr.check_noisy(res, ctx.debug_compare_H(d + 1, d), Xn, truth, *dims, what="d=%d no landmarks" % d)
    assert len(res["landmark_err"]) == 0 and res["n_landmarks"] == 0 and res["sum_el2"] == 0.0 and res["max_el"] == 0.0
    # several robots (201 poses in four chain slices, a long landmark row)
    ctx, dims, truth, g = catalogue("robots-d%d" % d)
    for k, proper in ((d, True), (5, False)):
        Xn = cr.gauge_copy(truth, *dims, k, rng)[0] + 1e-2 * rng.standard_normal((len(truth), k))
        res = ctx.compare(Xn, truth, proper=proper)
        cr.check_noisy(res, ctx.debug_compare_H(k, d), Xn, truth, *dims, proper=proper, what="robots-d%d k=%d" % (d, k))
        against_host_form(ctx, res, Xn, truth, dims, proper=proper, what="robots-d%d k=%d" % (d, k))
    if d == 2:  # a graph with priors: the origin pose is not part of the trajectory
        ctx, dims, truth, g = catalogue("rplm_priors")
        assert g.has_priors
        sel = np.ones(dims[3], dtype=np.uint8)
        sel[g.poses["O0"]] = 0
        Xn = cr.gauge_copy(truth, *dims, 3, rng)[0] + 1e-2 * rng.standard_normal((len(truth), 3))
        res = ctx.compare(Xn, truth, select=sel)
        cr.check_noisy(res, ctx.debug_compare_H(3, 2), Xn, truth, *dims, select=sel, what="rplm_priors")
        assert res["m"] == dims[1] - 1 and res["pose_trans_err"][g.poses["O0"]] == 0.0


@pytest.mark.parametrize("d", [2, 3])
def test_reflection(d):
    ctx, dims, truth = built(d, 65)
    rng = np.random.default_rng(30 + d)
    M, Bm, cm = cr.gauge_copy(truth, *dims, d, rng, mirror=True)
    free = ctx.compare(M, truth)
    assert np.linalg.det(free["A"]) < 0
    _, _, xc, gc, H = cr.centred(M, truth, *dims)
    cr.check_gauge(free, Bm, cm, truth, *dims, xc, gc, what="d=%d mirrored" % d)
    prop = ctx.compare(M, truth, proper=True)
    assert abs(np.linalg.det(prop["A"]) - 1.0) <= 64 * d * cr.EPS
    opt = cr.optimum(xc, gc, H, True)[0]
    print("d=%d: sum et^2 with a proper rotation %.17g, reference %.17g" % (d, prop["sum_et2"], opt))
    assert opt > 1.0 and abs(prop["sum_et2"] - opt) <= 1e-12 * opt
    cr.check_entries(prop, M, truth, *dims, what="d=%d mirrored, proper" % d)
    cr.check_statistics(prop)
    # the corrected alignment itself, device and host form, against the reference's.  With D = diag(1, .., 1, -1) the
    # last pair of singular vectors enters A one by one, and a singular vector moves by |dH| over its gap to the nearest
    # other singular value: 4 |tol|_F / (sigma_{d-1} - sigma_d) + 64 k eps, the polar-factor bound with the gap in the
    # place of sigma_min.
    A_ref, s, D = cr.kabsch(H, True)
    assert D[-1] == -1.0
    bound = 4 * np.linalg.norm(cr.h_tolerance(xc, gc)) / (s[-2] - s[-1]) + 64 * d * cr.EPS
    for form in (prop, ctx.debug_compare_host(M, truth, proper=True)):
        assert np.linalg.norm(form["A"] - A_ref) <= bound, (np.linalg.norm(form["A"] - A_ref), bound)


@pytest.mark.parametrize("d", [2, 3])
def test_selection(d):
    ctx, dims, truth = built(d, 300)
    _, n, r, nt = dims
    rng = np.random.default_rng(40 + d)
    masks = [rng.uniform(size=nt) < 0.5, np.arange(nt) >= 64, np.arange(nt) % 7 == 3]
    masks[0][n:] = [True, False, True]
    masks[1][n:] = False  # nothing in the first 64 poses, no landmark
    for j, sel in enumerate(masks):
        sel = sel.astype(np.uint8)
        k = (d, d + 1, 5)[j]
        Xn = cr.gauge_copy(truth, *dims, k, rng)[0] + 1e-2 * rng.standard_normal((len(truth), k))
        res = ctx.compare(Xn, truth, select=sel)
        cr.check_noisy(res, ctx.debug_compare_H(k, d), Xn, truth, *dims, select=sel, what="d=%d mask %d" % (d, j))
        Xo = Xn.copy()
        off = np.flatnonzero(sel == 0)
        Xo[cr.rows(*dims)[2][off]] = 1e6
        Xo[cr.rows(*dims)[0][off[off < n]].ravel()] = 1e6
        again = ctx.compare(Xo, truth, select=sel)
        for key in OUTPUTS:
            assert np.array_equal(res[key], again[key]), (j, key)
        assert np.all(res["pose_trans_err"][sel[:n] == 0] == 0.0) and np.all(res["pose_rot_err"][sel[:n] == 0] == 0.0)
        assert np.all(res["landmark_err"][sel[n:] == 0] == 0.0)
    with pytest.raises(capi.CoraError) as e:
        ctx.compare(Xn, truth, select=np.arange(nt) >= n)  # landmarks only
    assert e.value.code == ERR_ARG


@pytest.mark.parametrize("d", [2, 3])
def test_degenerate_cases(d):
    rng = np.random.default_rng(50 + d)
    for n in (1, 2):
        ctx, dims, truth = built(d, n)
        for k in (d, 5, 24):
            X = cr.gauge_copy(truth, *dims, k, rng)[0]
            cr.check_degenerate(ctx.compare(X, truth, proper=(k == d), aligned=True), k, "n = %d k = %d" % (n, k))
    if d == 3:
        ctx, dims, truth = built(3, 65)
        line = truth.copy()
        line[cr.rows(*dims)[2]] = np.outer(np.arange(dims[3], dtype=float), [1.0, 2.0, -0.5])
        for k in (3, 4):
            X = cr.gauge_copy(line, *dims, k, rng)[0]
            cr.check_degenerate(ctx.compare(X, line, proper=(k == 3)), k, "straight line k = %d" % k)


@pytest.mark.parametrize("d", [2, 3])
def test_aligned_vector_on_the_device(d):
    import torch
    ctx, dims, truth = built(d, 65)
    N = len(truth)
    rows = int(ctx.L.cora_rows(ctx.h))
    rng = np.random.default_rng(60 + d)
    for k, kr in ((d, d), (5, d), (5, 5), (3, 1)):
        Ref = cr.reference_of_rank(truth, *dims, kr, rng) if kr >= d else truth[:, :1].copy()
        Xn = cr.gauge_copy(Ref, *dims, k, rng)[0] + 1e-2 * rng.standard_normal((N, k))
        x, ref = ctx.dev_alloc(k), ctx.dev_alloc(kr)
        ctx.upload(Xn, x)
        ctx.upload(Ref, ref)
        ld = max(kr, 2)
        al = torch.full((rows * ld,), 7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        res = ctx.compare_dev(x, k, ref, kr, d_aligned=al.data_ptr())
        plain = ctx.compare_dev(x, k, ref, kr)
        for key in OUTPUTS:
            assert np.array_equal(res[key], plain[key]), key  # the errors do not depend on the optional output
        cr.check_entries(res, Xn, Ref, *dims, what="d=%d k=%d kr=%d" % (d, k, kr))
        cr.check_aligned(ctx.download(al.data_ptr(), kr), res, Xn, Ref, *dims, N, what="aligned d=%d k=%d kr=%d" % (d, k, kr))
        whole = al.cpu().numpy().reshape(rows, ld)
        assert not np.any(whole == 7.0)  # every row and the padding column were written
        assert np.sum(~whole.any(axis=1)) >= rows - N  # the padding rows are zero
        if kr == 1:
            assert np.all(whole[:, 1] == 0.0)
        for alias in (x, ref):
            with pytest.raises(capi.CoraError) as e:
                ctx.compare_dev(x, k, ref, kr, d_aligned=alias)
            assert e.value.code == ERR_ARG
        ctx.dev_free(x)
        ctx.dev_free(ref)


@pytest.mark.parametrize("d", [2, 3])
def test_reproducible_and_the_handle_untouched(d):
    g = make_graph(d=d, n=70, n_landmarks=3, n_ranges=100, n_loops=10)
    A = asm.assemble(g)
    Q = orc.CSR.from_scipy(A["Q"])
    dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
    ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val)
    dims, truth = (dm.d, dm.n, dm.r, dm.n_trans), ground_truth(g)
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
    for k, kr in ranks(d):
        Ref = cr.reference_of_rank(truth, *dims, kr, rng)
        Xn = cr.gauge_copy(Ref, *dims, k, rng)[0] + 1e-2 * rng.standard_normal((dm.N, k))
        a = ctx.compare(Xn, Ref, proper=(k == kr), aligned=True)
        b = ctx.compare(Xn, Ref, proper=(k == kr), aligned=True)
        for key in OUTPUTS + ("aligned",):
            assert np.array_equal(a[key], b[key]), (k, kr, key)
    # the current point itself as the estimate, on the device
    ref = ctx.dev_alloc(d)
    ctx.upload(truth, ref)
    a = ctx.compare_dev(y, p, ref, d)
    b = ctx.compare_dev(y, p, ref, d)
    assert all(np.array_equal(a[key], b[key]) for key in OUTPUTS)
    after = state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    for ptr in (y, v, o1, o2, ref):
        ctx.dev_free(ptr)
    ctx.close()


def test_solve_returns_to_the_ground_truth_of_the_noise_free_fixture():
    case = os.path.join(GOLDEN, "small_ra_slam_problem")
    path = os.path.join(case, "factor_graph.pyfg")
    P = host.Problem.from_pyfg(path)
    P.update()
    res = P.solve(read_dense(os.path.join(case, "X_gt.mm")))
    cmp = P.compare(res["x"], P.ground_truth(path))
    print("small_ra_slam_problem: translation RMSE %.3e, rotation RMSE %.3e, landmark RMSE %.3e" % (
        cmp["trans_rmse"], cmp["rot_rmse"], cmp["landmark_rmse"]))
    assert cmp["m"] == P.dims()["n"] and cmp["trans_rmse"] <= 1e-5
    # the implicit formulation: the variable has no translation rows, the comparison completes it first
    Pi = host.Problem.from_pyfg(path)
    Pi.update()
    Pi.set_formulation(True)
    truth = Pi.ground_truth(path)
    assert truth.shape[0] == Pi.dims()["N"] > Pi.variable_size()
    res = Pi.solve(np.asfortranarray(truth[:Pi.variable_size()]))
    assert res["x"].shape[0] == Pi.variable_size()
    cmp = Pi.compare(res["x"], truth, aligned=True)
    print("implicit: translation RMSE %.3e, rotation RMSE %.3e" % (cmp["trans_rmse"], cmp["rot_rmse"]))
    assert cmp["trans_rmse"] <= 1e-5
    dm = Pi.dims()
    t = dm["d"] * dm["n"] + dm["r"] + np.arange(dm["n"])
    # (a position's distance from the truth in the aligned estimate IS its translation error)
    assert np.abs(np.linalg.norm(cmp["aligned"][t] - truth[t], axis=1) - cmp["pose_trans_err"]).max() <= 1e-12


# ---- the robust case of tests/test_gpu_gnc.py, judged by its distance from the truth ----------------------------------
BAD = (3, 11, 19, 27, 42, 55)
SHIFT, BARC2 = 10.0, 25.0


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


@pytest.mark.parametrize("d", [2, 3])
def test_robust_solve_is_closer_to_the_truth(d):
    g = make_graph(d=d, n=30, n_landmarks=3, n_ranges=60, n_loops=5)
    for i in BAD:
        a, b, r, cov = g.ranges[i]
        g.ranges[i] = (a, b, r + SHIFT, cov)
    truth = ground_truth(g)
    plain_problem = _problem(g)
    plain = plain_problem.compare(plain_problem.solve(truth, max_rank=10)["x"], truth)
    P = _problem(g)
    res = P.solve_robust(truth, {"range": np.full(len(g.ranges), BARC2)}, cost="tls")
    robust = P.compare(res["x"], truth)
    print("d=%d: translation RMSE of the plain solve %.6g, of the robust solve %.6g (landmarks %.6g -> %.6g)" % (
        d, plain["trans_rmse"], robust["trans_rmse"], plain["landmark_rmse"], robust["landmark_rmse"]))
    assert res["converged"] and robust["trans_rmse"] < plain["trans_rmse"]


# ---- the command-line driver ------------------------------------------------------------------------------------------
def _evaluate_lines(text):
    """{'all' | robot character | 'landmarks': (count, translation RMSE, max, rotation RMSE in degrees, max)} of the
    driver's 'evaluate:' lines."""
    import re
    out = {}
    for line in text.splitlines():
        m = re.match(r"evaluate: (?:robot '(.)' )?(\d+) poses  translation RMSE (\S+) max (\S+)  rotation RMSE (\S+) deg max (\S+) deg$", line)
        if m:
            out[m.group(1) or "all"] = (int(m.group(2)),) + tuple(float(v) for v in m.groups()[2:])
        m = re.match(r"evaluate: (\d+) landmarks  position RMSE (\S+) max (\S+)$", line)
        if m:
            out["landmarks"] = (int(m.group(1)), float(m.group(2)), float(m.group(3)))
    return out


def _pose_symbols(path):
    return [line.split()[2] for line in open(path) if line.startswith(("VERTEX_SE2 ", "VERTEX_SE3:QUAT "))]


def test_command_line_driver_evaluates_against_the_files_own_vertices(tmp_path):
    import subprocess
    from cora_amd import build as _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = _build.build()
    exe = str(tmp_path / "cora_main")
    subprocess.run([_build.HIPCC, "-O1", "-std=c++17", "-I" + os.path.join(root, "include"),
                    "-I" + os.path.join(root, "cora_amd", "csrc", "host"), os.path.join(root, "examples", "main.cpp"),
                    "-L" + os.path.dirname(lib), "-lcora_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe],
                   check=True, timeout=600)
    REL = 2e-5  # the lines print six significant digits

    def run(name, *flags):
        r = subprocess.run([exe, os.path.join(GOLDEN, "datasets", name + ".pyfg"), "--evaluate"] + list(flags),
                           stdout=subprocess.PIPE, text=True, timeout=300, check=True)
        return r.stdout, _evaluate_lines(r.stdout)

    # several robots: a line each, from the per-pose errors under the joint alignment
    path = os.path.join(GOLDEN, "datasets", "mrclam6.pyfg")
    symbols = _pose_symbols(path)
    text, ev = run("mrclam6")
    robots = sorted(set(s[0] for s in symbols))
    assert len(robots) > 1 and sorted(k for k in ev if k not in ("all", "landmarks")) == robots, text[-2000:]
    for c in robots:
        assert ev[c][0] == sum(s[0] == c for s in symbols)  # the poses of that symbol character
    n_all, t_all, tmax_all, a_all, amax_all = ev["all"]
    assert n_all == len(symbols) == sum(ev[c][0] for c in robots)
    for col, whole in ((1, t_all), (3, a_all)):  # an RMSE over all poses is the count-weighted one of the robots'
        assert abs(np.sqrt(sum(ev[c][0] * ev[c][col] ** 2 for c in robots) / n_all) - whole) <= REL * whole
    assert max(ev[c][2] for c in robots) == tmax_all and max(ev[c][4] for c in robots) == amax_all
    assert all(ev[c][1] <= ev[c][2] and ev[c][3] <= ev[c][4] for c in robots + ["all"])
    assert ev["landmarks"][0] == sum(line.startswith(("VERTEX_XY ", "VERTEX_XYZ ")) for line in open(path))
    # one robot: no robot line; the aligned trajectory's distance from the file's own positions IS the translation error
    path = os.path.join(GOLDEN, "datasets", "plaza2.pyfg")
    tum = str(tmp_path / "aligned.tum")
    text, ev = run("plaza2", "--aligned-tum", tum)
    assert sorted(ev) == ["all", "landmarks"] and "wrote " + tum in text
    truth = np.array([[float(v) for v in line.split()[3:5]] for line in open(path) if line.startswith("VERTEX_SE2 ")])
    got = np.loadtxt(tum)
    assert got.shape == (len(truth), 8) and ev["all"][0] == len(truth)
    dist = np.linalg.norm(got[:, 1:3] - truth, axis=1)  # (plaza2 lists its poses in symbol order, the order of the file)
    assert abs(np.sqrt(np.mean(dist ** 2)) - ev["all"][1]) <= REL * ev["all"][1] and abs(dist.max() - ev["all"][2]) <= REL * ev["all"][2]
    # with the robust solve: the lines are there, and with nothing to reject they are the plain solve's to solver accuracy
    text_r, ev_r = run("plaza2", "--robust", "tls", "--barc2", "range=25")
    assert "robust solve (tls)" in text_r and sorted(ev_r) == ["all", "landmarks"] and ev_r["all"][0] == ev["all"][0]
    if ", 0 of " in text_r:
        assert abs(ev_r["all"][1] - ev["all"][1]) <= 1e-3 * ev["all"][1]
