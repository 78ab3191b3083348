"""The landmark initialisation from ranges on the device: cora_multilaterate_dev (twice) and cora_multilaterate bit for bit
against the host mirror (cora_debug_multilaterate_host) on every case of tests/test_multilat_cpu.py and on the catalogue's
graphs that have ranges -- rows, statuses, costs, chosen points, degenerate flags --, within the bound of
tests/multilat_ref.py; the fallback directions applied afterwards; Problem.op("rangeAidedInitialization") against
Problem.op("odometryInitialization") from the same seed; the range residuals of the start on exact data; the driver's
--landmark-init."""
import os
import re
import subprocess

import numpy as np
import pytest

import multilat_ref as ml
import odom_ref as od
import residuals_ref as rr
import topologies as tp
from conftest import GOLDEN
from test_gpu_odom_init import cora_main  # noqa: F401  (the fixture that builds the driver)
from test_multilat_cpu import CATALOGUE, SYNTHETIC, case, mirror_of, reference_of

pytestmark = pytest.mark.gpu
EPS = ml.EPS
bits = ml.bits


def steps_of(name):
    if name in ("lengths", ):
        return (0, 5, 16)
    if name in ("noisy", "exact_zero"):
        return (0, 3, 16) if name == "noisy" else (0, 16)
    return (0,) if name in ("no_landmark", "no_range") else (3,) if name in ("masks", "many") else (5,)


def same(a, b):
    for key in ("status", "chosen", "degenerate"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("cost_linear", "cost_final"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    for key in ("solved", "not_solved", "n_degenerate", "steps"):
        assert a[key] == b[key], key


def run_all_forms(name, d, gn):
    ctx, dims, table, X, kw, _ = case(name, d, device=0)
    dd = dims[0]
    mirror, ref = mirror_of(name, d, gn), reference_of(name, d, gn)
    assert ctx.multilateration_counts() == ref["counts"]
    got = ctx.multilaterate(X, gn)
    assert np.array_equal(bits(got["X"]), bits(mirror["X"]))
    same(got, mirror)
    worst = ml.check(got, *dims, table, ref)
    # the resident form, twice: the same bits
    x = ctx.dev_alloc(dd)
    try:
        for _ in range(2):
            ctx.upload(X, x)
            res = ctx.multilaterate_dev(x, gn)
            assert np.array_equal(bits(ctx.download(x, dd)), bits(mirror["X"]))
            same(res, mirror)
        # the rare path: directions for the degenerate rows, afterwards
        idx = np.flatnonzero(mirror["degenerate"])
        if len(idx):
            dirs = np.random.default_rng(1).uniform(-1, 1, (len(idx), dd))
            ctx.odometry_set_range_rows_dev(idx, dirs, x)
            Xd = ctx.download(x, dd)
            rows = table[2][idx, 0]
            assert np.abs(Xd[rows] - dirs / np.linalg.norm(dirs, axis=1)[:, None]).max() <= 4 * EPS
            Xd[rows] = 0.0
            assert np.array_equal(bits(Xd), bits(mirror["X"]))
    finally:
        ctx.dev_free(x)
    return worst


@pytest.mark.parametrize("name,d,gn", [(name, d, gn) for name, d in SYNTHETIC for gn in steps_of(name)])
def test_device_on_the_synthetic_cases(name, d, gn):
    worst = run_all_forms(name, d, gn)
    print("%s d=%d gn=%d: worst error / (eps kappa scale) %.3f" % (name, d, gn, worst))


@pytest.mark.parametrize("name", CATALOGUE)
def test_device_on_the_catalogue(name):
    worst = run_all_forms(name, None, 5)
    print("%s: worst error / (eps kappa scale) %.3f" % (name, worst))


def test_device_refusals():
    """The device forms refuse what the mirror refuses, and report a sum that is not finite through the flag word."""
    from cora_amd import capi
    from test_multilat_cpu import ERR_ARG, ERR_NAN, ERR_NOT_READY, ERR_SHAPE, lonely
    (dims, table, X), _, _ = lonely(3)
    ctx = capi.Context(*dims, *ml.diagonal_q(*dims), device=0)
    x = ctx.dev_alloc(3)
    try:
        def code(fn, *a):
            with pytest.raises(capi.CoraError) as e:
                fn(*a)
            return e.value.code
        assert code(ctx.multilaterate_dev, x, 1) == ERR_NOT_READY      # no measurement table
        ctx.set_measurements(*table)
        assert code(ctx.multilaterate, X, 1) == ERR_NOT_READY          # no multilateration tables
        ctx.set_multilateration()
        assert code(ctx.multilaterate_dev, x, 17) == ERR_ARG and code(ctx.multilaterate_dev, x, -1) == ERR_ARG
        assert code(ctx.multilaterate_dev, 0, 1) == ERR_ARG            # a null vector
        out = (capi.C.c_int64 * 4)()
        Xf = np.asfortranarray(X)
        assert ctx.L.cora_multilaterate(ctx.h, capi._d(Xf), ctx.N - 1, 1, out, None, None, None, None, None) == ERR_SHAPE
        assert ctx.L.cora_multilaterate(ctx.h, capi._d(Xf), ctx.N, 1, out, None, None, None, None, None) == 0 and out[0] == 2
        rd = table[3].copy()
        rd[0, 0] = 1e200   # r^2 overflows
        ctx.set_measurements(table[0], table[1], table[2], rd)
        assert ctx.multilateration_counts() == (0, 0, 0, 0)            # the lists went with the table
        ctx.set_multilateration()
        ctx.upload(X, x)
        assert code(ctx.multilaterate_dev, x, 1) == ERR_NAN
    finally:
        ctx.dev_free(x)


@pytest.mark.parametrize("name", ("robots-d2", "robots-d3", "hub-d2", "lm_lm", "singletons", "pp_only", "n1"))
def test_problem_start_against_the_odometry_start(name):
    """From the same seed: the pose rows and the rows of the landmarks that are not solved have
    odometryInitialization's bits (the same draws in the same order, the same lift); the solved landmarks are those of
    the reference run on that start brought back to d columns.  Bound: the reference's, C a + b, plus the two lifts -- the
    start is known through x Q and (x Q) Q^T, each (d + 2) eps |x| per entry, which moves an anchor by 2 (d + 2) eps |t|
    and the solution by kappa times that, and the landmark's own row by the same once more."""
    A, _, dm, g = tp.build(name)
    d, n, r, nt, p = dm.d, dm.n, dm.r, dm.n_trans, 5
    P = tp.to_problem(name, rank=p)
    old = P.op("odometryInitialization")
    new, info = P.range_aided_initialization(seed=7, gn_steps=5)
    assert np.array_equal(bits(P.op("rangeAidedInitialization")), bits(new))
    assert old.shape == new.shape == (dm.N, p)
    t0 = d * n + r
    table, chains = rr.table(g), od.chains_of(g)
    keep = np.ones(dm.N, dtype=bool)
    keep[d * n:t0] = False
    keep[t0 + n:] = info["status"] != 0
    assert np.array_equal(bits(new[keep]), bits(old[keep]))
    # on the manifold (the binding ran checkVariablesAreValid): orthonormal pose blocks, unit range rows
    for i in range(n):
        B = new[d * i:d * i + d]
        assert np.abs(B @ B.T - np.eye(d)).max() < 1e-12
    if r:
        assert np.abs(np.linalg.norm(new[d * n:t0], axis=1) - 1).max() < 1e-12
    first = table[0][chains[0][0], 0] if chains else 0
    Qd = old[first:first + d]
    assert np.abs(Qd @ Qd.T - np.eye(d)).max() < 1e-14
    x_old, x_new = old @ Qd.T, new @ Qd.T
    pose_ok = np.zeros(n, dtype=bool)
    for ch in chains:
        pose_ok[table[0][ch[0], 0] // d] = True
        pose_ok[table[0][ch, 1] // d] = True
    ref = ml.reference(d, n, r, nt, table, x_old, 5, pose_ok=pose_ok)
    assert np.array_equal(info["status"], ref["status"])
    assert info["solved"] == int((ref["status"] == 0).sum()) and info["not_solved"] == nt - n - info["solved"]
    scale = np.abs(x_old[t0:t0 + n]).max() if n else 0.0
    worst = 0.0
    for l in np.flatnonzero(ref["status"] == 0):
        one = ref["lm"][l]
        a, b = ref["bound"][l]
        lift = 2 * (d + 2) * EPS * (scale * (1 + max(one["kappa_lin"], one["kappa_gn"])) + np.abs(x_new[t0 + n + l]).max())
        # (a point whose cost ties with the least within rounding may be taken instead: the nearest visited point)
        origin = ref["X"][t0 + n + l] - one["y"]
        err = min(float(np.sqrt(np.sum((x_new[t0 + n + l] - (origin + v)) ** 2))) for v in one["visited"])
        assert err <= ml.C_BOUND * a + b + lift, (l, err, ml.C_BOUND * a + b + lift)
        worst = max(worst, err / (ml.C_BOUND * a + b + lift))
    print("%s: %d of %d landmarks solved, largest error / bound %.3f" % (name, info["solved"], nt - n, worst))


def exact_problem(d, seed):
    """40 poses on a random walk with exact odometry, 4 landmarks with 9 exact ranges each (both orders), 6 pose-pose ranges."""
    from cora_amd import capi, host
    from synth import _rot
    rng = np.random.default_rng(seed)
    n, nl = 40, 4
    R, T = [np.eye(d)], [np.zeros(d)]
    for i in range(1, n):
        R.append(R[-1] @ _rot(d, rng, 0.2))
        T.append(T[-1] + R[-2] @ (np.eye(d)[0] + rng.normal(0, 0.3, d)))
    L = [T[rng.integers(0, n)] + 8 * rng.uniform(-1, 1, d) for _ in range(nl)]
    P = host.Problem.new(d, rank=5, precond=capi.PRECOND_JACOBI)
    for i in range(n):
        P.add_pose("A%d" % i)
    for l in range(nl):
        P.add_landmark("L%d" % l)
    cov = np.diag([0.05 ** 2] * d + [0.01 ** 2] * (3 if d == 3 else 1))
    for i in range(n - 1):
        P.add_rel_pose("A%d" % i, "A%d" % (i + 1), R[i].T @ R[i + 1], R[i].T @ (T[i + 1] - T[i]), cov)
    wr2 = 0.0
    for l in range(nl):
        for k, i in enumerate(rng.choice(n, size=9, replace=False)):
            dist = float(np.linalg.norm(T[i] - L[l]))
            a, b = ("A%d" % i, "L%d" % l) if k % 2 else ("L%d" % l, "A%d" % i)
            P.add_range(a, b, dist, 0.01)
            wr2 += dist ** 2 / 0.01
    for k in range(6):
        i, j = 3 * k, 3 * k + 17
        dist = float(np.linalg.norm(T[i] - T[j]))
        P.add_range("A%d" % i, "A%d" % j, dist, 0.01)
        wr2 += dist ** 2 / 0.01
    P.update()
    return P, wr2, nl


@pytest.mark.parametrize("d", (2, 3))
def test_range_residuals_of_the_start_on_exact_data(d):
    """Exact odometry and exact ranges: the new start's range residual sum is <= 1e-18 sum omega r^2; the old start's, with
    its random landmarks, is not."""
    P, wr2, nl = exact_problem(d, 90 + d)
    new, info = P.range_aided_initialization(seed=7, gn_steps=5)
    assert info["solved"] == nl and info["not_solved"] == 0
    got = P.measurement_residuals(new)["range_sum"]
    old = P.measurement_residuals(P.op("odometryInitialization"))["range_sum"]
    print("d = %d: range residual sum / sum omega r^2: new start %.3e, old start %.3e" % (d, got / wr2, old / wr2))
    assert got <= 1e-18 * wr2
    assert not old <= 1e-18 * wr2


def test_driver_landmark_init(cora_main):  # noqa: F811
    """cora_main --odom-init --device-init --landmark-init prints its line; without --device-init it is refused."""
    data = os.path.join(GOLDEN, "datasets", "plaza2.pyfg")
    r = subprocess.run([cora_main, data, "--odom-init", "--device-init", "--landmark-init", "--gn-steps", "3"], stdout=subprocess.PIPE,
                       text=True, timeout=300, check=True)
    m = re.search(r"landmark init: (\d+) landmarks solved, (\d+) not solved \((\d+) Gauss-Newton steps\); range residual sum at the "
                  r"start ([0-9.eE+-]+) with it, ([0-9.eE+-]+) without", r.stdout)
    assert m, r.stdout[-2000:]
    print(m.group(0))
    assert int(m.group(1)) + int(m.group(2)) > 0 and int(m.group(3)) <= 3 * int(m.group(1))
    assert float(m.group(4)) < float(m.group(5))
    assert re.search(r"final cost ([0-9.eE+-]+)", r.stdout)
    r = subprocess.run([cora_main, data, "--odom-init", "--landmark-init"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "--device-init" in r.stderr
