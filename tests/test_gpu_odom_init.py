"""The odometry initialisation on the device: cora_odometry_init_dev / cora_odometry_init bit for bit against the host
mirror (cora_debug_odometry_init_host) on the catalogue's graphs and on the synthetic chains of
tests/test_odom_init_cpu.py (every boundary of the scan's shape, a second sweep of the middle pass), within the derived
bounds of tests/odom_ref.py, reproducible, with the reference's count and flags of degenerate rows;
Problem.op("odometryInitialization") against Problem.op("getOdomInitialization") from the same seed; the driver's
--device-init."""
import os
import re
import subprocess

import numpy as np
import pytest

import odom_ref as od
import topologies as tp
from conftest import GOLDEN
from test_odom_init_cpu import TOPOLOGIES, bits, catalogue, reference_of, synthetic

pytestmark = pytest.mark.gpu
EPS = od.EPS


def run_all_forms(ctx, dims, table, starts, lm, ref):
    d, n, r, nt = dims
    mirror = ctx.debug_odometry_init_host(starts, lm)
    got = ctx.odometry_init(starts, lm)
    assert np.array_equal(bits(got["X"]), bits(mirror["X"]))
    worst = od.check(got["X"], *dims, table, ref)
    assert got["written"] == ref["written"] == mirror["written"]
    assert got["n_degenerate"] == ref["degenerate"].sum() and np.array_equal(got["degenerate"], ref["degenerate"])
    # the resident form, twice: the same bits
    x = ctx.dev_alloc(d)
    try:
        for _ in range(2):
            res = ctx.odometry_init_dev(starts, lm, x)
            assert np.array_equal(bits(ctx.download(x, d)), bits(mirror["X"]))
            assert res["written"] == ref["written"] and np.array_equal(res["degenerate"], ref["degenerate"])
        # the rare path: directions for the degenerate rows
        idx = np.flatnonzero(ref["degenerate"])
        if len(idx):
            dirs = np.random.default_rng(1).uniform(-1, 1, (len(idx), d))
            ctx.odometry_set_range_rows_dev(idx, dirs, x)
            X = ctx.download(x, d)
            rows = table[2][idx, 0]
            assert np.abs(X[rows] - dirs / np.linalg.norm(dirs, axis=1)[:, None]).max() <= 4 * EPS
            X[rows] = 0.0
            assert np.array_equal(bits(X), bits(mirror["X"]))
    finally:
        ctx.dev_free(x)
    return worst


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_device_on_the_catalogue(name):
    ctx, dims, table, chains = catalogue(name, device=0)
    starts, lm, ref = reference_of(name, dims, table, chains)
    worst = run_all_forms(ctx, dims, table, starts, lm, ref)
    print("%s: worst error / bound: rotation %.3f translation %.3f range %.3f" % (name, *worst))


@pytest.mark.parametrize("name", ("singletons", "n1"))
def test_device_degenerate_ranges(name):
    ctx, dims, table, chains = catalogue(name, device=0)
    starts, lm, ref = reference_of(name, dims, table, chains, seed=9, landmarks=False)
    assert ref["degenerate"].any()
    run_all_forms(ctx, dims, table, starts, None, ref)


@pytest.mark.parametrize("d", (2, 3))
@pytest.mark.parametrize("kind", ("boundaries", "sweeps", "ones"))
def test_device_on_the_boundaries_of_the_scan(d, kind):
    ctx, dims, table, chains = synthetic(d, kind, device=0)
    starts, lm, ref = reference_of(("syn", d, kind), dims, table, chains)
    worst = run_all_forms(ctx, dims, table, starts, lm, ref)
    print("d = %d, %s: worst error / bound: rotation %.3f translation %.3f range %.3f" % (d, kind, *worst))


@pytest.mark.parametrize("name", ("robots-d2", "robots-d3", "reversed", "singletons", "pp_only", "n1", "n128"))
def test_problem_start_against_the_host_function(name):
    """From the same seed the device start is the host function's up to rounding: both are within the bounds of the exact
    composition, so they differ by at most twice the bounds, lifted through |Q|, plus (d + 2) eps |x| |Q| for the lift.
    Q (its first d rows) is read off the host's own output: the head of the first chain, or any pose no chain reaches, is
    (I, 0), and I Q is exact.  The scales come from the host's start brought back to d columns (Q Q^T = I).  On
    `singletons` the fallback directions of the degenerate rows pin the order of the draws."""
    A, _, dm, g = tp.build(name)
    d, n, r, nt, p = dm.d, dm.n, dm.r, dm.n_trans, 5
    P = tp.to_problem(name, rank=p)
    host = P.op("getOdomInitialization")
    dev = P.op("odometryInitialization")
    assert host.shape == dev.shape == (dm.N, p)
    import residuals_ref as rr
    table, chains = rr.table(g), od.chains_of(g)
    er = table[0]
    first = er[chains[0][0], 0] if chains else 0
    Qd = host[first:first + d]
    assert np.abs(Qd @ Qd.T - np.eye(d)).max() < 1e-14
    assert np.array_equal(bits(dev[first:first + d]), bits(Qd))   # the same draws in the same order
    x = host @ Qd.T
    t0 = d * n + r
    starts = np.array([x[er[ch[0], 2]] for ch in chains]).reshape(len(chains), d)
    ref = od.reference(d, n, r, nt, table, chains, starts, x[t0 + n:])
    rot_b, trn_b, rng_b = (np.asarray(b, dtype=np.float64) for b in od.row_bounds(d, n, r, nt, table, ref))
    row_b = np.zeros(dm.N)
    row_b[:d * n] = np.repeat(rot_b, d)
    row_b[t0:] = trn_b
    row_b[table[2][:, 0]] = np.where(ref["degenerate"], 4 * EPS, rng_b)
    absQ = np.abs(Qd)
    bound = 2 * row_b[:, None] * absQ.sum(axis=0)[None, :] + (d + 2) * EPS * (np.abs(x) @ absQ)
    # (the scales are known to a relative eps only, and a pose written exactly has no bound of its own)
    bound = bound * (1 + 1e-6) + (d + 2) * EPS * 1e-300
    err = np.abs(dev - host)
    worst = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)).max()
    print("%s: largest |device - host| / bound %.3f" % (name, worst))
    assert worst <= 1.0
    if name == "singletons":
        assert ref["degenerate"].sum() >= 3


@pytest.fixture(scope="module")
def cora_main(tmp_path_factory):
    from cora_amd import build as _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = _build.build()
    exe = str(tmp_path_factory.mktemp("odom") / "cora_main")
    subprocess.run([_build.HIPCC, "-O1", "-std=c++17", "-I" + os.path.join(root, "include"),
                    "-I" + os.path.join(root, "cora_amd", "csrc", "host"), os.path.join(root, "examples", "main.cpp"),
                    "-L" + os.path.dirname(lib), "-lcora_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe],
                   check=True, timeout=600)
    return exe


def test_driver_device_init(cora_main):
    """cora_main --odom-init --device-init on plaza2.pyfg ends on the cost --odom-init ends on (the tolerance of
    tests/test_gpu_datasets.py for this data set); --device-init alone is refused."""
    data = os.path.join(GOLDEN, "datasets", "plaza2.pyfg")
    cost = {}
    for flags in (("--odom-init",), ("--odom-init", "--device-init")):
        r = subprocess.run([cora_main, data, *flags], stdout=subprocess.PIPE, text=True, timeout=300, check=True)
        m = re.search(r"final cost ([0-9.eE+-]+)", r.stdout)
        assert m, r.stdout[-2000:]
        cost[flags] = float(m.group(1))
    print("plaza2 from the odometry start: host %.6f, device %.6f" % tuple(cost.values()))
    assert abs(cost[("--odom-init", "--device-init")] - cost[("--odom-init",)]) < 2e-3
    r = subprocess.run([cora_main, data, "--device-init"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "--odom-init" in r.stderr
