"""The outlier-robust multilateration on the device: cora_multilaterate_robust and the resident cora_multilaterate_robust_dev
(twice on one upload) bit for bit against the host mirror on every case of tests/test_range_consensus_cpu.py, the list of 16 385
entries included -- rows, statuses, costs, chosen, elected, consensus, list lengths, inlier bytes, counts --; the device error
paths; Problem.range_aided_initialization with a consensus vote on a hub whose landmarks have a quarter of their ranges
lengthened (the flags are the construction's, and the start is better than the plain one's); without the vote it has the plain
call's bits; the operator form; the driver's --range-consensus."""
import re
import subprocess

import numpy as np
import pytest

import multilat_ref as ml
from test_gpu_odom_init import cora_main  # noqa: F401  (the fixture that builds the driver)
from test_range_consensus_cpu import BARC2, CASES, SIGMA, case, mirror_of, nan_case, robust_refusals, vote_of

pytestmark = pytest.mark.gpu
bits = ml.bits


def same(a, b):
    for key in ("status", "chosen", "elected", "consensus", "list_len", "inlier", "degenerate"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("cost_linear", "cost_final"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    for key in ("solved", "not_solved", "n_degenerate", "steps", "no_consensus", "excluded"):
        assert a[key] == b[key], key


@pytest.mark.parametrize("name,d,gn", [(name, d, gn) for name, d in CASES for gn in (0, 5)] + [("long", 2, 5)])
def test_device_on_the_cases(name, d, gn):
    ctx, dims, table, X, kw, _, _ = case(name, d, device=0)
    vote = vote_of(name, d)
    mirror = mirror_of(name, d, gn)
    got = ctx.multilaterate_robust(X, BARC2, gn, **vote)
    assert np.array_equal(bits(got["X"]), bits(mirror["X"]))
    same(got, mirror)
    # the resident form, twice on the same upload: the second call starts from the first one's result
    x = ctx.dev_alloc(d)
    try:
        ctx.upload(X, x)
        res = ctx.multilaterate_robust_dev(x, BARC2, gn, **vote)
        assert np.array_equal(bits(ctx.download(x, d)), bits(mirror["X"]))
        same(res, mirror)
        again = ctx.multilaterate_robust_dev(x, BARC2, gn, **vote)
        twice = case(name, d)[0].debug_multilaterate_robust_host(mirror["X"], BARC2, gn, **vote)
        assert np.array_equal(bits(ctx.download(x, d)), bits(twice["X"]))
        same(again, twice)
        solved = again["status"] == 0
        assert np.all(again["cost_final"][solved] <= again["cost_linear"][solved])   # never worse, as doubles
    finally:
        ctx.dev_free(x)
    if name == "long":
        assert ctx.multilateration_counts()[3] == 65 and got["list_len"][0] == 16385 and got["status"][0] == 0


def test_device_refusals():
    """The device forms refuse what the mirror refuses, and report a row that is not finite through the flag word."""
    from cora_amd import capi
    from test_range_consensus_cpu import ERR_NAN, comb
    new = lambda dims: capi.Context(*dims, *ml.diagonal_q(*dims), device=0)
    robust_refusals(new, lambda ctx, X, gn, b, m: ctx.multilaterate_robust(X, b, gn, m),
                    lambda ctx: (ctx.L.cora_multilaterate_robust, lambda X, ldx: (None if X is None else capi._d(X), ldx)))
    held = []

    def resident(ctx, X, gn, b, m):
        if not held:
            held.append(ctx.dev_alloc(2))
            ctx.upload(X, held[0])
        return ctx.multilaterate_robust_dev(held[0], b, gn, m)
    ((dims, _, _), _), _, _ = comb()
    ctx = new(dims)   # (the resident vector exists before the tables do)
    try:
        # (the raw C call of the resident form: a device pointer or NULL, no leading dimension)
        robust_refusals(lambda dims: ctx, resident,
                        lambda c: (c.L.cora_multilaterate_robust_dev, lambda X, ldx: (None if X is None else capi.C.c_void_p(held[0]),)), has_ldx=False)
        with pytest.raises(capi.CoraError) as e:
            ctx.multilaterate_robust_dev(0, BARC2)      # a null vector
        assert e.value.code == 5
    finally:
        ctx.dev_free(held[0])
    dims, table, X = nan_case()
    ctx = new(dims)
    ctx.set_measurements(*table)
    ctx.set_multilateration()
    with pytest.raises(capi.CoraError) as e:
        ctx.multilaterate_robust(X, BARC2)
    assert e.value.code == ERR_NAN


_HUB = {}


def hub(d):
    """A hub of multilat_ref.graph -- 320 poses on a walk of exact odometry from the identity at the origin, 3 landmarks with 300
    ranges each, sigma = 0.05 -- with a quarter of each landmark's ranges lengthened by 5 .. 20 m, as a Problem; the same with the
    ranges as measured; the truth of the landmarks; per range 1 (as measured) | 0 (lengthened)."""
    if d in _HUB:
        return _HUB[d]
    from cora_amd import capi, host
    from synth import _rot
    rng = np.random.default_rng(700 + d)
    n, nl, k = 320, 3, 300
    R, T = [np.eye(d)], [np.zeros(d)]
    for i in range(1, n):
        R.append(R[-1] @ _rot(d, rng, 0.3))
        T.append(T[-1] + 3.0 * rng.normal(0, 1, d) / np.sqrt(d))
    lms = np.array([T[rng.integers(0, n)] + 10 * rng.uniform(-1, 1, d) for _ in range(nl)])
    ranges = [(int(p), n + l) for l in range(nl) for p in rng.choice(n, size=k, replace=False)]
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    (_, _, r, _), table, _ = ml.graph(d, np.array(T), lms, ranges, noise=SIGMA, seed=d)
    good = np.ones(r, dtype=np.uint8)
    for l in range(nl):
        mine = np.flatnonzero([b == n + l for _, b in ranges])
        good[rng.choice(mine, size=k // 4, replace=False)] = 0
    dist = table[3][:, 0].copy()
    dist[good == 0] += rng.uniform(5, 20, int(np.sum(good == 0)))
    cov = np.diag([0.05 ** 2] * d + [0.01 ** 2] * (3 if d == 3 else 1))

    def problem(dists):
        P = host.Problem.new(d, rank=5, precond=capi.PRECOND_JACOBI)
        for i in range(n):
            P.add_pose("A%d" % i)
        for l in range(nl):
            P.add_landmark("L%d" % l)
        for i in range(n - 1):
            P.add_rel_pose("A%d" % i, "A%d" % (i + 1), R[i].T @ R[i + 1], R[i].T @ (T[i + 1] - T[i]), cov)
        for m, (a, b) in enumerate(ranges):
            P.add_range("A%d" % a, "L%d" % (b - n), float(dists[m]), SIGMA ** 2)
        P.update()
        return P
    _HUB[d] = dict(P=problem(dist), clean=problem(table[3][:, 0]), lms=lms, good=good, n=n, nl=nl, R=R, T=T, ranges=ranges, dist=dist, cov=cov)
    return _HUB[d]


@pytest.mark.parametrize("d", (2, 3))
def test_contaminated_hub_start(d):
    """From the same seed the plain start fits every range of a landmark and the robust one those that agree: its flags are
    exactly the lengthened ranges, every landmark has status 0, its landmark RMSE against the truth is strictly lower, and so is
    its objective over the graph's ranges as measured."""
    h = hub(d)
    P, n, nl = h["P"], h["n"], h["nl"]
    plain, pinfo = P.range_aided_initialization(seed=7)
    robust, info = P.range_aided_initialization(seed=7, consensus_barc2=BARC2)
    assert np.array_equal(info["inlier"], h["good"]), np.flatnonzero(info["inlier"] != h["good"])[:10]
    assert list(info["status"]) == [0] * nl and info["no_consensus"] == 0 and info["excluded"] == int(np.sum(h["good"] == 0))
    assert list(info["list_len"]) == [300] * nl and list(info["consensus"]) == [225] * nl
    assert list(pinfo["status"]) == [0] * nl and "inlier" not in pinfo

    def rmse(x0):
        x = x0 @ x0[:d].T   # (the start in the frame of the first pose, which the truth is in)
        return float(np.sqrt(np.mean(np.sum((x[-nl:] - h["lms"]) ** 2, axis=1))))
    r_plain, r_robust = rmse(plain), rmse(robust)
    f_plain, f_robust = (h["clean"].op("evaluateObjective", x) for x in (plain, robust))
    print("contaminated hub d=%d: landmark RMSE %.4g plain, %.4g robust; objective over the ranges as measured %.6g plain, %.6g robust"
          % (d, r_plain, r_robust, f_plain, f_robust))
    assert r_robust < r_plain
    assert f_robust < f_plain
    # the operator form is the method with the operator's defaults
    assert np.array_equal(bits(P.op("rangeAidedInitializationConsensus")), bits(P.range_aided_initialization(seed=7, gn_steps=5, consensus_barc2=100.0)[0]))


def test_without_the_vote_the_bits_are_the_plain_calls():
    """consensus_barc2=None is the path of before: the operator form (Problem::rangeAidedInitialization with its defaults) and the
    method agree bit for bit, and the info has no field of the vote."""
    P = hub(2)["P"]
    x0, info = P.range_aided_initialization(seed=7, consensus_barc2=None)
    assert np.array_equal(bits(x0), bits(P.op("rangeAidedInitialization")))
    assert np.array_equal(bits(x0), bits(P.range_aided_initialization(seed=7)[0]))
    assert "inlier" not in info and "consensus" not in info and "no_consensus" not in info


def test_driver_range_consensus(cora_main, tmp_path):  # noqa: F811
    """cora_main --landmark-init --range-consensus on the contaminated hub (d = 2) exits 0 and prints the counts of
    test_contaminated_hub_start; without --landmark-init the flag is refused."""
    h = hub(2)
    data = str(tmp_path / "hub.pyfg")
    with open(data, "w") as f:
        for i in range(h["n"]):
            f.write("VERTEX_SE2 %d.0 A%d 0 0 0\n" % (i, i))
        for l in range(h["nl"]):
            f.write("VERTEX_XY L%d 0 0\n" % l)
        up = " ".join("%.17g" % h["cov"][r, c] for r in range(3) for c in range(r, 3))
        for i in range(h["n"] - 1):
            Rr, t = h["R"][i].T @ h["R"][i + 1], h["R"][i].T @ (h["T"][i + 1] - h["T"][i])
            f.write("EDGE_SE2 %d.0 A%d A%d %.17g %.17g %.17g %s\n" % (i, i, i + 1, t[0], t[1], np.arctan2(Rr[1, 0], Rr[0, 0]), up))
        for m, (a, b) in enumerate(h["ranges"]):
            f.write("EDGE_RANGE %d.0 A%d L%d %.17g %.17g\n" % (m, a, b - h["n"], h["dist"][m], SIGMA ** 2))
    flags = ["--odom-init", "--device-init", "--landmark-init", "--range-consensus", "%g" % BARC2]
    r = subprocess.run([cora_main, data, *flags], stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    m = re.search(r"range consensus: (\d+) landmarks without consensus, (\d+) ranges excluded; smallest consensus / list length ([0-9.]+)", r.stdout)
    assert m, r.stdout[-2000:]
    print(m.group(0))
    assert [int(m.group(1)), int(m.group(2))] == [0, 225] and float(m.group(3)) == 0.75
    r = subprocess.run([cora_main, data, "--odom-init", "--device-init", "--range-consensus", "%g" % BARC2], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "--landmark-init" in r.stderr
