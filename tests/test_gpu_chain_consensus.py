"""The outlier-robust chain placement on the device: cora_place_chains_robust and the resident cora_place_chains_robust_dev
(twice on one upload) bit for bit against the host mirror on every case of tests/test_chain_consensus_cpu.py, under level and
greedy tables -- rows, statuses, costs, chosen, transforms, elected, consensus, list lengths, inlier bytes, counts --; the
device error paths; a clean hub against cora_place_chains_batched_dev bit for bit; the call behind a blocked caller's stream;
Problem.multi_robot_initialization with the vote on a fleet with a tenth of its ranges lengthened, against the reference's chain
errors; the driver's --chain-consensus; a NaN in the vector made visible through the resident form."""
import numpy as np
import pytest

import chain_consensus_ref as cc
import placement_ref as pl
from test_gpu_odom_init import cora_main  # noqa: F401  (the fixture that builds the driver)
from stream_gate import KINDS, Gate, Plain, differing, same as same_bits, stream, stream_ptr
from test_chain_consensus_cpu import BARC2, CASES, ERR_NAN, PLAIN_KEYS, ROBUST_KEYS, case, hub_lens, mirror_of, nan_case, robust_refusals, same

pytestmark = pytest.mark.gpu
bits = pl.bits
KEYS = [k for k in ROBUST_KEYS if k != "X"]


@pytest.mark.parametrize("name,d,gn,order", [(name, d, gn, cc.LEVELS) for name, d in CASES for gn in (0, 5)] +
                         [("hub", d, 5, cc.GREEDY) for d in (2, 3)])
def test_device_on_the_cases(name, d, gn, order):
    ctx, dims, table, X = case(name, d, order, device=0)[:4]
    mirror = mirror_of(name, d, gn, order)
    got = ctx.place_chains_robust(X, BARC2, gn)
    same(got, mirror, ROBUST_KEYS)
    # the resident form, twice on the same upload: the second call starts from the first one's result
    x = ctx.dev_alloc(d)
    try:
        ctx.upload(X, x)
        res = ctx.place_chains_robust_dev(x, BARC2, gn)
        assert np.array_equal(bits(ctx.download(x, d)), bits(mirror["X"]))
        same(res, mirror, KEYS)
        again = ctx.place_chains_robust_dev(x, BARC2, gn)
        twice = case(name, d, order)[0].debug_place_chains_robust_host(mirror["X"], BARC2, gn)
        assert np.array_equal(bits(ctx.download(x, d)), bits(twice["X"]))
        same(again, twice, KEYS)
        assert np.all(again["cost_final"] <= again["cost_start"])   # never worse over the inliers, as doubles
    finally:
        ctx.dev_free(x)


@pytest.mark.parametrize("d", (2, 3))
def test_min_consensus_one_on_the_device(d):
    """The lists of m and m + 1 entries fitted too: the mirror's bits."""
    ctx, dims, table, X = case("hub", d, device=0)[:4]
    same(ctx.place_chains_robust(X, BARC2, 5, 1), mirror_of("hub", d, 5, cc.LEVELS, 1), ROBUST_KEYS)


@pytest.mark.parametrize("d", (2, 3))
def test_a_clean_hub_has_the_batched_call_s_bits(d):
    """No outlier: X, costs, chosen, transforms and out[0..5] are cora_place_chains_batched_dev's on the same tables, bit for
    bit, and every inlier byte of a stage list is 1."""
    ctx, dims, table, X = case("clean_hub", d, device=0)[:4]
    xr, xb = ctx.dev_alloc(d), ctx.dev_alloc(d)
    try:
        for gn in (0, 5):
            ctx.upload(X, xr)
            ctx.upload(X, xb)
            got, plain = ctx.place_chains_robust_dev(xr, BARC2, gn, 1), ctx.place_chains_batched_dev(xb, gn)
            assert np.array_equal(bits(ctx.download(xr, d)), bits(ctx.download(xb, d)))
            same(got, plain, [k for k in PLAIN_KEYS if k != "X"] + ["levels"])
            assert got["no_consensus"] == 0 and got["excluded"] == 0 and np.all(got["inlier"] == 1)
            assert list(got["consensus"][1:]) == hub_lens(d)
    finally:
        ctx.dev_free(xr)
        ctx.dev_free(xb)


def test_device_refusals():
    """The device forms refuse what the mirror refuses, and report a row that is not finite through the flag word."""
    from cora_amd import capi
    from test_chain_consensus_cpu import exact
    new = lambda dims: capi.Context(*dims, *pl.diagonal_q(*dims), device=0)  # noqa: E731
    robust_refusals(new, lambda ctx, X, gn, b, m: ctx.place_chains_robust(X, b, gn, m),
                    lambda ctx: (ctx.L.cora_place_chains_robust, lambda X, ldx: (None if X is None else capi._d(X), ldx), True))
    held = []

    def resident(ctx, X, gn, b, m):
        if not held:
            held.append(ctx.dev_alloc(2))
            ctx.upload(X, held[0])
        return ctx.place_chains_robust_dev(held[0], b, gn, m)
    dims = exact(2)[0][0]
    ctx = new(dims)   # (the resident vector exists before the tables do)
    try:
        # (the raw C call of the resident form: a device pointer or NULL, no leading dimension)
        robust_refusals(lambda dims: ctx, resident,
                        lambda c: (c.L.cora_place_chains_robust_dev, lambda X, ldx: (None if X is None else capi.C.c_void_p(held[0]),), False))
        with pytest.raises(capi.CoraError) as e:
            ctx.place_chains_robust_dev(0, BARC2)      # a null vector
        assert e.value.code == 5
    finally:
        ctx.dev_free(held[0])
    dims, table, X, chains, kw = nan_case()
    ctx = new(dims)
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_chain_placement_order(order=cc.LEVELS, **kw)
    with pytest.raises(capi.CoraError) as e:
        ctx.place_chains_robust(X, BARC2)
    assert e.value.code == ERR_NAN


_STREAM = {}


@pytest.mark.parametrize("kind", KINDS)
def test_behind_a_blocked_stream(kind):
    """The call waits at its end; what is checked is that it waits for the caller's stream first: the operand is uploaded behind
    a gate on the caller's stream (the pattern of test_gpu_streams.py::test_evaluation_and_initialisers, with its helpers)."""
    import test_chain_consensus_cpu as m
    from test_gpu_streams import _in_place, _twin, reference
    if "made" not in _STREAM:
        shared, mine = _twin(m, ("line", 2, cc.LEVELS, 0), lambda: m.case("line", 2, device=0))
        _STREAM["made"] = (shared[0], mine[0], _in_place(shared[3], lambda c, x: c.place_chains_robust_dev(x, BARC2, 5)))
    shared, mine, run = _STREAM["made"]
    s = stream(kind)
    mine.set_stream(stream_ptr(s))
    want = reference(("eval", "place_chains_robust"), lambda: run(shared, Plain(shared)))
    got = run(mine, Gate(mine, s))
    assert same_bits(got, want), differing(got, want)
    assert np.array_equal(bits(got["X"]), bits(mirror_of("line", 2)["X"]))


# ------------------------------------------------------------------------------------------------- through Problem
_FLEET = {}
LENS = [40, 40, 40]


def fleet(d):
    """Three robots of 40 poses as a Problem: exact odometry, 300 ranges from each of B and C to A with sigma = 0.05, 10 % of them
    lengthened by +5 .. 20 m; the scene's table and chains (the Problem's, by construction: poses, edges and ranges are added in
    table order), the truth in the world frame, per range 1 (lengthened) | 0."""
    if d in _FLEET:
        return _FLEET[d]
    from cora_amd import capi, host
    from test_chain_consensus_cpu import SIGMA, _contaminate
    from test_placement_cpu import _pairs
    rng = np.random.default_rng(900 + d)
    ranges = _pairs(rng, 0, 40, 40, 40, 300) + _pairs(rng, 0, 40, 80, 40, 300)
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    dims, table, X, chains, truth = pl.scene(d, LENS, ranges, seed=300 + d, noise=SIGMA, omega=[1 / SIGMA ** 2] * len(ranges))
    bad = _contaminate(rng, table, ranges, 40)
    n, t0 = dims[1], dims[0] * dims[1] + dims[2]
    world = np.concatenate([X[t0 + 40 * c:t0 + 40 * (c + 1)] @ truth[c][0].T + truth[c][1] for c in range(3)])
    cov = np.diag([0.05 ** 2] * d + [0.01 ** 2] * (3 if d == 3 else 1))
    name = lambda i: "%s%d" % ("ABC"[i // 40], i % 40)  # noqa: E731
    P = host.Problem.new(d, rank=5, precond=capi.PRECOND_JACOBI)
    for i in range(n):
        P.add_pose(name(i))
    for row, dat in zip(table[0], table[1]):
        a, b = int(row[0]) // d, int(row[1]) // d
        P.add_rel_pose(name(a), name(b), dat[:d * d].reshape(d, d), dat[d * d:d * d + d], cov)
    for m, (a, b) in enumerate(ranges):
        P.add_range(name(a), name(b), float(table[3][m, 0]), SIGMA ** 2)
    P.update()
    _FLEET[d] = dict(P=P, dims=dims, table=table, chains=chains, world=world, bad=bad, ranges=ranges, cov=cov, name=name)
    return _FLEET[d]


def chain_errors(x, world, t0):
    """Per chain B, C: the largest | |x_i - x_j| - |w_i - w_j| | over its poses i and A's poses j: the misplacement of the chain
    against A, whatever the frame and the lift of x."""
    x = np.asarray(x, dtype=np.float64)
    out = []
    for c in (1, 2):
        mine, base = x[t0 + 40 * c:t0 + 40 * (c + 1)], x[t0:t0 + 40]
        got = np.linalg.norm(mine[:, None, :] - base[None, :, :], axis=2)
        want = np.linalg.norm(world[40 * c:40 * (c + 1), None, :] - world[None, :40, :], axis=2)
        out.append(float(np.abs(got - want).max()))
    return np.array(out)


@pytest.mark.parametrize("d", (2, 3))
def test_contaminated_start_through_problem(d):
    """Problem.multi_robot_initialization from the same seed without and with the vote.  The reference (placement_ref for the
    plain start, chain_consensus_ref for the robust one, both on the odometry start brought back to d columns) gives each
    chain's error against A; the starts have the reference's errors within 1e-6 m (the rows' bound plus the two lifts is below
    1e-9), the inlier bytes are the construction's, and the ratio plain / robust is at least HALF the reference's ratio -- a
    margin of 2 where the errors agree to six digits -- which the reference puts above 20."""
    f = fleet(d)
    P, dims, table, chains, world = f["P"], f["dims"], f["table"], f["chains"], f["world"]
    t0 = dims[0] * dims[1] + dims[2]
    old = P.op("odometryInitialization")
    x_old = old @ old[:d].T
    plain, pinfo = P.multi_robot_initialization(seed=7, gn_steps=5)
    robust, info = P.multi_robot_initialization(seed=7, gn_steps=5, consensus_barc2=BARC2)
    ref_p = pl.reference(*dims, table, chains, x_old, 5)
    ref_r = cc.reference(*dims, table, chains, x_old, 5, BARC2, None, order=cc.GREEDY)
    assert cc.committed(ref_r), (ref_r["ambiguous"][:3], ref_r["band"][:3], ref_r["margin"])
    e_ref_p, e_ref_r = chain_errors(ref_p["X"], world, t0), chain_errors(ref_r["X"], world, t0)
    e_p, e_r = chain_errors(plain, world, t0), chain_errors(robust, world, t0)
    print("fleet d=%d: chain errors plain %s robust %s; reference plain %s robust %s" % (d, e_p, e_r, e_ref_p, e_ref_r))
    assert np.all(e_ref_p / e_ref_r > 20)
    assert np.abs(e_p - e_ref_p).max() < 1e-6 and np.abs(e_r - e_ref_r).max() < 1e-6
    assert np.all(e_p / e_r >= 0.5 * e_ref_p / e_ref_r)
    assert np.array_equal(info["inlier"] == 0, f["bad"]) and info["excluded"] == int(f["bad"].sum()) and info["no_consensus"] == 0
    assert list(info["status"]) == [4, 0, 0] and list(info["list_len"]) == [0, 300, 300] and info["placed"] == 2 and info["levels"] == 2
    assert np.array_equal(info["consensus"], ref_r["consensus"]) and "inlier" not in pinfo
    # the level order has the same lists here, and the vote off has the plain call's bits
    lev, linfo = P.multi_robot_initialization(seed=7, gn_steps=5, order="levels", consensus_barc2=BARC2)
    assert np.array_equal(bits(lev), bits(robust)) and linfo["levels"] == 1 and np.array_equal(linfo["inlier"], info["inlier"])
    assert np.array_equal(bits(P.multi_robot_initialization(seed=7, gn_steps=5, consensus_barc2=None)[0]), bits(plain))


def test_driver_chain_consensus(cora_main, tmp_path):  # noqa: F811
    """cora_main --place-chains --chain-consensus on the contaminated fleet (d = 2) exits 0 and prints the counts of
    test_contaminated_start_through_problem, under both orders; without --place-chains the flag is refused."""
    import re
    import subprocess
    f = fleet(2)
    n, name, table = f["dims"][1], f["name"], f["table"]
    data = str(tmp_path / "fleet.pyfg")
    with open(data, "w") as out:
        for i in range(n):
            out.write("VERTEX_SE2 %d.0 %s 0 0 0\n" % (i, name(i)))
        up = " ".join("%.17g" % f["cov"][r, c] for r in range(3) for c in range(r, 3))
        for k, (row, dat) in enumerate(zip(table[0], table[1])):
            a, b = int(row[0]) // 2, int(row[1]) // 2
            out.write("EDGE_SE2 %d.0 %s %s %.17g %.17g %.17g %s\n" % (k, name(a), name(b), dat[4], dat[5], np.arctan2(dat[2], dat[0]), up))
        for m, (a, b) in enumerate(f["ranges"]):
            out.write("EDGE_RANGE %d.0 %s %s %.17g %.17g\n" % (m, name(a), name(b), table[3][m, 0], 0.05 ** 2))
    for extra in ([], ["--chain-levels"]):
        flags = ["--odom-init", "--device-init", "--place-chains", *extra, "--chain-consensus", "%g" % BARC2]
        r = subprocess.run([cora_main, data, *flags], stdout=subprocess.PIPE, text=True, timeout=600, check=True)
        m = re.search(r"chain consensus: (\d+) chains without consensus, (\d+) ranges excluded; smallest consensus / list length ([0-9.]+)", r.stdout)
        assert m, r.stdout[-2000:]
        print(m.group(0))
        assert [int(m.group(1)), int(m.group(2))] == [0, int(f["bad"].sum())] and 0.8 < float(m.group(3)) < 1.0
        assert re.search(r"chain placement: 2 chains placed, 0 not placed", r.stdout)
    r = subprocess.run([cora_main, data, "--odom-init", "--device-init", "--chain-consensus", "%g,20" % BARC2], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "--place-chains" in r.stderr


def test_a_nan_is_no_vote():
    """A NaN in the position of a pose of B that one entry of B's list ranges from, and no entry of C's list to: every
    hypothesis whose sample holds the entry is refused, every other hypothesis does not count it, and the fit leaves it out.  The
    resident call ends in CORA_ERR_NAN at that measurement's range row, after the chains' rows were written: every other row
    has the bits of the mirror on the same vector with the pose finite and that range lengthened by 1 000 m instead -- the same
    elected hypothesis, the same inliers, the same masked sums.  (Were a NaN score a vote, the entry would be an inlier and
    every row of B not a number.)"""
    from cora_amd import capi
    from test_chain_consensus_cpu import exact
    (dims, table, X, chains, _), kw, _ = exact(2)
    d, t0 = 2, dims[0] * dims[1] + dims[2]
    rr = np.asarray(table[2])
    rows = rr[:, 1:] - t0
    in_b = lambda v: (v >= 30) & (v < 60)  # noqa: E731
    to_c = set(int(v) for v in rows[(rows.max(axis=1) >= 60)].ravel() if 30 <= v < 60)
    first = next(m for m in range(len(rr)) if rows[m].max() < 60)   # the origin of B's list stays finite
    pick = next(m for m in range(len(rr)) if m != first and rows[m].max() < 60 and int(rows[m][in_b(rows[m])][0]) not in to_c and
                np.sum(rows == rows[m][in_b(rows[m])][0]) == 1)
    pose = int(rows[pick][in_b(rows[pick])][0])
    Xn = X.copy()
    Xn[t0 + pose, 0] = np.nan
    far = [np.array(t, copy=True) for t in table]
    far[3][pick, 0] += 1000.0
    host = capi.Context(*dims, *pl.diagonal_q(*dims), device=-1)
    host.set_measurements(*far)
    host.set_odometry_chains(chains)
    host.set_chain_placement_order(order=cc.LEVELS, **kw)
    want = host.debug_place_chains_robust_host(X, BARC2, 5)
    assert want["inlier"][pick] == 0 and want["excluded"] == 1 and list(want["status"]) == [4, 0, 0]
    ctx = case("exact", 2, device=0)[0]
    x = ctx.dev_alloc(d)
    try:
        ctx.upload(Xn, x)
        with pytest.raises(capi.CoraError) as e:
            ctx.place_chains_robust_dev(x, BARC2, 5)
        assert e.value.code == ERR_NAN
        got = ctx.download(x, d)
    finally:
        ctx.dev_free(x)
    keep = np.ones(len(X), dtype=bool)
    keep[t0 + pose] = False
    keep[rr[:, 0]] = False   # (the range rows: the mirror's are of the other table)
    assert np.isnan(got[t0 + pose]).any() and np.array_equal(bits(got[keep]), bits(want["X"][keep]))
