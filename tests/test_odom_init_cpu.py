"""The odometry initialisation without a GPU: cora_debug_odometry_init_host (the composition function the kernels call, in
the device's bracket order, on plan-only handles) against the longdouble reference of tests/odom_ref.py within its derived
bounds -- on the catalogue's graphs and on synthetic chains whose lengths sit on every boundary of the scan's shape --,
Problem::odometryChains against a Python restatement of the rule, every refusal, and the exact cases.
Problem.op("odometryInitialization") runs the device form (there is no host fall-back): tests/test_gpu_odom_init.py."""
import numpy as np
import pytest

import odom_ref as od
import residuals_ref as rr
import topologies as tp
from cora_amd import capi

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
TOPOLOGIES = ("robots-d2", "robots-d3", "reversed", "dups", "singletons", "pp_only", "n1", "n2", "n63", "n64", "n65", "n128")

_BUILT = {}


def catalogue(name, device=-1):
    """(ctx, (d, n, r, nt), table, chains) of a catalogue entry with its measurement table and chains installed."""
    key = (name, device)
    if key not in _BUILT:
        A, Q, dm, g = tp.build(name)
        ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=device)
        table, chains = rr.table(g), od.chains_of(g)
        ctx.set_measurements(*table)
        ctx.set_odometry_chains(chains)
        _BUILT[key] = (ctx, (dm.d, dm.n, dm.r, dm.n_trans), table, chains)
    return _BUILT[key]


def synthetic(d, kind, device=-1):
    """(ctx, dims, table, chains) of a string of poses cut into chains: 'boundaries' (every boundary of the scan's shape),
    'sweeps' (the same and enough tiles for a second sweep of the middle pass), 'ones' (every chain of length 1)."""
    key = ("syn", d, kind, device)
    if key not in _BUILT:
        probe = capi.Context(2, 1, 0, 1, *od.diagonal_q(2, 1, 0, 1), device=-1)
        tile, sweep = probe.odometry_scan_shape()
        if kind == "ones":
            lengths = [1] * (tile + 40)
        else:
            lengths, _ = od.boundary_lengths(tile, sweep, kind == "sweeps")
        n = sum(m + 1 for m in lengths) + 3   # three poses in no chain at the end
        r = 12
        table = od.synthetic_table(d, n, r, seed=17 * d + len(kind), step=1.0 if kind != "sweeps" else 30.0)
        ctx = capi.Context(d, n, r, n, *od.diagonal_q(d, n, r, n), device=device)
        ctx.set_measurements(*table)
        chains = od.synthetic_chains(lengths)
        ctx.set_odometry_chains(chains)
        assert ctx.odometry_chains_count() == (len(lengths), n - 3)
        _BUILT[key] = (ctx, (d, n, r, n), table, chains)
    return _BUILT[key]


def reference_of(key, dims, table, chains, seed=5, landmarks=True):
    """(starts, landmarks, reference), computed once and shared (tests/test_gpu_odom_init.py reads the same)."""
    key = ("ref", key, seed, landmarks)
    if key not in _BUILT:
        d, n, r, nt = dims
        starts, lm = od.draw_inputs(d, len(chains), nt - n, seed)
        lm = lm if landmarks else None
        _BUILT[key] = (starts, lm, od.reference(d, n, r, nt, table, chains, starts, lm))
    return _BUILT[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_host_mirror_on_the_catalogue(name):
    ctx, dims, table, chains = catalogue(name)
    starts, lm, ref = reference_of(name, dims, table, chains)
    got = ctx.debug_odometry_init_host(starts, lm)
    worst = od.check(got["X"], *dims, table, ref)
    print("%s: %d chains, %d positions; worst error / bound: rotation %.3f translation %.3f range %.3f"
          % (name, len(chains), ref["written"], *worst))
    assert got["written"] == ref["written"] == ctx.odometry_chains_count()[1]
    assert got["n_degenerate"] == ref["degenerate"].sum() and np.array_equal(got["degenerate"], ref["degenerate"])


@pytest.mark.parametrize("name", ("singletons", "pp_only", "n1"))
def test_unreached_poses_and_degenerate_ranges(name):
    """Without landmarks every landmark sits at zero beside the poses no chain reaches: their ranges are degenerate."""
    ctx, dims, table, chains = catalogue(name)
    d, n, r, nt = dims
    starts, lm, ref = reference_of(name, dims, table, chains, seed=9, landmarks=False)
    got = ctx.debug_odometry_init_host(starts, None)
    od.check(got["X"], *dims, table, ref)
    assert np.array_equal(got["degenerate"], ref["degenerate"]) and got["n_degenerate"] == ref["degenerate"].sum()
    if name != "pp_only":
        assert got["n_degenerate"] > 0
    X = got["X"]
    for m in np.flatnonzero(ref["degenerate"]):
        assert not X[table[2][m, 0]].any()
    reached = np.zeros(n, dtype=bool)
    for ch in chains:
        reached[table[0][ch[0], 0] // d] = True
        reached[table[0][ch, 1] // d] = True
    assert name == "pp_only" or not reached.all()
    for i in np.flatnonzero(~reached):   # exactly (I, 0)
        assert np.array_equal(bits(X[d * i:d * i + d]), bits(np.eye(d))) and not X[d * n + r + i].any()


@pytest.mark.parametrize("d", (2, 3))
@pytest.mark.parametrize("kind", ("boundaries", "sweeps", "ones"))
def test_host_mirror_on_the_boundaries_of_the_scan(d, kind):
    ctx, dims, table, chains = synthetic(d, kind)
    tile, sweep = ctx.odometry_scan_shape()
    lengths = [len(ch) for ch in chains]
    if kind == "ones":
        assert set(lengths) == {1} and sum(m + 1 for m in lengths) > 2 * tile
    else:
        assert {1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3} <= set(lengths)
        assert (sum(m + 1 for m in lengths) > tile * sweep) == (kind == "sweeps")
    starts, lm, ref = reference_of(("syn", d, kind), dims, table, chains)
    got = ctx.debug_odometry_init_host(starts, lm)
    worst = od.check(got["X"], *dims, table, ref)
    print("d = %d, %s: %d chains, %d positions; worst error / bound: rotation %.3f translation %.3f range %.3f"
          % (d, kind, len(chains), ref["written"], *worst))
    assert got["written"] == ref["written"]
    assert np.array_equal(got["degenerate"], ref["degenerate"])
    again = ctx.debug_odometry_init_host(starts, lm)
    assert np.array_equal(bits(again["X"]), bits(got["X"]))


@pytest.mark.parametrize("name", [t for t in TOPOLOGIES if t != "dups"])
def test_problem_chains_follow_the_rule(name):
    """Problem::odometryChains against the Python restatement (CORA::Problem refuses the repeated measurements of `dups`,
    as the reference does: the last-duplicate rule is covered on the handle, test_host_mirror_on_the_catalogue)."""
    P = tp.to_problem(name)
    want = od.chains_of(tp.build(name)[3])
    got = P.odometry_chains()
    assert [list(c) for c in got] == want


def test_the_last_duplicate_wins():
    g = tp.build("dups")[3]
    chains = od.chains_of(g)
    pairs = [(m[0], m[1]) for m in g.rpms]
    used = {e for ch in chains for e in ch}
    for e, pr in enumerate(pairs):
        later = [f for f in range(e + 1, len(pairs)) if pairs[f] == pr]
        if later:
            assert e not in used and (later[-1] in used)
    assert len(chains) == 1 and len(chains[0]) == 69


def small(d=3, n=12, r=4):
    table = od.synthetic_table(d, n, r, seed=3)
    ctx = capi.Context(d, n, r, n, *od.diagonal_q(d, n, r, n), device=-1)
    return ctx, table


def refused(ctx, chains, code, *words):
    with pytest.raises(capi.CoraError) as e:
        ctx.set_odometry_chains(chains)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals():
    ctx, table = small()
    refused(ctx, [[0, 1]], ERR_NOT_READY, "measurement table")
    with pytest.raises(capi.CoraError) as e:
        ctx.debug_odometry_init_host(np.zeros((0, 3)))
    assert e.value.code == ERR_NOT_READY
    er, ed, rg, rd = table
    # an edge without a rotation part: edge 7 as a pose-landmark style measurement
    er2 = er.copy()
    er2[7, 1] = -1
    ctx.set_measurements(er2, ed, rg, rd)
    good = [[0, 1, 2], [4, 5]]
    ctx.set_odometry_chains(good)
    assert ctx.odometry_chains_count() == (2, 7)
    starts = np.array([[0.0, 0, 0], [1.0, 2, 3]])
    before = ctx.debug_odometry_init_host(starts)["X"]
    refused(ctx, [[0, 11]], ERR_ARG, "edge 11", "chain 0")
    refused(ctx, [[0], [-1]], ERR_ARG, "edge -1", "chain 1")
    refused(ctx, [[6, 7]], ERR_ARG, "edge 7", "no rotation part")
    refused(ctx, [[0, 1], []], ERR_ARG, "chain 1", "empty")
    refused(ctx, [[0, 2]], ERR_ARG, "edge 2", "does not start at the pose")
    refused(ctx, [[0, 1], [1, 2]], ERR_ARG, "head of chain 1", "another position writes")   # the head of chain 1 is pose 1
    refused(ctx, [[0, 1], [3], [0]], ERR_ARG, "chain 2", "another position writes")
    # every refused call left the tables as they were
    assert ctx.odometry_chains_count() == (2, 7)
    assert np.array_equal(bits(ctx.debug_odometry_init_host(starts)["X"]), bits(before))
    # inputs
    for bad in (np.nan, np.inf):
        s = starts.copy()
        s[1, 2] = bad
        with pytest.raises(capi.CoraError) as e:
            ctx.debug_odometry_init_host(s)
        assert e.value.code == ERR_ARG and "start" in str(e.value)
    with pytest.raises(capi.CoraError) as e:
        ctx.debug_odometry_init_host(starts[:1])
    assert e.value.code == ERR_ARG
    # device forms on a plan-only handle
    with pytest.raises(capi.CoraError) as e:
        ctx.odometry_init(starts)
    assert e.value.code == ERR_HIP
    # n_chains = 0 clears; a new measurement table drops the chains
    ctx.set_odometry_chains(good)
    ctx.set_odometry_chains([])
    assert ctx.odometry_chains_count() == (0, 0)
    ctx.set_odometry_chains(good)
    ctx.set_measurements(*table)
    assert ctx.odometry_chains_count() == (0, 0)
    X = ctx.debug_odometry_init_host(np.zeros((0, 3)))["X"]   # no chains: every pose is (I, 0)
    assert np.array_equal(X[:36], np.tile(np.eye(3), (12, 1))) and not X[36 + 4:].any()
    # two measurements that name one range row
    rg2 = rg.copy()
    rg2[2, 0] = rg2[1, 0]
    ctx.set_measurements(er, ed, rg2, rd)
    refused(ctx, good, ERR_ARG, "range measurement 2")


def test_a_landmark_that_is_not_finite_is_refused():
    ctx, dims, table, chains = catalogue("n2")
    starts, lm, _ = reference_of("n2", dims, table, chains)
    bad = lm.copy()
    bad[1, 0] = np.inf
    with pytest.raises(capi.CoraError) as e:
        ctx.debug_odometry_init_host(starts, bad)
    assert e.value.code == ERR_ARG and "landmark" in str(e.value)
    with pytest.raises(capi.CoraError) as e:
        ctx.debug_odometry_init_host(starts, lm[:1])
    assert e.value.code == ERR_ARG


def test_a_product_that_is_not_finite_is_reported():
    ctx, (er, ed, rg, rd) = small(d=2, n=6, r=0)
    ed = ed.copy()
    ed[:, :4] = np.eye(2).reshape(-1)
    ed[:, 4:6] = 1.5e308
    ctx.set_measurements(er, ed, rg, rd)
    ctx.set_odometry_chains([[0, 1, 2]])
    with pytest.raises(capi.CoraError) as e:
        ctx.debug_odometry_init_host(np.zeros((1, 2)))
    assert e.value.code == ERR_NAN


def test_partitioned_handles_are_refused():
    A, Q, dm, g = tp.build("robots-d2")
    p = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=2)
    refused(p, od.chains_of(g), ERR_ARG, "partitioned")
    with pytest.raises(capi.CoraError) as e:
        p.debug_odometry_init_host(np.zeros((0, 2)))
    assert e.value.code == ERR_ARG


@pytest.mark.parametrize("d", (2, 3))
def test_exact_cases(d):
    n, r = 700, 6
    er, ed, rg, rd = od.synthetic_table(d, n, r, seed=40 + d)
    ctx = capi.Context(d, n, r, n, *od.diagonal_q(d, n, r, n), device=-1)
    lengths = [300, 1, 64, 255, 70]
    chains = od.synthetic_chains(lengths, first=2)   # poses 0 and 1 and the last ones are in no chain
    rng = np.random.default_rng(d)
    starts = np.round(100 * rng.uniform(-1, 1, (len(chains), d)))
    t0 = d * n + r
    # identity edges give exact identities, and every pose of a chain sits on its start
    ed1 = ed.copy()
    ed1[:, :d * d] = np.eye(d).reshape(-1)
    ed1[:, d * d:d * d + d] = 0.0
    ctx.set_measurements(er, ed1, rg, rd)
    ctx.set_odometry_chains(chains)
    X = ctx.debug_odometry_init_host(starts)["X"]
    assert np.array_equal(bits(X[:d * n]), bits(np.tile(np.eye(d), (n, 1))))
    for c, ch in enumerate(chains):
        for i in range(ch[0], ch[-1] + 2):
            assert np.array_equal(X[t0 + i], starts[c])
    # pure translations by integers: the sums are exact in every bracket order
    ed2 = ed1.copy()
    ed2[:, d * d:d * d + d] = rng.integers(-1000, 1000, (n - 1, d))
    ctx.set_measurements(er, ed2, rg, rd)
    ctx.set_odometry_chains(chains)
    X = ctx.debug_odometry_init_host(starts)["X"]
    assert np.array_equal(bits(X[:d * n]), bits(np.tile(np.eye(d), (n, 1))))
    reached = np.zeros(n, dtype=bool)
    for c, ch in enumerate(chains):
        want = starts[c] + np.vstack([np.zeros((1, d)), np.cumsum(ed2[ch, d * d:d * d + d], axis=0)])
        assert np.array_equal(X[t0 + ch[0]:t0 + ch[-1] + 2], want)
        reached[ch[0]:ch[-1] + 2] = True
    # an unreached pose is exactly (I, 0)
    assert (~reached).sum() == n - sum(m + 1 for m in lengths) and not X[t0:t0 + n][~reached].any()
