"""The relative pose error without a GPU: cora_debug_rpe_host (the definitions of cora_rpe_dev on the host, in the
device's lane and tree order) on plan-only handles against the longdouble reference of tests/rpe_ref.py within the two
bounds of include/cora_hip.h, the exact cases, known answers, the pair builders of Problem against rpe_ref's, and every
refusal."""
import ctypes as C

import numpy as np
import pytest

import residuals_ref as rr
import rpe_ref as rp
import topologies as tp
from cora_amd import capi, host
from oracle import assemble as asm
from oracle import oracle as orc
from synth import ground_truth, make_graph

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
TOPOLOGIES = ("robots-d2", "robots-d3", "n1", "n2", "n64", "n65", "singletons", "priors_chain_odd")

_BUILT = {}


def built(d, n):
    """(ctx, (d, n, r, nt), ground truth, chains) of a graph of tests/synth.py on a plan-only handle, once per process."""
    key = (d, n)
    if key not in _BUILT:
        g = make_graph(d=d, n=n, n_landmarks=3, n_ranges=min(20, n * 3), n_loops=0)
        A = asm.assemble(g)
        Q = orc.CSR.from_scipy(A["Q"])
        dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
        ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1)
        _BUILT[key] = (ctx, (dm.d, dm.n, dm.r, dm.n_trans), ground_truth(g), [list(range(n))])
    return _BUILT[key]


def catalogue(name):
    key = ("tp", name)
    if key not in _BUILT:
        A, Q, dm, g = tp.build(name)
        ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1)
        symbols = [s for s, _ in sorted(g.poses.items(), key=lambda kv: kv[1])]
        _BUILT[key] = (ctx, (dm.d, dm.n, dm.r, dm.n_trans), A["truth"], rp.chains_of(symbols))
    return _BUILT[key]


def some_pairs(chains, n, rng):
    """Steps 1 and 3 of every chain, a self pair, a backward pair and pairs across the whole graph."""
    parts = [rp.pairs_by_step(chains, 1)[0], rp.pairs_by_step(chains, 3)[0], np.array([[0, 0], [n - 1, 0]], dtype=np.int32),
             rng.integers(0, n, (17, 2)).astype(np.int32)]
    return np.concatenate(parts)


def estimate(Ref, truth, dims, k, rng, noise=1e-2):
    """An estimate of k columns near the reference's motions: a gauge copy where k >= kr, else the truth at rank k."""
    base = rp.gauge_copy(Ref, *dims, k, rng) if k >= Ref.shape[1] else rp.reference_of_rank(truth, k, rng)
    return base + noise * rng.standard_normal(base.shape)


def run_all_ranks(ctx, dims, truth, chains, rng, what):
    d, n = dims[0], dims[1]
    pairs = some_pairs(chains, n, rng)
    ctx.set_pose_pairs(pairs)
    assert ctx.pose_pairs_count() == len(pairs)
    for k, kr in rp.RANKS(d):
        Ref = rp.reference_of_rank(truth, kr, rng)
        X = estimate(Ref, truth, dims, k, rng)
        res = ctx.debug_rpe_host(X, Ref)
        rp.check(res, X, Ref, *dims, pairs, what="%s k=%d kr=%d" % (what, k, kr))
        assert np.array_equal(ctx.debug_rpe_host(X, Ref, arrays=False)["raw"], res["raw"])


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", [30, 65])
def test_host_form_against_the_reference_on_synthetic_graphs(d, n):
    ctx, dims, truth, chains = built(d, n)
    run_all_ranks(ctx, dims, truth, chains, np.random.default_rng(10 * n + d), "synth d=%d n=%d" % (d, n))


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_host_form_against_the_reference_on_the_catalogue(name):
    ctx, dims, truth, chains = catalogue(name)
    run_all_ranks(ctx, dims, truth, chains, np.random.default_rng(len(name)), name)


def test_far_from_the_origin_the_bound_still_holds():
    """x_j - x_i carries one relative eps: a trajectory 10^6 away does not cancel beyond the bound's |x_j - x_i| term."""
    ctx, dims, truth, chains = built(3, 30)
    rng = np.random.default_rng(5)
    pairs = rp.pairs_by_step(chains, 1)[0]
    ctx.set_pose_pairs(pairs)
    Ref = truth.copy()
    Ref[rp.rows(*dims)[1]] += 1e6
    X = estimate(Ref, truth, dims, 4, rng)
    rp.check(ctx.debug_rpe_host(X, Ref), X, Ref, *dims, pairs, what="far from the origin")


@pytest.mark.parametrize("d", [2, 3])
def test_exact_cases(d):
    ctx, dims, truth, chains = built(d, 65)
    rng = np.random.default_rng(40 + d)
    n = dims[1]
    # self pairs, and one pair repeated at several places of a table that spans three blocks
    pairs = np.concatenate([rp.pairs_by_step(chains, 1)[0], [[7, 7], [3, 40]], rp.pairs_by_step(chains, 2)[0], [[3, 40], [0, 0]]]).astype(np.int32)
    pairs[0] = (3, 40)
    pairs[33] = (3, 40)
    ctx.set_pose_pairs(pairs)
    for k, kr in rp.RANKS(d):
        Ref = rp.reference_of_rank(truth, kr, rng)
        X = rng.standard_normal((truth.shape[0], k))  # (off the manifold: X_i X_i^T is not G_i G_i^T)
        res = ctx.debug_rpe_host(X, Ref)
        same = pairs[:, 0] == pairs[:, 1]
        assert same.sum() == 2 and np.all(res["trans_err"][same] == 0.0) and np.all(res["rot_err"][same] == 0.0)
        rep = np.flatnonzero((pairs[:, 0] == 3) & (pairs[:, 1] == 40))
        assert len(rep) == 4 and res["rot_err"][rep[0]] > 0.0
        for key in ("trans_err", "rot_err"):
            assert np.all(res[key][rep] == res[key][rep[0]]), (k, kr, key)
        again = ctx.debug_rpe_host(X, Ref)
        assert all(np.array_equal(res[key], again[key]) for key in ("raw", "trans_err", "rot_err"))
    assert n == 65


@pytest.mark.parametrize("d", [2, 3])
def test_known_answers(d):
    ctx, dims, truth, chains = built(d, 30)
    _, n, r, nt = dims
    rng = np.random.default_rng(60 + d)
    pairs = np.array([[4, 9], [9, 4], [10, 11], [2, 20]], dtype=np.int32)
    ctx.set_pose_pairs(pairs)
    # pose 9 turned by theta: the pairs that end or start there see 2 sqrt 2 |sin(theta / 2)|, the others nothing
    for theta in (0.3, -2.0, np.pi):
        Q = rp.rotation(d, theta, axis=[1.0, -2.0, 0.5])
        X = rp.rotate_pose(truth, d, 9, Q)
        res = ctx.debug_rpe_host(X, truth)
        want = 2 * np.sqrt(2) * abs(np.sin(theta / 2))
        _, br = rp.bounds(X, truth, *dims, pairs)
        # (the bound of the reference: Q itself and the product Q G_j are rounded too, d + 2 more eps of |Q| |G_j| = d)
        slack = (d + 2) * rp.EPS * d
        assert abs(res["rot_err"][0] - want) <= br[0] + slack and abs(res["rot_err"][1] - want) <= br[1] + slack, theta
        assert np.all(res["rot_err"][2:] <= br[2:])
    # pose 20 moved by delta in the frame of pose 2: the pair (2, 20) sees |delta|
    delta = rng.standard_normal(d) * 0.7
    X = rp.shift_pose(truth, d, n, r, 2, 20, delta)
    res = ctx.debug_rpe_host(X, truth)
    bt, _ = rp.bounds(X, truth, *dims, pairs)
    slack = (d + 2) * rp.EPS * np.linalg.norm(delta) * d  # (delta X_i and its addition are rounded)
    assert abs(res["trans_err"][3] - np.linalg.norm(delta)) <= bt[3] + slack
    assert np.all(res["trans_err"][:3] <= bt[:3]) and np.all(res["rot_err"] <= rp.bounds(X, truth, *dims, pairs)[1])
    # a gauge copy has the reference's motions: errors at most the bound plus the rounding of the copy itself
    allp = rp.pairs_by_step(chains, 1)[0]
    ctx.set_pose_pairs(allp)
    for k in (d + 1, 5, 24):
        X = rp.gauge_copy(truth, *dims, k, rng)
        res = ctx.debug_rpe_host(X, truth)
        bt, br = rp.bounds(X, truth, *dims, allp)
        # X = Ref B is itself rounded: (d + 2) eps per entry against |Ref row| |B| -- on E twice, on u against |x| too
        rot, trn = rp.rows(*dims)
        scale = np.linalg.norm(X[trn[allp[:, 1]]], axis=1) + np.linalg.norm(X[trn[allp[:, 0]]], axis=1)
        copy_t = 4 * (d + 2) * rp.EPS * np.sqrt(d) * (scale + 1.0)
        copy_r = 4 * (d + 2) * rp.EPS * d
        assert np.all(res["trans_err"] <= bt + copy_t), (k, float((res["trans_err"] / (bt + copy_t)).max()))
        assert np.all(res["rot_err"] <= br + copy_r), (k, float((res["rot_err"] / (br + copy_r)).max()))


def _problem(name):
    P = tp.to_problem(name)
    A, Q, dm, g = tp.build(name)
    symbols = [s for s, _ in sorted(g.poses.items(), key=lambda kv: kv[1])]
    return P, A["truth"], (dm.d, dm.n, dm.r, dm.n_trans), rp.chains_of(symbols)


@pytest.mark.parametrize("name", ["robots-d2", "robots-d3", "singletons", "n1", "n2"])
def test_pair_builders_against_the_reference(name):
    P, truth, dims, chains = _problem(name)
    d, n, r, nt = dims
    longest = max(len(c) for c in chains)
    for step in (1, 2, 10, 36, longest - 1, longest, longest + 5):
        if step < 1:
            continue
        pairs, path = P.pose_pairs_by_step(step)
        want, wpath = rp.pairs_by_step(chains, step)
        assert np.array_equal(pairs, want) and np.array_equal(path, wpath), (name, step)
        if step >= longest:
            assert len(pairs) == 0
            res = P.relative_error(truth, truth, (pairs, path))  # an empty table: zeros, no device needed, no error
            assert res["m"] == 0 and res["sum_et2"] == 0 and res["max_er"] == 0 and res["trans_rmse"] == 0 and res["mean_trans_drift"] == 0
    positions = truth[rp.rows(*dims)[1][:n]]
    total = max((np.linalg.norm(np.diff(positions[c], axis=0), axis=1).sum() if len(c) > 1 else 0.0) for c in chains)
    for L in (1e-9, 0.5, 2.0, 7.5, 0.5 * total + 1e-3, total * 2 + 1.0):
        pairs, path = P.pose_pairs_by_distance(truth, L)
        want, wpath = rp.pairs_by_distance(chains, positions, L)
        assert np.array_equal(pairs, want), (name, L)
        assert np.all(np.abs(path - wpath) <= 4 * n * rp.EPS * np.maximum(wpath, 1.0)) and np.all(path >= L)
        if L > total:
            assert len(pairs) == 0  # no start reaches it
        elif longest > 1 and L <= 0.5 * total:
            starts = set(pairs[:, 0].tolist())
            assert len(starts) == len(pairs) and len(pairs) < n  # the last pose of a chain never starts a pair
    with pytest.raises(host.HostError):
        P.pose_pairs_by_step(0)
    with pytest.raises(host.HostError):
        P.pose_pairs_by_distance(truth, 0.0)
    with pytest.raises(host.HostError):
        P.pose_pairs_by_distance(truth[:-1], 1.0)


def test_relative_error_needs_a_live_handle_and_checks_its_shapes():
    P, truth, dims, chains = _problem("n2")
    pairs = P.pose_pairs_by_step(1)
    assert len(pairs[0]) == 1
    with pytest.raises(host.HostError, match="no live device handle"):
        P.relative_error(truth, truth, pairs)
    with pytest.raises(host.HostError):
        P.relative_error(truth[:-1], truth, pairs)
    with pytest.raises(host.HostError):
        P.relative_error(truth, truth[:-1], pairs)
    with pytest.raises(host.HostError):
        P.relative_error(truth, truth, pairs[0], path_length=[1.0, 2.0])


def _raw(ctx, X, Ref, x=True, ref=True, out=True, fn="cora_debug_rpe_host"):
    X, Ref = np.asfortranarray(X), np.asfortranarray(Ref)
    dp = C.POINTER(C.c_double)
    o = np.zeros(6)
    return getattr(ctx.L, fn)(ctx.h, X.ctypes.data_as(dp) if x else None, X.shape[0], X.shape[1],
                              Ref.ctypes.data_as(dp) if ref else None, Ref.shape[0], Ref.shape[1], None, None,
                              o.ctypes.data_as(dp) if out else None)


def _set_raw(ctx, m, pairs):
    p = np.ascontiguousarray(pairs, dtype=np.int32) if pairs is not None else None
    return ctx.L.cora_set_pose_pairs(ctx.h, C.c_int64(m), p.ctypes.data_as(C.POINTER(C.c_int32)) if p is not None else None)


def test_refusals_and_the_handle_is_left_alone():
    g = make_graph(d=2, n=30, n_landmarks=3, n_ranges=20, n_loops=0)
    A = asm.assemble(g)
    Q = orc.CSR.from_scipy(A["Q"])
    dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
    ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1)
    truth = ground_truth(g)
    N, n = dm.N, dm.n
    X = np.random.default_rng(3).standard_normal((N, 3))
    ctx.set_measurements(*rr.table(g))
    ctx.assembly_build(Q.rowptr, Q.col)

    def state():
        return ctx.measurement_counts(), ctx.assembly_info(), ctx.format_digest()

    before = state()
    # no table yet
    assert ctx.pose_pairs_count() == 0 and _raw(ctx, X, truth) == ERR_NOT_READY
    # the table's own refusals leave what is installed
    good = np.array([[0, 1], [1, 2], [5, 29]], dtype=np.int32)
    ctx.set_pose_pairs(good)
    for bad in ([[0, 1], [1, n]], [[0, 1], [-1, 2]], [[n, 0]]):
        assert _set_raw(ctx, len(bad), bad) == ERR_ARG
        first = [i for i, p in enumerate(bad) if min(p) < 0 or max(p) >= n][0]
        assert ("pair %d " % first) in ctx.L.cora_last_error(ctx.h).decode()
        assert ctx.pose_pairs_count() == 3
    assert _set_raw(ctx, 2, None) == ERR_ARG and _set_raw(ctx, -1, good) == ERR_ARG
    assert ctx.pose_pairs_count() == 3
    assert ctx.pose_pairs_equal(good) and not ctx.pose_pairs_equal(good[:2]) and not ctx.pose_pairs_equal(good[::-1])
    assert not ctx.pose_pairs_equal(good[:, ::-1]) and not ctx.pose_pairs_equal(None)
    ok = ctx.debug_rpe_host(X, truth)
    for bad_k in (0, 25):
        assert _raw(ctx, np.zeros((N, bad_k)), truth) == ERR_SHAPE
        assert _raw(ctx, X, np.zeros((N, bad_k))) == ERR_SHAPE
    for missing in ("x", "ref", "out"):
        assert _raw(ctx, X, truth, **{missing: False}) == ERR_ARG
    for bad in (float("inf"), float("nan")):
        Xb = X.copy()
        Xb[N - dm.n_trans + 1, 0] = bad  # the position of pose 1
        assert _raw(ctx, Xb, truth) == ERR_NAN
    with pytest.raises(capi.CoraError) as e:
        ctx.rpe(X, truth)  # plan-only: no device, no fall-back
    assert e.value.code == ERR_HIP
    assert np.array_equal(ctx.debug_rpe_host(X, truth)["raw"], ok["raw"])
    # a second call replaces the table, an empty one clears it
    ctx.set_pose_pairs(good[:1])
    assert ctx.pose_pairs_count() == 1 and ctx.debug_rpe_host(X, truth)["trans_err"][0] == ok["trans_err"][0]
    ctx.set_pose_pairs(None)
    assert ctx.pose_pairs_count() == 0 and _raw(ctx, X, truth) == ERR_NOT_READY
    assert ctx.pose_pairs_equal(None) and not ctx.pose_pairs_equal(good)
    assert state() == before
    ctx.close()
    # a partitioned handle has no pair table
    p = capi.Context(2, A["n"], A["r"], A["N"] - 2 * A["n"] - A["r"], Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=2)
    assert _set_raw(p, 1, [[0, 1]]) == ERR_ARG and "partitioned" in p.L.cora_last_error(p.h).decode()
    assert _raw(p, truth, truth) == ERR_ARG and "partitioned" in p.L.cora_last_error(p.h).decode()
    p.close()
