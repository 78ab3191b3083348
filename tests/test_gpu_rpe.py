"""The relative pose error on the device (k_rpe, k_rpe_argmax and the partial reductions behind cora_rpe*) against the
longdouble reference of tests/rpe_ref.py within the two bounds of include/cora_hip.h, bit for bit against the host mirror
(per-pair values, maxima, first maximum; the sums within m eps sum: the mirror adds them in pair order), at the launch
edges, what the call must leave alone, and end to end on the robust case of tests/test_gpu_gnc.py."""
import numpy as np
import pytest

import rpe_ref as rp
from cora_amd import capi, host
from oracle import assemble as asm
from oracle import oracle as orc
from synth import ground_truth, make_graph

pytestmark = pytest.mark.gpu

_BUILT = {}
ARRAYS = ("trans_err", "rot_err")


def built(d, n):
    """(ctx, (d, n, r, nt), ground truth, chains) of a graph of make_graph at its default seed, once per process."""
    key = (d, n)
    if key not in _BUILT:
        g = make_graph(d=d, n=n, n_landmarks=3, n_ranges=min(20, n * 3), n_loops=0)
        A = asm.assemble(g)
        Q = orc.CSR.from_scipy(A["Q"])
        dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
        _BUILT[key] = (capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val), (dm.d, dm.n, dm.r, dm.n_trans),
                       ground_truth(g), [list(range(n))])
    return _BUILT[key]


def estimate(Ref, truth, dims, k, rng, noise=1e-2):
    base = rp.gauge_copy(Ref, *dims, k, rng) if k >= Ref.shape[1] else rp.reference_of_rank(truth, k, rng)
    return base + noise * rng.standard_normal(base.shape)


def against_host_mirror(dev, mir, m, what):
    for key in ARRAYS:
        assert np.array_equal(dev[key], mir[key]), (what, key)
    for key in ("m", "max_et", "max_er", "argmax_et"):
        assert dev[key] == mir[key], (what, key)
    for key in ("sum_et2", "sum_er2"):
        assert abs(dev[key] - mir[key]) <= max(m, 1) * rp.EPS * mir[key], (what, key, dev[key], mir[key])


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", [30, 64, 65, 300])
def test_device_against_the_reference_and_the_host_mirror(d, n):
    ctx, dims, truth, chains = built(d, n)
    rng = np.random.default_rng(100 * d + n)
    pairs = np.concatenate([rp.pairs_by_step(chains, 1)[0], rp.pairs_by_step(chains, 7)[0], [[0, 0], [n - 1, 0]],
                            rng.integers(0, n, (9, 2))]).astype(np.int32)
    ctx.set_pose_pairs(pairs)
    for k, kr in rp.RANKS(d):
        what = "d=%d n=%d k=%d kr=%d" % (d, n, k, kr)
        Ref = rp.reference_of_rank(truth, kr, rng)
        X = estimate(Ref, truth, dims, k, rng)
        dev = ctx.rpe(X, Ref)
        rp.check(dev, X, Ref, *dims, pairs, what=what)
        against_host_mirror(dev, ctx.debug_rpe_host(X, Ref), len(pairs), what)


def test_even_stride_against_an_odd_reference_stride_in_the_plane():
    """d = 2 with 16-byte pieces of X and 8-byte pieces of the reference: k = 4 against kr = 3, the one pair of piece widths
    that rpe_ref.RANKS(2) does not hold (its reference strides 2 and 24 are even, and 5 goes with k = 5)."""
    d, n = 2, 30
    ctx, dims, truth, chains = built(d, n)
    rng = np.random.default_rng(43)
    pairs = np.concatenate([rp.pairs_by_step(chains, 1)[0], rp.pairs_by_step(chains, 7)[0], [[0, 0], [n - 1, 0]]]).astype(np.int32)
    ctx.set_pose_pairs(pairs)
    Ref = rp.reference_of_rank(truth, 3, rng)
    X = estimate(Ref, truth, dims, 4, rng)
    dev = ctx.rpe(X, Ref)
    rp.check(dev, X, Ref, *dims, pairs, what="d=2 k=4 kr=3")
    against_host_mirror(dev, ctx.debug_rpe_host(X, Ref), len(pairs), "d=2 k=4 kr=3")


@pytest.mark.parametrize("d", [2, 3])
def test_launch_edges_resident_vectors_and_table_replacement(d):
    """m = 1, 31, 32, 33 (one block, its last group, a second block of one pair), 2 945 pairs (93 blocks of partials: more
    than one round of the 256-thread finish would need 8 192 pairs, so 8 200 pairs are there too -- the finishing kernels
    stride over any number of partials, they have no limit of their own), a shorter table after a longer one and back."""
    ctx, dims, truth, chains = built(d, 300)
    n = dims[1]
    rng = np.random.default_rng(7 + d)
    k, kr = d + 1, d
    X = estimate(truth, truth, dims, k, rng)
    x, ref = ctx.dev_alloc(k), ctx.dev_alloc(kr)
    ctx.upload(X, x)
    ctx.upload(truth, ref)
    steps = np.concatenate([rp.pairs_by_step(chains, s)[0] for s in range(1, 11)])
    assert len(steps) == 2945
    many = np.concatenate([steps, steps[::-1, ::-1], rng.integers(0, n, (8200 - 2 * 2945, 2))]).astype(np.int32)
    tables = [steps[:1], steps[:31], steps[:32], steps[:33], steps, many, steps[:5], steps[:40]]
    for pairs in tables:
        m = len(pairs)
        ctx.set_pose_pairs(pairs)
        assert ctx.pose_pairs_count() == m
        dev = ctx.rpe_dev(x, k, ref, kr)
        rp.check(dev, X, truth, *dims, pairs, what="d=%d m=%d" % (d, m))
        against_host_mirror(dev, ctx.debug_rpe_host(X, truth), m, "m=%d" % m)
        # sums only: the same six numbers bit for bit; and a second call gives the same bits
        assert np.array_equal(ctx.rpe_dev(x, k, ref, kr, arrays=False)["raw"], dev["raw"])
        again = ctx.rpe_dev(x, k, ref, kr)
        assert all(np.array_equal(again[key], dev[key]) for key in ARRAYS + ("raw",))
    # the first of several pairs that attain the maximum: the largest error of `steps`, planted again further on
    ctx.set_pose_pairs(steps)
    top = int(ctx.rpe_dev(x, k, ref, kr)["argmax_et"])
    twice = np.concatenate([steps[:top + 50] if top + 50 < len(steps) else steps, steps[top:top + 1], steps[top:top + 1]]).astype(np.int32)
    ctx.set_pose_pairs(twice)
    res = ctx.rpe_dev(x, k, ref, kr)
    assert res["argmax_et"] == top and np.sum(res["trans_err"] == res["max_et"]) == 3
    ctx.set_pose_pairs(None)
    with pytest.raises(capi.CoraError) as e:
        ctx.rpe_dev(x, k, ref, kr)
    assert e.value.code == 2
    ctx.dev_free(x)
    ctx.dev_free(ref)


@pytest.mark.parametrize("d", [2, 3])
def test_the_handle_is_left_alone(d):
    import residuals_ref as rr
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
    ctx.set_measurements(*rr.table(g))
    ctx.assembly_build(Q.rowptr, Q.col)
    y, v, o1, o2 = (ctx.dev_alloc(p) for _ in range(4))
    ctx.upload(Y, y)
    ctx.upload(V, v)
    ctx.set_point_dev(y)

    def state():
        ctx.hvp_dev(v, o1)
        ctx.precondition_projected_dev(v, o2)
        return (ctx.download(o1, p).copy(), ctx.download(o2, p).copy(), ctx.point_cost(), ctx.measurement_counts(),
                ctx.assembly_info(), ctx.format_digest(), ctx.measurement_residuals(Y)["sums"].copy())

    before = state()
    ctx.set_pose_pairs(rp.pairs_by_step([list(range(dm.n))], 1)[0])
    for k, kr in rp.RANKS(d):
        Ref = rp.reference_of_rank(truth, kr, rng)
        ctx.rpe(estimate(Ref, truth, dims, k, rng), Ref)
    # the current point itself as the estimate, on the device
    ref = ctx.dev_alloc(d)
    ctx.upload(truth, ref)
    a = ctx.rpe_dev(y, p, ref, d)
    rp.check(a, Y, truth, *dims, rp.pairs_by_step([list(range(dm.n))], 1)[0], what="the current point")
    after = state()
    for b, a_ in zip(before, after):
        assert np.array_equal(b, a_) if isinstance(b, np.ndarray) else b == a_
    for ptr in (y, v, o1, o2, ref):
        ctx.dev_free(ptr)
    ctx.close()


# ---- the robust case of tests/test_gpu_gnc.py, judged by the error of its steps ---------------------------------------
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
def test_plain_and_robust_solve_end_to_end(d):
    g = make_graph(d=d, n=30, n_landmarks=3, n_ranges=60, n_loops=5)
    for i in BAD:
        a, b, r, cov = g.ranges[i]
        g.ranges[i] = (a, b, r + SHIFT, cov)
    truth = ground_truth(g)
    dims = (d, 30, len(g.ranges), 33)
    plain_problem = _problem(g)
    x_plain = plain_problem.solve(truth, max_rank=10)["x"]
    pairs = plain_problem.pose_pairs_by_step(1)
    assert np.array_equal(pairs[0], rp.pairs_by_step([list(range(30))], 1)[0])
    plain = plain_problem.relative_error(x_plain, truth, pairs)
    rp.check(plain, x_plain, truth, *dims, pairs[0], what="plain solve")
    P = _problem(g)
    res = P.solve_robust(truth, {"range": np.full(len(g.ranges), BARC2)}, cost="tls")
    robust = P.relative_error(res["x"], truth, pairs)
    print("d=%d: step-1 RPE of the plain solve: translation RMSE %.6g rotation RMSE %.6g; of the robust solve: %.6g, %.6g" % (
        d, plain["trans_rmse"], plain["rot_rmse"], robust["trans_rmse"], robust["rot_rmse"]))
    for r_ in (plain, robust):
        assert r_["m"] == 29 and all(np.isfinite(r_[key]) for key in ("trans_rmse", "rot_rmse", "mean_trans_drift", "mean_rot_drift"))
        assert np.all(np.isfinite(r_["trans_err"])) and np.all(np.isfinite(r_["rot_err"]))
    # a relaxed level (rank d + 2 near the solution) has the RPE of any O(k) gauge of itself, within the bound of each
    k = d + 2
    rng = np.random.default_rng(90 + d)
    lifted = np.hstack([x_plain, np.zeros((x_plain.shape[0], k - d))]) + 1e-3 * rng.standard_normal((x_plain.shape[0], k))
    G = np.linalg.qr(rng.standard_normal((k, k)))[0]
    turned = lifted @ G
    a = P.relative_error(lifted, truth, pairs)
    b = P.relative_error(turned, truth, pairs)
    bt_a, br_a = rp.bounds(lifted, truth, *dims, pairs[0])
    bt_b, br_b = rp.bounds(turned, truth, *dims, pairs[0])
    # (turned = lifted G is itself rounded: k + 2 eps of |row| per entry, so E and u of the turned copy are those of the
    # lifted one within 4 (k + 2) eps |X_i| |X_j| and 4 (k + 2) eps |X_i| (|x_i| + |x_j|))
    rot, trn = rp.rows(*dims)
    i, j = pairs[0][:, 0], pairs[0][:, 1]
    ni = np.linalg.norm(turned[rot[i]], axis=(1, 2))
    nj = np.linalg.norm(turned[rot[j]], axis=(1, 2))
    copy_r = 4 * (k + 2) * rp.EPS * ni * nj
    copy_t = 4 * (k + 2) * rp.EPS * ni * (np.linalg.norm(turned[trn[i]], axis=1) + np.linalg.norm(turned[trn[j]], axis=1))
    assert np.all(np.abs(a["trans_err"] - b["trans_err"]) <= bt_a + bt_b + copy_t)
    assert np.all(np.abs(a["rot_err"] - b["rot_err"]) <= br_a + br_b + copy_r)
