"""The landmark initialisation from ranges without a GPU: cora_debug_multilaterate_host (the functions the kernels call, in
the device's bracket order, on plan-only handles) against the longdouble reference of tests/multilat_ref.py -- statuses,
counts, the chosen point, the rows within the derived bound -- on list lengths that sit on every boundary of the reduction's
shape, on degenerate geometry on either side of the pivot rule, on the catalogue's graphs that have ranges, with both
masks, and every refusal.  The device forms against the mirror, bit for bit: tests/test_gpu_multilat.py."""
import numpy as np
import pytest

import multilat_ref as ml
import topologies as tp
import residuals_ref as rr
from cora_amd import capi

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
CATALOGUE = ("robots-d2", "robots-d3", "hub-d2", "hub-d3", "fat_landmark", "lm_lm", "dups", "pp_only", "n1", "singletons")

_BUILT = {}


def _walk(rng, n, d, step=1.0):
    return np.cumsum(step * rng.normal(0, 1, (n, d)), axis=0)


def _mixed(rng, lists, n):
    """The ranges of lists (landmark index -> pose indices) in a shuffled table order, every other one landmark -> pose."""
    ranges = [(p, n + l) for l, poses in enumerate(lists) for p in poses]
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    return [(b, a) if m % 2 else (a, b) for m, (a, b) in enumerate(ranges)]


def lengths(d, noise=0.0, offset=0.0):
    """Lists of d (status 1), d + 1 (the least solvable), 1, 63, 64, 65, 255, 256, 257, 513 and 16 385 entries (a second
    round of the fold's lanes), every one with the next beside it in the chunk table."""
    rng = np.random.default_rng(40 + d)
    lens = [d, d + 1, 1, 63, 64, 65, 255, 256, 257, 513, 16385]
    n = 16500
    poses = _walk(rng, n, d) + offset
    lms = poses[rng.integers(0, n, len(lens))] + 20 * rng.uniform(-1, 1, (len(lens), d))
    lists = [rng.choice(n, size=k, replace=False) for k in lens]
    return ml.graph(d, poses, lms, _mixed(rng, lists, n), noise=noise, seed=d), {}, dict(lens=lens, truth=lms)


def noisy(d, masks=False):
    """Noisy ranges, every range measured twice, pose-pose and landmark-landmark ranges in between."""
    rng = np.random.default_rng(50 + d)
    lens = [d + 1, 5, 65, 257, 513]
    n = 700
    poses = _walk(rng, n, d)
    lms = 15 * rng.uniform(-1, 1, (len(lens), d))
    lists = [np.repeat(rng.choice(n, size=(k + 1) // 2, replace=False), 2)[:k] for k in lens]
    ranges = _mixed(rng, lists, n)
    extra = [(int(a), int(b)) for a, b in rng.integers(0, n, (40, 2)) if a != b] + [(n, n + 1), (n + 3, n + 2), (n + 4, n)]
    for k, e in enumerate(extra):
        ranges.insert(7 * k + 3, e)
    omega = rng.uniform(0.5, 4.0, len(ranges))
    kw = {}
    if masks:
        kw = dict(pose_ok=rng.uniform(0, 1, n) < 0.7, landmark_on=np.array([1, 1, 0, 1, 1], dtype=bool))
    return ml.graph(d, poses, lms, ranges, noise=0.05, seed=d, omega=omega), kw, lens


def many(d):
    """300 landmarks of 4 .. 6 ranges each."""
    rng = np.random.default_rng(60 + d)
    n, nl = 400, 300
    poses = _walk(rng, n, d, 2.0)
    lms = poses[rng.integers(0, n, nl)] + 10 * rng.uniform(-1, 1, (nl, d))
    lists = [rng.choice(n, size=rng.integers(4, 7), replace=False) for _ in range(nl)]
    return ml.graph(d, poses, lms, _mixed(rng, lists, n), noise=0.02, seed=d), {}, None


def flat(d):
    """Anchors on a line (d = 2) / in a plane (d = 3) over 50 m: exactly (status 2), with a scatter of 0.3 (solved), with a
    scatter of 1e-4 (status 2); coincident anchors (status 2).  The reference's pivots are asserted 100 x away from 1e-8."""
    rng = np.random.default_rng(70 + d)
    k = 40
    groups = []
    for sigma in (0.0, 0.3, 1e-4):
        p = np.zeros((k, d))
        p[:, :d - 1] = rng.uniform(0, 50, (k, d - 1))
        p[:, d - 1] = sigma * rng.normal(0, 1, k)
        groups.append(p)
    groups.append(np.tile(np.array([3.0, 4.0, 5.0])[:d], (k, 1)))
    poses = np.concatenate(groups)
    lms = np.array([[20.0, 7.0, 9.0][:d]] * 4) + np.arange(4)[:, None]
    lists = [np.arange(g * k, (g + 1) * k) for g in range(4)]
    return ml.graph(d, poses, lms, _mixed(rng, lists, len(poses)), seed=d), {}, None


def exact_zero(d):
    """The landmark ON its first anchor, the other anchors at integer distances from it (Pythagorean vectors): every b is
    exactly zero, so y is exactly zero, r_0 = 0 and the estimate sits on an anchor (J_0 = 0).  A second landmark beside it."""
    offsets = {2: [[0, 0], [3, 4], [-4, 3], [5, 12], [8, -6]], 3: [[0, 0, 0], [3, 4, 0], [0, 3, 4], [2, 3, 6], [1, 4, 8], [2, 6, 9]]}
    poses = np.array(offsets[d], dtype=np.float64) + 3.0
    n = len(poses)
    lms = np.array([poses[0], poses[1] + 0.75])
    ranges = [(i, n) for i in range(n)] + [(n + 1, i) for i in range(n)]
    return ml.graph(d, poses, lms, ranges, seed=d), {}, None


def no_landmark(d):
    rng = np.random.default_rng(80 + d)
    poses = _walk(rng, 30, d)
    return ml.graph(d, poses, np.zeros((0, d)), [(i, (i + 7) % 30) for i in range(12)], seed=d), {}, None


def no_range(d):
    rng = np.random.default_rng(81 + d)
    return ml.graph(d, _walk(rng, 30, d), rng.normal(0, 1, (3, d)), [], seed=d), {}, None


def lonely(d):
    """A landmark with no range (status 3) between two that have ten."""
    rng = np.random.default_rng(82 + d)
    poses = _walk(rng, 30, d)
    lists = [np.arange(0, 10), np.arange(0), np.arange(12, 22)]
    return ml.graph(d, poses, 5 * rng.normal(0, 1, (3, d)), _mixed(rng, lists, 30), seed=d), {}, None


BUILDERS = dict(lengths=lengths, lengths_noisy=lambda d: lengths(d, noise=0.1), offset=lambda d: lengths(d, offset=1e6),
                noisy=noisy, masks=lambda d: noisy(d, masks=True), many=many, flat=flat, exact_zero=exact_zero,
                no_landmark=no_landmark, no_range=no_range, lonely=lonely)
SYNTHETIC = [(name, d) for name in BUILDERS for d in (2, 3)]


def case(name, d=None, device=-1):
    """(ctx, dims, table, X, masks, extra) of a synthetic case (name, d) or of a catalogue entry (d None), tables installed."""
    key = (name, d, device)
    if key not in _BUILT:
        if d is None:
            A, Q, dm, g = tp.build(name)
            dims, table = (dm.d, dm.n, dm.r, dm.n_trans), rr.table(g)
            X = np.array(A["truth"], dtype=np.float64)
            X[dm.d * dm.n + dm.r + dm.n:] = 77.25   # the landmarks' rows: a marker the solve must replace
            ctx = capi.Context(*dims, Q.rowptr, Q.col, Q.val, device=device)
            kw, extra = {}, None
        else:
            (dims, table, X), kw, extra = BUILDERS[name](d)
            ctx = capi.Context(*dims, *ml.diagonal_q(*dims), device=device)
        ctx.set_measurements(*table)
        ctx.set_multilateration(**kw)
        _BUILT[key] = (ctx, dims, table, X, kw, extra)
    return _BUILT[key]


def reference_of(name, d, gn):
    """Computed once and shared (tests/test_gpu_multilat.py reads the same)."""
    key = ("ref", name, d, gn)
    if key not in _BUILT:
        ctx, dims, table, X, kw, _ = case(name, d)
        _BUILT[key] = ml.reference(*dims, table, X, gn, **kw)
    return _BUILT[key]


def mirror_of(name, d, gn):
    key = ("mirror", name, d, gn)
    if key not in _BUILT:
        ctx, dims, table, X, kw, _ = case(name, d)
        _BUILT[key] = ctx.debug_multilaterate_host(X, gn)
    return _BUILT[key]


def check_case(name, d, gn):
    ctx, dims, table, X, kw, _ = case(name, d)
    dd, n, r, nt = dims
    t0 = dd * n + r
    ref, got = reference_of(name, d, gn), mirror_of(name, d, gn)
    assert ctx.multilateration_counts() == ref["counts"]
    worst = ml.check(got, *dims, table, ref)
    assert got["steps"] == ref["steps"]
    # rows of the poses and of the landmarks that are not solved keep their bits
    keep = np.ones(len(X), dtype=bool)
    keep[dd * n:t0] = False
    keep[t0 + n:] = ref["status"] != 0
    assert np.array_equal(ml.bits(got["X"][keep]), ml.bits(X[keep]))
    again = ctx.debug_multilaterate_host(X, gn)
    assert np.array_equal(ml.bits(again["X"]), ml.bits(got["X"])) and np.array_equal(ml.bits(again["cost_final"]), ml.bits(got["cost_final"]))
    kl = max([o["kappa_lin"] for o in ref["lm"]] + [0.0])
    kg = max([o["kappa_gn"] for o in ref["lm"]] + [0.0])
    print("%s d=%s gn=%d: solved %d of %d, steps %d, kappa(M) <= %.3g, kappa(H) <= %.3g, worst error / (eps kappa scale) %.3f"
          % (name, d, gn, got["solved"], nt - n, got["steps"], kl, kg, worst))
    return ref, got


@pytest.mark.parametrize("gn", (0, 5, 16))
@pytest.mark.parametrize("d", (2, 3))
def test_list_lengths_on_the_boundaries_of_the_reduction(d, gn):
    ref, got = check_case("lengths", d, gn)
    ctx, dims, table, X, _, extra = case("lengths", d)
    lens, truth = extra["lens"], extra["truth"]
    assert list(got["status"]) == [1, 0, 1] + [0] * 8
    assert ctx.multilateration_counts() == (len(lens), sum(lens), 0, sum((k + 255) // 256 for k in lens))
    assert sum((k + 255) // 256 for k in lens[-1:]) > 64
    # noise-free ranges in general position: the landmark is recovered.  The ranges of the table are the true distances
    # rounded to fp64, a perturbation of the size of the terms' own rounding: twice the bound.
    dd, n, r, nt = dims
    for l in np.flatnonzero(ref["status"] == 0):
        a, b = ref["bound"][l]
        for m in np.flatnonzero((table[2][:, 1:] == dd * n + r + n + l).any(axis=1))[:50]:
            pose = table[2][m, 1] + table[2][m, 2] - (dd * n + r + n + l)
            dist = np.linalg.norm(got["X"][dd * n + r + n + l] - X[pose])
            assert abs(dist - table[3][m, 0]) <= 2 * (ml.C_BOUND * a + b) + 4 * ml.EPS * dist, (l, m)
        assert np.linalg.norm(truth[l] - got["X"][dd * n + r + n + l]) <= 2 * (ml.C_BOUND * a + b)


@pytest.mark.parametrize("name,d", [c for c in SYNTHETIC if c[0] not in ("lengths", "flat", "exact_zero")])
def test_synthetic_cases(name, d):
    gn = 0 if name in ("no_landmark", "no_range") else 3 if name in ("noisy", "masks", "many") else 5
    ref, got = check_case(name, d, gn)
    ctx, dims, table, X, kw, _ = case(name, d)
    if name == "no_landmark":
        assert ctx.multilateration_counts() == (0, 0, 12, 0) and got["solved"] == got["not_solved"] == 0
    if name == "no_range":
        assert ctx.multilateration_counts() == (0, 0, 0, 0) and list(got["status"]) == [3, 3, 3]
    if name == "lonely":
        assert list(got["status"]) == [0, 3, 0] and ctx.multilateration_counts()[0] == 2
    if name in ("noisy", "masks"):
        assert ctx.multilateration_counts()[2] >= 40   # pose-pose and landmark-landmark ranges are skipped and counted
        assert (got["chosen"][got["status"] == 0] > 0).any()
    if name == "masks":
        assert got["status"][2] == 3 and ref["counts"][0] <= 4 and len(ml.lists_of(*dims, table[2], **kw)[0][2]) == 0
        assert sum(len(lst) for lst in ml.lists_of(*dims, table[2], **kw)[0]) < 0.8 * ref["counts"][1]
        assert ctx.multilateration_counts()[1] == case("noisy", d)[0].multilateration_counts()[1]
    if name == "many":
        assert got["solved"] >= 250
    if name == "offset":
        assert np.abs(X[dims[0] * dims[1] + dims[2]]).min() > 9e5


@pytest.mark.parametrize("gn", (0, 16))
@pytest.mark.parametrize("name,d", [c for c in SYNTHETIC if c[0] in ("noisy", "exact_zero")])
def test_no_step_and_sixteen_steps(name, d, gn):
    ref, got = check_case(name, d, gn)
    ctx, dims, table, X, kw, _ = case(name, d)
    assert got["steps"] <= gn * got["solved"]
    if gn == 0:
        assert not got["chosen"][got["status"] == 0].any()
    if name == "exact_zero":
        dd, n, r, nt = dims
        t0 = dd * n + r
        assert list(got["status"]) == [0, 0]
        if gn == 0:   # y is exactly zero: the row is the anchor's
            assert np.array_equal(ml.bits(got["X"][t0 + n]), ml.bits(X[t0])) and got["cost_linear"][0] == 0
        assert got["degenerate"][0] and got["n_degenerate"] >= 1


@pytest.mark.parametrize("d", (2, 3))
def test_flat_and_coincident_anchors(d):
    ref, got = check_case("flat", d, 5)
    assert list(got["status"]) == [2, 0, 2, 2]
    piv = [min(o["pivots"]) for o in ref["lm"][:3]]
    print("least pivots of the reference:", piv)
    assert piv[0] <= 1e-10 and piv[1] >= 1e-6 and piv[2] <= 1e-10
    assert ref["lm"][3]["L"] == 0.0


@pytest.mark.parametrize("name", CATALOGUE)
def test_catalogue(name):
    ref, got = check_case(name, None, 5)
    ctx, dims, table, X, _, _ = case(name)
    d, n, r, nt = dims
    with_lm = [m for m in range(len(table[2])) if (table[2][m, 1] >= d * n + r + n) != (table[2][m, 2] >= d * n + r + n)]
    assert ctx.multilateration_counts()[1] == len(with_lm) and sum(ctx.multilateration_counts()[1:3]) == len(table[2])
    if name == "lm_lm":
        assert ctx.multilateration_counts()[2] == 8
    if name == "pp_only":
        assert ctx.multilateration_counts()[:2] == (0, 0)


def _raises(code, fn, *a, **kw):
    with pytest.raises(capi.CoraError) as e:
        fn(*a, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_refusals():
    (dims, table, X), _, _ = lonely(2)
    ctx = capi.Context(*dims, *ml.diagonal_q(*dims), device=-1)
    assert "measurement table" in _raises(ERR_NOT_READY, ctx.set_multilateration)
    assert "measurement table" in _raises(ERR_NOT_READY, ctx.debug_multilaterate_host, X, 1)
    ctx.set_measurements(*table)
    assert "multilateration tables" in _raises(ERR_NOT_READY, ctx.debug_multilaterate_host, X, 1)
    ctx.set_multilateration()
    counts = ctx.multilateration_counts()
    _raises(ERR_ARG, ctx.debug_multilaterate_host, X, -1)
    _raises(ERR_ARG, ctx.debug_multilaterate_host, X, 17)
    _raises(ERR_ARG, ctx.set_multilateration, pose_ok=np.ones(3))
    nul = capi.C.c_void_p(None)
    out = (capi.C.c_int64 * 4)()
    assert ctx.L.cora_debug_multilaterate_host(ctx.h, nul, ctx.N, 1, out, nul, nul, nul, nul, nul) == ERR_ARG
    Xf = np.asfortranarray(X)
    assert ctx.L.cora_debug_multilaterate_host(ctx.h, capi._d(Xf), ctx.N - 1, 1, out, nul, nul, nul, nul, nul) == ERR_SHAPE
    # device forms on a plan-only handle
    _raises(ERR_HIP, ctx.multilaterate, X, 1)
    _raises(ERR_HIP, ctx.multilaterate_dev, 0, 1)
    # a refused call left the tables as they were; every array may be NULL
    rg2 = table[2].copy()
    assert ctx.multilateration_counts() == counts
    assert ctx.L.cora_debug_multilaterate_host(ctx.h, capi._d(Xf), ctx.N, 1, out, nul, nul, nul, nul, nul) == 0 and out[0] == 2
    # two range measurements that name one range row; a new measurement table drops the lists
    rg2[2, 0] = rg2[1, 0]
    ctx.set_measurements(table[0], table[1], rg2, table[3])
    assert ctx.multilateration_counts() == (0, 0, 0, 0)
    assert "range measurement 2" in _raises(ERR_ARG, ctx.set_multilateration)
    _raises(ERR_NOT_READY, ctx.debug_multilaterate_host, X, 1)
    # a sum that is not finite
    rd = table[3].copy()
    rd[0, 0] = 1e200
    ctx.set_measurements(table[0], table[1], table[2], rd)
    ctx.set_multilateration()
    _raises(ERR_NAN, ctx.debug_multilaterate_host, X, 1)


def test_partitioned_handles_are_refused():
    A, Q, dm, g = tp.build("robots-d2")
    p = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=2)
    assert "partitioned" in _raises(ERR_ARG, p.set_multilateration)
    _raises(ERR_ARG, p.debug_multilaterate_host, np.zeros((p.N, 2)), 1)
