"""The outlier-robust multilateration without a GPU: cora_debug_multilaterate_robust_host (the functions the kernels call, in
the device's bracket order, on plan-only handles) against the longdouble reference of tests/range_consensus_ref.py -- the
election unambiguous by the reference alone, then elected entry, consensus, statuses, flags and counts exactly and rows, costs
and the chosen point within multilat_ref's bound over the inliers -- on list lengths at the sample's and the reduction's edges,
on exact ranges whose outliers are the last entries (the plain call's bits on the graph without them), with a threshold nothing
exceeds (the plain call's bits), on contaminated hubs and a comb (the flags are the construction's), on degenerate lists, with
both masks, and every refusal.  The device forms against the mirror, bit for bit: tests/test_gpu_range_consensus.py.

Scale of the thresholds: sigma = 0.05 m, omega = 1 / sigma^2, outliers lengthened by 5 .. 20 m.  Under a clean hypothesis an
inlier's weighted squared residual stays below about 100 (ten sigma after the sample's geometry) and an outlier's above (5 /
0.05)^2 = 1e4 less what the hypothesis is off by, about 9e3; BARC2 is their geometric middle, and the hub and comb tests assert
on the reference's residuals that nothing lies within a factor of 2 of it."""
import numpy as np
import pytest

import multilat_ref as ml
import range_consensus_ref as rc
import topologies as tp
from cora_amd import capi

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
SIGMA = 0.05
BARC2 = 950.0   # sqrt(100 x 9e3)
bits = ml.bits

_BUILT = {}


def _table(d, poses, lms, lists, bad, rng, noise=SIGMA, shuffle=True):
    """A graph of ranges over lists (landmark -> pose indices, in list order) with the entries flagged in bad (landmark -> bool
    per entry) lengthened by 5 .. 20 m; the table order is shuffled between the lists (never within one) and every other range
    is stored landmark -> pose.  Returns (dims, table, X), good: per range measurement 1 (as measured) | 0 (lengthened)."""
    n = len(poses)
    per = [[(int(p), n + l, bool(b)) for p, b in zip(ps, bad[l])] for l, ps in enumerate(lists)]
    order = []
    at = [0] * len(per)
    pick = np.concatenate([np.full(len(p), l) for l, p in enumerate(per)]) if per else np.zeros(0, dtype=int)
    if shuffle and len(pick):
        pick = pick[rng.permutation(len(pick))]
    for l in pick:
        order.append(per[l][at[l]])
        at[l] += 1
    ranges = [(b, a) if m % 2 else (a, b) for m, (a, b, _) in enumerate(order)]
    good = np.array([0 if o[2] else 1 for o in order], dtype=np.uint8)
    dims, table, X = ml.graph(d, poses, lms, ranges, noise=noise, seed=int(rng.integers(1 << 30)), omega=np.full(len(ranges), 1 / SIGMA ** 2))
    table[3][good == 0, 0] += rng.uniform(5, 20, int(np.sum(good == 0)))
    return (dims, table, X), good


def _outliers(rng, k, share):
    bad = np.zeros(k, dtype=bool)
    bad[rng.choice(k, size=int(share * k), replace=False)] = True
    return bad


def lens_of(d):
    return [d + 1, d + 2, 2 * (d + 1) - 1, 2 * (d + 1), 63, 64, 65, 255, 256, 257, 513]


def lengths(d, seed=None):
    """Lists at the sample's edges (d + 1: s = 1 and every sample is the whole list; d + 2; 2 (d + 1) - 1; 2 (d + 1): s = 2) and at
    the reduction's (63 .. 513), anchors uniform in a 20 m box.  30 % outliers where the scheme carries them (from 63 entries at
    d = 2, from 255 at d = 3), 10 % in the lists of 63 .. 65 at d = 3, none in the short lists (they have no consensus above
    d + 1, or just one)."""
    rng = np.random.default_rng({2: 101, 3: 103}[d] if seed is None else seed)
    lens = lens_of(d)
    n = 700
    poses = rng.uniform(0, 20, (n, d))
    lms = rng.uniform(0, 20, (len(lens), d))
    lists = [rng.choice(n, size=k, replace=False) for k in lens]
    share = lambda k: 0.0 if k < 63 else 0.3 if (d == 2 or k >= 255) else 0.1
    bad = [_outliers(rng, k, share(k)) for k in lens]
    return _table(d, poses, lms, lists, bad, rng), {}, dict(lens=lens, truth=lms)


def hubs(d, seed=None):
    """Three landmarks seen from 300 poses each of a 3 m-step walk, 30 % of the ranges lengthened."""
    rng = np.random.default_rng({2: 201, 3: 204}[d] if seed is None else seed)
    n = 400
    poses = np.cumsum(3.0 * rng.normal(0, 1, (n, d)) / np.sqrt(d), axis=0)
    lms = poses[rng.integers(0, n, 3)] + 10 * rng.uniform(-1, 1, (3, d))
    lists = [rng.choice(n, size=300, replace=False) for _ in range(3)]
    bad = [_outliers(rng, 300, 0.3) for _ in range(3)]
    return _table(d, poses, lms, lists, bad, rng), {}, dict(truth=lms)


def comb(d=2, seed=None):
    """60 landmarks of 8 ranges each, one of them lengthened (d = 2)."""
    rng = np.random.default_rng(310 if seed is None else seed)
    n, nl = 200, 60
    poses = rng.uniform(0, 20, (n, d))
    lms = rng.uniform(0, 20, (nl, d))
    lists = [rng.choice(n, size=8, replace=False) for _ in range(nl)]
    bad = [_outliers(rng, 8, 1 / 8) for _ in range(nl)]
    return _table(d, poses, lms, lists, bad, rng), {}, dict(truth=lms)


def degenerate(d, masks=False):
    """0: 40 collinear anchors (no valid hypothesis: consensus 0, status 5, every flag 0); 1: 12 ranges, 9 of them lengthened (the
    consensus stays below min_consensus = 6: status 5); 2: d ranges (status 1); 3: no range (status 3); 4: a clean list of 30; 5: a
    list of 30 with 6 lengthened.  masks: landmark 4 off, a third of the poses not ok."""
    rng = np.random.default_rng(400 + d)
    n = 200
    poses = rng.uniform(0, 20, (n, d))
    poses[:40] = np.outer(np.linspace(0, 30, 40), np.ones(d) / np.sqrt(d)) + 3.0
    lms = rng.uniform(0, 20, (6, d))
    lists = [np.arange(40), rng.choice(np.arange(40, n), 12, replace=False), np.array([41, 44, 47])[:d], np.arange(0),
             rng.choice(np.arange(40, n), 30, replace=False), rng.choice(np.arange(40, n), 30, replace=False)]
    bad = [np.zeros(40, dtype=bool), _outliers(rng, 12, 0.75), np.zeros(d, dtype=bool), np.zeros(0, dtype=bool), np.zeros(30, dtype=bool),
           _outliers(rng, 30, 0.2)]
    kw = {}
    if masks:
        ok = np.ones(n, dtype=bool)
        ok[40::3] = False
        kw = dict(pose_ok=ok, landmark_on=np.array([1, 1, 1, 1, 0, 1], dtype=bool))
    return _table(d, poses, lms, lists, bad, rng), kw, dict(truth=lms, vote=dict(min_consensus=6))


def trailing(d):
    """Exact ranges; the lengthened ones are the LAST entries of their lists: 40 + 5, 256 + 1 (one chunk becomes two: the second
    holds the outlier alone), 250 + 10 and 600 + 30.  The table is not shuffled within a list, so the lists of the graph without the
    lengthened ranges are these lists' heads."""
    rng = np.random.default_rng(500 + d)
    sizes = [(40, 5), (256, 1), (250, 10), (600, 30)]
    n = 700
    poses = rng.uniform(0, 20, (n, d))
    lms = rng.uniform(0, 20, (len(sizes), d))
    lists = [rng.choice(n, size=a + b, replace=False) for a, b in sizes]
    bad = [np.arange(a + b) >= a for a, b in sizes]
    return _table(d, poses, lms, lists, bad, rng, noise=0.0), {}, dict(sizes=sizes, lists=lists, poses=poses, lms=lms)


def long_list():
    """One list of 16 385 entries at d = 2 (65 chunks: the vote's walk and the fold's lanes go round twice; the election's stride
    loop runs 257 times), 30 % lengthened."""
    rng = np.random.default_rng(600)
    n = 16500
    poses = rng.uniform(0, 20, (n, 2))
    lists = [rng.choice(n, size=16385, replace=False)]
    return _table(2, poses, rng.uniform(0, 20, (1, 2)), lists, [_outliers(rng, 16385, 0.3)], rng), {}, None


BUILDERS = dict(lengths=lengths, hubs=hubs, comb=comb, degenerate=degenerate, masks=lambda d: degenerate(d, masks=True), trailing=trailing)
CASES = [(name, d) for name in ("lengths", "hubs", "degenerate", "masks", "trailing") for d in (2, 3)] + [("comb", 2)]


def case(name, d, device=-1):
    """(ctx, dims, table, X, masks, good, extra) of a case, tables installed."""
    key = (name, d, device)
    if key not in _BUILT:
        ((dims, table, X), good), kw, extra = long_list() if name == "long" else BUILDERS[name](d)
        ctx = capi.Context(*dims, *ml.diagonal_q(*dims), device=device)
        ctx.set_measurements(*table)
        ctx.set_multilateration(**kw)
        _BUILT[key] = (ctx, dims, table, X, kw, good, extra)
    return _BUILT[key]


def vote_of(name, d):
    extra = case(name, d)[6]
    return dict(extra.get("vote", {})) if extra else {}


def reference_of(name, d, gn):
    """Computed once and shared (tests/test_gpu_range_consensus.py reads the same); the vote does not depend on gn."""
    key = ("ref", name, d, gn)
    if key not in _BUILT:
        ctx, dims, table, X, kw, _, _ = case(name, d)
        other = _BUILT.get(("ref", name, d, 5 - gn))
        _BUILT[key] = rc.reference(*dims, table, X, gn, BARC2, **vote_of(name, d), **kw, votes=other["votes"] if other else None)
    return _BUILT[key]


def mirror_of(name, d, gn):
    key = ("mirror", name, d, gn)
    if key not in _BUILT:
        ctx, dims, table, X, kw, _, _ = case(name, d)
        _BUILT[key] = ctx.debug_multilaterate_robust_host(X, BARC2, gn, **vote_of(name, d))
    return _BUILT[key]


def margins(ref):
    """(largest residual of an inlier, least residual of an entry outside) under the elected hypotheses of the voted lists."""
    inside, outside = [0.0], [np.inf]
    for vote in ref["votes"]:
        if vote is None or vote["consensus"] == 0:
            continue
        r = np.asarray(vote["hyp"][vote["elected"]]["r"], dtype=np.float64)
        inside.append(r[vote["inlier"]].max(initial=0.0))
        outside.append(r[~vote["inlier"]].min(initial=np.inf))
    return max(inside), min(outside)


@pytest.mark.parametrize("gn", (0, 5))
@pytest.mark.parametrize("name,d", CASES)
def test_mirror_on_the_cases(name, d, gn):
    ctx, dims, table, X, kw, good, extra = case(name, d)
    dd, n, r, nt = dims
    t0 = dd * n + r
    ref, got = reference_of(name, d, gn), mirror_of(name, d, gn)
    # the condition on a committed case, by the reference alone
    assert ref["ambiguous"] == [] and ref["band"] == [], (ref["ambiguous"][:3], ref["band"][:3])
    worst = rc.check(got, *dims, table, ref)
    assert got["steps"] == ref["steps"]
    keep = np.ones(len(X), dtype=bool)   # rows of the poses and of the landmarks that are not solved keep their bits
    keep[dd * n:t0] = False
    keep[t0 + n:] = ref["status"] != 0
    assert np.array_equal(bits(got["X"][keep]), bits(X[keep]))
    solved = got["status"] == 0
    assert np.all(got["cost_final"][solved] <= got["cost_linear"][solved])   # never worse, as doubles
    lo, hi = margins(ref)
    print("%s d=%d gn=%d: statuses %s consensus %s of %s; worst error / (a + b) %.4f; residuals inside <= %.4g, outside >= %.4g"
          % (name, d, gn, got["status"][:12], got["consensus"][:12], got["list_len"][:12], worst, lo, hi))
    if name == "lengths":
        lens = extra["lens"]
        assert list(got["list_len"]) == lens and ctx.multilateration_counts()[3] == sum((k + 255) // 256 for k in lens)
        assert got["status"][0] == 5 and got["consensus"][0] == d + 1     # every sample is the whole list: d + 1 votes, no more
        assert np.all(got["status"][4:] == 0)
        assert list(got["consensus"][7:]) == [k - int(0.3 * k) for k in lens[7:]]
        for l in range(7, len(lens)):
            assert np.linalg.norm(got["X"][t0 + n + l] - extra["truth"][l]) < 0.1
    if name in ("hubs", "comb"):   # the flags are the construction's, and nothing is near the threshold
        assert np.array_equal(got["inlier"], good) and got["excluded"] == int(np.sum(good == 0)) and got["no_consensus"] == 0
        assert np.all(got["status"] == 0)
        assert lo <= BARC2 / 2 and hi >= 2 * BARC2, (lo, hi)
        assert np.linalg.norm(got["X"][t0 + n:] - extra["truth"], axis=1).max() < (0.1 if name == "hubs" else 0.5)
    if name in ("degenerate", "masks"):
        lists = ml.lists_of(*dims, table[2], **kw)[0]
        expect = [5, 5, 1, 3, 0, 0] if name == "degenerate" else [5, 5, 1, 3, 3, 0]
        assert list(got["status"]) == expect, got["status"]
        assert got["consensus"][0] == 0 and got["elected"][0] == 0 and not got["inlier"][[m for _, m in lists[0]]].any()
        assert got["consensus"][1] < 6 and got["inlier"][[m for _, m in lists[1]]].sum() == got["consensus"][1]
        assert got["elected"][2] == got["elected"][3] == -1 and got["consensus"][2] == got["consensus"][3] == 0
        ms2 = [m for m in range(len(table[2])) if (table[2][m, 1:] == t0 + n + 2).any()]
        assert np.all(got["inlier"][ms2] == 2)                            # a list that is too short: byte 2
        assert got["no_consensus"] == 2
        if name == "masks":
            ms4 = [m for m in range(len(table[2])) if (table[2][m, 1:] == t0 + n + 4).any()]
            assert np.all(got["inlier"][ms4] == 2) and got["elected"][4] == -1
            masked = [m for m in range(len(table[2])) if not kw["pose_ok"][min(table[2][m, 1:]) - t0]]
            assert len(masked) > 10 and np.all(got["inlier"][masked] == 2)
            assert got["list_len"][5] < 30
        assert np.array_equal(got["inlier"][[m for _, m in lists[5]]], good[[m for _, m in lists[5]]])


@pytest.mark.parametrize("gn", (0, 5))
@pytest.mark.parametrize("d", (2, 3))
def test_trailing_outliers_give_the_plain_bits_of_the_graph_without_them(d, gn):
    """An entry outside I adds +0.0 for each of its terms, as the lane beyond the shorter list's end does: rows, costs and the
    chosen point of the robust call ARE the plain call's on the graph without the lengthened ranges -- across 256 -> 257 with
    the trailing chunk that holds nothing but the outlier."""
    ctx, dims, table, X, kw, good, extra = case("trailing", d)
    got = mirror_of("trailing", d, gn)
    heads = [lst[:a] for lst, (a, b) in zip(extra["lists"], extra["sizes"])]
    rng = np.random.default_rng(1)
    (cdims, ctable, cX), _ = _table(d, extra["poses"], extra["lms"], heads, [np.zeros(len(h), dtype=bool) for h in heads], rng, noise=0.0)
    plain_ctx = capi.Context(*cdims, *ml.diagonal_q(*cdims), device=-1)
    plain_ctx.set_measurements(*ctable)
    plain_ctx.set_multilateration()
    assert plain_ctx.multilateration_counts()[3] == 1 + 1 + 1 + 3 and ctx.multilateration_counts()[3] == 1 + 2 + 2 + 3
    plain = plain_ctx.debug_multilaterate_host(cX, gn)
    n = dims[1]
    assert list(got["consensus"]) == [a for a, _ in extra["sizes"]] and np.array_equal(got["inlier"], good)
    assert np.array_equal(bits(got["X"][dims[0] * n + dims[2] + n:]), bits(plain["X"][cdims[0] * n + cdims[2] + n:]))
    for key in ("cost_linear", "cost_final"):
        assert np.array_equal(bits(got[key]), bits(plain[key])), key
    assert np.array_equal(got["chosen"], plain["chosen"]) and np.array_equal(got["status"], plain["status"]) and got["steps"] == plain["steps"]


@pytest.mark.parametrize("name,d", [("lengths", 2), ("lengths", 3), ("degenerate", 2), ("masks", 3), ("hubs", 3)])
def test_a_threshold_nothing_exceeds_gives_the_plain_bits(name, d):
    """barc2 = 1e300: every finite residual agrees, so wherever a list has a valid hypothesis the consensus is its length, I the
    whole list, and the landmark has the plain call's bits."""
    ctx, dims, table, X, kw, _, _ = case(name, d)
    got, plain = ctx.debug_multilaterate_robust_host(X, 1e300, 5, min_consensus=1), ctx.debug_multilaterate_host(X, 5)
    full = (got["consensus"] == got["list_len"]) & (got["elected"] >= 0)
    assert full.sum() >= 2
    t0n = dims[0] * dims[1] + dims[2] + dims[1]
    assert np.array_equal(bits(got["X"][t0n:][full]), bits(plain["X"][t0n:][full]))
    for key in ("cost_linear", "cost_final"):
        assert np.array_equal(bits(got[key][full]), bits(plain[key][full])), key
    assert np.array_equal(got["chosen"][full], plain["chosen"][full]) and np.array_equal(got["status"][full], plain["status"][full])
    assert np.all(got["status"][~full & (got["elected"] >= 0)] == 5)
    # and the plain call between two robust ones keeps its bits and the tables
    again = ctx.debug_multilaterate_host(X, 5)
    assert np.array_equal(bits(again["X"]), bits(plain["X"])) and np.array_equal(bits(again["cost_final"]), bits(plain["cost_final"]))


def test_a_list_of_16385_entries():
    """The mirror alone (no longdouble reference at this length): the elected hypothesis has the construction's inliers."""
    ctx, dims, table, X, kw, good, _ = case("long", 2)
    got = mirror_of("long", 2, 5)
    assert ctx.multilateration_counts()[3] == 65
    assert got["list_len"][0] == 16385 and got["consensus"][0] == int(np.sum(good == 1)) == 16385 - int(0.3 * 16385)
    assert np.array_equal(got["inlier"], good) and got["status"][0] == 0 and 0 <= got["elected"][0] < 16385
    assert got["cost_final"][0] <= got["cost_linear"][0]


def test_the_bound_constant_is_four_times_the_measured_ratio():
    """C_BOUND's measurement (range_consensus_ref.measure_constant) over the cases of this file."""
    new = lambda dims: capi.Context(*dims, *ml.diagonal_q(*dims), device=-1)
    worst = 0.0
    for name, d in CASES:
        ctx, dims, table, X, kw, _, _ = case(name, d)
        ratio = rc.measure_constant(new, *dims, table, X, **kw)
        print("%s d=%d: worst |y_mirror - y_ref| / a %.4f" % (name, d, ratio))
        worst = max(worst, ratio)
    print("worst ratio %.4f; C_BOUND %.3g" % (worst, rc.C_BOUND))
    assert 4 * worst <= rc.C_BOUND


def robust_refusals(ctx_of, call, raw, has_ldx=True):
    """The error paths of one form of the robust call (shared with tests/test_gpu_range_consensus.py): ctx_of(dims) a fresh
    handle, call(ctx, X, gn, barc2, min_consensus), raw(ctx): the C function and how it takes the vector (and its leading
    dimension, has_ldx)."""
    ((dims, table, X), _), _, _ = comb()
    ctx = ctx_of(dims)

    def code(*a):
        with pytest.raises(capi.CoraError) as e:
            call(ctx, *a)
        return e.value.code
    assert code(X, 1, BARC2, 4) == ERR_NOT_READY          # no measurement table
    ctx.set_measurements(*table)
    assert code(X, 1, BARC2, 4) == ERR_NOT_READY          # no multilateration tables
    ctx.set_multilateration()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert code(X, 1, bad, 4) == ERR_ARG
    assert code(X, 1, BARC2, 0) == ERR_ARG
    assert code(X, -1, BARC2, 4) == ERR_ARG and code(X, 17, BARC2, 4) == ERR_ARG
    fn, lead = raw(ctx)
    out = (capi.C.c_int64 * 6)()
    Xf = np.asfortranarray(X)
    none = [None] * 9
    bar = capi.C.c_double(BARC2)
    if has_ldx:
        assert fn(ctx.h, *lead(Xf, ctx.N - 1), 1, bar, 4, out, *none) == ERR_SHAPE
    assert fn(ctx.h, *lead(None, ctx.N), 1, bar, 4, out, *none) == ERR_ARG
    assert fn(ctx.h, *lead(Xf, ctx.N), 1, bar, 4, None, *none) == ERR_ARG
    assert fn(ctx.h, *lead(Xf, ctx.N), 1, bar, 4, out, *none) == 0 and list(out)[:2] == [60, 0] and list(out)[4:] == [0, 60]   # every output may be NULL
    return ctx


def nan_case():
    """The comb with a NaN in the position of a pose that several lists range to."""
    ((dims, table, X), _), _, _ = comb()
    X = X.copy()
    pose = int(min(table[2][0, 1:])) - (dims[0] * dims[1] + dims[2])
    X[dims[0] * dims[1] + dims[2] + pose, 0] = np.nan
    return dims, table, X


def test_refusals():
    ctx = robust_refusals(lambda dims: capi.Context(*dims, *ml.diagonal_q(*dims), device=-1),
                          lambda ctx, X, gn, b, m: ctx.debug_multilaterate_robust_host(X, b, gn, m),
                          lambda ctx: (ctx.L.cora_debug_multilaterate_robust_host, lambda X, ldx: (None if X is None else capi._d(X), ldx)))
    ((dims, table, X), _), _, _ = comb()
    for form in (lambda: ctx.multilaterate_robust(X, BARC2), lambda: ctx.multilaterate_robust_dev(0, BARC2)):
        with pytest.raises(capi.CoraError) as e:
            form()                                     # a device form on a plan-only handle
        assert e.value.code == ERR_HIP
    dims, table, X = nan_case()
    with pytest.raises(capi.CoraError) as e:
        ctx.debug_multilaterate_robust_host(X, BARC2)
    assert e.value.code == ERR_NAN


def test_partitioned_handles_are_refused():
    A, Q, dm, g = tp.build("robots-d2")
    p = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=2)
    with pytest.raises(capi.CoraError) as e:
        p.debug_multilaterate_robust_host(np.zeros((p.N, 2)), BARC2)
    assert e.value.code == ERR_ARG and "partitioned" in str(e.value)


def test_range_consensus_validation_of_the_host_interface():
    """host.Problem.range_aided_initialization refuses a threshold that is not positive before it reaches the library (None is
    the plain call: tests/test_gpu_range_consensus.py compares its bits on the device)."""
    from cora_amd import host
    P = host.Problem.synthetic(dim=2, n_poses=30, n_landmarks=2, n_ranges=20, seed=1)
    P.update()
    for bad in (0.0, -3.0, float("nan")):
        with pytest.raises(host.HostError):
            P.range_aided_initialization(consensus_barc2=bad)
