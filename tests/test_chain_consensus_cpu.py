"""The outlier-robust chain placement without a GPU: cora_debug_place_chains_robust_host (the functions the kernels call, in
the device's bracket order, on plan-only handles) against the longdouble reference of tests/chain_consensus_ref.py -- elected
entry, consensus, statuses and inlier bytes exactly, transforms, rows and costs within placement_ref's bound over the inliers
-- on hubs with 10 % lengthened ranges whose lists sit on the chunk edges (m, m + 1, 255, 256, 257, 513), under greedy and
level tables, on a relay whose middle chain lies on a line (every sample degenerate: consensus 0, status 5, and the chain
behind it still placed), with a list below min_consensus next to lists above it in one level, on exact ranges, on a NaN, with
every refusal; a clean hub against the plain mirror bit for bit; the constant of the score bound.  A committed case passes
chain_consensus_ref.committed BY THE REFERENCE ALONE (seeds that miss it were passed over: profiles/chain_consensus.md).  The
device forms against the mirror, bit for bit: tests/test_gpu_chain_consensus.py."""
import numpy as np
import pytest

import chain_consensus_ref as cc
import placement_ref as pl
import topologies as tp
from cora_amd import capi
from test_placement_cpu import _pairs

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
BARC2 = 950.0   # (as the range-consensus cases: sigma = 0.05, omega = 1 / sigma^2 = 400, so |e| <= 1.54 m)
SIGMA = 0.05
bits = pl.bits
_BUILT = {}


def least(d):
    return cc.terms(d)


LINE_SEED = {2: 0, 3: 1}   # (d = 3: seed 0 has a refused hypothesis with a pivot in its band of the rule)


def hub_lens(d):
    return [least(d), least(d) + 1, 255, 256, 257, 513]


def _contaminate(rng, table, ranges, first, share=0.1):
    """Lengthens `share` of the ranges whose chain end lies at or after pose `first` by +5 .. 20 m; returns the mask."""
    rd = table[3]
    bad = np.array([max(a, b) >= first for a, b in ranges]) & (rng.random(len(ranges)) < share)
    rd[bad, 0] += rng.uniform(5, 20, int(bad.sum()))
    return bad


def hub(d, seed=0, share=0.1, noise=SIGMA):
    """Chain 0 of 30 poses, fixed, and six chains of 40 with lists of m, m + 1, 255, 256, 257 and 513 entries against it, one
    level of six stages: 10 % of the ranges of the four long lists lengthened by +5 .. 20 m.  The two short lists are clean;
    their consensus (at most m + 1) is below the default min_consensus 2 m: status 5 next to four lists above it."""
    rng = np.random.default_rng(500 + 10 * seed + d)
    lens = hub_lens(d)
    ranges = []
    for c, k in enumerate(lens):
        ranges += _pairs(rng, 0, 30, 30 + 40 * c, 40, k)
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    sc = pl.scene(d, [30] + [40] * len(lens), ranges, seed=200 + seed + d, noise=noise, omega=[1 / SIGMA ** 2] * len(ranges))
    bad = _contaminate(rng, sc[1], ranges, 30 + 40 * 2, share)
    return sc, dict(min_ranges=least(d)), dict(bad=bad, lens=lens)


def clean_hub(d):
    return hub(d, share=0.0)


def exact(d):
    """A - B - C with exact ranges and no outlier: every valid hypothesis has the whole list's votes."""
    rng = np.random.default_rng(520 + d)
    ranges = _pairs(rng, 0, 30, 30, 30, 40) + _pairs(rng, 30, 30, 60, 30, 45)
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    sc = pl.scene(d, [30] * 3, ranges, seed=220 + d, omega=[1 / SIGMA ** 2] * len(ranges))
    return sc, dict(min_ranges=least(d)), dict(bad=np.zeros(len(ranges), dtype=bool))


def line(d, seed=None):
    """A - B - C, B's positions on a line (in its own frame: exactly): every sample of B's list is refused by the linear stage,
    B elects entry 0 with consensus 0 and keeps its rows (status 5); C, with 70 ranges against A (below min_ranges = 80) and 20
    against B, stands a level behind B, anchors on B's rows as they are and is still placed.  (A list against B alone would be
    degenerate too: its anchors lie on the line; a sample needs about eight anchors off it at d = 3.)"""
    seed = LINE_SEED[d] if seed is None else seed   # (seeds passed over: profiles/chain_consensus.md)
    rng = np.random.default_rng(530 + 10 * seed + d)
    world = [np.cumsum(rng.normal(0, 3, (30, d)), axis=0), np.zeros((30, d)), 20 + np.cumsum(rng.normal(0, 3, (30, d)), axis=0)]
    world[1][:, 0] = np.arange(30) * 2.0
    ranges = _pairs(rng, 0, 30, 30, 30, 80) + _pairs(rng, 30, 30, 60, 30, 20) + _pairs(rng, 0, 30, 60, 30, 70)
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    sc = pl.scene(d, [30] * 3, ranges, seed=230 + d, noise=SIGMA, omega=[1 / SIGMA ** 2] * len(ranges), world=np.concatenate(world),
                  moved=[False, False, True])
    bad = _contaminate(rng, sc[1], ranges, 60)
    return sc, dict(min_ranges=80), dict(bad=bad)


BUILDERS = dict(hub=hub, clean_hub=clean_hub, exact=exact, line=line)
CASES = [(name, d) for name in BUILDERS for d in (2, 3)]


def case(name, d, order=cc.LEVELS, device=-1):
    key = (name, d, order, device)
    if key not in _BUILT:
        (dims, table, X, chains, truth), kw, extra = BUILDERS[name](d)
        ctx = capi.Context(*dims, *pl.diagonal_q(*dims), device=device)
        ctx.set_measurements(*table)
        ctx.set_odometry_chains(chains)
        ctx.set_chain_placement_order(order=order, **kw)
        _BUILT[key] = (ctx, dims, table, X, chains, kw, extra, truth)
    return _BUILT[key]


def mirror_of(name, d, gn=5, order=cc.LEVELS, min_consensus=None):
    key = ("mirror", name, d, gn, order, min_consensus)
    if key not in _BUILT:
        ctx, dims, table, X = case(name, d, order)[:4]
        got = ctx.debug_place_chains_robust_host(X, BARC2, gn, min_consensus)
        got["X_in"] = X
        _BUILT[key] = got
    return _BUILT[key]


def reference_of(name, d, gn=5, order=cc.LEVELS, min_consensus=None):
    """The reference of a case; the vote (which does not depend on gn_steps or min_consensus) is computed once per (case, order)."""
    key = ("ref", name, d, gn, order, min_consensus)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw = case(name, d, order)[:6]
        votes = _BUILT.get(("votes", name, d, order))
        ref = cc.reference(*dims, table, chains, X, gn, BARC2, min_consensus, order=order, votes=votes, **kw)
        _BUILT[("votes", name, d, order)] = ref["votes"]
        _BUILT[key] = ref
    return _BUILT[key]


def same(a, b, keys):
    for key in keys:
        x, y = a[key], b[key]
        if isinstance(x, np.ndarray) and x.dtype == np.float64:
            assert np.array_equal(bits(x), bits(y)), key
        else:
            assert np.array_equal(x, y), key


PLAIN_KEYS = ("X", "status", "chosen", "degenerate", "cost_start", "cost_linear", "cost_final", "transforms", "placed", "not_placed", "steps",
              "n_degenerate", "stages")
ROBUST_KEYS = PLAIN_KEYS + ("levels", "no_consensus", "excluded", "elected", "consensus", "list_len", "inlier")


@pytest.mark.parametrize("name,d", CASES)
def test_mirror_against_the_reference(name, d):
    dims, table = case(name, d)[1:3]
    ref = reference_of(name, d)
    got = mirror_of(name, d)
    worst = cc.check(got, *dims, table, ref)
    shares = [(len(v["hyp"]), v["valid"]) for v in ref["votes"]]
    print("%s d=%d: worst error / (a + b) %.4f; consensus %s of %s; valid hypotheses %s; margins %.3g / %.3g of barc2; statuses %s" %
          (name, d, worst, got["consensus"], got["list_len"], shares, ref["margin"][0], ref["margin"][1], got["status"]))


@pytest.mark.parametrize("d", (2, 3))
def test_the_hub_finds_the_lengthened_ranges(d):
    """The inlier bytes are the truth's on the four long lists: every lengthened range is excluded and no other; the two short
    lists stay below min_consensus in the same level and keep their rows, bit for bit."""
    ctx, dims, table, X, chains, kw, extra, truth = case("hub", d)
    got = mirror_of("hub", d)
    m = least(d)
    assert list(got["status"]) == [4, 5, 5, 0, 0, 0, 0] and list(got["list_len"]) == [0] + extra["lens"]
    assert list(got["consensus"][1:3]) == [m, m + 1] and got["no_consensus"] == 2 and got["not_placed"] == 2 and got["levels"] == 1
    rr = np.asarray(table[2])
    t0 = dims[0] * dims[1] + dims[2]
    long_list = np.array([max(a, b) - t0 >= 30 + 40 * 2 for a, b in rr[:, 1:]])
    assert np.array_equal(got["inlier"][long_list] == 0, extra["bad"][long_list]) and extra["bad"].sum() > 100
    assert np.all(got["inlier"][~long_list] == 1)
    for c in (1, 2):   # no consensus: the caller's bits
        rows = slice(t0 + 30 + 40 * (c - 1), t0 + 30 + 40 * c)
        assert np.array_equal(bits(got["X"][rows]), bits(X[rows]))
        assert got["chosen"][c] == -1 and got["cost_final"][c] == 0
    # the placed chains are at the noise level; the plain call's are metres off
    plain = ctx.debug_place_chains_host(X, 5)
    for c in range(3, 7):
        R, t = truth[c]
        rows = slice(t0 + 30 + 40 * (c - 1), t0 + 30 + 40 * c)
        world = X[rows] @ R.T + t
        err_r, err_p = np.linalg.norm(got["X"][rows] - world, axis=1).max(), np.linalg.norm(plain["X"][rows] - world, axis=1).max()
        print("d=%d chain %d: robust %.3g m, plain %.3g m" % (d, c, err_r, err_p))
        assert err_r < 10 * SIGMA and err_p > 10 * err_r


@pytest.mark.parametrize("d", (2, 3))
def test_short_lists_with_min_consensus_one(d):
    """min_consensus 1: the lists of m and m + 1 entries are fitted too (consensus m, m + 1), against the reference."""
    dims, table = case("hub", d)[1:3]
    got, ref = mirror_of("hub", d, 5, cc.LEVELS, 1), reference_of("hub", d, 5, cc.LEVELS, 1)
    cc.check(got, *dims, table, ref)
    assert got["no_consensus"] == 0 and np.all(got["status"][1:] != 5)


@pytest.mark.parametrize("name,d", [("hub", 2), ("hub", 3), ("line", 2), ("line", 3)])
def test_greedy_and_level_tables(name, d):
    """The same problem under both orders: every chain ranges only against earlier levels, so the lists coincide and so do the
    bits; the greedy tables hold one stage per level."""
    a, b = mirror_of(name, d, 5, cc.LEVELS), mirror_of(name, d, 5, cc.GREEDY)
    same(a, b, [k for k in ROBUST_KEYS if k != "levels"])
    assert (a["levels"], b["levels"]) == ((2, 2) if name == "line" else (1, 6))
    dims, table = case(name, d, cc.GREEDY)[1:3]
    cc.check(b, *dims, table, reference_of(name, d, 5, cc.GREEDY))


@pytest.mark.parametrize("d", (2, 3))
def test_a_line_has_no_consensus_and_the_chain_behind_it_is_placed(d):
    got = mirror_of("line", d)
    ref = reference_of("line", d)
    assert list(got["status"]) == [4, 5, 0] and list(got["consensus"][:2]) == [0, 0] and list(got["elected"][:2]) == [-1, 0]
    assert ref["votes"][0]["valid"] == 0 and got["consensus"][2] >= 2 * least(d) and list(got["list_len"]) == [0, 80, 90]
    ctx, dims, table, X, chains, kw, extra, truth = case("line", d)
    rr, t0 = np.asarray(table[2]), dims[0] * dims[1] + dims[2]
    to_a = (rr[:, 1:].min(axis=1) - t0 < 30) & (rr[:, 1:].max(axis=1) - t0 < 60)   # B's list: its 80 ranges against A
    assert to_a.sum() == 80 and np.all(got["inlier"][to_a] == 0) and np.all(got["inlier"][~to_a] != 2)
    assert np.array_equal(got["inlier"][~to_a] == 0, extra["bad"][~to_a]) and extra["bad"].sum() >= 5   # C's list: the lengthened ranges
    rows = slice(t0 + 30, t0 + 60)
    assert np.array_equal(bits(got["X"][rows]), bits(X[rows]))   # B keeps the caller's bits
    R, t = truth[2]
    rows = slice(t0 + 60, t0 + 90)
    assert np.linalg.norm(got["X"][rows] - (X[rows] @ R.T + t), axis=1).max() < 10 * SIGMA


@pytest.mark.parametrize("d", (2, 3))
def test_a_clean_hub_has_the_plain_call_s_bits(d):
    """No outlier: I is the whole list, every masked sum is the plain sum, and X, costs, chosen, transforms and out[0..5] are
    cora_debug_place_chains_host's on the same tables, bit for bit; every inlier byte of a stage list is 1."""
    ctx, dims, table, X = case("clean_hub", d)[:4]
    got = mirror_of("clean_hub", d, 5, cc.LEVELS, 1)
    plain = ctx.debug_place_chains_host(X, 5)
    same(got, plain, PLAIN_KEYS)
    assert got["levels"] == 1 and got["no_consensus"] == 0 and got["excluded"] == 0
    assert np.all(got["inlier"] == 1) and list(got["consensus"][1:]) == list(got["list_len"][1:]) == hub_lens(d)
    for gn in (0, 16):
        same(ctx.debug_place_chains_robust_host(X, BARC2, gn, 1), ctx.debug_place_chains_host(X, gn), PLAIN_KEYS)


@pytest.mark.parametrize("d", (2, 3))
def test_exact_ranges(d):
    got = mirror_of("exact", d)
    assert list(got["status"]) == [4, 0, 0] and list(got["consensus"][1:]) == [40, 45] and got["excluded"] == 0 and got["levels"] == 2
    ctx, dims, table, X, chains, kw, extra, truth = case("exact", d)
    t0 = dims[0] * dims[1] + dims[2]
    for c in (1, 2):
        R, t = truth[c]
        rows = slice(t0 + 30 * c, t0 + 30 * (c + 1))
        assert np.linalg.norm(got["X"][rows] - (X[rows] @ R.T + t), axis=1).max() < 1e-6


def test_the_constant_of_the_score_bound():
    """C_BOUND is 4 x the worst ratio of the mirror's polished hypotheses to the reference over samples of the committed hubs'
    lists (every fourth sample of a list longer than 64)."""
    worst, count = 0.0, 0
    for d in (2, 3):
        ctx, dims, table, X, chains, kw = case("hub", d)[:6]
        S = cc.structure(cc.LEVELS, *dims, table, chains, **kw)
        rd = np.asarray(table[3])
        for st in S["stages"]:
            qi, ai, ms = np.array(st["q"]), np.array(st["a"]), np.array(st["m"])
            ratio, k = cc.measure_constant(lambda dm: capi.Context(*dm, *pl.diagonal_q(*dm), device=-1), d, X[qi], X[ai], rd[ms, 0], rd[ms, 1],
                                           stride=4 if len(ms) > 64 else 1)
            print("d=%d list of %d: worst ratio %.3f over %d samples" % (d, len(ms), ratio, k))
            worst, count = max(worst, ratio), count + k
    print("worst ratio %.3f over %d samples; C_BOUND %.2f" % (worst, count, cc.C_BOUND))
    assert count > 300 and 4 * worst <= cc.C_BOUND


def robust_refusals(ctx_of, call, raw):
    """Every refusal of a robust form: ctx_of(dims) a fresh handle, call(ctx, X, gn, barc2, min) the form under test through the
    wrapper, raw(ctx) = (function, leading arguments of (X, ldx), whether it takes a leading dimension)."""
    (dims, table, X, chains, _), kw, _ = exact(2)
    ctx = ctx_of(dims)

    def code(*a):
        with pytest.raises(capi.CoraError) as e:
            call(ctx, *a)
        return e.value.code
    assert code(X, 1, BARC2, 4) == ERR_NOT_READY          # no measurement table
    ctx.set_measurements(*table)
    assert code(X, 1, BARC2, 4) == ERR_NOT_READY          # no chain tables
    ctx.set_odometry_chains(chains)
    assert code(X, 1, BARC2, 4) == ERR_NOT_READY          # no placement tables
    ctx.set_chain_placement_order(order=cc.LEVELS, **kw)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert code(X, 1, bad, 4) == ERR_ARG
    assert code(X, 1, BARC2, 0) == ERR_ARG
    assert code(X, -1, BARC2, 4) == ERR_ARG and code(X, 17, BARC2, 4) == ERR_ARG
    fn, lead, has_ldx = raw(ctx)
    out = (capi.C.c_int64 * 8)()
    Xf = np.asfortranarray(X)
    none = [None] * 11
    bar = capi.C.c_double(BARC2)
    if has_ldx:
        assert fn(ctx.h, *lead(Xf, ctx.N - 1), 1, bar, 4, out, *none) == ERR_SHAPE
    assert fn(ctx.h, *lead(None, ctx.N), 1, bar, 4, out, *none) == ERR_ARG
    assert fn(ctx.h, *lead(Xf, ctx.N), 1, bar, 4, None, *none) == ERR_ARG
    assert fn(ctx.h, *lead(Xf, ctx.N), 1, bar, 4, out, *none) == 0 and list(out) == [2, 0, list(out)[2], 0, 2, 2, 0, 0]   # every output may be NULL
    return ctx


def nan_case():
    """The exact relay with a NaN in the position of a pose of chain B that its list ranges from."""
    (dims, table, X, chains, _), kw, _ = exact(2)
    X = X.copy()
    X[dims[0] * dims[1] + dims[2] + 30 + 3, 0] = np.nan
    return dims, table, X, chains, kw


def test_refusals():
    ctx = robust_refusals(lambda dims: capi.Context(*dims, *pl.diagonal_q(*dims), device=-1),
                          lambda ctx, X, gn, b, m: ctx.debug_place_chains_robust_host(X, b, gn, m),
                          lambda ctx: (ctx.L.cora_debug_place_chains_robust_host, lambda X, ldx: (None if X is None else capi._d(X), ldx), True))
    X = exact(2)[0][2]
    for form in (lambda: ctx.place_chains_robust(X, BARC2), lambda: ctx.place_chains_robust_dev(0, BARC2)):
        with pytest.raises(capi.CoraError) as e:
            form()                                     # a device form on a plan-only handle
        assert e.value.code == ERR_HIP
    # a NaN in the vector is no vote: the hypotheses whose samples hold it are refused, every other hypothesis does not count
    # the entry, the election stands -- and the call then ends as the plain call does on such a vector, at the NaN range row
    dims, table, Xn, chains, kw = nan_case()
    with pytest.raises(capi.CoraError) as e:
        ctx.debug_place_chains_robust_host(Xn, BARC2)
    assert e.value.code == ERR_NAN


def test_partitioned_handles_are_refused():
    A, Q, dm, g = tp.build("robots-d2")
    p = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=2)
    with pytest.raises(capi.CoraError) as e:
        p.debug_place_chains_robust_host(np.zeros((p.N, 2)), BARC2)
    assert e.value.code == ERR_ARG and "partitioned" in str(e.value)


def test_chain_consensus_validation_of_the_host_interface():
    """host.Problem.multi_robot_initialization refuses a threshold that is not positive before it reaches the library (None is
    the plain call: tests/test_gpu_chain_consensus.py compares its bits, and the start with the vote, on the device)."""
    from cora_amd import host
    P = host.Problem.synthetic(dim=2, n_poses=30, n_landmarks=2, n_ranges=20, seed=1)
    P.update()
    for bad in (0.0, -3.0, float("nan")):
        with pytest.raises(host.HostError):
            P.multi_robot_initialization(consensus_barc2=bad)
