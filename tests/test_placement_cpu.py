"""The chain placement from inter-robot ranges without a GPU: cora_debug_place_chains_host (the functions the kernels call,
in the device's bracket order, on plan-only handles) against the longdouble reference of tests/placement_ref.py -- statuses,
the order of the stages, counts, the chosen point, the degenerate flags, the transforms and rows within the derived bound,
never worse on the range cost -- on entry lists that sit on every boundary of the reduction's shape, on degenerate geometry
on either side of the pivot rule, on the catalogue's multi-robot graphs, with masks, and every refusal.  The device forms
against the mirror, bit for bit: tests/test_gpu_placement.py."""
import numpy as np
import pytest

import odom_ref as od
import placement_ref as pl
import residuals_ref as rr
import topologies as tp
from cora_amd import capi

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
CATALOGUE = ("pp_only", "robots-d2", "robots-d3", "n128")
LENS = lambda d: [pl.unknowns(d) + 1, 63, 64, 65, 255, 256, 257, 513]  # noqa: E731

_BUILT = {}


def _pairs(rng, first_a, len_a, first_b, len_b, k, twice=False):
    """k ranges between chain positions of A and of B, distinct pairs (every one twice in a row with `twice`), every other
    one given as (b, a)."""
    draw = (k + 1) // 2 if twice else k
    flat = rng.choice(len_a * len_b, size=draw, replace=False)
    out = [(first_a + int(f) // len_b, first_b + int(f) % len_b) for f in flat]
    if twice:
        out = [p for p in out for _ in range(2)][:k]
    return [(b, a) if m % 2 else (a, b) for m, (a, b) in enumerate(out)]


def lengths(d, noise=0.0, twice=False, offset=0.0):
    """Chain 0 of 30 poses, fixed, and one chain of 40 poses per entry-list length: min_ranges (the least admitted, 8 / 17),
    63, 64, 65, 255, 256, 257 and 513 entries against chain 0, both orders of (a, b), shuffled in the table."""
    rng = np.random.default_rng(140 + d)
    lens = LENS(d)
    ranges = []
    for c, k in enumerate(lens):
        ranges += _pairs(rng, 0, 30, 30 + 40 * c, 40, k, twice)
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    return pl.scene(d, [30] + [40] * len(lens), ranges, seed=d, noise=noise, offset=offset), dict(min_ranges=pl.unknowns(d) + 1), lens


def order(d):
    """A, B, C: C has entries only against B, so it is taken after B although its index is the lowest free one at first."""
    rng = np.random.default_rng(150 + d)
    ranges = _pairs(rng, 40, 30, 70, 30, 50) + _pairs(rng, 0, 40, 70, 30, 45)   # C-B... chains: A = 0, C = 1, B = 2
    return pl.scene(d, [40, 30, 30], ranges, seed=10 + d), dict(min_ranges=pl.unknowns(d) + 1), [2, 1]


def tie(d):
    """B and C with 40 entries each against A: B (the lowest index) first; C then also counts its 20 entries against B."""
    rng = np.random.default_rng(160 + d)
    ranges = _pairs(rng, 0, 40, 70, 30, 40) + _pairs(rng, 0, 40, 40, 30, 40) + _pairs(rng, 40, 30, 70, 30, 20)
    return pl.scene(d, [40, 30, 30], ranges, seed=20 + d, noise=0.05), dict(min_ranges=pl.unknowns(d) + 1), [1, 2]


def statuses(d):
    """Default min_ranges (28 / 64).  B is placed; C has min_ranges - 1 entries (status 1); D has none (status 3); ranges to
    two landmarks, to two free poses and inside chains are skipped and change nothing."""
    rng = np.random.default_rng(170 + d)
    mr = pl.default_min_ranges(d)
    n = 30 + 40 + 40 + 10 + 2
    ranges = _pairs(rng, 0, 30, 30, 40, mr + 5) + _pairs(rng, 0, 30, 70, 40, mr - 1)
    ranges += [(3, n), (n + 1, 35), (n - 1, 4), (40, n - 2), (2, 9), (31, 60), (n, n + 1), (n - 1, n - 2), (115, 111)]
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    return pl.scene(d, [30, 40, 40, 10], ranges, seed=30 + d, n_free=2, n_lm=2, noise=0.02), {}, dict(skipped=9, order=[1])


def two_fixed(d):
    """A mask that fixes A and C: B is placed against both."""
    rng = np.random.default_rng(180 + d)
    ranges = _pairs(rng, 0, 30, 30, 40, 20) + _pairs(rng, 70, 30, 30, 40, 25)
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    return pl.scene(d, [30, 40, 30], ranges, seed=40 + d, moved=[False, True, False]), dict(min_ranges=40, chain_fixed=[1, 0, 1]), [1]


def flat(d):
    """The positions of a chain on a line (d = 2) / in a plane (d = 3) over 50 m: exactly (the linear stage refused), with a
    scatter of 0.3 (solved), with a scatter of 1e-6 (refused); a chain whose entries all name ONE anchor (refused).  The
    reference's pivots are asserted 100 x away from 1e-8 (test_flat_pivots).  (The least pivot goes with the square of the
    scatter; at 1e-4 it is 1.8e-8 at d = 2 and 9e-11 at d = 3, on the rule itself, so the small scatter is 1e-6.)"""
    rng = np.random.default_rng(190 + d)
    k, world = 60, []
    world.append(np.cumsum(rng.normal(0, 3, (30, d)), axis=0))
    for sigma in (0.0, 0.3, 1e-6, 0.3):
        p = np.zeros((40, d))
        p[:, :d - 1] = rng.uniform(0, 50, (40, d - 1))
        p[:, d - 1] = sigma * rng.normal(0, 1, 40)
        world.append(p)
    ranges = []
    for c in range(3):
        ranges += _pairs(rng, 0, 30, 30 + 40 * c, 40, k)
    ranges += [(7, 150 + int(j)) if m % 2 else (150 + int(j), 7) for m, j in enumerate(rng.choice(40, size=k))]   # coincident anchors
    return pl.scene(d, [30, 40, 40, 40, 40], ranges, seed=50 + d, world=np.concatenate(world)), dict(min_ranges=k), None


def flat_anchors(d):
    """The ANCHORS on a line / in a plane (chain 0 is flat), the chains general: scatter 0, 0.3 and 1e-6 of chain 0 in three
    scenes joined as one would be one chain 0; so three fixed chains with one chain placed against each."""
    rng = np.random.default_rng(200 + d)
    world, lens, ranges, fixed = [], [], [], []
    for g, sigma in enumerate((0.0, 0.3, 1e-6)):
        p = np.zeros((30, d))
        p[:, :d - 1] = rng.uniform(0, 50, (30, d - 1))
        p[:, d - 1] = sigma * rng.normal(0, 1, 30)
        world += [p, 25 + np.cumsum(rng.normal(0, 3, (40, d)), axis=0)]
        lens += [30, 40]
        fixed += [1, 0]
        ranges += _pairs(rng, 70 * g, 30, 70 * g + 30, 40, 60)
    return pl.scene(d, lens, ranges, seed=60 + d, world=np.concatenate(world)), dict(min_ranges=60, chain_fixed=fixed), None


def short_chain(d):
    """A chain of two poses -- one edge -- with every pair to chain 0 measured."""
    ranges = [(a, 30 + b) if (a + b) % 2 else (30 + b, a) for a in range(30) for b in range(2)]
    return pl.scene(d, [30, 2], ranges, seed=70 + d), dict(min_ranges=pl.unknowns(d) + 1), [1]


BUILDERS = dict(lengths=lengths, lengths_noisy=lambda d: lengths(d, noise=0.1), lengths_twice=lambda d: lengths(d, twice=True),
                offset=lambda d: lengths(d, offset=1e6), order=order, tie=tie, statuses=statuses, two_fixed=two_fixed, flat=flat,
                flat_anchors=flat_anchors, short_chain=short_chain)
SYNTHETIC = [(name, d) for name in BUILDERS for d in (2, 3)]


def steps_of(name):
    return (0, 5, 16) if name in ("lengths", "tie") else (5,)


def case(name, d=None, device=-1):
    """(ctx, dims, table, X, chains, kw, extra) of a synthetic case (name, d) or of a catalogue entry (d None: its chains
    composed in their own frames by the odometry initialisation's mirror, every start at zero), tables installed."""
    key = (name, d, device)
    if key not in _BUILT:
        if d is None:
            A, Q, dm, g = tp.build(name)
            dims, table = (dm.d, dm.n, dm.r, dm.n_trans), rr.table(g)
            chains = od.chains_of(g)
            ctx = capi.Context(*dims, Q.rowptr, Q.col, Q.val, device=device)
            kw, extra = dict(min_ranges=pl.unknowns(dm.d) + 1), None
        else:
            (dims, table, X, chains, truth), kw, extra = BUILDERS[name](d)
            ctx = capi.Context(*dims, *pl.diagonal_q(*dims), device=device)
        ctx.set_measurements(*table)
        ctx.set_odometry_chains(chains)
        if d is None:
            truth_X = np.array(A["truth"], dtype=np.float64)
            t0 = dm.d * dm.n + dm.r
            host = capi.Context(*dims, Q.rowptr, Q.col, Q.val, device=-1) if device >= 0 else ctx
            if host is not ctx:
                host.set_measurements(*table)
                host.set_odometry_chains(chains)
            X = host.debug_odometry_init_host(np.zeros((len(chains), dm.d)), truth_X[t0 + dm.n:])["X"]
        ctx.set_chain_placement(**kw)
        _BUILT[key] = (ctx, dims, table, X, chains, kw, extra)
    return _BUILT[key]


def reference_of(name, d, gn):
    """Computed once and shared (tests/test_gpu_placement.py reads the same)."""
    key = ("ref", name, d, gn)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, _ = case(name, d)
        _BUILT[key] = pl.reference(*dims, table, chains, X, gn, **kw)
    return _BUILT[key]


def mirror_of(name, d, gn):
    key = ("mirror", name, d, gn)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, _ = case(name, d)
        got = ctx.debug_place_chains_host(X, gn)
        got["X_in"] = X
        _BUILT[key] = got
    return _BUILT[key]


def check_case(name, d, gn):
    ctx, dims, table, X, chains, kw, extra = case(name, d)
    ref, got = reference_of(name, d, gn), mirror_of(name, d, gn)
    assert ctx.chain_placement_counts() == ref["struct"]["counts"]
    assert list(ctx.chain_placement_order()) == [s["chain"] for s in ref["struct"]["stages"]]
    worst = pl.check(got, *dims, table, ref)
    return worst, got, ref, extra


@pytest.mark.parametrize("name,d,gn", [(name, d, gn) for name, d in SYNTHETIC for gn in steps_of(name)])
def test_mirror_on_the_synthetic_cases(name, d, gn):
    worst, got, ref, extra = check_case(name, d, gn)
    print("%s d=%d gn=%d: worst error / (a + b) %.4f; statuses %s chosen %s" % (name, d, gn, worst, got["status"], got["chosen"]))
    order_got = [s["chain"] for s in ref["struct"]["stages"]]
    if name.startswith("lengths") or name == "offset":
        lens = extra
        assert sorted(order_got) == list(range(1, len(lens) + 1)) and [lens[c - 1] for c in order_got] == sorted(lens, reverse=True)
        # (every range twice: the shortest list holds half as many distinct pairs as the linear stage has unknowns)
        assert np.all(got["status"][1 + (name == "lengths_twice"):] == 0) and got["status"][0] == 4
        if name in ("lengths", "offset") and gn > 0:   # exact ranges: the transform is the truth's
            _, _, _, _, truth = BUILDERS[name](d)[0]
            for c in range(1, len(lens) + 1):
                Rc, tc = truth[c]
                one = ref["stage"][order_got.index(c)]
                assert np.abs(np.asarray(ref["transforms"][c][:d * d], dtype=np.float64).reshape(d, d) - Rc).max() < 1e-6 * (1 + 1e3 * (name == "offset")), (c, one["costs"])
    if name in ("order", "tie", "short_chain", "two_fixed"):
        assert order_got == extra
    if name == "statuses":
        assert list(got["status"]) == [4, 0, 1, 3] and order_got == extra["order"] and ref["struct"]["skipped"] == extra["skipped"]
        assert got["placed"] == 1 and got["not_placed"] == 2
    if name == "short_chain":
        assert got["status"][1] in (0, 2)


@pytest.mark.parametrize("name", CATALOGUE)
def test_mirror_on_the_catalogue(name):
    worst, got, ref, _ = check_case(name, None, 5)
    print("%s: worst error / (a + b) %.4f; statuses %s chosen %s" % (name, worst, got["status"], got["chosen"]))


@pytest.mark.parametrize("d", (2, 3))
def test_flat_pivots(d):
    """The flat cases sit on both sides of the pivot rule, each at least 100 x away from it in the reference's pivots."""
    for name, expect in (("flat", [2, 0, 2, 2]), ("flat_anchors", [2, 0, 2])):
        ref = reference_of(name, d, 5)
        stages = ref["struct"]["stages"]
        by_chain = {st["chain"]: ref["stage"][k] for k, st in enumerate(stages)}
        got = [by_chain[c]["status"] for c in sorted(by_chain)]
        assert got == expect, (name, got)
        for c in sorted(by_chain):
            piv = by_chain[c]["pivots"]
            least = min(piv) if piv else 0.0
            print("%s d=%d chain %d: status %d, least pivot of the linear stage %.3e" % (name, d, c, by_chain[c]["status"], least))
            assert least >= 100 * pl.MIN_PIVOT or least <= pl.MIN_PIVOT / 100, (name, c, piv)


@pytest.mark.parametrize("d", (2, 3))
def test_exact_data(d):
    """Three robots with exact odometry and 40 exact ranges between each pair: every chain is placed, the range residual sum
    of the inter-robot ranges is <= 1e-18 sum omega r^2 afterwards and not before, and the transforms are the truth's."""
    rng = np.random.default_rng(300 + d)
    ranges = _pairs(rng, 0, 30, 30, 30, 40) + _pairs(rng, 0, 30, 60, 30, 40) + _pairs(rng, 30, 30, 60, 30, 40)
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    dims, table, X, chains, truth = pl.scene(d, [30, 30, 30], ranges, seed=80 + d)
    ctx = capi.Context(*dims, *pl.diagonal_q(*dims), device=-1)
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_chain_placement(min_ranges=pl.unknowns(d) + 1)
    got = ctx.debug_place_chains_host(X, 5)
    got["X_in"] = X
    ref = pl.reference(*dims, table, chains, X, 5, min_ranges=pl.unknowns(d) + 1)
    pl.check(got, *dims, table, ref)
    assert got["placed"] == 2 and got["not_placed"] == 0 and list(got["status"]) == [4, 0, 0]
    rrows, rd = table[2], table[3]

    def residual_sum(Y):
        diff = Y[rrows[:, 2]] - Y[rrows[:, 1]]
        return float(np.sum(rd[:, 1] * (np.linalg.norm(diff, axis=1) - rd[:, 0]) ** 2))
    scale = float(np.sum(rd[:, 1] * rd[:, 0] ** 2))
    print("d=%d: range residual sum %.3e -> %.3e, sum omega r^2 %.3e" % (d, residual_sum(X), residual_sum(got["X"]), scale))
    assert residual_sum(got["X"]) <= 1e-18 * scale and not residual_sum(X) <= 1e-18 * scale
    # the residuals of the table with the rewritten range rows: |x_t(b) - x_t(a) + r x_rho|^2
    Y = got["X"]
    full = Y[rrows[:, 2]] - Y[rrows[:, 1]] + rd[:, :1] * Y[rrows[:, 0]]
    assert float(np.sum(rd[:, 1] * np.sum(full * full, axis=1))) <= 1e-18 * scale
    for c in (1, 2):   # within the reference's bound of the truth: the truth is the reference's minimiser up to its own convergence
        Rc, tc = truth[c]
        one = ref["stage"][[s["chain"] for s in ref["struct"]["stages"]].index(c)]
        tol = pl.C_BOUND * one["a"] * (1 + float(np.linalg.norm(np.asarray(one["q0"], dtype=np.float64))) / one["L"]) + 64 * pl.EPS * (1 + np.linalg.norm(tc))
        assert np.abs(got["transforms"][c][:d * d].reshape(d, d) - Rc).max() <= tol / one["L"] + 64 * pl.EPS
        assert np.abs(got["transforms"][c][d * d:] - tc).max() <= tol


def test_refusals():
    (dims, table, X, chains, _), kw, _ = order(2)
    ctx = capi.Context(*dims, *pl.diagonal_q(*dims), device=-1)

    def code(fn, *a, **k):
        with pytest.raises(capi.CoraError) as e:
            fn(*a, **k)
        return e.value.code
    assert code(ctx.set_chain_placement) == ERR_NOT_READY                      # no measurement table
    assert code(ctx.debug_place_chains_host, X, 1) == ERR_NOT_READY
    ctx.set_measurements(*table)
    assert code(ctx.set_chain_placement) == ERR_NOT_READY                      # no chain tables
    ctx.set_odometry_chains(chains)
    assert code(ctx.debug_place_chains_host, X, 1) == ERR_NOT_READY            # no placement tables
    assert code(ctx.set_chain_placement, min_ranges=7) == ERR_ARG              # below the unknowns + 1
    assert code(ctx.set_chain_placement, chain_fixed=[0, 0, 0], min_ranges=8) == ERR_ARG   # a mask that fixes no chain
    assert ctx.chain_placement_counts() == (0, 0, 0, 0)
    ctx.set_chain_placement(min_ranges=8)
    assert ctx.chain_placement_counts()[0] == 2
    assert code(ctx.debug_place_chains_host, X, 17) == ERR_ARG and code(ctx.debug_place_chains_host, X, -1) == ERR_ARG
    out = (capi.C.c_int64 * 5)()
    Xf = np.asfortranarray(X)
    none = [None] * 7
    assert ctx.L.cora_debug_place_chains_host(ctx.h, capi._d(Xf), ctx.N - 1, 1, out, *none) == ERR_SHAPE
    assert ctx.L.cora_debug_place_chains_host(ctx.h, None, ctx.N, 1, out, *none) == ERR_ARG
    assert ctx.L.cora_debug_place_chains_host(ctx.h, capi._d(Xf), ctx.N, 1, None, *none) == ERR_ARG
    assert ctx.L.cora_debug_place_chains_host(ctx.h, capi._d(Xf), ctx.N, 1, out, *none) == 0 and out[0] == 2 and out[4] == 2
    assert code(ctx.place_chains, X, 1) == ERR_HIP                             # a device form on a plan-only handle
    # new chains and a new measurement table drop the placement tables
    ctx.set_odometry_chains(chains)
    assert ctx.chain_placement_counts() == (0, 0, 0, 0) and code(ctx.debug_place_chains_host, X, 1) == ERR_NOT_READY
    ctx.set_chain_placement(min_ranges=8)
    rd = table[3].copy()
    rd[0, 0] = 1e200   # r^2 overflows
    ctx.set_measurements(table[0], table[1], table[2], rd)
    assert ctx.chain_placement_counts() == (0, 0, 0, 0)
    ctx.set_odometry_chains(chains)
    ctx.set_chain_placement(min_ranges=8)
    assert code(ctx.debug_place_chains_host, X, 1) == ERR_NAN
    (dims3, table3, X3, chains3, _), _, _ = order(3)
    ctx3 = capi.Context(*dims3, *pl.diagonal_q(*dims3), device=-1)
    ctx3.set_measurements(*table3)
    ctx3.set_odometry_chains(chains3)
    assert code(ctx3.set_chain_placement, min_ranges=16) == ERR_ARG
    ctx3.set_chain_placement(min_ranges=17)


def test_partitioned_handles_are_refused():
    A, Q, dm, g = tp.build("robots-d2")
    p = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=2)
    for fn, args in ((p.set_chain_placement, ()), (p.debug_place_chains_host, (np.zeros((p.N, 2)), 1))):
        with pytest.raises(capi.CoraError) as e:
            fn(*args)
        assert e.value.code == ERR_ARG and "partitioned" in str(e.value)
