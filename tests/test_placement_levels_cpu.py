"""The level order of the chain placement from inter-robot ranges without a GPU (include/cora_hip.h,
cora_set_chain_placement_order): the tables of CORA_PL_ORDER_LEVELS against the pure-Python restatement of the rule in
tests/placement_levels_ref.py -- stages, levels, counts, statuses -- on a star, a relay, a diamond, a mask of two chains, a
chain an entry short, a chain without a range and skipped ranges; CORA_PL_ORDER_GREEDY through the new setter against
cora_set_chain_placement; the host mirror run on level tables against the longdouble stage of tests/placement_ref.py applied
to the level lists, with its bound and its constant; and the bits of the level order against the greedy order where the
lists coincide.  The batched device call against the mirror, bit for bit: tests/test_gpu_placement_levels.py."""
import numpy as np
import pytest

import placement_levels_ref as plr
import placement_ref as pl
from cora_amd import capi
from test_placement_cpu import _pairs, statuses, two_fixed

ERR_ARG = 5
bits = pl.bits
_BUILT = {}


def least(d):
    return pl.unknowns(d) + 1


def _shuffled(rng, ranges):
    return [ranges[i] for i in rng.permutation(len(ranges))]


def star(d):
    """Chain 0 of 30 poses and five chains of 40 with lists of min_ranges (8 / 17), 255, 256, 257 and 513 entries against it:
    one level, the lists of both orders coincide."""
    rng = np.random.default_rng(400 + d)
    ranges = []
    for c, k in enumerate([least(d), 255, 256, 257, 513]):
        ranges += _pairs(rng, 0, 30, 30 + 40 * c, 40, k)
    return pl.scene(d, [30] + [40] * 5, _shuffled(rng, ranges), seed=90 + d, noise=0.02), dict(min_ranges=least(d)), dict(levels=[1] * 5, chains=[1, 2, 3, 4, 5])


def relay(d):
    """A - B - C - D: three levels of one stage, the greedy order's stages and lists."""
    rng = np.random.default_rng(410 + d)
    ranges = _pairs(rng, 60, 30, 90, 30, 40) + _pairs(rng, 0, 30, 30, 30, 45) + _pairs(rng, 30, 30, 60, 30, 50)
    return pl.scene(d, [30] * 4, _shuffled(rng, ranges), seed=100 + d, noise=0.02), dict(min_ranges=least(d)), dict(levels=[1, 2, 3], chains=[1, 2, 3])


def diamond(d):
    """B against A, C against A and against B: B and C share level 1 and C's list holds its 30 entries against A only (the
    greedy order takes B, then C with all 55)."""
    rng = np.random.default_rng(420 + d)
    ranges = _pairs(rng, 0, 40, 40, 30, 40) + _pairs(rng, 0, 40, 70, 30, 30) + _pairs(rng, 40, 30, 70, 30, 25)
    return pl.scene(d, [40, 30, 30], _shuffled(rng, ranges), seed=110 + d, noise=0.05), dict(min_ranges=least(d)), dict(levels=[1, 1], chains=[1, 2], entries=70)


def two_levels_masked(d):
    """A mask fixing A and D; B against both (level 1), C against B and against D but below min_ranges against D alone
    (level 2, with its entries against B and D), E against C only (level 3)."""
    rng = np.random.default_rng(430 + d)
    ranges = _pairs(rng, 0, 30, 30, 30, 20) + _pairs(rng, 90, 30, 30, 30, 25) + _pairs(rng, 30, 30, 60, 30, 35) + _pairs(rng, 90, 30, 60, 30, 10)
    ranges += _pairs(rng, 60, 30, 120, 30, 42)
    sc = pl.scene(d, [30] * 5, _shuffled(rng, ranges), seed=120 + d, noise=0.02, moved=[False, True, True, False, True])
    return sc, dict(min_ranges=40, chain_fixed=[1, 0, 0, 1, 0]), dict(levels=[1, 2, 3], chains=[1, 2, 4])


def _wrap(builder, **extra):
    def build(d):
        sc, kw, old = builder(d)
        return sc, kw, extra
    return build


BUILDERS = dict(star=star, relay=relay, diamond=diamond, two_levels_masked=two_levels_masked,
                two_fixed=_wrap(two_fixed, levels=[1], chains=[1]), statuses=_wrap(statuses, levels=[1], chains=[1], status=[4, 0, 1, 3], skipped=9))
CASES = [(name, d) for name in BUILDERS for d in (2, 3)]
SAME_LISTS = ("star", "relay", "two_fixed", "statuses")   # every chain ranges only against earlier levels


def case(name, d, order=plr.LEVELS, device=-1):
    """(ctx, dims, table, X, chains, kw, extra) with the tables of `order` installed (None: cora_set_chain_placement)."""
    key = (name, d, order, device)
    if key not in _BUILT:
        (dims, table, X, chains, _), kw, extra = BUILDERS[name](d)
        ctx = capi.Context(*dims, *pl.diagonal_q(*dims), device=device)
        ctx.set_measurements(*table)
        ctx.set_odometry_chains(chains)
        if order is None:
            ctx.set_chain_placement(**kw)
        else:
            ctx.set_chain_placement_order(order=order, **kw)
        _BUILT[key] = (ctx, dims, table, X, chains, kw, extra)
    return _BUILT[key]


def mirror_of(name, d, gn, order=plr.LEVELS):
    key = ("mirror", name, d, gn, order)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, _ = case(name, d, order)
        got = ctx.debug_place_chains_host(X, gn)
        got["X_in"] = X
        _BUILT[key] = got
    return _BUILT[key]


def same(a, b, keys=("placed", "not_placed", "steps", "n_degenerate", "stages")):
    for key in ("status", "chosen", "degenerate"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("cost_start", "cost_linear", "cost_final", "transforms"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    for key in keys:
        assert a[key] == b[key], key


@pytest.mark.parametrize("name,d", CASES)
def test_structure_of_the_level_order(name, d):
    ctx, dims, table, X, chains, kw, extra = case(name, d)
    S = plr.structure(*dims, table, chains, kw.get("chain_fixed"), kw.get("min_ranges"))
    assert ctx.chain_placement_counts() == S["counts"]
    assert list(ctx.chain_placement_order()) == [s["chain"] for s in S["stages"]] == extra["chains"]
    assert list(ctx.chain_placement_levels()) == S["level"] == extra["levels"]
    got = mirror_of(name, d, 0)
    stage_chains = set(extra["chains"])
    for c, init in enumerate(S["init"]):   # a chain that is no stage keeps the status of the tables
        assert (got["status"][c] == init) if c not in stage_chains else (init == 0 and got["status"][c] in (0, 2))
    assert got["stages"] == len(S["stages"]) and got["not_placed"] == sum(1 for s in S["init"] if s in (1, 3))
    if "status" in extra:
        assert list(got["status"]) == extra["status"] and S["skipped"] == extra["skipped"]
    if "entries" in extra:   # the diamond: 40 of B and C's 30 against A; the 25 between B and C are in no list
        assert S["counts"][1] == extra["entries"] and [len(s["m"]) for s in S["stages"]] == [40, 30]
        greedy = case(name, d, plr.GREEDY)[0]
        assert greedy.chain_placement_counts()[1] == 40 + 55 and list(greedy.chain_placement_levels()) == [1, 2]


@pytest.mark.parametrize("name,d", CASES)
def test_greedy_through_the_new_setter(name, d):
    """Order 0 gives the tables and the results of cora_set_chain_placement exactly; every stage is a level of its own."""
    new, old = case(name, d, plr.GREEDY)[0], case(name, d, None)[0]
    assert new.chain_placement_counts() == old.chain_placement_counts()
    assert list(new.chain_placement_order()) == list(old.chain_placement_order())
    ns = new.chain_placement_counts()[0]
    assert list(new.chain_placement_levels()) == list(old.chain_placement_levels()) == list(range(1, ns + 1))
    a, b = mirror_of(name, d, 5, plr.GREEDY), mirror_of(name, d, 5, None)
    assert np.array_equal(bits(a["X"]), bits(b["X"]))
    same(a, b)


@pytest.mark.parametrize("name,d,gn", [(name, d, gn) for name, d in CASES for gn in ((0, 5, 16) if name in ("star", "diamond") else (5,))])
def test_mirror_on_level_tables(name, d, gn):
    """cora_debug_place_chains_host on level tables, stage after stage, against the longdouble stage over the level lists:
    the bound and C = 3.2 of tests/placement_ref.py."""
    ctx, dims, table, X, chains, kw, _ = case(name, d)
    ref = plr.reference(*dims, table, chains, X, gn, **kw)
    got = mirror_of(name, d, gn)
    worst = pl.check(got, *dims, table, ref, C=pl.C_BOUND)
    print("%s d=%d gn=%d: worst error / (a + b) %.4f; statuses %s chosen %s" % (name, d, gn, worst, got["status"], got["chosen"]))
    for c in range(len(chains)):
        assert got["cost_final"][c] <= got["cost_start"][c]


@pytest.mark.parametrize("name,d", [(name, d) for name in SAME_LISTS for d in (2, 3)])
def test_levels_equal_greedy_where_the_lists_coincide(name, d):
    """Every chain ranges only against chains of earlier levels: the lists are the greedy order's, whatever the order of the
    stages, so X and the per-chain outputs have the same bits."""
    a, b = mirror_of(name, d, 5, plr.LEVELS), mirror_of(name, d, 5, plr.GREEDY)
    assert np.array_equal(bits(a["X"]), bits(b["X"]))
    same(a, b)


def test_the_diamond_differs_from_greedy():
    a, b = mirror_of("diamond", 2, 5, plr.LEVELS), mirror_of("diamond", 2, 5, plr.GREEDY)
    assert np.array_equal(bits(a["transforms"][1]), bits(b["transforms"][1]))       # B: the same list
    assert not np.array_equal(bits(a["cost_start"][2]), bits(b["cost_start"][2]))   # C: 30 entries against 55


def test_refusals():
    (dims, table, X, chains, _), kw, _ = diamond(2)
    ctx = capi.Context(*dims, *pl.diagonal_q(*dims), device=-1)
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_chain_placement_order(order=plr.LEVELS, **kw)
    before = (ctx.chain_placement_counts(), list(ctx.chain_placement_levels()))
    for bad in (dict(order=2, **kw), dict(order=-1, **kw), dict(order=plr.LEVELS, min_ranges=7), dict(order=plr.LEVELS, min_ranges=8, chain_fixed=[0, 0, 0])):
        with pytest.raises(capi.CoraError) as e:
            ctx.set_chain_placement_order(**bad)
        assert e.value.code == ERR_ARG
        assert (ctx.chain_placement_counts(), list(ctx.chain_placement_levels())) == before   # a refused call leaves the tables
    assert ctx.L.cora_chain_placement_levels(ctx.h, None) == ERR_ARG
    with pytest.raises(capi.CoraError) as e:   # a device form on a plan-only handle
        ctx.place_chains_batched(X, 1)
    assert e.value.code == 4
    ctx.set_chain_placement_order(order=plr.LEVELS, min_ranges=1000)   # no stage at all
    assert ctx.chain_placement_counts()[:3] == (0, 0, 0) and len(ctx.chain_placement_levels()) == 0
    got = ctx.debug_place_chains_host(X, 5)
    assert list(got["status"]) == [4, 1, 1] and got["stages"] == 0 and got["not_placed"] == 2
