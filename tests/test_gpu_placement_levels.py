"""A level's chains placed together on the device: cora_place_chains_batched_dev and cora_place_chains_batched bit for bit
against cora_place_chains_dev on the same tables and against the host mirror (cora_debug_place_chains_host) -- every row of
X, statuses, the three costs, chosen points, transforms, degenerate bytes, counts -- on the shapes at which the batching can
go wrong: lists on every boundary of a chunk side by side in one level, a stage of 65 chunks beside a stage of one, a level of
65 stages, chains on every boundary of an apply tile, a level that mixes refused, under-determined and solved stages, the
diamond, a mask, tables without a stage, and the greedy order's tables; twice the same bits; a sum that is not finite;
Problem.multi_robot_initialization with the level order; the driver's --chain-levels."""
import numpy as np
import pytest

import placement_levels_ref as plr
import placement_ref as pl
import test_placement_levels_cpu as cpu
from cora_amd import capi
from test_gpu_odom_init import cora_main  # noqa: F401  (the fixture that builds the driver)
from test_placement_cpu import _pairs

pytestmark = pytest.mark.gpu
bits = pl.bits
ERR_NAN = 3
_BUILT = {}


def long_fold(d):
    """One stage of 65 chunks (16 640 entries: the fold's lanes take a second chunk at stride 64) beside a stage of one."""
    rng = np.random.default_rng(500 + d)
    ranges = _pairs(rng, 0, 150, 150, 150, 65 * 256) + _pairs(rng, 0, 150, 300, 40, cpu.least(d))
    return pl.scene(d, [150, 150, 40], ranges, seed=130 + d, noise=0.02), dict(min_ranges=cpu.least(d)), dict(levels=[1, 1])


def wide_level(d):
    """A level of 65 stages (65 chains of 6 poses against chain 0) and a level of one (a chain against chain 1 only)."""
    rng = np.random.default_rng(510 + d)
    ranges = []
    for c in range(65):
        ranges += _pairs(rng, 0, 30, 30 + 6 * c, 6, cpu.least(d))
    ranges += _pairs(rng, 30, 6, 30 + 6 * 65, 6, cpu.least(d))
    return pl.scene(d, [30] + [6] * 66, cpu._shuffled(rng, ranges), seed=140 + d), dict(min_ranges=cpu.least(d)), dict(levels=[1] * 65 + [2])


def tiles(d):
    """Chains of 2, 255, 256 and 257 poses in one level: apply tiles of 2, 255, 256 and 256 + 1 positions."""
    rng = np.random.default_rng(520 + d)
    lens, first, ranges = [2, 255, 256, 257], 30, []
    for n in lens:
        ranges += _pairs(rng, 0, 30, first, n, 60)
        first += n
    return pl.scene(d, [30] + lens, cpu._shuffled(rng, ranges), seed=150 + d, noise=0.02), dict(min_ranges=60), dict(levels=[1] * 4)


def mixed_level(d):
    """One level with a refused stage (every entry names ONE anchor: status 2), an under-determined one (every range twice,
    half as many distinct pairs as unknowns: status 2) and two solved ones."""
    rng = np.random.default_rng(530 + d)
    k = cpu.least(d)
    ranges = [(7, 30 + int(j)) if m % 2 else (30 + int(j), 7) for m, j in enumerate(rng.choice(40, size=k))]
    ranges += _pairs(rng, 0, 30, 70, 40, k, twice=True) + _pairs(rng, 0, 30, 110, 40, 300) + _pairs(rng, 0, 30, 150, 40, 60)
    return pl.scene(d, [30] + [40] * 4, cpu._shuffled(rng, ranges), seed=160 + d, noise=0.02), dict(min_ranges=k), dict(levels=[1] * 4, status=[4, 2, 2, 0, 0])


def no_stage(d):
    sc, kw, _ = cpu.diamond(d)
    return sc, dict(min_ranges=1000), dict(levels=[])


BUILDERS = dict(cpu.BUILDERS, long_fold=long_fold, wide_level=wide_level, tiles=tiles, mixed_level=mixed_level, no_stage=no_stage)
# (name, order of the tables)
SHAPES = [("star", plr.LEVELS), ("long_fold", plr.LEVELS), ("wide_level", plr.LEVELS), ("tiles", plr.LEVELS), ("mixed_level", plr.LEVELS),
          ("diamond", plr.LEVELS), ("two_levels_masked", plr.LEVELS), ("no_stage", plr.LEVELS), ("diamond", plr.GREEDY), ("star", plr.GREEDY)]


def case(name, d, order):
    key = (name, d, order)
    if key not in _BUILT:
        (dims, table, X, chains, _), kw, extra = BUILDERS[name](d)
        ctx = capi.Context(*dims, *pl.diagonal_q(*dims), device=0)
        ctx.set_measurements(*table)
        ctx.set_odometry_chains(chains)
        ctx.set_chain_placement_order(order=order, **kw)
        _BUILT[key] = (ctx, dims, X, extra)
    return _BUILT[key]


def same(got, want):
    assert np.array_equal(bits(got["X"]), bits(want["X"]))
    cpu.same(got, want)


@pytest.mark.parametrize("name,order,d,gn", [(name, order, d, gn) for name, order in SHAPES for d in (2, 3) for gn in (0, 5, 16)])
def test_batched_against_plain_and_mirror(name, order, d, gn):
    ctx, dims, X, extra = case(name, d, order)
    levels = list(ctx.chain_placement_levels())
    if order == plr.LEVELS:
        assert levels == extra["levels"]
    else:
        assert levels == list(range(1, len(levels) + 1))
    mirror = ctx.debug_place_chains_host(X, gn)
    plain = ctx.place_chains(X, gn)
    got = ctx.place_chains_batched(X, gn)
    same(plain, mirror)
    same(got, plain)
    same(got, mirror)
    assert got["levels"] == (levels[-1] if levels else 0) and got["stages"] == len(levels)
    if "status" in extra and order == plr.LEVELS:
        assert list(got["status"]) == extra["status"]
    for c in range(len(got["status"])):   # never worse, as doubles
        assert got["cost_final"][c] <= got["cost_start"][c]
    # the resident form, twice on one upload: the second call starts from the first one's result, as the mirror's does
    x = ctx.dev_alloc(dims[0])
    try:
        ctx.upload(X, x)
        res = ctx.place_chains_batched_dev(x, gn)
        assert np.array_equal(bits(ctx.download(x, dims[0])), bits(mirror["X"]))
        cpu.same(res, mirror)
        again = ctx.place_chains_batched_dev(x, gn)
        twice = ctx.debug_place_chains_host(mirror["X"], gn)
        assert np.array_equal(bits(ctx.download(x, dims[0])), bits(twice["X"]))
        cpu.same(again, twice)
    finally:
        ctx.dev_free(x)
    same(ctx.place_chains_batched(X, gn), got)   # two calls, the same bits


@pytest.mark.parametrize("d", (2, 3))
def test_a_sum_that_is_not_finite(d):
    """Both device calls report a sum that is not finite through the flag word.  (cora_set_measurements refuses a NaN in the
    measurement table itself, asserted here, so the range is one whose square overflows, as in the plain call's test, and
    the NaN stands in the vector.)"""
    (dims, table, X, chains, _), kw, _ = cpu.diamond(d)
    ctx = capi.Context(*dims, *pl.diagonal_q(*dims), device=0)

    def code(fn, *a):
        with pytest.raises(capi.CoraError) as e:
            fn(*a)
        return e.value.code
    m = plr.structure(*dims, table, chains, None, kw["min_ranges"])["stages"][1]["m"][0]   # an entry of C's list (a range between B and C is in no list)
    rd = table[3].copy()
    rd[m, 0] = np.nan
    assert code(ctx.set_measurements, table[0], table[1], table[2], rd) == cpu.ERR_ARG
    rd[m, 0] = 1e200   # r^2 overflows
    ctx.set_measurements(table[0], table[1], table[2], rd)
    ctx.set_odometry_chains(chains)
    ctx.set_chain_placement_order(order=plr.LEVELS, **kw)
    assert code(ctx.place_chains, X, 5) == ERR_NAN and code(ctx.place_chains_batched, X, 5) == ERR_NAN
    assert code(ctx.debug_place_chains_host, X, 5) == ERR_NAN
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_chain_placement_order(order=plr.LEVELS, **kw)
    Xn = X.copy()
    Xn[table[2][m, 1]] = np.nan   # the translation row of an end of that range
    assert code(ctx.place_chains, Xn, 5) == ERR_NAN and code(ctx.place_chains_batched, Xn, 5) == ERR_NAN
    same(ctx.place_chains_batched(X, 5), ctx.place_chains(X, 5))   # and the handle serves the next call


def test_device_refusals():
    (dims, table, X, chains, _), kw, _ = cpu.diamond(3)
    ctx = capi.Context(*dims, *pl.diagonal_q(*dims), device=0)
    x = ctx.dev_alloc(3)
    try:
        def code(fn, *a):
            with pytest.raises(capi.CoraError) as e:
                fn(*a)
            return e.value.code
        assert code(ctx.place_chains_batched_dev, x, 1) == 2          # no measurement table
        ctx.set_measurements(*table)
        ctx.set_odometry_chains(chains)
        assert code(ctx.place_chains_batched, X, 1) == 2              # no placement tables
        ctx.set_chain_placement_order(order=plr.LEVELS, **kw)
        assert code(ctx.place_chains_batched_dev, x, 17) == cpu.ERR_ARG and code(ctx.place_chains_batched_dev, x, -1) == cpu.ERR_ARG
        assert code(ctx.place_chains_batched_dev, 0, 1) == cpu.ERR_ARG   # a null vector
        out = (capi.C.c_int64 * 6)()
        Xf = np.asfortranarray(X)
        none = [None] * 7
        assert ctx.L.cora_place_chains_batched(ctx.h, capi._d(Xf), ctx.N - 1, 1, out, *none) == 1
        assert ctx.L.cora_place_chains_batched(ctx.h, capi._d(Xf), ctx.N, 1, None, *none) == cpu.ERR_ARG
        assert ctx.L.cora_place_chains_batched(ctx.h, capi._d(Xf), ctx.N, 1, out, *none) == 0 and out[0] == 2 and out[4] == 2 and out[5] == 1
    finally:
        ctx.dev_free(x)


@pytest.mark.parametrize("name", ("pp_only", "robots-d2"))
def test_problem_start_with_the_level_order(name):
    """Problem::multiRobotInitialization: the default argument and ChainOrder::Greedy have the bits of the call without the
    argument.  ChainOrder::Levels against the C-ABI sequence by hand -- cora_set_chain_placement_order and the stages of the
    level order run on the odometry start brought back to d columns: stages, levels and statuses equal, the placed rows
    within the bound of tests/test_gpu_placement.py (C a + b per row plus the two lifts); where the lists of both orders
    coincide (pp_only) the whole start has the greedy order's bits."""
    import odom_ref as od
    import residuals_ref as rr
    import topologies as tp
    A, Q, dm, g = tp.build(name)
    d, n, r, nt, p = dm.d, dm.n, dm.r, dm.n_trans, 5
    P = tp.to_problem(name, rank=p)
    mr = pl.unknowns(d) + 1
    base, binfo = P.multi_robot_initialization(seed=7, gn_steps=5, min_ranges=mr)
    greedy, ginfo = P.multi_robot_initialization(seed=7, gn_steps=5, min_ranges=mr, order="greedy")
    assert np.array_equal(bits(base), bits(greedy)) and "levels" not in binfo and ginfo["levels"] == ginfo["stages"]
    for key in ("status", "cost_start", "cost_linear", "cost_final", "transforms"):
        assert np.array_equal(bits(np.asarray(binfo[key], dtype=np.float64)), bits(np.asarray(ginfo[key], dtype=np.float64))), key
    assert np.array_equal(bits(P.op("multiRobotInitialization")), bits(P.multi_robot_initialization(order="greedy")[0]))
    new, info = P.multi_robot_initialization(seed=7, gn_steps=5, min_ranges=mr, order="levels")
    table, chains = rr.table(g), od.chains_of(g)
    S, S0 = plr.structure(d, n, r, nt, table, chains, None, mr), pl.structure(d, n, r, nt, table, chains, None, mr)
    ctx = capi.Context(d, n, r, nt, Q.rowptr, Q.col, Q.val, device=0)   # the sequence by hand
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_chain_placement_order(min_ranges=mr, order=plr.LEVELS)
    levels = list(ctx.chain_placement_levels())
    assert info["stages"] == len(levels) == len(S["stages"]) and info["levels"] == (levels[-1] if levels else 0) == max(S["level"] + [0])
    old = P.op("odometryInitialization")
    first = table[0][chains[0][0], 0]
    Qd = old[first:first + d]
    x_old, x_new = old @ Qd.T, new @ Qd.T
    hand = ctx.place_chains_batched(x_old, 5)
    assert np.array_equal(info["status"], hand["status"]) and info["placed"] == hand["placed"] and info["not_placed"] == hand["not_placed"]
    ref = plr.reference(d, n, r, nt, table, chains, x_old, 5, min_ranges=mr, struct=S)
    t0 = d * n + r
    scale = np.abs(x_old[t0:t0 + n]).max()
    for k, st in enumerate(S["stages"]):
        one, c = ref["stage"][k], st["chain"]
        kap = max(one["kappa_lin"], one["kappa_gn"], 1.0)
        for rot, trn in S["positions"][c]:
            x, _ = one["rows_before"][trn]
            lift = 2 * (d + 2) * pl.EPS * (scale * (1 + kap) * (1 + float(pl._norm(x - one["q0"])) / one["L"]) + np.abs(x_new[trn]).max())
            bound = pl.C_BOUND * ref["row_a"][trn] + ref["row_b"][trn] + lift
            assert float(pl._norm(x_new[trn] - hand["X"][trn])) <= 2 * bound, (c, trn)
    if [s["m"] for s in sorted(S["stages"], key=lambda s: s["chain"])] == [s["m"] for s in sorted(S0["stages"], key=lambda s: s["chain"])]:
        assert np.array_equal(bits(new), bits(base))
    else:
        assert not np.array_equal(bits(new), bits(base))
    print("%s: %d stages in %d levels, statuses %s" % (name, info["stages"], info["levels"], info["status"]))


def test_driver_chain_levels(cora_main):  # noqa: F811
    """cora_main --place-chains --chain-levels on the four-robot data set: three stages in one level, the placement's line,
    a solve; without --place-chains the flag is refused."""
    import os
    import re
    import subprocess
    from conftest import GOLDEN
    data = os.path.join(GOLDEN, "datasets", "tiers.pyfg")
    r = subprocess.run([cora_main, data, "--odom-init", "--device-init", "--place-chains", "--chain-levels", "--landmark-init"],
                       stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    m = re.search(r"chain placement: (\d+) chains placed, (\d+) not placed", r.stdout)
    assert m and int(m.group(1)) == 3 and int(m.group(2)) == 0, r.stdout[-2000:]
    assert "chain placement: level order, 3 stages in 1 levels" in r.stdout and re.search(r"final cost ([0-9.eE+-]+)", r.stdout)
    r = subprocess.run([cora_main, data, "--odom-init", "--device-init", "--chain-levels"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "--place-chains" in r.stderr
