"""The initialisers share device buffers on a handle (the range-row step's exchanged rows and flag bytes, the reduction
scratch, the flag word): on ONE handle with the chain tables and all four placement tables installed, the device-pointer forms
-- odometry, multilateration, chain placement, placement from sightings, from closures, from closures with the consensus
vote -- run one after another on copies of one start vector, in two orders.  Each result, `degenerate` included, has its
mirror's bits and the bits of a fresh handle with that one feature alone.  The same after set_measurements with the same data
(which frees every dependent table) and a reinstall, and on the graph without any range measurement for the features that
need none.  d = 2 and d = 3; 3 chains of 10 poses, 2 landmarks."""
import numpy as np
import pytest

import closure_ref as cl
import placement_ref as pl
from cora_amd import capi

pytestmark = pytest.mark.gpu
bits = cl.bits
LENS = [10, 10, 10]
ORDERS = (("odom", "multilat", "chains", "sightings", "closures", "closures_robust"),
          ("closures_robust", "sightings", "multilat", "closures", "odom", "chains"))
NO_RANGES = ("odom", "sightings", "closures")   # the features that need no range measurement


def graph(d, with_ranges):
    """Chains 0, 1, 2 over poses 0-9, 10-19, 20-29, landmarks 30 and 31.  Ranges: 2 x (d + 2) pose-landmark from chain 0 (a
    list per landmark for the multilateration), 20 between chains 0 and 1 and 20 between chains 0 | 1 and 2 (a stage each at
    min_ranges = unknowns + 1 = 8 | 17).  Sightings: both landmarks from chain 0, and from chains 1 and 2 (d = 2: a C-stage at
    min_sightings = d; d = 3 has too few landmarks for one: the L-stage and the REFIT).  Closures: 3 between chains 0 and 1, 3
    between 1 and 2 (two stages at min_closures = 1)."""
    rng = np.random.default_rng(910 + d)
    ranges = []
    if with_ranges:
        ranges += [(int(rng.integers(10)), 30 + lm) for lm in (0, 1) for _ in range(d + 2)]
        ranges += [(int(rng.integers(10)), 10 + int(rng.integers(10))) for _ in range(20)]
        ranges += [(int(rng.integers(20)), 20 + int(rng.integers(10))) for _ in range(20)]
    sights = [(int(rng.integers(10 * c, 10 * c + 10)), lm) for c in range(3) for lm in (0, 1) for _ in range(3)]
    closures = [(int(rng.integers(10)), 10 + int(rng.integers(10))) for _ in range(3)]
    closures += [(20 + int(rng.integers(10)), 10 + int(rng.integers(10))) for _ in range(3)]
    dims, table, X, chains, _ = cl.scene(d, LENS, closures, seed=70 + d, n_lm=2, noise=0.02, ranges=ranges, sights=sights)
    starts = X[d * dims[1] + dims[2] + np.array([0, 10, 20])]
    return dims, table, X, chains, starts


INSTALL = dict(odom=lambda ctx, d: None,
               multilat=lambda ctx, d: ctx.set_multilateration(),
               chains=lambda ctx, d: ctx.set_chain_placement(min_ranges=pl.unknowns(d) + 1),
               sightings=lambda ctx, d: ctx.set_sighting_placement(min_sightings=d),
               closures=lambda ctx, d: ctx.set_closure_placement(min_closures=1),
               closures_robust=lambda ctx, d: ctx.set_closure_placement(min_closures=1))
COUNTS = dict(multilat=lambda ctx: ctx.multilateration_counts()[3], chains=lambda ctx: ctx.chain_placement_counts()[0],
              sightings=lambda ctx: ctx.sighting_placement_counts()[0], closures=lambda ctx: ctx.closure_placement_counts()[0],
              closures_robust=lambda ctx: ctx.closure_placement_counts()[0])


def device_form(ctx, name, x, starts):
    return dict(odom=lambda: ctx.odometry_init_dev(starts, None, x), multilat=lambda: ctx.multilaterate_dev(x, 2),
                chains=lambda: ctx.place_chains_dev(x, 2), sightings=lambda: ctx.place_by_sightings_dev(x),
                closures=lambda: ctx.place_by_closures_dev(x), closures_robust=lambda: ctx.place_by_closures_robust_dev(x, 1.0, 1))[name]()


def mirror_form(ctx, name, X, starts):
    return dict(odom=lambda: ctx.debug_odometry_init_host(starts), multilat=lambda: ctx.debug_multilaterate_host(X, 2),
                chains=lambda: ctx.debug_place_chains_host(X, 2), sightings=lambda: ctx.debug_place_by_sightings_host(X),
                closures=lambda: ctx.debug_place_by_closures_host(X),
                closures_robust=lambda: ctx.debug_place_by_closures_robust_host(X, 1.0, 1))[name]()


def handle(d, dims, table, chains, features):
    ctx = capi.Context(*dims, *cl.diagonal_q(*dims), device=0)
    install(ctx, d, table, chains, features)
    return ctx


def install(ctx, d, table, chains, features):
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    for name in features:
        INSTALL[name](ctx, d)
        if name in COUNTS:
            assert COUNTS[name](ctx) > 0, "%s has no stage" % name


def same(got, want, what):
    assert set(got) == set(want) - {"X"}, what
    for key, v in got.items():
        w = want[key]
        if isinstance(v, np.ndarray) and v.dtype.kind == "f":
            assert np.array_equal(bits(v), bits(w)), (what, key)
        elif isinstance(v, np.ndarray):
            assert v.dtype == w.dtype and np.array_equal(v, w), (what, key)
        else:
            assert v == w, (what, key)


def run_in_order(ctx, dd, order, X, starts, mirrors, alone):
    x = ctx.dev_alloc(dd)
    try:
        for name in order:
            ctx.upload(X, x)
            got = device_form(ctx, name, x, starts)
            rows = ctx.download(x, dd)
            for what, (res, ref_rows) in (("mirror", mirrors[name]), ("a handle of its own", alone[name])):
                same(got, res, "%s against %s" % (name, what))
                assert np.array_equal(bits(rows), bits(ref_rows)), "%s against %s: rows" % (name, what)
    finally:
        ctx.dev_free(x)


def references(d, dims, table, X, chains, starts, features):
    """Per feature (result, rows) of the mirror and of the device form on a fresh handle that has this feature alone."""
    dd = dims[0]
    mirrors, alone = {}, {}
    for name in features:
        ctx = handle(d, dims, table, chains, [name])
        res = mirror_form(ctx, name, X, starts)
        mirrors[name] = (res, res["X"])
        x = ctx.dev_alloc(dd)
        try:
            ctx.upload(X, x)
            got = device_form(ctx, name, x, starts)
            alone[name] = (dict(got, X=None), ctx.download(x, dd))
        finally:
            ctx.dev_free(x)
            ctx.close()
    return mirrors, alone


@pytest.mark.parametrize("d", (2, 3))
def test_the_forms_share_one_handle(d):
    dims, table, X, chains, starts = graph(d, True)
    features = ORDERS[0]
    mirrors, alone = references(d, dims, table, X, chains, starts, features)
    assert mirrors["odom"][0]["degenerate"].shape == (dims[2],) and dims[2] > 0
    ctx = handle(d, dims, table, chains, features)
    for order in ORDERS:
        run_in_order(ctx, dims[0], order, X, starts, mirrors, alone)
    # the same data again: every dependent table goes, the range-row step's arrays with them
    ctx.set_measurements(*table)
    assert ctx.odometry_chains_count() == (0, 0) and ctx.multilateration_counts()[3] == 0
    assert ctx.chain_placement_counts()[0] == ctx.sighting_placement_counts()[0] == ctx.closure_placement_counts()[0] == 0
    install(ctx, d, table, chains, features)
    run_in_order(ctx, dims[0], ORDERS[1], X, starts, mirrors, alone)
    ctx.close()


@pytest.mark.parametrize("d", (2, 3))
def test_the_forms_share_one_handle_without_ranges(d):
    dims, table, X, chains, starts = graph(d, False)
    assert dims[2] == 0 and len(table[2]) == 0
    mirrors, alone = references(d, dims, table, X, chains, starts, NO_RANGES)
    ctx = handle(d, dims, table, chains, NO_RANGES)
    for order in (NO_RANGES, NO_RANGES[::-1]):
        run_in_order(ctx, dims[0], order, X, starts, mirrors, alone)
        for name in order:
            assert mirrors[name][0]["n_degenerate"] == 0 and len(mirrors[name][0]["degenerate"]) == 0
    ctx.close()
