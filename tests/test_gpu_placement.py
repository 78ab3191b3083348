"""The chain placement from inter-robot ranges on the device: cora_place_chains_dev (twice on one upload) and
cora_place_chains bit for bit against the host mirror (cora_debug_place_chains_host) on every case of
tests/test_placement_cpu.py and on the catalogue's multi-robot graphs -- rows, statuses, costs, chosen points, transforms,
degenerate flags, counts --, within the bound of tests/placement_ref.py; the device refusals;
Problem.multi_robot_initialization against Problem.range_aided_initialization from the same seed; the driver's
--place-chains."""
import numpy as np
import pytest

import placement_ref as pl
from test_gpu_odom_init import cora_main  # noqa: F401  (the fixture that builds the driver)
from test_placement_cpu import CATALOGUE, SYNTHETIC, case, mirror_of, reference_of, steps_of

pytestmark = pytest.mark.gpu
bits = pl.bits


def same(a, b):
    for key in ("status", "chosen", "degenerate"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("cost_start", "cost_linear", "cost_final", "transforms"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    for key in ("placed", "not_placed", "steps", "n_degenerate", "stages"):
        assert a[key] == b[key], key


def run_all_forms(name, d, gn):
    ctx, dims, table, X, chains, kw, _ = case(name, d, device=0)
    dd = dims[0]
    mirror, ref = mirror_of(name, d, gn), reference_of(name, d, gn)
    assert ctx.chain_placement_counts() == ref["struct"]["counts"]
    assert list(ctx.chain_placement_order()) == [s["chain"] for s in ref["struct"]["stages"]]
    got = ctx.place_chains(X, gn)
    assert np.array_equal(bits(got["X"]), bits(mirror["X"]))
    same(got, mirror)
    got["X_in"] = X
    worst = pl.check(got, *dims, table, ref)
    # the resident form, twice on the same upload: the second call starts from the first one's result
    x = ctx.dev_alloc(dd)
    try:
        ctx.upload(X, x)
        res = ctx.place_chains_dev(x, gn)
        assert np.array_equal(bits(ctx.download(x, dd)), bits(mirror["X"]))
        same(res, mirror)
        again = ctx.place_chains_dev(x, gn)
        twice = ctx.debug_place_chains_host(mirror["X"], gn)
        assert np.array_equal(bits(ctx.download(x, dd)), bits(twice["X"]))
        same(again, twice)
        for c in range(len(again["status"])):   # never worse, as doubles
            assert again["cost_final"][c] <= again["cost_start"][c]
    finally:
        ctx.dev_free(x)
    return worst


@pytest.mark.parametrize("name,d,gn", [(name, d, gn) for name, d in SYNTHETIC for gn in steps_of(name)])
def test_device_on_the_synthetic_cases(name, d, gn):
    worst = run_all_forms(name, d, gn)
    print("%s d=%d gn=%d: worst error / (a + b) %.4f" % (name, d, gn, worst))


@pytest.mark.parametrize("name", CATALOGUE)
def test_device_on_the_catalogue(name):
    worst = run_all_forms(name, None, 5)
    print("%s: worst error / (a + b) %.4f" % (name, worst))


def test_device_refusals():
    """The device forms refuse what the mirror refuses, and report a sum that is not finite through the flag word."""
    from cora_amd import capi
    from test_placement_cpu import ERR_ARG, ERR_NAN, ERR_NOT_READY, ERR_SHAPE, order
    (dims, table, X, chains, _), _, _ = order(3)
    ctx = capi.Context(*dims, *pl.diagonal_q(*dims), device=0)
    x = ctx.dev_alloc(3)
    try:
        def code(fn, *a, **k):
            with pytest.raises(capi.CoraError) as e:
                fn(*a, **k)
            return e.value.code
        assert code(ctx.place_chains_dev, x, 1) == ERR_NOT_READY        # no measurement table
        ctx.set_measurements(*table)
        assert code(ctx.place_chains_dev, x, 1) == ERR_NOT_READY        # no chain tables
        ctx.set_odometry_chains(chains)
        assert code(ctx.place_chains, X, 1) == ERR_NOT_READY            # no placement tables
        assert code(ctx.set_chain_placement, min_ranges=16) == ERR_ARG
        assert code(ctx.set_chain_placement, chain_fixed=[0, 0, 0], min_ranges=17) == ERR_ARG
        ctx.set_chain_placement(min_ranges=17)
        assert code(ctx.place_chains_dev, x, 17) == ERR_ARG and code(ctx.place_chains_dev, x, -1) == ERR_ARG
        assert code(ctx.place_chains_dev, 0, 1) == ERR_ARG              # a null vector
        out = (capi.C.c_int64 * 5)()
        Xf = np.asfortranarray(X)
        none = [None] * 7
        assert ctx.L.cora_place_chains(ctx.h, capi._d(Xf), ctx.N - 1, 1, out, *none) == ERR_SHAPE
        assert ctx.L.cora_place_chains(ctx.h, capi._d(Xf), ctx.N, 1, None, *none) == ERR_ARG
        assert ctx.L.cora_place_chains(ctx.h, capi._d(Xf), ctx.N, 1, out, *none) == 0 and out[0] == 2 and out[1] == 0
        ctx.set_odometry_chains(chains)                                  # new chains: the stages went with the old ones
        assert ctx.chain_placement_counts() == (0, 0, 0, 0) and code(ctx.place_chains, X, 1) == ERR_NOT_READY
        ctx.set_chain_placement(min_ranges=17)
        rd = table[3].copy()
        rd[0, 0] = 1e200   # r^2 overflows
        ctx.set_measurements(table[0], table[1], table[2], rd)
        assert ctx.chain_placement_counts() == (0, 0, 0, 0)             # and with the table
        ctx.set_odometry_chains(chains)
        ctx.set_chain_placement(min_ranges=17)
        ctx.upload(X, x)
        assert code(ctx.place_chains_dev, x, 1) == ERR_NAN
    finally:
        ctx.dev_free(x)


@pytest.mark.parametrize("name", ("pp_only", "robots-d2", "robots-d3", "n1"))
def test_problem_start_against_the_range_aided_start(name):
    """From the same seed: the rows of the chains that are not placed and of the landmarks that are not solved have
    rangeAidedInitialization's bits (the same draws in the same order, the same lift); pose blocks are orthonormal and range
    rows unit; the placed chains are those of the reference run on the odometry start brought back to d columns.  Bound:
    the reference's, C a + b per row, plus the two lifts -- the start is known through x Q and (x Q) Q^T, each (d + 2) eps
    |x| per entry, which moves an entry's points by 2 (d + 2) eps |t| and the transform by kappa times that, and the row
    itself by the same once more (the argument of test_problem_start_against_the_odometry_start)."""
    import odom_ref as od
    import residuals_ref as rr
    import topologies as tp
    A, _, dm, g = tp.build(name)
    d, n, r, nt, p = dm.d, dm.n, dm.r, dm.n_trans, 5
    P = tp.to_problem(name, rank=p)
    mr = pl.unknowns(d) + 1
    old = P.op("odometryInitialization")
    base, binfo = P.range_aided_initialization(seed=7, gn_steps=5)
    new, info = P.multi_robot_initialization(seed=7, gn_steps=5, min_ranges=mr)
    default, dinfo = P.multi_robot_initialization(seed=7, gn_steps=5)
    assert np.array_equal(bits(P.op("multiRobotInitialization")), bits(default))
    assert new.shape == base.shape == (dm.N, p)
    t0 = d * n + r
    table, chains = rr.table(g), od.chains_of(g)
    S = pl.structure(d, n, r, nt, table, chains, None, mr)
    assert info["stages"] == len(S["stages"]) == info["placed"] and len(info["status"]) == len(chains)
    assert info["placed"] + info["not_placed"] == max(len(chains) - 1, 0)
    for res, inf in ((new, info), (default, dinfo)):
        for c in range(len(chains)):
            if inf["status"][c] in (0, 2):
                continue
            for rot, trn in S["positions"][c]:
                assert np.array_equal(bits(res[trn]), bits(base[trn])) and np.array_equal(bits(res[rot:rot + d]), bits(base[rot:rot + d]))
        lm = (inf["landmarks"]["status"] != 0) & (binfo["status"] != 0)
        assert np.array_equal(bits(res[t0 + n:][lm]), bits(base[t0 + n:][lm]))
        if inf["placed"] == 0:
            assert np.array_equal(bits(res), bits(base))
        for i in range(n):
            B = res[d * i:d * i + d]
            assert np.abs(B @ B.T - np.eye(d)).max() < 1e-12
        if r:
            assert np.abs(np.linalg.norm(res[d * n:t0], axis=1) - 1).max() < 1e-12
    if not chains:
        return
    first = table[0][chains[0][0], 0]
    Qd = old[first:first + d]
    assert np.abs(Qd @ Qd.T - np.eye(d)).max() < 1e-14
    x_old, x_new = old @ Qd.T, new @ Qd.T
    ref = pl.reference(d, n, r, nt, table, chains, x_old, 5, min_ranges=mr)
    assert np.array_equal(info["status"], ref["status"])
    scale = np.abs(x_old[t0:t0 + n]).max()
    worst = 0.0
    for k, st in enumerate(S["stages"]):
        one, c = ref["stage"][k], st["chain"]
        kap = max(one["kappa_lin"], one["kappa_gn"], 1.0)
        for rot, trn in S["positions"][c]:
            x, _ = one["rows_before"][trn]
            lift = 2 * (d + 2) * pl.EPS * (scale * (1 + kap) * (1 + float(pl._norm(x - one["q0"])) / one["L"]) + np.abs(x_new[trn]).max())
            bound = pl.C_BOUND * ref["row_a"][trn] + ref["row_b"][trn] + lift
            # (a point whose cost ties with the least within rounding may be taken instead: the nearest visited point)
            err = min(float(pl._norm(x_new[trn] - (Rv @ x + tv))) for Rv, tv in
                      (pl.full_transform(one, one["q0"], one["a0"], v) for v in range(len(one["visited"]))))
            assert err <= bound, (c, trn, err, bound)
            worst = max(worst, err / bound)
    print("%s: %d of %d chains placed (min_ranges %d), largest error / bound %.3f; default min_ranges: %d placed" %
          (name, info["placed"], len(chains), mr, worst, dinfo["placed"]))


def test_driver_place_chains(cora_main):  # noqa: F811
    """cora_main --odom-init --device-init --place-chains --landmark-init on the four-robot data set prints its line, places
    or refuses every chain but the fixed one, lowers the range residual sum of the start it was given, and solves; without
    --device-init the flag is refused."""
    import os
    import re
    import subprocess
    from conftest import GOLDEN
    data = os.path.join(GOLDEN, "datasets", "tiers.pyfg")
    r = subprocess.run([cora_main, data, "--odom-init", "--device-init", "--place-chains", "--landmark-init", "--gn-steps", "5"],
                       stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    m = re.search(r"chain placement: (\d+) chains placed, (\d+) not placed \((\d+) Gauss-Newton steps\); range residual sum at the "
                  r"start ([0-9.eE+-]+) with it, ([0-9.eE+-]+) without", r.stdout)
    assert m, r.stdout[-2000:]
    print(m.group(0))
    assert int(m.group(1)) + int(m.group(2)) == 4 - 1 and int(m.group(3)) <= 5 * int(m.group(1))
    assert float(m.group(4)) < float(m.group(5))
    assert re.search(r"final cost ([0-9.eE+-]+)", r.stdout)
    r = subprocess.run([cora_main, data, "--odom-init", "--place-chains"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "--device-init" in r.stderr
