"""The placement from pose-landmark sightings on the device: cora_place_by_sightings_dev (twice on one upload) and
cora_place_by_sightings bit for bit against the host mirror (cora_debug_place_by_sightings_host) on every case of
tests/test_sighting_cpu.py -- rows, statuses, costs, chosen, transforms, degenerate flags, counts --, within the bound of
tests/sighting_ref.py; the device refusals; Problem.sighting_initialization against Problem.multi_robot_initialization from
the same seed on mrclam5a and on a graph without sightings; the driver's --sightings."""
import os

import numpy as np
import pytest

import sighting_ref as sg
from conftest import GOLDEN
from test_gpu_odom_init import cora_main  # noqa: F401  (the fixture that builds the driver)
from test_sighting_cpu import SYNTHETIC, case, mirror_of, reference_of

pytestmark = pytest.mark.gpu
bits = sg.bits
MRCLAM5A = os.path.join(GOLDEN, "datasets", "mrclam5a.pyfg")


def same(a, b):
    for key in ("status", "chosen", "landmark_status", "degenerate"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("cost_start", "cost_final", "transforms", "landmark_cost"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    for key in ("placed", "not_placed", "landmarks_placed", "landmarks_not_placed", "n_degenerate", "stages"):
        assert a[key] == b[key], key


@pytest.mark.parametrize("name,d", SYNTHETIC)
def test_device_on_the_synthetic_cases(name, d):
    ctx, dims, table, X, chains, kw, _, _ = case(name, d, device=0)
    mirror, ref = mirror_of(name, d), reference_of(name, d)
    assert ctx.sighting_placement_counts() == ref["struct"]["counts"]
    assert [(k, list(map(int, items))) for k, items in ctx.sighting_placement_order()] == ref["struct"]["order"]
    got = ctx.place_by_sightings(X)
    assert np.array_equal(bits(got["X"]), bits(mirror["X"]))
    same(got, mirror)
    got["X_in"] = X
    worst = sg.check(got, *dims, table, ref)
    # the resident form, twice on the same upload: the second call starts from the first one's result
    dd = dims[0]
    x = ctx.dev_alloc(dd)
    try:
        ctx.upload(X, x)
        res = ctx.place_by_sightings_dev(x)
        assert np.array_equal(bits(ctx.download(x, dd)), bits(mirror["X"]))
        same(res, mirror)
        again = ctx.place_by_sightings_dev(x)
        twice = ctx.debug_place_by_sightings_host(mirror["X"])
        assert np.array_equal(bits(ctx.download(x, dd)), bits(twice["X"]))
        same(again, twice)
        for c in range(len(again["status"])):   # never worse, as doubles
            assert again["cost_final"][c] <= again["cost_start"][c]
    finally:
        ctx.dev_free(x)
    print("%s d=%d: worst error / (a + b) %.4f" % (name, d, worst))


def test_device_refusals():
    """The device forms refuse what the mirror refuses, and report a sum that is not finite through the flag word."""
    from cora_amd import capi
    from test_sighting_cpu import ERR_ARG, ERR_NAN, ERR_NOT_READY, ERR_SHAPE, relay
    (dims, table, X, chains, _, _), _, _ = relay(3)
    ctx = capi.Context(*dims, *sg.diagonal_q(*dims), device=0)
    x = ctx.dev_alloc(3)
    try:
        def code(fn, *a, **k):
            with pytest.raises(capi.CoraError) as e:
                fn(*a, **k)
            return e.value.code
        assert code(ctx.place_by_sightings_dev, x) == ERR_NOT_READY        # no measurement table
        ctx.set_measurements(*table)
        assert code(ctx.place_by_sightings_dev, x) == ERR_NOT_READY        # no chain tables
        ctx.set_odometry_chains(chains)
        assert code(ctx.place_by_sightings, X) == ERR_NOT_READY            # no sighting tables
        assert code(ctx.set_sighting_placement, min_sightings=2) == ERR_ARG
        assert code(ctx.set_sighting_placement, chain_fixed=[0, 0, 0]) == ERR_ARG
        ctx.set_sighting_placement()
        assert code(ctx.place_by_sightings_dev, 0) == ERR_ARG              # a null vector
        out = (capi.C.c_int64 * 6)()
        Xf = np.asfortranarray(X)
        none = [None] * 8
        assert ctx.L.cora_place_by_sightings(ctx.h, capi._d(Xf), ctx.N - 1, out, *none) == ERR_SHAPE
        assert ctx.L.cora_place_by_sightings(ctx.h, capi._d(Xf), ctx.N, None, *none) == ERR_ARG
        assert ctx.L.cora_place_by_sightings(ctx.h, capi._d(Xf), ctx.N, out, *none) == 0 and out[0] == 2 and out[2] == 8 and out[5] == 5
        ctx.set_odometry_chains(chains)                                  # new chains: the lists went with the old ones
        assert ctx.sighting_placement_counts() == (0, 0, 0, 0) and code(ctx.place_by_sightings, X) == ERR_NOT_READY
        ctx.set_sighting_placement()
        ed = table[1].copy()
        ed[table[0][:, 1] < 0, 3 * 3 + 3 + 1] = 1e308   # tau of every sighting: sum tau overflows
        ctx.set_measurements(table[0], ed, table[2], table[3])
        assert ctx.sighting_placement_counts() == (0, 0, 0, 0)             # and with the table
        ctx.set_odometry_chains(chains)
        ctx.set_sighting_placement()
        ctx.upload(X, x)
        assert code(ctx.place_by_sightings_dev, x) == ERR_NAN
    finally:
        ctx.dev_free(x)


def test_mrclam5a_start():
    """mrclam5a (1 080 poses, 1 127 sightings, no pose-landmark range): the sighting step fixes or places all 5 chains and
    places all 15 landmarks; the lifted start has a strictly lower objective and a strictly lower landmark RMSE against the
    file's ground truth than multi_robot_initialization from the same seed."""
    from cora_amd import host
    P = host.Problem.from_pyfg(MRCLAM5A)
    P.update()
    P.set_rank(5)
    dm = P.dims()
    assert dm["n"] == 1080
    gt = P.ground_truth(MRCLAM5A)
    old, _ = P.multi_robot_initialization(seed=7)
    new, info = P.sighting_initialization(seed=7)
    assert len(P.measurement_residuals(new)["pose_landmark"]) == 1127
    assert info["fixed"] + info["placed"] == 5 and info["landmarks_placed"] == 15, info
    f_old, f_new = P.op("evaluateObjective", old), P.op("evaluateObjective", new)
    r_old, r_new = P.compare(old, gt, proper=False)["landmark_rmse"], P.compare(new, gt, proper=False)["landmark_rmse"]
    print("mrclam5a: f(x0) %.6g -> %.6g; landmark RMSE %.4g -> %.4g m; statuses %s, range placement %s" %
          (f_old, f_new, r_old, r_new, info["status"], info["chains"]))
    assert f_new < f_old
    assert r_new < r_old
    assert np.array_equal(bits(P.op("sightingInitialization")), bits(new))


@pytest.mark.parametrize("name", ("robots-d2", "robots-d3"))
def test_no_sightings_is_a_no_op(name):
    """On a catalogue graph without sightings the step takes nothing and draws nothing: multi_robot_initialization's bits."""
    import topologies as tp
    P = tp.to_problem(name, rank=5)
    old, oinfo = P.multi_robot_initialization(seed=7)
    new, info = P.sighting_initialization(seed=7)
    assert info["stages"] == 0 and info["placed"] == 0 and info["landmarks_placed"] == 0
    assert np.array_equal(info["chains"]["status"], oinfo["status"])
    assert np.array_equal(bits(new), bits(old))


def test_driver_sightings(cora_main):  # noqa: F811
    """cora_main --odom-init --device-init --sightings on mrclam5a exits 0 and prints the counts of test_mrclam5a_start;
    without --device-init the flag is refused."""
    import re
    import subprocess
    r = subprocess.run([cora_main, MRCLAM5A, "--odom-init", "--device-init", "--sightings"], stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    m = re.search(r"sighting placement: (\d+) chains fixed or placed, (\d+) not placed; (\d+) landmarks placed, (\d+) not placed \((\d+) stages\); "
                  r"sighting cost at the start ([0-9.eE+-]+) with it, ([0-9.eE+-]+) without", r.stdout)
    assert m, r.stdout[-2000:]
    print(m.group(0))
    assert [int(m.group(k)) for k in (1, 2, 3, 4)] == [5, 0, 15, 0]
    assert float(m.group(6)) < float(m.group(7))
    r = subprocess.run([cora_main, MRCLAM5A, "--odom-init", "--sightings"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "--device-init" in r.stderr
