"""The placement from inter-chain relative-pose edges on the device: cora_place_by_closures_dev (twice on one upload) and
cora_place_by_closures bit for bit against the host mirror (cora_debug_place_by_closures_host) on every case of
tests/test_closure_cpu.py -- rows, statuses, costs, chosen, transforms, degenerate flags, counts --, within the bound of
tests/closure_ref.py; the device refusals; Problem.closure_initialization against Problem.sighting_initialization from the
same seed on graphs without inter-chain closures (the same bits) and on a path of four robots that only closures connect
(a strictly lower objective and position RMSE); the operator; the driver's --closures."""
import os

import numpy as np
import pytest

import closure_ref as cl
from conftest import GOLDEN
from test_closure_cpu import SYNTHETIC, case, mirror_of, reference_of
from test_gpu_odom_init import cora_main  # noqa: F401  (the fixture that builds the driver)

pytestmark = pytest.mark.gpu
bits = cl.bits
MRCLAM5A = os.path.join(GOLDEN, "datasets", "mrclam5a.pyfg")


def same(a, b):
    for key in ("status", "chosen", "degenerate"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("cost_start", "cost_final", "transforms"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    for key in ("placed", "not_placed", "n_degenerate", "stages", "refused"):
        assert a[key] == b[key], key


@pytest.mark.parametrize("name,d", SYNTHETIC)
def test_device_on_the_synthetic_cases(name, d):
    ctx, dims, table, X, chains, kw, _, _ = case(name, d, device=0)
    mirror, ref = mirror_of(name, d), reference_of(name, d)
    assert ctx.closure_placement_counts() == ref["struct"]["counts"]
    assert [list(map(int, items)) for items in ctx.closure_placement_order()] == ref["struct"]["order"]
    got = ctx.place_by_closures(X)
    assert np.array_equal(bits(got["X"]), bits(mirror["X"]))
    same(got, mirror)
    got["X_in"] = X
    worst = cl.check(got, *dims, table, ref)
    # the resident form, twice on the same upload: the second call starts from the first one's result
    dd = dims[0]
    x = ctx.dev_alloc(dd)
    try:
        ctx.upload(X, x)
        res = ctx.place_by_closures_dev(x)
        assert np.array_equal(bits(ctx.download(x, dd)), bits(mirror["X"]))
        same(res, mirror)
        again = ctx.place_by_closures_dev(x)
        twice = ctx.debug_place_by_closures_host(mirror["X"])
        assert np.array_equal(bits(ctx.download(x, dd)), bits(twice["X"]))
        same(again, twice)
        for c in range(len(again["status"])):   # never worse, as doubles
            assert again["cost_final"][c] <= again["cost_start"][c]
        # and within the reference's bound from where the first call ended
        again.update(X=ctx.download(x, dd), X_in=mirror["X"])
        cl.check(again, *dims, table, cl.reference(*dims, table, chains, mirror["X"], **kw))
    finally:
        ctx.dev_free(x)
    print("%s d=%d: worst error / (a + b) %.4f" % (name, d, worst))


def test_device_refusals():
    """The device forms refuse what the mirror refuses, and report a sum that is not finite through the flag word."""
    from cora_amd import capi
    from test_closure_cpu import ERR_ARG, ERR_NAN, ERR_NOT_READY, ERR_SHAPE, relay
    (dims, table, X, chains, _), _, _ = relay(3)
    ctx = capi.Context(*dims, *cl.diagonal_q(*dims), device=0)
    x = ctx.dev_alloc(3)
    try:
        def code(fn, *a, **k):
            with pytest.raises(capi.CoraError) as e:
                fn(*a, **k)
            return e.value.code
        assert code(ctx.place_by_closures_dev, x) == ERR_NOT_READY        # no measurement table
        ctx.set_measurements(*table)
        assert code(ctx.place_by_closures_dev, x) == ERR_NOT_READY        # no chain tables
        ctx.set_odometry_chains(chains)
        assert code(ctx.place_by_closures, X) == ERR_NOT_READY            # no closure tables
        assert code(ctx.set_closure_placement, min_closures=0) == ERR_ARG
        assert code(ctx.set_closure_placement, chain_fixed=[0, 0, 0, 0]) == ERR_ARG
        ctx.set_closure_placement(min_closures=4)
        assert code(ctx.place_by_closures_dev, 0) == ERR_ARG              # a null vector
        out = (capi.C.c_int64 * 5)()
        Xf = np.asfortranarray(X)
        none = [None] * 6
        assert ctx.L.cora_place_by_closures(ctx.h, capi._d(Xf), ctx.N - 1, out, *none) == ERR_SHAPE
        assert ctx.L.cora_place_by_closures(ctx.h, capi._d(Xf), ctx.N, None, *none) == ERR_ARG
        assert ctx.L.cora_place_by_closures(ctx.h, capi._d(Xf), ctx.N, out, *none) == 0 and list(out) == [3, 0, 0, 3, 0]
        ctx.set_odometry_chains(chains)                                  # new chains: the lists went with the old ones
        assert ctx.closure_placement_counts() == (0, 0, 0, 0) and code(ctx.place_by_closures, X) == ERR_NOT_READY
        ctx.set_closure_placement()
        ed = table[1].copy()
        ed[len(table[0]) - 18:, 3 * 3 + 3 + 1] = 1e308   # tau of every closure: sum tau overflows
        ctx.set_measurements(table[0], ed, table[2], table[3])
        assert ctx.closure_placement_counts() == (0, 0, 0, 0)             # and with the table
        ctx.set_odometry_chains(chains)
        ctx.set_closure_placement()
        ctx.upload(X, x)
        assert code(ctx.place_by_closures_dev, x) == ERR_NAN
    finally:
        ctx.dev_free(x)


def _no_op(P):
    old, oinfo = P.sighting_initialization(seed=7)
    new, info = P.closure_initialization(seed=7)
    assert info["stages"] == 0 and info["placed"] == 0 and info["closures_used"] == 0 and info["fixed"] == 1
    assert info["status"][0] == 4 and np.all(info["status"][1:] == 3)
    assert np.array_equal(info["sightings"]["status"], oinfo["status"]) and np.array_equal(info["chains"]["status"], oinfo["chains"]["status"])
    assert np.array_equal(bits(new), bits(old))
    return info


@pytest.mark.parametrize("name", ("robots-d2", "robots-d3"))
def test_intra_chain_closures_only_is_a_no_op(name):
    """On a catalogue graph whose closures all lie inside one chain the step takes nothing and draws nothing:
    sighting_initialization's bits, and the 12 closures are counted as skipped."""
    import topologies as tp
    info = _no_op(tp.to_problem(name, rank=5))
    assert info["edges_skipped"] == 12


def test_mrclam5a_is_a_no_op():
    """mrclam5a has no relative-pose edge outside the chains: sighting_initialization's bits."""
    from cora_amd import host
    P = host.Problem.from_pyfg(MRCLAM5A)
    P.update()
    P.set_rank(5)
    info = _no_op(P)
    assert info["edges_skipped"] == 0


def test_path_of_four_robots_start():
    """Four robots on a path A - B - C - D that only closures connect (no ranges, no landmarks): sighting_initialization
    leaves B, C and D at their random draws, closure_initialization places them in three stages.  The lifted start has a
    strictly lower objective and a strictly lower position RMSE against the truth; the operator has the method's bits."""
    w = cl.path_world(2)
    P = cl.world_problem(w, rank=5)
    gt = w.truth()
    old, oinfo = P.sighting_initialization(seed=7)
    new, info = P.closure_initialization(seed=7)
    assert list(info["status"]) == [4, 0, 0, 0] and info["stages"] == 3 and info["closures_used"] == 9 and info["edges_skipped"] == 0
    assert np.all(info["chosen"][1:] == 1) and np.all(info["cost_final"][1:] < info["cost_start"][1:])
    assert list(info["sightings"]["status"]) == [4, 4, 4, 4]   # the closure step's chains are the sighting step's fixed set
    f_old, f_new = P.op("evaluateObjective", old), P.op("evaluateObjective", new)
    r_old, r_new = P.compare(old, gt, proper=False)["trans_rmse"], P.compare(new, gt, proper=False)["trans_rmse"]
    print("path of four robots: f(x0) %.6g -> %.6g; position RMSE %.4g -> %.4g; closure cost per chain %s -> %s" %
          (f_old, f_new, r_old, r_new, info["cost_start"], info["cost_final"]))
    assert f_new < f_old
    assert r_new < r_old
    assert np.array_equal(bits(P.op("closureInitialization")), bits(new))


def test_driver_closures(cora_main, tmp_path):  # noqa: F811
    """cora_main --odom-init --device-init --closures on the path of four robots exits 0 and prints the counts of
    test_path_of_four_robots_start and a closure cost that fell; without --device-init the flag is refused."""
    import re
    import subprocess
    data = str(tmp_path / "path.pyfg")
    cl.write_pyfg(cl.path_world(2), data)
    r = subprocess.run([cora_main, data, "--odom-init", "--device-init", "--closures"], stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    m = re.search(r"closure placement: (\d+) chains fixed or placed, (\d+) not placed, (\d+) refused \((\d+) stages, (\d+) closures used, "
                  r"(\d+) edges skipped or unused\); closure cost at the start ([0-9.eE+-]+) with it, ([0-9.eE+-]+) without", r.stdout)
    assert m, r.stdout[-2000:]
    print(m.group(0))
    assert [int(m.group(k)) for k in range(1, 7)] == [4, 0, 0, 3, 9, 0]
    assert float(m.group(7)) < float(m.group(8))
    r = subprocess.run([cora_main, data, "--odom-init", "--closures"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "--device-init" in r.stderr
