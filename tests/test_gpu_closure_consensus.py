"""The outlier-robust placement from closures on the device: cora_place_by_closures_robust and the resident
cora_place_by_closures_robust_dev (twice on one upload) bit for bit against the host mirror on every case of
tests/test_closure_consensus_cpu.py -- rows, statuses, costs, chosen, transforms, consensus, list lengths, inlier bytes,
counts --, within the bound of tests/closure_consensus_ref.py; the device error paths; Problem.closure_initialization with a
consensus vote on the path of four robots with one wrong closure added per link (the flags are the construction's, and the
start is better than the plain one's); without the vote it has the plain call's bits; the driver's --closure-consensus."""
import numpy as np
import pytest

import closure_consensus_ref as cc
import closure_ref as cl
from test_closure_consensus_cpu import BARC2, CASES, case, mirror_of, nan_case, reference_of, robust_refusals
from test_gpu_odom_init import cora_main  # noqa: F401  (the fixture that builds the driver)

pytestmark = pytest.mark.gpu
bits = cl.bits
# The path world's chains are composed from odometry (0.01 rad and 0.05 m of noise per step, 40 - 60 steps), so a true
# closure under another true closure's hypothesis carries the drift between their poses.  On the odometry start of the
# contaminated path (d = 2) the reference's residuals fall in two classes, true under true <= 3.5e3 and every other pair
# >= 2.8e4; the threshold is their geometric middle, and the test asserts that nothing lies within a factor of 2 of it.
PATH_BARC2 = 1e4


def same(a, b):
    for key in ("status", "chosen", "consensus", "list_len", "inlier"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("cost_start", "cost_final", "transforms"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    for key in ("placed", "not_placed", "n_degenerate", "stages", "refused", "no_consensus", "excluded"):
        assert a[key] == b[key], key


@pytest.mark.parametrize("name,d", CASES)
def test_device_on_the_cases(name, d):
    ctx, dims, table, X, chains, kw, vote, _, _ = case(name, d, device=0)
    mirror, ref = mirror_of(name, d), reference_of(name, d)
    got = ctx.place_by_closures_robust(X, BARC2, **vote)
    assert np.array_equal(bits(got["X"]), bits(mirror["X"]))
    same(got, mirror)
    got["X_in"] = X
    worst = cc.check(got, *dims, table, ref)
    # the resident form, twice on the same upload: the second call starts from the first one's result
    x = ctx.dev_alloc(d)
    try:
        ctx.upload(X, x)
        res = ctx.place_by_closures_robust_dev(x, BARC2, **vote)
        assert np.array_equal(bits(ctx.download(x, d)), bits(mirror["X"]))
        same(res, mirror)
        again = ctx.place_by_closures_robust_dev(x, BARC2, **vote)
        twice = case(name, d)[0].debug_place_by_closures_robust_host(mirror["X"], BARC2, **vote)
        assert np.array_equal(bits(ctx.download(x, d)), bits(twice["X"]))
        same(again, twice)
        for c in range(len(again["status"])):   # never worse, as doubles
            assert again["cost_final"][c] <= again["cost_start"][c]
    finally:
        ctx.dev_free(x)
    print("%s d=%d: worst error / (a + b) %.4f" % (name, d, worst))


def test_device_refusals():
    """The device forms refuse what the mirror refuses, and report a sum that is not finite through the flag word."""
    from cora_amd import capi
    from test_closure_consensus_cpu import ERR_NAN
    new = lambda dims: capi.Context(*dims, *cl.diagonal_q(*dims), device=0)
    robust_refusals(new, lambda ctx, X, b, m: ctx.place_by_closures_robust(X, b, m),
                    lambda ctx: (ctx.L.cora_place_by_closures_robust, lambda X, ldx: (None if X is None else capi._d(X), ldx)))
    held = []

    def resident(ctx, X, b, m):
        if not held:
            held.append(ctx.dev_alloc(2))
            ctx.upload(X, held[0])
        return ctx.place_by_closures_robust_dev(held[0], b, m)
    ctx = new((2, 100, 0, 100))   # (relay(2)'s dims: the resident vector exists before the tables do)
    try:
        # (the raw C call of the resident form: a device pointer or NULL, no leading dimension)
        robust_refusals(lambda dims: ctx, resident,
                        lambda c: (c.L.cora_place_by_closures_robust_dev, lambda X, ldx: (None if X is None else capi.C.c_void_p(held[0]),)), has_ldx=False)
        with pytest.raises(capi.CoraError) as e:
            ctx.place_by_closures_robust_dev(0, BARC2)      # a null vector
        assert e.value.code == 5
    finally:
        ctx.dev_free(held[0])
    dims, table, X, chains = nan_case()
    ctx = new(dims)
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_closure_placement()
    with pytest.raises(capi.CoraError) as e:
        ctx.place_by_closures_robust(X, BARC2)
    assert e.value.code == ERR_NAN


def _path(contaminated):
    w = cl.path_world(2)
    before = cc.contaminate_world(w) if contaminated else len(w.g.rpms)
    return w, before, cl.world_problem(w, rank=5)


def _unlifted(P, d):
    """The odometry start the closure step sees, d columns, in the frame of the first pose (the residuals and the transforms'
    bound do not depend on the frame): sighting_initialization is the same pipeline without the closure step."""
    x0, _ = P.sighting_initialization(seed=7)
    return x0 @ x0[:d].T


def test_contaminated_path_start():
    """The path of four robots (3 closures per link) with one wrong closure appended per link, a third of the link's.  From
    the same seed the plain closure step fits all four closures of a link and the robust one the three that agree: its inlier
    flags are the construction's, every chain has status 0 and consensus 3, its position RMSE against the truth is strictly
    lower, and so is its objective over the graph's true measurements.  (The objective of the contaminated graph itself
    cannot be lower: per link the plain step takes the exact minimiser of all four closures' cost, wrong one included, and
    the graph's objective is the sum of these costs; it is printed.)  The robust transforms ARE those of the plain placement
    of the clean graph, bit for bit, and so within the reference's bound of it: the wrong closure is the last entry of its
    list and adds +0.0 where the clean list's lane beyond the end adds +0.0."""
    import odom_ref as od
    import residuals_ref as rr
    d = 2
    w, before, P = _path(True)
    _, _, Pc = _path(False)
    gt = w.truth()
    n = len(w.names)
    dims, table, chains = (d, n, 0, n), rr.table(w.g), od.chains_of(w.g)
    plain, pinfo = P.closure_initialization(seed=7)
    robust, info = P.closure_initialization(seed=7, consensus_barc2=PATH_BARC2)
    clean, cinfo = Pc.closure_initialization(seed=7)
    # the reference at the vector the step saw: nothing near the threshold, the same votes and flags
    ref = cc.reference(*dims, table, chains, _unlifted(P, d), PATH_BARC2)
    assert ref["band"] == [], ref["band"]
    assert np.array_equal(info["inlier"], ref["inlier"]) and np.array_equal(info["consensus"], ref["consensus"])
    chain_edges = {e for ch in chains for e in ch}
    built = np.array([2 if e in chain_edges else (1 if e < before else 0) for e in range(len(table[0]))], dtype=np.uint8)
    assert np.array_equal(info["inlier"], built), (info["inlier"][before - 9:], built[before - 9:])
    assert list(info["status"]) == [4, 0, 0, 0] and list(info["consensus"]) == [0, 3, 3, 3] and list(info["list_len"]) == [0, 4, 4, 4]
    assert info["no_consensus"] == 0 and info["excluded"] == 3 and list(pinfo["status"]) == [4, 0, 0, 0]
    r_plain, r_robust = (P.compare(x, gt, proper=False)["trans_rmse"] for x in (plain, robust))
    f_plain, f_robust = (Pc.op("evaluateObjective", x) for x in (plain, robust))
    g_plain, g_robust = (P.op("evaluateObjective", x) for x in (plain, robust))
    print("contaminated path: position RMSE %.4g plain, %.4g robust; objective over the true measurements %.6g plain, %.6g robust "
          "(over the contaminated graph %.6g plain, %.6g robust)" % (r_plain, r_robust, f_plain, f_robust, g_plain, g_robust))
    assert r_robust < r_plain
    assert f_robust < f_plain
    # against the plain placement of the clean graph, the parent's code path: the same sums, the same bits
    assert list(cinfo["status"]) == [4, 0, 0, 0] and np.all(cinfo["chosen"][1:] == 1)
    for key in ("transforms", "cost_start", "cost_final"):
        assert np.array_equal(bits(info[key]), bits(cinfo[key])), (key, info[key], cinfo[key])
    assert np.array_equal(bits(robust), bits(clean))
    assert np.array_equal(bits(P.op("closureInitializationConsensus")), bits(P.closure_initialization(seed=7, consensus_barc2=200.0)[0]))


def test_without_the_vote_the_bits_are_the_plain_calls():
    """consensus_barc2=None is the path of before: the operator form (Problem::closureInitialization with its defaults) and the
    method agree bit for bit, and the info has no field of the vote."""
    _, _, P = _path(True)
    x0, info = P.closure_initialization(seed=7, consensus_barc2=None)
    assert np.array_equal(bits(x0), bits(P.op("closureInitialization")))
    assert np.array_equal(bits(x0), bits(P.closure_initialization(seed=7)[0]))
    assert "inlier" not in info and "consensus" not in info


def test_driver_closure_consensus(cora_main, tmp_path):  # noqa: F811
    """cora_main --closures --closure-consensus on the contaminated path exits 0 and prints the counts of
    test_contaminated_path_start; without --closures the flag is refused."""
    import re
    import subprocess
    w, _, _ = _path(True)
    data = str(tmp_path / "path.pyfg")
    cl.write_pyfg(w, data)
    flags = ["--odom-init", "--device-init", "--closures", "--closure-consensus", "%g" % PATH_BARC2, "--closure-min-consensus", "2"]
    r = subprocess.run([cora_main, data, *flags], stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    m = re.search(r"closure consensus: (\d+) chains without consensus, (\d+) closures excluded; smallest consensus / list length ([0-9.]+)", r.stdout)
    assert m, r.stdout[-2000:]
    print(m.group(0))
    assert [int(m.group(1)), int(m.group(2))] == [0, 3] and float(m.group(3)) == 0.75
    r = subprocess.run([cora_main, data, "--odom-init", "--device-init", "--closure-consensus", "200"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode != 0 and "--closures" in r.stderr
