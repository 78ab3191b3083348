"""The outlier-robust placement from sightings on the device: cora_place_by_sightings_robust and the resident
cora_place_by_sightings_robust_dev (twice on one upload) bit for bit against the host mirror on every case of
tests/test_sighting_consensus_cpu.py -- rows, statuses, costs, chosen, transforms, consensus, list lengths, inlier bytes, all ten
counts --, within the bound of tests/sighting_consensus_ref.py; the device error paths; Problem.sighting_initialization with a
consensus vote on a world of four robots and twelve landmarks with one wrong-id sighting appended per five true ones (the
flags are the construction's, the start is better than the plain one's and has the bits of the plain start of the clean
graph); without the vote it has the plain call's bits; the driver's --sighting-consensus."""
import numpy as np
import pytest

import sighting_consensus_ref as sc
import sighting_ref as sg
from test_gpu_odom_init import cora_main  # noqa: F401  (the fixture that builds the driver)
from test_sighting_consensus_cpu import CASES, ERR_ARG, ERR_NAN, ERR_NOT_READY, ERR_SHAPE, INTS, PLAIN_COUNTS, REALS, case, mirror_of, reference_of, relay

pytestmark = pytest.mark.gpu
bits = sg.bits


def same(a, b):
    for key in INTS:
        assert np.array_equal(a[key], b[key]), key
    for key in REALS[1:]:
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    for key in PLAIN_COUNTS + sc.COUNTS:
        assert a[key] == b[key], key


@pytest.mark.parametrize("name,d", CASES)
def test_device_on_the_cases(name, d):
    ctx, dims, table, X, chains, kw, rkw, _ = case(name, d, device=0)
    mirror, (barc2, ref) = mirror_of(name, d), reference_of(name, d)
    got = ctx.place_by_sightings_robust(X, barc2, **rkw)
    assert np.array_equal(bits(got["X"]), bits(mirror["X"]))
    same(got, mirror)
    got["X_in"] = X
    worst = sc.check(got, *dims, table, ref)
    # the resident form, twice on the same upload: the second call starts from the first one's result
    x = ctx.dev_alloc(d)
    try:
        ctx.upload(X, x)
        res = ctx.place_by_sightings_robust_dev(x, barc2, **rkw)
        assert np.array_equal(bits(ctx.download(x, d)), bits(mirror["X"]))
        same(res, mirror)
        again = ctx.place_by_sightings_robust_dev(x, barc2, **rkw)
        twice = case(name, d)[0].debug_place_by_sightings_robust_host(mirror["X"], barc2, **rkw)
        assert np.array_equal(bits(ctx.download(x, d)), bits(twice["X"]))
        same(again, twice)
        for c in range(len(again["status"])):   # never worse, as doubles
            assert got["cost_final"][c] <= got["cost_start"][c] and again["cost_final"][c] <= again["cost_start"][c]
    finally:
        ctx.dev_free(x)
    print("%s d=%d: worst error / (a + b) %.4f" % (name, d, worst))


def test_device_refusals():
    """The device forms refuse what the mirror refuses, and report a sum that is not finite through the flag word."""
    from cora_amd import capi
    (dims, table, X, chains, _, _), _, _, _ = relay(3)
    ctx = capi.Context(*dims, *sg.diagonal_q(*dims), device=0)
    x = ctx.dev_alloc(3)
    try:
        def code(fn, *a, **k):
            with pytest.raises(capi.CoraError) as e:
                fn(*a, **k)
            return e.value.code
        assert code(ctx.place_by_sightings_robust_dev, x, 1e-8) == ERR_NOT_READY        # no measurement table
        ctx.set_measurements(*table)
        assert code(ctx.place_by_sightings_robust_dev, x, 1e-8) == ERR_NOT_READY        # no chain tables
        ctx.set_odometry_chains(chains)
        assert code(ctx.place_by_sightings_robust, X, 1e-8) == ERR_NOT_READY            # no sighting tables
        ctx.set_sighting_placement()
        assert code(ctx.place_by_sightings_robust_dev, 0, 1e-8) == ERR_ARG              # a null vector
        for bad in (0.0, -1.0, np.inf, np.nan):
            assert code(ctx.place_by_sightings_robust_dev, x, bad) == ERR_ARG and code(ctx.place_by_sightings_robust, X, bad) == ERR_ARG
        assert code(ctx.place_by_sightings_robust, X, 1e-8, min_landmark_consensus=0) == ERR_ARG
        out = (capi.C.c_int64 * 10)()
        Xf = np.asfortranarray(X)
        none = [None] * 14
        b = capi.C.c_double(1e-8)
        assert ctx.L.cora_place_by_sightings_robust(ctx.h, capi._d(Xf), ctx.N, b, 0, 1, out, *none) == ERR_ARG
        assert ctx.L.cora_place_by_sightings_robust(ctx.h, capi._d(Xf), ctx.N - 1, b, 4, 1, out, *none) == ERR_SHAPE
        assert ctx.L.cora_place_by_sightings_robust(ctx.h, capi._d(Xf), ctx.N, b, 4, 1, None, *none) == ERR_ARG
        assert ctx.L.cora_place_by_sightings_robust(ctx.h, capi._d(Xf), ctx.N, b, 4, 1, out, *none) == 0 and out[5] == 5 and out[6] == 0
        ed = table[1].copy()
        ed[table[0][:, 1] < 0, 3 * 3 + 3 + 1] = 1e308   # tau of every sighting: sum tau overflows
        ctx.set_measurements(table[0], ed, table[2], table[3])
        ctx.set_odometry_chains(chains)
        ctx.set_sighting_placement()
        ctx.upload(X, x)
        assert code(ctx.place_by_sightings_robust_dev, x, 1e-8) == ERR_NAN              # through the flag word
        assert code(ctx.place_by_sightings_robust, X, 1e-8) == ERR_NAN
    finally:
        ctx.dev_free(x)


@pytest.fixture(scope="module")
def start(tmp_path_factory):
    """The contaminated world and its clean twin as PyFG files and problems, the start the sighting step sees, the threshold
    and the reference there."""
    import odom_ref as od
    import residuals_ref as rr
    from cora_amd import host
    d = 2
    tmp = tmp_path_factory.mktemp("sighting_consensus")
    w, n_true, n_wrong = sc.start_world()
    wc, _, _ = sc.start_world(contaminated=False)
    paths = str(tmp / "contaminated.pyfg"), str(tmp / "clean.pyfg")
    sc.write_pyfg(w, paths[0])
    sc.write_pyfg(wc, paths[1])
    P, Pc = (host.Problem.from_pyfg(p) for p in paths)
    for q in (P, Pc):
        q.update()
        q.set_rank(5)
    n = len(w.names)
    dims, table, chains = (d, n, 0, n + len(w.L)), rr.table(w.g), od.chains_of(w.g)
    x0 = P.op("odometryInitialization")
    seen = x0 @ x0[:d].T     # d columns, in the frame of the first pose (the residuals do not depend on the frame)
    first = sc.reference(*dims, table, chains, seen, 1e-10)
    barc2 = sc.middle_barc2(first["classes"])
    ref = sc.reference(*dims, table, chains, seen, barc2)
    return dict(w=w, n_true=n_true, n_wrong=n_wrong, paths=paths, P=P, Pc=Pc, dims=dims, table=table, chains=chains, barc2=barc2, ref=ref)


def test_contaminated_start(start):
    """Four robots of 30 poses and 12 landmarks, exact odometry and sightings, 36 true sightings per robot and 7 wrong-id
    sightings appended per robot.  From the same seed the plain sighting step averages the wrong sightings into the landmarks
    and aligns the chains onto them, the robust one votes them out: the reference's band at the vector the step saw is empty,
    the inlier bytes are the construction's, landmark and position RMSE against the truth are strictly lower, and so is the
    objective over the true measurements.  The wrong sightings are the last entries of their lists and add +0.0 where the
    clean list's lanes beyond the end add +0.0: the robust start HAS the bits of the plain start of the clean graph."""
    P, Pc, ref, barc2 = start["P"], start["Pc"], start["ref"], start["barc2"]
    gt = P.ground_truth(start["paths"][0])
    plain, pinfo = P.sighting_initialization(seed=7)
    robust, info = P.sighting_initialization(seed=7, consensus_barc2=barc2)
    clean, cinfo = Pc.sighting_initialization(seed=7)
    print("contaminated start: barc2 %.3e between the residual classes <= %.3e and >= %.3e" % (barc2, *ref["classes"]))
    assert ref["band"] == [], ref["band"][:8]
    for key in sc.INTEGERS:
        assert np.array_equal(info[key], ref[key]), key
    ic, il = sc.built_flags(start["w"], start["table"], start["chains"], start["n_true"])
    assert np.array_equal(info["inlier_chain"], ic) and np.array_equal(info["inlier_landmark"], il)
    assert list(info["status"]) == [4, 0, 0, 0] and np.all(info["landmark_status"] == 0) and list(pinfo["status"]) == [4, 0, 0, 0]
    assert [info[k] for k in ("chains_no_consensus", "landmarks_no_consensus", "chain_excluded", "landmark_excluded")] == [0, 0, 21, 28]
    cmp_plain, cmp_robust = (P.compare(x, gt, proper=False) for x in (plain, robust))
    f_plain, f_robust = (Pc.op("evaluateObjective", x) for x in (plain, robust))
    g_plain, g_robust = (P.op("evaluateObjective", x) for x in (plain, robust))
    print("contaminated start: landmark RMSE %.4g plain, %.4g robust; position RMSE %.4g plain, %.4g robust; objective over the true "
          "measurements %.6g plain, %.6g robust (over the contaminated graph %.6g plain, %.6g robust)" %
          (cmp_plain["landmark_rmse"], cmp_robust["landmark_rmse"], cmp_plain["trans_rmse"], cmp_robust["trans_rmse"], f_plain, f_robust,
           g_plain, g_robust))
    assert cmp_robust["landmark_rmse"] < cmp_plain["landmark_rmse"]
    assert cmp_robust["trans_rmse"] < cmp_plain["trans_rmse"]
    assert f_robust < f_plain
    # against the plain placement of the clean graph, the parent's code path: the same sums, the same bits
    assert list(cinfo["status"]) == [4, 0, 0, 0] and np.all(cinfo["chosen"][1:] == 1)
    for key in ("transforms", "cost_start", "cost_final", "landmark_cost"):
        assert np.array_equal(bits(info[key]), bits(cinfo[key])), (key, info[key], cinfo[key])
    assert np.array_equal(bits(robust), bits(clean))
    assert np.array_equal(bits(P.op("sightingInitializationConsensus")), bits(P.sighting_initialization(seed=7, consensus_barc2=1.0)[0]))


def test_without_the_vote_the_bits_are_the_plain_calls(start):
    """consensus_barc2=None is the path of before: the operator form (Problem::sightingInitialization with its defaults) and the
    method agree bit for bit, and the info has no field of the vote."""
    P = start["P"]
    x0, info = P.sighting_initialization(seed=7, consensus_barc2=None)
    assert np.array_equal(bits(x0), bits(P.op("sightingInitialization")))
    assert np.array_equal(bits(x0), bits(P.sighting_initialization(seed=7)[0]))
    assert not any(k.startswith("inlier") or "consensus" in k or "excluded" in k for k in info)


def test_driver_sighting_consensus(cora_main, start):  # noqa: F811
    """cora_main --sightings --sighting-consensus on the contaminated world exits 0 and prints the counts of
    test_contaminated_start; without --sightings the flag is refused."""
    import re
    import subprocess
    data = start["paths"][0]
    flags = ["--odom-init", "--device-init", "--sightings", "--sighting-consensus", "%.17g" % start["barc2"], "--sighting-min-consensus", "3",
             "--sighting-min-landmark-consensus", "2"]
    r = subprocess.run([cora_main, data, *flags], stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    m = re.search(r"sighting consensus: (\d+) chains without consensus, (\d+) landmarks without consensus, (\d+) chain sightings excluded, "
                  r"(\d+) landmark sightings excluded; smallest consensus / list length ([0-9.]+)", r.stdout)
    assert m, r.stdout[-2000:]
    print(m.group(0))
    assert [int(m.group(k)) for k in (1, 2, 3, 4)] == [0, 0, 21, 28] and 0.5 < float(m.group(5)) < 1.0
    r = subprocess.run([cora_main, data, "--odom-init", "--device-init", "--sighting-consensus", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode != 0 and "--sightings" in r.stderr
