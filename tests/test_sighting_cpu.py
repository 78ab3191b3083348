"""The placement from pose-landmark sightings without a GPU: cora_debug_place_by_sightings_host (the functions the kernels
call, in the device's bracket order, on plan-only handles) against the longdouble / mpmath reference of tests/sighting_ref.py
-- the order of the stages, counts, statuses, chosen, the degenerate flags, the transforms and every written row within the
derived bound, never worse on the sighting cost -- on lists that sit on every boundary of the reduction's shape, with several
chains in one C-stage, a relay through a landmark only a placed chain sees, degenerate geometry on either side of the refusal
rule, masks, skipped edges, and every refusal.  The device forms against the mirror, bit for bit: tests/test_gpu_sighting.py."""
import numpy as np
import pytest

import sighting_ref as sg
import topologies as tp
from cora_amd import capi

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
LIST_LENS = (1, 255, 256, 257, 64 * 256 + 1)   # the last wraps the fold's lane loop

_BUILT = {}


def _see(rng, first, length, lms, k):
    """k sightings from random positions of the chain [first, first + length) of the landmarks lms in turn."""
    return [(first + int(rng.integers(length)), lms[j % len(lms)]) for j in range(k)]


def lengths(d, noise=0.0, offset=0.0):
    """Chain 0 (30 poses, fixed) sights landmark j with LIST_LENS[j] sightings: the L-stage's lists.  Chains 1 .. 5 (40 poses
    each, each in a frame of its own) sight landmarks 1 .. 4 with d, 255, 256, 257 and 64 * 256 + 1 sightings: five lists of
    ONE C-stage.  Landmark 5 is sighted by chain 5 only: a second L-stage.  Weights in [0.5, 2], the table shuffled."""
    rng = np.random.default_rng(240 + d)
    sights = []
    for j, k in enumerate(LIST_LENS):
        sights += _see(rng, 0, 30, [j], k)
    for c, k in enumerate((d,) + LIST_LENS[1:]):
        sights += _see(rng, 30 + 40 * c, 40, [1, 2, 3, 4], k)
    sights += _see(rng, 30 + 40 * 4, 40, [5], 3)
    sights = [sights[i] for i in rng.permutation(len(sights))]
    tau = rng.uniform(0.5, 2.0, len(sights))
    expect = [("L", [0, 1, 2, 3, 4]), ("C", [1, 2, 3, 4, 5]), ("L", [5]), ("REFIT", [0, 1, 2, 3, 4, 5])]
    return sg.scene(d, [30] + [40] * 5, sights, seed=d, n_lm=6, noise=noise, tau=tau, offset=offset), dict(min_sightings=d), expect


def side_by_side(d, chains_taken):
    """Two / three chains taken in ONE C-stage, default min_sightings, noisy sightings."""
    rng = np.random.default_rng(250 + d + chains_taken)
    sights = _see(rng, 0, 30, list(range(6)), 60)
    for c in range(chains_taken):
        sights += _see(rng, 30 + 25 * c, 25, list(range(6)), 40 + c)
    sights = [sights[i] for i in rng.permutation(len(sights))]
    expect = [("L", list(range(6))), ("C", list(range(1, chains_taken + 1))), ("REFIT", list(range(6)))]
    return sg.scene(d, [30] + [25] * chains_taken, sights, seed=10 + d, n_lm=6, noise=0.05), {}, expect


def relay(d):
    """Chain 1 sights landmarks 0 .. 3 (which chain 0 sights) and 4 .. 7 (which only chains 1 and 2 sight); chain 2 sights
    4 .. 7 only: it becomes placeable through landmarks that the first C-stage's chain placed.  L, C, L, C, REFIT.  18 range
    measurements between the chains and to the landmarks have their rows recomputed."""
    rng = np.random.default_rng(260 + d)
    sights = _see(rng, 0, 30, [0, 1, 2, 3], 40) + _see(rng, 30, 30, list(range(8)), 80) + _see(rng, 60, 30, [4, 5, 6, 7], 40)
    sights = [sights[i] for i in rng.permutation(len(sights))]
    expect = [("L", [0, 1, 2, 3]), ("C", [1]), ("L", [4, 5, 6, 7]), ("C", [2]), ("REFIT", list(range(8)))]
    ranges = [(int(a), 30 + int(b)) if m % 2 else (60 + int(b), int(a)) for m, (a, b) in enumerate(rng.integers(30, size=(12, 2)))]
    ranges += [(int(a), 90 + int(l)) for a, l in zip(rng.integers(90, size=6), rng.integers(8, size=6))]   # pose - landmark
    return sg.scene(d, [30, 30, 30], sights, seed=20 + d, n_lm=8, noise=0.02, ranges=ranges), {}, expect


def statuses(d):
    """Default min_sightings (4 d).  Chain 1 is placed; chain 2 has 4 d - 1 sightings (status 1); chain 3 sights ONE landmark
    4 d + 5 times (status 1 by the distinct count); chain 4 has no sighting (status 3).  Landmark 6 is fixed and keeps its row
    through the REFIT although chains 0 and 1 sight it; landmark 7 is sighted by chain 2 only (status 1); landmark 8 by
    nobody; every sighting of landmark 9 has tau = 0 (status 2).  Skipped: a landmark prior (from the origin, a free pose),
    a sighting from the other free pose and an edge without a second rotation between two poses."""
    rng = np.random.default_rng(270 + d)
    n = 30 + 30 + 20 + 20 + 10
    sights = _see(rng, 0, 30, list(range(7)), 70) + _see(rng, 30, 30, list(range(7)), 50)
    sights += _see(rng, 60, 20, [0, 1, 2, 7], 4 * d - 1) + _see(rng, 80, 20, [3], 4 * d + 5)
    sights += _see(rng, 0, 30, [9], 5)
    sights = [sights[i] for i in rng.permutation(len(sights))]
    tau = [0.0 if l == 9 else 1.0 for _, l in sights] + [1.0, 1.0]
    sights += [(n, 2), (n + 1, 4)]
    known = [0] * 10
    known[6] = 1
    expect = [("L", [0, 1, 2, 3, 4, 5, 9]), ("C", [1]), ("REFIT", [0, 1, 2, 3, 4, 5, 9])]
    return (sg.scene(d, [30, 30, 20, 20, 10], sights, seed=30 + d, n_free=2, n_lm=10, noise=0.02, tau=tau, known=(6,), pose_sights=[(3, 40)]),
            dict(landmark_fixed=known), expect)


def degenerate(d):
    """Every landmark fixed at its true place (no L-stage, no REFIT).  Chain 1 sights landmarks 0 .. 3, all at ONE point
    (status 2: no spread).  Chain 2 sights 4 .. 8 on a line: refused at d = 3 (rank 1), placed at d = 2.  Chain 3 sights 9 ..
    13 on a line with a scatter of 1e-3 of its length: placed.  Chain 4 sights 14 .. 18 in general position: placed.  The
    refused chains keep their rows.  Exact sightings."""
    rng = np.random.default_rng(280 + d)
    lm = np.zeros((19, d))
    lm[0:4] = rng.uniform(-5, 5, d)
    u = rng.normal(0, 1, d)
    u /= np.linalg.norm(u)
    lm[4:9] = rng.uniform(-5, 5, d) + np.outer(np.linspace(0, 40, 5), u)
    lm[9:14] = rng.uniform(-5, 5, d) + np.outer(np.linspace(0, 40, 5), u) + 0.04 * rng.normal(0, 1, (5, d))
    lm[14:19] = rng.uniform(-20, 20, (5, d))
    sights = []
    for c in range(4):
        sights += _see(rng, 20 + 25 * c, 25, list(range((0, 4, 9, 14)[c], (4, 9, 14, 19)[c])), 50)
    expect = [("C", [1, 2, 3, 4])]
    return sg.scene(d, [20] + [25] * 4, sights, seed=40 + d, n_lm=19, lm_world=lm, known=tuple(range(19))), dict(landmark_fixed=[1] * 19), expect


def in_place(d):
    """A chain already in place, on exactly representable data: unit steps along the first axis, identity rotations,
    landmarks on integer points, fixed.  cost_start is 0 exactly, so nothing is below it: chosen 0, the rows bit-identical."""
    n, nl = 12 + 12, 5
    t0 = d * n
    X = np.zeros((t0 + n + nl, d))
    er, ed, chains = [], [], []
    for c in range(2):
        chains.append(list(range(len(er), len(er) + 11)))
        for i in range(12 * c, 12 * c + 12):
            X[d * i:d * i + d] = np.eye(d)
            X[t0 + i, 0], X[t0 + i, 1] = i - 12 * c, 7 * c
            if i < 12 * c + 11:
                er.append([d * i, d * (i + 1), t0 + i, t0 + i + 1])
                ed.append(np.concatenate([np.eye(d).reshape(-1), np.eye(d)[0], [1.0, 1.0]]))
    rng = np.random.default_rng(290 + d)
    X[t0 + n:] = rng.integers(-8, 9, (nl, d))
    for k in range(8 * d):
        i, l = 12 + int(rng.integers(12)), k % nl
        er.append([d * i, -1, t0 + i, t0 + n + l])
        ed.append(np.concatenate([np.zeros(d * d), X[t0 + n + l] - X[t0 + i], [0.0, 1.0]]))
    table = (np.array(er, dtype=np.int32), np.array(ed), np.zeros((0, 3), dtype=np.int32), np.zeros((0, 2)))
    return ((d, n, 0, n + nl), table, X, chains, None, X[t0 + n:].copy()), dict(landmark_fixed=[1] * nl), [("C", [1])]


BUILDERS = dict(lengths=lengths, lengths_noisy=lambda d: lengths(d, noise=0.1), offset=lambda d: lengths(d, offset=1e4),
                two_chains=lambda d: side_by_side(d, 2), three_chains=lambda d: side_by_side(d, 3), relay=relay, statuses=statuses,
                degenerate=degenerate, in_place=in_place)
SYNTHETIC = [(name, d) for name in BUILDERS for d in (2, 3)]


def case(name, d, device=-1):
    """(ctx, dims, table, X, chains, kw, expect, truth) of a synthetic case, tables installed."""
    key = (name, d, device)
    if key not in _BUILT:
        (dims, table, X, chains, truth, lm_true), kw, expect = BUILDERS[name](d)
        ctx = capi.Context(*dims, *sg.diagonal_q(*dims), device=device)
        ctx.set_measurements(*table)
        ctx.set_odometry_chains(chains)
        ctx.set_sighting_placement(**kw)
        _BUILT[key] = (ctx, dims, table, X, chains, kw, expect, truth)
    return _BUILT[key]


def reference_of(name, d):
    """Computed once and shared (tests/test_gpu_sighting.py reads the same)."""
    key = ("ref", name, d)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, _, _ = case(name, d)
        _BUILT[key] = sg.reference(*dims, table, chains, X, **kw)
    return _BUILT[key]


def mirror_of(name, d):
    key = ("mirror", name, d)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, _, _ = case(name, d)
        got = ctx.debug_place_by_sightings_host(X)
        got["X_in"] = X
        _BUILT[key] = got
    return _BUILT[key]


def check_structure(ctx, ref):
    assert ctx.sighting_placement_counts() == ref["struct"]["counts"]
    order = ctx.sighting_placement_order()
    assert [(k, list(map(int, items))) for k, items in order] == ref["struct"]["order"]


def all_sightings(table, ref):
    """The edges of every list of the REFIT (all sightings of unfixed landmarks by placed chains) and of the C-stages."""
    es = set()
    for st in ref["struct"]["stages"]:
        if st["kind"] != "L":
            for _, e in st["lists"]:
                es.update(e)
    return sorted(es)


@pytest.mark.parametrize("name,d", SYNTHETIC)
def test_mirror_on_the_synthetic_cases(name, d):
    ctx, dims, table, X, chains, kw, expect, truth = case(name, d)
    ref, got = reference_of(name, d), mirror_of(name, d)
    check_structure(ctx, ref)
    assert ref["struct"]["order"] == expect, ref["struct"]["order"]
    worst = sg.check(got, *dims, table, ref)
    kap = max([one.get("kappa", 0.0) for one in ref["chain"].values()] + [0.0])
    print("%s d=%d: worst error / (a + b) %.4f (largest condition %.3g); statuses %s chosen %s landmarks %s" %
          (name, d, worst, kap, got["status"], got["chosen"], got["landmark_status"]))
    for c in range(len(chains)):
        assert got["cost_final"][c] <= got["cost_start"][c]
    # the REFIT does not raise the total sighting cost over the placed chains (the weighted mean minimises it for the poses
    # as they stand): against the landmarks' rows before the REFIT, in longdouble
    es = all_sightings(table, ref)
    t0 = dims[0] * dims[1] + dims[2]
    before = np.array(got["X"], dtype=sg.LD)
    before[t0 + dims[1]:] = ref["X_before_refit"][t0 + dims[1]:]
    c_after, c_before = sg.sighting_cost(*dims[:3], table, got["X"], es), sg.sighting_cost(*dims[:3], table, before, es)
    assert c_after <= c_before * (1 + 64 * sg.EPS) + 1e-300, (float(c_after), float(c_before))
    if name.startswith("lengths") or name == "offset":
        assert list(got["status"]) == [4, 0, 0, 0, 0, 0] and np.all(got["landmark_status"] == 0) and got["placed"] == 5
    if name in ("two_chains", "three_chains", "relay"):
        assert np.all(got["status"][1:] == 0) and np.all(got["chosen"][1:] == 1) and got["landmarks_not_placed"] == 0
    if name == "statuses":
        assert list(got["status"]) == [4, 0, 1, 1, 3] and list(got["landmark_status"]) == [0, 0, 0, 0, 0, 0, 3, 1, 1, 2]
        assert ref["struct"]["skipped"] == 3 and got["placed"] == 1 and got["not_placed"] == 3
        assert got["landmarks_placed"] == 6 and got["landmarks_not_placed"] == 3
        assert np.array_equal(sg.bits(got["X"][t0 + dims[1] + 6]), sg.bits(X[t0 + dims[1] + 6]))   # the fixed landmark's row
    if name == "degenerate":
        assert list(got["status"]) == ([4, 2, 0, 0, 0] if d == 2 else [4, 2, 2, 0, 0]) and np.all(got["landmark_status"] == 3)
        for c in range(1, 5):   # either side of the rule, 100 x away in the reference's singular values
            m = ref["chain"][c]["margin"]
            print("  chain %d: status %d, the rule's quantity / threshold %s" % (c, got["status"][c], m))
            assert m is None or m >= 100 or m <= 0.01, (c, m)
    if name == "in_place":
        assert list(got["status"]) == [4, 0] and got["chosen"][1] == 0 and got["cost_start"][1] == 0
        assert np.array_equal(sg.bits(got["X"]), sg.bits(X))


@pytest.mark.parametrize("name,d", [(name, d) for name in ("lengths", "offset") for d in (2, 3)])
def test_exact_data(name, d):
    """Noise-free sightings, every chain displaced by a known rigid motion: the transform is the truth's within the bound,
    and the sighting cost afterwards is <= 1e-18 sum tau |t|^2 (composition error is n eps per length, squared, n <= 1e3)."""
    ctx, dims, table, X, chains, kw, expect, truth = case(name, d)
    ref, got = reference_of(name, d), mirror_of(name, d)
    es = all_sightings(table, ref)
    ed = table[1][es]
    scale = float(np.sum(ed[:, d * d + d + 1] * np.sum(ed[:, d * d:d * d + d] ** 2, axis=1)))
    after, before = float(sg.sighting_cost(*dims[:3], table, got["X"], es)), float(sg.sighting_cost(*dims[:3], table, X, es))
    print("%s d=%d: sighting cost %.3e -> %.3e, sum tau |t|^2 %.3e" % (name, d, before, after, scale))
    assert after <= 1e-18 * scale and not before <= 1e-18 * scale
    for c in range(1, len(chains)):
        Rc, tc = truth[c]
        one = ref["chain"][c]
        a_T = one["a_R"] * float(sg._norm(one["cp"])) + one["a_t"]
        # (the truth is the reference's minimiser up to the rounding of the data it was built from)
        slack = 64 * sg.EPS * (1 + np.linalg.norm(tc) + float(sg._norm(one["cp"]))) * max(one["kappa"], 1.0)
        assert np.abs(got["transforms"][c][:d * d].reshape(d, d) - Rc).max() <= sg.C_BOUND * one["a_R"] + slack
        assert np.abs(got["transforms"][c][d * d:] - tc).max() <= sg.C_BOUND * a_T + one["b_t"] + slack * (1 + float(sg._norm(one["cp"])))


@pytest.mark.parametrize("name,d", [("lengths_noisy", 2), ("relay", 3), ("degenerate", 3)])
def test_two_calls_give_the_same_bits(name, d):
    ctx, dims, table, X, chains, kw, _, _ = case(name, d)
    a, b = mirror_of(name, d), ctx.debug_place_by_sightings_host(X)
    for key in ("X", "cost_start", "cost_final", "transforms", "landmark_cost"):
        assert np.array_equal(sg.bits(a[key]), sg.bits(b[key])), key
    for key in ("status", "chosen", "landmark_status", "degenerate"):
        assert np.array_equal(a[key], b[key]), key


def test_no_sightings_is_a_no_op():
    """A catalogue graph without sightings: no stage, nothing written but the range rows."""
    import odom_ref as od
    import residuals_ref as rr
    A, Q, dm, g = tp.build("robots-d2")
    dims, table, chains = (dm.d, dm.n, dm.r, dm.n_trans), rr.table(g), od.chains_of(g)
    ctx = capi.Context(*dims, Q.rowptr, Q.col, Q.val, device=-1)
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_sighting_placement()
    assert ctx.sighting_placement_counts()[:3] == (0, 0, 0) and ctx.sighting_placement_order() == []
    X = np.array(A["truth"], dtype=np.float64)
    got = ctx.debug_place_by_sightings_host(X)
    t0 = dm.d * dm.n + dm.r
    assert got["stages"] == 0 and got["placed"] == 0 and got["landmarks_placed"] == 0
    assert np.array_equal(sg.bits(got["X"][:dm.d * dm.n]), sg.bits(X[:dm.d * dm.n])) and np.array_equal(sg.bits(got["X"][t0:]), sg.bits(X[t0:]))


def test_refusals():
    (dims, table, X, chains, _, _), kw, _ = relay(2)
    ctx = capi.Context(*dims, *sg.diagonal_q(*dims), device=-1)

    def code(fn, *a, **k):
        with pytest.raises(capi.CoraError) as e:
            fn(*a, **k)
        return e.value.code
    assert code(ctx.set_sighting_placement) == ERR_NOT_READY                      # no measurement table
    assert code(ctx.debug_place_by_sightings_host, X) == ERR_NOT_READY
    ctx.set_measurements(*table)
    assert code(ctx.set_sighting_placement) == ERR_NOT_READY                      # no chain tables
    ctx.set_odometry_chains(chains)
    assert code(ctx.debug_place_by_sightings_host, X) == ERR_NOT_READY            # no sighting tables
    assert code(ctx.set_sighting_placement, min_sightings=1) == ERR_ARG           # below d
    assert code(ctx.set_sighting_placement, chain_fixed=[0, 0, 0]) == ERR_ARG     # a mask that fixes no chain
    assert ctx.sighting_placement_counts() == (0, 0, 0, 0)
    ctx.set_sighting_placement(min_sightings=2)
    counts = ctx.sighting_placement_counts()
    assert counts[0] == 5
    assert code(ctx.set_sighting_placement, min_sightings=1) == ERR_ARG and ctx.sighting_placement_counts() == counts   # a refused call keeps the tables
    out = (capi.C.c_int64 * 6)()
    Xf = np.asfortranarray(X)
    none = [None] * 8
    assert ctx.L.cora_debug_place_by_sightings_host(ctx.h, capi._d(Xf), ctx.N - 1, out, *none) == ERR_SHAPE
    assert ctx.L.cora_debug_place_by_sightings_host(ctx.h, None, ctx.N, out, *none) == ERR_ARG
    assert ctx.L.cora_debug_place_by_sightings_host(ctx.h, capi._d(Xf), ctx.N, None, *none) == ERR_ARG
    assert ctx.L.cora_debug_place_by_sightings_host(ctx.h, capi._d(Xf), ctx.N, out, *none) == 0 and out[0] == 2 and out[2] == 8 and out[5] == 5
    assert code(ctx.place_by_sightings, X) == ERR_HIP                             # a device form on a plan-only handle
    # new chains and a new measurement table drop the sighting tables
    ctx.set_odometry_chains(chains)
    assert ctx.sighting_placement_counts() == (0, 0, 0, 0) and code(ctx.debug_place_by_sightings_host, X) == ERR_NOT_READY
    ctx.set_sighting_placement()
    ed = table[1].copy()
    ed[table[0][:, 1] < 0, 2 * 2 + 2 + 1] = 1e308   # tau of every sighting: sum tau overflows
    ctx.set_measurements(table[0], ed, table[2], table[3])
    assert ctx.sighting_placement_counts() == (0, 0, 0, 0)
    ctx.set_odometry_chains(chains)
    ctx.set_sighting_placement()
    assert code(ctx.debug_place_by_sightings_host, X) == ERR_NAN


def test_partitioned_handles_are_refused():
    A, Q, dm, g = tp.build("robots-d2")
    p = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=2)
    for fn, args in ((p.set_sighting_placement, ()), (p.debug_place_by_sightings_host, (np.zeros((p.N, 2)),))):
        with pytest.raises(capi.CoraError) as e:
            fn(*args)
        assert e.value.code == ERR_ARG and "partitioned" in str(e.value)
