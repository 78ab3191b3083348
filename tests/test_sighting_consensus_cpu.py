"""The outlier-robust placement from sightings without a GPU: cora_debug_place_by_sightings_robust_host (the functions the
kernels call, in the device's bracket order, on plan-only handles) against the longdouble / mpmath reference of
tests/sighting_consensus_ref.py -- votes, elections, inlier flags, consensus, list lengths and the four counts exactly (the
reference's band is empty on every case: no residual near the threshold, no hypothesis near the refusal rule), statuses,
transforms and every written row within sighting_ref's bound over the inliers -- on lists that sit on every boundary of the
vote's tiles and the reduction's shape, with the origin an outlier, ties, invalid samples, lists without consensus, a zero
weight, many lists side by side and alternating stages; a clean graph has the plain mirror's bits.  The device forms against
the mirror, bit for bit: tests/test_gpu_sighting_consensus.py."""
import numpy as np
import pytest

import sighting_consensus_ref as sc
import sighting_ref as sg
from cora_amd import capi

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
LM_LENS = (1, 2, 255, 256, 257, 513)

_BUILT = {}


def _see(rng, first, length, lms, k):
    """k sightings from random positions of the chain [first, first + length) of the landmarks lms in turn."""
    return [(first + int(rng.integers(length)), lms[j % len(lms)]) for j in range(k)]


def _shuffled(rng, sights):
    return [sights[i] for i in rng.permutation(len(sights))]


def _lists(scene, kw):
    """The stages' lists (sighting_ref.structure) of a scene."""
    dims, table, X, chains = scene[:4]
    return sg.structure(*dims, table, chains, kw.get("chain_fixed"), kw.get("landmark_fixed"), kw.get("min_sightings"))["stages"]


def lengths(d):
    """Chain 0 (30 poses, fixed) sights landmark j with LM_LENS[j] sightings: the L-stage's lists of 1, 2, 255, 256, 257, 513.
    Chains 1 .. 6 (40 poses each, each in a frame of its own) sight landmarks 2 .. 5 with d, d + 1, 255, 256, 257 and 513
    sightings: six lists of ONE C-stage, min_sightings = d.  Exact sightings, weights in [0.5, 2], the table shuffled.  In
    every list of 255 and more, 30 % of the sightings have a wrong t; among them the FIRST entry of the landmark list of 256
    and of the chain list of 257: their origin is an outlier."""
    rng = np.random.default_rng(340 + d)
    sights = []
    for j, k in enumerate(LM_LENS):
        sights += _see(rng, 0, 30, [j], k)
    for c, k in enumerate((d, d + 1) + LM_LENS[2:]):
        sights += _see(rng, 30 + 40 * c, 40, [2, 3, 4, 5], k)
    sights = _shuffled(rng, sights)
    tau = rng.uniform(0.5, 2.0, len(sights))
    scene = sg.scene(d, [30] + [40] * 6, sights, seed=d, n_lm=6, tau=tau)
    kw = dict(min_sightings=d)
    wrong = set()
    for st in _lists(scene, kw)[:2]:
        for item, es in st["lists"]:
            if len(es) >= 255:
                wrong.update(int(e) for e in rng.choice(es, size=(3 * len(es)) // 10, replace=False))
            if len(es) in (256, 257):
                wrong.add(int(es[0]))
    sc.spoil(d, scene[1], sorted(wrong), rng, relabel=False)
    return scene, kw, dict(min_chain_consensus=d), wrong


def tie(d):
    """Landmarks 0 .. 3 fixed at the truth, 4 .. 7 fixed at the truth moved by one rigid motion M: chain 1's 12 sightings of
    0 .. 3 agree with its true motion g, its 12 sightings of 4 .. 7 with M g -- two groups of equal vote in one chain list.
    Landmark 8 (free) has 6 true sightings by chain 0 and 6 sightings of landmark 9 credited to it: two groups of equal vote
    in one landmark list.  The lowest entry among equal votes wins.  Chain 1's list is in table order."""
    rng = np.random.default_rng(350 + d)
    # entry h of chain 1's list: group h % 2, so that the samples (h, h + 24 / d, ..) are of one group; the landmark moves on
    # along a sample (at d = 2 not for every h: those samples repeat a landmark and are refused)
    sights = [(30 + int(rng.integers(30)), 4 * (h % 2) + (h // 2 + h // 8) % 4) for h in range(24)]
    sights += _shuffled(rng, _see(rng, 0, 30, [8], 6) + _see(rng, 0, 30, [9], 6))
    scene = sg.scene(d, [30, 30], sights, seed=50 + d, n_lm=10, known=tuple(range(8)))
    (dd, n, r, nt), table, X = scene[0], scene[1], scene[2]
    t0 = d * n + r
    M, s = sc.sg.pl._rot(d, rng, 1.0), rng.uniform(3, 6, d)
    X[t0 + n + 4:t0 + n + 8] = X[t0 + n + 4:t0 + n + 8] @ M.T + s
    er = table[0]
    er[er[:, 3] == t0 + n + 9, 3] = t0 + n + 8
    fixed = [1] * 8 + [0, 0]
    return scene, dict(landmark_fixed=fixed, min_sightings=2 * d), {}, set()


def invalid_samples(d):
    """One chain list of 12 entries in table order whose landmark pattern gives the samples of some entries (entry 0 among
    them) a repeated landmark, and at d = 3 three landmarks on one line (9, 10, 11): those hypotheses are refused by the
    plain rule, have vote 0 and set no flag.  All landmarks fixed at the truth; every entry is an inlier of the elected."""
    rng = np.random.default_rng(360 + d)
    lms = [0, 1, 2, 3, 4, 5, 0, 1, 2, 6, 7, 8] if d == 2 else [0, 1, 2, 9, 0, 4, 5, 10, 6, 7, 8, 11]
    lm = rng.uniform(-10, 10, (12, d))
    u = rng.normal(0, 1, d)
    lm[9:12] = lm[9] + np.outer([0.0, 3.0, 7.0], u / np.linalg.norm(u))
    sights = [(20 + int(rng.integers(20)), l) for l in lms]
    scene = sg.scene(d, [20, 20], sights, seed=60 + d, n_lm=12, lm_world=lm, known=tuple(range(12)))
    return scene, dict(landmark_fixed=[1] * 12, min_sightings=d), {}, set()


def no_consensus(d):
    """Chain 1's sightings of the placed landmarks 0 .. 3 all have a wrong t: no d + 1 of them agree (status 5, its rows not
    touched).  Landmark 4 has three sightings by chain 0, all wrong: below min_landmark_consensus = 2 (status 5, its row not
    touched).  The later stages still run: chain 2 is placed from 0 .. 3; landmark 5, which only chain 1 sights, is set in a
    second L-stage from chain 1's rows as they stand; landmark 6, which only chain 2 sights, from the moved chain 2."""
    rng = np.random.default_rng(370 + d)
    tagged = [(s, 0) for s in _see(rng, 0, 30, [0, 1, 2, 3], 40)] + [(s, 1) for s in _see(rng, 30, 20, [0, 1, 2, 3], 4 * d + 2)]
    tagged += [(s, 1) for s in _see(rng, 0, 30, [4], 3)] + [(s, 0) for s in _see(rng, 50, 20, [0, 1, 2, 3], 30)]
    tagged += [(s, 0) for s in _see(rng, 30, 20, [5], 4) + _see(rng, 50, 20, [6], 4)]
    tagged = _shuffled(rng, tagged)
    scene = sg.scene(d, [30, 20, 20], [s for s, _ in tagged], seed=70 + d, n_lm=7)
    n_odo = sum(len(ch) for ch in scene[3])
    wrong = {n_odo + k for k, (_, w) in enumerate(tagged) if w}
    sc.spoil(d, scene[1], sorted(wrong), rng, relabel=False)
    return scene, {}, dict(min_landmark_consensus=2), wrong


def zero_tau(d):
    """relay's shape with tau = 0 on one sighting of every tenth, a wrong id on one of every five of the others."""
    rng = np.random.default_rng(380 + d)
    sights = _shuffled(rng, _see(rng, 0, 30, [0, 1, 2, 3], 60) + _see(rng, 30, 30, [0, 1, 2, 3], 60))
    tau = np.where(np.arange(len(sights)) % 10 == 3, 0.0, rng.uniform(0.5, 2.0, len(sights)))
    scene = sg.scene(d, [30, 30], sights, seed=80 + d, n_lm=4, tau=tau)
    n_odo = sum(len(ch) for ch in scene[3])
    wrong = {n_odo + k for k in range(len(sights)) if k % 5 == 1}
    sc.spoil(d, scene[1], sorted(wrong), rng)
    return scene, {}, {}, wrong


def star(d):
    """40 landmarks sighted by chain 0 (40 lists in one L-stage) and by 6 more chains (6 lists in one C-stage; 40 in the
    REFIT); one sighting in five credited to a wrong landmark."""
    rng = np.random.default_rng(390 + d)
    sights = _see(rng, 0, 30, list(range(40)), 400)
    for c in range(6):
        sights += _see(rng, 30 + 15 * c, 15, list(rng.permutation(40)), 60)
    sights = _shuffled(rng, sights)
    scene = sg.scene(d, [30] + [15] * 6, sights, seed=90 + d, n_lm=40)
    n_odo = sum(len(ch) for ch in scene[3])
    wrong = {n_odo + k for k in range(len(sights)) if k % 5 == 2}
    sc.spoil(d, scene[1], sorted(wrong), rng)
    return scene, {}, {}, wrong


def relay(d, spoiled=True):
    """Chain 1 sights landmarks 0 .. 3 (which chain 0 sights) and 4 .. 7 (which only chains 1 and 2 sight); chain 2 sights
    4 .. 7 only: L, C, L, C, REFIT.  One sighting in five is credited to a wrong landmark of its own group of four; 18 range
    measurements have their rows recomputed."""
    rng = np.random.default_rng(400 + d)
    sights = _see(rng, 0, 30, [0, 1, 2, 3], 60) + _see(rng, 30, 30, list(range(8)), 120) + _see(rng, 60, 30, [4, 5, 6, 7], 60)
    sights = _shuffled(rng, sights)
    ranges = [(int(a), 30 + int(b)) if m % 2 else (60 + int(b), int(a)) for m, (a, b) in enumerate(rng.integers(30, size=(12, 2)))]
    ranges += [(int(a), 90 + int(l)) for a, l in zip(rng.integers(90, size=6), rng.integers(8, size=6))]
    scene = sg.scene(d, [30, 30, 30], sights, seed=100 + d, n_lm=8, ranges=ranges)
    wrong = set()
    if spoiled:
        (dd, n, r, nt), table = scene[0], scene[1]
        n_odo, lm0 = sum(len(ch) for ch in scene[3]), d * n + r + n
        for k in range(len(sights)):
            if k % 5 == 4:
                e = n_odo + k
                group = (int(table[0][e, 3]) - lm0) // 4
                sc.spoil(d, table, [e], rng, rows=lm0 + 4 * group + np.arange(4))
                wrong.add(e)
    return scene, {}, {}, wrong


BUILDERS = dict(lengths=lengths, tie=tie, invalid_samples=invalid_samples, no_consensus=no_consensus, zero_tau=zero_tau, star=star,
                relay=relay, clean=lambda d: relay(d, spoiled=False))
CASES = [(name, d) for name in BUILDERS for d in (2, 3)]
CLEAN_BARC2 = 1e-8   # (a clean graph has one residual class only: nothing to take the middle of)


def case(name, d, device=-1):
    """(ctx, dims, table, X, chains, kw, robust kw, wrong edges) of a case, tables installed."""
    key = (name, d, device)
    if key not in _BUILT:
        (dims, table, X, chains, truth, lm_true), kw, rkw, wrong = BUILDERS[name](d)
        ctx = capi.Context(*dims, *sg.diagonal_q(*dims), device=device)
        ctx.set_measurements(*table)
        ctx.set_odometry_chains(chains)
        ctx.set_sighting_placement(**kw)
        _BUILT[key] = (ctx, dims, table, X, chains, kw, rkw, wrong)
    return _BUILT[key]


def reference_of(name, d):
    """(barc2, reference), computed once and shared (tests/test_gpu_sighting_consensus.py reads the same).  barc2: the
    geometric middle of the two residual classes the reference finds at a provisional threshold; the reference at that barc2
    must find the same two classes."""
    key = ("ref", name, d)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, rkw, _ = case(name, d)
        if name in ("clean", "invalid_samples"):
            barc2 = CLEAN_BARC2
            ref = sc.reference(*dims, table, chains, X, barc2, **rkw, **kw)
            assert ref["classes"][1] == np.inf and ref["classes"][0] < 1e-6 * barc2
        else:
            first = sc.reference(*dims, table, chains, X, 1e-10, **rkw, **kw)
            barc2 = sc.middle_barc2(first["classes"])
            ref = sc.reference(*dims, table, chains, X, barc2, **rkw, **kw)
            assert ref["classes"] == first["classes"], (ref["classes"], first["classes"])
        _BUILT[key] = (barc2, ref)
    return _BUILT[key]


def mirror_of(name, d):
    key = ("mirror", name, d)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, rkw, _ = case(name, d)
        got = ctx.debug_place_by_sightings_robust_host(X, reference_of(name, d)[0], **rkw)
        got["X_in"] = X
        _BUILT[key] = got
    return _BUILT[key]


REALS = ("X", "cost_start", "cost_final", "transforms", "landmark_cost")
INTS = ("status", "chosen", "landmark_status", "degenerate") + sc.INTEGERS
PLAIN_COUNTS = ("placed", "not_placed", "landmarks_placed", "landmarks_not_placed", "n_degenerate", "stages")


def same_bits(a, b, robust=True):
    for key in REALS:
        assert np.array_equal(sg.bits(a[key]), sg.bits(b[key])), key
    for key in INTS[:4] + (sc.INTEGERS if robust else ()):
        assert np.array_equal(a[key], b[key]), key
    for key in PLAIN_COUNTS + (sc.COUNTS if robust else ()):
        assert a[key] == b[key], key


@pytest.mark.parametrize("name,d", CASES)
def test_band_is_empty(name, d):
    """The condition on the inputs, from the reference alone."""
    barc2, ref = reference_of(name, d)
    print("%s d=%d: barc2 %.3e between the residual classes <= %.3e and >= %.3e" % (name, d, barc2, *ref["classes"]))
    assert ref["band"] == [], ref["band"][:8]


@pytest.mark.parametrize("name,d", CASES)
def test_mirror_against_the_reference(name, d):
    ctx, dims, table, X, chains, kw, rkw, wrong = case(name, d)
    (barc2, ref), got = reference_of(name, d), mirror_of(name, d)
    counts = ctx.sighting_placement_counts()
    assert counts == ref["struct"]["counts"]
    worst = sc.check(got, *dims, table, ref)
    print("%s d=%d: worst error / (a + b) %.4f; statuses %s landmarks %s; consensus %s of %s; landmarks %s of %s; counts %s" %
          (name, d, worst, got["status"], got["landmark_status"], got["chain_consensus"], got["chain_list_len"], got["landmark_consensus"],
           got["landmark_list_len"], [got[k] for k in sc.COUNTS]))
    for c in range(len(chains)):
        assert got["cost_final"][c] <= got["cost_start"][c]
    # a wrong sighting is outside I wherever it is in a list of a chain or landmark that found its consensus
    er = table[0]
    t0, n = dims[0] * dims[1] + dims[2], dims[1]
    for e in sorted(wrong):
        lmk = int(er[e, 3]) - t0 - n
        if got["inlier_landmark"][e] != 2 and got["landmark_status"][lmk] == 0 and name != "no_consensus":
            assert got["inlier_landmark"][e] == 0, e
    same_bits(got, ctx.debug_place_by_sightings_robust_host(X, barc2, **rkw))           # two calls, the same bits
    kinds = [k for k, _ in ref["struct"]["order"]]
    if name == "lengths":
        assert sorted(got["chain_list_len"][1:]) == sorted((d, d + 1) + LM_LENS[2:]) and list(got["status"]) == [4, 0, 0, 0, 0, 0, 0]
        assert np.all(got["landmark_status"] == 0) and got["chain_excluded"] > 300 and got["landmark_excluded"] > 600
        lists = ref["struct"]["stages"]
        assert sorted(len(es) for _, es in lists[0]["lists"]) == list(LM_LENS)
        for st in lists[:2]:   # the origin of the list of 256 (landmarks) and of 257 (chains) is an outlier
            es = [es for _, es in st["lists"] if len(es) == (256 if st["kind"] == "L" else 257)][0]
            assert es[0] in wrong and (got["inlier_landmark"] if st["kind"] == "L" else got["inlier_chain"])[es[0]] == 0
    if name == "tie":
        assert got["chain_consensus"][1] == 12 and got["chain_list_len"][1] == 24 and got["status"][1] == 0
        assert got["landmark_consensus"][8] == 6 and got["landmark_list_len"][8] == 12
        for key, votes in ref["votes"].items():
            h = ref["elected"][key]
            assert np.sum(votes == votes[h]) >= 2 and h == int(np.nonzero(votes == votes[h])[0][0])   # a tie, the lowest wins
    if name == "invalid_samples":
        (key, votes), = ref["votes"].items()
        bad = (0, 1, 2, 6, 7, 8) if d == 2 else (0, 4, 8, 3, 7, 11)
        assert all(votes[h] == 0 for h in bad) and all(votes[h] == 12 for h in range(12) if h not in bad)
        assert ref["elected"][key] == (3 if d == 2 else 1) and got["chain_consensus"][1] == 12 and got["chain_excluded"] == 0
    if name == "no_consensus":
        assert list(got["status"]) == [4, 5, 0] and got["chains_no_consensus"] == 1 and got["not_placed"] == 0
        assert list(got["landmark_status"]) == [0, 0, 0, 0, 5, 0, 0] and got["landmarks_no_consensus"] == 1
        assert kinds == ["L", "C", "L", "REFIT"] and got["chosen"][1] == 0 and got["chain_consensus"][1] <= d
        for rot, trn in ref["struct"]["positions"][1]:
            assert np.array_equal(sg.bits(got["X"][trn]), sg.bits(X[trn])) and np.array_equal(sg.bits(got["X"][rot:rot + d]), sg.bits(X[rot:rot + d]))
        assert np.array_equal(sg.bits(got["X"][t0 + n + 4]), sg.bits(X[t0 + n + 4]))
    if name == "zero_tau":
        assert np.all(got["status"][1:] == 0) and np.all(got["landmark_status"] == 0)
    if name == "star":
        assert len(ref["struct"]["stages"][0]["lists"]) == 40 and len(ref["struct"]["stages"][1]["lists"]) == 6
        assert np.all(got["status"][1:] == 0) and np.all(got["chosen"][1:] == 1) and np.all(got["landmark_status"] == 0)
    if name in ("relay", "clean"):
        assert kinds == ["L", "C", "L", "C", "REFIT"] and np.all(got["status"][1:] == 0) and np.all(got["landmark_status"] == 0)


@pytest.mark.parametrize("d", (2, 3))
def test_a_clean_graph_has_the_plain_bits(d):
    ctx, dims, table, X, chains, kw, rkw, _ = case("clean", d)
    got, plain = mirror_of("clean", d), ctx.debug_place_by_sightings_host(X)
    same_bits(got, plain, robust=False)
    assert np.all(got["inlier_chain"][got["inlier_chain"] != 2] == 1) and np.all(got["inlier_landmark"][got["inlier_landmark"] != 2] == 1)
    assert [got[k] for k in sc.COUNTS] == [0, 0, 0, 0]
    assert np.array_equal(got["chain_consensus"], got["chain_list_len"]) and np.array_equal(got["landmark_consensus"], got["landmark_list_len"])


@pytest.mark.parametrize("name,d", [("lengths", 2), ("star", 3), ("no_consensus", 3)])
def test_the_plain_call_is_not_disturbed(name, d):
    """The plain call before and after a robust call: the same bits; the tables' counts unchanged."""
    ctx, dims, table, X, chains, kw, rkw, _ = case(name, d)
    counts, before = ctx.sighting_placement_counts(), ctx.debug_place_by_sightings_host(X)
    ctx.debug_place_by_sightings_robust_host(X, reference_of(name, d)[0], **rkw)
    same_bits(before, ctx.debug_place_by_sightings_host(X), robust=False)
    assert ctx.sighting_placement_counts() == counts


def test_the_start_world_on_a_stand_in_start():
    """The world of the end-to-end test (tests/test_gpu_sighting_consensus.py) at a stand-in for its odometry start: the band
    is empty, the mirror's flags are the construction's, and the transforms have the bits of the plain mirror on the clean
    graph (the wrong sightings are the last entries of their lists)."""
    import odom_ref as od
    import residuals_ref as rr
    w, n_true, n_wrong = sc.start_world()
    wc, _, _ = sc.start_world(contaminated=False)
    d, n = 2, len(w.names)
    dims, table, chains = (d, n, 0, n + len(w.L)), rr.table(w.g), od.chains_of(w.g)
    X = sc.standin_start(w)
    first = sc.reference(*dims, table, chains, X, 1e-10)
    barc2 = sc.middle_barc2(first["classes"])
    ref = sc.reference(*dims, table, chains, X, barc2)
    print("start world: barc2 %.3e between the residual classes <= %.3e and >= %.3e" % (barc2, *ref["classes"]))
    assert ref["band"] == [] and [k for k, _ in ref["struct"]["order"]] == ["L", "C", "REFIT"]
    ctx = capi.Context(*dims, *sg.diagonal_q(*dims), device=-1)
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_sighting_placement()
    got = ctx.debug_place_by_sightings_robust_host(X, barc2)
    got["X_in"] = X
    sc.check(got, *dims, table, ref)
    ic, il = sc.built_flags(w, table, chains, n_true)
    assert np.array_equal(got["inlier_chain"], ic) and np.array_equal(got["inlier_landmark"], il)
    assert got["chain_excluded"] == 3 * (n_wrong // 4) and got["landmark_excluded"] == n_wrong and list(got["status"]) == [4, 0, 0, 0]
    clean = capi.Context(*dims, *sg.diagonal_q(*dims), device=-1)
    clean.set_measurements(*rr.table(wc.g))
    clean.set_odometry_chains(chains)
    clean.set_sighting_placement()
    same_bits(got, clean.debug_place_by_sightings_host(X), robust=False)


def test_refusals():
    (dims, table, X, chains, _, _), kw, rkw, _ = relay(2)
    ctx = capi.Context(*dims, *sg.diagonal_q(*dims), device=-1)

    def code(fn, *a, **k):
        with pytest.raises(capi.CoraError) as e:
            fn(*a, **k)
        return e.value.code
    assert code(ctx.debug_place_by_sightings_robust_host, X, 1e-8) == ERR_NOT_READY     # no measurement table
    ctx.set_measurements(*table)
    assert code(ctx.debug_place_by_sightings_robust_host, X, 1e-8) == ERR_NOT_READY     # no chain tables
    ctx.set_odometry_chains(chains)
    assert code(ctx.debug_place_by_sightings_robust_host, X, 1e-8) == ERR_NOT_READY     # no sighting tables
    ctx.set_sighting_placement()
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert code(ctx.debug_place_by_sightings_robust_host, X, bad) == ERR_ARG
    assert code(ctx.debug_place_by_sightings_robust_host, X, 1e-8, min_landmark_consensus=0) == ERR_ARG
    out = (capi.C.c_int64 * 10)()
    Xf = np.asfortranarray(X)
    none = [None] * 14
    raw = ctx.L.cora_debug_place_by_sightings_robust_host
    b = capi.C.c_double(1e-8)
    assert raw(ctx.h, capi._d(Xf), ctx.N, b, 0, 1, out, *none) == ERR_ARG             # a chain minimum below 1 (the raw call has no default)
    assert raw(ctx.h, capi._d(Xf), ctx.N, b, 3, 0, out, *none) == ERR_ARG
    assert raw(ctx.h, capi._d(Xf), ctx.N - 1, b, 3, 1, out, *none) == ERR_SHAPE
    assert raw(ctx.h, None, ctx.N, b, 3, 1, out, *none) == ERR_ARG
    assert raw(ctx.h, capi._d(Xf), ctx.N, b, 3, 1, None, *none) == ERR_ARG
    assert raw(ctx.h, capi._d(Xf), ctx.N, b, 3, 1, out, *none) == 0 and out[5] == 5 and out[6] == 0    # every array may be NULL
    assert code(ctx.place_by_sightings_robust, X, 1e-8) == ERR_HIP                       # a device form on a plan-only handle
    ed = table[1].copy()
    ed[table[0][:, 1] < 0, 2 * 2 + 2 + 1] = 1e308   # tau of every sighting: sum tau overflows
    ctx.set_measurements(table[0], ed, table[2], table[3])
    ctx.set_odometry_chains(chains)
    ctx.set_sighting_placement()
    assert code(ctx.debug_place_by_sightings_robust_host, X, 1e-8) == ERR_NAN
    Xn = X.copy()
    Xn[dims[0] * dims[1] + dims[2] + 3] = np.inf     # a pose of chain 0 that sights: an elected hypothesis that is not finite
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_sighting_placement()
    assert code(ctx.debug_place_by_sightings_robust_host, Xn, 1e-8) == ERR_NAN
