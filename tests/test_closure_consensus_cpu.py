"""The outlier-robust placement from closures without a GPU: cora_debug_place_by_closures_robust_host (the functions the
kernels call, in the device's bracket order, on plan-only handles) against the longdouble / mpmath reference of
tests/closure_consensus_ref.py -- votes, election, inlier flags and counts exactly (no residual of any case lies within a
factor of 2 of the threshold), statuses, the transforms and every written row within closure_ref's bound over the inliers --
on lists on either side of every edge of the vote's tile loop (1, 2, 255, 256, 257, 513 entries: one, two and three chunks),
a tie between two consistent groups, an outlier as the list's first entry, an entry without a rotation weight, a list without
any consensus, a star of 40 lists in one stage, a relay of three dependent stages, a clean list against the plain mirror, and
the error paths.  The device forms against the mirror, bit for bit: tests/test_gpu_closure_consensus.py.

Inputs: positions within about +-10 m (closure_ref.scene), inlier noise 1e-3 rad and 1e-3 m, kappa = tau = 1e4, 30 - 40 %
outliers (a rotation of at least 0.5 rad and 2 - 8 m per axis).  A true closure under a true hypothesis then has a residual of
the order kappa (2e-3)^2 d + tau (2e-3 + 2e-3 x 20 m)^2 < 100, a wrong one at least tau 2^2 d = 8e4: barc2 = 200, and every case
asserts that the reference finds no residual between 100 and 400."""
import numpy as np
import pytest

import closure_consensus_ref as cc
import closure_ref as cl
import test_closure_cpu as tc
from cora_amd import capi

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
BARC2 = 200.0
NOISE, WEIGHT = 1e-3, 1e4
LIST_LENS = (1, 2, 255, 256, 257, 513)

_BUILT = {}


def _scene(d, lens, pairs, seed, wrong=(), kappa=None, **kw):
    """closure_ref.scene with the noise and weights above, the closures in the order of `pairs` (no shuffle: the order
    of a list is the test's), then the closures `wrong` (indices into pairs) spoiled.  Returns the scene and, per closure, 1
    where it is as measured."""
    k = len(pairs)
    kappa = [WEIGHT] * k if kappa is None else kappa
    dims, table, X, chains, truth = cl.scene(d, lens, pairs, seed=seed, noise=NOISE, kappa=kappa, tau=[WEIGHT] * k, **kw)
    first = len(table[0]) - k
    cc.spoil(d, table[1], [first + i for i in wrong], np.random.default_rng(7000 + seed))
    good = np.ones(k, dtype=np.uint8)
    good[list(wrong)] = 0
    return (dims, table, X, chains, truth), first, good


def lengths(d):
    """Chain 0 (30 poses, fixed); chains 1 .. 6 (40 poses each) have 1, 2, 255, 256, 257 and 513 closures against it: six
    lists of one stage.  The one closure of chain 1 is right; the two of chain 2 disagree (the second is wrong); of the others
    35 % are wrong, in the list of 257 the FIRST entry among them.  min_consensus = 2: chains 1 and 2 have status 5."""
    rng = np.random.default_rng(500 + d)
    pairs, wrong = [], []
    for c, k in enumerate(LIST_LENS):
        at = len(pairs)
        pairs += tc._pairs(rng, 0, 30, 30 + 40 * c, 40, k)
        if k == 2:
            wrong.append(at + 1)
        elif k > 2:
            bad = rng.choice(np.arange(1, k), int(0.35 * k), replace=False)
            if k == 257:
                bad[0] = 0
            wrong += [at + int(b) for b in sorted(set(int(b) for b in bad))]
    sc, first, good = _scene(d, [30] + [40] * 6, pairs, 100 + d, wrong)
    return sc, {}, dict(min_consensus=2), good, [4, 5, 5, 0, 0, 0, 0]


def lengths_min1(d):
    """The same with min_consensus = 1: the single closure places chain 1, and of the two disagreeing closures of chain 2 both
    have vote 1, entry 0 is elected and places it; the wrong one is flagged 0."""
    sc, kw, _, good, _ = lengths(d)
    return sc, kw, dict(min_consensus=1), good, [4, 0, 0, 0, 0, 0, 0]


def tie(d):
    """12 exact closures of chain 1 against chain 0: the even entries say where the chain is, the odd entries agree with one
    another on a second place (the chain's poses moved by one rigid motion before the closure was taken).  Two disjoint groups
    of 6: both have vote 6, the group with entry 0 wins, the other group is flagged 0."""
    rng = np.random.default_rng(520 + d)
    pairs = tc._pairs(rng, 0, 20, 20, 20, 12)
    (dims, table, X, chains, truth), first, good = _scene(d, [20, 20], pairs, 120 + d)
    _, n, r, _ = dims
    t0 = d * n + r
    Rc, tcx = truth[1]
    Gb, sb = cc._big_rot(d, rng), rng.uniform(2, 8, d)
    ed = table[1]
    for k, (i, j) in enumerate(pairs):
        world = {}
        for p in (i, j):
            Rp, Tp = (Rc, tcx) if p >= 20 else (np.eye(d), np.zeros(d))
            Rw, Tw = Rp @ X[d * p:d * p + d].T, Rp @ X[t0 + p] + Tp
            if p >= 20 and k % 2:
                Rw, Tw = Gb @ Rw, Gb @ Tw + sb
            world[p] = (Rw, Tw)
        (Ri, Ti), (Rj, Tj) = world[i], world[j]
        ed[first + k, :d * d] = (Ri.T @ Rj).reshape(-1)
        ed[first + k, d * d:d * d + d] = Ri.T @ (Tj - Ti)
        good[k] = 0 if k % 2 else 1
    return (dims, table, X, chains, truth), {}, dict(min_consensus=2), good, [4, 0]


def no_rotation_weight(d):
    """8 closures, entries 5 and 6 wrong, entry 2 with kappa = 0 and a right translation: an invalid hypothesis (vote 0) that
    still votes for the others: consensus 6, and it is an inlier."""
    rng = np.random.default_rng(530 + d)
    pairs = tc._pairs(rng, 0, 20, 20, 20, 8)
    kappa = [WEIGHT] * 8
    kappa[2] = 0.0
    sc, first, good = _scene(d, [20, 20], pairs, 130 + d, [5, 6], kappa=kappa)
    return sc, {}, dict(min_consensus=2), good, [4, 0]


def inconsistent(d):
    """5 closures, each wrong in its own way: every vote is 1 (an entry agrees with itself), consensus 1, status 5.  What the
    elected entry 0 takes for its inliers is itself alone."""
    rng = np.random.default_rng(540 + d)
    pairs = tc._pairs(rng, 0, 20, 20, 20, 5)
    sc, first, good = _scene(d, [20, 20], pairs, 140 + d, [0, 1, 2, 3, 4])
    good[0] = 1   # (the elected entry's own flag)
    return sc, {}, dict(min_consensus=2), good, [4, 5]


def star(d):
    """40 chains of 6 poses with 5 closures each against chain 0, two of them wrong in every list: 40 lists in one stage."""
    rng = np.random.default_rng(550 + d)
    pairs, wrong = [], []
    for c in range(40):
        bad = rng.choice(5, 2, replace=False)
        wrong += [len(pairs) + int(b) for b in bad]
        pairs += tc._pairs(rng, 0, 20, 20 + 6 * c, 6, 5)
    sc, first, good = _scene(d, [20] + [6] * 40, pairs, 150 + d, wrong)
    return sc, {}, dict(min_consensus=2), good, [4] + [0] * 40


def relay(d):
    """A path 0 - 1 - 2 - 3 with 7 closures per link, two of them wrong: three stages, and the references of stage 2 are the
    chain stage 1 placed robustly."""
    rng = np.random.default_rng(560 + d)
    pairs = tc._pairs(rng, 0, 25, 25, 25, 7) + tc._pairs(rng, 25, 25, 50, 25, 7) + tc._pairs(rng, 50, 25, 75, 25, 7)
    sc, first, good = _scene(d, [25] * 4, pairs, 160 + d, [1, 4, 7, 12, 15, 20])
    return sc, {}, dict(min_consensus=2), good, [4, 0, 0, 0]


def clean(d):
    """10 closures, none wrong: I is the whole list."""
    rng = np.random.default_rng(570 + d)
    sc, first, good = _scene(d, [20, 20], tc._pairs(rng, 0, 20, 20, 20, 10), 170 + d)
    return sc, {}, dict(min_consensus=2), good, [4, 0]


BUILDERS = dict(lengths=lengths, lengths_min1=lengths_min1, tie=tie, no_rotation_weight=no_rotation_weight, inconsistent=inconsistent,
                star=star, relay=relay, clean=clean)
CASES = [(name, d) for name in BUILDERS for d in (2, 3)]


def case(name, d, device=-1):
    """(ctx, dims, table, X, chains, kw, vote, good, expect) of a case, tables installed."""
    key = (name, d, device)
    if key not in _BUILT:
        (dims, table, X, chains, _), kw, vote, good, expect = BUILDERS[name](d)
        ctx = capi.Context(*dims, *cl.diagonal_q(*dims), device=device)
        ctx.set_measurements(*table)
        ctx.set_odometry_chains(chains)
        ctx.set_closure_placement(**kw)
        _BUILT[key] = (ctx, dims, table, X, chains, kw, vote, good, expect)
    return _BUILT[key]


def reference_of(name, d):
    """Computed once and shared (tests/test_gpu_closure_consensus.py reads the same)."""
    key = ("ref", name, d)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, vote, _, _ = case(name, d)
        _BUILT[key] = cc.reference(*dims, table, chains, X, BARC2, **vote, **kw)
    return _BUILT[key]


def mirror_of(name, d):
    key = ("mirror", name, d)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, vote, _, _ = case(name, d)
        got = ctx.debug_place_by_closures_robust_host(X, BARC2, **vote)
        got["X_in"] = X
        _BUILT[key] = got
    return _BUILT[key]


@pytest.mark.parametrize("name,d", CASES)
def test_mirror_on_the_cases(name, d):
    ctx, dims, table, X, chains, kw, vote, good, expect = case(name, d)
    ref, got = reference_of(name, d), mirror_of(name, d)
    tc.check_structure(ctx, ref)
    worst = cc.check(got, *dims, table, ref)
    print("%s d=%d: worst error / (a + b) %.4f; statuses %s consensus %s of %s" % (name, d, worst, got["status"], got["consensus"], got["list_len"]))
    assert list(got["status"]) == expect, got["status"]
    # the flags are the construction's: 1 where the closure is as measured, 0 where it was spoiled, 2 on the chains' own edges
    k = len(good)
    assert np.array_equal(got["inlier"][-k:], good) and np.all(got["inlier"][:-k] == 2)
    assert got["excluded"] == int(np.sum(good == 0))
    for c in range(1, len(chains)):
        assert got["cost_final"][c] <= got["cost_start"][c]
        if got["status"][c] == 0:
            assert got["chosen"][c] == 1
    if name.startswith("lengths"):
        assert list(got["list_len"]) == [0] + list(LIST_LENS) and ctx.closure_placement_counts()[2] == 1 + 1 + 1 + 1 + 2 + 3
        assert list(got["consensus"][:3]) == [0, 1, 1] and list(got["consensus"][3:]) == [k - int(0.35 * k) for k in LIST_LENS[2:]]
        assert ref["elected"][2] == 0 and ref["elected"][5] > 0 and got["inlier"][-k:][LIST_LENS[0] + LIST_LENS[1] + 255 + 256] == 0   # the list of 257 begins with an outlier
        if name == "lengths":   # without consensus: the caller's bits (closure_ref.check has compared them)
            assert got["no_consensus"] == 2 and np.all(got["chosen"][1:3] == 0)
    if name == "tie":
        assert got["consensus"][1] == 6 and ref["elected"][1] == 0
    if name == "no_rotation_weight":
        assert got["consensus"][1] == 6 and got["inlier"][-k:][2] == 1
    if name == "inconsistent":
        assert got["consensus"][1] == 1 and got["no_consensus"] == 1 and got["placed"] == 0
    if name == "star":
        assert np.all(got["consensus"][1:] == 3) and got["stages"] == 1 and got["placed"] == 40
    if name == "relay":
        assert got["stages"] == 3 and list(got["consensus"]) == [0, 5, 5, 5]


@pytest.mark.parametrize("d", [2, 3])
def test_a_clean_list_agrees_with_the_plain_mirror(d):
    """I is the whole list, so both calls form the same sums term by term: the same bits, transforms and rows (each is within
    the bound of the one reference: test_mirror_on_the_cases, tests/test_closure_cpu.py's check below)."""
    ctx, dims, table, X, chains, kw, vote, good, _ = case("clean", d)
    ref, got = reference_of("clean", d), mirror_of("clean", d)
    plain = ctx.debug_place_by_closures_host(X)
    assert got["consensus"][1] == got["list_len"][1] == 10 and got["excluded"] == 0
    plain["X_in"] = X
    cl.check(plain, *dims, table, ref)   # the plain mirror within the same reference's bound
    for key in ("X", "transforms", "cost_start", "cost_final"):
        assert np.array_equal(cl.bits(got[key]), cl.bits(plain[key])), key


@pytest.mark.parametrize("name,d", [("lengths", 2), ("relay", 3), ("star", 3)])
def test_two_calls_give_the_same_bits(name, d):
    ctx, dims, table, X, chains, kw, vote, _, _ = case(name, d)
    a, b = mirror_of(name, d), ctx.debug_place_by_closures_robust_host(X, BARC2, **vote)
    for key in ("X", "cost_start", "cost_final", "transforms"):
        assert np.array_equal(cl.bits(a[key]), cl.bits(b[key])), key
    for key in ("status", "chosen", "consensus", "list_len", "inlier"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("d", [2, 3])
def test_the_plain_call_keeps_its_bits_and_the_tables_stay(d):
    """A robust call between two plain calls on one handle changes neither the tables nor the plain call's result."""
    ctx, dims, table, X, chains, kw, vote, _, _ = case("relay", d)
    before, counts = ctx.debug_place_by_closures_host(X), ctx.closure_placement_counts()
    ctx.debug_place_by_closures_robust_host(X, BARC2, **vote)
    after = ctx.debug_place_by_closures_host(X)
    assert ctx.closure_placement_counts() == counts
    for key in ("X", "cost_start", "cost_final", "transforms"):
        assert np.array_equal(cl.bits(before[key]), cl.bits(after[key])), key


def robust_refusals(ctx_of, call, raw, has_ldx=True):
    """The error paths of one form of the robust call (shared with tests/test_gpu_closure_consensus.py): ctx_of() a fresh
    handle, call(ctx, X, barc2, min_consensus), raw(ctx): the C function and how it takes the vector (and its leading
    dimension, has_ldx)."""
    (dims, table, X, chains, _), kw, _, _, _ = relay(2)
    ctx = ctx_of(dims)

    def code(*a):
        with pytest.raises(capi.CoraError) as e:
            call(ctx, *a)
        return e.value.code
    assert code(X, BARC2, 2) == ERR_NOT_READY          # no measurement table
    ctx.set_measurements(*table)
    assert code(X, BARC2, 2) == ERR_NOT_READY          # no chain tables
    ctx.set_odometry_chains(chains)
    assert code(X, BARC2, 2) == ERR_NOT_READY          # no closure tables
    ctx.set_closure_placement()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert code(X, bad, 2) == ERR_ARG
    assert code(X, BARC2, 0) == ERR_ARG
    fn, lead = raw(ctx)
    out = (capi.C.c_int64 * 7)()
    Xf = np.asfortranarray(X)
    none = [None] * 8
    bar = capi.C.c_double(BARC2)
    if has_ldx:
        assert fn(ctx.h, *lead(Xf, ctx.N - 1), bar, 2, out, *none) == ERR_SHAPE
    assert fn(ctx.h, *lead(None, ctx.N), bar, 2, out, *none) == ERR_ARG
    assert fn(ctx.h, *lead(Xf, ctx.N), bar, 2, None, *none) == ERR_ARG
    assert fn(ctx.h, *lead(Xf, ctx.N), bar, 2, out, *none) == 0 and list(out) == [3, 0, 0, 3, 0, 0, 6]   # every output may be NULL
    return ctx


def nan_case(d=2):
    """closure_ref's exactly representable scene (every residual 0 exactly, so every closure is an inlier of every hypothesis)
    with tau = 1e308: the sum of tau over I overflows."""
    (dims, table, X, chains, _), _, _ = tc.in_place(d)
    ed = table[1].copy()
    ed[len(chains[0]) + len(chains[1]):, d * d + d + 1] = 1e308
    return dims, (table[0], ed, table[2], table[3]), X, chains


def test_refusals():
    ctx = robust_refusals(lambda dims: capi.Context(*dims, *cl.diagonal_q(*dims), device=-1),
                          lambda ctx, X, b, m: ctx.debug_place_by_closures_robust_host(X, b, m),
                          lambda ctx: (ctx.L.cora_debug_place_by_closures_robust_host, lambda X, ldx: (None if X is None else capi._d(X), ldx)))
    (dims, table, X, chains, _), _, _, _, _ = relay(2)
    with pytest.raises(capi.CoraError) as e:
        ctx.place_by_closures_robust(X, BARC2)       # a device form on a plan-only handle
    assert e.value.code == ERR_HIP
    dims, table, X, chains = nan_case()
    ctx = capi.Context(*dims, *cl.diagonal_q(*dims), device=-1)
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_closure_placement()
    with pytest.raises(capi.CoraError) as e:
        ctx.debug_place_by_closures_robust_host(X, BARC2)
    assert e.value.code == ERR_NAN
