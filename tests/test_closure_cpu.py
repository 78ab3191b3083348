"""The placement from inter-chain relative-pose edges without a GPU: cora_debug_place_by_closures_host (the functions the
kernels call, in the device's bracket order, on plan-only handles) against the longdouble / mpmath reference of
tests/closure_ref.py -- the order of the stages, counts, statuses, chosen, the degenerate flags, the transforms and every
written row within the derived bound, never worse on the closure cost, cost_start against the table's own residuals -- on
lists that sit on every boundary of the reduction's shape, a relay of three dependent stages, two chains in one stage with
unused closures between them, masks, skipped edges, a single edge, degenerate geometry on either side of the refusal rule, and
every refusal.  The device forms against the mirror, bit for bit: tests/test_gpu_closure.py."""
import math

import numpy as np
import pytest

import closure_ref as cl
import topologies as tp
from cora_amd import capi

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
LIST_LENS = (1, 255, 256, 257, 64 * 256 + 1)   # the last wraps the fold's lane loop

_BUILT = {}


def _pairs(rng, first_a, len_a, first_b, len_b, k):
    """k closures between random poses of two chains, the direction (which end is a) random."""
    out = []
    for _ in range(k):
        i, j = first_a + int(rng.integers(len_a)), first_b + int(rng.integers(len_b))
        out.append((i, j) if rng.integers(2) else (j, i))
    return out


def lengths(d, noise=0.0, offset=0.0):
    """Chain 0 (30 poses, fixed); chains 1 .. 5 (40 poses each, each in a frame of its own) have 1, 255, 256, 257 and
    64 * 256 + 1 closures against it: five lists of ONE stage.  Directions mixed, weights in [0.5, 2], the table shuffled."""
    rng = np.random.default_rng(340 + d)
    pairs = []
    for c, k in enumerate(LIST_LENS):
        pairs += _pairs(rng, 0, 30, 30 + 40 * c, 40, k)
    kappa, tau = rng.uniform(0.5, 2.0, len(pairs)), rng.uniform(0.5, 2.0, len(pairs))
    return (cl.scene(d, [30] + [40] * 5, pairs, seed=d, noise=noise, kappa=kappa, tau=tau, offset=offset, shuffle=True), {},
            [[1, 2, 3, 4, 5]])


def relay(d):
    """A path 0 - 1 - 2 - 3 with min_closures = 4: 6 closures 0-1, 5 closures 1-2, 5 closures 2-3 and 2 closures 1-3.  Chain 3
    has too few closures against placed chains until chain 2 is placed: three dependent stages, and the 1-3 closures enter
    chain 3's list only.  12 range measurements between the chains have their rows recomputed."""
    rng = np.random.default_rng(360 + d)
    pairs = _pairs(rng, 0, 30, 30, 30, 6) + _pairs(rng, 30, 30, 60, 30, 5) + _pairs(rng, 60, 30, 90, 30, 5) + _pairs(rng, 30, 30, 90, 30, 2)
    ranges = [(int(a), 30 + int(b)) if m % 2 else (60 + int(b), 90 + int(a)) for m, (a, b) in enumerate(rng.integers(30, size=(12, 2)))]
    return cl.scene(d, [30] * 4, pairs, seed=20 + d, noise=0.02, ranges=ranges, shuffle=True), dict(min_closures=4), [[1], [2], [3]]


def same_stage(d):
    """Chains 1 and 2 are taken together (8 and 9 closures against chain 0); the 4 closures between them are unused."""
    rng = np.random.default_rng(370 + d)
    pairs = _pairs(rng, 0, 30, 30, 25, 8) + _pairs(rng, 0, 30, 55, 25, 9) + _pairs(rng, 30, 25, 55, 25, 4)
    return cl.scene(d, [30, 25, 25], pairs, seed=30 + d, noise=0.05, shuffle=True), {}, [[1, 2]]


def statuses(d):
    """min_closures = 3; chains 0 and 4 fixed.  Chain 1 has 5 closures against chain 0 and 3 against chain 4: placed.  Chain 2
    has 2 closures against chain 0 (status 1, both unused); chain 3 has none (status 3).  Skipped: a closure inside chain 1, a
    closure from the first free pose, a prior (a relative-pose edge from the second free pose, the origin).  A sighting of the
    one landmark has no rotation part: it is no relative-pose edge and is not counted."""
    rng = np.random.default_rng(380 + d)
    n = 30 + 30 + 20 + 20 + 20
    pairs = _pairs(rng, 0, 30, 30, 30, 5) + _pairs(rng, 100, 20, 30, 30, 3) + _pairs(rng, 0, 30, 60, 20, 2)
    pairs += [(33, 52), (n, 35), (n + 1, 61)]
    return (cl.scene(d, [30, 30, 20, 20, 20], pairs, seed=40 + d, n_free=2, n_lm=1, noise=0.02, sights=[(7, 0)],
                     moved=[False, True, True, True, False], shuffle=True),
            dict(chain_fixed=[1, 0, 0, 0, 1], min_closures=3), [[1]])


def single_edge(d):
    """One closure, min_closures = 1: the chain lands exactly where the edge says."""
    return cl.scene(d, [12, 15], [(4, 20)], seed=50 + d), {}, [[1]]


def single_edge_reversed(d):
    return cl.scene(d, [12, 15], [(20, 4)], seed=55 + d), {}, [[1]]


def degenerate(d):
    """One stage against chain 0, exact closures with a = a pose of chain 0 (so q = x_t(b) of the moving chain).  Chain 1: all
    kappa = 0 and every closure to ONE pose of the chain (refused: no spread).  Chain 2: kappa = 0, its poses on a line:
    refused at d = 3 (rank 1), placed at d = 2.  Chain 3: kappa = 0, the line scattered by 1e-3 of its length: placed.
    Chain 4: kappa > 0, tau = 0: placed by the rotations alone (W = 0: s = l_0 - G q_0)."""
    rng = np.random.default_rng(390 + d)
    lens = [20, 10, 10, 10, 10]
    u = rng.normal(0, 1, d)
    u /= np.linalg.norm(u)
    line = np.outer(np.linspace(0, 40, 10), u)
    world = np.concatenate([np.cumsum(rng.normal(0, 1, (20, d)), axis=0), rng.uniform(-5, 5, (10, d)), rng.uniform(-5, 5, d) + line,
                            rng.uniform(-5, 5, d) + line + 0.04 * rng.normal(0, 1, (10, d)), rng.uniform(-5, 5, (10, d))])
    pairs, kappa, tau = [], [], []
    for c in range(1, 5):
        for k in range(12):
            j = 20 + 10 * (c - 1) + (3 if c == 1 else k % 10)
            pairs.append((int(rng.integers(20)), j))
            kappa.append(1.0 if c == 4 else 0.0)
            tau.append(0.0 if c == 4 else 1.0)
    return cl.scene(d, lens, pairs, seed=60 + d, kappa=kappa, tau=tau, world=world), {}, [[1, 2, 3, 4]]


def in_place(d):
    """A chain already in place, on exactly representable data: unit steps along the first axis, identity rotations, exact
    closures in both directions.  cost_start is 0 exactly, so nothing is below it: chosen 0, the rows bit-identical."""
    n = 12 + 12
    t0 = d * n
    X = np.zeros((t0 + n, d))
    er, ed, chains = [], [], []
    for c in range(2):
        chains.append(list(range(len(er), len(er) + 11)))
        for i in range(12 * c, 12 * c + 12):
            X[d * i:d * i + d] = np.eye(d)
            X[t0 + i, 0], X[t0 + i, 1] = i - 12 * c, 7 * c
            if i < 12 * c + 11:
                er.append([d * i, d * (i + 1), t0 + i, t0 + i + 1])
                ed.append(np.concatenate([np.eye(d).reshape(-1), np.eye(d)[0], [1.0, 1.0]]))
    rng = np.random.default_rng(400 + d)
    for k in range(8 * d):
        i, j = int(rng.integers(12)), 12 + int(rng.integers(12))
        if k % 2:
            i, j = j, i
        er.append([d * i, d * j, t0 + i, t0 + j])
        ed.append(np.concatenate([np.eye(d).reshape(-1), X[t0 + j] - X[t0 + i], [1.0, 2.0]]))
    table = (np.array(er, dtype=np.int32), np.array(ed), np.zeros((0, 3), dtype=np.int32), np.zeros((0, 2)))
    return ((d, n, 0, n), table, X, chains, None), {}, [[1]]


BUILDERS = dict(lengths=lengths, lengths_noisy=lambda d: lengths(d, noise=0.05), offset=lambda d: lengths(d, offset=1e4),
                offset_noisy=lambda d: lengths(d, noise=0.05, offset=1e4), relay=relay, same_stage=same_stage, statuses=statuses,
                single_edge=single_edge, single_edge_reversed=single_edge_reversed, degenerate=degenerate, in_place=in_place)
SYNTHETIC = [(name, d) for name in BUILDERS for d in (2, 3)]


def case(name, d, device=-1):
    """(ctx, dims, table, X, chains, kw, expect, truth) of a synthetic case, tables installed."""
    key = (name, d, device)
    if key not in _BUILT:
        (dims, table, X, chains, truth), kw, expect = BUILDERS[name](d)
        ctx = capi.Context(*dims, *cl.diagonal_q(*dims), device=device)
        ctx.set_measurements(*table)
        ctx.set_odometry_chains(chains)
        ctx.set_closure_placement(**kw)
        _BUILT[key] = (ctx, dims, table, X, chains, kw, expect, truth)
    return _BUILT[key]


def reference_of(name, d):
    """Computed once and shared (tests/test_gpu_closure.py reads the same)."""
    key = ("ref", name, d)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, _, _ = case(name, d)
        _BUILT[key] = cl.reference(*dims, table, chains, X, **kw)
    return _BUILT[key]


def mirror_of(name, d):
    key = ("mirror", name, d)
    if key not in _BUILT:
        ctx, dims, table, X, chains, kw, _, _ = case(name, d)
        got = ctx.debug_place_by_closures_host(X)
        got["X_in"] = X
        _BUILT[key] = got
    return _BUILT[key]


def check_structure(ctx, ref):
    assert ctx.closure_placement_counts() == ref["struct"]["counts"]
    assert [list(map(int, items)) for items in ctx.closure_placement_order()] == ref["struct"]["order"]


def used_entries(ref):
    return [e for st in ref["struct"]["stages"] for _, es in st for e in es]


@pytest.mark.parametrize("name,d", SYNTHETIC)
def test_mirror_on_the_synthetic_cases(name, d):
    ctx, dims, table, X, chains, kw, expect, truth = case(name, d)
    ref, got = reference_of(name, d), mirror_of(name, d)
    check_structure(ctx, ref)
    assert ref["struct"]["order"] == expect, ref["struct"]["order"]
    worst = cl.check(got, *dims, table, ref)
    kap = max([one.get("kappa", 0.0) for one in ref["chain"].values()] + [0.0])
    print("%s d=%d: worst error / (a + b) %.4f (largest condition %.3g); statuses %s chosen %s" % (name, d, worst, kap, got["status"], got["chosen"]))
    for c in range(len(chains)):
        assert got["cost_final"][c] <= got["cost_start"][c]
    if name.startswith("lengths") or name.startswith("offset"):
        assert list(got["status"]) == [4, 0, 0, 0, 0, 0] and got["placed"] == 5 and np.all(got["chosen"][1:] == 1)
        assert ref["struct"]["counts"] == (1, sum(LIST_LENS), 1 + 1 + 1 + 2 + 65, 0)
    if name == "relay":
        assert np.all(got["status"][1:] == 0) and np.all(got["chosen"][1:] == 1) and got["stages"] == 3
        assert [len(es) for st in ref["struct"]["stages"] for _, es in st] == [6, 5, 7] and ref["struct"]["unused"] == 0
    if name == "same_stage":
        assert list(got["status"]) == [4, 0, 0] and ref["struct"]["unused"] == 4 and ref["struct"]["counts"] == (1, 17, 2, 4)
    if name == "statuses":
        assert list(got["status"]) == [4, 0, 1, 3, 4] and got["placed"] == 1 and got["not_placed"] == 2 and got["refused"] == 0
        assert ref["struct"]["skipped"] == 3 and ref["struct"]["unused"] == 2 and ref["struct"]["counts"] == (1, 8, 1, 5)
    if name == "degenerate":
        assert list(got["status"]) == ([4, 2, 0, 0, 0] if d == 2 else [4, 2, 2, 0, 0]) and got["refused"] == (1 if d == 2 else 2)
        for c in range(1, 5):   # either side of the rule, 100 x away on the exact sums
            m = ref["chain"][c]["margin"]
            print("  chain %d: status %d, the rule's quantity / threshold %s" % (c, got["status"][c], m))
            assert m is None or m >= 100 or m <= 0.01, (c, m)
        assert got["chosen"][4] == 1   # rotation only
    if name == "in_place":
        assert list(got["status"]) == [4, 0] and got["chosen"][1] == 0 and got["cost_start"][1] == 0
        assert np.array_equal(cl.bits(got["X"]), cl.bits(X))


@pytest.mark.parametrize("name,d", SYNTHETIC)
def test_cost_start_is_the_tables_own_residual(name, d):
    """An independent path: cora_debug_measurement_residuals_host's rot + trans over the list's edges, at the vector as it
    stood when the list was solved (the chains placed before it moved, the list's chain not yet), to a few ulps of the sum."""
    ctx, dims, table, X, chains, kw, expect, truth = case(name, d)
    ref, got = reference_of(name, d), mirror_of(name, d)
    for st in ref["struct"]["stages"]:
        for c, es in st:
            V = np.array(got["X"])
            for rot, trn in ref["struct"]["positions"][c]:
                V[rot:rot + d], V[trn] = X[rot:rot + d], X[trn]
            res = ctx.debug_measurement_residuals_host(V)
            e = [k for k, _ in es]
            total = math.fsum(res["edge_rot"][e]) + math.fsum(res["edge_trans"][e])
            assert abs(got["cost_start"][c] - total) <= 16 * cl.EPS * total, (c, got["cost_start"][c], total)
            assert abs(float(ref["cost_start"][c]) - total) <= 16 * cl.EPS * total


@pytest.mark.parametrize("name,d", [(name, d) for name in ("lengths", "offset") for d in (2, 3)])
def test_exact_data(name, d):
    """Noise-free closures, every chain displaced by a known rigid motion: the transform is the truth's within the bound, and
    the closure cost afterwards is below 1e-18 sum (kappa d + tau |l|^2) (the rounding of the written numbers is eps per
    length and per rotation entry, squared; composition over <= 1e3 positions)."""
    ctx, dims, table, X, chains, kw, expect, truth = case(name, d)
    ref, got = reference_of(name, d), mirror_of(name, d)
    es = used_entries(ref)
    _, _, l, kappa, tau, *_ = cl.entries(d, table, np.asarray(got["X"], dtype=cl.LD), es)
    scale = float(np.sum(kappa * d + tau * np.sum(l * l, axis=1)))
    after, before = float(cl.closure_cost(d, table, got["X"], es)), float(cl.closure_cost(d, table, X, es))
    print("%s d=%d: closure cost %.3e -> %.3e, sum (kappa d + tau |l|^2) %.3e, ratio %.3e" % (name, d, before, after, scale, after / scale))
    assert after < 1e-18 * scale and not before < 1e-18 * scale
    for c in range(1, len(chains)):
        Rc, tc = truth[c]
        one = ref["chain"][c]
        a_T = one["a_R"] * float(cl._norm(one["cq"])) + one["a_t"]
        # (the truth is the reference's minimiser up to the rounding of the data it was built from)
        slack = 64 * cl.EPS * (1 + np.linalg.norm(tc) + float(cl._norm(one["cq"]))) * max(one["kappa"], 1.0)
        assert np.abs(got["transforms"][c][:d * d].reshape(d, d) - Rc).max() <= cl.C_BOUND * one["a_R"] + slack
        assert np.abs(got["transforms"][c][d * d:] - tc).max() <= cl.C_BOUND * a_T + one["b_t"] + slack * (1 + float(cl._norm(one["cq"])))


@pytest.mark.parametrize("name,d", [(name, d) for name in ("single_edge", "single_edge_reversed") for d in (2, 3)])
def test_a_single_edge_is_met(name, d):
    """Both residuals of the one closure are zero to rounding afterwards: rot <= (16 eps)^2 kappa d, trans <= (16 eps)^2 tau
    (|x_t(a)| + |x_t(b)| + |t|)^2."""
    ctx, dims, table, X, chains, kw, _, _ = case(name, d)
    got = mirror_of(name, d)
    e = len(table[0]) - 1
    res = ctx.debug_measurement_residuals_host(got["X"])
    size = np.linalg.norm(got["X"][table[0][e, 2]]) + np.linalg.norm(got["X"][table[0][e, 3]]) + np.linalg.norm(table[1][e, d * d:d * d + d])
    assert got["chosen"][1] == 1 and got["cost_final"][1] <= (16 * cl.EPS) ** 2 * (d + size ** 2)
    assert res["edge_rot"][e] <= (16 * cl.EPS) ** 2 * d and res["edge_trans"][e] <= (16 * cl.EPS * size) ** 2


@pytest.mark.parametrize("name,d", [("lengths_noisy", 2), ("relay", 3), ("degenerate", 3)])
def test_two_calls_give_the_same_bits(name, d):
    ctx, dims, table, X, chains, kw, _, _ = case(name, d)
    a, b = mirror_of(name, d), ctx.debug_place_by_closures_host(X)
    for key in ("X", "cost_start", "cost_final", "transforms"):
        assert np.array_equal(cl.bits(a[key]), cl.bits(b[key])), key
    for key in ("status", "chosen", "degenerate"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("name,d", [("lengths", 3), ("lengths_noisy", 2), ("relay", 2), ("relay", 3), ("same_stage", 3), ("degenerate", 2), ("single_edge", 3)])
def test_a_second_application_stays_within_the_bound(name, d):
    """From where the first call ended: the reference's structure and bound again, never worse."""
    ctx, dims, table, X, chains, kw, _, _ = case(name, d)
    first = mirror_of(name, d)
    again = ctx.debug_place_by_closures_host(first["X"])
    again["X_in"] = first["X"]
    cl.check(again, *dims, table, cl.reference(*dims, table, chains, first["X"], **kw))


def test_no_inter_chain_closure_is_a_no_op():
    """A catalogue graph whose closures all lie inside one chain: no stage, nothing written but the range rows."""
    import odom_ref as od
    import residuals_ref as rr
    A, Q, dm, g = tp.build("robots-d2")
    dims, table, chains = (dm.d, dm.n, dm.r, dm.n_trans), rr.table(g), od.chains_of(g)
    ctx = capi.Context(*dims, Q.rowptr, Q.col, Q.val, device=-1)
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_closure_placement()
    assert ctx.closure_placement_counts()[:3] == (0, 0, 0) and ctx.closure_placement_order() == []
    X = np.array(A["truth"], dtype=np.float64)
    got = ctx.debug_place_by_closures_host(X)
    t0 = dm.d * dm.n + dm.r
    assert got["stages"] == 0 and got["placed"] == 0 and got["status"][0] == 4 and np.all(got["status"][1:] == 3)
    assert np.array_equal(cl.bits(got["X"][:dm.d * dm.n]), cl.bits(X[:dm.d * dm.n])) and np.array_equal(cl.bits(got["X"][t0:]), cl.bits(X[t0:]))


@pytest.mark.parametrize("d", [2, 3])
def test_path_of_four_robots(d):
    """The graph of tests/test_gpu_closure.py's start test (four robots on a path A - B - C - D, 3 noisy closures per pair, both
    directions), every chain after A's in a frame of its own: three stages of one chain each, the mirror within the
    reference's bound, and the closure cost falls from the displaced frames' to the noise's level."""
    import odom_ref as od
    import residuals_ref as rr
    from oracle import assemble as asm
    from oracle import oracle as orc
    import placement_ref as pl
    w = cl.path_world(d)
    A = asm.assemble(w.g)
    Q = orc.CSR.from_scipy(A["Q"])
    n = A["n"]
    dims, table, chains = (d, n, A["r"], n), rr.table(w.g), od.chains_of(w.g)
    ctx = capi.Context(*dims, Q.rowptr, Q.col, Q.val, device=-1)
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_closure_placement()
    assert [list(map(int, s)) for s in ctx.closure_placement_order()] == [[1], [2], [3]] and ctx.closure_placement_counts() == (3, 9, 3, 0)
    X = w.truth()
    rng = np.random.default_rng(5)
    first = np.cumsum([0, 40, 60, 47, 53])
    for c in range(1, 4):
        G, s = pl._rot(d, rng, 2.5), 10 * rng.uniform(-1, 1, d)
        for i in range(first[c], first[c + 1]):
            X[d * i:d * i + d] = X[d * i:d * i + d] @ G.T
            X[d * n + i] = G @ X[d * n + i] + s
    got = ctx.debug_place_by_closures_host(X)
    got["X_in"] = X
    ref = cl.reference(*dims, table, chains, X)
    worst = cl.check(got, *dims, table, ref)
    es = used_entries(ref)
    before, after, truth = (float(cl.closure_cost(d, table, V, es)) for V in (X, got["X"], w.truth()))
    print("path of four robots d=%d: closure cost %.4g -> %.4g (at the truth %.4g); worst error / (a + b) %.4f" % (d, before, after, truth, worst))
    assert list(got["status"]) == [4, 0, 0, 0] and np.all(got["chosen"][1:] == 1)
    # (a list's minimum is at most its cost at the motion that agrees with the chains placed before it, the edges' own noise)
    assert after < 1e-3 * before and after <= truth * (1 + 1e-9)


def test_refusals():
    (dims, table, X, chains, _), kw, _ = relay(2)
    ctx = capi.Context(*dims, *cl.diagonal_q(*dims), device=-1)

    def code(fn, *a, **k):
        with pytest.raises(capi.CoraError) as e:
            fn(*a, **k)
        return e.value.code
    assert code(ctx.set_closure_placement) == ERR_NOT_READY                      # no measurement table
    assert code(ctx.debug_place_by_closures_host, X) == ERR_NOT_READY
    ctx.set_measurements(*table)
    assert code(ctx.set_closure_placement) == ERR_NOT_READY                      # no chain tables
    ctx.set_odometry_chains(chains)
    assert code(ctx.debug_place_by_closures_host, X) == ERR_NOT_READY            # no closure tables
    assert code(ctx.set_closure_placement, min_closures=0) == ERR_ARG            # below 1
    assert code(ctx.set_closure_placement, chain_fixed=[0, 0, 0, 0]) == ERR_ARG  # a mask that fixes no chain
    assert ctx.closure_placement_counts() == (0, 0, 0, 0)
    ctx.set_closure_placement(min_closures=4)
    counts = ctx.closure_placement_counts()
    assert counts == (3, 18, 3, 0)
    assert code(ctx.set_closure_placement, min_closures=0) == ERR_ARG and ctx.closure_placement_counts() == counts   # a refused call keeps the tables
    out = (capi.C.c_int64 * 5)()
    Xf = np.asfortranarray(X)
    none = [None] * 6
    assert ctx.L.cora_debug_place_by_closures_host(ctx.h, capi._d(Xf), ctx.N - 1, out, *none) == ERR_SHAPE
    assert ctx.L.cora_debug_place_by_closures_host(ctx.h, None, ctx.N, out, *none) == ERR_ARG
    assert ctx.L.cora_debug_place_by_closures_host(ctx.h, capi._d(Xf), ctx.N, None, *none) == ERR_ARG
    assert ctx.L.cora_debug_place_by_closures_host(ctx.h, capi._d(Xf), ctx.N, out, *none) == 0 and list(out) == [3, 0, 0, 3, 0]
    assert code(ctx.place_by_closures, X) == ERR_HIP                             # a device form on a plan-only handle
    # two range measurements that name one range row: the chain tables refuse such a table before the closure tables can
    rows = table[2].copy()
    rows[1, 0] = rows[0, 0]
    ctx.set_measurements(table[0], table[1], rows, table[3])
    assert code(ctx.set_odometry_chains, chains) == ERR_ARG and code(ctx.set_closure_placement) == ERR_NOT_READY
    ctx.set_measurements(*table)
    ctx.set_odometry_chains(chains)
    ctx.set_closure_placement(min_closures=4)
    # new chains and a new measurement table drop the closure tables
    ctx.set_odometry_chains(chains)
    assert ctx.closure_placement_counts() == (0, 0, 0, 0) and code(ctx.debug_place_by_closures_host, X) == ERR_NOT_READY
    ctx.set_closure_placement()
    ed = table[1].copy()
    ed[len(table[0]) - 18:, 2 * 2 + 2 + 1] = 1e308   # tau of every closure: sum tau overflows
    ctx.set_measurements(table[0], ed, table[2], table[3])
    assert ctx.closure_placement_counts() == (0, 0, 0, 0)
    ctx.set_odometry_chains(chains)
    ctx.set_closure_placement()
    assert code(ctx.debug_place_by_closures_host, X) == ERR_NAN


def test_partitioned_handles_are_refused():
    A, Q, dm, g = tp.build("robots-d2")
    p = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=2)
    for fn, args in ((p.set_closure_placement, ()), (p.debug_place_by_closures_host, (np.zeros((p.N, 2)),))):
        with pytest.raises(capi.CoraError) as e:
            fn(*args)
        assert e.value.code == ERR_ARG and "partitioned" in str(e.value)
