"""The rounding to SE(d) without a GPU: cora_debug_round_host (the functions the kernels call, on plan-only handles)
against the mpmath / longdouble reference of tests/round_ref.py within the calibrated bound, the basis on its own, every
family of rowops_ref's block catalogue lifted into a relaxed point, the exact and degenerate cases, the majority rule,
and the refusals.  Problem.round_solution against Problem.project_solution and its implicit formulation run the device form
(there is no host fall-back), so they live in tests/test_gpu_round.py."""
import numpy as np
import pytest

import round_ref as rf
import rowops_ref as ro
import topologies as tp
from cora_amd import capi, host
from oracle import assemble as asm
from oracle import oracle as orc
from synth import ground_truth, make_graph

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_HIP, ERR_ARG = 1, 2, 3, 4, 5
TOPOLOGIES = ("robots-d2", "robots-d3", "n1", "n2", "n64", "n65", "singletons", "priors_chain_odd")

_BUILT = {}


def built(d, n):
    """(ctx, (d, n, r, nt), ground truth) of a graph of tests/synth.py on a plan-only handle, once per process."""
    key = (d, n)
    if key not in _BUILT:
        g = make_graph(d=d, n=n, n_landmarks=3, n_ranges=min(20, n * 3), n_loops=0)
        A = asm.assemble(g)
        Q = orc.CSR.from_scipy(A["Q"])
        dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
        ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1)
        _BUILT[key] = (ctx, (dm.d, dm.n, dm.r, dm.n_trans), ground_truth(g))
    return _BUILT[key]


def catalogue(name):
    key = ("tp", name)
    if key not in _BUILT:
        A, Q, dm, g = tp.build(name)
        ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1)
        _BUILT[key] = (ctx, (dm.d, dm.n, dm.r, dm.n_trans), A["truth"])
    return _BUILT[key]


# ---- calibration of the bound
def test_calibration():
    """The float64 route the bound is calibrated on stays below the constants of round_ref (the library gets twice)."""
    for d in (2, 3):
        worst = worst_orth = 0.0
        for k in rf.KS(d):
            Vd = rf.basis(d, k)
            for name, kk, seed in rf.catalogue(d):
                Yi = rf.lifted(ro.block(name, kk, d, d, seed), Vd)
                got = rf.svd_route(Yi, Vd)
                err, kap, _ = rf.block_error(got, Yi, Vd)
                worst, worst_orth = max(worst, err), max(worst_orth, ro.orth_error(got))
        print("d = %d: float64 SVD route worst %.3f eps kappa, |R R^T - I| %.3e" % (d, worst, worst_orth))
        assert worst <= rf.REF_ROUND_WORST


def test_calibration_of_the_singular_values():
    """numpy's eigh on the float64 Gram matrix against eigh on the longdouble one, over every input the host-mirror tests
    and the device tests round (the same graphs, column counts and seeds): the library's singular values get twice this."""
    worst = 0.0
    for d in (2, 3):
        for n in (1, 2, 30, 64, 65, 300):
            g = make_graph(d=d, n=n, n_landmarks=3, n_ranges=min(20, n * 3), n_loops=0)
            A = asm.assemble(g)
            dims, truth = (A["d"], A["n"], A["r"], A["N"] - A["d"] * A["n"] - A["r"]), ground_truth(g)
            for seed in (10 * n + d, 100 * d + n):
                rng = np.random.default_rng(seed)
                for k in rf.KS(d):
                    Y = rf.relaxed_point(truth, *dims, k, rng)
                    worst = max(worst, rf.sigma_error(rf.sigma_float64_route(Y), Y))
    for name in TOPOLOGIES:
        A, Q, dm, g = tp.build(name)
        rng = np.random.default_rng(len(name))
        for k in rf.KS(dm.d):
            Y = rf.relaxed_point(A["truth"], dm.d, dm.n, dm.r, dm.n_trans, k, rng)
            worst = max(worst, rf.sigma_error(rf.sigma_float64_route(Y), Y))
    print("float64 Gram + eigh: worst singular-value error %.3f eps sigma_1^2 / sigma" % worst)
    assert worst <= rf.REF_SIGMA_WORST


# ---- the host mirror against the reference
def run_all_ranks(ctx, dims, truth, rng, what):
    d = dims[0]
    for k in rf.KS(d):
        Y = rf.relaxed_point(truth, *dims, k, rng)
        res = ctx.debug_round_host(Y)
        rf.check(res, Y, *dims, what="%s k=%d" % (what, k))
        rf.basis_checks(res, Y, what="%s k=%d" % (what, k))
        again = ctx.debug_round_host(Y, basis=res["Vd"])
        assert np.array_equal(again["X"], res["X"]) and again["count"] == res["count"] and again["flipped"] == res["flipped"]


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", [30, 65])
def test_host_mirror_against_the_reference_on_synthetic_graphs(d, n):
    ctx, dims, truth = built(d, n)
    run_all_ranks(ctx, dims, truth, np.random.default_rng(10 * n + d), "synth d=%d n=%d" % (d, n))


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_host_mirror_against_the_reference_on_the_catalogue(name):
    ctx, dims, truth = catalogue(name)
    run_all_ranks(ctx, dims, truth, np.random.default_rng(len(name)), name)


# ---- every family of the block catalogue as pose blocks
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("large", [False, True])
def test_catalogue_blocks_lifted_into_a_relaxed_point(d, large):
    ctx, dims, truth = built(d, 30)
    rng = np.random.default_rng(300 + d)
    cat = rf.catalogue(d, large)
    assert len(cat) <= dims[1]
    blocks = [ro.block(name, kk, d, d, seed) for name, kk, seed in cat]
    for k in rf.KS(d):
        Vd = rf.basis(d, k)
        Y = rf.with_blocks(rf.in_span(truth, dims, Vd, rng), d, blocks, Vd)
        res = ctx.debug_round_host(Y, basis=Vd)
        assert np.array_equal(res["Vd"], Vd)
        rf.check(res, Y, *dims, what="catalogue d=%d k=%d large=%s" % (d, k, large))


# ---- exact and edge cases
@pytest.mark.parametrize("d", [2, 3])
def test_degenerate_blocks(d):
    ctx, dims, truth = built(d, 30)
    rng = np.random.default_rng(500 + d)
    rot = rf.rows(*dims)[0]
    for k in rf.KS(d):
        Vd = rf.basis(d, k)
        u = rng.standard_normal(d)
        rank1 = np.outer(rng.standard_normal(d), u)
        blocks = [np.zeros((d, d)), rank1, np.outer(np.eye(d)[0], u)]  # zero, rank 1, one row only
        if d == 3:
            B = rng.standard_normal((3, 3))
            B[2] = 0.5 * B[0] - 2.0 * B[1]
            C = rng.standard_normal((3, 3))
            C[1] = 0.0
            blocks += [B, C]  # rank 2: a dependent row, a zero row
        Y = rf.with_blocks(rf.in_span(truth, dims, Vd, rng), d, blocks, Vd, first=3)
        res = ctx.debug_round_host(Y, basis=Vd)
        rf.check(res, Y, *dims, what="degenerate d=%d k=%d" % (d, k), blocks=False)
        X = res["X"]
        assert np.array_equal(X[rot[3]], np.eye(d)), "a zero block gives exactly the identity"
        for j, B in enumerate(blocks):
            R = X[rot[3 + j]]
            M = (Y[rot[3 + j]].astype(rf.LD) @ Vd.astype(rf.LD)).astype(np.float64)
            if res["flipped"]:
                M[:, -1] = -M[:, -1]
            sig = np.linalg.svd(M, compute_uv=False)
            # the smallest singular value is zero up to rounding: every rotation that maps the directions that are there
            # onto each other attains tr(R^T M) = the sum of the others; the deviation is of second order in the error of
            # R, and is held here to the first-order bound of d^2 entries of size sigma_1
            assert np.trace(R.T @ M) >= sig.sum() - 2 * sig[-1] - rf.ROUND_BOUND * rf.EPS * d * d * sig[0], (d, k, j)
            assert ro.orth_error(R) <= rf.ORTH_BOUND and abs(np.linalg.det(R) - 1.0) <= 1e-12


@pytest.mark.parametrize("d", [2, 3])
def test_a_reflection_block_gets_its_smallest_direction_flipped(d):
    ctx, dims, truth = built(d, 30)
    rng = np.random.default_rng(600 + d)
    rot = rf.rows(*dims)[0]
    Vd = rf.basis(d, d + 1)
    u, _ = np.linalg.qr(rng.standard_normal((d, d)))
    v, _ = np.linalg.qr(rng.standard_normal((d, d)))
    sig = np.array([3.0, 2.0, 0.5][:d])
    sig[-1] = 0.5
    D = np.eye(d)
    D[-1, -1] = -1.0 if np.linalg.det(u @ v.T) > 0 else 1.0   # det(B) < 0
    B = (u * sig) @ D @ v.T
    assert np.linalg.det(B) < 0
    Y = rf.with_blocks(rf.in_span(truth, dims, Vd, rng), d, [B], Vd, first=5)
    res = ctx.debug_round_host(Y, basis=Vd)
    assert not res["flipped"]
    R = res["X"][rot[5]]
    # the maximiser: u diag(1, .., 1, -1) (D v^T) with the minus on the direction of sigma = 0.5
    E = np.eye(d)
    E[-1, -1] = -1.0
    want = u @ E @ D @ v.T
    assert abs(np.linalg.det(want) - 1.0) < 1e-12
    assert np.abs(R - want).max() <= 1e-13
    assert abs(np.trace(R.T @ B) - (sig[:-1].sum() - sig[-1])) <= 1e-13


@pytest.mark.parametrize("d", [2, 3])
def test_a_zero_range_row_stays_zero(d):
    ctx, dims, truth = built(d, 30)
    rng = np.random.default_rng(700 + d)
    rng_rows = rf.rows(*dims)[1]
    Y = rf.relaxed_point(truth, *dims, 5, rng)
    Y[rng_rows[2]] = 0.0
    Y[rng_rows[4]] *= 1e-170
    Y[rng_rows[5]] *= 1e120
    res = ctx.debug_round_host(Y)
    assert np.all(res["X"][rng_rows[2]] == 0.0)
    others = np.delete(rng_rows, 2)
    assert np.all(np.abs(np.linalg.norm(res["X"][others], axis=1) - 1.0) <= 4 * rf.EPS)
    rf.check(res, Y, *dims, what="zero range row d=%d" % d)


# ---- the majority rule
@pytest.mark.parametrize("name", ["n1", "n2", "n65"])
def test_the_majority_rule_at_its_edges(name):
    ctx, dims, truth = catalogue(name)
    d, n = dims[0], dims[1]
    rng = np.random.default_rng(800 + n)
    rot = rf.rows(*dims)[0]
    k = d + 2
    Vd = rf.basis(d, k)
    base = truth @ Vd.T
    tried = set()
    for positive in (n // 2 - 1, n // 2, n // 2 + 1, 0, n):
        if positive < 0 or positive > n or positive in tried:
            continue
        tried.add(positive)
        Y = base.copy()
        for i in rng.permutation(n)[positive:]:      # a reflection of the other blocks: the last column of Y_i Vd negated
            M = Y[rot[i]] @ Vd
            M[:, -1] = -M[:, -1]
            Y[rot[i]] = M @ Vd.T
        res = ctx.debug_round_host(Y, basis=Vd)
        assert res["count"] == positive, (name, positive, res["count"])
        assert res["flipped"] == (positive < n // 2), (name, positive)
        rf.check(res, Y, *dims, what="majority %s %d of %d" % (name, positive, n))


# ---- refusals and paths
def test_refusals():
    ctx, dims, truth = built(3, 30)
    rng = np.random.default_rng(9)
    for k in (1, 2, 25):
        with pytest.raises(capi.CoraError) as e:
            ctx.debug_round_host(rng.standard_normal((truth.shape[0], k)))
        assert e.value.code == ERR_SHAPE, k
    for bad in (np.nan, np.inf, -np.inf):
        Y = rf.relaxed_point(truth, *dims, 5, rng)
        Y[17, 3] = bad
        with pytest.raises(capi.CoraError) as e:
            ctx.debug_round_host(Y)
        assert e.value.code == ERR_NAN, bad
    with pytest.raises(capi.CoraError) as e:   # the device forms need a device
        ctx.round(rf.relaxed_point(truth, *dims, 5, rng))
    assert e.value.code == ERR_HIP


def test_a_partitioned_handle_is_refused():
    g = make_graph(d=2, n=30, n_landmarks=3, n_ranges=20, n_loops=0)
    A = asm.assemble(g)
    Q = orc.CSR.from_scipy(A["Q"])
    dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
    ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=2)
    with pytest.raises(capi.CoraError) as e:
        ctx.debug_round_host(np.zeros((dm.N, 4)))
    assert e.value.code == ERR_ARG


@pytest.mark.parametrize("d", [2, 3])
def test_no_lift_at_k_equal_d(d):
    """k = d: Vd is a signed permutation of the axes when the Gram matrix is diagonal, an orthogonal matrix otherwise; a
    point of the manifold comes back as itself times Vd."""
    ctx, dims, truth = built(d, 30)
    res = ctx.debug_round_host(truth)
    rf.check(res, truth, *dims, what="k = d")
    assert np.abs(res["Vd"].T @ res["Vd"] - np.eye(d)).max() <= 4 * rf.EPS
    assert not res["flipped"] or res["count"] < dims[1] // 2
    rot, rng_rows, trn = rf.rows(*dims)
    want = truth @ res["Vd"]
    if res["flipped"]:
        want[:, -1] = -want[:, -1]
    assert np.abs(res["X"] - want).max() <= 1e-13 * max(1.0, np.abs(truth).max())


def test_extreme_scales_take_the_scaled_gram_matrix():
    """An input whose squares overflow or vanish altogether is rounded like its scaled copy."""
    ctx, dims, truth = built(3, 30)
    rng = np.random.default_rng(11)
    Y = rf.relaxed_point(truth, *dims, 5, rng)
    base = ctx.debug_round_host(Y)
    rot = rf.rows(*dims)[0]
    for e in (600, -600, 1000, -1040, -1060):   # (the last two: every entry subnormal, some of them zero)
        res = ctx.debug_round_host(np.ldexp(Y, e))
        assert res["count"] == base["count"] and res["flipped"] == base["flipped"]
        # (below 2^-1022 an entry keeps 52 - (1022 - its exponent) bits: the input itself is a rounded copy)
        lost = 2.0 ** max(0, -e - 1022 + 8)
        assert np.abs(res["X"][rot.ravel()] - base["X"][rot.ravel()]).max() <= 1e-9 * lost, e
        for i in range(dims[1]):
            R = res["X"][rot[i]]
            assert ro.orth_error(R) <= rf.ORTH_BOUND and abs(np.linalg.det(R) - 1.0) <= 1e-12
        if abs(e) <= 600:
            assert np.abs(res["sigma"][:3] / np.ldexp(base["sigma"][:3], e) - 1).max() <= 1e-9


def test_problem_round_solution_checks_its_row_count():
    """A wrong row count is refused before anything reaches the device (the column counts are checked by the device form:
    tests/test_gpu_round.py)."""
    P = tp.to_problem("n2")
    A, Q, dm, g = tp.build("n2")
    with pytest.raises(host.HostError, match="expected %d rows" % A["truth"].shape[0]):
        P.round_solution(A["truth"][:-1])
