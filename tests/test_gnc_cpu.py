"""The GNC weight step without a GPU: cora_debug_gnc_weights_host (the device's sequence of operations on the host) on
plan-only handles -- its unweighted residuals against tests/residuals_ref.py, its weights and statistics against the
longdouble reference of tests/gnc_ref.py within that file's derived bounds, and every refusal."""
import ctypes as C
import os

import numpy as np
import pytest

import assembly_ref as ar
import gnc_ref as gr
import residuals_ref as rr
from conftest import GOLDEN
from cora_amd import capi, host

ERR_SHAPE, ERR_NOT_READY, ERR_NAN, ERR_ARG = 1, 2, 3, 5
REL = 1e-10  # tests/test_gpu_residuals.py: relative to the largest value, only the summation order differs
MUS = (1e-8, 0.3, 1.0, 1.4, 1e2, 1e8)
BARC2 = (1e-6, 1.0, 7.8, 1e5)
INF = float("inf")


def built(name):
    g, Q, dm, ref = ar.graph(name)
    ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1)
    ctx.set_measurements(*rr.table(g))
    ctx.assembly_build(Q.rowptr, Q.col)
    return ctx, g, Q, dm, ref


def flat(ref):
    return np.concatenate([ref["edge_rot"], ref["edge_trans"], ref["range"]])


@pytest.mark.parametrize("name", ["small_ra_slam_problem", "rplm_priors", "hub-d3", "single_range", "single_rpm"])
def test_residuals_are_the_references_and_unweighted(name):
    ctx, g, Q, dm, ref = built(name)
    nw, ne = ref.n_weights, len(rr.edges(g))
    rng = np.random.default_rng(3)
    barc2 = np.full(nw, 7.8)
    before = {}
    for k in (1, dm.d, 5, 8, 17, 24):
        X = rng.standard_normal((dm.N, k))
        got = ctx.debug_gnc_weights_host(X, barc2, "tls", 1.4)
        want = flat(rr.reference(g, X))
        err = np.abs(got["r2"] - want).max(initial=0.0)
        print("%s k=%d: max error %.3e of largest value %.3e" % (name, k, err, want.max(initial=0.0)))
        assert err <= REL * max(want.max(initial=0.0), 1e-300)
        no_rot = rr.table(g)[0][:, 1] < 0
        assert np.all(got["r2"][:ne][no_rot] == 0.0)  # the rot slot of an edge without a rotation part
        before[k] = (X, got)
    # after a re-weighting with zeros the table's kappa, tau, omega are base * w: the step does not see them
    w = ar.random_weights(nw, 12)
    assert nw < 8 or np.any(w == 0.0)
    ctx.assemble_values(w)
    for k, (X, got) in before.items():
        again = ctx.debug_gnc_weights_host(X, barc2, "tls", 1.4)
        for key in ("r2", "w", "stats_raw"):
            assert np.array_equal(got[key], again[key]), (k, key)
    weighted = flat(ctx.debug_measurement_residuals_host(before[5][0]))
    assert nw < 8 or not np.array_equal(weighted, before[5][1]["r2"])  # (the residuals mirror does follow the weights)
    ctx.close()


def _thresholds(r2, ne, cost, mu, couple, rng):
    """Thresholds that put the ratios where the formulas can go wrong: the four magnitudes of BARC2, +inf, and for TLS
    ratios at both boundaries -- exactly there for mu = 1 (the boundaries 1/2 and 2 are powers of two), within an ulp
    otherwise."""
    nw = len(r2)
    c = rng.choice(BARC2, nw)
    c[rng.uniform(size=nw) < 0.1] = INF
    judged = r2.copy()
    if couple:
        judged[:ne] = judged[ne:2 * ne] = r2[:ne] + r2[ne:2 * ne]
    lo, hi = mu / (mu + 1), (mu + 1) / mu
    at = np.flatnonzero(judged > 0)
    for j, i in enumerate(at[:24]):
        b = (lo, hi, np.sqrt(lo * hi) * 1.3)[j % 3]  # a boundary, the other one, the middle band
        c[i] = judged[i] / b
    if mu == 1.0 and len(at) >= 2:
        assert judged[at[0]] / c[at[0]] == 0.5 and judged[at[1]] / c[at[1]] == 2.0
    return c


@pytest.mark.parametrize("couple", [False, True])
@pytest.mark.parametrize("cost", [gr.NONE, gr.TLS, gr.GM])
@pytest.mark.parametrize("name", ["small_ra_slam_problem", "rplm_priors"])
def test_weights_and_statistics_against_the_reference(name, cost, couple):
    ctx, g, Q, dm, ref = built(name)
    ne = len(rr.edges(g))
    rng = np.random.default_rng(17)
    X = rng.standard_normal((dm.N, dm.d)) * 0.3
    r2 = ctx.debug_gnc_weights_host(X, np.full(ref.n_weights, INF), gr.NONE)["r2"]
    worst, mid = 0.0, 0
    for mu in MUS:
        c = _thresholds(r2, ne, cost, mu, couple, rng)
        got = ctx.debug_gnc_weights_host(X, c, cost, mu, couple)
        assert np.array_equal(got["r2"], r2)
        worst = max(worst, gr.check_weights(got["w"], r2, c, ne, cost, mu, couple, name))
        gr.check_statistics(got["stats_raw"], r2, c, got["w"], ne, couple, name)
        assert np.all(got["w"][np.isinf(c) & ~(couple & (np.arange(len(c)) < ne))] == 1.0)  # trusted
        assert np.all((got["w"] >= 0.0) & (got["w"] <= 1.0))
        if couple:
            assert np.array_equal(got["w"][:ne], got["w"][ne:2 * ne])
            st = got["stats"]["rot"]
            assert st["max_rho"] == 0.0 and st["n_mid"] == 0.0 and st["n_out"] == 0.0
        if cost == gr.NONE:
            assert np.all(got["w"] == 1.0)
        mid += int(sum(got["stats"][s]["n_mid"] for s in ("rot", "trans", "range")))
    assert cost == gr.NONE or mid > 0  # the middle band was exercised
    print("%s %s coupled=%d: worst |dw| / bound = %.3f" % (name, cost, couple, worst))
    # r2 = 0 everywhere: every ratio is 0 and every weight 1, whatever the cost
    zero = ctx.debug_gnc_weights_host(np.zeros((dm.N, 3)), np.full(ref.n_weights, 1e-6), cost, 1e-8, couple)
    assert np.all(zero["r2"] == 0.0) and np.all(zero["w"] == 1.0) and np.all(zero["stats_raw"] == 0.0)
    ctx.close()


def test_tls_exact_boundaries():
    """rho exactly mu / (mu + 1) is an inlier (w = 1), exactly (mu + 1) / mu an outlier (w = 0); one ulp inside either is
    in the middle band, within the bound of 1 and of 0."""
    ctx, g, Q, dm, ref = built("small_ra_slam_problem")
    ne, nw = len(rr.edges(g)), ref.n_weights
    X = np.random.default_rng(5).standard_normal((dm.N, 3))
    r2 = ctx.debug_gnc_weights_host(X, np.full(nw, INF), gr.NONE)["r2"]
    i, j = 2 * ne, 2 * ne + 1  # two ranges
    c = np.full(nw, INF)
    c[i], c[j] = 2.0 * r2[i], 0.5 * r2[j]
    got = ctx.debug_gnc_weights_host(X, c, gr.TLS, 1.0)
    assert got["w"][i] == 1.0 and got["w"][j] == 0.0
    c[i], c[j] = np.nextafter(c[i], 0.0), np.nextafter(c[j], INF)
    got = ctx.debug_gnc_weights_host(X, c, gr.TLS, 1.0)
    assert 1.0 - 16 * gr.EPS <= got["w"][i] <= 1.0 and 0.0 <= got["w"][j] <= 16 * gr.EPS
    gr.check_weights(got["w"], r2, c, ne, gr.TLS, 1.0, False, "boundaries")
    ctx.close()


def _raw(ctx, X, barc2, cost, mu, w=True, x=True, c=True):
    X = np.asfortranarray(X)
    out, st = np.zeros(max(len(barc2), 1)), np.zeros(12)
    dp = C.POINTER(C.c_double)
    return ctx.L.cora_debug_gnc_weights_host(ctx.h, X.ctypes.data_as(dp) if x else None, X.shape[0], X.shape[1],
                                             barc2.ctypes.data_as(dp) if c else None, int(cost), 0, C.c_double(mu),
                                             out.ctypes.data_as(dp) if w else None, None, st.ctypes.data_as(dp))


def test_refusals_leave_the_handle_answering_as_before():
    g, Q, dm, ref = ar.graph("small_ra_slam_problem")
    nw = ref.n_weights
    X = np.random.default_rng(9).standard_normal((dm.N, 3))
    ones = np.full(nw, 7.8)
    ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1)

    def refused(code, call):
        with pytest.raises(capi.CoraError) as e:
            call()
        assert e.value.code == code, str(e.value)

    assert _raw(ctx, X, ones, 1, 1.0) == ERR_NOT_READY  # no table
    ctx.set_measurements(*rr.table(g))
    assert _raw(ctx, X, ones, 1, 1.0) == ERR_NOT_READY  # no term map
    ctx.assembly_build(Q.rowptr, Q.col)
    w = ar.random_weights(nw, 4)
    vals = ctx.debug_assemble_values_host(w)
    res = ctx.debug_measurement_residuals_host(X)
    good = ctx.debug_gnc_weights_host(X, ones, "gm", 2.0)
    refused(ERR_SHAPE, lambda: ctx.debug_gnc_weights_host(np.zeros((dm.N, 25)), ones, "tls", 1.0))
    assert _raw(ctx, np.zeros((dm.N, 0)), ones, 1, 1.0) == ERR_SHAPE
    for missing in ("w", "x", "c"):
        assert _raw(ctx, X, ones, 1, 1.0, **{missing: False}) == ERR_ARG
    refused(ERR_ARG, lambda: ctx.debug_gnc_weights_host(X, ones, 3, 1.0))
    refused(ERR_ARG, lambda: ctx.debug_gnc_weights_host(X, ones, -1, 1.0))
    for mu in (0.0, -1.0, float("nan"), INF):
        for cost in ("tls", "gm"):
            refused(ERR_ARG, lambda: ctx.debug_gnc_weights_host(X, ones, cost, mu))
        ctx.debug_gnc_weights_host(X, ones, "none", mu)  # ignored by NONE
    for bad in (0.0, -1.0, float("nan"), -INF):
        c = ones.copy()
        c[nw // 2] = bad
        refused(ERR_ARG, lambda: ctx.debug_gnc_weights_host(X, c, "tls", 1.0))
    c = ones.copy()
    c[0] = -1.0  # a rot threshold: not read when the edges are coupled
    ctx.debug_gnc_weights_host(X, c, "tls", 1.0, True)
    for bad in (INF, float("nan")):
        Xb = X.copy()
        Xb[dm.N - 1, 0] = bad
        refused(ERR_NAN, lambda: ctx.debug_gnc_weights_host(Xb, ones, "tls", 1.0))
    refused(capi.CoraError(4, "").code, lambda: ctx.gnc_weights(X, ones, "tls", 1.0))  # plan-only: no device, no fall-back
    # nothing of the handle moved
    assert np.array_equal(vals, ctx.debug_assemble_values_host(w))
    again = ctx.debug_measurement_residuals_host(X)
    assert all(np.array_equal(res[k], again[k]) for k in res)
    after = ctx.debug_gnc_weights_host(X, ones, "gm", 2.0)
    assert all(np.array_equal(good[k], after[k]) for k in ("w", "r2", "stats_raw"))
    ctx.close()
    # a partitioned handle has no measurement table and is refused as such
    g2, Q2, dm2, ref2 = ar.graph("hub-d2")
    p = capi.Context(dm2.d, dm2.n, dm2.r, dm2.n_trans, Q2.rowptr, Q2.col, Q2.val, device=-1, rank=0, world=2)
    assert _raw(p, np.zeros((dm2.N, 2)), np.ones(ref2.n_weights), 1, 1.0) == ERR_ARG
    assert "partitioned" in p.L.cora_last_error(p.h).decode()
    p.close()


def test_problem_gnc_weights_without_a_live_handle_raises():
    P = host.Problem.from_pyfg(os.path.join(GOLDEN, "small_ra_slam_problem", "factor_graph.pyfg"))
    P.update()
    Y = np.zeros((P.variable_size(), P.dims()["d"]))
    with pytest.raises(host.HostError, match="no live device handle"):
        P.gnc_weights(Y, {"range": np.full(P.dims()["r"], 25.0)}, "tls", 1.0)
    with pytest.raises(host.HostError):
        P.gnc_weights(Y, {"nonsense": [1.0]}, "tls", 1.0)
