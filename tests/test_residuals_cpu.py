"""Per-measurement residuals without a GPU: the measurement table of a plan-only handle (device = -1), its row
translation into the internal order and its validation, through the host execution hook
(cora_debug_measurement_residuals_host), against the numpy reference of tests/residuals_ref.py."""
import os

import numpy as np
import pytest

import residuals_ref as rr
from conftest import EXPECTED_COST, GOLDEN
from cora_amd import capi
from mmio import read_dense
from oracle import assemble as asm
from oracle import oracle as orc
from synth import make_graph

ERR_NOT_READY, ERR_ARG = 2, 5


def _ctx(g, world=1):
    A = asm.assemble(g)
    Q = orc.CSR.from_scipy(A["Q"])
    dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
    return capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=-1, rank=0, world=world), dm


def _golden(case):
    g = asm.parse_pyfg(os.path.join(GOLDEN, case, "factor_graph.pyfg"))
    ctx, dm = _ctx(g)
    ctx.set_measurements(*rr.table(g))
    return g, ctx, dm


def _close(got, ref, rel):
    for key in ("edge_rot", "edge_trans", "range", "sums"):
        assert got[key].shape == ref[key].shape, key
        scale = max(np.abs(ref[key]).max(initial=0.0), 1e-300)
        assert np.abs(got[key] - ref[key]).max(initial=0.0) <= rel * scale, key


def test_golden_at_random_point(case):
    g, ctx, dm = _golden(case)
    assert ctx.measurement_counts() == (len(rr.edges(g)), len(g.ranges))
    X = read_dense(os.path.join(GOLDEN, case, "X_rand_dim2.mm"))
    got = ctx.debug_measurement_residuals_host(X)
    _close(got, rr.reference(g, X), 1e-12)
    cost = EXPECTED_COST[case]
    assert abs(0.5 * got["sums"].sum() - cost) < 1e-9 * max(1.0, abs(cost))


def test_golden_at_ground_truth(case):
    g, ctx, dm = _golden(case)
    X = read_dense(os.path.join(GOLDEN, case, "X_gt.mm"))
    got = ctx.debug_measurement_residuals_host(X)
    for key in ("edge_rot", "edge_trans", "range", "sums"):
        assert np.all(got[key] < 1e-12), key
        assert np.all(got[key] >= 0.0), key


@pytest.mark.parametrize("d", [2, 3])
def test_values_survive_the_row_permutation(d):
    g = make_graph(d=d, n=70, n_landmarks=3, n_ranges=100, n_loops=10)
    ctx, dm = _ctx(g)
    ctx.set_measurements(*rr.table(g))
    assert not np.array_equal(ctx.row_map(), np.arange(dm.N))  # the internal order IS a permutation here
    rng = np.random.default_rng(d)
    for k in (1, d, 5, 24):
        X = rng.standard_normal((dm.N, k))
        _close(ctx.debug_measurement_residuals_host(X), rr.reference(g, X), 1e-12)


def test_second_call_replaces_the_table():
    g = make_graph(d=2, n=70, n_landmarks=3, n_ranges=100, n_loops=10)
    ctx, dm = _ctx(g)
    er, ed, rg, rd = rr.table(g)
    ctx.set_measurements(er, ed, rg, rd)
    X = np.random.default_rng(0).standard_normal((dm.N, 3))
    full = ctx.debug_measurement_residuals_host(X)
    ctx.set_measurements(er[17:18], ed[17:18], rg[41:42], rd[41:42])
    assert ctx.measurement_counts() == (1, 1)
    one = ctx.debug_measurement_residuals_host(X)
    assert one["edge_rot"][0] == full["edge_rot"][17] and one["edge_trans"][0] == full["edge_trans"][17]
    assert one["range"][0] == full["range"][41]
    ctx.set_measurements(er[:0], ed[:0], rg[:0], rd[:0])  # an empty table is a table
    assert ctx.measurement_counts() == (0, 0)
    assert np.all(ctx.debug_measurement_residuals_host(X)["sums"] == 0.0)


def test_error_paths():
    g = make_graph(d=3, n=70, n_landmarks=3, n_ranges=100, n_loops=10)
    ctx, dm = _ctx(g)
    X = np.zeros((dm.N, 3))
    with pytest.raises(capi.CoraError) as e:
        ctx.debug_measurement_residuals_host(X)
    assert e.value.code == ERR_NOT_READY
    with pytest.raises(capi.CoraError) as e:
        ctx.measurement_residuals(X)
    assert e.value.code == ERR_NOT_READY
    er, ed, rg, rd = rr.table(g)

    def refused(er_=er, ed_=ed, rg_=rg, rd_=rd, on=ctx):
        with pytest.raises(capi.CoraError) as err:
            on.set_measurements(er_, ed_, rg_, rd_)
        assert err.value.code == ERR_ARG, err.value
        assert on.measurement_counts() == (0, 0)  # a refused call installs nothing

    bad = er.copy()
    bad[5, 0] += 1  # a rotation row that is not a multiple of d
    refused(er_=bad)
    bad = er.copy()
    bad[5, 1] = dm.dn  # ... or not below d * n
    refused(er_=bad)
    bad = er.copy()
    bad[7, 3] = dm.dn + 2  # a translation row inside the range block
    refused(er_=bad)
    bad = rg.copy()
    bad[3, 2] = dm.dn + 1
    refused(rg_=bad)
    bad = rg.copy()
    bad[3, 0] = dm.dn + dm.r  # a range row outside the range block
    refused(rg_=bad)
    bad = ed.copy()
    bad[11, -1] = np.nan  # a NaN precision
    refused(ed_=bad)
    bad = rd.copy()
    bad[0, 1] = np.inf
    refused(rd_=bad)
    part, _ = _ctx(g, world=2)  # partitioned handles are refused for now
    refused(on=part)
    ctx.set_measurements(er, ed, rg, rd)
    with pytest.raises(capi.CoraError) as e:  # the device pass needs a device: no CPU fallback
        ctx.measurement_residuals(X)
    assert e.value.code == 4
    with pytest.raises(capi.CoraError):
        ctx.debug_measurement_residuals_host(np.zeros((dm.N, 25)))


def test_set_stream_needs_a_device():
    """cora_set_stream on a plan-only handle: CORA_ERR_HIP, for a stream and for stream 0, and the handle stays usable."""
    g = make_graph(d=2, n=12, n_landmarks=2, n_ranges=6, n_loops=1)
    ctx, dm = _ctx(g)
    for stream in (0, 0x1000):
        with pytest.raises(capi.CoraError) as e:
            ctx.set_stream(stream)
        assert e.value.code == 4
    ctx.set_measurements(*rr.table(g))
    assert ctx.measurement_counts() == (len(rr.edges(g)), len(g.ranges))
