"""New values of Q on a live handle, without a GPU: a plan-only handle (device = -1) updated in place through the source
map against a handle freshly created from the same values, executed on the host (cora_debug_format_spmm_host).  The same
values land in the same slots, so every comparison is bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cora_amd import capi
from synth import make_problem

ERR_ARG = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 3, 8)


def pair_factors(rowptr, col, seed=7, zero_every=11):
    """A factor per entry (i, j) that depends on the unordered pair {i, j} only (so Q stays bitwise symmetric): 1 + half a
    64-bit hash of (min, max) / 2^64, and exactly 0 for every zero_every-th off-diagonal pair."""
    rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.uint64), np.diff(rowptr))
    c = col.astype(np.uint64)
    lo, hi = np.minimum(rows, c), np.maximum(rows, c)
    with np.errstate(over="ignore"):
        h = lo * np.uint64(0x9E3779B97F4A7C15) + hi * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(seed)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    f = 1.0 + 0.5 * (h.astype(np.float64) / 2.0 ** 64)
    f[(h % np.uint64(zero_every) == 0) & (lo != hi)] = 0.0
    return f


def graph(d, seed=3):
    """The graph of tests/test_gpu_lambda_fold.py: ragged last pose slice (head values), loop closures (general slots),
    several ranges per pose (tails), landmark rows above kLongRow (long-row chunks)."""
    A, Q, dm = make_problem(d=d, n=333, n_landmarks=3, n_ranges=500, n_loops=7, seed=seed)
    vals1 = np.array(Q.val, dtype=np.float64)
    vals2 = vals1 * pair_factors(Q.rowptr, Q.col)
    assert np.count_nonzero(vals2 == 0.0) > np.count_nonzero(vals1 == 0.0)
    return Q, dm, vals1, vals2


def plan(Q, dm, vals, rank=0, world=1, whole=False):
    return capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, vals, device=-1, rank=rank, world=world,
                        whole_long_rows=whole)


def products(ctx, dm):
    rng = np.random.default_rng(5)
    return [ctx.debug_format_spmm_host(rng.standard_normal((dm.N, k))) for k in KS]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def roundtrip(Q, dm, vals1, vals2, **kw):
    a, b = plan(Q, dm, vals1, **kw), plan(Q, dm, vals2, **kw)
    first, fresh = products(a, dm), products(b, dm)
    assert not same(first, fresh)
    a.update_values(Q.rowptr, Q.col, vals2)
    assert same(products(a, dm), fresh)
    a.update_values(Q.rowptr, Q.col, vals1)  # (the map of the first call, the pattern checked by its hash)
    assert same(products(a, dm), first)
    a.close()
    b.close()


@pytest.mark.parametrize("d", [2, 3])
def test_update_matches_fresh_handle(d):
    roundtrip(*graph(d))


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("d", [2, 3])
def test_partitioned_plans(d, whole):
    Q, dm, vals1, vals2 = graph(d)
    for rank in range(3):
        roundtrip(Q, dm, vals1, vals2, rank=rank, world=3, whole=whole)


def test_map_built_ahead():
    Q, dm, vals1, vals2 = graph(3)
    a, b = plan(Q, dm, vals1), plan(Q, dm, vals2)
    a.values_map_build(Q.rowptr, Q.col)
    a.update_values(Q.rowptr, Q.col, vals2)
    assert same(products(a, dm), products(b, dm))


_PLAIN = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_update_values_cpu as t
Q, dm, vals1, vals2 = t.graph(3)
t.roundtrip(Q, dm, vals1, vals2)
t.roundtrip(Q, dm, vals1, vals2, rank=1, world=3)
print("plain layout ok")
"""


def test_plain_layout_in_a_child_process():
    """CORA_CHAIN_SLICES=0 is read when the library is loaded: every pose slice in the plain layout."""
    env = dict(os.environ, CORA_CHAIN_SLICES="0")
    r = subprocess.run([sys.executable, "-c", _PLAIN % (ROOT, os.path.join(ROOT, "tests"))], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"plain layout ok" in r.stdout, r.stdout.decode(errors="replace")


def _mirror_entry(Q, dm):
    """CSR position of Q(t_P, rot(P)_0) of pose 5: the chain layout reads it from Q(rot(P)_0, t_P)."""
    row, c = dm.d * dm.n + dm.r + 5, dm.d * 5
    q = np.arange(Q.rowptr[row], Q.rowptr[row + 1])
    q = q[Q.col[q] == c]
    assert len(q) == 1
    return int(q[0])


def test_rejected_updates_leave_the_handle_alone():
    Q, dm, vals1, vals2 = graph(3)
    a = plan(Q, dm, vals1)
    first = products(a, dm)
    rowptr, col = np.array(Q.rowptr, dtype=np.int32), np.array(Q.col, dtype=np.int32)

    def refused(rp, ci, v):
        with pytest.raises(capi.CoraError) as e:
            a.update_values(rp, ci, v)
        assert e.value.code == ERR_ARG, str(e.value)
        assert same(products(a, dm), first)

    def cases():
        moved = col.copy()  # a changed column index (still sorted, still in range: row 0 gets a column it did not have)
        row0 = set(col[rowptr[0]:rowptr[1]].tolist())
        moved[rowptr[1] - 1] = next(c for c in range(dm.N - 1, 0, -1) if c not in row0)
        yield rowptr, moved, vals2
        short = rowptr.copy()  # a different nnz
        short[-1] -= 1
        yield short, col[:-1], vals2[:-1]
        ulp = vals2.copy()  # one of a mirror pair changed by an ulp
        q = _mirror_entry(Q, dm)
        assert ulp[q] != 0.0
        ulp[q] = np.nextafter(ulp[q], np.inf)
        yield rowptr, col, ulp
        nan = vals2.copy()
        nan[len(nan) // 2] = np.nan
        yield rowptr, col, nan

    for when in ("before the map exists", "with the map"):
        for rp, ci, v in cases():
            refused(rp, ci, v)
        a.update_values(rowptr, col, vals1)
        assert same(products(a, dm), first), when


def test_duplicate_columns_are_refused():
    """Creation sums repeated entries of a row; the update has no source map for them (include/cora_hip.h)."""
    Q, dm, vals1, _ = graph(2)
    rowptr, col = np.array(Q.rowptr, dtype=np.int32), np.array(Q.col, dtype=np.int32)
    at = int(rowptr[1])  # repeat the last entry of row 0
    rp = rowptr.copy()
    rp[1:] += 1
    ci = np.insert(col, at, col[at - 1])
    v = np.insert(vals1, at, 0.25)
    a = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, rp, ci, v, device=-1)
    with pytest.raises(capi.CoraError) as e:
        a.update_values(rp, ci, v)
    assert e.value.code == ERR_ARG


# ---- CORA::Problem without a GPU: the weighted assembly ---------------------------------------------------------------

def _problem(case):
    from conftest import GOLDEN
    from cora_amd import host
    from oracle import assemble as asm
    path = os.path.join(GOLDEN, case, "factor_graph.pyfg")
    P = host.Problem.from_pyfg(path)
    P.update()
    return P, asm.parse_pyfg(path), host


def _random_weights(P, rng):
    """Every kind the problem has, about a fifth of the weights exactly 0."""
    w = {}
    for kind, ones in P.get_measurement_weights().items():
        assert np.all(ones == 1.0)
        if len(ones):
            w[kind] = rng.uniform(0.25, 2.0, len(ones)) * (rng.uniform(size=len(ones)) > 0.2)
    return w


def test_problem_unit_weights_are_bit_identical(case):
    P, g, host = _problem(case)
    before = P.matrix("DataMatrix")
    P.set_measurement_weights({k: v for k, v in P.get_measurement_weights().items() if len(v)})
    after = P.matrix("DataMatrix")
    for a, b in zip(before[2:], after[2:]):
        assert np.array_equal(a, b)
    assert np.array_equal(before[4].view(np.int64), after[4].view(np.int64))


def test_problem_weighted_cost_and_pattern(case):
    import residuals_ref as rr
    P, g, host = _problem(case)
    unit = P.matrix("DataMatrix")
    rng = np.random.default_rng(17)
    w = _random_weights(P, rng)
    assert any(np.any(v == 0.0) for v in w.values()) or sum(len(v) for v in w.values()) < 4
    P.set_measurement_weights(w)
    got = P.get_measurement_weights()
    for kind, v in w.items():
        assert np.array_equal(got[kind], v)
    weighted = P.matrix("DataMatrix")
    assert np.array_equal(unit[2], weighted[2]) and np.array_equal(unit[3], weighted[3])  # zero weights keep the pattern
    Q = P.scipy_matrix("DataMatrix")
    X = rng.standard_normal((Q.shape[0], 4))
    f = 0.5 * float(np.sum(X * (Q @ X)))
    ref = rr.by_kind(rr.reference(g, X))  # residuals are linear in kappa, tau and omega: scaled by the weights
    total = sum(float(np.sum(ref[kind] * w.get(kind, 1.0))) for kind in host.Problem.WEIGHT_KINDS)
    assert abs(0.5 * total - f) <= 1e-9 * max(1.0, abs(f))
    P.set_measurement_weights({})  # back to ones: the unweighted matrix, bit for bit
    assert np.array_equal(P.matrix("DataMatrix")[4].view(np.int64), unit[4].view(np.int64))


def test_problem_bad_weights_raise():
    P, g, host = _problem("small_ra_slam_problem")
    unit = P.matrix("DataMatrix")
    n = len(P.get_measurement_weights()["range"])
    assert n > 1
    for bad in ({"range": np.ones(n + 1)}, {"range": np.ones(n - 1)}, {"range": -np.ones(n)},
                {"range": np.full(n, np.nan)}, {"range": np.full(n, np.inf)}):
        with pytest.raises(host.HostError):
            P.set_measurement_weights(bad)
    with pytest.raises(host.HostError):
        P.set_measurement_weights({"ranges": np.ones(n)})
    assert np.array_equal(P.matrix("DataMatrix")[4], unit[4])
