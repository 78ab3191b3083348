"""The catalogue of tests/topologies.py without a GPU: every entry has the shape it declares (cora_debug_format_shape), the
format executed on the host (cora_debug_format_spmm_host) reproduces the oracle's Q X on one handle and on 2 and 3
partitions with distributed and with whole long rows, the partitions own every row once, new values land where a fresh
handle puts them (bit for bit), the C++ host assembles the same data matrix from the same measurements, and the whole
catalogue again with every pose slice in the plain layout (CORA_CHAIN_SLICES=0, a child process).

Bound of the products: 1e-12 of the largest entry (test_format_cpu.test_format_on_fixtures); observed 1.6e-15 at worst
(profiles/topologies.md).  What the DEVICE makes of the same formats is tests/test_gpu_topologies.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import topologies as topo
from oracle import oracle as orc
from test_update_values_cpu import pair_factors, plan, products, roundtrip, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-12
KS = (1, 5, 10)
PARTS = [(1, False), (2, False), (2, True), (3, False), (3, True)]   # world, whole_long_rows


def relerr(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


@pytest.mark.parametrize("name", topo.NAMES)
def test_declared_shape(name):
    A, Q, dm, g = topo.build(name)
    ctx = plan(Q, dm, Q.val)
    got = topo.check_shape(name, ctx)
    print("\n%s: N=%d nnz=%d %s" % (name, dm.N, Q.nnz, got))
    assert got["chain_slices"] + got["plain_slices"] == (dm.n + 63) // 64
    ctx.close()


@pytest.mark.parametrize("world,whole", PARTS)
@pytest.mark.parametrize("name", topo.NAMES)
def test_host_executed_format_and_partition(name, world, whole):
    """Q X of the format against the oracle at 1, 5 and 10 columns, put together from the ranks as
    test_format_cpu.test_partition_covers_all_rows does: a rank writes its own rows and its partial sums of the
    distributed long rows, nothing else; every row has one owner; the local non-zeros add up to nnz(Q)."""
    A, Q, dm, g = topo.build(name)
    rowlen = np.diff(Q.rowptr)
    tb = dm.dn + dm.r
    want_long = np.zeros(dm.N, dtype=bool)
    if world > 1 and not whole:
        want_long[tb:] = rowlen[tb:] > topo.K_LONG_ROW   # pose rows and landmark rows alike
    Xs = {k: np.random.default_rng(k).standard_normal((dm.N, k)) for k in KS}
    refs = {k: orc.spmm(Q, Xs[k]) for k in KS}
    totals = {k: np.zeros_like(refs[k]) for k in KS}
    owned = np.zeros(dm.N, dtype=int)
    maps, nnz, remote_pairs = [], 0, 0
    for rank in range(world):
        ctx = plan(Q, dm, Q.val, rank=rank, world=world, whole=whole)
        m = ctx.row_map()
        maps.append(m)
        mine = (m >= ctx.shard_begin) & (m < ctx.shard_begin + ctx.shard_rows)
        owned += mine
        is_long = np.zeros(dm.N, dtype=bool)
        is_long[ctx.long_rows()] = True
        assert np.array_equal(is_long, want_long)
        for k in KS:
            got = ctx.debug_format_spmm_host(Xs[k])
            totals[k][mine & ~is_long] = got[mine & ~is_long]
            totals[k][is_long] += got[is_long]
            assert np.abs(got[~mine & ~is_long]).max(initial=0) == 0.0
        assert ctx.rows == world * ctx.shard_rows
        nnz += ctx.format_stats()["local_nnz"]
        rot = m[:dm.dn].reshape(dm.n, dm.d)
        assert np.all(np.diff(rot, axis=1) == 1)   # a pose's rotation rows stay together on one rank
        remote_pairs += ctx.format_shape()["remote_tail_pairs"]
        ctx.close()
    assert np.all(owned == 1)
    for m in maps[1:]:
        assert np.array_equal(m, maps[0])
    assert len(set(maps[0].tolist())) == dm.N
    assert nnz == Q.nnz
    if world == 1:
        assert remote_pairs == 0
    worst = max(relerr(totals[k], refs[k]) for k in KS)
    print("\n%s world %d whole %s: worst %.2e, %d remote tail pairs" % (name, world, whole, worst, remote_pairs))
    assert worst < BOUND


@pytest.mark.parametrize("world,whole", PARTS)
@pytest.mark.parametrize("name", topo.NAMES)
def test_update_values_roundtrip(name, world, whole):
    """test_update_values_cpu.roundtrip on every rank; a rank that owns no row (n1, n2 at world 3) has nothing that
    could differ: its products are all zero before and after."""
    A, Q, dm, g = topo.build(name)
    vals1 = np.array(Q.val, dtype=np.float64)
    vals2 = vals1 * pair_factors(Q.rowptr, Q.col)
    for rank in range(world):
        kw = dict(rank=rank, world=world, whole=whole)
        probe = plan(Q, dm, vals1, **kw)
        empty = probe.format_stats()["local_nnz"] == 0
        if empty:
            assert world > 1 and dm.n < world
            zero = products(probe, dm)
            assert all(not np.any(z) for z in zero)
            probe.update_values(Q.rowptr, Q.col, vals2)
            assert same(products(probe, dm), zero)
        probe.close()
        if not empty:
            roundtrip(Q, dm, vals1, vals2, **kw)


@pytest.mark.parametrize("name", [n for n in topo.NAMES if n not in ("dups", "fat_landmark")])
def test_host_problem_assembles_the_same_matrix(name):
    """The graph through host.Problem.new + add_* (what the sharded GPU tests build their ranks from).  dups and
    fat_landmark repeat measurements, which CORA::Problem refuses (next test): they reach the library as matrices."""
    A, Q, dm, g = topo.build(name)
    P = topo.to_problem(name)
    d = P.dims()
    assert (d["d"], d["n"], d["l"], d["r"], d["N"]) == (A["d"], A["n"], A["l"], A["r"], A["N"])
    got = P.scipy_matrix("DataMatrix")
    assert got.shape == A["Q"].shape
    assert abs(got - A["Q"]).max() <= 1e-12 * abs(A["Q"]).max()
    P.close()


@pytest.mark.parametrize("name", ["dups", "fat_landmark"])
def test_host_problem_refuses_repeated_measurements(name):
    from cora_amd import host
    assert topo.has_duplicates(name)
    g = topo.build(name)[3]
    P = host.Problem.new(g.dim)
    a, b, dist, cov = g.ranges[0]
    P.add_pose(a)
    (P.add_landmark if b in g.landmarks else P.add_pose)(b)
    P.add_range(a, b, dist, cov)
    with pytest.raises(host.HostError, match="already exists"):
        P.add_range(a, b, dist, cov)
    assert not any(topo.has_duplicates(n) for n in topo.NAMES if n not in ("dups", "fat_landmark"))


_PLAIN = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import topologies as topo
from oracle import oracle as orc
from test_update_values_cpu import plan
worst = 0.0
for name in topo.NAMES:
    A, Q, dm, g = topo.build(name)
    ctx = plan(Q, dm, Q.val)
    s = ctx.format_shape()
    assert s["chain_slices"] == 0 and s["plain_slices"] == (dm.n + 63) // 64, (name, s)
    for k in (1, 5, 10):
        X = np.random.default_rng(k).standard_normal((dm.N, k))
        ref = orc.spmm(Q, X)
        err = np.abs(ctx.debug_format_spmm_host(X) - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err < %r, (name, k, err)
    ctx.close()
print("plain layout ok: worst %%.2e" %% worst)
"""


def test_plain_layout_in_a_child_process():
    """CORA_CHAIN_SLICES=0 is read when the library is loaded: the whole catalogue with every pose slice in the plain
    layout (every pose's translation row in the row slices or on the chunk path)."""
    env = dict(os.environ, CORA_CHAIN_SLICES="0")
    r = subprocess.run([sys.executable, "-c", _PLAIN % (ROOT, os.path.join(ROOT, "tests"), BOUND)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    print(out[-500:])
    assert r.returncode == 0 and "plain layout ok" in out, out[-4000:]


@pytest.mark.parametrize("name", topo.NAMES)
def test_reference_takes_two_interior_steps(name):
    """The kappa check of tests/test_gpu_topologies.py compares the device STPCG after 1 and 2 iterations with
    tests/stpcg_ref.py: at the points it uses (topologies.near_truth) the reference's own curvature is positive with a
    margin at every stride, so the step is the interior one and a wrong kappa shows in s and r."""
    import topologies_worker as W
    d = topo.CATALOGUE[name][1]
    for p in W.strides(d):
        if p <= W.KAPPA_MAX_P:
            R = W.references(name, p)
            assert W.interior(R) is None, (name, p, W.interior(R))
            print("%s p=%d kappa_rel %s" % (name, p, ["%.2e" % s["kappa_rel"] for s in R["states"]]))
