"""The exact integer reference of tests/spmm_exact.py is right before a GPU sees it, on every entry of the catalogue
(tests/topologies.py): the integer matrix keeps the format shape the entry declares; the format executed on the host
(cora_debug_format_spmm_host) returns the exact Q X bit for bit at 1, 5 and 10 columns, on one handle and on the partitions
of test_topologies_cpu.PARTS; the fp64 C oracle returns the exact Q X, Lambda blocks, S X, tangent projection, Hessian-
vector product and cost bit for bit at p = d and at one wide p; every case tests/test_gpu_spmm_exact.py runs has its
magnitude certificate below 2^52 (the condition under which that equality is a theorem).

The mutation check records the gap this closes: a row of Q X that drops, negates or repeats its smallest term passes
the suite's norm-wise bound (1e-10 of the largest entry of the result) and fails the exact comparison.  It mutates a copy
of the row's terms on the CPU, never device code.  Figures: profiles/spmm_exact.md."""
import math

import numpy as np
import pytest

import long_rows_graphs as lrg
import spmm_exact as sx
import topologies as topo
import topologies_worker as W
from oracle import oracle as orc
from test_topologies_cpu import KS, PARTS
from test_update_values_cpu import plan

WIDE_P = 9
REL = 1e-10   # test_gpu_parity.REL, the bound whose slack the mutation check measures


def _log2(x):
    return math.log2(max(x, 1.0))


@pytest.mark.parametrize("name", topo.NAMES)
def test_declared_shape(name):
    A, Q, dm, g = topo.build(name)
    Qi = sx.case(Q, dm, name, dm.d, op="qx")["Qi"]
    assert np.array_equal(Qi.rowptr, Q.rowptr) and np.array_equal(Qi.col, Q.col)
    assert np.array_equal(Qi.to_scipy().toarray(), Qi.to_scipy().toarray().T)
    ctx = plan(Qi, dm, Qi.val)
    topo.check_shape(name, ctx)
    ctx.close()


@pytest.mark.parametrize("world,whole", PARTS)
@pytest.mark.parametrize("name", topo.NAMES)
def test_host_executor_is_exact(name, world, whole):
    """As test_topologies_cpu.test_host_executed_format_and_partition puts the ranks together (a rank writes its rows and
    its partial sums of the distributed long rows: sums of integers, exact as well), with array_equal for the bound."""
    A, Q, dm, g = topo.build(name)
    cases = {k: sx.case(Q, dm, name, dm.d, k=k, op="qx") for k in KS}
    totals = {k: np.zeros_like(cases[k]["qx"]) for k in KS}
    for rank in range(world):
        ctx = plan(cases[KS[0]]["Qi"], dm, cases[KS[0]]["Qi"].val, rank=rank, world=world, whole=whole)
        m = ctx.row_map()
        mine = (m >= ctx.shard_begin) & (m < ctx.shard_begin + ctx.shard_rows)
        is_long = np.zeros(dm.N, dtype=bool)
        is_long[ctx.long_rows()] = True
        for k in KS:
            R = cases[k]
            assert R["cert"]["qx"] < sx.LIMIT
            assert np.array_equal(R["Qi"].val, cases[KS[0]]["Qi"].val)   # one matrix for every column count
            got = ctx.debug_format_spmm_host(R["X"])
            totals[k][mine & ~is_long] = got[mine & ~is_long]
            totals[k][is_long] += got[is_long]
        ctx.close()
    for k in KS:
        assert np.array_equal(totals[k], cases[k]["qx"]), (name, k)


def _oracle_equals_exact(Q, dm, key, p):
    Rq = sx.case(Q, dm, key, p, op="qx")
    R = sx.case(Q, dm, key, p, op="point")
    Gc = sx.gradient_case(Q, dm, key, p)
    for what, c in list(R["cert"].items()) + [("QX", Rq["cert"]["qx"])] + [("stpcg." + k, v) for k, v in Gc["cert"].items()]:
        assert c < sx.LIMIT, (key, p, what, c)
    Qi, Y = R["Qi"], R["Y"]
    assert np.array_equal(orc.spmm(Rq["Qi"], Rq["X"]), Rq["qx"])
    assert np.array_equal(orc.spmm(Rq["Qi"], Rq["X"], rowwise=True), Rq["qx"])
    assert np.array_equal(orc.egrad(Qi, Y), R["G"])
    st, ob = orc.lambda_blocks(Qi, dm, Y)
    assert np.array_equal(st, R["st"]) and np.array_equal(ob, R["ob"])
    assert np.array_equal(orc.S_apply(Qi, dm, st, ob, R["Xp"]), R["sx"])
    W0 = sx.integer_block(dm.N, p, np.random.default_rng(p), sx.GRADES["point"][1])
    w2, c = R["E"].tangent_proj2(R["Yi"], W0)
    assert c < sx.LIMIT and np.array_equal(orc.tangent_proj(dm, Y, sx.f64(W0)), sx.f64(w2, 1))
    assert np.array_equal(orc.tangent_proj(dm, Y, R["V"]), R["V"])   # V is a tangent vector
    assert np.array_equal(orc.hvp(Qi, dm, Y, R["G"], R["V"]), R["hv"])
    assert orc.cost(Qi, Y) == R["f"]
    assert np.array_equal(orc.hvp(Gc["Qi"], dm, Gc["Y"], Gc["G"], Gc["g"]), Gc["hg"])
    assert orc.inner(Gc["g"], Gc["g"]) == Gc["rr"] and orc.inner(Gc["g"], Gc["hg"]) == Gc["kappa"] > 0


@pytest.mark.parametrize("name", topo.NAMES)
def test_oracle_is_exact(name):
    A, Q, dm, g = topo.build(name)
    for p in (dm.d, WIDE_P):
        _oracle_equals_exact(Q, dm, name, p)


def test_oracle_is_exact_on_the_long_row_graphs():
    for name in lrg.NAMES:
        A, Q, dm = lrg.build(name)
        _oracle_equals_exact(Q, dm, "long-" + name, 5)


def test_certificates_of_every_device_case():
    """Every case of tests/test_gpu_spmm_exact.py (spmm_exact.device_cases), below 2^52; the largest per operator is
    printed for profiles/spmm_exact.md."""
    worst = {}
    count = 0
    for key, Q, dm, p, k, op in sx.device_cases():
        R = sx.gradient_case(Q, dm, key, p) if op == "gradient" else sx.case(Q, dm, key, p, k=k, op=op)
        count += 1
        for what, c in R["cert"].items():
            tag = "%s.%s" % (op, what)
            assert c < sx.LIMIT, (key, p, k, tag, c)
            if c > worst.get(tag, (0, None))[0]:
                worst[tag] = (c, "%s p=%d k=%d" % (key, p, k))
    print("\n%d cases; largest certificates:" % count)
    for tag, (c, where) in sorted(worst.items()):
        print("  %-16s 2^%.1f  (%s)" % (tag, _log2(c), where))
    assert count > 300


MUTATIONS = {"drop": 0.0, "negate": -1.0, "duplicate": 2.0}


@pytest.mark.parametrize("how", list(MUTATIONS))
@pytest.mark.parametrize("name", ["robots-d3", "fat_landmark", "n65"])
def test_mutation_passes_the_normwise_bound_and_fails_the_exact_one(name, how):
    """The row of Q X whose smallest non-zero term is the smallest of all rows, that term dropped, negated or counted
    twice, the row summed again in fp64 (exact either way: the certificate covers twice the term): the norm-wise relerr
    of the suite accepts the result, array_equal does not."""
    A, Q, dm, g = topo.build(name)
    R = sx.case(Q, dm, name, 5, op="qx")
    Qi, X, ref = R["Qi"], R["X"], R["qx"]
    assert 2 * R["cert"]["qx"] < 2.0 ** 53
    rows = np.repeat(np.arange(dm.N), np.diff(Qi.rowptr))
    terms = Qi.val[:, None] * X[Qi.col]                      # nnz x k, every one an exact product
    mag = np.where(terms != 0, np.abs(terms), np.inf)
    q, c = np.unravel_index(np.argmin(mag), mag.shape)
    row = rows[q]
    mutated = terms[Qi.rowptr[row]:Qi.rowptr[row + 1], c].copy()
    mutated[q - Qi.rowptr[row]] *= MUTATIONS[how]
    got = ref.copy()
    assert got[row, c] == np.sum(terms[Qi.rowptr[row]:Qi.rowptr[row + 1], c])
    got[row, c] = np.sum(mutated)
    old = W.relerr(got, ref)
    print("\n%s %s: row %d of %d terms, term %g, entry %g, largest entry %g: norm-wise error %.2e (bound %.0e)" % (
        name, how, row, len(mutated), terms[q, c], ref[row, c], np.abs(ref).max(), old, REL))
    assert 0 < old < REL
    assert not np.array_equal(got, ref)
