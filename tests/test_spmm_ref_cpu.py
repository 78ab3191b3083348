"""The entrywise bounds of tests/spmm_ref.py without a GPU: the fp64 C oracle and the format executed on the host
(cora_debug_format_spmm_host) meet them on every entry of every result, on the graded data the device is given in
tests/test_gpu_spmm_ref.py -- so the bounds are attainable by a correct fp64 evaluation, two of them, before the device
is held to them.  Then the gap they close: a row of Q X that loses its smallest term still passes the suite's norm-wise
1e-10 and is outside its own entry's bound.  Observed ratios: profiles/spmm_exact.md."""
import numpy as np
import pytest

import spmm_ref as sr
import topologies as topo
import topologies_worker as W
from oracle import oracle as orc
from test_update_values_cpu import plan

REL = 1e-10   # test_gpu_parity.REL

CASES = [(name, p) for name in sr.ENTRIES for p in sr.ranks(topo.CATALOGUE[name][1])]


@pytest.mark.parametrize("name,p", CASES, ids=["%s-p%d" % c for c in CASES])
def test_oracle_and_host_executor_meet_the_entrywise_bounds(name, p):
    R = sr.case(name, p)
    Q, dm, Y, X, V = R["Q"], R["dm"], R["Y"], R["X"], R["V"]
    worst = {}
    worst["QX oracle"] = sr.check("Q X (oracle)", orc.spmm(Q, X), *R["qx"])
    ctx = plan(Q, dm, Q.val)
    worst["QX host format"] = sr.check("Q X (host executor)", ctx.debug_format_spmm_host(X), *R["qx"])
    ctx.close()
    st, ob = orc.lambda_blocks(Q, dm, Y)
    worst["Lambda"] = max(sr.check("Lambda, Stiefel blocks", st, *R["lam_st"]), sr.check("Lambda, oblique", ob, *R["lam_ob"]))
    worst["SX"] = sr.check("(Q - Lambda) X", orc.S_apply(Q, dm, st, ob, X), *R["sx"])
    worst["Proj"] = sr.check("tangent projection", orc.tangent_proj(dm, Y, R["V0"]), *R["proj"])
    worst["Hvp"] = sr.check("Hvp", orc.hvp(Q, dm, Y, R["G"], V), *R["hv"])
    worst["f"] = sr.check("cost", orc.cost(Q, Y), *R["f"])
    print("\n%s p=%d: worst err / bound  %s" % (name, p, "  ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("name", ["robots-d3", "fat_landmark", "n65"])
def test_dropped_term_passes_the_normwise_bound_and_breaks_the_entrywise_one(name):
    """Over all rows and columns of Q X: the term that is the smallest of its row, more than 4 bounds of its entry and the
    smallest against the largest entry of the result.  Dropped (the row summed again in fp64), the norm-wise relerr of
    the suite accepts the result; sr.check refuses it."""
    p = 5
    R = sr.case(name, p)
    Q, dm, X = R["Q"], R["dm"], R["X"]
    ref, B, c = R["qx"]
    rows = np.repeat(np.arange(dm.N), np.diff(Q.rowptr))
    terms = Q.val[:, None] * X[Q.col]
    mag = np.where(terms != 0, np.abs(terms), np.inf)
    smallest = np.minimum.reduceat(mag, Q.rowptr[:-1], axis=0)            # N x p: each entry's smallest term
    bound = c[:, None] * sr.EPS * B
    eligible = np.where((smallest > 4 * bound) & np.isfinite(smallest), smallest, np.inf)
    row, col = np.unravel_index(np.argmin(eligible), eligible.shape)
    assert np.isfinite(eligible[row, col])
    seg = slice(Q.rowptr[row], Q.rowptr[row + 1])
    keep = mag[seg, col] != smallest[row, col]
    assert np.count_nonzero(~keep) == 1
    got = orc.spmm(Q, X)
    sr.check("Q X", got, ref, B, c)
    got[row, col] = np.sum(terms[seg, col][keep])
    old = W.relerr(got, np.asarray(ref, dtype=np.float64))
    print("\n%s: row %d (%d terms), dropped term %.3e of an entry %.3e with bound %.3e; largest entry %.3e: norm-wise "
          "error %.2e (bound %.0e)" % (name, row, seg.stop - seg.start, smallest[row, col], float(ref[row, col]),
                                       bound[row, col], float(np.abs(ref).max()), old, REL))
    assert 0 < old < REL
    with pytest.raises(AssertionError, match="outside their bound"):
        sr.check("Q X with a dropped term", got, ref, B, c)
