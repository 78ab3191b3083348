"""The product kernels (k_spmm and the long-row chunks, cora_amd/csrc/kernels/spmm.inc) against the EXACT result.

tests/spmm_exact.py replaces the values of every catalogue matrix (tests/topologies.py) by symmetric integers on the
unchanged pattern and takes an integer point, integer vectors and an integer tangent gradient; Q X, the Lambda blocks,
(Q - Lambda) X, the Hessian-vector product and the cost are then sums of products of integers and of halves, every partial
sum of every order a double (its magnitude certificate, asserted here for every case, is below 2^52).  A correct device
product therefore returns the integer reference BIT FOR BIT: a term that is dropped, repeated, read from the wrong slot or
given the wrong sign shows even where it is 2^-44 of the largest entry -- under the norm-wise 1e-10 of the other product
tests it does not (tests/test_spmm_exact_cpu.py, the mutation check).  Nothing here compares the device with another
fp64 run: the reference is integer arithmetic.

Every entry, in both forms of the pose slices, at p = d and the strides of topologies_worker.WIDE_STRIDES; one interior
iteration of the device STPCG (p <= KAPPA_MAX_P), whose Hp is exact and whose step s = alpha p is the one division of the
whole file; then the forced stagger, update_values, the long-row graphs and partitioned handles.  After a library error
(a HIP error among them) every further test of the module fails without touching the device."""
import functools

import numpy as np
import pytest

import long_rows_graphs as lrg
import spmm_exact as sx
import topologies as topo
import topologies_worker as W
from cora_amd import capi

pytestmark = pytest.mark.gpu

_STATE = {"fatal": None}


@pytest.fixture(autouse=True)
def device_in_order():
    if _STATE["fatal"]:
        pytest.fail(_STATE["fatal"])


def _guard(fn):
    """A library error (a HIP error among them) ends the module's use of the device."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        try:
            return fn(*a, **kw)
        except capi.CoraError as e:
            _STATE["fatal"] = "an earlier test ended with a library error: %s" % e
            raise
    return wrapped


@pytest.fixture
def switches():
    """The form of the pose slices and the stagger gate, put back afterwards."""
    L = capi.load()
    win = L.cora_debug_spmm_window_min_slices(0)
    L.cora_debug_spmm_window_min_slices(win)
    force = L.cora_debug_spmm_stagger_force(-1)
    ticks = L.cora_debug_spmm_stagger_ticks(-1)
    yield L
    L.cora_debug_spmm_stagger_ticks(ticks)
    L.cora_debug_spmm_stagger_force(force)
    L.cora_debug_spmm_window_min_slices(win)


def _certified(R, tag):
    for what, c in R["cert"].items():
        assert c < sx.LIMIT, (tag, what, c)


def _exact(tag, what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        diff = np.abs(got - want)
        raise AssertionError("%s: %s is not exact: %d of %d entries differ, first at %s (got %r, exact %r), largest "
                             "difference %g where the largest entry is %g" % (
                                 tag, what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])],
                                 np.nanmax(diff), np.abs(want).max()))


def _context(Qi, dm, p, **kw):
    c = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Qi.rowptr, Qi.col, Qi.val, **kw)
    c.set_rank(p)
    return c


def _check_qx(tag, c, R):
    _certified(R, tag)
    _exact(tag, "Q X at %d columns" % R["X"].shape[1], c.dataMatrixProduct(R["X"]), R["qx"])


def _check_point(tag, c, R, p):
    """Every operator at the point on handle c (of R["Qi"])."""
    _certified(R, tag)
    _exact(tag, "Q X (point's matrix)", c.dataMatrixProduct(R["X"]), R["qx"])
    st, ob = c.compute_Lambda_blocks(R["Y"])
    _exact(tag, "Lambda, Stiefel blocks", st, R["st"])
    _exact(tag, "Lambda, oblique entries", ob, R["ob"])
    c.set_point(R["Y"])
    assert c.point_cost() == R["f"], (tag, "point_cost", c.point_cost(), R["f"])
    _exact(tag, "(Q - Lambda) X", c.certificate_product(R["Xp"]), R["sx"])
    _exact(tag, "Hvp, host pointers", c.Riemannian_Hessian_vector_product(R["Y"], R["G"], R["V"]), R["hv"])
    c.set_point(R["Y"])   # (the Hvp with a gradient from outside leaves its own Lambda on the handle)
    x, o = c.dev_alloc(p), c.dev_alloc(p)
    c.upload(R["V"], x)
    c.hvp_dev(x, o)
    _exact(tag, "hvp_dev", c.download(o, p), R["hv"])
    c.dev_free(x)
    c.dev_free(o)


def _check_stpcg(tag, c, R, p):
    """One iteration of the device STPCG without a preconditioner from the integer tangent gradient g: p_0 = -g,
    Hp = H p_0 = -(H g) exactly (EPI_HVP_K writes it), kappa = <p_0, Hp> = <g, H g> and <r, r> = <g, g> are sums of
    integers and quarters below 2^52 (certificates `kappa`, `rr`): the device holds them exactly whatever its order.

    The step is s = alpha p_0 with alpha = <r, r> / kappa (kernels/common.inc, `S.r_v / kappa`): the one operation of this
    file that rounds, by design.  The reference forms a = fl(<r, r> / kappa) from the two exact scalars -- one rounding --
    and s_i = fl(a p_i) -- one more.  A device whose division is correctly rounded and which multiplies once (s = 0 +
    alpha p by FMA is that multiplication) returns the same bits.  The bound allows a division good to one ulp instead:
    alpha' = a (1 + e), |e| <= 2^-52, moves a p_i by at most 2^-52 |a p_i|, and the two final roundings differ by at most
    2^-53 |a p_i| each: |got - ref| <= 2 x 2^-52 |ref| to first order, 2 ulp per entry.  Returns the worst entry in units
    of 2^-52 |ref|."""
    y, gr, s, r, v, pk, hp = (c.dev_alloc(p) for _ in range(7))
    c.upload(R["Y"], y)
    c.set_point_dev(y)
    c.upload(R["g"], gr)
    c.precond_setup(capi.PRECOND_NONE)
    it, sM = c.stpcg_dev(gr, W.FAR, s, r, v, pk, hp, kappa_fgr=W.NO_TARGET, theta=0.0, max_iters=1)
    assert it == 1, (tag, it)
    _exact(tag, "Hp of the first STPCG iteration", c.download(hp, p), -R["hg"])
    alpha = R["rr"] / R["kappa"]
    want = alpha * (-R["g"])
    got = c.download(s, p)
    err = np.abs(got - want)
    bound = 2.0 * 2.0 ** -52 * np.abs(want)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    assert np.all(err <= bound), (tag, "STPCG step", worst)
    for q in (y, gr, s, r, v, pk, hp):
        c.dev_free(q)
    return float((err / np.where(want != 0, 2.0 ** -52 * np.abs(want), 1.0)).max())


CASES = [(name, p) for name in topo.NAMES for p in W.strides(topo.CATALOGUE[name][1])]


@pytest.mark.parametrize("name,p", CASES, ids=["%s-p%d" % c for c in CASES])
@_guard
def test_every_operator_is_exact(name, p, switches):
    A, Q, dm, g = topo.build(name)
    Rq = sx.case(Q, dm, name, p, op="qx")
    R = sx.point_case(Q, dm, name, p)
    for form, win in W.FORMS:
        tag = "%s p=%d %s" % (name, p, form)
        switches.cora_debug_spmm_window_min_slices(win)
        c = _context(Rq["Qi"], dm, p)
        topo.check_shape(name, c)   # the DEVICE handle of the integer matrix has the declared shape
        _check_qx(tag, c, Rq)
        if name in sx.QX_SUBSET and p == dm.d:
            for k in sx.QX_COLS:
                _check_qx(tag, c, sx.case(Q, dm, name, p, k=k, op="qx"))
        c.close()
        c = _context(R["Qi"], dm, p)
        _check_point(tag, c, R, p)
        if p <= W.KAPPA_MAX_P:
            ulps = _check_stpcg(tag, c, R, p)
            print("\n%s: STPCG step within %.2f eps of fl(fl(<r,r>/kappa) p)" % (tag, ulps))
        c.close()


@pytest.mark.parametrize("name", sx.REPEATED)
@_guard
def test_exact_under_the_forced_stagger(name, switches):
    """Every pose slice sleeps before its first load (cora_debug_spmm_stagger_force(2), window form): the same bits."""
    A, Q, dm, g = topo.build(name)
    p = 5
    Rq, R = sx.case(Q, dm, name, p, op="qx"), sx.point_case(Q, dm, name, p)
    switches.cora_debug_spmm_window_min_slices(0)
    switches.cora_debug_spmm_stagger_force(2)
    switches.cora_debug_spmm_stagger_ticks(50)
    c = _context(Rq["Qi"], dm, p)
    _check_qx(name + " staggered", c, Rq)
    c.close()
    c = _context(R["Qi"], dm, p)
    _check_point(name + " staggered", c, R, p)
    _check_stpcg(name + " staggered", c, R, p)
    c.close()


@pytest.mark.parametrize("name", sx.REPEATED)
@_guard
def test_exact_after_update_values(name, switches):
    """A handle created with one integer matrix and given another (cora_update_values): the products of the second,
    bit for bit those of a fresh handle AND the exact ones, in both forms."""
    A, Q, dm, g = topo.build(name)
    p = 5
    first = sx.case(Q, dm, name, p, op="point")
    Rq, R = sx.case(Q, dm, name + "#2", p, op="qx"), sx.case(Q, dm, name + "#2", p, op="point")
    assert not np.array_equal(first["Qi"].val, R["Qi"].val)
    for form, win in W.FORMS:
        tag = "%s updated %s" % (name, form)
        switches.cora_debug_spmm_window_min_slices(win)
        c = _context(first["Qi"], dm, p)
        _check_point(tag + " (before)", c, first, p)
        c.update_values(Q.rowptr, Q.col, Rq["Qi"].val)
        _check_qx(tag, c, Rq)
        c.update_values(Q.rowptr, Q.col, R["Qi"].val)
        _check_point(tag, c, R, p)
        fresh = _context(R["Qi"], dm, p)
        for h in (c, fresh):
            h.set_point(R["Y"])
        _exact(tag, "Q X against a fresh handle", c.dataMatrixProduct(R["X"]), fresh.dataMatrixProduct(R["X"]))
        _exact(tag, "(Q - Lambda) X against a fresh handle", c.certificate_product(R["Xp"]), fresh.certificate_product(R["Xp"]))
        c.close()
        fresh.close()


@pytest.mark.parametrize("name", lrg.NAMES)
@_guard
def test_long_row_graphs_are_exact(name, switches):
    """tests/long_rows_graphs.py (several pieces per XCD, a run cut again, the path without ticket) with integer values:
    Q X at 2, 5 and 10 columns, every operator at a point at p = 3 and 5."""
    A, Q, dm = lrg.build(name)
    key = "long-" + name
    for form, win in W.FORMS:
        switches.cora_debug_spmm_window_min_slices(win)
        c = None
        for k in sx.LONG_QX_COLS:
            Rq = sx.case(Q, dm, key, 5, k=k, op="qx")
            c = c or _context(Rq["Qi"], dm, 5)
            _check_qx("%s %s" % (key, form), c, Rq)
        c.close()
        for p in sx.LONG_HVP_P:
            R = sx.case(Q, dm, key, p, op="point")
            c = _context(R["Qi"], dm, p)
            _check_point("%s p=%d %s" % (key, p, form), c, R, p)
            c.close()


@pytest.mark.parametrize("name", sx.PARTITIONED)
@_guard
def test_partitions_without_communication_are_exact(name, switches):
    """World 3, whole long rows (tests/test_gpu_topologies.py test_partitions_without_communication): every rank's shard
    of Q X and of the Hvp is exact, and the shards cover every row once."""
    A, Q, dm, g = topo.build(name)
    p, world = sx.PARTITION_P, 3
    Rq, R = sx.case(Q, dm, name, p, op="qx"), sx.point_case(Q, dm, name, p)
    _certified(Rq, name)
    _certified(R, name)
    for form, win in W.FORMS:
        switches.cora_debug_spmm_window_min_slices(win)
        owned = np.zeros(dm.N, dtype=int)
        for rank in range(world):
            tag = "%s %s rank %d of %d" % (name, form, rank, world)
            c = _context(Rq["Qi"], dm, p, rank=rank, world=world, whole_long_rows=True)
            m = c.row_map()
            mine = (m >= c.shard_begin) & (m < c.shard_begin + c.shard_rows)
            owned += mine
            x, o = c.dev_alloc(p), c.dev_alloc(p)
            c.upload(Rq["X"], x)
            c.spmm_dev(x, p, o)
            _exact(tag, "the shard of Q X", c.download(o, p)[mine], Rq["qx"][mine])
            c.close()
            c = _context(R["Qi"], dm, p, rank=rank, world=world, whole_long_rows=True)
            assert np.array_equal(c.row_map(), m)
            c.set_point(R["Y"])
            x, o = c.dev_alloc(p), c.dev_alloc(p)
            c.upload(R["V"], x)
            c.hvp_dev(x, o)
            _exact(tag, "the shard of the Hvp", c.download(o, p)[mine], R["hv"][mine])
            c.close()
        assert np.all(owned == 1)
