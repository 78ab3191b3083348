"""The chain slices' epilogues read S_P = sym(Q_PP) - Lambda_P (one symmetric d x d block per pose, written by
k_point_finish at every point) instead of the pose's own block and Lambda_P.  The Hessian-vector product, its kappa form
and the certificate operator against the CPU oracle at every row stride, in both forms of the pose slices; S follows the
point; the full-size graph; partitioned handles (serial and overlapped products); and Q X, which keeps the own slots."""
import threading

import numpy as np
import pytest

from cora_amd import capi, host
from cora_amd.dist import NativeLocalComm, NativeLocalGroup
from oracle import oracle as orc
from synth import make_problem

pytestmark = pytest.mark.gpu
REL = 1e-10
FORMS = (("window", 0), ("gather", 1 << 30))  # cora_debug_spmm_window_min_slices: LDS windows always / never


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def ctx_for(Q, dm, p):
    c = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val)
    c.set_rank(p)
    return c


@pytest.fixture
def restore_form():
    L = capi.load()
    old = L.cora_debug_spmm_window_min_slices(0)
    L.cora_debug_spmm_window_min_slices(old)
    yield L
    L.cora_debug_spmm_window_min_slices(old)


@pytest.mark.parametrize("d,p", [(d, p) for d in (2, 3) for p in range(max(d, 2), 25)])
def test_folded_epilogues_at_every_row_stride(d, p, restore_form):
    """Hvp, Hvp with kappa (one device STPCG product) and (Q - Lambda) X against the oracle, window and gather forms:
    ragged last slice, loop closures (general slots), several ranges per pose (tails)."""
    A, Q, dm = make_problem(d=d, n=333, n_landmarks=3, n_ranges=500, n_loops=7, seed=90 + p)
    rng = np.random.default_rng(100 + p)
    Y = orc.project_manifold(dm, rng.uniform(-1, 1, (dm.N, p)))
    G = orc.egrad(Q, Y)
    V = orc.tangent_proj(dm, Y, rng.uniform(-1, 1, (dm.N, p)))
    X = rng.standard_normal((dm.N, p))
    st, ob = orc.lambda_blocks(Q, dm, Y)
    ref_h = orc.hvp(Q, dm, Y, G, V)
    ref_s = orc.S_apply(Q, dm, st, ob, X)
    for form, win in FORMS:
        restore_form.cora_debug_spmm_window_min_slices(win)
        c = ctx_for(Q, dm, p)
        c.set_point(Y)
        assert relerr(c.certificate_product(X), ref_s) < REL, form
        assert relerr(c.Riemannian_Hessian_vector_product(Y, G, V), ref_h) < REL, form
        if p <= 12:
            y, g, s, r, v, pk, hp = (c.dev_alloc(p) for _ in range(7))
            c.upload(Y, y)
            c.set_point_dev(y)
            c.upload(V, g)
            c.precond_setup(capi.PRECOND_NONE)
            c.stpcg_dev(g, 1e-30, s, r, v, pk, hp, max_iters=1)  # radius ~ 0: one product, then the boundary step
            assert relerr(c.download(hp, p), orc.hvp(Q, dm, Y, G, c.download(pk, p))) < REL, form
        c.close()


def test_S_follows_the_point(restore_form):
    """S is rewritten at every point: products at Y2 after Y1 match the oracle at Y2, and the product of a handle that
    has no point yet is refused as before."""
    p = 5
    A, Q, dm = make_problem(d=3, n=400, n_landmarks=3, n_ranges=250, n_loops=5, seed=21)
    rng = np.random.default_rng(4)
    Y1 = orc.project_manifold(dm, rng.uniform(-1, 1, (dm.N, p)))
    Y2 = orc.project_manifold(dm, rng.uniform(-1, 1, (dm.N, p)))
    X = rng.standard_normal((dm.N, 7))
    V = orc.tangent_proj(dm, Y2, rng.uniform(-1, 1, (dm.N, p)))
    st2, ob2 = orc.lambda_blocks(Q, dm, Y2)
    for form, win in FORMS:
        restore_form.cora_debug_spmm_window_min_slices(win)
        c = ctx_for(Q, dm, p)
        with pytest.raises(capi.CoraError):
            c.certificate_product(X)
        assert relerr(c.dataMatrixProduct(X), orc.spmm(Q, X)) < REL
        c.set_point(Y1)
        st1, ob1 = orc.lambda_blocks(Q, dm, Y1)
        assert relerr(c.certificate_product(X), orc.S_apply(Q, dm, st1, ob1, X)) < REL, form
        c.set_point(Y2)
        assert relerr(c.certificate_product(X), orc.S_apply(Q, dm, st2, ob2, X)) < REL, form
        y, x, o = c.dev_alloc(p), c.dev_alloc(p), c.dev_alloc(p)
        c.upload(Y2, y)
        c.upload(V, x)
        c.hvp_dev(x, o)  # the point set by set_point(Y2)
        assert relerr(c.download(o, p), orc.hvp(Q, dm, Y2, orc.egrad(Q, Y2), V)) < REL, form
        c.close()


def test_full_size_graph():
    """The 10^5-pose graph bench.py times: Hvp at rank 5, (Q - Lambda) X with 10 columns, and Q X."""
    P = host.Problem.synthetic(dim=3, n_poses=100_000, n_landmarks=10, n_ranges=50_000, seed=42)
    P.update()
    dm = P.dims()
    _, _, rowptr, colidx, vals = P.matrix("DataMatrix")
    Q = orc.CSR(rowptr, colidx, vals, dm["N"])
    dims = orc.Dims(dm["d"], dm["n"], dm["r"], dm["N"])
    del P
    p = 5
    c = capi.Context(dims.d, dims.n, dims.r, dm["n"] + dm["l"], Q.rowptr, Q.col, Q.val)
    c.set_rank(p)
    rng = np.random.default_rng(8)
    Y = orc.project_manifold(dims, rng.uniform(-1, 1, (dims.N, p)))
    G = orc.egrad(Q, Y)
    V = orc.tangent_proj(dims, Y, rng.uniform(-1, 1, (dims.N, p)))
    X10 = rng.uniform(-1, 1, (dims.N, 10))
    assert relerr(c.Riemannian_Hessian_vector_product(Y, G, V), orc.hvp(Q, dims, Y, G, V)) < REL
    c.set_point(Y)
    st, ob = orc.lambda_blocks(Q, dims, Y)
    assert relerr(c.certificate_product(X10), orc.S_apply(Q, dims, st, ob, X10)) < REL
    assert relerr(c.dataMatrixProduct(X10), orc.spmm(Q, X10)) < REL
    c.close()


@pytest.mark.parametrize("world,n", [(2, 900), (4, 6000)])
def test_partitioned_handles(world, n):
    """Every rank's S covers its own poses: Hvp and (Q - Lambda) X of partitioned handles against the oracle, the
    overlapped product (interior slices ahead of the exchange) bit-equal to the serial one."""
    p = 5

    def make():
        P = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=5, n_ranges=n // 2, n_loops=4, seed=11)
        P.update()
        P.set_rank(p)
        return P
    P1 = make()
    dm = P1.dims()
    _, _, rowptr, colidx, vals = P1.matrix("DataMatrix")
    Q = orc.CSR(rowptr, colidx, vals, dm["N"])
    dims = orc.Dims(dm["d"], dm["n"], dm["r"], dm["N"])
    del P1
    rng = np.random.default_rng(12)
    Y = orc.project_manifold(dims, rng.uniform(-1, 1, (dims.N, p)))
    V = orc.tangent_proj(dims, Y, rng.uniform(-1, 1, (dims.N, p)))
    X7 = rng.uniform(-1, 1, (dims.N, 7))
    ref_h = orc.hvp(Q, dims, Y, orc.egrad(Q, Y), V)
    st, ob = orc.lambda_blocks(Q, dims, Y)
    ref_s = orc.S_apply(Q, dims, st, ob, X7)

    group = NativeLocalGroup(world)
    out, err = [None] * world, [None] * world

    def body(r):
        P = make()
        comm = P.set_partition(r, world, lambda ctx: NativeLocalComm(ctx, group))
        ctx = capi.Context.from_handle(P.context_ptr(), dm["d"], dm["n"], dm["r"], dm["n"] + dm["l"])
        y, x, o, x7, o7 = ctx.dev_alloc(p), ctx.dev_alloc(p), ctx.dev_alloc(p), ctx.dev_alloc(7), ctx.dev_alloc(7)
        ctx.upload(Y, y)
        ctx.set_point_dev(y)
        ctx.upload(V, x)
        ctx.upload(X7, x7)
        res = {}
        for mode in (2, 0):
            comm.overlap(mode)
            ctx.hvp_dev(x, o)
            ctx.certificate_product_dev(x7, 7, o7)
            res[mode] = (ctx.download(o, p), ctx.download(o7, 7))
        return res

    def run(r):
        try:
            out[r] = body(r)
        except BaseException as e:  # noqa: BLE001
            err[r] = e
            group.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(900)
    for e in err:
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise e
    for e in err:
        if e is not None:
            raise e
    for res in out:
        for H, S in res.values():
            assert relerr(H, ref_h) < REL
            assert relerr(S, ref_s) < REL
        assert np.array_equal(res[2][0], res[0][0]) and np.array_equal(res[2][1], res[0][1])
