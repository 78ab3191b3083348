"""What a handle allocates it frees, counted: every device and pinned block of the C API goes through one set of helpers
(cora_amd/csrc/capi.hip) that keep a process-wide count, cora_debug_live_allocations.  As a PROCESS of its own
(tests/test_gpu_handle_memory.py starts one per d) because the count is process-wide: another test's handle being collected
in the middle would move it.  python tests/handle_memory_worker.py <d>

CORA_TRI_TOP_INV=0 before the library loads, as in tests/stpcg_forms_worker.py: its graph `two` then gets a two-stage factor,
the smallest plan that uses the factor arena's sub-block arrays and scratch slots 6 and 7.

One CYCLE touches every owner of device memory of a handle.  Two handles live through it, because one graph cannot serve
both halves: the solver's half runs on graph `two` (a host.Problem, whose Cholesky factor is the handle's own ordering and
plan, with the raw calls on the borrowed handle), the initialisers' half on the multi-robot graph of
tests/test_gpu_init_shared.py (three chains, two landmarks, ranges, sightings, closures; a diagonal Q).  The count is one
number for the process, so the assertions are the same as for one handle:
  - the count after a SECOND identical cycle equals the count after the first: every re-install frees what it replaces
  - after the handles are destroyed the count is 0
  - the same for a handle created and destroyed with no call in between, for a host.Problem built from plaza2.pyfg, solved
    at max_rank = 4 and closed, and a creation refused for its arguments leaves the count unchanged
Every step prints `COUNT <step> <count>`, so a failure names the call that leaked; `DONE` ends a clean run.  No case provokes
a HIP error; any error of the library is an exception that nothing catches."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

POOL_MAX = 16  # kPoolMax of cora_dev_free (cora_amd/csrc/capi/resident.inc)


def count(step):
    from cora_amd import capi
    n = capi.live_allocations()
    print("COUNT %s %d" % (step, n), flush=True)
    return n


class Solver:
    """Graph `two` of tests/stpcg_forms_worker.py: the Problem, its measurement table and the borrowed handle."""

    def __init__(self, d):
        import residuals_ref as rr
        import stpcg_forms_worker as W
        from cora_amd import capi, host
        from oracle import assemble as asm
        n, l, r, loops, seed = W.GRAPHS[d]["two"]
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "two.pyfg")
            self.P, self.gt = host.Problem.synthetic(dim=d, n_poses=n, n_landmarks=l, n_ranges=r, n_loops=loops, seed=seed,
                                                     precond=capi.PRECOND_REGULARIZED_CHOLESKY, pyfg_out=path, ground_truth=True)
            self.table = rr.table(asm.parse_pyfg(path))
        self.P.update()
        dm = self.P.dims()
        assert dm["N"] == (d + 1) * n + l + r
        self.d, self.N, self.n = d, dm["N"], n
        _, _, self.rowptr, self.colidx, self.vals = self.P.matrix("DataMatrix")
        self.P.set_rank(d + 2)
        self.P.precond_info()
        self.h = capi.Context.from_handle(self.P.context_ptr(), dm["d"], dm["n"], dm["r"], dm["n"] + dm["l"])
        assert self.h.precond_stats()["stages"] == 2 and self.h.precond_entries()["sub_blocks"] >= 3
        self.rng = np.random.default_rng(40 + d)

    def cycle(self, tag):
        from cora_amd import capi
        P, h, d, N = self.P, self.h, self.d, self.N
        p = d + 2
        # rank, point, products, the preconditioner (installed again: the value updates below drop it), one inner solve
        P.set_preconditioner(capi.PRECOND_REGULARIZED_CHOLESKY)
        P.set_rank(p)
        P.precond_info()
        h.p = p
        Y = P.op("projectToManifold", np.hstack([self.gt, np.zeros((N, p - d))]) + 0.02 * self.rng.standard_normal((N, p)))
        vecs = [h.dev_alloc(p) for _ in range(POOL_MAX + 1)]  # one more than the pool keeps: the last free synchronises and frees
        count(tag + " rank-and-vectors")
        h.upload(Y, vecs[5])
        h.set_point_dev(vecs[5])
        h.spmm_dev(vecs[5], p, vecs[6])
        h.hvp_dev(vecs[6], vecs[7])
        count(tag + " point-product-hvp")
        iters, _ = h.stpcg_dev(h.point_ptrs()[2], 1e30, *vecs[:5], kappa_fgr=1e-300, theta=0.0, max_iters=3)
        assert iters >= 1 and h.stpcg_path() == 2  # the sweep-fused form: scratch slots 6 and 7
        count(tag + " cholesky-stpcg")
        back = h.download(vecs[5], p)
        assert np.array_equal(back, Y)
        for q in vecs:
            h.dev_free(q)
        count(tag + " upload-download-free")
        # the measurement table and what hangs on it
        X = np.asfortranarray(self.rng.standard_normal((N, d + 1)))
        h.set_measurements(*self.table)
        h.measurement_residuals(X)
        count(tag + " measurements-residuals")
        h.values_map_build(self.rowptr, self.colidx)
        h.update_values(self.rowptr, self.colidx, self.vals)
        count(tag + " value-map-update")
        h.assembly_build(self.rowptr, self.colidx)
        nw = h.assembly_info()["n_weights"]
        h.assemble_values(np.ones(nw))
        count(tag + " assembly-assemble")
        h.gnc_weights(X, np.full(nw, 7.8), "tls", 1.4)
        count(tag + " gnc")
        # comparison, pair table, rounding
        res = h.compare(Y, self.gt, aligned=True)
        assert res["aligned"].shape == (N, d)
        count(tag + " compare")
        h.set_pose_pairs([(i, i + 1) for i in range(self.n - 1)])
        h.rpe(Y, self.gt)
        count(tag + " pose-pairs-rpe")
        h.round(Y)
        count(tag + " round")
        P.set_rank(p + 1)
        P.precond_info()  # (the Problem applies the rank when it next needs the handle)
        assert h.L.cora_get_rank(h.h) == p + 1
        count(tag + " other-rank")

    def close(self):
        self.P.close()


class Initialisers:
    """The multi-robot graph of tests/test_gpu_init_shared.py on a handle of its own, every placement table installed."""

    def __init__(self, d):
        import closure_ref as cl
        import test_gpu_init_shared as shared
        from cora_amd import capi
        self.shared, self.d = shared, d
        self.dims, self.table, self.X, self.chains, self.starts = shared.graph(d, True)
        self.ctx = capi.Context(*self.dims, *cl.diagonal_q(*self.dims), device=0)

    def cycle(self, tag):
        shared, ctx, d, X = self.shared, self.ctx, self.d, self.X
        shared.install(ctx, d, self.table, self.chains, shared.ORDERS[0])
        count(tag + " tables")
        x = ctx.dev_alloc(d)
        for name in shared.ORDERS[0]:
            ctx.upload(X, x)
            shared.device_form(ctx, name, x, self.starts)
            count(tag + " " + name + "-dev")
        nr = ctx.measurement_counts()[1]
        dirs = np.ones((2, d))
        ctx.odometry_set_range_rows_dev([0, nr - 1], dirs, x)
        ctx.dev_free(x)
        count(tag + " range-rows")
        for name, form in (("odom", lambda: ctx.odometry_init(self.starts)), ("multilat", lambda: ctx.multilaterate(X, 2)),
                           ("chains", lambda: ctx.place_chains(X, 2)), ("sightings", lambda: ctx.place_by_sightings(X)),
                           ("closures", lambda: ctx.place_by_closures(X)),
                           ("closures_robust", lambda: ctx.place_by_closures_robust(X, 1.0, 1))):
            form()
            count(tag + " " + name + "-host-pointer")

    def close(self):
        self.ctx.close()


def main():
    d = int(sys.argv[1])
    os.environ["CORA_TRI_TOP_INV"] = "0"  # before the library loads: read once
    import closure_ref as cl
    import test_gpu_init_shared as shared
    from cora_amd import capi, host
    capi.load()
    assert count("start") == 0

    # a handle with no call in between
    dims = shared.graph(d, True)[0]
    Qd = cl.diagonal_q(*dims)
    ctx = capi.Context(*dims, *Qd, device=0)
    assert count("bare-handle-created") > 0
    ctx.close()
    assert count("bare-handle-destroyed") == 0

    # creations refused for their arguments (CORA_ERR_SHAPE): a rowptr that does not match N -- one entry short, refused
    # before the library is entered, and of the right length but not starting at 0, refused by the library's format builder
    rowptr, colidx, vals = Qd
    ctx = capi.Context(*dims, *Qd, device=0)
    before = count("before-refused-creations")
    for bad in (rowptr[:-1], np.concatenate([[1], rowptr[1:]]).astype(np.int32)):
        try:
            capi.Context(*dims, bad, colidx, vals, device=0)
        except capi.CoraError as e:
            assert e.code == 1, e
        else:
            raise AssertionError("a creation with a bad rowptr was accepted")
    assert count("after-refused-creations") == before
    ctx.close()
    assert count("second-handle-destroyed") == 0

    # two identical cycles on the same handles
    S, I = Solver(d), Initialisers(d)
    count("handles-created")
    after = []
    for k in (1, 2):
        S.cycle("cycle%d solver" % k)
        I.cycle("cycle%d init" % k)
        after.append(count("cycle%d end" % k))
    assert after[1] == after[0], after
    I.close()
    count("initialisers-destroyed")
    S.close()
    assert count("solver-destroyed") == 0

    # a whole solve through the host
    P = host.Problem.from_pyfg(os.path.join(ROOT, "tests", "golden", "datasets", "plaza2.pyfg"))
    P.update()
    P.set_preconditioner(capi.PRECOND_REGULARIZED_CHOLESKY)
    P.precond_info()
    P.solve(P.op("getRandomInitialGuess"), max_rank=4, max_seconds=60)
    assert count("plaza2-solved") > 0
    P.close()
    assert count("plaza2-closed") == 0
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
