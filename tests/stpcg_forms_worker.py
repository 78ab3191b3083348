"""Every form of the device-resident STPCG iteration at every row stride, on graphs of a few hundred poses, as a PROCESS of
its own (tests/test_gpu_stpcg_forms.py starts one per d).  python tests/stpcg_forms_worker.py <d> [spread]

A process of its own because the two-stage Cholesky plans must be reachable on small graphs: CORA_TRI_TOP_INV is read once,
when the library loads, and is set to 0 here before that.  The child runs every case of its d, prints one line
`CASE {json}` per case -- the case's id, the iteration form observed (stpcg_path), discrete mismatches (`fail`) and the worst
deviations from the numpy reference (`checks`: [name, value, kind]; the bounds per kind live in the test) -- and ends with
`DONE`.  Any error of the library (a HIP error among them) is an exception that nothing catches: the exit status is non-zero.

`spread` (no GPU): the reference against itself -- plain float64 inner products and an unrefined Cholesky solve against the
long-double / refined reference -- for every case, printed in the same format (lambda from scipy instead of the device)."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# Graphs (host.Problem.synthetic): poses, landmarks, ranges, loop closures, seed.  N = (d + 1) n + l + r.
#   two: the smallest n (n not a multiple of 64, N even, r = n // 2) whose plan under CORA_TRI_TOP_INV=0 has a stage of
#        substitution blocks (more than kTopCap = 1536 rows); that it allows the sweep-fused form is what the cases assert
#   one: N - 1 <= 1536, one explicit inverse;  odd: the same with N odd
GRAPHS = {
    2: dict(two=(438, 5, 219, 4, 3), one=(300, 4, 150, 4, 7), odd=(301, 4, 150, 3, 9)),
    3: dict(two=(342, 5, 171, 4, 8), one=(250, 4, 124, 4, 3), odd=(251, 5, 124, 3, 9)),
}
P_MAX_FUSED = 12   # row strides of the fused vector passes
FAR = 1e30         # a radius no step reaches
NO_TARGET = 1e-300  # a residual target no iteration reaches
MARGIN = 1e-3      # how far the reference's deciding quantity stays from its threshold in the exit cases
NEAR_NOISE = 0.02  # perturbation of the lifted ground truth, every entry
POINT_SEED = 0


def sweep_strides(d):
    return list(range(2, 12)) if d == 2 else list(range(3, 9))


def exit_stride(d):
    return d + 2


def odd_stride(d):
    return 3 if d == 2 else 5


def case_ids(d):
    ids = ["graph-two", "graph-one", "graph-odd"]
    for p in sweep_strides(d):
        ids += ["sweep-fold-p%d" % p, "sweep-nofold-p%d" % p, "warm-p%d" % p]
    ids += ["edge-path1-p%d" % p for p in ((9, 12) if d == 3 else (12,))]
    ids += ["edge-path0-p13", "oddN-path0-p%d" % odd_stride(d)]
    ids += ["inverse-p%d" % p for p in range(d, P_MAX_FUSED + 1)]
    ids += ["inverse-off-path1-p%d" % exit_stride(d), "nofuse-path0-p%d" % exit_stride(d)]
    ids += ["jacobi-p%d" % p for p in range(d, P_MAX_FUSED + 1)]
    ids += ["exit-%s-path%d" % (e, path) for path in range(4) for e in ("boundary", "curvature", "target")]
    ids += ["proj-p%d" % p for p in range(d, 25)]
    ids += ["proj-inplace-p4", "proj-inplace-p13"]
    return ids


def emit(case, **kw):
    kw["id"] = case
    print("CASE " + json.dumps(kw), flush=True)


class Graph:
    """One synthetic problem with everything the reference needs (and, on the GPU, the handle)."""

    def __init__(self, d, name, precond, device):
        from cora_amd import capi, host
        from oracle import oracle as orc
        import stpcg_ref as ref
        n, l, r, loops, seed = GRAPHS[d][name]
        self.d, self.name, self.device = d, name, device
        self.jacobi = precond == capi.PRECOND_JACOBI
        self.P, self.gt = host.Problem.synthetic(dim=d, n_poses=n, n_landmarks=l, n_ranges=r, n_loops=loops, seed=seed,
                                                 precond=precond, ground_truth=True)
        self.P.update()
        dm = self.P.dims()
        assert n % 64 != 0 and dm["N"] == (d + 1) * n + l + r
        _, _, rowptr, colidx, vals = self.P.matrix("DataMatrix")
        self.Q = orc.CSR(rowptr, colidx, vals, dm["N"])
        self.dm = orc.Dims(dm["d"], dm["n"], dm["r"], dm["N"])
        self.nt = dm["n"] + dm["l"]
        self.seed = seed
        self.lam = None
        self.stats = dict(n=n, landmarks=l, ranges=r, loops=loops, N=dm["N"])
        if not self.jacobi:
            if device:
                import ctypes as C
                self.P.set_rank(d)
                self.lam = self.P.precond_info()["lam"]
                st = (C.c_int64 * 4)()
                capi.load().cora_precond_stats(C.c_void_p(self.P.context_ptr()), st)
                h = capi.Context.from_handle(self.P.context_ptr(), dm["d"], dm["n"], dm["r"], self.nt)
                self.stats.update(stages=int(st[0]), top_rows=int(st[3]), blocks=h.precond_entries()["sub_blocks"])
            else:  # lambda_reg = ||Q||_2 / (1e6 - 1), src/CORA_problem.cpp:591
                import scipy.sparse.linalg as spl
                self.lam = float(spl.eigsh(self.Q.to_scipy(), k=1, which="LA", return_eigenvectors=False)[0]) / (1e6 - 1)
                pp = self.P.plan_probe(self.lam)
                self.stats.update(stages=pp["stages"], blocks=pp["blocks"], top_rows=pp["top_rows"])
            self.chol = ref.RegularizedCholesky(self.Q, self.dm, self.lam)
            self.chol_plain = ref.RegularizedCholesky(self.Q, self.dm, self.lam, plain=True)
        self._points = {}

    # ---- where the solves start
    def point(self, kind, p):
        """near: the lifted ground truth, rotated in R^p and perturbed in every column (positive curvature along the first
        directions);  far: a random point of the manifold (these Hessians are indefinite there)."""
        from oracle import oracle as orc
        key = (kind, p)
        if key not in self._points:
            rng = np.random.default_rng(POINT_SEED + 1000 * self.seed + 10 * p + (kind == "far"))
            N = self.dm.N
            if kind == "near":
                R, _ = np.linalg.qr(rng.standard_normal((p, p)))
                lifted = np.hstack([self.gt, np.zeros((N, p - self.d))])
                Y = orc.project_manifold(self.dm, (lifted + NEAR_NOISE * rng.standard_normal((N, p))) @ R)
            else:
                Y = orc.project_manifold(self.dm, rng.uniform(-1, 1, (N, p)))
            G = orc.egrad(self.Q, Y)
            self._points[key] = (Y, G, orc.tangent_proj(self.dm, Y, G))
        return self._points[key]

    def operators(self, kind, p, plain=False):
        from oracle import oracle as orc
        Y, G, g = self.point(kind, p)
        hess = lambda V: orc.hvp(self.Q, self.dm, Y, G, V)  # noqa: E731
        if self.jacobi:
            precon = lambda V: orc.precond_jacobi(self.Q, self.dm, Y, V)  # noqa: E731
        else:
            c = self.chol_plain if plain else self.chol
            precon = lambda V: c.precond(Y, V)  # noqa: E731
        return hess, precon, g

    def reference(self, kind, p, Delta=FAR, kappa_fgr=NO_TARGET, plain=False):
        from oracle import oracle as orc
        import stpcg_ref as ref
        hess, precon, g = self.operators(kind, p, plain)
        return ref.stpcg(hess, precon, g, Delta, kappa_fgr, 0.0, 3, dot=orc.inner if plain else ref.ldot)


class Device:
    """The handle of a Graph at one relaxation rank, with the work vectors of cora_stpcg_dev."""

    def __init__(self, G, p):
        from cora_amd import capi
        G.P.set_rank(p)
        G.P.precond_info()
        dm = G.dm
        self.G, self.p = G, p
        self.h = capi.Context.from_handle(G.P.context_ptr(), dm.d, dm.n, dm.r, G.nt)
        self.vecs = [self.h.dev_alloc(p) for _ in range(8)]
        self.grad = None

    def set_point(self, kind):
        Y = self.G.point(kind, self.p)[0]
        y = self.vecs[5]
        self.h.upload(Y, y)
        self.h.set_point_dev(y)
        self.grad = self.h.point_ptrs()[2]

    def first_direction(self):
        """p_0 = -P g as the device computes it."""
        pg = self.vecs[6]
        self.h.precondition_projected_dev(self.grad, pg)
        return -self.h.download(pg, self.p)

    def run(self, Delta, kappa_fgr, max_iters, env=(), warm=False):
        h, p = self.h, self.p
        s, r, v, pk, hp = self.vecs[:5]
        for var in env:
            os.environ[var] = "1"
        try:
            if warm:
                pg = self.vecs[6]
                h.precondition_projected_dev(self.grad, pg)
                g_g, g_pg = h.dot_dev(self.grad, self.grad, p), h.dot_dev(self.grad, pg, p)
                iters, sM = h.stpcg_warm_dev(self.grad, pg, g_g, g_pg, Delta, s, r, v, pk, hp, kappa_fgr=kappa_fgr, theta=0.0,
                                             max_iters=max_iters)
            else:
                iters, sM = h.stpcg_dev(self.grad, Delta, s, r, v, pk, hp, kappa_fgr=kappa_fgr, theta=0.0, max_iters=max_iters)
        finally:
            for var in env:
                os.environ.pop(var, None)
        return dict(iters=iters, sM=sM, path=h.stpcg_path(), folded=bool(h.stpcg_phase_us()["kappa_folded"]),
                    s=h.download(s, p), r=h.download(r, p), v=h.download(v, p), p=h.download(pk, p), Hp=h.download(hp, p))

    def close(self):
        for q in self.vecs:
            self.h.dev_free(q)


class Checks:
    """Worst value per name over everything a case compares."""

    def __init__(self):
        self.worst, self.fail = {}, []

    def add(self, name, value, kind):
        value = float(value)
        if not math.isfinite(value):
            self.fail.append("%s is not finite" % name)
            value = 1e300
        if name not in self.worst or value > self.worst[name][0]:
            self.worst[name] = (value, kind)

    def vectors(self, dm, name, got, want, kind="vec"):
        import stpcg_ref as ref
        if not np.all(np.isfinite(got)):
            self.fail.append("%s holds a non-finite value" % name)
            return
        for cls, e in ref.class_errors(dm, got, want).items():
            self.add("%s.%s" % (name, cls), e, kind)

    def expect(self, what, got, want):
        if got != want:
            self.fail.append("%s: %r, expected %r" % (what, got, want))

    def out(self):
        return dict(fail=self.fail, checks=[[k, v[0], v[1]] for k, v in sorted(self.worst.items())])


def rel(a, b):
    return abs(a - b) / abs(b)


# ---------------------------------------------------------------- the cases, reference side and device side together
def parity(G, p, want_path, with_v, env=(), dev=None, want_folded=None):
    """The state after 1, 2 and 3 iterations (iteration limit) against the reference's."""
    from oracle import oracle as orc
    C = Checks()
    states, how = G.reference("near", p)
    C.expect("reference exit", (how, len(states)), ("limit", 3))
    for st in states:  # the limit must be what ends the reference: curvature well on the positive side
        if not st["kappa_rel"] >= MARGIN:
            C.fail.append("reference curvature %.3e too close to zero" % st["kappa_rel"])
    path = None
    if dev is None:  # the reference against itself
        plain, _ = G.reference("near", p, plain=True)
        for k in range(min(len(states), len(plain))):
            for name in ("s", "r", "p") + (("v",) if with_v else ()):
                C.vectors(G.dm, name, plain[k][name], states[k][name])
            C.add("sM", rel(plain[k]["sM"], states[k]["sM"]), "vec")
    else:
        Y, Gr, _ = G.point("near", p)
        dev.set_point("near")
        prev = dev.first_direction()
        for k in range(1, len(states) + 1):
            out = dev.run(FAR, NO_TARGET, k, env)
            st = states[k - 1]
            path = out["path"]
            C.expect("path after %d" % k, out["path"], want_path)
            C.expect("iterations after %d" % k, out["iters"], k)
            if want_folded is not None:
                C.expect("kappa folded", out["folded"], want_folded)
            for name in ("s", "r", "p") + (("v",) if with_v else ()):
                C.vectors(G.dm, name, out[name], st[name])
            C.add("sM", rel(out["sM"], st["sM"]), "vec")
            # the product: Hp of the device against the oracle's product of the DEVICE'S OWN previous direction
            C.vectors(G.dm, "Hp", out["Hp"], orc.hvp(G.Q, G.dm, Y, Gr, prev), "prod")
            prev = out["p"]
    return dict(path=path, want_path=want_path, p=p, **C.out())


def warm_case(G, p, dev):
    C = Checks()
    if dev is None:
        return dict(path=None, want_path=2, p=p, **C.out())
    dev.set_point("near")
    cold = dev.run(FAR, NO_TARGET, 3)
    warm = dev.run(FAR, NO_TARGET, 3, warm=True)
    C.expect("path", warm["path"], 2)
    C.expect("iterations", warm["iters"], cold["iters"])
    C.expect("cold iterations", cold["iters"], 3)
    C.vectors(G.dm, "s", warm["s"], cold["s"])
    C.add("sM", rel(warm["sM"], cold["sM"]), "vec")
    return dict(path=warm["path"], want_path=2, p=p, **C.out())


def exit_inputs(G, p, how):
    """(point, Delta, kappa_fgr, iteration, failures): inputs under which the REFERENCE leaves the loop the intended way, the
    deciding quantity at least MARGIN (relative) away from its threshold."""
    bad = []
    if how == "curvature":
        base, _ = G.reference("far", p)
        j = next((k for k, st in enumerate(base) if not st["kappa"] > 0), None)
        if j is None:
            return "far", FAR, NO_TARGET, 0, ["the reference meets no non-positive curvature within three iterations"]
        for k, st in enumerate(base[:j + 1]):
            if not (st["kappa_rel"] >= MARGIN if k < j else st["kappa_rel"] <= -MARGIN):
                bad.append("curvature %.3e of iteration %d too close to zero" % (st["kappa_rel"], k + 1))
        Delta = 2.0 * math.sqrt(base[j]["sig_prev"]) if j > 0 else 1.0  # (inside iterations < j + 1: sigma <= Delta^2 / 4)
        return "far", Delta, NO_TARGET, j + 1, bad
    base, end = G.reference("near", p)
    if (end, len(base)) != ("limit", 3):
        return "near", FAR, NO_TARGET, 0, ["the reference does not run three iterations from the near point"]
    if how == "boundary":  # iteration 2 crosses: sigma_1 < Delta^2 <= sigma_2
        s1, s2 = base[0]["sig_next"], base[1]["sig_next"]
        D2 = 0.5 * (s1 + s2)
        if not (s1 <= D2 * (1 - MARGIN) and s2 >= D2 * (1 + MARGIN)):
            bad.append("squared step norms %.6e, %.6e leave no margin" % (s1, s2))
        return "near", math.sqrt(D2), NO_TARGET, 2, bad
    r0, r1, r2 = base[0]["r0"], math.sqrt(base[0]["rr"]), math.sqrt(base[1]["rr"])  # iteration 2 meets the target
    target = math.sqrt(r1 * r2)
    if not (r2 <= target * (1 - MARGIN) and r1 >= target * (1 + MARGIN) and target < r0):
        bad.append("residual norms %.6e, %.6e, %.6e leave no margin" % (r0, r1, r2))
    return "near", FAR, target / r0, 2, bad


EXIT_ENV = {0: ("CORA_NO_FUSE",), 1: ("CORA_NO_SWEEP_FUSE",), 2: (), 3: ()}


def exit_case(G, p, how, path, dev):
    C = Checks()
    kind, Delta, kfgr, it, bad = exit_inputs(G, p, how)
    C.fail += bad
    if it:
        states, end = G.reference(kind, p, Delta, kfgr)
        C.expect("reference exit", (end, len(states)), (how, it))
        want = states[-1]
        if dev is None:
            plain, pend = G.reference(kind, p, Delta, kfgr, plain=True)
            C.expect("plain reference exit", (pend, len(plain)), (how, it))
            C.vectors(G.dm, "s", plain[-1]["s"], want["s"])
            C.add("sM", rel(plain[-1]["sM"], want["sM"]), "vec")
        else:
            dev.set_point(kind)
            out = dev.run(Delta, kfgr, 3, EXIT_ENV[path])
            C.expect("path", out["path"], path)
            C.expect("iterations", out["iters"], it)
            C.vectors(G.dm, "s", out["s"], want["s"])
            C.add("sM", rel(out["sM"], want["sM"]), "vec")
    return dict(path=path if dev is None else out["path"] if it else None, want_path=path, p=p, exit=how, iteration=it, **C.out())


def proj_case(G, p, dev):
    """cora_precondition_projected_dev at a point against Proj_Y(M^-1 V), and the plain solve's residual."""
    C = Checks()
    Y = G.point("far", p)[0]
    V = np.asfortranarray(np.random.default_rng(50 + p).standard_normal((G.dm.N, p)))
    want = G.chol.precond(Y, V)
    if dev is None:
        C.vectors(G.dm, "PV", G.chol_plain.precond(Y, V), want, "proj")
        return dict(path=None, want_path=None, p=p, **C.out())
    dev.set_point("far")
    v, o = dev.vecs[6], dev.vecs[7]
    dev.h.upload(V, v)
    dev.h.precondition_projected_dev(v, o)
    C.vectors(G.dm, "PV", dev.h.download(o, p), want, "proj")
    x = G.P.op("precondition", V)  # the unprojected solve of the same plan: M x = V on the first N - 1 rows
    C.expect("pinned row", bool(np.all(x[-1] == 0.0)), True)
    C.add("residual", np.abs(G.chol.M @ x[:-1] - V[:-1]).max() / np.abs(V).max(), "proj")
    return dict(path=None, want_path=None, p=p, **C.out())


def inplace_case(G, p, dev):
    C = Checks()
    if dev is not None:
        dev.set_point("far")
        v, o = dev.vecs[6], dev.vecs[7]
        dev.h.upload(np.random.default_rng(70 + p).uniform(-1, 1, (G.dm.N, p)), v)
        dev.h.precondition_projected_dev(v, o)
        a = dev.h.download(o, p)
        dev.h.precondition_projected_dev(v, v)
        C.expect("in place equals out of place bit for bit", bool(np.array_equal(a, dev.h.download(v, p))), True)
        C.expect("finite", bool(np.all(np.isfinite(a))), True)
    return dict(path=None, want_path=None, p=p, **C.out())


def main():
    d = int(sys.argv[1])
    device = not (len(sys.argv) > 2 and sys.argv[2] == "spread")
    os.environ["CORA_TRI_TOP_INV"] = "0"   # before the library loads: read once
    from cora_amd import capi
    capi.load()
    CH, JA = capi.PRECOND_REGULARIZED_CHOLESKY, capi.PRECOND_JACOBI
    two, one, odd = Graph(d, "two", CH, device), Graph(d, "one", CH, device), Graph(d, "odd", CH, device)
    jac = Graph(d, "one", JA, device)
    for G in (two, one, odd):
        emit("graph-" + G.name, fail=[], checks=[], path=None, want_path=None, **G.stats)

    devices = {}

    def at(G, p):  # one Device per (graph, stride) at a time: set_rank frees what the last one held
        if not device:
            return None
        key = (id(G), p)
        if devices.get("key") != key:
            if "dev" in devices:
                devices["dev"].close()
            devices["dev"], devices["key"] = Device(G, p), key
        return devices["dev"]

    for p in sweep_strides(d):
        emit("sweep-fold-p%d" % p, **parity(two, p, 2, False, (), at(two, p), want_folded=True))
        emit("sweep-nofold-p%d" % p, **parity(two, p, 2, False, ("CORA_NO_KAPPA_FOLD",), at(two, p), want_folded=False))
        emit("warm-p%d" % p, **warm_case(two, p, at(two, p)))
    for p in ((9, 12) if d == 3 else (12,)):
        emit("edge-path1-p%d" % p, **parity(two, p, 1, True, (), at(two, p)))
    emit("edge-path0-p13", **parity(two, 13, 0, True, (), at(two, 13)))
    p = odd_stride(d)
    assert (odd.dm.N * p) % 2 == 1 and two.dm.N % 2 == 0 and one.dm.N % 2 == 0
    emit("oddN-path0-p%d" % p, **parity(odd, p, 0, True, (), at(odd, p)))
    for p in range(d, P_MAX_FUSED + 1):
        emit("inverse-p%d" % p, **parity(one, p, 3, False, (), at(one, p)))
    p = exit_stride(d)
    emit("inverse-off-path1-p%d" % p, **parity(one, p, 1, True, ("CORA_NO_INVERSE_FUSE",), at(one, p)))
    emit("nofuse-path0-p%d" % p, **parity(one, p, 0, True, ("CORA_NO_FUSE",), at(one, p)))
    for p in range(d, P_MAX_FUSED + 1):
        emit("jacobi-p%d" % p, **parity(jac, p, 1, True, (), at(jac, p)))
    p = exit_stride(d)
    for path in range(4):
        G = one if path == 3 else two
        for how in ("boundary", "curvature", "target"):
            emit("exit-%s-path%d" % (how, path), **exit_case(G, p, how, path, at(G, p)))
    for p in range(d, 25):
        emit("proj-p%d" % p, **proj_case(two, p, at(two, p)))
    for p in (4, 13):
        emit("proj-inplace-p%d" % p, **inplace_case(two, p, at(two, p)))
    if "dev" in devices:
        devices["dev"].close()
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
