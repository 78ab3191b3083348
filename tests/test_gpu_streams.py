"""The caller's-stream contract of the resident API (include/cora_hip.h, cora_set_stream): a handle moved to a stream of
the caller's enqueues everything there, in order with the caller's own work on that stream.

Every case runs a library call behind a gate (tests/stream_gate.py: a delay on the caller's stream, then a copy that makes
the real operand readable) on three kinds of stream -- torch.cuda.Stream(), torch.cuda.Stream(priority=-1) and stream 0,
the legacy default stream -- and compares, bit for bit, with a second handle of the same problem that stays on its own
stream and is used with host waits.  That results do not depend on when launches are enqueued is what
test_gpu_determinism.py and test_gpu_solver.py::test_host_loop_forms_take_the_same_path_bit_for_bit establish.  One result
per group is also held to the float64 oracle at the bound of that operation's own test, so that the file does not compare
the library with itself only.

CORA_STPCG_GRAPH stays unset: a stream capture on stream 0 is not legal HIP (the combination is documented as
unsupported in include/cora_hip.h).  The two-stage Cholesky plans (STPCG path 2) need CORA_TRI_TOP_INV=0 before the library
loads, as in tests/test_gpu_stpcg_forms.py: those cases run in one child process (`python test_gpu_streams.py sweep`)."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

if __name__ == "__main__":   # the child of test_stpcg_sweep_fused_in_a_child
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stpcg_ref as sref  # noqa: E402
from cora_amd import capi, host  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from stream_gate import KINDS, Gate, Plain, differing, same, stream, stream_ptr  # noqa: E402

pytestmark = pytest.mark.gpu

JACOBI, CHOLESKY = capi.PRECOND_JACOBI, capi.PRECOND_REGULARIZED_CHOLESKY
RANKS = [(2, 2), (3, 5), (3, 12), (3, 24)]
RANK_IDS = ["d%dp%d" % c for c in RANKS]
SEED = 17


def _bounds():
    """The bounds of the operations' own tests, imported where they are used (the modules are GPU test files)."""
    from test_gpu_parity import REL
    from test_gpu_stpcg_forms import BOUND
    return REL, BOUND


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class Side:
    """One handle of a synthetic problem with what the oracle needs."""

    def __init__(self, d, p, precond):
        n = 600 if precond == CHOLESKY else 300
        self.P, self.gt = host.Problem.synthetic(dim=d, n_poses=n, n_landmarks=4, n_ranges=150, n_loops=6, seed=SEED,
                                                 precond=precond, ground_truth=True)
        self.P.update()
        self.P.set_rank(p)
        self.lam = self.P.precond_info()["lam"]
        dm = self.P.dims()
        self.h = capi.Context.from_handle(self.P.context_ptr(), dm["d"], dm["n"], dm["r"], dm["n"] + dm["l"])
        _, _, self.rowptr, self.colidx, self.vals = self.P.matrix("DataMatrix")
        self.Q = orc.CSR(self.rowptr, self.colidx, self.vals, dm["N"])
        self.dims = orc.Dims(dm["d"], dm["n"], dm["r"], dm["N"])
        self.d, self.p, self.N, self.precond = d, p, dm["N"], precond


def data(side, p=None):
    """Host operands of a side at rank p: a point near the lifted ground truth, tangent and plain vectors."""
    p = side.p if p is None else p
    rng = np.random.default_rng(1000 * side.d + 10 * p + side.precond)
    N, dm = side.N, side.dims
    R, _ = np.linalg.qr(rng.standard_normal((p, p)))
    lifted = np.hstack([side.gt, np.zeros((N, p - side.d))])
    Y = orc.project_manifold(dm, (lifted + 0.02 * rng.standard_normal((N, p))) @ R)
    D = dict(p=p, Y=Y, V=orc.tangent_proj(dm, Y, rng.uniform(-1, 1, (N, p))), X=rng.uniform(-1, 1, (N, 24)),
             S=1e-2 * orc.tangent_proj(dm, Y, rng.uniform(-1, 1, (N, p))),
             X0=orc.project_manifold(dm, rng.uniform(-1, 1, (N, p))))
    for name in ("A", "W", "W2", "W3"):
        D[name] = rng.uniform(-1, 1, (N, p))
    D["C"] = [rng.uniform(-1, 1, (p, 3)), rng.uniform(-1, 1, (10, 3))]
    return D


_PAIRS, _REFS, _DATA = {}, {}, {}


def pair(d, p, precond, tag=""):
    """(handle under test, reference handle) of one problem; the reference never leaves its own stream."""
    key = (d, p, precond, tag)
    if key not in _PAIRS:
        _PAIRS[key] = (Side(d, p, precond), Side(d, p, precond))
        _DATA[key] = data(_PAIRS[key][0])
    return _PAIRS[key] + (_DATA[key],)


def on(side, kind):
    s = stream(kind)
    side.h.set_stream(stream_ptr(s))
    return s


def reference(key, fn):
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


def gated(name, d, p, precond, kind, case, *args, tag=""):
    """Runs `case` behind gates on the handle under test (on the stream of `kind`) and, once, with host waits on the
    reference handle; asserts the same bits.  Returns (result, data, side under test)."""
    t, r, D = pair(d, p, precond, tag)
    s = on(t, kind)
    want = reference((name, d, p, precond, tag) + args, lambda: case(r.h, lambda: Plain(r.h), D, *args))
    got = case(t.h, lambda: Gate(t.h, s), D, *args)
    assert same(got, want), differing(got, want)
    return got, D, t


# ---------------------------------------------------------------------------------------------------------------- cases
def case_spmm(c, mk, D, k):
    B = mk()
    x, out = B.operand(D["X"][:, :k]), B.result(k)
    with B:
        c.spmm_dev(x.ptr, k, out.ptr)
    res = {"out": B.host(out)}
    B.free()
    return res


def case_hvp(c, mk, D):
    B, p = mk(), D["p"]
    y, v, out = B.operand(D["Y"]), B.operand(D["V"]), B.result(p)
    with B:
        c.set_point_dev(y.ptr)
        c.hvp_dev(v.ptr, out.ptr)
    res = {"out": B.host(out), "f": c.point_cost(), "egrad": c.download(c.point_ptrs()[1], p),
           "rgrad": c.download(c.point_ptrs()[2], p)}
    B.free()
    return res


def case_certificate(c, mk, D):
    B = mk()
    y, x, out = B.operand(D["Y"]), B.operand(D["X"][:, :10]), B.result(10)
    with B:
        c.set_point_dev(y.ptr)
        c.certificate_product_dev(x.ptr, 10, out.ptr)
    res = {"out": B.host(out)}
    B.free()
    return res


def rowops_calls(c, B, D):
    """The row operations, none of which waits on the host: (thunks, collect)."""
    p = D["p"]
    v, a, w, w2, w3 = (B.operand(D[n]) for n in ("V", "A", "W", "W2", "W3"))
    x10, y10 = B.operand(D["X"][:, :10]), B.operand(D["X"][:, 10:20])
    o = [B.result(p) for _ in range(5)]
    calls = [lambda: c.tangent_space_projection_dev(v.ptr, o[0].ptr),
             lambda: c.project_to_manifold_dev(a.ptr, o[1].ptr),
             lambda: c.retract_dev(v.ptr, 0.5, o[2].ptr),
             lambda: c.axpby_dev(0.3, v.ptr, -1.1, w.ptr),
             lambda: c.axpy2_dev(0.7, v.ptr, w2.ptr, -0.2, a.ptr, w3.ptr),
             lambda: c.axpby_cols_dev(10, 2.0, x10.ptr, 0.5, y10.ptr),
             lambda: c.copy_dev(w.ptr, p, o[3].ptr),
             lambda: c.fill_random_dev(p, 99, o[4].ptr)]
    names = dict(tangent=o[0], manifold=o[1], retract=o[2], axpby=w, axpy2_1=w2, axpy2_2=w3, axpby_cols=y10, copy=o[3],
                 random=o[4])
    return calls, lambda: {n: B.host(b) for n, b in names.items()}


def case_rowops(c, mk, D):
    c.set_point(D["Y"])
    B = mk()
    calls, collect = rowops_calls(c, B, D)
    with B:
        for call in calls:
            call()
    res = collect()
    B.free()
    return res


def case_scalars(c, mk, D):
    """Calls that return scalars to the host, each behind a gate of its own (each waits)."""
    p, res = D["p"], {}
    B = mk()
    a, b, w = B.operand(D["A"]), B.operand(D["V"]), B.operand(D["W"])
    with B:
        res["dots"] = c.dots_dev([(a.ptr, b.ptr), (b.ptr, w.ptr), (a.ptr, a.ptr)])
    B.free()
    B = mk()
    x, v = B.operand(D["X"][:, :10]), B.operand(D["V"])
    with B:
        res["gram"] = c.gram_dev(x.ptr, 10, v.ptr, p)
    B.free()
    B = mk()
    x, v, a = B.operand(D["X"][:, :10]), B.operand(D["V"]), B.operand(D["A"])
    with B:
        res["gram_batch"] = c.gram_batch_dev([(v.ptr, p, a.ptr, p), (x.ptr, 10, x.ptr, 10)])
    B.free()
    B = mk()
    x, v, out = B.operand(D["X"][:, :10]), B.operand(D["V"]), B.result(3)
    with B:
        c.combine_dev([v.ptr, x.ptr], [p, 10], D["C"], 3, out.ptr)
    res["combine"] = B.host(out)
    B.free()
    B = mk()
    y = B.operand(D["Y"])
    with B:
        res["objective"] = c.objective_dev(y.ptr)
    B.free()
    return res


def case_precondition(c, mk, D):
    c.set_point(D["Y"])
    B, p = mk(), D["p"]
    v, v2, out = B.operand(D["V"]), B.operand(D["V"]), B.result(p)
    with B:
        c.precondition_projected_dev(v.ptr, out.ptr)
        c.precondition_projected_dev(v2.ptr, v2.ptr)
    res = {"out": B.host(out), "in_place": B.host(v2)}
    B.free()
    return res


def case_stpcg(c, mk, D, warm):
    """Eight iterations of the inner solve from a right-hand side that becomes readable when the gate opens."""
    p = D["p"]
    c.set_point(D["Y"])
    G = c.download(c.point_ptrs()[2], p)
    g_g = g_pg = 0.0
    if warm:  # what TNT hands over: P g, <g, g>, <g, P g>, with host waits before the gate
        gv, pgv = c.dev_alloc(p), c.dev_alloc(p)
        c.upload(G, gv)
        c.precondition_projected_dev(gv, pgv)
        PG, g_g, g_pg = c.download(pgv, p), c.dot_dev(gv, gv, p), c.dot_dev(gv, pgv, p)
        c.dev_free(gv)
        c.dev_free(pgv)
    B = mk()
    g = B.operand(G)
    pg = B.operand(PG) if warm else None
    s, r, v, pk, hp = (B.result(p) for _ in range(5))
    with B:
        if warm:
            it, sm = c.stpcg_warm_dev(g.ptr, pg.ptr, g_g, g_pg, 1e30, s.ptr, r.ptr, v.ptr, pk.ptr, hp.ptr, kappa_fgr=1e-300,
                                      theta=0.0, max_iters=8)
        else:
            it, sm = c.stpcg_dev(g.ptr, 1e30, s.ptr, r.ptr, v.ptr, pk.ptr, hp.ptr, kappa_fgr=1e-300, theta=0.0, max_iters=8)
    res = dict(iterations=it, step=sm, path=c.stpcg_path(), s=B.host(s), r=B.host(r), v=B.host(v), p=B.host(pk), hp=B.host(hp))
    B.free()
    return res


def case_trial_accept(c, mk, D):
    """A gate in front of the trial and a second one between trial and accept: the kept product survives the wait."""
    p = D["p"]
    c.set_point(D["Y"])
    B = mk()
    s, hs, xp, pg = B.operand(D["S"]), B.result(p), B.result(p), B.result(p)
    with B:
        trial = c.tnt_trial_dev(s.ptr, hs.ptr, xp.ptr)
        B.open(stage=False)
        accept = c.tnt_accept_dev(xp.ptr, pg.ptr)
    res = dict(trial=trial, accept=accept, hs=B.host(hs), xp=B.host(xp), pg=B.host(pg), f=c.point_cost(),
               rgrad=c.download(c.point_ptrs()[2], p))
    B.free()
    return res


def case_round_trip(c, mk, D):
    """gnc_weights_dev -> assemble_values_dev into a torch tensor -> update_values_dev from it -> set_point_dev ->
    hvp_dev, the weights a torch tensor that only torch touches between the calls."""
    p, C = D["p"], D["round_trip"]
    B = mk()
    x, barc2 = B.operand(C["X"]), B.raw_operand(C["barc2"])
    w, vals = B.raw_result(len(C["barc2"])), B.raw_result(C["nnz"])
    y, v, out = B.operand(D["Y"]), B.operand(D["V"]), B.result(p)
    with B:
        st = c.gnc_weights_dev(x.ptr, p, barc2.ptr, "tls", 1.4, True, w.ptr)
        B.open(stage=False)
        B.between(w)
        c.assemble_values_dev(w.ptr, vals.ptr)
        c.update_values_dev(vals.ptr)
        c.set_point_dev(y.ptr)
        c.hvp_dev(v.ptr, out.ptr)
    res = dict(stats=st["raw"], w=B.raw(w), vals=B.raw(vals), out=B.host(out), f=c.point_cost())
    B.free()
    return res


# ---------------------------------------------------------------------------------------------------------- the control
def test_the_gate_bites():
    """The control: the same pattern with the handle LEFT ON ITS OWN STREAM.  cora_spmm_dev (linear, no data-dependent
    loop) runs at once, ahead of the gate on the caller's stream, reads the NaN prefill and gives a non-finite result."""
    _, r, D = pair(3, 5, JACOBI)
    s = stream("plain")
    B = Gate(r.h, s)
    x, out = B.operand(D["X"][:, :5]), B.result(5)
    with B:
        r.h.spmm_dev(x.ptr, 5, out.ptr)
        r.h.sync()
    got = B.host(out)
    assert not np.all(np.isfinite(got))
    assert np.all(np.isfinite(B.host(x)))  # (the operand did arrive, after the product had read its prefill)
    print("\ncontrol: %d of %d entries of the product are not finite; gate %.1f ms" % (np.sum(~np.isfinite(got)), got.size,
                                                                                      B.delays[0]))


# ------------------------------------------------------------------------- a. products and row operations behind the gate
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,p", RANKS, ids=RANK_IDS)
def test_products(d, p, kind):
    REL, _ = _bounds()
    for k in sorted({1, p, 10}):
        got, D, t = gated("spmm", d, p, JACOBI, kind, case_spmm, k)
    assert relerr(got["out"], orc.spmm(t.Q, np.asfortranarray(D["X"][:, :k]))) < REL
    got, D, t = gated("hvp", d, p, JACOBI, kind, case_hvp)
    assert relerr(got["out"], orc.hvp(t.Q, t.dims, D["Y"], orc.egrad(t.Q, D["Y"]), D["V"])) < REL
    gated("certificate", d, p, JACOBI, kind, case_certificate)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,p", RANKS, ids=RANK_IDS)
def test_row_operations(d, p, kind):
    got, D, t = gated("rowops", d, p, JACOBI, kind, case_rowops)
    REL, _ = _bounds()
    assert same(got["copy"], got["axpby"])
    assert relerr(got["retract"], orc.retract(t.dims, D["Y"], 0.5 * D["V"])) < REL


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,p", RANKS, ids=RANK_IDS)
def test_scalars_reach_the_host_behind_a_blocked_stream(d, p, kind):
    REL, _ = _bounds()
    got, D, t = gated("scalars", d, p, JACOBI, kind, case_scalars)
    f = orc.cost(t.Q, D["Y"])
    assert abs(got["objective"] - f) < REL * abs(f)


# ------------------------------------------------------------------------------------- b. preconditioner and inner solve
_CHOL = {}


def _cholesky_reference(t):
    key = (t.d, t.N)
    if key not in _CHOL:
        _CHOL[key] = sref.RegularizedCholesky(t.Q, t.dims, t.lam)
    return _CHOL[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("precond", [JACOBI, CHOLESKY], ids=["jacobi", "cholesky"])
@pytest.mark.parametrize("d,p", RANKS, ids=RANK_IDS)
def test_precondition(d, p, precond, kind):
    _, BOUND = _bounds()
    got, D, t = gated("precondition", d, p, precond, kind, case_precondition)
    assert same(got["out"], got["in_place"])
    if precond == CHOLESKY:
        want = _cholesky_reference(t).precond(D["Y"], D["V"])
    else:
        want = orc.precond_jacobi(t.Q, t.dims, D["Y"], D["V"])
    for cls, e in sref.class_errors(t.dims, got["out"], want).items():
        assert e <= BOUND["proj"], (cls, e)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("precond", [JACOBI, CHOLESKY], ids=["jacobi", "cholesky"])
@pytest.mark.parametrize("d,p", RANKS, ids=RANK_IDS)
def test_stpcg(d, p, precond, warm, kind):
    got, D, t = gated("stpcg", d, p, precond, kind, case_stpcg, warm)
    assert got["iterations"] > 1 and np.all(np.isfinite(got["s"]))
    print("\nstpcg path %d after %d iterations" % (got["path"], got["iterations"]))
    # Jacobi: the fused vector passes up to stride 12, one operation per launch above; the one-inverse Cholesky plans of
    # these graphs: the inverse-fused form up to stride 12
    assert got["path"] == (0 if p > 12 else 1 if precond == JACOBI else 3)


SWEEP_RANKS = [(2, 2), (3, 5), (3, 12)]


def sweep_main():
    """The child of test_stpcg_sweep_fused_in_a_child: the Cholesky cases with two-stage plans."""
    os.environ["CORA_TRI_TOP_INV"] = "0"   # before the library loads: read once
    capi.load()
    for d, p in SWEEP_RANKS:
        for warm in (False, True):
            for kind in KINDS:
                t, r, D = pair(d, p, CHOLESKY)
                s = on(t, kind)
                want = reference(("stpcg", d, p, warm), lambda: case_stpcg(r.h, lambda: Plain(r.h), D, warm))
                got = case_stpcg(t.h, lambda: Gate(t.h, s), D, warm)
                print("CASE " + json.dumps(dict(d=d, p=p, warm=warm, kind=kind, path=got["path"], iterations=got["iterations"],
                                                differing=differing(got, want), finite=bool(np.all(np.isfinite(got["s"]))))),
                      flush=True)
    print("DONE", flush=True)


def test_stpcg_sweep_fused_in_a_child():
    """STPCG path 2 (the passes ride on the two sweeps of a two-stage Cholesky plan) behind the gate on every kind of
    stream, cold and warm."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "sweep"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=240)
    cases = [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("CASE ")]
    assert r.returncode == 0 and "DONE" in r.stdout.splitlines(), r.stdout[-4000:]
    assert len(cases) == len(SWEEP_RANKS) * 2 * len(KINDS)
    print("\n" + "\n".join(json.dumps(c) for c in cases))
    for c in cases:
        assert c["differing"] == [] and c["finite"] and c["iterations"] > 1, c
        # strides 9 to 12 of a two-stage plan at d = 3 take the fused vector passes (tests/stpcg_forms_worker.py)
        assert c["path"] == (1 if (c["d"], c["p"]) == (3, 12) else 2), c


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("precond", [JACOBI, CHOLESKY], ids=["jacobi", "cholesky"])
@pytest.mark.parametrize("d,p", RANKS, ids=RANK_IDS)
def test_trial_then_accept(d, p, precond, kind):
    got, D, t = gated("trial_accept", d, p, precond, kind, case_trial_accept)
    REL, _ = _bounds()
    f = orc.cost(t.Q, got["xp"])
    assert abs(got["accept"][0] - f) < REL * abs(f)


@pytest.mark.parametrize("kind", KINDS)
def test_whole_solve_with_a_second_thread_on_the_stream(kind):
    """P.tnt with the Problem's handle on the caller's stream while a second Python thread enqueues torch kernels on that
    stream between the solver's calls: iterations, status, product count, cost and point of the own-stream run."""
    import torch
    t, r, D = pair(3, 5, JACOBI)
    x0 = D["X0"]
    want = reference(("tnt",), lambda: r.P.tnt(x0, max_iterations=10))
    s = on(t, kind)
    stop, running, count = threading.Event(), threading.Event(), [0]

    def poke():
        try:
            with torch.cuda.stream(s):
                acc = torch.zeros(4096, dtype=torch.float64, device="cuda:0")
                ev = torch.cuda.Event()
                while not stop.is_set():
                    acc.add_(1.0)
                    ev.record()
                    ev.synchronize()   # paced by the stream itself: one kernel in flight, between the solver's launches
                    count[0] += 1
                    if count[0] == 3:
                        running.set()
                poke.total = float(acc.sum().item())
        finally:
            running.set()   # (an error in this thread must not leave the test waiting)

    th = threading.Thread(target=poke)
    th.start()
    try:
        assert running.wait(60) and count[0] >= 3   # the thread is up and enqueueing before the solver starts
        first = count[0]
        got = t.P.tnt(x0, max_iterations=10)
        during = count[0] - first
    finally:
        stop.set()
        th.join()
    print("\n%d torch kernels between the calls of %d iterations (%d products)" % (during, got["iterations"], got["hvps"]))
    assert during > 0 and poke.total == 4096.0 * count[0]
    assert (got["iterations"], got["status"], got["hvps"]) == (want["iterations"], want["status"], want["hvps"])
    assert same(got["f"], want["f"]) and same(got["x"], want["x"])
    assert got["hvps"] > 10


# ---------------------------------------------------------------------- c. a device round trip with no host wait between
def _round_trip_pair(d, p):
    t, r, D = pair(d, p, JACOBI, "round-trip")
    if "round_trip" not in D:
        for side in (t, r):
            side.P.reweight({})   # installs the measurement table (unit weights) and the term map on the handle
            side.h.values_map_build(side.rowptr, side.colidx)
        nw = r.h.assembly_info()["n_weights"]
        rng = np.random.default_rng(90 + 10 * d + p)
        X = D["Y"] + 0.05 * rng.standard_normal(D["Y"].shape)
        r2 = r.h.debug_gnc_weights_host(X, np.full(nw, np.inf), "none")["r2"]
        barc2 = rng.choice([0.3, 1.0, 7.8, 40.0], nw) * np.median(r2)
        barc2[rng.uniform(size=nw) < 0.1] = np.inf
        D["round_trip"] = dict(X=X, barc2=barc2, nnz=len(t.vals))
    return t, r, D


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,p", RANKS, ids=RANK_IDS)
def test_device_round_trip(d, p, kind):
    REL, _ = _bounds()
    _round_trip_pair(d, p)
    got, D, t = gated("round_trip", d, p, JACOBI, kind, case_round_trip, tag="round-trip")
    w = got["w"]
    assert np.all((w >= 0) & (w <= 1)) and np.any(w < 1) and np.any(w == 1)
    Qw = orc.CSR(t.rowptr, t.colidx, got["vals"].copy(), t.N)   # the assembled values against the oracle's product
    assert relerr(got["out"], orc.hvp(Qw, t.dims, D["Y"], orc.egrad(Qw, D["Y"]), D["V"])) < REL
    assert not same(got["vals"], t.vals)


# ----------------------------------------------------------------------------------- d. evaluation and initialisers
# These calls wait at their end; what is checked is that they wait for the caller's stream first.  Each on the smallest
# synthetic case of its own GPU test, from the builders of the test_*_cpu.py files as those tests take them.  The
# reference is the builders' own device handle (cached there, on its own stream); the handle under test is a twin.
def _twin(mod, key, build):
    """(the module's cached case, the same case built once more) -- the builder run again with the cache entry put aside,
    so that the handle that goes to a caller's stream is not the one the module's other users share."""
    shared = build()
    kept = mod._BUILT.pop(key)
    try:
        mine = build()
    finally:
        mod._BUILT[key] = kept
    assert mine[0] is not shared[0]
    return shared, mine


def _in_place(X, call):
    """A case whose call rewrites a resident vector of d columns in place."""
    def run(c, B):
        x = B.operand(X)
        with B:
            res = dict(call(c, x.ptr))
        res["X"] = B.host(x)
        B.free()
        return res
    return run


def _placement():
    import placement_ref as pl
    import test_placement_cpu as m
    name, d, gn = "short_chain", 2, 5
    shared, mine = _twin(m, (name, d, 0), lambda: m.case(name, d, device=0))
    _, dims, table, X = shared[:4]

    def check(got):
        got = dict(got, X_in=X)
        pl.check(got, *dims, table, m.reference_of(name, d, gn))   # asserts the bound of tests/placement_ref.py
        assert same(got["X"], m.mirror_of(name, d, gn)["X"])
    return shared[0], mine[0], _in_place(X, lambda c, x: c.place_chains_dev(x, gn)), check


def _from_case(module, name, d, call):
    def make():
        import importlib
        m = importlib.import_module(module)
        shared, mine = _twin(m, (name, d, 0), lambda: m.case(name, d, device=0))
        return shared[0], mine[0], _in_place(shared[3], lambda c, x: call(m, shared, c, x)), None
    return make


def _odometry():
    import test_odom_init_cpu as m
    shared, mine = _twin(m, ("syn", 2, "ones", 0), lambda: m.synthetic(2, "ones", device=0))
    _, dims, table, chains = shared
    starts, lm, _ = m.reference_of(("syn", 2, "ones"), dims, table, chains)

    def run(c, B):
        x = B.result(dims[0])
        with B:
            res = dict(c.odometry_init_dev(starts, lm, x.ptr))
        res["X"] = B.host(x)
        B.free()
        return res
    return shared[0], mine[0], run, None


_SMALL = {}


def _small_graph():
    """Two handles of the n = 30 graph of tests/test_gpu_round.py, test_gpu_rpe.py (the smallest with more than two poses)."""
    if not _SMALL:
        import residuals_ref as rr
        import rpe_ref as rp
        from synth import make_graph
        from test_gpu_round import graph_ctx
        g = make_graph(d=2, n=30, n_landmarks=3, n_ranges=20, n_loops=0)
        pairs = rp.pairs_by_step([list(range(30))], 1)[0].astype(np.int32)
        for name in ("shared", "mine"):
            ctx, dims, truth = graph_ctx(g)
            ctx.set_measurements(*rr.table(g))
            ctx.set_pose_pairs(pairs)
            _SMALL[name] = ctx
        _SMALL.update(dims=dims, truth=truth, pairs=pairs)
    return _SMALL


def _evaluation(which):
    def make():
        import compare_ref as cr
        import round_ref as rf
        import rpe_ref as rp
        G = _small_graph()
        dims, truth = G["dims"], G["truth"]
        d, N = dims[0], len(truth)
        rng = np.random.default_rng(31)
        k = 5
        Ref = cr.reference_of_rank(truth, *dims, d, rng)
        Xn = cr.gauge_copy(Ref, *dims, k, rng)[0] + 1e-2 * rng.standard_normal((N, k))
        Y = rf.relaxed_point(truth, *dims, k, rng)
        check = None

        def run(c, B):
            if which == "residuals":
                x = B.operand(0.2 * Xn)
                with B:
                    res = dict(c.measurement_residuals_dev(x.ptr, k))
            elif which == "compare":
                x, ref, al = B.operand(Xn), B.operand(Ref), B.result(d)
                with B:
                    res = dict(c.compare_dev(x.ptr, k, ref.ptr, d, d_aligned=al.ptr))
                res["aligned"] = B.host(al)
            elif which == "rpe":
                x, ref = B.operand(Xn), B.operand(Ref)
                with B:
                    res = dict(c.rpe_dev(x.ptr, k, ref.ptr, d))
            else:
                y, out = B.operand(Y), B.result(d)
                with B:
                    res = dict(c.round_dev(y.ptr, k, out.ptr))
                res["X"] = B.host(out)
            B.free()
            return res
        if which == "round":
            check = lambda got: rf.check(got, Y, *dims, what="round behind the gate")  # noqa: E731  (round_ref's own bounds)
        if which == "rpe":
            check = lambda got: rp.check(got, Xn, Ref, *dims, G["pairs"], what="rpe behind the gate")  # noqa: E731
        return G["shared"], G["mine"], run, check
    return make


def _robust_ranges(m, shared, c, x):
    return c.multilaterate_robust_dev(x, m.BARC2, 5, **m.vote_of("lengths", 2))


def _robust_closures(m, shared, c, x):
    return c.place_by_closures_robust_dev(x, m.BARC2, **shared[6])


EVAL = {
    "measurement_residuals": _evaluation("residuals"), "compare": _evaluation("compare"), "rpe": _evaluation("rpe"),
    "round": _evaluation("round"), "odometry_init": _odometry,
    "multilaterate": _from_case("test_multilat_cpu", "lengths", 2, lambda m, sh, c, x: c.multilaterate_dev(x, 5)),
    "multilaterate_robust": _from_case("test_range_consensus_cpu", "lengths", 2, _robust_ranges),
    "place_chains": _placement,
    "place_by_sightings": _from_case("test_sighting_cpu", "two_chains", 2, lambda m, sh, c, x: c.place_by_sightings_dev(x)),
    "place_by_closures": _from_case("test_closure_cpu", "single_edge", 2, lambda m, sh, c, x: c.place_by_closures_dev(x)),
    "place_by_closures_robust": _from_case("test_closure_consensus_cpu", "clean", 2, _robust_closures),
}
_EVAL_BUILT = {}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", sorted(EVAL))
def test_evaluation_and_initialisers(op, kind):
    if op not in _EVAL_BUILT:
        _EVAL_BUILT[op] = EVAL[op]()
    shared, mine, run, check = _EVAL_BUILT[op]
    s = stream(kind)
    mine.set_stream(stream_ptr(s))
    want = reference(("eval", op), lambda: run(shared, Plain(shared)))
    got = run(mine, Gate(mine, s))
    assert same(got, want), differing(got, want)
    if check:
        check(got)


# ----------------------------------------------------------------------------------------------------- e. life cycle
def _hold(c, D):
    """What a handle holds across a move: a kept trial product, vectors returned to the pool, scratch."""
    p = D["p"]
    c.set_point(D["Y"])
    s, hs, xp, pg = (c.dev_alloc(p) for _ in range(4))
    c.upload(D["S"], s)
    trial = c.tnt_trial_dev(s, hs, xp)
    a, b = c.dev_alloc(p), c.dev_alloc(p)
    c.upload(D["V"], a)
    c.upload(D["A"], b)
    c.dev_free(a)
    c.dev_free(b)
    return dict(trial=trial, f=c.objective_dev(xp), vecs=(s, hs, xp, pg))


def _use(c, D, held):
    p = D["p"]
    s, hs, xp, pg = held["vecs"]
    accept = c.tnt_accept_dev(xp, pg)
    a, b = c.dev_alloc(p), c.dev_alloc(p)   # re-issued from the pool, zeroed on the handle's stream
    zero = not c.download(a, p).any() and not c.download(b, p).any()
    c.axpby_dev(1.0, hs, 0.0, a)
    res = dict(trial=held["trial"], f=held["f"], accept=accept, pg=c.download(pg, p), rgrad=c.download(c.point_ptrs()[2], p),
               zero=zero, again=c.objective_dev(xp), hs=c.download(a, p))
    for q in (s, hs, xp, pg, a, b):
        c.dev_free(q)
    return res


def test_life_cycle_across_streams():
    """own -> s1 -> s2 -> stream 0 -> s1, holding a kept trial product, pooled vectors and scratch across each move, and a
    new rank after the second."""
    REL, _ = _bounds()
    t, r = Side(3, 5, JACOBI), Side(3, 5, JACOBI)
    D = data(t)
    for step, kind in enumerate(("plain", "second", "zero", "plain")):
        held_t, held_r = _hold(t.h, D), _hold(r.h, D)
        s = on(t, kind)
        got, want = _use(t.h, D, held_t), _use(r.h, D, held_r)
        assert got["zero"] and same(got, want), (kind, differing(got, want))
        if step == 1:
            for side in (t, r):
                side.h.set_rank(7)
            D = data(t, 7)
        for case, args in ((case_spmm, (10,)), (case_hvp, ()), (case_rowops, ())):
            want = case(r.h, lambda: Plain(r.h), D, *args)
            got = case(t.h, lambda: Gate(t.h, s), D, *args)
            assert same(got, want), (kind, case.__name__, differing(got, want))
    assert relerr(got["retract"], orc.retract(t.dims, D["Y"], 0.5 * D["V"])) < REL


MOVES = [("plain", "high"), ("zero", "plain"), ("high", "zero")]


@pytest.mark.parametrize("src,dst", MOVES, ids=["%s-%s" % m for m in MOVES])
def test_set_stream_waits_for_the_old_stream(src, dst):
    """A product pending behind a gate on the old stream, the move, a product of its result on the new stream: the move
    returns when the old stream has drained, so the second product reads the first one's result."""
    import torch
    t, r, D = pair(3, 5, JACOBI)
    want = reference(("twice",), lambda: _twice(r.h, D))
    s1 = on(t, src)
    B = Gate(t.h, s1)
    x, mid, out = B.operand(D["X"][:, :5]), B.result(5), B.result(5)
    B.open()
    t.h.spmm_dev(x.ptr, 5, mid.ptr)
    done = torch.cuda.Event()
    done.record(s1)
    s2 = on(t, dst)
    drained = done.query()
    t.h.spmm_dev(mid.ptr, 5, out.ptr)
    t.h.sync()
    B.snapshot()
    B.wait()
    assert drained
    assert same(B.host(out), want)


def _twice(c, D):
    B = Plain(c)
    x, mid, out = B.operand(D["X"][:, :5]), B.result(5), B.result(5)
    c.spmm_dev(x.ptr, 5, mid.ptr)
    c.spmm_dev(mid.ptr, 5, out.ptr)
    res = B.host(out)
    B.free()
    return res


@pytest.mark.parametrize("kind", KINDS)
def test_a_recycled_vector_is_zeroed_in_stream_order(kind):
    """A vector goes back to the pool with a write to it still pending behind the gate and is issued again at once: the
    zeroing is ordered behind that write on the caller's stream."""
    t, r, D = pair(3, 5, JACOBI)
    s = on(t, kind)
    c, p = t.h, 5
    B = Gate(c, s)
    x = B.operand(D["V"])
    held = [c.dev_alloc(p) for _ in range(16)]   # every pooled vector of this size is out, with room left in the pool
    v = held.pop()
    B.open()
    c.copy_dev(x.ptr, p, v)
    c.dev_free(v)
    again = c.dev_alloc(p)
    B.snapshot()
    B.wait()
    got = c.download(again, p)
    for q in held + [again]:
        c.dev_free(q)
    assert again == v   # (the pool handed the same vector out again)
    assert not got.any()


@pytest.mark.parametrize("kind", KINDS)
def test_timer_and_sync_are_on_the_callers_stream(kind):
    import torch
    t, r, D = pair(3, 5, JACOBI)
    s = on(t, kind)
    B = Gate(t.h, s)
    t.h.timer_start()
    B.open()
    ms = t.h.timer_stop_ms()
    B.wait()
    assert ms >= B.delays[0], (ms, B.delays)
    B = Gate(t.h, s)
    B.open()
    done = torch.cuda.Event()
    done.record(s)
    t.h.sync()
    assert done.query()   # cora_sync returned only after the gate
    B.wait()


@pytest.mark.parametrize("kind", KINDS)
def test_close_behind_a_gate(kind):
    """cora_ctx_destroy of a handle on a caller's stream waits for the handle's pending work (on stream 0 too), returns
    every allocation, and leaves the torch stream usable."""
    import torch
    REL, _ = _bounds()
    _, r, D = pair(3, 5, JACOBI)
    want = reference(("twice",), lambda: _twice(r.h, D))
    s = stream(kind)
    before = capi.live_allocations()
    ctx = capi.Context(r.d, r.dims.n, r.dims.r, r.dims.n_trans, r.rowptr, r.colidx, r.vals)
    assert capi.live_allocations() > before
    ctx.set_stream(stream_ptr(s))
    B = Gate(ctx, s)
    x, out = B.operand(D["X"][:, :5]), B.result(5)
    scratch = ctx.dev_alloc(5)
    B.open()
    ctx.spmm_dev(x.ptr, 5, scratch)
    ctx.spmm_dev(scratch, 5, out.ptr)
    done = torch.cuda.Event()
    done.record(s)
    ctx.close()
    assert done.query()   # the pending products have run when the handle is gone
    with torch.cuda.stream(stream("second" if kind != "second" else "plain")):
        early = out.tensor.clone()   # read from ANOTHER stream, with no wait of its own
    torch.cuda.synchronize()
    assert capi.live_allocations() == before
    with torch.cuda.stream(s):   # the caller's stream was not destroyed with the handle
        acc = torch.ones(1024, dtype=torch.float64, device="cuda:0")
        acc.mul_(3.0)
    s.synchronize()
    assert float(acc.sum().item()) == 3072.0
    rows = int(r.h.rows)
    got = r.h.download(early.data_ptr(), 5)
    assert early.numel() == rows * 5 and same(got, want)
    Qx = orc.spmm(r.Q, orc.spmm(r.Q, np.asfortranarray(D["X"][:, :5])))
    assert relerr(got, Qx) < 10 * REL   # (two products in a row)


# ------------------------------------------------------------------------------- f. two handles, two streams, one thread
DUOS = [("plain", "second"), ("high", "zero"), ("zero", "plain")]


def _mixed_calls(c, B, D):
    """Calls of groups a and b that do not wait on the host, on one handle: (thunks, collect)."""
    p = D["p"]
    calls, collect_rows = rowops_calls(c, B, D)
    x, q, v, hv, pv = B.operand(D["X"][:, :10]), B.result(10), B.operand(D["V"]), B.result(p), B.result(p)
    calls = [lambda: c.spmm_dev(x.ptr, 10, q.ptr), lambda: c.hvp_dev(v.ptr, hv.ptr),
             lambda: c.precondition_projected_dev(v.ptr, pv.ptr)] + calls
    return calls, lambda: dict(collect_rows(), spmm=B.host(q), hvp=B.host(hv), precondition=B.host(pv))


def _alone(c, D):
    c.set_point(D["Y"])
    B = Plain(c)
    calls, collect = _mixed_calls(c, B, D)
    for call in calls:
        call()
    B.wait()
    res = collect()
    B.free()
    return res


@pytest.mark.parametrize("k1,k2", DUOS, ids=["%s-%s" % m for m in DUOS])
def test_two_handles_two_streams_one_thread(k1, k2):
    REL, _ = _bounds()
    sides = [pair(3, 5, JACOBI), pair(2, 2, CHOLESKY)]
    wants = [reference(("alone", i), lambda: _alone(r.h, D)) for i, (t, r, D) in enumerate(sides)]
    gates, lists, collects = [], [], []
    for (t, r, D), kind in zip(sides, (k1, k2)):
        s = on(t, kind)
        t.h.set_point(D["Y"])
        B = Gate(t.h, s)
        calls, collect = _mixed_calls(t.h, B, D)
        gates.append(B)
        lists.append(calls)
        collects.append(collect)
    for B in gates:
        B.open()
    for one, two in zip(*lists):   # alternately, no host wait until the end
        one()
        two()
    for B in gates:
        B.snapshot()
    for B in gates:
        B.wait()
    for (t, r, D), collect, want, kind in zip(sides, collects, wants, (k1, k2)):
        got = collect()
        assert same(got, want), (kind, differing(got, want))
        assert relerr(got["hvp"], orc.hvp(t.Q, t.dims, D["Y"], orc.egrad(t.Q, D["Y"]), D["V"])) < REL


if __name__ == "__main__" and sys.argv[1:] == ["sweep"]:
    sweep_main()
