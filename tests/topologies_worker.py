"""Device side of tests/test_gpu_topologies.py: one catalogue entry of tests/topologies.py at one row stride on one
handle, every operator against the CPU oracle, and the references those comparisons share.

`measure` is called in process by the tests and, for the plain layout, by this file run as a program:
`topologies_worker.py plain` (started with CORA_CHAIN_SLICES=0, which the library reads once when it loads) prints one
`CASE <json>` line per (entry, stride) and `DONE`.  Any error of the library (a HIP error among them) is an exception
that nothing catches: the exit status is non-zero."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import stpcg_ref as ref   # noqa: E402
import topologies as topo   # noqa: E402
from oracle import oracle as orc   # noqa: E402

FORMS = (("window", 0), ("gather", 1 << 30))   # cora_debug_spmm_window_min_slices: LDS windows always / never
# one row stride per compile-time regime of pose_slice (cora_amd/csrc/kernels/spmm.inc): p = d, kEarly / kFuseT, kNxtRegs,
# kCoopT (D LD <= 18), the translation window (LD <= 8), kStaged (LD <= 9), one wavefront per SIMD, an odd wide stride,
# the widest
WIDE_STRIDES = (5, 6, 7, 9, 10, 13, 24)
KAPPA_MAX_P = 12    # the device-resident STPCG's fused passes (test_gpu_parity.test_window_form_of_every_row_stride)
FAR = 1e30          # a radius no step reaches
NO_TARGET = 1e-300  # a residual target no iteration reaches
MARGIN = 1e-3       # the reference's curvature <p, Hp> / (|p| |Hp|) stays this far above zero (stpcg_forms_worker.MARGIN)
PLAIN_ENTRIES = ("robots-d2", "robots-d3")


def strides(d):
    return (d,) + WIDE_STRIDES


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def class_errors(dm, got, want):
    """stpcg_ref.class_errors over the row classes the graph has (no landmark-free or range-free division by zero)."""
    out = {}
    for name, (lo, hi) in ref.row_classes(dm).items():
        if hi > lo:
            den = float(np.abs(want[lo:hi]).max())
            num = float(np.abs(got[lo:hi] - want[lo:hi]).max())
            out[name] = num / den if den > 0 else (0.0 if num == 0 else float("inf"))
    return out


_REFS = {}


def references(name, p):
    """Everything the comparisons of (entry, p) need from the oracle, computed once per process and left unchanged."""
    key = (name, p)
    if key not in _REFS:
        A, Q, dm, g = topo.build(name)
        rng = np.random.default_rng(7000 + p)
        Y = topo.near_truth(name, p)
        G = orc.egrad(Q, Y)
        V = orc.tangent_proj(dm, Y, rng.uniform(-1, 1, (dm.N, p)))
        X = rng.standard_normal((dm.N, p))
        st, ob = orc.lambda_blocks(Q, dm, Y)
        R = dict(Y=Y, G=G, V=V, X=X, st=st, ob=ob, qx=orc.spmm(Q, X), sx=orc.S_apply(Q, dm, st, ob, X),
                 hv=orc.hvp(Q, dm, Y, G, V))
        if p <= KAPPA_MAX_P:
            R["grad"] = orc.tangent_proj(dm, Y, G)
            R["states"], R["exit"] = ref.stpcg(lambda W: orc.hvp(Q, dm, Y, G, W), lambda W: orc.tangent_proj(dm, Y, W),
                                               R["grad"], FAR, NO_TARGET, 0.0, 2)
        _REFS[key] = R
    return _REFS[key]


def interior(R):
    """Why the reference did NOT take two interior steps with clearly positive curvature, or None."""
    if R["exit"] != "limit" or len(R["states"]) != 2:
        return "exit %s after %d iterations" % (R["exit"], len(R["states"]))
    for k, st in enumerate(R["states"]):
        if not (st["kappa"] > 0 and st["kappa_rel"] >= MARGIN and st["sig_next"] < FAR * FAR):
            return "iteration %d: kappa %.3e, relative %.3e" % (k + 1, st["kappa"], st["kappa_rel"])
    return None


def measure(name, p, L, win):
    """The figures of one handle: dict shape (Context.format_shape + stats), checks [[what, value, kind]] with kind in
    prod | lam | vec (the bounds of tests/test_gpu_topologies.py), fail [discrete mismatches]."""
    from cora_amd import capi
    A, Q, dm, g = topo.build(name)
    R = references(name, p)
    Y, G, V, X = R["Y"], R["G"], R["V"], R["X"]
    checks, fail = [], []
    L.cora_debug_spmm_window_min_slices(win)
    c = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val)
    c.set_rank(p)
    shape = topo.shape_of(c)
    checks.append(["QX", relerr(c.dataMatrixProduct(X), R["qx"]), "prod"])
    st, ob = c.compute_Lambda_blocks(Y)
    checks.append(["Lambda", float(max(np.abs(st - R["st"]).max(initial=0), np.abs(ob - R["ob"]).max(initial=0))), "lam"])
    c.set_point(Y)
    checks.append(["SX", relerr(c.certificate_product(X), R["sx"]), "prod"])
    checks.append(["Hvp", relerr(c.Riemannian_Hessian_vector_product(Y, G, V), R["hv"]), "prod"])
    c.set_point(Y)
    x, o = c.dev_alloc(p), c.dev_alloc(p)
    c.upload(V, x)
    c.hvp_dev(x, o)
    checks.append(["hvp_dev", relerr(c.download(o, p), R["hv"]), "prod"])
    if p <= KAPPA_MAX_P:
        why = interior(R)
        if why:
            fail.append("the reference takes no interior step: " + why)
        y, gr, s, r, v, pk, hp = (c.dev_alloc(p) for _ in range(7))
        c.upload(Y, y)
        c.set_point_dev(y)
        c.upload(R["grad"], gr)
        c.precond_setup(capi.PRECOND_NONE)
        prev = R["states"][0]["p_prev"]
        for k, state in enumerate(R["states"], 1):
            it, sM = c.stpcg_dev(gr, FAR, s, r, v, pk, hp, kappa_fgr=NO_TARGET, theta=0.0, max_iters=k)
            if it != k:
                fail.append("%d iterations where %d were asked for" % (it, k))
            Hp = c.download(hp, p)
            for what, got, want, kind in (("s", c.download(s, p), state["s"], "vec"), ("r", c.download(r, p), state["r"], "vec"),
                                          ("Hp.ref", Hp, state["Hp"], "vec"),
                                          ("Hp", Hp, orc.hvp(Q, dm, Y, G, prev), "prod")):   # of the DEVICE'S direction
                if not np.all(np.isfinite(got)):
                    fail.append("%s after %d holds a non-finite value" % (what, k))
                    continue
                for cls, e in class_errors(dm, got, want).items():
                    checks.append(["%s%d.%s" % (what, k, cls), e, kind])
            checks.append(["sM%d" % k, abs(sM - state["sM"]) / state["sM"], "vec"])
            prev = c.download(pk, p)
    c.close()
    for chk in checks:
        if not np.isfinite(chk[1]):
            fail.append("%s is not finite" % chk[0])
            chk[1] = 1e300
    return dict(shape=shape, checks=checks, fail=fail)


def plain_case_ids():
    return ["%s-p%d-%s" % (name, p, form) for name in PLAIN_ENTRIES for p in strides(topo.CATALOGUE[name][1])
            for form, _ in FORMS]


def main(which):
    from cora_amd import capi
    assert which == "plain" and os.environ.get("CORA_CHAIN_SLICES") == "0"
    L = capi.load()
    for name in PLAIN_ENTRIES:
        for p in strides(topo.CATALOGUE[name][1]):
            for form, win in FORMS:
                out = measure(name, p, L, win)
                print("CASE " + json.dumps(dict(id="%s-p%d-%s" % (name, p, form), **out)), flush=True)
    print("DONE", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
