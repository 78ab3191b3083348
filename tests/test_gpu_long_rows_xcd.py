"""The long rows through their device image (cora_amd/csrc/long_image.h: a row's entries sorted by the XCD whose slices
read the column, cut into pieces, every piece launched on that XCD) on the graphs of tests/long_rows_graphs.py -- rows of
several pieces on some XCDs only (`random`), runs cut again at the piece size (`cut`), a row of one piece (`single`).

Q X at 2, 5 and 10 columns, the Hvp at p = 3 and 5 and the certificate operator at 10 columns against the oracle, 1e-10 of
the largest entry (test_gpu_parity.REL); two interior iterations of cora_stpcg_warm_dev against tests/stpcg_ref.py within
the bounds of test_gpu_stpcg_forms (the long rows' own kappa slots of EPI_HVP_K: a wrong kappa leaves Hp right and moves s
and r); five launches of every product bit for bit; new values on a live handle against a handle created from them, bit
for bit."""
import numpy as np
import pytest

import long_rows_graphs as lrg
import stpcg_ref as ref
from cora_amd import capi
from oracle import oracle as orc
from test_update_values_cpu import pair_factors

pytestmark = pytest.mark.gpu
REL = 1e-10                          # test_gpu_parity.REL
STPCG = {"prod": 1e-10, "vec": 1e-9}  # test_gpu_stpcg_forms.BOUND
FAR, NO_TARGET, MARGIN = 1e30, 1e-300, 1e-3   # topologies_worker
KS, PS, K_CERT = (2, 5, 10), (3, 5), 10


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


_REFS = {}


def references(name):
    """Operands and the oracle's products of a graph, computed once and left unchanged."""
    if name not in _REFS:
        A, Q, dm = lrg.build(name)
        rng = np.random.default_rng(31)
        R = dict(X={k: rng.standard_normal((dm.N, k)) for k in KS}, Y={}, V={}, hv={}, grad={})
        R["qx"] = {k: orc.spmm(Q, R["X"][k]) for k in KS}
        for p in PS:
            Y = lrg.near_truth(name, p)
            G = orc.egrad(Q, Y)
            R["Y"][p], R["V"][p] = Y, orc.tangent_proj(dm, Y, rng.uniform(-1, 1, (dm.N, p)))
            R["hv"][p] = orc.hvp(Q, dm, Y, G, R["V"][p])
            R["grad"][p] = (G, orc.tangent_proj(dm, Y, G))
        st, ob = orc.lambda_blocks(Q, dm, R["Y"][5])
        R["sx"] = orc.S_apply(Q, dm, st, ob, R["X"][K_CERT])
        _REFS[name] = R
    return _REFS[name]


def handle(Q, dm, vals=None):
    return capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val if vals is None else vals)


def products(c, dm, R, repeat=1):
    """{what: [result of every launch]}: Q X at KS, the Hvp at PS (the point near the truth), (Q - Lambda) X at the point
    of p = 5."""
    out = {}
    for k in KS:
        x, o = c.dev_alloc(k), c.dev_alloc(k)
        c.upload(R["X"][k], x)
        out["qx%d" % k] = []
        for _ in range(repeat):
            c.spmm_dev(x, k, o)
            out["qx%d" % k].append(c.download(o, k))
    for p in PS:
        c.set_rank(p)
        y, x, o = c.dev_alloc(p), c.dev_alloc(p), c.dev_alloc(p)
        c.upload(R["Y"][p], y)
        c.set_point_dev(y)
        c.upload(R["V"][p], x)
        out["hvp%d" % p] = []
        for _ in range(repeat):
            c.hvp_dev(x, o)
            out["hvp%d" % p].append(c.download(o, p))
    x, o = c.dev_alloc(K_CERT), c.dev_alloc(K_CERT)   # (the handle is at p = 5 and its point)
    c.upload(R["X"][K_CERT], x)
    out["cert"] = []
    for _ in range(repeat):
        c.certificate_product_dev(x, K_CERT, o)
        out["cert"].append(c.download(o, K_CERT))
    return out


@pytest.mark.parametrize("name", lrg.NAMES)
def test_products_against_the_oracle_and_bit_for_bit(name):
    A, Q, dm = lrg.build(name)
    R = references(name)
    c = handle(Q, dm)
    out = products(c, dm, R, repeat=5)
    c.close()
    want = {"qx%d" % k: R["qx"][k] for k in KS}
    want.update({"hvp%d" % p: R["hv"][p] for p in PS})
    want["cert"] = R["sx"]
    for what, runs in out.items():
        err = relerr(runs[0], want[what])
        print("%s %s: %.2e" % (name, what, err))
        assert err < REL, what
        for again in runs[1:]:
            assert np.array_equal(again, runs[0]), what


@pytest.mark.parametrize("name", lrg.NAMES)
def test_warm_stpcg_takes_the_reference_iterations(name):
    A, Q, dm = lrg.build(name)
    R = references(name)
    p = 5
    Y, (G, grad) = R["Y"][p], R["grad"][p]
    states, how = ref.stpcg(lambda W: orc.hvp(Q, dm, Y, G, W), lambda W: orc.tangent_proj(dm, Y, W), grad, FAR, NO_TARGET,
                            0.0, 2)
    assert how == "limit" and len(states) == 2
    for st in states:   # interior steps with clearly positive curvature: kappa decides s and r
        assert st["kappa"] > 0 and st["kappa_rel"] >= MARGIN and st["sig_next"] < FAR * FAR
    c = handle(Q, dm)
    c.set_rank(p)
    y, gr, pg, s, r, v, pk, hp = (c.dev_alloc(p) for _ in range(8))
    c.upload(Y, y)
    c.set_point_dev(y)
    c.upload(grad, gr)
    c.precond_setup(capi.PRECOND_NONE)
    c.precondition_projected_dev(gr, pg)
    g_g, g_pg = c.dot_dev(gr, gr, p), c.dot_dev(gr, pg, p)
    prev = states[0]["p_prev"]
    for k, st in enumerate(states, 1):
        it, sM = c.stpcg_warm_dev(gr, pg, g_g, g_pg, FAR, s, r, v, pk, hp, kappa_fgr=NO_TARGET, theta=0.0, max_iters=k)
        assert it == k
        Hp = c.download(hp, p)
        for what, got, want, kind in (("s", c.download(s, p), st["s"], "vec"), ("r", c.download(r, p), st["r"], "vec"),
                                      ("Hp.ref", Hp, st["Hp"], "vec"), ("Hp", Hp, orc.hvp(Q, dm, Y, G, prev), "prod")):
            assert np.all(np.isfinite(got)), what
            for cls, e in ref.class_errors(dm, got, want).items():
                print("%s %s%d.%s: %.2e" % (name, what, k, cls, e))
                assert e <= STPCG[kind], (what, k, cls)
        assert abs(sM - st["sM"]) <= STPCG["vec"] * st["sM"]
        prev = c.download(pk, p)
    c.close()


@pytest.mark.parametrize("name", lrg.NAMES)
def test_new_values_on_a_live_handle(name):
    A, Q, dm = lrg.build(name)
    R = references(name)
    vals2 = np.asarray(Q.val, dtype=np.float64) * pair_factors(Q.rowptr, Q.col)
    live, fresh = handle(Q, dm), handle(Q, dm, vals2)
    before = products(live, dm, R)
    live.update_values(Q.rowptr, Q.col, vals2)
    after, want = products(live, dm, R), products(fresh, dm, R)
    live.close()
    fresh.close()
    for what in want:
        assert not np.array_equal(before[what][0], want[what][0]), what
        assert np.array_equal(after[what][0], want[what][0]), what
