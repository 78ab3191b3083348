"""The product kernels on graded floating-point data, every entry of every result inside a bound of its own.

The data, the np.longdouble reference, the majorants and the derivation of the bounds |got - ref|_i <= c_i 2^-52 B_i are
tests/spmm_ref.py: weights over 1e-6 .. 1e6, translation rows at 1e3 beside landmark rows at 1e-3, columns over 1e-3 ..
1e3 -- the spread the norm-wise 1e-10 of the other product tests cannot see into (tests/test_spmm_ref_cpu.py shows a
dropped term passing it).  The fp64 oracle and the host executor meet the same bounds there; here the device: Q X, the
Lambda blocks, the cost, (Q - Lambda) X and the Hessian-vector product through the host-pointer and the resident entry
points, in both forms of the pose slices.  Nothing is filtered.  Observed ratios: profiles/spmm_exact.md."""
import functools

import pytest

import spmm_ref as sr
import topologies as topo
import topologies_worker as W
from cora_amd import capi

pytestmark = pytest.mark.gpu

_STATE = {"fatal": None}
CASES = [(name, p) for name in sr.ENTRIES for p in sr.ranks(topo.CATALOGUE[name][1])]


@pytest.fixture(autouse=True)
def device_in_order():
    if _STATE["fatal"]:
        pytest.fail(_STATE["fatal"])


@pytest.fixture
def restore_form():
    L = capi.load()
    old = L.cora_debug_spmm_window_min_slices(0)
    L.cora_debug_spmm_window_min_slices(old)
    yield L
    L.cora_debug_spmm_window_min_slices(old)


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


@pytest.mark.parametrize("name,p", CASES, ids=["%s-p%d" % c for c in CASES])
@_guard
def test_every_entry_is_inside_its_bound(name, p, restore_form):
    R = sr.case(name, p)
    Q, dm, Y, X, V = R["Q"], R["dm"], R["Y"], R["X"], R["V"]
    for form, win in W.FORMS:
        tag = "%s p=%d %s: " % (name, p, form)
        restore_form.cora_debug_spmm_window_min_slices(win)
        c = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val)
        c.set_rank(p)
        worst = {}
        worst["QX"] = sr.check(tag + "Q X", c.dataMatrixProduct(X), *R["qx"])
        st, ob = c.compute_Lambda_blocks(Y)
        worst["Lambda"] = max(sr.check(tag + "Lambda, Stiefel blocks", st, *R["lam_st"]),
                              sr.check(tag + "Lambda, oblique entries", ob, *R["lam_ob"]))
        c.set_point(Y)
        worst["f"] = sr.check(tag + "point_cost", c.point_cost(), *R["f"])
        worst["SX"] = sr.check(tag + "(Q - Lambda) X", c.certificate_product(X), *R["sx"])
        worst["Hvp"] = sr.check(tag + "Hvp, host pointers", c.Riemannian_Hessian_vector_product(Y, R["G"], V), *R["hv"])
        c.set_point(Y)   # (the Hvp with a gradient from outside leaves its own Lambda on the handle)
        x, o = c.dev_alloc(p), c.dev_alloc(p)
        c.upload(V, x)
        c.hvp_dev(x, o)
        worst["hvp_dev"] = sr.check(tag + "hvp_dev", c.download(o, p), *R["hv"])
        c.close()
        print("\nRATIO %s%s" % (tag, "  ".join("%s %.3f" % kv for kv in worst.items())))
