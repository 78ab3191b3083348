"""The numpy STPCG that tests/test_gpu_stpcg_forms.py compares the device with (tests/stpcg_ref.py) against the oracle's
own restatement of the algorithm (oracle/tnt.py::stpcg), which only returns the step: same step, M-norm and iteration count
under each of the four ways out of the loop, and a refined Cholesky solve whose residual is at rounding level."""
import math

import numpy as np
import pytest

import stpcg_ref as ref
from oracle import oracle as orc
from oracle import tnt as otnt
from synth import make_problem


@pytest.fixture(scope="module")
def small():
    _, Q, dm = make_problem(d=3, n=60, n_landmarks=3, n_ranges=40, n_loops=3, seed=4)
    far = orc.project_manifold(dm, np.random.default_rng(1).uniform(-1, 1, (dm.N, 5)))
    Y = otnt.tnt(Q, dm, far, max_iterations=12)["x"]   # a dozen outer iterations in: ordinary iterations, positive curvature
    return _at(Q, dm, Y), _at(Q, dm, far)


def _at(Q, dm, Y):
    G = orc.egrad(Q, Y)
    hess = lambda V: orc.hvp(Q, dm, Y, G, V)  # noqa: E731
    precon = lambda V: orc.precond_jacobi(Q, dm, Y, V)  # noqa: E731
    return Q, dm, Y, hess, precon, orc.tangent_proj(dm, Y, G)


def _both(small, Delta, kappa_fgr, k):
    _, dm, _, hess, precon, g = small
    states, how = ref.stpcg(hess, precon, g, Delta, kappa_fgr, 0.0, k)
    s, sM, it = otnt.stpcg(hess, precon, g, Delta, dict(kappa_fgr=kappa_fgr, theta=0.0, max_TPCG_iterations=k))
    assert it == len(states)
    assert abs(sM - states[-1]["sM"]) <= 1e-12 * sM
    assert max(ref.class_errors(dm, states[-1]["s"], s).values()) < 1e-11
    return states, how


def test_reference_takes_the_oracles_exits(small):
    small, far = small
    # non-positive curvature: a random point of the manifold (the Hessian is indefinite there)
    states, how = _both(far, 1e30, 1e-300, 6)
    assert how == "curvature" and not states[-1]["kappa"] > 0 and all(st["kappa"] > 0 for st in states[:-1])
    base, how = _both(small, 1e30, 1e-300, 6)
    assert how == "limit" and len(base) == 6 and all(st["kappa"] > 0 for st in base)
    n_ok = len(base)
    # the boundary between the first two steps' M-norms: iteration 2 crosses it
    D = math.sqrt(0.5 * (base[0]["sig_next"] + base[1]["sig_next"]))
    states, how = _both(small, D, 1e-300, 6)
    assert (how, len(states)) == ("boundary", 2) and states[-1]["sM"] == D
    # a residual target between |r_1| and |r_2|, where the residual falls
    r = [base[0]["r0"]] + [math.sqrt(st["rr"]) for st in base[:n_ok]]
    k = next(i for i in range(1, len(r)) if r[i] < min(r[:i]))
    states, how = _both(small, 1e30, math.sqrt(r[k] * min(r[:k])) / r[0], 6)
    assert (how, len(states)) == ("target", k)
    # the limit
    states, how = _both(small, 1e30, 1e-300, 1)
    assert (how, len(states)) == ("limit", 1)
    # the state is the device's: p is the NEW direction, Hp the product of the one the iteration started with
    st = states[0]
    assert np.array_equal(st["p"], -st["v"] + st["beta"] * st["p_prev"]) and np.array_equal(st["Hp"], small[3](st["p_prev"]))


def test_refined_cholesky_solve(small):
    Q, dm, Y = small[0][:3]
    lam = 1e-6 * abs(Q.val).max()
    c = ref.RegularizedCholesky(Q, dm, lam)
    plain = ref.RegularizedCholesky(Q, dm, lam, plain=True)
    V = np.asfortranarray(np.random.default_rng(2).standard_normal((dm.N, 5)))
    x = c.full_solve(V)
    assert np.all(x[-1] == 0.0)
    # residual at the level of one rounding of the products it is made of, and no worse than the unrefined solve's
    scale = abs(c.M).max() * np.abs(x).max()
    res = float(np.abs(c.residual(x[:-1], V[:-1])).max()) / scale
    res_plain = float(np.abs(c.residual(plain.full_solve(V)[:-1], V[:-1])).max()) / scale
    print("residual / (|M| |x|): refined %.2e, plain %.2e" % (res, res_plain))
    assert res < 4 * np.finfo(float).eps and res <= res_plain
    assert max(ref.class_errors(dm, c.precond(Y, V), orc.tangent_proj(dm, Y, x)).values()) == 0.0
