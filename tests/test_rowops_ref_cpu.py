"""The references of tests/rowops_ref.py against the oracle, the calibration of the polar-factor tolerances on the
reference's own float64 route, and the block catalogue against its own description.  No GPU."""
import numpy as np
import pytest

import rowops_ref as rr
from oracle import oracle as orc


def _dims(d, n, r, nt):
    return orc.Dims(d, n, r, d * n + r + nt)


@pytest.mark.parametrize("d,p", [(2, 2), (2, 5), (3, 3), (3, 7), (3, 24)])
def test_references_agree_with_oracle(d, p):
    n, r, nt = 6, 5, 8
    dm = _dims(d, n, r, nt)
    rng = np.random.default_rng(100 * d + p)
    A = rng.uniform(-1, 1, (dm.N, p))
    Y = rr.project_manifold(A, d, n, r, nt)
    assert np.abs(Y - orc.project_manifold(dm, A)).max() < 1e-13
    V = rng.standard_normal((dm.N, p))
    T = rr.tangent_proj(Y, V, d, n, r, nt)
    assert np.abs(T - orc.tangent_proj(dm, Y, V)).max() < 1e-13
    R = rr.retract(Y, T, 0.3, d, n, r, nt)
    assert np.abs(R - orc.retract(dm, Y, 0.3 * T)).max() < 1e-13
    v, mag = rr.dot(V, T)
    assert abs(v - orc.inner(V, T)) < 1e-13 * mag
    G, Gm = rr.gram(V, T)
    assert np.all(np.abs(G - V.T @ T) <= 1e-13 * Gm)
    C1, C2 = rng.standard_normal((p, 3)), rng.standard_normal((p, 3))
    O, Om = rr.combine([V, T], [C1, C2])
    assert np.all(np.abs(O - (V @ C1 + T @ C2)) <= 1e-13 * Om)


def test_fma_rounds_once():
    # (1 + 2^-27)^2 + 2^-53 = 1 + 2^-26 + 3/4 ulp: one rounding goes up, product-then-sum goes 1/4 ulp down, then a tie to even
    a = 1.0 + 2.0 ** -27
    assert a * a + 2.0 ** -53 == 1.0 + 2.0 ** -26
    assert rr.fma(a, np.array([a]), np.array([2.0 ** -53]))[0] == 1.0 + 2.0 ** -26 + 2.0 ** -52
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(50), rng.standard_normal(50)
    assert np.array_equal(rr.fma(4.0, x, y), 4.0 * x + y)     # a power of two: the product is exact


def test_unit_rows_at_every_scale():
    rng = np.random.default_rng(1)
    base = rng.uniform(-1, 1, (7, 5))
    for s in (1e-300, 1e-160, 1.0, 1e160, 1e300):
        U = rr.unit_rows(base * s)
        assert np.abs(np.sqrt((U.astype(rr.LD) ** 2).sum(axis=1)) - 1).max() < 2 * rr.EPS
    assert np.array_equal(rr.unit_rows(np.zeros((2, 3))), np.zeros((2, 3)))


@pytest.mark.parametrize("d", [2, 3])
def test_calibration(d, record_property):
    """The reference's own route (float64 thin SVD, U @ Vt) on every block the GPU test uses, on the scale-invariant
    input: its worst error against polar() and its worst departure from orthonormality are what the GPU tolerances are
    twice of (rowops_ref.REF_POLAR_WORST, REF_ORTH_WORST; profiles/rowops.md)."""
    worst, worst_at, orth, orth_at = 0.0, None, 0.0, None
    for p in rr.strides(d):
        for name, k, seed in rr.catalogue(d, p):
            B = rr.scaled_base(d, p, seed) if name == "scaled" else rr.block(name, k, d, p, seed)
            P, sig = rr.base_polar(d, p, seed) if name == "scaled" else rr.block_polar(name, k, d, p, seed)
            got = rr.svd_route(B)
            e, o = rr.polar_error(got, P, sig), rr.orth_error(got)
            if e > worst:
                worst, worst_at = e, (name, k, p, seed)
            if o > orth:
                orth, orth_at = o, (name, k, p, seed)
    print("d=%d: float64 SVD route, worst polar error %.3f eps*kappa at %s, worst |UU^T - I| %.3e at %s"
          % (d, worst, worst_at, orth, orth_at))
    record_property("polar_worst", worst)
    record_property("orth_worst", orth)
    assert worst <= rr.REF_POLAR_WORST, (worst, worst_at)
    assert orth <= rr.REF_ORTH_WORST, (orth, orth_at)
    assert rr.POLAR_BOUND == 2 * rr.REF_POLAR_WORST and rr.ORTH_BOUND == 2 * rr.REF_ORTH_WORST


@pytest.mark.parametrize("d,p", [(2, 2), (2, 3), (3, 3), (3, 5), (3, 24)])
def test_catalogue_is_what_it_claims(d, p):
    names = {name for name, _, _ in rr.catalogue(d, p)}
    assert names == set(rr.FAMILIES) - (set() if p == d else {"reflection"})
    for k, kappa in enumerate(rr.FAMILIES["cond"]):
        _, sig = rr.block_polar("cond", k, d, p, 0)
        assert abs(sig[0] / sig[-1] / kappa - 1) < 0.01
    for seed in (0, 1):
        B = rr.block("orthonormal", 0, d, p, seed)
        assert rr.orth_error(B) < 8 * rr.EPS
        B = rr.block("equal_norm", 0, d, p, seed)
        sq = [sum(x * x for x in row) for row in B[:2].tolist()]       # any order of summation: the squares are equal
        assert sq[0] == sq[1] and np.dot(B[0], B[0]) == np.dot(B[1], B[1])
        assert not np.array_equal(B[0], B[1]) and np.dot(B[0], B[1]) != 0.0
        B = rr.block("parallel", 0, d, p, seed)
        u, w = (x.astype(rr.LD) / np.sqrt((x.astype(rr.LD) ** 2).sum()) for x in B[:2])
        ang = float(np.sqrt(((u - w) ** 2).sum()))      # chord of the unit vectors = the angle, to second order
        assert abs(ang / 1e-7 - 1) < 0.01
        B = rr.block("identity_noise", 0, d, p, seed)
        off = B - np.eye(d, p)
        assert np.array_equal(np.diag(B), np.ones(d)) and 0 < np.abs(off).max() < 1e-16
        if p == d:
            assert np.linalg.det(rr.block("reflection", 0, d, p, seed)) < 0
    for k, alpha in enumerate(rr.FAMILIES["retract"]):
        B = rr.block("retract", k, d, p, 0)
        if alpha == 0:
            assert rr.orth_error(B) < 8 * rr.EPS
    for k, s in enumerate(rr.FAMILIES["scaled"]):
        B, base = rr.block("scaled", k, d, p, 0), rr.scaled_base(d, p, 0)
        assert np.array_equal(B, base * s)
        _, sig = rr.base_polar(d, p, 0)
        assert abs(sig[0] / sig[-1] / 10 - 1) < 0.01
        assert abs(np.abs(B).max() / (np.abs(base).max() * s) - 1) < 1e-15


def test_polar_is_scale_invariant_and_memoised():
    B = rr.scaled_base(3, 5, 0)
    P, sig = rr.polar(B)
    for k, s in enumerate(rr.FAMILIES["scaled"]):
        Ps, sigs = rr.block_polar("scaled", k, 3, 5, 0)
        assert np.abs(Ps - P).max() < 4 * rr.EPS and np.abs(sigs / (sig * s) - 1).max() < 4 * rr.EPS
        assert rr.block_polar("scaled", k, 3, 5, 0)[0] is Ps
