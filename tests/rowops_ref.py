"""Plain high-precision references of the row-unit, reduction and block operations (cora_amd/csrc/kernels/rows.inc), and
the catalogue of d x p blocks the polar-factor tests run on.  No GPU, no library: mpmath for the polar factor,
np.longdouble for everything that is a sum of products, exact rational arithmetic for a single fused multiply-add.

Conventions: a pose block is d x p with the pose's d rows as its rows (rows of the N x p matrix), so a point of the
manifold has blocks with orthonormal ROWS; eps = 2^-52; the error of a polar factor is the largest |entry| of the
difference to polar(), in units of eps * kappa_polar(singular values)."""
import functools
from fractions import Fraction

import mpmath
import numpy as np

EPS = float(np.finfo(np.float64).eps)
MP_DIGITS = 45
LD = np.longdouble

# Calibration (tests/test_rowops_ref_cpu.py::test_calibration, figures in profiles/rowops.md): the worst error of the
# reference's own float64 route -- thin SVD, U @ Vt: numpy here, Eigen::JacobiSVD in src/StiefelProduct.cpp:8-36 -- over
# every block of the catalogue at every (d, p) of the GPU test.  The GPU test allows TWICE these.
REF_POLAR_WORST = 14.4      # eps * kappa_polar: measured 14.312 (d = 3; 2.390 at d = 2); test_calibration fails above it
REF_ORTH_WORST = 1.78e-15   # max |U U^T - I|: measured 1.776e-15 at both d
POLAR_BOUND = 2.0 * REF_POLAR_WORST
ORTH_BOUND = 2.0 * REF_ORTH_WORST


# --------------------------------------------------------------------------------------------------------------------
# polar factor
# --------------------------------------------------------------------------------------------------------------------
def polar(block):
    """(P, sigma): P = float64 rounding of the polar factor U V^T of a d x p block (d <= p, full rank) from mpmath's
    svd_r at MP_DIGITS digits, sigma = its singular values (descending, float64)."""
    A = np.asarray(block, dtype=np.float64)
    d, p = A.shape
    with mpmath.workdps(MP_DIGITS):
        # svd_r of the tall transpose (p x d) is the cheaper orientation: A^T = U S V  =>  polar(A) = (U V)^T
        U, S, V = mpmath.svd_r(mpmath.matrix(A.T.tolist()), full_matrices=False)
        P = (U * V).T
        out = np.array([[float(P[i, j]) for j in range(p)] for i in range(d)])
        sig = np.array(sorted((float(S[i]) for i in range(d)), reverse=True))
    return out, sig


def kappa_polar(sig, p):
    """Condition number of the polar factor of a d x p block with singular values sig (descending)."""
    d = len(sig)
    if p > d or d == 1:
        return sig[0] / sig[-1]
    return 2.0 * sig[0] / (sig[-1] + sig[-2])


def polar_error(got, ref, sig):
    """max |got - ref| in units of eps * kappa_polar."""
    return float(np.abs(got - ref).max()) / (EPS * kappa_polar(sig, got.shape[1]))


def orth_error(U):
    return float(np.abs(U @ U.T - np.eye(U.shape[0])).max())


def svd_route(block):
    """The reference's own route in float64: U @ Vt of the thin SVD."""
    u, _, vt = np.linalg.svd(np.asarray(block, dtype=np.float64), full_matrices=False)
    return u @ vt


# --------------------------------------------------------------------------------------------------------------------
# block families: name -> parameter values; every block is a function of (name, parameter index, d, p, seed) only
# --------------------------------------------------------------------------------------------------------------------
FAMILIES = {
    "cond": (1.0, 1e3, 1e6, 1e9, 1e12),          # U diag(logspace(0, -log10 kappa)) V^T
    "orthonormal": (None,),                      # already a point of the manifold
    "equal_norm": (None,),                       # two rows of bitwise equal squared norm: zeta == +-0
    "parallel": (1e-7,),                         # angle between the first two rows
    "identity_noise": (1e-17,),                  # I plus off-diagonal noise: gamma tiny, zeta overflows or is 0 / gamma
    "reflection": (None,),                       # p == d only: det < 0
    "retract": (0.0, 1e-8, 1.0, 1e4, 1e8),       # orthonormal Y plus alpha V
    "scaled": (1e-160, 1e-100, 1e-60, 1e60, 1e100, 1e160),   # a kappa = 10 block times s
}
_FAMILY_ID = {name: i for i, name in enumerate(FAMILIES)}


def _orthonormal_rows(rng, d, p):
    q, _ = np.linalg.qr(rng.standard_normal((p, d)))
    return q.T


def _cond_block(rng, d, p, kappa):
    u, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return (u * np.logspace(0.0, -np.log10(kappa), d)) @ _orthonormal_rows(rng, d, p)


def scaled_base(d, p, seed):
    """The kappa = 10 block that `scaled` multiplies (the scale-invariant input of the calibration)."""
    return _cond_block(np.random.default_rng([_FAMILY_ID["scaled"], d, p, seed]), d, p, 10.0)


@functools.lru_cache(maxsize=None)
def _block(name, k, d, p, seed):
    par = FAMILIES[name][k]
    rng = np.random.default_rng([_FAMILY_ID[name], k, d, p, seed])
    if name == "cond":
        B = _cond_block(rng, d, p, par)
    elif name == "orthonormal":
        B = _orthonormal_rows(rng, d, p)
    elif name == "equal_norm":
        B = rng.uniform(-1, 1, (d, p))
        sign = np.ones(p)
        sign[rng.permutation(p)[:max(1, p // 2)]] = -1.0     # at least one of each sign (p >= 2): the rows differ
        B[1] = B[0] * sign
    elif name == "parallel":
        B = rng.uniform(-1, 1, (d, p))
        u = B[0] / np.linalg.norm(B[0])
        w = rng.standard_normal(p)
        w -= (w @ u) * u
        w /= np.linalg.norm(w)
        B[1] = 0.7 * (np.cos(par) * u + np.sin(par) * w)
    elif name == "identity_noise":
        B = np.eye(d, p) + par * rng.standard_normal((d, p)) * (1.0 - np.eye(d, p))
    elif name == "reflection":
        assert p == d
        B = rng.uniform(-1, 1, (d, d))
        if np.linalg.det(B) > 0:
            B[0] = -B[0]
    elif name == "retract":
        B = _orthonormal_rows(rng, d, p) + par * rng.standard_normal((d, p))
    elif name == "scaled":
        B = scaled_base(d, p, seed) * par
    else:
        raise KeyError(name)
    B.setflags(write=False)
    return B


def block(name, k, d, p, seed=0):
    """Block `seed` of family `name` at its k-th parameter value (read-only, shared)."""
    return _block(name, int(k), int(d), int(p), int(seed))


@functools.lru_cache(maxsize=None)
def block_polar(name, k, d, p, seed=0):
    """polar() of block(...), computed once per process (the CPU and the GPU tests share it)."""
    P, sig = polar(block(name, k, d, p, seed))
    P.setflags(write=False)
    sig.setflags(write=False)
    return P, sig


@functools.lru_cache(maxsize=None)
def base_polar(d, p, seed=0):
    """polar() of scaled_base(...), once per process."""
    return polar(scaled_base(d, p, seed))


def catalogue(d, p):
    """[(name, k, seed)] of every block the tests use at (d, p): every parameter value of the families that have
    several, two seeds of the others."""
    out = []
    for name, pars in FAMILIES.items():
        if name == "reflection" and p != d:
            continue
        for k in range(len(pars)):
            for seed in ((0,) if len(pars) > 1 else (0, 1)):
                out.append((name, k, seed))
    return out


def strides(d):
    """Every compiled row stride at dimension d."""
    return list(range(d, 25))


# --------------------------------------------------------------------------------------------------------------------
# whole N x p matrices: rows [0, d n) pose blocks, [d n, d n + r) range rows, then nt translation rows
# --------------------------------------------------------------------------------------------------------------------
def fma(a, x, y):
    """round(a * x + y) with ONE rounding, elementwise (exact rational arithmetic; small arrays only)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    fa = Fraction(float(a))
    out = np.empty(x.shape)
    for idx in np.ndindex(x.shape):
        out[idx] = float(fa * Fraction(float(x[idx])) + Fraction(float(y[idx])))
    return out


def unit_rows(A):
    """Rows of A normalised in longdouble (after an exact power-of-two scaling, so that no square leaves the range)."""
    A = np.asarray(A, dtype=np.float64)
    m, e = np.frexp(np.abs(A).max(axis=1, keepdims=True))
    S = np.ldexp(A, -e).astype(LD)
    nrm = np.sqrt((S * S).sum(axis=1, keepdims=True))
    return np.where(nrm > 0, S / np.where(nrm > 0, nrm, 1), S).astype(np.float64)


def project_manifold(A, d, n, r, nt, polar_fn=None):
    """projectToManifold of an N x p matrix: polar factor of every pose block (polar_fn(i, block) -> d x p, default
    polar()), unit range rows, translation rows unchanged."""
    A = np.asarray(A, dtype=np.float64)
    out = A.copy()
    for i in range(n):
        blk = A[d * i:d * i + d]
        out[d * i:d * i + d] = polar(blk)[0] if polar_fn is None else polar_fn(i, blk)
    if r:
        out[d * n:d * n + r] = unit_rows(A[d * n:d * n + r])
    return out


def retract(Y, V, alpha, d, n, r, nt, polar_fn=None):
    """projectToManifold(fma(alpha, V, Y))."""
    return project_manifold(fma(alpha, V, Y), d, n, r, nt, polar_fn)


def tangent_proj(Y, V, d, n, r, nt):
    """Proj_Y(V) in longdouble, rounded once: V_i - sym(V_i Y_i^T) Y_i per pose block, v - <y, v> y per range row,
    translation rows unchanged."""
    Yl, Vl = np.asarray(Y, dtype=np.float64).astype(LD), np.asarray(V, dtype=np.float64).astype(LD)
    out = Vl.copy()
    for i in range(n):
        y, v = Yl[d * i:d * i + d], Vl[d * i:d * i + d]
        m = v @ y.T
        out[d * i:d * i + d] = v - (0.5 * (m + m.T)) @ y
    if r:
        y, v = Yl[d * n:d * n + r], Vl[d * n:d * n + r]
        out[d * n:d * n + r] = v - (y * v).sum(axis=1, keepdims=True) * y
    return out.astype(np.float64)


# --------------------------------------------------------------------------------------------------------------------
# sums of products, with the magnitude sums their forward-error bounds need
# --------------------------------------------------------------------------------------------------------------------
def dot(a, b):
    """(sum a_i b_i, sum |a_i b_i|) in longdouble over all entries."""
    pr = np.asarray(a, dtype=np.float64).astype(LD).ravel() * np.asarray(b, dtype=np.float64).astype(LD).ravel()
    return float(pr.sum()), float(np.abs(pr).sum())


def gram(A, B):
    """(A^T B, |A|^T |B|) in longdouble."""
    Al, Bl = np.asarray(A, dtype=np.float64).astype(LD), np.asarray(B, dtype=np.float64).astype(LD)
    return (Al.T @ Bl).astype(np.float64), (np.abs(Al).T @ np.abs(Bl)).astype(np.float64)


def combine(Xs, Cs):
    """(sum_i X_i C_i, sum_i |X_i| |C_i|) in longdouble."""
    tot = mag = 0
    for X, Cm in zip(Xs, Cs):
        Xl, Cl = np.asarray(X, dtype=np.float64).astype(LD), np.asarray(Cm, dtype=np.float64).astype(LD)
        tot = tot + Xl @ Cl
        mag = mag + np.abs(Xl) @ np.abs(Cl)
    return tot.astype(np.float64), mag.astype(np.float64)
