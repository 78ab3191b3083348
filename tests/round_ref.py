"""The rounding of include/cora_hip.h (cora_round_dev) restated without the library: the projection of a d x d block to
SO(d) from mpmath's svd_r at rowops_ref.MP_DIGITS digits, the products, the Gram matrix and the normalisation in
np.longdouble, the error measure and its calibrated bound, and the inputs the tests use.  API row order: d n rotation
rows, r range rows, n + l translation rows.

Error measure of a pose block: the largest |entry| of the difference to so_project(Y_i Vd) in units of
eps kappa + (k + 2) eps max(|Y_i| |Vd|) kappa / sigma_1 -- the conditioning of the projection, kappa =
2 sigma_1 / (sigma_{d-1} + s sigma_d) of M_i = Y_i Vd with s the sign of det(M_i), plus the forward error of the product
carried through the same conditioning."""
import functools

import mpmath
import numpy as np

import rowops_ref as ro

EPS = ro.EPS
LD = ro.LD
KS = lambda d: sorted({d, d + 1, 5, 8, 13, 24})  # noqa: E731  (the column counts every test runs at)

# Calibration (tests/test_round_cpu.py::test_calibration, figures in profiles/round.md): the worst error of the float64
# route -- Y_i @ Vd, numpy.linalg.svd, U diag(1, .., det(U Vt)) Vt -- over every block of rowops_ref's catalogue at (d, d),
# lifted to every k of KS(d).  The library is allowed TWICE this, the margin POLAR_BOUND gives polar_rows.
REF_ROUND_WORST = 0.37      # measured 0.366 (d = 3; 0.304 at d = 2); test_calibration fails above it
ROUND_BOUND = 2.0 * REF_ROUND_WORST
# The same for the singular values (test_calibration_of_the_singular_values): the worst error of numpy's eigh on the float64
# Gram matrix Y^T Y against eigh on the longdouble one, in units of eps sigma_1^2 / sigma, over every input of the host-mirror
# tests.  One unit cannot hold: a float64 Gram matrix of N rows carries a rounding error of its own in every entry.
REF_SIGMA_WORST = 3.0       # measured 2.961; test_calibration_of_the_singular_values fails above it
SIGMA_BOUND = 2.0 * REF_SIGMA_WORST
ORTH_BOUND = ro.ORTH_BOUND


def rows(d, n, r, nt):
    """(rotation rows [n, d], range rows [r], translation rows [nt]) in API order."""
    return np.arange(d * n).reshape(n, d), d * n + np.arange(r), d * n + r + np.arange(nt)


def _mpf(x):
    """An np.longdouble as an mpf, exactly (two float64 pieces)."""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def so_project(M):
    """(R, sigma, s): the float64 rounding of the R in SO(d) that maximises tr(R^T M) -- U diag(1, .., 1, det(U V)) V of
    svd_r at MP_DIGITS digits --, the singular values (descending, float64) and s = det(U V) = the sign of det(M).
    M: d x d, float64 or longdouble."""
    M = np.asarray(M)
    d = M.shape[0]
    with mpmath.workdps(ro.MP_DIGITS):
        A = mpmath.matrix(d, d)
        for i in range(d):
            for j in range(d):
                A[i, j] = _mpf(LD(M[i, j]))
        U, S, V = mpmath.svd_r(A)
        order = sorted(range(d), key=lambda i: -S[i])
        s = 1.0 if mpmath.det(U) * mpmath.det(V) > 0 else -1.0
        D = mpmath.eye(d)
        D[order[-1], order[-1]] = s
        P = U * D * V
        R = np.array([[float(P[i, j]) for j in range(d)] for i in range(d)])
        sig = np.array([float(S[i]) for i in order])
    return R, sig, s


def kappa(sig, s):
    d = len(sig)
    den = sig[d - 2] + s * sig[d - 1]
    return 2.0 * sig[0] / den if den > 0 else np.inf


def block_error(got, Yi, Vd, flip=False):
    """(error in the units of the module's head, kappa, R) of a rounded pose block `got` for the input rows Yi (d x k) and the basis
    Vd (k x d); flip: the last column of Yi Vd is negated first."""
    Yl, Vl = np.asarray(Yi, dtype=np.float64).astype(LD), np.asarray(Vd, dtype=np.float64).astype(LD)
    M = Yl @ Vl
    if flip:
        M[:, -1] = -M[:, -1]
    R, sig, s = so_project(M)
    kap = kappa(sig, s)
    k = Yl.shape[1]
    forward = (k + 2) * EPS * float((np.abs(Yl) @ np.abs(Vl)).max()) * kap / sig[0]
    err = float(np.abs(np.asarray(got) - R).max()) / (EPS * kap + forward)
    return err, kap, R


def svd_route(Yi, Vd):
    """The float64 route the bound is calibrated on."""
    M = np.asarray(Yi, dtype=np.float64) @ np.asarray(Vd, dtype=np.float64)
    u, _, vt = np.linalg.svd(M)
    D = np.eye(M.shape[0])
    D[-1, -1] = 1.0 if np.linalg.det(u @ vt) > 0 else -1.0
    return u @ D @ vt


@functools.lru_cache(maxsize=None)
def basis(d, k, seed=0):
    """A k x d matrix with orthonormal columns (a function of d, k and the seed alone; read-only)."""
    q = np.linalg.qr(np.random.default_rng([77, d, k, seed]).standard_normal((k, d)))[0]
    q.setflags(write=False)
    return q


def lifted(block, Vd):
    """The d x k rows whose product with Vd reproduces the d x d block up to rounding."""
    return np.asarray(block) @ np.asarray(Vd).T


def catalogue(d, large=None):
    """rowops_ref's catalogue at (d, d) as [(name, parameter index, seed)]; large: None all, True only the `scaled` blocks
    above 1, False the others.  (One input cannot hold 1e-160 and 1e160 together: the squares of the one vanish against
    the other whatever the scaling.)"""
    out = []
    for name, kk, seed in ro.catalogue(d, d):
        big = name == "scaled" and ro.FAMILIES[name][kk] > 1.0
        if large is None or big == large:
            out.append((name, kk, seed))
    return out


# ---- whole matrices
def with_blocks(Y, d, blocks, Vd, first=0):
    """Y with the pose blocks first, first + 1, .. replaced by the d x d blocks lifted through Vd."""
    Y = Y.copy()
    for j, B in enumerate(blocks):
        Y[d * (first + j):d * (first + j) + d] = lifted(B, Vd)
    return Y


def in_span(truth, dims, Vd, rng, noise=1e-2):
    """A noisy relaxed point all of whose rows lie in the span of Vd's columns."""
    Z = truth + noise * rng.standard_normal(truth.shape)
    return Z @ Vd.T


def gram(Y):
    return ro.gram(Y, Y)


def reference(Y, Vd, d, n, r, nt, flipped, poses=True):
    """(X, M dets' signs are not decided here): the rounded N x d matrix for the basis Vd and the flip given -- pose blocks by
    so_project, range rows normalised in longdouble, translation rows y Vd in longdouble."""
    Y = np.asarray(Y, dtype=np.float64)
    P = Y.astype(LD) @ np.asarray(Vd, dtype=np.float64).astype(LD)
    if flipped:
        P[:, -1] = -P[:, -1]
    X = P.astype(np.float64)
    rot, rng_rows, _ = rows(d, n, r, nt)
    for i in range(n if poses else 0):   # (poses=False leaves the products there: check() takes the blocks one by one)
        X[rot[i]] = so_project(P[rot[i]])[0]
    if r:
        S = P[rng_rows]
        m, e = np.frexp(np.abs(S).max(axis=1, keepdims=True).astype(np.float64))
        S = S * (LD(2.0) ** (-e))
        nrm = np.sqrt((S * S).sum(axis=1, keepdims=True))
        X[rng_rows] = np.where(nrm > 0, S / np.where(nrm > 0, nrm, 1), S).astype(np.float64)
    return X


def dets(Y, Vd, d, n):
    """det(Y_i Vd) of every pose block in longdouble, scaled by the block's largest entry (signs and relative sizes)."""
    P = np.asarray(Y, dtype=np.float64)[:d * n].astype(LD) @ np.asarray(Vd, dtype=np.float64).astype(LD)
    out = np.zeros(n)
    for i in range(n):
        M = P[d * i:d * i + d]
        top = np.abs(M).max()
        if top > 0:
            M = M / top
        if d == 2:
            out[i] = float(M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0])
        else:
            out[i] = float(M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
                           + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))
    return out


def check(res, Y, d, n, r, nt, what="", blocks=True):
    """A result of Context.round / debug_round_host (or round_dev plus the downloaded X) against the reference ON THE
    RESULT'S OWN Vd: the count and the flip (blocks whose scaled determinant is within 1e-10 of zero may count either
    way), every pose block within ROUND_BOUND and orthonormal within ORTH_BOUND with determinant +1, range and translation
    rows within their forward bounds.  Returns the worst block error."""
    Y = np.asarray(Y, dtype=np.float64)
    k = Y.shape[1]
    Vd, X = res["Vd"], res["X"]
    dt = dets(Y, Vd, d, n)
    sure, unsure = int((dt > 1e-10).sum()), int((np.abs(dt) <= 1e-10).sum())
    assert sure <= res["count"] <= sure + unsure, (what, res["count"], sure, unsure)
    assert res["flipped"] == (res["count"] < n // 2), (what, res["count"], n)
    want = reference(Y, Vd, d, n, r, nt, res["flipped"], poses=False)
    rot, rng_rows, trn = rows(d, n, r, nt)
    worst = 0.0
    for i in range(n):
        got = X[rot[i]]
        assert ro.orth_error(got) <= ORTH_BOUND, (what, i, ro.orth_error(got))
        assert abs(np.linalg.det(got) - 1.0) <= 1e-12, (what, i)
        if blocks:
            err, kap, _ = block_error(got, Y[rot[i]], Vd, res["flipped"])
            if np.isfinite(kap):
                worst = max(worst, err)
                assert err <= ROUND_BOUND, (what, i, err, kap)
    mag = np.abs(Y) @ np.abs(Vd)
    fwd = (k + 2) * EPS * mag
    assert np.all(np.abs(X[trn] - want[trn]) <= fwd[trn]), (what, "translation rows")
    if r:
        Pr = Y[rng_rows].astype(LD) @ Vd.astype(LD)
        nrm = np.sqrt((Pr * Pr).sum(axis=1)).astype(np.float64)  # (longdouble: the squares of a 1e-170 row stay in range)
        fwd_rel = (fwd[rng_rows].max(axis=1).astype(LD) / np.where(nrm > 0, np.sqrt((Pr * Pr).sum(axis=1)), 1)).astype(np.float64)
        zero = nrm == 0
        assert np.all(X[rng_rows][zero] == 0.0), (what, "zero range rows")
        lim = 2 * fwd_rel + (d + 3) * EPS
        assert np.all(np.abs(X[rng_rows] - want[rng_rows]).max(axis=1)[~zero] <= lim[~zero]), (what, "range rows")
    print("%s: worst block error %.3f eps kappa (bound %.1f)" % (what, worst, ROUND_BOUND))
    return worst


def relaxed_point(truth, d, n, r, nt, k, rng, noise=1e-2):
    """A gauge copy of the ground truth at rank k (truth times a d x k matrix with orthonormal rows, the translation rows
    shifted) plus noise."""
    B = np.linalg.qr(rng.standard_normal((k, d)))[0].T
    Y = truth @ B
    Y[rows(d, n, r, nt)[2]] += rng.standard_normal(k) * 3.0
    return Y + noise * rng.standard_normal(Y.shape)


def basis_checks(res, Y, what=""):
    """The basis on its own: orthonormality and the eigen-residual against the longdouble Gram matrix, both within twice
    the same quantity of numpy.linalg.eigh plus the entrywise bound of a float64 Gram matrix; the sign convention exactly;
    the singular values within SIGMA_BOUND eps sigma_1^2 / sigma of numpy's (sigma_error)."""
    Y = np.asarray(Y, dtype=np.float64)
    N, k = Y.shape
    Vd, sig = res["Vd"], res["sigma"]
    d = Vd.shape[1]
    G, Gabs = gram(Y)
    w, V = np.linalg.eigh(G)
    w, V = w[::-1], V[:, ::-1]
    ref_orth = float(np.abs(V[:, :d].T @ V[:, :d] - np.eye(d)).max())
    ref_res = float(np.abs(G @ V[:, :d] - V[:, :d] * w[:d]).max())
    gram_slack = (N + 2) * EPS * float(Gabs.max())
    orth = float(np.abs(Vd.T @ Vd - np.eye(d)).max())
    resid = float(np.abs(G @ Vd - Vd * sig[:d] ** 2).max())
    print("%s: |Vd^T Vd - I| %.3e (eigh %.3e)  residual %.3e (eigh %.3e, Gram slack %.3e)" % (what, orth, ref_orth, resid, ref_res, gram_slack))
    assert orth <= 2 * ref_orth + (N + 2) * EPS, (what, orth, ref_orth)  # (the Gram bound, relative to the largest entry)
    assert resid <= 2 * ref_res + 2 * gram_slack, (what, resid, ref_res, gram_slack)
    for j in range(d):
        big = int(np.argmax(np.abs(Vd[:, j])))
        assert Vd[big, j] > 0, (what, "sign convention", j)
    assert np.all(np.diff(sig) <= 0), (what, "descending")
    err = sigma_error(sig, Y)
    print("%s: singular values, worst error %.3f eps sigma_1^2 / sigma (bound %.2f)" % (what, err, SIGMA_BOUND))
    assert err <= SIGMA_BOUND, (what, err)


def sigma_error(sig, Y):
    """The largest |sigma - numpy's| in units of eps sigma_1^2 / sigma, numpy's being the square roots of eigh's eigenvalues
    of the longdouble Gram matrix (rounded to float64); sigma in the unit: the larger of the two values."""
    G, _ = gram(Y)
    want = np.sqrt(np.maximum(np.linalg.eigh(G)[0][::-1], 0.0))
    unit = EPS * want[0] * want[0] / np.maximum(np.maximum(want, np.asarray(sig)), 1e-300)
    return float((np.abs(np.asarray(sig) - want) / unit).max())


def sigma_float64_route(Y):
    """The float64 route SIGMA_BOUND is calibrated on: numpy's eigh of the float64 Gram matrix Y^T Y."""
    Y = np.asarray(Y, dtype=np.float64)
    return np.sqrt(np.maximum(np.linalg.eigh(Y.T @ Y)[0][::-1], 0.0))
