"""The trajectory comparison of include/cora_hip.h (cora_compare_dev) restated in numpy: every sum in longdouble, the SVD
numpy.linalg.svd in float64, plus the rounding bounds the tests hold the library to.  API row order: d n rotation rows,
r range rows, n + l translation rows (poses, then landmarks)."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


def rows(d, n, r, nt):
    """(rotation rows [n, d], range rows [r], translation rows [nt]) in API order."""
    return np.arange(d * n).reshape(n, d), d * n + np.arange(r), d * n + r + np.arange(nt)


def selection(select, nt):
    return np.ones(nt, dtype=bool) if select is None else np.asarray(select) != 0


def centred(X, Ref, d, n, r, nt, select=None):
    """xbar, gbar, the selected poses' centred rows (m x k, m x kr) and H, all longdouble."""
    sel = selection(select, nt)
    t = rows(d, n, r, nt)[2][:n][sel[:n]]
    x, g = X[t].astype(LD), Ref[t].astype(LD)
    xbar, gbar = x.sum(0) / len(t), g.sum(0) / len(t)
    xc, gc = x - xbar, g - gbar
    return xbar, gbar, xc, gc, xc.T @ gc


def kabsch(H, proper):
    """A = U D V^T (float64 SVD of the longdouble H rounded to float64), the singular values."""
    U, s, Vt = np.linalg.svd(np.asarray(H, dtype=np.float64), full_matrices=False)
    D = np.ones(len(s))
    if proper:
        D[-1] = np.sign(np.linalg.det(U @ Vt))
    return (U * D) @ Vt, s, D


def optimum(xc, gc, H, proper):
    """min over A^T A = I (det A = +1 when proper) of sum |xc A - gc|^2, for k == kr or A^T A = I with k >= kr:
    |xc A|^2 summed is tr(A^T xc^T xc A); for k == kr that is |xc|^2, and the optimum is |xc|^2 + |gc|^2 - 2 sum D s."""
    A, s, D = kabsch(H, proper)
    r = xc @ A.astype(LD) - gc
    return float((r * r).sum()), A, s


def errors(X, Ref, d, n, r, nt, A, xbar, gbar, select=None):
    """et [n], er [n], el [l] in longdouble with the GIVEN A, xbar, gbar; unselected entries 0."""
    sel = selection(select, nt)
    rot, _, trn = rows(d, n, r, nt)
    A, xbar, gbar = A.astype(LD), np.asarray(xbar, dtype=LD), np.asarray(gbar, dtype=LD)
    Xl, Gl = X.astype(LD), Ref.astype(LD)
    dt = (Xl[trn] - xbar) @ A - (Gl[trn] - gbar)
    e_all = np.sqrt((dt * dt).sum(1)) * sel
    dr = Xl[rot.ravel()] @ A - Gl[rot.ravel()]
    er = np.sqrt((dr * dr).sum(1).reshape(n, d).sum(1)) * sel[:n]
    return e_all[:n], er, e_all[n:]


def entry_bound(X, Ref, d, n, r, nt, xbar, gbar, factor=8):
    """factor (k + kr) eps (|x_i - xbar| + |g_i - gbar| + |xbar| + |gbar|) per translation row [nt]; the rotation
    blocks' rows are unit-size, far inside the same bound of their pose."""
    trn = rows(d, n, r, nt)[2]
    k, kr = X.shape[1], Ref.shape[1]
    nx = np.linalg.norm(X[trn] - xbar, axis=1) + np.linalg.norm(Ref[trn] - gbar, axis=1)
    return factor * (k + kr) * EPS * (nx + np.linalg.norm(xbar) + np.linalg.norm(gbar))


def aligned(X, d, n, r, nt, A, xbar, gbar):
    """The estimate in the reference's frame with the GIVEN A, xbar, gbar (longdouble)."""
    trn = rows(d, n, r, nt)[2]
    out = X.astype(LD) @ A.astype(LD)
    out[trn] = (X[trn].astype(LD) - np.asarray(xbar, dtype=LD)) @ A.astype(LD) + np.asarray(gbar, dtype=LD)
    return out


def reference_of_rank(truth, d, n, r, nt, kr, rng, spread=10.0):
    """A reference of kr columns.  kr == d: the ground truth itself.  kr > d: the ground truth's rotation and range rows
    in a random orthonormal frame of R^kr, and positions scattered independently by `spread` in all kr dimensions -- a
    trajectory's own third singular value is small against its first, and m - 1 = 29 centred positions cannot keep it
    apart from 21 more dimensions; independent positions keep H of full rank with sigma_min / sigma_max about
    ((sqrt(m) - sqrt(kr)) / (sqrt(m) + sqrt(kr)))^2, 2e-3 at m = 30 and kr = 24."""
    if kr == truth.shape[1]:
        return truth
    Ref = np.hstack([truth, np.zeros((len(truth), kr - truth.shape[1]))]) @ np.linalg.qr(rng.standard_normal((kr, kr)))[0]
    Ref[rows(d, n, r, nt)[2]] = spread * rng.standard_normal((nt, kr))
    return Ref


def gauge_copy(Ref, d, n, r, nt, k, rng, mirror=False):
    """X = Ref B^T (+ 1 c^T on the translation rows), B random k x kr with orthonormal columns, c random: what the
    comparison must map back onto Ref with A = B.  mirror (k == kr): det B < 0."""
    kr = Ref.shape[1]
    B = np.linalg.qr(rng.standard_normal((k, kr)))[0]
    if k == kr and (np.linalg.det(B) < 0) != mirror:
        B[:, -1] = -B[:, -1]
    c = rng.standard_normal(k) * 3.0
    X = Ref @ B.T
    X[rows(d, n, r, nt)[2]] += c
    return X, B, c


def check_statistics(res, what=""):
    """The maxima are the maxima of the arrays exactly; the sums within m eps sum."""
    et, er, el = res["pose_trans_err"], res["pose_rot_err"], res["landmark_err"]
    assert res["max_et"] == et.max(initial=0.0) and res["max_er"] == er.max(initial=0.0), what
    assert res["max_el"] == el.max(initial=0.0), what
    for key, v, cnt in (("sum_et2", et, res["m"]), ("sum_er2", er, res["m"]), ("sum_el2", el, res["n_landmarks"])):
        want = float((v.astype(LD) ** 2).sum())
        assert abs(res[key] - want) <= max(cnt, 1) * EPS * want, (what, key, res[key], want)


def h_tolerance(xc, gc):
    """(m + 4) eps sum_P |x_ia - xbar_a| |g_ib - gbar_b| per entry of H (k x kr, float64): two subtractions, one
    product and m - 1 additions, each one rounding."""
    return np.asarray((len(xc) + 4) * EPS * (np.abs(xc).T @ np.abs(gc)), dtype=np.float64)


def alignment_bound(xc, gc, k):
    """How far the A of one form may be from the exact polar factor of the exact H, in the Frobenius norm, where D = I and
    H has full column rank: 4 |tol|_F / sigma_min(H) + 64 k eps, tol the H tolerance above (the polar factor moves by at
    most 2 |dH|_F / (sigma_min + sigma_next); the rest is the SVD's own rounding).  Fixed by the inputs."""
    s = np.linalg.svd(np.asarray(xc.T @ gc, dtype=np.float64), compute_uv=False)
    return 4 * np.linalg.norm(h_tolerance(xc, gc)) / s[-1] + 64 * k * EPS


def mean_bound(X, Ref, d, n, r, nt, select=None):
    """eps sum_P |x_ic| per column of X and of Ref: what one form's means may be off by."""
    sel = selection(select, nt)
    t = rows(d, n, r, nt)[2][:n][sel[:n]]
    return EPS * np.abs(X[t]).sum(0), EPS * np.abs(Ref[t]).sum(0)


def check_noisy(res, H_got, X, Ref, d, n, r, nt, select=None, proper=False, what=""):
    """Everything the issue asks of a comparison of a noisy estimate; returns the worst ratios to the bounds."""
    sel = selection(select, nt)
    k, kr = X.shape[1], Ref.shape[1]
    xbar, gbar, xc, gc, H = centred(X, Ref, d, n, r, nt, select)
    t = rows(d, n, r, nt)[2][:n][sel[:n]]
    worst = {}
    bx, bg = EPS * np.abs(X[t]).sum(0), EPS * np.abs(Ref[t]).sum(0)
    ex, eg = np.abs(res["xbar"] - xbar).astype(np.float64), np.abs(res["gbar"] - gbar).astype(np.float64)
    assert np.all(ex <= bx) and np.all(eg <= bg), (what, "means", ex, bx, eg, bg)
    worst["mean"] = float(max((ex / np.maximum(bx, 1e-300)).max(), (eg / np.maximum(bg, 1e-300)).max()))
    tol = h_tolerance(xc, gc)
    eh = np.abs(H_got - H).astype(np.float64)
    worst["H"] = float((eh / np.maximum(tol, 1e-300)).max())
    print("%s: worst |dH| / tolerance = %.3f" % (what, worst["H"]))
    assert np.all(eh <= tol), (what, "H", worst["H"])
    A = res["A"]
    orth = np.linalg.norm(A.T @ A - np.eye(kr))
    assert orth <= 64 * k * EPS, (what, "A^T A - I", orth)
    opt, _, s = optimum(xc, gc, H, proper)
    print("%s: sum et^2 %.17g, reference optimum %.17g, sigma_min / sigma_max %.3e" % (what, res["sum_et2"], opt, s[-1] / s[0]))
    assert abs(res["sum_et2"] - opt) <= 1e-12 * opt, (what, res["sum_et2"], opt)
    if proper:
        assert abs(np.linalg.det(A) - 1.0) <= 64 * k * EPS, what
    check_entries(res, X, Ref, d, n, r, nt, select, what=what, worst=worst)
    check_statistics(res, what)
    assert res["m"] == sel[:n].sum() and res["n_landmarks"] == sel[n:].sum()
    return worst


def check_entries(res, X, Ref, d, n, r, nt, select=None, factor=8, what="", worst=None):
    """The per-entry errors against a longdouble recomputation with the RETURNED A, xbar, gbar; unselected entries 0."""
    sel = selection(select, nt)
    et, er, el = errors(X, Ref, d, n, r, nt, res["A"], res["xbar"], res["gbar"], select)
    bound = entry_bound(X, Ref, d, n, r, nt, res["xbar"], res["gbar"], factor)
    for key, want, b, on in (("pose_trans_err", et, bound[:n], sel[:n]), ("pose_rot_err", er, bound[:n], sel[:n]),
                             ("landmark_err", el, bound[n:], sel[n:])):
        got = res[key]
        assert np.all(got[~on] == 0.0), (what, key, "unselected entries")
        err = np.abs(got - want).astype(np.float64)
        ratio = float((err / np.maximum(b, 1e-300)).max(initial=0.0))
        print("%s: %s worst |error| / bound = %.3f" % (what, key, ratio))
        assert np.all(err <= b), (what, key, ratio)
        if worst is not None:
            worst[key] = ratio


def check_gauge(res, B, c, Ref, d, n, r, nt, xc, gc, what=""):
    """X was a gauge copy of Ref: errors at rounding level, A = B up to the perturbation bound of the polar factor."""
    k, kr = B.shape
    s = res["sigma"]
    assert s[-1] / s[0] >= 1e-4, (what, "not a well conditioned case", s)
    trn = rows(d, n, r, nt)[2]
    gbar = res["gbar"]
    scale = np.linalg.norm(Ref[trn] - gbar, axis=1) + np.linalg.norm(gbar) + np.linalg.norm(c) + 1.0
    bound = 64 * (k + kr) * EPS * scale
    for key, b in (("pose_trans_err", bound[:n]), ("pose_rot_err", bound[:n]), ("landmark_err", bound[n:])):
        ratio = float((res[key] / b).max(initial=0.0))
        print("%s: %s worst / bound = %.3f" % (what, key, ratio))
        assert np.all(res[key] <= b), (what, key, ratio)
    dH = np.linalg.norm(h_tolerance(xc, gc))
    dA = np.linalg.norm(res["A"] - B)
    print("%s: |A - B| = %.3e, bound %.3e" % (what, dA, 4 * dH / s[-1] + 64 * k * EPS))
    assert dA <= 4 * dH / s[-1] + 64 * k * EPS, (what, dA)


def check_degenerate(res, k, what=""):
    kr = res["A"].shape[1]
    for key in ("pose_trans_err", "pose_rot_err", "landmark_err", "sigma", "xbar", "gbar", "A", "raw"):
        assert np.all(np.isfinite(res[key])), (what, key)
    assert np.linalg.norm(res["A"].T @ res["A"] - np.eye(kr)) <= 64 * k * EPS, what


def check_aligned(al, res, X, Ref, d, n, r, nt, N, what=""):
    """The aligned estimate against the formula with the returned A, xbar, gbar, at the per-entry bound (a rotation or
    range row has no centred norms: its own unit norm stands for them)."""
    want = aligned(X, d, n, r, nt, res["A"], res["xbar"], res["gbar"])
    k, kr = X.shape[1], res["A"].shape[1]
    xbar, gbar = res["xbar"], res["gbar"]
    trn = rows(d, n, r, nt)[2]
    b = np.full(N, 8 * (k + kr) * EPS * (1.0 + np.linalg.norm(xbar) + np.linalg.norm(gbar)))
    b[trn] = 8 * (k + kr) * EPS * (np.linalg.norm(X[trn] - xbar, axis=1) + np.linalg.norm(Ref[trn] - gbar, axis=1)
                                   + np.linalg.norm(xbar) + np.linalg.norm(gbar))
    err = np.abs(al - want).astype(np.float64).max(1)
    assert np.all(err <= b), (what, float((err / b).max()))
