"""Reference of the GNC weight step (cora_gnc_weights*, include/cora_hip.h) -- TEST INFRASTRUCTURE ONLY.

The weight formulas and the statistics in np.longdouble (64-bit mantissa here: eps = 1.1e-19, so the reference's own error
is four orders below the fp64 bounds), with the unweighted residuals r2 as an INPUT: what is checked is the step from
residuals to weights, the residuals have their own reference (tests/residuals_ref.py).

Layout everywhere: [rot of every edge | trans of every edge | range], n_w = 2 n_edges + n_ranges.

BOUNDS of an fp64 evaluation in the stated order against this reference, per weight:
  TLS  |dw| <= 8 eps (mu + 1)    rho = r2 / barc2, mu (mu + 1), / rho, sqrt, - mu: five operations of one rounding each; the
                                 square root is at most mu + 1 in the middle band, so every rounding moves w by at most
                                 about eps (mu + 1); the two hard branches are continuous with the middle one, so a ratio that
                                 rounds across a boundary stays inside.  8 leaves room for the amplification of the first
                                 three roundings through the square root (a factor 1/2 each) and the sum mu + 1.
  GM   |dw| <= 8 eps             quotient, sum, quotient, product: t <= 1, each rounding moves w by at most 2 eps.
  sum  |d sum_wr2| <= (n + 3) eps sum |w r2|   an n-term sum plus the product's rounding."""
import numpy as np

EPS = np.finfo(np.float64).eps
L = np.longdouble
NONE, TLS, GM = "none", "tls", "gm"


def weight_bound(cost, mu):
    return {NONE: 0.0, TLS: 8 * EPS * (mu + 1), GM: 8 * EPS}[cost]


def slots(r2, barc2, n_edges, couple_edges):
    """(r2, barc2) each slot is judged by, in longdouble: the slot's own, or for a coupled edge rot + trans (one fp64
    addition, as the library forms it) against the threshold of the trans slot, in both of its slots."""
    r2 = np.asarray(r2, dtype=np.float64)
    c = np.asarray(barc2, dtype=np.float64).copy()
    m = r2.copy()
    if couple_edges:
        ne = n_edges
        m[:ne] = m[ne:2 * ne] = r2[:ne] + r2[ne:2 * ne]
        c[:ne] = c[ne:2 * ne]
    return m.astype(L), c.astype(L)


def ratios(r2, barc2, n_edges, couple_edges):
    m, c = slots(r2, barc2, n_edges, couple_edges)
    with np.errstate(invalid="ignore"):
        return np.where(np.isinf(c), L(0), m / c)


def weights(r2, barc2, n_edges, cost, mu, couple_edges):
    """The weights in longdouble."""
    rho = ratios(r2, barc2, n_edges, couple_edges)
    if cost == NONE:
        return np.ones(len(rho), dtype=L)
    mu = L(mu)
    if cost == GM:
        t = mu / (rho + mu)
        return t * t
    assert cost == TLS
    with np.errstate(divide="ignore", invalid="ignore"):
        mid = np.sqrt(mu * (mu + 1) / rho) - mu
    return np.where(rho <= mu / (mu + 1), L(1), np.where(rho >= (mu + 1) / mu, L(0), mid))


def weights_float64(r2, barc2, n_edges, cost, mu, couple_edges):
    """The same formulas in plain float64, one numpy operation per rounding in the stated order (ratio; TLS: mu (mu + 1),
    / rho, sqrt, - mu, clamped to [0, 1]; GM: rho + mu, mu / that, squared): what a user's own numpy weight step computes."""
    m, c = slots(r2, barc2, n_edges, couple_edges)
    m, c = m.astype(np.float64), c.astype(np.float64)
    with np.errstate(invalid="ignore"):
        rho = np.where(np.isinf(c), 0.0, m / c)
    if cost == NONE:
        return np.ones(len(rho))
    mu = np.float64(mu)
    if cost == GM:
        t = mu / (rho + mu)
        return t * t
    with np.errstate(divide="ignore", invalid="ignore"):
        mid = np.clip(np.sqrt(mu * (mu + 1.0) / rho) - mu, 0.0, 1.0)
    return np.where(rho <= mu / (mu + 1.0), 1.0, np.where(rho >= (mu + 1.0) / mu, 0.0, mid))


def statistics(r2, barc2, w, n_edges, couple_edges):
    """stats[3][4] = {sum_wr2, max_rho, n_mid, n_out} of rot, trans, range for the fp64 weights w the library returned:
    the counts and the maxima are functions of w and of the fp64 ratio (one correctly rounded division), so they are
    EXACT; the sums are formed in longdouble, with sum |w r2| beside them for the bound."""
    r2 = np.asarray(r2, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    ne = n_edges
    m, c = slots(r2, barc2, ne, couple_edges)
    with np.errstate(invalid="ignore"):
        rho = np.where(np.isinf(c), 0.0, m.astype(np.float64) / c.astype(np.float64))
    segs = (slice(0, ne), slice(ne, 2 * ne), slice(2 * ne, len(r2)))
    out, mags = np.zeros((3, 4), dtype=L), np.zeros(3, dtype=L)
    for s, seg in enumerate(segs):
        prod = w[seg].astype(L) * r2[seg].astype(L)
        out[s, 0] = prod.sum()
        mags[s] = np.abs(prod).sum()
        if couple_edges and s == 0:
            continue  # a coupled edge is counted and maximised in the trans segment only
        out[s, 1] = rho[seg].max(initial=0.0)
        out[s, 2] = np.sum((w[seg] > 0) & (w[seg] < 1))
        out[s, 3] = np.sum(w[seg] < 0.5)
    return out, mags


def check_weights(got, r2, barc2, n_edges, cost, mu, couple_edges, what=""):
    """Asserts the bound; returns the worst |dw| / bound (0 for cost NONE, which must be exact)."""
    ref = weights(r2, barc2, n_edges, cost, mu, couple_edges)
    err = np.abs(np.asarray(got, dtype=np.float64).astype(L) - ref).max(initial=0.0)
    bound = weight_bound(cost, mu)
    print("%s %s mu=%g coupled=%d: max |dw| = %.3e, bound %.3e" % (what, cost, mu, couple_edges, float(err), bound))
    assert err <= bound, (what, cost, mu, float(err), bound)
    return float(err / bound) if bound else 0.0


def check_statistics(got, r2, barc2, w, n_edges, couple_edges, what=""):
    ref, mags = statistics(r2, barc2, w, n_edges, couple_edges)
    got = np.asarray(got, dtype=np.float64).reshape(3, 4)
    sizes = (n_edges, n_edges, len(np.asarray(r2)) - 2 * n_edges)
    for s in range(3):
        assert got[s, 1] == float(ref[s, 1]) and got[s, 2] == float(ref[s, 2]) and got[s, 3] == float(ref[s, 3]), (what, s, got[s], ref[s])
        err = abs(L(got[s, 0]) - ref[s, 0])
        bound = (sizes[s] + 3) * EPS * mags[s]
        print("%s segment %d: |d sum_wr2| = %.3e, bound %.3e" % (what, s, float(err), float(bound)))
        assert err <= bound, (what, s, float(err), float(bound))
