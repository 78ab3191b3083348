"""numpy.longdouble / mpmath reference of the outlier-robust placement from closures (include/cora_hip.h,
cora_place_by_closures_robust_dev) -- TEST INFRASTRUCTURE ONLY.  The structure is closure_ref.structure's.  Per
list: every r(h, j) in longdouble, the votes, the election (largest vote, lowest entry) and the inliers I; then closure_ref's
exact minimiser (weighted Kabsch in mpmath) over the sub-list I, with the origin terms of the list's actual first entry.

The counts are integers and are compared exactly.  That is fair only where no residual sits on the threshold: the reference
reports every r(h, j) with barc2 / 2 <= r <= 2 barc2 in `band`, over all h and j of every list, and every test case asserts
that `band` is empty.  (The device's r differs from the exact one by rounding, a relative 1e-12 at most on these data; a factor
of 2 either side is no rounding.)

The result has the layout of closure_ref.reference's, so closure_ref.check applies: the bound is closure_ref's, over I."""
import numpy as np

import closure_ref as cl
import placement_ref as pl

LD, EPS = cl.LD, cl.EPS
_lsum, _norm = cl._lsum, cl._norm
# 4 x the worst ratio error / (a + b) of the mirror over the cases of tests/test_closure_consensus_cpu.py stays below
# closure_ref.C_BOUND (profiles/closure_consensus.md), so the constant is closure_ref's
C_BOUND = cl.C_BOUND


def residuals(P, q, l, kappa, tau):
    """r[h, j]: the coupled residual of entry j under the hypothesis of entry h, about the first entry (longdouble)."""
    qq, ll = q - q[0], l - l[0]
    sp = ll - np.einsum("hak,hk->ha", P, qq)                                  # s'_h
    rot = np.sum((P[:, None] - P[None]) ** 2, axis=(2, 3))                    # |G_h - P_j|^2
    pred = np.einsum("hak,jk->hja", P, qq) + sp[:, None, :] - ll[None]        # G_h q'_j + s'_h - l'_j
    return kappa[None] * rot + tau[None] * np.sum(pred ** 2, axis=2)


def reference(d, n, r, nt, table, chains, X, barc2, min_consensus=2, chain_fixed=None, min_closures=1):
    """closure_ref.reference's dict for the robust call, plus consensus, list_len (per chain), inlier (per edge: 1 | 0 | 2),
    elected (per taken chain: the entry), no_consensus, excluded and band (the residuals too close to the threshold)."""
    rr = np.asarray(table[2])
    X = np.array(X, dtype=LD)
    S = cl.structure(d, n, r, nt, table, chains, chain_fixed, min_closures)
    nch, ne = len(chains), len(table[0])
    res = dict(struct=S, status=np.array(S["chain_init"], dtype=np.uint8), chosen=np.full(nch, -1, dtype=np.int32),
               cost_start=np.zeros(nch, dtype=LD), cost_final=np.zeros(nch, dtype=LD),
               transforms=np.tile(np.concatenate([np.eye(d).reshape(-1), np.zeros(d)]), (nch, 1)).astype(LD), chain={},
               level={}, rot_level={}, round={}, consensus=np.zeros(nch, dtype=np.int32), list_len=np.zeros(nch, dtype=np.int32),
               inlier=np.full(ne, 2, dtype=np.uint8), elected={}, band=[])
    level, rot_level = res["level"], res["rot_level"]
    for st in S["stages"]:
        moves = []
        for c, es in st:
            P, q, l, kappa, tau, resid, ra, rb, ta, tb, tn = cl.entries(d, table, X, es)
            R = residuals(P, q, l, kappa, tau)
            res["band"] += [(c, int(h), int(j), float(R[h, j])) for h, j in zip(*np.nonzero((R >= barc2 / 2) & (R <= 2 * barc2)))]
            votes = np.where(kappa > 0, np.sum(R <= barc2, axis=1), 0)
            h = int(np.argmax(votes))    # (the first of the largest)
            I = np.nonzero(R[h] <= barc2)[0]
            res["consensus"][c], res["list_len"][c], res["elected"][c] = votes[h], len(es), h
            res["inlier"][[e for e, _ in es]] = 0
            res["inlier"][[es[j][0] for j in I]] = 1
            start = _lsum(resid[I]) if len(I) else LD(0)
            # a cost of this size is the rounding of the written numbers (closure_ref's floor, over I)
            floor = (64 * EPS) ** 2 * float(_lsum(kappa[I] * d + tau[I] * (np.sum(q[I] * q[I], axis=1) + np.sum(l[I] * l[I], axis=1)))) if len(I) else 0.0
            one = dict(es=es, G=np.eye(d, dtype=LD), s=np.zeros(d, dtype=LD), a_R=0.0, a_t=0.0, b_t=0.0, sv=None, margin=None,
                       costs=(float(start), float(start)), cost_floor=floor, chosen=False, I=I, quad=0.0)
            res["chain"][c] = one
            res["cost_start"][c] = res["cost_final"][c] = start
            res["chosen"][c] = 0
            if votes[h] < min_consensus:
                res["status"][c] = 5
                continue
            q0, l0 = q[0], l[0]     # the origin: the list's first entry, an inlier or not
            P, q, l, kappa, tau, ra, rb, ta, tb, tn = (v[I] for v in (P, q, l, kappa, tau, ra, rb, ta, tb, tn))
            W, K = _lsum(tau), _lsum(kappa)
            H = _lsum(kappa[:, None, None] * P)
            sq = sl = LD(0)
            if W > 0:
                cq, cl_ = _lsum(tau[:, None] * q) / W, _lsum(tau[:, None] * l) / W
                qc, lc = q - cq, l - cl_
                H = H + _lsum(tau[:, None, None] * lc[:, :, None] * qc[:, None, :])
                sq, sl = _lsum(tau * np.sum(qc * qc, axis=1)), _lsum(tau * np.sum(lc * lc, axis=1))
            else:
                cq, cl_ = q0, l0
            no, one["margin"] = cl.rule(d, H, K, W, sq, sl)
            if no:
                res["status"][c] = 2
                continue
            res["status"][c] = 0
            G, sv = cl.kabsch(H)
            s = cl_ - G @ cq
            final = _lsum(kappa * np.sum((G - P) ** 2, axis=(1, 2)) + tau * np.sum((q @ G.T + s - l) ** 2, axis=1))
            res["cost_final"][c] = final
            Wf, Kf = float(W), float(K)
            Lq = float(np.sqrt(_lsum(tau * np.sum((q - q0) ** 2, axis=1)) / W)) if W > 0 else 0.0
            Ll = float(np.sqrt(_lsum(tau * np.sum((l - l0) ** 2, axis=1)) / W)) if W > 0 else 0.0
            dp = np.array([level.get(int(b), 0.0) + rot_level.get(int(a), 0.0) * float(k) + EPS * (float(_norm(X[b])) + float(k))
                           for a, b, k in zip(ra, ta, tn)])
            delta = float((dp + np.array([level.get(int(b), 0.0) for b in tb])).max())
            dP = max(rot_level.get(int(a), 0.0) + rot_level.get(int(b), 0.0) for a, b in zip(ra, rb)) + 4 * EPS * np.sqrt(d)
            size = Kf * np.sqrt(d) + Wf * Lq * Ll
            gap = (sv[0] + sv[1]) if d == 2 else (sv[1] + sv[2])
            dH = EPS * size + Kf * dP + Wf * (Lq + Ll) * delta
            one.update(G=G, s=s, cq=cq, cl=cl_, sv=sv, a_R=dH / gap, a_t=2 * delta + EPS * (Lq + Ll), kappa=size / gap,
                       b_t=EPS * float(_norm(q0) + _norm(l0) + _norm(s) + _norm(cq) + _norm(cl_)), chosen=bool(final < start),
                       costs=(float(start), float(final)),
                       # what the cost at a motion within the bound of the minimiser lies above the minimum by: second order
                       quad=size * (C_BOUND * dH / gap) ** 2 + Wf * (C_BOUND * (dH / gap * Lq + 2 * delta + EPS * (Lq + Ll))) ** 2)
            res["chosen"][c] = 1 if final < start else 0
            if final < start:
                res["transforms"][c] = np.concatenate([G.reshape(-1), s])
                moves.append((c, G, s))
            else:
                res["cost_final"][c] = start
        for c, G, s in moves:
            one = res["chain"][c]
            for rot, trn in S["positions"][c]:
                x = X[trn].copy()
                xn = G @ x + s
                X[rot:rot + d] = X[rot:rot + d] @ G.T
                X[trn] = xn
                level[trn] = level.get(trn, 0.0) + one["a_R"] * float(_norm(x - one["cq"])) + one["a_t"]
                rot_level[rot] = rot_level.get(rot, 0.0) + one["a_R"] + 4 * EPS
                res["round"][trn] = one["b_t"] + EPS * float(_norm(x) + _norm(xn))
    deg, norm = np.zeros(len(rr), dtype=bool), np.zeros(len(rr), dtype=LD)
    for m in range(len(rr)):
        diff = X[rr[m, 2]] - X[rr[m, 1]]
        nrm = norm[m] = np.sqrt(np.sum(diff * diff))
        deg[m] = nrm < 1e-5
        X[rr[m, 0]] = 0 if deg[m] else -diff / nrm
    res.update(X=X, degenerate=deg, norm=norm, no_consensus=int(np.sum(res["status"] == 5)), excluded=int(np.sum(res["inlier"] == 0)))
    return res


def check(got, d, n, r, nt, table, ref):
    """The band is empty; the integer results equal the reference's exactly; then closure_ref.check (statuses, counts, chosen,
    the transforms and every written row within the bound over I).  Returns the worst error / (a + b)."""
    assert ref["band"] == [], ref["band"][:8]
    for key in ("consensus", "list_len", "inlier"):
        assert np.array_equal(got[key], ref[key]), (key, got[key], ref[key])
    assert got["no_consensus"] == ref["no_consensus"] and got["excluded"] == ref["excluded"]
    # cost_start and cost_final are sums over I: against the reference's.  A sum of n terms w r^2 whose r carry the rounding of
    # the written numbers (floor: the sum of w delta^2) differs by at most 2 sqrt(cost floor) + floor (Cauchy-Schwarz) and n eps
    # of the sum; the cost at the mirror's motion lies above the minimum by the second-order term `quad` (twice: cross terms)
    for c, one in ref["chain"].items():
        n_eps = (len(one["I"]) + 8) * EPS
        for key, k in (("cost_start", 0), ("cost_final", 1)):
            want = one["costs"][k] if (k == 0 or got["chosen"][c]) else one["costs"][0]
            tol = 2 * np.sqrt(want * one["cost_floor"]) + one["cost_floor"] + n_eps * want + (2 * one["quad"] if k else 0.0)
            assert abs(got[key][c] - want) <= tol, (key, c, got[key][c], want, tol)
    # (the robust call returns the count of the degenerate range rows, not the bytes: asserted through n_degenerate)
    return cl.check(dict(got, degenerate=ref["degenerate"]), d, n, r, nt, table, ref, C=C_BOUND)


def _big_rot(d, rng):
    """A rotation by 0.5 .. pi radians, either sense, about a random axis."""
    th = rng.uniform(0.5, np.pi) * rng.choice([-1.0, 1.0])
    if d == 2:
        return np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    ax = rng.normal(0, 1, 3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def spoil(d, ed, edges, rng):
    """The edges `edges` of the edge data ed made wrong, in place: R <- R Z with Z a random rotation of at least 0.5 rad, t <- t
    + an offset of 2 .. 8 m per axis, either sign."""
    for e in edges:
        ed[e, :d * d] = (ed[e, :d * d].reshape(d, d) @ _big_rot(d, rng)).reshape(-1)
        ed[e, d * d:d * d + d] += rng.uniform(2, 8, d) * rng.choice([-1.0, 1.0], d)


def contaminate_world(w, seed=5):
    """A topologies.World whose graph has, per ordered pair of robots with rel_pose edges between them, wrong closures
    amounting to one third of the pair's closures appended: between random poses of the two robots, the true relative pose
    spoiled as `spoil` does.  Returns the number of edges before (the appended ones follow)."""
    rng = np.random.default_rng(seed)
    g, d = w.g, w.g.dim
    idx = {s: i for i, s in enumerate(w.names)}
    robot = lambda s: s[0]
    links = {}
    for a, b, R, t, cov in g.rpms:
        if robot(a) != robot(b):
            links.setdefault(tuple(sorted((robot(a), robot(b)))), []).append((a, b, cov))
    before = len(g.rpms)
    for (ra, rb), es in sorted(links.items()):
        A, B = [s for s in w.names if robot(s) == ra], [s for s in w.names if robot(s) == rb]
        for k in range(max(len(es) // 3, 1)):
            a, b = A[int(rng.integers(len(A)))], B[int(rng.integers(len(B)))]
            if k % 2:
                a, b = b, a
            i, j = idx[a], idx[b]
            ed = np.concatenate([(w.R[i].T @ w.R[j]).reshape(-1), w.R[i].T @ (w.T[j] - w.T[i])])[None].copy()
            spoil(d, ed, [0], rng)
            g.rpms.append((a, b, ed[0, :d * d].reshape(d, d), ed[0, d * d:], es[0][2]))
    return before


__all__ = ["reference", "check", "residuals", "spoil", "contaminate_world", "C_BOUND", "pl"]
