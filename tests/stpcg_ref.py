"""Plain numpy Steihaug-Toint PCG that stops after exactly k iterations and keeps every iteration's state -- the reference
of tests/test_gpu_stpcg_forms.py (through tests/stpcg_forms_worker.py).  Same published algorithm as oracle/tnt.py::stpcg
(Conn, Gould & Toint, Alg. 7.5.1), on the oracle's operators only: nothing here calls the library under test.

Inner products are accumulated in np.longdouble; the Cholesky preconditioner gets one step of iterative refinement with
the residual formed in np.longdouble, so that the reference's own solve error is negligible next to the 1e-9 the device is
held to (`plain=True` switches both off: what the reference differs from itself by, tests/stpcg_forms_worker.py spread)."""
import math

import numpy as np

from oracle import oracle as orc

CLASSES = ("rot", "rng", "trn")


def row_classes(dm):
    """Row ranges of the three classes of rows the fused epilogues treat differently."""
    return {"rot": (0, dm.dn), "rng": (dm.dn, dm.dn + dm.r), "trn": (dm.dn + dm.r, dm.N)}


def class_errors(dm, got, ref):
    """max |got - ref| over each row class, relative to that class's largest reference entry."""
    out = {}
    for name, (lo, hi) in row_classes(dm).items():
        den = float(np.abs(ref[lo:hi]).max())
        num = float(np.abs(got[lo:hi] - ref[lo:hi]).max())
        out[name] = num / den if den > 0 else (0.0 if num == 0 else float("inf"))
    return out


def ldot(a, b):
    return float(np.dot(np.asarray(a, dtype=np.longdouble).ravel(order="F"), np.asarray(b, dtype=np.longdouble).ravel(order="F")))


class RegularizedCholesky:
    """Proj_Y((Q + lam I)[:N-1, :N-1]^-1 .) with the last row pinned to zero (blockCholeskySolve semantics)."""

    def __init__(self, Q, dm, lam, plain=False):
        import scipy.sparse as sp
        self.dm, self.plain = dm, plain
        self.M = (Q.to_scipy() + lam * sp.eye(dm.N)).tocsr()[:dm.N - 1, :dm.N - 1].tocsr()
        self.M.sort_indices()
        self.chol = orc.Cholesky(orc.CSR.from_scipy(self.M))
        assert self.chol.ok
        self._val = self.M.data.astype(np.longdouble)

    def residual(self, X, B):
        """B - M X with every product and sum in np.longdouble (every row of M holds its diagonal: no empty row)."""
        prod = self._val[:, None] * np.asarray(X, dtype=np.longdouble)[self.M.indices]
        return np.asarray(B, dtype=np.longdouble) - np.add.reduceat(prod, self.M.indptr[:-1], axis=0)

    def solve(self, B):
        X = self.chol.solve(np.asfortranarray(B))
        if self.plain:
            return X
        return np.asfortranarray(X + self.chol.solve(np.asfortranarray(self.residual(X, B).astype(np.float64))))

    def full_solve(self, V):
        out = np.zeros_like(V, order="F")
        out[:-1] = self.solve(V[:-1])
        return out

    def precond(self, Y, V):
        return orc.tangent_proj(self.dm, Y, self.full_solve(V))


def stpcg(hess, precon, g, Delta, kappa_fgr, theta, max_iters, dot=ldot):
    """Returns (states, exit): one dict per iteration that ran, exit in limit | boundary | curvature | target.
    A state holds what the device holds after that iteration: s, r, v, p (the NEW direction), Hp (of the direction the
    iteration started with, p_prev), and the scalars alpha, beta, kappa, rr, rv, sM; sig_prev / sig_next are the squared
    M-norms of the step before and after (what the trust-region test compares with Delta^2)."""
    s = np.zeros_like(g)
    r = g.copy()
    v = precon(r)
    p = -v
    r0 = math.sqrt(dot(r, r))
    r_v = dot(r, v)
    target = r0 * min(kappa_fgr, r0 ** theta)
    sig2, s_Mp, p_M2 = 0.0, 0.0, r_v
    states = []
    while len(states) < max_iters:
        Hp = hess(p)
        kappa = dot(p, Hp)
        alpha = r_v / kappa if kappa != 0 else float("inf")
        nxt = sig2 + 2 * alpha * s_Mp + alpha * alpha * p_M2
        st = dict(p_prev=p, Hp=Hp, kappa=kappa, kappa_rel=kappa / math.sqrt(dot(p, p) * dot(Hp, Hp)), alpha=alpha,
                  sig_prev=sig2, sig_next=nxt, target=target, r0=r0)
        states.append(st)
        if not (kappa > 0) or nxt >= Delta * Delta:
            tau = (-s_Mp + math.sqrt(s_Mp * s_Mp + p_M2 * (Delta * Delta - sig2))) / p_M2
            st.update(s=s + tau * p, r=r, v=v, p=p, tau=tau, sM=Delta, rr=dot(r, r), rv=r_v, beta=None)
            return states, ("boundary" if kappa > 0 else "curvature")
        s = s + alpha * p
        sig2 = nxt
        r = r + alpha * Hp
        v = precon(r)
        rr = dot(r, r)
        st.update(s=s, r=r, v=v, sM=math.sqrt(sig2), rr=rr)
        if math.sqrt(rr) <= target:
            st.update(p=p, rv=dot(r, v), beta=None)
            return states, "target"
        rv_new = dot(r, v)
        beta = rv_new / r_v
        r_v = rv_new
        p = -v + beta * p
        s_Mp = beta * (s_Mp + alpha * p_M2)
        p_M2 = r_v + beta * beta * p_M2
        st.update(p=p, rv=rv_new, beta=beta)
    return states, "limit"
