"""The level order of the chain placement from inter-robot ranges (include/cora_hip.h, cora_set_chain_placement_order) --
TEST INFRASTRUCTURE ONLY.  A pure-Python restatement of the rule, independent of the library, and the longdouble reference
of tests/placement_ref.py (its stage, its bound, its constant) run over the level lists.

The rule.  Level 0: the fixed chains (chain 0, or the chains of the mask).  Level k >= 1: every chain not yet placed whose
ranges against chains of levels < k number at least min_ranges, in ascending chain index; a stage's list holds the chain's
ranges against chains of levels < k only, in table order (a range to a chain of the same level is not in it).  The order
ends where a level would be empty; a chain left over has status 1 where it has a range to another chain, else 3."""
import numpy as np

import placement_ref as pl
from placement_ref import C_BOUND, CHUNK, EPS, LD, _norm, bits, check, diagonal_q, full_transform, solve_stage, unknowns  # noqa: F401

GREEDY, LEVELS = 0, 1


def structure(d, n, r, nt, table, chains, chain_fixed=None, min_ranges=None):
    """placement_ref.structure's dict for the level order, plus level (per stage, from 1) and level_of (per chain: 0 fixed,
    k, or -1 never placed)."""
    er, rr = np.asarray(table[0]), np.asarray(table[2])
    min_ranges = pl.default_min_ranges(d) if min_ranges is None else min_ranges
    nch = len(chains)
    positions, chain_of = [], {}
    for c, ch in enumerate(chains):
        pos = [(int(er[ch[0], 0]), int(er[ch[0], 2]))] + [(int(er[e, 1]), int(er[e, 3])) for e in ch]
        positions.append(pos)
        for _, trn in pos:
            chain_of[trn] = c
    level_of = [0 if (c == 0 if chain_fixed is None else bool(chain_fixed[c])) else -1 for c in range(nch)]
    use, skipped = [], 0
    for m in range(len(rr)):
        ca, cb = chain_of.get(int(rr[m, 1]), -1), chain_of.get(int(rr[m, 2]), -1)
        if ca < 0 or cb < 0 or ca == cb:
            skipped += 1
        else:
            use.append((m, ca, cb))
    stages, level, k = [], [], 1
    while True:
        lists = {c: dict(chain=c, q=[], a=[], m=[]) for c in range(nch) if level_of[c] < 0}
        for m, ca, cb in use:   # table order
            for mine, other, q, a in ((ca, cb, 1, 2), (cb, ca, 2, 1)):
                if mine in lists and level_of[other] >= 0:   # (levels < k: this level's chains are marked after the loop)
                    lists[mine]["q"].append(int(rr[m, q])), lists[mine]["a"].append(int(rr[m, a])), lists[mine]["m"].append(m)
        members = [c for c in sorted(lists) if len(lists[c]["m"]) >= min_ranges]
        if not members:
            break
        for c in members:
            stages.append(lists[c])
            level.append(k)
        for c in members:
            level_of[c] = k
        k += 1
    init = []
    for c in range(nch):
        any_range = any(c in (ca, cb) for _, ca, cb in use)
        init.append(4 if level_of[c] == 0 else 0 if level_of[c] > 0 else 1 if any_range else 3)
    entries = sum(len(s["m"]) for s in stages)
    chunks = sum((len(s["m"]) + CHUNK - 1) // CHUNK for s in stages)
    return dict(stages=stages, init=init, skipped=skipped, positions=positions, counts=(len(stages), entries, chunks, skipped), level=level,
                level_of=level_of)


def reference(d, n, r, nt, table, chains, X, gn_steps, chain_fixed=None, min_ranges=None, struct=None):
    """placement_ref.reference over the stages of `struct` (default: the level order's), stage after stage in table order --
    a legal dependent order of the levels.  The same dict."""
    rr, rd = np.asarray(table[2]), np.asarray(table[3], dtype=np.float64)
    X = np.array(X, dtype=LD)
    S = structure(d, n, r, nt, table, chains, chain_fixed, min_ranges) if struct is None else struct
    nch = len(chains)
    res = dict(struct=S, status=np.array(S["init"], dtype=np.uint8), chosen=np.full(nch, -1, dtype=np.int32),
               cost_start=np.zeros(nch, dtype=LD), cost_linear=np.zeros(nch, dtype=LD), cost_final=np.zeros(nch, dtype=LD), steps=0,
               transforms=np.tile(np.concatenate([np.eye(d).reshape(-1), np.zeros(d)]), (nch, 1)).astype(LD), stage=[], row_a={}, row_b={})
    for st in S["stages"]:
        qi, ai, ms = np.array(st["q"]), np.array(st["a"]), np.array(st["m"])
        q, a = X[qi], X[ai]
        one = solve_stage(d, q, a, rd[ms, 0].astype(LD), rd[ms, 1].astype(LD), gn_steps)
        c = st["chain"]
        res["status"][c], res["chosen"][c], res["steps"] = one["status"], one["chosen"], res["steps"] + one["steps"]
        res["cost_start"][c], res["cost_linear"][c], res["cost_final"][c] = one["costs"][0], one["costs"][1], one["costs"][one["chosen"]]
        R, t = full_transform(one, q[0], a[0], one["chosen"])
        res["transforms"][c] = np.concatenate([R.reshape(-1), t])
        L, tp = one["L"], float(_norm(one["visited"][one["chosen"]][1]))
        kap = max(one["kappa_lin"], one["kappa_gn"], 1.0)
        delta = max([res["row_a"].get(int(x), 0.0) for x in ai] + [0.0])
        one.update(q0=q[0].copy(), a0=a[0].copy(), rows_before={},
                   a=EPS * max(one["kappa_lin"] * (tp + L) ** 2 / L, one["kappa_gn"] * (tp + L), tp + L) + kap * delta)
        for rot, trn in S["positions"][c]:
            x = X[trn].copy()
            one["rows_before"][trn] = (x, X[rot:rot + d].copy())
            xn = R @ x + t
            X[rot:rot + d] = X[rot:rot + d] @ R.T
            X[trn] = xn
            res["row_a"][trn] = one["a"] * (1 + float(_norm(x - q[0])) / L)
            res["row_b"][trn] = EPS * float(_norm(q[0]) + _norm(a[0]) + _norm(t) + _norm(x) + _norm(xn))
        res["stage"].append(one)
    deg, norm = np.zeros(len(rr), dtype=bool), np.zeros(len(rr), dtype=LD)
    for m in range(len(rr)):
        diff = X[rr[m, 2]] - X[rr[m, 1]]
        nrm = norm[m] = np.sqrt(np.sum(diff * diff))
        deg[m] = nrm < 1e-5
        X[rr[m, 0]] = 0 if deg[m] else -diff / nrm
    res.update(X=X, degenerate=deg, norm=norm)
    return res
