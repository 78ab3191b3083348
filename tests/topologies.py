"""A catalogue of small named graphs whose SHAPE is the test: several robots, hubs, fat landmarks, reversed edges, priors,
duplicates, tiny pose counts -- the structures the one recipe of tests/synth.py (one chain, closures with i < j, ranges to a
few landmarks) never builds, each sized to reach one path of the format (cora_amd/csrc/format_build.cpp) and of the
product kernel (cora_amd/csrc/kernels/spmm.inc).  numpy only; the measurements are drawn from a ground truth plus noise
as synth.make_graph draws them, so that the tangent Hessian near the truth is positive semi-definite.

Every entry of CATALOGUE names what it targets (its builder's docstring) and declares the shape it must have
(Context.format_shape / format_stats, one handle): tests/test_topologies_cpu.py asserts the declaration without a GPU,
tests/test_gpu_topologies.py again on the device handle, so that no case can silently miss its path.  The table with the
observed numbers is profiles/topologies.md."""
import numpy as np

from oracle import assemble as asm
from oracle import oracle as orc
from synth import _rot

K_LONG_ROW = 96      # cora_internal.h kLongRow: translation rows above it go to the chunk path
K_LONG_CHUNK = 1024  # kLongChunk: non-zeros of one chunk of a long row


class World:
    """Ground truth (poses by index, landmarks) and the PyFG of the measurements drawn from it."""

    def __init__(self, d, seed, step=1.0):
        self.d = d
        self.step = step   # length scale of the world (distance between consecutive poses)
        self.rng = np.random.default_rng(seed)
        self.g = asm.PyFG()
        self.g.dim = d
        self.R, self.T, self.names = [], [], []
        self.L = []
        self.pos = {}   # symbol -> position (poses and landmarks)
        self.cov = np.diag([0.05 ** 2] * d + [0.01 ** 2] * (3 if d == 3 else 1))
        self.covt = np.eye(d) * 0.05 ** 2
        self.covp = np.diag([0.5 ** 2] * d + [0.1 ** 2] * (3 if d == 3 else 1))   # priors: weak, as priors are

    # ---- variables
    def robot(self, letter, n):
        """A random-walk trajectory of n poses `letter`0 .. ; returns their pose indices."""
        d, rng = self.d, self.rng
        assert not self.g.has_priors, "poses before priors: the origin pose is the last one"
        R = _rot(d, rng, 1.0) if self.names else np.eye(d)
        t = self.step * rng.uniform(-10, 10, d) if self.names else np.zeros(d)
        e1 = np.zeros(d)
        e1[0] = 1.0
        idx = []
        for i in range(n):
            if i:
                t = t + self.step * (R @ (e1 + rng.normal(0, 0.1, d)))
                R = R @ _rot(d, rng, 0.05)
            name = "%s%d" % (letter, i)
            self.g._add_pose(name)
            idx.append(len(self.names))
            self.names.append(name)
            self.R.append(R)
            self.T.append(t)
            self.pos[name] = t
        return idx

    def landmarks(self, k):
        T = np.array(self.T)
        lo, hi = T.min(0) - 20 * self.step, T.max(0) + 20 * self.step
        out = []
        for _ in range(k):
            name = "L%d" % len(self.L)
            self.g.landmarks[name] = len(self.L)
            p = self.rng.uniform(lo, hi)
            self.L.append(p)
            self.pos[name] = p
            out.append(name)
        return out

    # ---- measurements
    def rel_pose(self, i, j):
        """Relative pose measured FROM pose i TO pose j (indices): i > j is an edge recorded backwards."""
        d, rng = self.d, self.rng
        Rm = self.R[i].T @ self.R[j] @ _rot(d, rng, 0.01)
        tm = self.R[i].T @ (self.T[j] - self.T[i]) + self.step * rng.normal(0, 0.05, d)
        self.g.rpms.append((self.names[i], self.names[j], Rm, tm, self.cov))

    def odometry(self, idx, reverse_every=0, duplicate_every=0):
        for k in range(len(idx) - 1):
            a, b = idx[k], idx[k + 1]
            if reverse_every and k % reverse_every == reverse_every - 1:
                a, b = b, a
            self.rel_pose(a, b)
            if duplicate_every and k % duplicate_every == 0:
                self.rel_pose(a, b)

    def range(self, a, b):
        """Range between two symbols (poses or landmarks)."""
        dist = np.linalg.norm(self.pos[a] - self.pos[b]) + self.step * self.rng.normal(0, 0.1)
        self.g.ranges.append((a, b, abs(float(dist)), 0.01))

    def pose_landmark(self, i, lm):
        tm = self.R[i].T @ (self.pos[lm] - self.T[i]) + self.step * self.rng.normal(0, 0.05, self.d)
        self.g.rplms.append((self.names[i], lm, tm, self.covt))

    def pose_prior(self, i):
        Rm = self.R[i] @ _rot(self.d, self.rng, 0.01)
        tm = self.T[i] + self.step * self.rng.normal(0, 0.05, self.d)
        self.g.pose_priors.append((self.names[i], Rm, tm, self.covp))
        self.g._origin()

    def pick(self, pool, k):
        """k distinct members of a list."""
        return [pool[i] for i in self.rng.choice(len(pool), size=k, replace=False)]

    # ---- what the tests take
    def truth(self):
        """N x d: the point the measurements were drawn from, in the rows of Q (the origin pose of a graph with priors
        is the last pose: identity at zero)."""
        d, g = self.d, self.g
        R, T = list(self.R), list(self.T)
        if g.has_priors:
            R.append(np.eye(d))
            T.append(np.zeros(d))
        n, r, l = len(R), len(g.ranges), len(self.L)
        assert n == len(g.poses)
        X = np.zeros(((d + 1) * n + r + l, d))
        for i in range(n):
            X[d * i:d * i + d] = R[i].T
        for k, (a, b, _, _) in enumerate(g.ranges):
            v = self.pos[a] - self.pos[b]
            X[d * n + k] = v / np.linalg.norm(v)
        X[d * n + r:d * n + r + n] = T
        if l:
            X[d * n + r + n:] = self.L
        return X


def _chain(w, letter, n, loops=0, **kw):
    idx = w.robot(letter, n)
    w.odometry(idx, **kw)
    seen = set()
    while len(seen) < loops:   # loop closures in both index directions
        i, j = (int(x) for x in w.rng.choice(idx, size=2, replace=False))
        if abs(i - j) < 2 or (i, j) in seen or (j, i) in seen:
            continue
        seen.add((i, j))
        w.rel_pose(i, j)
    return idx


def _spread(w, lm, poses, k):
    """k ranges from k distinct poses of `poses` to landmark lm."""
    for i in w.pick(poses, k):
        w.range(w.names[i], lm)


# ---------------------------------------------------------------- the entries
# A prior measures a pose against the origin, so Q holds tau |t|^2 with t the pose's POSITION, not a step of the walk.  At
# a step of 1 and the odometry's covariances the 150-pose graphs have entries of 1e8 in Q and of 1e6 in the Lambda
# blocks, which cancel from products of 1e10: rounding alone is 1e-8 there, above the ABSOLUTE 1e-9 the Lambda blocks
# are held to (tests/test_gpu_parity.py TOL; observed 9e-8 on the device, 1e-17 of the products).  The graphs with priors
# therefore live in a small world with weak priors (World.covp): the same structure, Lambda blocks below 1e3.
PRIOR_STEP = 0.05


def robots(d):
    """Robots of 64, 37 and 100 poses, 40 inter-robot pose-pose ranges, 12 closures in both directions, landmarks with 5,
    30 and 60 ranges: a robot boundary on a slice edge (zero head block, last lane without a successor) and one
    mid-slice; other poses' translation rows in the tails; landmark rows in the row slices and on the chunk path."""
    w = World(d, 100 + d)
    rb = [_chain(w, c, n, loops=4) for c, n in (("A", 64), ("B", 37), ("C", 100))]
    every = rb[0] + rb[1] + rb[2]
    seen = set()
    while len(seen) < 40:
        a, b = (int(x) for x in w.rng.choice(3, size=2, replace=False))
        i, j = int(w.rng.choice(rb[a])), int(w.rng.choice(rb[b]))
        if (i, j) in seen or (j, i) in seen:
            continue
        seen.add((i, j))
        w.range(w.names[i], w.names[j])
    for lm, k in zip(w.landmarks(3), (5, 30, 60)):
        _spread(w, lm, every, k)
    return w


def reversed_edges(d=3):
    """One chain of 130, every third odometry edge recorded successor -> predecessor, 9 closures (both directions):
    column t_{P-1} in the general slots of a lane, rot(P+1) columns in its tail."""
    w = World(d, 7)
    idx = _chain(w, "A", 130, reverse_every=3)
    for i, j in ((90, 20), (120, 64), (63, 5), (129, 0), (70, 10), (100, 69), (40, 3), (65, 63), (128, 126)):
        w.rel_pose(i, j)   # j < i
    for lm in w.landmarks(2):
        _spread(w, lm, idx, 20)
    return w


def hub(d):
    """100 poses; pose 70 (lane 6 of slice 1) with 60 ranges to 60 landmarks, every landmark with 2 more: a pose's
    translation row above kLongRow -- its slice keeps the plain layout, the pose row goes to the chunk path and the 35
    other translation rows of the slice go back to row slices."""
    w = World(d, 20 + d)
    idx = _chain(w, "A", 100, loops=3)
    others = [i for i in idx if i != 70]
    for lm in w.landmarks(60):
        w.range(w.names[70], lm)
        _spread(w, lm, others, 2)
    return w


def near_hub(d=3):
    """100 poses; pose 70 with 43 ranges (interior row at d = 3: 9 + 2 x 43 = 95 non-zeros, the longest that stays at or
    below kLongRow), lanes 0-5 of its slice with 5 ranges each (the hub's pairs 30..72 straddle the 64-pair round) and
    every later lane with 3: the longest lane tail, T > 64, all in the chain layout."""
    w = World(d, 31)
    idx = _chain(w, "A", 100)
    lms = w.landmarks(43)
    for lm in lms:
        w.range(w.names[70], lm)
    for i in range(64, 100):
        if i != 70:
            for lm in w.pick(lms, 5 if i < 70 else 3):
                w.range(w.names[i], lm)
    for i in (3, 17, 40):
        w.range(w.names[i], lms[0])
    return w


def fat_landmark(d=3):
    """130 poses; L0 with 63 ranges from EVERY pose (row of 1 + 130 + 8190 non-zeros: 9 chunks), L1 with a row of exactly
    kLongChunk non-zeros, L2 with kLongChunk + 1: the ticket hand-off of a multi-chunk row, its 8-unrolled partial sum
    with a remainder, a one-entry last chunk, the kappa slot of a long row."""
    w = World(d, 41)
    idx = _chain(w, "A", 130)
    l0, l1, l2 = w.landmarks(3)
    for i in idx:
        for _ in range(63):
            w.range(w.names[i], l0)
    for lm, row in ((l1, K_LONG_CHUNK), (l2, K_LONG_CHUNK + 1)):
        k = row - 1 - len(idx)   # the diagonal, one column per pose, one per range
        for c in range(k):
            w.range(w.names[idx[c % len(idx)]], lm)
    return w


def rplm_priors(d=2):
    """Two robots (70 and 45 poses), 60 pose-landmark translation measurements, 7 pose priors, a few ranges: landmark
    columns in the general slots, the origin pose as the last lane with the priors' poses in its general slots."""
    w = World(d, 51, step=PRIOR_STEP)
    a, b = _chain(w, "A", 70, loops=2), _chain(w, "B", 45, loops=2)
    lms = w.landmarks(8)
    for i in w.pick(a + b, 60):
        w.pose_landmark(i, lms[int(w.rng.integers(len(lms)))])
    for lm in lms[:3]:
        _spread(w, lm, a + b, 12)
    for i in w.pick(a + b, 7):
        w.pose_prior(i)
    return w


def _priors(d, n, which, seed):
    w = World(d, seed, step=PRIOR_STEP)
    idx = _chain(w, "A", n, loops=2)
    for lm in w.landmarks(2):
        _spread(w, lm, idx, 15)
    for i in which:
        w.pose_prior(i)
    return w


def priors_wide(d=3):
    """150 poses, priors on 104 of them: the origin pose's translation row is above kLongRow (a long POSE row, the last
    slice in the plain layout with more than 300 slots per lane)."""
    return _priors(d, 150, list(range(0, 104)), 61)


def priors_chain_even(d=3):
    """150 poses, priors on 85 (not the origin's index predecessor): the origin lane stays in the chain layout with
    4 x 85 = 340 general slots (even width through the unrolled slot loop) and a tail of 85 entries."""
    return _priors(d, 150, list(range(10, 95)), 62)


def priors_chain_odd(d=3):
    """The same with the origin's index predecessor among the 85: its rotation block is the implied previous block, its
    translation one general slot -- 4 x 84 + 1 = 337 general slots, an odd width."""
    return _priors(d, 150, list(range(10, 94)) + [149], 63)


def lm_lm(d=2):
    """70 poses, 6 landmarks, 40 pose-landmark ranges and 8 landmark-landmark ranges (no pose on either end)."""
    w = World(d, 71)
    idx = _chain(w, "A", 70, loops=2)
    lms = w.landmarks(6)
    for lm in lms:
        _spread(w, lm, idx, 7)
    for k in range(8):
        w.range(lms[k % 6], lms[(k + 1 + k // 6) % 6])
    return w


def dups(d=3):
    """70 poses, every fifth odometry edge and every range measured twice (different noise): entries that are sums."""
    w = World(d, 81)
    idx = _chain(w, "A", 70, duplicate_every=5)
    for lm in w.landmarks(3):
        for i in w.pick(idx, 10):
            w.range(w.names[i], lm)
            w.range(w.names[i], lm)
    w.range(w.names[5], w.names[40])
    w.range(w.names[5], w.names[40])
    return w


def pp_only(d=2):
    """Two robots (40 and 50 poses), no landmark, 30 pose-pose ranges between them: l = 0, every tail column a pose."""
    w = World(d, 91)
    a, b = _chain(w, "A", 40), _chain(w, "B", 50)
    seen = set()
    while len(seen) < 30:
        i, j = int(w.rng.choice(a)), int(w.rng.choice(b))
        if (i, j) not in seen:
            seen.add((i, j))
            w.range(w.names[i], w.names[j])
    return w


def _tiny(n, d, seed, split=None):
    w = World(d, seed)
    if split:
        idx = _chain(w, "A", split) + _chain(w, "B", n - split)
        for k in range(6):
            w.range(w.names[idx[5 * k]], w.names[idx[split + 7 * k]])
    else:
        idx = _chain(w, "A", n, loops=2 if n > 10 else 0)
    lms = w.landmarks(2)
    for lm in lms:
        _spread(w, lm, idx, min(n, 20))
    if n == 1:   # one pose: a pose-landmark measurement gives its rotation rows something to hold
        w.pose_landmark(0, lms[0])
        w.range(lms[0], lms[1])
    return w


def n1(d=3):
    """One pose, two landmarks: one single-lane slice, no chain neighbour."""
    return _tiny(1, d, 201)


def n2(d=3):
    """Two poses."""
    return _tiny(2, d, 202)


def n63(d=2):
    """63 poses: one slice, one lane short of full."""
    return _tiny(63, d, 203)


def n64(d=3):
    """64 poses: exactly one full slice (the last lane has no successor)."""
    return _tiny(64, d, 204)


def n65(d=2):
    """65 poses: a second slice of one lane whose predecessor is the head block."""
    return _tiny(65, d, 205)


def n128(d=3):
    """Two robots of 64: two full slices, the robot boundary on the slice edge."""
    return _tiny(128, d, 206, split=64)


def singletons(d=3):
    """Robots of 1, 1, 30 and 1 poses tied together by ranges only: lanes with no chain neighbour at all, in the middle
    and at the end of a slice."""
    w = World(d, 211)
    a, b = w.robot("A", 1), w.robot("B", 1)
    c = _chain(w, "C", 30)
    e = w.robot("E", 1)
    lm = w.landmarks(1)[0]
    for i, j in ((a[0], b[0]), (a[0], c[3]), (b[0], c[10]), (e[0], c[29]), (e[0], a[0]), (b[0], e[0]), (a[0], c[20])):
        w.range(w.names[i], w.names[j])
    for i in (a[0], b[0], e[0], c[0], c[15]):
        w.range(w.names[i], lm)
    return w


# name -> (builder, d, declared shape: key -> (at least, at most); None = no bound).  Keys of Context.format_shape() on ONE
# handle, plus "slices"/"max_width"/"long_rows" of Context.format_stats().
CATALOGUE = {}


def _entry(name, fn, d, **shape):
    CATALOGUE[name] = (fn, d, shape)


ALL_CHAIN = dict(plain_slices=(0, 0), long_pose_rows=(0, 0))
for _d in (2, 3):
    _entry("robots-d%d" % _d, robots, _d, chain_slices=(4, 4), long_landmark_rows=(1, 1), max_general=(1, None), **ALL_CHAIN)
    _entry("hub-d%d" % _d, hub, _d, chain_slices=(1, 1), plain_slices=(1, 1), long_pose_rows=(1, 1))
_entry("reversed", reversed_edges, 3, chain_slices=(3, 3), max_general=(2, None), **ALL_CHAIN)
_entry("near_hub", near_hub, 3, chain_slices=(2, 2), max_T=(65, None), max_lane_tail=(43, 43), slices_T_gt_64=(1, None),
       straddling_tails=(1, None),
       **ALL_CHAIN)
_entry("fat_landmark", fat_landmark, 3, chain_slices=(3, 3), long_landmark_rows=(3, 3), max_chunks=(9, None), **ALL_CHAIN)
_entry("rplm_priors", rplm_priors, 2, chain_slices=(2, 2), max_general=(21, None), **ALL_CHAIN)
_entry("priors_wide", priors_wide, 3, plain_slices=(1, 1), chain_slices=(2, 2), long_pose_rows=(1, 1), max_width=(301, None))
_entry("priors_chain_even", priors_chain_even, 3, chain_slices=(3, 3), max_general=(340, 340), max_lane_tail=(43, 43),
       **ALL_CHAIN)
_entry("priors_chain_odd", priors_chain_odd, 3, chain_slices=(3, 3), max_general=(337, 337), **ALL_CHAIN)
_entry("lm_lm", lm_lm, 2, chain_slices=(2, 2), **ALL_CHAIN)
_entry("dups", dups, 3, chain_slices=(2, 2), **ALL_CHAIN)
_entry("pp_only", pp_only, 2, chain_slices=(2, 2), long_landmark_rows=(0, 0), max_T=(1, None), **ALL_CHAIN)
_entry("n1", n1, 3, chain_slices=(1, 1), **ALL_CHAIN)
_entry("n2", n2, 3, chain_slices=(1, 1), **ALL_CHAIN)
_entry("n63", n63, 2, chain_slices=(1, 1), **ALL_CHAIN)
_entry("n64", n64, 3, chain_slices=(1, 1), **ALL_CHAIN)
_entry("n65", n65, 2, chain_slices=(2, 2), **ALL_CHAIN)
_entry("n128", n128, 3, chain_slices=(2, 2), **ALL_CHAIN)
_entry("singletons", singletons, 3, chain_slices=(1, 1), max_T=(1, None), **ALL_CHAIN)
NAMES = list(CATALOGUE)

_BUILT = {}


def build(name):
    """(A, Q, dm, g) of a catalogue entry, built once per process and shared: A = oracle.assemble's matrices plus
    A["truth"] (N x d), Q the oracle's CSR, dm its Dims, g the PyFG."""
    if name not in _BUILT:
        fn, d, _ = CATALOGUE[name]
        w = fn(d)
        A = asm.assemble(w.g)
        A["truth"] = w.truth()
        Q = orc.CSR.from_scipy(A["Q"])
        dm = orc.Dims(A["d"], A["n"], A["r"], A["N"])
        assert A["truth"].shape == (dm.N, d)
        _BUILT[name] = (A, Q, dm, w.g)
    return _BUILT[name]


def shape_of(ctx):
    """format_shape() and the format_stats() fields a declaration may name."""
    s = ctx.format_shape()
    st = ctx.format_stats()
    s.update(slices=st["slices"], max_width=st["max_width"], long_rows=st["long_rows"])
    return s


def check_shape(name, ctx):
    """The entry's declared shape holds on this (unpartitioned) handle; returns the observed shape."""
    got = shape_of(ctx)
    for key, (lo, hi) in CATALOGUE[name][2].items():
        assert lo is None or got[key] >= lo, (name, key, got[key], "at least", lo)
        assert hi is None or got[key] <= hi, (name, key, got[key], "at most", hi)
    return got


def near_truth(name, p, noise=0.02, seed=0):
    """A point of the manifold at rank p near the lifted ground truth (rotated in R^p, every entry perturbed): the
    tangent Hessian has positive curvature along the gradient there."""
    A, Q, dm, g = build(name)
    rng = np.random.default_rng(1000 * seed + p)
    R, _ = np.linalg.qr(rng.standard_normal((p, p)))
    lifted = np.hstack([A["truth"], np.zeros((dm.N, p - dm.d))])
    return orc.project_manifold(dm, (lifted + noise * rng.standard_normal((dm.N, p))) @ R)


def has_duplicates(name):
    """Whether the graph repeats a measurement between the same two symbols (dups, fat_landmark)."""
    g = build(name)[3]
    pairs = [(m[0], m[1]) for m in g.rpms] + [("r", m[0], m[1]) for m in g.ranges]
    return len(set(pairs)) < len(pairs)


def to_problem(name, rank=None, precond=None):
    """The same graph fed into the C++ host through its programmatic API (host.Problem.new + add_*), updated.  The host
    refuses a second measurement between the same two symbols, as the reference's CORA::Problem does: the entries with
    duplicates exist as matrices only (capi.Context)."""
    from cora_amd import capi, host
    A, Q, dm, g = build(name)
    if has_duplicates(name):
        raise ValueError("%s repeats measurements: CORA::Problem refuses them" % name)
    P = host.Problem.new(g.dim, rank=rank or g.dim, precond=capi.PRECOND_JACOBI if precond is None else precond)
    for sym, _ in sorted(g.poses.items(), key=lambda kv: kv[1]):
        if not (g.has_priors and sym == "O0"):
            P.add_pose(sym)
    for sym, _ in sorted(g.landmarks.items(), key=lambda kv: kv[1]):
        P.add_landmark(sym)
    for a, b, R, t, cov in g.rpms:
        P.add_rel_pose(a, b, R, t, cov)
    for s, R, t, cov in g.pose_priors:
        P.add_pose_prior(s, R, t, cov)
    for a, b, t, cov in g.rplms:
        P.add_rel_pose_landmark(a, b, t, cov)
    for a, b, dist, cov in g.ranges:
        P.add_range(a, b, dist, cov)
    P.update()
    return P
