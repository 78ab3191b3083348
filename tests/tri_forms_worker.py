"""The staged Cholesky solve (k_rowop, k_blockop, k_subblock: cora_amd/csrc/kernels/tri.inc) on every form of the solve
plan and on factors of arbitrary structure, as a PROCESS of its own: python tests/tri_forms_worker.py <set> [host]

A process per ENVIRONMENT SET, because the switches that decide a plan's form and its row classes are read once, when
the library loads; the switches read per call (CORA_TRI_SUB, CORA_TRI_UNFOLD_MIN, CORA_SUB_IO_LISTS) are flipped around
single installs.  The child prints one line `CASE {json}` per case -- its id, the plan's shape as the probe reports it
(cora_debug_factor_shape on the handle; `host`: cora_debug_factor_image for the same factor, row map, groups and layout on
a plan-only handle -- and on the device the two must agree in every field but the install count), discrete mismatches (`fail`) and the worst
deviations (`checks`: [name, value, kind]; the bound of each kind lives in BOUND below) -- and ends with `DONE`.  Any error
of the library that a case does not expect is an exception nothing catches: the exit status is non-zero.

`host` (no GPU; tests/test_tri_forms_cpu.py): the same cases with the plan built and executed on the host
(cora_debug_factor_solve_host), and the reference against itself (refined against unrefined solve, kind spread-*).

Sets and what their fixtures (tests/tri_forms.py) give -- asserted case by case, so a fixture that drifts to another
form fails instead of testing something else:
  A   CORA_TRI_TOP_INV=20000: substitution blocks (aux sums folded / as their own product, row I/O from run tables / from
      index lists), dense blocks in 2 and 3 stages, an incomplete factor, a branching tree whose tiles exceed 64 KB of LDS
  B   defaults: one explicit inverse
  C   CORA_TRI_CHUNK=64 CORA_TRI_WAVE_ROW=64 CORA_TRI_SHORT_ROW=8: one inverse of order 4300 whose longest rows have more
      than 64 chunks (the ticket reduction's second round), all three row classes in one product
  C0  the same with CORA_TRI_TOP_INV=0: substitution blocks above 64 KB whose top stage has long rows, dense blocks with
      every row class in three products.  (Under CORA_TRI_TOP_INV=0 no plan is one inverse beyond 1536 rows, so no row
      reaches 64 chunks of 64 entries there: that case is C's.)
  P   CORA_TRI_TOP_INV=20000, the preconditioner's entry: Q + lambda I of a synthetic graph factorised in numpy, N - 1 rows"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# the project's own bounds for these plans (tests/test_trisolve_cpu.py, tests/test_gpu_stpcg_forms.py): relative to the
# largest entry of the reference.  spread-*: the reference against itself, 1/100 of the bound it serves.
BOUND = {"complete": 1e-11, "incomplete": 1e-10, "reg": 1e-8, "prod": 1e-10, "vec": 1e-9}
BOUND.update({"spread-" + k: v / 100 for k, v in list(BOUND.items())})
TILE_LIMIT = 64 * 1024   # dynamic LDS a kernel gets without asking
COLUMNS = list(range(1, 25))

ENV = {
    "A": {"CORA_TRI_TOP_INV": "20000"},
    "B": {},
    "C": {"CORA_TRI_CHUNK": "64", "CORA_TRI_WAVE_ROW": "64", "CORA_TRI_SHORT_ROW": "8"},
    "C0": {"CORA_TRI_TOP_INV": "0", "CORA_TRI_CHUNK": "64", "CORA_TRI_WAVE_ROW": "64", "CORA_TRI_SHORT_ROW": "8"},
    "P": {"CORA_TRI_TOP_INV": "20000"},
}
SUB0 = {"CORA_TRI_SUB": "0"}
UNFOLD = {"CORA_TRI_UNFOLD_MIN": "0"}
LISTS = {"CORA_SUB_IO_LISTS": "1"}

# (id, fixture, permutation, switches of the install, expected shape: key -> value | (lo, hi) with None = open)
PLAIN, DENSE, SUB = 0, 1, 2
AUX_CASES = {
    "A": [
        ("sub-fold-scrambled", "ndchain-1700", "scrambled", {},
         dict(form=SUB, stages=2, blocks=(3, None), aux_sum=0, io_runs=0, max_npl=8)),
        ("sub-fold-runs", "ndchain-1700", "identity", {}, dict(form=SUB, stages=2, blocks=(3, None), aux_sum=0, io_runs=1)),
        ("sub-fold-lists", "ndchain-1700", "identity", LISTS, dict(form=SUB, stages=2, aux_sum=0, io_runs=0)),
        ("sub-auxsum", "ndchain-1700", "scrambled", UNFOLD, dict(form=SUB, stages=2, aux_sum=1, io_runs=0)),
        ("sub-auxsum-runs", "ndchain-1700", "identity", UNFOLD, dict(form=SUB, stages=2, aux_sum=1, io_runs=1)),
        ("dense-2-stages", "ndchain-1700", "scrambled", SUB0, dict(form=DENSE, stages=2, blocks=(30, None))),
        ("sub-2600", "ndchain-2600", "identity", {}, dict(form=SUB, stages=2, blocks=(10, None), io_runs=1)),
        ("dense-3-stages", "random-2600", "scrambled", {}, dict(form=DENSE, stages=3, blocks=(100, None))),
        ("incomplete", "incomplete-2600", "scrambled", {}, dict(form=DENSE, stages=3, blocks=(100, None))),
        ("dense-2600-chain", "ndchain-2600", "scrambled", SUB0, dict(form=DENSE, stages=2, blocks=(50, None))),
        ("dense-random-1600", "random-1600", "scrambled", {},
         dict(form=DENSE, stages=2, blocks=(100, None), block_rows=64, mixed_products=(1, None))),
        ("sub-tree-64k", "tree-2000", "scrambled", {},
         dict(form=SUB, stages=2, blocks=(10, None), max_rows=(342, None), lds24=(TILE_LIMIT + 1, None), io_runs=0)),
        ("dense-tree", "tree-2000", "identity", SUB0, dict(form=DENSE, stages=2, blocks=(30, None))),
        ("arrow", "arrow-2500", "scrambled", {}, dict(form=DENSE, stages=3, mixed_products=(1, None))),
    ],
    "B": [
        ("inverse-chain", "ndchain-1700", "scrambled", {}, dict(form=PLAIN, stages=1, top_rows=1700, mixed_products=(1, None))),
        ("inverse-random", "random-1600", "identity", {}, dict(form=PLAIN, stages=1, top_rows=1600, long_rows=(1, None))),
        ("inverse-tree", "tree-2000", "scrambled", {}, dict(form=PLAIN, stages=1, top_rows=2000)),
    ],
    "C": [
        ("inverse-64-chunks", "ndchain-4300", "scrambled", {},
         dict(form=PLAIN, stages=1, top_rows=4300, max_chunks=(65, None), mixed_products=(1, None))),
    ],
    "C0": [
        ("sub-long-top-64k", "ndchain-4300", "identity", {},
         dict(form=SUB, stages=2, blocks=(10, None), max_rows=(342, None), lds24=(TILE_LIMIT + 1, None), io_runs=1,
              long_rows=(1, None), mixed_products=(1, None))),
        ("sub-long-top-auxsum", "ndchain-4300", "scrambled", UNFOLD,
         dict(form=SUB, stages=2, aux_sum=1, io_runs=0, lds24=(TILE_LIMIT + 1, None), mixed_products=(1, None))),
        ("dense-every-class", "ndchain-4300", "scrambled", SUB0,
         dict(form=DENSE, stages=2, blocks=(50, None), mixed_products=(3, None), max_chunks=(33, None))),
    ],
}
HOST_KEYS = ("generation",)   # what only an install on a device knows
IMAGE_KEYS = ("io_runs", "fuse_ok")   # what the device image of a plan decides (cora_debug_factor_image), not the plan


def case_ids(which):
    if which == "P":
        return (["precond-%s" % f for f in ("sub", "sub-split", "dense")] +
                ["proj-%s-p%d" % (f, p) for f in ("sub", "sub-split", "dense") for p in PROJ_RANKS] + ["stpcg-dense"])
    ids = [c[0] for c in AUX_CASES[which]]
    if which == "A":
        ids.append("reinstall")
    if which == "B":
        ids.append("errors")
    return ids


def emit(case, **kw):
    kw["id"] = case
    print("CASE " + json.dumps(kw), flush=True)


class switches:
    """environment variables the library reads per call, set around one call"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k in self.env:
            os.environ.pop(k, None)


class Checks:
    """Worst value per name over everything a case compares."""

    def __init__(self):
        self.worst, self.fail = {}, []

    def add(self, name, value, kind):
        value = float(value)
        if not math.isfinite(value):
            self.fail.append("%s is not finite" % name)
            value = 1e300
        if name not in self.worst or value > self.worst[name][0]:
            self.worst[name] = (value, kind)

    def expect(self, what, got, want):
        if got != want:
            self.fail.append("%s: %r, expected %r" % (what, got, want))

    def shape(self, got, want):
        for key, w in want.items():
            g = got[key]
            if isinstance(w, tuple):
                if (w[0] is not None and g < w[0]) or (w[1] is not None and g > w[1]):
                    self.fail.append("plan %s = %d outside %r" % (key, g, w))
            elif g != w:
                self.fail.append("plan %s = %d, expected %d" % (key, g, w))

    def out(self):
        return dict(fail=self.fail, checks=[[k, v[0], v[1]] for k, v in sorted(self.worst.items())])


def rel(got, ref):
    import tri_forms as TF
    return TF.rel_err(got, ref)


def host_plan(L, env):
    from cora_amd import capi
    with switches(env):
        return capi.factor_plan_host(L.indptr, L.indices, L.data)


def host_solve(L, B, env):
    """X = (L L^T)^-1 B by the plan's products executed on the host, in launch order."""
    import ctypes as C
    from cora_amd import capi
    lib = capi.load()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    Lp, Li, Lx = capi._csc_factor(L.indptr, L.indices, L.data)
    B = np.asfortranarray(B, dtype=np.float64)
    X = np.zeros_like(B, order="F")
    with switches(env):
        rc = lib.cora_debug_factor_solve_host(L.shape[0], Lp.ctypes.data_as(ip), Li.ctypes.data_as(ip), Lx.ctypes.data_as(dp),
                                              B.shape[1], B.ctypes.data_as(dp), X.ctypes.data_as(dp), None)
    if rc:
        raise RuntimeError(lib.cora_last_error(None).decode())
    return X


# ---------------------------------------------------------------- handles
_handles = {}


def handle(N, device=True):
    """A handle whose vectors have N rows (d = 2: N = 3 n + l + r with l = 3), one per N and process; on the device, or
    plan-only (the same format and row order, no GPU)."""
    if N not in _handles:
        from cora_amd import capi
        from synth import make_problem
        n = N // 4
        A, Q, dm = make_problem(d=2, n=n, n_landmarks=3, n_ranges=N - 3 * n - 3, n_loops=3, seed=N)
        assert dm.N == N
        _handles[N] = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, device=0 if device else -1)
    return _handles[N]


def image_shape(h, L, perm, env, grouped=False):
    """The shape cora_debug_factor_image gives an install of L on h under perm (API rows, new -> old): the handle's row
    map, its rotation rows and vector length; grouped: the groups cora_precond_set_cholesky forms (a pose's rotation
    rows), and the pinned row where the factor leaves one out."""
    from cora_amd import capi
    rm, dn = h.row_map(), h.d * h.n
    rot0 = int(rm[:dn].min())
    assert np.array_equal(rm[:dn], rot0 + np.arange(dn)), "rotation rows are not one run of the internal order"
    left = np.setdiff1d(np.arange(h.N), perm)
    assert len(left) <= 1
    with switches(env):
        return capi.factor_image(L.indptr, L.indices, L.data, row_map=rm[perm], group=np.where(perm < dn, perm // h.d, -1) if grouped else None,
                                 d=h.d, rot0=rot0, rot1=rot0 + dn, rows=h.rows, zero_row=int(rm[left[0]]) if len(left) else -1)[1]


def expect_image(C, shape, img):
    """an install reports what the image hook derives without a device"""
    from cora_amd import capi
    for key in capi.SHAPE_KEYS:
        if key not in HOST_KEYS:
            C.expect("installed plan %s against cora_debug_factor_image" % key, shape[key], img[key])


def permutation(h, fx, how):
    """perm (new -> old, API rows) of the fixture's factor on the handle.  identity: the factor's row i lands on the
    handle's i-th internal row -- the identity in the order the vectors are stored in, so a subtree of a factor in
    nested-dissection order (a run of consecutive factor rows) is one run of consecutive rows of the vectors;
    scrambled: anywhere."""
    N = fx["n"]
    if how == "scrambled":
        return np.random.default_rng(N + 7).permutation(N).astype(np.int32)
    return np.argsort(h.row_map(), kind="stable").astype(np.int32)   # API row of the i-th internal row


class Vectors:
    """right-hand side and solution vectors of every column count on one handle"""

    def __init__(self, h):
        self.h = h
        self.v = {k: (h.dev_alloc(k), h.dev_alloc(k)) for k in COLUMNS}

    def close(self):
        for b, x in self.v.values():
            self.h.dev_free(b)
            self.h.dev_free(x)


def solve_checks(C, h, vec, perm, B, X, kind, Xhost=None):
    """Every column count: the solve against the reference; nothing of the NaN prefill left; the right-hand side untouched;
    the same bits from a second solve and from a third one after a solve with another column count."""
    N = len(perm)
    Bapi, Xapi = np.empty_like(B), np.empty_like(X)
    Bapi[perm], Xapi[perm] = B, X
    nan = np.full((N, 24), np.nan, order="F")
    for k in COLUMNS:
        h.upload(Bapi[:, :k], vec.v[k][0])
    for k in COLUMNS:
        b, x = vec.v[k]
        other = k % 24 + 1
        runs = []
        for rep in range(3):
            h.upload(nan[:, :k], x)
            if rep == 2:
                h.upload(nan[:, :other], vec.v[other][1])
                h.aux_solve_dev(vec.v[other][0], other, vec.v[other][1])
            h.aux_solve_dev(b, k, x)
            runs.append(h.download(x, k))
        got = runs[0]
        if not np.all(np.isfinite(got)):
            C.fail.append("k = %d: %d entries of the solution are not finite" % (k, int((~np.isfinite(got)).sum())))
            continue
        C.expect("k = %d: right-hand side unchanged" % k, bool(np.array_equal(h.download(b, k), Bapi[:, :k])), True)
        C.expect("k = %d: second solve bit-identical" % k, bool(np.array_equal(runs[1], got)), True)
        C.expect("k = %d: solve after a solve of %d columns bit-identical" % (k, other), bool(np.array_equal(runs[2], got)), True)
        C.add("x", rel(got, Xapi[:, :k]), kind)
        C.add("x.k%d" % k, rel(got, Xapi[:, :k]), "info")
        if Xhost is not None:
            C.add("x-host", rel(got[perm], Xhost[:, :k]), "info")


def aux_case(spec, device, state):
    import tri_forms as TF
    from cora_amd import capi
    cid, name, how, env, want = spec
    fx = TF.fixture(name)
    kind = "incomplete" if fx["A"] is None else "complete"
    C = Checks()
    L, B, X = fx["L"], fx["B"], fx["X"]
    hp = host_plan(L, env)
    Xhost = host_solve(L, B, env)
    C.add("host", rel(Xhost, X), kind)
    C.add("reference", rel(fx["ref"].plain(B), X), "spread-" + kind)
    h = handle(fx["n"], device)
    perm = permutation(h, fx, how)
    img = image_shape(h, L, perm, env)
    if not device:
        C.shape(hp, {k: v for k, v in want.items() if k not in HOST_KEYS + IMAGE_KEYS})
        C.shape(img, {k: v for k, v in want.items() if k not in HOST_KEYS})
        for key in capi.SHAPE_KEYS:   # the image's plan is the plan the host probe builds
            if key not in HOST_KEYS + IMAGE_KEYS:
                C.expect("image plan %s against the host probe" % key, img[key], hp[key])
        return dict(shape=img, fixture=name, **C.out())
    before = state.get(fx["n"], 0)
    with switches(env):
        h.aux_set_cholesky(L.indptr, L.indices, L.data, perm)
    shape = h.factor_shape(capi.FACTOR_AUX)
    state[fx["n"]] = shape["generation"]
    C.shape(shape, want)
    C.expect("installs on the handle", shape["generation"], before + 1)
    expect_image(C, shape, img)
    for key in capi.SHAPE_KEYS:   # the device's plan is the plan the host probe builds
        if key not in HOST_KEYS + IMAGE_KEYS:
            C.expect("device plan %s against the host probe" % key, shape[key], hp[key])
    if not C.fail:   # (a plan of another form would be compared under the wrong name)
        vec = Vectors(h)
        solve_checks(C, h, vec, perm, B, X, kind, Xhost)
        vec.close()
    return dict(shape=shape, fixture=name, **C.out())


def reinstall_case(device, state):
    """A second, different factor on a handle that already holds one (the arena of the first is written over), then the
    first one again: each solves its own system and the probe follows."""
    import tri_forms as TF
    from cora_amd import capi
    C = Checks()
    if not device:
        return dict(shape={}, fixture="", **C.out())
    big, small = TF.fixture("random-2600"), TF.fixture("ndchain-2600")
    h = handle(2600)
    vec = Vectors(h)
    shape = {}
    for fx, env, form in ((big, {}, DENSE), (small, {}, SUB), (big, {}, DENSE), (small, SUB0, DENSE)):
        perm = permutation(h, fx, "scrambled")
        with switches(env):
            h.aux_set_cholesky(fx["L"].indptr, fx["L"].indices, fx["L"].data, perm)
        shape = h.factor_shape(capi.FACTOR_AUX)
        expect_image(C, shape, image_shape(h, fx["L"], perm, env))
        C.expect("form after installing %s" % fx["name"], shape["form"], form)
        C.expect("nnz(L) after installing %s" % fx["name"], shape["nnzL"], fx["L"].nnz)
        C.expect("installs", shape["generation"], state[2600] + 1)
        state[2600] = shape["generation"]
        Bapi, Xapi = np.empty_like(fx["B"]), np.empty_like(fx["X"])
        Bapi[perm], Xapi[perm] = fx["B"], fx["X"]
        for k in (1, 5, 24):
            b, x = vec.v[k]
            h.upload(Bapi[:, :k], b)
            h.upload(np.full((2600, k), np.nan), x)
            h.aux_solve_dev(b, k, x)
            C.add("x", rel(h.download(x, k), Xapi[:, :k]), "complete")
    vec.close()
    return dict(shape=shape, fixture="random-2600, ndchain-2600", **C.out())


def errors_case(device):
    """Refused calls answer with their status, fault nothing and leave the handle usable."""
    import tri_forms as TF
    from cora_amd import capi
    C = Checks()
    if not device:
        return dict(shape={}, fixture="", **C.out())
    fx = TF.fixture("random-1600")
    N = fx["n"]
    from synth import make_problem
    A, Q, dm = make_problem(d=2, n=N // 4, n_landmarks=3, n_ranges=N - 3 * (N // 4) - 3, n_loops=0, seed=3)
    h = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val)   # a fresh handle: nothing installed
    L = fx["L"]
    perm = np.arange(N, dtype=np.int32)
    b, x, b5 = h.dev_alloc(3), h.dev_alloc(3), h.dev_alloc(5)

    def status(call):
        try:
            call()
        except capi.CoraError as e:
            return capi.STATUS.get(e.code, str(e.code))
        return "CORA_OK"

    def not_ready(what):
        C.expect(what + ": solve", status(lambda: h.aux_solve_dev(b, 3, x)), "CORA_ERR_NOT_READY")
        C.expect(what + ": probe", status(lambda: h.factor_shape(capi.FACTOR_AUX)), "CORA_ERR_NOT_READY")

    not_ready("before any install")
    C.expect("m != N", status(lambda: h.aux_set_cholesky(L.indptr[:N], L.indices, L.data, perm[:N - 1])), "CORA_ERR_ARG")
    not_ready("after m != N")
    twice = perm.copy()
    twice[5] = twice[6]
    C.expect("perm with a row twice", status(lambda: h.aux_set_cholesky(L.indptr, L.indices, L.data, twice)), "CORA_ERR_ARG")
    outside = perm.copy()
    outside[0] = N
    C.expect("perm with a row outside", status(lambda: h.aux_set_cholesky(L.indptr, L.indices, L.data, outside)), "CORA_ERR_ARG")
    Li = L.indices.copy()   # column 0: the diagonal is no longer its first entry
    p0, p1 = L.indptr[0], L.indptr[1]
    assert p1 - p0 >= 2
    Li[p0], Li[p0 + 1] = Li[p0 + 1], Li[p0]
    C.expect("diagonal not first", status(lambda: h.aux_set_cholesky(L.indptr, Li, L.data, perm)), "CORA_ERR_ARG")
    not_ready("after refused installs")
    C.expect("install", status(lambda: h.aux_set_cholesky(L.indptr, L.indices, L.data, perm)), "CORA_OK")
    C.expect("output aliases the right-hand side", status(lambda: h.aux_solve_dev(b, 3, b)), "CORA_ERR_ARG")
    C.expect("k = 0", status(lambda: h.aux_solve_dev(b, 0, x)), "CORA_ERR_ARG")
    C.expect("k = 25", status(lambda: h.aux_solve_dev(b, 25, x)), "CORA_ERR_ARG")
    # a refused install on a handle that holds a factor: the old one is gone, nothing half-installed answers
    C.expect("diagonal not first, over a factor", status(lambda: h.aux_set_cholesky(L.indptr, Li, L.data, perm)), "CORA_ERR_ARG")
    not_ready("after a refused install over a factor")
    C.expect("install again", status(lambda: h.aux_set_cholesky(L.indptr, L.indices, L.data, perm)), "CORA_OK")
    shape = h.factor_shape(capi.FACTOR_AUX)
    h.upload(fx["B"][:, :3], b)
    h.aux_solve_dev(b, 3, x)
    C.add("x after the refused calls", rel(h.download(x, 3), fx["X"][:, :3]), "complete")
    for q in (b, x, b5):
        h.dev_free(q)
    h.close()
    return dict(shape=shape, fixture="random-1600", **C.out())


# ---------------------------------------------------------------- the preconditioner's entry
PROJ_N = 1700        # even, and N - 1 > 1536: the plan builder cuts
PROJ_RANKS = (2, 4, 12, 13)   # d, d + 2, the last stride of the fused sweeps, the first beyond
PROJ_GRAPH = dict(n_loops=8, seed=7)   # (loop closures: a better-conditioned Q, and fill across the separators)


class Regularised:
    """Q + lambda I of a synthetic graph (d = 2), its first N - 1 rows factorised in numpy in a nested-dissection order
    of the pose chain: rows of pose i (rotation rows, range rows measured from it, translation) at position i, halves
    first, one pose between them last, landmarks at the end (loop closures are left to the fill).  `split`: a pose's translation between its two rotation
    rows, so that no tile holds a pose's rotation rows at consecutive positions."""

    def __init__(self):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
        import stpcg_ref as ref
        import tri_forms as TF
        from synth import make_problem
        N = PROJ_N
        n = N // 4
        self.A, self.Q, self.dm = make_problem(d=2, n=n, n_landmarks=3, n_ranges=N - 3 * n - 3, **PROJ_GRAPH)
        dm = self.dm
        assert dm.N == N
        Qs = self.Q.to_scipy().tocsr()
        self.lam = float(spl.eigsh(Qs, k=1, which="LA", return_eigenvectors=False)[0]) / (1e6 - 1)  # src/CORA_problem.cpp:591
        self.chol = ref.RegularizedCholesky(self.Q, dm, self.lam)
        self.chol_plain = ref.RegularizedCholesky(self.Q, dm, self.lam, plain=True)
        M = (Qs + self.lam * sp.eye(N)).tocsr()[:N - 1, :N - 1]
        tb = dm.dn + dm.r
        pose_of_range = np.full(dm.r, -1)
        for k in range(dm.r):   # the pose a range row is measured from: its neighbour among the poses' translations
            cols = Qs.indices[Qs.indptr[dm.dn + k]:Qs.indptr[dm.dn + k + 1]]
            c = cols[(cols >= tb) & (cols < tb + n)]
            pose_of_range[k] = c[0] - tb
        self.perm, self.L = {}, {}
        for split in (False, True):
            rows_of = []
            for i in range(n):
                rng_rows = [dm.dn + k for k in np.nonzero(pose_of_range == i)[0]]
                rows_of.append([2 * i] + ([tb + i] if split else []) + [2 * i + 1] + rng_rows + ([] if split else [tb + i]))
            order = [r for i in TF.bisection_order(0, n, 4, 1) for r in rows_of[i]] + list(range(tb + n, N - 1))
            perm = np.array(order, dtype=np.int32)
            assert len(perm) == N - 1 and len(set(order)) == N - 1
            self.perm[split] = perm
            self.L[split] = TF.factor_csc(M[perm][:, perm])


def precond_cases(device):
    import tri_forms as TF
    from cora_amd import capi
    from oracle import oracle as orc
    import stpcg_ref as ref
    R = Regularised()
    dm, N = R.dm, PROJ_N
    forms = (("sub", False, {}, dict(form=SUB, stages=2, blocks=(3, None), zero_row=(0, None))),
             ("sub-split", True, {}, dict(form=SUB, stages=2, blocks=(3, None), fuse_ok=0)),
             ("dense", False, SUB0, dict(form=DENSE, stages=2, blocks=(10, None), fuse_ok=0)))
    h = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, R.Q.rowptr, R.Q.col, R.Q.val, device=0 if device else -1)
    rng = np.random.default_rng(5)
    points = {p: orc.project_manifold(dm, rng.uniform(-1, 1, (N, p))) for p in PROJ_RANKS}
    for name, split, env, want in forms:
        L, perm = R.L[split], R.perm[split]
        C = Checks()
        hp = host_plan(L, env)
        V = np.asfortranarray(np.random.default_rng(9).standard_normal((N, 24)))
        want_x = R.chol.full_solve(V)
        xh = np.zeros_like(V)
        xh[perm] = host_solve(L, V[perm], env)
        C.add("host", rel(xh, want_x), "reg")
        C.add("reference", rel(R.chol_plain.full_solve(V), want_x), "spread-reg")
        shape = img = image_shape(h, L, perm, env, grouped=True)
        if name == "sub":
            C.expect("the sweeps can take the projection", img["fuse_ok"], 1)
        if not device:
            C.shape(hp, {k: v for k, v in want.items() if k not in HOST_KEYS + IMAGE_KEYS + ("zero_row",)})
            C.shape(img, {k: v for k, v in want.items() if k not in HOST_KEYS})
        else:
            with switches(env):
                h.precond_set_cholesky(L.indptr, L.indices, L.data, perm)
            h.precond_setup(capi.PRECOND_REGULARIZED_CHOLESKY)
            shape = h.factor_shape(capi.FACTOR_PRECOND)
            C.shape(shape, want)
            expect_image(C, shape, img)
            C.expect("cora_precond_stats", h.precond_stats(),
                     dict(stages=shape["stages"], nnzW=shape["nnzW"], nnzL=L.nnz, top_rows=shape["top_rows"]))
            C.expect("substitution blocks of cora_precond_entries", h.precond_entries()["sub_blocks"],
                     shape["blocks"] if shape["form"] == SUB else 0)
            if name == "sub":
                C.expect("the sweeps take the projection", shape["fuse_ok"], 1)
            for p in (2, 3, 7, 24):   # cora_precondition: the pinned row exactly zero, the others the solve
                h.set_rank(p)
                x = h.precondition(V[:, :p])
                C.expect("p = %d: pinned row exactly zero" % p, bool(np.all(x[-1] == 0.0)), True)
                C.add("x", rel(x, want_x[:, :p]), "reg")
        emit("precond-" + name, shape=shape, fixture="Q + lambda I, N = %d" % N, **C.out())
        for p in PROJ_RANKS:   # Proj_Y of the solve: fused into the backward sweep where the plan and the stride allow
            C = Checks()
            Y = points[p]
            Vp = np.asfortranarray(V[:, :p])
            want_pv = R.chol.precond(Y, Vp)
            C.add("reference", rel(R.chol_plain.precond(Y, Vp), want_pv), "spread-reg")
            if device:
                h.set_rank(p)
                y, v, o = h.dev_alloc(p), h.dev_alloc(p), h.dev_alloc(p)
                h.upload(Y, y)
                h.set_point_dev(y)
                h.upload(Vp, v)
                h.upload(np.full((N, p), np.nan), o)
                h.precondition_projected_dev(v, o)
                got = h.download(o, p)
                C.expect("finite", bool(np.all(np.isfinite(got))), True)
                for cls, e in ref.class_errors(dm, np.nan_to_num(got), want_pv).items():
                    C.add("PV." + cls, e, "reg")
                C.expect("right-hand side unchanged", bool(np.array_equal(h.download(v, p), Vp)), True)
                h.precondition_projected_dev(v, o)
                C.expect("second apply bit-identical", bool(np.array_equal(h.download(o, p), got)), True)
                for q in (y, v, o):
                    h.dev_free(q)
            emit("proj-%s-p%d" % (name, p), shape=shape, fixture="Q + lambda I, N = %d" % N, **C.out())
    # three STPCG iterations on the dense-block plan (installed last): neither sweep-fused nor one-inverse, so the vector
    # passes are the fused ones (path 1, stpcg.inc) at an even N x stride <= 12
    C = Checks()
    p = 4
    prng = np.random.default_rng(31)
    # near the minimiser (positive curvature along the first directions): the lifted ground truth, rotated in R^p and
    # perturbed in every entry
    rot, _ = np.linalg.qr(prng.standard_normal((p, p)))
    lifted = np.hstack([R.A["truth"], np.zeros((N, p - dm.d))])
    Y = orc.project_manifold(dm, (lifted + 0.02 * prng.standard_normal((N, p))) @ rot)
    G = orc.egrad(R.Q, Y)
    g = orc.tangent_proj(dm, Y, G)
    hess = lambda W: orc.hvp(R.Q, dm, Y, G, W)  # noqa: E731
    states, how = ref.stpcg(hess, lambda W: R.chol.precond(Y, W), g, 1e30, 1e-300, 0.0, 3)
    plain, _ = ref.stpcg(hess, lambda W: R.chol_plain.precond(Y, W), g, 1e30, 1e-300, 0.0, 3, dot=orc.inner)
    C.expect("reference exit", (how, len(states)), ("limit", 3))
    for st in states:  # the limit must be what ends the reference: curvature well on the positive side
        if not st["kappa_rel"] >= 1e-3:
            C.fail.append("reference curvature %.3e too close to zero" % st["kappa_rel"])
    kept = list(range(len(states))) if how == "limit" else []
    for k in kept:
        if k < len(plain):
            for nm in ("s", "r", "p"):
                for cls, e in ref.class_errors(dm, plain[k][nm], states[k][nm]).items():
                    C.add("%s.%s" % (nm, cls), e, "spread-vec")
    path = None
    if device:
        h.set_rank(p)
        vs = [h.dev_alloc(p) for _ in range(6)]
        h.upload(Y, vs[5])
        h.set_point_dev(vs[5])
        grad = h.point_ptrs()[2]
        prev = None
        for k in kept:
            s, r, v, pk, hpv = vs[:5]
            it, sM = h.stpcg_dev(grad, 1e30, s, r, v, pk, hpv, kappa_fgr=1e-300, theta=0.0, max_iters=k + 1)
            path = h.stpcg_path()
            C.expect("path after %d" % (k + 1), path, 1)
            C.expect("iterations after %d" % (k + 1), it, k + 1)
            st = states[k]
            for nm, q in (("s", s), ("r", r), ("p", pk)):
                for cls, e in ref.class_errors(dm, h.download(q, p), st[nm]).items():
                    C.add("%s.%s" % (nm, cls), e, "vec")
            C.add("sM", abs(sM - st["sM"]) / abs(st["sM"]), "vec")
            prev = st["p_prev"] if prev is None else prev
            for cls, e in ref.class_errors(dm, h.download(hpv, p), orc.hvp(R.Q, dm, Y, G, prev)).items():
                C.add("Hp." + cls, e, "prod")
            prev = h.download(pk, p)
        for q in vs:
            h.dev_free(q)
    emit("stpcg-dense", shape={}, fixture="Q + lambda I, N = %d" % N, path=path, iterations=len(kept), **C.out())


def main():
    which = sys.argv[1]
    device = not (len(sys.argv) > 2 and sys.argv[2] == "host")
    os.environ.update(ENV[which])   # before the library loads: read once
    from cora_amd import capi
    capi.load()
    if which == "P":
        precond_cases(device)
    else:
        state = {}
        for spec in AUX_CASES[which]:
            emit(spec[0], **aux_case(spec, device, state))
        if which == "A":
            emit("reinstall", **reinstall_case(device, state))
        if which == "B":
            emit("errors", **errors_case(device))
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
