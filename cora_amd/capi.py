"""ctypes binding of libcora_hip.so (include/cora_hip.h).

Plumbing for tests/ and bench.py only: the product is the shared library and
the C++ host behind it.  There is no fallback -- if the library is missing or
no gfx950 device is usable, calls raise CoraError."""
import ctypes as C
import os

import numpy as np

from . import build as _build

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_LIB = None

STATUS = {0: "CORA_OK", 1: "CORA_ERR_SHAPE", 2: "CORA_ERR_NOT_READY", 3: "CORA_ERR_NAN",
          4: "CORA_ERR_HIP", 5: "CORA_ERR_ARG", 6: "CORA_ERR_NOMEM"}
PRECOND_NONE, PRECOND_JACOBI, PRECOND_BLOCK_CHOLESKY, PRECOND_REGULARIZED_CHOLESKY = 0, 1, 2, 3
PL_ORDER_GREEDY, PL_ORDER_LEVELS = 0, 1   # cora_set_chain_placement_order


# callback types of cora_set_comm (user pointer, device / host pointer as an integer, count)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)


# fields of cora_debug_factor_shape / cora_debug_factor_plan_host (include/cora_hip.h), in order
SHAPE_KEYS = ("stages", "form", "blocks", "block_rows", "max_rows", "max_lev", "max_level_lanes", "max_npl", "io_runs",
              "fuse_ok", "aux_rows", "aux_sum", "top_rows", "zero_row", "n8", "n64", "long_rows", "chunks", "max_chunks",
              "lds24", "nnzL", "nnzW", "mixed_products", "generation")
# fields of cora_debug_format_shape (include/cora_hip.h), in order
FORMAT_SHAPE_KEYS = ("chain_slices", "plain_slices", "max_general", "max_T", "max_lane_tail", "slices_T_gt_64",
                     "remote_tail_pairs", "long_pose_rows", "long_landmark_rows", "max_chunks", "straddling_tails")
FORM_PLAIN, FORM_DENSE, FORM_SUB = 0, 1, 2
FACTOR_PRECOND, FACTOR_IMPLICIT, FACTOR_AUX = 0, 1, 2


def _csc_factor(Lp, Li, Lx):
    return (np.ascontiguousarray(Lp, dtype=np.int32), np.ascontiguousarray(Li, dtype=np.int32),
            np.ascontiguousarray(Lx, dtype=np.float64))


def factor_plan_host(Lp, Li, Lx, aux_ok=True):
    """Shape of the solve plan of a factor (CSC, diagonal first) that is installed nowhere: dict over SHAPE_KEYS
    (cora_debug_factor_plan_host; no GPU needed)."""
    L = load()
    Lp, Li, Lx = _csc_factor(Lp, Li, Lx)
    out = (C.c_int64 * len(SHAPE_KEYS))()
    rc = L.cora_debug_factor_plan_host(len(Lp) - 1, Lp.ctypes.data_as(_ip), Li.ctypes.data_as(_ip), _d(Lx),
                                       int(bool(aux_ok)), out)
    if rc:
        raise CoraError(rc, L.cora_last_error(None).decode())
    return dict(zip(SHAPE_KEYS, [int(v) for v in out]))


def factor_plan_digest(Lp, Li, Lx, group=None, aux_ok=True):
    """Digest of the whole solve plan of a factor that is installed nowhere: (integers and indices, bits of the doubles),
    two 64-bit FNV-1a values (cora_debug_factor_plan_digest; no GPU needed).  group: None or one id per variable."""
    L = load()
    Lp, Li, Lx = _csc_factor(Lp, Li, Lx)
    m = len(Lp) - 1
    g = None
    if group is not None:
        g = np.ascontiguousarray(group, dtype=np.int32)
        assert g.shape == (m,)
    out = (C.c_uint64 * 2)()
    rc = L.cora_debug_factor_plan_digest(m, Lp.ctypes.data_as(_ip), Li.ctypes.data_as(_ip), _d(Lx),
                                         g.ctypes.data_as(_ip) if g is not None else None, int(bool(aux_ok)), out)
    if rc:
        raise CoraError(rc, L.cora_last_error(None).decode())
    return int(out[0]), int(out[1])


def factor_image(Lp, Li, Lx, row_map=None, group=None, aux_ok=True, d=0, rot0=0, rot1=0, rows=0, zero_row=-1):
    """What an install of a factor would upload, for a factor that is installed nowhere (cora_debug_factor_image; no GPU
    needed): (digest, shape) -- the digest of plan + device image in upload order (integers, doubles) and the dict over
    SHAPE_KEYS with io_runs and fuse_ok as an install decides them.  row_map: None (identity) or the internal row of every
    variable; rows: rows of a vector (0: the factor's order); d, rot0, rot1: the rotation rows [rot0, rot1), d per pose."""
    L = load()
    Lp, Li, Lx = _csc_factor(Lp, Li, Lx)
    m = len(Lp) - 1
    opt = []
    for v in (row_map, group):
        a = None if v is None else np.ascontiguousarray(v, dtype=np.int32)
        assert a is None or a.shape == (m,)
        opt.append(a)
    dig, shape = (C.c_uint64 * 2)(), (C.c_int64 * len(SHAPE_KEYS))()
    rc = L.cora_debug_factor_image(m, Lp.ctypes.data_as(_ip), Li.ctypes.data_as(_ip), _d(Lx),
                                   *[a.ctypes.data_as(_ip) if a is not None else None for a in opt], int(bool(aux_ok)),
                                   C.c_int64(int(rows)), C.c_int32(int(zero_row)), int(d), C.c_int64(int(rot0)),
                                   C.c_int64(int(rot1)), dig, shape)
    if rc:
        raise CoraError(rc, L.cora_last_error(None).decode())
    return (int(dig[0]), int(dig[1])), dict(zip(SHAPE_KEYS, [int(v) for v in shape]))


class CoraError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (STATUS.get(code, str(code)), msg))
        self.code = code


def lib_path():
    return _build.LIB


def load():
    """Loads the in-tree shared library (building it first when stale)."""
    global _LIB
    if _LIB is None:
        # torch bundles its own libamdhip64.so.7: load it FIRST so that the process has one
        # HIP runtime (our library then binds to the already-loaded SONAME); the other order
        # leaves two runtimes and hipSetDevice fails with "no ROCm-capable device".
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        path = _build.LIB
        # lab builds of one kernel group (cora_amd/build.py, CORA_VARIANT): never set outside measurement scripts
        variant = os.environ.get("CORA_LIB_VARIANT")
        if variant:
            path = os.path.join(_build.LIBDIR, "variants", variant, "libcora_hip.so")
            if not os.path.exists(path):
                raise RuntimeError("CORA_LIB_VARIANT=%s: %s does not exist" % (variant, path))
        elif _build.needs_build():
            try:
                _build.build()
            except Exception as e:  # hipcc missing on a box that ships the prebuilt .so
                if not os.path.exists(path):
                    raise RuntimeError("libcora_hip.so is missing and cannot be built: %s" % e)
        _LIB = C.CDLL(path)
        L = _LIB
        L.cora_last_error.restype = C.c_char_p
        L.cora_last_error.argtypes = [C.c_void_p]
        for name in ("cora_rows", "cora_shard_rows", "cora_shard_begin", "cora_nnz", "cora_dim"):
            getattr(L, name).restype = C.c_int64
            getattr(L, name).argtypes = [C.c_void_p]
        for name in ("cora_point_Y_dev", "cora_point_egrad_dev", "cora_point_rgrad_dev"):
            getattr(L, name).restype = C.c_void_p
            getattr(L, name).argtypes = [C.c_void_p]
        L.cora_ctx_destroy.restype = None
        L.cora_ctx_destroy.argtypes = [C.c_void_p]
        L.cora_debug_live_allocations.restype = C.c_int64
        L.cora_debug_live_allocations.argtypes = []
    return _LIB


def live_allocations():
    """Device and pinned blocks the handles of this process hold now (cora_debug_live_allocations): 0 once all are destroyed."""
    return int(load().cora_debug_live_allocations())


def _d(a):
    return a.ctypes.data_as(_dp)


def _f(a):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    return np.asfortranarray(a)


class Context:
    """One device-resident problem (cora_ctx).  Host arrays are column-major
    N x k float64, as in the reference (Eigen::MatrixXd)."""

    def __init__(self, d, n_poses, n_ranges, n_trans, rowptr, colidx, vals, device=0, rank=0, world=1,
                 whole_long_rows=False):
        self.L = load()
        self.d, self.n, self.r, self.nt = int(d), int(n_poses), int(n_ranges), int(n_trans)
        self.N = self.d * self.n + self.r + self.nt
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        colidx = np.ascontiguousarray(colidx, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if len(rowptr) != self.N + 1:
            raise CoraError(1, "rowptr must have N+1 entries")
        h = C.c_void_p()
        rc = self.L.cora_ctx_create_part_opts(C.c_int(device), self.d, self.n, self.r, self.nt,
                                              rowptr.ctypes.data_as(_ip), colidx.ctypes.data_as(_ip), _d(vals),
                                              C.c_int(rank), C.c_int(world), C.c_uint(1 if whole_long_rows else 0),
                                              C.byref(h))
        if rc:
            raise CoraError(rc, self.L.cora_last_error(None).decode())
        self.h = h
        self.p = 0

    @classmethod
    def from_handle(cls, ptr, d, n_poses, n_ranges, n_trans):
        """Borrow a cora_ctx owned by someone else (e.g. CORA::Problem::context()); never destroyed here."""
        self = cls.__new__(cls)
        self.L = load()
        self.d, self.n, self.r, self.nt = int(d), int(n_poses), int(n_ranges), int(n_trans)
        self.N = self.d * self.n + self.r + self.nt
        self.h = C.c_void_p(ptr)
        self.p = self.L.cora_get_rank(self.h)
        self._borrowed = True
        return self

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.L.cora_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise CoraError(rc, self.L.cora_last_error(self.h).decode())

    # ---- queries
    def set_rank(self, p):
        self._chk(self.L.cora_set_rank(self.h, int(p)))
        self.p = int(p)

    @property
    def ld(self):
        return self.L.cora_ld(self.h)

    @property
    def rows(self):
        return self.L.cora_rows(self.h)

    @property
    def shard_rows(self):
        return self.L.cora_shard_rows(self.h)

    @property
    def shard_begin(self):
        return self.L.cora_shard_begin(self.h)

    @property
    def nnz(self):
        return self.L.cora_nnz(self.h)

    def row_map(self):
        m = np.empty(self.N, dtype=np.int32)
        self._chk(self.L.cora_row_map(self.h, m.ctypes.data_as(_ip)))
        return m

    def remote_rows(self):
        """Internal rows outside this rank's shard that its part of Q reads (ascending, int64)."""
        n = C.c_int64()
        self._chk(self.L.cora_remote_rows(self.h, None, C.byref(n)))
        r = np.empty(max(n.value, 1), dtype=np.int32)
        self._chk(self.L.cora_remote_rows(self.h, r.ctypes.data_as(_ip), C.byref(n)))
        return r[:n.value].astype(np.int64)

    def long_rows(self):
        """API rows of the distributed long rows of a partitioned handle (empty on one GPU)."""
        n = C.c_int64(0)
        self._chk(self.L.cora_long_rows(self.h, None, C.byref(n)))
        r = np.zeros(max(n.value, 1), dtype=np.int32)
        self._chk(self.L.cora_long_rows(self.h, r.ctypes.data_as(_ip), C.byref(n)))
        return r[:n.value].astype(np.int64)

    def format_stats(self):
        s = (C.c_int64 * 8)()
        self._chk(self.L.cora_format_stats(self.h, s))
        keys = ["slices", "padded_nnz", "long_nnz", "long_rows", "long_chunks", "local_rows", "local_nnz",
                "max_width"]
        return dict(zip(keys, [int(x) for x in s]))

    def format_bytes(self):
        b = (C.c_int64 * 4)()
        self._chk(self.L.cora_format_bytes(self.h, b))
        return dict(zip(["values", "indices", "descriptors", "total"], [int(x) for x in b]))

    def format_shape(self):
        """Shape of the handle's format of Q (cora_debug_format_shape; no GPU needed): dict over FORMAT_SHAPE_KEYS."""
        out = (C.c_int64 * len(FORMAT_SHAPE_KEYS))()
        self._chk(self.L.cora_debug_format_shape(self.h, out))
        return dict(zip(FORMAT_SHAPE_KEYS, [int(v) for v in out]))

    def format_digest(self):
        """Digest of the handle's whole format of Q: (integers and indices, bits of the doubles), two 64-bit FNV-1a
        values (cora_debug_format_digest; no GPU needed)."""
        out = (C.c_uint64 * 2)()
        self._chk(self.L.cora_debug_format_digest(self.h, out))
        return int(out[0]), int(out[1])

    def value_map_digest(self):
        """Digest of the handle's source map (values_map_build): (sources, mirror pairs); CoraError while there is none."""
        out = (C.c_uint64 * 2)()
        self._chk(self.L.cora_debug_value_map_digest(self.h, out))
        return int(out[0]), int(out[1])

    def debug_long_image(self, piece=0):
        """The device image of the long rows (cora_debug_long_image; no GPU needed): dict with `placed`, `chunks`
        (dict of int32 arrays: row, k0, k1, nchunks, first, slot), `chunk_order`, `lval`, `lcol` (internal rows), `perm`, `home`
        and `home_pose_first` (int8 per internal row, -1 = no slice owns it).  piece <= 0: the library's piece size."""
        s = (C.c_int64 * 5)()
        self._chk(self.L.cora_debug_long_image(self.h, int(piece), s, None, None, None, None, None, None, None))
        chunks = np.zeros((int(s[0]), 8), dtype=np.int32)
        order = np.zeros(int(s[1]), dtype=np.int32)
        lval = np.zeros(int(s[2]), dtype=np.float64)
        lcol = np.zeros(int(s[2]), dtype=np.int32)
        perm = np.zeros(int(s[2]), dtype=np.int32)
        home = np.zeros(int(s[3]), dtype=np.int8)
        home_pf = np.zeros(int(s[3]), dtype=np.int8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._chk(self.L.cora_debug_long_image(self.h, int(piece), s, vp(chunks), vp(order), vp(lval), vp(lcol), vp(perm),
                                               vp(home), vp(home_pf)))
        names = ["row", "k0", "k1", "nchunks", "first", "slot"]
        return {"placed": bool(s[4]), "chunks": {k: chunks[:, i].copy() for i, k in enumerate(names)}, "chunk_order": order,
                "lval": lval, "lcol": lcol, "perm": perm, "home": home, "home_pose_first": home_pf}

    def precond_entries(self):
        """Entries the installed preconditioner's solve plan stores (cora_precond_entries)."""
        s = (C.c_int64 * 6)()
        self._chk(self.L.cora_precond_entries(self.h, s))
        keys = ["top_forward", "top_backward", "sub_forward_slots", "sub_backward_slots", "sub_blocks", "aux_rows"]
        return dict(zip(keys, [int(x) for x in s]))

    def precond_stats(self):
        """Solve plan of the installed preconditioner (cora_precond_stats)."""
        s = (C.c_int64 * 4)()
        self._chk(self.L.cora_precond_stats(self.h, s))
        return dict(zip(["stages", "nnzW", "nnzL", "top_rows"], [int(x) for x in s]))

    def factor_shape(self, which):
        """Shape of the solve plan of an installed factor (FACTOR_PRECOND | FACTOR_IMPLICIT | FACTOR_AUX): dict over
        SHAPE_KEYS (cora_debug_factor_shape); CORA_ERR_NOT_READY where none is installed."""
        out = (C.c_int64 * len(SHAPE_KEYS))()
        self._chk(self.L.cora_debug_factor_shape(self.h, int(which), out))
        return dict(zip(SHAPE_KEYS, [int(v) for v in out]))

    def _set_cholesky(self, call, Lp, Li, Lx, perm, m=None):
        Lp, Li, Lx = _csc_factor(Lp, Li, Lx)
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        self._chk(call(self.h, int(len(Lp) - 1 if m is None else m), Lp.ctypes.data_as(_ip), Li.ctypes.data_as(_ip), _d(Lx),
                       perm.ctypes.data_as(_ip)))

    def precond_set_cholesky(self, Lp, Li, Lx, perm, m=None):
        """Installs L (CSC, diagonal first) of P (Q + lambda I)[0:m] P^T, m = N or N - 1, perm new -> old in API rows."""
        self._set_cholesky(self.L.cora_precond_set_cholesky, Lp, Li, Lx, perm, m)

    def aux_set_cholesky(self, Lp, Li, Lx, perm, m=None):
        """Installs a factor of the caller's own matrix, N rows (cora_aux_set_cholesky)."""
        self._set_cholesky(self.L.cora_aux_set_cholesky, Lp, Li, Lx, perm, m)

    def aux_solve_dev(self, b, k, x):
        """x = (P^T L L^T P)^-1 b on k-column resident vectors, b != x (cora_aux_solve_dev)."""
        self._chk(self.L.cora_aux_solve_dev(self.h, C.c_void_p(b), int(k), C.c_void_p(x)))

    def set_stream(self, stream_ptr):
        self._chk(self.L.cora_set_stream(self.h, C.c_void_p(stream_ptr)))

    # ---- multi-GPU building blocks (include/cora_hip.h, cora_set_comm)
    @property
    def rank(self):
        return self.L.cora_rank(self.h)

    @property
    def world(self):
        return self.L.cora_world(self.h)

    def set_comm(self, exchange, allreduce, allgather):
        """ctypes callbacks (EXCHANGE_FN / ALLREDUCE_FN / ALLGATHER_FN); the caller keeps them alive."""
        self._chk(self.L.cora_set_comm(self.h, exchange, allreduce, allgather, None))

    def pack_rows_dev(self, x, ld, rows_ptr, n, packed):
        self._chk(self.L.cora_pack_rows_dev(self.h, C.c_void_p(x), int(ld), C.c_void_p(rows_ptr), C.c_int64(n),
                                            C.c_void_p(packed)))

    def scatter_rows_dev(self, packed, ld, rows_ptr, n, x):
        self._chk(self.L.cora_scatter_rows_dev(self.h, C.c_void_p(packed), int(ld), C.c_void_p(rows_ptr), C.c_int64(n),
                                               C.c_void_p(x)))

    def copy_rows_dev(self, src, ld, rows_ptr, n, dst):
        self._chk(self.L.cora_copy_rows_dev(self.h, C.c_void_p(src), int(ld), C.c_void_p(rows_ptr), C.c_int64(n),
                                            C.c_void_p(dst)))

    def copy_shard_dev(self, src, ld, shard, dst):
        self._chk(self.L.cora_copy_shard_dev(self.h, C.c_void_p(src), int(ld), int(shard), C.c_void_p(dst)))

    # ---- host-pointer operator API (mirrors CORA::Problem)
    def _out(self, k):
        return np.zeros((self.N, k), order="F")

    def dataMatrixProduct(self, X):
        X = _f(X)
        out = self._out(X.shape[1])
        self._chk(self.L.cora_data_matrix_product(self.h, _d(X), X.shape[0], X.shape[1], _d(out), self.N))
        return out

    def evaluateObjective(self, Y):
        Y = _f(Y)
        f = C.c_double()
        self._chk(self.L.cora_evaluate_objective(self.h, _d(Y), Y.shape[0], C.byref(f)))
        return f.value

    def Euclidean_gradient(self, Y):
        Y = _f(Y)
        out = self._out(self.p)
        self._chk(self.L.cora_euclidean_gradient(self.h, _d(Y), Y.shape[0], _d(out), self.N))
        return out

    def Riemannian_gradient(self, Y):
        Y = _f(Y)
        out = self._out(self.p)
        self._chk(self.L.cora_riemannian_gradient(self.h, _d(Y), Y.shape[0], _d(out), self.N))
        return out

    def tangent_space_projection(self, Y, V):
        Y, V = _f(Y), _f(V)
        out = self._out(self.p)
        self._chk(self.L.cora_tangent_space_projection(self.h, _d(Y), Y.shape[0], _d(V), V.shape[0], _d(out),
                                                       self.N))
        return out

    def Riemannian_Hessian_vector_product(self, Y, G, Ydot):
        Y, G, Ydot = _f(Y), _f(G), _f(Ydot)
        out = self._out(self.p)
        self._chk(self.L.cora_riemannian_hessian_vector_product(
            self.h, _d(Y), Y.shape[0], _d(G), G.shape[0], _d(Ydot), Ydot.shape[0], _d(out), self.N))
        return out

    def projectToManifold(self, A):
        A = _f(A)
        out = self._out(self.p)
        self._chk(self.L.cora_project_to_manifold(self.h, _d(A), A.shape[0], _d(out), self.N))
        return out

    def retract(self, Y, V):
        Y, V = _f(Y), _f(V)
        out = self._out(self.p)
        self._chk(self.L.cora_retract(self.h, _d(Y), Y.shape[0], _d(V), V.shape[0], _d(out), self.N))
        return out

    def precond_setup(self, kind):
        self._chk(self.L.cora_precond_setup(self.h, int(kind)))

    def precondition(self, V):
        V = _f(V)
        out = self._out(self.p)
        self._chk(self.L.cora_precondition(self.h, _d(V), V.shape[0], _d(out), self.N))
        return out

    def compute_Lambda_blocks(self, Y):
        Y = _f(Y)
        st = np.zeros((self.d, max(self.d * self.n, 1)), order="F")
        ob = np.zeros(max(self.r, 1))
        self._chk(self.L.cora_compute_lambda_blocks(self.h, _d(Y), Y.shape[0], _d(st), _d(ob)))
        return st[:, :self.d * self.n], ob[:self.r]

    def set_point(self, Y):
        Y = _f(Y)
        self._chk(self.L.cora_set_point(self.h, _d(Y), Y.shape[0]))

    def point_cost(self):
        f = C.c_double()
        self._chk(self.L.cora_point_cost(self.h, C.byref(f)))
        return f.value

    def certificate_product(self, X):
        X = _f(X)
        out = self._out(X.shape[1])
        self._chk(self.L.cora_certificate_product(self.h, _d(X), X.shape[0], X.shape[1], _d(out), self.N))
        return out

    def inner_product(self, A, B):
        A, B = _f(A), _f(B)
        v = C.c_double()
        self._chk(self.L.cora_inner_product(self.h, _d(A), A.shape[0], _d(B), B.shape[0], A.shape[1],
                                            C.byref(v)))
        return v.value

    # ---- resident API (raw device pointers as ints)
    def dev_alloc(self, k):
        p = _dp()
        self._chk(self.L.cora_dev_alloc(self.h, int(k), C.byref(p)))
        return C.cast(p, C.c_void_p).value

    def dev_free(self, ptr):
        self._chk(self.L.cora_dev_free(self.h, C.c_void_p(ptr)))

    def upload(self, host, ptr):
        host = _f(host)
        self._chk(self.L.cora_upload(self.h, _d(host), host.shape[0], host.shape[1], C.c_void_p(ptr)))

    def download(self, ptr, k, out=None):
        """N x k host copy of a resident vector; `out` (column-major, at least N rows: its row count is the leading
        dimension) is filled in place when given."""
        if out is None:
            out = self._out(k)
        self._chk(self.L.cora_download(self.h, C.c_void_p(ptr), int(k), _d(out), out.shape[0]))
        return out

    def set_point_dev(self, ptr):
        self._chk(self.L.cora_set_point_dev(self.h, C.c_void_p(ptr)))

    def spmm_dev(self, x, k, out):
        self._chk(self.L.cora_spmm_dev(self.h, C.c_void_p(x), int(k), C.c_void_p(out)))

    def hvp_dev(self, x, out):
        self._chk(self.L.cora_hvp_dev(self.h, C.c_void_p(x), C.c_void_p(out)))

    def certificate_product_dev(self, x, k, out):
        self._chk(self.L.cora_certificate_product_dev(self.h, C.c_void_p(x), int(k), C.c_void_p(out)))

    def tangent_space_projection_dev(self, v, out):
        self._chk(self.L.cora_tangent_space_projection_dev(self.h, C.c_void_p(v), C.c_void_p(out)))

    def precondition_projected_dev(self, v, out):
        self._chk(self.L.cora_precondition_projected_dev(self.h, C.c_void_p(v), C.c_void_p(out)))

    def retract_dev(self, v, alpha, out):
        self._chk(self.L.cora_retract_dev(self.h, C.c_void_p(v), C.c_double(alpha), C.c_void_p(out)))

    def objective_dev(self, y):
        """f(y) for a resident y without changing the current point."""
        f = C.c_double()
        self._chk(self.L.cora_objective_dev(self.h, C.c_void_p(y), C.byref(f)))
        return f.value

    def tnt_trial_dev(self, s, hs, xprop):
        """hs = Hess(s), xprop = Retr_Y(s); returns [<grad, s>, <s, Hess s>, <s, s>, f(xprop)] in one wait."""
        out = (C.c_double * 4)()
        self._chk(self.L.cora_tnt_trial_dev(self.h, C.c_void_p(s), C.c_void_p(hs), C.c_void_p(xprop), out))
        return [out[i] for i in range(4)]

    def tnt_accept_dev(self, x, pg):
        """x becomes the current point, pg = projected preconditioned gradient; returns [f, <g,g>, <Pg,Pg>, <g,Pg>]."""
        out = (C.c_double * 4)()
        self._chk(self.L.cora_tnt_accept_dev(self.h, C.c_void_p(x), C.c_void_p(pg), out))
        return [out[i] for i in range(4)]

    def project_to_manifold_dev(self, a, out):
        self._chk(self.L.cora_project_to_manifold_dev(self.h, C.c_void_p(a), C.c_void_p(out)))

    def axpby_dev(self, a, x, b, y):
        self._chk(self.L.cora_axpby_dev(self.h, C.c_double(a), C.c_void_p(x), C.c_double(b), C.c_void_p(y)))

    def axpy2_dev(self, a1, x1, y1, a2, x2, y2):
        self._chk(self.L.cora_axpy2_dev(self.h, C.c_double(a1), C.c_void_p(x1), C.c_void_p(y1), C.c_double(a2),
                                        C.c_void_p(x2), C.c_void_p(y2)))

    def axpby_cols_dev(self, k, a, x, b, y):
        """y = a x + b y on vectors allocated with k columns (cora_axpby_cols_dev)."""
        self._chk(self.L.cora_axpby_cols_dev(self.h, int(k), C.c_double(a), C.c_void_p(x), C.c_double(b), C.c_void_p(y)))

    def fill_random_dev(self, k, seed, x):
        """x (k columns) = numbers in (-1, 1) that depend on (seed, API row, column) only (cora_fill_random_dev)."""
        self._chk(self.L.cora_fill_random_dev(self.h, int(k), C.c_ulonglong(seed), C.c_void_p(x)))

    def copy_dev(self, x, k, y):
        """y = x on vectors allocated with k columns (cora_copy_dev)."""
        self._chk(self.L.cora_copy_dev(self.h, C.c_void_p(x), int(k), C.c_void_p(y)))

    def stpcg_dev(self, grad, Delta, s, r, v, p, hp, kappa_fgr=0.1, theta=0.8, max_iters=80):
        """Device-resident Steihaug-Toint PCG at the current point; returns (Hessian-vector products, ||s||_M)."""
        it = C.c_int()
        sm = C.c_double()
        self._chk(self.L.cora_stpcg_dev(self.h, C.c_void_p(grad), C.c_double(Delta), C.c_double(kappa_fgr),
                                        C.c_double(theta), int(max_iters), C.c_void_p(s), C.c_void_p(r), C.c_void_p(v),
                                        C.c_void_p(p), C.c_void_p(hp), C.byref(it), C.byref(sm)))
        return it.value, sm.value

    def stpcg_warm_dev(self, grad, pg, g_g, g_pg, Delta, s, r, v, p, hp, kappa_fgr=0.1, theta=0.8, max_iters=80):
        """stpcg_dev started from a known preconditioned gradient pg = P grad, <grad, grad> and <grad, pg>."""
        it = C.c_int()
        sm = C.c_double()
        self._chk(self.L.cora_stpcg_warm_dev(self.h, C.c_void_p(grad), C.c_void_p(pg), C.c_double(g_g), C.c_double(g_pg),
                                             C.c_double(Delta), C.c_double(kappa_fgr), C.c_double(theta), int(max_iters),
                                             C.c_void_p(s), C.c_void_p(r), C.c_void_p(v), C.c_void_p(p), C.c_void_p(hp),
                                             C.byref(it), C.byref(sm)))
        return it.value, sm.value

    def profile_stpcg(self, on=True):
        self._chk(self.L.cora_debug_profile_stpcg(self.h, int(on)))

    def stpcg_path(self):
        """Iteration form of the last stpcg_dev call: 0 unfused, 1 fused vector passes, 2 sweep-fused (the passes ride on
        the two sweeps of a two-stage Cholesky plan), 3 inverse-fused (on the two products of a one-inverse plan)."""
        return int(self.L.cora_debug_stpcg_path(self.h))

    def stpcg_graph_stats(self):
        """(graphs captured, batches replayed) of the device-resident STPCG (cora_debug_stpcg_graph)."""
        out = (C.c_long * 2)()
        self._chk(self.L.cora_debug_stpcg_graph(self.h, out))
        return int(out[0]), int(out[1])

    def stpcg_hvp_us(self):
        """(mean microseconds, count) of the Hessian-vector products of the last stpcg_dev call (profile_stpcg on)."""
        us, cnt = C.c_double(), C.c_int()
        self._chk(self.L.cora_debug_stpcg_hvp_us(self.h, C.byref(us), C.byref(cnt)))
        return us.value, cnt.value

    def stpcg_phase_us(self):
        """Mean microseconds per launch of the sweep-fused iteration of the last stpcg_dev call (profile_stpcg(2)):
        dict product | kappa | forward_sweep | top_forward | top_backward | backward_sweep; None where not recorded."""
        us = (C.c_double * 8)()
        self._chk(self.L.cora_debug_stpcg_phase_us(self.h, us))
        names = ("product", "kappa", "forward_sweep", "top_forward", "top_backward", "backward_sweep", "event_overhead")
        out = {k: (float(v) if v >= 0 else None) for k, v in zip(names, us)}
        out["kappa_folded"] = bool(us[7])
        if out["kappa_folded"]:
            out["kappa"] = None
        return out

    def gram_dev(self, a, ka, b, kb):
        """G = A^T B (ka x kb) of two resident blocks."""
        G = np.zeros((ka, kb), order="F")
        self._chk(self.L.cora_gram_dev(self.h, C.c_void_p(a), int(ka), C.c_void_p(b), int(kb),
                                       G.ctypes.data_as(C.POINTER(C.c_double))))
        return G

    def gram_batch_dev(self, pairs):
        """[A^T B for (a, ka, b, kb) in pairs] with one synchronisation (cora_gram_batch_dev)."""
        n = len(pairs)
        Gs = [np.zeros((ka, kb), order="F") for _, ka, _, kb in pairs]
        pa = (C.c_void_p * n)(*[C.c_void_p(a) for a, _, _, _ in pairs])
        pb = (C.c_void_p * n)(*[C.c_void_p(b) for _, _, b, _ in pairs])
        ka = (C.c_int * n)(*[int(k) for _, k, _, _ in pairs])
        kb = (C.c_int * n)(*[int(k) for _, _, _, k in pairs])
        out = (C.c_void_p * n)(*[G.ctypes.data_as(C.c_void_p) for G in Gs])
        self._chk(self.L.cora_gram_batch_dev(self.h, n, pa, ka, pb, kb, out))
        return Gs

    def combine_dev(self, xs, ks, Cs, kout, out):
        """out = sum_i X_i C_i with host coefficient matrices C_i (k_i x kout)."""
        n = len(xs)
        ptrs = (C.c_void_p * n)(*[C.c_void_p(x) for x in xs])
        kk = (C.c_int * n)(*[int(k) for k in ks])
        mats = [np.asfortranarray(np.array(M, dtype=np.float64)) for M in Cs]
        cp = (C.c_void_p * n)(*[M.ctypes.data_as(C.c_void_p) for M in mats])
        self._chk(self.L.cora_combine_dev(self.h, n, ptrs, kk, cp, int(kout), C.c_void_p(out)))

    def dot_dev(self, a, b, k):
        v = C.c_double()
        self._chk(self.L.cora_dot_dev(self.h, C.c_void_p(a), C.c_void_p(b), int(k), C.byref(v)))
        return v.value

    def dots_dev(self, pairs):
        """Several inner products with one reduction and one synchronisation (the three metric() calls of
        an STPCG iteration, src/CORA.cpp:119-122)."""
        n = len(pairs)
        A = (C.c_void_p * n)(*[C.c_void_p(a) for a, _ in pairs])
        B = (C.c_void_p * n)(*[C.c_void_p(b) for _, b in pairs])
        out = (C.c_double * n)()
        self._chk(self.L.cora_dots_dev(self.h, n, A, B, out))
        return [out[i] for i in range(n)]

    def point_ptrs(self):
        return (self.L.cora_point_Y_dev(self.h), self.L.cora_point_egrad_dev(self.h),
                self.L.cora_point_rgrad_dev(self.h))

    def timer_start(self):
        self._chk(self.L.cora_timer_start(self.h))

    def timer_stop_ms(self):
        ms = C.c_float()
        self._chk(self.L.cora_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value

    def sync(self):
        self._chk(self.L.cora_sync(self.h))

    # ---- per-measurement residuals (include/cora_hip.h, cora_set_measurements)
    def set_measurements(self, edge_rows, edge_data, range_rows, range_data):
        """edge_rows [m][4] / range_rows [r][3] int32 API rows, edge_data [m][d*d + d + 2] = R row-major, t, kappa, tau,
        range_data [r][2] = r, omega.  Replaces the handle's table."""
        er = np.ascontiguousarray(np.asarray(edge_rows, dtype=np.int32).reshape(-1, 4))
        ed = np.ascontiguousarray(np.asarray(edge_data, dtype=np.float64).reshape(-1, self.d * self.d + self.d + 2))
        rr = np.ascontiguousarray(np.asarray(range_rows, dtype=np.int32).reshape(-1, 3))
        rd = np.ascontiguousarray(np.asarray(range_data, dtype=np.float64).reshape(-1, 2))
        if len(er) != len(ed) or len(rr) != len(rd):
            raise CoraError(1, "rows and data of a measurement table must have the same length")
        self._chk(self.L.cora_set_measurements(self.h, C.c_int64(len(er)), er.ctypes.data_as(_ip), _d(ed),
                                               C.c_int64(len(rr)), rr.ctypes.data_as(_ip), _d(rd)))

    def measurement_counts(self):
        """(edges, ranges) of the handle's measurement table."""
        out = (C.c_int64 * 2)()
        self._chk(self.L.cora_measurement_counts(self.h, out))
        return int(out[0]), int(out[1])

    def _residuals(self, call):
        ne, nr = self.measurement_counts()
        rot, trn, rng = np.zeros(max(ne, 1)), np.zeros(max(ne, 1)), np.zeros(max(nr, 1))
        sums = np.zeros(3)
        self._chk(call(_d(rot), _d(trn), _d(rng), _d(sums)))
        return dict(edge_rot=rot[:ne], edge_trans=trn[:ne], range=rng[:nr], sums=sums)

    def measurement_residuals(self, X):
        """Residuals of every measurement of the table at the host matrix X (N x k): dict edge_rot, edge_trans, range,
        sums = [sum rot, sum trans, sum range]; 1/2 sum(sums) = evaluateObjective(X)."""
        X = _f(X)
        return self._residuals(lambda *o: self.L.cora_measurement_residuals(self.h, _d(X), X.shape[0], X.shape[1], *o))

    def measurement_residuals_dev(self, x, k):
        """The same at a resident vector x of k columns."""
        return self._residuals(lambda *o: self.L.cora_measurement_residuals_dev(self.h, C.c_void_p(x), int(k), *o))

    def debug_measurement_residuals_host(self, X):
        """Test hook: the translated table executed on the host (no GPU needed)."""
        X = _f(X)
        return self._residuals(lambda *o: self.L.cora_debug_measurement_residuals_host(self.h, _d(X), X.shape[0],
                                                                                      X.shape[1], *o))

    # ---- new values of Q on the same pattern (include/cora_hip.h, cora_update_values)
    @staticmethod
    def _csr(rowptr, colidx):
        return (np.ascontiguousarray(rowptr, dtype=np.int32), np.ascontiguousarray(colidx, dtype=np.int32))

    def values_map_build(self, rowptr, colidx):
        rowptr, colidx = self._csr(rowptr, colidx)
        if len(rowptr) != self.N + 1:
            raise CoraError(5, "rowptr must have N+1 entries")
        self._chk(self.L.cora_values_map_build(self.h, rowptr.ctypes.data_as(_ip), colidx.ctypes.data_as(_ip)))

    def update_values(self, rowptr, colidx, vals):
        """Replaces the values of Q in place (host values, CSR order, the pattern of creation).  Afterwards the handle
        is in the state of a fresh one: set the point and the preconditioner again."""
        rowptr, colidx = self._csr(rowptr, colidx)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if len(rowptr) != self.N + 1:
            raise CoraError(5, "rowptr must have N+1 entries")
        if len(colidx) != rowptr[-1] or len(vals) != rowptr[-1]:
            raise CoraError(5, "colidx and vals must have rowptr[N] entries")
        self._chk(self.L.cora_update_values(self.h, rowptr.ctypes.data_as(_ip), colidx.ctypes.data_as(_ip), _d(vals)))

    def update_values_dev(self, d_vals):
        """The same from nnz doubles in CSR order on the device (a raw pointer as an int); needs the map."""
        self._chk(self.L.cora_update_values_dev(self.h, C.c_void_p(d_vals)))

    def update_values_times(self):
        """Milliseconds of the last update: map build, host check, upload, device passes, host refresh."""
        out = (C.c_double * 5)()
        self._chk(self.L.cora_update_values_times(self.h, out))
        return [out[i] for i in range(5)]

    # ---- Q(w) assembled from per-measurement weights (include/cora_hip.h, cora_assembly_build)
    def assembly_build(self, rowptr, colidx):
        """Builds the term map of Q(w) over the pattern the handle was created with; needs a measurement table."""
        rowptr, colidx = self._csr(rowptr, colidx)
        if len(rowptr) != self.N + 1:
            raise CoraError(5, "rowptr must have N+1 entries")
        if len(colidx) != rowptr[-1]:
            raise CoraError(5, "colidx must have rowptr[N] entries")
        self._chk(self.L.cora_assembly_build(self.h, rowptr.ctypes.data_as(_ip), colidx.ctypes.data_as(_ip)))
        self._asm_nnz = int(rowptr[-1])

    def assembly_info(self):
        """dict n_weights, n_terms, long_entries, max_terms of the term map."""
        out = (C.c_int64 * 4)()
        self._chk(self.L.cora_assembly_info(self.h, out))
        return dict(zip(["n_weights", "n_terms", "long_entries", "max_terms"], [int(x) for x in out]))

    def _weights(self, w):
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        if len(w) != self.assembly_info()["n_weights"]:
            raise CoraError(5, "the weight vector must have 2 * n_edges + n_ranges entries")
        return w

    def assemble_values(self, w):
        """Q(w) from host weights [rot | trans | range]; returns the assembled CSR values (the handle's new bits).
        Afterwards the handle is in the state of a fresh one, with the measurement table following the weights."""
        w = self._weights(w)
        vals = np.zeros(max(self._asm_nnz, 1))
        self._chk(self.L.cora_assemble_values(self.h, _d(w), _d(vals)))
        return vals[:self._asm_nnz]

    def assemble_values_dev(self, d_w, d_vals_out=None):
        """The same from weights on the device (raw pointers as ints); d_vals_out: None or nnz device doubles."""
        self._chk(self.L.cora_assemble_values_dev(self.h, C.c_void_p(d_w), C.c_void_p(d_vals_out)))

    def debug_assemble_values_host(self, w):
        """Test hook: the term map executed on the host in the device's order (no GPU needed, the handle is unchanged)."""
        w = self._weights(w)
        vals = np.zeros(max(self._asm_nnz, 1))
        self._chk(self.L.cora_debug_assemble_values_host(self.h, _d(w), _d(vals)))
        return vals[:self._asm_nnz]

    def assemble_times(self):
        """Milliseconds: term map build, weight check, assembly kernels (events), update passes, copies + host refresh."""
        out = (C.c_double * 5)()
        self._chk(self.L.cora_assemble_times(self.h, out))
        return [out[i] for i in range(5)]

    # ---- the weight step of a robust-cost (GNC) loop (include/cora_hip.h, cora_gnc_weights_dev)
    GNC_COSTS = {"none": 0, "tls": 1, "gm": 2}

    @staticmethod
    def _gnc_stats(st):
        names = ("sum_wr2", "max_rho", "n_mid", "n_out")
        return {seg: dict(zip(names, st[4 * i:4 * i + 4])) for i, seg in enumerate(("rot", "trans", "range"))}

    def _gnc_host(self, fn, X, barc2, cost, mu, couple_edges):
        X = _f(X)
        barc2 = self._weights(barc2)
        w, r2, st = np.zeros(max(len(barc2), 1)), np.zeros(max(len(barc2), 1)), np.zeros(12)
        self._chk(fn(self.h, _d(X), X.shape[0], X.shape[1], _d(barc2), int(self.GNC_COSTS.get(cost, cost)),
                     int(bool(couple_edges)), C.c_double(mu), _d(w), _d(r2), _d(st)))
        return dict(w=w[:len(barc2)], r2=r2[:len(barc2)], stats=self._gnc_stats(st), stats_raw=st)

    def gnc_weights(self, X, barc2, cost, mu=1.0, couple_edges=False):
        """Weight step at the host matrix X (N x k).  barc2: thresholds in the weight layout [rot | trans | range] (+inf:
        trusted); cost: 'none' | 'tls' | 'gm' (or the integer).  Returns dict w, r2 (unweighted residuals), stats
        ({'rot' | 'trans' | 'range': sum_wr2, max_rho, n_mid, n_out}) and stats_raw (the 12 doubles)."""
        return self._gnc_host(self.L.cora_gnc_weights, X, barc2, cost, mu, couple_edges)

    def debug_gnc_weights_host(self, X, barc2, cost, mu=1.0, couple_edges=False):
        """Test hook: the same sequence on the host (no GPU needed, the handle is unchanged)."""
        return self._gnc_host(self.L.cora_debug_gnc_weights_host, X, barc2, cost, mu, couple_edges)

    def gnc_weights_dev(self, x, k, d_barc2, cost, mu, couple_edges, d_w_out, d_r2_out=None):
        """The same on device vectors (raw pointers as ints): x a resident vector of k columns, d_barc2 / d_w_out /
        d_r2_out (or None) n_weights device doubles.  Returns the statistics (dict, 'raw': the 12 doubles)."""
        st = np.zeros(12)
        self._chk(self.L.cora_gnc_weights_dev(self.h, C.c_void_p(x), int(k), C.c_void_p(d_barc2),
                                              int(self.GNC_COSTS.get(cost, cost)), int(bool(couple_edges)), C.c_double(mu),
                                              C.c_void_p(d_w_out), C.c_void_p(d_r2_out), _d(st)))
        out = self._gnc_stats(st)
        out["raw"] = st
        return out

    # ---- trajectory error against a reference after an orthogonal alignment (include/cora_hip.h, cora_compare_dev)
    COMPARE_PROPER = 1

    def _select(self, select):
        if select is None:
            return None, None
        s = np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8)
        if s.shape != (self.nt,):
            raise CoraError(1, "select must have n_trans = %d entries" % self.nt)
        return s, s.ctypes.data_as(C.c_void_p)

    def _compare_result(self, k, kr, et, er, el, out, aligned=None):
        o = 8 + kr
        names = ("m", "sum_et2", "max_et", "sum_er2", "max_er", "n_landmarks", "sum_el2", "max_el")
        res = dict(zip(names, out[:8]))
        res.update(pose_trans_err=et[:self.n], pose_rot_err=er[:self.n], landmark_err=el[:self.nt - self.n], sigma=out[8:o],
                   xbar=out[o:o + k], gbar=out[o + k:o + k + kr], A=out[o + k + kr:].reshape(kr, k).T.copy(), raw=out)
        if aligned is not None:
            res["aligned"] = aligned
        return res

    def _compare_host(self, fn, X, Ref, select, proper, aligned):
        X, Ref = _f(X), _f(Ref)
        k, kr = X.shape[1], Ref.shape[1]
        sel, selp = self._select(select)
        et, er, el = np.zeros(max(self.n, 1)), np.zeros(max(self.n, 1)), np.zeros(max(self.nt - self.n, 1))
        out = np.zeros(8 + kr + k + kr + k * kr)
        al = self._out(kr) if aligned else None
        self._chk(fn(self.h, _d(X), X.shape[0], k, _d(Ref), Ref.shape[0], kr, selp, self.COMPARE_PROPER if proper else 0,
                     _d(et), _d(er), _d(el), _d(al) if aligned else None, self.N, _d(out)))
        return self._compare_result(k, kr, et, er, el, out, al)

    def compare(self, X, Ref, select=None, proper=False, aligned=False):
        """Errors of the host matrix X (N x k) against Ref (N x kr) after the alignment on the selected poses' positions.
        select: n_trans flags (poses, then landmarks) or None = all.  Returns dict m, sum_et2, max_et, sum_er2, max_er,
        n_landmarks, sum_el2, max_el, pose_trans_err, pose_rot_err, landmark_err, sigma, xbar, gbar, A (k x kr), raw, and
        aligned (N x kr) when asked for."""
        return self._compare_host(self.L.cora_compare, X, Ref, select, proper, aligned)

    def debug_compare_host(self, X, Ref, select=None, proper=False, aligned=False):
        """The same operations on the host (no GPU needed, the handle is unchanged)."""
        return self._compare_host(self.L.cora_debug_compare_host, X, Ref, select, proper, aligned)

    def compare_dev(self, x, k, ref, kr, select=None, proper=False, d_aligned=None):
        """The same on resident vectors (raw pointers as ints); d_aligned: a resident vector of kr columns or None."""
        sel, selp = self._select(select)
        et, er, el = np.zeros(max(self.n, 1)), np.zeros(max(self.n, 1)), np.zeros(max(self.nt - self.n, 1))
        out = np.zeros(8 + kr + k + kr + k * kr)
        self._chk(self.L.cora_compare_dev(self.h, C.c_void_p(x), int(k), C.c_void_p(ref), int(kr), selp,
                                          self.COMPARE_PROPER if proper else 0, _d(et), _d(er), _d(el), C.c_void_p(d_aligned),
                                          _d(out)))
        return self._compare_result(k, kr, et, er, el, out)

    def debug_compare_H(self, k, kr):
        """Test hook: H (k x kr) of the last comparison on this handle."""
        H = np.zeros((k, kr), order="F")
        self._chk(self.L.cora_debug_compare_H(self.h, int(k), int(kr), _d(H)))
        return H

    # ---- relative pose error over a pair table kept on the handle (include/cora_hip.h, cora_rpe_dev)
    def set_pose_pairs(self, pairs):
        """Installs the table of pose pairs (m x 2 API pose indices; None or an empty table clears it)."""
        if pairs is None:
            self._chk(self.L.cora_set_pose_pairs(self.h, C.c_int64(0), None))
            return
        p = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        self._chk(self.L.cora_set_pose_pairs(self.h, C.c_int64(len(p)), p.ctypes.data_as(_ip) if len(p) else None))

    def pose_pairs_count(self):
        m = C.c_int64(0)
        self._chk(self.L.cora_pose_pairs_count(self.h, C.byref(m)))
        return int(m.value)

    def pose_pairs_equal(self, pairs):
        """Whether the table holds exactly these pairs in this order (None or empty: no table)."""
        p = np.zeros((0, 2), dtype=np.int32) if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        same = C.c_int(0)
        self._chk(self.L.cora_pose_pairs_equal(self.h, C.c_int64(len(p)), p.ctypes.data_as(_ip) if len(p) else None, C.byref(same)))
        return bool(same.value)

    @staticmethod
    def _rpe_result(m, et, er, out, arrays=True):
        names = ("m", "sum_et2", "max_et", "sum_er2", "max_er", "argmax_et")
        res = dict(zip(names, out))
        res["raw"] = out
        if arrays:
            res.update(trans_err=et[:m], rot_err=er[:m])
        return res

    def _rpe_host(self, fn, X, Ref, arrays):
        X, Ref = _f(X), _f(Ref)
        m = self.pose_pairs_count()
        et, er, out = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(6)
        self._chk(fn(self.h, _d(X), X.shape[0], X.shape[1], _d(Ref), Ref.shape[0], Ref.shape[1], _d(et) if arrays else None,
                     _d(er) if arrays else None, _d(out)))
        return self._rpe_result(m, et, er, out, arrays)

    def rpe(self, X, Ref, arrays=True):
        """Relative pose errors of the host matrix X (N x k) against Ref (N x kr; k and kr independent) over the pair
        table.  Returns dict m, sum_et2, max_et, sum_er2, max_er, argmax_et (first pair that attains max_et), raw, and
        trans_err, rot_err (m each) unless arrays is False."""
        return self._rpe_host(self.L.cora_rpe, X, Ref, arrays)

    def debug_rpe_host(self, X, Ref, arrays=True):
        """The same definitions on the host in the device's lane and tree order (no GPU needed, the handle is unchanged)."""
        return self._rpe_host(self.L.cora_debug_rpe_host, X, Ref, arrays)

    def rpe_dev(self, x, k, ref, kr, arrays=True):
        """The same on resident vectors (raw pointers as ints); arrays=False reads back the six statistics only."""
        m = self.pose_pairs_count()
        et, er, out = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(6)
        self._chk(self.L.cora_rpe_dev(self.h, C.c_void_p(x), int(k), C.c_void_p(ref), int(kr), _d(et) if arrays else None,
                                      _d(er) if arrays else None, _d(out)))
        return self._rpe_result(m, et, er, out, arrays)

    # ---- rounding of a relaxed point to SE(d) (include/cora_hip.h, cora_round_dev)
    def _round_result(self, k, out, rounded=None):
        d = self.d
        res = dict(count=int(out[0]), flipped=bool(out[1]), sigma=out[2:2 + k].copy(),
                   Vd=out[2 + k:2 + k + k * d].reshape(d, k).T.copy(), raw=out)
        if rounded is not None:
            res["X"] = rounded
        return res

    def round(self, Y):
        """Rounds the host matrix Y (N x k, d <= k <= 24) to SE(d) on the device.  Returns dict X (N x d), count (pose
        blocks of positive determinant), flipped, sigma (k singular values), Vd (k x d), raw."""
        Y = _f(Y)
        k = Y.shape[1]
        X, out = np.zeros((Y.shape[0], self.d), order="F"), np.zeros(2 + k + k * self.d)
        self._chk(self.L.cora_round(self.h, _d(Y), Y.shape[0], int(k), _d(X), X.shape[0], _d(out)))
        return self._round_result(k, out, X)

    def debug_round_host(self, Y, basis=None):
        """The same on the host through the functions the kernels call (no GPU needed).  basis: a k x d matrix to use in
        place of the eigenvectors of this form's own Gram matrix (the Vd of a device call: the rows, the count and the flip
        then have the device's bits)."""
        Y = _f(Y)
        k = Y.shape[1]
        X, out = np.zeros((Y.shape[0], self.d), order="F"), np.zeros(2 + k + k * self.d)
        B = None if basis is None else np.asfortranarray(np.asarray(basis, dtype=np.float64).reshape(k, self.d))
        self._chk(self.L.cora_debug_round_host(self.h, _d(Y), Y.shape[0], int(k), None if B is None else _d(B), _d(X),
                                               X.shape[0], _d(out)))
        return self._round_result(k, out, X)

    def round_dev(self, y, k, out_ptr):
        """The same on resident vectors (raw pointers as ints): y has k columns, out_ptr d columns; they must not overlap.
        Returns the dict of round() without X."""
        out = np.zeros(2 + k + k * self.d)
        self._chk(self.L.cora_round_dev(self.h, C.c_void_p(y), int(k), C.c_void_p(out_ptr), _d(out)))
        return self._round_result(k, out)

    # ---- odometry initialisation by a segmented scan of SE(d) (include/cora_hip.h, cora_odometry_init_dev)
    def set_odometry_chains(self, chains):
        """Installs the chains (a list of lists of edge indices into the measurement table; None or [] clears them)."""
        chains = [np.asarray(ch, dtype=np.int32).reshape(-1) for ch in (chains or [])]
        ptr = np.zeros(len(chains) + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([len(ch) for ch in chains])
        edges = np.ascontiguousarray(np.concatenate(chains) if chains else np.zeros(0), dtype=np.int32)
        edges = np.concatenate([edges, np.zeros(1, dtype=np.int32)])  # (never an empty buffer)
        self._chk(self.L.cora_set_odometry_chains(self.h, C.c_int64(len(chains)), ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  edges.ctypes.data_as(_ip)))

    def _two_int64(self, fn):
        out = (C.c_int64 * 2)()
        self._chk(fn(self.h, out))
        return int(out[0]), int(out[1])

    def odometry_chains_count(self):
        """(chains, positions) of the installed tables."""
        return self._two_int64(self.L.cora_odometry_chains_count)

    def odometry_scan_shape(self):
        """(positions per tile, tile totals per sweep of the middle pass)."""
        return self._two_int64(self.L.cora_odometry_scan_shape)

    def _odom_inputs(self, starts, landmarks):
        n_ch = self.odometry_chains_count()[0]
        s = np.ascontiguousarray(np.zeros((0, self.d)) if starts is None else starts, dtype=np.float64).reshape(-1, self.d)
        if len(s) != n_ch:
            raise CoraError(5, "one start per chain: %d chains, %d starts" % (n_ch, len(s)))
        lm = None
        if landmarks is not None:
            lm = np.ascontiguousarray(landmarks, dtype=np.float64).reshape(-1, self.d)
            if len(lm) != self.nt - self.n:
                raise CoraError(5, "one row per landmark: %d landmarks, %d rows" % (self.nt - self.n, len(lm)))
            lm = np.concatenate([lm.reshape(-1), np.zeros(1)])
        return np.concatenate([s.reshape(-1), np.zeros(1)]), lm

    def _odom_result(self, out, deg, X=None):
        nr = self.measurement_counts()[1]
        res = dict(written=int(out[0]), n_degenerate=int(out[1]), degenerate=deg[:nr].astype(bool))
        if X is not None:
            res["X"] = X
        return res

    def _odom_host(self, fn, starts, landmarks):
        s, lm = self._odom_inputs(starts, landmarks)
        X, out = self._out(self.d), (C.c_int64 * 2)()
        deg = np.zeros(max(self.measurement_counts()[1], 1), dtype=np.uint8)
        self._chk(fn(self.h, _d(s), None if lm is None else _d(lm), _d(X), X.shape[0], out, deg.ctypes.data_as(C.c_void_p)))
        return self._odom_result(out, deg, X)

    def odometry_init(self, starts, landmarks=None):
        """The odometry start on the device: starts [chains][d], landmarks [nt - n][d] or None (zeros).  Returns dict X
        (N x d), written (poses the chains wrote), n_degenerate, degenerate (bool per range measurement of the table)."""
        return self._odom_host(self.L.cora_odometry_init, starts, landmarks)

    def debug_odometry_init_host(self, starts, landmarks=None):
        """The same on the host in the device's bracket order (no GPU needed): X has the device's bits."""
        return self._odom_host(self.L.cora_debug_odometry_init_host, starts, landmarks)

    def odometry_init_dev(self, starts, landmarks, out_ptr):
        """The same into a resident vector of d columns (a raw pointer as an int); the dict of odometry_init without X."""
        s, lm = self._odom_inputs(starts, landmarks)
        out = (C.c_int64 * 2)()
        deg = np.zeros(max(self.measurement_counts()[1], 1), dtype=np.uint8)
        self._chk(self.L.cora_odometry_init_dev(self.h, _d(s), None if lm is None else _d(lm), C.c_void_p(out_ptr), out,
                                                deg.ctypes.data_as(C.c_void_p)))
        return self._odom_result(out, deg)

    def odometry_set_range_rows_dev(self, range_idx, dirs, out_ptr):
        """Writes the normalised directions (m x d) into the rows of the range measurements range_idx of a resident vector."""
        idx = np.ascontiguousarray(range_idx, dtype=np.int32).reshape(-1)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(len(idx), self.d)
        if len(idx):
            self._chk(self.L.cora_odometry_set_range_rows_dev(self.h, C.c_int64(len(idx)), idx.ctypes.data_as(_ip), _d(dirs),
                                                              C.c_void_p(out_ptr)))

    # ---- shared by the initialisers below
    def _mask(self, a, m, what):
        """(array, pointer) of a mask of m entries as bytes, (None, None) for None; the array owns the pointer's memory."""
        if a is None:
            return None, None
        a = np.ascontiguousarray(np.asarray(a).reshape(-1) != 0, dtype=np.uint8)
        if len(a) != m:
            raise CoraError(5, "%s needs %d entries, not %d" % (what, m, len(a)))
        a = np.concatenate([a, np.zeros(1, dtype=np.uint8)])  # (never an empty buffer)
        return a, a.ctypes.data_as(C.c_void_p)

    def _with_host_X(self, call, fn, X, *args):
        """call's dict of a host-matrix form fn (handle, X, ldx, ..) on a copy of X (N x d), the copy attached as X."""
        X = np.array(X, dtype=np.float64, order="F", copy=True)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise CoraError(1, "X must have d columns")
        res = call(lambda *a: fn(self.h, _d(X), X.shape[0], *a), *args)
        res["X"] = X
        return res

    # ---- landmark initialisation from ranges: multilateration (include/cora_hip.h, cora_multilaterate_dev)
    def set_multilateration(self, pose_ok=None, landmark_on=None):
        """Groups the usable ranges of the measurement table per landmark: pose_ok [n] / landmark_on [nt - n] masks or
        None (all)."""
        po, ppo = self._mask(pose_ok, self.n, "pose_ok")
        lo, plo = self._mask(landmark_on, self.nt - self.n, "landmark_on")
        self._chk(self.L.cora_set_multilateration(self.h, ppo, plo))

    def multilateration_counts(self):
        """(landmarks with a list, usable ranges, skipped ranges, chunks) of the installed tables."""
        out = (C.c_int64 * 4)()
        self._chk(self.L.cora_multilateration_counts(self.h, out))
        return tuple(int(v) for v in out)

    def _ml_call(self, fn, gn_steps):
        nl, nr = self.nt - self.n, self.measurement_counts()[1]
        out = (C.c_int64 * 4)()
        status, chosen = np.zeros(nl + 1, dtype=np.uint8), np.zeros(nl + 1, dtype=np.int32)
        cl, cf, deg = np.zeros(nl + 1), np.zeros(nl + 1), np.zeros(nr + 1, dtype=np.uint8)
        self._chk(fn(int(gn_steps), out, status.ctypes.data_as(C.c_void_p), _d(cl), _d(cf), chosen.ctypes.data_as(_ip),
                     deg.ctypes.data_as(C.c_void_p)))
        return dict(solved=int(out[0]), not_solved=int(out[1]), n_degenerate=int(out[2]), steps=int(out[3]), status=status[:nl],
                    cost_linear=cl[:nl], cost_final=cf[:nl], chosen=chosen[:nl], degenerate=deg[:nr].astype(bool))

    def multilaterate(self, X, gn_steps=5):
        """The landmarks of the host matrix X (N x d) from the ranges, on the device.  Returns dict X (a copy with the
        landmark and range rows rewritten), solved, not_solved, n_degenerate, steps, status, cost_linear, cost_final,
        chosen (per landmark), degenerate (bool per range measurement)."""
        return self._with_host_X(self._ml_call, self.L.cora_multilaterate, X, gn_steps)

    def debug_multilaterate_host(self, X, gn_steps=5):
        """The same on the host in the device's bracket order (no GPU needed): X has the device's bits."""
        return self._with_host_X(self._ml_call, self.L.cora_debug_multilaterate_host, X, gn_steps)

    def multilaterate_dev(self, x_ptr, gn_steps=5):
        """The same in place in a resident vector of d columns (a raw pointer as an int); the dict without X."""
        return self._ml_call(lambda *a: self.L.cora_multilaterate_dev(self.h, C.c_void_p(x_ptr), *a), gn_steps)

    # ---- outlier-robust multilateration (include/cora_hip.h, cora_multilaterate_robust_dev)
    def _mlr_call(self, fn, gn_steps, barc2, min_consensus):
        nl, nr = self.nt - self.n, self.measurement_counts()[1]
        out = (C.c_int64 * 6)()
        status, chosen = np.zeros(nl + 1, dtype=np.uint8), np.zeros(nl + 1, dtype=np.int32)
        cl, cf, deg = np.zeros(nl + 1), np.zeros(nl + 1), np.zeros(nr + 1, dtype=np.uint8)
        el, cons, ll = (np.zeros(nl + 1, dtype=np.int32) for _ in range(3))
        inl = np.zeros(nr + 1, dtype=np.uint8)
        self._chk(fn(int(gn_steps), C.c_double(barc2), int(min_consensus), out, status.ctypes.data_as(C.c_void_p), _d(cl), _d(cf),
                     chosen.ctypes.data_as(_ip), el.ctypes.data_as(_ip), cons.ctypes.data_as(_ip), ll.ctypes.data_as(_ip),
                     inl.ctypes.data_as(C.c_void_p), deg.ctypes.data_as(C.c_void_p)))
        return dict(solved=int(out[0]), not_solved=int(out[1]), n_degenerate=int(out[2]), steps=int(out[3]), no_consensus=int(out[4]),
                    excluded=int(out[5]), status=status[:nl], cost_linear=cl[:nl], cost_final=cf[:nl], chosen=chosen[:nl], elected=el[:nl],
                    consensus=cons[:nl], list_len=ll[:nl], inlier=inl[:nr], degenerate=deg[:nr].astype(bool))

    def multilaterate_robust(self, X, barc2, gn_steps=5, min_consensus=None):
        """multilaterate with a consensus vote in front of the fit: every entry of a landmark's list proposes the point its
        sample of d + 1 ranges determines, the proposal most ranges agree with (weighted squared residual <= barc2) is elected
        and the fit runs over the agreeing ranges only.  min_consensus None: d + 2.  Returns multilaterate's dict plus elected,
        consensus and list_len (per landmark), inlier (per range measurement: 1 | 0 | 2 in no list that is voted on),
        no_consensus (landmarks of status 5) and excluded (ranges with byte 0)."""
        return self._with_host_X(self._mlr_call, self.L.cora_multilaterate_robust, X, gn_steps, barc2, self._ml_min(min_consensus))

    def debug_multilaterate_robust_host(self, X, barc2, gn_steps=5, min_consensus=None):
        """The same on the host in the device's bracket order (no GPU needed): the device's bits."""
        return self._with_host_X(self._mlr_call, self.L.cora_debug_multilaterate_robust_host, X, gn_steps, barc2, self._ml_min(min_consensus))

    def multilaterate_robust_dev(self, x_ptr, barc2, gn_steps=5, min_consensus=None):
        """The same in place in a resident vector of d columns (a raw pointer as an int); the dict without X."""
        return self._mlr_call(lambda *a: self.L.cora_multilaterate_robust_dev(self.h, C.c_void_p(x_ptr), *a), gn_steps, barc2,
                              self._ml_min(min_consensus))

    def _ml_min(self, min_consensus):
        return self.d + 2 if min_consensus is None else int(min_consensus)

    # ---- chain placement from inter-robot ranges (include/cora_hip.h, cora_place_chains_dev)
    def set_chain_placement(self, chain_fixed=None, min_ranges=None):
        """Orders the odometry chains into stages from the pose-pose ranges between them: chain_fixed a mask per chain or
        None (chain 0); min_ranges None: 4 x the unknowns of the linear stage (28 at d = 2, 64 at d = 3)."""
        if min_ranges is None:
            min_ranges = 4 * (7 if self.d == 2 else 16)
        keep, ptr = self._mask(chain_fixed, self.odometry_chains_count()[0], "chain_fixed")
        self._chk(self.L.cora_set_chain_placement(self.h, ptr, int(min_ranges)))

    def set_chain_placement_order(self, chain_fixed=None, min_ranges=None, order=PL_ORDER_LEVELS):
        """set_chain_placement with the order of the stages chosen: PL_ORDER_GREEDY (its tables exactly) or PL_ORDER_LEVELS
        (level k: every chain not yet placed with min_ranges entries against the chains of levels < k, its list those
        entries only)."""
        if min_ranges is None:
            min_ranges = 4 * (7 if self.d == 2 else 16)
        keep, ptr = self._mask(chain_fixed, self.odometry_chains_count()[0], "chain_fixed")
        self._chk(self.L.cora_set_chain_placement_order(self.h, ptr, int(min_ranges), int(order)))

    def chain_placement_counts(self):
        """(stages, entries, chunks, skipped ranges) of the installed tables."""
        out = (C.c_int64 * 4)()
        self._chk(self.L.cora_chain_placement_counts(self.h, out))
        return tuple(int(v) for v in out)

    def chain_placement_order(self):
        """The chain of every stage, in the order of the stages."""
        order = np.zeros(self.chain_placement_counts()[0] + 1, dtype=np.int32)
        self._chk(self.L.cora_chain_placement_order(self.h, order.ctypes.data_as(_ip)))
        return order[:-1]

    def chain_placement_levels(self):
        """The level (>= 1; level 0 holds the fixed chains) of every stage, in the order of the stages."""
        level = np.zeros(self.chain_placement_counts()[0] + 1, dtype=np.int32)
        self._chk(self.L.cora_chain_placement_levels(self.h, level.ctypes.data_as(_ip)))
        return level[:-1]

    def _pl_call(self, fn, gn_steps, batched=False):
        nch, nr, g = self.odometry_chains_count()[0], self.measurement_counts()[1], self.d * self.d + self.d
        out = (C.c_int64 * 6)()
        status, chosen = np.zeros(nch + 1, dtype=np.uint8), np.zeros(nch + 1, dtype=np.int32)
        cs, cl, cf, tr = np.zeros(nch + 1), np.zeros(nch + 1), np.zeros(nch + 1), np.zeros((nch + 1) * g)
        deg = np.zeros(nr + 1, dtype=np.uint8)
        self._chk(fn(int(gn_steps), out, status.ctypes.data_as(C.c_void_p), _d(cs), _d(cl), _d(cf), chosen.ctypes.data_as(_ip), _d(tr),
                     deg.ctypes.data_as(C.c_void_p)))
        res = dict(placed=int(out[0]), not_placed=int(out[1]), steps=int(out[2]), n_degenerate=int(out[3]), stages=int(out[4]),
                   status=status[:nch], cost_start=cs[:nch], cost_linear=cl[:nch], cost_final=cf[:nch], chosen=chosen[:nch],
                   transforms=tr[:nch * g].reshape(nch, g), degenerate=deg[:nr].astype(bool))
        if batched:
            res["levels"] = int(out[5])
        return res

    def place_chains(self, X, gn_steps=5):
        """The chains of the host matrix X (N x d) moved rigidly onto the fixed chains from the ranges between chains, on
        the device.  Returns dict X (a copy with the chains' rows and the range rows rewritten), placed, not_placed, steps,
        n_degenerate, stages, status, cost_start, cost_linear, cost_final, chosen (per chain), transforms (per chain: R
        row-major, then t), degenerate (bool per range measurement)."""
        return self._with_host_X(self._pl_call, self.L.cora_place_chains, X, gn_steps)

    def debug_place_chains_host(self, X, gn_steps=5):
        """The same on the host in the device's bracket order (no GPU needed): X has the device's bits."""
        return self._with_host_X(self._pl_call, self.L.cora_debug_place_chains_host, X, gn_steps)

    def place_chains_dev(self, x_ptr, gn_steps=5):
        """The same in place in a resident vector of d columns (a raw pointer as an int); the dict without X."""
        return self._pl_call(lambda *a: self.L.cora_place_chains_dev(self.h, C.c_void_p(x_ptr), *a), gn_steps)

    def place_chains_batched(self, X, gn_steps=5):
        """place_chains with every launch serving all stages of one level of the installed tables (the same bits); the dict
        also holds levels."""
        return self._with_host_X(lambda fn, g: self._pl_call(fn, g, batched=True), self.L.cora_place_chains_batched, X, gn_steps)

    def place_chains_batched_dev(self, x_ptr, gn_steps=5):
        """The same in place in a resident vector of d columns (a raw pointer as an int); the dict without X."""
        return self._pl_call(lambda *a: self.L.cora_place_chains_batched_dev(self.h, C.c_void_p(x_ptr), *a), gn_steps, batched=True)

    # ---- outlier-robust chain placement (include/cora_hip.h, cora_place_chains_robust_dev)
    def _plr_call(self, fn, gn_steps, barc2, min_consensus):
        nch, nr, g = self.odometry_chains_count()[0], self.measurement_counts()[1], self.d * self.d + self.d
        out = (C.c_int64 * 8)()
        status, chosen = np.zeros(nch + 1, dtype=np.uint8), np.zeros(nch + 1, dtype=np.int32)
        cs, cl, cf, tr = np.zeros(nch + 1), np.zeros(nch + 1), np.zeros(nch + 1), np.zeros((nch + 1) * g)
        el, cons, ll = (np.zeros(nch + 1, dtype=np.int32) for _ in range(3))
        inl, deg = np.zeros(nr + 1, dtype=np.uint8), np.zeros(nr + 1, dtype=np.uint8)
        self._chk(fn(int(gn_steps), C.c_double(barc2), int(min_consensus), out, status.ctypes.data_as(C.c_void_p), _d(cs), _d(cl), _d(cf),
                     chosen.ctypes.data_as(_ip), _d(tr), el.ctypes.data_as(_ip), cons.ctypes.data_as(_ip), ll.ctypes.data_as(_ip),
                     inl.ctypes.data_as(C.c_void_p), deg.ctypes.data_as(C.c_void_p)))
        return dict(placed=int(out[0]), not_placed=int(out[1]), steps=int(out[2]), n_degenerate=int(out[3]), stages=int(out[4]),
                    levels=int(out[5]), no_consensus=int(out[6]), excluded=int(out[7]), status=status[:nch], cost_start=cs[:nch],
                    cost_linear=cl[:nch], cost_final=cf[:nch], chosen=chosen[:nch], transforms=tr[:nch * g].reshape(nch, g),
                    elected=el[:nch], consensus=cons[:nch], list_len=ll[:nch], inlier=inl[:nr], degenerate=deg[:nr].astype(bool))

    def place_chains_robust(self, X, barc2, gn_steps=5, min_consensus=None):
        """place_chains_batched with a consensus vote in front of the fit: every entry of a stage's list proposes the motion its
        sample of m ranges determines (m = 8 at d = 2, 17 at d = 3: the linear stage, then 3 Gauss-Newton steps on the sample),
        the proposal most ranges agree with (weighted squared residual <= barc2) is elected and the fit runs over the agreeing
        ranges only.  min_consensus None: 2 m.  Returns place_chains_batched's dict plus elected, consensus and list_len (per
        chain), inlier (per range measurement: 1 | 0 | 2 in no stage list), no_consensus (stages of status 5) and excluded
        (ranges with byte 0)."""
        return self._with_host_X(self._plr_call, self.L.cora_place_chains_robust, X, gn_steps, barc2, self._pl_min(min_consensus))

    def debug_place_chains_robust_host(self, X, barc2, gn_steps=5, min_consensus=None):
        """The same on the host in the device's bracket order (no GPU needed): the device's bits."""
        return self._with_host_X(self._plr_call, self.L.cora_debug_place_chains_robust_host, X, gn_steps, barc2, self._pl_min(min_consensus))

    def place_chains_robust_dev(self, x_ptr, barc2, gn_steps=5, min_consensus=None):
        """The same in place in a resident vector of d columns (a raw pointer as an int); the dict without X."""
        return self._plr_call(lambda *a: self.L.cora_place_chains_robust_dev(self.h, C.c_void_p(x_ptr), *a), gn_steps, barc2,
                              self._pl_min(min_consensus))

    def _pl_min(self, min_consensus):
        return 2 * (8 if self.d == 2 else 17) if min_consensus is None else int(min_consensus)

    # ---- placement from pose-landmark sightings (include/cora_hip.h, cora_place_by_sightings_dev)
    def set_sighting_placement(self, chain_fixed=None, landmark_fixed=None, min_sightings=None):
        """Orders landmarks and odometry chains into stages from the pose-landmark sightings: chain_fixed a mask per chain
        or None (chain 0); landmark_fixed a mask per landmark or None (none); min_sightings None: 4 d."""
        if min_sightings is None:
            min_sightings = 4 * self.d
        kc, pc = self._mask(chain_fixed, self.odometry_chains_count()[0], "chain_fixed")
        kl, plm = self._mask(landmark_fixed, self.nt - self.n, "landmark_fixed")
        self._chk(self.L.cora_set_sighting_placement(self.h, pc, plm, int(min_sightings)))

    def sighting_placement_counts(self):
        """(stages, sightings used, chunks, skipped edges) of the installed tables."""
        out = (C.c_int64 * 4)()
        self._chk(self.L.cora_sighting_placement_counts(self.h, out))
        return tuple(int(v) for v in out)

    def sighting_placement_order(self):
        """The stages in order as a list of (kind, items): kind "L", "C" or "REFIT", items the landmarks or chains."""
        ns, _, nc, _ = self.sighting_placement_counts()
        kind, ptr = np.zeros(ns + 1, dtype=np.int32), np.zeros(ns + 2, dtype=np.int32)
        items = np.zeros(nc + 1, dtype=np.int32)  # (a list has at least one chunk)
        self._chk(self.L.cora_sighting_placement_order(self.h, kind.ctypes.data_as(_ip), ptr.ctypes.data_as(_ip), items.ctypes.data_as(_ip)))
        return [(("L", "C", "REFIT")[kind[s]], items[ptr[s]:ptr[s + 1]].copy()) for s in range(ns)]

    def _sg_call(self, fn):
        nch, nr, g, nl = self.odometry_chains_count()[0], self.measurement_counts()[1], self.d * self.d + self.d, self.nt - self.n
        out = (C.c_int64 * 6)()
        status, chosen = np.zeros(nch + 1, dtype=np.uint8), np.zeros(nch + 1, dtype=np.int32)
        cs, cf, tr = np.zeros(nch + 1), np.zeros(nch + 1), np.zeros((nch + 1) * g)
        ls, lc = np.zeros(nl + 1, dtype=np.uint8), np.zeros(nl + 1)
        deg = np.zeros(nr + 1, dtype=np.uint8)
        self._chk(fn(out, status.ctypes.data_as(C.c_void_p), _d(cs), _d(cf), chosen.ctypes.data_as(_ip), _d(tr),
                     ls.ctypes.data_as(C.c_void_p), _d(lc), deg.ctypes.data_as(C.c_void_p)))
        return dict(placed=int(out[0]), not_placed=int(out[1]), landmarks_placed=int(out[2]), landmarks_not_placed=int(out[3]),
                    n_degenerate=int(out[4]), stages=int(out[5]), status=status[:nch], cost_start=cs[:nch], cost_final=cf[:nch],
                    chosen=chosen[:nch], transforms=tr[:nch * g].reshape(nch, g), landmark_status=ls[:nl], landmark_cost=lc[:nl],
                    degenerate=deg[:nr].astype(bool))

    def place_by_sightings(self, X):
        """Landmarks and chains of the host matrix X (N x d) placed from the sightings, on the device.  Returns dict X (a
        copy with the landmarks', the chains' and the range rows rewritten), placed, not_placed, landmarks_placed,
        landmarks_not_placed, n_degenerate, stages, status, cost_start, cost_final, chosen (per chain), transforms (per
        chain: R row-major, then t), landmark_status, landmark_cost (per landmark), degenerate (bool per range measurement)."""
        return self._with_host_X(self._sg_call, self.L.cora_place_by_sightings, X)

    def debug_place_by_sightings_host(self, X):
        """The same on the host in the device's bracket order (no GPU needed): X has the device's bits."""
        return self._with_host_X(self._sg_call, self.L.cora_debug_place_by_sightings_host, X)

    def place_by_sightings_dev(self, x_ptr):
        """The same in place in a resident vector of d columns (a raw pointer as an int); the dict without X."""
        return self._sg_call(lambda *a: self.L.cora_place_by_sightings_dev(self.h, C.c_void_p(x_ptr), *a))

    # ---- outlier-robust placement from sightings (include/cora_hip.h, cora_place_by_sightings_robust_dev)
    def _sgr_call(self, fn, barc2, min_chain_consensus, min_landmark_consensus):
        nch, (ne, nr), g, nl = self.odometry_chains_count()[0], self.measurement_counts()[:2], self.d * self.d + self.d, self.nt - self.n
        if min_chain_consensus is None or min_chain_consensus <= 0:
            min_chain_consensus = self.d + 1
        out = (C.c_int64 * 10)()
        status, chosen = np.zeros(nch + 1, dtype=np.uint8), np.zeros(nch + 1, dtype=np.int32)
        cs, cf, tr = np.zeros(nch + 1), np.zeros(nch + 1), np.zeros((nch + 1) * g)
        ls, lc = np.zeros(nl + 1, dtype=np.uint8), np.zeros(nl + 1)
        deg = np.zeros(nr + 1, dtype=np.uint8)
        cc, cl = np.zeros(nch + 1, dtype=np.int32), np.zeros(nch + 1, dtype=np.int32)
        lcn, ll = np.zeros(nl + 1, dtype=np.int32), np.zeros(nl + 1, dtype=np.int32)
        ic, il = np.zeros(ne + 1, dtype=np.uint8), np.zeros(ne + 1, dtype=np.uint8)
        self._chk(fn(C.c_double(barc2), int(min_chain_consensus), int(min_landmark_consensus), out, status.ctypes.data_as(C.c_void_p), _d(cs),
                     _d(cf), chosen.ctypes.data_as(_ip), _d(tr), ls.ctypes.data_as(C.c_void_p), _d(lc), deg.ctypes.data_as(C.c_void_p),
                     cc.ctypes.data_as(_ip), cl.ctypes.data_as(_ip), lcn.ctypes.data_as(_ip), ll.ctypes.data_as(_ip),
                     ic.ctypes.data_as(C.c_void_p), il.ctypes.data_as(C.c_void_p)))
        return dict(placed=int(out[0]), not_placed=int(out[1]), landmarks_placed=int(out[2]), landmarks_not_placed=int(out[3]),
                    n_degenerate=int(out[4]), stages=int(out[5]), chains_no_consensus=int(out[6]), landmarks_no_consensus=int(out[7]),
                    chain_excluded=int(out[8]), landmark_excluded=int(out[9]), status=status[:nch], cost_start=cs[:nch], cost_final=cf[:nch],
                    chosen=chosen[:nch], transforms=tr[:nch * g].reshape(nch, g), landmark_status=ls[:nl], landmark_cost=lc[:nl],
                    degenerate=deg[:nr].astype(bool), chain_consensus=cc[:nch], chain_list_len=cl[:nch], landmark_consensus=lcn[:nl],
                    landmark_list_len=ll[:nl], inlier_chain=ic[:ne], inlier_landmark=il[:ne])

    def place_by_sightings_robust(self, X, barc2, min_chain_consensus=0, min_landmark_consensus=1):
        """place_by_sightings with a consensus vote in front of every fit: every sighting of a list proposes (a landmark at
        its own prediction; a chain motion from a sample of d sightings), the proposal most sightings agree with (tau |.|^2 <=
        barc2) is elected and the fit runs over the agreeing sightings only.  min_chain_consensus <= 0: d + 1.  Returns
        place_by_sightings' dict plus chain_consensus, chain_list_len (per chain), landmark_consensus, landmark_list_len (per
        landmark, the REFIT's), inlier_chain, inlier_landmark (per edge of the measurement table: 1 | 0 | 2 in no list),
        chains_no_consensus, landmarks_no_consensus (status 5) and chain_excluded, landmark_excluded (entries outside the inliers)."""
        return self._with_host_X(self._sgr_call, self.L.cora_place_by_sightings_robust, X, barc2, min_chain_consensus, min_landmark_consensus)

    def debug_place_by_sightings_robust_host(self, X, barc2, min_chain_consensus=0, min_landmark_consensus=1):
        """The same on the host in the device's bracket order (no GPU needed): the device's bits."""
        return self._with_host_X(self._sgr_call, self.L.cora_debug_place_by_sightings_robust_host, X, barc2, min_chain_consensus,
                                 min_landmark_consensus)

    def place_by_sightings_robust_dev(self, x_ptr, barc2, min_chain_consensus=0, min_landmark_consensus=1):
        """The same in place in a resident vector of d columns (a raw pointer as an int); the dict without X."""
        return self._sgr_call(lambda *a: self.L.cora_place_by_sightings_robust_dev(self.h, C.c_void_p(x_ptr), *a), barc2, min_chain_consensus,
                              min_landmark_consensus)

    # ---- placement from inter-chain relative-pose edges (include/cora_hip.h, cora_place_by_closures_dev)
    def set_closure_placement(self, chain_fixed=None, min_closures=1):
        """Orders the odometry chains into stages from the relative-pose edges between chains: chain_fixed a mask per chain
        or None (chain 0); min_closures >= 1."""
        kc, pc = self._mask(chain_fixed, self.odometry_chains_count()[0], "chain_fixed")
        self._chk(self.L.cora_set_closure_placement(self.h, pc, int(min_closures)))

    def closure_placement_counts(self):
        """(stages, closures used, chunks, skipped + unused edges) of the installed tables."""
        out = (C.c_int64 * 4)()
        self._chk(self.L.cora_closure_placement_counts(self.h, out))
        return tuple(int(v) for v in out)

    def closure_placement_order(self):
        """The stages in order: a list with the chains of each stage, ascending."""
        ns, _, nc, _ = self.closure_placement_counts()
        ptr, items = np.zeros(ns + 2, dtype=np.int32), np.zeros(nc + 1, dtype=np.int32)  # (a list has at least one chunk)
        self._chk(self.L.cora_closure_placement_order(self.h, ptr.ctypes.data_as(_ip), items.ctypes.data_as(_ip)))
        return [items[ptr[s]:ptr[s + 1]].copy() for s in range(ns)]

    def _cl_call(self, fn):
        nch, nr, g = self.odometry_chains_count()[0], self.measurement_counts()[1], self.d * self.d + self.d
        out = (C.c_int64 * 5)()
        status, chosen = np.zeros(nch + 1, dtype=np.uint8), np.zeros(nch + 1, dtype=np.int32)
        cs, cf, tr = np.zeros(nch + 1), np.zeros(nch + 1), np.zeros((nch + 1) * g)
        deg = np.zeros(nr + 1, dtype=np.uint8)
        self._chk(fn(out, status.ctypes.data_as(C.c_void_p), _d(cs), _d(cf), chosen.ctypes.data_as(_ip), _d(tr), deg.ctypes.data_as(C.c_void_p)))
        return dict(placed=int(out[0]), not_placed=int(out[1]), n_degenerate=int(out[2]), stages=int(out[3]), refused=int(out[4]),
                    status=status[:nch], cost_start=cs[:nch], cost_final=cf[:nch], chosen=chosen[:nch],
                    transforms=tr[:nch * g].reshape(nch, g), degenerate=deg[:nr].astype(bool))

    def place_by_closures(self, X):
        """The chains of the host matrix X (N x d) placed from the closures, on the device.  Returns dict X (a copy with the
        chains' and the range rows rewritten), placed, not_placed, n_degenerate, stages, refused, status, cost_start,
        cost_final, chosen (per chain), transforms (per chain: G row-major, then s), degenerate (bool per range measurement)."""
        return self._with_host_X(self._cl_call, self.L.cora_place_by_closures, X)

    def debug_place_by_closures_host(self, X):
        """The same on the host in the device's bracket order (no GPU needed): X has the device's bits."""
        return self._with_host_X(self._cl_call, self.L.cora_debug_place_by_closures_host, X)

    def place_by_closures_dev(self, x_ptr):
        """The same in place in a resident vector of d columns (a raw pointer as an int); the dict without X."""
        return self._cl_call(lambda *a: self.L.cora_place_by_closures_dev(self.h, C.c_void_p(x_ptr), *a))

    # ---- outlier-robust placement from closures (include/cora_hip.h, cora_place_by_closures_robust_dev)
    def _clr_call(self, fn, barc2, min_consensus):
        nch, ne, g = self.odometry_chains_count()[0], self.measurement_counts()[0], self.d * self.d + self.d
        out = (C.c_int64 * 7)()
        status, chosen = np.zeros(nch + 1, dtype=np.uint8), np.zeros(nch + 1, dtype=np.int32)
        cs, cf, tr = np.zeros(nch + 1), np.zeros(nch + 1), np.zeros((nch + 1) * g)
        cons, ll = np.zeros(nch + 1, dtype=np.int32), np.zeros(nch + 1, dtype=np.int32)
        inl = np.zeros(ne + 1, dtype=np.uint8)
        self._chk(fn(C.c_double(barc2), int(min_consensus), out, status.ctypes.data_as(C.c_void_p), _d(cs), _d(cf), chosen.ctypes.data_as(_ip),
                     _d(tr), cons.ctypes.data_as(_ip), ll.ctypes.data_as(_ip), inl.ctypes.data_as(C.c_void_p)))
        return dict(placed=int(out[0]), not_placed=int(out[1]), n_degenerate=int(out[2]), stages=int(out[3]), refused=int(out[4]),
                    no_consensus=int(out[5]), excluded=int(out[6]), status=status[:nch], cost_start=cs[:nch], cost_final=cf[:nch],
                    chosen=chosen[:nch], transforms=tr[:nch * g].reshape(nch, g), consensus=cons[:nch], list_len=ll[:nch], inlier=inl[:ne])

    def place_by_closures_robust(self, X, barc2, min_consensus=2):
        """place_by_closures with a consensus vote in front of the fit: every closure of a list proposes a motion, the proposal
        most closures agree with (coupled residual <= barc2) is elected and the fit runs over the agreeing closures only.
        Returns place_by_closures' dict without degenerate, plus consensus and list_len (per chain), inlier (per edge of the
        measurement table: 1 | 0 | 2 in no list), no_consensus (chains of status 5) and excluded (entries outside the inliers)."""
        return self._with_host_X(self._clr_call, self.L.cora_place_by_closures_robust, X, barc2, min_consensus)

    def debug_place_by_closures_robust_host(self, X, barc2, min_consensus=2):
        """The same on the host in the device's bracket order (no GPU needed): the device's bits."""
        return self._with_host_X(self._clr_call, self.L.cora_debug_place_by_closures_robust_host, X, barc2, min_consensus)

    def place_by_closures_robust_dev(self, x_ptr, barc2, min_consensus=2):
        """The same in place in a resident vector of d columns (a raw pointer as an int); the dict without X."""
        return self._clr_call(lambda *a: self.L.cora_place_by_closures_robust_dev(self.h, C.c_void_p(x_ptr), *a), barc2, min_consensus)

    # ---- test hook
    def debug_format_spmm_host(self, X):
        X = _f(X)
        out = self._out(X.shape[1])
        self._chk(self.L.cora_debug_format_spmm_host(self.h, _d(X), X.shape[0], X.shape[1], _d(out), self.N))
        return out
