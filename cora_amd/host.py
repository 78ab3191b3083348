"""ctypes binding of the C++ host (include/cora_host.h) -- plumbing for tests/ and bench.py."""
import ctypes as C

import numpy as np

from . import capi

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
SOLVE_DEVICE_ROUNDING = 1  # CORA_SOLVE_DEVICE_ROUNDING (include/cora_host.h): a flag of cora_problem_solve_flags


class HostError(RuntimeError):
    pass


def _lib():
    L = capi.load()
    if not getattr(L, "_host_ready", False):
        L.cora_host_last_error.restype = C.c_char_p
        L.cora_problem_destroy.restype = None
        L.cora_problem_destroy.argtypes = [C.c_void_p]
        L.cora_problem_context.restype = C.c_void_p
        L.cora_problem_context.argtypes = [C.c_void_p]
        L._host_ready = True
    return L


class Problem:
    """CORA::Problem of the C++ host."""

    def __init__(self, handle):
        self.L = _lib()
        self.h = handle

    @staticmethod
    def from_pyfg(path):
        L = _lib()
        h = C.c_void_p()
        if L.cora_problem_from_pyfg(path.encode(), C.byref(h)):
            raise HostError(L.cora_host_last_error().decode())
        return Problem(h)

    @staticmethod
    def synthetic(dim=3, n_poses=1000, n_landmarks=10, n_ranges=500, n_loops=0, seed=42,
                  precond=capi.PRECOND_JACOBI, pyfg_out=None, sigmas=None, ground_truth=False):
        """SURVEY 8(d) generator.  sigmas = (sigma_t, sigma_R, sigma_range) overrides the noise;
        ground_truth=True returns (problem, X_gt) with X_gt the N x dim truth in the explicit layout."""
        L = _lib()
        h = C.c_void_p()
        sg = np.ascontiguousarray(sigmas, dtype=np.float64) if sigmas is not None else None
        gt = np.zeros(((dim + 1) * n_poses + n_landmarks + n_ranges, dim), order="F") if ground_truth else None
        rc = L.cora_problem_synthetic_ex(dim, n_poses, n_landmarks, n_ranges, n_loops, C.c_uint64(seed), precond,
                                         sg.ctypes.data_as(_dp) if sg is not None else None,
                                         pyfg_out.encode() if pyfg_out else None,
                                         gt.ctypes.data_as(_dp) if gt is not None else None, C.byref(h))
        if rc:
            raise HostError(L.cora_host_last_error().decode())
        return (Problem(h), gt) if ground_truth else Problem(h)

    @staticmethod
    def new(dim, rank=None, implicit=False, precond=capi.PRECOND_REGULARIZED_CHOLESKY):
        """Empty CORA::Problem to be filled with add_* (the reference's programmatic API)."""
        L = _lib()
        h = C.c_void_p()
        if L.cora_problem_new(int(dim), int(rank or dim), int(bool(implicit)), int(precond), C.byref(h)):
            raise HostError(L.cora_host_last_error().decode())
        return Problem(h)

    @staticmethod
    def _m(a):
        a = np.asfortranarray(np.asarray(a, dtype=np.float64))
        return a, a.ctypes.data_as(_dp)

    def add_pose(self, sym):
        self._chk(self.L.cora_problem_add_pose(self.h, sym.encode()))

    def add_landmark(self, sym):
        self._chk(self.L.cora_problem_add_landmark(self.h, sym.encode()))

    def add_range(self, a, b, dist, cov):
        self._chk(self.L.cora_problem_add_range(self.h, a.encode(), b.encode(), C.c_double(dist), C.c_double(cov)))

    def add_rel_pose(self, a, b, R, t, cov):
        (_, pr), (_, pt), (_, pc) = self._m(R), self._m(t), self._m(cov)
        self._chk(self.L.cora_problem_add_rel_pose(self.h, a.encode(), b.encode(), pr, pt, pc))

    def add_rel_pose_landmark(self, a, b, t, cov):
        (_, pt), (_, pc) = self._m(t), self._m(cov)
        self._chk(self.L.cora_problem_add_rel_pose_landmark(self.h, a.encode(), b.encode(), pt, pc))

    def add_pose_prior(self, sym, R, t, cov):
        (_, pr), (_, pt), (_, pc) = self._m(R), self._m(t), self._m(cov)
        self._chk(self.L.cora_problem_add_pose_prior(self.h, sym.encode(), pr, pt, pc))

    def add_landmark_prior(self, sym, pos, cov):
        (_, pp), (_, pc) = self._m(pos), self._m(cov)
        self._chk(self.L.cora_problem_add_landmark_prior(self.h, sym.encode(), pp, pc))

    def close(self):
        if getattr(self, "h", None):
            self.L.cora_problem_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise HostError(self.L.cora_host_last_error().decode())

    def update(self):
        self._chk(self.L.cora_problem_update(self.h))

    def dims(self):
        d = (C.c_int64 * 8)()
        self._chk(self.L.cora_problem_dims(self.h, d))
        keys = ["d", "n", "l", "r", "N", "nnz", "rpm", "rank"]
        return dict(zip(keys, [int(x) for x in d]))

    def matrix(self, name="DataMatrix"):
        """(rows, cols, rowptr, colidx, vals) as numpy copies."""
        rows, cols, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        rp, ci, va = _ip(), _ip(), _dp()
        self._chk(self.L.cora_problem_matrix(self.h, name.encode(), C.byref(rows), C.byref(cols), C.byref(nnz),
                                             C.byref(rp), C.byref(ci), C.byref(va)))
        n = nnz.value
        rowptr = np.ctypeslib.as_array(rp, shape=(rows.value + 1,)).copy()
        colidx = np.ctypeslib.as_array(ci, shape=(max(n, 1),))[:n].copy() if n else np.zeros(0, np.int32)
        vals = np.ctypeslib.as_array(va, shape=(max(n, 1),))[:n].copy() if n else np.zeros(0)
        return rows.value, cols.value, rowptr, colidx, vals

    def certificate_matrix(self, Y):
        """Problem::get_certificate_matrix: S = Q - Lambda(Y) as a scipy CSR matrix."""
        import scipy.sparse as sp
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        rows, nnz = C.c_int64(), C.c_int64()
        rp, ci, va = _ip(), _ip(), _dp()
        self._chk(self.L.cora_problem_certificate_matrix(self.h, Y.ctypes.data_as(_dp), Y.shape[0], C.byref(rows),
                                                         C.byref(nnz), C.byref(rp), C.byref(ci), C.byref(va)))
        n = nnz.value
        return sp.csr_matrix((np.ctypeslib.as_array(va, shape=(n,)).copy(), np.ctypeslib.as_array(ci, shape=(n,)).copy(),
                              np.ctypeslib.as_array(rp, shape=(rows.value + 1,)).copy()), shape=(rows.value, rows.value))

    def scipy_matrix(self, name="DataMatrix"):
        import scipy.sparse as sp
        r, c, rp, ci, va = self.matrix(name)
        return sp.csr_matrix((va, ci, rp), shape=(r, c))

    def set_rank(self, p):
        self._chk(self.L.cora_problem_set_rank(self.h, int(p)))

    def set_preconditioner(self, kind):
        self._chk(self.L.cora_problem_set_preconditioner(self.h, int(kind)))

    def set_formulation(self, implicit):
        """Formulation::Implicit (translations marginalised) when true, Explicit otherwise."""
        self._chk(self.L.cora_problem_set_formulation(self.h, int(bool(implicit))))

    def variable_size(self):
        """Problem::getExpectedVariableSize(): N when explicit, d*n + r when implicit."""
        rows = C.c_int64()
        self._chk(self.L.cora_problem_variable_size(self.h, C.byref(rows)))
        return rows.value

    def set_device(self, dev):
        self._chk(self.L.cora_problem_set_device(self.h, int(dev)))

    def set_partition(self, rank, world, make_comm):
        """Problem::setPartition: this process (or thread) owns partition `rank` of `world` of the rows of Q.
        `make_comm(ctx)` builds the communicator (cora_amd.dist.TorchComm / ThreadComm) once the partitioned handle
        exists; it installs its callbacks on the handle itself.  Collective: every rank calls it."""
        from . import capi
        none = (capi.EXCHANGE_FN(), capi.ALLREDUCE_FN(), capi.ALLGATHER_FN())
        self._chk(self.L.cora_problem_set_partition(self.h, int(rank), int(world), none[0], none[1], none[2], None))
        dm = self.dims()
        ctx = capi.Context.from_handle(self.context_ptr(), dm["d"], dm["n"], dm["r"], dm["n"] + dm["l"])
        self._comm = make_comm(ctx)
        return self._comm

    def op(self, name, A=None, B=None, C_=None):
        dm = self.dims()
        N, p = self.variable_size(), dm["rank"]

        def ptr(x):
            if x is None:
                return None
            x = np.asfortranarray(np.asarray(x, dtype=np.float64))
            if x.shape[0] != N:
                raise HostError("expected %d rows, got %d" % (N, x.shape[0]))
            cols.append(x.shape[1])
            keep.append(x)
            return x.ctypes.data_as(_dp)

        keep, cols = [], []
        if name == "evaluateObjective":
            out = np.zeros(1)
        pa, pb, pc = ptr(A), ptr(B), ptr(C_)
        if name != "evaluateObjective":
            full = name in ("getOdomInitialization", "odometryInitialization", "rangeAidedInitialization", "rangeAidedInitializationConsensus", "multiRobotInitialization", "sightingInitialization", "sightingInitializationConsensus", "closureInitialization",
                            "closureInitializationConsensus",
                            "getTranslationExplicitSolution", "alignEstimateToOrigin")
            out = np.zeros((dm["N"] if full else N, cols[0] if cols else p), order="F")
        if len(set(cols)) > 1:
            raise HostError("operands have different column counts: %s" % cols)
        self._chk(self.L.cora_problem_op(self.h, name.encode(), cols[0] if cols else p, pa, pb, pc,
                                         out.ctypes.data_as(_dp)))
        return float(out[0]) if name == "evaluateObjective" else out

    def odometry_chains(self):
        """Problem::odometryChains: the chains getOdomInitialization composes, a list of int32 arrays of indices into the
        relative-pose measurements in the order they were added."""
        cnt = (C.c_int64 * 2)()
        self._chk(self.L.cora_problem_odometry_chains(self.h, cnt, None, None))
        ptr = np.zeros(int(cnt[0]) + 1, dtype=np.int64)
        edges = np.zeros(max(int(cnt[1]), 1), dtype=np.int32)
        self._chk(self.L.cora_problem_odometry_chains(self.h, cnt, ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      edges.ctypes.data_as(C.POINTER(C.c_int32))))
        return [edges[ptr[i]:ptr[i + 1]].copy() for i in range(int(cnt[0]))]

    def range_aided_initialization(self, seed=7, gn_steps=5, consensus_barc2=None, min_consensus=0):
        """Problem::rangeAidedInitialization: (x0, info) with info a dict solved, not_solved, n_degenerate, steps, status,
        cost_linear, cost_final (per landmark).  The start has passed checkVariablesAreValid.
        consensus_barc2: None, the plain multilateration; a threshold > 0, the multilateration with a consensus vote
        (RangeConsensus, CORA_problem.h): the fit of a landmark runs over the ranges that agree with the elected proposal, a
        landmark whose elected proposal has fewer than min_consensus (0: d + 2) votes has status 5, and info gains no_consensus,
        excluded, consensus and list_len (per landmark) and inlier (per range measurement as added: 1 | 0 | 2 in no voted list)."""
        dm = self.dims()
        nl = dm["N"] - (dm["d"] + 1) * dm["n"] - dm["r"]
        robust = consensus_barc2 is not None
        if robust and not consensus_barc2 > 0:
            raise HostError("consensus_barc2 must be positive (None: no consensus vote)")
        nr = dm["r"]
        out = np.zeros((dm["N"], dm["rank"]), order="F")
        cnt, vcnt = (C.c_int64 * 4)(), (C.c_int64 * 2)()
        status, cl, cf = np.zeros(nl + 1, dtype=np.uint8), np.zeros(nl + 1), np.zeros(nl + 1)
        cons, ll, inl = np.zeros(nl + 1, dtype=np.int32), np.zeros(nl + 1, dtype=np.int32), np.zeros(nr + 1, dtype=np.uint8)
        i32 = C.POINTER(C.c_int32)
        self._chk(self.L.cora_problem_range_aided_initialization_consensus(
            self.h, C.c_uint64(seed), int(gn_steps), C.c_double(consensus_barc2 if robust else 0.0), int(min_consensus),
            out.ctypes.data_as(_dp), cnt, status.ctypes.data_as(C.c_void_p), cl.ctypes.data_as(_dp), cf.ctypes.data_as(_dp), vcnt,
            cons.ctypes.data_as(i32), ll.ctypes.data_as(i32), inl.ctypes.data_as(C.c_void_p)))
        extra = dict(no_consensus=int(vcnt[0]), excluded=int(vcnt[1]), consensus=cons[:nl], list_len=ll[:nl], inlier=inl[:nr]) if robust else {}
        return out, dict(**extra, solved=int(cnt[0]), not_solved=int(cnt[1]), n_degenerate=int(cnt[2]), steps=int(cnt[3]),
                         status=status[:nl], cost_linear=cl[:nl], cost_final=cf[:nl])

    def multi_robot_initialization(self, seed=7, gn_steps=5, min_ranges=0, order=None, consensus_barc2=None, min_consensus=0):
        """Problem::multiRobotInitialization: (x0, info) with info a dict placed, not_placed, steps, stages, status, cost_start,
        cost_linear, cost_final, transforms (per chain of odometry_chains()), landmarks (the dict of
        range_aided_initialization without the costs).  min_ranges 0: the default.  The start has passed checkVariablesAreValid.
        order: None, the call without the argument (ChainOrder::Greedy); "greedy" | "levels", the ChainOrder given, and info
        gains levels.
        consensus_barc2: None, the plain placement; a threshold > 0, the placement with a consensus vote (ChainRangeConsensus,
        CORA_problem.h) under the order given (None: greedy): the fit of a chain runs over the ranges that agree with the elected
        proposal, a chain whose elected proposal has fewer than min_consensus (0: 2 m, m = 8 / 17) votes has status 5, and info
        gains levels, no_consensus, excluded, consensus and list_len (per chain) and inlier (per range measurement as added:
        1 | 0 | 2 in no stage list)."""
        if order not in (None, "greedy", "levels"):
            raise ValueError("order must be None, 'greedy' or 'levels'")
        robust = consensus_barc2 is not None
        if robust and not consensus_barc2 > 0:
            raise HostError("consensus_barc2 must be positive (None: no consensus vote)")
        dm = self.dims()
        d = dm["d"]
        nl = dm["N"] - (d + 1) * dm["n"] - dm["r"]
        nch = len(self.odometry_chains())
        out = np.zeros((dm["N"], dm["rank"]), order="F")
        cnt, lcnt = (C.c_int64 * 5)(), (C.c_int64 * 4)()
        status, lstatus = np.zeros(nch + 1, dtype=np.uint8), np.zeros(nl + 1, dtype=np.uint8)
        cs, cl, cf, tr = np.zeros(nch + 1), np.zeros(nch + 1), np.zeros(nch + 1), np.zeros(nch * (d * d + d) + 1)
        tail = (out.ctypes.data_as(_dp), cnt, status.ctypes.data_as(C.c_void_p), cs.ctypes.data_as(_dp), cl.ctypes.data_as(_dp),
                cf.ctypes.data_as(_dp), tr.ctypes.data_as(_dp), lcnt, lstatus.ctypes.data_as(C.c_void_p))
        if robust:
            nr, i32 = dm["r"], C.POINTER(C.c_int32)
            vcnt = (C.c_int64 * 2)()
            cons, ll, inl = np.zeros(nch + 1, dtype=np.int32), np.zeros(nch + 1, dtype=np.int32), np.zeros(nr + 1, dtype=np.uint8)
            self._chk(self.L.cora_problem_multi_robot_initialization_consensus(
                self.h, C.c_uint64(seed), int(gn_steps), int(min_ranges), 1 if order == "levels" else 0, C.c_double(consensus_barc2),
                int(min_consensus), *tail, vcnt, cons.ctypes.data_as(i32), ll.ctypes.data_as(i32), inl.ctypes.data_as(C.c_void_p)))
            order = order or "greedy"
        elif order is None:
            self._chk(self.L.cora_problem_multi_robot_initialization(self.h, C.c_uint64(seed), int(gn_steps), int(min_ranges), *tail))
        else:
            self._chk(self.L.cora_problem_multi_robot_initialization_order(self.h, C.c_uint64(seed), int(gn_steps), int(min_ranges),
                                                                           1 if order == "levels" else 0, *tail))
        extra = {} if order is None else dict(levels=int(cnt[4]))
        if robust:
            extra.update(no_consensus=int(vcnt[0]), excluded=int(vcnt[1]), consensus=cons[:nch], list_len=ll[:nch], inlier=inl[:nr])
        return out, dict(**extra, placed=int(cnt[0]), not_placed=int(cnt[1]), steps=int(cnt[2]), stages=int(cnt[3]), status=status[:nch],
                         cost_start=cs[:nch], cost_linear=cl[:nch], cost_final=cf[:nch], transforms=tr[:-1].reshape(nch, d * d + d),
                         landmarks=dict(solved=int(lcnt[0]), not_solved=int(lcnt[1]), n_degenerate=int(lcnt[2]), steps=int(lcnt[3]),
                                        status=lstatus[:nl]))

    def sighting_initialization(self, seed=7, gn_steps=5, min_ranges=0, min_sightings=0, consensus_barc2=None, min_chain_consensus=0,
                                min_landmark_consensus=1):
        """Problem::sightingInitialization: (x0, info) with info a dict fixed, placed, not_placed, landmarks_placed,
        landmarks_not_placed, stages, status, cost_start, cost_final, chosen, transforms (per chain of odometry_chains()),
        landmark_status, landmark_cost (per landmark) of the sighting step; chains (placed, not_placed, steps, stages, status
        of the range placement that followed) and landmarks (the dict of range_aided_initialization without the costs).
        0: the defaults.  The start has passed checkVariablesAreValid.
        consensus_barc2: None, the plain sighting step; a threshold > 0, the sighting step with a consensus vote
        (SightingConsensus, CORA_problem.h): every fit runs over the sightings that agree with the elected proposal, a chain
        below min_chain_consensus (0: d + 1) or a landmark below min_landmark_consensus has status 5, and info gains
        chains_no_consensus, landmarks_no_consensus, chain_excluded, landmark_excluded, chain_consensus, chain_list_len (per chain),
        landmark_consensus, landmark_list_len (per landmark), inlier_chain and inlier_landmark (per edge of the measurement table,
        relative poses first: 1 | 0 | 2 in no list)."""
        dm = self.dims()
        d = dm["d"]
        nl = dm["N"] - (d + 1) * dm["n"] - dm["r"]
        nch = len(self.odometry_chains())
        robust = consensus_barc2 is not None
        if robust and not consensus_barc2 > 0:
            raise HostError("consensus_barc2 must be positive (None: no consensus vote)")
        mcnt, vcnt = (C.c_int64 * 5)(), (C.c_int64 * 4)()
        self._chk(self.L.cora_problem_measurement_counts(self.h, mcnt))
        ne = int(sum(mcnt[:4]))
        i32 = C.POINTER(C.c_int32)
        cc, cl, lcn, ll = (np.zeros(k + 1, dtype=np.int32) for k in (nch, nch, nl, nl))
        ic, il = np.zeros(ne + 1, dtype=np.uint8), np.zeros(ne + 1, dtype=np.uint8)
        out = np.zeros((dm["N"], dm["rank"]), order="F")
        cnt, ccnt, lcnt = (C.c_int64 * 6)(), (C.c_int64 * 4)(), (C.c_int64 * 4)()
        status, cstatus, chosen = np.zeros(nch + 1, dtype=np.uint8), np.zeros(nch + 1, dtype=np.uint8), np.zeros(nch + 1, dtype=np.int32)
        ls, rls, lc = np.zeros(nl + 1, dtype=np.uint8), np.zeros(nl + 1, dtype=np.uint8), np.zeros(nl + 1)
        cs, cf, tr = np.zeros(nch + 1), np.zeros(nch + 1), np.zeros(nch * (d * d + d) + 1)
        self._chk(self.L.cora_problem_sighting_initialization_consensus(
            self.h, C.c_uint64(seed), int(gn_steps), int(min_ranges), int(min_sightings), C.c_double(consensus_barc2 if robust else 0.0),
            int(min_chain_consensus), int(min_landmark_consensus), out.ctypes.data_as(_dp), cnt,
            status.ctypes.data_as(C.c_void_p), cs.ctypes.data_as(_dp), cf.ctypes.data_as(_dp), chosen.ctypes.data_as(i32),
            tr.ctypes.data_as(_dp), ls.ctypes.data_as(C.c_void_p), lc.ctypes.data_as(_dp), vcnt, cc.ctypes.data_as(i32), cl.ctypes.data_as(i32),
            lcn.ctypes.data_as(i32), ll.ctypes.data_as(i32), ic.ctypes.data_as(C.c_void_p), il.ctypes.data_as(C.c_void_p), ccnt,
            cstatus.ctypes.data_as(C.c_void_p), lcnt, rls.ctypes.data_as(C.c_void_p)))
        extra = dict(chains_no_consensus=int(vcnt[0]), landmarks_no_consensus=int(vcnt[1]), chain_excluded=int(vcnt[2]),
                     landmark_excluded=int(vcnt[3]), chain_consensus=cc[:nch], chain_list_len=cl[:nch], landmark_consensus=lcn[:nl],
                     landmark_list_len=ll[:nl], inlier_chain=ic[:ne], inlier_landmark=il[:ne]) if robust else {}
        return out, dict(**extra, fixed=int(cnt[0]), placed=int(cnt[1]), not_placed=int(cnt[2]), landmarks_placed=int(cnt[3]),
                         landmarks_not_placed=int(cnt[4]), stages=int(cnt[5]), status=status[:nch], cost_start=cs[:nch], cost_final=cf[:nch],
                         chosen=chosen[:nch], transforms=tr[:-1].reshape(nch, d * d + d), landmark_status=ls[:nl], landmark_cost=lc[:nl],
                         chains=dict(placed=int(ccnt[0]), not_placed=int(ccnt[1]), steps=int(ccnt[2]), stages=int(ccnt[3]), status=cstatus[:nch]),
                         landmarks=dict(solved=int(lcnt[0]), not_solved=int(lcnt[1]), n_degenerate=int(lcnt[2]), steps=int(lcnt[3]),
                                        status=rls[:nl]))

    def closure_initialization(self, seed=7, gn_steps=5, min_ranges=0, min_sightings=0, min_closures=0, consensus_barc2=None, min_consensus=2):
        """Problem::closureInitialization: (x0, info) with info a dict fixed, placed, not_placed, refused, stages,
        closures_used, edges_skipped, status, cost_start, cost_final, chosen, transforms (per chain of odometry_chains()) of
        the closure step; sightings (fixed, placed, not_placed, landmarks_placed, landmarks_not_placed, stages, status,
        landmark_status of the sighting step that followed), chains and landmarks as sighting_initialization has them.
        0: the defaults.  The start has passed checkVariablesAreValid.
        consensus_barc2: None, the plain closure step; a threshold > 0, the closure step with a consensus vote
        (ClosureConsensus, CORA_problem.h): the fit of a chain runs over the closures that agree with the elected one, a chain
        whose elected closure has fewer than min_consensus votes has status 5, and info gains no_consensus, excluded, consensus
        and list_len (per chain) and inlier (per edge of the measurement table, relative poses first: 1 | 0 | 2 in no list)."""
        dm = self.dims()
        d = dm["d"]
        nl = dm["N"] - (d + 1) * dm["n"] - dm["r"]
        nch = len(self.odometry_chains())
        robust = consensus_barc2 is not None
        if robust and not consensus_barc2 > 0:
            raise HostError("consensus_barc2 must be positive (None: no consensus vote)")
        mcnt, vcnt = (C.c_int64 * 5)(), (C.c_int64 * 2)()
        self._chk(self.L.cora_problem_measurement_counts(self.h, mcnt))
        ne = int(sum(mcnt[:4]))
        cons, ll, inl = np.zeros(nch + 1, dtype=np.int32), np.zeros(nch + 1, dtype=np.int32), np.zeros(ne + 1, dtype=np.uint8)
        i32 = C.POINTER(C.c_int32)
        out = np.zeros((dm["N"], dm["rank"]), order="F")
        cnt, scnt, ccnt, lcnt = (C.c_int64 * 7)(), (C.c_int64 * 6)(), (C.c_int64 * 4)(), (C.c_int64 * 4)()
        status, sstatus, cstatus = (np.zeros(nch + 1, dtype=np.uint8) for _ in range(3))
        chosen = np.zeros(nch + 1, dtype=np.int32)
        ls, rls = np.zeros(nl + 1, dtype=np.uint8), np.zeros(nl + 1, dtype=np.uint8)
        cs, cf, tr = np.zeros(nch + 1), np.zeros(nch + 1), np.zeros(nch * (d * d + d) + 1)
        self._chk(self.L.cora_problem_closure_initialization_consensus(
            self.h, C.c_uint64(seed), int(gn_steps), int(min_ranges), int(min_sightings), int(min_closures),
            C.c_double(consensus_barc2 if robust else 0.0), int(min_consensus), out.ctypes.data_as(_dp), cnt,
            status.ctypes.data_as(C.c_void_p), cs.ctypes.data_as(_dp), cf.ctypes.data_as(_dp), chosen.ctypes.data_as(i32),
            tr.ctypes.data_as(_dp), vcnt, cons.ctypes.data_as(i32), ll.ctypes.data_as(i32), inl.ctypes.data_as(C.c_void_p), scnt,
            sstatus.ctypes.data_as(C.c_void_p), ls.ctypes.data_as(C.c_void_p), ccnt, cstatus.ctypes.data_as(C.c_void_p), lcnt,
            rls.ctypes.data_as(C.c_void_p)))
        extra = dict(no_consensus=int(vcnt[0]), excluded=int(vcnt[1]), consensus=cons[:nch], list_len=ll[:nch], inlier=inl[:ne]) if robust else {}
        return out, dict(**extra, fixed=int(cnt[0]), placed=int(cnt[1]), not_placed=int(cnt[2]), refused=int(cnt[3]), stages=int(cnt[4]),
                         closures_used=int(cnt[5]), edges_skipped=int(cnt[6]), status=status[:nch], cost_start=cs[:nch], cost_final=cf[:nch],
                         chosen=chosen[:nch], transforms=tr[:-1].reshape(nch, d * d + d),
                         sightings=dict(fixed=int(scnt[0]), placed=int(scnt[1]), not_placed=int(scnt[2]), landmarks_placed=int(scnt[3]),
                                        landmarks_not_placed=int(scnt[4]), stages=int(scnt[5]), status=sstatus[:nch], landmark_status=ls[:nl]),
                         chains=dict(placed=int(ccnt[0]), not_placed=int(ccnt[1]), steps=int(ccnt[2]), stages=int(ccnt[3]), status=cstatus[:nch]),
                         landmarks=dict(solved=int(lcnt[0]), not_solved=int(lcnt[1]), n_degenerate=int(lcnt[2]), steps=int(lcnt[3]),
                                        status=rls[:nl]))

    def lambda_blocks(self, Y):
        dm = self.dims()
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        st = np.zeros((dm["d"], max(dm["d"] * dm["n"], 1)), order="F")
        ob = np.zeros(max(dm["r"], 1))
        self._chk(self.L.cora_problem_lambda_blocks(self.h, Y.ctypes.data_as(_dp), st.ctypes.data_as(_dp),
                                                    ob.ctypes.data_as(_dp)))
        return st[:, :dm["d"] * dm["n"]], ob[:dm["r"]]

    def measurement_residuals(self, Y):
        """Problem::measurementResiduals: dict of numpy arrays rel_pose_rot, rel_pose_trans, pose_prior_rot,
        pose_prior_trans, pose_landmark, landmark_prior, range (each in the order the measurements were added) and the
        scalars rot_sum, trans_sum, range_sum; 1/2 of the three sums is evaluateObjective(Y).  Y: variable_size() rows,
        1..24 columns."""
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        if Y.ndim != 2 or Y.shape[0] != self.variable_size():
            raise HostError("expected %d rows, got shape %s" % (self.variable_size(), Y.shape))
        cnt = (C.c_int64 * 5)()
        self._chk(self.L.cora_problem_measurement_counts(self.h, cnt))
        names = ["rel_pose_rot", "rel_pose_trans", "pose_prior_rot", "pose_prior_trans", "pose_landmark",
                 "landmark_prior", "range"]
        sizes = [cnt[0], cnt[0], cnt[1], cnt[1], cnt[2], cnt[3], cnt[4]]
        out = {k: np.zeros(max(int(n), 1)) for k, n in zip(names, sizes)}
        sums = np.zeros(3)
        self._chk(self.L.cora_problem_measurement_residuals(self.h, Y.ctypes.data_as(_dp), int(Y.shape[1]),
                                                            *[out[k].ctypes.data_as(_dp) for k in names],
                                                            sums.ctypes.data_as(_dp)))
        res = {k: out[k][:int(n)] for k, n in zip(names, sizes)}
        res.update(rot_sum=float(sums[0]), trans_sum=float(sums[1]), range_sum=float(sums[2]))
        return res

    WEIGHT_KINDS = ("rel_pose_rot", "rel_pose_trans", "pose_prior_rot", "pose_prior_trans", "pose_landmark",
                    "landmark_prior", "range")

    def set_measurement_weights(self, weights):
        """Problem::setMeasurementWeights: dict kind -> array of weights (kinds as in measurement_residuals; a missing or
        empty kind means all ones).  Re-assembles Q; an existing device handle is updated in place (context_ptr() does
        not change).  measurement_residuals() then returns weighted residuals."""
        unknown = set(weights) - set(self.WEIGHT_KINDS)
        if unknown:
            raise HostError("unknown measurement kinds: %s" % sorted(unknown))
        arrs = [np.ascontiguousarray(weights.get(k, ()), dtype=np.float64).reshape(-1) for k in self.WEIGHT_KINDS]
        ptrs = (_dp * 7)(*[a.ctypes.data_as(_dp) if a.size else None for a in arrs])
        lens = (C.c_int64 * 7)(*[a.size for a in arrs])
        self._chk(self.L.cora_problem_set_measurement_weights(self.h, ptrs, lens))

    def reweight(self, weights):
        """Problem::reweight: set_measurement_weights with Q(w) assembled on the device through the handle's term map
        (falls back to set_measurement_weights without a live handle).  The two agree to rounding, not to the bit."""
        unknown = set(weights) - set(self.WEIGHT_KINDS)
        if unknown:
            raise HostError("unknown measurement kinds: %s" % sorted(unknown))
        arrs = [np.ascontiguousarray(weights.get(k, ()), dtype=np.float64).reshape(-1) for k in self.WEIGHT_KINDS]
        ptrs = (_dp * 7)(*[a.ctypes.data_as(_dp) if a.size else None for a in arrs])
        lens = (C.c_int64 * 7)(*[a.size for a in arrs])
        self._chk(self.L.cora_problem_reweight(self.h, ptrs, lens))

    def get_measurement_weights(self):
        cnt = (C.c_int64 * 5)()
        self._chk(self.L.cora_problem_measurement_counts(self.h, cnt))
        sizes = [cnt[0], cnt[0], cnt[1], cnt[1], cnt[2], cnt[3], cnt[4]]
        arrs = [np.zeros(max(int(n), 1)) for n in sizes]
        ptrs = (_dp * 7)(*[a.ctypes.data_as(_dp) for a in arrs])
        self._chk(self.L.cora_problem_get_measurement_weights(self.h, ptrs))
        return {k: a[:int(n)] for k, a, n in zip(self.WEIGHT_KINDS, arrs, sizes)}

    GNC_COSTS = {"none": 0, "tls": 1, "gm": 2}

    def _seven(self, arrays, what):
        unknown = set(arrays) - set(self.WEIGHT_KINDS)
        if unknown:
            raise HostError("unknown measurement kinds in %s: %s" % (what, sorted(unknown)))
        arrs = [np.ascontiguousarray(arrays.get(k, ()), dtype=np.float64).reshape(-1) for k in self.WEIGHT_KINDS]
        ptrs = (_dp * 7)(*[a.ctypes.data_as(_dp) if a.size else None for a in arrs])
        lens = (C.c_int64 * 7)(*[a.size for a in arrs])
        return arrs, ptrs, lens

    def gnc_weights(self, Y, thresholds, cost, mu=1.0, couple_edges=True):
        """Problem::gncWeights: one weight step of a robust-cost loop on the device at Y.  thresholds: dict kind -> array
        of barc2 (kinds as in reweight; a missing kind is trusted), cost 'none' | 'tls' | 'gm'.  The residuals behind the
        weights are UNWEIGHTED whatever the current weights.  Returns (weights, stats): weights a dict for reweight(),
        stats {'rot' | 'trans' | 'range': dict sum_wr2, max_rho, n_mid, n_out}.  Needs a live handle (HostError)."""
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        if Y.ndim != 2 or Y.shape[0] != self.variable_size():
            raise HostError("expected %d rows, got shape %s" % (self.variable_size(), Y.shape))
        keep, ptrs, lens = self._seven(thresholds, "thresholds")
        cnt = (C.c_int64 * 5)()
        self._chk(self.L.cora_problem_measurement_counts(self.h, cnt))
        sizes = [cnt[0], cnt[0], cnt[1], cnt[1], cnt[2], cnt[3], cnt[4]]
        arrs = [np.zeros(max(int(n), 1)) for n in sizes]
        out = (_dp * 7)(*[a.ctypes.data_as(_dp) for a in arrs])
        st = np.zeros(12)
        self._chk(self.L.cora_problem_gnc_weights(self.h, Y.ctypes.data_as(_dp), int(Y.shape[1]), ptrs, lens,
                                                  int(self.GNC_COSTS[cost]), C.c_double(mu), int(bool(couple_edges)), out,
                                                  st.ctypes.data_as(_dp)))
        names = ("sum_wr2", "max_rho", "n_mid", "n_out")
        stats = {seg: dict(zip(names, st[4 * i:4 * i + 4])) for i, seg in enumerate(("rot", "trans", "range"))}
        return {k: a[:int(n)] for k, a, n in zip(self.WEIGHT_KINDS, arrs, sizes)}, stats

    def ground_truth(self, path):
        """parsePyfgGroundTruth: the VERTEX_* values of a PyFG file as a point of this problem (N x d: rotation rows
        R_i^T, unit range rows, positions), the reference of compare()."""
        dm = self.dims()
        X = np.zeros((dm["N"], dm["d"]), order="F")
        self._chk(self.L.cora_problem_ground_truth(self.h, str(path).encode(), X.ctypes.data_as(_dp)))
        return X

    def compare(self, Y, Ref, select=None, proper=True, aligned=False):
        """Problem::compareToReference: errors of Y (variable_size() x k) against Ref (N x kr, kr <= k) after the
        orthogonal alignment on the selected poses' positions (include/cora_hip.h, cora_compare_dev).  select: None
        (every pose and landmark but the origin pose of a problem with priors) or n + l flags; proper needs k == kr.
        Returns dict m, n_landmarks, pose_trans_err, pose_rot_err, landmark_err, sum_et2, max_et, sum_er2, max_er,
        sum_el2, max_el, trans_rmse, rot_rmse, landmark_rmse, sigma, xbar, gbar, A (k x kr), and aligned (N x kr) when
        asked for."""
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        Ref = np.asfortranarray(np.asarray(Ref, dtype=np.float64))
        dm = self.dims()
        if Y.ndim != 2 or Y.shape[0] != self.variable_size():
            raise HostError("expected %d rows, got shape %s" % (self.variable_size(), Y.shape))
        if Ref.ndim != 2 or Ref.shape[0] != dm["N"]:
            raise HostError("the reference needs %d rows, got shape %s" % (dm["N"], Ref.shape))
        k, kr, n, nl = Y.shape[1], Ref.shape[1], dm["n"], dm["l"]
        sel = None
        if select is not None:
            sel = np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8)
            if sel.shape != (n + nl,):
                raise HostError("select needs %d flags" % (n + nl))
        et, er, el = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros(max(nl, 1))
        al = np.zeros((dm["N"], kr), order="F") if aligned else None
        out = np.zeros(8 + kr + k + kr + k * kr)
        self._chk(self.L.cora_problem_compare(self.h, Y.ctypes.data_as(_dp), int(k), Ref.ctypes.data_as(_dp), int(kr),
                                              sel.ctypes.data_as(C.c_void_p) if sel is not None else None, int(bool(proper)),
                                              et.ctypes.data_as(_dp), er.ctypes.data_as(_dp), el.ctypes.data_as(_dp),
                                              al.ctypes.data_as(_dp) if aligned else None, out.ctypes.data_as(_dp)))
        o = 8 + kr
        res = dict(zip(("m", "sum_et2", "max_et", "sum_er2", "max_er", "n_landmarks", "sum_el2", "max_el"), out[:8]))
        res.update(pose_trans_err=et[:n], pose_rot_err=er[:n], landmark_err=el[:nl], sigma=out[8:o], xbar=out[o:o + k],
                   gbar=out[o + k:o + k + kr], A=out[o + k + kr:].reshape(kr, k).T.copy(),
                   trans_rmse=float(np.sqrt(out[1] / max(out[0], 1))), rot_rmse=float(np.sqrt(out[3] / max(out[0], 1))),
                   landmark_rmse=float(np.sqrt(out[6] / max(out[5], 1))))
        if aligned:
            res["aligned"] = al
        return res

    def _pose_pairs(self, step, Ref, L):
        n = self.dims()["n"]
        pairs, path, m = np.zeros((max(n, 1), 2), dtype=np.int32), np.zeros(max(n, 1)), C.c_int64(0)
        refp, cols = None, 0
        if Ref is not None:
            Ref = np.asfortranarray(np.asarray(Ref, dtype=np.float64))
            if Ref.ndim != 2 or Ref.shape[0] != self.dims()["N"]:
                raise HostError("the reference needs %d rows, got shape %s" % (self.dims()["N"], Ref.shape))
            refp, cols = Ref.ctypes.data_as(_dp), Ref.shape[1]
        self._chk(self.L.cora_problem_pose_pairs(self.h, int(step), refp, int(cols), C.c_double(L),
                                                 pairs.ctypes.data_as(C.POINTER(C.c_int32)), path.ctypes.data_as(_dp), C.byref(m)))
        return pairs[:m.value].copy(), path[:m.value].copy()

    def pose_pairs_by_step(self, step):
        """Problem::posePairsByStep: (pairs [m, 2] of pose indices, path_length [m] = step) -- (c[a], c[a + step]) for
        every robot's chain c."""
        return self._pose_pairs(step, None, 0.0)

    def pose_pairs_by_distance(self, Ref, L):
        """Problem::posePairsByDistance: for every start the first later pose of the same robot at least L along Ref's
        positions; (pairs [m, 2], path_length [m])."""
        return self._pose_pairs(0, Ref, L)

    def relative_error(self, Y, Ref, pairs, path_length=None):
        """Problem::relativeError: relative pose errors of Y (variable_size() x k) against Ref (N x kr; k and kr
        independent) over the pairs (include/cora_hip.h, cora_rpe_dev).  pairs: [m, 2] or the tuple a pair builder
        returned.  Returns dict m, trans_err, rot_err, sum_et2, max_et, sum_er2, max_er, argmax_et, trans_rmse, rot_rmse,
        mean_trans_drift, mean_rot_drift (means of error / path_length over pairs with a positive length)."""
        if isinstance(pairs, tuple):
            pairs, path_length = pairs
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        m = len(pairs)
        path = np.ones(m) if path_length is None else np.ascontiguousarray(path_length, dtype=np.float64).reshape(-1)
        if len(path) != m:
            raise HostError("path_length needs one value per pair")
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        Ref = np.asfortranarray(np.asarray(Ref, dtype=np.float64))
        if Y.ndim != 2 or Y.shape[0] != self.variable_size():
            raise HostError("expected %d rows, got shape %s" % (self.variable_size(), Y.shape))
        if Ref.ndim != 2 or Ref.shape[0] != self.dims()["N"]:
            raise HostError("the reference needs %d rows, got shape %s" % (self.dims()["N"], Ref.shape))
        et, er, out = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(8)
        self._chk(self.L.cora_problem_relative_error(self.h, Y.ctypes.data_as(_dp), int(Y.shape[1]), Ref.ctypes.data_as(_dp),
                                                     int(Ref.shape[1]), C.c_int64(m),
                                                     pairs.ctypes.data_as(C.POINTER(C.c_int32)) if m else None,
                                                     path.ctypes.data_as(_dp) if m else None, et.ctypes.data_as(_dp),
                                                     er.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        res = dict(zip(("m", "sum_et2", "max_et", "sum_er2", "max_er", "argmax_et", "mean_trans_drift", "mean_rot_drift"), out))
        res.update(trans_err=et[:m], rot_err=er[:m], trans_rmse=float(np.sqrt(out[1] / max(out[0], 1))),
                   rot_rmse=float(np.sqrt(out[3] / max(out[0], 1))))
        return res

    def solve_robust(self, x0, thresholds, cost="tls", couple_edges=True, mu_factor=1.4, max_outer=100, max_rank=10,
                     verbose=False):
        """solveRobustCORA: graduated non-convexity over solve().  Returns solve()'s dict (of the last solve) plus
        outer_iterations, converged, mu_history, sum_wr2_history and weights (the final ones: the problem stays weighted
        with them)."""
        dm = self.dims()
        x0 = np.asfortranarray(np.asarray(x0, dtype=np.float64))
        keep, ptrs, lens = self._seven(thresholds, "thresholds")
        out = np.zeros((self.variable_size(), dm["d"]), order="F")
        st, rb = np.zeros(11), np.zeros(3)
        mu_h, sum_h = np.zeros(max_outer + 1), np.zeros(max_outer + 1)
        self._chk(self.L.cora_problem_solve_robust(self.h, x0.ctypes.data_as(_dp), int(max_rank), int(verbose), ptrs, lens,
                                                   int(self.GNC_COSTS[cost]), int(bool(couple_edges)), C.c_double(mu_factor),
                                                   int(max_outer), out.ctypes.data_as(_dp), st.ctypes.data_as(_dp),
                                                   rb.ctypes.data_as(_dp), mu_h.ctypes.data_as(_dp), sum_h.ctypes.data_as(_dp)))
        nh = int(rb[2])
        return dict(x=out, f=st[0], grad_norm=st[1], certified=bool(st[2]), eta=st[3], theta=st[4],
                    final_rank=int(st[5]), levels=int(st[6]), hvps=int(st[7]), seconds=st[8],
                    relaxation_certified=bool(st[9]), relaxation_rank=int(st[10]), outer_iterations=int(rb[0]),
                    converged=bool(rb[1]), mu_history=mu_h[:nh].copy(), sum_wr2_history=sum_h[:nh].copy(),
                    weights=self.get_measurement_weights())

    def tnt(self, x0, max_iterations=0, max_inner=0, grad_tol=0, pgrad_tol=0, max_seconds=0, verbose=False,
            host_stpcg=False):
        dm = self.dims()
        x0 = np.asfortranarray(np.asarray(x0, dtype=np.float64))
        assert x0.shape == (self.variable_size(), dm["rank"])
        opts = np.array([max_iterations, max_inner, grad_tol, pgrad_tol, max_seconds, float(verbose),
                         float(host_stpcg)])
        out = np.zeros_like(x0, order="F")
        st = np.zeros(7)
        self._chk(self.L.cora_problem_tnt(self.h, x0.ctypes.data_as(_dp), opts.ctypes.data_as(_dp),
                                          out.ctypes.data_as(_dp), st.ctypes.data_as(_dp)))
        return dict(x=out, f=st[0], grad_norm=st[1], pgrad_norm=st[2], iterations=int(st[3]), hvps=int(st[4]),
                    status=int(st[5]), seconds=st[6])

    def tnt_step(self, x, Delta, host_stpcg=False):
        """One outer TNT iteration from (x, Delta): cora_problem_tnt_step."""
        dm = self.dims()
        x = np.asfortranarray(np.asarray(x, dtype=np.float64))
        assert x.shape == (self.variable_size(), dm["rank"])
        out = np.zeros_like(x, order="F")
        st = np.zeros(8)
        self._chk(self.L.cora_problem_tnt_step(self.h, x.ctypes.data_as(_dp), C.c_double(Delta), int(host_stpcg),
                                               out.ctypes.data_as(_dp), st.ctypes.data_as(_dp)))
        return dict(x=out, f=st[0], Delta=st[1], inner=int(st[2]), rho=st[3], accepted=bool(st[4]), h_norm=st[5],
                    h_M_norm=st[6], status=int(st[7]))

    def certify(self, Y, eta, nx=10):
        dm = self.dims()
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        out = np.zeros(3)
        x = np.zeros(dm["N"])
        self._chk(self.L.cora_problem_certify(self.h, Y.ctypes.data_as(_dp), C.c_double(eta), int(nx),
                                              out.ctypes.data_as(_dp), x.ctypes.data_as(_dp)))
        return dict(is_certified=bool(out[0]), theta=out[1], iters=int(out[2]), x=x)

    def certify_resident(self, Y, eta, nx=10, first=True):
        """The certification of solveCORA's own loop: the first level starts the eigensolver from the point, later levels
        from the block the previous call left on the device (cora_problem_certify_resident)."""
        dm = self.dims()
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        out = np.zeros(3)
        x = np.zeros(dm["N"])
        self._chk(self.L.cora_problem_certify_resident(self.h, Y.ctypes.data_as(_dp), C.c_double(eta), int(nx), int(bool(first)),
                                                       out.ctypes.data_as(_dp), x.ctypes.data_as(_dp)))
        return dict(is_certified=bool(out[0]), theta=out[1], iters=int(out[2]), x=x)

    def saddle_escape(self, Y, theta, v, grad_tol=1e-4, pgrad_tol=1e-4):
        """saddleEscape (src/CORA.cpp:245-350) from the saddle point Y (N x (rank - 1); set_rank(rank) first, as
        solveCORA increments the rank before the call) along the certificate's direction v."""
        dm = self.dims()
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        v = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
        assert Y.shape == (self.variable_size(), dm["rank"] - 1) and v.shape == (self.variable_size(),)
        out = np.zeros((self.variable_size(), dm["rank"]), order="F")
        info = np.zeros(3)
        self._chk(self.L.cora_problem_saddle_escape(self.h, Y.ctypes.data_as(_dp), C.c_double(theta), v.ctypes.data_as(_dp),
                                                    C.c_double(grad_tol), C.c_double(pgrad_tol), out.ctypes.data_as(_dp),
                                                    info.ctypes.data_as(_dp)))
        return dict(x=out, f_saddle=info[0], f=info[1], moved=bool(info[2]))

    def project_solution(self, Y):
        """projectSolution (src/CORA.cpp:352-441): N x rank -> N x d."""
        dm = self.dims()
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        assert Y.shape == (self.variable_size(), dm["rank"])
        out = np.zeros((self.variable_size(), dm["d"]), order="F")
        self._chk(self.L.cora_problem_project_solution(self.h, Y.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        return out

    def round_solution(self, Y, info=False):
        """Problem::roundSolution: projectSolution on the device (include/cora_hip.h, cora_round) -- variable_size() x k,
        d <= k <= 24, to variable_size() x d.  info=True: (X, dict count, flipped, sigma)."""
        dm = self.dims()
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        if Y.ndim != 2 or Y.shape[0] != self.variable_size():
            raise HostError("expected %d rows, got shape %s" % (self.variable_size(), Y.shape))
        k = Y.shape[1]
        out = np.zeros((self.variable_size(), dm["d"]), order="F")
        st = np.zeros(2 + max(k, 1))
        self._chk(self.L.cora_problem_round_solution(self.h, Y.ctypes.data_as(_dp), int(k), out.ctypes.data_as(_dp),
                                                     st.ctypes.data_as(_dp)))
        if not info:
            return out
        return out, dict(count=int(st[0]), flipped=bool(st[1]), sigma=st[2:2 + k].copy())

    def certify_chain(self, Y, eta, nx=10, resident=False):
        """Two certifications in a row, the second started from the first one's Ritz block (host hand-over or resident)."""
        dm = self.dims()
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        out = np.zeros(6)
        x = np.zeros(dm["N"])
        self._chk(self.L.cora_problem_certify_chain(self.h, Y.ctypes.data_as(_dp), C.c_double(eta), int(nx), int(bool(resident)),
                                                    out.ctypes.data_as(_dp), x.ctypes.data_as(_dp)))
        return dict(first=dict(is_certified=bool(out[0]), theta=out[1], iters=int(out[2])),
                    second=dict(is_certified=bool(out[3]), theta=out[4], iters=int(out[5]), x=x))

    def set_verification_lab(self, seed=True, ildl=True):
        """Test switches of certify()'s eigensolver stage (step 3 of fast_verification)."""
        self._chk(self.L.cora_problem_set_verification_lab(self.h, int(bool(seed)), int(bool(ildl))))

    def certification_reached_step3(self):
        v = C.c_int(0)
        self._chk(self.L.cora_problem_certification_reached_step3(self.h, C.byref(v)))
        return bool(v.value)

    def solve(self, x0, max_rank=10, verbose=False, max_seconds=0, max_iterations=0, device_rounding=False):
        """solveCORA.  device_rounding: round the certified point with round_solution (on the device) in place of
        project_solution (CoraSolveInfo::device_rounding)."""
        dm = self.dims()
        x0 = np.asfortranarray(np.asarray(x0, dtype=np.float64))
        opts = np.array([max_iterations, 0, 0, 0, max_seconds, 0.0])
        out = np.zeros((self.variable_size(), dm["d"]), order="F")
        st = np.zeros(11)
        if device_rounding:
            self._chk(self.L.cora_problem_solve_flags(self.h, x0.ctypes.data_as(_dp), int(max_rank), int(verbose),
                                                      opts.ctypes.data_as(_dp), SOLVE_DEVICE_ROUNDING, out.ctypes.data_as(_dp),
                                                      st.ctypes.data_as(_dp)))
        else:
            self._chk(self.L.cora_problem_solve(self.h, x0.ctypes.data_as(_dp), int(max_rank), int(verbose),
                                                opts.ctypes.data_as(_dp), out.ctypes.data_as(_dp),
                                                st.ctypes.data_as(_dp)))
        return dict(x=out, f=st[0], grad_norm=st[1], certified=bool(st[2]), eta=st[3], theta=st[4],
                    final_rank=int(st[5]), levels=int(st[6]), hvps=int(st[7]), seconds=st[8],
                    relaxation_certified=bool(st[9]), relaxation_rank=int(st[10]))

    def save_trajectory(self, X, path, g2o=False, robot=None):
        """saveSolnToTum / saveSolnToG20 for an N x d solution; robot = symbol character or None for all poses."""
        X = np.asfortranarray(np.asarray(X, dtype=np.float64))
        self._chk(self.L.cora_problem_save_trajectory(self.h, X.ctypes.data_as(_dp), int(bool(g2o)),
                                                      ord(robot) if robot else 0, path.encode()))

    def precond_info(self):
        info = np.zeros(3)
        self._chk(self.L.cora_problem_precond_info(self.h, info.ctypes.data_as(_dp)))
        return dict(lam=info[0], nnz=int(info[1]), levels=int(info[2]))

    def cholesky_solve(self, B, m=None, shift=0.0, leaf_poses=16):
        dm = self.dims()
        m = dm["N"] - 1 if m is None else m
        B = np.asfortranarray(np.array(B, dtype=np.float64, copy=True))
        assert B.shape[0] == m
        info = (C.c_int64 * 3)()
        self._chk(self.L.cora_problem_cholesky_solve(self.h, int(m), C.c_double(shift), int(leaf_poses),
                                                     B.ctypes.data_as(_dp), B.shape[1], info))
        return B, dict(ok=bool(info[0]), nnz=int(info[1]), height=int(info[2]))

    def cholesky_probe(self, m=None, shift=0.0, leaf_poses=16, bump=None):
        """Host factorisation of (Q + shift I)[0:m, 0:m]: ok, nnz, first failing column, digest of L, negative direction.
        bump = {row: value}: added to those diagonal entries of a copy of Q first."""
        dm = self.dims()
        m = dm["N"] - 1 if m is None else m
        info = (C.c_int64 * 3)()
        digest = np.zeros(2)
        neg = np.zeros(dm["N"])
        rows = np.array(sorted(bump or {}), dtype=np.int32)
        vals = np.array([bump[r] for r in rows], dtype=np.float64) if len(rows) else np.zeros(0)
        self._chk(self.L.cora_problem_cholesky_probe_bumped(
            self.h, int(m), C.c_double(shift), int(leaf_poses), len(rows), rows.ctypes.data_as(C.POINTER(C.c_int32)),
            vals.ctypes.data_as(_dp), info, digest.ctypes.data_as(_dp), neg.ctypes.data_as(_dp)))
        return dict(ok=bool(info[0]), nnz=int(info[1]), failed_column=int(info[2]), digest=digest, negative_direction=neg)

    def plan_probe(self, shift, leaf_poses=2):
        """Host factorisation of (Q + shift I)[0:N-1] + the device solve plan built from it, no GPU involved."""
        info = (C.c_int64 * 4)()
        self._chk(self.L.cora_problem_plan_probe(self.h, C.c_double(shift), int(leaf_poses), info))
        return dict(stages=int(info[0]), nnzL=int(info[1]), blocks=int(info[2]), top_rows=int(info[3]))

    def context_ptr(self):
        c = self.L.cora_problem_context(self.h)
        if not c:
            raise HostError(self.L.cora_host_last_error().decode())
        return c


def manifold_op(kind, op, p, n, k=0, A=None, B=None, seed=0):
    """StiefelProduct(k, p, n) (kind "stiefel") / ObliqueManifold(p, n) (kind "oblique") of the reference, on the GPU."""
    L = _lib()
    cols = k * n if kind == "stiefel" else n
    f = lambda M: None if M is None else np.asfortranarray(np.asarray(M, dtype=np.float64))
    A, B = f(A), f(B)
    out = np.zeros(1) if op == "innerProduct" else np.zeros((p, cols), order="F")
    if L.cora_host_manifold_op(0 if kind == "stiefel" else 1, int(k), int(p), int(n), op.encode(),
                               None if A is None else A.ctypes.data_as(_dp), None if B is None else B.ctypes.data_as(_dp),
                               C.c_uint64(seed), out.ctypes.data_as(_dp)):
        raise HostError(L.cora_host_last_error().decode())
    return float(out[0]) if op == "innerProduct" else out


def block_cholesky_solve(A, block_sizes, B):
    """getBlockCholeskyFactorization + blockCholeskySolve of the reference's public interface, on the host."""
    import scipy.sparse as sp
    L = _lib()
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    rp = np.ascontiguousarray(A.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(A.indices, dtype=np.int32)
    va = np.ascontiguousarray(A.data, dtype=np.float64)
    bs = np.ascontiguousarray(block_sizes, dtype=np.int32)
    B = np.asfortranarray(np.asarray(B, dtype=np.float64).reshape(len(B), -1))
    X = np.zeros_like(B, order="F")
    ip = C.POINTER(C.c_int32)
    if L.cora_host_block_cholesky_solve(n, rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), va.ctypes.data_as(_dp), len(bs),
                                        bs.ctypes.data_as(ip), B.shape[0], B.shape[1], B.ctypes.data_as(_dp),
                                        X.ctypes.data_as(_dp)):
        raise HostError(L.cora_host_last_error().decode())
    return X


def fast_verification(S, eta, X0=None, nx=1, max_iters=1000, lab=None, split=None):
    """CORA::fast_verification on an arbitrary symmetric scipy sparse matrix.  lab = dict(max_fill_factor, drop_tol,
    seed, ildl) exposes the knobs of step 3 (tests) and adds `step3` to the result."""
    import scipy.sparse as sp
    L = _lib()
    S = sp.csr_matrix(S)
    S.sort_indices()
    n = S.shape[0]
    rp = np.ascontiguousarray(S.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(S.indices, dtype=np.int32)
    va = np.ascontiguousarray(S.data, dtype=np.float64)
    out = np.zeros(3)
    x = np.zeros(n)
    xp = None
    if X0 is not None:
        X0 = np.asfortranarray(np.asarray(X0, dtype=np.float64).reshape(n, -1))
        nx = X0.shape[1]
        xp = X0.ctypes.data_as(_dp)
    if split is not None:
        rc = L.cora_host_fast_verification_pieces(n, rp.ctypes.data_as(_ip), ci.ctypes.data_as(_ip), va.ctypes.data_as(_dp),
                                                  C.c_double(eta), xp, int(nx), int(split), int(max_iters),
                                                  out.ctypes.data_as(_dp), x.ctypes.data_as(_dp))
    elif lab is not None:
        out = np.zeros(4)
        opts = np.array([lab.get("max_fill_factor", 3.0), lab.get("drop_tol", 1e-3), float(lab.get("seed", True)),
                         float(lab.get("ildl", True))])
        rc = L.cora_host_fast_verification_lab(n, rp.ctypes.data_as(_ip), ci.ctypes.data_as(_ip), va.ctypes.data_as(_dp),
                                               C.c_double(eta), xp, int(nx), int(max_iters), opts.ctypes.data_as(_dp),
                                               out.ctypes.data_as(_dp), x.ctypes.data_as(_dp))
    else:
        rc = L.cora_host_fast_verification(n, rp.ctypes.data_as(_ip), ci.ctypes.data_as(_ip), va.ctypes.data_as(_dp),
                                           C.c_double(eta), xp, int(nx), int(max_iters), out.ctypes.data_as(_dp),
                                           x.ctypes.data_as(_dp))
    if rc:
        raise HostError(L.cora_host_last_error().decode())
    res = dict(is_certified=bool(out[0]), theta=out[1], iters=int(out[2]), x=x)
    if lab is not None:
        res["step3"] = bool(out[3])
    return res
