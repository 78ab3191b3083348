"""The product kernel (k_spmm and the long-row chunks, cora_amd/csrc/kernels/spmm.inc) on the catalogue of
tests/topologies.py -- several robots, hubs, fat landmarks, reversed edges, priors, duplicates, tiny pose counts: the
formats the host executor already reproduces (tests/test_topologies_cpu.py), now read by the device.

Every entry, in both forms of the pose slices (LDS windows / direct gathers), at one row stride per compile-time regime of
pose_slice (topologies_worker.WIDE_STRIDES and p = d): Q X, the Lambda blocks, (Q - Lambda) X, the Hessian-vector product
through the host-pointer and the resident entry points, and -- because a wrong kappa leaves Hp right -- the device STPCG
without a preconditioner after 1 and 2 INTERIOR iterations against tests/stpcg_ref.py (p <= 12; that the reference's step
is interior is asserted from its own kappa, here and in test_topologies_cpu).  Before anything is compared the handle's
format has the shape the entry declares (cora_debug_format_shape).

Then: `robots` again with every pose slice in the plain layout (a child process under CORA_CHAIN_SLICES=0, started once,
under its own time limit: if it ends by signal or timeout every test of the module fails and nothing further runs on
the device); partitioned handles without communication (world 3, whole long rows, NaN in every row cora_remote_rows does
not list); partitioned handles with the library's own communication at world 2 and 3, serial and overlapped, in both
forms, with one device-resident TNT step against the single handle.

Bounds, the project's own and none from a run: products 1e-10 of the largest entry (test_gpu_parity.REL), Lambda blocks
1e-9 absolute (test_gpu_parity.TOL), STPCG vectors and |s|_M 1e-9 and its product 1e-10 per row class
(test_gpu_stpcg_forms.BOUND), the TNT step as test_gpu_sharded.test_sharded_operators_and_tnt_match_single_handle.
Observed: profiles/topologies.md."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import topologies as topo
import topologies_worker as W
from cora_amd import capi
from cora_amd.dist import NativeLocalComm
from oracle import oracle as orc
from test_gpu_sharded import _run_ranks
from test_gpu_stpcg_forms import BOUND as STPCG_BOUND

pytestmark = pytest.mark.gpu

REL = 1e-10   # test_gpu_parity.REL
TOL = 1e-9    # test_gpu_parity.TOL
BOUND = {"prod": REL, "lam": TOL, "vec": STPCG_BOUND["vec"]}
assert STPCG_BOUND["prod"] == REL
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "topologies_worker.py")
FAULT_WORDS = ("illegal memory access", "HSA_STATUS_ERROR", "Memory access fault", "CORA_ERR_HIP", "hipError")
PLAIN_LIMIT_S = 240
_STATE = {"fatal": None}   # set when the plain-layout child ended by signal or timeout: the device gets no further work


@pytest.fixture(autouse=True)
def device_in_order():
    if _STATE["fatal"]:
        pytest.fail(_STATE["fatal"])


@pytest.fixture
def restore_form():
    L = capi.load()
    old = L.cora_debug_spmm_window_min_slices(0)
    L.cora_debug_spmm_window_min_slices(old)
    yield L
    L.cora_debug_spmm_window_min_slices(old)


def _judge(tag, out):
    print("\n%s: %s" % (tag, "  ".join("%s %.2e" % (n, v) for n, v, _ in out["checks"])))
    assert out["fail"] == [], tag
    assert [n for n, _, k in out["checks"] if k == "prod"], "nothing was compared"
    for what, value, kind in out["checks"]:
        assert value <= BOUND[kind], (tag, what, value, BOUND[kind])


CASES = [(name, p) for name in topo.NAMES for p in W.strides(topo.CATALOGUE[name][1])]


@pytest.mark.parametrize("name,p", CASES, ids=["%s-p%d" % c for c in CASES])
def test_operators_on_every_topology(name, p, restore_form):
    for form, win in W.FORMS:
        out = W.measure(name, p, restore_form, win)
        got = out["shape"]
        for key, (lo, hi) in topo.CATALOGUE[name][2].items():   # the DEVICE handle has the declared shape
            assert (lo is None or got[key] >= lo) and (hi is None or got[key] <= hi), (name, key, got[key], lo, hi)
        if p <= W.KAPPA_MAX_P:
            assert any(n.startswith("s2.") for n, _, _ in out["checks"]), "the kappa check did not run"
        _judge("%s p=%d %s" % (name, p, form), out)


# ---- the plain layout: one child process ----------------------------------------------------------------------------------
def _run_plain_child():
    env = dict(os.environ, CORA_CHAIN_SLICES="0")
    try:
        r = subprocess.run([sys.executable, WORKER, "plain"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=PLAIN_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
        return {}, "the plain-layout child did not finish in time:\n%s" % out[-4000:], True
    cases = {}
    for line in r.stdout.splitlines():
        if line.startswith("CASE "):
            c = json.loads(line[5:])
            cases[c["id"]] = c
    fault = next((w for w in FAULT_WORDS if w in r.stdout), None)
    if r.returncode != 0 or fault or "DONE" not in r.stdout.splitlines():
        msg = "the plain-layout child ended with status %d%s:\n%s" % (
            r.returncode, " and '%s' in its output" % fault if fault else "", r.stdout[-4000:])
        return cases, msg, bool(r.returncode < 0 or fault)
    return cases, None, False


@pytest.fixture(scope="module")
def plain_child():
    cases, fatal, device_suspect = _run_plain_child()
    if device_suspect:
        _STATE["fatal"] = fatal
    return dict(cases=cases, fatal=fatal)


@pytest.mark.parametrize("cid", W.plain_case_ids())
def test_plain_layout(plain_child, cid):
    """EPI_NONE, EPI_S, EPI_HVP and EPI_HVP_K of a pose slice that holds every column explicitly (the cooperative and the
    per-lane epilogue by stride), its translation rows in the row slices: every pose slice of `robots` is plain."""
    if plain_child["fatal"]:
        pytest.fail(plain_child["fatal"])
    assert cid in plain_child["cases"], "the child printed nothing for %s" % cid
    c = plain_child["cases"][cid]
    assert c["shape"]["chain_slices"] == 0 and c["shape"]["plain_slices"] == 4
    _judge("plain " + cid, c)


# ---- partitions without communication ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["robots-d3", "hub-d3", "fat_landmark", "reversed"])
def test_partitions_without_communication(name, restore_form):
    """test_gpu_parity.test_partitioned_handles_match_single on the catalogue: world 3, whole long rows, every rank's
    shard of the Hvp is the single handle's; only the rows cora_remote_rows lists are read outside the shard."""
    A, Q, dm, g = topo.build(name)
    p, world = 5, 3
    R = W.references(name, p)
    Y, V, ref = R["Y"], R["V"], R["hv"]
    for form, win in W.FORMS:
        restore_form.cora_debug_spmm_window_min_slices(win)
        total = np.zeros_like(ref)
        fsum = 0.0
        for rank in range(world):
            c = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, rank=rank, world=world,
                             whole_long_rows=True)
            c.set_rank(p)
            c.set_point(Y)
            fsum += c.point_cost()
            x, o = c.dev_alloc(p), c.dev_alloc(p)
            c.upload(V, x)
            c.hvp_dev(x, o)
            got = c.download(o, p)
            m = c.row_map()
            mine = (m >= c.shard_begin) & (m < c.shard_begin + c.shard_rows)
            total[mine] = got[mine]
            need = c.remote_rows()
            assert need.size and np.all((need < c.shard_begin) | (need >= c.shard_begin + c.shard_rows))
            keep = mine | np.isin(m, need)
            Vp = V.copy()
            Vp[~keep] = np.nan
            c.upload(Vp, x)
            c.hvp_dev(x, o)
            assert np.array_equal(c.download(o, p)[mine], got[mine]), (form, rank)
            c.close()
        err = W.relerr(total, ref)
        print("\n%s %s: Hvp over 3 partitions %.2e" % (name, form, err))
        assert err < REL, form
        assert abs(fsum - orc.cost(Q, Y)) < 1e-11 * orc.cost(Q, Y)


# ---- partitions with the library's own communication ------------------------------------------------------------------------
# Whether some rank that has remote tail pairs SPLITS its product under comm.overlap(2) (interior slices ahead of the
# exchange, kSliceSkipRemoteTail / kSliceRemoteTailOnly): a rank splits only where it has interior AND boundary slices
# (capi/products.inc, product_overlaps_exchange), and a chain slice runs ahead only where its general slots are local.
# Where the entry is False no rank splits -- every slice of these small shards reads a remote row -- and "overlapped
# equals serial" compares the serial product with itself: stated here so that nobody reads more into it.
SPLITS = {("robots-d2", 2): True, ("robots-d2", 3): True, ("robots-d3", 2): True, ("robots-d3", 3): True,
          ("hub-d2", 2): False, ("hub-d2", 3): False, ("hub-d3", 2): False, ("hub-d3", 3): False,
          ("fat_landmark", 2): True, ("fat_landmark", 3): False}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["robots-d2", "robots-d3", "hub-d2", "hub-d3", "fat_landmark"])
def test_partitions_with_native_communication(name, world, restore_form):
    """Pose-pose ranges across shards (remote pairs in the tails: kSliceSkipRemoteTail / kSliceRemoteTailOnly in the
    overlapped product), a distributed long row owned by a POSE (hub), long rows of several chunks per rank
    (fat_landmark): Hvp and Q V against the oracle, overlapped equal to serial bit for bit, in both forms; then two
    interior iterations of the device STPCG against tests/stpcg_ref.py -- kappa over the ranks: the partials of the
    slices, of the remote tails and, through k_long_finish, of the distributed long rows (several chunks per rank in
    fat_landmark).  robots and hub are built by the C++ host (topologies.to_problem) and take one device-resident TNT step
    against the single handle; fat_landmark repeats measurements, which CORA::Problem refuses: its ranks are handles of
    the matrix and take no TNT step."""
    A, Q, dm, g = topo.build(name)
    p = 5
    R = W.references(name, p)
    Y, V = R["Y"], R["V"]
    ref_qv = orc.spmm(Q, V)
    by_problem = not topo.has_duplicates(name)
    single = None
    if by_problem:
        P1 = topo.to_problem(name, rank=p)
        got = P1.scipy_matrix("DataMatrix")
        assert abs(got - A["Q"]).max() <= 1e-12 * abs(A["Q"]).max()
        single = P1.tnt(Y, max_iterations=1)
        P1.close()

    def body(r, group):
        if by_problem:
            P = topo.to_problem(name, rank=p)
            comm = P.set_partition(r, world, lambda ctx: NativeLocalComm(ctx, group))
            ctx = capi.Context.from_handle(P.context_ptr(), dm.d, dm.n, dm.r, dm.n_trans)
        else:
            P = None
            ctx = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val, rank=r, world=world)
            ctx.set_rank(p)
            comm = NativeLocalComm(ctx, group)
        shape = ctx.format_shape()
        shape["distributed_long_rows"] = len(ctx.long_rows())
        y, x, o = ctx.dev_alloc(p), ctx.dev_alloc(p), ctx.dev_alloc(p)
        ctx.upload(Y, y)
        ctx.set_point_dev(y)
        ctx.upload(V, x)
        out = {}
        for mode in (0, 2):
            comm.overlap(mode)
            if mode == 0:
                assert not comm.overlap_active()
            else:   # (a rank splits its product only where it has interior AND boundary slices: not every shard this small)
                shape["overlapped"] = int(comm.overlap_active())
            ctx.hvp_dev(x, o)
            H = ctx.download(o, p)
            ctx.spmm_dev(x, p, o)
            out[mode] = (H, ctx.download(o, p))
        comm.overlap(1)
        res = P.tnt(Y, max_iterations=1) if by_problem else None
        # kappa on partitions (last: it replaces the handle's point and preconditioner)
        gr, s, rr, v, pk, hp = (ctx.dev_alloc(p) for _ in range(6))
        ctx.set_point_dev(y)
        ctx.upload(R["grad"], gr)
        ctx.precond_setup(capi.PRECOND_NONE)
        steps = []
        for k in (1, 2):
            it, sM = ctx.stpcg_dev(gr, W.FAR, s, rr, v, pk, hp, kappa_fgr=W.NO_TARGET, theta=0.0, max_iters=k)
            steps.append((it, sM, ctx.download(s, p), ctx.download(rr, p)))
        return shape, out, res, steps

    worst = worst_vec = 0.0
    for form, win in W.FORMS:   # (the switch is process-wide: set while no rank is running)
        restore_form.cora_debug_spmm_window_min_slices(win)
        outs = _run_ranks(world, body, "native")
        shapes = [o[0] for o in outs]
        print("\n%s world %d %s: (remote tail pairs, long pose rows, most chunks) per rank %s" % (
            name, world, form, [(s["remote_tail_pairs"], s["long_pose_rows"], s["max_chunks"]) for s in shapes]))
        print("overlapped product taken on ranks %s" % [r for r, s in enumerate(shapes) if s["overlapped"]])
        assert sum(s["remote_tail_pairs"] for s in shapes) > 0
        split = any(s["overlapped"] and s["remote_tail_pairs"] > 0 for s in shapes)
        assert split == SPLITS[name, world], (name, world, split)
        if name.startswith("hub"):
            assert all(s["distributed_long_rows"] == 1 for s in shapes) and sum(s["long_pose_rows"] for s in shapes) >= 1
        if name == "fat_landmark":
            assert all(s["distributed_long_rows"] == 3 for s in shapes) and max(s["max_chunks"] for s in shapes) >= 2
        assert W.interior(R) is None
        for shape, out, res, steps in outs:
            for k, (it, sM, s_dev, r_dev) in enumerate(steps, 1):
                state = R["states"][k - 1]
                assert it == k
                errs = {"s%d.%s" % (k, c): e for c, e in W.class_errors(dm, s_dev, state["s"]).items()}
                errs.update({"r%d.%s" % (k, c): e for c, e in W.class_errors(dm, r_dev, state["r"]).items()})
                errs["sM%d" % k] = abs(sM - state["sM"]) / state["sM"]
                worst_vec = max(worst_vec, max(errs.values()))
                for what, e in errs.items():
                    assert e <= BOUND["vec"], (form, what, e)
            for mode in (0, 2):
                H, QV = out[mode]
                worst = max(worst, W.relerr(H, R["hv"]), W.relerr(QV, ref_qv))
                assert W.relerr(H, R["hv"]) < REL and W.relerr(QV, ref_qv) < REL, (form, mode)
            assert np.array_equal(out[0][0], out[2][0]) and np.array_equal(out[0][1], out[2][1]), form
            if by_problem:
                assert res["iterations"] == single["iterations"] and res["hvps"] == single["hvps"]
                assert abs(res["f"] - single["f"]) < 1e-10 * abs(single["f"])
                assert np.abs(res["x"] - single["x"]).max() < 1e-8
        for o in outs[1:]:
            if by_problem:
                assert np.array_equal(o[2]["x"], outs[0][2]["x"])
    print("%s world %d: worst product error %.2e, worst STPCG vector error %.2e" % (name, world, worst, worst_vec))
