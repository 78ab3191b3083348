"""Time of the per-measurement residual pass (cora_measurement_residuals_dev) on the benchmark's synthetic graph, beside
the two things it replaces: the download of X (cora_download) and the one-core host loop over the measurements.
python tools/residuals_time.py [--poses 100000] [--rank 5]      (prints markdown: profiles/residuals.md)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cora_amd import capi, host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--rank", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    n, p = a.poses, a.rank
    P = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=10, n_ranges=n // 2, seed=42)
    P.update()
    P.set_rank(p)
    dm = P.dims()
    d = dm["d"]
    Y = P.op("getRandomInitialGuess")
    res = P.measurement_residuals(Y)  # installs the table on the handle
    f = P.op("evaluateObjective", Y)
    half = 0.5 * (res["rot_sum"] + res["trans_sum"] + res["range_sum"])
    ctx = capi.Context.from_handle(P.context_ptr(), d, dm["n"], dm["r"], dm["n"] + dm["l"])
    ne, nr = ctx.measurement_counts()
    ld = ctx.L.cora_ld_for(p)
    # rows of X the table touches, from the incidence matrices (an edge's pose a is the -1 of its row, b the +1)
    Ap, Ar = P.scipy_matrix("Apose").tocoo(), P.scipy_matrix("Arange").tocoo()
    with_rot = dm["rpm"] + int(P_counts(P)[1])
    rot_poses = set(Ap.col[Ap.data < 0].tolist()) | set(Ap.col[(Ap.data > 0) & (Ap.row < with_rot)].tolist())
    trans = set(Ap.col.tolist()) | set(Ar.col.tolist())
    rows = d * len(rot_poses) + nr + len(trans)
    table_bytes = ne * (4 * 4 + (d * d + d + 2) * 8) + nr * (3 * 4 + 2 * 8)
    x = ctx.dev_alloc(p)
    ctx.upload(Y, x)
    sums = np.zeros(3)
    rot, trn, rng = np.zeros(ne), np.zeros(ne), np.zeros(nr)
    dp = C.POINTER(C.c_double)

    def call(values):
        o = [v.ctypes.data_as(dp) for v in (rot, trn, rng)] if values else [None, None, None]
        ctx._chk(ctx.L.cora_measurement_residuals_dev(ctx.h, C.c_void_p(x), p, o[0], o[1], o[2], sums.ctypes.data_as(dp)))

    def timed(fn):
        ev, wall = [], []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            ctx.timer_start()
            fn()
            ms = ctx.timer_stop_ms()
            if i >= a.warmup:
                ev.append(ms * 1e3)
                wall.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(ev)), float(np.median(wall))

    pass_ev, pass_wall = timed(lambda: call(False))
    vals_ev, vals_wall = timed(lambda: call(True))
    back = np.zeros((ctx.N, p), order="F")  # (allocated and touched once: the download alone is timed)
    down_ev, down_wall = timed(lambda: ctx._chk(ctx.L.cora_download(ctx.h, C.c_void_p(x), p, back.ctypes.data_as(dp), ctx.N)))
    assert np.array_equal(back, Y)
    t0 = time.perf_counter()
    hostres = ctx.debug_measurement_residuals_host(Y)
    host_us = (time.perf_counter() - t0) * 1e6
    scale = max(rot.max(), trn.max(), rng.max())
    err = max(np.abs(hostres["edge_rot"] - rot).max(), np.abs(hostres["edge_trans"] - trn).max(),
              np.abs(hostres["range"] - rng).max()) / scale
    ctx.dev_free(x)
    print("| quantity | value |")
    print("|---|---|")
    print("| graph | %d poses, %d landmarks, d = %d, p = %d (row stride %d): %d edges, %d ranges |" % (dm["n"], dm["l"], d, p, ld, ne, nr))
    print("| measurement table | %.2f MB |" % (table_bytes / 1e6))
    print("| distinct rows of X read | %d rows, %.2f MB |" % (rows, rows * ld * 8 / 1e6))
    print("| residual pass, totals only (median of %d, event timer / wall clock) | %.1f us / %.1f us |" % (a.calls, pass_ev, pass_wall))
    print("| residual pass + the %d values copied to the host | %.1f us / %.1f us |" % (2 * ne + nr, vals_ev, vals_wall))
    print("| cora_download of X (what the pass replaces) | %.1f us / %.1f us |" % (down_ev, down_wall))
    print("| host loop over the translated table, one core (one call) | %.0f us |" % host_us)
    print("| device values vs host loop, largest difference / largest value | %.1e |" % err)
    print("| 1/2 of the totals vs evaluateObjective | %.12g vs %.12g |" % (half, f))
    print("| effective rate of the pass (table + distinct rows) | %.2f TB/s |" % ((table_bytes + rows * ld * 8) / pass_ev / 1e6))


def P_counts(P):
    cnt = (C.c_int64 * 5)()
    P._chk(P.L.cora_problem_measurement_counts(P.h, cnt))
    return [int(v) for v in cnt]


if __name__ == "__main__":
    main()
