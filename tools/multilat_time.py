"""Time and value of the landmark initialisation from ranges (cora_multilaterate_dev, include/cora_hip.h).
Time: the device call with 5 Gauss-Newton steps on a resident vector -- the handle's event timer and the wall clock of
the call -- against the host mirror (cora_debug_multilaterate_host, one thread, wall clock) in the same run, alternated
and reported as medians, on the benchmark's 10^5-pose synthetic graph (10 landmarks, 5 10^4 ranges: a hub) and on a graph
of 10^4 landmarks with 8 ranges each.  Value: f(x0), the landmark RMSE against the ground truth
(Problem::compareToReference) and the landmarks solved / refused with and without it on the shipped data sets and on the
10^4-pose synthetic graph.  --kernels-only runs the hub graph's device call alone (the program of a
`rocprofv3 --kernel-trace --stats` run of its own); --stats-csv adds that run's per-kernel table.
Writes the section between the two markers of profiles/multilateration.md.
python tools/multilat_time.py [--reps 9] [--out profiles/multilateration.md] [--stats-csv x_kernel_stats.csv] [--kernels-only]"""
import argparse
import csv
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cora_amd import capi, host  # noqa: E402

BEGIN, END = "<!-- measured:begin -->", "<!-- measured:end -->"
GN = 5


def hub_graph():
    """(ctx, X, keep): the 10^5-pose synthetic graph's handle with its tables and the odometry start in d columns."""
    P = host.Problem.synthetic(dim=3, n_poses=100000, n_landmarks=10, n_ranges=50000, seed=42)
    P.update()
    P.set_rank(5)
    dm = P.dims()
    P.op("odometryInitialization")   # installs the measurement table and the chain tables
    ctx = capi.Context.from_handle(P.context_ptr(), dm["d"], dm["n"], dm["r"], dm["n"] + dm["l"])
    rng = np.random.default_rng(1)
    x = ctx.dev_alloc(dm["d"])
    ctx.odometry_init_dev(10 * rng.uniform(-1, 1, (ctx.odometry_chains_count()[0], dm["d"])), 10 * rng.uniform(-1, 1, (dm["l"], dm["d"])), x)
    X = np.asfortranarray(ctx.download(x, dm["d"]))
    ctx.dev_free(x)
    ctx.set_multilateration()
    return ctx, X, P


def wide_graph(nl=10000, per=8, n=20000, d=3):
    """(ctx, X, keep): ranges only, nl landmarks of `per` noisy ranges each to random poses of a random walk."""
    rng = np.random.default_rng(2)
    poses = np.cumsum(rng.normal(0, 1, (n, d)), axis=0)
    lms = poses[rng.integers(0, n, nl)] + 10 * rng.uniform(-1, 1, (nl, d))
    r = nl * per
    t0 = d * n + r
    who = rng.integers(0, n, (nl, per))
    rr = np.zeros((r, 3), dtype=np.int32)
    rr[:, 0] = d * n + np.arange(r)
    rr[:, 1] = t0 + who.reshape(-1)
    rr[:, 2] = t0 + n + np.repeat(np.arange(nl), per)
    rd = np.ones((r, 2))
    rd[:, 0] = np.abs(np.linalg.norm(poses[who.reshape(-1)] - np.repeat(lms, per, axis=0), axis=1) + 0.05 * rng.normal(0, 1, r))
    order = rng.permutation(r)
    rr[:, 1:], rd = rr[order, 1:], rd[order]
    N = t0 + n + nl
    ctx = capi.Context(d, n, r, n + nl, np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32), np.ones(N))
    ctx.set_measurements(np.zeros((0, 4), dtype=np.int32), np.zeros((0, d * d + d + 2)), rr, rd)
    ctx.set_multilateration()
    X = np.zeros((N, d), order="F")
    for c in range(d):
        X[c:d * n:d, c] = 1.0
    X[t0:t0 + n] = poses
    return ctx, X, None


def mirror_ms(ctx, X):
    """Wall clock of the host mirror alone (the C call on a prepared copy)."""
    Y = np.array(X, order="F", copy=True)
    out = (C.c_int64 * 4)()
    t0 = time.perf_counter()
    rc = ctx.L.cora_debug_multilaterate_host(ctx.h, Y.ctypes.data_as(C.POINTER(C.c_double)), Y.shape[0], GN, out, None, None, None, None, None)
    t1 = time.perf_counter()
    assert rc == 0, rc
    return (t1 - t0) * 1e3, Y


def time_graph(name, make, reps):
    ctx, X, keep = make()
    d = ctx.d
    x = ctx.dev_alloc(d)
    t = dict(event=[], call=[], mirror=[])
    res = same = None
    for rep in range(reps + 1):
        ctx.upload(X, x)
        ctx.sync()
        a0 = time.perf_counter()
        res = ctx.multilaterate_dev(x, GN)
        a1 = time.perf_counter()
        got = ctx.download(x, d)
        ctx.upload(X, x)
        ctx.timer_start()
        ctx.multilaterate_dev(x, GN)
        ev = ctx.timer_stop_ms()
        mm, Y = mirror_ms(ctx, X)
        same = bool(np.array_equal(got.view(np.int64), Y.view(np.int64)))
        if rep:  # (the first round warms the allocator and the kernels' code objects)
            t["event"].append(ev)
            t["call"].append((a1 - a0) * 1e3)
            t["mirror"].append(mm)
    ctx.dev_free(x)
    counts = ctx.multilateration_counts()
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}
    return dict(name=name, counts=counts, solved=res["solved"], steps=res["steps"], same=same, med=med, spread=spread, reps=reps)


def value_rows():
    rows = []
    data = os.path.join(ROOT, "tests", "golden", "datasets")
    cases = [(n, os.path.join(data, n + ".pyfg")) for n in ("plaza1", "plaza2", "tiers", "single_drone")] + [("synthetic 10^4 poses", None)]
    for name, path in cases:
        if path:
            P = host.Problem.from_pyfg(path)
            P.update()
            P.set_rank(5)
            gt = P.ground_truth(path)
        else:
            P, gt = host.Problem.synthetic(dim=3, n_poses=10000, n_landmarks=10, n_ranges=5000, seed=42, ground_truth=True)
            P.update()
            P.set_rank(5)
        old = P.op("odometryInitialization")
        new, info = P.range_aided_initialization(seed=7, gn_steps=GN)
        rows.append(dict(name=name, l=P.dims()["l"], f_old=P.op("evaluateObjective", old), f_new=P.op("evaluateObjective", new),
                         rmse_old=P.compare(old, gt, proper=False)["landmark_rmse"], rmse_new=P.compare(new, gt, proper=False)["landmark_rmse"],
                         range_old=P.measurement_residuals(old)["range_sum"], range_new=P.measurement_residuals(new)["range_sum"],
                         solved=info["solved"], refused=info["not_solved"], status=np.bincount(info["status"], minlength=4).tolist()))
    return rows


def stats_rows(path):
    out = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "k_ml_" in name or "k_odom_ranges" in name or "k_round_finish" in name:
                out.append((name, int(row["Calls"]), float(row["AverageNs"]) * 1e-3, float(row["MinNs"]) * 1e-3, float(row["MaxNs"]) * 1e-3))
    if not out:
        raise SystemExit("%s names none of the multilateration's kernels" % path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multilateration.md"))
    ap.add_argument("--stats-csv")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-value", action="store_true")
    a = ap.parse_args()
    if a.kernels_only:
        ctx, X, keep = hub_graph()
        x = ctx.dev_alloc(ctx.d)
        for _ in range(20):
            ctx.upload(X, x)
            ctx.multilaterate_dev(x, GN)
        ctx.dev_free(x)
        return
    lines = [BEGIN, "", "Device call with %d Gauss-Newton steps (%d launches of the stages, 2 of the range rows) against the host mirror, alternated in one run;"
             % (GN, 2 * (GN + 2)), "medians of the repetitions after one warm-up round (least .. largest in brackets), milliseconds.", "",
             "| graph | landmarks with a list | usable ranges | chunks | solved | device, events | device, wall clock of the call | host mirror, one thread | mirror / device (wall) | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, make in (("10^5 poses, 10 landmarks, 5 10^4 ranges (hub)", hub_graph), ("10^4 landmarks x 8 ranges", wide_graph)):
        g = time_graph(name, make, a.reps)
        cell = lambda k: "%.3f (%.3f .. %.3f)" % (g["med"][k], *g["spread"][k])  # noqa: E731
        lines.append("| %s | %d | %d | %d | %d | %s | %s | %s | %.1f | %s |" % (name, g["counts"][0], g["counts"][1], g["counts"][3], g["solved"],
                     cell("event"), cell("call"), cell("mirror"), g["med"]["mirror"] / g["med"]["call"], "yes" if g["same"] else "NO"))
        print(lines[-1], flush=True)
    if a.stats_csv:
        lines += ["", "Per kernel, from one `rocprofv3 --kernel-trace --stats` run of `--kernels-only` (20 calls on the hub graph), microseconds.", "",
                  "| kernel | calls | mean | least | largest |", "|---|---|---|---|---|"]
        for name, calls, mean, lo, hi in stats_rows(a.stats_csv):
            lines.append("| `%s` | %d | %.2f | %.2f | %.2f |" % (name.replace("|", "\\|"), calls, mean, lo, hi))
    if not a.no_value:
        lines += ["", "The start with and without the landmark initialisation (seed 7, %d steps, rank 5): the objective, the range residual sum" % GN,
                  "(`measurementResiduals`), the landmark RMSE against the ground truth after the alignment on all positions", "(`Problem::compareToReference`), landmarks by status.", "",
                  "| graph | landmarks | f(x0) without | f(x0) with | range residual sum without | with | landmark RMSE without | with | solved | refused | status 0 / 1 / 2 / 3 |",
                  "|---|---|---|---|---|---|---|---|---|---|---|"]
        for v in value_rows():
            lines.append("| %s | %d | %.6g | %.6g | %.6g | %.6g | %.4g | %.4g | %d | %d | %s |" % (v["name"], v["l"], v["f_old"], v["f_new"], v["range_old"],
                         v["range_new"], v["rmse_old"], v["rmse_new"], v["solved"], v["refused"], " / ".join(str(s) for s in v["status"])))
            print(lines[-1], flush=True)
    lines += ["", END]
    text = open(a.out).read() if os.path.exists(a.out) else ""
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + "\n".join(lines) + text[text.index(END) + len(END):]
    else:
        text = text + "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
