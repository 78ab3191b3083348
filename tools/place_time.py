"""Time and value of the chain placement from inter-robot ranges (cora_place_chains_dev, include/cora_hip.h).
Time: the device call with 5 Gauss-Newton steps on a resident vector -- the handle's event timer and the wall clock of
the call -- against the host mirror (cora_debug_place_chains_host, one thread, wall clock) in the same run, alternated
and reported as medians, on 10^5 poses in 10 chains with 10^5 ranges between chains and on 10^3 chains of 100 poses with
80 ranges each against the first.  Value: f(x0), the range residual sum, the position RMSE against the ground truth
(Problem::compareToReference) and the chains by status with and without it on the shipped multi-robot data sets.
--kernels-only runs the first graph's device call alone (the program of a `rocprofv3 --kernel-trace --stats --output-format csv`
run of its own); --stats-csv adds that run's per-kernel table.  Writes the section between the two markers of
profiles/chain_placement.md.
python tools/place_time.py [--reps 9] [--out profiles/chain_placement.md] [--stats-csv x_kernel_stats.csv] [--kernels-only]"""
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


def chains_graph(nch, per, ranges_of, d=3, seed=3, noise=0.02, device=0):
    """(ctx, X): nch chains of `per` poses (identity rotations, random walks in one world frame), every chain after the first
    held in a frame of its own; ranges_of(rng) -> (a, b) pose indices [r][2] measured in the world frame."""
    rng = np.random.default_rng(seed)
    n = nch * per
    world = (20 * rng.uniform(-1, 1, (nch, 1, d)) + np.cumsum(rng.normal(0, 1, (nch, per, d)), axis=1)).reshape(n, d)
    ab = ranges_of(rng)
    r = len(ab)
    t0 = d * n + r
    own = world.copy()
    for c in range(1, nch):
        th = rng.uniform(-2.5, 2.5)
        Rc = np.eye(d)
        Rc[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        own[c * per:(c + 1) * per] = (world[c * per:(c + 1) * per] - 10 * rng.uniform(-1, 1, d)) @ Rc   # R^T (x - t)
    N = t0 + n
    X = np.zeros((N, d), order="F")
    for c in range(d):
        X[c:d * n:d, c] = 1.0
    # (the rotation blocks stay the identity: the placement moves them with the chain, and the ranges read positions only)
    X[t0:] = own
    heads = np.arange(n).reshape(nch, per)[:, :-1].reshape(-1)
    er = np.stack([d * heads, d * (heads + 1), t0 + heads, t0 + heads + 1], axis=1).astype(np.int32)
    ed = np.zeros((len(heads), d * d + d + 2))
    ed[:, :d * d] = np.eye(d).reshape(-1)
    ed[:, d * d:d * d + d] = own[heads + 1] - own[heads]
    ed[:, d * d + d:] = 1.0
    rr = np.stack([d * n + np.arange(r), t0 + ab[:, 0], t0 + ab[:, 1]], axis=1).astype(np.int32)
    rd = np.ones((r, 2))
    rd[:, 0] = np.abs(np.linalg.norm(world[ab[:, 0]] - world[ab[:, 1]], axis=1) + noise * rng.normal(0, 1, r))
    ctx = capi.Context(d, n, r, n, np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32), np.ones(N), device=device)
    ctx.set_measurements(er, ed, rr, rd)
    edges = np.arange(len(heads)).reshape(nch, per - 1)
    ctx.set_odometry_chains([edges[c] for c in range(nch)])
    ctx.set_chain_placement()
    return ctx, X


def ten_chains(device=0):
    nch, per, r = 10, 10000, 100000

    def ranges_of(rng):
        ca = rng.integers(0, nch, r)
        cb = (ca + rng.integers(1, nch, r)) % nch
        return np.stack([ca * per + rng.integers(0, per, r), cb * per + rng.integers(0, per, r)], axis=1)
    return chains_graph(nch, per, ranges_of, device=device)


def thousand_chains(device=0):
    nch, per, each = 1000, 100, 80

    def ranges_of(rng):
        c = np.repeat(np.arange(1, nch), each)
        ab = np.stack([c * per + rng.integers(0, per, len(c)), rng.integers(0, per, len(c))], axis=1)
        flip = rng.uniform(0, 1, len(c)) < 0.5
        ab[flip] = ab[flip][:, ::-1]
        return ab[rng.permutation(len(c))]
    return chains_graph(nch, per, ranges_of, device=device)


def mirror_ms(ctx, X):
    """Wall clock of the host mirror alone (the C call on a prepared copy)."""
    Y = np.array(X, order="F", copy=True)
    out = (C.c_int64 * 5)()
    t0 = time.perf_counter()
    rc = ctx.L.cora_debug_place_chains_host(ctx.h, Y.ctypes.data_as(C.POINTER(C.c_double)), Y.shape[0], GN, out, None, None, None, None, None, None, None)
    t1 = time.perf_counter()
    assert rc == 0, rc
    return (t1 - t0) * 1e3, Y


def time_graph(name, make, reps):
    ctx, X = make()
    d = ctx.d
    x = ctx.dev_alloc(d)
    t = dict(event=[], call=[], mirror=[])
    res = same = None
    for rep in range(reps + 1):
        ctx.upload(X, x)
        ctx.sync()
        a0 = time.perf_counter()
        res = ctx.place_chains_dev(x, GN)
        a1 = time.perf_counter()
        got = ctx.download(x, d)
        ctx.upload(X, x)
        ctx.timer_start()
        ctx.place_chains_dev(x, GN)
        ev = ctx.timer_stop_ms()
        mm, Y = mirror_ms(ctx, X)
        same = bool(np.array_equal(got.view(np.int64), Y.view(np.int64)))
        if rep:  # (the first round warms the allocator and the kernels' code objects)
            t["event"].append(ev)
            t["call"].append((a1 - a0) * 1e3)
            t["mirror"].append(mm)
    ctx.dev_free(x)
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}
    return dict(name=name, counts=ctx.chain_placement_counts(), placed=res["placed"], steps=res["steps"], same=same, med=med, spread=spread)


def value_rows():
    rows = []
    data = os.path.join(ROOT, "tests", "golden", "datasets")
    for name in ("tiers", "mrclam3b", "mrclam5a", "mrclam6"):
        path = os.path.join(data, name + ".pyfg")
        P = host.Problem.from_pyfg(path)
        P.update()
        P.set_rank(5)
        gt = P.ground_truth(path)
        old, _ = P.range_aided_initialization(seed=7, gn_steps=GN)
        new, info = P.multi_robot_initialization(seed=7, gn_steps=GN)
        rows.append(dict(name=name, chains=len(info["status"]), f_old=P.op("evaluateObjective", old), f_new=P.op("evaluateObjective", new),
                         rmse_old=P.compare(old, gt, proper=False)["trans_rmse"], rmse_new=P.compare(new, gt, proper=False)["trans_rmse"],
                         range_old=P.measurement_residuals(old)["range_sum"], range_new=P.measurement_residuals(new)["range_sum"],
                         placed=info["placed"], refused=info["not_placed"], status=np.bincount(info["status"], minlength=5).tolist(),
                         costs=[(float(a), float(b)) for a, b, s in zip(info["cost_start"], info["cost_final"], info["status"]) if s in (0, 2)]))
    return rows


def stats_rows(path):
    out = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "k_pl_" in name or "k_odom_ranges" in name:
                out.append((name, int(row["Calls"]), float(row["AverageNs"]) * 1e-3, float(row["MinNs"]) * 1e-3, float(row["MaxNs"]) * 1e-3))
    if not out:
        raise SystemExit("%s names none of the placement's kernels" % path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_placement.md"))
    ap.add_argument("--stats-csv")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-value", action="store_true")
    a = ap.parse_args()
    if a.kernels_only:
        ctx, X = ten_chains()
        x = ctx.dev_alloc(ctx.d)
        for _ in range(20):
            ctx.upload(X, x)
            ctx.place_chains_dev(x, GN)
        ctx.dev_free(x)
        return
    lines = [BEGIN, "", "Device call with %d Gauss-Newton steps (%d launches per stage, one stage after the other, 2 of the range rows) against the host"
             % (GN, 2 * (GN + 3) + 1), "mirror, alternated in one run; medians of the repetitions after one warm-up round (least .. largest in brackets), milliseconds.", "",
             "| graph | stages | entries | chunks | placed | device, events | device, wall clock of the call | host mirror, one thread | mirror / device (wall) | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, make in (("10^5 poses in 10 chains, 10^5 ranges between chains", ten_chains), ("10^3 chains x 100 poses, 80 ranges each against the first", thousand_chains)):
        g = time_graph(name, make, a.reps)
        cell = lambda k: "%.3f (%.3f .. %.3f)" % (g["med"][k], *g["spread"][k])  # noqa: E731
        lines.append("| %s | %d | %d | %d | %d | %s | %s | %s | %.1f | %s |" % (name, g["counts"][0], g["counts"][1], g["counts"][2], g["placed"],
                     cell("event"), cell("call"), cell("mirror"), g["med"]["mirror"] / g["med"]["call"], "yes" if g["same"] else "NO"))
        print(lines[-1], flush=True)
    if a.stats_csv:
        lines += ["", "Per kernel, from one `rocprofv3 --kernel-trace --stats --output-format csv` run of `--kernels-only` (20 calls on the first graph), microseconds.", "",
                  "| kernel | calls | mean | least | largest |", "|---|---|---|---|---|"]
        for name, calls, mean, lo, hi in stats_rows(a.stats_csv):
            lines.append("| `%s` | %d | %.2f | %.2f | %.2f |" % (name.replace("|", "\\|"), calls, mean, lo, hi))
    if not a.no_value:
        lines += ["", "The start with the chains placed (`multiRobotInitialization`) and without (`rangeAidedInitialization`), seed 7, %d steps, rank 5, the default" % GN,
                  "`min_ranges`: the objective, the range residual sum (`measurementResiduals`), the position RMSE against the ground truth after the",
                  "alignment on all positions (`Problem::compareToReference`), chains by status, and per placed chain the range cost over its stage's",
                  "entries at the identity and at the transform written.", "",
                  "| data set | chains | f(x0) without | f(x0) with | range residual sum without | with | position RMSE without | with | placed | not placed | status 0 / 1 / 2 / 3 / 4 | stage cost: start -> written |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for v in value_rows():
            lines.append("| %s | %d | %.6g | %.6g | %.6g | %.6g | %.4g | %.4g | %d | %d | %s | %s |" % (
                v["name"], v["chains"], v["f_old"], v["f_new"], v["range_old"], v["range_new"], v["rmse_old"], v["rmse_new"], v["placed"], v["refused"],
                " / ".join(str(s) for s in v["status"]), "; ".join("%.4g -> %.4g" % c for c in v["costs"])))
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
