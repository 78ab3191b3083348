"""Time and value of the level order of the chain placement (cora_set_chain_placement_order, cora_place_chains_batched_dev;
include/cora_hip.h).
Time: on the two graphs of tools/place_time.py (10 chains with 10^5 ranges between them; 10^3 chains of 100 poses with 80
ranges each against the first), with 5 Gauss-Newton steps on a resident vector and LEVEL tables: the batched call, the plain
call (cora_place_chains_dev) on the same tables and the host mirror (one thread), alternated in one process, medians of
the wall clock of the call after one warm-up round, and the same bits asserted.  --plain-only times the plain call alone on
the GREEDY tables through cora_set_chain_placement: with CORA_LIB_VARIANT naming another build of the library
(cora_amd/lib/variants/<name>/libcora_hip.so, the parent commit's) that is the parent's column; the run itself starts it
as a child (--parent-variant NAME) beside the same measurement of this build.  --kernels-only runs the batched call on the
10^3-chain graph 20 times, the program of a `rocprofv3 --kernel-trace --stats --output-format csv` run of its own;
--stats-csv adds that run's per-kernel table.  Every step that uses the GPU is a child process under its own time limit;
the first that fails ends the run.
Value: both orders through Problem::multiRobotInitialization on the shipped multi-robot data sets: status per chain, the
stage cost from start to written, the position RMSE (Problem::compareToReference).
Writes the section between the two markers of profiles/chain_placement_levels.md.
python tools/place_levels_time.py [--reps 9] [--out ..] [--parent-variant parent] [--stats-csv x_kernel_stats.csv] [--kernels-only]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import place_time as pt  # noqa: E402
from cora_amd import capi, host  # noqa: E402

BEGIN, END, GN = pt.BEGIN, pt.END, pt.GN
GRAPHS = {"ten": ("10^5 poses in 10 chains, 10^5 ranges between chains", pt.ten_chains, 600),
          "thousand": ("10^3 chains x 100 poses, 80 ranges each against the first", pt.thousand_chains, 600)}


def wall_ms(fn):
    t0 = time.perf_counter()
    res = fn()
    return (time.perf_counter() - t0) * 1e3, res


def step(name, reps, plain_only):
    """One graph in this process: a JSON line of medians and spreads."""
    ctx, X = GRAPHS[name][1]()      # (greedy tables: place_time's)
    d = ctx.d
    if not plain_only:
        ctx.set_chain_placement_order(order=capi.PL_ORDER_LEVELS)
    x = ctx.dev_alloc(d)
    t = dict(plain=[]) if plain_only else dict(batched=[], plain=[], mirror=[])
    same, res = True, None
    for rep in range(reps + 1):
        row = {}
        ctx.upload(X, x)
        ctx.sync()
        row["plain"], res = wall_ms(lambda: ctx.place_chains_dev(x, GN))
        if not plain_only:
            plain = ctx.download(x, d)
            ctx.upload(X, x)
            ctx.sync()
            row["batched"], res = wall_ms(lambda: ctx.place_chains_batched_dev(x, GN))
            got = ctx.download(x, d)
            row["mirror"], Y = pt.mirror_ms(ctx, X)
            same = same and bool(np.array_equal(got.view(np.int64), Y.view(np.int64)) and np.array_equal(got.view(np.int64), plain.view(np.int64)))
        if rep:   # (the first round warms the allocator and the kernels' code objects)
            for k, v in row.items():
                t[k].append(v)
    ctx.dev_free(x)
    out = dict(name=name, counts=ctx.chain_placement_counts(), levels=res.get("levels", res["stages"]), placed=res["placed"], same=same,
               med={k: float(np.median(v)) for k, v in t.items()}, spread={k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()})
    print("RESULT " + json.dumps(out), flush=True)


def child(args, limit, env=None):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise SystemExit("%s ended with %d; nothing more is started\n%s" % (" ".join(args), r.returncode, r.stdout[-2000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def value():
    rows = []
    data = os.path.join(ROOT, "tests", "golden", "datasets")
    for name in ("tiers", "mrclam3b", "mrclam5a", "mrclam6"):
        path = os.path.join(data, name + ".pyfg")
        P = host.Problem.from_pyfg(path)
        P.update()
        P.set_rank(5)
        gt = P.ground_truth(path)
        for order in ("greedy", "levels"):
            x0, info = P.multi_robot_initialization(seed=7, gn_steps=GN, order=order)
            rows.append(dict(name=name, order=order, stages=info["stages"], levels=info["levels"], status=" ".join(str(int(s)) for s in info["status"]),
                             rmse=P.compare(x0, gt, proper=False)["trans_rmse"], range_sum=P.measurement_residuals(x0)["range_sum"],
                             costs="; ".join("%.4g -> %.4g" % (float(a), float(b)) for a, b, s in zip(info["cost_start"], info["cost_final"], info["status"]) if s in (0, 2))))
    print("RESULT " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_placement_levels.md"))
    ap.add_argument("--parent-variant")
    ap.add_argument("--stats-csv")
    ap.add_argument("--step", choices=sorted(GRAPHS))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--value", action="store_true")
    ap.add_argument("--no-value", action="store_true")
    a = ap.parse_args()
    if a.kernels_only:
        ctx, X = pt.thousand_chains()
        ctx.set_chain_placement_order(order=capi.PL_ORDER_LEVELS)
        x = ctx.dev_alloc(ctx.d)
        for _ in range(20):
            ctx.upload(X, x)
            ctx.place_chains_batched_dev(x, GN)
        ctx.dev_free(x)
        return
    if a.step:
        return step(a.step, a.reps, a.plain_only)
    if a.value:
        return value()
    lines = [BEGIN, "", "Level tables, %d Gauss-Newton steps (%d launches per level for the batched call, per stage for the plain one, then 2 of the range rows);"
             % (GN, 2 * (GN + 3) + 1), "the three alternated in one process, wall clock of the call, medians after one warm-up round (least .. largest), milliseconds.", "",
             "| graph | stages | levels | entries | chunks | batched | plain, same tables | host mirror, one thread | plain / batched | mirror / batched | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    cell = lambda g, k: "%.3f (%.3f .. %.3f)" % (g["med"][k], *g["spread"][k])  # noqa: E731
    parent_lines = []
    for name in ("ten", "thousand"):
        g = child(["--step", name, "--reps", str(a.reps)], GRAPHS[name][2])
        lines.append("| %s | %d | %d | %d | %d | %s | %s | %s | %.1f | %.1f | %s |" % (
            GRAPHS[name][0], g["counts"][0], g["levels"], g["counts"][1], g["counts"][2], cell(g, "batched"), cell(g, "plain"), cell(g, "mirror"),
            g["med"]["plain"] / g["med"]["batched"], g["med"]["mirror"] / g["med"]["batched"], "yes" if g["same"] else "NO"))
        print(lines[-1], flush=True)
        if a.parent_variant:
            here = child(["--step", name, "--reps", str(a.reps), "--plain-only"], GRAPHS[name][2])
            there = child(["--step", name, "--reps", str(a.reps), "--plain-only"], GRAPHS[name][2], env={"CORA_LIB_VARIANT": a.parent_variant})
            parent_lines.append("| %s | %d | %s | %s |" % (GRAPHS[name][0], here["counts"][0], cell(here, "plain"), cell(there, "plain")))
            print(parent_lines[-1], flush=True)
    if parent_lines:
        lines += ["", "The plain call on the greedy tables (`cora_set_chain_placement`), this build and the parent commit's (`CORA_LIB_VARIANT`), a process each.", "",
                  "| graph | stages | plain call, this build | plain call, parent |", "|---|---|---|---|"] + parent_lines
    if a.stats_csv:
        lines += ["", "Per kernel, from one `rocprofv3 --kernel-trace --stats --output-format csv` run of `--kernels-only` (20 batched calls on the 10^3-chain graph: one level), microseconds.",
                  "", "| kernel | calls | mean | least | largest |", "|---|---|---|---|---|"]
        total = 0.0
        for name, calls, mean, lo, hi in pt.stats_rows(a.stats_csv):
            lines.append("| `%s` | %d | %.2f | %.2f | %.2f |" % (name.replace("|", "\\|"), calls, mean, lo, hi))
            total += calls * mean
        lines += ["", "Sum of the kernels' times per call: %.3f ms." % (total / 20 * 1e-3)]
    if not a.no_value:
        lines += ["", "Both orders through `multiRobotInitialization`, seed 7, %d steps, rank 5, the default `min_ranges`: status per chain, the range cost of every" % GN,
                  "stage over its own entries at the identity and at the transform written, the range residual sum and the position RMSE of the start", "(`Problem::compareToReference`).", "",
                  "| data set | order | stages | levels | status per chain | stage cost: start -> written | range residual sum | position RMSE |", "|---|---|---|---|---|---|---|---|"]
        for v in child(["--value"], 600):
            lines.append("| %s | %s | %d | %d | %s | %s | %.6g | %.4g |" % (v["name"], v["order"], v["stages"], v["levels"], v["status"], v["costs"], v["range_sum"], v["rmse"]))
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
