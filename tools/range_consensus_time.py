"""Time of the outlier-robust multilateration (cora_multilaterate_robust_dev, include/cora_hip.h) beside the plain one
(cora_multilaterate_dev) on identical tables: the handle's event timer around the device calls on a resident vector, medians
after one warm-up round, the two calls alternated.  Graphs (those of tools/multilat_time.py, d = 3, 5 Gauss-Newton steps): the
benchmark's hub, 10 lists of 5 000 ranges (2.5e8 scores: the vote is the call), and a comb of 10^4 lists of 8 (64 scores per
list: the robust call is the plain one plus two launches and one more residual per entry in the masked passes).  The threshold
is one nothing exceeds (the ranges are as generated: every entry is an inlier, checked), so that both calls fit the same entries;
the vote's work does not depend on it.  On the hub the vote is also given as scores per second beside what its arithmetic would
allow at the part's fp64 vector rate.  --plain-only times the plain call alone: with CORA_LIB_VARIANT naming another build of the
library (cora_amd/lib/variants/<name>/libcora_hip.so, e.g. the parent commit's) that is the column the robust call is compared
with.  --kernels-only runs the hub's robust call 20 times for a kernel trace of its own.  Every step that uses the GPU is a
child process of its own under its own time limit; the first that fails ends the run.  Writes the section between the two markers
of profiles/range_consensus.md.
python tools/range_consensus_time.py [--reps 20] [--out profiles/range_consensus.md] [--plain-only] [--kernels-only]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from multilat_time import GN, hub_graph, wide_graph  # noqa: E402

BEGIN, END = "<!-- measured:begin -->", "<!-- measured:end -->"
BARC2 = 1e300
# ml_cost_at<3>, the vote's score of one entry, is 9 fp64 vector instructions (3 subtractions, 3 fused multiply-adds, the
# difference to the range, 2 products) and one square root, the compare and the count beside them; the part's fp64 vector peak
# is 78.6 TFLOP/s, that is 39.3e12 instruction-lanes a second
PEAK_SCORES = 39.3e12 / 9
GRAPHS = dict(hub=("10^5 poses, 10 landmarks, 5 10^4 ranges (hub)", hub_graph, 600), comb=("10^4 landmarks x 8 ranges (comb)", wide_graph, 300))


def time_graph(name, reps, plain_only):
    ctx, X, keep = GRAPHS[name][1]()
    d = ctx.d
    x = ctx.dev_alloc(d)
    calls = [("plain", lambda p: ctx.multilaterate_dev(p, GN))]
    if not plain_only:
        calls.append(("robust", lambda p: ctx.multilaterate_robust_dev(p, BARC2, GN, min_consensus=1)))
    t = {k: [] for k, _ in calls}
    got = {}
    for rep in range(reps + 1):
        for key, call in calls:
            ctx.upload(X, x)
            ctx.timer_start()
            res = call(x)
            ev = ctx.timer_stop_ms()
            got[key] = (ctx.download(x, d), res)
            if rep:  # (the first round warms the allocator and the kernels' code objects)
                t[key].append(ev)
    ctx.dev_free(x)
    out = dict(counts=ctx.multilateration_counts(), med={k: float(np.median(v)) for k, v in t.items()},
               spread={k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}, solved=int(got["plain"][1]["solved"]))
    if not plain_only:
        r = got["robust"][1]
        voted = r["elected"] >= 0
        assert r["excluded"] == 0 and np.array_equal(r["consensus"][voted], r["list_len"][voted])   # every entry an inlier
        lens = r["list_len"][voted].astype(np.float64)
        out.update(scores=float(np.sum(lens * lens)), no_consensus=int(r["no_consensus"]),
                   same=bool(np.array_equal(got["plain"][0].view(np.int64), got["robust"][0].view(np.int64))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_consensus.md"))
    ap.add_argument("--only", help="comma-separated graphs (default: all)")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--step", help="(internal) run one step in this process and print its result as JSON")
    a = ap.parse_args()
    if a.kernels_only:
        ctx, X, keep = hub_graph()
        x = ctx.dev_alloc(ctx.d)
        for _ in range(20):
            ctx.upload(X, x)
            ctx.multilaterate_robust_dev(x, BARC2, GN, min_consensus=1)
        ctx.dev_free(x)
        return
    if a.step:
        print("RESULT " + json.dumps(time_graph(a.step, a.reps, a.plain_only)))
        return
    got = {}
    for name in (a.only.split(",") if a.only else GRAPHS):
        cmd = ["timeout", "-k", "10", str(GRAPHS[name][2]), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps)]
        r = subprocess.run(cmd + (["--plain-only"] if a.plain_only else []), stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:   # nothing more is started on the GPU after a step that failed
            raise SystemExit("step %s ended with status %d\n%s" % (name, r.returncode, r.stdout[-2000:]))
        got[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(name, got[name], flush=True)
    if a.plain_only:
        return
    lines = [BEGIN, "", "GPU.  Event-timed device calls on a resident vector, medians of %d calls after one warm-up round (least .. largest in" % a.reps,
             "brackets), the two calls alternated; milliseconds.  d = 3, %d Gauss-Newton steps, every entry an inlier (checked: none" % GN,
             "excluded, so both calls have the same bits).  Beyond plain: the robust call's time beyond the plain call's (vote, election, the",
             "masked passes' extra residual, two more launches) as a share of the robust call.  Scores: the sum of L^2 over the lists; the 9",
             "fp64 instructions of one score at the 78.6 TFLOP/s fp64 vector peak would allow %.3g a second." % PEAK_SCORES, "",
             "| graph | lists | entries | chunks | scores | robust | plain | robust / plain | beyond plain | scores / s | of the arithmetic's bound | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, g in got.items():
        cell = lambda k: "%.3f (%.3f .. %.3f)" % (g["med"][k], *g["spread"][k])  # noqa: E731
        vote = max(g["med"]["robust"] - g["med"]["plain"], 1e-9)
        rate = g["scores"] / (vote * 1e-3)
        quad = g["scores"] >= 1e7
        lines.append("| %s | %d | %d | %d | %.4g | %s | %s | %.2f | %.0f %% | %s | %s | %s |" % (
            GRAPHS[name][0], g["counts"][0], g["counts"][1], g["counts"][3], g["scores"], cell("robust"), cell("plain"),
            g["med"]["robust"] / g["med"]["plain"], 100 * vote / g["med"]["robust"], "%.3g" % rate if quad else "(launches)",
            "%.1f %%" % (100 * rate / PEAK_SCORES) if quad else "", "yes" if g["same"] else "NO"))
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
