"""Time of the outlier-robust placement from closures (cora_place_by_closures_robust_dev, include/cora_hip.h) beside the plain
one (cora_place_by_closures_dev) and the host mirrors of both, on identical tables: the handle's event timer around the device
calls on a resident vector, the wall clock of the mirrors (one thread), medians after one warm-up round.  Graphs (those of
tools/closure_time.py): a star of 999 chains with 8 closures each (one stage), a relay of 31 dependent stages, and one pair of
chains with 4 096 and with 65 536 closures, the quadratic case.  What the robust call takes beyond the plain call is the vote,
the election, one more residual per entry in the masked passes and two more launches per stage.  On the two quadratic graphs,
where the vote is nearly all of that, it is reported as a share of the call and as residual evaluations per second beside what
the vote's arithmetic would allow at the part's fp64 vector rate (an upper estimate of k_cl_vote's time, so a lower one of its
rate); on the star and the relay it is launches, and no rate is given.  Every step
that uses the GPU is a child process of its own under its own time limit; the first that fails ends the run.  Writes the
section between the two markers of profiles/closure_consensus.md.
python tools/closure_consensus_time.py [--reps 5] [--out profiles/closure_consensus.md]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from closure_time import chains_graph  # noqa: E402

BEGIN, END = "<!-- measured:begin -->", "<!-- measured:end -->"
BARC2 = 200.0
# cl_cost_rel<3>, the vote's score of one entry, is 36 fp64 vector instructions (21 fused multiply-adds, 12 subtractions, 2
# products, 1 sum), the compare and the count beside them; the part's fp64 vector peak is 78.6 TFLOP/s, that is 39.3e12
# instruction-lanes a second
PEAK_EVALS = 39.3e12 / 36
QUADRATIC = 1e7   # evaluations from which the vote is the call
GRAPHS = dict(
    star=("star: 999 chains x 8 closures against chain 0", lambda: chains_graph([(0, c) for c in range(1, 1000)], nch=1000), 300),
    relay=("relay: 32 chains on a path, 8 closures per pair (31 stages)", lambda: chains_graph([(c, c + 1) for c in range(31)], nch=32), 300),
    pair4096=("one pair of chains, 4 096 closures", lambda: chains_graph([(0, 1)], nch=2, each=4096), 300),
    pair65536=("one pair of chains, 65 536 closures", lambda: chains_graph([(0, 1)], nch=2, each=65536), 900))


def mirror_ms(ctx, X, robust):
    Y = np.array(X, order="F", copy=True)
    out = (C.c_int64 * 7)()
    p = Y.ctypes.data_as(C.POINTER(C.c_double))
    t0 = time.perf_counter()
    if robust:
        rc = ctx.L.cora_debug_place_by_closures_robust_host(ctx.h, p, Y.shape[0], C.c_double(BARC2), 2, out, *([None] * 8))
    else:
        rc = ctx.L.cora_debug_place_by_closures_host(ctx.h, p, Y.shape[0], out, *([None] * 6))
    assert rc == 0, rc
    return (time.perf_counter() - t0) * 1e3, Y


def time_graph(name, reps):
    ctx, X = GRAPHS[name][1]()
    d = ctx.d
    x = ctx.dev_alloc(d)
    t = dict(robust=[], plain=[])
    got = {}
    for rep in range(reps + 1):
        for key, call in (("plain", ctx.place_by_closures_dev), ("robust", lambda p: ctx.place_by_closures_robust_dev(p, BARC2))):
            ctx.upload(X, x)
            ctx.timer_start()
            res = call(x)
            ev = ctx.timer_stop_ms()
            got[key] = (ctx.download(x, d), res)
            if rep:  # (the first round warms the allocator and the kernels' code objects)
                t[key].append(ev)
    ctx.dev_free(x)
    # the mirrors once each: the robust one is L^2 on one thread
    mp, Yp = mirror_ms(ctx, X, False)
    mr, Yr = mirror_ms(ctx, X, True)
    same = bool(np.array_equal(got["plain"][0].view(np.int64), Yp.view(np.int64)) and np.array_equal(got["robust"][0].view(np.int64), Yr.view(np.int64)))
    assert got["robust"][1]["excluded"] == 0 and got["robust"][1]["no_consensus"] == 0   # (the work is the same either way; the label is not)
    counts = ctx.closure_placement_counts()
    lens = got["robust"][1]["list_len"].astype(np.float64)
    return dict(counts=counts, evals=float(np.sum(lens * lens)), excluded=got["robust"][1]["excluded"], placed=got["robust"][1]["placed"], same=same,
                med={k: float(np.median(v)) for k, v in t.items()}, spread={k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()},
                mirror=dict(plain=mp, robust=mr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closure_consensus.md"))
    ap.add_argument("--only", help="comma-separated graphs (default: all)")
    ap.add_argument("--step", help="(internal) run one step in this process and print its result as JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(time_graph(a.step, a.reps)))
        return
    got = {}
    for name in (a.only.split(",") if a.only else GRAPHS):
        r = subprocess.run(["timeout", "-k", "10", str(GRAPHS[name][2]), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps)],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:   # nothing more is started on the GPU after a step that failed
            raise SystemExit("step %s ended with status %d\n%s" % (name, r.returncode, r.stdout[-2000:]))
        got[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(name, got[name], flush=True)
    lines = [BEGIN, "", "GPU.  Event-timed device calls on a resident vector, medians of the repetitions after one warm-up round (least .. largest in",
             "brackets); the mirrors once each, one thread, wall clock; milliseconds.  d = 3, barc2 = %g, every closure an inlier (checked: none" % BARC2,
             "excluded).  Beyond plain: the robust call's time beyond the plain call's (vote, election, the masked passes' extra residual, two",
             "more launches per stage) as a share of the robust call.  On the quadratic graphs that is the vote, given as residual evaluations",
             "(sum of L^2 over the lists) per second; the 36 fp64 instructions of one evaluation at the 78.6 TFLOP/s fp64 vector peak would",
             "allow %.3g a second." % PEAK_EVALS, "",
             "| graph | stages | entries | excluded | evaluations | robust, device | plain, device | robust mirror | plain mirror | beyond plain | evaluations / s | of the arithmetic's bound | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, g in got.items():
        cell = lambda k: "%.3f (%.3f .. %.3f)" % (g["med"][k], *g["spread"][k])  # noqa: E731
        vote = max(g["med"]["robust"] - g["med"]["plain"], 1e-9)
        rate = g["evals"] / (vote * 1e-3)
        quad = g["evals"] >= QUADRATIC
        lines.append("| %s | %d | %d | %d | %.4g | %s | %s | %.2f | %.2f | %.0f %% | %s | %s | %s |" % (
            GRAPHS[name][0], g["counts"][0], g["counts"][1], g["excluded"], g["evals"], cell("robust"), cell("plain"), g["mirror"]["robust"],
            g["mirror"]["plain"], 100 * vote / g["med"]["robust"], "%.3g" % rate if quad else "(launches)",
            "%.1f %%" % (100 * rate / PEAK_EVALS) if quad else "", "yes" if g["same"] else "NO"))
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
