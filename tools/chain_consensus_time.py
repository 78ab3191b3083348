"""Time of the outlier-robust chain placement (cora_place_chains_robust_dev, include/cora_hip.h) beside the batched one
(cora_place_chains_batched_dev) on identical LEVEL tables: the handle's event timer around the device calls on a resident
vector, medians after one warm-up round, the two calls alternated.  Graphs (d = 3, 5 Gauss-Newton steps): the star of
tools/place_time.py, 10^3 chains of 100 poses with 80 ranges each against the first (one level of 999 lists of 80: 6.4e6 scores,
the call is its launches), and 5 chains of 2 000 poses with 4 000 ranges each against the first (one level of 4 lists of 4 000:
6.4e7 scores and 16 000 hypotheses, the vote is the call).  The threshold is one nothing exceeds (the ranges are as generated:
every entry is an inlier, checked), so that both calls fit the same entries and have the same bits; the vote's work does not
depend on it.  --plain-only times the batched call alone: with CORA_LIB_VARIANT naming another build of the library
(cora_amd/lib/variants/<name>/libcora_hip.so, the parent commit's) that is the column the robust call is compared with; the run
itself starts it as a child (--parent-variant NAME) beside the same measurement of this build.  --kernels-only GRAPH runs the
robust call 20 times, the program of a `rocprofv3 --kernel-trace --stats --output-format csv` run of its own; --stats-csv
GRAPH=FILE adds that run's per-kernel table.  Every step that uses the GPU is a child process of its own under its own time
limit; the first that fails ends the run.  Writes the section between the two markers of profiles/chain_consensus.md.
python tools/chain_consensus_time.py [--reps 20] [--out ..] [--parent-variant parent] [--stats-csv star=x.csv] [--kernels-only star]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_time as pt  # noqa: E402
from cora_amd import capi  # noqa: E402

BEGIN, END, GN = pt.BEGIN, pt.END, pt.GN
BARC2 = 1e300


def few_long(device=0):
    nch, per, each = 5, 2000, 4000

    def ranges_of(rng):
        c = np.repeat(np.arange(1, nch), each)
        ab = np.stack([c * per + rng.integers(0, per, len(c)), rng.integers(0, per, len(c))], axis=1)
        flip = rng.uniform(0, 1, len(c)) < 0.5
        ab[flip] = ab[flip][:, ::-1]
        return ab[rng.permutation(len(c))]
    return pt.chains_graph(nch, per, ranges_of, device=device)


GRAPHS = dict(star=("10^3 chains x 100 poses, 80 ranges each against the first (star)", pt.thousand_chains, 600),
              long=("5 chains x 2 000 poses, 4 000 ranges each against the first", few_long, 600))


def make(name):
    ctx, X = GRAPHS[name][1]()
    ctx.set_chain_placement_order(order=capi.PL_ORDER_LEVELS)
    return ctx, X


def time_graph(name, reps, plain_only):
    ctx, X = make(name)
    d = ctx.d
    x = ctx.dev_alloc(d)
    calls = [("batched", lambda p: ctx.place_chains_batched_dev(p, GN))]
    if not plain_only:
        calls.append(("robust", lambda p: ctx.place_chains_robust_dev(p, BARC2, GN, min_consensus=1)))
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
    out = dict(counts=ctx.chain_placement_counts(), med={k: float(np.median(v)) for k, v in t.items()},
               spread={k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}, levels=int(got["batched"][1]["levels"]))
    if not plain_only:
        r = got["robust"][1]
        voted = r["elected"] >= 0
        assert r["excluded"] == 0 and r["no_consensus"] == 0 and np.array_equal(r["consensus"][voted], r["list_len"][voted])   # every entry an inlier
        lens = r["list_len"][voted].astype(np.float64)
        out.update(scores=float(np.sum(lens * lens)), same=bool(np.array_equal(got["batched"][0].view(np.int64), got["robust"][0].view(np.int64))))
    return out


def child(args, limit, env=None):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:   # nothing more is started on the GPU after a step that failed
        raise SystemExit("%s ended with status %d\n%s" % (" ".join(args), r.returncode, r.stdout[-2000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_consensus.md"))
    ap.add_argument("--only", help="comma-separated graphs (default: all)")
    ap.add_argument("--parent-variant")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--kernels-only", choices=sorted(GRAPHS))
    ap.add_argument("--stats-csv", action="append", default=[], help="GRAPH=FILE")
    ap.add_argument("--step", help="(internal) run one step in this process and print its result as JSON")
    a = ap.parse_args()
    if a.kernels_only:
        ctx, X = make(a.kernels_only)
        x = ctx.dev_alloc(ctx.d)
        for _ in range(20):
            ctx.upload(X, x)
            ctx.place_chains_robust_dev(x, BARC2, GN, min_consensus=1)
        ctx.dev_free(x)
        return
    if a.step:
        print("RESULT " + json.dumps(time_graph(a.step, a.reps, a.plain_only)))
        return
    names = a.only.split(",") if a.only else list(GRAPHS)
    cell = lambda g, k: "%.3f (%.3f .. %.3f)" % (g["med"][k], *g["spread"][k])  # noqa: E731
    lines = [BEGIN, "", "GPU.  Event-timed device calls on a resident vector, medians of %d calls after one warm-up round (least .. largest in" % a.reps,
             "brackets), the two calls alternated; milliseconds.  d = 3, %d Gauss-Newton steps, level tables, every entry an inlier" % GN,
             "(checked: none excluded, so both calls have the same bits).  Beyond batched: the robust call's time beyond the batched call's",
             "(hypotheses, vote, election, the masked passes' extra residual, three more launches per level) as a share of the robust call.", "",
             "| graph | stages | levels | entries | chunks | scores | robust | batched, same tables | robust / batched | beyond batched | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    parent_lines = []
    for name in names:
        g = child(["--step", name, "--reps", str(a.reps)], GRAPHS[name][2])
        lines.append("| %s | %d | %d | %d | %d | %.4g | %s | %s | %.2f | %.0f %% | %s |" % (
            GRAPHS[name][0], g["counts"][0], g["levels"], g["counts"][1], g["counts"][2], g["scores"], cell(g, "robust"), cell(g, "batched"),
            g["med"]["robust"] / g["med"]["batched"], 100 * (g["med"]["robust"] - g["med"]["batched"]) / g["med"]["robust"], "yes" if g["same"] else "NO"))
        print(lines[-1], flush=True)
        if a.parent_variant:
            here = child(["--step", name, "--reps", str(a.reps), "--plain-only"], GRAPHS[name][2])
            there = child(["--step", name, "--reps", str(a.reps), "--plain-only"], GRAPHS[name][2], env={"CORA_LIB_VARIANT": a.parent_variant})
            parent_lines.append("| %s | %s | %s | %s | %.2f |" % (GRAPHS[name][0], cell(g, "robust"), cell(here, "batched"), cell(there, "batched"),
                                                               g["med"]["robust"] / there["med"]["batched"]))
            print(parent_lines[-1], flush=True)
    if parent_lines:
        lines += ["", "The batched call alone, this build and the parent commit's (`CORA_LIB_VARIANT`), a process each, beside the robust call of the table above.", "",
                  "| graph | robust call | batched call, this build | batched call, parent | robust / parent's batched |", "|---|---|---|---|---|"] + parent_lines
    for item in a.stats_csv:
        name, path = item.split("=", 1)
        lines += ["", "Per kernel on `%s`, from one `rocprofv3 --kernel-trace --stats --output-format csv` run of `--kernels-only %s` (20 robust calls), microseconds." % (name, name),
                  "", "| kernel | calls | mean | least | largest | share of the kernels' time |", "|---|---|---|---|---|---|"]
        rows = pt.stats_rows(path)
        total = sum(calls * mean for _, calls, mean, _, _ in rows)
        for kname, calls, mean, lo, hi in rows:
            lines.append("| `%s` | %d | %.2f | %.2f | %.2f | %.1f %% |" % (kname.replace("|", "\\|"), calls, mean, lo, hi, 100 * calls * mean / total))
        lines += ["", "Sum of the kernels' times per call: %.3f ms." % (total / 20 * 1e-3)]
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
