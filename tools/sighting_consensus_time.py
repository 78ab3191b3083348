"""Time of the outlier-robust placement from sightings (cora_place_by_sightings_robust_dev, include/cora_hip.h) beside the plain
one (cora_place_by_sightings_dev) and the host mirrors of both, on identical tables: the handle's event timer around the device
calls on a resident vector, the wall clock of the mirrors (one thread), medians after one warm-up round.  Graphs: a star of
999 chains with 40 sightings each of 16 landmarks (three stages, 999 lists side by side), a relay of 24 chains through landmark
groups that only the chain before places (48 dependent stages of short lists: launches), and one moving chain with 4 096 and
with 65 536 sightings, the quadratic case.  What the robust call takes beyond the plain call is the hypotheses, the vote, the
election, one more residual per entry in the masked passes and two (L-stage, REFIT) or three (C-stage) more launches per
stage.  On the quadratic graphs, where the vote is nearly all of that, it is reported as a share of the call and as residual
evaluations per second beside what the vote's arithmetic would allow at the part's fp64 vector rate (an upper estimate of the
vote kernels' time, so a lower one of their rate); on the star and the relay it is launches, and no rate is given.  Every step
that uses the GPU is a child process of its own under its own time limit; the first that fails ends the run.  Writes the
section between the two markers of profiles/sighting_consensus.md.
python tools/sighting_consensus_time.py [--reps 5] [--out profiles/sighting_consensus.md]"""
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
from cora_amd import capi  # noqa: E402
from sighting_time import thousand_chains  # noqa: E402

BEGIN, END = "<!-- measured:begin -->", "<!-- measured:end -->"
BARC2 = 1e-8
# sg_cost_rel<3>, the vote's score of one entry of a chain list, is 16 fp64 vector instructions (12 fused multiply-adds, 3
# subtractions, 1 product), the compare and the count beside them (a landmark list's: 7); the part's fp64 vector peak is
# 78.6 TFLOP/s, that is 39.3e12 instruction-lanes a second
PEAK_EVALS = 39.3e12 / 16
QUADRATIC = 1e7      # evaluations from which the vote is the call
MIRROR_MAX = 2e8     # evaluations up to which the robust mirror (one thread) is run beside the device


def relay_chains(device=0, nch=24, per=20, group=8, each=24, d=3, seed=9):
    """(ctx, X): nch chains of `per` poses (identity rotations in the world), every chain after the first in a frame of its own.
    Chain c sights the landmark groups c and c + 1 (`group` landmarks each, `each` sightings of either): chain 0 is fixed, its
    L-stage sets groups 0 and 1, chain 1 is aligned onto group 1, its L-stage sets group 2, and so on: two stages per chain."""
    rng = np.random.default_rng(seed)
    n, nl = nch * per, group * (nch + 1)
    world = (20 * rng.uniform(-1, 1, (nch, 1, d)) + np.cumsum(rng.normal(0, 1, (nch, per, d)), axis=1)).reshape(n, d)
    lm = 30 * rng.uniform(-1, 1, (nl, d))
    t0 = d * n
    N = t0 + n + nl
    X = np.zeros((N, d), order="F")
    own, rot = world.copy(), np.tile(np.eye(d), (nch, 1, 1))
    for c in range(1, nch):
        th = rng.uniform(-2.5, 2.5)
        Rc = np.eye(d)
        Rc[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        own[c * per:(c + 1) * per] = (world[c * per:(c + 1) * per] - 10 * rng.uniform(-1, 1, d)) @ Rc
        rot[c] = Rc.T
    for i in range(n):
        X[d * i:d * i + d] = rot[i // per].T
    X[t0:t0 + n] = own
    X[t0 + n:] = 10 * rng.uniform(-1, 1, (nl, d))
    heads = np.arange(n).reshape(nch, per)[:, :-1].reshape(-1)
    er = np.stack([d * heads, d * (heads + 1), t0 + heads, t0 + heads + 1], axis=1).astype(np.int32)
    ed = np.zeros((len(heads), d * d + d + 2))
    ed[:, :d * d] = np.eye(d).reshape(-1)
    ed[:, d * d:d * d + d] = np.einsum("nij,nj->ni", rot[heads // per].transpose(0, 2, 1), own[heads + 1] - own[heads])
    ed[:, d * d + d:] = 1.0
    pose = np.repeat(np.arange(nch), 2 * each) * per + rng.integers(0, per, nch * 2 * each)
    which = (np.repeat(np.arange(nch), 2 * each) * group + np.tile(np.arange(2 * each) % (2 * group), nch))
    sr = np.stack([d * pose, -np.ones_like(pose), t0 + pose, t0 + n + which], axis=1).astype(np.int32)
    sd = np.zeros((len(pose), d * d + d + 2))
    sd[:, d * d:d * d + d] = lm[which] - world[pose]
    sd[:, d * d + d + 1] = 1.0
    order = rng.permutation(len(pose))
    er, ed = np.concatenate([er, sr[order]]), np.concatenate([ed, sd[order]])
    ctx = capi.Context(d, n, 0, n + nl, np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32), np.ones(N), device=device)
    ctx.set_measurements(er, ed, np.zeros((0, 3), dtype=np.int32), np.zeros((0, 2)))
    edges = np.arange(len(heads)).reshape(nch, per - 1)
    ctx.set_odometry_chains([edges[c] for c in range(nch)])
    ctx.set_sighting_placement()
    return ctx, X


GRAPHS = dict(
    star=("star: 999 chains x 40 sightings of 16 landmarks", lambda: thousand_chains(noise=0.0), 300),
    relay=("relay: 24 chains through landmark groups, 48 sightings each (48 stages)", relay_chains, 300),
    one4096=("one moving chain, 4 096 sightings", lambda: thousand_chains(nch=2, each=4096, noise=0.0), 300),
    one65536=("one moving chain, 65 536 sightings", lambda: thousand_chains(nch=2, each=65536, noise=0.0), 900))


def mirror_ms(ctx, X, robust):
    Y = np.array(X, order="F", copy=True)
    out = (C.c_int64 * 10)()
    p = Y.ctypes.data_as(C.POINTER(C.c_double))
    t0 = time.perf_counter()
    if robust:
        rc = ctx.L.cora_debug_place_by_sightings_robust_host(ctx.h, p, Y.shape[0], C.c_double(BARC2), ctx.d + 1, 1, out, *([None] * 14))
    else:
        rc = ctx.L.cora_debug_place_by_sightings_host(ctx.h, p, Y.shape[0], out, *([None] * 8))
    assert rc == 0, rc
    return (time.perf_counter() - t0) * 1e3, Y


def time_graph(name, reps):
    ctx, X = GRAPHS[name][1]()
    d = ctx.d
    x = ctx.dev_alloc(d)
    t = dict(robust=[], plain=[])
    got = {}
    for rep in range(reps + 1):
        for key, call in (("plain", ctx.place_by_sightings_dev), ("robust", lambda p: ctx.place_by_sightings_robust_dev(p, BARC2))):
            ctx.upload(X, x)
            ctx.timer_start()
            res = call(x)
            ev = ctx.timer_stop_ms()
            got[key] = (ctx.download(x, d), res)
            if rep:  # (the first round warms the allocator and the kernels' code objects)
                t[key].append(ev)
    ctx.dev_free(x)
    res = got["robust"][1]
    assert res["chain_excluded"] == 0 and res["landmark_excluded"] == 0 and res["chains_no_consensus"] == 0   # (every sighting an inlier)
    # the evaluations of a call: L^2 per list of every stage (the L-stages' lists are not reported: from the order and the REFIT's)
    lens_c, lens_l = res["chain_list_len"].astype(np.float64), res["landmark_list_len"].astype(np.float64)
    evals = float(np.sum(lens_c * lens_c) + np.sum(lens_l * lens_l))
    mp, Yp = mirror_ms(ctx, X, False)
    same = bool(np.array_equal(got["plain"][0].view(np.int64), Yp.view(np.int64)))
    mr = None
    if evals <= MIRROR_MAX:   # (the robust mirror is L^2 on one thread)
        mr, Yr = mirror_ms(ctx, X, True)
        same = same and bool(np.array_equal(got["robust"][0].view(np.int64), Yr.view(np.int64)))
    return dict(counts=ctx.sighting_placement_counts(), evals=evals, placed=res["placed"], same=same, robust_checked=mr is not None,
                med={k: float(np.median(v)) for k, v in t.items()}, spread={k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()},
                mirror=dict(plain=mp, robust=mr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sighting_consensus.md"))
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
             "brackets); the mirrors once each, one thread, wall clock (the robust mirror only up to %.0e evaluations); milliseconds.  d = 3," % MIRROR_MAX,
             "barc2 = %g, exact sightings, every sighting an inlier (checked: none excluded).  Beyond plain: the robust call's time beyond the" % BARC2,
             "plain call's as a share of the robust call.  Evaluations: the sum of L^2 over the C-stages' and the REFIT's lists (the L-stages'",
             "come on top).  On the quadratic graphs the time beyond plain is the vote, given as evaluations per second; the 16 fp64",
             "instructions of one chain evaluation at the 78.6 TFLOP/s fp64 vector peak would allow %.3g a second." % PEAK_EVALS, "",
             "| graph | stages | entries | evaluations | robust, device | plain, device | robust mirror | plain mirror | beyond plain | evaluations / s | of the arithmetic's bound | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, g in got.items():
        cell = lambda k: "%.3f (%.3f .. %.3f)" % (g["med"][k], *g["spread"][k])  # noqa: E731
        vote = max(g["med"]["robust"] - g["med"]["plain"], 1e-9)
        rate = g["evals"] / (vote * 1e-3)
        quad = g["evals"] >= QUADRATIC
        lines.append("| %s | %d | %d | %.4g | %s | %s | %s | %.2f | %.0f %% | %s | %s | %s |" % (
            GRAPHS[name][0], g["counts"][0], g["counts"][1], g["evals"], cell("robust"), cell("plain"),
            "%.2f" % g["mirror"]["robust"] if g["robust_checked"] else "not run", g["mirror"]["plain"], 100 * vote / g["med"]["robust"],
            "%.3g" % rate if quad else "(launches)", "%.1f %%" % (100 * rate / PEAK_EVALS) if quad else "",
            ("yes" if g["robust_checked"] else "plain only: yes") if g["same"] else "NO"))
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
