"""Time of the placement from inter-chain relative-pose edges (cora_place_by_closures_dev, include/cora_hip.h): the device call
on a resident vector -- the handle's event timer and the wall clock of the call -- against the host mirror
(cora_debug_place_by_closures_host, one thread, wall clock) in the same run, alternated and reported as medians, on a relay
graph (32 chains of 100 poses on a path, 8 closures per neighbouring pair: 31 dependent stages) and on a star of 10^3 chains of
100 poses with 8 closures per chain against chain 0 (one stage).  Every step that uses the GPU is a child process of its own
under its own time limit; the first that fails ends the run.  Writes the section between the two markers of
profiles/closure_placement.md.
python tools/closure_time.py [--reps 9] [--out profiles/closure_placement.md]"""
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
from cora_amd import capi  # noqa: E402

BEGIN, END = "<!-- measured:begin -->", "<!-- measured:end -->"
LIMITS = dict(relay=300, star=300)   # seconds per step


def chains_graph(pairs, device=0, nch=1000, per=100, each=8, d=3, seed=5, noise=0.02):
    """(ctx, X): nch chains of `per` poses (identity rotations, random walks in one world frame), every chain after the first
    held in a frame of its own; `each` closures (both directions, the table shuffled) per pair of chains of `pairs`."""
    rng = np.random.default_rng(seed)
    n = nch * per
    world = (20 * rng.uniform(-1, 1, (nch, 1, d)) + np.cumsum(rng.normal(0, 1, (nch, per, d)), axis=1)).reshape(n, d)
    t0 = d * n
    N = t0 + n
    X = np.zeros((N, d), order="F")
    rot = np.tile(np.eye(d), (nch, 1, 1))
    own = world.copy()
    for c in range(1, nch):
        th = rng.uniform(-2.5, 2.5)
        Rc = np.eye(d)
        Rc[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        own[c * per:(c + 1) * per] = (world[c * per:(c + 1) * per] - 10 * rng.uniform(-1, 1, d)) @ Rc   # R^T (x - t)
        rot[c] = Rc.T                                                                                  # the chain's poses: R^T I
    for i in range(n):
        X[d * i:d * i + d] = rot[i // per].T
    X[t0:t0 + n] = own
    heads = np.arange(n).reshape(nch, per)[:, :-1].reshape(-1)
    er = np.stack([d * heads, d * (heads + 1), t0 + heads, t0 + heads + 1], axis=1).astype(np.int32)
    ed = np.zeros((len(heads), d * d + d + 2))
    ed[:, :d * d] = np.eye(d).reshape(-1)
    ed[:, d * d:d * d + d] = np.einsum("nij,nj->ni", rot[heads // per].transpose(0, 2, 1), own[heads + 1] - own[heads])
    ed[:, d * d + d:] = 1.0
    pairs = np.repeat(np.asarray(pairs, dtype=np.int64), each, axis=0)
    flip = rng.integers(0, 2, len(pairs)).astype(bool)
    pairs[flip] = pairs[flip][:, ::-1]
    a, b = (pairs[:, k] * per + rng.integers(0, per, len(pairs)) for k in (0, 1))
    cr = np.stack([d * a, d * b, t0 + a, t0 + b], axis=1).astype(np.int32)
    cd = np.zeros((len(a), d * d + d + 2))
    cd[:, :d * d] = np.eye(d).reshape(-1)                                                   # (world rotations are the identity)
    cd[:, d * d:d * d + d] = world[b] - world[a] + noise * rng.normal(0, 1, (len(a), d))
    cd[:, d * d + d:] = 1.0
    order = rng.permutation(len(a))
    er, ed = np.concatenate([er, cr[order]]), np.concatenate([ed, cd[order]])
    ctx = capi.Context(d, n, 0, n, np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32), np.ones(N), device=device)
    ctx.set_measurements(er, ed, np.zeros((0, 3), dtype=np.int32), np.zeros((0, 2)))
    edges = np.arange(len(heads)).reshape(nch, per - 1)
    ctx.set_odometry_chains([edges[c] for c in range(nch)])
    ctx.set_closure_placement()
    return ctx, X


def relay(device=0):
    return chains_graph([(c, c + 1) for c in range(31)], device=device, nch=32)


def star(device=0):
    return chains_graph([(0, c) for c in range(1, 1000)], device=device, nch=1000)


def mirror_ms(ctx, X):
    """Wall clock of the host mirror alone (the C call on a prepared copy)."""
    Y = np.array(X, order="F", copy=True)
    out = (C.c_int64 * 5)()
    t0 = time.perf_counter()
    rc = ctx.L.cora_debug_place_by_closures_host(ctx.h, Y.ctypes.data_as(C.POINTER(C.c_double)), Y.shape[0], out, *([None] * 6))
    t1 = time.perf_counter()
    assert rc == 0, rc
    return (t1 - t0) * 1e3, Y


def time_graph(make, reps):
    ctx, X = make()
    d = ctx.d
    x = ctx.dev_alloc(d)
    t = dict(event=[], call=[], mirror=[])
    res = same = None
    for rep in range(reps + 1):
        ctx.upload(X, x)
        ctx.sync()
        a0 = time.perf_counter()
        res = ctx.place_by_closures_dev(x)
        a1 = time.perf_counter()
        got = ctx.download(x, d)
        ctx.upload(X, x)
        ctx.timer_start()
        ctx.place_by_closures_dev(x)
        ev = ctx.timer_stop_ms()
        mm, Y = mirror_ms(ctx, X)
        same = bool(np.array_equal(got.view(np.int64), Y.view(np.int64)))
        if rep:  # (the first round warms the allocator and the kernels' code objects)
            t["event"].append(ev)
            t["call"].append((a1 - a0) * 1e3)
            t["mirror"].append(mm)
    ctx.dev_free(x)
    counts = ctx.closure_placement_counts()
    # (the range rows: the rows' kernel and the count's; without range measurements the count's alone)
    return dict(counts=counts, launches=5 * counts[0] + (2 if ctx.measurement_counts()[1] else 1), placed=res["placed"], refused=res["refused"], same=same,
                med={k: float(np.median(v)) for k, v in t.items()}, spread={k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closure_placement.md"))
    ap.add_argument("--step", help="(internal) run one step in this process and print its result as JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(time_graph(relay if a.step == "relay" else star, a.reps)))
        return
    got = {}
    for name in ("relay", "star"):
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps)],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:   # nothing more is started on the GPU after a step that failed
            raise SystemExit("step %s ended with status %d\n%s" % (name, r.returncode, r.stdout[-2000:]))
        got[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(name, got[name], flush=True)
    lines = [BEGIN, "", "GPU.  Device call against the host mirror, alternated in one run; medians of the repetitions after one warm-up round (least ..",
             "largest in brackets), milliseconds.  Launches: 5 per stage, 2 of the range rows (1 on a graph without range measurements, as these).", "",
             "| graph | stages | launches | entries | chunks | chains placed | device, events | device, wall clock of the call | per launch (events) | host mirror, one thread | mirror / device (wall) | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, label in (("relay", "relay: 32 chains x 100 poses on a path, 8 closures per pair"),
                        ("star", "star: 10^3 chains x 100 poses, 8 closures per chain against chain 0")):
        g = got[name]
        cell = lambda k: "%.3f (%.3f .. %.3f)" % (g["med"][k], *g["spread"][k])  # noqa: E731
        lines.append("| %s | %d | %d | %d | %d | %d | %s | %s | %.4f | %s | %.1f | %s |" % (
            label, g["counts"][0], g["launches"], g["counts"][1], g["counts"][2], g["placed"], cell("event"), cell("call"),
            g["med"]["event"] / g["launches"], cell("mirror"), g["med"]["mirror"] / g["med"]["call"], "yes" if g["same"] else "NO"))
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
