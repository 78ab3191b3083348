"""Time and value of the placement from pose-landmark sightings (cora_place_by_sightings_dev, include/cora_hip.h).
Time: the device call on a resident vector -- the handle's event timer and the wall clock of the call -- against the host
mirror (cora_debug_place_by_sightings_host, one thread, wall clock) in the same run, alternated and reported as medians, on
mrclam6.pyfg (13 121 sightings, 5 robots, 15 landmarks) and on a synthetic graph of 10^3 chains of 100 poses that all sight the
same 16 landmarks 40 times each.  Value: f(x0) and the landmark RMSE against the ground truth (Problem::compareToReference)
of sightingInitialization against multiRobotInitialization on the three MR.CLAM data sets.
Every step that uses the GPU is a child process of its own under its own time limit; the first that fails ends the run.
Writes the section between the two markers of profiles/sighting_placement.md.
python tools/sighting_time.py [--reps 9] [--out profiles/sighting_placement.md] [--no-value]"""
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
from cora_amd import capi, host  # noqa: E402

BEGIN, END = "<!-- measured:begin -->", "<!-- measured:end -->"
DATA = os.path.join(ROOT, "tests", "golden", "datasets")
LIMITS = dict(mrclam6=300, thousand=300, value=600)   # seconds per step


def thousand_chains(device=0, nch=1000, per=100, nl=16, each=40, d=3, seed=5, noise=0.02):
    """(ctx, X): nch chains of `per` poses (identity rotations, random walks in one world frame), every chain after the first
    held in a frame of its own; every chain sights the same nl landmarks, `each` sightings in all."""
    rng = np.random.default_rng(seed)
    n = nch * per
    world = (20 * rng.uniform(-1, 1, (nch, 1, d)) + np.cumsum(rng.normal(0, 1, (nch, per, d)), axis=1)).reshape(n, d)
    lm = 30 * rng.uniform(-1, 1, (nl, d))
    t0 = d * n
    N = t0 + n + nl
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
    X[t0 + n:] = 10 * rng.uniform(-1, 1, (nl, d))
    heads = np.arange(n).reshape(nch, per)[:, :-1].reshape(-1)
    er = np.stack([d * heads, d * (heads + 1), t0 + heads, t0 + heads + 1], axis=1).astype(np.int32)
    ed = np.zeros((len(heads), d * d + d + 2))
    ed[:, :d * d] = np.eye(d).reshape(-1)
    ed[:, d * d:d * d + d] = np.einsum("nij,nj->ni", rot[heads // per].transpose(0, 2, 1), own[heads + 1] - own[heads])
    ed[:, d * d + d:] = 1.0
    pose = (np.repeat(np.arange(nch), each) * per + rng.integers(0, per, nch * each))
    which = np.tile(np.arange(each) % nl, nch)
    sr = np.stack([d * pose, -np.ones_like(pose), t0 + pose, t0 + n + which], axis=1).astype(np.int32)
    sd = np.zeros((len(pose), d * d + d + 2))
    sd[:, d * d:d * d + d] = lm[which] - world[pose] + noise * rng.normal(0, 1, (len(pose), d))   # (world rotations are the identity)
    sd[:, d * d + d + 1] = 1.0
    order = rng.permutation(len(pose))
    er, ed = np.concatenate([er, sr[order]]), np.concatenate([ed, sd[order]])
    ctx = capi.Context(d, n, 0, n + nl, np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32), np.ones(N), device=device)
    ctx.set_measurements(er, ed, np.zeros((0, 3), dtype=np.int32), np.zeros((0, 2)))
    edges = np.arange(len(heads)).reshape(nch, per - 1)
    ctx.set_odometry_chains([edges[c] for c in range(nch)])
    ctx.set_sighting_placement()
    return ctx, X


def mrclam6(device=0):
    """(ctx, X) of mrclam6.pyfg on the problem's own handle (borrowed), whose measurement, chain and sighting tables one
    sightingInitialization has installed; X: the odometry start with every chain at the origin of its own frame and the
    landmarks at random places."""
    path = os.path.join(DATA, "mrclam6.pyfg")
    P = host.Problem.from_pyfg(path)
    P.update()
    P.set_rank(5)
    P.sighting_initialization(seed=7)
    dm = P.dims()
    d, n, r, N = dm["d"], dm["n"], dm["r"], dm["N"]
    ctx = capi.Context.from_handle(P.context_ptr(), d, n, r, N - d * n - r)
    ctx.problem = P   # (owns the handle)
    nl = N - (d + 1) * n - r
    x = ctx.dev_alloc(d)
    rng = np.random.default_rng(7)
    ctx.odometry_init_dev(np.zeros((ctx.odometry_chains_count()[0], d)), 10 * rng.uniform(-1, 1, (nl, d)), x)
    X = ctx.download(x, d)
    ctx.dev_free(x)
    return ctx, X


def mirror_ms(ctx, X):
    """Wall clock of the host mirror alone (the C call on a prepared copy)."""
    Y = np.array(X, order="F", copy=True)
    out = (C.c_int64 * 6)()
    t0 = time.perf_counter()
    rc = ctx.L.cora_debug_place_by_sightings_host(ctx.h, Y.ctypes.data_as(C.POINTER(C.c_double)), Y.shape[0], out, *([None] * 8))
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
        res = ctx.place_by_sightings_dev(x)
        a1 = time.perf_counter()
        got = ctx.download(x, d)
        ctx.upload(X, x)
        ctx.timer_start()
        ctx.place_by_sightings_dev(x)
        ev = ctx.timer_stop_ms()
        mm, Y = mirror_ms(ctx, X)
        same = bool(np.array_equal(got.view(np.int64), Y.view(np.int64)))
        if rep:  # (the first round warms the allocator and the kernels' code objects)
            t["event"].append(ev)
            t["call"].append((a1 - a0) * 1e3)
            t["mirror"].append(mm)
    ctx.dev_free(x)
    kinds = [k for k, _ in ctx.sighting_placement_order()]
    launches = sum({"L": 2, "C": 5, "REFIT": 4}[k] for k in kinds) + 2
    return dict(counts=ctx.sighting_placement_counts(), kinds=" ".join(kinds), launches=launches, placed=res["placed"],
                landmarks=res["landmarks_placed"], same=same, med={k: float(np.median(v)) for k, v in t.items()},
                spread={k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()})


def value_rows():
    rows = []
    for name in ("mrclam5a", "mrclam3b", "mrclam6"):
        path = os.path.join(DATA, name + ".pyfg")
        P = host.Problem.from_pyfg(path)
        P.update()
        P.set_rank(5)
        gt = P.ground_truth(path)
        old, _ = P.multi_robot_initialization(seed=7)
        new, info = P.sighting_initialization(seed=7)
        co, cn = P.compare(old, gt, proper=False), P.compare(new, gt, proper=False)
        rows.append(dict(name=name, f_old=P.op("evaluateObjective", old), f_new=P.op("evaluateObjective", new), lm_old=co["landmark_rmse"],
                         lm_new=cn["landmark_rmse"], pos_old=co["trans_rmse"], pos_new=cn["trans_rmse"], fixed=info["fixed"], placed=info["placed"],
                         not_placed=info["not_placed"], lm_placed=info["landmarks_placed"], lm_not=info["landmarks_not_placed"],
                         by_ranges=info["chains"]["placed"], stages=info["stages"],
                         sight_old=float(np.sum(P.measurement_residuals(old)["pose_landmark"])),
                         sight_new=float(np.sum(P.measurement_residuals(new)["pose_landmark"]))))
    return rows


def step(name, reps):
    if name == "value":
        return value_rows()
    return time_graph(mrclam6 if name == "mrclam6" else thousand_chains, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sighting_placement.md"))
    ap.add_argument("--no-value", action="store_true")
    ap.add_argument("--step", help="(internal) run one step in this process and print its result as JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.reps)))
        return
    got = {}
    for name in ("mrclam6", "thousand") + (() if a.no_value else ("value",)):
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps)],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:   # nothing more is started on the GPU after a step that failed
            raise SystemExit("step %s ended with status %d\n%s" % (name, r.returncode, r.stdout[-2000:]))
        got[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(name, got[name], flush=True)
    lines = [BEGIN, "", "Device call against the host mirror, alternated in one run; medians of the repetitions after one warm-up round (least ..",
             "largest in brackets), milliseconds.  Launches: 2 per L-stage, 5 per C-stage, 2 + 2 for the REFIT, 2 of the range rows.", "",
             "| graph | stages | launches | entries | chunks | chains placed | landmarks placed | device, events | device, wall clock of the call | host mirror, one thread | mirror / device (wall) | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, label in (("mrclam6", "mrclam6.pyfg"), ("thousand", "10^3 chains x 100 poses, 16 landmarks, 40 sightings per chain")):
        g = got[name]
        cell = lambda k: "%.3f (%.3f .. %.3f)" % (g["med"][k], *g["spread"][k])  # noqa: E731
        lines.append("| %s | %d (%s) | %d | %d | %d | %d | %d | %s | %s | %s | %.1f | %s |" % (
            label, g["counts"][0], g["kinds"], g["launches"], g["counts"][1], g["counts"][2], g["placed"], g["landmarks"], cell("event"), cell("call"),
            cell("mirror"), g["med"]["mirror"] / g["med"]["call"], "yes" if g["same"] else "NO"))
    if "value" in got:
        lines += ["", "The start with the sighting step (`sightingInitialization`) and without (`multiRobotInitialization`), seed 7, rank 5, defaults: the",
                  "objective, the summed sighting cost (`measurementResiduals`, pose-landmark), landmark and position RMSE against the ground truth",
                  "after the alignment on all positions (`Problem::compareToReference`), and what the sighting step and the range placement after it took.", "",
                  "| data set | f(x0) without | f(x0) with | sighting cost without | with | landmark RMSE without | with | position RMSE without | with | chains fixed / placed / not placed | then placed by ranges | landmarks placed / not placed | stages |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for v in got["value"]:
            lines.append("| %s | %.6g | %.6g | %.6g | %.6g | %.4g | %.4g | %.4g | %.4g | %d / %d / %d | %d | %d / %d | %d |" % (
                v["name"], v["f_old"], v["f_new"], v["sight_old"], v["sight_new"], v["lm_old"], v["lm_new"], v["pos_old"], v["pos_new"], v["fixed"],
                v["placed"], v["not_placed"], v["by_ranges"], v["lm_placed"], v["lm_not"], v["stages"]))
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
