"""Time of the odometry start on the benchmark's synthetic graph at several sizes: getOdomInitialization (the host
function: one thread, pose by pose; wall clock), Problem::odometryInitialization (the same start composed on the device,
end to end: draws, upload of the starts, the scan, the lift and the download of the N x p matrix; wall clock) and
cora_odometry_init_dev alone on a resident vector (the handle's event timer, after warm-up, and the wall clock of the
call).  Every repetition does all of them in turn and the medians are reported, so drift of the machine hits them alike.
Writes the section between the two timing markers of profiles/odom_init.md (the whole file when it has none).
python tools/odom_init_time.py [--poses 10000,100000,1000000] [--reps 7] [--out profiles/odom_init.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cora_amd import capi, host  # noqa: E402

BEGIN, END = "<!-- timing:begin -->", "<!-- timing:end -->"


def measure(n, reps, p=5):
    P = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=10, n_ranges=n // 2, seed=42)
    P.update()
    P.set_rank(p)
    dm = P.dims()
    d, r, nt = dm["d"], dm["r"], dm["n"] + dm["l"]
    t0 = time.perf_counter()
    dev0 = P.op("odometryInitialization")   # installs the measurement table and the chain tables
    first = time.perf_counter() - t0
    ctx = capi.Context.from_handle(P.context_ptr(), d, dm["n"], r, nt)
    chains, positions = ctx.odometry_chains_count()
    rng = np.random.default_rng(1)
    starts = 10 * rng.uniform(-1, 1, (chains, d))
    lms = 10 * rng.uniform(-1, 1, (dm["l"], d))
    x = ctx.dev_alloc(d)
    t = {key: [] for key in ("host", "device", "call", "event")}
    for rep in range(reps + 1):
        a0 = time.perf_counter()
        ref = P.op("getOdomInitialization")
        a1 = time.perf_counter()
        dev = P.op("odometryInitialization")
        a2 = time.perf_counter()
        ctx.odometry_init_dev(starts, lms, x)
        a3 = time.perf_counter()
        ctx.timer_start()
        ctx.odometry_init_dev(starts, lms, x)
        ev = ctx.timer_stop_ms()
        if rep:  # (the first round warms the allocator and the kernels' code objects)
            for key, v in (("host", a1 - a0), ("device", a2 - a1), ("call", a3 - a2), ("event", ev * 1e-3)):
                t[key].append(v * 1e3)
    ctx.dev_free(x)
    scale = np.abs(ref).max()
    return dict(n=n, N=dm["N"], r=r, l=dm["l"], chains=chains, positions=positions, first=first * 1e3,
                diff=float(np.abs(dev - ref).max() / scale), same=bool(np.array_equal(dev, dev0)), t=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", default="10000,100000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "odom_init.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/odom_init_time.py measures on a GPU: none found")
    rows = [measure(int(n), a.reps) for n in a.poses.split(",")]
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % (np.median(v), np.min(v), np.max(v))  # noqa: E731
    lines = [
        BEGIN,
        "Written by `python tools/odom_init_time.py --poses %s --reps %d` on %s (ROCm %s); medians (min .. max) of %d alternated"
        " repetitions after one warm-up round, in milliseconds.  Graphs: the benchmark's generator, d = 3, one chain, 10"
        " landmarks, n / 2 ranges, relaxation rank 5."
        % (a.poses, a.reps, torch.cuda.get_device_name(0), torch.version.hip, a.reps),
        "",
        "| poses | `getOdomInitialization` (host, wall clock) | `odometryInitialization` (device, end to end, wall clock) |"
        " `cora_odometry_init_dev` (wall clock of the call) | the same call between device events | first"
        " `odometryInitialization` (tables installed) | host / device end to end | largest relative difference of the two starts |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for m in rows:
        t = m["t"]
        lines.append("| %d | %s | %s | %s | %s | %.1f | %.2f x | %.2e |"
                     % (m["n"], fmt(t["host"]), fmt(t["device"]), fmt(t["call"]), fmt(t["event"]), m["first"],
                        np.median(t["host"]) / np.median(t["device"]), m["diff"]))
    lines += ["", "Host time per pose: " + ", ".join("%.2f us at %d poses" % (1e3 * np.median(m["t"]["host"]) / m["n"], m["n"]) for m in rows)
              + ".  Two device starts from the same seed have the same bits: %s." % all(m["same"] for m in rows),
              END]
    section = "\n".join(lines)
    text = section + "\n"
    if os.path.exists(a.out):
        old = open(a.out).read()
        if BEGIN in old and END in old:
            text = old[:old.index(BEGIN)] + section + old[old.index(END) + len(END):]
    with open(a.out, "w") as f:
        f.write(text)
    print(section)


if __name__ == "__main__":
    main()
