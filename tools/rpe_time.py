"""Time of the relative pose error on the benchmark's synthetic graph: cora_rpe_dev on two resident vectors with the
per-pair arrays read back, with the six statistics only (wall clock around the call, which ends in a stream
synchronisation), and the handle's event timer around the same call, beside what a caller had to do before it existed --
cora_download of the estimate and the same definitions in numpy float64 (the reference stays on the host).  Every
repetition does all of them in turn and the medians are reported, so drift of the machine hits them alike.  Pairs: the
steps 1, 10 and 100 of the one chain in one table.  Estimate: the ground truth in a random frame of R^k plus 1e-2 noise.
python tools/rpe_time.py [--poses 100000] [--reps 21] [--out profiles/rpe.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cora_amd import capi, host  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the data sheet's figure
HBM_MEASURED = 6.3e12  # what a streaming copy reaches


def numpy_rpe(X, Ref, d, n, r, pairs):
    i, j = pairs[:, 0], pairs[:, 1]
    t = d * n + r

    def motion(V):
        R = V[:d * n].reshape(n, d, -1)
        dx = V[t + j] - V[t + i]
        return np.einsum("mak,mbk->mab", R[i], R[j]), np.einsum("mak,mk->ma", R[i], dx)

    E, u = motion(X)
    S, v = motion(Ref)
    return np.sqrt(((u - v) ** 2).sum(1)), np.sqrt(((E - S) ** 2).sum((1, 2)))


def bytes_read_once(pairs, d, k, kr):
    """The pair table (16 bytes a pair) and every distinct row the pairs touch, once: d rotation rows and one translation
    row per distinct pose, of ld(k) and ld(kr) doubles; plus the two error arrays written (16 bytes a pair)."""
    poses = len(np.unique(pairs))
    ld = lambda c: max(c, 2)  # noqa: E731
    return 16 * len(pairs) + poses * (d + 1) * (ld(k) + ld(kr)) * 8, 16 * len(pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpe.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/rpe_time.py measures on a GPU: none found")
    n = a.poses
    P, truth = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=10, n_ranges=n // 2, seed=42, ground_truth=True)
    P.update()
    dm = P.dims()
    d, r, nt, N = dm["d"], dm["r"], dm["n"] + dm["l"], dm["N"]
    ctx = capi.Context.from_handle(P.context_ptr(), d, dm["n"], r, nt)
    pairs = np.concatenate([P.pose_pairs_by_step(s)[0] for s in (1, 10, 100)])
    m = len(pairs)
    ctx.set_pose_pairs(pairs)
    rng = np.random.default_rng(1)
    k, kr = 5, 3
    B = np.linalg.qr(rng.standard_normal((k, kr)))[0]
    X = truth @ B.T + 1e-2 * rng.standard_normal((N, k))
    X[d * n + r:] += 3.0 * rng.standard_normal(k)
    x, ref = ctx.dev_alloc(k), ctx.dev_alloc(kr)
    ctx.upload(X, x)
    ctx.upload(truth, ref)
    host_out = np.zeros((N, k), order="F")
    t = {key: [] for key in ("arrays", "sums", "event", "download", "numpy")}
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        dev = ctx.rpe_dev(x, k, ref, kr)
        t1 = time.perf_counter()
        ctx.rpe_dev(x, k, ref, kr, arrays=False)
        t2 = time.perf_counter()
        ctx.timer_start()
        ctx.rpe_dev(x, k, ref, kr, arrays=False)
        ev = ctx.timer_stop_ms()
        t3 = time.perf_counter()
        ctx.download(x, k, out=host_out)
        t4 = time.perf_counter()
        et, er = numpy_rpe(host_out, truth, d, n, r, pairs)
        t5 = time.perf_counter()
        if rep:  # (the first round warms the allocator and the kernels' code objects)
            for key, v in (("arrays", t1 - t0), ("sums", t2 - t1), ("event", ev * 1e-3), ("download", t4 - t3), ("numpy", t5 - t4)):
                t[key].append(v * 1e3)
    diff = max(np.abs(dev["trans_err"] - et).max(), np.abs(dev["rot_err"] - er).max())
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % (np.median(v), np.min(v), np.max(v))  # noqa: E731
    rd, wr = bytes_read_once(pairs, d, k, kr)
    ev_s = np.median(t["event"]) * 1e-3
    rate = (rd + wr) / ev_s
    floor_us = (rd + wr) / HBM_MEASURED * 1e6
    bound = ("bandwidth" if rate >= 0.5 * HBM_MEASURED else
             "the latency of its gathers and launches, not by bandwidth (how the time splits between k_rpe and the rest was not traced)")
    lines = [
        "# The relative pose error on the device against download + numpy",
        "",
        "Written by `python tools/rpe_time.py --poses %d --reps %d` on %s (ROCm %s); medians (min .. max) of %d alternated"
        " repetitions after one warm-up round, in milliseconds.  Graph: %d poses, %d landmarks, %d ranges, d = %d, N = %d;"
        " pairs: the steps 1, 10 and 100 in one table, m = %d; (k, kr) = (%d, %d)."
        % (n, a.reps, torch.cuda.get_device_name(0), torch.version.hip, a.reps, dm["n"], dm["l"], r, d, N, m, k, kr),
        "",
        "| what | time |",
        "|---|---|",
        "| `cora_rpe_dev`, per-pair arrays read back (wall clock of the caller) | %s |" % fmt(t["arrays"]),
        "| `cora_rpe_dev`, the six statistics only (wall clock of the caller) | %s |" % fmt(t["sums"]),
        "| the same call between `cora_timer_start` and `cora_timer_stop_ms` (device events) | %s |" % fmt(t["event"]),
        "| `cora_download` of the estimate | %s |" % fmt(t["download"]),
        "| the same definitions in numpy (float64) | %s |" % fmt(t["numpy"]),
        "",
        "Host path / device call with arrays: %.1f x; / statistics only: %.1f x.  Translation RMSE %.6g, rotation RMSE %.6g;"
        " largest difference of a per-pair error between the device and numpy %.2e."
        % ((np.median(t["download"]) + np.median(t["numpy"])) / np.median(t["arrays"]),
           (np.median(t["download"]) + np.median(t["numpy"])) / np.median(t["sums"]),
           np.sqrt(dev["sum_et2"] / m), np.sqrt(dev["sum_er2"] / m), diff),
        "",
        "Bytes the pass must move once: %d read (the pair table, 16 bytes a pair, and every distinct row the pairs touch of"
        " both vectors) and %d written (the two error arrays).  Over the event time that is %.1f GB/s, %.1f %% of the %.1f TB/s a"
        " streaming copy reaches on this part (%.1f %% of the data sheet's %.1f TB/s); at that rate the bytes alone would take %.1f us."
        "  The event time covers one launch of `k_rpe`, three single-block finishing kernels, two small copies and the"
        " synchronisation: the pass is bound by %s."
        % (rd, wr, rate / 1e9, 100 * rate / HBM_MEASURED, HBM_MEASURED / 1e12, 100 * rate / HBM_PEAK, HBM_PEAK / 1e12, floor_us, bound),
        "",
    ]
    text = "\n".join(lines)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    ctx.dev_free(x)
    ctx.dev_free(ref)


if __name__ == "__main__":
    main()
