"""Time of the rounding to SE(d) on the benchmark's synthetic graph: cora_round_dev on a resident vector (wall clock around
the call, which synchronises twice, and the handle's event timer around the same call) beside what a caller had to do
before it existed -- cora_download of the relaxed point and projectSolution on the host.  Every repetition does all of
them in turn and the medians are reported, so drift of the machine hits them alike.  Input: the ground truth in a random
frame of R^k plus 1e-2 noise, d = 3, k = 5.  Writes the section between the two timing markers of profiles/round.md (the
whole file when it has none).
python tools/round_time.py [--poses 100000] [--reps 21] [--out profiles/round.md]"""
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
BEGIN, END = "<!-- timing:begin -->", "<!-- timing:end -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/round_time.py measures on a GPU: none found")
    n = a.poses
    P, truth = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=10, n_ranges=n // 2, seed=42, ground_truth=True)
    P.update()
    dm = P.dims()
    d, r, nt, N = dm["d"], dm["r"], dm["n"] + dm["l"], dm["N"]
    ctx = capi.Context.from_handle(P.context_ptr(), d, dm["n"], r, nt)
    rng = np.random.default_rng(1)
    k = 5
    B = np.linalg.qr(rng.standard_normal((k, d)))[0]
    Y = truth @ B.T + 1e-2 * rng.standard_normal((N, k))
    P.set_rank(k)
    y, out = ctx.dev_alloc(k), ctx.dev_alloc(d)
    ctx.upload(Y, y)
    host_in = np.zeros((N, k), order="F")
    t = {key: [] for key in ("call", "event", "download", "project")}
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        dev = ctx.round_dev(y, k, out)
        t1 = time.perf_counter()
        ctx.timer_start()
        ctx.round_dev(y, k, out)
        ev = ctx.timer_stop_ms()
        t2 = time.perf_counter()
        ctx.download(y, k, out=host_in)
        t3 = time.perf_counter()
        Xh = P.project_solution(host_in)
        t4 = time.perf_counter()
        if rep:  # (the first round warms the allocator and the kernels' code objects)
            for key, v in (("call", t1 - t0), ("event", ev * 1e-3), ("download", t3 - t2), ("project", t4 - t3)):
                t[key].append(v * 1e3)
    Xd = ctx.download(out, d)
    R = np.linalg.lstsq(Xd, Xh, rcond=None)[0]
    diff = float(np.abs(Xd @ R - Xh).max())
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % (np.median(v), np.min(v), np.max(v))  # noqa: E731
    ld = lambda c: max(c, 2)  # noqa: E731
    rd, wr = 3 * N * ld(k) * 8 - (N - d * n) * ld(k) * 8, N * ld(d) * 8  # Gram + count (pose rows) + apply; one write
    ev_s = np.median(t["event"]) * 1e-3
    rate = (rd + wr) / ev_s
    lines = [
        BEGIN,
        "Written by `python tools/round_time.py --poses %d --reps %d` on %s (ROCm %s); medians (min .. max) of %d alternated"
        " repetitions after one warm-up round, in milliseconds.  Graph: %d poses, %d landmarks, %d ranges, d = %d, N = %d; k = %d."
        % (n, a.reps, torch.cuda.get_device_name(0), torch.version.hip, a.reps, dm["n"], dm["l"], r, d, N, k),
        "",
        "| what | time |",
        "|---|---|",
        "| `cora_round_dev` (wall clock of the caller) | %s |" % fmt(t["call"]),
        "| the same call between `cora_timer_start` and `cora_timer_stop_ms` (device events) | %s |" % fmt(t["event"]),
        "| `cora_download` of the relaxed point | %s |" % fmt(t["download"]),
        "| `projectSolution` on the host | %s |" % fmt(t["project"]),
        "",
        "Host route / device call: %.1f x.  %d of %d pose blocks with a positive determinant, flipped: %s; largest difference"
        " between the two rounded points after the one rotation that relates them: %.2e."
        % ((np.median(t["download"]) + np.median(t["project"])) / np.median(t["call"]), dev["count"], n, dev["flipped"], diff),
        "",
        "Bytes the call moves: %d read (the input three times -- the Gram pass, the pose rows again for the count, every row"
        " for the apply pass) and %d written.  Over the event time that is %.1f GB/s, %.1f %% of the %.1f TB/s a streaming copy"
        " reaches on this part (%.1f %% of the data sheet's %.1f TB/s).  The event time covers the Gram launch and its"
        " reduction, a synchronisation with the k x k eigenproblem on the host, three launches and the final synchronisation:"
        " the call is bound by launches and the host step, not by bandwidth."
        % (rd, wr, rate / 1e9, 100 * rate / HBM_MEASURED, HBM_MEASURED / 1e12, 100 * rate / HBM_PEAK, HBM_PEAK / 1e12),
        END,
    ]
    section = "\n".join(lines)
    text = section + "\n"
    if os.path.exists(a.out):
        old = open(a.out).read()
        if BEGIN in old and END in old:
            text = old[:old.index(BEGIN)] + section + old[old.index(END) + len(END):]
    with open(a.out, "w") as f:
        f.write(text)
    print(section)
    ctx.dev_free(y)
    ctx.dev_free(out)


if __name__ == "__main__":
    main()
