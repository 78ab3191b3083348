"""Time of the trajectory comparison on the benchmark's synthetic graph: cora_compare_dev on two resident vectors (wall
clock around the call, which ends in a stream synchronisation) beside what a caller had to do before it existed --
cora_download of the estimate and the same definitions in numpy (float64: means, centred rows, H, numpy.linalg.svd,
per-pose and per-landmark errors; the reference stays on the host).  Every repetition does both in turn and the medians
are reported, so drift of the machine hits both alike.  Estimate: the ground truth in a random frame plus 1e-2 noise.
python tools/compare_time.py [--poses 100000] [--reps 21] [--out profiles/compare.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cora_amd import capi, host  # noqa: E402


# NOT measured by this command: copied by hand from the output of the runs named in the text, and to be copied again when
# those change.  The generated file says so.
NOTES = """
## The robust case, judged by its distance from the truth

(This section is not produced by the command above.  The figures were copied from the printed output of one run of
`pytest -s -m gpu tests/test_gpu_compare.py` and of the driver on the same machine as the table.)

`tests/test_gpu_compare.py` rebuilds the robust case of `tests/test_gpu_gnc.py` -- `make_graph(d, n=30, n_landmarks=3,
n_ranges=60, n_loops=5)` at the generator's default seed 42, the ranges 3, 11, 19, 27, 42 and 55 made 10.0 longer, range
threshold 25, truncated least squares -- and compares both solutions with `ground_truth(g)` (all 30 poses selected, proper
rotation).  Translation RMSE of the poses, landmark RMSE in brackets:

| d | plain `solve` on the corrupted graph | `solve_robust` |
|---|---|---|
| 2 | 0.742567 (6.68719) | 0.0608807 (0.30916) |
| 3 | 1.35156 (19.1583) | 0.106012 (4.22379) |

The noise-free fixture `small_ra_slam_problem`, solved from `X_gt` and compared with its parsed ground truth, has a
translation RMSE of 9.4e-17 (rotation 2.2e-16, landmarks 3.6e-15).

`cora_main tests/golden/datasets/plaza2.pyfg --evaluate` (random start, as the driver does by default) ends at 4091 poses,
translation RMSE 0.27121 (max 0.626055), rotation RMSE 1.58116 deg (max 8.93564 deg), 4 landmarks at RMSE 0.0460468.
"""


def numpy_compare(X, Ref, d, n, r, nt):
    t = d * n + r + np.arange(nt)
    x, g = X[t[:n]], Ref[t[:n]]
    xbar, gbar = x.mean(0), g.mean(0)
    U, s, Vt = np.linalg.svd((x - xbar).T @ (g - gbar), full_matrices=False)
    A = U @ Vt
    if A.shape[0] == A.shape[1] and np.linalg.det(A) < 0:
        U[:, -1] = -U[:, -1]
        A = U @ Vt
    e = np.linalg.norm((X[t] - xbar) @ A - (Ref[t] - gbar), axis=1)
    er = np.sqrt(((X[:d * n] @ A - Ref[:d * n]) ** 2).sum(1).reshape(n, d).sum(1))
    return e[:n], er, e[n:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare.md"))
    a = ap.parse_args()
    import torch
    n = a.poses
    P, truth = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=10, n_ranges=n // 2, seed=42, ground_truth=True)
    P.update()
    dm = P.dims()
    d, r, nt, N = dm["d"], dm["r"], dm["n"] + dm["l"], dm["N"]
    ctx = capi.Context.from_handle(P.context_ptr(), d, dm["n"], r, nt)
    rng = np.random.default_rng(1)
    rows = []
    for k, kr in ((3, 3), (5, 3)):
        B = np.linalg.qr(rng.standard_normal((k, kr)))[0]
        if k == kr and np.linalg.det(B) < 0:
            B[:, -1] = -B[:, -1]
        X = truth @ B.T + 1e-2 * rng.standard_normal((N, k))
        X[d * n + r:] += 3.0 * rng.standard_normal(k)
        x, ref = ctx.dev_alloc(k), ctx.dev_alloc(kr)
        ctx.upload(X, x)
        ctx.upload(truth, ref)
        host_out = np.zeros((N, k), order="F")
        t_dev, t_host = [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            dev = ctx.compare_dev(x, k, ref, kr, proper=(k == kr))
            t1 = time.perf_counter()
            ctx.download(x, k, out=host_out)
            t2 = time.perf_counter()
            et, er, el = numpy_compare(host_out, truth, d, n, r, nt)
            t3 = time.perf_counter()
            if rep:  # (the first round warms the allocator and the kernels' code objects)
                t_dev.append((t1 - t0) * 1e3)
                t_host.append(((t2 - t1) * 1e3, (t3 - t2) * 1e3))
        diff = max(np.abs(dev["pose_trans_err"] - et).max(), np.abs(dev["pose_rot_err"] - er).max(),
                   np.abs(dev["landmark_err"] - el).max())
        th = np.array(t_host)
        rows.append("| %d | %d | %.3f (%.3f .. %.3f) | %.3f | %.3f | %.1f x | %.6g | %.2e |" % (
            k, kr, np.median(t_dev), np.min(t_dev), np.max(t_dev), np.median(th[:, 0]), np.median(th[:, 1]),
            np.median(th.sum(1)) / np.median(t_dev), np.sqrt(dev["sum_et2"] / dev["m"]), diff))
        ctx.dev_free(x)
        ctx.dev_free(ref)
    lines = [
        "# The trajectory comparison on the device against download + numpy",
        "",
        "Written by `python tools/compare_time.py --poses %d --reps %d` on %s (ROCm %s); medians (min .. max) of %d alternated"
        " repetitions after one warm-up round; wall clock of the calling thread in milliseconds.  Graph: %d poses, %d"
        " landmarks, %d ranges, d = %d, N = %d.  The device call is three kernels, the Gram kernel, three single-block"
        " reductions, one host SVD and two stream synchronisations: bound by latency and launches, not by bandwidth."
        % (n, a.reps, torch.cuda.get_device_name(0), torch.version.hip, a.reps, dm["n"], dm["l"], r, d, N),
        "",
        "| k | kr | `cora_compare_dev` | `cora_download` | numpy (float64) | host path / device | translation RMSE | largest"
        " difference of an error |",
        "|---|---|---|---|---|---|---|---|",
    ] + rows + [""]
    text = "\n".join(lines) + NOTES
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
