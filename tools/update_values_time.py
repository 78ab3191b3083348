"""Time of replacing the values of Q on a live handle (cora_update_values, cora_update_values_dev) on the benchmark's
synthetic graph, beside the alternative without it: destroying the handle and creating it again from the new values.
Every repetition does all of them in turn -- re-create, first update (builds the source map), steady host-pointer update,
device-pointer update -- and the medians are reported, so drift of the machine hits every figure alike.
python tools/update_values_time.py [--poses 100000] [--reps 11] [--out profiles/update_values.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cora_amd import capi, host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--rank", type=int, default=5)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_values.md"))
    a = ap.parse_args()
    import torch
    n, p = a.poses, a.rank
    P = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=10, n_ranges=n // 2, seed=42)
    P.update()
    dm = P.dims()
    _, _, rowptr, colidx, vals = P.matrix("DataMatrix")
    del P
    d, nt = dm["d"], dm["n"] + dm["l"]
    rng = np.random.default_rng(1)
    # a symmetric re-weighting: one factor per unordered pair {i, j}
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    lo, hi = np.minimum(rows, colidx).astype(np.int64), np.maximum(rows, colidx).astype(np.int64)
    key = lo * np.int64(len(rowptr)) + hi
    _, inv = np.unique(key, return_inverse=True)
    versions = [vals * rng.uniform(0.5, 1.5, inv.max() + 1)[inv] for _ in range(2)]
    dev = [torch.from_numpy(v).to("cuda:0") for v in versions]
    torch.cuda.synchronize()

    def create(v):
        c = capi.Context(d, dm["n"], dm["r"], nt, rowptr, colidx, v)
        c.set_rank(p)
        c.sync()
        return c

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    ctx = create(vals)
    stats = ctx.format_stats()
    t = {k: [] for k in ("recreate", "first", "map", "host", "check", "upload", "device", "refresh", "dev", "dev_event")}
    for rep in range(a.reps + 1):
        v, dv = versions[rep & 1], dev[rep & 1]

        def recreate():
            ctx.close()
            return create(v)
        ms, ctx = wall(recreate)
        ms_first, _ = wall(lambda: ctx.update_values(rowptr, colidx, versions[1 - (rep & 1)]))
        ph_first = ctx.update_values_times()
        ms_host, _ = wall(lambda: ctx.update_values(rowptr, colidx, v))
        ph = ctx.update_values_times()
        ctx.timer_start()
        ms_dev, _ = wall(lambda: ctx.update_values_dev(dv.data_ptr()))
        ev = ctx.timer_stop_ms()
        if rep == 0:
            continue  # warm-up: first touches of the allocator and of the kernels' code objects
        for k, x in zip(t, (ms, ms_first, ph_first[0], ms_host, ph[1], ph[2], ph[3], ph[4], ms_dev, ev)):
            t[k].append(x)
    # the updated handle against a fresh one, bit for bit
    fresh = create(versions[a.reps & 1])
    X = rng.standard_normal((ctx.N, p))
    same = np.array_equal(ctx.dataMatrixProduct(X), fresh.dataMatrixProduct(X))
    fresh.close()
    ctx.close()
    m = {k: float(np.median(x)) for k, x in t.items()}
    slots = stats["padded_nnz"] + stats["long_nnz"]
    nnz = len(vals)
    lines = [
        "# In-place update of Q's values against re-creating the handle",
        "",
        "Written by `python tools/update_values_time.py --poses %d --reps %d` on %s (ROCm %s); medians of %d"
        " alternated repetitions after one warm-up round, wall clock of the calling thread unless said otherwise."
        % (n, a.reps, torch.cuda.get_device_name(0), torch.version.hip, a.reps),
        "",
        "| quantity | value |",
        "|---|---|",
        "| graph | %d poses, %d landmarks, %d ranges, d = %d: N = %d, nnz(Q) = %d, %d stored value slots |"
        % (dm["n"], dm["l"], dm["r"], d, dm["N"], nnz, slots),
        "| destroy the handle + `cora_ctx_create` + `cora_set_rank` (the alternative) | %.2f ms |" % m["recreate"],
        "| first `cora_update_values` on a handle (builds the source map) | %.2f ms, of which map build %.2f ms |" % (m["first"], m["map"]),
        "| `cora_update_values`, host values, map in place | %.2f ms |" % m["host"],
        "| ... pattern hash + host check of the values | %.2f ms |" % (m["host"] - m["upload"] - m["device"] - m["refresh"]),
        "| ... upload of the %.1f MB of values | %.2f ms |" % (nnz * 8 / 1e6, m["upload"]),
        "| ... device: check kernel, flag read-back, gather passes | %.2f ms |" % m["device"],
        "| ... refresh of the host copy of the format | %.2f ms |" % m["refresh"],
        "| `cora_update_values_dev`, values already on the device | %.3f ms (event timer %.3f ms) |" % (m["dev"], m["dev_event"]),
        "| traffic of the gather passes (4 + 8 + 8 bytes per slot) / event time of the device call | %.2f TB/s |"
        % (20.0 * slots / (m["dev_event"] * 1e-3) / 1e12),
        "| re-create / host-pointer update | %.1f x |" % (m["recreate"] / m["host"]),
        "| re-create / device-pointer update | %.1f x |" % (m["recreate"] / m["dev"]),
        "| re-create / first update (map build included) | %.2f x |" % (m["recreate"] / m["first"]),
        "| updated handle against a fresh one (Q X, %d columns) | %s |" % (p, "bit-identical" if same else "DIFFERENT"),
        "",
    ]
    if m["recreate"] / m["host"] < 1.5:
        lines.append("The host-pointer update is NOT clearly faster than re-creating the handle on this graph.")
    else:
        lines.append("The in-place update is faster than re-creation once the map exists; the first update pays the map"
                     " build (%.2f x the re-creation)." % (m["first"] / m["recreate"]))
    lines += ["Re-creation also loses what the figures do not show: resident vectors, the measurement table, the"
              " communicator and the solve plan's device memory.", ""]
    text = "\n".join(lines)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
