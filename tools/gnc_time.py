"""Time of one round of a robust-cost (GNC) loop on the benchmark's synthetic graph: the device weight step
(cora_gnc_weights_dev) by events and by wall clock, the device round (weight step + cora_assemble_values_dev: residuals to
Q(w) without leaving the device), and beside them what the same round takes with the calls that existed before the weight
step: cora_measurement_residuals_dev to the host, division by the current weights, the weight formulas in numpy,
cora_assemble_values from the host.  Every repetition does all of them in turn and the medians are reported, so drift of
the machine hits every figure alike.  Geman-McClure throughout: its weights stay positive, which the division needs.
python tools/gnc_time.py [--poses 100000] [--reps 21] [--out profiles/gnc.md]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cora_amd import capi, host  # noqa: E402

NOTES = """
## Inputs of the robust-solve test

`tests/test_gpu_gnc.py` solves `make_graph(d, n=30, n_landmarks=3, n_ranges=60, n_loops=5)` at the generator's default
seed 42, d = 2 and 3, with the ranges 3, 11, 19, 27, 42 and 55 made 10.0 longer (100 sigma at sigma = 0.1) and the range
threshold 25.  With these the loop written out by hand in the test (solve, unweighted residuals from a second Problem,
numpy weights, reweight) and `solve_robust` both end on exactly the six ranges: TLS after 14 (d = 2) and 16 (d = 3) rounds
at f = 24.6662512 and 35.1962978, GM after 20 rounds at f = 22.6053815 and 32.3929307, the two loops with the same cost to
the last printed digit.  A restatement of the loop over the CPU oracle's TNT (rank d, no preconditioner) ended on the same
six at this shift and at 30.0, the inlier weights of GM no lower than 0.70.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--rank", type=int, default=5)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnc.md"))
    a = ap.parse_args()
    import torch
    n, p = a.poses, a.rank
    L = capi.load()
    P = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=10, n_ranges=n // 2, seed=42)
    P.update()
    P.set_rank(p)
    ptr = C.c_void_p(P.context_ptr())  # (the handle is live from here on)
    dm = P.dims()
    kinds = {k: len(v) for k, v in P.get_measurement_weights().items()}
    P.reweight({})  # installs the unit-weight table and the term map
    info = (C.c_int64 * 4)()
    assert L.cora_assembly_info(ptr, info) == 0
    nw = int(info[0])
    ne, nr = (nw - kinds["range"]) // 2, kinds["range"]
    ctx = capi.Context.from_handle(ptr.value, dm["d"], dm["n"], dm["r"], dm["n"] + dm["l"])
    X = P.op("getRandomInitialGuess")
    x = ctx.dev_alloc(p)
    ctx.upload(X, x)
    barc2 = np.full(nw, np.inf)
    barc2[2 * ne:] = 25.0
    mu = 50.0
    d_barc2 = torch.from_numpy(barc2).to("cuda:0")
    d_w = torch.zeros(nw, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dp = C.POINTER(C.c_double)
    st = np.zeros(12)
    rot, trn, rng, sums = np.zeros(max(ne, 1)), np.zeros(max(ne, 1)), np.zeros(max(nr, 1)), np.zeros(3)
    w_cur = np.ones(nw)  # what the table's kappa, tau, omega are scaled by at the moment

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def step():
        assert L.cora_gnc_weights_dev(ptr, C.c_void_p(x), p, C.c_void_p(d_barc2.data_ptr()), 2, 1, C.c_double(mu),
                                      C.c_void_p(d_w.data_ptr()), None, st.ctypes.data_as(dp)) == 0

    def device_round():
        step()
        assert L.cora_assemble_values_dev(ptr, C.c_void_p(d_w.data_ptr()), None) == 0

    def host_round():
        nonlocal w_cur
        assert L.cora_measurement_residuals_dev(ptr, C.c_void_p(x), p, rot.ctypes.data_as(dp), trn.ctypes.data_as(dp),
                                                rng.ctypes.data_as(dp), sums.ctypes.data_as(dp)) == 0
        r2 = np.concatenate([rot[:ne], trn[:ne], rng[:nr]]) / w_cur   # back to the unweighted residuals
        r2[:ne] = r2[ne:2 * ne] = r2[:ne] + r2[ne:2 * ne]             # coupled edges
        c = barc2.copy()
        c[:ne] = c[ne:2 * ne]
        t = mu / (np.where(np.isinf(c), 0.0, r2 / c) + mu)
        w = t * t
        assert L.cora_assemble_values(ptr, w.ctypes.data_as(dp), None) == 0
        w_cur = w

    t = {k: [] for k in ("step", "step_event", "device_round", "host_round")}
    for rep in range(a.reps + 1):
        assert L.cora_timer_start(ptr) == 0
        ms_step = wall(step)
        ev = C.c_float()
        assert L.cora_timer_stop_ms(ptr, C.byref(ev)) == 0
        ms_dev = wall(device_round)
        w_cur = d_w.cpu().numpy().copy()
        ms_host = wall(host_round)
        if rep == 0:
            continue  # warm-up: first touches of the allocator and of the kernels' code objects
        for k, v in zip(t, (ms_step, ev.value, ms_dev, ms_host)):
            t[k].append(v)
    # the two rounds on the same table and point: the weights they produce
    device_round()
    w_dev = d_w.cpu().numpy().copy()
    w_cur = w_dev.copy()
    host_round()
    diff = float(np.abs(w_cur - w_dev).max())
    m = {k: float(np.median(v)) for k, v in t.items()}
    lo = {k: float(np.min(v)) for k, v in t.items()}
    hi = {k: float(np.max(v)) for k, v in t.items()}
    table_bytes = ne * (4 * 4 + (9 + 3) * 8 + 6 * 8) + nr * (3 * 4 + 8 + 3 * 8)
    lines = [
        "# The GNC weight step on the device against the same round through the host",
        "",
        "Written by `python tools/gnc_time.py --poses %d --reps %d` on %s (ROCm %s); medians (min .. max) of %d alternated"
        " repetitions after one warm-up round.  Wall clock of the calling thread around calls that end in a stream"
        " synchronisation, unless said otherwise." % (n, a.reps, torch.cuda.get_device_name(0), torch.version.hip, a.reps),
        "",
        "| quantity | value |",
        "|---|---|",
        "| graph | %d poses, %d landmarks, %d ranges, d = %d: N = %d; table: %d edges, %d ranges, %d weights |"
        % (dm["n"], dm["l"], dm["r"], dm["d"], dm["N"], ne, nr, nw),
        "| point | %d columns; cost Geman-McClure, mu = %g, coupled edges, range threshold 25, edges trusted |" % (p, mu),
        "| `cora_gnc_weights_dev` (two fused passes, four single-block reductions, flag and statistics read back) |"
        " %.3f ms (%.3f .. %.3f) |" % (m["step"], lo["step"], hi["step"]),
        "| ... the same by the handle's event timer | %.3f ms (%.3f .. %.3f) |" % (m["step_event"], lo["step_event"], hi["step_event"]),
        "| table and vector bytes the two passes read or write once (%.1f MB; the rows of X are gathered on top) over the"
        " event time | %.3f TB/s -- the pass is bound by latency and launches, not by bandwidth |"
        % (table_bytes / 1e6, table_bytes / (m["step_event"] * 1e-3) / 1e12),
        "| device round: `cora_gnc_weights_dev` + `cora_assemble_values_dev` | %.3f ms (%.3f .. %.3f) |"
        % (m["device_round"], lo["device_round"], hi["device_round"]),
        "| the same round with the calls that existed before: `cora_measurement_residuals_dev` to the host, division by the"
        " current weights, numpy weights, `cora_assemble_values` | %.3f ms (%.3f .. %.3f) |"
        % (m["host_round"], lo["host_round"], hi["host_round"]),
        "| host round / device round | %.1f x |" % (m["host_round"] / m["device_round"]),
        "| largest difference of the two rounds' weights (the host round divides weighted residuals by the weights) | %.2e |" % diff,
        "",
    ]
    text = "\n".join(lines) + NOTES
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
