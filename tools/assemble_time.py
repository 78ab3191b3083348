"""Time of re-weighting the measurements of a live problem on the benchmark's synthetic graph: Problem::setMeasurementWeights
(host sparse algebra + cora_update_values) beside Problem::reweight (cora_assemble_values through the handle's term map) and
the device-pointer call under it (cora_assemble_values_dev), whose assembly and update passes are timed apart.  Every
repetition does all of them in turn and the medians are reported, so drift of the machine hits every figure alike.
python tools/assemble_time.py [--poses 100000] [--reps 11] [--out profiles/assemble_values.md]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cora_amd import capi, host  # noqa: E402

GATHER_TBS = 0.41  # profiles/update_values.md: what the gather passes of the update reach


def flatten(P, w):
    """The seven kinds in table order: rot of every edge | trans of every edge | ranges."""
    full = {k: w.get(k, v) for k, v in P.get_measurement_weights().items()}
    return np.concatenate([full["rel_pose_rot"], full["pose_prior_rot"],
                           np.ones(len(full["pose_landmark"]) + len(full["landmark_prior"])), full["rel_pose_trans"],
                           full["pose_prior_trans"], full["pose_landmark"], full["landmark_prior"], full["range"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--rank", type=int, default=5)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble_values.md"))
    a = ap.parse_args()
    import torch
    n, p = a.poses, a.rank
    L = capi.load()

    def problem():
        P = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=10, n_ranges=n // 2, seed=42)
        P.update()
        P.set_rank(p)
        return P, C.c_void_p(P.context_ptr())  # (the handle is live from here on)

    PA, _ = problem()          # setMeasurementWeights
    PB, ptr = problem()        # reweight
    dm = PB.dims()
    rng = np.random.default_rng(1)
    kinds = {k: len(v) for k, v in PB.get_measurement_weights().items() if len(v)}
    versions = [{k: rng.uniform(0.5, 1.5, m) for k, m in kinds.items()} for _ in range(2)]
    dev = [torch.from_numpy(flatten(PB, w)).to("cuda:0") for w in versions]
    torch.cuda.synchronize()

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    first = wall(lambda: PB.reweight(versions[0]))  # installs the unit table and builds the term map
    ph = (C.c_double * 5)()
    L.cora_assemble_times(ptr, ph)
    build_ms = ph[0]
    info = (C.c_int64 * 4)()
    assert L.cora_assembly_info(ptr, info) == 0
    n_weights, n_terms, n_long, max_terms = (int(x) for x in info)
    nnz = len(PB.matrix("DataMatrix")[4])
    t = {k: [] for k in ("set", "reweight", "dev", "dev_event", "check", "assembly", "update", "rest")}
    for rep in range(a.reps + 1):
        w, dw = versions[rep & 1], dev[rep & 1]
        ms_set = wall(lambda: PA.set_measurement_weights(w))
        ms_rew = wall(lambda: PB.reweight(w))
        assert L.cora_timer_start(ptr) == 0
        ms_dev = wall(lambda: L.cora_assemble_values_dev(ptr, C.c_void_p(dw.data_ptr()), None))
        ev = C.c_float()
        assert L.cora_timer_stop_ms(ptr, C.byref(ev)) == 0
        L.cora_assemble_times(ptr, ph)
        if rep == 0:
            continue  # warm-up: first touches of the allocator and of the kernels' code objects
        for k, x in zip(t, (ms_set, ms_rew, ms_dev, ev.value, ph[1], ph[2], ph[3], ph[4])):
            t[k].append(x)
    # the two methods on the same weights: agreement of the matrices and of a product on the device
    w = versions[a.reps & 1]
    PA.set_measurement_weights(w)
    PB.reweight(w)
    va, vb = PA.matrix("DataMatrix")[4], PB.matrix("DataMatrix")[4]
    rel = float(np.abs(va - vb).max() / np.abs(va).max())
    m = {k: float(np.median(x)) for k, x in t.items()}
    traffic = 12.0 * n_terms + 12.0 * nnz
    rate = traffic / (m["assembly"] * 1e-3) / 1e12
    lines = [
        "# Q(w) assembled on the device against the host assembly",
        "",
        "Written by `python tools/assemble_time.py --poses %d --reps %d` on %s (ROCm %s); medians of %d alternated"
        " repetitions after one warm-up round, wall clock of the calling thread unless said otherwise."
        % (n, a.reps, torch.cuda.get_device_name(0), torch.version.hip, a.reps),
        "",
        "| quantity | value |",
        "|---|---|",
        "| graph | %d poses, %d landmarks, %d ranges, d = %d: N = %d, nnz(Q) = %d |"
        % (dm["n"], dm["l"], dm["r"], dm["d"], dm["N"], nnz),
        "| term map | %d weights, %d terms, %d long entries (more than 128 terms), longest entry %d terms |"
        % (n_weights, n_terms, n_long, max_terms),
        "| `Problem::setMeasurementWeights` (host sparse algebra + `cora_update_values`; the baseline) | %.2f ms |" % m["set"],
        "| `Problem::reweight` (`cora_assemble_values`: upload of the weights, device passes, download of the %.1f MB of"
        " values, refresh of the host format) | %.2f ms |" % (nnz * 8 / 1e6, m["reweight"]),
        "| first `Problem::reweight` on a handle (unit table, source map and term map built) | %.1f ms, of which"
        " `cora_assembly_build` %.1f ms |" % (first, build_ms),
        "| `cora_assemble_values_dev`, weights already on the device | %.3f ms (event timer %.3f ms) |" % (m["dev"], m["dev_event"]),
        "| ... weight check + flag read-back (wall) | %.3f ms |" % m["check"],
        "| ... assembly kernels, short and long entries (events) | %.3f ms |" % m["assembly"],
        "| ... `cora_update_values_dev`'s passes: check, flag read-back, gathers (wall) | %.3f ms |" % m["update"],
        "| ... rescale of the table + final synchronisation (wall) | %.3f ms |" % m["rest"],
        "| traffic of the assembly (12 bytes per term, 4 + 8 per entry: %.0f MB) / its event time | %.2f TB/s (gather passes of"
        " the update: %.2f TB/s) |" % (traffic / 1e6, rate, GATHER_TBS),
        "| setMeasurementWeights / reweight | %.1f x |" % (m["set"] / m["reweight"]),
        "| setMeasurementWeights / device-pointer assembly | %.0f x |" % (m["set"] / m["dev"]),
        "| largest difference of the two methods' matrices, relative to the largest entry | %.2e |" % rel,
        "",
    ]
    text = "\n".join(lines)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
