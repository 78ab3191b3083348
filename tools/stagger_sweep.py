"""Delay sweep of the staggered start of k_spmm's pose slices (profiles/hvp_stagger.md): one handle, the delay set
between timed regions through cora_debug_spmm_stagger_ticks, the regions of all delays interleaved over several rounds.
usage: python tools/stagger_sweep.py [poses] [rank] [hvp|cert] [delays, comma separated] [rounds]
Prints us per launch (host time over 2000 back-to-back launches after 100 warm-up launches, as bench.py measures)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cora_amd import capi, host

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
p = int(sys.argv[2]) if len(sys.argv) > 2 else 5
op = sys.argv[3] if len(sys.argv) > 3 else "hvp"
delays = [int(s) for s in (sys.argv[4] if len(sys.argv) > 4 else "0,100,200,300,400,500").split(",")]
rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 3
P, _ = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=10, n_ranges=n // 2, seed=42, ground_truth=True)
P.update()
dm = P.dims()
_, _, rowptr, colidx, vals = P.matrix("DataMatrix")
ctx = capi.Context(dm["d"], dm["n"], dm["r"], dm["n"] + dm["l"], rowptr, colidx, vals, device=0)
ctx.set_rank(p)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(7)
dev = torch.device("cuda", 0)
y = torch.zeros(ctx.rows * ctx.ld, dtype=torch.float64, device=dev)
x = torch.zeros_like(y)
out = torch.zeros_like(y)
ctx.upload(rng.uniform(-1, 1, (dm["N"], p)), y.data_ptr())
ctx.project_to_manifold_dev(y.data_ptr(), y.data_ptr())
ctx.set_point_dev(y.data_ptr())
ctx.upload(rng.uniform(-1, 1, (dm["N"], p)), x.data_ptr())
ctx.tangent_space_projection_dev(x.data_ptr(), x.data_ptr())
L = ctx.L
L.cora_debug_spmm_stagger_force(1)  # (the sweep decides where the library applies the delay, not the other way round)


def step():
    if op == "cert":
        ctx.certificate_product_dev(x.data_ptr(), p, out.data_ptr())
    else:
        ctx.hvp_dev(x.data_ptr(), out.data_ptr())


def region(steps=2000, warmup=100):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


L.cora_debug_spmm_stagger_ticks(0)
step()
torch.cuda.synchronize()
ref = out.clone()
us = {d: [] for d in delays}
for _ in range(rounds):
    for d in delays:
        L.cora_debug_spmm_stagger_ticks(d)
        us[d].append(region())
        assert torch.equal(out, ref), "delay %d changed the result" % d
print("%s, %d poses, p = %d, row stride %d, %d slices" % (op, n, p, ctx.ld, ctx.format_stats()["slices"]))
for d in delays:
    v = us[d]
    print("delay %4d ticks: %s  median %.2f us" % (d, " ".join("%.2f" % t for t in v), float(np.median(v))), flush=True)
