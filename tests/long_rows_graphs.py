"""The graphs of tests/test_long_image_cpu.py and tests/test_gpu_long_rows_xcd.py: small problems whose landmark rows take
the long-row path (more than kLongRow = 96 entries) and reach every branch of the long rows' device image
(cora_amd/csrc/long_image.h).  Built once per process and shared; nothing here needs a GPU.

  random  synth.make_problem(d=3, n=200, n_landmarks=2, n_ranges=300): the ranges come from poses drawn at random, so
          every landmark row reads columns along the whole chain.  9 slices (4 pose, 5 range), per_xcd = 2: XCDs 0-4
          hold slices and pieces, XCDs 5-7 are empty (padding only).  Every row has several pieces (the ticket path).
  cut     n = 4200, one landmark ranged from every pose: 132 slices, per_xcd = 17, about 1050 entries of the row per
          XCD -- more than a piece of 1024, so every XCD's run is cut again.
  single  three landmarks, the second seen from poses 0 .. 49 only and the others from no pose below 50; 9 slices, per_xcd
          = 2, and XCD 0 runs the first pose slice and the first range slice: all columns of the second landmark's row
          are theirs -- one piece, the path without ticket (nchunks == 1)."""
import numpy as np

import synth
from oracle import assemble as asm
from oracle import oracle as orc

NAMES = ("random", "cut", "single")
_BUILT = {}


def _single():
    g = synth.make_graph(d=3, n=200, n_landmarks=3, n_ranges=450)
    R, T, L = g.truth
    rng = np.random.default_rng(17)
    keep = [m for m in g.ranges if m[1] != "L1" and int(m[0][1:]) >= 50]
    near = [("A%d" % i, "L1", abs(np.linalg.norm(T[i] - L[1]) + rng.normal(0, 0.1)), 0.01) for i in range(50)]
    g.ranges[:] = keep + near
    return g


def build(name):
    """(A, Q, dm) as synth.make_problem returns them (A["truth"]: the ground truth, N x d)."""
    if name not in _BUILT:
        if name == "random":
            g = synth.make_graph(d=3, n=200, n_landmarks=2, n_ranges=300)
        elif name == "cut":
            g = synth.make_graph(d=3, n=4200, n_landmarks=1, n_ranges=4200)
        else:
            g = _single()
        A = asm.assemble(g)
        A["truth"] = synth.ground_truth(g)
        _BUILT[name] = (A, orc.CSR.from_scipy(A["Q"]), orc.Dims(A["d"], A["n"], A["r"], A["N"]))
    return _BUILT[name]


def near_truth(name, p, noise=0.02, seed=0):
    """topologies.near_truth for these graphs: the lifted ground truth, rotated in R^p, every entry perturbed."""
    A, Q, dm = build(name)
    rng = np.random.default_rng(1000 * seed + p)
    R, _ = np.linalg.qr(rng.standard_normal((p, p)))
    lifted = np.hstack([A["truth"], np.zeros((dm.N, p - dm.d))])
    return orc.project_manifold(dm, (lifted + noise * rng.standard_normal((dm.N, p))) @ R)
