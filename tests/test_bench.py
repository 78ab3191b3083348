"""bench.py's plain run and --dump-outputs: the headline line alone, and the product of the last timed step written
to disk -- checked against the CPU oracle on the same seeded inputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("cora_bench", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """Below the size limit the array is written whole; above it a fixed sample of rows (the same one every run) with
    the row numbers beside it, within the limit."""
    bench = _bench_module()
    a = np.random.default_rng(1).uniform(-1, 1, (1000, 5))
    bench.dump_outputs(str(tmp_path / "whole"), "hvp", np.asfortranarray(a))
    got = np.load(tmp_path / "whole" / "hvp.npy")
    assert got.dtype == np.float64 and np.array_equal(got, a)
    assert not os.path.exists(tmp_path / "whole" / "hvp_rows.npy")

    monkeypatch.setattr(bench, "DUMP_LIMIT", 8 * 6 * 100)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), "hvp", a)
    rows = np.load(tmp_path / "s1" / "hvp_rows.npy")
    part = np.load(tmp_path / "s1" / "hvp.npy")
    assert rows.dtype == np.float64 and part.shape == (100, 5)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 1000
    assert np.array_equal(part, a[rows.astype(np.int64)])
    assert part.nbytes + rows.nbytes <= bench.DUMP_LIMIT
    assert np.array_equal(rows, np.load(tmp_path / "s2" / "hvp_rows.npy"))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_product(tmp_path):
    """A plain run times --steps products and prints the headline only; --dump-outputs holds the last step's Hvp, equal
    to the oracle's on the bench's own inputs (generator seed 42, operands U(-1, 1) seed 7)."""
    from cora_amd import host
    from oracle import oracle as orc

    n, p, steps = 2000, 5, 20
    out = tmp_path / "out"
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "3", "--poses", str(n),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "riemannian_hessian_vector_products_per_sec" and d["unit"] == "Hvp/s"
    assert d["dtype"] == "f64" and d["higher_is_better"] is True and d["steps"] == steps
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-9 * 1e3
    for key in ("roofline", "extras", "cpu_baseline", "parity_max_rel_err_vs_cpu", "value_stats"):
        assert key not in d, key

    P, _ = host.Problem.synthetic(dim=3, n_poses=n, n_landmarks=10, n_ranges=n // 2, seed=42, ground_truth=True)
    P.update()
    dm = P.dims()
    _, _, rowptr, colidx, vals = P.matrix("DataMatrix")
    Q = orc.CSR(rowptr, colidx, vals, dm["N"])
    dims = orc.Dims(dm["d"], dm["n"], dm["r"], dm["N"])
    rng = np.random.default_rng(7)
    Y = orc.project_manifold(dims, rng.uniform(-1, 1, (dm["N"], p)))
    V = orc.tangent_proj(dims, Y, rng.uniform(-1, 1, (dm["N"], p)))
    ref = orc.hvp(Q, dims, Y, orc.egrad(Q, Y), V)
    got = np.load(out / "hvp.npy")
    assert got.shape == (dm["N"], p) and got.dtype == np.float64
    assert np.abs(got - ref).max() < 1e-10 * np.abs(ref).max()
