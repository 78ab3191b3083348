"""cora_main --rpe / --rpe-dist: the lines parse, the pair counts are those of tests/rpe_ref.py's builders on the file's own
vertices, and the values are those of Problem.relative_error on the solution the driver wrote (--tum: the solution moved
to the origin pose's frame, which no relative pose error sees)."""
import os
import re
import subprocess

import numpy as np
import pytest

import rpe_ref as rp
from conftest import GOLDEN
from cora_amd import build as _build
from cora_amd import host

pytestmark = pytest.mark.gpu
REL = 2e-5  # the lines print six significant digits


def _rpe_lines(text):
    """{setting: (pairs, translation RMSE, max, rotation RMSE in degrees, max, drift per unit, degrees per unit)}"""
    out = {}
    for line in text.splitlines():
        m = re.match(r"rpe: (step \S+|distance \S+) (\d+) pairs  translation RMSE (\S+) max (\S+)  rotation RMSE (\S+) deg max (\S+) deg"
                     r"  drift (\S+) per unit (\S+) deg per unit$", line)
        if m:
            out[m.group(1)] = (int(m.group(2)),) + tuple(float(v) for v in m.groups()[2:])
    return out


def _vertices(path):
    """(pose symbols, positions [n, 2]) of a 2-D file, in file order (the pose order of the parsed problem)."""
    rec = [line.split() for line in open(path) if line.startswith("VERTEX_SE2 ")]
    return [r[2] for r in rec], np.array([[float(r[3]), float(r[4])] for r in rec])


def _solution_of_tum(tum, dm):
    """The N x 2 point a 2-D TUM file describes: rotation rows R_i^T, positions; range and landmark rows stay zero (no
    relative pose error reads them)."""
    d, n, r = dm["d"], dm["n"], dm["r"]
    got = np.loadtxt(tum).reshape(-1, 8)
    assert d == 2 and got.shape[0] == n
    X = np.zeros((dm["N"], d), order="F")
    yaw = 2.0 * np.arctan2(got[:, 6], got[:, 7])
    for i in range(n):
        R = np.array([[np.cos(yaw[i]), -np.sin(yaw[i])], [np.sin(yaw[i]), np.cos(yaw[i])]])
        X[d * i:d * i + d] = R.T
    X[d * n + r:d * n + r + n] = got[:, 1:3]
    return X


def _degrees(chordal):
    return 2.0 * np.degrees(np.arcsin(np.minimum(1.0, chordal / (2.0 * np.sqrt(2.0)))))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """cora_main, built once for the module as the --evaluate test builds it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = _build.build()
    out = str(tmp_path_factory.mktemp("driver") / "cora_main")
    subprocess.run([_build.HIPCC, "-O1", "-std=c++17", "-I" + os.path.join(root, "include"),
                    "-I" + os.path.join(root, "cora_amd", "csrc", "host"), os.path.join(root, "examples", "main.cpp"),
                    "-L" + os.path.dirname(lib), "-lcora_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", out],
                   check=True, timeout=600)
    return out


@pytest.mark.parametrize("name", ["mrclam6", "plaza2"])
def test_command_line_driver_reports_the_relative_pose_error(name, exe, tmp_path):
    path = os.path.join(GOLDEN, "datasets", name + ".pyfg")
    tum = str(tmp_path / "solution.tum")
    r = subprocess.run([exe, path, "--rpe", "1,10", "--rpe-dist", "5", "--tum", tum], stdout=subprocess.PIPE, text=True,
                       timeout=300, check=True)
    lines = _rpe_lines(r.stdout)
    assert sorted(lines) == ["distance 5", "step 1", "step 10"], r.stdout[-2000:]
    symbols, positions = _vertices(path)
    chains = rp.chains_of(symbols)
    assert (len(chains) > 1) == (name == "mrclam6")
    want = {"step 1": rp.pairs_by_step(chains, 1), "step 10": rp.pairs_by_step(chains, 10),
            "distance 5": rp.pairs_by_distance(chains, positions, 5.0)}
    P = host.Problem.from_pyfg(path)
    P.update()
    truth = P.ground_truth(path)
    dm = P.dims()
    X = _solution_of_tum(tum, dm)
    P.op("evaluateObjective", truth)  # (a live handle)
    mine = {"step 1": P.pose_pairs_by_step(1), "step 10": P.pose_pairs_by_step(10), "distance 5": P.pose_pairs_by_distance(truth, 5.0)}
    for setting, got in lines.items():
        pairs, path_length = want[setting]
        assert got[0] == len(pairs) > 0 and np.array_equal(mine[setting][0], pairs), setting
        res = P.relative_error(X, truth, mine[setting])
        ang = _degrees(res["rot_err"])
        values = (res["trans_rmse"], res["max_et"], float(np.sqrt(np.mean(ang ** 2))), float(ang.max()), res["mean_trans_drift"],
                  float(np.mean(ang / mine[setting][1])))
        print(name, setting, got, values)
        # the TUM file prints nine digits of positions up to a few hundred: 1e-6 absolute on top of the lines' six digits
        for a, b in zip(got[1:], values):
            assert abs(a - b) <= REL * abs(b) + 2e-6, (setting, got, values)
        assert got[1] <= got[2] and got[3] <= got[4]
