"""Every iteration form of the device-resident Steihaug-Toint PCG (cora_stpcg_dev, cora_amd/csrc/capi/stpcg.inc) at every
row stride it is compiled for, against a plain numpy STPCG on the oracle's operators (tests/stpcg_ref.py), after 1, 2 and 3
iterations -- before a CG solve has amplified any rounding, so every vector is held to the single-operator tolerances.

The cases run in a child process per d (tests/stpcg_forms_worker.py): CORA_TRI_TOP_INV=0 -- read once, when the library
loads -- makes the plan builder take substitution blocks as soon as more than 1536 rows are left, so the two-stage plan
(paths 2 and the fused backward sweep of cora_precondition_projected_dev) is reached on a few hundred poses.

Graphs (host.Problem.synthetic: landmarks, ranges, loop closures, n no multiple of 64): n scanned upwards with r = n // 2
and 5 landmarks for the first N even whose plan has a stage of substitution blocks (N - 1 > 1536); plan shapes from the
host plan probe (Problem.plan_probe: the handle's ordering and plan builder), asserted on the handle by
test_graphs_give_the_intended_plans, path 2 asserted by every sweep case:
  d = 2  two-stage  n = 438, N = 1538: 2 stages, 7 substitution blocks, 35 rows above them  (n = 437, N = 1534: one inverse)
         one-inverse n = 300, N = 1054 (and n = 301, N = 1057 odd): 1 stage
  d = 3  two-stage  n = 342, N = 1544: 2 stages, 5 substitution blocks, 30 rows above them  (n = 341: N odd; n = 339: one inverse)
         one-inverse n = 250, N = 1128 (and n = 251, N = 1133 odd): 1 stage

Bounds, from the project and not from the run: products 1e-10 (tests/test_gpu_parity.py REL), STPCG vectors and |s|_M 1e-9
(test_fused_stpcg_matches_unfused, there after 7 and 40 iterations), projected preconditioner and its residual 1e-8
(test_cholesky_preconditioner_apply) -- each PER ROW CLASS (rotation, range, translation rows), relative to that class's
largest reference entry.  The reference against itself (plain float64 inner products and an unrefined solve against long
double and one refinement step; `stpcg_forms_worker.py <d> spread`, no GPU) stays below 3e-12 for the vectors and 2e-13
for the preconditioner on these graphs: under 1/100 of each bound (profiles/stpcg_forms.md, which also takes the worst observed deviations)."""
import json
import os
import subprocess
import sys

import pytest

import stpcg_forms_worker as W

pytestmark = pytest.mark.gpu

BOUND = {"prod": 1e-10, "vec": 1e-9, "proj": 1e-8}
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stpcg_forms_worker.py")
FAULT_WORDS = ("illegal memory access", "HSA_STATUS_ERROR", "Memory access fault", "CORA_ERR_HIP", "hipError")


def _run_child(d):
    """(cases by id, fatal message or None) of the child for dimension d."""
    try:
        r = subprocess.run([sys.executable, WORKER, str(d)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=150)
    except subprocess.TimeoutExpired as e:
        out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
        return {}, "the d = %d child did not finish in time:\n%s" % (d, out[-4000:])
    cases = {}
    for line in r.stdout.splitlines():
        if line.startswith("CASE "):
            c = json.loads(line[5:])
            cases[c["id"]] = c
    fault = next((w for w in FAULT_WORDS if w in r.stdout), None)
    if r.returncode != 0 or fault or "DONE" not in r.stdout.splitlines():
        return cases, "the d = %d child ended with status %d%s:\n%s" % (
            d, r.returncode, " and '%s' in its output" % fault if fault else "", r.stdout[-4000:])
    return cases, None


@pytest.fixture(scope="module")
def children():
    """One child per d, the second only after the first has ended well (a faulted GPU gets no further work)."""
    out = {}
    fatal = None
    for d in (2, 3):
        if fatal is None:
            out[d], fatal = _run_child(d)
        else:
            out[d] = {}
    out["fatal"] = fatal
    return out


def _case(children, d, cid):
    if children["fatal"]:
        pytest.fail(children["fatal"])
    assert cid in children[d], "the child printed nothing for %s" % cid
    return children[d][cid]


CASES = [(d, cid) for d in (2, 3) for cid in W.case_ids(d) if not cid.startswith("graph-")]


@pytest.mark.parametrize("d", [2, 3])
def test_graphs_give_the_intended_plans(children, d):
    """The two-stage graph has a stage of several substitution blocks in front of one explicit inverse; the small graphs
    are one explicit inverse; parities of N as the fallback edges need them."""
    two, one, odd = (_case(children, d, "graph-" + k) for k in ("two", "one", "odd"))
    print("\nd=%d two-stage %s\n     one-inverse %s\n     odd %s" % (d, two, one, odd))
    assert two["stages"] == 2 and two["blocks"] >= 3 and two["n"] < 1500 and two["n"] % 64 and two["N"] % 2 == 0
    assert two["N"] - 1 > 1536
    for g in (one, odd):
        assert g["stages"] == 1 and g["blocks"] == 0 and g["N"] - 1 <= 1536 and g["n"] % 64
    assert one["N"] % 2 == 0 and odd["N"] % 2 == 1


@pytest.mark.parametrize("d,cid", CASES, ids=["d%d-%s" % c for c in CASES])
def test_stpcg_form(children, d, cid):
    """One case of the child: the iteration form that ran is the intended one, iteration counts and exits are the
    reference's, and every compared vector is within the bound of its kind in every row class."""
    c = _case(children, d, cid)
    print("\n%s d=%d path %s: %s" % (cid, d, c["path"], "  ".join("%s %.2e" % (n, v) for n, v, _ in c["checks"])))
    assert c["fail"] == []
    assert c["path"] == c["want_path"]
    if not cid.startswith("proj-inplace"):
        assert c["checks"], "nothing was compared"
    for name, value, kind in c["checks"]:
        assert value <= BOUND[kind], (name, value, BOUND[kind])
