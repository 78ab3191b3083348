"""The staged Cholesky solve kernels -- k_rowop, k_blockop, k_subblock (cora_amd/csrc/kernels/tri.inc) -- on every form of
the solve plan and on factors of arbitrary structure, through the entry points that take any factor
(cora_aux_set_cholesky / cora_aux_solve_dev) and through the preconditioner's (cora_precond_set_cholesky,
cora_precondition, cora_precondition_projected_dev, cora_stpcg_dev), against a dense float64 solve with one refinement
step in long double (tests/tri_forms.py).

The cases run in one child process per ENVIRONMENT SET (tests/tri_forms_worker.py, which lists the sets and what each
reaches), strictly one after the other, each under its own time limit; a child that faults, aborts or runs out of time
fails every test of the module, and no further child is started.  The handles come from synth.make_problem, sized so
that N is the fixture's order (1600 to 2600, one of 4300).

Before anything is compared, the form of the INSTALLED plan is asserted on the handle (cora_debug_factor_shape): one
inverse; substitution blocks with the aux sums folded / as their own product, row I/O from run tables (the identity in the
vectors' own row order: a block is a run of consecutive rows) / from index lists (a scrambled one, and CORA_SUB_IO_LISTS=1); dense blocks in 2 and in
3 stages; substitution blocks on a branching tree; an incomplete factor; all three row classes in one product; a row of
more than 64 chunks; tiles above 64 KB of LDS.  Every field the host probe knows must equal the host probe's.

Per form: solves of 1..24 columns (every row stride) into a NaN-filled output -- no NaN left, the right-hand side
unchanged bit for bit, the same bits from a second solve and from a third one after a solve of another column count (ticket
reset, scratch reuse); then other factors on the same handle (the arena is written over, the probe follows).
Preconditioner entry (N - 1 rows of Q + lambda I, factorised in numpy): the pinned row exactly zero, the projected apply at
p = d, d + 2, 12, 13 on a plan whose backward sweep takes the projection, on one whose tiles do not hold a pose's
rotation rows together (fuse_ok == 0) and on dense blocks; three STPCG iterations on the dense-block plan in the form
stpcg.inc prescribes for it (path 1).  Error paths: NOT_READY before an install and after a refused one, ARG for aliased
vectors, k = 0, k = 25, m != N, a perm that is none, a diagonal that is not first.

Bounds, the project's own for these plans (tests/test_trisolve_cpu.py, tests/test_gpu_stpcg_forms.py), relative to the
reference's largest entry (per row class where the rows are the graph's): 1e-11 complete factors, 1e-10 the incomplete
one, 1e-8 the regularised Q + lambda I, STPCG vectors 1e-9, products 1e-10.  The reference's own spread is under 1/100 of
each and the host emulation of the same plans at 1.2e-15 / 2.2e-13 (tests/test_tri_forms_cpu.py).  The deviation from the
host emulation of the same plan is printed, not asserted.  Observed on the device: profiles/tri_forms.md."""
import json
import os
import subprocess
import sys

import pytest

import tri_forms_worker as W

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tri_forms_worker.py")
FAULT_WORDS = ("illegal memory access", "HSA_STATUS_ERROR", "Memory access fault", "CORA_ERR_HIP", "hipError")
SETS = ("B", "A", "C", "C0", "P")   # the plain products first
LIMIT_S = {"A": 240, "B": 120, "C": 120, "C0": 150, "P": 150}


def _run_child(which):
    """(cases by id, fatal message or None) of the child of one environment set."""
    try:
        r = subprocess.run([sys.executable, WORKER, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=LIMIT_S[which])
    except subprocess.TimeoutExpired as e:
        out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
        return {}, "the child of set %s did not finish in time:\n%s" % (which, out[-4000:])
    cases = {}
    for line in r.stdout.splitlines():
        if line.startswith("CASE "):
            c = json.loads(line[5:])
            cases[c["id"]] = c
    fault = next((w for w in FAULT_WORDS if w in r.stdout), None)
    if r.returncode != 0 or fault or "DONE" not in r.stdout.splitlines():
        return cases, "the child of set %s ended with status %d%s:\n%s" % (
            which, r.returncode, " and '%s' in its output" % fault if fault else "", r.stdout[-4000:])
    return cases, None


@pytest.fixture(scope="module")
def children():
    """One child per set, each only after the one before has ended well (a faulted GPU gets no further work)."""
    out = {}
    fatal = None
    for which in SETS:
        if fatal is None:
            out[which], fatal = _run_child(which)
        else:
            out[which] = {}
    out["fatal"] = fatal
    return out


CASES = [(s, cid) for s in SETS for cid in W.case_ids(s)]


@pytest.mark.parametrize("which,cid", CASES, ids=["%s-%s" % c for c in CASES])
def test_tri_form(children, which, cid):
    """One case of a child: the installed plan has the intended form, nothing discrete went wrong, something was compared
    and every deviation is within the bound of its kind."""
    if children["fatal"]:
        pytest.fail(children["fatal"])
    assert cid in children[which], "the child printed nothing for %s" % cid
    c = children[which][cid]
    print("\n%s %s: %s\n  %s" % (which, cid, {k: v for k, v in c["shape"].items() if v not in (0, -1)},
                               "  ".join("%s %.2e" % (n, v) for n, v, k in c["checks"] if not n.startswith("x.k"))))
    per_k = sorted((int(n[3:]), v) for n, v, _ in c["checks"] if n.startswith("x.k"))
    if per_k:
        print("  per column count: " + " ".join("%d:%.1e" % kv for kv in per_k))
    assert c["fail"] == []
    compared = [n for n, _, k in c["checks"] if k in ("complete", "incomplete", "reg", "vec", "prod") and n != "host"]
    assert compared, "nothing was compared on the device"
    for name, value, kind in c["checks"]:
        if kind != "info":
            assert value <= W.BOUND[kind], (name, value, W.BOUND[kind])
