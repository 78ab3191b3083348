"""A handle frees what it allocates: the live count of the C API's allocation helpers (cora_debug_live_allocations,
cora_amd/csrc/capi.hip) over two identical cycles through every owner of device memory, after destruction, for a bare
handle, a refused creation and a whole host.Problem solve.  The work runs in a child process per d
(tests/handle_memory_worker.py, whose docstring lists the cycle): the count is process-wide, and another test's handle being
collected mid-test would move it.  Every assertion is an exact integer; the child prints the count after every step, so a
failure names the call that leaked."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "handle_memory_worker.py")
FAULT_WORDS = ("illegal memory access", "HSA_STATUS_ERROR", "Memory access fault", "CORA_ERR_HIP", "hipError")


@pytest.fixture(scope="module")
def children():
    """One child per d, the second only after the first has ended well (a faulted GPU gets no further work)."""
    out, fatal = {}, None
    for d in (2, 3):
        if fatal is not None:
            out[d] = (None, "not started: " + fatal)
            continue
        try:
            r = subprocess.run([sys.executable, WORKER, str(d)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                               timeout=150)
        except subprocess.TimeoutExpired as e:
            text = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
            fatal = "the d = %d child did not finish in time" % d
            out[d] = (None, fatal + ":\n" + text[-4000:])
            continue
        fault = next((w for w in FAULT_WORDS if w in r.stdout), None)
        if r.returncode != 0 or fault or "DONE" not in r.stdout.splitlines():
            fatal = "the d = %d child ended with status %d%s" % (d, r.returncode, " and '%s' in its output" % fault if fault else "")
            out[d] = (None, fatal + ":\n" + r.stdout[-6000:])
            continue
        out[d] = (r.stdout, None)
    return out


@pytest.mark.parametrize("d", [2, 3])
def test_a_handle_frees_what_it_allocates(children, d):
    text, failed = children[d]
    if failed:
        pytest.fail(failed)
    counts = {}
    for line in text.splitlines():
        if line.startswith("COUNT "):
            step, _, n = line[6:].rpartition(" ")
            counts[step] = int(n)
    print("\n" + "\n".join("%6d  %s" % (n, step) for step, n in counts.items()))
    # (the child asserts the same; here from what it printed, so that a child that stopped asserting is noticed)
    assert counts["start"] == 0
    assert counts["bare-handle-created"] > 0 and counts["bare-handle-destroyed"] == 0
    assert counts["after-refused-creations"] == counts["before-refused-creations"] and counts["second-handle-destroyed"] == 0
    assert counts["cycle1 end"] > counts["handles-created"] > 0
    assert counts["cycle2 end"] == counts["cycle1 end"]
    assert counts["solver-destroyed"] == 0
    assert counts["plaza2-solved"] > 0 and counts["plaza2-closed"] == 0
