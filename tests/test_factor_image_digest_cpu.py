"""What an install of a factor uploads -- the solve plan plus its device image (build_tri_image, walk_tri_image:
cora_amd/csrc/trisolve_image.h) -- is a function of the factor, the row map, the groups, the layout and the switches
alone: its digest (cora_debug_factor_image: FNV-1a over every uploaded array in upload order, and over the scalar members
of the kernels' argument blocks) equals the one recorded in tests/golden/factor_image_digests.json.  The table was recorded
from install_factor as it stood BEFORE the image was cut out of it (one function of 300 lines that derived and uploaded in
turns), with its upload lambda hashing instead of copying: profiles/factor_image_refactor.md shows the patch.  No GPU.

The factors, the groups, the environment sets and the per-call switches are those of tests/test_tri_plan_digest_cpu.py
(imported, not copied).  On top of them, per case: the row map -- identity, or the scrambled one of
tests/tri_forms_worker.py -- and the layout of a handle with d = 3 whose first 3 * ((m - 6) // 3) rows are rotation rows
(the rows the `runs3` groups cover under the identity map), vectors of m rows.  One substitution case is built with
CORA_SUB_IO_LISTS=1, and one plan of more than 64 blocks (set T: CORA_TRI_SUB_ROWS=32, so that the I/O lists are sorted
on several threads) by a child bound to one CPU and by one bound to all it may use.

python tests/test_factor_image_digest_cpu.py <A|B|T> [one]  is the child: one line `CASE {json}` per case, then `DONE`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_tri_plan_digest_cpu as PD

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_image_digests.json")
ENV = dict(PD.ENV, T={"CORA_TRI_TOP_INV": "100000", "CORA_TRI_SUB_ROWS": "32"})
MAPS = ("identity", "scrambled")
LISTS_CASE = "A/ndchain-1700/identity/none/aux1/lists"
THREADS_CASE = "T/ndchain-4300/identity/runs3/aux1/default"
D = 3


def case_ids(which):
    if which == "T":
        return [THREADS_CASE]
    ids = ["%s/%s/%s/%s/aux%d/%s" % (which, f, mp, g, a, s) for f in PD.FIXTURE_NAMES for mp in MAPS
           for g, a, s in PD.variants(which)]
    return ids + ([LISTS_CASE] if which == "A" else [])


def row_map(how, m):
    """internal row of every variable of the factor"""
    if how == "identity":
        return None
    return np.random.default_rng(m + 7).permutation(m).astype(np.int32)   # (tri_forms_worker.permutation, "scrambled")


# ---------------------------------------------------------------- the child
def child(which, one_cpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if one_cpu:   # as `taskset -c <first cpu>` around this process
        os.sched_setaffinity(0, {min(os.sched_getaffinity(0))})
    os.environ.update(ENV[which])   # before the library loads: read once
    from cora_amd import capi
    from tri_forms_worker import switches
    capi.load()
    factors = {}
    for cid in case_ids(which):
        _, name, how, gkind, aux, sw = cid.split("/")
        if name not in factors:
            factors = {name: PD.seeded_factor(name)}   # once per fixture
        L = factors[name]
        m = L.shape[0]
        env = {"CORA_SUB_IO_LISTS": "1"} if sw == "lists" else PD.SWITCHES[sw]
        with switches(env):
            dig, shape = capi.factor_image(L.indptr, L.indices, L.data, row_map=row_map(how, m), group=PD.groups(gkind, m),
                                           aux_ok=int(aux[3:]), d=D, rot0=0, rot1=D * ((m - 6) // D), rows=m)
        print("CASE " + json.dumps(dict(id=cid, digest=["%016x" % d for d in dig], shape=shape,
                                        cpus=len(os.sched_getaffinity(0)))), flush=True)
    print("DONE", flush=True)


# ---------------------------------------------------------------- the tests
_children = {}


def _child(which):
    """The cases of a child by id; all children are started at the first call (they run side by side).  "T1": set T
    bound to one CPU."""
    if not _children:
        procs = {w: subprocess.Popen([sys.executable, os.path.abspath(__file__), w[0]] + (["one"] if w == "T1" else []),
                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for w in ("A", "B", "T", "T1")}
        for w, proc in procs.items():
            out = proc.communicate(timeout=600)[0]
            cases = {}
            for line in out.splitlines():
                if line.startswith("CASE "):
                    c = json.loads(line[5:])
                    cases[c["id"]] = c
            assert proc.returncode == 0 and "DONE" in out.splitlines(), out[-4000:]
            _children[w] = cases
    return _children[which]


CASES = [(w, cid) for w in ("A", "B", "T") for cid in case_ids(w)]
_digests = {}


def digests():
    """id -> [digest of the integers, digest of the doubles], recorded from install_factor before the cut"""
    if not _digests:
        with open(GOLDEN) as f:
            _digests.update(json.load(f))
    return _digests


def test_the_cases_reach_every_derivation():
    """Before any digest is compared: the cases are not vacuous."""
    from cora_amd import capi
    sh = {cid: _child(w)[cid]["shape"] for w, cid in CASES}
    sub = {cid: s for cid, s in sh.items() if s["form"] == capi.FORM_SUB}
    assert [c for c, s in sub.items() if s["io_runs"] == 1]
    lists = [c for c, s in sub.items() if s["io_runs"] == 0]
    assert [c for c in lists if "/scrambled/" in c], "no index lists from a scrambled map"
    assert LISTS_CASE in lists and sub[LISTS_CASE[:-len("lists")] + "default"]["io_runs"] == 1, "no index lists from the switch alone"
    assert [c for c, s in sub.items() if s["fuse_ok"] == 1]
    assert [c for c, s in sub.items() if s["fuse_ok"] == 0]
    assert [c for c, s in sh.items() if s["form"] == capi.FORM_DENSE]
    # three stages: the only plans whose middle stage has all four row products (a stage 0 of these fixtures is dense or
    # substitution blocks whenever there is more than one stage, so no plan of theirs has three stages of row products alone)
    assert [c for c, s in sh.items() if s["stages"] >= 3], "no plan with three stages"
    assert [c for c, s in sub.items() if s["aux_sum"] == 1]
    assert [c for c, s in sh.items() if s["chunks"] > 0]
    assert sh[THREADS_CASE]["form"] == capi.FORM_SUB and sh[THREADS_CASE]["blocks"] >= 64   # (from 64 blocks on: threads)
    for s in sh.values():   # every field is filled but the handle's
        assert s["generation"] == -1 and s["fuse_ok"] in (0, 1) and (s["io_runs"] in (0, 1)) == (s["form"] == capi.FORM_SUB)


@pytest.mark.parametrize("which,cid", CASES, ids=[c[1] for c in CASES])
def test_image_digest_is_the_recorded_one(which, cid):
    got = _child(which)[cid]["digest"]
    print("\n%s %s %s" % (cid, got[0], got[1]))
    assert cid in digests(), "no digest recorded for %s" % cid
    assert got == digests()[cid]


def test_image_is_independent_of_the_thread_count():
    """The I/O lists of one plan sorted by a process bound to one CPU and by one bound to every CPU it may use: one
    image, the recorded one."""
    one, many = _child("T1")[THREADS_CASE], _child("T")[THREADS_CASE]
    assert one["cpus"] == 1
    assert one["digest"] == many["digest"] == digests()[THREADS_CASE]


if __name__ == "__main__":
    child(sys.argv[1], len(sys.argv) > 2 and sys.argv[2] == "one")
