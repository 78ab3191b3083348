"""The format of Q (build_format, cora_amd/csrc/format_build.cpp) is a function of the matrix, the partition and the
switches alone: its digest (cora_debug_format_digest: FNV-1a over every integer of the format -- layout, counters, row
maps, slice and chunk descriptors, column indices, both work orders -- and over the bits of every double) equals the one
recorded in tests/golden/format_digests.json, and so does the digest of the source map (cora_debug_value_map_digest: the
sources and the mirror pairs, which come from the builder's provenance mode and which no product test sees).  The table
was recorded with the builder as it stood BEFORE it was cut into phases (one function of 620 lines) plus the two digest
hooks and nothing else, so a builder that passes builds, bit for bit, the formats that one built; copy this file, the
fixture and the digest hooks onto that commit and it passes there too.  No GPU.

Handles (all plan-only, device = -1), the way tests/test_topologies_cpu.py builds them:
  * every entry of tests/topologies.py on one handle and on every rank of every entry of test_topologies_cpu.PARTS
    (world 2 and 3, distributed and whole long rows): 11 handles per entry;
  * the three golden fixtures of test_format_cpu.test_format_on_fixtures and test_update_values_cpu.graph(d), d = 2, 3;
  * all of these again with CORA_CHAIN_SLICES=0 (read once per process: the second child process);
  * the source map of every handle whose graph repeats no measurement (topologies.has_duplicates);
  * CORA_SLICE_LJF=0 (read per call) on robots-d3 and hub-d3: the second work order is empty, everything else is as it
    was -- the bits of the doubles and every count are the default's; the integers are pinned by the recorded digest;
  * robots-d3 (4 pose slices) and a chain of 4 200 poses (66 pose slices: from 64 on the builder takes several threads
    by itself) with CORA_FORMAT_THREADS=1, =7 and unset: one digest.

python tests/test_format_digest_cpu.py <chain|plain> is a child; it prints one line `CASE {json}` per handle and ends
with `DONE`."""
import json
import math
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import topologies as topo   # noqa: E402
from conftest import CASES as FIXTURES   # noqa: E402
from test_topologies_cpu import PARTS   # noqa: E402

ENV = {"chain": {}, "plain": {"CORA_CHAIN_SLICES": "0"}}
LJF_ENTRIES = ("robots-d3", "hub-d3")
THREADS_ENTRY = "robots-d3"
BIG = dict(d=3, n=4200, n_landmarks=3, n_ranges=2000, n_loops=20)   # synth.make_problem: 66 pose slices
THREAD_COUNTS = (1, 7)
EMPTY_ARRAY = "%016x" % ((0xcbf29ce484222325 * 0x100000001b3) % 2 ** 64)   # FNV-1a of the one word "length 0"


def part_ids():
    return ["w%dr%d%s" % (world, rank, "-whole" if whole else "") for world, whole in PARTS for rank in range(world)]


def case_ids(which):
    ids = ["%s/%s/%s" % (which, name, part) for name in topo.NAMES for part in part_ids()]
    ids += ["%s/fixture-%s/w1r0" % (which, f) for f in FIXTURES]
    ids += ["%s/update-d%d/w1r0" % (which, d) for d in (2, 3)]
    if which == "chain":
        ids += ["chain/%s/w1r0/ljf0" % name for name in LJF_ENTRIES]
        ids += ["chain/%s/w1r0/threads%d" % (THREADS_ENTRY, t) for t in THREAD_COUNTS]
        ids += ["chain/big/w1r0"] + ["chain/big/w1r0/threads%d" % t for t in THREAD_COUNTS]
    return ids


# ---------------------------------------------------------------- the child: handles and digests
def child(which):
    assert os.environ.get("CORA_CHAIN_SLICES") == ENV[which].get("CORA_CHAIN_SLICES")   # before the library loads: read once
    from cora_amd import capi
    from synth import make_problem
    from test_oracle_golden import load
    from test_update_values_cpu import graph, plan
    from tri_forms_worker import switches
    capi.load()

    def emit(cid, Q, dm, vals, with_map, env=None, **kw):
        with switches(env or {}):
            ctx = plan(Q, dm, vals, **kw)
            dig = ["%016x" % v for v in ctx.format_digest()]
            if with_map:
                ctx.values_map_build(Q.rowptr, Q.col)
                dig += ["%016x" % v for v in ctx.value_map_digest()]
        s, st, b = ctx.format_shape(), ctx.format_stats(), ctx.format_bytes()
        pose_slices = s["chain_slices"] + s["plain_slices"]
        # entries of perm[] from the descriptor bytes (cora_format_bytes: 32 per slice and per chunk, 4 per entry of perm
        # and of the chunk order, 8 per head value), 64 per slice of permuted translation rows
        head = (dm.d * dm.d + dm.d + 1) * pose_slices
        perm = (b["descriptors"] - 32 * (st["slices"] + st["long_chunks"]) - 8 * head) // 4 - st["long_chunks"]
        assert perm >= 0 and perm % 64 == 0
        print("CASE " + json.dumps(dict(id=cid, digest=" ".join(dig), chain=s["chain_slices"], plain=s["plain_slices"],
                                        long_rows=st["long_rows"], long_chunks=st["long_chunks"],
                                        perm_slices=perm // 64, stats=sorted(st.items()))), flush=True)
        ctx.close()

    for name in topo.NAMES:
        A, Q, dm, g = topo.build(name)
        with_map = not topo.has_duplicates(name)
        for world, whole in PARTS:
            for rank in range(world):
                emit("%s/%s/w%dr%d%s" % (which, name, world, rank, "-whole" if whole else ""), Q, dm, Q.val, with_map,
                     rank=rank, world=world, whole=whole)
        if which == "chain":
            if name in LJF_ENTRIES:
                emit("chain/%s/w1r0/ljf0" % name, Q, dm, Q.val, with_map, env={"CORA_SLICE_LJF": "0"})
            if name == THREADS_ENTRY:
                for t in THREAD_COUNTS:
                    emit("chain/%s/w1r0/threads%d" % (name, t), Q, dm, Q.val, with_map, env={"CORA_FORMAT_THREADS": str(t)})
    for f in FIXTURES:
        A, Q, dm = load(f)
        emit("%s/fixture-%s/w1r0" % (which, f), Q, dm, Q.val, True)
    for d in (2, 3):
        Q, dm, vals1, _ = graph(d)
        emit("%s/update-d%d/w1r0" % (which, d), Q, dm, vals1, True)
    if which == "chain":
        A, Q, dm = make_problem(**BIG)
        emit("chain/big/w1r0", Q, dm, Q.val, True)
        for t in THREAD_COUNTS:
            emit("chain/big/w1r0/threads%d" % t, Q, dm, Q.val, True, env={"CORA_FORMAT_THREADS": str(t)})
    print("DONE", flush=True)


# ---------------------------------------------------------------- the tests
_children = {}


def _child(which):
    """The cases of a set by id; both children are started at the first call (they run side by side)."""
    if not _children:
        procs = {w: subprocess.Popen([sys.executable, os.path.abspath(__file__), w], stdout=subprocess.PIPE,
                                     stderr=subprocess.STDOUT, text=True, env=dict(os.environ, **ENV[w])) for w in ENV}
        for w, proc in procs.items():
            out = proc.communicate(timeout=300)[0]
            cases = {}
            for line in out.splitlines():
                if line.startswith("CASE "):
                    c = json.loads(line[5:])
                    cases[c["id"]] = c
            assert proc.returncode == 0 and "DONE" in out.splitlines(), out[-4000:]
            _children[w] = cases
    return _children[which]


with open(os.path.join(HERE, "golden", "format_digests.json")) as _f:
    DIGESTS = json.load(_f)   # id -> "integers doubles" or "integers doubles sources mirror", recorded before the cut
CASES = [(w, cid) for w in ENV for cid in case_ids(w)]


def test_the_cases_reach_every_path():
    """Before any digest is compared: chain and plain pose slices, a long row whole on one handle, distributed long
    rows, slices of permuted translation rows, a source map with mirror pairs -- and the plain set has no chain slice at
    all.  (Not reached: a rank that holds NOTHING of a distributed long row, nch == 0 in the builder -- on every rank of
    every entry at world 2 and 3 each long row has at least one chunk; profiles/format_refactor.md.)"""
    cases = {cid: _child(w)[cid] for w, cid in CASES}
    chain = {cid: c for cid, c in cases.items() if cid.startswith("chain/")}
    dist = [c for cid, c in chain.items() if "/w1r0" not in cid and not cid.endswith("-whole")]
    assert any(c["chain"] > 0 for c in chain.values()) and any(c["plain"] > 0 for c in chain.values())
    assert all(c["chain"] == 0 for cid, c in cases.items() if cid.startswith("plain/"))
    assert any(c["long_rows"] > 0 for cid, c in chain.items() if "/w1r0" in cid or cid.endswith("-whole"))
    assert any(c["long_rows"] > 0 for c in dist)
    assert any(c["perm_slices"] > 0 for c in cases.values())
    with_map = [c["digest"].split() for c in cases.values() if len(c["digest"].split()) == 4]
    assert len(with_map) > len(cases) // 2 and any(d[3] != EMPTY_ARRAY for d in with_map)
    assert any(d[3] == EMPTY_ARRAY for d in with_map)   # (a plain handle records no pair: the constant is the right one)
    big = chain["chain/big/w1r0"]
    assert big["chain"] + big["plain"] == math.ceil(BIG["n"] / 64) >= 64


@pytest.mark.parametrize("which,cid", CASES, ids=[c[1] for c in CASES])
def test_format_digest_is_the_recorded_one(which, cid):
    got = _child(which)[cid]["digest"]
    print("\n%s %s" % (cid, got))
    assert cid in DIGESTS, "no digest recorded for %s" % cid
    assert got == DIGESTS[cid]


@pytest.mark.parametrize("name", LJF_ENTRIES)
def test_without_the_second_work_order_the_rest_is_unchanged(name):
    """CORA_SLICE_LJF=0 empties slices_pose_first and touches nothing else: the doubles, every count and the source map
    are the default's, the integers differ (by the list that is gone) and are the recorded ones."""
    cases = _child("chain")
    base, off = cases["chain/%s/w1r0" % name], cases["chain/%s/w1r0/ljf0" % name]
    b, o = base["digest"].split(), off["digest"].split()
    assert o[0] != b[0] and o[1:] == b[1:]
    assert {k: v for k, v in off.items() if k not in ("id", "digest")} == {k: v for k, v in base.items() if k not in ("id", "digest")}
    assert off["digest"] == DIGESTS[off["id"]]


def test_format_is_independent_of_the_thread_count():
    """The pose slices of one format built by 1 and by 7 threads (CORA_FORMAT_THREADS): the same format, and the one the
    default thread count builds -- four slices, and 66 (where the default is several threads)."""
    cases = _child("chain")
    for base in ("chain/%s/w1r0" % THREADS_ENTRY, "chain/big/w1r0"):
        for t in THREAD_COUNTS:
            assert cases["%s/threads%d" % (base, t)]["digest"] == cases[base]["digest"] == DIGESTS[base], (base, t)


def test_value_map_digest_needs_a_map():
    from cora_amd import capi
    from test_update_values_cpu import plan
    A, Q, dm, g = topo.build("n2")
    ctx = plan(Q, dm, Q.val)
    with pytest.raises(capi.CoraError) as e:
        ctx.value_map_digest()
    assert e.value.code == 2   # CORA_ERR_NOT_READY
    ctx.values_map_build(Q.rowptr, Q.col)
    assert len(ctx.value_map_digest()) == 2
    ctx.close()


if __name__ == "__main__":
    child(sys.argv[1])
