"""The solve plan of a factor (build_tri_plan, cora_amd/csrc/trisolve_build.cpp) is a function of the factor, the groups
and the switches alone: its digest (cora_debug_factor_plan_digest: FNV-1a over every integer, index and header of the plan,
and over the bits of every double) equals the one recorded below.  The table was recorded with the builder as it stood
BEFORE it was cut into phases (one function of 960 lines), so a builder that passes builds, bit for bit, the plans that
one built; copy this file and the digest hook onto that commit and it passes there too.  No GPU.

Inputs that are the same on every machine (no LAPACK takes part): the matrices of tests/tri_forms.py for their PATTERN
only, the factor's pattern by symbolic elimination (a column's rows are the matrix's rows below the diagonal united with
the rows of its elimination-tree children), values from a seeded generator (diagonal in [1, 2], the rest in [-0.5, 0.5]:
the builder never asks for positive definiteness); the incomplete factor drops entries of those by tri_forms.drop_entries.

Per fixture: no groups / runs of three consecutive variables as groups (a group is never cut: staging and supernodes),
the substitution form allowed or not, and the switches tests/tri_forms_worker.py reaches the plan forms with, set the way
it sets them: those read once (CORA_TRI_TOP_INV) in the environment of a child process before the library loads -- set A
and set B of that worker --, those read per call around the call.  python tests/test_tri_plan_digest_cpu.py <A|B> is that child; it prints
one line `CASE {json}` per case and ends with `DONE`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ENV = {"A": {"CORA_TRI_TOP_INV": "20000"}, "B": {}}
# switches read per call (name of the variant -> environment around the call)
SWITCHES = {"default": {}, "sub0": {"CORA_TRI_SUB": "0"}, "unfold": {"CORA_TRI_UNFOLD_MIN": "0"},
            "sncap8": {"CORA_TRI_SN_CAP": "8"}, "sncap4": {"CORA_TRI_SN_CAP": "4"},   # (by the tree's height: 4 or 8)
            "etree": {"CORA_TRI_CHECK_ETREE": "1"}}
FIXTURE_NAMES = ("ndchain-1700", "ndchain-2600", "ndchain-4300", "random-1600", "random-2600", "arrow-2500",
                 "incomplete-2600", "tree-2000")
THREADS_CASE = "A/ndchain-4300/none/aux1/default"   # substitution blocks: built by CORA_TRI_THREADS threads


def variants(which):
    """(group kind, aux_ok, switches) of every case of a fixture in the set"""
    if which == "B":   # defaults: one explicit inverse whatever the switches
        return [(g, 1, "default") for g in ("none", "runs3")]
    return [(g, a, s) for g in ("none", "runs3") for a, s in [(0, "default")] + [(1, s) for s in SWITCHES]]


def case_ids(which):
    return ["%s/%s/%s/aux%d/%s" % (which, f, g, a, s) for f in FIXTURE_NAMES for g, a, s in variants(which)]


# ---------------------------------------------------------------- the child: factors and digests
def symbolic_factor(A):
    """Pattern of the Cholesky factor of a matrix with A's pattern, as a boolean CSC matrix with sorted columns (the
    diagonal first): column by column, the rows below the first sub-diagonal row p of a column join column p."""
    import scipy.sparse as sp
    n = A.shape[0]
    M = np.zeros((n, n), dtype=bool, order="F")
    C = sp.tril(sp.csc_matrix(A), -1).tocoo()
    M[C.row, C.col] = True
    for j in range(n):
        rows = j + 1 + np.flatnonzero(M[j + 1:, j])
        if len(rows) > 1:
            M[rows[1:], rows[0]] = True
    M[np.arange(n), np.arange(n)] = True
    L = sp.csc_matrix(M)
    L.sort_indices()
    return L


def seeded_factor(name):
    """The fixture's matrix (tests/tri_forms.py, generated as fixture() generates it) -> pattern of its factor -> seeded
    values.  CSC float64, diagonal first in every column."""
    import tri_forms as TF
    kind, n, seed = TF.FIXTURES[name]
    rng = np.random.default_rng(seed)
    if kind == "ndchain":
        A = TF.nd_chain(n, rng)
    elif kind == "tree":
        A = TF.tree(n, rng)
    else:
        A = TF.spd(n, "random" if kind == "incomplete" else kind, rng)
    L = symbolic_factor(A).astype(np.float64)
    vals = np.random.default_rng(seed)
    L.data[:] = vals.uniform(-0.5, 0.5, L.nnz)
    L.data[L.indptr[:-1]] = vals.uniform(1.0, 2.0, n)
    assert np.array_equal(L.indices[L.indptr[:-1]], np.arange(n))
    if kind == "incomplete":
        L = TF.drop_entries(L, vals)
        assert np.array_equal(L.indices[L.indptr[:-1]], np.arange(n))
    return L


def groups(kind, m):
    if kind == "none":
        return None
    g = np.full(m, -1, dtype=np.int32)
    k = 3 * ((m - 6) // 3)
    g[:k] = np.arange(k) // 3
    return g


def child(which):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(ENV[which])   # before the library loads: read once
    from cora_amd import capi
    from tri_forms_worker import switches
    capi.load()

    def run(cid, L, gkind, aux_ok, env):
        with switches(env):
            key = (aux_ok, tuple(env.items()))
            if key not in shapes:   # (the probe takes no groups: once for both group kinds)
                shapes[key] = capi.factor_plan_host(L.indptr, L.indices, L.data, aux_ok=aux_ok)
            dig = capi.factor_plan_digest(L.indptr, L.indices, L.data, group=groups(gkind, L.shape[0]), aux_ok=aux_ok)
        shape = shapes[key]
        print("CASE " + json.dumps(dict(id=cid, digest=["%016x" % d for d in dig], form=shape["form"], aux_sum=shape["aux_sum"],
                                        blocks=shape["blocks"])), flush=True)

    for name in FIXTURE_NAMES:
        L = seeded_factor(name)   # once per fixture
        shapes = {}
        for gkind, aux_ok, sw in variants(which):
            cid = "%s/%s/%s/aux%d/%s" % (which, name, gkind, aux_ok, sw)
            run(cid, L, gkind, aux_ok, SWITCHES[sw])
            if cid == THREADS_CASE:
                for nth in (1, 7):
                    run("%s/threads%d" % (cid, nth), L, gkind, aux_ok, {"CORA_TRI_THREADS": str(nth)})
    print("DONE", flush=True)


# ---------------------------------------------------------------- the tests
_children = {}


def _child(which):
    """The cases of a set by id; both children are started at the first call (they run side by side)."""
    if not _children:
        procs = {w: subprocess.Popen([sys.executable, os.path.abspath(__file__), w], stdout=subprocess.PIPE,
                                     stderr=subprocess.STDOUT, text=True) for w in ENV}
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


CASES = [(w, cid) for w in ("A", "B") for cid in case_ids(w)]


def test_the_cases_reach_every_plan_form():
    """Before any digest is compared: one explicit inverse, dense blocks, substitution blocks with the aux sums folded
    and as a product of their own (a table that never saw a substitution block would prove little)."""
    from cora_amd import capi
    cases = [_child(w)[cid] for w, cid in CASES]
    forms = {c["form"] for c in cases}
    assert forms == {capi.FORM_PLAIN, capi.FORM_DENSE, capi.FORM_SUB}
    assert {c["aux_sum"] for c in cases if c["form"] == capi.FORM_SUB} == {0, 1}
    assert _child("A")[THREADS_CASE]["form"] == capi.FORM_SUB and _child("A")[THREADS_CASE]["blocks"] >= 10


@pytest.mark.parametrize("which,cid", CASES, ids=[c[1] for c in CASES])
def test_plan_digest_is_the_recorded_one(which, cid):
    got = _child(which)[cid]["digest"]
    print("\n%s %s %s" % (cid, got[0], got[1]))
    assert cid in DIGESTS, "no digest recorded for %s" % cid
    assert tuple(got) == DIGESTS[cid]


def test_checking_the_elimination_tree_changes_no_plan():
    """CORA_TRI_CHECK_ETREE computes the tree both ways and compares: the plan is the one built without it."""
    for w, cid in CASES:
        if cid.endswith("/etree"):
            assert DIGESTS[cid] == DIGESTS[cid[:-len("etree")] + "default"], cid


def test_plan_is_independent_of_the_thread_count():
    """The substitution blocks of one plan built by 1 and by 7 threads (CORA_TRI_THREADS): the same plan, and the one the
    default thread count builds."""
    cases = _child("A")
    one, seven = cases[THREADS_CASE + "/threads1"], cases[THREADS_CASE + "/threads7"]
    assert one["digest"] == seven["digest"] == cases[THREADS_CASE]["digest"]


# id -> (digest of the integers, digest of the doubles), recorded from the builder before it was cut into phases
DIGESTS = {
    "A/ndchain-1700/none/aux0/default": ("21fc028b50ef48ba", "5615f2f68e8f99d5"),
    "A/ndchain-1700/none/aux1/default": ("b570ef049bf44e04", "30d53959ade3a2d2"),
    "A/ndchain-1700/none/aux1/sub0": ("21fc028b50ef48ba", "5615f2f68e8f99d5"),
    "A/ndchain-1700/none/aux1/unfold": ("3f266adada2c5a93", "c387137d4ca888c9"),
    "A/ndchain-1700/none/aux1/sncap8": ("b570ef049bf44e04", "30d53959ade3a2d2"),
    "A/ndchain-1700/none/aux1/sncap4": ("1f1ca00076b2e937", "2dda24cc2737c3ea"),
    "A/ndchain-1700/none/aux1/etree": ("b570ef049bf44e04", "30d53959ade3a2d2"),
    "A/ndchain-1700/runs3/aux0/default": ("f9a601c4597338a0", "528954a4d8cc2a39"),
    "A/ndchain-1700/runs3/aux1/default": ("89b8777f7b11116f", "bf9df7471f8c2882"),
    "A/ndchain-1700/runs3/aux1/sub0": ("f9a601c4597338a0", "528954a4d8cc2a39"),
    "A/ndchain-1700/runs3/aux1/unfold": ("95c235ffabc1b690", "d144ead87302b67c"),
    "A/ndchain-1700/runs3/aux1/sncap8": ("89b8777f7b11116f", "bf9df7471f8c2882"),
    "A/ndchain-1700/runs3/aux1/sncap4": ("303141372a26071b", "ad93f4581994c5ec"),
    "A/ndchain-1700/runs3/aux1/etree": ("89b8777f7b11116f", "bf9df7471f8c2882"),
    "A/ndchain-2600/none/aux0/default": ("0e66d3dcb027dba8", "558d7238a349b009"),
    "A/ndchain-2600/none/aux1/default": ("ab268a1d1c154f70", "bd1a1202167b3d4a"),
    "A/ndchain-2600/none/aux1/sub0": ("0e66d3dcb027dba8", "558d7238a349b009"),
    "A/ndchain-2600/none/aux1/unfold": ("f801da27b7980a83", "1da40a0ea4bcffd8"),
    "A/ndchain-2600/none/aux1/sncap8": ("ab268a1d1c154f70", "bd1a1202167b3d4a"),
    "A/ndchain-2600/none/aux1/sncap4": ("433ed6159062d104", "8c471c890913571c"),
    "A/ndchain-2600/none/aux1/etree": ("ab268a1d1c154f70", "bd1a1202167b3d4a"),
    "A/ndchain-2600/runs3/aux0/default": ("2662dbd79d311f80", "af322524f1b08909"),
    "A/ndchain-2600/runs3/aux1/default": ("0c0ce51b0696ca44", "0f3374bac1db2ec5"),
    "A/ndchain-2600/runs3/aux1/sub0": ("2662dbd79d311f80", "af322524f1b08909"),
    "A/ndchain-2600/runs3/aux1/unfold": ("632864f83e20338e", "2b3bfb6ec042719e"),
    "A/ndchain-2600/runs3/aux1/sncap8": ("0c0ce51b0696ca44", "0f3374bac1db2ec5"),
    "A/ndchain-2600/runs3/aux1/sncap4": ("11f4419db6928c8b", "0ab39de2a31bdd45"),
    "A/ndchain-2600/runs3/aux1/etree": ("0c0ce51b0696ca44", "0f3374bac1db2ec5"),
    "A/ndchain-4300/none/aux0/default": ("3059eef1ef0316ce", "3f6891eeeccec355"),
    "A/ndchain-4300/none/aux1/default": ("42ebd7fbbfe1b7d8", "aafa2718f7fb1caf"),
    "A/ndchain-4300/none/aux1/sub0": ("3059eef1ef0316ce", "3f6891eeeccec355"),
    "A/ndchain-4300/none/aux1/unfold": ("30f360d42581619f", "95ae410ee55e8a62"),
    "A/ndchain-4300/none/aux1/sncap8": ("42ebd7fbbfe1b7d8", "aafa2718f7fb1caf"),
    "A/ndchain-4300/none/aux1/sncap4": ("de0d023379143922", "35c334d53f1cd451"),
    "A/ndchain-4300/none/aux1/etree": ("42ebd7fbbfe1b7d8", "aafa2718f7fb1caf"),
    "A/ndchain-4300/runs3/aux0/default": ("2936962347f9aba9", "c6cf0468cb22cfcd"),
    "A/ndchain-4300/runs3/aux1/default": ("7b96cfbadf48caf4", "6549716691614439"),
    "A/ndchain-4300/runs3/aux1/sub0": ("2936962347f9aba9", "c6cf0468cb22cfcd"),
    "A/ndchain-4300/runs3/aux1/unfold": ("dc76fce7f71033e5", "86be4df748c08b9f"),
    "A/ndchain-4300/runs3/aux1/sncap8": ("7b96cfbadf48caf4", "6549716691614439"),
    "A/ndchain-4300/runs3/aux1/sncap4": ("6626c14ec1240533", "c83259f64635acf1"),
    "A/ndchain-4300/runs3/aux1/etree": ("7b96cfbadf48caf4", "6549716691614439"),
    "A/random-1600/none/aux0/default": ("a0b6b88693ac1547", "b19041f990cfb1ad"),
    "A/random-1600/none/aux1/default": ("a0b6b88693ac1547", "b19041f990cfb1ad"),
    "A/random-1600/none/aux1/sub0": ("a0b6b88693ac1547", "b19041f990cfb1ad"),
    "A/random-1600/none/aux1/unfold": ("a0b6b88693ac1547", "b19041f990cfb1ad"),
    "A/random-1600/none/aux1/sncap8": ("a0b6b88693ac1547", "b19041f990cfb1ad"),
    "A/random-1600/none/aux1/sncap4": ("a0b6b88693ac1547", "b19041f990cfb1ad"),
    "A/random-1600/none/aux1/etree": ("a0b6b88693ac1547", "b19041f990cfb1ad"),
    "A/random-1600/runs3/aux0/default": ("025a3bed81bc18d7", "2d12db248f2aa299"),
    "A/random-1600/runs3/aux1/default": ("025a3bed81bc18d7", "2d12db248f2aa299"),
    "A/random-1600/runs3/aux1/sub0": ("025a3bed81bc18d7", "2d12db248f2aa299"),
    "A/random-1600/runs3/aux1/unfold": ("025a3bed81bc18d7", "2d12db248f2aa299"),
    "A/random-1600/runs3/aux1/sncap8": ("025a3bed81bc18d7", "2d12db248f2aa299"),
    "A/random-1600/runs3/aux1/sncap4": ("025a3bed81bc18d7", "2d12db248f2aa299"),
    "A/random-1600/runs3/aux1/etree": ("025a3bed81bc18d7", "2d12db248f2aa299"),
    "A/random-2600/none/aux0/default": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/none/aux1/default": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/none/aux1/sub0": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/none/aux1/unfold": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/none/aux1/sncap8": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/none/aux1/sncap4": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/none/aux1/etree": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/runs3/aux0/default": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/runs3/aux1/default": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/runs3/aux1/sub0": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/runs3/aux1/unfold": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/runs3/aux1/sncap8": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/runs3/aux1/sncap4": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/random-2600/runs3/aux1/etree": ("c7d05a10cdf6cc28", "1728abcc0a23112b"),
    "A/arrow-2500/none/aux0/default": ("1951228d0fe45002", "97e0bf0bf7685729"),
    "A/arrow-2500/none/aux1/default": ("1951228d0fe45002", "97e0bf0bf7685729"),
    "A/arrow-2500/none/aux1/sub0": ("1951228d0fe45002", "97e0bf0bf7685729"),
    "A/arrow-2500/none/aux1/unfold": ("1951228d0fe45002", "97e0bf0bf7685729"),
    "A/arrow-2500/none/aux1/sncap8": ("1951228d0fe45002", "97e0bf0bf7685729"),
    "A/arrow-2500/none/aux1/sncap4": ("1951228d0fe45002", "97e0bf0bf7685729"),
    "A/arrow-2500/none/aux1/etree": ("1951228d0fe45002", "97e0bf0bf7685729"),
    "A/arrow-2500/runs3/aux0/default": ("7730a20a9d37be64", "525e171a8840037c"),
    "A/arrow-2500/runs3/aux1/default": ("7730a20a9d37be64", "525e171a8840037c"),
    "A/arrow-2500/runs3/aux1/sub0": ("7730a20a9d37be64", "525e171a8840037c"),
    "A/arrow-2500/runs3/aux1/unfold": ("7730a20a9d37be64", "525e171a8840037c"),
    "A/arrow-2500/runs3/aux1/sncap8": ("7730a20a9d37be64", "525e171a8840037c"),
    "A/arrow-2500/runs3/aux1/sncap4": ("7730a20a9d37be64", "525e171a8840037c"),
    "A/arrow-2500/runs3/aux1/etree": ("7730a20a9d37be64", "525e171a8840037c"),
    "A/incomplete-2600/none/aux0/default": ("e6b0e2ebc2c2fcde", "511b25c198136f99"),
    "A/incomplete-2600/none/aux1/default": ("e6b0e2ebc2c2fcde", "511b25c198136f99"),
    "A/incomplete-2600/none/aux1/sub0": ("e6b0e2ebc2c2fcde", "511b25c198136f99"),
    "A/incomplete-2600/none/aux1/unfold": ("e6b0e2ebc2c2fcde", "511b25c198136f99"),
    "A/incomplete-2600/none/aux1/sncap8": ("e6b0e2ebc2c2fcde", "511b25c198136f99"),
    "A/incomplete-2600/none/aux1/sncap4": ("e6b0e2ebc2c2fcde", "511b25c198136f99"),
    "A/incomplete-2600/none/aux1/etree": ("e6b0e2ebc2c2fcde", "511b25c198136f99"),
    "A/incomplete-2600/runs3/aux0/default": ("be1c6b99f304619c", "33e52f13a42f4488"),
    "A/incomplete-2600/runs3/aux1/default": ("be1c6b99f304619c", "33e52f13a42f4488"),
    "A/incomplete-2600/runs3/aux1/sub0": ("be1c6b99f304619c", "33e52f13a42f4488"),
    "A/incomplete-2600/runs3/aux1/unfold": ("be1c6b99f304619c", "33e52f13a42f4488"),
    "A/incomplete-2600/runs3/aux1/sncap8": ("be1c6b99f304619c", "33e52f13a42f4488"),
    "A/incomplete-2600/runs3/aux1/sncap4": ("be1c6b99f304619c", "33e52f13a42f4488"),
    "A/incomplete-2600/runs3/aux1/etree": ("be1c6b99f304619c", "33e52f13a42f4488"),
    "A/tree-2000/none/aux0/default": ("a14a097e0e11b45a", "34c8ce6646a5f715"),
    "A/tree-2000/none/aux1/default": ("fd382385e7d84b73", "05aae887fbcb28f1"),
    "A/tree-2000/none/aux1/sub0": ("a14a097e0e11b45a", "34c8ce6646a5f715"),
    "A/tree-2000/none/aux1/unfold": ("a4c73c6287514c71", "f3339cd712524ff7"),
    "A/tree-2000/none/aux1/sncap8": ("fd382385e7d84b73", "05aae887fbcb28f1"),
    "A/tree-2000/none/aux1/sncap4": ("fd382385e7d84b73", "05aae887fbcb28f1"),
    "A/tree-2000/none/aux1/etree": ("fd382385e7d84b73", "05aae887fbcb28f1"),
    "A/tree-2000/runs3/aux0/default": ("a14a097e0e11b45a", "34c8ce6646a5f715"),
    "A/tree-2000/runs3/aux1/default": ("9d9d12b828db74a6", "05aae887fbcb28f1"),
    "A/tree-2000/runs3/aux1/sub0": ("a14a097e0e11b45a", "34c8ce6646a5f715"),
    "A/tree-2000/runs3/aux1/unfold": ("23bcfcea34dc221c", "f3339cd712524ff7"),
    "A/tree-2000/runs3/aux1/sncap8": ("9d9d12b828db74a6", "05aae887fbcb28f1"),
    "A/tree-2000/runs3/aux1/sncap4": ("9d9d12b828db74a6", "05aae887fbcb28f1"),
    "A/tree-2000/runs3/aux1/etree": ("9d9d12b828db74a6", "05aae887fbcb28f1"),
    "B/ndchain-1700/none/aux1/default": ("05028a3314a056a1", "f12923f0e7c13369"),
    "B/ndchain-1700/runs3/aux1/default": ("05028a3314a056a1", "f12923f0e7c13369"),
    "B/ndchain-2600/none/aux1/default": ("2796bdb7f058d152", "457087456cff5141"),
    "B/ndchain-2600/runs3/aux1/default": ("2796bdb7f058d152", "457087456cff5141"),
    "B/ndchain-4300/none/aux1/default": ("96bb47beeabccde3", "68279cf806295451"),
    "B/ndchain-4300/runs3/aux1/default": ("96bb47beeabccde3", "68279cf806295451"),
    "B/random-1600/none/aux1/default": ("dad72676c05b2b50", "ebc7a677c978cc8d"),
    "B/random-1600/runs3/aux1/default": ("dad72676c05b2b50", "ebc7a677c978cc8d"),
    "B/random-2600/none/aux1/default": ("437ca0061f1ccaaf", "b352bae4c591ad01"),
    "B/random-2600/runs3/aux1/default": ("437ca0061f1ccaaf", "b352bae4c591ad01"),
    "B/arrow-2500/none/aux1/default": ("abd8ec26598e2e3b", "bc5733faa9197271"),
    "B/arrow-2500/runs3/aux1/default": ("892cd5dea7ec1d46", "16206a3cf4762784"),
    "B/incomplete-2600/none/aux1/default": ("c5df049231f82258", "06aa960226e6f711"),
    "B/incomplete-2600/runs3/aux1/default": ("c5df049231f82258", "06aa960226e6f711"),
    "B/tree-2000/none/aux1/default": ("b55d0bcf3f36b018", "d6900c800e73a4fd"),
    "B/tree-2000/runs3/aux1/default": ("b55d0bcf3f36b018", "d6900c800e73a4fd"),
}


if __name__ == "__main__":
    child(sys.argv[1])
