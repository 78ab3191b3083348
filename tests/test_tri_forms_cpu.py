"""The fixtures of the staged Cholesky solve's GPU tests (tests/tri_forms.py) take the plan forms they are meant to take,
and the plans solve their systems -- without a GPU: every case of tests/tri_forms_worker.py in its `host` mode, one child
process per environment set (the sets of tests/test_gpu_tri_forms.py: the switches that decide a plan's form are read
once, when the library loads).  Per case
  - the host probe (cora_debug_factor_plan_host) reports the intended form: stages, kind of stage-0 blocks, where the aux
    sums go, tile size, row classes, chunks per row -- a fixture that drifts to another form fails here; and the device
    image of the plan under the case's row map, groups and layout (cora_debug_factor_image, on a plan-only handle) takes
    the decisions the case names: row I/O from run tables or index lists (io_runs), the projection in the sweeps (fuse_ok);
  - the plan's products executed on the host (cora_debug_factor_solve_host) meet the bound of the GPU test: 1e-11 for
    complete factors, 1e-10 for the incomplete one, 1e-8 for the regularised Q + lambda I (tests/test_trisolve_cpu.py,
    tests/test_gpu_stpcg_forms.py), relative to the reference's largest entry;
  - the reference against itself (one refinement step with a long-double residual against none; the STPCG reference
    with long-double inner products against plain ones) stays under 1/100 of that bound.
Observed: host emulation <= 1.2e-15 (complete and incomplete), 2.2e-13 (regularised); spread <= 8e-16, 5.5e-14 and, for
the three STPCG iterations, 5.4e-13."""
import json
import os
import subprocess
import sys

import pytest

import tri_forms_worker as W

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tri_forms_worker.py")
SETS = ("A", "B", "C", "C0", "P")
_children = {}


def _child(which):
    if which not in _children:
        r = subprocess.run([sys.executable, WORKER, which, "host"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=300)
        cases = {}
        for line in r.stdout.splitlines():
            if line.startswith("CASE "):
                c = json.loads(line[5:])
                cases[c["id"]] = c
        assert r.returncode == 0 and "DONE" in r.stdout.splitlines(), r.stdout[-4000:]
        _children[which] = cases
    return _children[which]


CASES = [(s, cid) for s in SETS for cid in W.case_ids(s) if cid not in ("reinstall", "errors")]


@pytest.mark.parametrize("which,cid", CASES, ids=["%s-%s" % c for c in CASES])
def test_fixture_takes_its_form_and_the_plan_solves_it(which, cid):
    cases = _child(which)
    assert cid in cases, "the child printed nothing for %s" % cid
    c = cases[cid]
    print("\n%s %s: %s\n  %s" % (which, cid, c["shape"], "  ".join("%s %.2e" % (n, v) for n, v, _ in c["checks"])))
    assert c["fail"] == []
    kinds = [k for _, _, k in c["checks"]]
    assert any(k.startswith("spread-") for k in kinds), "no reference spread"
    if not cid.startswith(("proj-", "stpcg-")):   # (those compare on the device only; here: their reference's spread)
        assert any(not k.startswith("spread-") for k in kinds), "nothing was solved"
    for name, value, kind in c["checks"]:
        assert value <= W.BOUND[kind], (name, value, W.BOUND[kind])


def test_every_form_is_among_the_cases():
    """Over all sets: one inverse, substitution blocks with the aux sums folded and as their own product, dense blocks
    in 2 and in 3 stages, substitution blocks on a structure that is no chain, an incomplete factor, a product with all
    three row classes, a row of more than 64 chunks, a tile above 64 KB, 8 entries per lane in a level -- and both
    answers of either decision of the device image."""
    shapes = {(s, cid): _child(s)[cid] for s, cid in CASES if not cid.startswith(("proj-", "stpcg-"))}
    sh = {k: c["shape"] for k, c in shapes.items()}
    fx = {k: c["fixture"] for k, c in shapes.items()}

    def some(pred):
        return [k for k in sh if pred(sh[k], fx[k])]

    assert some(lambda s, f: s["stages"] == 1 and s["form"] == W.PLAIN)
    assert some(lambda s, f: s["form"] == W.SUB and s["aux_sum"] == 0 and s["aux_rows"] > 0)
    assert some(lambda s, f: s["form"] == W.SUB and s["aux_sum"] == 1)
    assert some(lambda s, f: s["form"] == W.DENSE and s["stages"] == 2)
    assert some(lambda s, f: s["form"] == W.DENSE and s["stages"] == 3)
    assert some(lambda s, f: s["form"] == W.SUB and f.startswith("tree"))
    assert some(lambda s, f: f.startswith("incomplete") and s["stages"] >= 2)
    assert some(lambda s, f: s["mixed_products"] >= 1)
    assert some(lambda s, f: s["max_chunks"] > 64)
    assert some(lambda s, f: s["form"] == W.SUB and s["lds24"] > W.TILE_LIMIT and s["max_rows"] >= 342)
    assert some(lambda s, f: s["form"] == W.SUB and s["max_npl"] == 8)
    for key in W.IMAGE_KEYS:
        for answer in (0, 1):
            assert some(lambda s, f: s["form"] == W.SUB and s[key] == answer), (key, answer)
