"""The device image of the long rows (cora_amd/csrc/long_image.h, through cora_debug_long_image on plan-only handles): on
every entry of tests/topologies.py that has long rows and on the graphs of tests/long_rows_graphs.py, at the library's
piece size and at two small ones that cut the short rows of these graphs too.

Structure: perm permutes each row's range and the image's entries are the CSR row's; every entry lies in exactly one
piece; a row's pieces are consecutive and carry its first / nchunks / slot; the entries of a piece that have a home share
it, and the piece is launched on it (block index mod 8); both slice orders give the same homes; the XCDs' lists are padded
to equal length.  Value: the image multiplied on the host against cora_debug_format_spmm_host on the long rows, 1e-13
of the largest entry -- the two differ in the order of a sum of at most 8401 terms (graph `cut`)."""
import numpy as np
import pytest

import long_rows_graphs as lrg
import topologies as topo
from test_update_values_cpu import pair_factors, plan

TOPO_LONG = ("robots-d2", "hub-d2", "robots-d3", "hub-d3", "fat_landmark", "priors_wide")
CASES = [("topo", n) for n in TOPO_LONG] + [("lrg", n) for n in lrg.NAMES]
PIECES = (0, 64, 256)   # 0: the library's own
BOUND = 1e-13


def problem(case):
    kind, name = case
    if kind == "topo":
        A, Q, dm, g = topo.build(name)
    else:
        A, Q, dm = lrg.build(name)
    return Q, dm


def test_the_list_of_topologies_with_long_rows_is_complete():
    for name in topo.NAMES:
        A, Q, dm, g = topo.build(name)
        ctx = plan(Q, dm, Q.val)
        assert (ctx.format_stats()["long_rows"] > 0) == (name in TOPO_LONG), name
        ctx.close()


def rows_of(I):
    """{slot: indices of its pieces, in the order the last arriver adds them}"""
    ch = I["chunks"]
    out = {}
    for i, s in enumerate(ch["slot"]):
        out.setdefault(int(s), []).append(i)
    return out


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[1])
def test_structure(case, piece):
    Q, dm = problem(case)
    ctx = plan(Q, dm, Q.val)
    st = ctx.format_stats()
    m = ctx.row_map()
    inv = np.full(ctx.rows, -1, dtype=np.int64)
    inv[m] = np.arange(dm.N)
    I = ctx.debug_long_image(piece)
    ch, order, lcol, lval, perm, home = I["chunks"], I["chunk_order"], I["lcol"], I["lval"], I["perm"], I["home"]
    assert I["placed"]
    n_pieces, n_ent = len(ch["row"]), len(lval)
    assert n_ent == st["long_nnz"] and len(rows_of(I)) == st["long_rows"]
    limit = piece if piece > 0 else topo.K_LONG_CHUNK
    assert np.all(ch["k1"] > ch["k0"]) and np.all(ch["k1"] - ch["k0"] <= limit)
    if piece > 0:
        assert n_pieces > st["long_chunks"]   # these sizes do cut the rows

    # every entry in exactly one piece: the pieces tile [0, entries) in index order
    assert ch["k0"][0] == 0 and ch["k1"][-1] == n_ent and np.array_equal(ch["k0"][1:], ch["k1"][:-1])
    # a row's pieces: consecutive from `first`, nchunks of them, one internal row; perm permutes the row's range, and the
    # entries are the CSR row's (internal columns, same values)
    for slot, idx in rows_of(I).items():
        assert idx == list(range(idx[0], idx[0] + len(idx)))
        assert np.all(ch["first"][idx] == idx[0]) and np.all(ch["nchunks"][idx] == len(idx))
        assert len(set(ch["row"][idx].tolist())) == 1
        lo, hi = int(ch["k0"][idx[0]]), int(ch["k1"][idx[-1]])
        assert np.array_equal(np.sort(perm[lo:hi]), np.arange(lo, hi))
        api = int(inv[ch["row"][idx[0]]])
        a, b = Q.rowptr[api], Q.rowptr[api + 1]
        assert hi - lo == b - a > topo.K_LONG_ROW
        # (the format keeps the row in CSR order: position perm[i] of it is CSR entry a + perm[i] - lo)
        assert np.array_equal(lcol[lo:hi], m[Q.col[a:b]][perm[lo:hi] - lo])
        assert np.array_equal(lval[lo:hi], np.asarray(Q.val)[a:b][perm[lo:hi] - lo])

    # homes: every row of X but the long rows has one, and both slice orders agree
    is_long = np.zeros(ctx.rows, dtype=bool)
    is_long[ch["row"]] = True
    assert np.array_equal(home, I["home_pose_first"])
    assert np.all(home[m][~is_long[m]] >= 0) and np.all(home[m][is_long[m]] == -1) and home.max() < 8
    assert np.all(home[inv < 0] == -1)   # padding rows

    # launch order: 8 lists of equal length, every piece once, padding behind the pieces, the longest list full
    assert len(order) % 8 == 0
    cper = len(order) // 8
    lists = order.reshape(8, cper)
    assert np.array_equal(np.sort(order[order >= 0]), np.arange(n_pieces))
    counts = (lists >= 0).sum(axis=1)
    assert counts.max() == cper
    for x in range(8):
        assert np.all(lists[x, :counts[x]] >= 0) and np.all(lists[x, counts[x]:] == -1)
    # a piece's entries that have a home share it, and k_spmm's block (pos % cper) * 8 + x runs it on that XCD
    for pos, ci in enumerate(order):
        if ci < 0:
            continue
        x = pos // cper
        block = (pos % cper) * 8 + x
        h = home[lcol[ch["k0"][ci]:ch["k1"][ci]]]
        assert block % 8 == x and np.all(h[h >= 0] == x), (pos, ci)
        cols = lcol[ch["k0"][ci]:ch["k1"][ci]]
        assert np.all(np.diff(cols) > 0)   # ascending columns inside a piece
    # an entry without a home goes with the row's lowest home; a row's pieces follow the XCDs upwards
    xcd_of = np.zeros(n_pieces, dtype=np.int64)
    xcd_of[order[order >= 0]] = np.nonzero(order >= 0)[0] // cper
    for slot, idx in rows_of(I).items():
        assert np.all(np.diff(xcd_of[idx]) >= 0)
        for ci in idx:
            if xcd_of[ci] != xcd_of[idx[0]]:
                assert np.all(home[lcol[ch["k0"][ci]:ch["k1"][ci]]] >= 0)
    ctx.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[1])
def test_product_of_the_image(case):
    Q, dm = problem(case)
    ctx = plan(Q, dm, Q.val)
    m = ctx.row_map()
    inv = np.full(ctx.rows, -1, dtype=np.int64)
    inv[m] = np.arange(dm.N)
    for piece in PIECES:
        I = ctx.debug_long_image(piece)
        ch = I["chunks"]
        for k in (1, 5):
            X = np.random.default_rng(10 + k).standard_normal((dm.N, k))
            Xi = np.zeros((ctx.rows, k))
            Xi[m] = X
            ref = ctx.debug_format_spmm_host(X)
            rows = sorted(set(int(inv[r]) for r in ch["row"]))
            got = np.zeros((dm.N, k))
            for ci in range(len(ch["row"])):   # piece by piece, in the order the last arriver adds the partials
                lo, hi = ch["k0"][ci], ch["k1"][ci]
                got[inv[ch["row"][ci]]] += I["lval"][lo:hi] @ Xi[I["lcol"][lo:hi]]
            err = np.abs(got[rows] - ref[rows]).max() / np.abs(ref[rows]).max()
            print("%s piece %d k %d: %.2e" % (case[1], piece, k, err))
            assert err <= BOUND
    ctx.close()


def test_shapes_the_graphs_are_built_for():
    """random: per_xcd = 2, XCDs 5-7 empty, every row several pieces; cut: every XCD's run longer than a piece and cut
    again; single: a row of one piece."""
    got = {}
    for name in lrg.NAMES:
        A, Q, dm = lrg.build(name)
        ctx = plan(Q, dm, Q.val)
        I = ctx.debug_long_image()
        lists = I["chunk_order"].reshape(8, -1)
        got[name] = (ctx.format_stats()["slices"], (lists >= 0).sum(axis=1).tolist(), [len(v) for v in rows_of(I).values()])
        ctx.close()
    slices, per, pieces = got["random"]
    assert (slices + 7) // 8 == 2 and per[5:] == [0, 0, 0] and min(per[:5]) > 0 and min(pieces) > 1
    slices, per, pieces = got["cut"]
    assert (slices + 7) // 8 == 17 and min(per) >= 1 and pieces[0] > 8 and max(per) == 2
    slices, per, pieces = got["single"]
    assert 1 in pieces and max(pieces) > 1


def test_partitioned_handles_keep_the_formats_chunks():
    A, Q, dm = lrg.build("random")
    for whole in (False, True):
        for rank in range(2):
            ctx = plan(Q, dm, Q.val, rank=rank, world=2, whole=whole)
            I = ctx.debug_long_image()
            assert not I["placed"]
            assert len(I["chunks"]["row"]) == ctx.format_stats()["long_chunks"] == len(I["chunk_order"])
            assert np.array_equal(I["perm"], np.arange(len(I["perm"]))) and len(I["lval"]) == ctx.format_stats()["long_nnz"]
            ctx.close()


def test_image_follows_new_values():
    A, Q, dm = lrg.build("single")
    vals2 = np.asarray(Q.val) * pair_factors(Q.rowptr, Q.col)
    a, b = plan(Q, dm, Q.val), plan(Q, dm, vals2)
    Ia, Ib = a.debug_long_image(), b.debug_long_image()
    assert np.array_equal(Ia["perm"], Ib["perm"]) and not np.array_equal(Ia["lval"], Ib["lval"])
    a.update_values(Q.rowptr, Q.col, vals2)
    assert np.array_equal(a.debug_long_image()["lval"], Ib["lval"])
    a.close()
    b.close()
