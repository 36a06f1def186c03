"""The edge-shape fixture (tests/edge_shapes.py) pinned on the CPU: the
staircase's closed form against the oracle's trees, and what every batch
builder promises (the GPU tests of test_gpu_edge_shapes.py rely on both)."""
import numpy as np
import pytest

import edge_shapes as E


@pytest.mark.parametrize("m,part,arity,relax", [(2652, "basic", 8, 0), (700, "basic", 8, 0), (700, "greedy", 2, 10),
                                                 (700, "basic", 16, 0), (700, "basic", 2, 0)])
def test_staircase_closed_form_against_oracle(oracle_mod, m, part, arity, relax):
    dense = E.staircase(m)
    assert dense.shape == (m + 1, m) and not dense[0].any() and dense[m].all()
    np.testing.assert_array_equal(dense.sum(axis=1), np.arange(m + 1))
    t = oracle_mod.OracleTree.from_dense(dense, part, arity, relax)
    assert t.num_relations() == m * (m + 1) // 2
    rows = E.sweep_rows(m)
    off, cols = t.get_rows(rows)
    assert E.closed_form_ok(off, cols, E.staircase_count(rows, m))
    np.testing.assert_array_equal(np.diff(off.astype(np.int64))[: m + 1], np.arange(m + 1))
    # one reference for all rows serves every batch
    off_all, cols_all = t.get_rows(np.arange(m + 1, dtype=np.uint64))
    g_off, g_cols = E.gather_csr(off_all, cols_all, rows)
    np.testing.assert_array_equal(g_off, off)
    np.testing.assert_array_equal(g_cols, cols)


def test_staircase_pad_rows():
    m = 20
    empty = E.staircase(m, pad=50)
    assert empty.shape == (m + 51, m) and not empty[m + 1:].any()
    rep = E.staircase(m, pad=50, repeat=True)
    np.testing.assert_array_equal(rep[m + 1:], np.concatenate([rep[: m + 1]] * 3)[:50])
    one = E.staircase(m, pad=50, single=True)
    np.testing.assert_array_equal(one[: m + 1], empty[: m + 1])
    np.testing.assert_array_equal(np.nonzero(one[m + 1:])[1], np.arange(50) % m)
    for repeat, single, d in ((False, False, empty), (True, False, rep), (False, True, one)):
        np.testing.assert_array_equal(E.staircase_count(np.arange(m + 51), m, repeat, single), d.sum(axis=1))
    # the closed-form check rejects a wrong CSR
    off = np.array([0, 2, 5], dtype=np.uint64)
    assert E.closed_form_ok(off, np.array([1, 0, 2, 0, 1]), [2, 3])
    assert not E.closed_form_ok(off, np.array([1, 0, 2, 0, 3]), [2, 3])
    assert not E.closed_form_ok(off, np.array([1, 0, 2, 0, 1]), [3, 2])
    assert not E.closed_form_ok(off, np.array([1, 0, 2, 0]), [2, 3])


def test_batch_builders_small_matrix():
    """64 columns (the binary variable-length case): totals up to a tile of
    full rows, the heavy rows that exist."""
    m = 64
    for lo, hi in E.TILE_TOTAL_WINDOWS:
        tiles = E.tile_totals(m, lo, hi).reshape(-1, 64).astype(np.int64)
        np.testing.assert_array_equal(tiles.sum(axis=1), np.arange(lo, min(hi, 64 * m) + 1))
        assert int(tiles.max()) <= m
    assert E.geometry_heavy(m) == (m,)
    assert sorted(dict(E.copies(m))) == sorted(f"{n}x{k}" for k in (16, 17, 63, 64) for n in (64, 65))


@pytest.mark.parametrize("m", [700, 2652])
def test_batch_builders(m):
    sw = E.sweep_rows(m)
    assert len(sw) == 2 * (m + 1) and sw[0] == 0 and sw[m] == m and sw[m + 1] == m and sw[-1] == 0
    seen = set()
    for lo, hi in E.TILE_TOTAL_WINDOWS:
        rows = E.tile_totals(m, lo, hi)
        assert len(rows) == 64 * (hi - lo + 1) and int(rows.max()) <= m
        tiles = rows.reshape(-1, 64).astype(np.int64)
        np.testing.assert_array_equal(tiles.sum(axis=1), np.arange(lo, hi + 1))
        for i, tile in enumerate(tiles):
            nzl = np.nonzero(tile)[0].tolist()
            pair = E._LANE_PAIRS[i % 3]
            if lo + i <= 2 * m:   # two heavy rows, 62 copies of row 0
                assert set(nzl) <= set(pair)
                if len(nzl) == 2:
                    seen.add(pair)
            else:
                assert int((tile == m).sum()) >= (lo + i - 1) // m - 2   # full rows, then two rows
    assert seen == set(E._LANE_PAIRS)
    # the windows straddle 512 and every capacity a build may choose
    for edge in (512, 1024, 2048, 4096):
        assert any(lo <= edge < hi for lo, hi in E.TILE_TOTAL_WINDOWS)
    assert E.geometry_heavy(m) == (254, 255, 256, m)
    for k in E.geometry_heavy(m):
        g = dict(E.geometry(m, k))
        assert len(g) == 3 * len(E.GEOMETRY_SIZES)
        for n in E.GEOMETRY_SIZES:
            f, l, a = g[f"first-{n}"], g[f"last-{n}"], g[f"alone-{n}"]
            assert len(f) == len(l) == len(a) == n
            assert f[0] == k and l[n - 1] == k and a[n // 2] == k and int(a.sum()) == k
            assert int(f[1:].max(initial=0)) <= 7 and int(l[:-1].max(initial=0)) <= 7
    c = dict(E.copies(m))
    assert sorted(c) == sorted(f"{n}x{k}" for k in E.COPIES_LABELS for n in (64, 65))
    assert all(len(set(v.tolist())) == 1 for v in c.values())
    assert 64 * 16 <= 1024 < 64 * 17 and 64 * 63 < 4096 <= 64 * 64 < 64 * 65


# ---- the node-image fixtures ----------------------------------------------------

def _tile_totals_64(m, lo, hi):
    """tile_totals as it stood before the tile size became a parameter."""
    tiles = []
    for i, T in enumerate(range(lo, min(hi, 64 * m) + 1)):
        tile = np.zeros(64, dtype=np.uint64)
        p0, p1 = ((0, 63), (0, 1), (31, 32))[i % 3]
        free = [l for l in range(64) if l not in (p0, p1)]
        rest = T
        while rest > 2 * m:
            tile[free.pop(0)] = m
            rest -= m
        a = (1, rest // 2, min(m, rest))[(i // 3) % 3]
        a = min(max(a, rest - m, 0), min(m, rest))
        tile[p0], tile[p1] = a, rest - a
        tiles.append(tile)
    return np.concatenate(tiles)


@pytest.mark.parametrize("m", [64, 700, 2652])
def test_tile_totals_default_unchanged(m):
    assert E.lane_pairs(64) == E._LANE_PAIRS and E.TILE == 64
    for lo, hi in E.TILE_TOTAL_WINDOWS + ((1, 40), (126, 130)):
        want = _tile_totals_64(m, lo, hi)
        for got in (E.tile_totals(m, lo, hi), E.tile_totals(m, lo, hi, 64), E.tile_totals(m, lo, hi, lanes=E._LANE_PAIRS)):
            assert got.dtype == want.dtype
            np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("tile,pairs", [(16, ((0, 15), (0, 1), (7, 8))), (8, ((0, 7), (0, 1), (3, 4)))])
@pytest.mark.parametrize("m", [32, 70, 256, 512])
def test_tile_totals_node_tiles(tile, pairs, m):
    """The totals and the lane promises of the 64-row builder at the node
    kernels' 16-row rowblocks and 8-row chunks."""
    assert E.lane_pairs(tile) == pairs
    seen = set()
    for lo, hi in ((14, 18), (62, 66), (126, 130), (254, 258), (510, 514), (1022, 1026), (16 * 64 - 2, 16 * 64 + 2)):
        rows = E.tile_totals(m, lo, hi, tile=tile)
        top = min(hi, tile * m)
        assert len(rows) == tile * max(0, top - lo + 1) and int(rows.max(initial=0)) <= m
        tiles = rows.reshape(-1, tile).astype(np.int64)
        np.testing.assert_array_equal(tiles.sum(axis=1), np.arange(lo, top + 1))
        for i, t in enumerate(tiles):
            nzl = np.nonzero(t)[0].tolist()
            pair = pairs[i % 3]
            if lo + i <= 2 * m:   # two heavy rows, tile - 2 copies of row 0
                assert set(nzl) <= set(pair)
                if len(nzl) == 2:
                    seen.add(pair)
            else:                 # full rows, then two rows
                assert int((t == m).sum()) >= (lo + i - 1) // m - 2
    assert seen == set(pairs)
    # caller-given lanes
    rows = E.tile_totals(m, 20, 22, tile=tile, lanes=((2, 5),))
    assert all(set(np.nonzero(t)[0].tolist()) <= {2, 5} for t in rows.reshape(-1, tile))


# (m, top, shifts, partitioner, arity): the trees test_gpu_node_edges.py builds over windows();
# the shifts hold 0, one that straddles a boundary between two children of the root, and m - top
WINDOW_TREES = [E.WINDOWS_DEEP + ("basic", 2), E.windows_wide(16384) + ("basic", 8), E.windows_wide(16385) + ("basic", 8)]


@pytest.mark.parametrize("m,top,shifts,part,arity", WINDOW_TREES)
def test_windows_closed_form_against_oracle(oracle_mod, m, top, shifts, part, arity):
    dense = E.windows(m, top, shifts)
    n = len(shifts) * (top + 1)
    assert dense.shape == (n, m) and dense[:, 0].any() and dense[:, m - 1].any()
    ids = np.arange(n)
    np.testing.assert_array_equal(dense.sum(axis=1), E.windows_count(ids, top))
    np.testing.assert_array_equal(E.windows_count(ids, top), np.tile(np.arange(top + 1), len(shifts)))
    np.testing.assert_array_equal(E.windows_shift(ids, top, shifts), np.repeat(shifts, top + 1))
    assert shifts[0] == 0 and shifts[-1] == m - top
    t = oracle_mod.OracleTree.from_dense(dense, part, arity)
    ex = t.export()
    # a root-child boundary strictly inside one shift's widest row
    nc, fc = np.asarray(ex["num_children"]), np.asarray(ex["first_child"])

    lc = np.asarray(ex["leaf_column"])

    def leaves(u):   # the leaf columns below u, in pre-order
        return [int(lc[u])] if nc[u] == 0 else [x for c in range(int(nc[u])) for x in leaves(int(fc[u]) + c)]
    below = [leaves(int(fc[0]) + c) for c in range(int(nc[0]))]
    bounds = np.cumsum([len(b) for b in below])[:-1]
    assert sum(below, []) == list(range(m))   # (pre-order is column order: the order of a row's labels)
    if len(shifts) > 2:
        assert any(s < b < s + top for s in shifts for b in bounds), (shifts, bounds)
    off, cols = t.get_rows(ids.astype(np.uint64))
    assert E.closed_form_ok(off, cols, E.windows_count(ids, top), E.windows_shift(ids, top, shifts))
    assert not E.closed_form_ok(off, cols, E.windows_count(ids, top), E.windows_shift(ids, top, shifts) + 1)
    assert not E.closed_form_ok(off, cols, E.windows_count(ids, top))
    # row ids by label count, the shift cycling
    want = np.array([5, 0, top, 1, 2, 3, 4], dtype=np.uint64)
    rows = E.windows_rows(want, top, len(shifts))
    np.testing.assert_array_equal(E.windows_count(rows, top), want)
    np.testing.assert_array_equal(E.windows_shift(rows, top, shifts), np.asarray(shifts)[np.arange(7) % len(shifts)])
    g_off, g_cols = E.gather_csr(off, cols, rows)
    assert E.closed_form_ok(g_off, g_cols, want, E.windows_shift(rows, top, shifts))


def test_node_geometry():
    assert E.NODE_SIZES == (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 113, 449)
    for k in (0, 1, 33, 257):
        g = dict(E.node_geometry(k))
        assert len(g) == 3 * len(E.NODE_SIZES)
        for n in E.NODE_SIZES:
            f, l, a = g[f"first-{n}"], g[f"last-{n}"], g[f"alone-{n}"]
            assert len(f) == len(l) == len(a) == n
            assert f[0] == k and l[n - 1] == k and a[n // 2] == k and int(a.sum()) == k
            assert int(f[1:].max(initial=0)) <= 7 and int(l[:-1].max(initial=0)) <= 7
    assert [name for name, _ in E.node_geometry(9, (255, 256))] == ["first-255", "last-255", "alone-255", "first-256",
                                                                  "last-256", "alone-256"]
