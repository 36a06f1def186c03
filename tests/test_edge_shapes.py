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
