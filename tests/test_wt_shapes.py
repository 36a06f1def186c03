"""The BinRel-WT fixture (tests/wt_shapes.py) pinned on the CPU: the chunk
rule and the device-byte formula on hand-worked values, what every builder
and batch builder promises, and the numpy reference against a dense matrix
(the GPU tests of test_gpu_binrel_wt_edges.py rely on all of it)."""
import numpy as np
import pytest

import wt_shapes as S


def test_chunk_rule_and_widths():
    # k: the largest value <= 24 with 2^k * m < 2^31
    for m, k in ((0, 24), (1, 24), (3, 24), (127, 24), (128, 23), (2652, 19), (3173, 19), (8192, 17), (8193, 17),
                 (1 << 20, 10), ((1 << 21) - 1, 10), (1 << 21, 9), ((1 << 30) - 1, 1), (1 << 30, 0),
                 ((1 << 31) - 1, 0), (1 << 31, 0), ((1 << 32) - 1, 0), (1 << 32, 0), ((1 << 32) + 10, 0)):
        assert S.chunk_log2(m) == k, m
        assert k == 24 or (1 << (k + 1)) * m >= 1 << 31
        assert k == 0 or (1 << k) * max(m, 1) < 1 << 31
    for m, w in ((1, 1), (2, 1), (3, 2), (256, 8), (257, 9), (8192, 13), (1 << 20, 20), ((1 << 30) - 1, 30),
                 ((1 << 31) - 1, 31), (1 << 31, 31), ((1 << 31) + 1, 32), ((1 << 32) - 1, 32), (1 << 32, 32),
                 ((1 << 32) + 10, 32)):
        assert S.symbol_bits(m) == w and S.levels(m) == (w + 1) // 2, m
    assert S.num_chunks(0, 5) == 0 and S.num_chunks(1, 5) == 1
    assert S.num_chunks(1024, 1 << 20) == 1 and S.num_chunks(1025, 1 << 20) == 2


def test_expected_device_bytes_by_hand():
    # 5 rows over 2^20 columns: one chunk of 209 symbols, 10 levels of 2 + 1 blocks
    off = np.array([0, 0, 208, 208, 209, 209], dtype=np.uint64)
    assert S.expected_device_bytes(off, 1 << 20) == 6 * 8 + 10 * 64 * 3
    # the same rows over 2^31 - 1 columns: five chunks of 0, 208, 0, 1, 0 symbols, 16 levels
    np.testing.assert_array_equal(S.chunk_lengths(off, (1 << 31) - 1), [0, 208, 0, 1, 0])
    assert S.expected_device_bytes(off, (1 << 31) - 1) == 6 * 8 + 16 * 64 * (1 + 2 + 1 + 2 + 1)
    # two rows a chunk at 2^30 - 1 columns: 208, 1, 0 symbols, 15 levels
    np.testing.assert_array_equal(S.chunk_lengths(off, (1 << 30) - 1), [208, 1, 0])
    assert S.expected_device_bytes(off, (1 << 30) - 1) == 6 * 8 + 15 * 64 * (2 + 2 + 1)
    assert S.expected_device_bytes(np.zeros(1, dtype=np.uint64), 7) == 8


def _digits(cols, m):
    """[levels, 4] occurrence counts of each digit value at each level."""
    lv = S.levels(m)
    c = np.asarray(cols, dtype=np.int64)
    return np.array([np.bincount((c >> (2 * (lv - 1 - l))) & 3, minlength=4) for l in range(lv)])


@pytest.mark.parametrize("m", [(1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32])
def test_chunk_per_row(m):
    off, cols = S.chunk_per_row(m)
    S.check_csr(off, cols, m)
    n = len(off) - 1
    lens = np.diff(off.astype(np.int64))
    assert n == 90 == S.num_chunks(n, m) and S.levels(m) == 16
    assert lens[0] == 0 and lens[-1] == 0
    # the lengths, in order, once per law; the other rows are empty
    np.testing.assert_array_equal(lens[lens > 0], [x for x in S.LENGTHS if x] * 3)
    assert (lens == 0).sum() == 90 - 3 * 26
    for edge in (16, 64, 80, 144, 208, 416, 624):   # word, quarter (words 1, 5, 9 start a load) and block edges
        assert {edge - 1, edge, edge + 1} <= set(S.LENGTHS)
    assert 16 * 1 == 16 and 16 * 5 == 80 and 16 * 9 == 144 and 13 * 16 == 208
    # every digit value at every level; at the top level what the width allows
    d = _digits(cols, m)
    top = ((m - 1) >> 30) + 1
    assert (d[1:] > 0).all() and (d[0, :top] > 0).all() and (d[0, top:] == 0).all(), d
    assert top == (2 if m <= 1 << 31 else 4)
    have = set(cols.tolist())
    assert {0, 1, m - 1, S.ALL_LOW_DIGITS_3} <= have
    if m > 1 << 31:
        assert 0xFFFFFFFE in have and (0xFFFFFFFF in have) == (m == 1 << 32)
    # the laws
    a, b = S.law_ids("consecutive", 625, m), S.law_ids("top-digits", 625, m)
    assert (np.diff(a) == 1).all() and (a[0] >> 8) != (a[-1] >> 8)
    tops = 8 if m <= 1 << 31 else 16
    low = b & ((1 << 28) - 1)
    assert len(set((b >> 28).tolist())) == tops and (low[:tops] == low[0]).all()
    assert len(set(low.tolist())) == -(-625 // tops)
    for law in S.LAWS:
        ids = S.law_ids(law, 625, m)
        assert len(set(ids.tolist())) == 625
        for length in (1, 17, 209):   # a shorter row's ids lie in a longer row's
            assert set(S.law_ids(law, length, m).tolist()) <= set(ids.tolist())


def test_two_rows_per_chunk():
    off, cols = S.two_rows_per_chunk()
    m = S.M_TWO_ROWS
    S.check_csr(off, cols, m)
    lens = np.diff(off.astype(np.int64))
    assert len(lens) == 40 and S.num_chunks(40, m) == 20 and S.levels(m) == 15
    assert set(lens.tolist()) <= set(S.LENGTHS) and lens[S.heavy_row(off)] == S.HEAVY and (lens == 0).any()
    assert len(set(lens.tolist())) >= 20
    d = _digits(cols, m)
    assert (d > 0).all(), d


def test_k10():
    off, cols = S.k10()
    m = S.M_K10
    S.check_csr(off, cols, m)
    lens = np.diff(off.astype(np.int64))
    n = len(lens)
    assert n == 3 * 1024 + 5 and S.num_chunks(n, m) == 4 and S.levels(m) == 10
    assert 2.5 < lens.mean() < 3.5
    assert all(lens[r] > 0 for r in (1023, 1024, 2047, 2048)) and lens[1022] == 0 and lens[1025] == 0
    assert lens[S.K10_HEAVY_ROW] == S.HEAVY == lens.max() and S.heavy_row(off) == S.K10_HEAVY_ROW
    for c, where in S.K10_NAMED.items():
        np.testing.assert_array_equal(S.ref_column(off, cols, c), where)
    chunk = lambda c: sorted(set((S.ref_column(off, cols, c) >> np.uint64(10)).tolist()))
    assert chunk(S.K10_EVERY_CHUNK) == [0, 1, 2, 3] and chunk(S.K10_LAST_CHUNK_ONLY) == [3]
    assert chunk(S.K10_FIRST_CHUNK_ONLY) == [0]
    assert (S.chunk_lengths(off, m) > 0).all() and S.chunk_lengths(off, m).sum() == len(cols)


def test_k17():
    off, cols = S.k17()
    m = S.M_K17
    S.check_csr(off, cols, m)
    lens = np.diff(off.astype(np.int64))
    n = len(lens)
    assert n == 2 * 131072 + 77 and S.num_chunks(n, m) == 3 and S.levels(m) == 7
    assert 1.9 < lens.mean() < 2.1 and 400_000 < len(cols) < 600_000
    assert (lens == 0).any() and lens.max() == 4
    assert S.absent_columns(cols, m) == [2047, 4095, 6143, 8191]
    assert (_digits(cols, m)[1:] > 0).all()


def test_empty_middle():
    off, cols = S.empty_middle()
    m = S.M_EMPTY_MIDDLE
    S.check_csr(off, cols, m)
    n = len(off) - 1
    assert S.num_chunks(n, m) == 3
    cl = S.chunk_lengths(off, m)
    assert cl[0] > 0 and cl[1] == 0 and cl[2] > 0
    for c, where in S.EMPTY_MIDDLE_NAMED.items():
        np.testing.assert_array_equal(S.ref_column(off, cols, c), where)


def test_beyond_32_bits():
    off, cols = S.beyond_32_bits()
    S.check_csr(off, cols, S.M_BEYOND)
    assert len(off) == 21 and S.chunk_log2(S.M_BEYOND) == 0 and S.levels(S.M_BEYOND) == 16
    assert cols[off[3]:off[4]].tolist() == [5, 77, 1 << 31] and cols[off[4]:off[5]].tolist() == [5, 0xFFFFFFFF]
    assert S.ref_get(off, cols, [3, 3, 4], [5, (1 << 32) + 5, 0xFFFFFFFF]).tolist() == [True, False, True]
    assert len(S.ref_column(off, cols, (1 << 32) + 5)) == 0 and 3 in S.ref_column(off, cols, 5)


def test_reference_against_dense():
    rng = np.random.default_rng(3)
    dense = rng.random((60, 23)) < 0.2
    dense[7] = False
    off = np.zeros(61, dtype=np.uint64)
    np.cumsum(dense.sum(axis=1), out=off[1:])
    cols = np.nonzero(dense)[1].astype(np.uint32)
    S.check_csr(off, cols, 23)
    rows = np.array([5, 7, 7, 59, 0, 5], dtype=np.uint64)
    r_off, r_cols = S.ref_rows(off, cols, rows)
    np.testing.assert_array_equal(np.diff(r_off.astype(np.int64)), dense[rows.astype(np.int64)].sum(axis=1))
    np.testing.assert_array_equal(r_cols, np.concatenate([np.nonzero(dense[r])[0] for r in rows.astype(np.int64)]))
    ii, jj = np.meshgrid(np.arange(60), np.arange(23), indexing="ij")
    np.testing.assert_array_equal(S.ref_get(off, cols, ii.ravel(), jj.ravel()), dense.ravel())
    for c in range(23):
        np.testing.assert_array_equal(S.ref_column(off, cols, c), np.nonzero(dense[:, c])[0])
    np.testing.assert_array_equal(S.CsrDense(off, cols, 23)[[3, 7, 3, 59]], dense[[3, 7, 3, 59]])
    assert S.CsrDense(off, cols, 23).shape == (60, 23)
    with pytest.raises(AssertionError):
        S.check_csr(off, cols[::-1], 23)
    with pytest.raises(AssertionError):
        S.check_csr(off, cols, 22)
    # point queries: present ids answer 1, the absent one per row 0
    qr, qc, want = S.point_queries(off, cols, 23)
    np.testing.assert_array_equal(dense[qr.astype(np.int64), qc.astype(np.int64)], want)
    full = int((dense.sum(axis=1) > 0).sum())
    assert want.sum() == 2 * full and (~want).sum() >= 58


@pytest.mark.parametrize("shape", ["chunk_per_row", "two_rows_per_chunk", "k10", "k17", "empty_middle"])
def test_batches(shape):
    off, _ = S.chunk_per_row((1 << 31) - 1) if shape == "chunk_per_row" else getattr(S, shape)()
    lens = np.diff(off.astype(np.int64))
    n_rows, heavy = len(lens), S.heavy_row(off)
    b = dict(S.batches(off))
    assert len(b) == 3 * 5 + 3
    for n in (1, 255, 256, 257, 513):
        f, l, a = b[f"first-{n}"], b[f"last-{n}"], b[f"alone-{n}"]
        assert len(f) == len(l) == len(a) == n and int(max(f.max(), l.max(), a.max())) < n_rows
        assert f[0] == heavy and l[n - 1] == heavy and a[n // 2] == heavy
        assert lens[a.astype(np.int64)].sum() == lens[heavy]
    assert 257 % S.TILE == 1 and 513 % S.TILE == 1   # the heavy row last in a partial tile
    z = b["empty tile, then a non-empty one"].astype(np.int64)
    assert lens[z[: S.TILE]].sum() == 0 and z[S.TILE] == heavy and len(z) > S.TILE + 1
    assert b["300 copies"].tolist() == [heavy] * 300 and len(b["empty batch"]) == 0
    if n_rows > 1 << 17:   # the batches' rows reach every chunk
        assert set((b["first-513"] >> np.uint64(17)).tolist()) == {0, 1, 2}
