"""GPU parity of mbrwt_create_from_rows (csrc/rows_from.hip): row records
written straight from CSR rows under a tree shape.  Every context is checked
against the oracle tree of the same dense matrix, whose export() gives the
shape: ordered get_rows, get_batch, get_column, count_labels, num_relations,
and mbrwt_tree_export bit for bit (the BRWT over a shape is unique).  Integer
work: no tolerance anywhere."""
import os

import numpy as np
import pytest

import build_shapes as B
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALIGN = 360360


def _dense(n, m, d, seed):
    rng = np.random.default_rng(seed)
    if d <= 0:
        return np.zeros((n, m), dtype=bool)
    if d >= 1:
        return np.ones((n, m), dtype=bool)
    return rng.random((n, m)) < d


def _csr(dense, order="mixed", seed=0, key=None):
    """The rows of `dense` as a CSR; per row the columns 'ascending',
    'reversed', 'shuffled', 'mixed' (even rows reversed, odd rows shuffled) or
    by `key` (column -> rank: the tree's pre-order)."""
    rng = np.random.default_rng(seed)
    n = dense.shape[0]
    off = np.zeros(n + 1, dtype=np.uint64)
    parts = []
    for r in range(n):
        c = np.flatnonzero(dense[r]).astype(np.uint32)
        how = order if order != "mixed" else ("reversed" if r % 2 == 0 else "shuffled")
        if key is not None:
            c = c[np.argsort(key[c], kind="stable")]
        elif how == "reversed":
            c = c[::-1]
        elif how == "shuffled":
            c = rng.permutation(c)
        parts.append(c)
        off[r + 1] = off[r] + len(c)
    cols = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
    return off, cols.astype(np.uint32)


def _shape(tree):
    return {k: tree[k] for k in ("num_children", "first_child", "leaf_column")}


def _preorder_rank(shape):
    """column -> its index in the tree's pre-order of leaves."""
    nc, fc, lc = (np.asarray(shape[k]) for k in ("num_children", "first_child", "leaf_column"))
    order, st = [], [0]
    while st:
        u = st.pop()
        if nc[u] == 0:
            order.append(int(lc[u]))
        else:
            st.extend(range(int(fc[u]) + int(nc[u]) - 1, int(fc[u]) - 1, -1))
    rank = np.zeros(len(order), dtype=np.int64)
    rank[np.array(order)] = np.arange(len(order))
    return rank


def _count_labels(ctx, rows, m):
    import torch
    rows_t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.uint64).view(np.int64)).cuda()
    counts_t = torch.zeros(m, dtype=torch.int64, device="cuda")
    ctx.count_labels_device(rows_t, counts_t)
    torch.cuda.synchronize()
    return counts_t.cpu().numpy()


def _check(ctx, t, dense, rows=None, export=None, cells=20000, columns=6):
    """ctx answers as the oracle tree t of `dense`, and exports t."""
    n, m = dense.shape
    assert ctx.layout() == "rows"
    assert ctx.num_rows() == n and ctx.num_columns() == m
    assert ctx.num_relations() == int(dense.sum()) == t.num_relations()
    assert ctx.num_nodes() == len(t.export()["num_children"] if export is None else export["num_children"])
    rows = np.arange(n, dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64)
    woff, wcols = t.get_rows(rows)
    off, cols = ctx.get_rows(rows)
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(cols, wcols)
    if n * m <= cells:
        rr, cc = np.divmod(np.arange(n * m, dtype=np.uint64), np.uint64(m))
        np.testing.assert_array_equal(ctx.get_batch(rr, cc), dense.reshape(-1))
    rng = np.random.default_rng(n * 131 + m)
    for c in sorted(set([0, m - 1] + rng.integers(0, m, columns).tolist())):
        np.testing.assert_array_equal(ctx.get_column(c), np.flatnonzero(dense[:, c]).astype(np.uint64))
    np.testing.assert_array_equal(_count_labels(ctx, rows, m), dense[rows.astype(np.int64)].sum(axis=0))
    B.same_tree(ctx.export(), t.export() if export is None else export)


# ---- parity grid -----------------------------------------------------------------

@pytest.mark.parametrize("density", [0, 0.05, 0.5, 1])
@pytest.mark.parametrize("arity", [2, 3, 8, 64])
def test_parity_grid(oracle_mod, arity, density):
    from genome_graph_annotation_amd import BRWTDevice
    for n in (1, 2, 63, 64, 65, 1000):
        for m in (2, 3, 8, 9, 17, 65, 300):
            dense = _dense(n, m, density, 7 * n + m)
            t = oracle_mod.OracleTree.from_dense(dense, "basic", arity)
            ex = t.export()
            off, cols = _csr(dense, "mixed", seed=n + m)
            # the library's basic shape; at one n also the oracle's shape given
            for shape in (None, _shape(ex)) if n == 65 else (None,):
                ctx = BRWTDevice.from_rows(off, cols, m, arity=arity, shape=shape)
                _check(ctx, t, dense, export=ex, cells=20000 if shape is None else 0, columns=3)
                ctx.close()


# ---- other shapes ------------------------------------------------------------------

@pytest.mark.parametrize("name,relax", [("greedy_relax_small.npz", 0), ("greedy_relax_small.npz", 10),
                                        ("basic_relax_unbounded.npz", 2**64 - 1)])
def test_greedy_and_relaxed_shapes(oracle_mod, name, relax):
    """label_perm is not the identity under the greedy partitioner: rows given
    ascending by column are not ascending in pre-order (the sort runs); rows
    given in pre-order are (it does not)."""
    from genome_graph_annotation_amd import BRWTDevice
    f = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    dense = np.unpackbits(f["dense"], axis=1)[:, : int(f["m"])].astype(bool)
    t = oracle_mod.OracleTree.from_dense(dense, str(f["partitioner"]), int(f["arity"]), relax)
    ex = t.export()
    rank = _preorder_rank(ex)
    for order, key in (("ascending", None), ("shuffled", None), ("ascending", rank)):
        off, cols = _csr(dense, order, seed=3, key=key)
        ctx = BRWTDevice.from_rows(off, cols, dense.shape[1], shape=_shape(ex))
        _check(ctx, t, dense, export=ex)
        ctx.close()


# ---- row contents ------------------------------------------------------------------

def test_empty_full_and_long_rows(oracle_mod):
    """m = 300: empty rows, a full row, rows of 254 / 255 / 256 labels (the
    count byte; the always-spill rule), records past 64 and 128 bytes."""
    from genome_graph_annotation_amd import BRWTDevice
    m = 300
    rng = np.random.default_rng(5)
    counts = [0, 0, m, 254, 255, 256, 0, 1, 2, 60, 100, 150, 299, 0]
    dense = np.zeros((len(counts), m), dtype=bool)
    for r, k in enumerate(counts):
        dense[r, rng.choice(m, k, replace=False)] = True
    for arity in (2, 8):
        t = oracle_mod.OracleTree.from_dense(dense, "basic", arity)
        off, cols = _csr(dense, "mixed", seed=1)
        ctx = BRWTDevice.from_rows(off, cols, m, arity=arity)
        _check(ctx, t, dense)
        ref = BRWTDevice.from_tree(t.export(), layout="rows")
        assert ctx.rows_stats() == ref.rows_stats()
        ctx.close()
        ref.close()


def test_row_of_32767_labels_and_one_more(oracle_mod):
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError
    from genome_graph_annotation_amd import _lib as L
    n, m = 100, 40000
    rng = np.random.default_rng(11)
    dense = rng.random((n, m)) < 0.0005
    dense[37] = False
    picked = rng.choice(m, 32768, replace=False)
    dense[37, picked[:32767]] = True
    off, cols = _csr(dense, "shuffled", seed=2)
    ctx = BRWTDevice.from_rows(off, cols, m, arity=8)
    t = oracle_mod.OracleTree.from_dense(dense, "basic", 8)
    _check(ctx, t, dense, cells=0, columns=2)
    ctx.close()
    dense[37, picked[32767]] = True
    off, cols = _csr(dense, "ascending")
    with pytest.raises(MBRWTError) as e:
        BRWTDevice.from_rows(off, cols, m, arity=8)
    assert e.value.status == L.MBRWT_ERR_UNSUPPORTED


# ---- record forms --------------------------------------------------------------------

def _same_records_as_tree(oracle_mod, dense, arity, option, value, expect=None):
    """Under a build option: from_rows is checked as above, and its rows_stats()
    / rows_classes() equal those of from_tree(oracle tree, layout='rows')."""
    from genome_graph_annotation_amd import BRWTDevice
    from genome_graph_annotation_amd.brwt import build_option
    t = oracle_mod.OracleTree.from_dense(dense, "basic", arity)
    ex = t.export()
    off, cols = _csr(dense, "mixed", seed=9)
    with build_option(option, value):
        ctx = BRWTDevice.from_rows(off, cols, dense.shape[1], arity=arity)
        ref = BRWTDevice.from_tree(ex, layout="rows")
    _check(ctx, t, dense, export=ex)
    st, want = ctx.rows_stats(), ref.rows_stats()
    assert st == want
    if expect:
        for k, v in expect.items():
            assert st[k] == v, (k, st)
    ctx.close()
    ref.close()
    return st


@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_record_codes(oracle_mod, code):
    from genome_graph_annotation_amd import _lib as L
    for m, arity, d in ((64, 8, 0.1), (300, 4, 0.03), (17, 3, 0.5)):
        _same_records_as_tree(oracle_mod, _dense(500, m, d, m + code), arity, L.MBRWT_BUILD_ROWS_CODE, code)


def test_forced_variable_length_records(oracle_mod):
    from genome_graph_annotation_amd import _lib as L
    _same_records_as_tree(oracle_mod, _dense(1000, 64, 0.5, 21), 8, L.MBRWT_BUILD_ROWS_VAR, 1,
                          expect={"variable": True})


def test_forced_classes_on_repeated_rows(oracle_mod):
    from genome_graph_annotation_amd import _lib as L
    kinds = _dense(7, 40, 0.2, 33)
    dense = kinds[np.random.default_rng(4).integers(0, 7, 1000)]
    st = _same_records_as_tree(oracle_mod, dense, 8, L.MBRWT_BUILD_ROWS_CLASSES, 1)
    assert 0 < st["classes"] <= 7


@pytest.mark.parametrize("block", [64 << 8 | 1, 64 << 8 | 7, 128 << 8 | 15])
def test_block_overrides(oracle_mod, block):
    from genome_graph_annotation_amd import _lib as L
    _same_records_as_tree(oracle_mod, _dense(1000, 65, 0.1, block), 8, L.MBRWT_BUILD_ROWS_BLOCK, block,
                          expect={"block_bytes": block >> 8, "rows_per_block": block & 0xFF})


# ---- ranged build -----------------------------------------------------------------------

def test_ranged_build_three_ranges(oracle_mod):
    """MBRWT_BUILD_ROWS_RANGE = 360,360 over 2 x 360,360 + 17 rows: three
    ranges, the last partial."""
    from genome_graph_annotation_amd import BRWTDevice, _lib as L
    from genome_graph_annotation_amd.brwt import build_option
    n, m, arity = 2 * ALIGN + 17, 16, 4
    dense = np.random.default_rng(77).random((n, m)) < 0.15
    dense[ALIGN - 1] = True   # the rows either side of the first boundary differ
    dense[ALIGN] = False
    t = oracle_mod.OracleTree.from_dense(dense, "basic", arity)
    rr, cc = np.nonzero(dense)  # row-major: ascending columns per row
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(dense.sum(axis=1))
    with build_option(L.MBRWT_BUILD_ROWS_RANGE, ALIGN):
        ctx = BRWTDevice.from_rows(off, cc.astype(np.uint32), m, arity=arity)
    edges = np.concatenate([np.arange(k * ALIGN - 3, k * ALIGN + 3) for k in (1, 2)] + [np.arange(3), np.arange(n - 3, n)])
    rows = np.concatenate([edges, np.random.default_rng(1).integers(0, n, 100000)]).astype(np.uint64)
    assert ctx.layout() == "rows" and ctx.num_relations() == int(dense.sum())
    woff, wcols = t.get_rows(rows)
    off2, cols2 = ctx.get_rows(rows)
    np.testing.assert_array_equal(off2, woff)
    np.testing.assert_array_equal(cols2, wcols)
    B.same_tree(ctx.export(), t.export())
    ctx.close()


def test_ranged_build_with_unordered_rows(oracle_mod):
    """Two ranges whose rows need the sort, the second a few rows."""
    from genome_graph_annotation_amd import BRWTDevice, _lib as L
    from genome_graph_annotation_amd.brwt import build_option
    n, m = ALIGN + 5, 5
    dense = np.random.default_rng(78).random((n, m)) < 0.3
    t = oracle_mod.OracleTree.from_dense(dense, "basic", 2)
    rr, cc = np.nonzero(dense[:, ::-1])  # per row: descending columns
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(dense.sum(axis=1))
    with build_option(L.MBRWT_BUILD_ROWS_RANGE, ALIGN):
        ctx = BRWTDevice.from_rows(off, (m - 1 - cc).astype(np.uint32), m, arity=2)
    rows = np.concatenate([np.arange(ALIGN - 50, n), np.arange(2000)]).astype(np.uint64)
    woff, wcols = t.get_rows(rows)
    off2, cols2 = ctx.get_rows(rows)
    np.testing.assert_array_equal(off2, woff)
    np.testing.assert_array_equal(cols2, wcols)
    B.same_tree(ctx.export(), t.export())
    ctx.close()


# ---- consumers -----------------------------------------------------------------------------

def test_consumers_match_the_rows_context_of_the_tree(oracle_mod):
    from genome_graph_annotation_amd import BRWTDevice
    n, m = 3000, 40
    dense = _dense(n, m, 0.12, 50)
    t = oracle_mod.OracleTree.from_dense(dense, "basic", 4)
    off, cols = _csr(dense, "mixed", seed=6)
    ctx = BRWTDevice.from_rows(off, cols, m, arity=4)
    ref = BRWTDevice.from_tree(t.export(), layout="rows")
    rows = np.random.default_rng(8).integers(0, n, 5000).astype(np.uint64)
    for a, b in zip(ctx.get_rows16(rows), ref.get_rows16(rows)):
        np.testing.assert_array_equal(a, b)
    woff, wcols = t.get_rows(rows)
    o16, c16 = ctx.get_rows16(rows)
    np.testing.assert_array_equal(o16, woff)
    np.testing.assert_array_equal(c16.astype(np.uint32), wcols)
    cl = ctx.clone()
    for a, b in zip(cl.get_rows(rows), (woff, wcols)):
        np.testing.assert_array_equal(a, b)
    cl.close()
    reads = np.arange(0, len(rows) + 1, 50, dtype=np.uint64)
    for ratio in (0.0, 0.3, 1.0):
        for a, b in zip(ctx.get_labels_batch(rows, reads, ratio), ref.get_labels_batch(rows, reads, ratio)):
            np.testing.assert_array_equal(a, b)
    for a, b in zip(ctx.get_top_labels_batch(rows, reads, 5), ref.get_top_labels_batch(rows, reads, 5)):
        np.testing.assert_array_equal(a, b)
    ctx.close()
    ref.close()


# ---- errors ------------------------------------------------------------------------------------

def test_errors_and_a_valid_build_after_each(oracle_mod):
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    from genome_graph_annotation_amd.brwt import basic_shape, build_layout
    n, m = 200, 12
    dense = _dense(n, m, 0.3, 90)
    dense[5, :3] = True
    t = oracle_mod.OracleTree.from_dense(dense, "basic", 3)
    off, cols = _csr(dense, "ascending")

    def valid():
        ctx = BRWTDevice.from_rows(off, cols, m, arity=3)
        _check(ctx, t, dense, cells=0, columns=1)
        ctx.close()

    def fails(status, *args, **kw):
        with pytest.raises(MBRWTError) as e:
            BRWTDevice.from_rows(*args, **kw)
        assert e.value.status == status, e.value
        valid()

    valid()
    a = int(off[5])
    dup = cols.copy()
    dup[a + 2] = dup[a]  # row 5: a column twice (not adjacent)
    fails(L.MBRWT_ERR_INVALID, off, dup, m, arity=3)
    big = cols.copy()
    big[len(big) // 2] = m
    fails(L.MBRWT_ERR_INVALID, off, big, m, arity=3)
    o1 = off.copy()
    o1[0] = 1
    fails(L.MBRWT_ERR_INVALID, o1, cols, m, arity=3)
    desc = off.copy()
    desc[7] = desc[8] + 1  # offsets[7] > offsets[8]
    fails(L.MBRWT_ERR_INVALID, desc, cols, m, arity=3)
    sh = basic_shape(m, 3)
    bad = {k: np.array(v, copy=True) for k, v in sh.items()}
    leaves = np.flatnonzero(bad["num_children"] == 0)
    bad["leaf_column"][leaves[1]] = bad["leaf_column"][leaves[0]]  # not a permutation
    fails(L.MBRWT_ERR_INVALID, off, cols, m, shape=bad)
    fails(L.MBRWT_ERR_INVALID, off, cols, m, shape=basic_shape(m + 1, 3))  # leaf count != num_columns
    for layout in ("nodes", "both"):
        with build_layout(layout):
            with pytest.raises(MBRWTError) as e:
                BRWTDevice.from_rows(off, cols, m, arity=3)
        assert e.value.status == L.MBRWT_ERR_UNSUPPORTED
        valid()
    one = np.arange(n + 1, dtype=np.uint64)
    fails(L.MBRWT_ERR_UNSUPPORTED, one, np.zeros(n, dtype=np.uint32), 1, arity=3)  # a one-column tree


def test_empty_matrices_as_from_columns():
    from genome_graph_annotation_amd import BRWTDevice
    got = BRWTDevice.from_rows(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), 5, arity=2)
    want = BRWTDevice.from_columns([np.zeros(0, dtype=np.uint64)] * 5, 0, arity=2)
    assert (got.num_rows(), got.num_columns(), got.num_nodes(), got.layout()) == \
        (want.num_rows(), want.num_columns(), want.num_nodes(), want.layout())
    B.same_tree(got.export(), want.export())
    got.close()
    want.close()
