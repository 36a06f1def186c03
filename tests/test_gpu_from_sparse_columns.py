"""GPU parity of the build from sparse columns (csrc/rows_from_cols.hip,
DESIGN.md §11d): mbrwt_create_from_sparse_columns, mbrwt_sparse_columns_node_counts
and mbrwt_tree_shape_from_sparse_columns.  Every context is checked against
the oracle tree of the same dense matrix (ordered get_rows, get_batch,
get_column, count_labels, num_relations, export() word for word) and against
BRWTDevice.from_rows of the same matrix (rows_stats(), device_bytes(),
export()).  Integer work: no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import build_shapes as B
from conftest import gpu_available
from test_build_shapes import PLANTED, PLANTED_1M, SKIP3
from test_gpu_from_rows import _check, _dense, _shape
from test_relax_shape import KEYS, UNBOUNDED, _golden, numpy_counts

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

ALIGN = 360360


def _sparse(dense, dtype=np.uint64):
    """The columns of `dense`: (offsets [m + 1], ascending row ids per column)."""
    dense = np.asarray(dense, dtype=bool)
    off = np.zeros(dense.shape[1] + 1, dtype=np.uint64)
    off[1:] = np.cumsum(dense.sum(axis=0))
    return off, np.nonzero(dense.T)[1].astype(dtype)


def _csr(dense):
    dense = np.asarray(dense, dtype=bool)
    off = np.zeros(dense.shape[0] + 1, dtype=np.uint64)
    off[1:] = np.cumsum(dense.sum(axis=1))
    return off, np.nonzero(dense)[1].astype(np.uint32)


def _same_context(ctx, ref):
    """Indistinguishable from the from_rows context: the image and its tree."""
    assert ctx.rows_stats() == ref.rows_stats()
    assert ctx.device_bytes() == ref.device_bytes()
    assert ctx.num_relations() == ref.num_relations() and ctx.num_nodes() == ref.num_nodes()
    B.same_tree(ctx.export(), ref.export())


def _build_both(dense, dtype=np.uint64, **kw):
    """(from_sparse_columns, from_rows) of the same matrix and arguments."""
    from genome_graph_annotation_amd import BRWTDevice
    n, m = dense.shape
    ctx = BRWTDevice.from_sparse_columns(*_sparse(dense, dtype), n, m, **kw)
    ref = BRWTDevice.from_rows(*_csr(dense), m, **kw)
    return ctx, ref


def _same_shape(a, b, msg=""):
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=f"{msg} {k}")


# ---- parity grid -----------------------------------------------------------------

@pytest.mark.parametrize("density", [0, 0.05, 0.5, 1])
@pytest.mark.parametrize("arity", [2, 3, 8, 64])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_parity_grid(oracle_mod, n, arity, density):
    """n = 1: the sort of zero bits is skipped; density 0 and 1: empty slices,
    and slices of every row in every column; u64 ids and u32 ids."""
    from genome_graph_annotation_amd import BRWTDevice
    for m in (2, 3, 8, 9, 17, 65, 300):
        dense = _dense(n, m, density, 7 * n + m)
        t = oracle_mod.OracleTree.from_dense(dense, "basic", arity)
        ex = t.export()
        ctx, ref = _build_both(dense, arity=arity)
        _check(ctx, t, dense, export=ex, columns=3)
        _same_context(ctx, ref)
        narrow = BRWTDevice.from_sparse_columns(*_sparse(dense, np.uint32), n, m, arity=arity)
        _same_context(narrow, ref)
        rows = np.arange(n, dtype=np.uint64)
        for a, b in zip(narrow.get_rows(rows), ctx.get_rows(rows)):
            np.testing.assert_array_equal(a, b)
        for c in (ctx, ref, narrow):
            c.close()


def test_wide_keys(oracle_mod):
    """m = 65,536 at arity 64: key 0xFFFF sits beside the row bits of the pairs."""
    n, m = 65, 65536
    rng = np.random.default_rng(3)
    dense = np.zeros((n, m), dtype=bool)
    for r in range(n):
        dense[r, rng.integers(0, m, 5)] = True
    dense[::2, 0] = True
    dense[1::2, m - 1] = True
    dense[7, [0, 1, m - 2, m - 1]] = True
    t = oracle_mod.OracleTree.from_dense(dense, "basic", 64)
    for dtype in (np.uint64, np.uint32):
        ctx, ref = _build_both(dense, dtype, arity=64)
        _check(ctx, t, dense, cells=0, columns=2)
        _same_context(ctx, ref)
        ctx.close()
        ref.close()


@pytest.mark.parametrize("name,relax", [("greedy_relax_small.npz", 0), ("greedy_relax_small.npz", 10),
                                        ("basic_relax_unbounded.npz", UNBOUNDED)])
def test_shapes_whose_pre_order_is_not_column_order(oracle_mod, name, relax):
    """The slices are staged by pre-order leaf index, not by column id: under a
    greedy shape the two differ, and only the first leaves every row's keys
    ascending after the stable sort by row."""
    dense, part, arity = _golden(name)
    t = oracle_mod.OracleTree.from_dense(dense, part, arity, relax)
    ex = t.export()
    if part == "greedy":
        leaves = np.asarray(ex["leaf_column"])[np.asarray(ex["num_children"]) == 0]
        assert not np.array_equal(np.sort(leaves), leaves)  # (BFS leaf order here; pre-order differs too)
    ctx, ref = _build_both(dense, shape=_shape(ex))
    _check(ctx, t, dense, export=ex)
    _same_context(ctx, ref)
    ctx.close()
    ref.close()


# ---- ranges ----------------------------------------------------------------------------

@pytest.mark.parametrize("empty_middle", [False, True])
def test_three_ranges(oracle_mod, empty_middle):
    """MBRWT_BUILD_ROWS_RANGE = 360,360 over 2 x 360,360 + 17 rows: a column
    inside the middle range, an empty one, one with ids either side of both
    boundaries, one in the first range only, one set in every row; then the
    middle range without any label (L == 0 between two ranges with labels)."""
    from genome_graph_annotation_amd import _lib as L
    from genome_graph_annotation_amd.brwt import build_option, node_counts_from_rows, node_counts_from_sparse_columns
    n, m, arity = 2 * ALIGN + 17, 16, 4
    dense = np.random.default_rng(77).random((n, m)) < 0.1
    dense[:, 0] = False
    dense[ALIGN + 100:2 * ALIGN - 100:7, 0] = True      # entirely inside the middle range
    dense[:, 1] = False                                  # empty
    dense[:, 2] = False
    dense[[ALIGN - 1, ALIGN, 2 * ALIGN - 1, 2 * ALIGN], 2] = True
    dense[ALIGN:, 3] = False                             # the first range only
    dense[:, 4] = True                                   # every row
    if empty_middle:
        dense[ALIGN:2 * ALIGN] = False
    t = oracle_mod.OracleTree.from_dense(dense, "basic", arity)
    with build_option(L.MBRWT_BUILD_ROWS_RANGE, ALIGN):
        ctx, ref = _build_both(dense, arity=arity)
        counts = node_counts_from_sparse_columns(*_sparse(dense, np.uint32), n, m, arity=arity)
        want = node_counts_from_rows(*_csr(dense), m, arity=arity)
    np.testing.assert_array_equal(counts, want)
    from genome_graph_annotation_amd.brwt import basic_shape
    np.testing.assert_array_equal(counts, numpy_counts(dense, basic_shape(m, arity)))
    _same_context(ctx, ref)
    edges = np.concatenate([np.arange(k * ALIGN - 3, k * ALIGN + 3) for k in (1, 2)] + [np.arange(3), np.arange(n - 3, n)])
    rows = np.concatenate([edges, np.random.default_rng(1).integers(0, n, 50000)]).astype(np.uint64)
    assert ctx.layout() == "rows" and ctx.num_relations() == int(dense.sum())
    woff, wcols = t.get_rows(rows)
    off2, cols2 = ctx.get_rows(rows)
    np.testing.assert_array_equal(off2, woff)
    np.testing.assert_array_equal(cols2, wcols)
    for c in (0, 1, 2, 3, 4, m - 1):
        np.testing.assert_array_equal(ctx.get_column(c), np.flatnonzero(dense[:, c]).astype(np.uint64))
    B.same_tree(ctx.export(), t.export())
    ctx.close()
    ref.close()


# ---- row contents ---------------------------------------------------------------------

def test_row_of_32767_labels_and_one_more(oracle_mod):
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    from genome_graph_annotation_amd.brwt import node_counts_from_sparse_columns
    n, m = 100, 40000
    rng = np.random.default_rng(11)
    dense = rng.random((n, m)) < 0.0005
    dense[37] = False
    picked = rng.choice(m, 32768, replace=False)
    dense[37, picked[:32767]] = True
    ctx, ref = _build_both(dense, arity=8)
    t = oracle_mod.OracleTree.from_dense(dense, "basic", 8)
    _check(ctx, t, dense, cells=0, columns=2)
    _same_context(ctx, ref)
    ctx.close()
    ref.close()
    dense[37, picked[32767]] = True
    for fn in (BRWTDevice.from_sparse_columns, node_counts_from_sparse_columns):
        with pytest.raises(MBRWTError) as e:
            fn(*_sparse(dense), n, m, arity=8)
        assert e.value.status == L.MBRWT_ERR_UNSUPPORTED


# ---- record forms -------------------------------------------------------------------------

def _same_records(oracle_mod, dense, arity, option, value, expect=None):
    from genome_graph_annotation_amd.brwt import build_option
    t = oracle_mod.OracleTree.from_dense(dense, "basic", arity)
    with build_option(option, value):
        ctx, ref = _build_both(dense, arity=arity)
    _check(ctx, t, dense)
    _same_context(ctx, ref)
    st = ctx.rows_stats()
    for k, v in (expect or {}).items():
        assert st[k] == v, (k, st)
    ctx.close()
    ref.close()
    return st


@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_record_codes(oracle_mod, code):
    from genome_graph_annotation_amd import _lib as L
    for m, arity, d in ((64, 8, 0.1), (300, 4, 0.03), (17, 3, 0.5)):
        _same_records(oracle_mod, _dense(500, m, d, m + code), arity, L.MBRWT_BUILD_ROWS_CODE, code)


def test_forced_variable_length_records(oracle_mod):
    from genome_graph_annotation_amd import _lib as L
    _same_records(oracle_mod, _dense(1000, 64, 0.5, 21), 8, L.MBRWT_BUILD_ROWS_VAR, 1, expect={"variable": True})


def test_forced_classes_on_repeated_rows(oracle_mod):
    from genome_graph_annotation_amd import _lib as L
    kinds = _dense(7, 40, 0.2, 33)
    dense = kinds[np.random.default_rng(4).integers(0, 7, 1000)]
    st = _same_records(oracle_mod, dense, 8, L.MBRWT_BUILD_ROWS_CLASSES, 1)
    assert 0 < st["classes"] <= 7


def test_block_override(oracle_mod):
    from genome_graph_annotation_amd import _lib as L
    block = 64 << 8 | 7
    _same_records(oracle_mod, _dense(1000, 65, 0.1, block), 8, L.MBRWT_BUILD_ROWS_BLOCK, block,
                  expect={"block_bytes": 64, "rows_per_block": 7})


# ---- node counts ---------------------------------------------------------------------------

@pytest.mark.parametrize("density", [0, 0.05, 0.5, 1])
@pytest.mark.parametrize("arity", [2, 3, 8, 64])
def test_counts_grid(arity, density):
    from genome_graph_annotation_amd.brwt import basic_shape, node_counts_from_rows, node_counts_from_sparse_columns
    for n in (1, 2, 63, 64, 65, 1000):
        for m in (1, 2, 17, 300):
            dense = _dense(n, m, density, 7 * n + m)
            got = node_counts_from_sparse_columns(*_sparse(dense, np.uint32 if n % 2 else np.uint64), n, m,
                                                  arity=arity)
            np.testing.assert_array_equal(got, node_counts_from_rows(*_csr(dense), m, arity=arity))
            np.testing.assert_array_equal(got, numpy_counts(dense, basic_shape(m, arity)))


# ---- shapes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("part,arity,relax", [("basic", 5, 0), ("basic", 2, 10), ("greedy", 2, 0), ("greedy", 2, 10),
                                              ("greedy", 2, UNBOUNDED)])
def test_shapes_of_random_matrices(oracle_mod, part, arity, relax):
    from genome_graph_annotation_amd import BRWTDevice
    from genome_graph_annotation_amd.brwt import shape_from_rows, shape_from_sparse_columns
    for n, m, d, seed in ((300, 23, 0.1, 1), (1000, 70, 0.03, 2), (129, 40, 0.5, 3), (200, 16, 0.0, 4)):
        dense = _dense(n, m, d, seed)
        dense[:, [0, m // 2, m - 1]] = False
        got = shape_from_sparse_columns(*_sparse(dense), n, m, part, arity, relax)
        _same_shape(got, shape_from_rows(*_csr(dense), m, part, arity, relax), f"{n}x{m}")
        _same_shape(got, oracle_mod.OracleTree.from_dense(dense, part, arity, relax).export(), f"{n}x{m} oracle")
        ctx = BRWTDevice.from_sparse_columns(*_sparse(dense, np.uint32), n, m, arity=arity, partitioner=part,
                                             relax_max_arity=relax)
        ref = BRWTDevice.from_rows(*_csr(dense), m, arity=arity, partitioner=part, relax_max_arity=relax)
        _same_context(ctx, ref)
        ctx.close()
        ref.close()


@pytest.mark.parametrize("n,m,law", [(n, m, "mirror") for n, m in PLANTED] + [(n, m, "skip3") for n, m in SKIP3])
def test_greedy_planted_pairs(n, m, law):
    from genome_graph_annotation_amd.brwt import shape_from_rows, shape_from_sparse_columns
    dense, pairs = B.planted_pairs(n, m, law, 16)
    for relax in (0, 10):
        got = shape_from_sparse_columns(*_sparse(dense), n, m, "greedy", relax_max_arity=relax)
        _same_shape(got, shape_from_rows(*_csr(dense), m, "greedy", relax_max_arity=relax))
        if not relax:
            assert not set(pairs) - B.leaf_pairs(got)


@pytest.mark.parametrize("n,m", PLANTED_1M)
def test_greedy_at_the_sample_switch(n, m):
    """n = 1,000,000: every row is its own slot; n = 1,000,001: the reference's
    mt19937 sample intersected with every column.  The planted columns are
    short (each id looked up in the sample); the added dense ones are merged
    with it."""
    from genome_graph_annotation_amd.brwt import shape_from_rows, shape_from_sparse_columns
    dense, pairs = B.planted_pairs(n, m, "mirror", 5000)
    rng = np.random.default_rng(n)
    dense = np.concatenate([dense, rng.random((n, 3)) < 0.5, np.ones((n, 1), dtype=bool)], axis=1)
    dense[:, m + 1] = dense[:, m]  # two equal dense columns: a pair
    m += 4
    for relax in (0, 10):
        got = shape_from_sparse_columns(*_sparse(dense, np.uint32), n, m, "greedy", relax_max_arity=relax)
        _same_shape(got, shape_from_rows(*_csr(dense), m, "greedy", relax_max_arity=relax))
        if not relax:
            assert not set(pairs) - B.leaf_pairs(got)


# ---- errors --------------------------------------------------------------------------------------

def test_errors_and_a_valid_build_after_each(oracle_mod):
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    from genome_graph_annotation_amd.brwt import (build_layout, build_option, node_counts_from_sparse_columns,
                                                  shape_from_sparse_columns)
    n, m = 200, 12
    dense = _dense(n, m, 0.3, 90)
    dense[:6, 5] = True
    t = oracle_mod.OracleTree.from_dense(dense, "basic", 3)
    off, ids = _sparse(dense)
    lib = L.lib()

    def valid():
        ctx = BRWTDevice.from_sparse_columns(off, ids, n, m, arity=3)
        _check(ctx, t, dense, cells=0, columns=1)
        ctx.close()

    def fails(status, *args, **kw):
        for fn in (BRWTDevice.from_sparse_columns, node_counts_from_sparse_columns):
            with pytest.raises(MBRWTError) as e:
                fn(*args, **kw)
            assert e.value.status == status, (fn, e.value)
        with pytest.raises(MBRWTError) as e:  # every row is sampled: the greedy partitioner checks the ids too
            shape_from_sparse_columns(*args, partitioner="greedy")
        assert e.value.status == status, e.value
        with pytest.raises(MBRWTError) as e:  # the counts pass of the relax
            shape_from_sparse_columns(*args, partitioner="basic", arity=3, relax_max_arity=10)
        assert e.value.status == status, e.value
        valid()

    valid()
    a = int(off[5])
    big = ids.copy()
    big[int(off[6]) - 1] = n              # the last id of column 5 == num_rows
    fails(L.MBRWT_ERR_INVALID, off, big, n, m, arity=3)
    dup = ids.copy()
    dup[a + 2] = dup[a + 1]               # column 5: a row twice
    fails(L.MBRWT_ERR_INVALID, off, dup, n, m, arity=3)
    desc = ids.copy()
    desc[a + 2], desc[a + 3] = desc[a + 3], desc[a + 2]   # column 5: a descending pair
    fails(L.MBRWT_ERR_INVALID, off, desc, n, m, arity=3)
    o1 = off.copy()
    o1[0] = 1
    fails(L.MBRWT_ERR_INVALID, o1, ids, n, m, arity=3)
    od = off.copy()
    od[7] = od[8] + 1                     # offsets[7] > offsets[8]
    fails(L.MBRWT_ERR_INVALID, od, ids, n, m, arity=3)

    # both pointers, neither pointer, rows32 over more than 2^32 rows: straight at the C ABI
    ids32 = ids.astype(np.uint32)
    p64, p32, po = ids.ctypes.data_as(L.u64p), ids32.ctypes.data_as(L.u32p), off.ctypes.data_as(L.u64p)
    counts = np.zeros(64, dtype=np.uint64)
    for d in (L.SparseColumnsDesc(n, m, po, p64, p32), L.SparseColumnsDesc(n, m, po, None, None),
              L.SparseColumnsDesc(2**32 + 1, m, po, None, p32)):
        h = C.c_void_p()
        assert lib.mbrwt_create_from_sparse_columns(C.byref(d), None, 3, 0, C.byref(h)) == L.MBRWT_ERR_INVALID
        assert not h.value
        assert lib.mbrwt_sparse_columns_node_counts(C.byref(d), None, 3, 0, counts.ctypes.data_as(L.u64p)) == \
            L.MBRWT_ERR_INVALID
        assert lib.mbrwt_tree_shape_from_sparse_columns(C.byref(d), 1, 2, 0, 0, C.byref(h)) == L.MBRWT_ERR_INVALID
        valid()
    h = C.c_void_p()
    ok32 = L.SparseColumnsDesc(2**32, m, po, None, p32)   # num_rows == 2^32 is allowed with rows32
    assert lib.mbrwt_tree_shape_from_sparse_columns(C.byref(ok32), 0, 3, 0, 0, C.byref(h)) == L.MBRWT_OK
    lib.mbrwt_tree_free(h)

    for layout in ("nodes", "both"):
        with build_layout(layout):
            with pytest.raises(MBRWTError) as e:
                BRWTDevice.from_sparse_columns(off, ids, n, m, arity=3)
        assert e.value.status == L.MBRWT_ERR_UNSUPPORTED
        valid()
    with pytest.raises(MBRWTError) as e:  # a one-column tree
        BRWTDevice.from_sparse_columns(np.array([0, n], dtype=np.uint64), np.arange(n, dtype=np.uint64), n, 1)
    assert e.value.status == L.MBRWT_ERR_UNSUPPORTED
    valid()
    with pytest.raises(ValueError):
        BRWTDevice.from_sparse_columns(off, ids, n, m, shape={}, partitioner="greedy")


def test_descending_pair_in_a_later_range():
    """The ids of a range are checked when that range is staged: a pair out of
    order beyond the first 360,360 rows fails the build in its second range."""
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    from genome_graph_annotation_amd.brwt import build_option, node_counts_from_sparse_columns
    n, m = ALIGN + 100, 4
    dense = np.zeros((n, m), dtype=bool)
    dense[::1000, 0] = True
    dense[[5, ALIGN - 1, ALIGN, ALIGN + 20, ALIGN + 50], 2] = True
    dense[ALIGN + 7:, 3] = True
    off, ids = _sparse(dense)
    bad = ids.copy()
    a = int(off[3])
    assert bad[a - 2] == ALIGN + 20 and bad[a - 1] == ALIGN + 50
    bad[a - 2], bad[a - 1] = bad[a - 1], bad[a - 2]
    with build_option(L.MBRWT_BUILD_ROWS_RANGE, ALIGN):
        for fn in (BRWTDevice.from_sparse_columns, node_counts_from_sparse_columns):
            with pytest.raises(MBRWTError) as e:
                fn(off, bad, n, m, arity=2)
            assert e.value.status == L.MBRWT_ERR_INVALID
        ctx = BRWTDevice.from_sparse_columns(off, ids, n, m, arity=2)
    rows = np.arange(ALIGN - 5, n, dtype=np.uint64)
    got_off, got_cols = ctx.get_rows(rows)
    want_off, want_cols = _csr(dense[ALIGN - 5:])
    np.testing.assert_array_equal(got_off, want_off)
    np.testing.assert_array_equal(got_cols, want_cols)
    ctx.close()


def test_empty_matrices_as_from_columns():
    from genome_graph_annotation_amd import BRWTDevice
    from genome_graph_annotation_amd.brwt import node_counts_from_sparse_columns, shape_from_sparse_columns
    none = np.zeros(0, dtype=np.uint64)
    for n, m in ((0, 5), (7, 0), (0, 0)):
        off = np.zeros(m + 1, dtype=np.uint64)
        want = BRWTDevice.from_columns([np.zeros((n + 63) // 64, dtype=np.uint64)] * m, n, arity=2)
        got = BRWTDevice.from_sparse_columns(off, none, n, m, arity=2)
        assert (got.num_rows(), got.num_columns(), got.num_nodes(), got.layout()) == \
            (want.num_rows(), want.num_columns(), want.num_nodes(), want.layout())
        B.same_tree(got.export(), want.export())
        got.close()
        want.close()
    off5 = np.zeros(6, dtype=np.uint64)
    assert node_counts_from_sparse_columns(off5, none, 0, 5, arity=2).tolist() == [0] * 9
    assert len(node_counts_from_sparse_columns(np.zeros(1, dtype=np.uint64), none, 0, 0, arity=2)) == 0
    assert len(shape_from_sparse_columns(np.zeros(1, dtype=np.uint64), none, 0, 0, "greedy")["num_children"]) == 0
    assert len(shape_from_sparse_columns(off5, none, 0, 5, "greedy", relax_max_arity=10)["num_children"]) >= 6
