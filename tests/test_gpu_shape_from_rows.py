"""GPU parity of the tree shape from row-major data:
mbrwt_rows_node_counts (csrc/rows_counts.hip) against numpy,
mbrwt_tree_shape_from_rows (greedy over the scattered row sample, relax over
the counts of all rows) against the oracle's builders on the dense matrix, and
BRWTDevice.from_rows(partitioner=..., relax_max_arity=...) against the
from-columns build of the same matrix.  Integer work: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import build_shapes as B
from conftest import gpu_available
from test_build_shapes import PLANTED, PLANTED_1M, SKIP3
from test_gpu_parity import _check_rows
from test_relax_shape import KEYS, UNBOUNDED, _golden, _random, _shape, numpy_counts

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

ALIGN = 360360


def _csr(dense, order="ascending", seed=0):
    """The rows of `dense` as a CSR, per row the columns 'ascending',
    'reversed' or 'shuffled'."""
    dense = np.asarray(dense, dtype=bool)
    n, m = dense.shape
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(dense.sum(axis=1))
    if order == "reversed":
        cols = (m - 1 - np.nonzero(dense[:, ::-1])[1]).astype(np.uint32)
    else:
        cols = np.nonzero(dense)[1].astype(np.uint32)
    if order == "shuffled":
        rng = np.random.default_rng(seed)
        for r in range(n):
            a, b = int(off[r]), int(off[r + 1])
            cols[a:b] = rng.permutation(cols[a:b])
    return off, cols


def _counts_are(dense, shape, got, off):
    nc = np.asarray(shape["num_children"])
    np.testing.assert_array_equal(got, numpy_counts(dense, shape))
    assert int(got[nc == 0].sum()) == int(off[-1])          # the leaves: every label once
    assert int(got[0]) == int(dense.any(axis=1).sum())      # the root: the non-empty rows


def _same_shape(a, b, msg=""):
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=f"{msg} {k}")


# ---- counts against numpy ------------------------------------------------------

@pytest.mark.parametrize("density", [0, 0.05, 0.5, 1])
@pytest.mark.parametrize("arity", [2, 3, 8, 64])
def test_counts_grid(arity, density):
    """Row counts 1..1000 (partial waves, more than one workgroup), one column
    (the root a leaf) to 300, every row order: descending and shuffled rows
    take the sort."""
    from genome_graph_annotation_amd.brwt import basic_shape, node_counts_from_rows
    for n in (1, 2, 63, 64, 65, 1000):
        for m in (1, 2, 17, 300):
            dense = _random(n, m, density, 7 * n + m)
            shape = basic_shape(m, arity)
            for order in ("ascending", "reversed", "shuffled"):
                off, cols = _csr(dense, order, seed=n + m)
                # the library's basic shape; at one n also the same shape given
                got = node_counts_from_rows(off, cols, m, arity=arity)
                _counts_are(dense, shape, got, off)
                if n == 65:
                    np.testing.assert_array_equal(node_counts_from_rows(off, cols, m, shape=shape), got)


@pytest.mark.parametrize("relax", [0, 10])
def test_counts_under_a_greedy_shape(oracle_mod, relax):
    """label_perm is not the identity: ascending columns are not ascending keys."""
    from genome_graph_annotation_amd.brwt import node_counts_from_rows
    dense, part, arity = _golden("greedy_relax_small.npz")
    shape = _shape(oracle_mod.OracleTree.from_dense(dense, part, arity, relax).export())
    rank = {int(c): i for i, c in enumerate(np.asarray(shape["leaf_column"])[np.asarray(shape["num_children"]) == 0])}
    assert any(rank[c] != c for c in rank)
    for order in ("ascending", "reversed", "shuffled"):
        off, cols = _csr(dense, order, seed=3)
        _counts_are(dense, shape, node_counts_from_rows(off, cols, dense.shape[1], shape=shape), off)


def test_counts_shape_too_large_for_the_lds_table():
    """7,000 columns at arity 2: 13,999 nodes, past the LDS counter table --
    the plain global atomics."""
    from genome_graph_annotation_amd.brwt import basic_shape, node_counts_from_rows
    n, m = 700, 7000
    dense = _random(n, m, 0.002, 12)
    dense[5] = False
    shape = basic_shape(m, 2)
    assert len(shape["num_children"]) == 2 * m - 1
    off, cols = _csr(dense, "reversed")
    _counts_are(dense, shape, node_counts_from_rows(off, cols, m, arity=2), off)


def test_counts_row_of_32767_labels_and_one_more():
    from genome_graph_annotation_amd import MBRWTError, _lib as L
    from genome_graph_annotation_amd.brwt import basic_shape, node_counts_from_rows
    n, m = 100, 40000
    rng = np.random.default_rng(11)
    dense = rng.random((n, m)) < 0.0005
    dense[37] = False
    picked = rng.choice(m, 32768, replace=False)
    dense[37, picked[:32767]] = True
    off, cols = _csr(dense, "reversed")
    _counts_are(dense, basic_shape(m, 8), node_counts_from_rows(off, cols, m, arity=8), off)
    dense[37, picked[32767]] = True
    off, cols = _csr(dense)
    with pytest.raises(MBRWTError) as e:
        node_counts_from_rows(off, cols, m, arity=8)
    assert e.value.status == L.MBRWT_ERR_UNSUPPORTED


def test_counts_three_ranges():
    """MBRWT_BUILD_ROWS_RANGE = 360,360 over 2 x 360,360 + 1,000 rows: three
    ranges, the last one's rows unordered; the counts add up across them."""
    from genome_graph_annotation_amd import _lib as L
    from genome_graph_annotation_amd.brwt import basic_shape, build_option, node_counts_from_rows
    n, m, arity = 2 * ALIGN + 1000, 20, 4
    dense = np.random.default_rng(77).random((n, m)) < 0.1
    dense[ALIGN - 1] = True   # the rows either side of the first boundary differ
    dense[ALIGN] = False
    off, cols = _csr(dense)
    a = int(off[2 * ALIGN])
    tail = _csr(dense[2 * ALIGN:], "reversed")[1]
    assert not np.array_equal(cols[a:], tail)
    cols[a:] = tail
    shape = basic_shape(m, arity)
    one = node_counts_from_rows(off, cols, m, arity=arity)
    with build_option(L.MBRWT_BUILD_ROWS_RANGE, ALIGN):
        three = node_counts_from_rows(off, cols, m, arity=arity)
    np.testing.assert_array_equal(three, one)
    _counts_are(dense, shape, three, off)


# ---- greedy at the similarity and scatter edges ---------------------------------------

def _all_rows(n, cap=16385, sample=4000):
    if n <= cap:
        return np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(n)
    return np.concatenate([np.arange(64), np.arange(n - 64, n), rng.integers(0, n, sample)]).astype(np.uint64)


def _planted(O, n, m, law, s=16):
    from genome_graph_annotation_amd import BRWTDevice
    from genome_graph_annotation_amd.brwt import shape_from_rows
    dense, pairs = B.planted_pairs(n, m, law, s)
    words = B.pack(dense)
    off, cols = _csr(dense)
    got = B.leaf_pairs(shape_from_rows(off, cols, m, "greedy"))
    missing = sorted(set(pairs) - got)
    assert not missing, f"planted pairs not matched: {missing}"
    for relax in (0, 10):
        t = O.OracleTree.from_words(words.reshape(-1), n, m, "greedy", 2, relax)
        built = BRWTDevice.from_rows(off, cols, m, partitioner="greedy", relax_max_arity=relax)
        B.same_tree(built.export(), t.export())
        assert built.num_relations() == 2 * s * len(pairs)
        _check_rows(t, built, _all_rows(n), variants=(0,))
        built.close()


@pytest.mark.parametrize("n,m,law", [(n, m, "mirror") for n, m in PLANTED] + [(n, m, "skip3") for n, m in SKIP3])
def test_greedy_planted_pairs(oracle_mod, n, m, law):
    """Levels of 64, 65, 128, 129 nodes and 32 / 33 / 34 / 65 sample words
    through k_sample_scatter, k_similarity and the OR of the sample columns."""
    _planted(oracle_mod, n, m, law)


@pytest.mark.parametrize("n,m", PLANTED_1M)
def test_greedy_planted_pairs_at_the_sample_switch(oracle_mod, n, m):
    """n = 1,000,000: every row is the sample; n = 1,000,001: the reference's
    mt19937 sample gathered from the CSR."""
    _planted(oracle_mod, n, m, "mirror", s=5000)


# ---- random matrices ------------------------------------------------------------------------

@pytest.mark.parametrize("relax", [0, 2, 10, UNBOUNDED])
@pytest.mark.parametrize("part,arity", [("greedy", 2), ("basic", 2), ("basic", 5)])
def test_random_matrices(oracle_mod, part, arity, relax):
    """The shape is the oracle's; the context is the from-columns build's.
    All-zero columns: every product with them ties."""
    from genome_graph_annotation_amd import BRWTDevice
    from genome_graph_annotation_amd.brwt import shape_from_rows
    for n, m, d, seed in ((300, 23, 0.1, 1), (1000, 70, 0.03, 2), (129, 40, 0.5, 3), (200, 16, 0.0, 4)):
        dense = _random(n, m, d, seed)
        dense[:, [0, m // 2, m - 1]] = False
        off, cols = _csr(dense, "shuffled", seed=seed)
        want = oracle_mod.OracleTree.from_dense(dense, part, arity, relax).export()
        _same_shape(shape_from_rows(off, cols, m, part, arity, relax), want, f"{n}x{m}")
        ctx = BRWTDevice.from_rows(off, cols, m, arity=arity, partitioner=part, relax_max_arity=relax)
        ref = BRWTDevice.from_columns(B.pack(dense), n, arity, relax_max_arity=relax, layout="rows", partitioner=part)
        B.same_tree(ctx.export(), ref.export())
        B.same_tree(ctx.export(), want)
        assert ctx.num_relations() == ref.num_relations() == int(dense.sum())
        assert ctx.rows_stats() == ref.rows_stats()
        ctx.close()
        ref.close()


def test_empty_matrices():
    from genome_graph_annotation_amd.brwt import node_counts_from_rows, shape_from_rows
    none = np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    assert node_counts_from_rows(*none, 5, arity=2).tolist() == [0] * 9
    assert len(node_counts_from_rows(*none, 0, arity=2)) == 0
    assert len(shape_from_rows(*none, 0, "greedy")["num_children"]) == 0
    assert len(shape_from_rows(*none, 5, "greedy", relax_max_arity=10)["num_children"]) >= 6
    assert shape_from_rows(*none, 1, "greedy")["num_children"].tolist() == [0]


# ---- errors -------------------------------------------------------------------------------------

def test_errors_and_a_valid_call_after_each(oracle_mod):
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    from genome_graph_annotation_amd.brwt import _rows_desc, basic_shape, node_counts_from_rows, shape_from_rows
    n, m = 200, 12
    dense = _random(n, m, 0.3, 90)
    dense[5, :3] = True
    off, cols = _csr(dense)
    want = oracle_mod.OracleTree.from_dense(dense, "greedy", 2, 10).export()

    def valid():
        _same_shape(shape_from_rows(off, cols, m, "greedy", relax_max_arity=10), want)
        _counts_are(dense, basic_shape(m, 3), node_counts_from_rows(off, cols, m, arity=3), off)

    def fails(status, fn, *args, **kw):
        with pytest.raises(MBRWTError) as e:
            fn(*args, **kw)
        assert e.value.status == status, e.value
        valid()

    valid()
    fails(L.MBRWT_ERR_INVALID, shape_from_rows, off, cols, m, 7)  # no such partitioner
    for arity in (1, 65):
        fails(L.MBRWT_ERR_INVALID, shape_from_rows, off, cols, m, "basic", arity)
        fails(L.MBRWT_ERR_INVALID, shape_from_rows, off, cols, m, "basic", arity, 10)
    big = cols.copy()
    big[len(big) // 2] = m
    a = int(off[5])
    dup = cols.copy()
    dup[a + 2] = dup[a]  # row 5: a column twice (not adjacent)
    desc = off.copy()
    desc[7] = desc[8] + 1  # offsets[7] > offsets[8]
    for o, c in ((off, big), (off, dup), (desc, cols)):
        fails(L.MBRWT_ERR_INVALID, node_counts_from_rows, o, c, m, arity=3)
        fails(L.MBRWT_ERR_INVALID, shape_from_rows, o, c, m, "greedy")
        fails(L.MBRWT_ERR_INVALID, shape_from_rows, o, c, m, "basic", 3, 10)
    bad = {k: np.array(v, copy=True) for k, v in basic_shape(m, 3).items()}
    leaves = np.flatnonzero(bad["num_children"] == 0)
    bad["leaf_column"][leaves[1]] = bad["leaf_column"][leaves[0]]  # not a permutation
    fails(L.MBRWT_ERR_INVALID, node_counts_from_rows, off, cols, m, shape=bad)
    # null pointers, straight at the C ABI
    lib = L.lib()
    d, keep = _rows_desc(off, cols, m)
    counts = np.zeros(64, dtype=np.uint64)
    h = C.c_void_p()
    assert lib.mbrwt_rows_node_counts(None, None, 3, 0, counts.ctypes.data_as(L.u64p)) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_rows_node_counts(C.byref(d), None, 3, 0, None) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_tree_shape_from_rows(None, 1, 2, 0, 0, C.byref(h)) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_tree_shape_from_rows(C.byref(d), 1, 2, 0, 0, None) == L.MBRWT_ERR_INVALID
    no_off = L.RowsDesc(n, m, None, keep[1].ctypes.data_as(L.u32p))
    assert lib.mbrwt_rows_node_counts(C.byref(no_off), None, 3, 0, counts.ctypes.data_as(L.u64p)) == \
        L.MBRWT_ERR_INVALID
    assert lib.mbrwt_tree_shape_from_rows(C.byref(no_off), 1, 2, 0, 0, C.byref(h)) == L.MBRWT_ERR_INVALID
    valid()
    with pytest.raises(ValueError):
        BRWTDevice.from_rows(off, cols, m, shape=basic_shape(m, 2), partitioner="greedy")
    with pytest.raises(ValueError):
        BRWTDevice.from_rows(off, cols, m, shape=basic_shape(m, 2), relax_max_arity=10)
    valid()
