"""GPU parity of the device builder (csrc/build.hip) on the deterministic
fixture of tests/build_shapes.py instead of a random law.  Every comparison
is the whole tree, bit for bit (build_shapes.same_tree on export(): shape,
index lengths and every node's index words, unmasked), against the numpy
closed form of the bottom-up build and against the CPU oracle; the queries
over all rows come second.

k_or / k_pext / k_clear_tails (the level kernels):
  * row counts either side of a word (63..65, 127..129), of a 64-word run
    (4095..4097) and of one full 256-thread block of words (16383..16385)
  * all-ones parent words (pext64's shortcut), all-zero parents (children of
    index length 0), full 64-bit payloads that straddle two output words
  * groups of 2, 3, 8, all columns, 64; a pass-through on every level
  * the grid-stride loops (groups x words > 2^24): test_grid_stride
  * columns uploaded one by one, in any memory order, with garbage tails
k_popc_words / k_expand / relax_nodes: test_relax_*, the reference's grids.
k_similarity / k_gather_sample (greedy): planted pairs at the tile (64
columns) and chunk (32 sample words) edges, and either side of the row count
from which the row sample is gathered.
"""
import numpy as np
import pytest

import build_shapes as B
from conftest import gpu_available
from test_build_shapes import ARITIES, PLANTED, PLANTED_1M, ROWS, SKIP3
from test_gpu_parity import _check_rows, _grid

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU"),
              pytest.mark.usefixtures("nodes_layout")]

UNBOUNDED = 2**64 - 1


def _all_rows(n, cap=16385, sample=4000):
    """Every row up to `cap` rows; beyond, the first and last 64 and a random sample."""
    if n <= cap:
        return np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(n)
    return np.concatenate([np.arange(64), np.arange(n - 64, n), rng.integers(0, n, sample)]).astype(np.uint64)


def _built_is(built, t, n, m, variants=(0, 1)):
    """The built context holds the oracle's tree `t`, and answers like it."""
    B.same_tree(built.export(), t.export())
    assert built.num_rows() == n and built.num_columns() == m
    assert built.num_relations() == t.num_relations()
    _check_rows(t, built, _all_rows(n), variants=variants)


# ---- the basic builder --------------------------------------------------------

@pytest.mark.parametrize("n", ROWS)
def test_basic_builder_edge_columns(oracle_mod, n):
    """from_columns of the edge columns is the closed form's tree and the
    oracle's, for every arity; two cycles of columns give arity 64 more than
    one group."""
    from genome_graph_annotation_amd import BRWTDevice
    O = oracle_mod
    for m in (B.BASE_COLUMNS, 2 * B.BASE_COLUMNS + 17):
        dense = B.edge_columns(n, m)
        words = B.pack(dense)
        for arity in ARITIES:
            built = BRWTDevice.from_columns(words, n, arity)
            B.same_tree(built.export(), B.bottom_up(dense, arity))
            _built_is(built, O.OracleTree.from_dense(dense, "basic", arity, 0), n, m)


@pytest.mark.parametrize("relax", [0, UNBOUNDED])
@pytest.mark.parametrize("kind", ["zero", "one", "mixed"])
def test_reference_grids_through_the_builder(oracle_mod, kind, relax):
    """test_BRWT.cpp:152-212 / test_BRWT_optimizer.cpp:102-163: the grids 1..19
    x 1..19 at arity 2, built (and relaxed) on the device from their columns."""
    from genome_graph_annotation_amd import BRWTDevice
    O = oracle_mod
    for n in range(1, 20):
        for m in range(1, 20):
            dense = _grid(kind, n, m)
            built = BRWTDevice.from_columns(B.pack(dense), n, 2, relax_max_arity=relax)
            _built_is(built, O.OracleTree.from_dense(dense, "basic", 2, relax), n, m, variants=(0,))


@pytest.mark.parametrize("n", [65, 4097])
def test_upload_forms_and_tails(oracle_mod, n):
    """mbrwt_columns_desc takes one pointer per column: columns allocated one
    by one, laid out in reversed memory order, or as rows of a wider array
    (contiguous rows, another stride) take the per-column upload; bits past
    num_rows are ignored (include/mbrwt.h).  All build the contiguous build's tree."""
    from genome_graph_annotation_amd import BRWTDevice
    m, arity = 2 * B.BASE_COLUMNS, 8
    W = (n + 63) // 64
    dense = B.edge_columns(n, m)
    words = B.pack(dense)
    want = BRWTDevice.from_columns(words, n, arity).export()
    B.same_tree(want, B.bottom_up(dense, arity))

    def back_to_back(cols):
        return all(c.ctypes.data == cols[0].ctypes.data + 8 * W * j for j, c in enumerate(cols))

    assert back_to_back(list(words))
    garbage = B.with_tail_garbage(words, n)
    assert not np.array_equal(garbage, words)
    forms = {}
    forms["separate arrays"] = [words[j].copy() for j in range(m)]
    block = np.ascontiguousarray(words[::-1])
    forms["reversed memory order"] = [block[m - 1 - j] for j in range(m)]
    wide = np.full((m, W + 1), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    wide[:, :W] = words
    forms["rows of a wider array"] = [wide[j, :W] for j in range(m)]
    forms["tail garbage"] = garbage
    gwide = wide.copy()
    gwide[:, :W] = garbage
    forms["tail garbage, rows of a wider array"] = [gwide[j, :W] for j in range(m)]
    for name, cols in forms.items():
        cols = list(cols)
        assert all(c.flags.c_contiguous and len(c) == W for c in cols)
        assert back_to_back(cols) == (name == "tail garbage"), name
        if name == "reversed memory order":
            assert cols[1].ctypes.data == cols[0].ctypes.data - 8 * W
        for j in range(m):
            np.testing.assert_array_equal(cols[j], (garbage if "garbage" in name else words)[j])
        built = BRWTDevice.from_columns(cols, n, arity)
        B.same_tree(built.export(), want)
        assert built.num_relations() == int(dense.sum()), name


def test_columns_without_rows():
    """num_rows = 0 with columns: the reference builds the 2 m - 1 nodes over
    empty vectors.  The builder launches no level kernel over zero words and
    every image is its padding alone: the context reports the shape, answers
    an empty batch, and every row is out of range."""
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    m = 5
    built = BRWTDevice.from_columns([np.zeros(0, dtype=np.uint64) for _ in range(m)], 0, 2)
    assert built.num_rows() == 0 and built.num_columns() == m
    assert built.num_relations() == 0 and built.num_nodes() == 2 * m - 1
    off, cols = built.get_rows(np.zeros(0, dtype=np.uint64))
    assert off.tolist() == [0] and len(cols) == 0
    with pytest.raises(MBRWTError) as ei:
        built.get_rows(np.array([0], dtype=np.uint64))
    assert ei.value.status == L.MBRWT_ERR_RANGE


# ---- relax -------------------------------------------------------------------------

@pytest.mark.parametrize("relax", [2, 3, 4, 10, UNBOUNDED])
@pytest.mark.parametrize("n", [65, 4097, 16385])
def test_relax_edge_columns(oracle_mod, n, relax):
    """BRWTOptimizer::relax (BRWT_builders.cpp:166-297) of the arity-2 tree of
    the edge columns: builder + relax on the device and relax of the exported
    plain tree both give the oracle's relaxed tree -- the zero-length internal
    nodes are pruned (reassign without an index), the 97 % columns' parents
    expand through full words and 64-bit straddles."""
    from genome_graph_annotation_amd import BRWTDevice
    O = oracle_mod
    for m in (B.BASE_COLUMNS, 2 * B.BASE_COLUMNS):
        dense = B.edge_columns(n, m)
        words = B.pack(dense)
        plain = O.OracleTree.from_dense(dense, "basic", 2, 0)
        t = O.OracleTree.from_dense(dense, "basic", 2, relax)
        if relax >= 4:
            assert t.num_nodes() < plain.num_nodes()
        _built_is(BRWTDevice.from_columns(words, n, 2, relax_max_arity=relax), t, n, m)
        _built_is(BRWTDevice.from_tree(plain.export(), relax_max_arity=relax), t, n, m, variants=(0,))


@pytest.mark.parametrize("relax", [0, 2, 3, 4, 10, UNBOUNDED])
@pytest.mark.parametrize("n", [65, 4097, 16385])
def test_greedy_edge_columns(oracle_mod, n, relax):
    """The greedy partitioner (+ relax) on the edge columns: zero, identical
    and complementary columns give tied similarities at every level."""
    from genome_graph_annotation_amd import BRWTDevice
    O = oracle_mod
    m = 2 * B.BASE_COLUMNS
    dense = B.edge_columns(n, m)
    built = BRWTDevice.from_columns(B.pack(dense), n, 2, relax_max_arity=relax, partitioner="greedy")
    _built_is(built, O.OracleTree.from_dense(dense, "greedy", 2, relax), n, m, variants=(0,))


# ---- greedy: planted pairs ------------------------------------------------------------

def _planted(O, n, m, law, s=16):
    from genome_graph_annotation_amd import BRWTDevice
    dense, pairs = B.planted_pairs(n, m, law, s)
    words = B.pack(dense)
    built = BRWTDevice.from_columns(words, n, 2, partitioner="greedy")
    got = B.leaf_pairs(built.export())
    missing = sorted(set(pairs) - got)
    assert not missing, f"planted pairs not matched: {missing}"
    for relax in (0, 10):
        t = O.OracleTree.from_words(words.reshape(-1), n, m, "greedy", 2, relax)
        if relax:
            built = BRWTDevice.from_columns(words, n, 2, relax_max_arity=relax, partitioner="greedy")
        B.same_tree(built.export(), t.export())
        assert built.num_relations() == 2 * s * len(pairs)
        _check_rows(t, built, _all_rows(n), variants=(0,))


@pytest.mark.parametrize("n,m,law", [(n, m, "mirror") for n, m in PLANTED] + [(n, m, "skip3") for n, m in SKIP3])
def test_greedy_planted_pairs(oracle_mod, n, m, law):
    """k_similarity at its edges: levels of 64, 65, 128, 129 nodes, a partial
    diagonal tile, 32 / 33 / 34 / 65 sample words (a last chunk of one word).
    A product read as 0 breaks a planted pair: among zero products the
    comparator takes the smallest distance, never the planted partner."""
    _planted(oracle_mod, n, m, law)


@pytest.mark.parametrize("n,m", PLANTED_1M)
def test_greedy_planted_pairs_at_the_sample_switch(oracle_mod, n, m):
    """n = 1,000,000: the columns themselves are the sample; n = 1,000,001:
    k_gather_sample over the reference's row sample."""
    _planted(oracle_mod, n, m, "mirror", s=5000)


# ---- the grid-stride loops of the level kernels -------------------------------------------

def test_grid_stride(oracle_mod):
    """8,192 columns x 393,281 rows at arity 2: the leaf level holds 1.5 x 2^24
    group-words, so k_or and k_pext both take more than one stride under
    grid_of (test_build_shapes.test_grid_stride_case_strides_both_level_kernels)."""
    from genome_graph_annotation_amd import BRWTDevice
    O = oracle_mod
    c = B.GRID_STRIDE_CASE
    n, m = c["n"], c["m"]
    words = B.scattered(n, m, c["bits_per_column"], seed=5)
    t = O.OracleTree.from_words(words.reshape(-1), n, m, "basic", 2, 0)
    built = BRWTDevice.from_columns(B.with_tail_garbage(words, n), n, 2)
    del words
    B.same_tree(built.export(), t.export())
    assert built.num_relations() == t.num_relations()
    _check_rows(t, built, _all_rows(n, sample=2000), variants=(0,))
