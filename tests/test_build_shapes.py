"""The builder fixture (tests/build_shapes.py) pinned on the CPU: the closed
form of the bottom-up build against the oracle's trees, the planted pairs
against the oracle's greedy matching, and the properties of the fixture the
GPU tests of test_gpu_build_edges.py rely on."""
import numpy as np
import pytest

import build_shapes as B

ROWS = (1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 16383, 16384, 16385)
ARITIES = (2, 3, 8, B.BASE_COLUMNS, 64)
# (n, m) of the planted matrices: SW = 32, 33, 33, 34, 34 and 65 sample words;
# m = 64, 65, 128, 129, 130, 192 columns (one to three 64-column tiles)
PLANTED = ((2048, 64), (2112, 65), (2112, 128), (2113, 129), (2113, 130), (4097, 192))
PLANTED_1M = ((1_000_000, 12), (1_000_001, 12))
SKIP3 = ((2112, 66), (2112, 126), (2113, 132))
SIM_TILE, SIM_CHUNK = 64, 32   # csrc/build.hip kSimTile, kSimChunk


@pytest.mark.parametrize("n", ROWS)
def test_bottom_up_closed_form_against_oracle(oracle_mod, n):
    dense = B.edge_columns(n, B.BASE_COLUMNS)
    for arity in ARITIES:
        t = oracle_mod.OracleTree.from_dense(dense, "basic", arity, 0)
        mine = B.bottom_up(dense, arity)
        B.same_tree(mine, t.export())
        if arity >= B.BASE_COLUMNS:   # one group: the root is the only parent
            assert mine["num_nodes"] == B.BASE_COLUMNS + 1 and mine["num_children"][0] == B.BASE_COLUMNS


def test_bottom_up_two_cycles_and_one_column(oracle_mod):
    for n in (1, 65, 4097):
        for m, arity in ((2 * B.BASE_COLUMNS, 2), (2 * B.BASE_COLUMNS, 64), (65, 64), (1, 2), (2, 2), (3, 2)):
            dense = B.edge_columns(n, m)
            B.same_tree(B.bottom_up(dense, arity), oracle_mod.OracleTree.from_dense(dense, "basic", arity, 0).export())


def test_columns_without_rows(oracle_mod):
    """n = 0, m > 0: 2 m - 1 nodes over empty vectors."""
    dense = np.zeros((0, 5), dtype=bool)
    t = oracle_mod.OracleTree.from_dense(dense, "basic", 2, 0)
    mine = B.bottom_up(dense, 2)
    B.same_tree(mine, t.export())
    assert mine["num_nodes"] == 9 and not mine["vec_size"].any() and t.num_rows() == 0 and t.num_columns() == 5


def test_same_tree_sees_one_bit_and_one_length(oracle_mod):
    dense = B.edge_columns(129, B.BASE_COLUMNS)
    a = B.bottom_up(dense, 2)
    for key in ("words", "vec_size"):
        b = dict(a, words=[w.copy() for w in a["words"]], vec_size=a["vec_size"].copy())
        u = int(np.argmax(a["vec_size"] % 64 == 1))   # a node with one bit in its last word: same word count
        assert a["vec_size"][u] % 64 == 1
        if key == "words":
            b["words"][u][-1] ^= np.uint64(2)         # a bit past the length: the words are compared unmasked
        else:
            b["vec_size"][u] += 1
        with pytest.raises(AssertionError):
            B.same_tree(a, b)


def test_pack_and_tails():
    for n in (1, 63, 64, 65, 129):
        dense = B.edge_columns(n, 30)
        w = B.pack(dense)
        assert w.shape == (30, (n + 63) // 64) and w.dtype == np.uint64
        bits = np.unpackbits(w.view(np.uint8).reshape(30, -1), axis=1, bitorder="little")
        np.testing.assert_array_equal(bits[:, :n].astype(bool), dense.T)
        assert not bits[:, n:].any()
        g = B.with_tail_garbage(w, n)
        gb = np.unpackbits(g.view(np.uint8).reshape(30, -1), axis=1, bitorder="little")
        np.testing.assert_array_equal(gb[:, :n], bits[:, :n])
        assert gb[:, n:].all() and (n % 64 == 0 or not np.array_equal(g, w))
    s = B.scattered(1000, 7, 50, 3)
    assert s.shape == (7, 16) and not (s[:, -1] >> np.uint64(1000 % 64)).any()
    pop = np.unpackbits(s.view(np.uint8).reshape(7, -1), axis=1).sum(axis=1)
    assert (pop <= 50).all() and (pop >= 40).all()
    np.testing.assert_array_equal(s, B.scattered(1000, 7, 50, 3))


# ---- planted pairs -----------------------------------------------------------

def _greedy(O, dense, relax=0):
    return O.OracleTree.from_dense(dense, "greedy", 2, relax)


@pytest.mark.parametrize("n,m", PLANTED)
def test_planted_mirror_pairs_recovered_by_oracle(oracle_mod, n, m):
    dense, pairs = B.planted_pairs(n, m, "mirror")
    assert len(pairs) == m // 2 and len({b - a for a, b in pairs}) == len(pairs)   # every distance distinct
    np.testing.assert_array_equal(dense.sum(axis=0)[[c for p in pairs for c in p]], 16)
    assert int((dense.sum(axis=1) == 2).sum()) == 16 * len(pairs) and int(dense.sum(axis=1).max()) == 2
    assert set(pairs) <= B.leaf_pairs(_greedy(oracle_mod, dense).export())


@pytest.mark.parametrize("n,m", PLANTED_1M)
def test_planted_mirror_pairs_recovered_at_the_sample_switch(oracle_mod, n, m):
    dense, pairs = B.planted_pairs(n, m, "mirror", s=5000)
    t = oracle_mod.OracleTree.from_words(B.pack(dense).reshape(-1), n, m, "greedy", 2, 0)
    assert set(pairs) <= B.leaf_pairs(t.export())


@pytest.mark.parametrize("n,m", SKIP3)
def test_planted_skip3_pairs_recovered_by_oracle(oracle_mod, n, m):
    dense, pairs = B.planted_pairs(n, m, "skip3")
    assert len(pairs) == 3 * (m // 6) and all(b - a == 3 for a, b in pairs)
    # both partners inside one tile, but for at most two pairs across each tile edge
    inside = [(a, b) for a, b in pairs if a // SIM_TILE == b // SIM_TILE]
    assert len(inside) >= len(pairs) - 2 * (m // SIM_TILE)
    assert set(pairs) <= B.leaf_pairs(_greedy(oracle_mod, dense).export())


def test_planted_fixture_reaches_the_similarity_edges():
    """What the GPU tests rely on: the last, partial chunk of the sampled
    words and the last, partial tile of columns each decide a planted pair."""
    # n = 2112: 33 sample words, the last chunk is the single word 32
    n = 2112
    SW = (n + 63) // 64
    assert SW == 33 and SW % SIM_CHUNK == 1
    for m in (65, 128):
        dense, pairs = B.planted_pairs(n, m, "mirror")
        last = [(a, b) for a, b in pairs if (np.nonzero(dense[:, a])[0] // 64 >= SIM_CHUNK).all()]
        far = [(a, b) for a, b in last if b - a >= m / 2]
        assert len(far) >= 2, (m, last)
        # without the last chunk those partners share nothing; the comparator then
        # prefers the smallest distance among zero products: never the planted partner
        assert all(b - a > 1 for a, b in pairs if (a, b) in far)
    # m = 129 / 130: a mirror pair with a partner in the partial third tile
    for m in (129, 130):
        _, pairs = B.planted_pairs(2113, m, "mirror")
        assert m % SIM_TILE in (1, 2) and any(b // SIM_TILE == 2 and a // SIM_TILE == 0 for a, b in pairs)
    # skip3 at m = 132: a pair wholly inside the partial tile
    _, pairs = B.planted_pairs(2113, 132, "skip3")
    assert any(a // SIM_TILE == 2 and b // SIM_TILE == 2 for a, b in pairs)
    # a level of L = 64, 65, 128, 129 nodes: m = 64, 65, 128, 129 (first level) and 128, 129, 130 (second)
    assert {m for _, m in PLANTED} >= {64, 65, 128, 129} and (130 + 1) // 2 == 65 and (129 + 1) // 2 == 65
    # the sample switch: n <= 1,000,000 samples every row
    assert [n for n, _ in PLANTED_1M] == [1_000_000, 1_000_001]


# ---- edge columns: the structures the builder kernels must meet --------------

def _internal_zero_length(tree):
    nc = np.asarray(tree["num_children"])
    return np.nonzero((nc > 0) & (np.asarray(tree["vec_size"]) == 0))[0]


@pytest.mark.parametrize("n", [65, 4097, 16385])
def test_edge_columns_structures(oracle_mod, n):
    m = 2 * B.BASE_COLUMNS
    dense = B.edge_columns(n, m)
    assert dense.shape == (n, m)
    for cyc in range(2):
        c0 = cyc * B.BASE_COLUMNS
        assert not dense[:, [c0 + j for j in B.ZERO_COLUMNS]].any()          # an all-zero parent and grandparent
        a, b = (c0 + j for j in B.ONES_PARENT)
        assert (dense[:, a] | dense[:, b]).all() and not (dense[:, a] & dense[:, b]).any()   # all-ones parent words
        assert np.array_equal(dense[:, c0 + 20], dense[:, c0 + 21]) and dense[:, c0 + 20].any()
        assert dense[:, c0 + 22].mean() > 0.9
    # the second cycle differs from the first
    assert not np.array_equal(dense[:, 8], dense[:, 8 + B.BASE_COLUMNS])
    tree = B.bottom_up(dense, 2)
    zl = _internal_zero_length(tree)
    assert len(zl) >= 2 * 2, zl            # per cycle: the two parents of zero columns under a zero grandparent
    # a k_pext output that straddles two words with a 64-bit payload: a full parent word at an odd offset
    if n >= 4097:
        par = dense[:, 22] | dense[:, 23]
        full = par[: n // 64 * 64].reshape(-1, 64).all(axis=1)
        before = np.concatenate([[0], np.cumsum(par[: n // 64 * 64].reshape(-1, 64).sum(axis=1))[:-1]])
        assert (full & (before % 64 != 0)).any()


@pytest.mark.parametrize("n", [65, 4097, 16385])
@pytest.mark.parametrize("relax", [4, 10, 2**64 - 1])
def test_oracle_relax_prunes_the_zero_length_node(oracle_mod, n, relax):
    """BRWTOptimizer::relax removes the internal nodes of index length 0 (the
    !Wn branch of the device's reassign) and lowers the node count."""
    dense = B.edge_columns(n, B.BASE_COLUMNS)
    plain = oracle_mod.OracleTree.from_dense(dense, "basic", 2, 0).export()
    relaxed = oracle_mod.OracleTree.from_dense(dense, "basic", 2, relax).export()
    assert plain["num_nodes"] == 2 * B.BASE_COLUMNS - 1
    assert len(_internal_zero_length(plain)) == 2
    assert len(_internal_zero_length(relaxed)) == 0
    assert relaxed["num_nodes"] < plain["num_nodes"]


def test_grid_stride_case_strides_both_level_kernels():
    """csrc/build.hip grid_of caps x * y at 65,536 blocks: the leaf level of
    the grid-stride case takes more than one stride in k_or and in k_pext."""
    c = B.GRID_STRIDE_CASE
    W = (c["n"] + 63) // 64
    groups, children = c["m"] // 2, c["m"]
    assert W == 6146 and groups * W >= 3 * 2**23
    assert B.grid_of(W, groups) == 16 and B.grid_of(W, children) == 8
    s_or, s_pext = B.level_strides(W, groups, children)
    assert s_or >= 2 and s_pext >= 2, (s_or, s_pext)
    assert c["n"] % 64 != 0   # a tail for the garbage bits
