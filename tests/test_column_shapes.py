"""The fixtures of tests/column_shapes.py checked on the CPU: every matrix
reaches the lengths, block totals and gap features its GPU test
(tests/test_gpu_column_edges.py) is named for.  The model is plain numpy -- a
node's length is the number of rows with any column of its subtree set -- and
is compared with vec_size of the oracle's export (the oracle runs on the
CPU)."""
import numpy as np
import pytest

import column_shapes as S


def _export_matches_model(O, dense, tree, arity):
    """The oracle's tree of `dense` has the model's shape and lengths."""
    ex = O.OracleTree.from_dense(dense, "basic", arity).export()
    np.testing.assert_array_equal(np.asarray(ex["num_children"]), tree.num_children)
    internal = tree.num_children > 0
    np.testing.assert_array_equal(np.asarray(ex["first_child"])[internal], tree.first_child[internal])
    np.testing.assert_array_equal(np.asarray(ex["leaf_column"])[~internal], tree.leaf_column[~internal])
    lengths, vec_size = S.node_lengths(dense, tree)
    np.testing.assert_array_equal(np.asarray(ex["vec_size"]).astype(np.int64), vec_size)
    return lengths


# ---- the gap patterns ---------------------------------------------------------------

def test_gap_pattern_features():
    for K in list(range(1, 200)) + [8191, 8192, 8193, 8200, 16775, 33927]:
        bits = S.gap_pattern(K)
        f = S.gap_features(bits)
        assert int(bits.sum()) == K and bits[-1] and len(bits) % S.WORD == 7, K
        # a gap of at least 100 rows, empty blocks first and last, the final one at len - 1: always
        gaps = np.diff(np.flatnonzero(np.concatenate([[True], bits])))
        assert int(gaps.max()) > 100, K
        for name in ("empty_run_at_start", "empty_run_at_end", "partial_last_block_ends_on_a_one"):
            assert f[name], (K, name)
        if K >= S.FULL_FEATURES_FROM:
            assert all(f[name] for name in S.ALL_GAP_FEATURES), (K, f)
        # the k-th one opens a block whose rank-before is k - 1, after empty blocks
        if K >= 2:
            blocks = np.flatnonzero(bits) // S.WORD
            opens = np.flatnonzero(np.diff(np.concatenate([[-1], blocks])) > 1)
            assert len(opens) >= 1, K


def test_cut_pattern_features():
    for n in list(range(1, 130)) + [447, 449, 3955, 8200]:
        bits = S.cut_pattern(n)
        assert len(bits) == n and bits[0] == (n < 14 * S.WORD - 31) and bits[-1], n
        if n > S.WORD and n < 14 * S.WORD - 31:
            assert bits[S.WORD - 1] and bits[S.WORD], n          # bit 31 of block 0, bit 0 of block 1
        if (n + 31) // 32 >= 14:
            f = S.gap_features(bits)
            want = [k for k in S.ALL_GAP_FEATURES if k != "partial_last_block_ends_on_a_one" or n % S.WORD]
            assert all(f[k] for k in want), (n, f)


def test_patterns_mean_what_they_say():
    G = S.GROUP
    for L in sorted(set(S.MASK_LENGTHS + S.PACK_LENGTHS + (2 * G + 1,))):
        P = {k: fn(L) for k, fn in S.PATTERNS.items()}
        for k, p in P.items():
            assert len(p) == len(set(p.tolist())) and (np.diff(p) > 0).all() and (p >= 0).all() and (p < L).all(), (L, k)
        assert len(P["empty"]) == 0 and P["pos0"].tolist() == [0] and P["last"].tolist() == [L - 1]
        assert P["mod31"].tolist() == [j for j in range(L) if j % 32 == 31]
        assert P["mod0"].tolist() == [j for j in range(L) if j % 32 == 0]
        assert P["edge8192"].tolist() == [j for j in (G - 1, G) if j < L]
        assert (P["from8192"] >= G).all() and (len(P["from8192"]) > 0) == (L > G)
        w = P["wg0wg2"]
        assert (len(w) > 0) == (L > 2 * G)
        if len(w):
            assert (w < G).any() and (w >= 2 * G).any() and not ((w >= G) & (w < 2 * G)).any()
        assert len(P["full"]) == L
        # a name is listed exactly where its pattern has a position
        for k in ("mod31", "edge8192", "from8192", "wg0wg2"):
            assert (k in S.pattern_names(L)) == (len(P[k]) > 0), (L, k)
    # every pattern appears in some matrix of every slot count used, the top slot is 'last' or 'mod31'
    for L in S.MASK_LENGTHS:
        for slots in (1, 4, 7, 15, 31, 32, 63):
            parts = S.pattern_parts(L, slots)
            assert all(len(p) == slots for p in parts)
            assert set(S.pattern_names(L)) <= {name for p in parts for name in p}
            if slots > 1:
                assert all(p[-1] in ("last", "mod31") for p in parts)
            else:
                assert ["full"] in parts


# ---- the leaf-parent configurations -------------------------------------------------------

def _cases():
    for name, cfg in S.CONFIGS.items():
        for L in cfg.lengths:
            yield name, L


@pytest.mark.parametrize("name,L", list(_cases()))
def test_leaf_parent(oracle_mod, name, L):
    cfg = S.CONFIGS[name]
    tree = cfg.tree()
    seen = set()
    for part in range(cfg.parts(L)):
        f = cfg.build(L, part)
        assert (f.n, f.m) == f.dense.shape and f.m == cfg.m and f.L == L == len(f.R)
        # R is spread out: a gap of at least 100 rows, so the lift through the super-root moves positions
        gaps = np.diff(np.concatenate([[-1], f.R, [f.n]])) - 1
        assert int(gaps.max()) >= 100 and not np.array_equal(f.R, np.arange(L))
        lengths = _export_matches_model(oracle_mod, f.dense, tree, cfg.arity)
        assert int(lengths[cfg.node]) == L, (name, L, part, int(lengths[cfg.node]))
        # only the rows of R touch the extraction node's columns, every pattern column holds its pattern
        cols = tree.columns[cfg.node]
        np.testing.assert_array_equal(np.flatnonzero(f.dense[:, cols].any(axis=1)), f.R)
        for c, pname in f.patterns.items():
            np.testing.assert_array_equal(np.flatnonzero(f.dense[:, c]), f.R[S.PATTERNS[pname](L)])
            seen.add(pname)
        # the highest child slot (the top bit of the masks) holds 'last' or 'mod31'
        if cfg.slots > 1:
            assert f.patterns[int(cols.max())] in ("last", "mod31"), (name, L, part)
        if cfg.packed == "pack":
            pairs = S.pack_pairs(f.dense, tree, cfg.node)
            full = L // S.PACK_SPAN
            assert len(pairs) == (L + S.PACK_SPAN - 1) // S.PACK_SPAN
            want = np.full(full, S.PACK_AREA)
            if len(pairs) >= 20:
                want[S.PACK_SPILL_BLOCK] = S.PACK_AREA + 1      # spilled, between two inline blocks of 48
            np.testing.assert_array_equal(pairs[:full], want)
            assert (pairs[full:] == 3 * (L % S.PACK_SPAN)).all()
            assert int((pairs > S.PACK_AREA).sum()) * 20 <= len(pairs)   # or the builder declines PACK
        if cfg.packed in ("pack2", "packt"):
            sizes = S.record_sizes(f.dense, tree, cfg.node, cfg.packed == "packt")
            span, spilled = S.record_span(sizes, cfg.packed == "packt")
            assert span == cfg.stride(f) and int(sizes.max()) <= S.RECORD_BLOCK
            # the span the fixture is named for, once there are more records than one block of it holds
            # (fewer records fit one block of a larger span, which the builder then takes)
            assert span >= cfg.S and (span == cfg.S or L <= cfg.S), (name, L, span)
            if L >= 20 * 8 and name != "packt-wide" and cfg.S in (8, 4, 3) and name not in ("packt-s7", "packt-s5"):
                assert len(spilled) == 1 and 0 < spilled[0] < len(sizes) // span - 1, (name, L, spilled)
    assert set(S.pattern_names(L)) <= seen | {"full"}, (name, L, seen)
    assert "full" in seen


def test_configs_cover_the_issue():
    """The lengths and shapes the GPU file runs."""
    for name in ("mask8", "mask16", "mask32", "mask64-bit32", "mask64-bit63", "plane"):
        assert S.CONFIGS[name].lengths == (1, 31, 32, 33, 8191, 8192, 8193, 16385)
    assert S.CONFIGS["pack"].lengths == (1, 15, 16, 17, 31, 32, 33, 8191, 8192, 8193)
    for name, cfg in S.CONFIGS.items():
        if cfg.packed in ("pack2", "packt") and name != "packt-wide":
            want = {1, cfg.S - 1, cfg.S, cfg.S + 1, 31, 32, 33, 8191, 8192, 8193}
            assert set(cfg.lengths) == want, name
    assert any(32 % c.S for c in S.CONFIGS.values() if c.packed == "packt")
    t = S.CONFIGS["packt-wide"].tree()
    assert int(t.num_children[0]) > 8 and int(t.num_children[S.CONFIGS["packt-wide"].node]) > 8
    assert t.path(128)[0] == (0, 8)                      # the super-root lift at child slot 8
    assert S.CONFIGS["plane-wide"].tree().path(128) == [(0, 8), (9, 0)]
    assert S.CONFIGS["plane"].tree().path(8) == [(0, 1)]  # a leaf child of a PLANE node
    for name, top in (("mask64-bit32", 32), ("mask64-bit63", 63), ("mask32", 31), ("mask16", 15), ("mask8", 7)):
        assert S.CONFIGS[name].tree().path(top) == [(0, top)]


# ---- the lift fixture -------------------------------------------------------------------------

@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("T", S.LIFT_DEEPEST)
def test_lift_fixture(oracle_mod, T, mirror):
    f = S.lift_fixture(T, mirror)
    tree = S.BasicTree(16, 2)
    lengths = _export_matches_model(oracle_mod, f.dense, tree, 2)
    path = tree.path(f.column)
    assert len(path) == 4 and [s for _, s in path] == [int(mirror)] * 4   # root, A, B, C: three lifts and the super-root's
    R0, R1, R2, R3, R4 = f.sets
    assert [int(lengths[u]) for u, _ in path] == [len(R0), len(R1), len(R2), len(R3)] and len(R2) == T
    np.testing.assert_array_equal(np.flatnonzero(f.dense[:, f.column]), R4)
    for a, b in zip(f.sets, f.sets[1:]):
        assert len(b) < len(a) and np.isin(b, a).all()
    # the child column inside every image a lift searches: n rows (the super-root), R0 (the root), R1 (A)
    for cut, inside in zip(f.cuts[:3], (f.n, len(R0), len(R1))):
        feats = S.gap_features(cut)
        # (the cut to R2's T rows has no ones to spare for a full block below T = 35)
        want = [k for k in S.ALL_GAP_FEATURES if k != "full_block" or int(cut.sum()) >= S.FULL_FEATURES_FROM]
        assert len(cut) == inside and all(feats[k] for k in want), (T, feats)
    # ... and R2 (B), the deepest: one, two, three blocks, or more than a workgroup's positions
    deepest = S.gap_features(f.cuts[3])
    assert deepest["blocks"] == {31: 1, 64: 2, 65: 3, 8200: 257}[T]
    assert f.cuts[3][0] == (T < 8200) and f.cuts[3][-1]
    if T == 8200:
        assert all(deepest[k] for k in S.ALL_GAP_FEATURES) and len(R3) > 32 * 100
    if T == 65:
        assert f.cuts[3][31] and f.cuts[3][32] and f.cuts[3][64]   # bit 31, bit 0 of the next block, a one-bit last block
    # the other columns hold the differences, so every level's rows come out of some column
    other = (lambda c: 15 - c) if mirror else (lambda c: c)
    for col, rows, without in ((1, R3, R4), (2, R2, R3), (4, R1, R2), (8, R0, R1)):
        np.testing.assert_array_equal(np.flatnonzero(f.dense[:, other(col)]), np.setdiff1d(rows, without))
    assert f.n <= 140_000


def test_plane_wide_lift(oracle_mod):
    """The lift through a PLANE of nine children at child slot 8 (8 bytes per child in a block)."""
    cfg = S.CONFIGS["plane-wide"]
    f = cfg.build(70, 0)
    tree = cfg.tree()
    lengths = _export_matches_model(oracle_mod, f.dense, tree, 16)
    assert int(tree.num_children[0]) == 9 and int(lengths[9]) == 70
    child = np.isin(np.flatnonzero(f.dense.any(axis=1)), f.R)      # child 8's column in the root's image
    assert len(child) == int(lengths[0]) and all(S.gap_features(child)[k] for k in S.ALL_GAP_FEATURES)


# ---- row shards -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [257, 319])
def test_shard_matrix(n):
    d = S.shard_matrix(n)
    R, C = S.SHARD_ROWS, S.SHARD_COLUMNS
    assert n % R in (1, 63) and d.shape == (n, 8)
    shard = np.arange(n) // R
    per = lambda c: np.bincount(shard[d[:, c]], minlength=shard[-1] + 1)   # noqa: E731
    assert np.flatnonzero(d[:, C["boundary"]]).tolist() == [63, 64, n - 1]
    assert n - 1 >= 4 * R   # (the last shard is a partial one of its own)
    assert per(C["not_in_shard_0"])[0] == 0 and (per(C["not_in_shard_0"])[1:] > 0).all()
    assert per(C["not_in_a_middle_shard"])[2] == 0 and (np.delete(per(C["not_in_a_middle_shard"]), 2) > 0).all()
    assert per(C["first_shard_only"])[0] > 1 and (per(C["first_shard_only"])[1:] == 0).all()
    assert (per(C["first_three_shards"])[:3] > 1).all() and (per(C["first_three_shards"])[3:] == 0).all()
    assert (per(C["every_shard"]) >= (1 if n % R == 1 else 3)).all() and d[n - 1, C["every_shard"]]
    assert not d[:, C["empty"]].any() and d[:, C["full"]].all()
