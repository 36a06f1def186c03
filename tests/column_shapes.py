"""Deterministic fixtures of the get_column edge tests on the per-node images
and on row shards (plain numpy: no GPU import, no oracle import).

csrc/column.hip answers get_column in two steps.  EXTRACTION reads the
leaf's set positions out of the image of its parent (or of the PACK / PACK2 /
PACKT ancestor that holds the levels below it): one thread per 32 positions,
256 threads per workgroup (8192 positions), a count pass, a scan over the
workgroups, an ordered write.  LIFTS then map every position through the
ancestors, select1 over the 32-position rank blocks of each ancestor's image
(a binary search for the last block whose rank-before is below k, then a
select inside one word), the last of them through the super-root.

  leaf_parent()   a matrix built around ONE leaf parent of a chosen length L:
                  a set R of exactly L rows carries the parent's anchor
                  column, R is spread over the rows by gap_pattern() (so the
                  lift through the super-root is not the identity), and the
                  parent's other columns carry the PATTERNS, written in the
                  parent's position space (position j = the j-th row of R).
  lift_fixture()  16 columns under the basic binary tree: nested row sets
                  R0 > R1 > R2 > R3 > R4 down the path to column 0 (or, mirrored,
                  column 15); every set is cut from its parent by gap_pattern()
                  / cut_pattern(), whose features (runs of empty blocks, ones at
                  bits 0 and 31, a full block, a last one at len - 1) are
                  what gap_features() reports.
  BasicTree       the shape the reference's basic partitioner gives m columns
                  (bottom-up groups of `arity`, a group of one passed through),
                  in BFS numbering: device node = BFS node + 1.
  node_lengths()  the plain model: a node's length is the number of rows with
                  any column of its subtree set.
  pack_pairs(), record_sizes(), record_span()
                  the models of the PACK block totals and of the PACK2 / PACKT
                  record blocks (csrc/image.cpp): what decides inline / spilled
                  and the span S.
  shard_matrix()  the row-shard matrix (64-row shards).
"""
import numpy as np

WORD = 32            # positions per thread of k_col_count / k_col_write, per rank block of k_col_lift
GROUP = 8192         # positions per workgroup (256 threads)
PACK_SPAN = 16       # positions per KIND_PACK block
PACK_AREA = 48       # (child, position) pairs a KIND_PACK block holds inline
RECORD_BLOCK = 64    # bytes of a PACK2 / PACKT block; 64 - S of them hold records inline

MASK_LENGTHS = (1, 31, 32, 33, 8191, 8192, 8193, 16385)
PACK_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 8191, 8192, 8193)


def span_lengths(S):
    """L around the multiples of a PACK2 / PACKT span S and of 32, around 8192."""
    return tuple(sorted({1, max(S - 1, 1), S, S + 1, 31, 32, 33, 8191, 8192, 8193}))


# ---- gap patterns ----------------------------------------------------------------

def gap_pattern(K):
    """bool [len] with exactly K >= 1 ones, the last of them at len - 1.  In
    32-blocks: two empty blocks; a block with bit 0 alone; a block with bit 31
    alone; four empty blocks (a gap of 128); a full block; two empty blocks; a
    run of ones at every odd position (its first one the first one of a block
    after empty blocks); two empty blocks; a last block of 7 positions with
    the final one.  Parts are left out, from the full block down, where K has
    no ones for them: K = 1 keeps the empty blocks and the final one."""
    assert K >= 1
    left = K - 1
    parts = [np.zeros(2 * WORD, dtype=bool)]
    if left >= 1:
        b = np.zeros(WORD, dtype=bool)
        b[0] = True
        parts.append(b)
        left -= 1
    if left >= 1:
        b = np.zeros(WORD, dtype=bool)
        b[WORD - 1] = True
        parts.append(b)
        left -= 1
    parts.append(np.zeros(4 * WORD, dtype=bool))
    if left >= WORD:
        parts.append(np.ones(WORD, dtype=bool))
        left -= WORD
    parts.append(np.zeros(2 * WORD, dtype=bool))
    if left:
        run = np.zeros(2 * left, dtype=bool)
        run[1::2] = True
        parts.append(run)
        parts.append(np.zeros(-(2 * left) % WORD, dtype=bool))   # up to the block's end
    parts.append(np.zeros(2 * WORD, dtype=bool))
    last = np.zeros(7, dtype=bool)
    last[6] = True
    parts.append(last)
    bits = np.concatenate(parts)
    assert int(bits.sum()) == K and bits[-1]
    return bits


def cut_pattern(length):
    """bool [length] for a SHORT image (the deepest lift, the deepest
    extraction): top-down, so the length is the caller's.  From 14 blocks on:
    blocks 0-1 empty, block 2 bit 0 alone, block 3 bit 31 alone, block 6 full,
    two empty blocks in the middle, odd positions elsewhere, two empty blocks
    before the last block, which holds position length - 1 alone.  Shorter:
    positions 0 and length - 1, bit 31 of block 0 and bit 0 of block 1 where
    they exist, and every third position."""
    assert length >= 1
    bits = np.zeros(length, dtype=bool)
    nb = (length + WORD - 1) // WORD
    if nb >= 14:
        mid = nb // 2
        for b in range(7, nb - 3):
            if b not in (mid, mid + 1):
                bits[b * WORD + 1:(b + 1) * WORD:2] = True
        bits[2 * WORD] = True
        bits[3 * WORD + WORD - 1] = True
        bits[6 * WORD:7 * WORD] = True
    else:
        bits[1::3] = True
        bits[0] = True
        if length > WORD:
            bits[WORD - 1] = bits[WORD] = True
    bits[length - 1] = True
    return bits


def gap_features(bits):
    """What the lift's select1 meets in a child column `bits` of a parent's
    image: a dict of booleans (see lift_fixture)."""
    bits = np.asarray(bits, dtype=bool)
    n = len(bits)
    nb = (n + WORD - 1) // WORD
    pad = np.zeros(nb * WORD, dtype=bool)
    pad[:n] = bits
    blocks = pad.reshape(nb, WORD)
    cnt = blocks.sum(axis=1)
    empty = cnt == 0
    pairs = np.flatnonzero(empty[:-1] & empty[1:]) if nb > 1 else np.zeros(0, dtype=np.int64)
    nonempty = np.flatnonzero(~empty)
    first, last = (int(nonempty[0]), int(nonempty[-1])) if len(nonempty) else (0, 0)
    return {
        "empty_run_at_start": nb > 2 and bool(empty[0] and empty[1]),
        # two empty blocks with ones before and after them, beside the run that ends the column
        "empty_run_in_middle": bool(((pairs > first) & (pairs + 1 < last)).sum() >= 2),
        "empty_run_at_end": nb > 3 and bool(empty[nb - 2] and empty[nb - 3]),
        "one_at_bit_0": bool(blocks[:, 0].any()),
        "one_at_bit_31": bool(blocks[:, WORD - 1].any()),
        "full_block": bool((cnt == WORD).any()),
        "partial_last_block_ends_on_a_one": n % WORD != 0 and bool(bits[-1]),
        # the k-th one is the first one of its block, after an empty block: rank-before == k - 1 on a run of blocks
        "first_one_of_a_block_after_empty_blocks": bool((~empty[1:] & empty[:-1]).any()),
        "blocks": nb,
    }


ALL_GAP_FEATURES = ("empty_run_at_start", "empty_run_in_middle", "empty_run_at_end", "one_at_bit_0", "one_at_bit_31",
                    "full_block", "partial_last_block_ends_on_a_one", "first_one_of_a_block_after_empty_blocks")
FULL_FEATURES_FROM = 35   # gap_pattern(K) has every feature from K = 35 ones on (1 + 1 + 32 + the final one)


# ---- the patterns of a leaf parent's columns (positions in [0, L)) -------------------

def _pos(L, p):
    p = np.asarray(sorted(set(p)), dtype=np.int64)
    return p[(p >= 0) & (p < L)]


PATTERNS = {
    "empty": lambda L: _pos(L, []),
    "pos0": lambda L: _pos(L, [0]),
    "last": lambda L: _pos(L, [L - 1]),
    "mod31": lambda L: np.arange(WORD - 1, L, WORD, dtype=np.int64),
    "mod0": lambda L: np.arange(0, L, WORD, dtype=np.int64),
    "edge8192": lambda L: _pos(L, [GROUP - 1, GROUP]),
    "from8192": lambda L: np.arange(GROUP, L, 3, dtype=np.int64),   # the first workgroup counts zero
    "wg0wg2": lambda L: _pos(L, [5, GROUP - 1, 2 * GROUP, L - 1] if L > 2 * GROUP else []),   # none in workgroup 1
    "full": lambda L: np.arange(L, dtype=np.int64),
}
_MIDDLE = ("pos0", "mod31", "mod0", "empty", "last", "edge8192", "from8192", "wg0wg2")
_NEEDS = {"edge8192": GROUP, "from8192": GROUP + 1, "wg0wg2": 2 * GROUP + 1, "mod31": WORD}   # the least L with a position


def pattern_names(L):
    """The patterns that are not empty by accident at length L ('empty' is)."""
    return tuple(p for p in _MIDDLE if L >= _NEEDS.get(p, 1))


def pattern_parts(L, slots):
    """Lists of `slots` pattern names, one list per matrix: the last name (the
    parent's highest child slot: the top bit of its masks) is 'last' or
    'mod31' in turn; the others take pattern_names(L) in order, as many
    matrices as that needs.  With one slot every pattern gets its own matrix,
    'full' included (elsewhere the anchor column is the full one)."""
    names = list(pattern_names(L))
    if slots == 1:
        return [[p] for p in names + ["full"]]
    tops = ["last", "mod31" if L >= WORD else "last"]
    parts, free = [], slots - 1
    for i in range(0, max(len(names), 1), free):
        chunk = names[i:i + free]
        chunk += ["empty"] * (free - len(chunk))
        parts.append(chunk + [tops[len(parts) % 2]])
    return parts


# ---- the basic partitioner's tree -----------------------------------------------------

class BasicTree:
    """m columns under the basic partitioner of `arity` in BFS numbering:
    num_children, first_child, leaf_column (arrays, as the oracle's export),
    columns[u] (the columns below node u), parent[u], slot[u]."""

    def __init__(self, m, arity):
        level = [("leaf", c) for c in range(m)]
        while len(level) > 1:
            groups = [level[i:i + arity] for i in range(0, len(level), arity)]
            level = [g[0] if len(g) == 1 else ("node", g) for g in groups]
        order, at = [level[0]], 0
        self.parent, self.slot = [-1], [0]
        nc, fc = [], []
        while at < len(order):
            kind, body = order[at]
            if kind == "node":
                nc.append(len(body))
                fc.append(len(order))
                for s, ch in enumerate(body):
                    order.append(ch)
                    self.parent.append(at)
                    self.slot.append(s)
            else:
                nc.append(0)
                fc.append(0)
            at += 1
        self.m, self.arity = m, arity
        self.num_children = np.asarray(nc, dtype=np.int64)
        self.first_child = np.asarray(fc, dtype=np.int64)
        self.leaf_column = np.asarray([b if k == "leaf" else 0 for k, b in order], dtype=np.int64)

        def below(t):
            return [t[1]] if t[0] == "leaf" else [c for ch in t[1] for c in below(ch)]
        self.columns = [np.asarray(below(t), dtype=np.int64) for t in order]
        self.leaf_of = {int(self.leaf_column[u]): u for u in range(len(order)) if nc[u] == 0}

    def path(self, col):
        """[(node, child slot)] from the root down to the leaf's parent."""
        out, u = [], self.leaf_of[int(col)]
        while self.parent[u] >= 0:
            out.append((self.parent[u], self.slot[u]))
            u = self.parent[u]
        return out[::-1]

    def child(self, u, slot):
        return int(self.first_child[u]) + slot

    def internal_below(self, u):
        """The internal nodes of u's subtree (u first)."""
        out = [u]
        for v in out:
            out += [w for w in range(self.child(v, 0), self.child(v, 0) + int(self.num_children[v]))
                    if self.num_children[w]]
        return out


def node_reach(dense, tree):
    """bool [nodes, n]: the rows with any column of the node's subtree set."""
    return np.stack([dense[:, cols].any(axis=1) for cols in tree.columns])


def node_lengths(dense, tree):
    """The model's lengths: lengths[u] = rows that reach node u (the positions
    of u's image); vec_size[u] = the length of u's own index column = the
    lengths of its parent (the matrix's rows for the root)."""
    lengths = node_reach(dense, tree).sum(axis=1).astype(np.int64)
    vec_size = np.asarray([dense.shape[0] if p < 0 else lengths[p] for p in tree.parent], dtype=np.int64)
    return lengths, vec_size


# ---- the models of the packed images (csrc/image.cpp) --------------------------------

def pack_pairs(dense, tree, u):
    """Set (child, position) pairs of every 16-position block of a KIND_PACK node u."""
    reach = node_reach(dense, tree)
    rows = reach[u]
    kids = [tree.child(u, s) for s in range(int(tree.num_children[u]))]
    per_pos = reach[kids][:, rows].sum(axis=0)
    return np.add.reduceat(per_pos, np.arange(0, len(per_pos), PACK_SPAN)) if len(per_pos) else per_pos


def record_sizes(dense, tree, u, count_byte):
    """Bytes of the record of every position of node u: one mask per internal
    node of u's subtree that the position's row reaches (2 bytes for more than
    8 children), and with count_byte (KIND_PACKT) the label count."""
    reach = node_reach(dense, tree)
    rows = reach[u]
    size = np.full(int(rows.sum()), 1 if count_byte else 0, dtype=np.int64)
    for v in tree.internal_below(u):
        size += reach[v][rows] * (1 if tree.num_children[v] <= 8 else 2)
    return size


def record_span(sizes, any_span):
    """(S, spilled blocks) of upload_record_blocks: the largest span -- 8, 4, 2,
    1 positions per block, or (any_span: KIND_PACKT) 8, 7, ..., 1 -- at which at
    most one block in 20 holds more than 64 - S record bytes."""
    sizes = np.asarray(sizes, dtype=np.int64)
    assert len(sizes) and int(sizes.max()) <= RECORD_BLOCK
    for S in (range(8, 0, -1) if any_span else (8, 4, 2, 1)):
        per = np.add.reduceat(sizes, np.arange(0, len(sizes), S))
        spilled = np.flatnonzero(per > RECORD_BLOCK - S)
        if len(spilled) * 20 <= len(per):
            return S, spilled
    return 0, None


# ---- the leaf-parent fixture ------------------------------------------------------------

class LeafParent:
    """dense [n, m]; R: the L rows of the parent (ascending); patterns: column
    -> pattern name (the anchor and the always-set columns are 'full')."""

    def __init__(self, dense, R, patterns):
        self.dense, self.R, self.L, self.patterns = dense, R, len(R), patterns
        self.n, self.m = dense.shape

    def positions(self, col):
        return PATTERNS[self.patterns[col]](self.L)


def leaf_parent(L, m, lo, hi, patterns, anchor=None, always=(), extra=(), outside=None):
    """The matrix around the leaf parent whose columns are [lo, hi): `anchor`
    (column lo unless given) is set on all of R, `patterns` maps more of its columns to
    pattern names, `always` lists columns set on all of R, `extra` pairs
    (column, positions) set besides.  Every such column lies in [lo, hi) and
    only rows of R touch them.  outside = (column, 'nest'): R is cut out of a
    larger set R0 by gap_pattern and the column holds R0 - R; (column,
    'rest'): the column holds every row outside R (no empty row: a root that
    folds).  Without `outside`, R = the ones of gap_pattern(L)."""
    p1 = gap_pattern(L)
    if outside is not None and outside[1] == "nest":
        p0 = gap_pattern(len(p1))
        R0 = np.flatnonzero(p0)
        R, n = R0[p1], len(p0)
        out_rows = R0[~p1]
    else:
        R, n = np.flatnonzero(p1), len(p1)
        out_rows = np.flatnonzero(~p1)
    gaps = np.diff(np.concatenate([[-1], R, [n]])) - 1
    assert len(R) == L and (L == n or int(gaps.max()) >= 100), "R must leave a gap of 100 rows"
    dense = np.zeros((n, m), dtype=bool)
    named = {lo if anchor is None else anchor: "full"}
    for c in always:
        named[c] = "full"
    for c, p in patterns.items():
        assert c not in named
        named[c] = p
    for c, p in named.items():
        assert lo <= c < hi
        dense[R[PATTERNS[p](L)], c] = True
    for c, pos in extra:
        assert lo <= c < hi and c not in named
        dense[R[np.asarray(pos, dtype=np.int64)], c] = True
    if outside is not None:
        assert not lo <= outside[0] < hi
        dense[out_rows, outside[0]] = True
    touched = dense[:, lo:hi].any(axis=1)
    assert np.array_equal(np.flatnonzero(touched), R)
    return LeafParent(dense, R, named)


def mask_fixture(m, L, part):
    """Every column a child of the root (arity >= m): the root is the leaf
    parent, a MASK node of m leaves; part: an index into pattern_parts(L, m - 1)."""
    names = pattern_parts(L, m - 1)[part]
    return leaf_parent(L, m, 0, m, {c + 1: p for c, p in enumerate(names)})


def plane_fixture(L, part):
    """9 columns, arity 8: the root holds the node of columns 0..7 and the
    LEAF of column 8 -- a PLANE image with a leaf child at slot 1.  Column 0
    anchors the root's L rows, column 8 carries one pattern per matrix."""
    (name,) = pattern_parts(L, 1)[part]
    f = leaf_parent(L, 9, 0, 9, {8: name})
    return f


def wide_plane_fixture(L, part=0):
    """144 columns, arity 16: the root is a PLANE of nine MASK16 children.  The
    last child (slot 8: columns 128..143) is the leaf parent of L rows, nested
    in the root's rows, which column 0 extends."""
    names = pattern_parts(L, 15)[part]
    return leaf_parent(L, 144, 128, 144, {129 + c: p for c, p in enumerate(names)}, outside=(0, "nest"))


# PACK: 64 columns, arity 8 -- the root holds eight MASK8-shaped children.  The
# children 0, 1 and 7 are set at every position (columns 1, 8 = the anchor, 62),
# so every full block holds exactly 16 * 3 = 48 pairs and the patterns on the
# columns 0, 7, 56, 63 (first / last child, first / last leaf slot) only toggle
# leaf bits inside children that are set anyway.
PACK_PATTERN_COLUMNS = (0, 7, 56, 63)
PACK_SPILL_BLOCK = 3   # from 20 blocks on: this block holds 49 pairs, its neighbours 48


def _four(L, part):
    return dict(zip(PACK_PATTERN_COLUMNS, pattern_parts(L, 4)[part]))


def pack_fixture(L, part):
    extra = [(16, [PACK_SPILL_BLOCK * PACK_SPAN + 2])] if L >= 20 * PACK_SPAN else []
    return leaf_parent(L, 64, 0, 64, _four(L, part), anchor=8, always=(1, 62), extra=extra)


# PACK2 / PACKT over the 8 x 8 x 8 tree (512 columns, arity 8): the record of a
# position holds one mask per internal node reached, so its size is fixed by
# the ALWAYS-set columns (one per leaf parent to reach), and the patterns on
# the columns 0, 7, 504, 511 toggle leaf bits of the leaf parents (A0, B0) and
# (A7, B7), which columns 1 and 510 keep set.
def _b(A, B, leaf=1):
    return 64 * A + 8 * B + leaf


DEEP_PATTERN_COLUMNS = (0, 7, 504, 511)
DEEP_ALWAYS = {
    # name -> always-set columns besides the anchor, column 1 = (A0, B0, leaf 1); record bytes = 1 + A's + B's (+ 1 for PACKT)
    "sparse": (_b(7, 7, 6),),                                                         # 2 A, 2 B: 5 (PACKT 6)
    "dense": tuple(_b(0, B) for B in range(1, 6)) + tuple(_b(7, B, 6) for B in range(2, 8)),   # 2 A, 12 B: 15
    "span3": tuple(_b(0, B) for B in range(1, 5)) + tuple(_b(3, B) for B in range(5)) +
             tuple(_b(7, B, 6) for B in range(3, 8)),                                 # 3 A, 15 B: 19 (PACKT 20)
}
DEEP_SPILL = {
    # name -> (positions, columns set there besides): one block past its inline bytes, from 20 blocks on
    "sparse": (range(16, 24), tuple(_b(0, B) for B in range(1, 4))),   # S = 8: 8 records of 8 bytes = 64 > 56
    "dense": ([13], (_b(0, 6),)),                                     # S = 4: 15 + 15 + 16 + 15 = 61 > 60
    "span3": ([10], tuple(_b(3, B) for B in range(5, 8))),            # S = 3 (PACKT): 20 + 23 + 20 = 63 > 61
}


def deep_fixture(kind, L, part, filler=False):
    """512 columns (with filler: 513; the last one is a leaf child of the
    root, set on every row outside R, so that the root folds)."""
    m = 513 if filler else 512
    pats = dict(zip(DEEP_PATTERN_COLUMNS, pattern_parts(L, 4)[part]))
    pos, cols = DEEP_SPILL[kind]
    extra = [(c, list(pos)) for c in cols] if L >= 20 * 8 else []
    return leaf_parent(L, m, 0, 512, pats, anchor=1, always=DEEP_ALWAYS[kind], extra=extra,
                       outside=(512, "rest") if filler else None)


# PACKT over 65 columns, arity 8: the root holds the node U of columns 0..63
# (eight leaf parents of eight leaves) and the leaf of column 64, the filler.
# A record = count + U's mask + one mask per leaf parent reached.
SMALL_ALWAYS = {"s8": (24, 62), "s7": (9, 17, 24, 33, 62), "s5": (9, 17, 24, 33, 41, 49, 62)}   # 3 / 6 / 8 parents
SMALL_SPILL = ((range(16, 24)), (9, 17, 33))   # s8: 8 records of 8 bytes = 64 > 56


def small_packt_fixture(kind, L, part):
    pats = dict(zip(PACK_PATTERN_COLUMNS, pattern_parts(L, 4)[part]))
    extra = [(c, list(SMALL_SPILL[0])) for c in SMALL_SPILL[1]] if kind == "s8" and L >= 20 * 8 else []
    return leaf_parent(L, 65, 0, 64, pats, anchor=1, always=SMALL_ALWAYS[kind], extra=extra, outside=(64, "rest"))


def wide_packt_fixture(L, part=0):
    """145 columns, arity 16: the folded root holds nine leaf parents of 16
    leaves (two mask bytes each: PACKT records of 3 bytes) and the leaf of
    column 144, the filler.  The parent of L rows is the ninth (slot 8)."""
    names = pattern_parts(L, 15)[part]
    return leaf_parent(L, 145, 128, 144, {129 + c: p for c, p in enumerate(names)}, outside=(144, "rest"))


# ---- the lift fixture ---------------------------------------------------------------------

class Lift:
    pass


def lift_fixture(T, mirror=False):
    """16 columns, arity 2.  On the path root > A > B > C > leaf of column 0:
    the root's rows R0 are gap_pattern's ones among the n rows, A's rows R1
    among R0 and B's rows R2 among R1 likewise (R2 has exactly T rows: the
    length of the deepest image a lift searches); C's rows R3 among R2 and the
    leaf's rows R4 among R3 are cut_pattern's.  Column 0 = R4, column 1 =
    R3 - R4, column 2 = R2 - R3, column 4 = R1 - R2, column 8 = R0 - R1.
    mirror: column j becomes column 15 - j (every slot of the path 1, not 0)."""
    p3 = cut_pattern(T)
    p4 = cut_pattern(int(p3.sum()))
    p2 = gap_pattern(T)
    p1 = gap_pattern(len(p2))
    p0 = gap_pattern(len(p1))
    R0 = np.flatnonzero(p0)
    R1 = R0[p1]
    R2 = R1[p2]
    R3 = R2[p3]
    R4 = R3[p4]
    f = Lift()
    f.sets, f.cuts = (R0, R1, R2, R3, R4), (p0, p1, p2, p3, p4)
    f.n, f.m, f.T = len(p0), 16, T
    dense = np.zeros((f.n, 16), dtype=bool)
    for col, rows, without in ((0, R4, None), (1, R3, R4), (2, R2, R3), (4, R1, R2), (8, R0, R1)):
        dense[rows, col] = True
        if without is not None:
            dense[without, col] = False
    f.dense = dense[:, ::-1].copy() if mirror else dense
    f.column = 15 if mirror else 0
    return f


LIFT_DEEPEST = (31, 64, 65, 8200)   # one block, two, three, more than a workgroup's 8192 positions


# ---- row shards -----------------------------------------------------------------------------

SHARD_ROWS = 64
SHARD_COLUMNS = {"boundary": 0, "not_in_shard_0": 1, "not_in_a_middle_shard": 2, "first_shard_only": 3,
                 "first_three_shards": 4, "every_shard": 5, "empty": 6, "full": 7}


def shard_matrix(n):
    """bool [n, 8] for shards of 64 rows (n of more than four shards): column 0
    has the rows 63, 64 and n - 1; column 1 nothing in shard 0; column 2
    nothing in shard 2; column 3 rows of shard 0 only; column 4 of the shards
    0..2 only; column 5 three rows in every shard (first, middle, last of it);
    column 6 is empty; column 7 full."""
    assert n > 4 * SHARD_ROWS
    d = np.zeros((n, 8), dtype=bool)
    r = np.arange(n)
    d[[63, 64, n - 1], 0] = True
    d[:, 1] = (r >= SHARD_ROWS) & ((r % 5 == 0) | (r == n - 1))
    d[:, 2] = (r // SHARD_ROWS != 2) & ((r % 7 == 3) | (r == n - 1))
    d[:, 3] = (r < SHARD_ROWS) & (r % 9 == 1)
    d[:, 4] = (r < 3 * SHARD_ROWS) & (r % 11 == 2)
    for k in range((n + SHARD_ROWS - 1) // SHARD_ROWS):
        lo, hi = k * SHARD_ROWS, min(n, (k + 1) * SHARD_ROWS)
        d[[lo, (lo + hi) // 2, hi - 1], 5] = True
    d[:, 7] = True
    return d


# ---- the leaf-parent configurations (tests/test_column_shapes.py checks them on the CPU,
# tests/test_gpu_column_edges.py runs them) ----------------------------------------------------

KINDS_OFF, KINDS_PACK, KINDS_PACK2, KINDS_ALL = 0, 2, 6, 15   # MBRWT_BUILD_NODE_KINDS


class Config:
    """One leaf-parent configuration: the matrix build(L, part) over the basic
    tree (m, arity) under the build option node_kinds; `node` = the BFS node
    whose image get_column extracts from (device node `node` + 1), of `kind`
    and `length` L; slots: the pattern columns of one matrix; packed: None,
    'pack', 'pack2' or 'packt' (then S, the span the fixture aims at)."""

    def __init__(self, m, arity, node_kinds, kind, node, slots, lengths, build, packed=None, S=0):
        self.m, self.arity, self.node_kinds, self.kind, self.node = m, arity, node_kinds, kind, node
        self.slots, self.lengths, self.build, self.packed, self.S = slots, lengths, build, packed, S

    def parts(self, L):
        return len(pattern_parts(L, self.slots))

    def tree(self):
        return BasicTree(self.m, self.arity)

    def stride(self, f):
        """The stride the built node must report (mbrwt_node_info) for fixture f."""
        t = self.tree()
        if self.kind == "PLANE":
            s = 16
            while s < 8 * int(t.num_children[self.node]):
                s *= 2
            return s
        if self.packed == "pack":
            return 64
        if self.packed in ("pack2", "packt"):
            return record_span(record_sizes(f.dense, t, self.node, self.packed == "packt"), self.packed == "packt")[0]
        return 0


def _mask(m, arity, kind):
    return Config(m, arity, KINDS_OFF, kind, 0, m - 1, MASK_LENGTHS, lambda L, part: mask_fixture(m, L, part))


CONFIGS = {
    "mask8": _mask(8, 8, "MASK8"),
    "mask16": _mask(16, 16, "MASK16"),
    "mask32": _mask(32, 32, "MASK32"),
    "mask64-bit32": _mask(33, 64, "MASK64"),
    "mask64-bit63": _mask(64, 64, "MASK64"),
    "plane": Config(9, 8, KINDS_OFF, "PLANE", 0, 1, MASK_LENGTHS, plane_fixture),
    "plane-wide": Config(144, 16, KINDS_OFF, "MASK16", 9, 15, (70, 8193), wide_plane_fixture),
    "pack": Config(64, 8, KINDS_PACK, "PACK", 0, 4, PACK_LENGTHS, pack_fixture, "pack"),
    "pack2-sparse": Config(512, 8, KINDS_PACK2, "PACK2", 0, 4, span_lengths(8),
                           lambda L, part: deep_fixture("sparse", L, part), "pack2", 8),
    "pack2-dense": Config(512, 8, KINDS_PACK2, "PACK2", 0, 4, span_lengths(4),
                          lambda L, part: deep_fixture("dense", L, part), "pack2", 4),
    "packt-s8": Config(65, 8, KINDS_ALL, "PACKT", 1, 4, span_lengths(8),
                       lambda L, part: small_packt_fixture("s8", L, part), "packt", 8),
    "packt-s7": Config(65, 8, KINDS_ALL, "PACKT", 1, 4, span_lengths(7),
                       lambda L, part: small_packt_fixture("s7", L, part), "packt", 7),
    "packt-s5": Config(65, 8, KINDS_ALL, "PACKT", 1, 4, span_lengths(5),
                       lambda L, part: small_packt_fixture("s5", L, part), "packt", 5),
    "packt-s3-deep": Config(513, 8, KINDS_ALL, "PACKT", 1, 4, span_lengths(3),
                            lambda L, part: deep_fixture("span3", L, part, filler=True), "packt", 3),
    "packt-wide": Config(145, 16, KINDS_ALL, "PACKT", 9, 15, (1, 7, 8, 9, 33, 8193), wide_packt_fixture, "packt", 8),
}
