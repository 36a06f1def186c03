"""Deterministic edge-column fixture of the device builder's tests (plain
numpy: no GPU import, no oracle import).

edge_columns(n, m): structured columns whose arity-2 parents are all-ones
words, all-zero columns (children of index length 0), single bits in the
first and last row, bits either side of every word boundary, long index
columns with full 64-bit payloads that straddle two words.

planted_pairs(n, m, law): columns paired by a law, each pair sharing a private
block of rows and nothing else, so the greedy partitioner's matching is known
in closed form: leaf_pairs() of the built tree holds every planted pair.

bottom_up(dense, arity): the closed form of BRWTBottomUpBuilder::build
(BRWT_builders.cpp:119-163) with the basic partitioner, as a BFS tree dict
with the keys of BRWTDevice.export() / OracleTree.export().
"""
import numpy as np

# ---- edge columns ----------------------------------------------------------

# column laws over the row ids r of n rows; consecutive laws are the arity-2 groups
_BASE = (
    lambda r, n: r < 0, lambda r, n: r < 0, lambda r, n: r < 0, lambda r, n: r < 0,   # zero parent + grandparent
    lambda r, n: r % 2 == 0, lambda r, n: r % 2 == 1,                                 # parent: all ones
    lambda r, n: r >= 0, lambda r, n: r == 0,
    lambda r, n: r == n - 1, lambda r, n: r >= n - 2,
    lambda r, n: r % 64 == 63, lambda r, n: r % 64 == 0,
    lambda r, n: (r >= 62) & (r <= 66), lambda r, n: (r >= 127) & (r <= 129),
    lambda r, n: r < n // 2, lambda r, n: r >= n // 2,
    lambda r, n: r < 64 * (n // 128), lambda r, n: _rand(n, 17, 0.02),                # full words, then nothing
    lambda r, n: _rand(n, 18, 0.5), lambda r, n: _rand(n, 19, 0.5),
    lambda r, n: _rand(n, 20, 0.1), lambda r, n: _rand(n, 20, 0.1),                   # identical
    lambda r, n: _rand(n, 22, 0.97), lambda r, n: _rand(n, 23, 0.97),                 # long index columns
)
BASE_COLUMNS = len(_BASE)
ZERO_COLUMNS = (0, 1, 2, 3)     # of every cycle
ONES_PARENT = (4, 5)            # of every cycle: their OR is every row
CYCLE_ROTATION = 3              # rows the k-th cycle is rotated by, times k


def _rand(n, seed, p):
    return np.random.default_rng(seed).random(n) < p


def edge_columns(n, m):
    """bool [n, m]: column j follows law j % BASE_COLUMNS, rotated down by
    CYCLE_ROTATION * (j // BASE_COLUMNS) rows (cyclically)."""
    r = np.arange(n, dtype=np.int64)
    dense = np.zeros((n, m), dtype=bool)
    for j in range(m):
        col = np.asarray(_BASE[j % BASE_COLUMNS](r, n), dtype=bool)
        dense[:, j] = np.roll(col, CYCLE_ROTATION * (j // BASE_COLUMNS))
    return dense


# ---- planted pairs -----------------------------------------------------------

def pairing(m, law):
    """The column pairs of `law` over m columns, in pair order."""
    if law == "mirror":      # partners in different 64-column tiles, every distance distinct
        return [(k, m - 1 - k) for k in range(m // 2)]
    if law == "skip3":       # partners inside one tile, distance 3
        return [(6 * g + i, 6 * g + i + 3) for g in range(m // 6) for i in range(3)]
    raise ValueError(law)


def pair_rows(n, p, s):
    """The private block of pair p: even pairs from the front, odd pairs from
    the back (pair 1 owns the last s rows, pair 3 the s before them)."""
    if p % 2 == 0:
        return np.arange((p // 2) * s, (p // 2 + 1) * s)
    return np.arange(n - (p // 2 + 1) * s, n - (p // 2) * s)


def planted_pairs(n, m, law, s=16):
    """(bool [n, m], pairs): both columns of pair p hold pair_rows(n, p, s) and
    nothing else; a column in no pair is empty."""
    pairs = pairing(m, law)
    assert len(pairs) * s <= n, "the private blocks overlap"
    dense = np.zeros((n, m), dtype=bool)
    for p, (a, b) in enumerate(pairs):
        rows = pair_rows(n, p, s)
        dense[rows, a] = True
        dense[rows, b] = True
    return dense, pairs


# ---- packed words ------------------------------------------------------------

def pack(dense):
    """bool [n, m] -> uint64 [m, ceil(n / 64)], LSB first, zero tails."""
    dense = np.asarray(dense, dtype=bool)
    n, m = dense.shape
    W = (n + 63) // 64
    bits = np.zeros((m, W * 64), dtype=bool)
    bits[:, :n] = dense.T
    return np.packbits(bits.reshape(m, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(m, W).copy()


def with_tail_garbage(words, n):
    """A copy of the packed columns with every bit past n set in the last word."""
    out = np.array(words, dtype=np.uint64, copy=True)
    if n % 64:
        out[:, -1] |= ~np.uint64((1 << (n % 64)) - 1)
    return out


def scattered(n, m, bits_per_column, seed):
    """uint64 [m, ceil(n / 64)]: bits_per_column random rows set in every
    column (repeats allowed), packed without a dense matrix."""
    rng = np.random.default_rng(seed)
    W = (n + 63) // 64
    words = np.zeros((m, W), dtype=np.uint64)
    r = rng.integers(0, n, (m, bits_per_column))
    c = np.repeat(np.arange(m), bits_per_column).reshape(m, bits_per_column)
    np.bitwise_or.at(words, (c, r // 64), np.uint64(1) << (r % 64).astype(np.uint64))
    return words


# ---- the bottom-up builder in closed form --------------------------------------

def _words_of(bits):
    W = (len(bits) + 63) // 64
    pad = np.zeros(W * 64, dtype=bool)
    pad[: len(bits)] = bits
    return np.packbits(pad, bitorder="little").view(np.uint64).copy() if W else np.zeros(0, dtype=np.uint64)


def bottom_up(dense, arity):
    """BRWTBottomUpBuilder::build with the basic partitioner: consecutive
    groups of `arity` nodes per level, a group of one passes through, parent =
    OR of its children, a child's index = its bits at the parent's set rows,
    the root's index = its row column.  BFS tree dict (keys of export())."""
    dense = np.asarray(dense, dtype=bool)
    n, m = dense.shape
    nodes = [dict(children=[], column=j, rows=dense[:, j]) for j in range(m)]
    level = list(range(m))
    while len(level) > 1:
        nxt = []
        for g0 in range(0, len(level), arity):
            grp = level[g0:g0 + arity]
            if len(grp) == 1:
                nxt.append(grp[0])
                continue
            rows = np.logical_or.reduce([nodes[c]["rows"] for c in grp])
            for c in grp:
                nodes[c]["index"] = nodes[c]["rows"][rows]
            nxt.append(len(nodes))
            nodes.append(dict(children=grp, column=0xFFFFFFFF, rows=rows))
        level = nxt
    order = list(level)
    if order:
        nodes[order[0]]["index"] = nodes[order[0]]["rows"]
    for u in order:
        order.extend(nodes[u]["children"])
    bfs = {u: i for i, u in enumerate(order)}
    bn = [nodes[u] for u in order]
    return dict(num_nodes=len(bn), num_rows=n if m else 0, num_columns=m,
                num_children=np.array([len(b["children"]) for b in bn], dtype=np.uint32),
                first_child=np.array([bfs[b["children"][0]] if b["children"] else 0 for b in bn], dtype=np.uint32),
                leaf_column=np.array([b["column"] for b in bn], dtype=np.uint32),
                vec_size=np.array([len(b["index"]) for b in bn], dtype=np.uint64),
                words=[_words_of(b["index"]) for b in bn])


# ---- tree comparisons ------------------------------------------------------------

def same_tree(a, b):
    """Two BFS tree dicts are the same tree: shape, index lengths and every
    node's index words, unmasked (the words serialize() writes; the
    reference's files have zero tails)."""
    for k in ("num_children", "first_child", "leaf_column", "vec_size"):
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
    assert len(a["words"]) == len(b["words"]) == len(a["num_children"])
    for u, (wa, wb) in enumerate(zip(a["words"], b["words"])):
        np.testing.assert_array_equal(np.asarray(wa, dtype=np.uint64), np.asarray(wb, dtype=np.uint64),
                                      err_msg=f"index words of node {u}")


def leaf_pairs(tree):
    """The sorted leaf-column tuples under the nodes whose children are all leaves."""
    nc = np.asarray(tree["num_children"]).astype(np.int64)
    fc = np.asarray(tree["first_child"]).astype(np.int64)
    lc = np.asarray(tree["leaf_column"]).astype(np.int64)
    out = set()
    for u in np.nonzero(nc)[0]:
        kids = np.arange(fc[u], fc[u] + nc[u])
        if (nc[kids] == 0).all():
            out.add(tuple(sorted(lc[kids].tolist())))
    return out


# ---- the launch geometry of the level kernels (csrc/build.hip grid_of) -----------

GRID_STRIDE_CASE = dict(n=393_281, m=8192, bits_per_column=300)


def grid_of(n, ys=1):
    cap = max(1, 65536 // max(1, ys))
    return max(1, min((n + 255) // 256, cap))


def level_strides(W, groups, children):
    """Grid-stride iterations of k_or (one grid row per group) and k_pext (one
    per child) over W words: (ceil(W / threads of a grid row)) of each."""
    out = []
    for ys in (groups, children):
        threads = 256 * grid_of(W, min(65535, ys))
        out.append(-(-W // threads))
    return tuple(out)
