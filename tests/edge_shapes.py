"""Deterministic edge-shape fixture of the row-record and classify tests
(plain numpy: no GPU import, no oracle import).

The STAIRCASE matrix over m columns: row k <= m has columns [0, k) set, so
its rows carry every label count 0..m and every record size the tree can
produce -- every inline / spill / long boundary of every block shape lies on
some row without the test knowing where.  `pad` more rows follow: empty
(they lower the mean labels per row, which moves the tile capacity C down),
or, with repeat=True, rows 0..m again, cyclically (repeated records: the
record classes), or, with single=True, rows of one label (pad row i carries
column i % m: sparse rows, where terminal records are the smaller code).  The
closed form of any row id is staircase_count().

The batch builders return row ids of a staircase whose row 0 is empty and
whose row k <= m has k labels; they place rows of chosen label counts on
chosen lanes of the 64-row tiles get_rows works in -- or, for the node-image
kernels, of their 16-row rowblocks, 8-row chunks and 256-row tiles
(tile_totals(tile=...), node_geometry).  windows() is a low staircase placed
anywhere in the width (rows of few labels over a deep or a wide tree).
"""
import numpy as np

TILE = 64
# tile totals around 512 (k_compact_tiles' register copy) and around every
# tile capacity C the build may choose (1024, 2048, 4096; C in 1024..4096)
TILE_TOTAL_WINDOWS = ((500, 520), (1015, 1035), (2040, 2056), (4088, 4104))
GEOMETRY_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
GEOMETRY_HEAVY = (254, 255, 256)   # and m: geometry_heavy(m)
COPIES_LABELS = (16, 17, 63, 64, 65)   # 64 k straddles C = 1024 and C = 4096


def staircase(m, pad=0, repeat=False, single=False):
    """bool [m + 1 + pad, m]: row k <= m has columns [0, k); the pad rows
    are empty, or (repeat) row m + 1 + i is row i % (m + 1), or (single) row
    m + 1 + i has column i % m alone."""
    k = staircase_count(np.arange(m + 1 + pad), m, repeat)
    dense = np.arange(m)[None, :] < k[:, None]
    if single:
        assert not repeat
        dense[m + 1 + np.arange(pad), np.arange(pad) % m] = True
    return dense


def staircase_count(rows, m, repeat=False, single=False):
    """Labels of the staircase's rows `rows` (closed form)."""
    rows = np.asarray(rows, dtype=np.int64)
    if repeat:
        return rows % (m + 1)
    return np.where(rows <= m, rows, 1 if single else 0)


def sweep_rows(m):
    """Every row 0..m once in order, then the same reversed."""
    up = np.arange(m + 1, dtype=np.uint64)
    return np.concatenate([up, up[::-1]])


_LANE_PAIRS = ((0, 63), (0, 1), (31, 32))


def lane_pairs(tile):
    """The lanes of tile_totals' two heavy rows: first and last, the first
    two, the two around the middle -- (0, 63), (0, 1), (31, 32) at 64;
    (0, 15), (0, 1), (7, 8) at 16; (0, 7), (0, 1), (3, 4) at 8."""
    return ((0, tile - 1), (0, 1), (tile // 2 - 1, tile // 2))


def tile_totals(m, lo, hi, tile=TILE, lanes=None):
    """One `tile`-row tile per total T in [lo, hi]: rows a and T - a on the
    lanes of `lanes` (lane_pairs(tile) by default; cycled with T), tile - 2
    copies of row 0 around them; a cycles through 1, T // 2 and the largest
    row that fits.  Where two rows of at most m labels cannot reach T
    (T > 2 m), full rows (m labels) take the next free lanes until the rest
    fits two rows; totals beyond tile * m (a tile of full rows) are left out.
    The node kernels work in 16-row rowblocks, 8-row chunks and 256-row
    tiles, the row records in 64-row tiles (the default)."""
    lanes = lane_pairs(tile) if lanes is None else lanes
    tiles = []
    for i, T in enumerate(range(lo, min(hi, tile * m) + 1)):
        t = np.zeros(tile, dtype=np.uint64)
        p0, p1 = lanes[i % len(lanes)]
        free = [l for l in range(tile) if l not in (p0, p1)]
        rest = T
        while rest > 2 * m:
            t[free.pop(0)] = m
            rest -= m
        a = (1, rest // 2, min(m, rest))[(i // 3) % 3]
        a = min(max(a, rest - m, 0), min(m, rest))
        t[p0], t[p1] = a, rest - a
        assert int(t.sum()) == T and int(t.max()) <= m
        tiles.append(t)
    return np.concatenate(tiles) if tiles else np.zeros(0, dtype=np.uint64)


def geometry_heavy(m):
    return tuple(k for k in GEOMETRY_HEAVY if k <= m) + (m,)


def geometry(m, k):
    """Batches of n in GEOMETRY_SIZES rows around the heavy row k: (name,
    rows) with the heavy row first and last among light rows (0..7 labels),
    and alone in the middle of empty rows.  At n = 65, 257, 1025 the last
    tile is partial; 'last' then has the heavy row on its last lane."""
    out = []
    for n in GEOMETRY_SIZES:
        light = (np.arange(n) % 8).astype(np.uint64)
        first, last, alone = light.copy(), light.copy(), np.zeros(n, dtype=np.uint64)
        first[0] = k
        last[n - 1] = k
        alone[n // 2] = k
        out += [(f"first-{n}", first), (f"last-{n}", last), (f"alone-{n}", alone)]
    return out


def copies(m):
    """64 and 65 copies of one row of k labels, k in COPIES_LABELS."""
    return [(f"{c}x{k}", np.full(c, k, dtype=np.uint64)) for k in COPIES_LABELS if k <= m for c in (64, 65)]


def gather_csr(off, cols, rows):
    """The CSR of the batch `rows` out of the CSR of rows 0..n-1 (off, cols):
    one reference computed once serves every batch."""
    rows = np.asarray(rows, dtype=np.int64)
    off = np.asarray(off, dtype=np.int64)
    cnt = off[rows + 1] - off[rows]
    out_off = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum(cnt, out=out_off[1:])
    total = int(out_off[-1])
    start = np.repeat(off[rows] - out_off[:-1].astype(np.int64), cnt)
    return out_off, np.asarray(cols)[start + np.arange(total)]


def closed_form_ok(off, cols, counts, shifts=None):
    """diff(off) == counts and every row's labels, sorted, are range(count)
    -- or, with `shifts` (one per row), shift + range(count)."""
    off = np.asarray(off, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    if len(off) != len(counts) + 1 or off[0] != 0 or not np.array_equal(np.diff(off), counts):
        return False
    cols = np.asarray(cols, dtype=np.int64)
    if len(cols) != int(off[-1]):
        return False
    seg = np.repeat(np.arange(len(counts)), counts)
    order = np.lexsort((cols, seg))
    want = np.arange(int(off[-1])) - np.repeat(off[:-1], counts)
    if shifts is not None:
        want = want + np.repeat(np.asarray(shifts, dtype=np.int64), counts)
    return np.array_equal(cols[order], want)


# ---- the node-image fixtures (csrc/nodes_*.hip: 16-row rowblocks, 8-row chunks,
# 256-row tiles; tests/test_gpu_node_edges.py) ---------------------------------

def windows(m, top, shifts):
    """bool [len(shifts) * (top + 1), m], a LOW staircase: row i * (top + 1) + k
    has the columns [shifts[i], shifts[i] + k), k in 0..top.  Rows of at most
    `top` labels anywhere in the width: at shift 0, across a boundary between
    two children of the tree's root, up to the last column (shift m - top)."""
    shifts = np.asarray(shifts, dtype=np.int64)
    assert top >= 0 and (shifts >= 0).all() and (shifts + top <= m).all()
    ids = np.arange(len(shifts) * (top + 1))
    lo = windows_shift(ids, top, shifts)[:, None]
    c = np.arange(m)[None, :]
    return (c >= lo) & (c < lo + windows_count(ids, top)[:, None])


# (m, top, shifts) over a binary tree of 256 columns: the root's children
# split the width at column 128, which the rows of shift 112 straddle
WINDOWS_DEEP = (256, 32, (0, 112, 224))
WIDE_TOP = 140


def windows_wide(m):
    """(m, top, shifts) of the windows block of label_map_matrix(m)."""
    return m, WIDE_TOP, (0, m - WIDE_TOP)


def label_map_matrix(m):
    """About 300 rows over m >= 16,384 columns: windows(*windows_wide(m)),
    then one row each holding the columns 0, 16,383 and m - 1 alone, and one
    holding all of them."""
    w = windows(*windows_wide(m))
    extra = np.zeros((4, m), dtype=bool)
    for i, c in enumerate((0, 16383, m - 1)):
        extra[i, c] = extra[3, c] = True
    return np.concatenate([w, extra])


def windows_count(rows, top):
    """Labels of the rows `rows` of windows(m, top, shifts) (closed form)."""
    return np.asarray(rows, dtype=np.int64) % (top + 1)


def windows_shift(rows, top, shifts):
    """First column of the rows `rows` of windows(m, top, shifts)."""
    return np.asarray(shifts, dtype=np.int64)[np.asarray(rows, dtype=np.int64) // (top + 1)]


def windows_rows(counts, top, nshifts):
    """Row ids of windows(m, top, shifts) with the label counts `counts`
    (each <= top), the shift cycling with the position in the batch."""
    counts = np.asarray(counts, dtype=np.uint64)
    assert int(counts.max(initial=0)) <= top
    return (np.arange(len(counts), dtype=np.uint64) % np.uint64(nshifts)) * np.uint64(top + 1) + counts


# partial and full chunks (8), rowblocks (16), row-record tiles (64) and
# compaction tiles (256); 16 * 7 + 1 and 16 * 28 + 1: one rowblock more than
# the 7 (k_traverse_ptw) and 4 (k_traverse_p2w) waves of a workgroup take in
# one and in seven rounds
NODE_SIZES = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 16 * 7 + 1, 16 * 28 + 1)


def node_geometry(k, sizes=NODE_SIZES):
    """geometry() in the node kernels' units: batches of n in `sizes` rows
    around the heavy row k -- (name, rows) with the heavy row first and last
    among light rows (0..7 labels), and alone in the middle of empty rows."""
    out = []
    for n in sizes:
        light = (np.arange(n) % 8).astype(np.uint64)
        first, last, alone = light.copy(), light.copy(), np.zeros(n, dtype=np.uint64)
        first[0] = k
        last[n - 1] = k
        alone[n // 2] = k
        out += [(f"first-{n}", first), (f"last-{n}", last), (f"alone-{n}", alone)]
    return out
