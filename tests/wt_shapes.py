"""Deterministic fixture of the BinRel-WT edge tests (plain numpy: no GPU
import, no oracle import), after the pattern of tests/edge_shapes.py.

The engine (csrc/binrel_wt.hip) cuts the rows into chunks of 2^k rows, k the
largest value <= 24 with 2^k * num_columns < 2^31, every chunk a 4-ary
wavelet matrix of ceil(w / 2) digit levels; a level is a run of 64-byte rank
blocks of 208 positions (13 words of 16 digits, read in 16-byte quarters:
words 1, 5 and 9 start a new load) and one sentinel block.  The shapes here
are the smallest at which each of those paths exists; the sizes follow from
the chunk rule alone:

  chunk_per_row(m)      m >= 2^30: one row per chunk.  Row lengths LENGTHS
                        (word, quarter and block edges, one and two whole
                        blocks) under three id laws, empty rows between some,
                        the first and the last row empty.
  two_rows_per_chunk()  m = 2^30 - 1: 40 rows, lengths out of LENGTHS.
  k10()                 m = 2^20: 1,024 rows a chunk, 3 chunks and 5 rows.
  k17()                 m = 8,192: 131,072 rows a chunk, 2 chunks and 77 rows.
  empty_middle()        m = 2^20: three chunks, the middle one without a symbol.
  beyond_32_bits()      m = 2^32 + 10: 20 rows (ids are 32 bits wide: no row
                        can hold a column >= 2^32).

Every builder returns (offsets u64, cols u32) with each row's ids ascending.
The reference (ref_rows, ref_get, ref_column) is computed from that CSR alone.
"""
import numpy as np

from edge_shapes import gather_csr

BLOCK_POS = 208     # positions per rank block
BLOCK_BYTES = 64
TILE = 256          # rows per tile of k_wt_decode
HEAVY = 417         # two whole blocks and one position

LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 79, 80, 81, 143, 144, 145, 191, 192, 193, 207, 208, 209,
           415, 416, 417, 623, 624, 625)
LAWS = ("consecutive", "top-digits", "hash")
ALL_LOW_DIGITS_3 = 0x3FFFFFFF


# ---- the form of a built matrix ------------------------------------------------

def symbol_bits(m):
    """Bits of an id < m, 1..32 (ids are u32)."""
    w = 1
    while w < 32 and (1 << w) < m:
        w += 1
    return w


def levels(m):
    return (symbol_bits(m) + 1) // 2


def chunk_log2(m):
    """k: a chunk holds 2^k rows; the largest k <= 24 with 2^k * m < 2^31 (0 if none)."""
    k = 24
    while k > 0 and (1 << k) * max(int(m), 1) >= 1 << 31:
        k -= 1
    return k


def num_chunks(n, m):
    return ((n - 1) >> chunk_log2(m)) + 1 if n else 0


def chunk_lengths(off, m):
    """Symbols per chunk."""
    off = np.asarray(off, dtype=np.int64)
    n, k = len(off) - 1, chunk_log2(m)
    edges = np.minimum(np.arange(num_chunks(n, m) + 1, dtype=np.int64) << k, n)
    return np.diff(off[edges])


def expected_device_bytes(off, m):
    """(n + 1) offsets of 8 bytes and, per chunk, `levels` runs of
    ceil(len / 208) + 1 blocks of 64 bytes."""
    n = len(off) - 1
    blocks = (chunk_lengths(off, m) + BLOCK_POS - 1) // BLOCK_POS + 1
    return (n + 1) * 8 + int(blocks.sum()) * levels(m) * BLOCK_BYTES


# ---- CSR builders ----------------------------------------------------------------

def csr_of(rows):
    """CSR of a list of id arrays, every row sorted ascending."""
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    cols = np.concatenate([np.sort(np.asarray(r, dtype=np.int64)) for r in rows] + [np.zeros(0, np.int64)])
    return off, cols.astype(np.uint32)


def check_csr(off, cols, m):
    """offsets start at 0 and ascend; every row's ids ascend strictly and are < m."""
    off = np.asarray(off, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(cols)
    assert len(cols) == 0 or (0 <= int(cols.min()) and int(cols.max()) < m)
    inner = np.ones(len(cols), dtype=bool)
    inner[off[:-1][off[:-1] < len(cols)]] = False   # a row's first id has no predecessor
    assert (np.diff(cols)[inner[1:]] > 0).all()


def _hash_ids(count, m, salt):
    """`count` distinct ids < m in the order a multiplicative hash emits them."""
    i = np.arange(1, 2 * count + 64, dtype=np.uint64) + np.uint64(salt)
    h = ((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(11)) % np.uint64(m)
    _, first = np.unique(h, return_index=True)
    return h[np.sort(first)][:count].astype(np.int64)


def law_ids(law, length, m):
    """`length` distinct ids < m:
    consecutive  c .. c + length - 1 (they share all but the low digits; c ends
                 in ..F0, so a row of 17 ids carries into the third digit)
    top-digits   ids that differ only in the top two digits.  T such ids exist
                 (T = 8 at 31 bits, 16 at 30 and 32), so a longer row takes the
                 lower digits low0, low0 + 1, .. in turn, each under all T tops
    hash         a multiplicative-hash spread mod m with m - 1, 0, 0x3FFFFFFF,
                 1 and 0xFFFFFFFE (where < m) forced in, as many as fit
    The ids of a shorter row are a subset of a longer row's: a column is held
    by many rows, that is by many chunks."""
    m = int(m)
    if law == "consecutive":
        c = (m // 3) & ~0xFF | 0xF0
        return c + np.arange(length, dtype=np.int64)
    if law == "top-digits":
        sh = 2 * (levels(m) - 2)
        tops = ((m - 1) >> sh) + 1
        low0 = 0x0D5A5A5 & ((1 << (sh - 1)) - 1)   # < 2^(sh-1): every top stays below m
        t = np.arange(length, dtype=np.int64)
        ids = ((t % tops) << sh) + low0 + t // tops
        assert int(ids.max(initial=0)) < m
        return ids
    assert law == "hash"
    forced = [x for x in (m - 1, 0, ALL_LOW_DIGITS_3, 1, 0xFFFFFFFE) if 0 <= x < m]
    forced = list(dict.fromkeys(forced))[:length]
    spread = [int(x) for x in _hash_ids(length + len(forced), m, 7) if int(x) not in forced]
    return np.array(forced + spread[: length - len(forced)], dtype=np.int64)


def chunk_per_row(m):
    """LENGTHS under each law, an empty row after the rows of 17 and of 209
    ids and after each law's run: 90 rows, the first and the last empty."""
    assert chunk_log2(m) == 0
    rows = []
    for law in LAWS:
        for length in LENGTHS:
            rows.append(law_ids(law, length, m))
            if length in (17, 209):
                rows.append(np.zeros(0, np.int64))
        rows.append(np.zeros(0, np.int64))
    return csr_of(rows)


M_TWO_ROWS = (1 << 30) - 1


def two_rows_per_chunk():
    """40 rows over 2^30 - 1 columns: lengths LENGTHS[(7 i + 23) % 27] (row 0
    holds 417 ids), laws in turn."""
    m = M_TWO_ROWS
    assert chunk_log2(m) == 1
    return csr_of([law_ids(LAWS[i % 3], LENGTHS[(7 * i + 23) % len(LENGTHS)], m) for i in range(40)])


def _strata_rows(n, m, strata, keep, seed):
    """n rows: stratum j of `strata` equal parts of [0, m) gives one id with
    probability `keep`, never the stratum's last id (those stay absent)."""
    rng = np.random.default_rng(seed)
    width = m // strata
    ids = np.arange(strata, dtype=np.int64)[None, :] * width + rng.integers(0, width - 1, (n, strata))
    mask = rng.random((n, strata)) < keep
    return ids, mask


M_K10 = 1 << 20
K10_ROWS = 3 * 1024 + 5
K10_HEAVY_ROW = 1300
K10_EVERY_CHUNK = 777_777      # rows 5, 1023, 1024, 2047, 2048, 3072, 3076
K10_LAST_CHUNK_ONLY = 888_888  # rows 3073, 3076
K10_FIRST_CHUNK_ONLY = 99_999  # rows 0, 1023
K10_NAMED = {K10_EVERY_CHUNK: (5, 1023, 1024, 2047, 2048, 3072, 3076), K10_LAST_CHUNK_ONLY: (3073, 3076),
             K10_FIRST_CHUNK_ONLY: (0, 1023)}


def _rows_of_strata(ids, mask, reserved):
    rows = []
    for i in range(len(ids)):
        r = ids[i][mask[i]]
        rows.append(r[~np.isin(r, reserved)])
    return rows


def k10():
    """3,077 rows over 2^20 columns, about 3 ids a row; rows 1,022 and 1,025
    empty, the chunk edges 1,023 | 1,024 and 2,047 | 2,048 non-empty; row
    1,300 holds 417 ids; the columns of K10_NAMED on the rows listed there
    and nowhere else."""
    m, n = M_K10, K10_ROWS
    assert chunk_log2(m) == 10
    ids, mask = _strata_rows(n, m, 8, 3 / 8, 10)
    rows = _rows_of_strata(ids, mask, list(K10_NAMED))
    rows[1022] = rows[1025] = np.zeros(0, np.int64)
    rows[K10_HEAVY_ROW] = law_ids("hash", HEAVY, m)
    assert not np.isin(rows[K10_HEAVY_ROW], list(K10_NAMED)).any()
    for c, where in K10_NAMED.items():
        for r in where:
            rows[r] = np.append(rows[r], c)
    return csr_of(rows)


M_K17 = 8192
K17_ROWS = 2 * 131072 + 77


def k17():
    """262,221 rows over 8,192 columns, about 2 ids a row (one id of each of
    four strata with probability 1/2); ids 2,047, 4,095, 6,143 and 8,191 are
    held by no row."""
    m, n = M_K17, K17_ROWS
    assert chunk_log2(m) == 17
    ids, mask = _strata_rows(n, m, 4, 0.5, 17)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(mask.sum(axis=1), out=off[1:])
    return off, ids[mask].astype(np.uint32)


M_EMPTY_MIDDLE = 1 << 20
EMPTY_MIDDLE_ROWS = 2 * 1024 + 9
EMPTY_MIDDLE_BOTH = 424_242       # rows 3, 1000, 2048, 2056: chunks 0 and 2
EMPTY_MIDDLE_LAST_ONLY = 515_151  # rows 2050, 2051: chunk 2 alone
EMPTY_MIDDLE_NAMED = {EMPTY_MIDDLE_BOTH: (3, 1000, 2048, 2056), EMPTY_MIDDLE_LAST_ONLY: (2050, 2051)}


def empty_middle():
    """2,057 rows over 2^20 columns: rows 1,024..2,047 (chunk 1) are empty."""
    m, n = M_EMPTY_MIDDLE, EMPTY_MIDDLE_ROWS
    ids, mask = _strata_rows(n, m, 8, 3 / 8, 11)
    mask[1024:2048] = False
    rows = _rows_of_strata(ids, mask, list(EMPTY_MIDDLE_NAMED))
    rows[7] = np.zeros(0, np.int64)
    for c, where in EMPTY_MIDDLE_NAMED.items():
        for r in where:
            rows[r] = np.append(rows[r], c)
    return csr_of(rows)


M_BEYOND = (1 << 32) + 10


def beyond_32_bits():
    """20 rows over 2^32 + 10 columns; row 3 holds 5, row 4 holds 5 and
    0xFFFFFFFF, rows 0 and 19 are empty."""
    rows = [law_ids(LAWS[i % 3], (0, 3, 17, 64, 209)[i % 5], 1 << 32) for i in range(20)]
    rows[3] = np.array([5, 77, 1 << 31], dtype=np.int64)
    rows[4] = np.array([5, 0xFFFFFFFF], dtype=np.int64)
    rows[19] = np.zeros(0, np.int64)
    return csr_of(rows)


# ---- the reference: numpy over the CSR alone -----------------------------------------

def ref_rows(off, cols, rows):
    """get_rows: a row is its ascending ids."""
    return gather_csr(off, cols, rows)


def ref_get(off, cols, rows, qcols):
    """get: membership of qcols[i] in row rows[i]."""
    off = np.asarray(off, dtype=np.int64)
    owner = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    have = (owner << 33) | np.asarray(cols, dtype=np.int64)
    q = np.asarray(qcols, dtype=np.uint64)
    want = (np.asarray(rows, dtype=np.int64) << 33) | (q & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.isin(want, have) & (q <= np.uint64(0xFFFFFFFF))


def ref_column(off, cols, c):
    """get_column: the rows holding c, ascending."""
    if c > 0xFFFFFFFF:
        return np.zeros(0, dtype=np.uint64)
    hits = np.nonzero(np.asarray(cols) == np.uint32(c))[0]
    return (np.searchsorted(np.asarray(off, dtype=np.int64), hits, "right") - 1).astype(np.uint64)


class CsrDense:
    """What the classify references read of a dense bool matrix -- .shape
    and dense[row ids] -- served from the CSR (the matrix itself would be
    gigabytes)."""

    def __init__(self, off, cols, m):
        self.off, self.cols, self.shape = np.asarray(off, dtype=np.int64), np.asarray(cols), (len(off) - 1, m)

    def __getitem__(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        out = np.zeros((len(rows), self.shape[1]), dtype=bool)
        for i, r in enumerate(rows):
            out[i, self.cols[self.off[r]:self.off[r + 1]]] = True
        return out


# ---- queries -------------------------------------------------------------------------

def point_queries(off, cols, m):
    """(rows, cols, expected) of get: every non-empty row's first and last id,
    and one id the row does not hold per row -- of id - 1, id + 1 (around the
    row's first / last id), 0 and m - 1 in turn, the first that is absent."""
    off = np.asarray(off, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    n = len(off) - 1
    full = np.nonzero(np.diff(off) > 0)[0]
    first, last = cols[off[full]], cols[off[full + 1] - 1]
    r_abs, c_abs = [], []
    for r in range(n) if n <= 5000 else _sample_rows(n):
        row = cols[off[r]:off[r + 1]]
        cand = [0, m - 1] if not len(row) else [row[0] - 1, row[-1] + 1, 0, m - 1, row[0] + 1, row[-1] - 1]
        cand = cand[r % len(cand):] + cand[: r % len(cand)]
        for c in cand:
            if 0 <= c < m and c not in row:
                r_abs.append(r)
                c_abs.append(int(c))
                break
    qr = np.concatenate([full, full, np.array(r_abs, dtype=np.int64)]).astype(np.uint64)
    qc = np.concatenate([first, last, np.array(c_abs, dtype=np.int64)]).astype(np.uint64)
    want = np.concatenate([np.ones(2 * len(full), dtype=bool), np.zeros(len(r_abs), dtype=bool)])
    return qr, qc, want


def _sample_rows(n):
    """The rows around every 2^10 / 2^17 edge and every 97th row."""
    near = [e + d for k in (10, 17) for e in range(0, n + 1, 1 << k) for d in range(-3, 4)]
    return sorted({r for r in near if 0 <= r < n} | set(range(0, n, 97)))


def absent_columns(cols, m, count=4):
    """Columns < m that no row holds."""
    cand = [2, m - 2, 2047, 4095, 6143, 8191, ALL_LOW_DIGITS_3 - 1, (1 << 31) + 12345, m // 2 + 1, 0xFFFFFFFD]
    have = set(np.unique(cols).tolist())
    out = [c for c in dict.fromkeys(cand) if 0 <= c < m and c not in have][:count]
    assert len(out) >= 2
    return out


def heavy_row(off):
    """The first row of HEAVY ids, or the longest row."""
    lens = np.diff(np.asarray(off, dtype=np.int64))
    hit = np.nonzero(lens == HEAVY)[0]
    return int(hit[0]) if len(hit) else int(np.argmax(lens))


def batches(off):
    """(name, row ids) around the 256-row tile of k_wt_decode: n in 1, 255,
    256, 257, 513 with the heavy row first, last (at 257 and 513: last in a
    partial tile) and alone among empty rows; a tile of empty rows before a
    non-empty tile; 300 copies of the heavy row; the empty batch."""
    lens = np.diff(np.asarray(off, dtype=np.int64))
    n_rows = len(lens)
    heavy = heavy_row(off)
    empties = np.nonzero(lens == 0)[0]
    assert len(empties) and lens[heavy] > 0
    out = []
    step = n_rows // 7 + 1   # neighbours in a batch lie chunks apart
    for n in (1, 255, 256, 257, 513):
        light = (np.arange(n, dtype=np.int64) * step + 1) % n_rows
        light[n // 3] = n_rows - 1   # (the last chunk may be a few rows)
        first, last, alone = light.copy(), light.copy(), empties[np.arange(n) % len(empties)]
        first[0] = heavy
        last[n - 1] = heavy
        alone[n // 2] = heavy
        out += [(f"first-{n}", first), (f"last-{n}", last), (f"alone-{n}", alone)]
    zero_tile = np.concatenate([empties[np.arange(TILE) % len(empties)], [heavy], (np.arange(40) * step) % n_rows])
    out.append(("empty tile, then a non-empty one", zero_tile))
    out.append(("300 copies", np.full(300, heavy)))
    out.append(("empty batch", np.zeros(0, np.int64)))
    return [(name, np.asarray(rows, dtype=np.uint64)) for name, rows in out]
