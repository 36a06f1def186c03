"""Deterministic fixture of the wire edge tests (plain numpy: no GPU import,
nothing from oracle or dist), after the pattern of tests/edge_shapes.py and
tests/wt_shapes.py.

The wire (include/mbrwt.h mbrwt_pack_csr_device; csrc/packids.hip) is built
here a second time from the header's rules alone:

  pack_bits / unpack_bits   value i's low `bits` bits at bits [i*bits,
                            (i+1)*bits) of ceil(n*bits/32) u32 words, LSB-first
  labels_offset             mbrwt_wire_labels_offset in closed form
  segment_bytes             a segment's size for a label capacity
  wire_segment              the exact bytes of one rank's segment
  reassemble                the global CSR from the segments' bytes alone

and the shapes are the smallest at which each path of the kernels exists:
WIDTHS (which pack and unpack kernel each takes is stated there), ROW_EDGES,
LABEL_EDGES / LABEL_CAPS, SEGMENT_PLANS.  The value generators put bits above
`bits` into their values: only the low `bits` bits may reach the wire.
"""
from collections import namedtuple

import numpy as np

LOST = (1 << 64) - 1  # the header of a rank whose own CSR was too small

# (bits_count, bits_label) and the kernels the dispatch of mbrwt_pack_csr_device
# / mbrwt_unpack_labels_device takes for 16-byte aligned d_cols / d_values:
# k_pack_csr12 at 12/12 only, k_unpack_labels12 at every bits_label <= 12.
WIDTHS = (
    (1, 1),      # k_pack_csr    k_unpack_labels12
    (7, 7),      # k_pack_csr    k_unpack_labels12
    (11, 11),    # k_pack_csr    k_unpack_labels12
    (12, 12),    # k_pack_csr12  k_unpack_labels12
    (13, 12),    # k_pack_csr    k_unpack_labels12   (4,096 columns)
    (12, 11),    # k_pack_csr    k_unpack_labels12   (2,048 columns)
    (13, 13),    # k_pack_csr    k_unpack_labels_dev
    (16, 16),    # k_pack_csr    k_unpack_labels_dev
    (17, 17),    # k_pack_csr    k_unpack_labels_dev
    (31, 31),    # k_pack_csr    k_unpack_labels_dev
    (32, 32),    # k_pack_csr    k_unpack_labels_dev
)

# rows of a slice: the 8-value thread group of k_pack_csr12, the 32-value
# chunk, the 256-thread workgroup, kOffRows / kUnpackTile
ROW_EDGES = (0, 1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049)
# labels of a slice: those, and one workgroup of k_unpack_labels12
LABEL_EDGES = ROW_EDGES + (8191, 8192, 8193)
BIG_CAP = 8203  # above 8,192, a multiple of neither 8 nor 32
LABEL_CAPS = (1, 7, 8, 9, 31, 32, 33, BIG_CAP)


def _mask(bits):
    return (1 << bits) - 1


# ---- the bit packing --------------------------------------------------------

def pack_bits(values, bits):
    """u32 words of the values' low `bits` bits; O(n): every value is shifted
    to its place in a u64, whose low half goes into word w and whose high half
    into word w + 1 (the values of one word are OR-ed by a reduceat over the
    runs of equal w)."""
    assert 1 <= bits <= 32
    v = np.asarray(values).astype(np.uint64) & np.uint64(_mask(bits))
    n = len(v)
    nw = (n * bits + 31) // 32
    out = np.zeros(nw + 1, dtype=np.uint64)
    if n:
        pos = np.arange(n, dtype=np.uint64) * np.uint64(bits)
        w = (pos >> np.uint64(5)).astype(np.int64)
        x = v << (pos & np.uint64(31))
        starts = np.flatnonzero(np.diff(w, prepend=-1))
        out[w[starts]] |= np.bitwise_or.reduceat(x & np.uint64(0xFFFFFFFF), starts)
        out[w[starts] + 1] |= np.bitwise_or.reduceat(x >> np.uint64(32), starts)
    assert out[nw] == 0
    return out[:nw].astype(np.uint32)


def unpack_bits(words, n, bits):
    """The n values of `bits` bits in words (u32)."""
    assert 1 <= bits <= 32
    wd = np.concatenate([np.asarray(words, dtype=np.uint32).astype(np.uint64), np.zeros(1, dtype=np.uint64)])
    assert len(wd) - 1 >= (n * bits + 31) // 32
    pos = np.arange(n, dtype=np.uint64) * np.uint64(bits)
    w = (pos >> np.uint64(5)).astype(np.int64)
    x = wd[w] | (wd[w + 1] << np.uint64(32))
    return ((x >> (pos & np.uint64(31))) & np.uint64(_mask(bits))).astype(np.uint32)


# ---- the segment ------------------------------------------------------------

def _round16(x):
    return (x + 15) // 16 * 16


def labels_offset(n_rows, bits_c):
    """Byte of a segment's label field: header, whole 32-count chunks, 16-byte pad."""
    return _round16(8 + (n_rows + 31) // 32 * bits_c * 4)


def segment_bytes(lab_off, labels_cap, bits_l):
    return _round16(lab_off + max(1, (labels_cap + 31) // 32 * bits_l) * 4)


def wire_segment(offsets, cols, num_labels, cols_cap, labels_cap, bits_c, bits_l, lab_off, wire_bytes):
    """The bytes (u8 [wire_bytes]) mbrwt_pack_csr_device writes."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    n_rows = len(offsets) - 1
    assert lab_off % 16 == 0 and wire_bytes % 16 == 0 and lab_off >= labels_offset(n_rows, bits_c)
    assert lab_off + (labels_cap + 31) // 32 * bits_l * 4 <= wire_bytes
    seg = np.zeros(wire_bytes, dtype=np.uint8)
    if num_labels > cols_cap:
        seg[:8] = 0xFF
        return seg
    seg[:8] = np.frombuffer(int(num_labels).to_bytes(8, "little"), dtype=np.uint8)
    counts = (offsets[1:] - offsets[:-1]) & np.uint64(0xFFFFFFFF)
    cw = pack_bits(counts, bits_c).view(np.uint8)
    seg[8:8 + len(cw)] = cw
    nl = min(int(num_labels), labels_cap)
    lw = pack_bits(np.asarray(cols, dtype=np.uint32)[:nl], bits_l).view(np.uint8)
    seg[lab_off:lab_off + len(lw)] = lw
    return seg


def header(seg):
    return int.from_bytes(bytes(seg[:8]), "little")


def reassemble(segments, counts, lab_off, labels_cap, bits_c, bits_l, values_cap):
    """(offsets u64 [N+1], labels u32 [total], (total, bad)) of the segments
    (u8 arrays) holding counts[r] rows each: what mbrwt_unpack_offsets_device
    and mbrwt_unpack_labels_device promise.  bad: a header above labels_cap,
    or the clamped total above values_cap; no label is returned then."""
    cnt, labs, total, bad = [], [], 0, 0
    for seg, n in zip(segments, counts):
        seg = np.ascontiguousarray(seg, dtype=np.uint8)
        cnt.append(unpack_bits(seg[8:8 + (n * bits_c + 31) // 32 * 4].view(np.uint32), n, bits_c))
        L = header(seg)
        if L > labels_cap:
            bad = 1
        L = min(L, labels_cap)
        total += L
        labs.append(unpack_bits(seg[lab_off:lab_off + (L * bits_l + 31) // 32 * 4].view(np.uint32), L, bits_l))
    if total > values_cap:
        bad = 1
    c = np.concatenate(cnt + [np.zeros(0, dtype=np.uint32)]).astype(np.uint64)
    offs = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(c, dtype=np.uint64)])
    labels = np.concatenate(labs + [np.zeros(0, dtype=np.uint32)]) if not bad else np.zeros(0, dtype=np.uint32)
    return offs, labels.astype(np.uint32), (total, bad)


# ---- values -------------------------------------------------------------------

def specials(bits):
    """0, all ones, the top bit alone; below 32 bits also all ones and zero
    under garbage in bits `bits`..31."""
    s = [0, _mask(bits), 1 << (bits - 1)]
    if bits < 32:
        s += [0xFFFFFFFF, 0xFFFFFFFF & ~_mask(bits), (0xA5A5A5A5 & ~_mask(bits)) | (1 << (bits - 1))]
    return s


def values(n, bits, seed=0):
    """n u32 values: random ones, every second in range and every other with
    random bits above `bits`; specials(bits) at the front, at the back
    (reversed) and scattered."""
    rng = np.random.default_rng([seed, n & 0xFFFFFFFF, bits])
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    v[::2] &= np.uint32(_mask(bits))
    sp = np.array(specials(bits), dtype=np.uint32)
    k = min(n, len(sp))
    if n >= 2 * len(sp):
        v[n - len(sp):] = sp[::-1]
    if n >= 64:
        at = rng.integers(len(sp), n - len(sp), 4 * len(sp))
        v[at] = np.tile(sp, 4)
    v[:k] = sp[:k]
    if n == 1:
        v[0] = sp[-1]  # (a single value: the one that tempts a missing mask)
    return v


def counts(n, bits, seed=0):
    """n row counts (u32, bits above `bits` set in some): the largest count
    of the field first and last, a zero inside."""
    c = values(n, bits, seed + 1000)
    if n:
        c[0] = c[-1] = 0xFFFFFFFF if n > 1 else _mask(bits)
    if n > 2:
        c[n // 2] = 0
    return c


def offsets_of(cnt, base=0):
    """u64 CSR offsets from `base` with the counts as differences."""
    return np.uint64(base) + np.concatenate([np.zeros(1, dtype=np.uint64),
                                             np.cumsum(np.asarray(cnt).astype(np.uint64), dtype=np.uint64)])


# ---- shapes of the pack test ----------------------------------------------------

PackCase = namedtuple("PackCase", "n_rows num_labels labels_cap cols_cap")


def pack_cases():
    """Every ROW_EDGES and LABEL_EDGES value once, and every LABEL_CAPS
    capacity with cap - 1, cap, cap + 1 (fits cols_cap: clamped) and
    cols_cap + 1 (the lost header) labels: a reduced cross, rows cycling."""
    out = []
    R = ROW_EDGES
    for i, L in enumerate(LABEL_EDGES):
        out.append(PackCase(R[(len(R) - 1 - i) % len(R)], L, BIG_CAP, BIG_CAP + 100))
    k = 0
    for cap in LABEL_CAPS:
        for L in (cap - 1, cap, cap + 1, cap + 2):  # (cols_cap = cap + 1)
            out.append(PackCase(R[k % len(R)], L, cap, cap + 1))
            k += 5
    return out


# ---- segment plans --------------------------------------------------------------

Plan = namedtuple("Plan", "name cap labels rows")


def _plan(name, cap, labels):
    rows = [ROW_EDGES[(3 * i + len(labels)) % len(ROW_EDGES)] for i in range(len(labels))]
    return Plan(name, cap, tuple(labels), tuple(rows))


def _many(n):
    cyc = (0, 1, 7, 8, 9, 31, 32, 33, 0, 0, 255, 256, 257, 5)
    return [cyc[i % len(cyc)] for i in range(n)]


# per-segment label counts (the wire does not couple a segment's label count
# to its row counts: rows are ROW_EDGES values in turn); a segment above its
# plan's cap is an overflowing rank (the unpack flags the exchange)
SEGMENT_PLANS = (
    _plan("one-8193", BIG_CAP, [8193]),
    _plan("one-at-cap", 33, [33]),
    _plan("one-empty", 33, [0]),
    _plan("two-on-4096", BIG_CAP, [4096, 100]),            # a multiple of 8 and of 2,048
    _plan("two-on-8", BIG_CAP, [8, 13]),
    _plan("three-8k+1-8k+7", BIG_CAP, [17, 30, 50]),       # boundaries at 17 and 47
    _plan("three-on-2048", BIG_CAP, [2048, 2048, 5]),
    _plan("three-on-8192", BIG_CAP, [8192, 1, 8190]),      # boundaries at 8,192 and 8,193
    _plan("three-on-8191", BIG_CAP, [8191, 2, 7]),         # boundaries at 8,191 and 8,193
    _plan("three-first-empty", BIG_CAP, [0, 9, 40]),
    _plan("three-middle-empty", BIG_CAP, [9, 0, 40]),
    _plan("three-last-empty", BIG_CAP, [9, 40, 0]),
    _plan("three-all-empty", 9, [0, 0, 0]),
    _plan("three-over-cap", 33, [5, 34, 3]),
    _plan("seven-two-empty", BIG_CAP, [5, 0, 0, 13, 0, 8, 2049]),
    _plan("seven-cap-33", 33, [33, 32, 0, 31, 1, 33, 9]),
    _plan("eight-at-cap", BIG_CAP, [8192, 0, 1, 2047, 8, 7, BIG_CAP, 0]),
    _plan("eight-all-empty", BIG_CAP, [0] * 8),
    _plan("eight-small", 257, [1, 7, 0, 0, 9, 255, 257, 2]),
    _plan("nine", 257, _many(9)),
    _plan("sixty-three", 257, _many(63)),
    _plan("sixty-four", 257, _many(64)),
    _plan("sixty-four-last-only", 257, [0] * 63 + [257]),
) + tuple(_plan("two-cap-%d" % c, c, [c, c]) for c in LABEL_CAPS[:-1])  # the seg_words guard of the fast path


# per-segment row counts of the offset scan (1..8 segments): every ROW_EDGES
# value, empty segments first, in the middle, last, and all of them
OFFSET_PLANS = (
    (2049,), (0,),
    (0, 257), (2048, 1),
    (0, 0, 0), (7, 0, 2047), (33, 9, 0),
    (255, 256, 8, 31),
    (0, 2049, 0, 32, 0),
    (1, 7, 8, 9, 31, 32),
    (33, 255, 0, 0, 256, 257, 2047),
    (2048, 0, 2049, 1, 0, 2047, 8, 0),
)


def count_segments(seg_counts, bits):
    """(segments, lab_off, per, offsets u64 [N+1]) of segments that hold row
    counts only (header 0, no label): seg_counts[r] = the u32 counts of segment r."""
    lab_off = labels_offset(max(len(c) for c in seg_counts), bits)
    per = segment_bytes(lab_off, 0, bits)
    none = np.zeros(0, dtype=np.uint32)
    segs = [wire_segment(offsets_of(c), none, 0, 0, 0, bits, bits, lab_off, per) for c in seg_counts]
    c = np.concatenate(list(seg_counts) + [none]).astype(np.uint64) & np.uint64(_mask(bits))
    return segs, lab_off, per, np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(c, dtype=np.uint64)])


def plan_segments(plan, bits_c, bits_l, seed=0):
    """(segments [u8 arrays], per-segment (offsets, cols), lab_off, per) of a
    plan: every segment at the offset of the largest slice."""
    lab_off = labels_offset(max(plan.rows), bits_c)
    per = segment_bytes(lab_off, plan.cap, bits_l)
    segs, csr = [], []
    for r, (L, n) in enumerate(zip(plan.labels, plan.rows)):
        off = offsets_of(counts(n, bits_c, seed + r), base=(1 << 32) + 5 if r % 2 else 0)
        cols = values(max(L, 1), bits_l, seed + 100 + r)
        csr.append((off, cols))
        segs.append(wire_segment(off, cols, L, len(cols), plan.cap, bits_c, bits_l, lab_off, per))
    return segs, csr, lab_off, per
