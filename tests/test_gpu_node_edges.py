"""GPU parity of get_rows on the per-node images (csrc/query.hip and the csrc/nodes_*.hip kernel families) at the
edges of their output path, on the deterministic fixtures of
tests/edge_shapes.py.  The layout is pinned to 'nodes'; every config asserts
its traversal kernel first; every comparison is bit-exact on integers, against
the CPU oracle's CSR of all rows (one per matrix) and against the closed form.
MBRWT_OPT_SLOT_LABELS sets the slot size K exactly (0: auto_slots()).

Rowblock kernels (k_traverse_ptw narrow / wide / deep, k_traverse_p2w ->
k_compact_blocks; a rowblock of 16 rows holds C = 16 K labels):
  * the overflow decision `running > C`, offsets still written for an
    overflowing rowblock: tile_totals(tile=16) over C-2..C+2
  * k_compact_blocks' 128-label prefetch and C >= 128 against C < 128
    (K = 8 / 7): totals 126..130; its rounds of 16 U labels (U = 8 on a
    matrix of <= 32 labels per row -- the padded configs --, else 32):
    254..258, 382..386, 638..642, 1022..1026
  * the LDS rings (256 labels in ptw, 512 in p2w) and their `direct` branch
    `rtot + (running - flushed) > S`: 254..258, 510..514, single rows of
    255 / 256 / 257 labels
  * every rowblock overflowing, only the first, only the last, a partial last
    rowblock (n mod 16 in {1, 15}) overflowing with the heavy row on its last
    lane, one row alone over C among empty rows
  * partial chunks / rowblocks / tiles, four rowblocks per compaction wave,
    one rowblock more than a workgroup's 7 (ptw) and 4 (p2w) waves:
    node_geometry at k = K-1, K, K+1
k_traverse_fast2 (SMALLK at K = 32) -> k_compact_chunks (8-row chunks whose
kept labels are packed back to back in 8 K labels): _chunk_batches --
counts K-1 / K / K+1 on each chunk lane, an overflow row last in its chunk
after seven rows of K labels (with K < 32 its 32-label stage once ran past
the chunk's region), a chunk of eight overflow rows, empty rows before an
overflow row (the prow / brow search), chunks that store 63 / 64 / 65 labels
(the 64-label round), a partial last chunk, tile_totals(tile=8) around 64
and 8 K.
k_traverse_group (u32 masks G = 8, u64 masks G = 32) and the lane kernel
k_traverse (MBRWT_OPT_KERNEL = 1 on every tree) -> k_compact (256-row
tiles): counts 31 / 32 / 33 (the 32-label LDS stage) and K-1 / K / K+1 at
n = 255 / 256 / 257, the heavy row first, last and alone.
The label map's LDS limit (label_map_lds(): up to 16,384 entries staged by
the compaction; k_compact adds its own static LDS): test_label_map_limit.
Every batch also asserts mbrwt_overflow_rows(): the rows left to the direct
pass are exactly those of the rowblocks over C, or the rows over K.
"""
import numpy as np
import pytest

import edge_shapes as E
from conftest import gpu_available
from test_gpu_edge_shapes import _Case, _check_batch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

_NO_PACKT = {"MBRWT_PACKT": 0}
# name -> (matrix, (partitioner, arity), build options, the traversal kernel it must run)
# matrix: ("staircase", m, pad rows of one label each) or ("windows", m, top, shifts)
_CONFIGS = {
    "ptw": (("staircase", 512, 0), ("basic", 8), {}, "k_traverse_ptw"),
    # pad rows of one label: <= 32 labels per row (k_compact_blocks<BIG = false>, U = 8); empty
    # pad rows would unfold the root (it is folded when at least half of the rows are non-empty)
    "ptw-pad": (("staircase", 512, 3800), ("basic", 8), {}, "k_traverse_ptw"),
    "ptw-wide": (("staircase", 256, 0), ("basic", 16), {}, "k_traverse_ptw"),
    "ptw-deep": (("windows",) + E.WINDOWS_DEEP, ("basic", 2), {}, "k_traverse_ptw"),
    "p2w": (("staircase", 256, 0), ("basic", 4), _NO_PACKT, "k_traverse_p2w"),
    "p2w-pad": (("staircase", 256, 800), ("basic", 4), _NO_PACKT, "k_traverse_p2w"),
    "fast2": (("staircase", 512, 0), ("basic", 8), {"MBRWT_PACKT": 0, "MBRWT_PACK2": 0}, "k_traverse_fast2"),
    "fast2-nopack": (("staircase", 512, 0), ("basic", 8), {"MBRWT_PACKT": 0, "MBRWT_PACK2": 0, "MBRWT_PACK": 0},
                     "k_traverse_fast2"),
    "group-8": (("staircase", 256, 0), ("basic", 16), _NO_PACKT, "k_traverse_group"),
    "group-64bit": (("staircase", 70, 0), ("basic", 33), _NO_PACKT, "k_traverse_group"),
}
_ROWBLOCK = ("ptw", "ptw-pad", "ptw-wide", "ptw-deep", "p2w", "p2w-pad")
_CHUNK = ("fast2", "fast2-nopack")
_TILE = ("group-8", "group-64bit")

_cases = {}
_devs = {}


def _case(O, name):
    matrix, (part, arity), _, _ = _CONFIGS[name]
    key = (matrix, part, arity)
    if key not in _cases:
        if matrix[0] == "staircase":
            _, m, pad = matrix
            c = _Case(O, E.staircase(m, pad, single=True), part, arity, 0)
            np.testing.assert_array_equal(c.counts, E.staircase_count(np.arange(c.n), m, single=True))
            assert E.closed_form_ok(c.off[: m + 2], c.cols[: int(c.off[m + 1])], c.counts[: m + 1])
            c.closed, c.top, c.nshifts = False, m, 0   # (_check_batch: the closed form for row ids <= m)
        else:
            _, m, top, shifts = matrix
            c = _Case(O, E.windows(m, top, shifts), part, arity, 0)
            ids = np.arange(c.n)
            np.testing.assert_array_equal(c.counts, E.windows_count(ids, top))
            assert E.closed_form_ok(c.off, c.cols, c.counts, E.windows_shift(ids, top, shifts))
            c.closed, c.top, c.nshifts, c.shifts = False, top, len(shifts), shifts
        _cases[key] = c
    return _cases[key]


def _height(ex, u):
    nc, fc = ex["num_children"], ex["first_child"]
    return 0 if nc[u] == 0 else 1 + max(_height(ex, int(fc[u]) + c) for c in range(int(nc[u])))


def _device(O, build_env, name):
    """The context of _CONFIGS[name] (built once), its form asserted."""
    case = _case(O, name)
    if name not in _devs:
        from genome_graph_annotation_amd import BRWTDevice
        _, _, opts, kernel = _CONFIGS[name]
        for k, v in opts.items():
            build_env(k, v)
        dev = BRWTDevice.from_tree(case.ex, layout="nodes")
        print(name, dev.layout(), dev.traverse_kernel(), dev.num_rows(), dev.num_relations())
        assert dev.layout() == "nodes" and dev.rows_stats() is None
        assert dev.traverse_kernel().split("/")[0] == kernel, (name, dev.traverse_kernel())
        assert (dev.num_rows(), dev.num_relations()) == (case.n, int(case.counts.sum()))
        nc, fc = case.ex["num_children"], case.ex["first_child"]
        if name == "ptw-wide":
            assert int(nc[0]) > 8
        if name == "ptw-deep":
            assert max(_height(case.ex, int(fc[0]) + c) for c in range(int(nc[0]))) > 4
        if name == "group-64bit":
            assert int(np.asarray(nc).max()) > 32
        if name.endswith("-pad"):      # k_compact_blocks<BIG = false>
            assert dev.num_relations() <= 32 * dev.num_rows()
        elif name in _ROWBLOCK and name != "ptw-deep":
            assert dev.num_relations() > 32 * dev.num_rows()
        _devs[name] = dev
    return _devs[name], case


def _auto_slots(dev):
    """auto_slots() of csrc/nodes_walk.hpp."""
    mean = dev.num_relations() / dev.num_rows()
    k = 32
    while k < 2.0 * mean + 8.0 and k < 1024:
        k <<= 1
    return k


def _block_overflow(counts, C):
    """Rows of the 16-row rowblocks that hold more than C labels."""
    c = np.asarray(counts, dtype=np.int64)
    return sum(len(c[i:i + 16]) for i in range(0, len(c), 16) if int(c[i:i + 16].sum()) > C)


def _row_overflow(counts, K):
    """Rows of more than K labels."""
    return int((np.asarray(counts, dtype=np.int64) > K).sum())


def _run(dev, case, counts, name, overflow, extra=False):
    """The batch whose rows carry the label counts `counts`; `overflow`: the
    rows it must leave to the direct pass (no more, no fewer)."""
    counts = np.asarray(counts, dtype=np.uint64)
    assert int(counts.max(initial=0)) <= case.top, (name, int(counts.max()), case.top)
    if not case.nshifts:   # the staircase: row k has k labels (_check_batch checks the closed form)
        _check_batch(dev, case, counts, name, extra=extra)
    else:
        rows = E.windows_rows(counts, case.top, case.nshifts)
        off_e, cols_e = E.gather_csr(case.off, case.cols, rows)
        assert E.closed_form_ok(off_e, cols_e, counts, E.windows_shift(rows, case.top, case.shifts)), name
        _check_batch(dev, case, rows, name, extra=extra, closed=False)
    assert dev.overflow_rows() == overflow, (name, dev.overflow_rows(), overflow)


def _cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint64) for p in parts])


def _spread(total, n, cap, top):
    """n row counts of sum `total`, each <= cap, filled from the front."""
    out = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        out[i] = min(cap, total - int(out.sum()))
    assert int(out.sum()) == total and int(out.max()) <= top, (total, n, cap)
    return out


# ---- the rowblock kernels -------------------------------------------------------

_FIXED_WINDOWS = ((126, 130), (254, 258), (382, 386), (510, 514), (638, 642), (1022, 1026))


def _rowblock_batches(K, top):
    """(name, counts) for a rowblock of C = 16 K labels, rows of <= top labels."""
    C = 16 * K
    yield f"block totals {C - 2}..{C + 2}", E.tile_totals(top, max(C - 2, 0), C + 2, tile=16)
    for lo, hi in _FIXED_WINDOWS:
        if lo <= 16 * top:
            yield f"block totals {lo}..{hi}", E.tile_totals(top, lo, hi, tile=16)
    for k in (255, 256, 257):   # one round's labels against the 256-label ring
        if k <= top:
            b = np.zeros(16, dtype=np.uint64)
            yield f"single rows of {k}", _cat(*[np.roll(_cat([k], b[1:]), s) for s in (0, 7, 15)], [k, k], b[2:], [k])
    if C + 1 <= top:
        yield "one row over C among empty rows", _cat(np.zeros(20), [C + 1], np.zeros(27))
        yield "partial last block (1 row) overflowing", _cat(np.arange(16) % 8, [C + 1])
    if K + 1 <= top:
        over, full, under = np.full(16, K + 1), np.full(16, K), np.full(16, max(K, 1) - 1)
        yield "every block overflowing", _cat(over, over, over, over, over)
        yield "only the first block overflowing", _cat(over, full, under, full)
        yield "only the last block overflowing", _cat(full, under, full, over)
    if 2 * K + 1 <= top:
        yield "partial last block (15 rows) overflowing", _cat(np.full(16, K), np.full(14, K), [2 * K + 1])
        yield "partial last block (15 rows) full", _cat(np.full(16, K), np.full(14, K), [2 * K])


@pytest.mark.parametrize("K", [1, 7, 8, 16, 32, 64, 0])
@pytest.mark.parametrize("name", _ROWBLOCK)
def test_rowblock_kernels(oracle_mod, build_env, name, K):
    from genome_graph_annotation_amd import _lib as L
    dev, case = _device(oracle_mod, build_env, name)
    dev.set_option(L.MBRWT_OPT_SLOT_LABELS, K)
    try:
        k = K or _auto_slots(dev)
        ran = []
        for what, counts in _rowblock_batches(k, case.top):
            if len(counts):
                _run(dev, case, counts, f"{name} K={K}: {what}", _block_overflow(counts, 16 * k))
                ran.append(what)
        # (auto: the heavy rows of the ring's edge and the full row, with count_labels and get_batch)
        for heavy in sorted({max(k, 1) - 1, k, k + 1} | ({255, 256, 257, case.top} if K == 0 else set())):
            if heavy <= case.top:
                for what, counts in E.node_geometry(heavy):
                    _run(dev, case, counts, f"{name} K={K}: geometry k={heavy} {what}", _block_overflow(counts, 16 * k),
                         extra=K == 0)
        print(name, K, k, len(ran), "edge batches")
        # what the matrix can reach: the overflow decision wherever 16 rows hold C + 2 labels
        assert (f"block totals {16 * k - 2}..{16 * k + 2}" in ran) == (16 * k - 2 <= 16 * case.top)
        assert K == 0 or "every block overflowing" in ran or k + 1 > case.top
    finally:
        dev.set_option(L.MBRWT_OPT_SLOT_LABELS, 0)
    if K == 0 and case.nshifts == 0:   # the pad rows and the full row: the matrix's last rows, a partial block
        last = np.arange(max(case.n - 200, 0), case.n, dtype=np.uint64)
        _check_batch(dev, case, last, "last rows")
        assert dev.overflow_rows() == _block_overflow(case.counts[last.astype(np.int64)], 16 * _auto_slots(dev))


# ---- k_traverse_fast2 and k_compact_chunks --------------------------------------

def _chunk_batches(K, top):
    """(name, counts) for 8-row chunks whose kept labels share 8 K labels."""
    light = np.arange(8) % 8
    lanes, full_lanes = [], []
    for lane in range(8):
        for k in (K - 1, K, K + 1):
            c, f = light.copy(), np.full(8, K)
            c[lane] = f[lane] = k
            lanes.append(c)
            full_lanes.append(f)
    yield "K-1 / K / K+1 on each lane among light rows", _cat(*lanes)
    yield "K-1 / K / K+1 on each lane among rows of K", _cat(*full_lanes)
    seven = np.full(7, K)
    yield "overflow row last after seven rows of K", _cat(seven, [K + 1], np.full(8, K), seven, [top])
    yield "the same on the batch's only chunk", _cat(seven, [K + 1])
    yield "a chunk of eight overflow rows", _cat(light, np.full(8, K + 1), light, np.full(8, top), np.full(8, K))
    yield "empty rows before an overflow row", _cat([0, 0, K + 1, 0, 0, 3, K + 2, 5], [K + 1, 0, 0, 0, 0, 0, 0, 1],
                                                    np.zeros(7), [K + 1], [0, K, 0, K + 1, 0, 0, K, 0],
                                                    [K + 1, K + 1, 0, 0, 2, 0, K + 1, 0], [0, 0, 0, K + 1])
    for stored in (63, 64, 65, 127, 128, 129):
        if stored <= 7 * K:
            kept = _spread(stored, 7, K, top)
            yield f"a chunk storing {stored}", _cat(kept, [0], kept[::-1], [0], [0], kept)
            yield f"a chunk storing {stored} and an overflow row", _cat(kept, [K + 1], [K + 1], kept[::-1], kept[:3],
                                                                        [top], kept[3:], kept[:5])
    for r in range(1, 8):
        yield f"partial last chunk of {r}", _cat(np.full(8, K), (np.arange(r) % 2) * (K + 1) + K - 1)
    yield "chunk totals 62..66", E.tile_totals(top, 62, 66, tile=8)
    yield f"chunk totals {8 * K - 2}..{8 * K + 2}", E.tile_totals(top, 8 * K - 2, 8 * K + 2, tile=8)
    yield "every row", np.arange(top + 1)


@pytest.mark.parametrize("K", [16, 31, 32, 33, 64])
@pytest.mark.parametrize("name", _CHUNK)
def test_chunk_kernels(oracle_mod, build_env, name, K):
    from genome_graph_annotation_amd import _lib as L
    dev, case = _device(oracle_mod, build_env, name)
    dev.set_option(L.MBRWT_OPT_SLOT_LABELS, K)
    try:
        assert dev.traverse_kernel().split("/")[0] == "k_traverse_fast2"
        for what, counts in _chunk_batches(K, case.top):
            _run(dev, case, counts, f"{name} K={K}: {what}", _row_overflow(counts, K))
        for heavy in (K - 1, K, K + 1):
            for what, counts in E.node_geometry(heavy, (1, 7, 8, 9, 255, 256, 257)):
                _run(dev, case, counts, f"{name} K={K}: geometry k={heavy} {what}", _row_overflow(counts, K),
                     extra=K == 32)
    finally:
        dev.set_option(L.MBRWT_OPT_SLOT_LABELS, 0)


# ---- the group and lane kernels with k_compact ----------------------------------

def _tile_batches(K, top):
    for k in sorted({31, 32, 33, K - 1, K, K + 1}):
        if k <= top:
            yield from ((f"k={k} {what}", counts) for what, counts in E.node_geometry(k, (255, 256, 257)))
    over = min(K + 1, top)
    yield "overflow rows first and last in every tile", _cat([over], np.arange(254) % 8, [over, over],
                                                            np.arange(254) % 8, [over, over])
    yield "every row", np.arange(top + 1)
    yield "rows of K - 1, K, K + 1", np.tile(np.minimum([K - 1, K, K + 1], top), 100)


def _tile_checks(dev, case, name, K):
    from genome_graph_annotation_amd import _lib as L
    dev.set_option(L.MBRWT_OPT_SLOT_LABELS, K)
    try:
        for what, counts in _tile_batches(K, case.top):
            _run(dev, case, counts, f"{name} K={K}: {what}", _row_overflow(counts, K),
                 extra=K == 32 and what.endswith("-257"))
    finally:
        dev.set_option(L.MBRWT_OPT_SLOT_LABELS, 0)


@pytest.mark.parametrize("K", [16, 32, 64])
@pytest.mark.parametrize("name", _TILE)
def test_group_kernel(oracle_mod, build_env, name, K):
    dev, case = _device(oracle_mod, build_env, name)
    _tile_checks(dev, case, name, K)


@pytest.mark.parametrize("K", [16, 32, 64])
@pytest.mark.parametrize("name", [n for n in _CONFIGS if not n.endswith("-pad")])
def test_lane_kernel(oracle_mod, build_env, name, K):
    """MBRWT_OPT_KERNEL = 1 on every tree above: k_traverse, k_compact."""
    from genome_graph_annotation_amd import _lib as L
    dev, case = _device(oracle_mod, build_env, name)
    dev.set_option(L.MBRWT_OPT_KERNEL, 1)
    try:
        assert dev.traverse_kernel() == "k_traverse"
        _tile_checks(dev, case, f"{name} lane", K)
    finally:
        dev.set_option(L.MBRWT_OPT_KERNEL, 0)


# ---- the label map's LDS limit ---------------------------------------------------

_LABEL_MAP_KERNELS = {"default": ({}, 0, "k_traverse"), "lane": ({}, 1, "k_traverse"),
                      "group": (_NO_PACKT, 0, "k_traverse_group")}


@pytest.mark.parametrize("which", list(_LABEL_MAP_KERNELS))
@pytest.mark.parametrize("m", [16384, 16385])
def test_label_map_limit(oracle_mod, build_env, m, which):
    """A non-identity label map of 16,384 entries (label_map_lds()'s limit:
    64 KiB of LDS) and of 16,385 (read from global memory): the oracle's tree
    with leaf_column reversed, so every label c reads m - 1 - c in the
    oracle's order (the order of a row's labels is the leaves' pre-order).
    With K = 8 the longer rows take the direct pass (final_label from global
    memory).  k_compact keeps 2,056 bytes of static LDS beside the 64 KiB of
    the map: the launch is accepted (a gfx950 workgroup may take 160 KiB)."""
    from genome_graph_annotation_amd import BRWTDevice, _lib as L
    opts, variant, kernel = _LABEL_MAP_KERNELS[which]
    key = ("label-map", m)
    if key not in _cases:
        base = _Case(oracle_mod, E.label_map_matrix(m), "basic", 8, 0)
        _, top, shifts = E.windows_wide(m)
        nw = len(shifts) * (top + 1)
        ids = np.arange(nw)
        assert base.n == nw + 4 and 280 <= base.n <= 320
        assert E.closed_form_ok(base.off[: nw + 1], base.cols[: int(base.off[nw])], E.windows_count(ids, top),
                                E.windows_shift(ids, top, shifts))
        assert base.cols[int(base.off[nw]):].tolist() == [0, 16383, m - 1] + sorted({0, 16383, m - 1})
        nc = np.asarray(base.ex["num_children"])
        rev = dict(base.ex)
        rev["leaf_column"] = np.where(nc == 0, m - 1 - np.asarray(base.ex["leaf_column"]).astype(np.int64),
                                      base.ex["leaf_column"]).astype(np.uint32)
        c = _Case.__new__(_Case)
        c.dense, c.n, c.m, c.ex, c.off, c.counts, c.closed = base.dense[:, ::-1], base.n, m, rev, base.off, base.counts, False
        c.cols = (m - 1 - base.cols.astype(np.int64)).astype(base.cols.dtype)
        np.testing.assert_array_equal(np.bincount(c.cols, minlength=m), c.dense.sum(axis=0))
        _cases[key] = c
    case = _cases[key]
    for k, v in opts.items():
        build_env(k, v)
    dev = BRWTDevice.from_tree(case.ex, layout="nodes")
    dev.set_option(L.MBRWT_OPT_KERNEL, variant)
    print(m, which, dev.traverse_kernel())
    assert dev.layout() == "nodes" and dev.traverse_kernel() == kernel, dev.traverse_kernel()
    every = np.arange(case.n, dtype=np.uint64)
    tail = np.arange(case.n - 12, case.n, dtype=np.uint64)
    for K in (8, 0):
        dev.set_option(L.MBRWT_OPT_SLOT_LABELS, K)
        assert int((case.counts > 8).sum()) > 100 and _auto_slots(dev) > E.WIDE_TOP   # K = 8: a direct pass; auto: none
        _check_batch(dev, case, every, f"{m} {which} K={K}: every row", extra=True, closed=False)
        assert dev.overflow_rows() == (_row_overflow(case.counts, 8) if K else 0)
        _check_batch(dev, case, every[::-1], f"{m} {which} K={K}: every row, reversed", closed=False)
        _check_batch(dev, case, _cat(tail, every[:257 - 12]), f"{m} {which} K={K}: 257 rows", closed=False)
