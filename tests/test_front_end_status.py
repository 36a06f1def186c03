"""The early exits of the six build entry points over a label source (no GPU):
mbrwt_create_from_* / mbrwt_*_node_counts / mbrwt_tree_shape_from_* for CSR
rows and for sparse columns.  Every case returns before the first HIP call, so
the status and the mbrwt_last_error_message() text are pinned on the host
alone.  The three get_rows calls with a NULL context close the file."""
import ctypes as C

import pytest

from genome_graph_annotation_amd import _lib as L

N, M = 3, 4  # the 3-row x 4-column matrix every descriptor below describes
BAD_PTR = 0xDEAD0000  # an output word no entry point may keep when it refuses


def _u64(*v):
    return (C.c_uint64 * len(v))(*v)


def _u32(*v):
    return (C.c_uint32 * len(v))(*v)


class _Source:
    """One label source: its three entry points, its descriptor type, a good
    descriptor and the descriptors its host check refuses."""

    def __init__(self, key):
        self.key = key
        self.words = {"rows": "rows", "cols": "sparse columns"}[key]
        stem = {"rows": "rows", "cols": "sparse_columns"}[key]
        self.create = f"mbrwt_create_from_{stem}"
        self.counts = f"mbrwt_{stem}_node_counts"
        self.shape = f"mbrwt_tree_shape_from_{stem}"
        self.null_msg = f"null {self.words} description or output pointer"

    def good(self, num_rows=N, num_columns=M):
        """(descriptor, keep): rows {0,1} {2} {0,3}, i.e. columns {0,2} {0} {1} {2}"""
        if self.key == "rows":
            off, ids = _u64(0, 2, 3, 5), _u32(0, 1, 2, 0, 3)
            return L.RowsDesc(num_rows, num_columns, off, ids), (off, ids)
        off, ids = _u64(0, 2, 3, 4, 5), _u64(0, 2, 0, 1, 2)
        return L.SparseColumnsDesc(num_rows, num_columns, off, ids, None), (off, ids)

    def bad(self):
        """[(case, descriptor, keep, message)] of the host descriptor check"""
        out = []
        if self.key == "rows":
            ids = _u32(0, 1, 2, 3, 0, 1, 2)
            first = "row offsets: null array or first offset not 0"
            for name, off, msg in (
                    ("first offset not 0", _u64(1, 2, 3, 5), first),
                    ("descending offsets", _u64(0, 3, 2, 5), "row offsets not ascending"),
                    ("a row of 5 labels", _u64(0, 5, 6, 7), "a row of more labels than columns")):
                out.append((name, L.RowsDesc(N, M, off, ids), (off, ids), msg))
            out.append(("null offsets", L.RowsDesc(N, M, None, ids), (ids,), first))
            off = _u64(0, 2, 3, 5)
            out.append(("labels without cols", L.RowsDesc(N, M, off, None), (off,), first))
            return out
        ids, ids32 = _u64(0, 1, 2, 0, 1, 2), _u32(0, 1, 2, 0, 1, 2)
        good = _u64(0, 2, 3, 4, 5)
        first = "column offsets: null array or first offset not 0"
        out.append(("first offset not 0", L.SparseColumnsDesc(N, M, _u64(1, 2, 3, 4, 5), ids, None), (ids,), first))
        out.append(("null offsets", L.SparseColumnsDesc(N, M, None, ids, None), (ids,), first))
        out.append(("descending offsets", L.SparseColumnsDesc(N, M, _u64(0, 3, 2, 4, 5), ids, None), (ids,),
                    "column offsets not ascending"))
        out.append(("a column of more ids than rows", L.SparseColumnsDesc(N, M, _u64(0, 4, 5, 6, 6), ids, None),
                    (ids,), "a column of more row ids than rows"))
        out.append(("both rows and rows32", L.SparseColumnsDesc(N, M, good, ids, ids32), (good, ids, ids32),
                    "sparse columns: both rows and rows32 given"))
        out.append(("neither rows nor rows32", L.SparseColumnsDesc(N, M, good, None, None), (good,),
                    "sparse columns: neither rows nor rows32 given"))
        # (the check reads only the offsets: nothing of 2^32 + 1 rows stands behind the descriptor)
        out.append(("rows32 with 2^32 + 1 rows", L.SparseColumnsDesc((1 << 32) + 1, M, good, None, ids32),
                    (good, ids32), "sparse columns: rows32 with num_rows > 2^32"))
        return out


SOURCES = [_Source("rows"), _Source("cols")]
BAD = [pytest.param(s, i, id=f"{s.key}-{case[0]}") for s in SOURCES for i, case in enumerate(s.bad())]


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def _message(lib):
    return (lib.mbrwt_last_error_message() or b"").decode()


def _shape3():
    """(descriptor, keep): a root over two leaves"""
    nc, fc, lc = _u32(2, 0, 0), _u32(1, 0, 0), _u32(0, 0, 1)
    return L.ShapeDesc(3, nc, fc, lc), (nc, fc, lc)


@pytest.mark.parametrize("src", SOURCES, ids=lambda s: s.key)
def test_null_descriptor_or_output(lib, src):
    desc, keep = src.good()
    out = C.c_void_p(BAD_PTR)
    counts = _u64(7, 7, 7)
    for fn, null_desc, null_out in (
            (src.create, (None, None, 2, 0, C.byref(out)), (C.byref(desc), None, 2, 0, None)),
            (src.counts, (None, None, 2, 0, counts), (C.byref(desc), None, 2, 0, None)),
            (src.shape, (None, L.MBRWT_PARTITIONER_BASIC, 2, 0, 0, C.byref(out)),
             (C.byref(desc), L.MBRWT_PARTITIONER_BASIC, 2, 0, 0, None))):
        for args in (null_desc, null_out):
            lib.mbrwt_set_build_option(L.MBRWT_BUILD_LAYOUT, 99)  # (a refused call: leaves another message behind)
            assert getattr(lib, fn)(*args) == L.MBRWT_ERR_INVALID, fn
            assert _message(lib) == src.null_msg, fn
    assert list(counts) == [7, 7, 7]
    del keep


@pytest.mark.parametrize("src", SOURCES, ids=lambda s: s.key)
@pytest.mark.parametrize("partitioner", [-1, 2, 7])
def test_invalid_partitioner(lib, src, partitioner):
    desc, keep = src.good()
    out = C.c_void_p(BAD_PTR)
    assert getattr(lib, src.shape)(C.byref(desc), partitioner, 2, 0, 0, C.byref(out)) == L.MBRWT_ERR_INVALID
    assert _message(lib) == "partitioner must be MBRWT_PARTITIONER_BASIC or MBRWT_PARTITIONER_GREEDY"
    assert out.value is None  # (nulled before the check)
    del keep


@pytest.mark.parametrize("src", SOURCES, ids=lambda s: s.key)
@pytest.mark.parametrize("layout", [L.MBRWT_LAYOUT_NODES, L.MBRWT_LAYOUT_BOTH], ids=["nodes", "both"])
def test_create_builds_row_records_only(lib, src, layout):
    desc, keep = src.good()
    out = C.c_void_p(BAD_PTR)
    was = C.c_int64(0)
    assert lib.mbrwt_get_build_option(L.MBRWT_BUILD_LAYOUT, C.byref(was)) == L.MBRWT_OK
    assert lib.mbrwt_set_build_option(L.MBRWT_BUILD_LAYOUT, layout) == L.MBRWT_OK
    try:
        assert getattr(lib, src.create)(C.byref(desc), None, 2, 0, C.byref(out)) == L.MBRWT_ERR_UNSUPPORTED
        assert _message(lib) == f"{src.create} builds row records only: layout AUTO or ROWS"
        assert out.value is None
        # the gate stands in front of the empty-matrix route too
        empty, keep2 = src.good(num_rows=0)
        assert getattr(lib, src.create)(C.byref(empty), None, 2, 0, C.byref(out)) == L.MBRWT_ERR_UNSUPPORTED
        assert _message(lib) == f"{src.create} builds row records only: layout AUTO or ROWS"
    finally:
        assert lib.mbrwt_set_build_option(L.MBRWT_BUILD_LAYOUT, was.value) == L.MBRWT_OK
    del keep, keep2


@pytest.mark.parametrize("src,i", BAD)
def test_create_refuses_a_bad_descriptor(lib, src, i):
    _, desc, keep, msg = src.bad()[i]
    out = C.c_void_p(BAD_PTR)
    shape, keep_shape = _shape3()
    for sh in (None, C.byref(shape)):  # (the descriptor is checked before the shape)
        assert getattr(lib, src.create)(C.byref(desc), sh, 2, 0, C.byref(out)) == L.MBRWT_ERR_INVALID
        assert _message(lib) == msg
        assert out.value is None
    del keep, keep_shape


@pytest.mark.parametrize("src,i", BAD)
def test_counts_refuse_a_bad_descriptor(lib, src, i):
    _, desc, keep, msg = src.bad()[i]
    counts = _u64(7, 7, 7, 7, 7, 7, 7)
    assert getattr(lib, src.counts)(C.byref(desc), None, 2, 0, counts) == L.MBRWT_ERR_INVALID
    assert _message(lib) == msg
    assert list(counts) == [7] * 7
    del keep


@pytest.mark.parametrize("src,i", BAD)
@pytest.mark.parametrize("partitioner", [L.MBRWT_PARTITIONER_BASIC, L.MBRWT_PARTITIONER_GREEDY],
                         ids=["basic", "greedy"])
def test_shape_refuses_a_bad_descriptor(lib, src, i, partitioner):
    _, desc, keep, msg = src.bad()[i]
    out = C.c_void_p(BAD_PTR)
    assert getattr(lib, src.shape)(C.byref(desc), partitioner, 2, 4, 0, C.byref(out)) == L.MBRWT_ERR_INVALID
    assert _message(lib) == msg
    assert out.value is None
    del keep


@pytest.mark.parametrize("src", SOURCES, ids=lambda s: s.key)
@pytest.mark.parametrize("num_rows", [N, 0])
def test_counts_without_columns_are_zero(lib, src, num_rows):
    """num_columns = 0: the nodes the caller's shape names see no row -- OK and
    zeros, whatever else the descriptor holds, and nothing without a shape."""
    desc, keep = src.good(num_rows=num_rows, num_columns=0)
    shape, keep_shape = _shape3()
    counts = _u64(7, 7, 7, 7)
    assert getattr(lib, src.counts)(C.byref(desc), C.byref(shape), 0, 0, counts) == L.MBRWT_OK
    assert list(counts) == [0, 0, 0, 7]
    counts = _u64(7, 7, 7, 7)
    assert getattr(lib, src.counts)(C.byref(desc), None, 2, 0, counts) == L.MBRWT_OK
    assert list(counts) == [7, 7, 7, 7]
    # a descriptor the host check would refuse is not looked at
    _, bad, keep_bad, _ = src.bad()[0]
    bad.num_columns = 0
    counts = _u64(7, 7, 7, 7)
    assert getattr(lib, src.counts)(C.byref(bad), C.byref(shape), 0, 0, counts) == L.MBRWT_OK
    assert list(counts) == [0, 0, 0, 7]
    del keep, keep_shape, keep_bad


def test_get_rows_null_context(lib):
    """the u32 calls' argument check (tests/test_rows16_capi.py has the u16 calls')"""
    rows = _u64(0)
    off = _u64(7, 7)
    cols = _u32(9, 9, 9, 9)
    need = C.c_uint64(5)
    st3 = _u64(1, 1, 1)
    for call in (
            lambda: lib.mbrwt_get_rows(None, rows, 1, off, cols, 4, C.byref(need)),
            lambda: lib.mbrwt_get_rows_device(None, C.addressof(rows), 1, C.addressof(off), C.addressof(cols), 4,
                                              C.byref(need), None),
            lambda: lib.mbrwt_get_rows_device_async(None, C.addressof(rows), 1, C.addressof(off), C.addressof(cols),
                                                    4, C.addressof(st3), None)):
        lib.mbrwt_set_build_option(L.MBRWT_BUILD_LAYOUT, 99)  # (a refused call: leaves another message behind)
        assert call() == L.MBRWT_ERR_INVALID
        assert _message(lib) == "invalid argument"
    # a NULL d_status: refused by the argument check, before the context is looked at
    ctx = _u64(*([0] * 64))
    assert lib.mbrwt_get_rows_device_async(C.addressof(ctx), C.addressof(rows), 1, C.addressof(off),
                                           C.addressof(cols), 4, None, None) == L.MBRWT_ERR_INVALID
    assert _message(lib) == "invalid argument"
    assert list(off) == [7, 7] and list(cols) == [9] * 4 and need.value == 5 and list(st3) == [1, 1, 1]
    assert not any(ctx)
