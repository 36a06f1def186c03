"""Python mirror of the reference's BinaryMatrix surface over the HIP engine.

`BRWTDevice` answers the reference's BRWT queries (BinaryMatrix,
common/binary_matrix.hpp:9-29; BRWT, annotation/hierarchical_annotation/
BRWT.hpp:33-51) from a device-resident image through include/mbrwt.h.
The C++ mirror used by C++ callers is csrc/brwt_device.hpp; this module is
what the Python tests and bench.py drive.  Device-buffer entry points take
torch tensors only as plumbing for device memory and streams.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _lib as L


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _labels_batch(fn, h, rows, read_offsets, presence_ratio):
    """Host-buffer batched get_labels through `fn` (mbrwt[_wt]_get_labels_batch)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    if ro.size == 0:
        raise ValueError("read_offsets needs n_reads + 1 entries")
    lo = np.zeros(ro.size, dtype=np.uint64)
    need = C.c_uint64(0)
    cap = max(16, 4 * rows.size)
    while True:
        labs = np.zeros(cap, dtype=np.uint32)
        st = getattr(L.lib(), fn)(h, _p(rows, C.c_uint64), rows.size, _p(ro, C.c_uint64), ro.size - 1,
                                  float(presence_ratio), _p(lo, C.c_uint64), _p(labs, C.c_uint32), cap, C.byref(need))
        if st == L.MBRWT_ERR_CAPACITY:
            cap = int(need.value)
            continue
        L.check(st, fn)
        return lo, labs[: need.value]


def _top_labels_batch(fn, h, rows, read_offsets, num_top):
    """Host-buffer batched get_top_labels through `fn` (mbrwt[_wt]_get_top_labels_batch)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    if ro.size == 0:
        raise ValueError("read_offsets needs n_reads + 1 entries")
    lo = np.zeros(ro.size, dtype=np.uint64)
    need = C.c_uint64(0)
    cap = max(16, 4 * rows.size)
    while True:
        labs = np.zeros(cap, dtype=np.uint32)
        cnts = np.zeros(cap, dtype=np.uint64)
        st = getattr(L.lib(), fn)(h, _p(rows, C.c_uint64), rows.size, _p(ro, C.c_uint64), ro.size - 1,
                                  int(num_top), _p(lo, C.c_uint64), _p(labs, C.c_uint32), _p(cnts, C.c_uint64), cap,
                                  C.byref(need))
        if st == L.MBRWT_ERR_CAPACITY:
            cap = int(need.value)
            continue
        L.check(st, fn)
        return lo, labs[: need.value], cnts[: need.value]


def _labels_batch_device(fn, h, rows_t, read_off_t, presence_ratio, lab_off_t, labels_t, stream):
    """Device-buffer batched get_labels through `fn` (mbrwt[_multi]_get_labels_batch_device)
    on torch tensors; returns the label count, raises MBRWTError with .needed
    on MBRWT_ERR_CAPACITY."""
    need = C.c_uint64(0)
    st = getattr(L.lib(), fn)(
        h, rows_t.data_ptr(), rows_t.numel(), read_off_t.data_ptr(), read_off_t.numel() - 1,
        float(presence_ratio), lab_off_t.data_ptr(), labels_t.data_ptr() if labels_t is not None else None,
        labels_t.numel() if labels_t is not None else 0, C.byref(need), stream)
    if st == L.MBRWT_ERR_CAPACITY:
        e = L.MBRWTError(st, fn)
        e.needed = int(need.value)
        raise e
    L.check(st, fn)
    return int(need.value)


def _top_labels_batch_device(fn, h, rows_t, read_off_t, num_top, lab_off_t, labels_t, counts_t, stream):
    """Device-buffer batched get_top_labels through `fn`
    (mbrwt[_multi]_get_top_labels_batch_device); as _labels_batch_device."""
    need = C.c_uint64(0)
    out = labels_t is not None and counts_t is not None
    st = getattr(L.lib(), fn)(
        h, rows_t.data_ptr(), rows_t.numel(), read_off_t.data_ptr(), read_off_t.numel() - 1, int(num_top),
        lab_off_t.data_ptr(), labels_t.data_ptr() if out else None, counts_t.data_ptr() if out else None,
        min(labels_t.numel(), counts_t.numel()) if out else 0, C.byref(need), stream)
    if st == L.MBRWT_ERR_CAPACITY:
        e = L.MBRWTError(st, fn)
        e.needed = int(need.value)
        raise e
    L.check(st, fn)
    return int(need.value)


def tree_desc(tree):
    """mbrwt_tree_desc of a BFS tree dict (keys: num_rows, num_columns,
    num_children, first_child, leaf_column, vec_size, words); returns the
    struct and the arrays it points into (keep them alive while it is used)."""
    N = int(len(tree["num_children"]))
    nc = np.ascontiguousarray(tree["num_children"], dtype=np.uint32)
    fc = np.ascontiguousarray(tree["first_child"], dtype=np.uint32)
    lc = np.ascontiguousarray(tree["leaf_column"], dtype=np.uint32)
    vs = np.ascontiguousarray(tree["vec_size"], dtype=np.uint64)
    words = [np.ascontiguousarray(w, dtype=np.uint64) for w in tree["words"]]
    ptrs = (L.u64p * max(1, N))()
    for u, w in enumerate(words):
        ptrs[u] = _p(w, C.c_uint64) if w.size else None
    d = L.TreeDesc()
    d.num_rows = int(tree["num_rows"])
    d.num_columns = int(tree["num_columns"])
    d.num_nodes = N
    d.num_children = _p(nc, C.c_uint32)
    d.first_child = _p(fc, C.c_uint32)
    d.leaf_column = _p(lc, C.c_uint32)
    d.vec_size = _p(vs, C.c_uint64)
    d.vec_words = ptrs
    return d, (nc, fc, lc, vs, words, ptrs)


def _tree_dict(handle):
    """Copy an mbrwt_tree (include/mbrwt.h) into a BFS tree dict and free it."""
    lib = L.lib()
    try:
        d = lib.mbrwt_tree_get_desc(handle).contents
        N = int(d.num_nodes)
        out = dict(num_rows=int(d.num_rows), num_columns=int(d.num_columns), num_nodes=N)
        for key, dt in (("num_children", np.uint32), ("first_child", np.uint32), ("leaf_column", np.uint32),
                        ("vec_size", np.uint64)):
            ptr = getattr(d, key)
            out[key] = np.ctypeslib.as_array(ptr, shape=(N,)).astype(dt).copy() if N else np.zeros(0, dtype=dt)
        words = []
        for u in range(N):
            W = (int(out["vec_size"][u]) + 63) // 64
            words.append(np.ctypeslib.as_array(d.vec_words[u], shape=(W,)).copy() if W else
                         np.zeros(0, dtype=np.uint64))
        out["words"] = words
        return out
    finally:
        lib.mbrwt_tree_free(handle)


def parse_brwt(data: bytes):
    """BRWT::load (BRWT.cpp:87-111) of a reference BRWT stream -> (tree dict,
    bytes consumed).  Host only (include/mbrwt.h mbrwt_tree_parse)."""
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    h = C.c_void_p()
    used = C.c_uint64(0)
    L.check(L.lib().mbrwt_tree_parse(_p(buf, C.c_uint8), len(data), C.byref(used), C.byref(h)), "mbrwt_tree_parse")
    return _tree_dict(h), int(used.value)


def serialize_tree(tree) -> bytes:
    """BRWT::serialize (BRWT.cpp:113-128) of a tree dict.  Host only."""
    lib = L.lib()
    d, keep = tree_desc(tree)
    need = C.c_uint64(0)
    st = lib.mbrwt_tree_serialize(C.byref(d), None, 0, C.byref(need))
    if st != L.MBRWT_ERR_CAPACITY:
        L.check(st, "mbrwt_tree_serialize")
    buf = np.zeros(max(1, need.value), dtype=np.uint8)
    L.check(lib.mbrwt_tree_serialize(C.byref(d), _p(buf, C.c_uint8), len(buf), C.byref(need)), "mbrwt_tree_serialize")
    del keep
    return buf[: need.value].tobytes()


def basic_shape(num_columns, arity):
    """The shape of the basic partitioner's tree of `arity` over num_columns
    columns (mbrwt_tree_basic_shape; host only): the dict
    BRWTDevice.synthetic_shaped and BRWTDevice.from_rows take."""
    h = C.c_void_p()
    L.check(L.lib().mbrwt_tree_basic_shape(int(num_columns), int(arity), C.byref(h)), "mbrwt_tree_basic_shape")
    return _shape_dict(h)


def _shape_dict(handle):
    t = _tree_dict(handle)
    return dict(num_children=t["num_children"], first_child=t["first_child"], leaf_column=t["leaf_column"])


def _rows_desc(offsets, cols, num_columns):
    """mbrwt_rows_desc of a CSR and the arrays it points into."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    if off.size == 0:
        raise ValueError("offsets needs num_rows + 1 entries")
    cl = np.ascontiguousarray(cols, dtype=np.uint32)
    if cl.size == 0:
        cl = np.zeros(1, dtype=np.uint32)
    return L.RowsDesc(off.size - 1, int(num_columns), _p(off, C.c_uint64), _p(cl, C.c_uint32)), (off, cl)


def _shape_desc(shape):
    """mbrwt_shape_desc of a shape dict and the arrays it points into."""
    nc = np.ascontiguousarray(shape["num_children"], dtype=np.uint32)
    fc = np.ascontiguousarray(shape["first_child"], dtype=np.uint32)
    lc = np.ascontiguousarray(shape["leaf_column"], dtype=np.uint32)
    return L.ShapeDesc(len(nc), _p(nc, C.c_uint32), _p(fc, C.c_uint32), _p(lc, C.c_uint32)), (nc, fc, lc)


def _opt_shape_desc(shape):
    """(pointer to the mbrwt_shape_desc of `shape`, what it points into), or
    (None, None) without a shape."""
    if shape is None:
        return None, None
    s, keep = _shape_desc(shape)
    return C.byref(s), (s, keep)


def _node_counts(fn, make_desc, source, shape, arity, device):
    """The per-node row counts `fn` (mbrwt_rows_node_counts,
    mbrwt_sparse_columns_node_counts) gives on the matrix make_desc(*source)
    describes; num_columns is the last of `source`."""
    d, keep = make_desc(*source)
    sd, keep_s = _opt_shape_desc(shape)
    nodes = len((shape if shape is not None else basic_shape(source[-1], arity))["num_children"])
    counts = np.zeros(max(1, nodes), dtype=np.uint64)
    L.check(getattr(L.lib(), fn)(C.byref(d), sd, int(arity), device, _p(counts, C.c_uint64)), fn)
    del keep, keep_s
    return counts[:nodes]


def _shape_from(fn, make_desc, source, partitioner, arity, relax_max_arity, device):
    """The shape dict `fn` (mbrwt_tree_shape_from_rows,
    mbrwt_tree_shape_from_sparse_columns) gives on the matrix make_desc(*source) describes."""
    d, keep = make_desc(*source)
    part = L.PARTITIONERS[partitioner] if isinstance(partitioner, str) else int(partitioner)
    h = C.c_void_p()
    L.check(getattr(L.lib(), fn)(C.byref(d), part, int(arity), int(relax_max_arity), device, C.byref(h)), fn)
    del keep
    return _shape_dict(h)


def node_counts_from_rows(offsets, cols, num_columns, shape=None, arity=8, device=0):
    """Per BFS node of `shape` (None: basic_shape(num_columns, arity)) the
    number of CSR rows with a label below it (mbrwt_rows_node_counts): a
    leaf's column popcount, the root's non-empty rows.  uint64 array."""
    return _node_counts("mbrwt_rows_node_counts", _rows_desc, (offsets, cols, num_columns), shape, arity, device)


def relax_shape(shape, counts, max_arity):
    """BRWTOptimizer::relax(max_arity) of a shape dict given the per-node row
    counts of node_counts_from_rows (mbrwt_tree_relax_shape; host only)."""
    s, keep = _shape_desc(shape)
    cn = np.ascontiguousarray(counts, dtype=np.uint64)
    if cn.size < len(keep[0]):
        raise ValueError("counts needs one entry per node")
    if cn.size == 0:
        cn = np.zeros(1, dtype=np.uint64)
    h = C.c_void_p()
    L.check(L.lib().mbrwt_tree_relax_shape(C.byref(s), _p(cn, C.c_uint64), int(max_arity), C.byref(h)),
            "mbrwt_tree_relax_shape")
    del keep
    return _shape_dict(h)


def shape_from_rows(offsets, cols, num_columns, partitioner="basic", arity=8, relax_max_arity=0, device=0):
    """The shape the reference's builders give on the matrix of these CSR rows
    (mbrwt_tree_shape_from_rows): partitioner 'basic' (of `arity`) or 'greedy'
    (binary_grouping_greedy over the row sample), then BRWTOptimizer::relax
    over all rows when relax_max_arity > 1.  Returns the shape dict
    BRWTDevice.from_rows and BRWTDevice.synthetic_shaped take."""
    return _shape_from("mbrwt_tree_shape_from_rows", _rows_desc, (offsets, cols, num_columns), partitioner, arity,
                       relax_max_arity, device)


def _sparse_columns_desc(col_offsets, col_rows, num_rows, num_columns):
    """mbrwt_sparse_columns_desc and the arrays it points into: col_rows of
    dtype uint32 go in as rows32, anything else as uint64 rows."""
    off = np.ascontiguousarray(col_offsets, dtype=np.uint64)
    if off.size != int(num_columns) + 1:
        raise ValueError("col_offsets needs num_columns + 1 entries")
    rows = np.asarray(col_rows)
    narrow = rows.dtype == np.uint32
    rows = np.ascontiguousarray(rows, dtype=np.uint32 if narrow else np.uint64)
    if rows.size == 0:
        rows = np.zeros(1, dtype=rows.dtype)
    d = L.SparseColumnsDesc(int(num_rows), int(num_columns), _p(off, C.c_uint64),
                            None if narrow else _p(rows, C.c_uint64), _p(rows, C.c_uint32) if narrow else None)
    return d, (off, rows)


def node_counts_from_sparse_columns(col_offsets, col_rows, num_rows, num_columns, shape=None, arity=8, device=0):
    """node_counts_from_rows of the matrix given as sparse columns: column c
    holds the rows col_rows[col_offsets[c]:col_offsets[c + 1]], strictly
    ascending (mbrwt_sparse_columns_node_counts).  uint64 array."""
    return _node_counts("mbrwt_sparse_columns_node_counts", _sparse_columns_desc,
                        (col_offsets, col_rows, num_rows, num_columns), shape, arity, device)


def shape_from_sparse_columns(col_offsets, col_rows, num_rows, num_columns, partitioner="basic", arity=8,
                              relax_max_arity=0, device=0):
    """shape_from_rows of the matrix given as sparse columns
    (mbrwt_tree_shape_from_sparse_columns): the same shape dict, node for node."""
    return _shape_from("mbrwt_tree_shape_from_sparse_columns", _sparse_columns_desc,
                       (col_offsets, col_rows, num_rows, num_columns), partitioner, arity, relax_max_arity, device)


@contextlib.contextmanager
def build_layout(layout):
    """Device layout of the contexts created inside the block (None: the
    library default; 'nodes', 'rows', 'both' -- include/mbrwt.h)."""
    if layout is None:
        yield
        return
    with build_option(L.MBRWT_BUILD_LAYOUT, L.LAYOUTS[layout]):
        yield


@contextlib.contextmanager
def build_option(option, value):
    """mbrwt_set_build_option for the block; the calling thread's previous
    value is restored afterwards (mbrwt_get_build_option)."""
    lib = L.lib()
    prev = C.c_int64(0)
    L.check(lib.mbrwt_get_build_option(option, C.byref(prev)), "mbrwt_get_build_option")
    L.check(lib.mbrwt_set_build_option(option, int(value)), "mbrwt_set_build_option")
    try:
        yield
    finally:
        lib.mbrwt_set_build_option(option, prev.value)


class BRWTDevice:
    """A BRWT held in HBM; every query runs the HIP traversal kernels."""

    def __init__(self, handle, keepalive=None):
        self._h = handle
        self._keep = keepalive

    # -- construction -------------------------------------------------------
    @classmethod
    def from_tree(cls, tree, device=0, relax_max_arity=0, layout=None):
        """`tree`: BFS description (keys as include/mbrwt.h mbrwt_tree_desc:
        num_rows, num_columns, num_children, first_child, leaf_column,
        vec_size, words = list of uint64 arrays).  relax_max_arity > 1 runs
        BRWTOptimizer::relax on it first (mbrwt_create_relaxed)."""
        lib = L.lib()
        d, keep = tree_desc(tree)
        h = C.c_void_p()
        with build_layout(layout):
            if relax_max_arity:
                L.check(lib.mbrwt_create_relaxed(C.byref(d), int(relax_max_arity), device, C.byref(h)),
                        "mbrwt_create_relaxed")
            else:
                L.check(lib.mbrwt_create(C.byref(d), device, C.byref(h)), "mbrwt_create")
        return cls(h)

    @classmethod
    def synthetic(cls, num_rows, num_columns, density, arity=8, seed=42, device=0, layout=None):
        lib = L.lib()
        d = L.SynthDesc(num_rows, num_columns, float(density), arity, seed)
        h = C.c_void_p()
        with build_layout(layout):
            L.check(lib.mbrwt_create_synthetic(C.byref(d), device, C.byref(h)), "mbrwt_create_synthetic")
        return cls(h)

    @classmethod
    def synthetic_shaped(cls, num_rows, shape, density, seed=42, device=0, layout=None):
        """The synthetic law over a given tree shape (mbrwt_create_synthetic_shaped):
        `shape` = dict with num_children, first_child, leaf_column (BFS), e.g.
        the export of a greedy + relaxed tree."""
        sd, keep = _shape_desc(shape)
        m = int((keep[0] == 0).sum())
        d = L.SynthDesc(num_rows, m, float(density), 0, seed)
        h = C.c_void_p()
        with build_layout(layout):
            L.check(L.lib().mbrwt_create_synthetic_shaped(C.byref(d), C.byref(sd), device, C.byref(h)),
                    "mbrwt_create_synthetic_shaped")
        del keep
        return cls(h)

    @classmethod
    def from_columns(cls, columns, num_rows, arity=2, device=0, relax_max_arity=0, layout=None,
                     partitioner="basic"):
        """BRWTBottomUpBuilder::build on the device (include/mbrwt.h
        mbrwt_create_from_columns) with the basic partitioner of `arity` or,
        partitioner='greedy', binary_grouping_greedy (MBRWT_BUILD_PARTITIONER).
        `columns`: a sequence of uint64 arrays (ceil(num_rows/64) LSB-first
        words each), or a 2-D uint64 array [num_columns, words].
        relax_max_arity > 1 then runs BRWTOptimizer::relax
        (mbrwt_create_from_columns_relaxed)."""
        lib = L.lib()
        cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in columns]
        W = (num_rows + 63) // 64
        if any(len(c) < W for c in cols):
            raise ValueError("a column has fewer than ceil(num_rows/64) words")
        ptrs = (L.u64p * max(1, len(cols)))()
        for j, c in enumerate(cols):
            ptrs[j] = c.ctypes.data_as(L.u64p)
        d = L.ColumnsDesc(num_rows, len(cols), ptrs, arity)
        h = C.c_void_p()
        with build_option(L.MBRWT_BUILD_PARTITIONER, L.PARTITIONERS[partitioner]), build_layout(layout):
            if relax_max_arity:
                L.check(lib.mbrwt_create_from_columns_relaxed(C.byref(d), int(relax_max_arity), device,
                                                              C.byref(h)), "mbrwt_create_from_columns_relaxed")
            else:
                L.check(lib.mbrwt_create_from_columns(C.byref(d), device, C.byref(h)), "mbrwt_create_from_columns")
        return cls(h)

    @classmethod
    def from_rows(cls, offsets, cols, num_columns, arity=8, shape=None, device=0, partitioner="basic",
                  relax_max_arity=0):
        """Row records straight from CSR rows (mbrwt_create_from_rows): row r
        carries the columns cols[offsets[r]:offsets[r + 1]] (a set, any
        order).  `shape` = dict with num_children, first_child, leaf_column
        (BFS; e.g. shape_from_rows of the same rows), or None for the basic
        partitioner's tree of `arity` (basic_shape).  partitioner='greedy' or
        relax_max_arity > 1: the shape is shape_from_rows(...) of these rows
        (not together with `shape`).  No node image and no dense column is
        built; the context's layout is 'rows'."""
        return cls._from_source("mbrwt_create_from_rows", shape_from_rows, _rows_desc, (offsets, cols, num_columns),
                                arity, shape, device, partitioner, relax_max_arity)

    @classmethod
    def from_sparse_columns(cls, col_offsets, col_rows, num_rows, num_columns, arity=8, shape=None, device=0,
                            partitioner="basic", relax_max_arity=0):
        """Row records from sparse columns (mbrwt_create_from_sparse_columns):
        column c holds the rows col_rows[col_offsets[c]:col_offsets[c + 1]],
        strictly ascending (uint32 ids go in as they are, others as uint64).
        `shape`, `arity`, `partitioner` and `relax_max_arity` as in from_rows
        (the shape computed by shape_from_sparse_columns); the context equals
        from_rows of the same matrix."""
        return cls._from_source("mbrwt_create_from_sparse_columns", shape_from_sparse_columns, _sparse_columns_desc,
                                (col_offsets, col_rows, num_rows, num_columns), arity, shape, device, partitioner,
                                relax_max_arity)

    @classmethod
    def _from_source(cls, fn, shape_of, make_desc, source, arity, shape, device, partitioner, relax_max_arity):
        """from_rows / from_sparse_columns: the context `fn` builds of the matrix
        make_desc(*source) describes, under `shape` or the shape shape_of computes."""
        if partitioner != "basic" or relax_max_arity:
            if shape is not None:
                raise ValueError("give a shape, or a partitioner / relax_max_arity to compute one: not both")
            shape = shape_of(*source, partitioner, arity, relax_max_arity, device)
            if len(shape["num_children"]) == 0:  # no column: the call below builds the empty context
                shape = None
        d, keep = make_desc(*source)
        sd, keep_s = _opt_shape_desc(shape)
        h = C.c_void_p()
        L.check(getattr(L.lib(), fn)(C.byref(d), sd, int(arity), device, C.byref(h)), fn)
        del keep, keep_s
        return cls(h)

    @classmethod
    def load(cls, data: bytes, device=0, layout=None):
        """BRWT::load of a reference BRWT stream into HBM (mbrwt_load)."""
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
        h = C.c_void_p()
        with build_layout(layout):
            L.check(L.lib().mbrwt_load(_p(buf, C.c_uint8), len(data), None, device, C.byref(h)), "mbrwt_load")
        return cls(h)

    def export(self):
        """The tree this context holds, read back from its device image
        (mbrwt_tree_export), as a BFS tree dict."""
        h = C.c_void_p()
        L.check(L.lib().mbrwt_tree_export(self._h, C.byref(h)), "mbrwt_tree_export")
        return _tree_dict(h)

    def serialize(self) -> bytes:
        """BRWT::serialize (BRWT.cpp:113-128) of this matrix."""
        return serialize_tree(self.export())

    def clone(self) -> "BRWTDevice":
        """A second query context over the same device image
        (mbrwt_ctx_clone): its own workspaces, so its queries may run
        concurrently with this one's on another stream or thread."""
        h = C.c_void_p()
        L.check(L.lib().mbrwt_ctx_clone(self._h, C.byref(h)), "mbrwt_ctx_clone")
        return BRWTDevice(h.value)

    def close(self):
        if getattr(self, "_h", None):
            L.lib().mbrwt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- properties -----------------------------------------------------------
    def num_rows(self):
        return L.lib().mbrwt_num_rows(self._h)

    def num_columns(self):
        return L.lib().mbrwt_num_columns(self._h)

    def num_relations(self):
        return L.lib().mbrwt_num_relations(self._h)

    def num_nodes(self):
        return L.lib().mbrwt_num_nodes(self._h)

    def num_shards(self):
        """Row shards of the context (1 below 2^32 rows; include/mbrwt.h)."""
        return L.lib().mbrwt_num_shards(self._h)

    def device_bytes(self):
        return L.lib().mbrwt_device_bytes(self._h)

    def layout(self):
        """'nodes', 'rows' or 'both' (include/mbrwt.h "device layout")."""
        return L.LAYOUT_NAMES.get(L.lib().mbrwt_layout(self._h), "?")

    def rows_stats(self):
        """The row-record image (mbrwt_rows_stats) as a dict, None without one."""
        out = (C.c_uint64 * 8)()
        if L.lib().mbrwt_rows_stats(self._h, out) != L.MBRWT_OK:
            return None
        keys = ("block_bytes", "rows_per_block", "blocks_bytes", "spill_bytes", "record_bytes", "spilled_rows",
                "long_rows", "height")
        d = dict(zip(keys, [int(v) for v in out]))
        d["uniform_levels"] = (d["height"] >> 32) & 0xFF  # odometer walk when > 0
        d["nibble_codes"] = bool((d["height"] >> 40) & 1)  # masks as nibble codes (MBRWT_BUILD_ROWS_CODE)
        d["terminal_records"] = bool((d["height"] >> 41) & 1)  # terminal records (MBRWT_BUILD_ROWS_CODE = 2)
        d["variable"] = d["block_bytes"] == 0  # variable-length records (csrc/rows_var.hip)
        d["height"] &= 0xFFFFFFFF
        cl = (C.c_uint64 * 4)()
        if L.lib().mbrwt_rows_classes(self._h, cl) == L.MBRWT_OK:
            # record classes (csrc/rows_class.hip): 0 = none
            d["classes"], d["class_bits"], d["class_index_bytes"], d["class_sample_distinct"] = (int(v) for v in cl)
        return d

    def node_info(self, dnode, shard=0):
        """What was built for device node `dnode` of the per-node images
        (mbrwt_node_info; diagnostics, launches nothing): a dict of kind (a
        name of _lib.NODE_KIND_NAMES), arity, stride and length.  dnode 0 is
        the super-root, dnode u + 1 is node u of the tree description; `shard`
        picks the row shard of a sharded context."""
        out = (C.c_uint64 * 4)()
        L.check(L.lib().mbrwt_node_info(self._h, int(shard), int(dnode), out), "mbrwt_node_info")
        return {"kind": L.NODE_KIND_NAMES.get(int(out[0]), "?"), "arity": int(out[1]), "stride": int(out[2]),
                "length": int(out[3])}

    # -- host-buffer queries --------------------------------------------------
    def get_rows(self, rows):
        """Batched BRWT::get_row (BRWT.cpp:26-53) -> (offsets[n+1], cols)."""
        lib = L.lib()
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n = len(rows)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        need = C.c_uint64(0)
        cap = max(16, n * 16)
        while True:
            cols = np.zeros(cap, dtype=np.uint32)
            st = lib.mbrwt_get_rows(self._h, _p(rows, C.c_uint64), n, _p(offsets, C.c_uint64),
                                    _p(cols, C.c_uint32), cap, C.byref(need))
            if st == L.MBRWT_ERR_CAPACITY:
                cap = int(need.value)
                continue
            L.check(st, "mbrwt_get_rows")
            return offsets, cols[: need.value]

    def get_rows16(self, rows):
        """get_rows with 16-bit labels (mbrwt_get_rows16; at most 65,536
        columns) -> (offsets[n+1] uint64, cols uint16)."""
        lib = L.lib()
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n = len(rows)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        need = C.c_uint64(0)
        cap = max(16, n * 16)
        while True:
            cols = np.zeros(cap, dtype=np.uint16)
            st = lib.mbrwt_get_rows16(self._h, _p(rows, C.c_uint64), n, _p(offsets, C.c_uint64),
                                      _p(cols, C.c_uint16), cap, C.byref(need))
            if st == L.MBRWT_ERR_CAPACITY:
                cap = int(need.value)
                continue
            L.check(st, "mbrwt_get_rows16")
            return offsets, cols[: need.value]

    def get_row(self, row):
        off, cols = self.get_rows(np.array([row], dtype=np.uint64))
        return cols.tolist()

    def get_batch(self, rows, cols):
        """Batched BRWT::get (BRWT.cpp:9-24)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        out = np.zeros(max(1, len(rows)), dtype=np.uint8)
        L.check(L.lib().mbrwt_get_batch(self._h, _p(rows, C.c_uint64), _p(cols, C.c_uint64), len(rows),
                                        _p(out, C.c_uint8)), "mbrwt_get_batch")
        return out[: len(rows)].astype(bool)

    def get(self, row, col):
        return bool(self.get_batch([row], [col])[0])

    def get_column(self, col):
        """BRWT::get_column (BRWT.cpp:55-85): ascending rows carrying `col`."""
        need = C.c_uint64(0)
        st = L.lib().mbrwt_get_column(self._h, int(col), None, 0, C.byref(need))
        if st != L.MBRWT_ERR_CAPACITY:
            L.check(st, "mbrwt_get_column")
            return np.zeros(0, dtype=np.uint64)
        out = np.zeros(max(1, need.value), dtype=np.uint64)
        L.check(L.lib().mbrwt_get_column(self._h, int(col), _p(out, C.c_uint64), len(out), C.byref(need)),
                "mbrwt_get_column")
        return out[: need.value]

    def get_column_device(self, col, rows_t, stream=None):
        """Device variant: rows_t = 64-bit cuda tensor of capacity >= the column's
        size.  Returns the number of rows written; raises on capacity."""
        need = C.c_uint64(0)
        st = L.lib().mbrwt_get_column_device(self._h, int(col), rows_t.data_ptr(), rows_t.numel(), C.byref(need),
                                             stream if stream is not None else None)
        if st == L.MBRWT_ERR_CAPACITY:
            e = L.MBRWTError(st, "mbrwt_get_column_device")
            e.needed = int(need.value)
            raise e
        L.check(st, "mbrwt_get_column_device")
        return int(need.value)

    def _columns_arg(self, columns):
        # (columns array or None, its ctypes pointer or None, n_columns)
        if columns is None:
            return None, None, self.num_columns()
        columns = np.ascontiguousarray(columns, dtype=np.uint64)
        return columns, _p(columns, C.c_uint64), len(columns)

    def get_columns(self, columns=None, row_begin=0, row_end=None):
        """mbrwt_get_columns: the sparse columns of the rows [row_begin,
        row_end) as (offsets u64 [n_columns + 1], rows u64) -- slot j's
        ascending absolute row ids are rows[offsets[j]:offsets[j + 1]], in the
        caller's order of `columns` (None: every column in order).  The sizing
        call, then the filling call."""
        columns, cp, k = self._columns_arg(columns)
        row_end = self.num_rows() if row_end is None else int(row_end)
        offsets = np.zeros(k + 1, dtype=np.uint64)
        need = C.c_uint64(0)
        st = L.lib().mbrwt_get_columns(self._h, cp, k, int(row_begin), row_end, _p(offsets, C.c_uint64), None, 0,
                                       C.byref(need))
        if st != L.MBRWT_ERR_CAPACITY:
            L.check(st, "mbrwt_get_columns")
            return offsets, np.zeros(0, dtype=np.uint64)
        out = np.zeros(max(1, need.value), dtype=np.uint64)
        L.check(L.lib().mbrwt_get_columns(self._h, cp, k, int(row_begin), row_end, _p(offsets, C.c_uint64),
                                          _p(out, C.c_uint64), len(out), C.byref(need)), "mbrwt_get_columns")
        return offsets, out[: need.value]

    def get_columns_device(self, columns, row_begin, row_end, offsets_t, rows_t, stream=None):
        """Device variant: `columns` stays a host array (or None); offsets_t =
        64-bit cuda tensor [n_columns + 1], rows_t = 64-bit cuda tensor of
        capacity >= the total (None: size only).  Returns the total; raises on
        capacity with .needed set (offsets_t is complete then)."""
        columns, cp, k = self._columns_arg(columns)
        row_end = self.num_rows() if row_end is None else int(row_end)
        need = C.c_uint64(0)
        st = L.lib().mbrwt_get_columns_device(self._h, cp, k, int(row_begin), row_end, offsets_t.data_ptr(),
                                              rows_t.data_ptr() if rows_t is not None else None,
                                              rows_t.numel() if rows_t is not None else 0, C.byref(need),
                                              stream if stream is not None else None)
        if st == L.MBRWT_ERR_CAPACITY:
            e = L.MBRWTError(st, "mbrwt_get_columns_device")
            e.needed = int(need.value)
            raise e
        L.check(st, "mbrwt_get_columns_device")
        return int(need.value)

    def to_sparse_columns(self):
        """The whole matrix as (col_offsets, col_rows): what from_sparse_columns
        and shape_from_sparse_columns take."""
        return self.get_columns()

    # -- device-buffer queries (torch tensors as plumbing) ---------------------
    def get_rows_device(self, rows_t, offsets_t, cols_t, stream=None):
        """rows_t: uint64/int64 cuda tensor [n]; offsets_t: [n+1] 64-bit; cols_t:
        int32 [cap].  Returns the number of labels; raises on capacity."""
        need = C.c_uint64(0)
        st = L.lib().mbrwt_get_rows_device(self._h, rows_t.data_ptr(), rows_t.numel(), offsets_t.data_ptr(),
                                           cols_t.data_ptr(), cols_t.numel(), C.byref(need),
                                           stream if stream is not None else None)
        if st == L.MBRWT_ERR_CAPACITY:
            e = L.MBRWTError(st, "mbrwt_get_rows_device")
            e.needed = int(need.value)
            raise e
        L.check(st, "mbrwt_get_rows_device")
        return int(need.value)

    def get_rows_device_async(self, rows_t, offsets_t, cols_t, status_t, stream=None):
        """mbrwt_get_rows_device_async: enqueue only; status_t (device, 3 x
        int64) receives {labels needed, status, sticky status bits}."""
        L.check(L.lib().mbrwt_get_rows_device_async(self._h, rows_t.data_ptr(), rows_t.numel(), offsets_t.data_ptr(),
                                                    cols_t.data_ptr(), cols_t.numel(), status_t.data_ptr(), stream),
                "mbrwt_get_rows_device_async")

    @staticmethod
    def _cols16(cols_t):
        # torch's uint16 support is partial: int16 on the device, viewed as uint16 in numpy
        if cols_t is None:  # count only
            return None, 0
        if str(cols_t.dtype) != "torch.int16":
            raise TypeError(f"cols_t must be a torch.int16 tensor (u16 labels), not {cols_t.dtype}")
        return cols_t.data_ptr(), cols_t.numel()

    def get_rows16_device(self, rows_t, offsets_t, cols_t, stream=None):
        """get_rows_device with 16-bit labels: cols_t is an int16 [cap] cuda
        tensor (None: count only), any 2-byte alignment.  Returns the number
        of labels; raises on capacity."""
        ptr, cap = self._cols16(cols_t)
        need = C.c_uint64(0)
        st = L.lib().mbrwt_get_rows16_device(self._h, rows_t.data_ptr(), rows_t.numel(), offsets_t.data_ptr(),
                                             ptr, cap, C.byref(need), stream if stream is not None else None)
        if st == L.MBRWT_ERR_CAPACITY:
            e = L.MBRWTError(st, "mbrwt_get_rows16_device")
            e.needed = int(need.value)
            raise e
        L.check(st, "mbrwt_get_rows16_device")
        return int(need.value)

    def get_rows16_device_async(self, rows_t, offsets_t, cols_t, status_t, stream=None):
        """get_rows_device_async with 16-bit labels (cols_t: int16 [cap])."""
        ptr, cap = self._cols16(cols_t)
        L.check(L.lib().mbrwt_get_rows16_device_async(self._h, rows_t.data_ptr(), rows_t.numel(),
                                                      offsets_t.data_ptr(), ptr, cap, status_t.data_ptr(), stream),
                "mbrwt_get_rows16_device_async")

    def get_batch_device(self, rows_t, cols_t, out_t, stream=None):
        L.check(L.lib().mbrwt_get_batch_device(self._h, rows_t.data_ptr(), cols_t.data_ptr(), rows_t.numel(),
                                               out_t.data_ptr(), stream), "mbrwt_get_batch_device")

    def count_labels_device(self, rows_t, counts_t, stream=None):
        L.check(L.lib().mbrwt_count_labels_device(self._h, rows_t.data_ptr(), rows_t.numel(), counts_t.data_ptr(),
                                                  stream), "mbrwt_count_labels_device")

    def get_labels_batch_device(self, rows_t, read_off_t, presence_ratio, lab_off_t, labels_t, stream=None):
        """get_labels(indices, presence_ratio) for many reads (include/mbrwt.h
        mbrwt_get_labels_batch_device); torch device tensors; returns the
        label count (raises MBRWTError with .needed on MBRWT_ERR_CAPACITY)."""
        return _labels_batch_device("mbrwt_get_labels_batch_device", self._h, rows_t, read_off_t, presence_ratio,
                                    lab_off_t, labels_t, stream)

    def get_labels_batch(self, rows, read_offsets, presence_ratio):
        """Host-buffer form (include/mbrwt.h mbrwt_get_labels_batch): numpy in,
        (label offsets u64 [n_reads+1], labels u32) out."""
        return _labels_batch("mbrwt_get_labels_batch", self._h, rows, read_offsets, presence_ratio)

    def get_top_labels_batch(self, rows, read_offsets, num_top=2**64 - 1):
        """MultiLabelEncoded::get_top_labels(indices, num_top) for many reads
        (include/mbrwt.h mbrwt_get_top_labels_batch): -> (label offsets u64
        [n_reads+1], labels u32, counts u64), each read by count descending,
        equal counts by label ascending."""
        return _top_labels_batch("mbrwt_get_top_labels_batch", self._h, rows, read_offsets, num_top)

    def get_top_labels_batch_device(self, rows_t, read_off_t, num_top, lab_off_t, labels_t, counts_t, stream=None):
        """Device-buffer form on torch tensors (labels int32, counts int64);
        returns the label count (raises MBRWTError with .needed on capacity)."""
        return _top_labels_batch_device("mbrwt_get_top_labels_batch_device", self._h, rows_t, read_off_t, num_top,
                                        lab_off_t, labels_t, counts_t, stream)

    def count_work_device(self, rows_t, stream=None):
        v = C.c_uint64(0)
        lab = C.c_uint64(0)
        L.check(L.lib().mbrwt_count_work_device(self._h, rows_t.data_ptr(), rows_t.numel(), C.byref(v),
                                                C.byref(lab), stream), "mbrwt_count_work_device")
        return int(v.value), int(lab.value)

    # -- options / measurement ------------------------------------------------
    def set_option(self, option, value):
        L.check(L.lib().mbrwt_set_option(self._h, option, int(value)), "mbrwt_set_option")

    def traverse_kernel(self) -> str:
        """Name of the traversal kernel get_rows launches (diagnostics)."""
        return (L.lib().mbrwt_traverse_kernel(self._h) or b"").decode()

    def overflow_rows(self) -> int:
        """Rows the last get_rows*_device* call on the node images left to its direct pass (diagnostics)."""
        return int(L.lib().mbrwt_overflow_rows(self._h))

    def take_timing(self):
        ms = C.c_double(0)
        k = C.c_uint64(0)
        L.check(L.lib().mbrwt_take_timing(self._h, C.byref(ms), C.byref(k)), "mbrwt_take_timing")
        return ms.value, int(k.value)


class BRWTMulti:
    """One replica per device (include/mbrwt.h "multi-device").  get_rows: the
    batch is cut into contiguous slices, one per replica, and reassembled into
    one CSR.  get_labels_batch / get_top_labels_batch: the batch is cut
    between reads, every replica classifies its reads on its device, and only
    the reads' labels are gathered."""

    def __init__(self, handle, keepalive=None):
        self._h = handle
        self._keep = keepalive

    @classmethod
    def from_tree(cls, tree, devices=(0,), layout=None):
        lib = L.lib()
        d, keep = tree_desc(tree)
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        with build_layout(layout):
            L.check(lib.mbrwt_multi_create(C.byref(d), devs, len(devices), C.byref(h)), "mbrwt_multi_create")
        return cls(h)

    @classmethod
    def synthetic(cls, num_rows, num_columns, density, arity=8, seed=42, devices=(0,), layout=None):
        lib = L.lib()
        d = L.SynthDesc(num_rows, num_columns, float(density), arity, seed)
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        with build_layout(layout):
            L.check(lib.mbrwt_multi_create_synthetic(C.byref(d), devs, len(devices), C.byref(h)),
                    "mbrwt_multi_create_synthetic")
        return cls(h)

    def close(self):
        if getattr(self, "_h", None):
            L.lib().mbrwt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return L.lib().mbrwt_multi_size(self._h)

    def replica(self, i):
        """Replica i as a BRWTDevice view (owned by this handle)."""
        h = L.lib().mbrwt_multi_replica(self._h, i)
        if not h:
            raise IndexError(i)
        dev = BRWTDevice.__new__(BRWTDevice)
        dev._h = C.c_void_p(h)
        dev._keep = self
        dev.close = lambda: None  # the multi handle owns it
        return dev

    def get_rows(self, rows):
        lib = L.lib()
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n = len(rows)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        need = C.c_uint64(0)
        cap = max(16, n * 16)
        while True:
            cols = np.zeros(cap, dtype=np.uint32)
            st = lib.mbrwt_multi_get_rows(self._h, _p(rows, C.c_uint64), n, _p(offsets, C.c_uint64),
                                          _p(cols, C.c_uint32), cap, C.byref(need))
            if st == L.MBRWT_ERR_CAPACITY:
                cap = int(need.value)
                continue
            L.check(st, "mbrwt_multi_get_rows")
            return offsets, cols[: need.value]

    def get_rows_device(self, rows_t, offsets_t, cols_t, stream=None):
        need = C.c_uint64(0)
        st = L.lib().mbrwt_multi_get_rows_device(self._h, rows_t.data_ptr(), rows_t.numel(), offsets_t.data_ptr(),
                                                 cols_t.data_ptr(), cols_t.numel(), C.byref(need), stream)
        if st == L.MBRWT_ERR_CAPACITY:
            e = L.MBRWTError(st, "mbrwt_multi_get_rows_device")
            e.needed = int(need.value)
            raise e
        L.check(st, "mbrwt_multi_get_rows_device")
        return int(need.value)

    # -- batched classify: arguments and results as the BRWTDevice methods ------
    def get_labels_batch(self, rows, read_offsets, presence_ratio):
        return _labels_batch("mbrwt_multi_get_labels_batch", self._h, rows, read_offsets, presence_ratio)

    def get_top_labels_batch(self, rows, read_offsets, num_top=2**64 - 1):
        return _top_labels_batch("mbrwt_multi_get_top_labels_batch", self._h, rows, read_offsets, num_top)

    def get_labels_batch_device(self, rows_t, read_off_t, presence_ratio, lab_off_t, labels_t, stream=None):
        """Tensors on devices[0], ordered on `stream`; complete on return."""
        return _labels_batch_device("mbrwt_multi_get_labels_batch_device", self._h, rows_t, read_off_t,
                                    presence_ratio, lab_off_t, labels_t, stream)

    def get_top_labels_batch_device(self, rows_t, read_off_t, num_top, lab_off_t, labels_t, counts_t, stream=None):
        return _top_labels_batch_device("mbrwt_multi_get_top_labels_batch_device", self._h, rows_t, read_off_t,
                                        num_top, lab_off_t, labels_t, counts_t, stream)
