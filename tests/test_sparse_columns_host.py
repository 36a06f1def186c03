"""The host side of the build from sparse columns, without a GPU:
tests/cpp/from_sparse_columns/cols_host.cpp over csrc/cols_host.hpp (the slice
cutter, the staging, the sample intersection, the range sizing at 2^31 - 1
labels and one more) and the null-argument statuses of the three entry
points, from C++ and from Python."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "from_sparse_columns")


def test_cols_host_program():
    subprocess.run(["make", "-s", "-C", CPP, "_build/cols_host"], check=True)
    r = subprocess.run([os.path.join(CPP, "_build", "cols_host")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cols_host ok" in r.stdout, r.stdout


def test_null_arguments_need_no_gpu():
    from genome_graph_annotation_amd import _lib as L
    lib = L.lib()
    off = np.array([0, 1, 2], dtype=np.uint64)
    rows = np.array([0, 1], dtype=np.uint64)
    d = L.SparseColumnsDesc(4, 2, off.ctypes.data_as(L.u64p), rows.ctypes.data_as(L.u64p), None)
    h = C.c_void_p()
    counts = np.zeros(8, dtype=np.uint64)
    assert lib.mbrwt_create_from_sparse_columns(None, None, 8, 0, C.byref(h)) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_last_error_message()
    assert lib.mbrwt_create_from_sparse_columns(C.byref(d), None, 8, 0, None) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_sparse_columns_node_counts(None, None, 8, 0, counts.ctypes.data_as(L.u64p)) == \
        L.MBRWT_ERR_INVALID
    assert lib.mbrwt_sparse_columns_node_counts(C.byref(d), None, 8, 0, None) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_tree_shape_from_sparse_columns(None, 0, 8, 0, 0, C.byref(h)) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_tree_shape_from_sparse_columns(C.byref(d), 0, 8, 0, 0, None) == L.MBRWT_ERR_INVALID
    assert not h.value


def test_wrapper_picks_the_pointer_by_dtype():
    from genome_graph_annotation_amd.brwt import _sparse_columns_desc
    off = np.array([0, 1, 2], dtype=np.uint64)
    d, keep = _sparse_columns_desc(off, np.array([0, 1], dtype=np.uint32), 4, 2)
    assert not d.rows and d.rows32 and keep[1].dtype == np.uint32
    d, keep = _sparse_columns_desc(off, [0, 1], 4, 2)
    assert d.rows and not d.rows32 and keep[1].dtype == np.uint64
