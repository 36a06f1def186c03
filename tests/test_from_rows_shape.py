"""mbrwt_tree_basic_shape (host only) against the oracle's basic-partitioner
tree, and the no-GPU error paths of mbrwt_create_from_rows."""
import ctypes as C

import numpy as np
import pytest

MS = list(range(1, 131)) + [255, 256, 257, 513]
ARITIES = [2, 3, 8, 9, 64]


@pytest.mark.parametrize("arity", ARITIES)
def test_basic_shape_equals_the_oracle_tree(oracle_mod, arity):
    """Every m: leaves at mixed depths wherever a level ends in a group of one."""
    from genome_graph_annotation_amd.brwt import basic_shape
    for m in MS:
        want = oracle_mod.OracleTree.from_dense(np.zeros((1, m), dtype=bool), "basic", arity).export()
        got = basic_shape(m, arity)
        for key in ("num_children", "first_child", "leaf_column"):
            assert np.array_equal(np.asarray(got[key], dtype=np.uint32), want[key]), (m, arity, key)


def test_basic_shape_tree_is_owned_and_empty_of_data():
    from genome_graph_annotation_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    assert lib.mbrwt_tree_basic_shape(17, 4, C.byref(h)) == L.MBRWT_OK
    try:
        d = lib.mbrwt_tree_get_desc(h).contents
        assert d.num_columns == 17 and d.num_rows == 0
        N = int(d.num_nodes)
        nc = np.ctypeslib.as_array(d.num_children, shape=(N,))
        assert int((nc == 0).sum()) == 17
        assert all(int(d.vec_size[u]) == 0 for u in range(N))
    finally:
        lib.mbrwt_tree_free(h)
    h = C.c_void_p()
    assert lib.mbrwt_tree_basic_shape(0, 2, C.byref(h)) == L.MBRWT_OK
    assert lib.mbrwt_tree_get_desc(h).contents.num_nodes == 0
    lib.mbrwt_tree_free(h)


@pytest.mark.parametrize("arity", [0, 1, 65])
def test_basic_shape_arity_errors(arity):
    from genome_graph_annotation_amd import _lib as L
    h = C.c_void_p()
    assert L.lib().mbrwt_tree_basic_shape(10, arity, C.byref(h)) == L.MBRWT_ERR_INVALID
    assert not h.value
    assert L.lib().mbrwt_tree_basic_shape(10, 2, None) == L.MBRWT_ERR_INVALID


def test_create_from_rows_null_arguments_need_no_gpu():
    from genome_graph_annotation_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    assert lib.mbrwt_create_from_rows(None, None, 8, 0, C.byref(h)) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_last_error_message()
    off = np.zeros(2, dtype=np.uint64)
    cols = np.zeros(1, dtype=np.uint32)
    d = L.RowsDesc(1, 4, off.ctypes.data_as(L.u64p), cols.ctypes.data_as(L.u32p))
    assert lib.mbrwt_create_from_rows(C.byref(d), None, 8, 0, None) == L.MBRWT_ERR_INVALID
