"""The multi-device classify entry points (include/mbrwt.h "multi-device")
validate their arguments before any HIP call: a null handle is
MBRWT_ERR_INVALID with or without a GPU."""
import ctypes as C


def test_multi_classify_null_handle_fails_cleanly():
    from genome_graph_annotation_amd import _lib as L
    lib = L.lib()
    rows = (C.c_uint64 * 2)(0, 1)
    roff = (C.c_uint64 * 2)(0, 2)
    loff = (C.c_uint64 * 2)()
    labs = (C.c_uint32 * 4)()
    cnts = (C.c_uint64 * 4)()
    need = C.c_uint64(7)
    assert lib.mbrwt_multi_get_labels_batch(None, None, 0, None, 0, 0.5, None, None, 0, None) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_multi_get_labels_batch(None, rows, 2, roff, 1, 0.5, loff, labs, 4,
                                            C.byref(need)) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_multi_get_labels_batch_device(None, None, 0, None, 0, 0.5, None, None, 0, None,
                                                   None) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_multi_get_top_labels_batch(None, None, 0, None, 0, 3, None, None, None, 0,
                                                None) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_multi_get_top_labels_batch(None, rows, 2, roff, 1, 3, loff, labs, cnts, 4,
                                                C.byref(need)) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_multi_get_top_labels_batch_device(None, None, 0, None, 0, 3, None, None, None, 0, None,
                                                       None) == L.MBRWT_ERR_INVALID
    assert need.value == 7  # nothing written
    assert b"invalid argument" in lib.mbrwt_last_error_message()
