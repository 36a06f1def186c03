"""mbrwt_get_columns / mbrwt_get_columns_device without a GPU: the symbols and
their argument types, the null-argument statuses (checked before any HIP
call) and the chunk test hook's value."""
import ctypes as C

import numpy as np


def test_symbols_and_argument_types():
    from genome_graph_annotation_amd import _lib as L
    lib = L.lib()
    u64p = C.POINTER(C.c_uint64)
    host = lib.mbrwt_get_columns
    assert host.restype is C.c_int
    assert list(host.argtypes) == [C.c_void_p, u64p, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, C.c_uint64, u64p]
    dev = lib.mbrwt_get_columns_device
    assert dev.restype is C.c_int
    assert list(dev.argtypes) == [C.c_void_p, u64p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                  C.c_uint64, u64p, C.c_void_p]


def test_option_constant():
    from genome_graph_annotation_amd import _lib as L
    assert L.MBRWT_OPT_COLUMNS_CHUNK == 128


def test_null_context_is_invalid():
    from genome_graph_annotation_amd import _lib as L
    lib = L.lib()
    offsets = np.zeros(2, dtype=np.uint64)
    rows = np.zeros(4, dtype=np.uint64)
    cols = np.zeros(1, dtype=np.uint64)
    need = C.c_uint64(7)
    u64p = C.POINTER(C.c_uint64)
    assert lib.mbrwt_get_columns(None, cols.ctypes.data_as(u64p), 1, 0, 0, offsets.ctypes.data_as(u64p),
                                 rows.ctypes.data_as(u64p), 4, C.byref(need)) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_get_columns(None, None, 0, 0, 0, None, None, 0, None) == L.MBRWT_ERR_INVALID
    assert lib.mbrwt_get_columns_device(None, cols.ctypes.data_as(u64p), 1, 0, 0, None, None, 0, C.byref(need),
                                        None) == L.MBRWT_ERR_INVALID
    assert need.value == 7 and not offsets.any() and not rows.any()


def test_stand_alone_argument_checks():
    """tests/cpp/get_columns/args_host.cpp: the same statuses from a C++ program
    of its own (the program `make sanitize` builds with ASan / UBSan)."""
    import os
    import subprocess
    cpp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "cpp", "get_columns")
    subprocess.run(["make", "-s", "-C", cpp, "_build/args_host"], check=True)
    r = subprocess.run([os.path.join(cpp, "_build", "args_host")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 failed" in r.stdout, r.stdout + r.stderr
