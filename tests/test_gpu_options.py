"""The option contract of MBRWT_OPT_KERNEL and the timing / status plumbing
that the three get_rows drivers (node images, row records, variable-length
records) share: values accepted and rejected, launches and milliseconds
counted per call, return codes and messages of the ordinary API errors."""
import ctypes as C

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

N, M, DENSITY, ARITY = 2000, 64, 0.05, 4
RETIRED = set(range(2, 7)) | {10} | set(range(17, 21)) | set(range(24, 31))
# the messages of csrc/query.hip, rows.hip and rows_var.hip
MSG_RANGE = "row out of range"
MSG_CAPACITY = "cols_cap too small"


@pytest.fixture(scope="module")
def tree(oracle_mod):
    dense = np.random.default_rng(2064).random((N, M)) < DENSITY
    return oracle_mod.OracleTree.from_dense(dense, "basic", ARITY)


def _dev(tree, layout):
    from genome_graph_annotation_amd import BRWTDevice
    d = BRWTDevice.from_tree(tree.export(), layout=layout)
    assert d.layout() == layout
    return d


def test_kernel_option_contract(tree):
    """MBRWT_OPT_KERNEL: 0 and 1 are accepted (1 only with a node image), the
    retired values are unsupported, everything else invalid; a rejected value
    leaves the context answering like the oracle."""
    from genome_graph_annotation_amd import _lib as L
    set_option = L.lib().mbrwt_set_option
    rows = np.random.default_rng(1).integers(0, N, 100).astype(np.uint64)
    off_o, cols_o = tree.get_rows(rows)
    d = _dev(tree, "nodes")
    for v in range(-1, 41):
        rc = set_option(d._h, L.MBRWT_OPT_KERNEL, v)
        want = L.MBRWT_OK if v in (0, 1) else L.MBRWT_ERR_UNSUPPORTED if v in RETIRED else L.MBRWT_ERR_INVALID
        assert rc == want, (v, rc)
        if rc != L.MBRWT_OK:
            off_d, cols_d = d.get_rows(rows)
            np.testing.assert_array_equal(off_d, off_o)
            np.testing.assert_array_equal(cols_d, cols_o)
    r = _dev(tree, "rows")
    assert set_option(r._h, L.MBRWT_OPT_KERNEL, 1) == L.MBRWT_ERR_UNSUPPORTED
    assert set_option(r._h, L.MBRWT_OPT_KERNEL, 0) == L.MBRWT_OK


def _get_rows_rc(d, rt, ot, ct, cap, stream):
    """mbrwt_get_rows_device called directly: (return code, labels needed, message)."""
    from genome_graph_annotation_amd import _lib as L
    need = C.c_uint64(0)
    rc = L.lib().mbrwt_get_rows_device(d._h, rt.data_ptr(), rt.numel(), ot.data_ptr(), ct.data_ptr(), cap,
                                       C.byref(need), stream)
    return rc, int(need.value), (L.lib().mbrwt_last_error_message() or b"").decode()


@pytest.mark.parametrize("kind", ["nodes", "rows", "var"])
def test_timing_and_status_accounting(tree, build_env, kind):
    """MBRWT_OPT_TIMING counts one launch per get_rows call, synchronous or
    asynchronous, on every driver; take_timing clears it; the range and
    capacity errors keep their codes and messages."""
    import torch
    from genome_graph_annotation_amd import _lib as L
    if kind == "var":
        build_env("MBRWT_ROWS_VAR", "1")
    d = _dev(tree, "nodes" if kind == "nodes" else "rows")
    if kind != "nodes":
        assert bool(d.rows_stats()["variable"]) == (kind == "var")
    rows = np.random.default_rng(7).integers(0, N, 500).astype(np.uint64)
    off_o, cols_o = tree.get_rows(rows)
    total = len(cols_o)
    rt = torch.from_numpy(rows.view(np.int64)).cuda()
    s0 = torch.cuda.current_stream().cuda_stream

    def check_csr(ot, ct):
        np.testing.assert_array_equal(ot.cpu().numpy().view(np.uint64), off_o)
        np.testing.assert_array_equal(ct[:total].cpu().numpy().view(np.uint32), cols_o)

    def sync_call():
        ot = torch.empty(len(rows) + 1, dtype=torch.int64, device="cuda")
        ct = torch.empty(total + 1, dtype=torch.int32, device="cuda")
        assert d.get_rows_device(rt, ot, ct, s0) == total
        torch.cuda.synchronize()
        check_csr(ot, ct)

    d.take_timing()
    d.set_option(L.MBRWT_OPT_TIMING, 1)
    for _ in range(3):
        sync_call()
    launches = 3
    if kind != "nodes":
        torch.cuda.synchronize()
        s1 = torch.cuda.Stream()
        outs = []
        for _ in range(2):
            ot = torch.empty(len(rows) + 1, dtype=torch.int64, device="cuda")
            ct = torch.empty(total + 1, dtype=torch.int32, device="cuda")
            st = torch.zeros(3, dtype=torch.int64, device="cuda")
            outs.append((ot, ct, st))
        torch.cuda.synchronize()
        for ot, ct, st in outs:
            d.get_rows_device_async(rt, ot, ct, st, s1.cuda_stream)
        s1.synchronize()
        for ot, ct, st in outs:
            assert st.cpu().tolist() == [total, L.MBRWT_OK, 1 << L.MBRWT_OK]
            check_csr(ot, ct)
        launches = 5
    ms, k = d.take_timing()
    assert k == launches and ms > 0, (ms, k)
    assert d.take_timing() == (0.0, 0)
    d.set_option(L.MBRWT_OPT_TIMING, 0)
    sync_call()
    assert d.take_timing() == (0.0, 0)

    # the ordinary API errors: an out-of-range row id, a capacity one short
    ot = torch.empty(len(rows) + 1, dtype=torch.int64, device="cuda")
    ct = torch.empty(total + 1, dtype=torch.int32, device="cuda")
    bad = rt.clone()
    bad[17] = N
    rc, _, msg = _get_rows_rc(d, bad, ot, ct, total + 1, s0)
    assert (rc, msg) == (L.MBRWT_ERR_RANGE, MSG_RANGE)
    rc, need, msg = _get_rows_rc(d, rt, ot, ct, total - 1, s0)
    assert (rc, need, msg) == (L.MBRWT_ERR_CAPACITY, total, MSG_CAPACITY)
    sync_call()  # and a good call after them
