"""The option contract of MBRWT_OPT_KERNEL and the timing / status plumbing
that the three get_rows drivers (node images, row records, variable-length
records) share: values accepted and rejected, launches and milliseconds
counted per call, return codes and messages of the ordinary API errors; the
status protocol of the node-image point queries."""
import ctypes as C

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

N, M, DENSITY, ARITY = 2000, 64, 0.05, 4
RETIRED = set(range(2, 7)) | {10} | set(range(17, 21)) | set(range(24, 31))
# the messages of csrc/calls.cpp (shared by the node-image, rows.hip and rows_var.hip drivers)
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


@pytest.mark.parametrize("ctx", ["group", "lane", "shards"])
def test_node_point_queries_protocol(tree, build_env, ctx):
    """get_batch, count_labels and the work count (V, L) on the node images
    (the twin of test_gpu_edge_shapes.py test_point_queries_protocol): the
    group kernel, the lane-per-row kernel and a row-sharded context; an empty
    batch, one in-range row against the oracle, a batch whose last row is
    num_rows (MBRWT_ERR_RANGE from all three calls), a good call afterwards."""
    import torch
    from genome_graph_annotation_amd import BRWTDevice, _lib as L
    if ctx == "shards":
        build_env("MBRWT_LAYOUT", "nodes")
        build_env("MBRWT_SHARD_ROWS", "701")
        dev = BRWTDevice.from_tree(tree.export())
        assert dev.num_shards() == 3
    else:
        # without KIND_PACKT nodes the general kernel of variant 0 is k_traverse_group
        # (a tree with them runs the lane-per-row kernel under both variants)
        build_env("MBRWT_PACKT", "0")
        dev = _dev(tree, "nodes")
        dev.set_option(L.MBRWT_OPT_KERNEL, 1 if ctx == "lane" else 0)
        if ctx == "lane":  # (variant 0: MODE_WORK and MODE_COUNT run k_traverse_group)
            assert dev.traverse_kernel() == "k_traverse"
    lib = L.lib()
    assert dev.num_rows() == N and dev.num_columns() == M

    def dev_rows(rows):
        return torch.from_numpy(np.asarray(rows, dtype=np.uint64).view(np.int64)).cuda()

    def get_batch(rows, cols):
        rt, ct = dev_rows(rows), dev_rows(cols)
        out = torch.full((max(1, len(rows)),), 7, dtype=torch.uint8, device="cuda")
        st = lib.mbrwt_get_batch_device(dev._h, rt.data_ptr(), ct.data_ptr(), len(rows), out.data_ptr(), None)
        torch.cuda.synchronize()
        return st, out.cpu().numpy()

    def count_labels(rows):
        rt = dev_rows(rows)
        cnt = torch.full((M,), 7, dtype=torch.int64, device="cuda")
        st = lib.mbrwt_count_labels_device(dev._h, rt.data_ptr(), len(rows), cnt.data_ptr(), None)
        torch.cuda.synchronize()
        return st, cnt.cpu().numpy()

    def count_work(rows):
        rt = dev_rows(rows)
        v, lab = C.c_uint64(2**64 - 1), C.c_uint64(2**64 - 1)
        st = lib.mbrwt_count_work_device(dev._h, rt.data_ptr(), len(rows), C.byref(v), C.byref(lab), None)
        return st, int(v.value), int(lab.value)

    # n = 0
    st, out = get_batch([], [])
    assert st == L.MBRWT_OK and (out == 7).all()
    st, cnt = count_labels([])
    assert st == L.MBRWT_OK and (cnt == 0).all()
    assert count_work([]) == (L.MBRWT_OK, 0, 0)
    # one in-range row (past the first shard's rows) against the oracle
    off_all, _ = tree.get_rows(np.arange(N, dtype=np.uint64))
    r = 701 + int(np.argmax(np.diff(off_all.astype(np.int64))[701:] >= 3))
    _, cols_o, vis = tree.get_rows(np.array([r], dtype=np.uint64), with_visits=True)
    assert 3 <= len(cols_o) < M
    bits_o = np.isin(np.arange(M), cols_o).astype(np.uint8)
    st, out = get_batch([r] * M, np.arange(M))
    assert st == L.MBRWT_OK
    np.testing.assert_array_equal(out, bits_o)
    st, cnt = count_labels([r])
    assert st == L.MBRWT_OK
    np.testing.assert_array_equal(cnt, bits_o.astype(np.int64))
    assert count_work([r]) == (L.MBRWT_OK, int(vis.sum()), len(cols_o))
    # the last row of the batch is num_rows
    assert get_batch([r, 0, N], [0, 0, 0])[0] == L.MBRWT_ERR_RANGE
    assert count_labels([r, 0, N])[0] == L.MBRWT_ERR_RANGE
    assert count_work([r, 0, N])[0] == L.MBRWT_ERR_RANGE
    # (and the context still answers)
    st, out = get_batch([r] * M, np.arange(M))
    assert st == L.MBRWT_OK
    np.testing.assert_array_equal(out, bits_o)
    st, cnt = count_labels([r, r])
    assert st == L.MBRWT_OK
    np.testing.assert_array_equal(cnt, 2 * bits_o.astype(np.int64))
    assert count_work([r]) == (L.MBRWT_OK, int(vis.sum()), len(cols_o))
