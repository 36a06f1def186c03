"""Batched classify on the multi-device handle (include/mbrwt.h "multi-device":
mbrwt_multi_get_labels_batch[_device], mbrwt_multi_get_top_labels_batch[_device];
csrc/multi.hip classify_multi, csrc/multi_split.hpp): replicas on devices [0],
[0, 0] and [0, 0, 0] (several contexts on one device run the same split,
per-replica classify and reassembly as N devices; peer copies become
device-local copies), host and device buffers, against the reference
semantics computed from the CPU oracle's rows."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 20000, 300
DEVICES = [(0,), (0, 0), (0, 0, 0)]
ALL = 2**64 - 1


def _ref_get_labels(off_o, cols_o, read_offsets, m, ratio):
    """annotate_static.cpp:71-94 over the oracle's rows (std::ceil in double)."""
    out_off, out = [0], []
    for r in range(len(read_offsets) - 1):
        a, b = int(read_offsets[r]), int(read_offsets[r + 1])
        cnt = np.bincount(cols_o[off_o[a]:off_o[b]], minlength=m)
        thr = 1 if ratio == 0 else math.ceil((b - a) * ratio)
        out.extend(np.nonzero((cnt > 0) & (cnt >= thr))[0].tolist())
        out_off.append(len(out))
    return np.array(out_off, dtype=np.uint64), np.array(out, dtype=np.uint32)


def _ref_top_labels(off_o, cols_o, read_offsets, m, num_top):
    """annotate.cpp:57-83 over the oracle's rows; equal counts in ascending label order."""
    out_off, labs, cnts = [0], [], []
    for r in range(len(read_offsets) - 1):
        a, b = int(read_offsets[r]), int(read_offsets[r + 1])
        cnt = np.bincount(cols_o[off_o[a]:off_o[b]], minlength=m)
        nz = np.nonzero(cnt)[0]
        order = nz[np.lexsort((nz, -cnt[nz].astype(np.int64)))][:num_top]
        labs.extend(order.tolist())
        cnts.extend(cnt[order].tolist())
        out_off.append(len(labs))
    return np.array(out_off, dtype=np.uint64), np.array(labs, dtype=np.uint32), np.array(cnts, dtype=np.uint64)


class Fixture:
    """One oracle tree, one batch of reads with the oracle's rows, and the
    multi handles built from the tree (one per devices x layout, kept)."""

    def __init__(self, O):
        rng = np.random.default_rng(7)
        self.tree = O.OracleTree.from_dense(rng.random((N, M)) < 0.02, "basic", 8)
        lens = rng.integers(0, 60, 600)
        self.read_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        anchors = rng.integers(0, N - 100, len(lens))
        self.rows = np.concatenate([a + rng.integers(0, 100, k) for a, k in zip(anchors, lens)]).astype(np.uint64)
        self.off_o, self.cols_o = self.tree.get_rows(self.rows)
        self._multi = {}

    def multi(self, devices, layout=None):
        from genome_graph_annotation_amd import BRWTMulti
        key = (devices, layout)
        if key not in self._multi:
            self._multi[key] = BRWTMulti.from_tree(self.tree.export(), devices=devices, layout=layout)
            assert self._multi[key].size() == len(devices)
        return self._multi[key]

    def want_labels(self, rows, read_off, ratio):
        off_o, cols_o = (self.off_o, self.cols_o) if rows is self.rows else self.tree.get_rows(rows)
        return _ref_get_labels(off_o, cols_o, read_off, M, ratio)

    def want_top(self, rows, read_off, num_top):
        off_o, cols_o = (self.off_o, self.cols_o) if rows is self.rows else self.tree.get_rows(rows)
        return _ref_top_labels(off_o, cols_o, read_off, M, min(num_top, M + 1))


@pytest.fixture(scope="module")
def fx(oracle_mod):
    return Fixture(oracle_mod)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _labels_device(mu, rows, read_off, ratio):
    """get_labels_batch_device through the capacity protocol: the sizing call
    (no labels buffer), then the exact-size call; -> (offsets, labels, needed)."""
    import torch
    from genome_graph_annotation_amd import _lib as L
    rt, ot = _to_dev(rows), _to_dev(read_off)
    lo = torch.empty(len(read_off), dtype=torch.int64, device="cuda")
    try:
        need = mu.get_labels_batch_device(rt, ot, ratio, lo, None, _stream())
        assert need == 0
    except L.MBRWTError as e:
        assert e.status == L.MBRWT_ERR_CAPACITY
        need = e.needed
    lt = torch.empty(need, dtype=torch.int32, device="cuda")
    assert mu.get_labels_batch_device(rt, ot, ratio, lo, lt, _stream()) == need
    # complete on return: read back without synchronising the caller's stream first
    return lo.cpu().numpy().view(np.uint64), lt.cpu().numpy().view(np.uint32), need


def _top_device(mu, rows, read_off, num_top):
    import torch
    from genome_graph_annotation_amd import _lib as L
    rt, ot = _to_dev(rows), _to_dev(read_off)
    lo = torch.empty(len(read_off), dtype=torch.int64, device="cuda")
    try:
        need = mu.get_top_labels_batch_device(rt, ot, num_top, lo, None, None, _stream())
        assert need == 0
    except L.MBRWTError as e:
        assert e.status == L.MBRWT_ERR_CAPACITY
        need = e.needed
    lt = torch.empty(need, dtype=torch.int32, device="cuda")
    ct = torch.empty(need, dtype=torch.int64, device="cuda")
    assert mu.get_top_labels_batch_device(rt, ot, num_top, lo, lt, ct, _stream()) == need
    return lo.cpu().numpy().view(np.uint64), lt.cpu().numpy().view(np.uint32), ct.cpu().numpy().view(np.uint64)


def _rows_still_work(fx, mu):
    """After a failed call, an ordinary get_rows on the same handle succeeds."""
    rows = np.arange(5, dtype=np.uint64)
    off_o, cols_o = fx.tree.get_rows(rows)
    off_d, cols_d = mu.get_rows(rows)
    np.testing.assert_array_equal(off_d, off_o)
    np.testing.assert_array_equal(cols_d, cols_o)


@pytest.mark.parametrize("ratio", [0.0, 0.1, 0.5, 1.0])
@pytest.mark.parametrize("layout", ["nodes", "rows"])
@pytest.mark.parametrize("devices", DEVICES)
def test_multi_get_labels_like_reference(fx, devices, layout, ratio):
    mu = fx.multi(devices, layout)
    assert mu.replica(0).layout() == layout
    want_off, want = fx.want_labels(fx.rows, fx.read_off, ratio)
    got_off, got = mu.get_labels_batch(fx.rows, fx.read_off, ratio)
    np.testing.assert_array_equal(got_off, want_off)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("num_top", [ALL, 5, 1, 0])
@pytest.mark.parametrize("layout", ["nodes", "rows"])
@pytest.mark.parametrize("devices", DEVICES)
def test_multi_get_top_labels_like_reference(fx, devices, layout, num_top):
    mu = fx.multi(devices, layout)
    want = fx.want_top(fx.rows, fx.read_off, num_top)
    got = mu.get_top_labels_batch(fx.rows, fx.read_off, num_top)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def _edge_batches():
    rng = np.random.default_rng(11)
    some = rng.integers(0, N, 37).astype(np.uint64)
    none = np.zeros(0, dtype=np.uint64)
    return {
        "no_reads": (none, [0]),
        "one_read": (some, [0, 37]),
        "two_reads": (some, [0, 30, 37]),
        "middle_of_five": (some, [0, 0, 0, 37, 37, 37]),
        "reads_without_rows": (none, [0, 0, 0, 0, 0]),
    }


@pytest.mark.parametrize("name", list(_edge_batches()))
def test_multi_edge_batches(fx, name):
    """Batches with fewer reads than replicas, replicas without reads or rows:
    host and device forms on three replicas."""
    rows, read_off = _edge_batches()[name]
    read_off = np.array(read_off, dtype=np.uint64)
    mu = fx.multi((0, 0, 0))
    for ratio in (0.0, 0.5):
        want_off, want = fx.want_labels(rows, read_off, ratio)
        got_off, got = mu.get_labels_batch(rows, read_off, ratio)
        np.testing.assert_array_equal(got_off, want_off)
        np.testing.assert_array_equal(got, want)
        dev_off, dev, _ = _labels_device(mu, rows, read_off, ratio)
        np.testing.assert_array_equal(dev_off, want_off)
        np.testing.assert_array_equal(dev, want)
    for num_top in (ALL, 2):
        want = fx.want_top(rows, read_off, num_top)
        for got in (mu.get_top_labels_batch(rows, read_off, num_top), _top_device(mu, rows, read_off, num_top)):
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("devices", DEVICES)
def test_multi_device_forms_match_host_forms(fx, devices):
    """Tensors on device 0: the capacity protocol (null and too-small label
    buffers give MBRWT_ERR_CAPACITY with the total of all replicas, the
    exact-size call succeeds) and the outputs of the host forms."""
    import torch
    from genome_graph_annotation_amd import _lib as L
    mu = fx.multi(devices)
    want_off, want = mu.get_labels_batch(fx.rows, fx.read_off, 0.25)
    ref_off, ref = fx.want_labels(fx.rows, fx.read_off, 0.25)
    np.testing.assert_array_equal(want, ref)
    got_off, got, need = _labels_device(mu, fx.rows, fx.read_off, 0.25)  # sizing call with no buffer
    assert need == len(want) > 0
    np.testing.assert_array_equal(got_off, want_off)
    np.testing.assert_array_equal(got, want)
    rt, ot = _to_dev(fx.rows), _to_dev(fx.read_off)
    lo = torch.empty(len(fx.read_off), dtype=torch.int64, device="cuda")
    small = torch.empty(len(want) - 1, dtype=torch.int32, device="cuda")
    with pytest.raises(L.MBRWTError) as e:
        mu.get_labels_batch_device(rt, ot, 0.25, lo, small, _stream())
    assert e.value.status == L.MBRWT_ERR_CAPACITY and e.value.needed == len(want)

    want_t = mu.get_top_labels_batch(fx.rows, fx.read_off, 7)
    for g, w in zip(want_t, fx.want_top(fx.rows, fx.read_off, 7)):
        np.testing.assert_array_equal(g, w)
    for g, w in zip(_top_device(mu, fx.rows, fx.read_off, 7), want_t):  # sizing call with no buffers
        np.testing.assert_array_equal(g, w)
    n = len(want_t[1])
    with pytest.raises(L.MBRWTError) as e:
        mu.get_top_labels_batch_device(rt, ot, 7, lo, torch.empty(n - 1, dtype=torch.int32, device="cuda"),
                                       torch.empty(n, dtype=torch.int64, device="cuda"), _stream())
    assert e.value.status == L.MBRWT_ERR_CAPACITY and e.value.needed == n
    # the host forms' own capacity protocol, through the C ABI
    import ctypes as C
    from genome_graph_annotation_amd.brwt import _p
    need = C.c_uint64(0)
    lo_h = np.zeros(len(fx.read_off), dtype=np.uint64)
    st = L.lib().mbrwt_multi_get_labels_batch(mu._h, _p(fx.rows, C.c_uint64), fx.rows.size,
                                              _p(fx.read_off, C.c_uint64), fx.read_off.size - 1, 0.25,
                                              _p(lo_h, C.c_uint64), None, 0, C.byref(need))
    assert st == L.MBRWT_ERR_CAPACITY and need.value == len(want)


MALFORMED = ([0, 11], [1, 10], [0, 6, 4, 10], [0, 5, 9])  # 10 rows; [0, 6, 4, 10]: the descending pair on the cut


def test_multi_classify_errors(fx):
    """Errors keep their single-context meaning on two replicas and leave the
    handle usable."""
    from genome_graph_annotation_amd import BRWTMulti, _lib as L
    import torch
    mu = fx.multi((0, 0))
    rows = np.arange(10, dtype=np.uint64)
    whole = np.array([0, 10], dtype=np.uint64)
    with pytest.raises(L.MBRWTError) as e:  # an assert in the reference
        mu.get_labels_batch(rows, whole, 1.5)
    assert e.value.status == L.MBRWT_ERR_INVALID
    _rows_still_work(fx, mu)
    for bad in MALFORMED:
        bad = np.array(bad, dtype=np.uint64)
        for call in (lambda: mu.get_labels_batch(rows, bad, 0.0),
                     lambda: mu.get_top_labels_batch(rows, bad, 3)):
            with pytest.raises(L.MBRWTError) as e:
                call()
            assert e.value.status == L.MBRWT_ERR_INVALID
        rt, ot = _to_dev(rows), _to_dev(bad)
        lo = torch.empty(len(bad), dtype=torch.int64, device="cuda")
        lt = torch.empty(64, dtype=torch.int32, device="cuda")
        ct = torch.empty(64, dtype=torch.int64, device="cuda")
        for call in (lambda: mu.get_labels_batch_device(rt, ot, 0.0, lo, lt, _stream()),
                     lambda: mu.get_top_labels_batch_device(rt, ot, 3, lo, lt, ct, _stream())):
            with pytest.raises(L.MBRWTError) as e:
                call()
            assert e.value.status == L.MBRWT_ERR_INVALID
        _rows_still_work(fx, mu)
    with pytest.raises(L.MBRWTError) as e:  # zero reads but rows
        mu.get_labels_batch(rows, np.array([0], dtype=np.uint64), 0.0)
    assert e.value.status == L.MBRWT_ERR_INVALID
    # a row outside the matrix in the last replica's slice (reads [0, 5) and [5, 10): the cut is at row 5)
    out = rows.copy()
    out[9] = N
    halves = np.array([0, 5, 10], dtype=np.uint64)
    for call in (lambda: mu.get_labels_batch(out, halves, 0.0), lambda: mu.get_top_labels_batch(out, halves, 3)):
        with pytest.raises(L.MBRWTError) as e:
            call()
        assert e.value.status == L.MBRWT_ERR_RANGE
        _rows_still_work(fx, mu)
    # past the column limit of the device kernel
    big = BRWTMulti.synthetic(1000, 8193, 0.001, 8, 3, devices=(0, 0))
    with pytest.raises(L.MBRWTError) as e:
        big.get_top_labels_batch(np.arange(4, dtype=np.uint64), np.array([0, 2, 4], dtype=np.uint64), 3)
    assert e.value.status == L.MBRWT_ERR_UNSUPPORTED
    off, cols = big.get_rows(np.arange(4, dtype=np.uint64))
    assert len(off) == 5 and off[4] == len(cols)
    big.close()
    _rows_still_work(fx, mu)


def test_multi_mirror_classifies_on_the_replicas(oracle_mod):
    """C++ mirror: BRWTMultiDevice::labels_batch_csr / top_labels_batch_csr on
    {0, 0} return true (the batch ran on the replicas, not the annotator's
    per-read host fallback) and equal count_labels over the oracle matrix."""
    cpp = os.path.join(ROOT, "tests", "cpp", "multi")
    subprocess.run(["make", "-s", "-C", cpp, "mirror"], check=True)
    r = subprocess.run([os.path.join(cpp, "_build", "test_multi_mirror")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "3 tests, 0 failed checks" in r.stdout, r.stdout
