"""GPU parity of the BinRel-WT engine (csrc/binrel_wt.hip) at its chunk,
rank-block and symbol-width boundaries, on the deterministic fixture of
tests/wt_shapes.py.  Every comparison is bit-exact on integers, against the
numpy reference over the CSR the matrix was built from (the primary one) and
against the BinRel-WT(sdsl) oracle.

  * several chunks (2^k rows each): build_from_csr's per-chunk str0 and
    slicing, k_wt_decode / k_wt_get on rows of a chunk > 0, k_wt_col_range,
    k_wt_col_lift's search over coff (ties at a chunk without the column) and
    its per-chunk row search, serialize, classify -- k = 0, 1, 10, 17
  * symbols of 30, 31 and 32 bits: 15 and 16 digit levels (kWtMaxLevels)
  * chunk lengths at every word (16), quarter (words 1, 5, 9) and block (208)
    edge, one either side, one and two whole blocks; empty chunks first, last
    and in the middle (the sentinel block, padding read as digit 0)
  * the 256-row tile of k_wt_decode: wt_shapes.batches
  * num_columns beyond 2^32: exact or refused, never a wrong answer

Each case first asserts its built form -- device_bytes() equals the closed
form over the case's chunk and level counts, and those are the counts the
case is named for -- so no case quietly runs the one-chunk path."""
import ctypes as C

import numpy as np
import pytest

import wt_shapes as S
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

# name -> (builder, num_columns, chunks, digit levels)
_SHAPES = {
    "chunk-per-row": (lambda: S.chunk_per_row((1 << 31) - 1), (1 << 31) - 1, 90, 16),
    "two-rows-per-chunk": (S.two_rows_per_chunk, S.M_TWO_ROWS, 20, 15),
    "w32-all-ones": (lambda: S.chunk_per_row((1 << 32) - 1), (1 << 32) - 1, 90, 16),
    "w32": (lambda: S.chunk_per_row(1 << 32), 1 << 32, 90, 16),
    "k10": (S.k10, S.M_K10, 4, 10),
    "k17": (S.k17, S.M_K17, 3, 7),
    "empty-middle": (S.empty_middle, S.M_EMPTY_MIDDLE, 3, 10),
}
_NAMED = {"k10": S.K10_NAMED, "empty-middle": S.EMPTY_MIDDLE_NAMED}


class _Case:
    """A shape's CSR, its device matrix (form asserted), the oracle's tree
    and the numpy reference of every row, computed once."""

    def __init__(self, O, name):
        from genome_graph_annotation_amd import BinRelWTDevice
        build, self.m, chunks, levels = _SHAPES[name]
        self.name = name
        self.off, self.cols = build()
        S.check_csr(self.off, self.cols, self.m)
        self.n = len(self.off) - 1
        assert (S.num_chunks(self.n, self.m), S.levels(self.m)) == (chunks, levels), name
        assert chunks > 1
        self.dev = BinRelWTDevice.from_csr(self.off, self.cols, self.m)
        assert_form(self.dev, self.off, self.cols, self.m)
        self.t = O.OracleWT.from_csr(self.off, self.cols, self.m)
        self.lens = np.diff(self.off.astype(np.int64))

    def columns_present(self):
        """Every distinct id of the chunk-per-row shapes; elsewhere the
        named columns and 32 of the distinct ids, evenly spaced."""
        ids = np.unique(self.cols)
        if S.chunk_log2(self.m) <= 1:
            return ids.tolist()
        named = list(_NAMED.get(self.name, ()))
        return named + ids[np.linspace(0, len(ids) - 1, 32).astype(np.int64)].tolist()


def assert_form(dev, off, cols, m):
    assert dev.num_rows() == len(off) - 1 and dev.num_columns() == m and dev.num_relations() == len(cols)
    assert dev.device_bytes() == S.expected_device_bytes(off, m), (dev.device_bytes(), S.expected_device_bytes(off, m))


_cases = {}


def _case(O, name):
    if name not in _cases:
        _cases[name] = _Case(O, name)
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The shared device matrices go when the module's tests are done, not at interpreter exit."""
    yield
    _cases.clear()


def _dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _rows_device(dev, rt, ot, buf, cap):
    """mbrwt_wt_get_rows_device -> (status, cols_needed)."""
    import torch
    from genome_graph_annotation_amd import _lib as L
    need = C.c_uint64(2**64 - 1)
    st = L.lib().mbrwt_wt_get_rows_device(dev._h, rt.data_ptr(), rt.numel(), ot.data_ptr(),
                                          buf.data_ptr() if buf is not None else None, cap, C.byref(need), None)
    torch.cuda.synchronize()
    return st, int(need.value)


def _check_batch(dev, off, cols, rows, name, t=None):
    """`rows` through get_rows (host) and through get_rows_device with cap =
    total, cap = total - 1 (MBRWT_ERR_CAPACITY, needed == total) and a null
    label buffer (a sizing call); nothing is written past cap."""
    import torch
    from genome_graph_annotation_amd import _lib as L
    off_e, cols_e = S.ref_rows(off, cols, rows)
    tot = len(cols_e)
    if t is not None:
        off_o, cols_o = t.get_rows(rows)
        np.testing.assert_array_equal(off_o, off_e, err_msg=f"{name}: oracle offsets")
        np.testing.assert_array_equal(cols_o, cols_e, err_msg=f"{name}: oracle labels")
    off_h, cols_h = dev.get_rows(rows)
    np.testing.assert_array_equal(off_h, off_e, err_msg=f"{name}: get_rows offsets")
    np.testing.assert_array_equal(cols_h, cols_e, err_msg=f"{name}: get_rows labels")
    rt = _dev_u64(rows)
    ot = torch.full((len(rows) + 1,), -1, dtype=torch.int64, device="cuda")
    ct = torch.full((tot + 64,), -1, dtype=torch.int32, device="cuda")
    # cap = total
    assert _rows_device(dev, rt, ot, ct, tot) == (L.MBRWT_OK, tot), name
    np.testing.assert_array_equal(ot.cpu().numpy().view(np.uint64), off_e, err_msg=f"{name}: device offsets")
    np.testing.assert_array_equal(ct[:tot].cpu().numpy().view(np.uint32), cols_e, err_msg=f"{name}: device labels")
    assert (ct[tot:] == -1).all(), f"{name}: a label written past the total"
    if not tot:
        assert _rows_device(dev, rt, ot, None, 0) == (L.MBRWT_OK, 0), name
        return
    # cap = total - 1
    ct.fill_(-1)
    assert _rows_device(dev, rt, ot, ct, tot - 1) == (L.MBRWT_ERR_CAPACITY, tot), name
    assert (ct == -1).all(), f"{name}: labels written under MBRWT_ERR_CAPACITY"
    # a null label buffer sizes the batch (cols_cap counts as 0)
    assert _rows_device(dev, rt, ot, None, tot) == (L.MBRWT_ERR_CAPACITY, tot), name
    assert (ct == -1).all(), f"{name}: labels written by the sizing call"
    assert _rows_device(dev, rt, ot, ct, tot) == (L.MBRWT_OK, tot), name   # and the handle still answers
    np.testing.assert_array_equal(ct[:tot].cpu().numpy().view(np.uint32), cols_e, err_msg=f"{name}: after sizing")


def _check_answers(dev, off, cols, m, t=None, columns=None, what=""):
    """Every row, the point queries and `columns` (default: 8 present, the
    absent ones) of `dev` against the numpy reference (and the oracle t)."""
    n = len(off) - 1
    _check_batch(dev, off, cols, np.arange(n, dtype=np.uint64), f"{what}: every row", t)
    qr, qc, want = S.point_queries(off, cols, m)
    np.testing.assert_array_equal(S.ref_get(off, cols, qr, qc), want)
    np.testing.assert_array_equal(dev.get_batch(qr, qc), want, err_msg=f"{what}: get_batch")
    if columns is None:
        ids = np.unique(cols)
        columns = ids[np.linspace(0, len(ids) - 1, 8).astype(np.int64)].tolist()
    for c in columns:
        want_c = S.ref_column(off, cols, c)
        assert len(want_c) > 0
        np.testing.assert_array_equal(dev.get_column(c), want_c, err_msg=f"{what}: column {c}")
        if t is not None:
            np.testing.assert_array_equal(t.get_column(c), want_c, err_msg=f"{what}: oracle column {c}")
    for c in S.absent_columns(cols, m):
        assert len(S.ref_column(off, cols, c)) == 0
        assert len(dev.get_column(c)) == 0, f"{what}: absent column {c}"
        if t is not None:
            assert len(t.get_column(c)) == 0
    return qr, qc, want


@pytest.mark.parametrize("name", list(_SHAPES))
def test_get_rows(oracle_mod, name):
    """get_rows of every row and of the tile batches, host and device forms;
    a batch whose last row is num_rows is MBRWT_ERR_RANGE and the handle
    answers afterwards."""
    import torch
    from genome_graph_annotation_amd import MBRWTError, _lib as L
    c = _case(oracle_mod, name)
    _check_batch(c.dev, c.off, c.cols, np.arange(c.n, dtype=np.uint64), "every row", c.t)
    _check_batch(c.dev, c.off, c.cols, np.arange(c.n, dtype=np.uint64)[::-1], "every row, reversed")
    for bname, rows in S.batches(c.off):
        _check_batch(c.dev, c.off, c.cols, rows, bname)
    bad = np.array([S.heavy_row(c.off), 0, c.n], dtype=np.uint64)
    with pytest.raises(MBRWTError) as ei:
        c.dev.get_rows(bad)
    assert ei.value.status == L.MBRWT_ERR_RANGE
    ot = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    ct = torch.full((S.HEAVY + 700,), -1, dtype=torch.int32, device="cuda")
    assert _rows_device(c.dev, _dev_u64(bad), ot, ct, ct.numel())[0] == L.MBRWT_ERR_RANGE
    assert (ct == -1).all()
    _check_batch(c.dev, c.off, c.cols, bad[:2], "after the range error")


@pytest.mark.parametrize("name", list(_SHAPES))
def test_get_batch(oracle_mod, name):
    """get on every non-empty row's first and last id and on one absent id
    per row (id - 1, id + 1, 0, m - 1); the oracle on a sample of them."""
    from genome_graph_annotation_amd import MBRWTError, _lib as L
    c = _case(oracle_mod, name)
    qr, qc, want = S.point_queries(c.off, c.cols, c.m)
    assert want.any() and not want.all() and {0, c.m - 1} <= set(qc[~want].tolist())
    np.testing.assert_array_equal(S.ref_get(c.off, c.cols, qr, qc), want)
    np.testing.assert_array_equal(c.dev.get_batch(qr, qc), want)
    for i in np.linspace(0, len(qr) - 1, 600).astype(np.int64):
        assert c.t.get(int(qr[i]), int(qc[i])) == bool(want[i]), (qr[i], qc[i])
    for r, col in ((c.n, 0), (0, c.m)):
        with pytest.raises(MBRWTError) as ei:
            c.dev.get_batch([0, r], [0, col])
        assert ei.value.status == L.MBRWT_ERR_RANGE
    np.testing.assert_array_equal(c.dev.get_batch(qr[:5], qc[:5]), want[:5])


@pytest.mark.parametrize("name", list(_SHAPES))
def test_get_column(oracle_mod, name):
    """get_column of the columns present (every distinct id of the
    chunk-per-row shapes; the named columns and 32 more elsewhere) and of
    columns no row holds; mbrwt_wt_get_column_device's capacity protocol (as
    test_get_column_capacity_protocol holds the BRWT handle to): a null buffer
    sizes the column -- MBRWT_OK for a column no row holds, MBRWT_ERR_CAPACITY
    otherwise; a cap one short is MBRWT_ERR_CAPACITY with the size and writes
    nothing; the exact cap gives the rows and writes nothing past them; column
    == num_columns is MBRWT_ERR_RANGE."""
    import torch
    from genome_graph_annotation_amd import _lib as L
    c = _case(oracle_mod, name)
    present = c.columns_present()
    chunks_hit = set()
    for col in present:
        want = S.ref_column(c.off, c.cols, col)
        assert len(want) > 0
        chunks_hit.add(len(set((want >> np.uint64(S.chunk_log2(c.m))).tolist())))
        np.testing.assert_array_equal(c.dev.get_column(col), want, err_msg=f"column {col}")
        np.testing.assert_array_equal(c.t.get_column(col), want, err_msg=f"oracle column {col}")
    assert max(chunks_hit) > 1   # some column is lifted out of several chunks
    absent = S.absent_columns(c.cols, c.m)
    for col in absent:
        assert len(S.ref_column(c.off, c.cols, col)) == 0
        assert len(c.dev.get_column(col)) == 0 and len(c.t.get_column(col)) == 0, col
    lib = L.lib()

    def call(col, buf, cap):
        need = C.c_uint64(2**64 - 1)
        st = lib.mbrwt_wt_get_column_device(c.dev._h, col, buf.data_ptr() if buf is not None else None, cap,
                                            C.byref(need), None)
        torch.cuda.synchronize()
        return st, int(need.value)

    by_size = sorted(present, key=lambda col: len(S.ref_column(c.off, c.cols, col)))
    for col in dict.fromkeys(list(_NAMED.get(name, ())) + [by_size[0], by_size[len(by_size) // 2], by_size[-1]]):
        want = S.ref_column(c.off, c.cols, col)
        k = len(want)
        assert call(col, None, 0) == (L.MBRWT_ERR_CAPACITY, k), col
        buf = torch.full((k + 8,), -1, dtype=torch.int64, device="cuda")
        assert call(col, None, k) == (L.MBRWT_ERR_CAPACITY, k), col      # (rows_cap counts as 0)
        assert call(col, buf, k - 1) == (L.MBRWT_ERR_CAPACITY, k), col
        assert (buf == -1).all(), "rows written under MBRWT_ERR_CAPACITY"
        assert call(col, buf, k) == (L.MBRWT_OK, k), col
        np.testing.assert_array_equal(buf[:k].cpu().numpy().view(np.uint64), want, err_msg=f"column {col}")
        assert (buf[k:] == -1).all(), "a row written past the column's size"
    buf = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    assert call(absent[0], None, 0) == (L.MBRWT_OK, 0)
    assert call(absent[0], buf, 8) == (L.MBRWT_OK, 0) and (buf == -1).all()
    assert call(c.m, buf, 8)[0] == L.MBRWT_ERR_RANGE and (buf == -1).all()
    assert call(c.m, None, 0)[0] == L.MBRWT_ERR_RANGE
    assert "column out of range" in (lib.mbrwt_last_error_message() or b"").decode()
    np.testing.assert_array_equal(c.dev.get_column(by_size[-1]), S.ref_column(c.off, c.cols, by_size[-1]))


@pytest.mark.parametrize("name", ["k10", "empty-middle", "chunk-per-row"])
def test_round_trip(oracle_mod, name):
    """serialize() of the chunked matrix equals serialize_csr of its CSR, and
    load() of those bytes builds the same form and answers as the reference."""
    from genome_graph_annotation_amd import BinRelWTDevice
    from genome_graph_annotation_amd.binrel_wt import parse_stream, serialize_csr
    c = _case(oracle_mod, name)
    data = serialize_csr(c.off, c.cols, c.m)
    assert c.dev.serialize() == data
    p_off, p_cols, p_m, used = parse_stream(data)
    assert p_m == c.m and used == len(data)
    np.testing.assert_array_equal(p_off, c.off)
    np.testing.assert_array_equal(p_cols, c.cols)
    d = BinRelWTDevice.load(data)
    assert_form(d, c.off, c.cols, c.m)
    _check_answers(d, c.off, c.cols, c.m, columns=list(_NAMED.get(name, ())) or None, what="loaded")
    assert d.serialize() == data


def test_classify_across_chunks(oracle_mod):
    """get_labels_batch / get_top_labels_batch on k17 (8,192 columns: the
    smallest width at which classify meets several chunks): reads inside one
    chunk, across two and across three, an empty read, a read that repeats one
    row twice and another three times; against _ref_labels / _ref_top of
    test_gpu_edge_shapes.py, their counts taken from the CSR."""
    from test_gpu_edge_shapes import _check_labels, _check_top
    c = _case(oracle_mod, "k17")
    R, n = 1 << 17, c.n
    full = np.nonzero(c.lens >= 2)[0]
    r, s, q = int(full[0]), int(full[full >= R][0]), int(full[full >= 2 * R][0])
    reads = [
        list(range(100, 130)), list(range(R + 5, R + 40)), list(range(2 * R, n)),        # one chunk each
        list(range(R - 20, R + 20)), list(range(2 * R - 3, 2 * R + 30)), [r, q],         # two chunks
        [R - 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 0, n - 1],                  # three chunks
        [],
        [r, r, s, s, s, q], [s, s], [q, r, q],                                            # repeated rows
        np.arange(0, n, n // 600).tolist(),                                               # 600 rows of every chunk
        [n - 1],
    ]
    chunks_of = [len({x >> 17 for x in rd}) for rd in reads]
    assert chunks_of[:7] == [1, 1, 1, 2, 2, 2, 3] and chunks_of[7] == 0 and chunks_of[11] == 3
    dense = S.CsrDense(c.off, c.cols, c.m)
    for ratio in (0.0, 0.5, 1.0):
        off, labs = _check_labels(c.dev, dense, reads, ratio, "k17")
        if ratio == 0.5:   # the row repeated three times out of six carries the read
            np.testing.assert_array_equal(labs[int(off[8]):int(off[9])], c.cols[c.off[s]:c.off[s + 1]])
        assert off[7] == off[8]
    for num_top in (1, 3, 2**64 - 1):
        off, labs, cnts = _check_top(c.dev, dense, reads, num_top, "k17")
        assert cnts[int(off[8])] == 3 and off[7] == off[8]
    assert int(off[12] - off[11]) > 1000   # a read of many distinct labels, from three chunks


def test_columns_beyond_32_bits():
    """num_columns = 2^32 + 10: exact or refused, never a wrong answer.  The
    ids are 32 bits, so no row holds a column >= 2^32: get answers 0 for it and
    get_column no rows (include/mbrwt_wt.h, at mbrwt_binrel_desc).

    Before k_wt_get and wt_get_column stopped taking a column's low 32 bits
    for the column, get(r, 2^32 + c) and get_column(2^32 + c) answered as
    column c does: on an MI355X, get(3, 2^32 + 5) read back 1 for the row
    holding 5."""
    from genome_graph_annotation_amd import BinRelWTDevice, MBRWTError, _lib as L
    off, cols = S.beyond_32_bits()
    m = S.M_BEYOND
    try:
        d = BinRelWTDevice.from_csr(off, cols, m)
    except MBRWTError as e:
        assert e.status in (L.MBRWT_ERR_INVALID, L.MBRWT_ERR_UNSUPPORTED)
        return
    assert_form(d, off, cols, m)
    assert S.num_chunks(len(off) - 1, m) == 20 and S.levels(m) == 16
    _check_batch(d, off, cols, np.arange(20, dtype=np.uint64), "every row")
    _check_batch(d, off, cols, np.array([4, 3, 19, 4, 0], dtype=np.uint64), "a batch")
    big = 1 << 32
    assert d.get(3, 5) and d.get(4, 5) and d.get(4, 0xFFFFFFFF) and not d.get(3, 0xFFFFFFFF)
    assert not d.get(3, big + 5) and not d.get(4, big + 5) and not d.get(3, big + 9) and not d.get(4, big)
    qr, qc, want = S.point_queries(off, cols, m)
    np.testing.assert_array_equal(d.get_batch(qr, qc), want)
    np.testing.assert_array_equal(S.ref_get(off, cols, qr, qc), want)
    # every id again with bit 32 set (those below 10: in range, held by no row), beside the id itself
    rows_of = np.repeat(np.arange(20), np.diff(off.astype(np.int64))).astype(np.uint64)
    low = cols.astype(np.uint64) < 10
    both_r = np.concatenate([rows_of[low], rows_of])
    both_c = np.concatenate([cols[low].astype(np.uint64) + np.uint64(big), cols.astype(np.uint64)])
    assert low.sum() >= 3
    np.testing.assert_array_equal(d.get_batch(both_r, both_c), np.concatenate([np.zeros(low.sum(), bool),
                                                                               np.ones(len(cols), bool)]))
    for col in (5, 0xFFFFFFFF, 0, 1 << 31, 77):
        want_c = S.ref_column(off, cols, col)
        assert len(want_c) > 0
        np.testing.assert_array_equal(d.get_column(col), want_c, err_msg=f"column {col}")
    for col in (big + 5, big, big + 9, 2):
        assert len(d.get_column(col)) == 0, col
    for col in (m, m + 1, 2**64 - 1):
        with pytest.raises(MBRWTError) as ei:
            d.get_column(col)
        assert ei.value.status == L.MBRWT_ERR_RANGE
    with pytest.raises(MBRWTError) as ei:
        d.get_batch([3], [m])
    assert ei.value.status == L.MBRWT_ERR_RANGE
    assert d.get(3, 5)
