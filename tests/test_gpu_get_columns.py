"""GPU parity of mbrwt_get_columns / mbrwt_get_columns_device
(csrc/rows_columns.hip): the sparse columns of a row window
for many columns at once.  The expected values are numpy on the dense matrix,
np.nonzero(dense[b:e, c])[0] + b per requested slot, cross-checked against
the context's own get_column(c) clipped to the window.  Integer work: no
tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from conftest import gpu_available
from test_gpu_from_rows import _csr as _csr_mixed, _dense, _shape
from test_gpu_from_sparse_columns import ALIGN, _csr, _same_context, _sparse
from test_relax_shape import _golden

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

U64P = C.POINTER(C.c_uint64)


def _expect(dense, columns=None, b=0, e=None):
    n, m = dense.shape
    e = n if e is None else e
    cols = range(m) if columns is None else columns
    parts = [np.flatnonzero(dense[b:e, int(c)]).astype(np.uint64) + np.uint64(b) for c in cols]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    return off, (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)).astype(np.uint64)


def _check(ctx, dense, columns=None, b=0, e=None, cross=3):
    """get_columns == numpy; a few slots also == the context's get_column, clipped."""
    woff, wrows = _expect(dense, columns, b, e)
    off, rows = ctx.get_columns(columns, b, e)
    assert off.dtype == np.uint64 and rows.dtype == np.uint64
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(rows, wrows)
    e = dense.shape[0] if e is None else e
    cols = list(range(dense.shape[1])) if columns is None else [int(c) for c in columns]
    for j in list(range(len(cols)))[:: max(1, len(cols) // cross)][:cross]:
        col = ctx.get_column(cols[j])
        col = col[(col >= b) & (col < e)]
        np.testing.assert_array_equal(rows[int(off[j]):int(off[j + 1])], col)
    return off, rows


def _from_rows(dense, **kw):
    from genome_graph_annotation_amd import BRWTDevice
    return BRWTDevice.from_rows(*_csr(dense), dense.shape[1], **kw)


def _packed_columns(dense):
    """dense as bit-packed columns: [m, ceil(n / 64)] uint64, LSB first."""
    n, m = dense.shape
    W = (n + 63) // 64
    bits = np.zeros((m, W * 64), dtype=bool)
    bits[:, :n] = dense.T
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view(np.uint64).reshape(m, W)


# ---- parity grid -----------------------------------------------------------------

@pytest.mark.parametrize("density", [0, 0.05, 0.5, 1])
@pytest.mark.parametrize("arity", [2, 8, 64])
def test_parity_grid(arity, density):
    """Every column (columns=None) == _sparse(dense): density 1 at m = 300
    reaches rows longer than a block (spills), density 0 gives empty slots."""
    for n in (1, 2, 63, 64, 65, 1000):
        for m in (2, 3, 9, 65, 300):
            dense = _dense(n, m, density, 7 * n + m)
            ctx = _from_rows(dense, arity=arity)
            off, rows = ctx.get_columns()
            woff, wrows = _sparse(dense)
            np.testing.assert_array_equal(off, woff, err_msg=f"n={n} m={m}")
            np.testing.assert_array_equal(rows, wrows, err_msg=f"n={n} m={m}")
            ctx.close()


# ---- column lists -------------------------------------------------------------------

@pytest.fixture(scope="module")
def lists_ctx():
    dense = _dense(65, 300, 0.05, 5)
    dense[:, 7] = False
    ctx = _from_rows(dense, arity=8)
    yield ctx, dense
    ctx.close()


@pytest.mark.parametrize("which", ["first", "last", "empty", "reversed", "subset17", "pair", "none"])
def test_column_lists(lists_ctx, which):
    """Slots come in the caller's order, which need not ascend."""
    ctx, dense = lists_ctx
    m = dense.shape[1]
    columns = {"first": [0], "last": [m - 1], "empty": [7], "reversed": list(range(m))[::-1],
               "subset17": np.random.default_rng(17).permutation(m)[:17].tolist(), "pair": [5, 3], "none": []}[which]
    off, rows = _check(ctx, dense, columns)
    if which == "empty":
        assert off.tolist() == [0, 0] and len(rows) == 0
    if which == "none":
        assert off.tolist() == [0] and len(rows) == 0


# ---- windows -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def windows_ctx():
    dense = _dense(1000, 65, 0.1, 11)
    ctx = _from_rows(dense, arity=8)
    yield ctx, dense
    ctx.close()


def test_windows(windows_ctx):
    ctx, dense = windows_ctx
    n = dense.shape[0]
    S = ctx.rows_stats()["rows_per_block"]
    assert S >= 1
    wins = [(0, 0), (500, 500), (n, n), (0, n), (1, n - 1), (63, 65), (64, 128), (999, 1000), (S - 1, S + 1)]
    if S >= 2:
        wins.append((1, 2))  # starts and ends inside one record block
    for b, e in wins:
        _check(ctx, dense, None, b, e)
        _check(ctx, dense, [64, 0, 33], b, e)


# ---- chunks ----------------------------------------------------------------------------

@pytest.mark.parametrize("chunk,emptied", [(1, False), (7, False), (64, False), (65, False), (129, False),
                                           (130, False), (131, False), (20, True)])
def test_chunks(chunk, emptied):
    """MBRWT_OPT_COLUMNS_CHUNK: the per-slot cursors across chunks; a column in
    every row and one only in the last row; with rows 40..99 emptied and
    chunks of 20 rows, chunks without any pair.  == the unchunked call == numpy."""
    from genome_graph_annotation_amd import _lib as L
    n, m = 130, 33
    dense = _dense(n, m, 0.3, 9)
    dense[:, 4] = True
    dense[:, 20] = False
    dense[129, 20] = True
    if emptied:
        dense[40:100] = False
    ctx = _from_rows(dense, arity=8)
    lists = (None, list(range(m))[::-1], [20, 4], [4])
    plain = [ctx.get_columns(c) for c in lists]
    plain_w = ctx.get_columns(None, 3, 127)
    ctx.set_option(L.MBRWT_OPT_COLUMNS_CHUNK, chunk)
    try:
        for c, (poff, prows) in zip(lists, plain):
            off, rows = _check(ctx, dense, c)
            np.testing.assert_array_equal(off, poff)
            np.testing.assert_array_equal(rows, prows)
        off, rows = _check(ctx, dense, None, 3, 127)
        np.testing.assert_array_equal(off, plain_w[0])
        np.testing.assert_array_equal(rows, plain_w[1])
    finally:
        ctx.set_option(L.MBRWT_OPT_COLUMNS_CHUNK, 0)
    ctx.close()


def test_chunk_halved_on_dense_rows():
    """A chunk is sized for twice the window's mean pairs per row: ten full rows
    among nearly empty ones count more pairs than the chunk's buffers hold, so
    the chunk is halved and recounted (10 -> 5 -> 2 rows) until it fits."""
    from genome_graph_annotation_amd import _lib as L
    n, m = 130, 33
    dense = _dense(n, m, 0.03, 19)
    dense[60:70] = True
    assert 2 * dense.sum() / n * 10 + 1 < 10 * m / 2  # (the first halving is not enough either)
    ctx = _from_rows(dense, arity=8)
    plain = ctx.get_columns()
    ctx.set_option(L.MBRWT_OPT_COLUMNS_CHUNK, 10)
    for columns, b, e in ((None, 0, None), (list(range(m))[::-1], 3, 127), ([4], 0, None)):
        _check(ctx, dense, columns, b, e)
    off, rows = ctx.get_columns()
    np.testing.assert_array_equal(off, plain[0])
    np.testing.assert_array_equal(rows, plain[1])
    ctx.close()


# ---- every record form -------------------------------------------------------------------

def _form(dense, arity, option, value):
    from genome_graph_annotation_amd.brwt import build_option
    with build_option(option, value):
        return _from_rows(dense, arity=arity)


@pytest.mark.parametrize("code", [1, 2, 3])
def test_record_codes(code):
    """Nibble codes (1), terminal records (2), byte masks (3).  Nibble codes are
    built on uniform trees only, so code 1 runs on 64 columns (8 x 8), the
    others on 65."""
    from genome_graph_annotation_amd import _lib as L
    n, m = 1000, 64 if code == 1 else 65
    dense = _dense(n, m, 0.05, m + code)
    ctx = _form(dense, 8, L.MBRWT_BUILD_ROWS_CODE, code)
    st = ctx.rows_stats()
    assert not st["variable"] and not st.get("classes")
    assert st["nibble_codes"] == (code == 1) and st["terminal_records"] == (code == 2), st
    _check(ctx, dense)
    _check(ctx, dense, [m - 1, 1, 40], 100, 901)
    ctx.close()


def test_masks_wider_than_16_bits():
    from genome_graph_annotation_amd import _lib as L
    dense = _dense(1000, 300, 0.05, 300)
    ctx = _form(dense, 64, L.MBRWT_BUILD_ROWS_CODE, 3)
    st = ctx.rows_stats()
    assert not st["variable"] and not st["nibble_codes"] and not st["terminal_records"], st
    _check(ctx, dense)
    _check(ctx, dense, [299, 1, 64, 63], 100, 901)
    ctx.close()


def test_variable_length_records():
    from genome_graph_annotation_amd import _lib as L
    dense = _dense(1000, 64, 0.5, 21)  # (64 columns: the variable-length records need a uniform tree)
    ctx = _form(dense, 8, L.MBRWT_BUILD_ROWS_VAR, 1)
    assert ctx.rows_stats()["variable"]
    _check(ctx, dense)
    _check(ctx, dense, [63, 0, 13], 12, 990)
    ctx.set_option(L.MBRWT_OPT_COLUMNS_CHUNK, 13)
    _check(ctx, dense, [63, 0, 13], 12, 990)
    ctx.close()


def test_record_classes():
    from genome_graph_annotation_amd import _lib as L
    kinds = _dense(9, 65, 0.2, 33)
    dense = kinds[np.random.default_rng(4).integers(0, 9, 1000)]
    ctx = _form(dense, 8, L.MBRWT_BUILD_ROWS_CLASSES, 1)
    assert 0 < ctx.rows_stats()["classes"] <= 9
    _check(ctx, dense)
    _check(ctx, dense, [64, 0, 13], 12, 990)
    ctx.set_option(L.MBRWT_OPT_COLUMNS_CHUNK, 100)
    _check(ctx, dense, list(range(65))[::-1], 1, 999)
    ctx.close()


# ---- shapes whose pre-order is not column order ------------------------------------------

@pytest.mark.parametrize("relax", [0, 10])
def test_greedy_shapes(oracle_mod, relax):
    """Slot order is the caller's, not the tree's pre-order."""
    dense, part, arity = _golden("greedy_relax_small.npz")
    ex = oracle_mod.OracleTree.from_dense(dense, part, arity, relax).export()
    ctx = _from_rows(dense, shape=_shape(ex))
    m = dense.shape[1]
    _check(ctx, dense)
    _check(ctx, dense, list(range(m))[::-1], 17, dense.shape[0] - 5)
    ctx.close()


# ---- wide keys ---------------------------------------------------------------------------

def test_wide_keys():
    """m = 65,536: 65,536 slots beside the "not asked for" value of the slot map."""
    n, m = 65, 65536
    rng = np.random.default_rng(3)
    dense = np.zeros((n, m), dtype=bool)
    for r in range(n):
        dense[r, rng.integers(0, m, 5)] = True
    dense[::2, 0] = True
    dense[1::2, m - 1] = True
    dense[7, [0, 1, m - 2, m - 1]] = True
    ctx = _from_rows(dense, arity=64)
    off, rows = ctx.get_columns()
    woff, wrows = _sparse(dense)
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(rows, wrows)
    _check(ctx, dense, [65535, 0])
    ctx.close()


# ---- other layouts -------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["nodes", "both"])
def test_layouts_from_columns(layout):
    from genome_graph_annotation_amd import BRWTDevice
    dense = _dense(1000, 65, 0.1, 13)
    ctx = BRWTDevice.from_columns(_packed_columns(dense), 1000, arity=4, layout=layout)
    assert ctx.layout() == layout
    _check(ctx, dense)
    _check(ctx, dense, list(range(65))[::-1], 63, 901)
    _check(ctx, dense, [], 0, 10)
    ctx.close()


def test_row_shards(oracle_mod):
    from genome_graph_annotation_amd import BRWTDevice
    from genome_graph_annotation_amd.brwt import build_layout
    from test_gpu_shards import _sharded
    dense = _dense(500, 20, 0.2, 3)
    t = oracle_mod.OracleTree.from_dense(dense, "basic", 2, 0)
    with build_layout("nodes"):
        ctx = _sharded(64, lambda: BRWTDevice.from_tree(t.export()))
    assert ctx.num_shards() == 8
    _check(ctx, dense)
    _check(ctx, dense, list(range(20))[::-1], 60, 130)  # straddles the shard boundaries 64 and 128
    ctx.close()


# ---- capacity and errors -------------------------------------------------------------------

def _raw(ctx, columns, k, b, e, offsets, rows, cap):
    from genome_graph_annotation_amd import _lib as L
    need = C.c_uint64(0)
    st = L.lib().mbrwt_get_columns(ctx._h, None if columns is None else columns.ctypes.data_as(U64P), k, b, e,
                                   offsets.ctypes.data_as(U64P), None if rows is None else rows.ctypes.data_as(U64P),
                                   cap, C.byref(need))
    return st, int(need.value)


def test_capacity(lists_ctx):
    from genome_graph_annotation_amd import _lib as L
    ctx, dense = lists_ctx
    n, m = dense.shape
    woff, wrows = _expect(dense)
    total = len(wrows)
    SENT = np.uint64(0xDEADBEEFDEADBEEF)
    off = np.zeros(m + 1, dtype=np.uint64)
    rows = np.full(total, SENT, dtype=np.uint64)
    st, need = _raw(ctx, None, m, 0, n, off, rows, total - 1)
    assert st == L.MBRWT_ERR_CAPACITY and need == total
    np.testing.assert_array_equal(off, woff)  # complete
    assert (rows == SENT).all()               # untouched
    off[:] = 0
    st, need = _raw(ctx, None, m, 0, n, off, rows, total)
    assert st == L.MBRWT_OK and need == total
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(rows, wrows)
    # NULL rows: refused with a total, fine without one
    st, need = _raw(ctx, None, m, 0, n, off, None, 0)
    assert st == L.MBRWT_ERR_CAPACITY and need == total
    seven = np.array([7], dtype=np.uint64)
    off1 = np.ones(2, dtype=np.uint64)
    st, need = _raw(ctx, seven, 1, 0, n, off1, None, 0)
    assert st == L.MBRWT_OK and need == 0 and off1.tolist() == [0, 0]
    # rows_needed may be NULL
    assert L.lib().mbrwt_get_columns(ctx._h, seven.ctypes.data_as(U64P), 1, 0, n, off1.ctypes.data_as(U64P), None, 0,
                                     None) == L.MBRWT_OK


def test_errors(lists_ctx):
    from genome_graph_annotation_amd import _lib as L
    ctx, dense = lists_ctx
    n, m = dense.shape
    off = np.zeros(m + 2, dtype=np.uint64)
    rows = np.zeros(dense.sum() + 1, dtype=np.uint64)

    def call(columns, k, b, e):
        columns = None if columns is None else np.array(columns, dtype=np.uint64)
        return _raw(ctx, columns, k, b, e, off, rows, len(rows))[0]

    assert call([0, m], 2, 0, n) == L.MBRWT_ERR_RANGE
    assert call([3, 3], 2, 0, n) == L.MBRWT_ERR_INVALID
    assert "3" in (L.lib().mbrwt_last_error_message() or b"").decode()
    assert call([1], 1, 0, n + 1) == L.MBRWT_ERR_RANGE
    assert call([1], 1, 5, 4) == L.MBRWT_ERR_RANGE
    assert call(None, m - 1, 0, n) == L.MBRWT_ERR_INVALID
    assert L.lib().mbrwt_get_columns(ctx._h, None, m, 0, n, None, rows.ctypes.data_as(U64P), len(rows),
                                     None) == L.MBRWT_ERR_INVALID
    assert call(None, m, 0, n) == L.MBRWT_OK
    assert call(None, 0, 0, n) == L.MBRWT_OK  # no column: legal


# ---- device form -----------------------------------------------------------------------------

def test_device_form(windows_ctx):
    """torch tensors on a non-default stream, two calls back to back with
    different windows, after a get_rows_device_async queued on another stream
    (the workspace fence): everything as the host form."""
    import torch
    from genome_graph_annotation_amd import MBRWTError, _lib as L
    ctx, dense = windows_ctx
    n, m = dense.shape
    columns = [64, 0, 33, 5]
    s_rows, s_cols = torch.cuda.Stream(), torch.cuda.Stream()
    q = np.random.default_rng(2).integers(0, n, 4000).astype(np.uint64)
    q_t = torch.from_numpy(q.view(np.int64)).cuda()
    ro_t = torch.empty(len(q) + 1, dtype=torch.int64, device="cuda")
    rc_t = torch.empty(int(dense[q.astype(np.int64)].sum()) + 1, dtype=torch.int32, device="cuda")
    st_t = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.get_rows_device_async(q_t, ro_t, rc_t, st_t, s_rows.cuda_stream)
    outs = []
    for b, e in ((10, 700), (0, n)):
        woff, wrows = _expect(dense, columns, b, e)
        off_t = torch.full((len(columns) + 1,), -1, dtype=torch.int64, device="cuda")
        rows_t = torch.full((len(wrows) + 3,), -1, dtype=torch.int64, device="cuda")
        got = ctx.get_columns_device(columns, b, e, off_t, rows_t, s_cols.cuda_stream)
        outs.append((got, off_t, rows_t, woff, wrows))
    torch.cuda.synchronize()
    for got, off_t, rows_t, woff, wrows in outs:
        assert got == len(wrows)
        np.testing.assert_array_equal(off_t.cpu().numpy().view(np.uint64), woff)
        np.testing.assert_array_equal(rows_t.cpu().numpy().view(np.uint64)[:got], wrows)
        assert (rows_t.cpu().numpy()[got:] == -1).all()
    want_off = np.zeros(len(q) + 1, dtype=np.uint64)
    want_off[1:] = np.cumsum(dense[q.astype(np.int64)].sum(axis=1))
    assert st_t.cpu().numpy()[1] == L.MBRWT_OK
    np.testing.assert_array_equal(ro_t.cpu().numpy().view(np.uint64), want_off)
    np.testing.assert_array_equal(rc_t.cpu().numpy()[:-1].view(np.uint32), np.nonzero(dense[q.astype(np.int64)])[1])
    # all columns, sizing only, then too small: the offsets are complete
    woff, wrows = _expect(dense)
    off_t = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(MBRWTError) as err:
        ctx.get_columns_device(None, 0, None, off_t, None, s_cols.cuda_stream)
    assert err.value.status == L.MBRWT_ERR_CAPACITY and err.value.needed == len(wrows)
    np.testing.assert_array_equal(off_t.cpu().numpy().view(np.uint64), woff)


# ---- round trip ---------------------------------------------------------------------------------

def _as_dense(ctx):
    n, m = ctx.num_rows(), ctx.num_columns()
    off, cols = ctx.get_rows(np.arange(n, dtype=np.uint64))
    out = np.zeros((n, m), dtype=bool)
    out[np.repeat(np.arange(n), np.diff(off.astype(np.int64))), cols.astype(np.int64)] = True
    return out


def test_round_trip(oracle_mod):
    from genome_graph_annotation_amd import BRWTDevice
    from genome_graph_annotation_amd.brwt import shape_from_sparse_columns
    dense = _dense(1000, 70, 0.03, 2)
    n, m = dense.shape
    ex = oracle_mod.OracleTree.from_dense(dense, "basic", 4).export()
    src = BRWTDevice.from_rows(*_csr_mixed(dense, "mixed", seed=1), m, shape=_shape(ex))
    off, rows = src.to_sparse_columns()
    np.testing.assert_array_equal(off, _sparse(dense)[0])
    np.testing.assert_array_equal(rows, _sparse(dense)[1])
    back = BRWTDevice.from_sparse_columns(off, rows, n, m, shape=_shape(ex))
    _same_context(back, src)
    back.close()
    # the image re-partitioned under the greedy + relax shape: the same label sets
    shape = shape_from_sparse_columns(off, rows, n, m, partitioner="greedy", relax_max_arity=10)
    other = BRWTDevice.from_sparse_columns(off, rows, n, m, shape=shape)
    np.testing.assert_array_equal(_as_dense(other), dense)
    np.testing.assert_array_equal(_as_dense(src), dense)
    other.close()
    src.close()


# ---- one ranged build --------------------------------------------------------------------------

def test_ranged_build_window():
    """2 x 360,360 + 17 rows built in three ranges; a window over both range
    boundaries (the only case above 10^5 rows)."""
    from genome_graph_annotation_amd import _lib as L
    from genome_graph_annotation_amd.brwt import build_option
    n, m, arity = 2 * ALIGN + 17, 16, 4
    dense = np.random.default_rng(77).random((n, m)) < 0.1
    dense[:, 1] = False
    dense[:, 2] = False
    dense[[ALIGN - 1, ALIGN, 2 * ALIGN - 1, 2 * ALIGN], 2] = True
    dense[:, 4] = True
    with build_option(L.MBRWT_BUILD_ROWS_RANGE, ALIGN):
        ctx = _from_rows(dense, arity=arity)
    b, e = ALIGN - 5, 2 * ALIGN + 5
    off, rows = ctx.get_columns(None, b, e)
    woff, wrows = _sparse(dense[b:e])
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(rows, wrows + np.uint64(b))
    ctx.close()
