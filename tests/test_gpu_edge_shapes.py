"""GPU parity at the exact boundaries of the row-record output path and of
the classify kernels, on the deterministic fixture of tests/edge_shapes.py
(the staircase matrix: every label count 0..m, so every inline / spill /
long record boundary of every block shape lies on some row) instead of a
random law.  Every comparison is bit-exact on integers, against the CPU
oracle and against the fixture's closed form.

get_rows (csrc/rows.hip k_traverse_rows -> k_compact_tiles):
  * the inline count byte (a row of >= 255 labels spills): sweep_rows, geometry
  * a spill entry equal to / longer than a block: sweep_rows under every
    block shape (test_staircase_rows[bs-*], [m2652-*])
  * a tile total <= 512 or > 512, <= C or > C: tile_totals, copies, with
    C = 1024 / 2048 / 4096 ([C1024], [C2048], the others)
  * four tiles per compaction wave, a partial last tile, offsets[n] stored by
    lane nr - 1: geometry
  * the labels-per-row limit of the 15-bit temp count: test_labels_per_row_limit
get_column's capacity protocol (csrc/rows_select.hpp) and the point queries'
empty batch / one row / row == num_rows (finish_record_call), on a block, a
variable-length and a record-class form: test_get_column_capacity_protocol,
test_point_queries_protocol.
classify (csrc/classify.hip): test_classify_*.
The untested fallback of a ranged build: test_ranged_terminal_limit.
"""
import contextlib
import math

import numpy as np
import pytest

import edge_shapes as E
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]


# ---- the reference: one oracle CSR of all rows per matrix, shared ----------

class _Case:
    """A matrix, its oracle tree and the oracle's CSR of every row."""

    def __init__(self, O, dense, part, arity, relax):
        self.dense = dense
        self.n, self.m = dense.shape
        self.t = O.OracleTree.from_dense(dense, part, arity, relax)
        self.ex = self.t.export()
        self.off, self.cols = self.t.get_rows(np.arange(self.n, dtype=np.uint64))
        self.counts = dense.sum(axis=1).astype(np.int64)
        self.closed = True   # the rows' labels are prefixes [0, count)


_cases = {}


def _staircase_case(O, m, pad, kind, part, arity, relax):
    """kind: the pad rows -- False empty, True rows 0..m repeated, "single" one label each."""
    key = (m, pad, kind, part, arity, relax)
    if key not in _cases:
        repeat, single = kind is True, kind == "single"
        c = _Case(O, E.staircase(m, pad, repeat, single), part, arity, relax)
        np.testing.assert_array_equal(c.counts, E.staircase_count(np.arange(c.n), m, repeat, single))
        c.closed = not single
        head = slice(0, c.n if c.closed else m + 1)   # the oracle against the closed form, once
        assert E.closed_form_ok(c.off[: head.stop + 1], c.cols[: int(c.off[head.stop])], c.counts[head])
        _cases[key] = c
    return _cases[key]


def _check_batch(dev, case, rows, name, extra=False, closed=True):
    """`rows` through get_rows (host), get_rows_device and
    get_rows_device_async (cap = total; cap = total - 1: MBRWT_ERR_CAPACITY
    and nothing written past cap) against the oracle and the closed form;
    extra: count_labels_device and get_batch too."""
    import torch
    from genome_graph_annotation_amd import _lib as L
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    off_e, cols_e = E.gather_csr(case.off, case.cols, rows)
    cnt = case.counts[rows.astype(np.int64)]
    if closed and (case.closed or int(rows.max(initial=0)) <= case.m):
        assert E.closed_form_ok(off_e, cols_e, cnt), name
    tot = len(cols_e)
    off_h, cols_h = dev.get_rows(rows)
    np.testing.assert_array_equal(off_h, off_e, err_msg=f"{name}: get_rows offsets")
    np.testing.assert_array_equal(cols_h, cols_e, err_msg=f"{name}: get_rows labels")
    s = torch.cuda.current_stream().cuda_stream
    rt = torch.from_numpy(rows.view(np.int64)).cuda()
    ot = torch.full((len(rows) + 1,), -1, dtype=torch.int64, device="cuda")
    ct = torch.full((tot + 64,), -1, dtype=torch.int32, device="cuda")
    got = dev.get_rows_device(rt, ot, ct[:max(tot, 1)], s)
    torch.cuda.synchronize()
    assert got == tot, name
    np.testing.assert_array_equal(ot.cpu().numpy().view(np.uint64), off_e, err_msg=f"{name}: device offsets")
    np.testing.assert_array_equal(ct[:tot].cpu().numpy().view(np.uint32), cols_e, err_msg=f"{name}: device labels")
    assert (ct[tot:] == -1).all(), f"{name}: a label written past the total"
    st = torch.zeros(3, dtype=torch.int64, device="cuda")
    for cap in ((tot, tot - 1) if tot else (0,)):
        st.zero_()
        ct.fill_(-1)
        ot.fill_(-1)
        dev.get_rows_device_async(rt, ot, ct[:cap], st, s)
        torch.cuda.synchronize()
        need, status, sticky = st.cpu().tolist()
        assert need == tot, (name, cap, need, tot)
        if cap >= tot:
            assert status == L.MBRWT_OK and sticky == 1 << L.MBRWT_OK, (name, cap, status, sticky)
            np.testing.assert_array_equal(ot.cpu().numpy().view(np.uint64), off_e, err_msg=f"{name}: async offsets")
            np.testing.assert_array_equal(ct[:tot].cpu().numpy().view(np.uint32), cols_e,
                                          err_msg=f"{name}: async labels")
        else:
            assert status == L.MBRWT_ERR_CAPACITY and sticky == 1 << L.MBRWT_ERR_CAPACITY, (name, cap, status)
        assert (ct[cap:] == -1).all(), f"{name}: a label written past the capacity {cap}"
    if extra:
        from test_gpu_rows import _count_labels
        np.testing.assert_array_equal(_count_labels(dev, rows), np.bincount(cols_e, minlength=case.m),
                                      err_msg=f"{name}: count_labels")
        # point queries on each row's last set and first unset column
        for qc in (np.maximum(cnt - 1, 0), np.minimum(cnt, case.m - 1)):
            want = case.dense[rows.astype(np.int64), qc]
            np.testing.assert_array_equal(dev.get_batch(rows, qc.astype(np.uint64)), want,
                                          err_msg=f"{name}: get_batch")


def _all_batches(dev, case, m):
    """Every batch of the fixture (ids of the staircase's first m + 1 rows)."""
    _check_batch(dev, case, E.sweep_rows(m), "sweep")
    for lo, hi in E.TILE_TOTAL_WINDOWS:
        _check_batch(dev, case, E.tile_totals(m, lo, hi), f"tile_totals {lo}..{hi}")
    for k in E.geometry_heavy(m):
        for name, rows in E.geometry(m, k):
            _check_batch(dev, case, rows, f"geometry k={k} {name}", extra=True)
    for name, rows in E.copies(m):
        _check_batch(dev, case, rows, f"copies {name}")
    if case.n > m + 1:  # the pad rows: the matrix's last rows, a partial tile
        _check_batch(dev, case, np.arange(case.n - 200, case.n, dtype=np.uint64), "pad rows")


def _full_row_mask_bytes(ex):
    """Byte-mask bytes of a full row's record: one mask of ceil(children / 8)
    bytes per internal node (a full row reaches every node)."""
    nc = np.asarray(ex["num_children"]).astype(np.int64)
    return int(((nc[nc > 0] + 7) // 8).sum())


# name -> (m, pad, repeat, (partitioner, arity, relax), layout, build options, expectation)
_ROWS = "rows"
_BLOCK_BYTES = {"MBRWT_ROWS_VAR": 0, "MBRWT_ROWS_CODE": 3}   # block records of byte masks
_CONFIGS = {
    "terminal-default": (700, 0, False, ("basic", 8, 0), _ROWS, {"MBRWT_ROWS_VAR": 0}, "default-code"),
    # (15,000 rows of one label: three bytes as terminal fields, five as byte masks -- more
    # than the staircase's dense rows lose, so the forced terminal records are kept)
    "terminal-forced-padded": (700, 15000, "single", ("basic", 8, 0), _ROWS,
                               {"MBRWT_ROWS_VAR": 0, "MBRWT_ROWS_CODE": 2, "classes": 0}, "forced-terminal"),
    "byte-masks": (700, 0, False, ("basic", 8, 0), _ROWS, {"MBRWT_ROWS_VAR": 0, "MBRWT_ROWS_CODE": 3}, "bytes"),
    "nibble-codes": (700, 0, False, ("basic", 8, 0), _ROWS, {"MBRWT_ROWS_VAR": 0, "MBRWT_ROWS_CODE": 1}, "nibble"),
    "walks": (700, 0, False, ("basic", 8, 0), _ROWS, {"MBRWT_ROWS_VAR": 0, "MBRWT_ROWS_CODE": 3}, "walks"),
    "tree-odometer": (700, 0, False, ("greedy", 2, 10), _ROWS, {"MBRWT_ROWS_VAR": 0, "MBRWT_ROWS_CODE": 3},
                      "bytes-tree"),
    "two-byte-masks": (700, 0, False, ("basic", 16, 0), _ROWS, _BLOCK_BYTES, "bytes-tree"),
    "wide-nodes": (700, 0, False, ("basic", 33, 0), _ROWS, {"MBRWT_ROWS_VAR": 0}, "wide"),
    "bs-64,1": (700, 0, False, ("basic", 8, 0), _ROWS, dict(_BLOCK_BYTES, MBRWT_ROWS_BS="64,1"), "bytes"),
    "bs-64,8": (700, 0, False, ("basic", 8, 0), _ROWS, dict(_BLOCK_BYTES, MBRWT_ROWS_BS="64,8"), "bytes"),
    "bs-128,1": (700, 0, False, ("basic", 8, 0), _ROWS, dict(_BLOCK_BYTES, MBRWT_ROWS_BS="128,1"), "bytes"),
    "bs-128,15": (700, 0, False, ("basic", 8, 0), _ROWS, dict(_BLOCK_BYTES, MBRWT_ROWS_BS="128,15"), "bytes"),
    # labels / rows <= 11: the smallest tile capacity (C = 1024); <= 27: the middle one
    # (classes 0: the repeated empty rows would otherwise be taken as record classes)
    "C1024": (700, 22300, False, ("basic", 8, 0), _ROWS, dict(_BLOCK_BYTES, classes=0), "bytes"),
    "C2048": (700, 11500, False, ("basic", 8, 0), _ROWS, dict(_BLOCK_BYTES, classes=0), "bytes"),
    "C1024-auto-classes": (700, 22300, False, ("basic", 8, 0), _ROWS, dict(_BLOCK_BYTES, classes=-1), "classes"),
    "m2652": (2652, 0, False, ("basic", 8, 0), _ROWS, {"MBRWT_ROWS_VAR": 0, "MBRWT_ROWS_CODE": 3}, "bytes"),
    # (at m = 700 no spill entry outgrows a 128-byte block; at m = 2652 they do)
    "m2652-bs-128,3": (2652, 0, False, ("basic", 8, 0), _ROWS, dict(_BLOCK_BYTES, MBRWT_ROWS_BS="128,3"), "bytes"),
    "var-8": (700, 0, False, ("basic", 8, 0), _ROWS, {"MBRWT_ROWS_VAR": 1}, "variable"),
    "var-8-G1": (700, 0, False, ("basic", 8, 0), _ROWS, {"MBRWT_ROWS_VAR": 1, "MBRWT_VAR_G": "1"}, "variable"),
    # (binary: the variable-length records need a uniform tree of at most 5 levels
    # above the leaf parents -- 64 columns; a tile then totals at most 4,096)
    "var-2": (64, 0, False, ("basic", 2, 0), _ROWS, {"MBRWT_ROWS_VAR": 1}, "variable"),
    "var-2-G1": (64, 0, False, ("basic", 2, 0), _ROWS, {"MBRWT_ROWS_VAR": 1, "MBRWT_VAR_G": "1"}, "variable"),
    "var-2-block": (700, 0, False, ("basic", 2, 0), _ROWS, {"MBRWT_ROWS_VAR": 1, "MBRWT_ROWS_CODE": 3}, "bytes-tree"),
    "classes": (700, 3 * 701, True, ("basic", 8, 0), _ROWS, {"MBRWT_ROWS_VAR": 0, "classes": 1}, "classes"),
    "nodes": (700, 0, False, ("basic", 8, 0), "nodes", {}, "nodes"),
    "auto": (700, 0, False, ("basic", 8, 0), None, {}, "auto"),
}


@pytest.mark.parametrize("name", list(_CONFIGS))
def test_staircase_rows(oracle_mod, build_env, name):
    """Every batch of the fixture through every get_rows entry point (and
    count_labels / get_batch on the geometry batches), on one built form per
    case; the form is asserted first (layout, record code, block shape,
    spilled and long rows, the variable flag)."""
    O = oracle_mod
    from genome_graph_annotation_amd import BRWTDevice, _lib as L
    from genome_graph_annotation_amd.brwt import build_option
    m, pad, repeat, (part, arity, relax), layout, opts, expect = _CONFIGS[name]
    case = _staircase_case(O, m, pad, repeat, part, arity, relax)
    opts = dict(opts)
    classes = opts.pop("classes", None)
    for k, v in opts.items():
        build_env(k, v)
    if classes is not None:
        with build_option(L.MBRWT_BUILD_ROWS_CLASSES, classes):
            dev = BRWTDevice.from_tree(case.ex, layout=layout)
    else:
        dev = BRWTDevice.from_tree(case.ex, layout=layout)
    st = dev.rows_stats()
    print(name, dev.layout(), dev.traverse_kernel(), st)
    # -- the built form ---------------------------------------------------
    if expect == "nodes":
        assert dev.layout() == "nodes" and st is None
        # (a full row's record under the 512-column root child is over a record block's 64
        # bytes, so that child is not packed: no rowblock kernel and no fast2 on this tree.
        # Their edges are tests/test_gpu_node_edges.py's.)
        assert dev.traverse_kernel() == "k_traverse_group", dev.traverse_kernel()
    elif expect == "auto":
        # whatever AUTO picks must be exact; dense rows of a uniform tree:
        # the variable-length records (test_auto_layout) or the node images
        assert dev.layout() in ("rows", "nodes")
        assert dev.layout() == "nodes" or dev.traverse_kernel() in ("k_traverse_rows", "k_var_decode")
    else:
        kernel = "k_var_decode" if expect == "variable" else "k_traverse_rows"
        assert dev.layout() == "rows" and dev.traverse_kernel() == kernel, (dev.layout(), dev.traverse_kernel())
        assert dev.num_relations() == int(case.counts.sum())
    if expect == "variable":
        assert st["variable"], st
    elif expect not in ("nodes", "auto"):
        assert not st["variable"], st
        # rows of >= 255 labels always spill: m - 254 of them in every copy of the staircase
        copies_of = 1 + (pad // (m + 1) if repeat is True else 0)
        if expect != "classes":   # (classes: one record per distinct row)
            assert st["spilled_rows"] >= (m - 254) * copies_of, st
        if "MBRWT_ROWS_BS" in opts:
            assert (st["block_bytes"], st["rows_per_block"]) == tuple(int(x) for x in opts["MBRWT_ROWS_BS"].split(","))
    if expect in ("bytes", "bytes-tree", "walks", "wide"):
        assert not st["nibble_codes"], st
        if expect != "wide":
            assert not st["terminal_records"], st
            # a full row's spill entry (8 + its mask bytes) against the block
            assert (st["long_rows"] > 0) == (8 + _full_row_mask_bytes(case.ex) > st["block_bytes"]), st
            assert st["record_bytes"] >= _full_row_mask_bytes(case.ex) + case.n
        if m == 2652:
            assert st["long_rows"] > 0, st
    if expect in ("bytes", "walks"):
        assert st["uniform_levels"] > 0, st   # a uniform tree: the path odometer
    if expect == "bytes-tree":
        assert st["uniform_levels"] == 0, st  # greedy + relax: the tree odometer
    if expect == "wide":
        assert int(np.asarray(case.ex["num_children"]).max()) > 16
    if expect in ("default-code", "nibble", "forced-terminal"):
        # MBRWT_BUILD_ROWS_CODE (include/mbrwt.h): the
        # smaller code is kept where it shrinks the first range's records,
        # byte masks otherwise -- the staircase's dense rows favour bytes, the
        # padded one's one-label rows the terminal fields
        with build_option(L.MBRWT_BUILD_ROWS_CODE, 3):
            plain = BRWTDevice.from_tree(case.ex, layout="rows").rows_stats()
        flag = "nibble_codes" if expect == "nibble" else "terminal_records"
        assert st["record_bytes"] <= plain["record_bytes"], (st, plain)
        assert st[flag] == (st["record_bytes"] < plain["record_bytes"]), (st, plain)
        assert not st["terminal_records" if expect == "nibble" else "nibble_codes"], st
        if expect == "forced-terminal":
            assert st["terminal_records"] and st["long_rows"] > 0, (st, plain)
    if expect == "classes":
        assert st["classes"] == m + 1 and st["rows_per_block"] == 1, st
    elif st is not None:
        assert st.get("classes", 0) == 0, st
    # -- the batches --------------------------------------------------------
    if expect == "walks":
        for walk in (6, 4):   # the mask-1 walk, the general walk
            dev.set_option(L.MBRWT_OPT_ROWS_WALK, walk)
            _all_batches(dev, case, m)
        return
    _all_batches(dev, case, m)
    if expect == "classes":  # the repeated rows
        _check_batch(dev, case, np.arange(case.n, dtype=np.uint64)[::-1], "every row, reversed")


# ---- the small drivers the three record forms share ----------------------------

_FORMS = {"blocks": "byte-masks", "variable": "var-8", "classes": "classes"}   # form -> its _CONFIGS entry
_forms = {}


def _short_staircase(O, name):
    """The staircase of _CONFIGS[name] with its last column cleared: the
    longest row is shorter than the width, so no row holds column m - 1."""
    m, pad, kind, (part, arity, relax), _, _, _ = _CONFIGS[name]
    key = ("short", m, pad, kind, part, arity, relax)
    if key not in _cases:
        dense = E.staircase(m, pad, kind is True)
        dense[:, m - 1] = False
        _cases[key] = _Case(O, dense, part, arity, relax)
    return _cases[key]


def _record_form(O, build_env, form):
    """One built form of the short staircase under the build options of its
    _CONFIGS entry, asserted through rows_stats(); shared by the tests below."""
    from genome_graph_annotation_amd import BRWTDevice, _lib as L
    from genome_graph_annotation_amd.brwt import build_option
    case = _short_staircase(O, _FORMS[form])
    if form not in _forms:
        opts = dict(_CONFIGS[_FORMS[form]][5])
        classes = opts.pop("classes", None)
        for k, v in opts.items():
            build_env(k, v)
        with build_option(L.MBRWT_BUILD_ROWS_CLASSES, classes) if classes is not None else contextlib.nullcontext():
            dev = BRWTDevice.from_tree(case.ex, layout="rows")
        st = dev.rows_stats()
        assert dev.layout() == "rows", dev.layout()
        assert bool(st["variable"]) == (form == "variable"), st
        assert (st.get("classes", 0) > 0) == (form == "classes"), st
        _forms[form] = dev
    return _forms[form], case


@pytest.mark.parametrize("form", list(_FORMS))
def test_get_column_capacity_protocol(oracle_mod, build_env, form):
    """mbrwt_get_column_device on each record form (include/mbrwt.h): a null
    buffer sizes the column -- *rows_needed = its rows, MBRWT_OK for a column
    no row holds, MBRWT_ERR_CAPACITY otherwise (rows_cap counts as 0); rows_cap
    one short is MBRWT_ERR_CAPACITY with the size and 'rows_cap too small';
    rows_cap = the size gives the oracle's ascending rows and writes nothing
    past them; column == num_columns is MBRWT_ERR_RANGE."""
    import ctypes as C
    import torch
    from genome_graph_annotation_amd import _lib as L
    dev, case = _record_form(oracle_mod, build_env, form)
    lib, m = L.lib(), case.m

    def call(col, buf, cap):
        need = C.c_uint64(2**64 - 1)
        st = lib.mbrwt_get_column_device(dev._h, col, buf.data_ptr() if buf is not None else None, cap,
                                         C.byref(need), None)
        torch.cuda.synchronize()
        return st, int(need.value), (lib.mbrwt_last_error_message() or b"").decode()

    copies = case.n // (m + 1)
    for col in (0, 254, m - 2):
        want = np.asarray(case.t.get_column(col), dtype=np.uint64)
        np.testing.assert_array_equal(want, np.nonzero(case.dense[:, col])[0])
        k = len(want)
        assert k == (m - col) * copies > 0   # rows col + 1 .. m of every copy of the staircase
        st, need, msg = call(col, None, 0)
        print(form, col, "null buffer:", st, need)
        assert (st, need) == (L.MBRWT_ERR_CAPACITY, k) and "rows_cap too small" in msg, (col, st, need, msg)
        buf = torch.full((k + 8,), -1, dtype=torch.int64, device="cuda")
        st, need, msg = call(col, buf, k - 1)
        assert (st, need) == (L.MBRWT_ERR_CAPACITY, k) and "rows_cap too small" in msg, (col, st, need, msg)
        assert "rows_cap too small" in L.MBRWTError(st).args[0]
        assert (buf == -1).all(), "rows written under MBRWT_ERR_CAPACITY"
        st, need, _ = call(col, buf, k)
        assert (st, need) == (L.MBRWT_OK, k), (col, st, need)
        np.testing.assert_array_equal(buf[:k].cpu().numpy().view(np.uint64), want, err_msg=f"column {col}")
        assert (buf[k:] == -1).all(), "a row written past the column's size"
        np.testing.assert_array_equal(dev.get_column(col), want, err_msg=f"column {col} (host)")
    # the column no row holds
    assert not case.dense[:, m - 1].any() and len(case.t.get_column(m - 1)) == 0
    assert call(m - 1, None, 0)[:2] == (L.MBRWT_OK, 0)
    buf = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    assert call(m - 1, buf, 8)[:2] == (L.MBRWT_OK, 0) and (buf == -1).all()
    assert len(dev.get_column(m - 1)) == 0
    # column == num_columns
    assert dev.num_columns() == m
    st, _, msg = call(m, buf, 8)
    assert st == L.MBRWT_ERR_RANGE and "column out of range" in msg, (st, msg)
    assert call(m, None, 0)[0] == L.MBRWT_ERR_RANGE


@pytest.mark.parametrize("form", list(_FORMS))
def test_point_queries_protocol(oracle_mod, build_env, form):
    """get_batch, count_labels and the work count (V, L) on each record form:
    an empty batch, one in-range row, and a batch whose last row is num_rows
    (MBRWT_ERR_RANGE)."""
    import ctypes as C
    import torch
    from genome_graph_annotation_amd import _lib as L
    dev, case = _record_form(oracle_mod, build_env, form)
    lib, m, n = L.lib(), case.m, case.n
    assert dev.num_rows() == n

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
        cnt = torch.full((m,), 7, dtype=torch.int64, device="cuda")
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
    # one in-range row: row r holds the columns [0, r)
    r = 300
    assert case.counts[r] == r
    st, out = get_batch([r, r], [r - 1, r])
    assert st == L.MBRWT_OK and out.tolist() == [1, 0]
    st, cnt = count_labels([r])
    assert st == L.MBRWT_OK
    np.testing.assert_array_equal(cnt, (np.arange(m) < r).astype(np.int64))
    _, cols_o, vis = case.t.get_rows(np.array([r], dtype=np.uint64), with_visits=True)
    assert len(cols_o) == r
    assert count_work([r]) == (L.MBRWT_OK, int(vis.sum()), r)
    # the last row of the batch is num_rows
    assert get_batch([r, 0, n], [0, 0, 0])[0] == L.MBRWT_ERR_RANGE
    assert count_labels([r, 0, n])[0] == L.MBRWT_ERR_RANGE
    assert count_work([r, 0, n])[0] == L.MBRWT_ERR_RANGE
    # (and the context still answers)
    assert get_batch([r], [0])[1].tolist() == [1]


# ---- the labels-per-row limit of the records ------------------------------------

_HEAVY = {32767: (32767,), 32768: (32767, 32768), 40000: (32767, 32768, 40000), 65536: (65536,), 4096: (4096,)}


def _heavy_case(O, m, arity, heaviest):
    """300 sparse rows (about 3 labels a row, rows 0..9 empty) and hand-placed
    heavy rows (prefixes [0, k)) at ids 300.., the heaviest last."""
    key = ("heavy", m, arity, heaviest)
    if key not in _cases:
        rng = np.random.default_rng(m + heaviest)
        ks = _HEAVY[heaviest]
        dense = np.zeros((300 + len(ks), m), dtype=bool)
        dense[:300] = rng.random((300, m)) < 3.0 / m
        dense[:10] = False
        dense[10:300, m - 1] |= rng.random(290) < 0.5   # (the last column in use)
        for i, k in enumerate(ks):
            dense[300 + i, :k] = True
        _cases[key] = _Case(O, dense, "basic", arity, 0)
    return _cases[key]


def _heavy_batches(case):
    """The heavy rows first, last and mid-tile, next to empty rows and next to
    each other."""
    h = np.arange(300, case.n, dtype=np.uint64)
    sparse = np.arange(10, 300, dtype=np.uint64)
    e = np.zeros(3, dtype=np.uint64)
    yield "heavy alone", h[-1:]
    yield "heavy first/mid/last", np.concatenate([h[-1:], e, sparse[:27], h, h[::-1], e, sparse[27:100], e, h[-1:]])
    yield "heavy mid-tile among empty rows", np.concatenate([np.zeros(31, np.uint64), h[-1:], np.zeros(40, np.uint64)])
    yield "heavy on a partial tile's last lane", np.concatenate([sparse[:64], e, h[:1]])
    yield "every row", np.arange(case.n, dtype=np.uint64)


def _exact_or_refused(case, opts_env, must_build, expect_variable=None):
    """The contract of a row beyond the records' labels-per-row limit: layout
    'rows' answers bit-exactly or is refused with MBRWT_ERR_UNSUPPORTED, AUTO
    answers bit-exactly (the node images after a refusal); never a wrong CSR."""
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    try:
        dev = BRWTDevice.from_tree(case.ex, layout="rows")
    except MBRWTError as e:
        assert not must_build, f"within the records' limits, refused: {e}"
        assert e.status == L.MBRWT_ERR_UNSUPPORTED
        dev = None
    if dev is not None:
        assert dev.layout() == "rows"
        if expect_variable is not None:
            assert dev.rows_stats()["variable"] == expect_variable, dev.rows_stats()
        for name, rows in _heavy_batches(case):
            _check_batch(dev, case, rows, f"rows: {name}", extra=True, closed=False)
    auto = BRWTDevice.from_tree(case.ex)
    assert auto.layout() in ("rows", "nodes")
    if dev is None:
        assert auto.layout() == "nodes"
        small = BRWTDevice.from_tree(_small_tree(case), layout="rows")   # the refused build leaked nothing
        assert small.layout() == "rows"
    for name, rows in _heavy_batches(case):
        _check_batch(auto, case, rows, f"auto: {name}", extra=True, closed=False)
    return dev is not None


def _small_tree(case):
    import oracle as O
    return O.OracleTree.from_dense(case.dense[:300, :64], "basic", 8).export()


@pytest.mark.parametrize("m,arity,heaviest", [(40000, 8, 32767), (40000, 8, 32768), (40000, 8, 40000),
                                              (65536, 16, 65536)])
def test_labels_per_row_limit(oracle_mod, build_env, m, arity, heaviest):
    """A row's label count travels from k_traverse_rows to k_compact_tiles in
    15 bits (bit 15 flags a long record): 32,767 labels is the most a row of
    the block records can carry.  A matrix up to that builds as row records
    and answers bit-exactly; one beyond it answers bit-exactly or is refused
    (MBRWT_ERR_UNSUPPORTED under layout 'rows', the node images under AUTO).

    Before the limit was enforced in k_rows_measure, a row of 32,768 labels
    read back as 0 and one of 40,000 as 7,232: offsets[] of a silently wrong
    CSR beside a correct total."""
    build_env("MBRWT_ROWS_VAR", 0)
    build_env("MBRWT_ROWS_CODE", 3)
    case = _heavy_case(oracle_mod, m, arity, heaviest)
    assert int(case.counts.max()) == heaviest
    _exact_or_refused(case, None, must_build=heaviest <= 32767, expect_variable=False)


@pytest.mark.parametrize("m,arity,heaviest", [(4096, 4, 4096), (40000, 8, 32767), (40000, 8, 32768)])
def test_labels_per_row_limit_variable(oracle_mod, build_env, m, arity, heaviest):
    """The same with the variable-length records forced (k_var_measure holds
    the same 15-bit bound): a full row over 4,096 columns at arity 4 is
    variable and exact; at 40,000 columns whichever record layout the build
    takes is exact up to 32,767 labels, exact or refused beyond."""
    build_env("MBRWT_ROWS_VAR", 1)
    build_env("MBRWT_ROWS_CODE", 3)
    case = _heavy_case(oracle_mod, m, arity, heaviest)
    _exact_or_refused(case, None, must_build=heaviest <= 32767, expect_variable=True if m == 4096 else None)


# ---- classify boundaries (k_read_labels, k_read_top_labels) --------------------

def _read_counts(dense, rows, a, b):
    """Per-label counts of the read rows[a:b]: numpy over the dense rows
    (unique rows weighted by their multiplicity)."""
    u, mult = np.unique(np.asarray(rows[a:b], dtype=np.int64), return_counts=True)
    if not len(u):
        return np.zeros(dense.shape[1], dtype=np.int64)
    return mult.astype(np.int64) @ dense[u].astype(np.int64)


def _ref_labels(dense, rows, roff, ratio):
    out_off, out = [0], []
    for r in range(len(roff) - 1):
        a, b = int(roff[r]), int(roff[r + 1])
        cnt = _read_counts(dense, rows, a, b)
        thr = 1 if ratio == 0 else math.ceil((b - a) * ratio)   # (std::ceil in double)
        out.append(np.nonzero((cnt > 0) & (cnt >= thr))[0])
        out_off.append(out_off[-1] + len(out[-1]))
    return np.array(out_off, dtype=np.uint64), np.concatenate(out + [np.zeros(0, np.int64)]).astype(np.uint32)


def _ref_top(dense, rows, roff, num_top):
    out_off, labs, cnts = [0], [], []
    for r in range(len(roff) - 1):
        cnt = _read_counts(dense, rows, int(roff[r]), int(roff[r + 1]))
        nz = np.nonzero(cnt)[0]
        order = nz[np.lexsort((nz, -cnt[nz]))][:num_top]   # count descending, ties by ascending label
        labs.append(order)
        cnts.append(cnt[order])
        out_off.append(out_off[-1] + len(order))
    z = np.zeros(0, np.int64)
    return (np.array(out_off, dtype=np.uint64), np.concatenate(labs + [z]).astype(np.uint32),
            np.concatenate(cnts + [z]).astype(np.uint64))


def _reads(read_list):
    roff = np.concatenate([[0], np.cumsum([len(r) for r in read_list])]).astype(np.uint64)
    rows = np.concatenate([np.asarray(r, dtype=np.uint64) for r in read_list] + [np.zeros(0, np.uint64)])
    return rows, roff


def _check_labels(dev, dense, read_list, ratio, what):
    rows, roff = _reads(read_list)
    want_off, want = _ref_labels(dense, rows, roff, ratio)
    got_off, got = dev.get_labels_batch(rows, roff, ratio)
    np.testing.assert_array_equal(got_off, want_off, err_msg=f"{what}: ratio {ratio} offsets")
    np.testing.assert_array_equal(got, want, err_msg=f"{what}: ratio {ratio} labels")
    return want_off, want


def _check_top(dev, dense, read_list, num_top, what):
    rows, roff = _reads(read_list)
    want = _ref_top(dense, rows, roff, min(num_top, dense.shape[1] + 1))
    got = dev.get_top_labels_batch(rows, roff, num_top)
    for g, w, part in zip(got, want, ("offsets", "labels", "counts")):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: num_top {num_top} {part}")
    return want


def _layers(k):
    """{k, k/2, k/4, ...}: label c is carried by every row > c -- strictly layered counts."""
    out = []
    while k > 0:
        out.append(k)
        k //= 2
    return out


_NZ = (0, 1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2652)


def _classify_devices(O, which):
    from genome_graph_annotation_amd import BinRelWTDevice, BRWTDevice
    if which == "wt":   # the BinRel-WT engine on the m = 700 staircase
        dense = E.staircase(700)
        return BinRelWTDevice.from_dense(dense), dense
    case = _staircase_case(O, 2652, 0, False, "basic", 8, 0)
    dev = BRWTDevice.from_tree(case.ex, layout=None if which == "default" else which)
    if which == "nodes":
        assert dev.layout() == "nodes"
    return dev, case.dense


@pytest.mark.parametrize("which", ["default", "nodes", "wt"])
def test_classify_staircase(oracle_mod, which):
    """One-row reads (k distinct labels of count 1: ties in ascending label
    order), layered reads, every nz around the sort paths of k_read_top_labels
    (the compact u32 sort up to 1,024 distinct labels, Q padded from 4 up,
    the j >= 256 LDS steps from Q = 512, the whole-histogram u64 sort beyond)
    with num_top around each nz, all reads in one batch."""
    dev, dense = _classify_devices(oracle_mod, which)
    m = dense.shape[1]
    nzs = [k for k in _NZ if k <= m] + ([m] if m not in _NZ else [])
    # one-row reads of every row: row k has exactly k labels, all of count 1
    every = [[k] for k in range(m + 1)]
    off, labs = _check_labels(dev, dense, every, 0.0, "one-row reads")
    np.testing.assert_array_equal(np.diff(off.astype(np.int64)), np.arange(m + 1))
    off, labs, cnts = _check_top(dev, dense, every, 2**64 - 1, "one-row reads")
    assert (cnts == 1).all()
    for k in (1, 5, 256, 1025, m):
        if k <= m:
            np.testing.assert_array_equal(labs[int(off[k]):int(off[k + 1])], np.arange(k))
    # layered reads: strictly layered counts
    layered = [_layers(k) for k in nzs]
    off, labs, cnts = _check_top(dev, dense, layered, 2**64 - 1, "layered reads")
    for i, k in enumerate(nzs):
        c = cnts[int(off[i]):int(off[i + 1])].astype(np.int64)
        assert len(c) == k and (np.diff(c) <= 0).all() and (k == 0 or c[0] == len(_layers(k)))
    for ratio in (0.0, 0.5, 1.0):
        _check_labels(dev, dense, layered, ratio, "layered reads")
    # neighbouring reads on different sort paths, num_top around every nz
    mixed = []
    for i, k in enumerate(nzs):
        mixed.append([k] if i % 2 else _layers(k))
    tops = sorted({0, 1, 2**64 - 1} | {t for k in nzs for t in (k - 1, k, k + 1) if t >= 0})
    for num_top in tops:
        _check_top(dev, dense, mixed, num_top, "mixed reads")


@pytest.mark.parametrize("which", ["default", "nodes", "wt"])
def test_classify_count_limit_and_threshold(oracle_mod, which):
    """The u32 sort key holds counts < 2^18 (a read of fewer than 2^18 rows):
    reads of 2^18 - 1 and of 2^18 rows, exact on both sides.  get_labels at
    ratios whose product with the read's length rounds up in double
    (25 * 0.28 == 7.000000000000001: the threshold is 8, not 7), ratio 1.0
    on duplicated rows, an empty read between two non-empty ones."""
    dev, dense = _classify_devices(oracle_mod, which)
    N = 2**18
    big = [[3] * (N - 2) + [5], [7], [3] * (N - 1) + [5], [], [3] * (N - 1), [3] * N, [9, 9]]
    assert [len(r) for r in big[:6]] == [N - 1, 1, N, 0, N - 1, N]
    for num_top in (2, 3, 4, 2**64 - 1):
        off, labs, cnts = _check_top(dev, dense, big, num_top, "2^18 rows")
    assert cnts[0] == N - 1 and cnts[int(off[2])] == N and cnts[int(off[2]) + 3] == 1
    assert cnts[int(off[4])] == N - 1 and cnts[int(off[5])] == N
    _check_labels(dev, dense, big, 1.0, "2^18 rows")
    _check_labels(dev, dense, big, 0.999999, "2^18 rows")
    # double rounding of len * ratio
    assert 25 * 0.28 > 7 and math.ceil(25 * 0.28) == 8 and 50 * 0.14 > 7 and math.ceil(50 * 0.14) == 8
    seven_eight = [200] * 7 + [100] + [0] * 17          # labels < 100: count 8; 100..199: count 7
    r25 = seven_eight
    r50 = [206, 205, 204, 203, 202, 201, 200, 100] + [0] * 42   # the same counts from distinct rows
    reads = [r25, [], r50, [5, 5, 9, 9, 9], [0], r25[::-1]]
    for ratio, n in ((0.28, 25), (0.14, 50)):
        off, labs = _check_labels(dev, dense, reads, ratio, "rounded threshold")
        i = (0, 2)[n == 50]
        assert len(reads[i]) == n
        np.testing.assert_array_equal(labs[int(off[i]):int(off[i + 1])], np.arange(100))   # count 8 only
    for ratio in (1.0, 0.0, 7 / 25, 8 / 25):
        _check_labels(dev, dense, reads, ratio, "rounded threshold")
    off, labs = _check_labels(dev, dense, reads, 1.0, "ratio 1.0")
    np.testing.assert_array_equal(labs[int(off[3]):int(off[4])], np.arange(5))   # [5, 5, 9, 9, 9]
    assert off[1] == off[2]


def _prefix_matrix(m):
    """64 rows over m columns: full prefixes of 255 / 256 / 257 and more
    columns, a full row, sparse rows, the last column in use."""
    rng = np.random.default_rng(m)
    dense = rng.random((64, m)) < 4.0 / m
    for i, k in enumerate((255, 256, 257, 1024, 1025, 2000, m - 1, m)):
        dense[8 + i] = np.arange(m) < k
    dense[0] = False
    dense[1, m - 1] = True
    dense[2, m - 1] = True
    return dense


@pytest.mark.parametrize("layout", [None, "nodes"])
def test_classify_column_limits(oracle_mod, layout):
    """get_labels at 15,360 columns (the LDS histogram's limit; 15,361 is
    MBRWT_ERR_UNSUPPORTED) and get_top_labels at 8,192 (the whole-histogram
    sort at the largest P, on reads of > 1,024 distinct labels)."""
    O = oracle_mod
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    dense = _prefix_matrix(15360)
    dev = BRWTDevice.from_tree(O.OracleTree.from_dense(dense, "basic", 8).export(), layout=layout)
    reads = [[8], [9], [10], [1, 2], [], list(range(64)), [15, 15, 14], [8, 9, 10, 11, 12, 13, 14, 15], [1]]
    for ratio in (0.0, 0.5, 1.0):
        off, labs = _check_labels(dev, dense, reads, ratio, "15,360 columns")
    assert labs[-1] == 15359   # the last column, from the last read
    wide = np.zeros((64, 15361), dtype=bool)
    wide[:, :15360] = dense
    wide[3, 15360] = True
    over = BRWTDevice.from_tree(O.OracleTree.from_dense(wide, "basic", 8).export(), layout=layout)
    with pytest.raises(MBRWTError) as ei:
        over.get_labels_batch(np.arange(4, dtype=np.uint64), np.array([0, 4], dtype=np.uint64), 0.5)
    assert ei.value.status == L.MBRWT_ERR_UNSUPPORTED
    dense = _prefix_matrix(8192)
    dev = BRWTDevice.from_tree(O.OracleTree.from_dense(dense, "basic", 8).export(), layout=layout)
    reads = [[12], [1], [13, 12, 8], list(range(64)), [], [15, 15, 14, 2], [11], [12, 13], [14], [15]]
    for num_top in (2**64 - 1, 0, 1, 1024, 1025, 8191, 8192, 8193):
        off, labs, cnts = _check_top(dev, dense, reads, num_top, "8,192 columns")
    assert int(off[4] - off[3]) == 8192 and int(off[10] - off[9]) == 8192


# ---- a later range of a ranged build breaks the terminal records' limit --------

def test_ranged_terminal_limit(oracle_mod, build_env):
    """MBRWT_BUILD_ROWS_RANGE = 360,360 on 360,424 rows: the first range is
    sparse (terminal records are chosen); row 360,365, in the second range, is
    full over 2,100 columns -- 263 leaf parents, beyond the 256 nodes the
    terminal records' transcoding holds.  AUTO falls back to the node images
    and stays exact; layout 'rows' is refused and leaks nothing; byte masks
    build the same matrix as row records."""
    O = oracle_mod
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    R, m = 360360, 2100
    n, full = R + 64, R + 5
    W = (n + 63) // 64
    rng = np.random.default_rng(19)
    words = np.zeros((m, W), dtype=np.uint64)
    r = rng.integers(0, n, 3 * n)
    c = rng.integers(0, m, 3 * n)
    np.bitwise_or.at(words, (c, r // 64), np.uint64(1) << (r % 64).astype(np.uint64))
    words[:, full // 64] |= np.uint64(1) << np.uint64(full % 64)
    t = O.OracleTree.from_words(words.reshape(-1), n, m, "basic", 8)
    ex = t.export()
    nc = np.asarray(ex["num_children"])
    fc = np.asarray(ex["first_child"])
    leaf_parents = sum(1 for u in np.nonzero(nc)[0] if (nc[fc[u]:fc[u] + nc[u]] == 0).all())
    assert leaf_parents == 263 > 256
    rows = np.concatenate([np.arange(full - 8, full + 9), [0, R - 1, R, n - 1], [full] * 3,
                           rng.integers(0, n, 10000)]).astype(np.uint64)
    off_o, cols_o = t.get_rows(rows)
    assert int(off_o[9] - off_o[8]) == m

    def exact(dev):
        off_d, cols_d = dev.get_rows(rows)
        np.testing.assert_array_equal(off_d, off_o)
        np.testing.assert_array_equal(cols_d, cols_o)

    build_env("MBRWT_ROWS_RANGE", R)
    build_env("MBRWT_ROWS_VAR", 0)
    build_env("MBRWT_ROWS_CODE", 2)
    # the first range alone takes terminal records: the failure below is the later range's
    hw = np.ascontiguousarray(words[:, : (R + 63) // 64])
    hw[:, -1] &= np.uint64((1 << (R % 64)) - 1)
    first = O.OracleTree.from_words(hw.reshape(-1), R, m, "basic", 8)
    head = BRWTDevice.from_tree(first.export(), layout="rows")
    assert head.rows_stats()["terminal_records"], head.rows_stats()
    del head
    auto = BRWTDevice.from_tree(ex)
    assert auto.layout() == "nodes"
    exact(auto)
    with pytest.raises(MBRWTError) as ei:
        BRWTDevice.from_tree(ex, layout="rows")
    assert ei.value.status == L.MBRWT_ERR_UNSUPPORTED
    build_env("MBRWT_ROWS_CODE", 3)
    for layout in ("rows", None):   # a following build on the same thread succeeds
        rec = BRWTDevice.from_tree(ex, layout=layout)
        assert rec.layout() == "rows" and not rec.rows_stats()["terminal_records"]
        exact(rec)
