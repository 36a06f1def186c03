"""get_rows with 16-bit labels (mbrwt_get_rows16 / _device / _device_async)
against the oracle's CSR cast to u16, bit-exact, on the staircase fixture of
tests/edge_shapes.py and the built forms of test_gpu_edge_shapes._CONFIGS.

Every u16 output lies inside a larger buffer of 0xFFFF canaries (no label of
a matrix of at most 2,652 columns), GUARD elements in front of it -- an odd
number, so the caller's buffer is aligned to 2 bytes and no more -- and 64
after it: nothing outside [0, min(total, cap)) may change.  Each batch also
goes through the u32 device call; the two outputs must be equal after
widening.

Which kernel path a config drives:
  byte-masks, terminal-default, nibble-codes  k_compact_tiles<false, u16>, one record code each
  wide-nodes       k_compact_tiles<true, u16>
  tree-odometer    greedy + relax: labels not ascending within a row
  C1024            tile totals beyond C = 1024 become direct tiles (walked into the u16 CSR)
  m2652-bs-128,3   records longer than a block: the long-record walk over places the copy filled
  classes          the class-mapped direct pass
  var-8, var-8-G1, var-2   k_var_decode<G, WPB, u16> with G = 4, 1, 2
  nodes, shards    no row records: the u32 query into a workspace, then the narrowing kernel

k_var_decode's two store paths (csrc/rows_var.hip var_geometry_of: the stage
holds CS labels per wave; a tile of R = 64 / G rows goes through LDS -- peeled
head, aligned groups of 8, tail -- while total + sh <= CS, sh < 8 the
destination's phase, and straight to global memory beyond):
  var-8     mean 350 labels a row -> G = 4, R = 16, CS = 6,592: the sweep's tiles of
            rows k .. k + 15 total 16 k + 120, so rows up to ~400 take LDS and the
            denser ones the global path; tile_totals / geometry / copies: LDS
  var-8-G1  G = 1, R = 64, CS = 16,384 (the cap): sweep tiles 64 k + 2,016, LDS up to
            k ~ 224, global beyond (tiles of 64 rows of about 650 labels: 41,600)
  var-2     m = 64, mean 32 -> G = 2, R = 32, CS = 1,472: rows 0 .. 31 total 496 (LDS),
            rows 32 .. 63 total 1,520 (global); geometry tiles of light rows: LDS
"""
import ctypes as C

import numpy as np
import pytest

import edge_shapes as E
from conftest import gpu_available
from test_gpu_edge_shapes import _CONFIGS, _Case, _staircase_case

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

GUARD = 65   # canaries in front of the output: odd, so the output starts at an odd element
TAIL = 64    # canaries after it


def _odd_tile_offset(off_e, n):
    """A 64-row tile of the batch (k_var_decode: a multiple of its tiles) starts at an odd label offset."""
    return bool((np.asarray(off_e[64:n:64], dtype=np.uint64) & np.uint64(1)).any())


def _check_batch16(dev, case, rows, name, canary=0xFFFF):
    """`rows` through mbrwt_get_rows16, _device and _device_async, each at
    cap = total and cap = total - 1 (MBRWT_ERR_CAPACITY with the total, and
    nothing written at or past cap), between canaries; the expected labels
    are the oracle's cast to u16; then the u32 device call on the same rows.
    Returns whether a tile of the batch started at an odd label offset."""
    import torch
    from genome_graph_annotation_amd import MBRWTError, _lib as L
    lib = L.lib()
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    n = len(rows)
    off_e, cols_e = E.gather_csr(case.off, case.cols, rows)
    assert int(cols_e.max(initial=0)) < 65536
    cols16 = cols_e.astype(np.uint16)
    assert not (cols16 == canary).any(), "the canary must not be a label of the batch"
    tot = len(cols16)
    caps = (tot, tot - 1) if tot else (0,)
    ci16 = int(np.array([canary], dtype=np.uint16).view(np.int16)[0])

    def intact(buf, cap, what):
        """Canaries in front, and from min(tot, cap) on: nothing written outside [0, min(tot, cap))."""
        lo = GUARD + min(tot, cap)
        assert (buf[:GUARD] == canary).all(), f"{name}: {what} wrote in front of the buffer (cap {cap})"
        assert (buf[lo:] == canary).all(), f"{name}: {what} wrote at or past min(total, cap) (cap {cap})"

    # -- host buffers ---------------------------------------------------------
    off_h, cols_h = dev.get_rows16(rows)
    assert cols_h.dtype == np.uint16 and off_h.dtype == np.uint64
    np.testing.assert_array_equal(off_h, off_e, err_msg=f"{name}: get_rows16 offsets")
    np.testing.assert_array_equal(cols_h, cols16, err_msg=f"{name}: get_rows16 labels")
    for cap in caps:
        big = np.full(GUARD + tot + TAIL, canary, dtype=np.uint16)
        offs = np.zeros(n + 1, dtype=np.uint64)
        need = C.c_uint64(0)
        st = lib.mbrwt_get_rows16(dev._h, rows.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                  offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                  C.cast(big.ctypes.data + 2 * GUARD, C.POINTER(C.c_uint16)), cap, C.byref(need))
        assert need.value == tot, (name, cap, need.value, tot)
        assert st == (L.MBRWT_OK if cap >= tot else L.MBRWT_ERR_CAPACITY), (name, cap, st)
        if cap >= tot:
            np.testing.assert_array_equal(offs, off_e, err_msg=f"{name}: host offsets")
            np.testing.assert_array_equal(big[GUARD:GUARD + tot], cols16, err_msg=f"{name}: host labels")
        intact(big, cap, "mbrwt_get_rows16")

    # -- device buffers -------------------------------------------------------
    s = torch.cuda.current_stream().cuda_stream
    rt = torch.from_numpy(rows.view(np.int64)).cuda()
    ot = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    big = torch.full((GUARD + tot + TAIL,), ci16, dtype=torch.int16, device="cuda")
    assert big[GUARD:].data_ptr() % 4 == 2   # aligned to 2 bytes, not to 4

    def host(t):
        return t.cpu().numpy().view(np.uint16)

    for cap in caps:
        big.fill_(ci16)
        ot.fill_(-1)
        ct = big[GUARD:GUARD + max(cap, 1 if tot == 0 else 0)]
        if cap >= tot:
            got = dev.get_rows16_device(rt, ot, ct, s)
            torch.cuda.synchronize()
            assert got == tot, name
            np.testing.assert_array_equal(ot.cpu().numpy().view(np.uint64), off_e, err_msg=f"{name}: device offsets")
            np.testing.assert_array_equal(host(big)[GUARD:GUARD + tot], cols16, err_msg=f"{name}: device labels")
        else:
            with pytest.raises(MBRWTError) as ei:
                dev.get_rows16_device(rt, ot, ct, s)
            torch.cuda.synchronize()
            assert ei.value.status == L.MBRWT_ERR_CAPACITY and ei.value.needed == tot, (name, cap)
        intact(host(big), cap, "mbrwt_get_rows16_device")
    st = torch.zeros(3, dtype=torch.int64, device="cuda")
    for cap in caps:
        st.zero_()
        big.fill_(ci16)
        ot.fill_(-1)
        dev.get_rows16_device_async(rt, ot, big[GUARD:GUARD + cap], st, s)
        torch.cuda.synchronize()
        need, status, sticky = st.cpu().tolist()
        assert need == tot, (name, cap, need, tot)
        if cap >= tot:
            assert status == L.MBRWT_OK and sticky == 1 << L.MBRWT_OK, (name, cap, status, sticky)
            np.testing.assert_array_equal(ot.cpu().numpy().view(np.uint64), off_e, err_msg=f"{name}: async offsets")
            np.testing.assert_array_equal(host(big)[GUARD:GUARD + tot], cols16, err_msg=f"{name}: async labels")
        else:
            assert status == L.MBRWT_ERR_CAPACITY and sticky == 1 << L.MBRWT_ERR_CAPACITY, (name, cap, status)
        intact(host(big), cap, "mbrwt_get_rows16_device_async")
    # -- the u32 call on the same rows: equal after widening ---------------------
    c32 = torch.full((tot + 1,), -1, dtype=torch.int32, device="cuda")
    o32 = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    assert dev.get_rows_device(rt, o32, c32[:max(tot, 1)], s) == tot
    big.fill_(ci16)
    assert dev.get_rows16_device(rt, ot, big[GUARD:GUARD + max(tot, 1)], s) == tot
    torch.cuda.synchronize()
    assert torch.equal(o32, ot), f"{name}: u32 and u16 offsets differ"
    np.testing.assert_array_equal(host(big)[GUARD:GUARD + tot].astype(np.uint32),
                                  c32[:tot].cpu().numpy().view(np.uint32), err_msg=f"{name}: u16 labels != u32 labels")
    return _odd_tile_offset(off_e, n)


def _all_batches16(dev, case, m):
    """The fixture's batches of test_gpu_edge_shapes._all_batches; whether any had an odd tile offset."""
    odd = _check_batch16(dev, case, E.sweep_rows(m), "sweep")
    for lo, hi in E.TILE_TOTAL_WINDOWS:
        odd |= _check_batch16(dev, case, E.tile_totals(m, lo, hi), f"tile_totals {lo}..{hi}")
    for k in E.geometry_heavy(m):
        for name, rows in E.geometry(m, k):
            odd |= _check_batch16(dev, case, rows, f"geometry k={k} {name}")
    for name, rows in E.copies(m):
        odd |= _check_batch16(dev, case, rows, f"copies {name}")
    if case.n > m + 1:  # the pad rows: the matrix's last rows, a partial tile
        odd |= _check_batch16(dev, case, np.arange(case.n - 200, case.n, dtype=np.uint64), "pad rows")
    return odd


def _build(O, build_env, name, shard_rows=0):
    """(device, case) of _CONFIGS[name], built as test_staircase_rows builds it."""
    from genome_graph_annotation_amd import BRWTDevice, _lib as L
    from genome_graph_annotation_amd.brwt import build_option
    m, pad, repeat, (part, arity, relax), layout, opts, expect = _CONFIGS[name]
    case = _staircase_case(O, m, pad, repeat, part, arity, relax)
    opts = dict(opts)
    classes = opts.pop("classes", None)
    for k, v in opts.items():
        build_env(k, v)
    if shard_rows:
        build_env("MBRWT_SHARD_ROWS", shard_rows)
    if classes is not None:
        with build_option(L.MBRWT_BUILD_ROWS_CLASSES, classes):
            dev = BRWTDevice.from_tree(case.ex, layout=layout)
    else:
        dev = BRWTDevice.from_tree(case.ex, layout=layout)
    return dev, case, expect


_ROWS16 = ("byte-masks", "terminal-default", "nibble-codes", "wide-nodes", "tree-odometer", "C1024",
           "m2652-bs-128,3", "classes", "var-8", "var-8-G1", "var-2", "nodes")


@pytest.mark.parametrize("name", _ROWS16)
def test_staircase_rows16(oracle_mod, build_env, name):
    """Every batch of the fixture through the three u16 calls on one built
    form per case (the module's docstring: which kernel path each drives)."""
    dev, case, expect = _build(oracle_mod, build_env, name)
    st = dev.rows_stats()
    print(name, dev.layout(), dev.traverse_kernel(), st)
    if expect == "nodes":
        assert dev.layout() == "nodes" and st is None
    else:
        kernel = "k_var_decode" if expect == "variable" else "k_traverse_rows"
        assert dev.layout() == "rows" and dev.traverse_kernel() == kernel, (dev.layout(), dev.traverse_kernel())
        assert bool(st["variable"]) == (expect == "variable"), st
        if expect == "wide":
            assert int(np.asarray(case.ex["num_children"]).max()) > 16
        if expect == "classes":
            assert st["classes"] == case.m + 1, st
        if name.startswith("m2652"):
            assert st["long_rows"] > 0, st
    assert _all_batches16(dev, case, case.m), "no batch with an odd tile offset was run"
    if expect == "classes":  # the repeated rows
        _check_batch16(dev, case, np.arange(case.n, dtype=np.uint64)[::-1], "every row, reversed")


def test_staircase_rows16_shards(oracle_mod, build_env):
    """Three row shards of per-node images (the hook of tests/test_gpu_shards.py):
    the sharded u32 query into the workspace, then the narrowing kernel."""
    dev, case, _ = _build(oracle_mod, build_env, "nodes", shard_rows=234)
    assert dev.num_shards() == 3 and dev.layout() == "nodes", (dev.num_shards(), dev.layout())
    assert _all_batches16(dev, case, case.m), "no batch with an odd tile offset was run"


def test_forced_kernel_variant16(oracle_mod, build_env):
    """A row-record context (layout both) with MBRWT_OPT_KERNEL = 1 answers
    through the node kernel and the narrowing kernel."""
    from genome_graph_annotation_amd import BRWTDevice, _lib as L
    m, pad, repeat, (part, arity, relax), _, opts, _ = _CONFIGS["byte-masks"]
    case = _staircase_case(oracle_mod, m, pad, repeat, part, arity, relax)
    for k, v in opts.items():
        build_env(k, v)
    dev = BRWTDevice.from_tree(case.ex, layout="both")
    assert dev.layout() == "both"
    dev.set_option(L.MBRWT_OPT_KERNEL, 1)
    _check_batch16(dev, case, E.sweep_rows(m), "sweep, kernel variant 1")
    dev.set_option(L.MBRWT_OPT_KERNEL, 0)
    _check_batch16(dev, case, E.sweep_rows(m), "sweep, row records again")


# ---- label limits ---------------------------------------------------------------

def test_labels_up_to_65535(oracle_mod):
    """65,536 columns (allowed: row records, as test_gpu_rows.test_many_columns_rows
    shows): rows holding columns 32,767 and 32,768 (the int16 sign bit) and
    65,535 (the top value, a label and no sentinel)."""
    from genome_graph_annotation_amd import BRWTDevice
    n, m = 300, 65536
    rng = np.random.default_rng(16)
    dense = rng.random((n, m)) < 3.0 / m
    for i, c in enumerate((32767, 32768, 65535)):
        dense[i::7, c] = True
    dense[5::11, 32767:32769] = True
    dense[5::11, 65535] = True
    case = _Case(oracle_mod, dense, "basic", 16, 0)
    dev = BRWTDevice.from_tree(case.ex)
    assert dev.layout() == "rows" and dev.traverse_kernel() == "k_traverse_rows"
    assert dev.num_columns() == 65536
    rows = np.concatenate([np.arange(n), rng.integers(0, n, 700)]).astype(np.uint64)
    _, cols_e = E.gather_csr(case.off, case.cols, rows)
    for c in (32767, 32768, 65535):
        assert (cols_e == c).sum() > 20
    canary = 0x5A5A   # 0xFFFF is a label here
    assert not (case.cols == canary).any()
    _check_batch16(dev, case, rows, "65536 columns", canary=canary)
    off_h, cols_h = dev.get_rows16(rows)
    assert cols_h.dtype == np.uint16 and int(cols_h.max()) == 65535


def test_more_than_65536_columns_unsupported(oracle_mod):
    """65,537 columns (the node layout): the three calls answer
    MBRWT_ERR_UNSUPPORTED with the reason, before any launch -- offsets,
    labels and the status block stay as they were; the u32 call answers."""
    import torch
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    lib = L.lib()
    n, m = 200, 65537
    rng = np.random.default_rng(17)
    dense = rng.random((n, m)) < 3.0 / m
    dense[::3, m - 1] = True
    t = oracle_mod.OracleTree.from_dense(dense, "basic", 16, 0)
    dev = BRWTDevice.from_tree(t.export())
    assert dev.layout() == "nodes" and dev.num_columns() == m
    rows = np.arange(n, dtype=np.uint64)
    off_o, cols_o = t.get_rows(rows)
    off_d, cols_d = dev.get_rows(rows)
    np.testing.assert_array_equal(off_d, off_o)
    np.testing.assert_array_equal(cols_d, cols_o)

    def message():
        return (lib.mbrwt_last_error_message() or b"").decode()

    with pytest.raises(MBRWTError) as ei:
        dev.get_rows16(rows)
    assert ei.value.status == L.MBRWT_ERR_UNSUPPORTED
    assert "65536 columns" in message() and str(m) in message(), message()
    cap = len(cols_o) + 64
    big = np.full(cap, 0xFFFF, dtype=np.uint16)
    offs = np.full(n + 1, 77, dtype=np.uint64)
    need = C.c_uint64(123)
    st = lib.mbrwt_get_rows16(dev._h, rows.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                              offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                              big.ctypes.data_as(C.POINTER(C.c_uint16)), cap, C.byref(need))
    assert st == L.MBRWT_ERR_UNSUPPORTED and need.value == 123
    assert (big == 0xFFFF).all() and (offs == 77).all()
    s = torch.cuda.current_stream().cuda_stream
    rt = torch.from_numpy(rows.view(np.int64)).cuda()
    ot = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    ct = torch.full((cap,), -1, dtype=torch.int16, device="cuda")
    status = torch.full((3,), 9, dtype=torch.int64, device="cuda")
    with pytest.raises(MBRWTError) as ei:
        dev.get_rows16_device(rt, ot, ct, s)
    assert ei.value.status == L.MBRWT_ERR_UNSUPPORTED and "65536 columns" in message()
    with pytest.raises(MBRWTError) as ei:
        dev.get_rows16_device_async(rt, ot, ct, status, s)
    assert ei.value.status == L.MBRWT_ERR_UNSUPPORTED and "65536 columns" in message()
    torch.cuda.synchronize()
    assert (ct == -1).all() and (ot == -1).all() and (status == 9).all()


# ---- the protocol's corners -------------------------------------------------------

@pytest.mark.parametrize("name", ["byte-masks", "var-8", "nodes"])
def test_empty_batch_and_null_cols16(oracle_mod, build_env, name):
    """n = 0: offsets[0] = 0, no label, MBRWT_OK.  A NULL d_cols counts only:
    `need` is the batch's total (MBRWT_ERR_CAPACITY when it is not 0), whatever
    cols_cap says, and nothing is written."""
    import torch
    from genome_graph_annotation_amd import MBRWTError, _lib as L
    lib = L.lib()
    dev, case, _ = _build(oracle_mod, build_env, name)
    s = torch.cuda.current_stream().cuda_stream
    # the empty batch
    off_h, cols_h = dev.get_rows16(np.zeros(0, dtype=np.uint64))
    assert off_h.tolist() == [0] and len(cols_h) == 0 and cols_h.dtype == np.uint16
    rt0 = torch.zeros(0, dtype=torch.int64, device="cuda")
    ot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ct = torch.full((8,), -1, dtype=torch.int16, device="cuda")
    assert dev.get_rows16_device(rt0, ot, ct, s) == 0
    torch.cuda.synchronize()
    assert ot.tolist() == [0] and (ct == -1).all()
    st = torch.zeros(3, dtype=torch.int64, device="cuda")
    ot.fill_(-1)
    dev.get_rows16_device_async(rt0, ot, ct, st, s)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, L.MBRWT_OK, 1 << L.MBRWT_OK] and ot.tolist() == [0] and (ct == -1).all()
    # NULL d_cols: rows 0 (no label: MBRWT_OK) and 0 .. 99 (4,950 labels)
    for rows, tot in ((np.zeros(3, dtype=np.uint64), 0), (np.arange(100, dtype=np.uint64), 4950)):
        off_e, cols_e = E.gather_csr(case.off, case.cols, rows)
        assert len(cols_e) == tot
        rt = torch.from_numpy(rows.view(np.int64)).cuda()
        ot = torch.full((len(rows) + 1,), -1, dtype=torch.int64, device="cuda")
        need = C.c_uint64(2**64 - 1)
        rc = lib.mbrwt_get_rows16_device(dev._h, rt.data_ptr(), len(rows), ot.data_ptr(), None, 1 << 20,
                                         C.byref(need), s)
        torch.cuda.synchronize()
        assert (rc, need.value) == (L.MBRWT_ERR_CAPACITY if tot else L.MBRWT_OK, tot), (name, rc, need.value)
        if tot:
            with pytest.raises(MBRWTError) as ei:
                dev.get_rows16_device(rt, ot, None, s)
            assert ei.value.status == L.MBRWT_ERR_CAPACITY and ei.value.needed == tot
        st.zero_()
        dev.get_rows16_device_async(rt, ot, None, st, s)
        torch.cuda.synchronize()
        want = L.MBRWT_ERR_CAPACITY if tot else L.MBRWT_OK
        assert st.cpu().tolist() == [tot, want, 1 << want], (name, st.cpu().tolist())
        need = C.c_uint64(2**64 - 1)
        offs = np.zeros(len(rows) + 1, dtype=np.uint64)
        rc = lib.mbrwt_get_rows16(dev._h, rows.ctypes.data_as(C.POINTER(C.c_uint64)), len(rows),
                                  offs.ctypes.data_as(C.POINTER(C.c_uint64)), None, 1 << 20, C.byref(need))
        assert (rc, need.value) == (want, tot), (name, rc, need.value)


def test_rows_out_of_range16(oracle_mod, build_env):
    """A row == num_rows: MBRWT_ERR_RANGE from the three calls, as the u32 ones."""
    import torch
    from genome_graph_annotation_amd import MBRWTError, _lib as L
    for name in ("byte-masks", "nodes"):
        dev, case, _ = _build(oracle_mod, build_env, name)
        rows = np.array([3, case.n, 5], dtype=np.uint64)
        with pytest.raises(MBRWTError) as ei:
            dev.get_rows16(rows)
        assert ei.value.status == L.MBRWT_ERR_RANGE
        s = torch.cuda.current_stream().cuda_stream
        rt = torch.from_numpy(rows.view(np.int64)).cuda()
        ot = torch.zeros(4, dtype=torch.int64, device="cuda")
        ct = torch.zeros(64, dtype=torch.int16, device="cuda")
        with pytest.raises(MBRWTError) as ei:
            dev.get_rows16_device(rt, ot, ct, s)
        assert ei.value.status == L.MBRWT_ERR_RANGE
        st = torch.zeros(3, dtype=torch.int64, device="cuda")
        dev.get_rows16_device_async(rt, ot, ct, st, s)
        torch.cuda.synchronize()
        assert st.cpu().tolist()[1:] == [L.MBRWT_ERR_RANGE, 1 << L.MBRWT_ERR_RANGE]
        off, cols = dev.get_rows16(np.array([3], dtype=np.uint64))   # (and the context still answers)
        assert cols.tolist() == [0, 1, 2]


def test_cols_dtype_is_checked(oracle_mod, build_env):
    """The device methods take an int16 tensor (viewed as uint16 on the host) and nothing else."""
    import torch
    dev, case, _ = _build(oracle_mod, build_env, "byte-masks")
    rt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ot = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = torch.zeros(3, dtype=torch.int64, device="cuda")
    for dtype in (torch.int32, torch.uint8, torch.float16):
        bad = torch.zeros(16, dtype=dtype, device="cuda")
        with pytest.raises(TypeError):
            dev.get_rows16_device(rt, ot, bad, None)
        with pytest.raises(TypeError):
            dev.get_rows16_device_async(rt, ot, bad, st, None)
