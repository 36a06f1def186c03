"""GPU parity of get_column on the per-node images (csrc/column.hip) and on
row shards (sharded_get_column, csrc/shards.hip), and of get_columns where it
runs on them (columns_get_columns, csrc/rows_columns.hip), at the edges of
their kernels, on the deterministic fixtures of tests/column_shapes.py (which
tests/test_column_shapes.py checks on the CPU).  The layout is pinned to
'nodes' and MBRWT_BUILD_NODE_KINDS to the kinds a case is named for; every
context asserts through mbrwt_node_info the kind, stride and length of the
node get_column extracts from.  Every comparison is exact, on integers: the
expected column is np.flatnonzero(dense[:, c]), cross-checked against the CPU
oracle's get_column.

Extraction (k_col_count, k_col_write, column_word; one thread per 32
positions, 8192 per workgroup), at L = 1, 31, 32, 33, 8191, 8192, 8193 and
(kinds off) 16385 positions -- the tail mask `rem < 32`, one workgroup against
two and three, block_offsets across workgroups -- with columns that are empty,
full, hold position 0 or L - 1 alone, every position = 31 or = 0 mod 32, 8191
and 8192, positions from 8192 on only (the first workgroup counts zero),
workgroups 0 and 2 but not 1:
  * MASK8 / 16 / 32 / 64 leaf parents (bit 32 and bit 63 of a MASK64 mask on
    the highest child slot) and a leaf child of a PLANE node, kinds off
  * PACK: 16-position blocks of exactly 48 pairs (inline) around one of 49
    (spilled), first / last child and first / last leaf slot
  * PACK2 at S = 8 (sparse records) and S = 4 (dense), PACKT at S = 8, 7, 5, 3
    (a block straddles a 32-position word where 32 % S != 0), a spilled block
    between inline ones, L around the multiples of S; PACKT nodes of 16
    children (two mask bytes) under a folded root of 10
Lifts (k_col_lift): three PLANE levels and the super-root over nested row
sets cut by gap patterns -- runs of empty rank blocks at the start, in the
middle and at the end, ones at bits 0 and 31, a full block, the k-th one the
first of its block --, the deepest image of 1, 2, 3 and 257 blocks; a PLANE
of nine children lifted at child slot 8; the folded super-root at slot 8.
The capacity protocol of include/mbrwt.h on a MASK fixture, a PACKT fixture
and a sharded context; row shards of 64 rows with n mod 64 in {1, 63} and the
shortage of a short buffer in the first, a middle and the last shard.
"""
import ctypes as C

import numpy as np
import pytest

import column_shapes as S
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

_KIND_SWITCHES = (("MBRWT_FOLD_ROOT", 1), ("MBRWT_PACK", 2), ("MBRWT_PACK2", 4), ("MBRWT_PACKT", 8))


def _set_kinds(build_env, kinds):
    """MBRWT_BUILD_NODE_KINDS = kinds for the rest of the test."""
    from genome_graph_annotation_amd import _lib as L
    for name, bit in _KIND_SWITCHES:
        build_env(name, 1 if kinds & bit else 0)
    cur = C.c_int64(-1)
    L.check(L.lib().mbrwt_get_build_option(L.MBRWT_BUILD_NODE_KINDS, C.byref(cur)), "mbrwt_get_build_option")
    assert cur.value == kinds


def _build(O, dense, arity, layout="nodes"):
    from genome_graph_annotation_amd import BRWTDevice
    t = O.OracleTree.from_dense(dense, "basic", arity)
    dev = BRWTDevice.from_tree(t.export(), layout=layout)
    assert dev.layout() == layout and (dev.num_rows(), dev.num_columns()) == dense.shape
    return t, dev


def _check_columns(dev, t, dense, cols, what):
    for c in cols:
        want = np.flatnonzero(dense[:, c]).astype(np.uint64)
        np.testing.assert_array_equal(np.asarray(t.get_column(int(c)), dtype=np.uint64), want,
                                      err_msg=f"{what}: the oracle's column {c}")
        got = dev.get_column(int(c))
        assert got.dtype == np.uint64
        np.testing.assert_array_equal(got, want, err_msg=f"{what}: column {c}")


def _check_points(dev, dense, cols, what):
    """get_batch on every set position of the columns `cols` and on its row and column neighbours."""
    n, m = dense.shape
    qr, qc = [], []
    for c in cols:
        r = np.flatnonzero(dense[:, c])
        for dr, dc in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
            qr.append(np.clip(r + dr, 0, n - 1))
            qc.append(np.full(len(r), min(max(c + dc, 0), m - 1)))
    qr, qc = np.concatenate(qr), np.concatenate(qc)
    if len(qr):
        np.testing.assert_array_equal(dev.get_batch(qr.astype(np.uint64), qc.astype(np.uint64)), dense[qr, qc],
                                      err_msg=f"{what}: get_batch")


# ---- extraction --------------------------------------------------------------------------

def _cases():
    for name, cfg in S.CONFIGS.items():
        for L in cfg.lengths:
            yield name, L


@pytest.mark.parametrize("name,L", list(_cases()))
def test_extraction(oracle_mod, build_env, name, L):
    cfg = S.CONFIGS[name]
    tree = cfg.tree()
    _set_kinds(build_env, cfg.node_kinds)
    for part in range(cfg.parts(L)):
        f = cfg.build(L, part)
        what = f"{name} L={L} part {part}"
        t, dev = _build(oracle_mod, f.dense, cfg.arity)
        # -- what was built: the node the extraction reads, the root, the super-root
        info = dev.node_info(cfg.node + 1)
        print(what, f.dense.shape, info, dev.node_info(0), dev.node_info(1))
        assert info == {"kind": cfg.kind, "arity": int(tree.num_children[cfg.node]), "stride": cfg.stride(f),
                        "length": L}, (what, info)
        top, root = dev.node_info(0), dev.node_info(1)
        assert top["length"] == f.n
        if cfg.node_kinds & 1:      # the folded root: its children hang off the super-root
            assert root["kind"] == "FOLDED" and top["kind"] == "PLANE" and top["arity"] == int(tree.num_children[0])
            assert top["stride"] == (16 if top["arity"] <= 2 else 128)
        else:
            assert (top["kind"], top["arity"], top["stride"]) == ("PLANE", 1, 16)
            assert root["length"] == int(f.dense.any(axis=1).sum())
        if name == "plane-wide":
            assert (root["kind"], root["arity"], root["stride"]) == ("PLANE", 9, 128)
        if name == "packt-wide":
            assert top["arity"] == 10 and info["arity"] == 16
        # -- the columns: all of them (the first matrix of a wide fixture), else the node's patterned ones
        named = sorted(f.patterns)
        every = range(f.m) if part == 0 or f.m <= 145 else sorted(set(named) | {0, f.m - 1})
        _check_columns(dev, t, f.dense, every, what)
        _check_points(dev, f.dense, named, what)
        dev.close()


# ---- lifts -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("T", S.LIFT_DEEPEST)
def test_lifts(oracle_mod, build_env, T, mirror):
    """Columns 0 and 15 of the 16-column binary tree: the leaf's positions
    climb through C's parent B, A, the root and the super-root."""
    _set_kinds(build_env, S.KINDS_OFF)
    f = S.lift_fixture(T, mirror)
    tree = S.BasicTree(16, 2)
    t, dev = _build(oracle_mod, f.dense, 2)
    path = tree.path(f.column)
    infos = [dev.node_info(u + 1) for u, _ in path]
    print(T, mirror, f.dense.shape, dev.node_info(0), infos)
    assert dev.node_info(0) == {"kind": "PLANE", "arity": 1, "stride": 16, "length": f.n}
    want = [len(r) for r in f.sets[:4]]
    assert [i["length"] for i in infos] == want and want[2] == T
    assert [i["kind"] for i in infos] == ["PLANE", "PLANE", "PLANE", "MASK8"]
    assert all(i["stride"] == 16 and i["arity"] == 2 for i in infos[:3]) and infos[3]["arity"] == 2
    _check_columns(dev, t, f.dense, range(16), f"lift T={T} mirror={mirror}")
    _check_points(dev, f.dense, [c for c in range(16) if f.dense[:, c].any()], f"lift T={T}")
    dev.close()


# ---- the capacity protocol -------------------------------------------------------------------------

def _call(dev, col, buf, cap):
    import torch
    from genome_graph_annotation_amd import _lib as L
    need = C.c_uint64(2**64 - 1)
    st = L.lib().mbrwt_get_column_device(dev._h, col, buf.data_ptr() if buf is not None else None, cap,
                                         C.byref(need), None)
    torch.cuda.synchronize()
    return st, int(need.value), (L.lib().mbrwt_last_error_message() or b"").decode()


def _protocol(dev, t, dense, cols, empty_col, what):
    """The protocol of test_gpu_edge_shapes.test_get_column_capacity_protocol
    (include/mbrwt.h): a null buffer sizes the column; rows_cap one short is
    MBRWT_ERR_CAPACITY with the size, 'rows_cap too small' and the rows
    untouched; rows_cap = the size gives the ascending rows and writes
    nothing past them; a column no row holds is MBRWT_OK with 0; column ==
    num_columns is MBRWT_ERR_RANGE."""
    import torch
    from genome_graph_annotation_amd import _lib as L
    m = dense.shape[1]
    for col in cols:
        want = np.flatnonzero(dense[:, col]).astype(np.uint64)
        np.testing.assert_array_equal(np.asarray(t.get_column(col), dtype=np.uint64), want)
        k = len(want)
        assert k > 0
        st, need, msg = _call(dev, col, None, 0)
        assert (st, need) == (L.MBRWT_ERR_CAPACITY, k) and "rows_cap too small" in msg, (what, col, st, need, msg)
        buf = torch.full((k + 8,), -1, dtype=torch.int64, device="cuda")
        st, need, msg = _call(dev, col, buf, k - 1)
        assert (st, need) == (L.MBRWT_ERR_CAPACITY, k) and "rows_cap too small" in msg, (what, col, st, need, msg)
        assert "rows_cap too small" in L.MBRWTError(st).args[0]
        assert (buf == -1).all(), f"{what}: rows written under MBRWT_ERR_CAPACITY (column {col})"
        st, need, _ = _call(dev, col, buf, k)
        assert (st, need) == (L.MBRWT_OK, k), (what, col, st, need)
        np.testing.assert_array_equal(buf[:k].cpu().numpy().view(np.uint64), want, err_msg=f"{what}: column {col}")
        assert (buf[k:] == -1).all(), f"{what}: a row written past the column's size"
        np.testing.assert_array_equal(dev.get_column(col), want, err_msg=f"{what}: column {col} (host)")
    assert not dense[:, empty_col].any() and len(t.get_column(empty_col)) == 0
    assert _call(dev, empty_col, None, 0)[:2] == (L.MBRWT_OK, 0)
    buf = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    assert _call(dev, empty_col, buf, 8)[:2] == (L.MBRWT_OK, 0) and (buf == -1).all()
    assert len(dev.get_column(empty_col)) == 0
    assert dev.num_columns() == m
    st, _, msg = _call(dev, m, buf, 8)
    assert st == L.MBRWT_ERR_RANGE and "column out of range" in msg, (what, st, msg)
    assert _call(dev, m, None, 0)[0] == L.MBRWT_ERR_RANGE and (buf == -1).all()


def _sharded(O, dense, arity=4):
    from conftest import with_build
    from genome_graph_annotation_amd import BRWTDevice
    t = O.OracleTree.from_dense(dense, "basic", arity)
    dev = with_build("MBRWT_SHARD_ROWS", S.SHARD_ROWS, lambda: BRWTDevice.from_tree(t.export(), layout="nodes"))
    n = dense.shape[0]
    K = (n + S.SHARD_ROWS - 1) // S.SHARD_ROWS
    assert dev.layout() == "nodes" and dev.num_shards() == K
    # node_info reports the shard asked for: its super-root spans the shard's rows
    assert [dev.node_info(0, k)["length"] for k in range(K)] == [S.SHARD_ROWS] * (K - 1) + [n - (K - 1) * S.SHARD_ROWS]
    return t, dev


@pytest.mark.parametrize("which", ["mask", "packt", "shards"])
def test_capacity_protocol(oracle_mod, build_env, which):
    if which == "shards":
        dense = S.shard_matrix(319)
        t, dev = _sharded(oracle_mod, dense)
        cols, empty = [S.SHARD_COLUMNS[k] for k in ("boundary", "not_in_shard_0", "every_shard", "full")], 6
    else:
        name, L = ("mask16", 8193) if which == "mask" else ("packt-s7", 8193)
        cfg = S.CONFIGS[name]
        _set_kinds(build_env, cfg.node_kinds)
        f = cfg.build(L, 0)
        dense = f.dense
        t, dev = _build(oracle_mod, dense, cfg.arity)
        assert dev.node_info(cfg.node + 1)["kind"] == cfg.kind and dev.node_info(cfg.node + 1)["length"] == L
        pats = {p: c for c, p in f.patterns.items()}
        # (the PACKT fixture: column 3 is neither a pattern column nor an always-set one)
        cols, empty = [pats["full"], pats["pos0"], pats["mod31"], pats["last"]], pats["empty"] if which == "mask" else 3
    _protocol(dev, t, dense, cols, empty, which)
    dev.close()


# ---- row shards ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [257, 319])
def test_row_shards(oracle_mod, n):
    """Shards of 64 rows, the last one of 1 or 63.  A buffer too short by
    one row for the shards up to shard k -- so the shortage falls in shard k,
    the first, a middle or the last one -- is refused with the column's whole
    size and left as it was."""
    import torch
    from genome_graph_annotation_amd import _lib as L
    dense = S.shard_matrix(n)
    t, dev = _sharded(oracle_mod, dense)
    R, K = S.SHARD_ROWS, dev.num_shards()
    _check_columns(dev, t, dense, range(8), f"shards n={n}")
    _check_points(dev, dense, range(6), f"shards n={n}")
    tried = set()
    for col in range(8):
        want = np.flatnonzero(dense[:, col]).astype(np.uint64)
        per = np.bincount((want // R).astype(np.int64), minlength=K)
        for k in np.flatnonzero(per):
            cap = int(per[:k + 1].sum()) - 1
            buf = torch.full((len(want) + 4,), -1, dtype=torch.int64, device="cuda")
            st, need, msg = _call(dev, col, buf, cap)
            assert (st, need) == (L.MBRWT_ERR_CAPACITY, len(want)) and "rows_cap too small" in msg, (col, k, st, need)
            assert (buf == -1).all(), f"column {col}: rows written by a refused call (shortage in shard {k} of {K})"
            tried.add("first" if k == 0 else "last" if k == K - 1 else "middle")
        buf = torch.full((len(want) + 4,), -1, dtype=torch.int64, device="cuda")
        st, need, _ = _call(dev, col, buf, len(want))
        assert (st, need) == (L.MBRWT_OK, len(want))
        np.testing.assert_array_equal(buf[:len(want)].cpu().numpy().view(np.uint64), want)
        assert (buf[len(want):] == -1).all()
    assert tried == {"first", "middle", "last"}
    dev.close()


# ---- get_columns on the node images and on shards ----------------------------------------------------

def _gc_contexts(O, which):
    """(dense, build) of a context without row records ('nodes', 'shards') or with both."""
    if which == "shards":
        dense = S.shard_matrix(319)
        return dense, lambda: _sharded(O, dense)[1]
    dense = S.lift_fixture(64).dense
    return dense, lambda: _build(O, dense, 2, layout=which)[1]


@pytest.mark.parametrize("which", ["nodes", "both", "shards"])
def test_get_columns(oracle_mod, which):
    """mbrwt_get_columns where it stages each column whole and clips it
    (k_gc_clip, k_gc_copy): window ends on a one, one before and one after
    it; windows that are empty for some slots only; (b, b) and (0, n); the
    slots ordered so that the staged column grows in mid-loop (ws_gc_pairs is
    regrown) and the reverse; the capacity refusal with complete offsets and
    untouched rows; the device form on a non-default stream."""
    import torch
    from genome_graph_annotation_amd import MBRWTError, _lib as L
    from test_gpu_get_columns import _check, _expect, _raw
    dense, build = _gc_contexts(oracle_mod, which)
    n, m = dense.shape
    sizes = dense.sum(axis=0)
    order = [int(c) for c in np.argsort(sizes, kind="stable")]       # the smallest column first
    nonzero = sizes[sizes > 0]
    assert sizes[order[0]] == 0 and nonzero.max() > 4 * nonzero.min() and len(set(sizes.tolist())) > 3
    # fresh contexts: the staging buffer starts empty and grows with the slots, or is sized by the first
    for columns in (order, order[::-1]):
        ctx = build()
        assert (ctx.rows_stats() is None) == (which != "both")
        _check(ctx, dense, columns)
        ctx.close()
    ctx = build()
    big = order[-1]
    ones = np.flatnonzero(dense[:, big])
    r1, r2 = int(ones[len(ones) // 3]), int(ones[2 * len(ones) // 3])
    assert 0 < r1 < r2 < n - 1
    wins = [(b, e) for b in (r1 - 1, r1, r1 + 1) for e in (r2 - 1, r2, r2 + 1)] + [(r1, r1), (0, 0), (n, n), (0, n)]
    for b, e in wins:
        _check(ctx, dense, None, b, e)
        _check(ctx, dense, order[::-1][:5], b, e)
    # a window that holds rows of some slots only
    small = next(c for c in order if sizes[c] > 0)
    lo = int(np.flatnonzero(dense[:, small])[0])
    woff, _ = _expect(dense, None, lo, lo + 1)
    assert 0 < int((np.diff(woff.astype(np.int64)) == 0).sum()) < m and woff[-1] > 0
    _check(ctx, dense, None, lo, lo + 1)
    # the capacity refusal: offsets complete, rows untouched (host form)
    woff, wrows = _expect(dense)
    total = len(wrows)
    SENT = np.uint64(0xDEADBEEFDEADBEEF)
    off = np.zeros(m + 1, dtype=np.uint64)
    rows = np.full(total, SENT, dtype=np.uint64)
    st, need = _raw(ctx, None, m, 0, n, off, rows, total - 1)
    assert st == L.MBRWT_ERR_CAPACITY and need == total
    np.testing.assert_array_equal(off, woff)
    assert (rows == SENT).all()
    # the device form on a non-default stream: refused one short, then filled
    stream = torch.cuda.Stream()
    off_t = torch.full((m + 1,), -1, dtype=torch.int64, device="cuda")
    rows_t = torch.full((total + 3,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(MBRWTError) as err:
        ctx.get_columns_device(None, 0, None, off_t, rows_t[:total - 1], stream.cuda_stream)
    torch.cuda.synchronize()
    assert err.value.status == L.MBRWT_ERR_CAPACITY and err.value.needed == total
    np.testing.assert_array_equal(off_t.cpu().numpy().view(np.uint64), woff)
    assert (rows_t == -1).all(), "rows written by a refused get_columns_device"
    b, e = r1, r2 + 1
    woff, wrows = _expect(dense, order, b, e)
    off_t.fill_(-1)
    torch.cuda.synchronize()
    got = ctx.get_columns_device(order, b, e, off_t, rows_t, stream.cuda_stream)
    torch.cuda.synchronize()
    assert got == len(wrows)
    np.testing.assert_array_equal(off_t.cpu().numpy().view(np.uint64), woff)
    np.testing.assert_array_equal(rows_t[:got].cpu().numpy().view(np.uint64), wrows)
    assert (rows_t[got:] == -1).all()
    ctx.close()
