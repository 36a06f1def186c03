"""The wire fixture (tests/wire_shapes.py) pinned on the CPU: the bit packing
against Python's big integers and against dist._pack, the segment builder and
the reassembly against each other over every segment plan, the label offset
against the library's host function, and what the shape lists promise (the
GPU tests of test_gpu_wire_edges.py rely on all of it)."""
import numpy as np
import pytest

import wire_shapes as S


def _big_int_words(vals, bits):
    x = sum((int(v) & ((1 << bits) - 1)) << (i * bits) for i, v in enumerate(vals))
    nw = (len(vals) * bits + 31) // 32
    return np.frombuffer(x.to_bytes(4 * nw, "little"), dtype=np.uint32)


@pytest.mark.parametrize("bits", range(1, 33))
def test_pack_bits_against_big_integers(bits):
    for n in (0, 1, 2, 31, 32, 33, 1000):
        v = S.values(n, bits, seed=bits)
        w = S.pack_bits(v, bits)
        assert w.dtype == np.uint32 and len(w) == (n * bits + 31) // 32
        np.testing.assert_array_equal(w, _big_int_words(v, bits))
        back = S.unpack_bits(w, n, bits)
        assert back.dtype == np.uint32
        np.testing.assert_array_equal(back, v & np.uint32((1 << bits) - 1))
        # (trailing words are not read)
        np.testing.assert_array_equal(S.unpack_bits(np.concatenate([w, ~w[:1], ~w[:1]]), n, bits), back)


@pytest.mark.parametrize("bits", [1, 7, 12, 13, 31, 32])
def test_value_generators(bits):
    m = (1 << bits) - 1
    for n in (12, 64, 2049):
        v = S.values(n, bits)
        low = v & np.uint32(m)
        for want in (0, m, 1 << (bits - 1)):
            assert (low == want).any()
        if n >= 64:
            assert (v <= m).sum() > n // 4               # values in range
        if bits < 32:
            assert n < 64 or (v > m).sum() > n // 4      # and values with bits above `bits`
            assert (v == 0xFFFFFFFF).any() and ((v > m) & (low == 0)).any()
        c = S.counts(n, bits)
        assert c[0] & m == m and c[-1] & m == m and (c == 0).any()
    assert len(S.values(0, bits)) == 0 and len(S.counts(0, bits)) == 0
    assert S.values(1, bits)[0] & m == 1 << (bits - 1)
    np.testing.assert_array_equal(S.values(100, bits, 3), S.values(100, bits, 3))


@pytest.mark.parametrize("bits", [1, 7, 12, 13, 17, 31, 32])
def test_pack_bits_against_dist_pack(bits):
    import torch
    from genome_graph_annotation_amd.dist import _pack, _unpack, _words
    for n in (1, 33, 1000):
        v = S.values(n, bits, seed=7) & np.uint32((1 << bits) - 1)  # (_pack takes values in range)
        out = torch.zeros(_words(n, bits), dtype=torch.int32)
        _pack(torch.from_numpy(v.view(np.int32).copy()), n, bits, out)
        np.testing.assert_array_equal(out.numpy().view(np.uint32), S.pack_bits(v, bits))
        back = torch.zeros(n, dtype=torch.int32)
        _unpack(torch.from_numpy(S.pack_bits(v, bits).view(np.int32).copy()), n, bits, back)
        np.testing.assert_array_equal(back.numpy().view(np.uint32), v)


def test_labels_offset_against_the_library():
    from genome_graph_annotation_amd import _lib as L
    for bits in range(1, 33):
        for n in S.ROW_EDGES + (2_097_152, 2_097_153, (1 << 32) + 1):
            assert S.labels_offset(n, bits) == L.lib().mbrwt_wire_labels_offset(n, bits), (n, bits)
    assert S.labels_offset(0, 12) == 16 and S.labels_offset(10, 12) == 64
    # the per-segment size rule of dist.DeviceAllGatherV
    assert S.segment_bytes(16, 0, 12) == 32 and S.segment_bytes(64, 33, 12) == 64 + 96
    assert S.segment_bytes(16, 1, 1) == 32 and S.segment_bytes(16, 8203, 13) == 13392  # (16 + 257 * 13 * 4 = 13,380)


def test_wire_segment_by_hand():
    # 3 rows of 1, 0 and 4,097 (= 1 in 12 bits) labels, 5 labels of which 3 fit the capacity
    off = np.array([7, 8, 8, 8 + 4097], dtype=np.uint64) + np.uint64(1 << 32)
    cols = np.array([0xFFF, 0x1001, 0x800, 5, 6], dtype=np.uint32)
    seg = S.wire_segment(off, cols, 5, 5, 3, 12, 12, 64, 112)
    assert len(seg) == 112 and S.header(seg) == 5
    assert bytes(seg[8:16]) == (1 | 0 << 12 | 1 << 24).to_bytes(8, "little")
    assert bytes(seg[64:72]) == (0xFFF | 0x001 << 12 | 0x800 << 24).to_bytes(8, "little")
    assert not seg[16:64].any() and not seg[72:].any()
    lost = S.wire_segment(off, cols, 6, 5, 3, 12, 12, 64, 112)
    assert S.header(lost) == S.LOST and not lost[8:].any()
    o, l, st = S.reassemble([seg, lost], [3, 0], 64, 3, 12, 12, 100)
    np.testing.assert_array_equal(o, [0, 1, 1, 2])
    assert st == (6, 1) and len(l) == 0
    fits = S.wire_segment(off, cols, 3, 5, 3, 12, 12, 64, 112)
    np.testing.assert_array_equal(fits[8:], seg[8:])
    o, l, st = S.reassemble([fits], [3], 64, 3, 12, 12, 3)
    assert st == (3, 0)
    np.testing.assert_array_equal(l, [0xFFF, 0x001, 0x800])


@pytest.mark.parametrize("plan", S.SEGMENT_PLANS, ids=lambda p: p.name)
def test_segment_plans_round_trip(plan):
    for bits_c, bits_l in S.WIDTHS:
        segs, csr, lab_off, per = S.plan_segments(plan, bits_c, bits_l)
        assert all(len(s) == per for s in segs) and per % 16 == 0 and lab_off % 16 == 0
        want_l = [c[:min(L, plan.cap)] & np.uint32((1 << bits_l) - 1) for (_, c), L in zip(csr, plan.labels)]
        total = sum(len(x) for x in want_l)
        cnt = np.concatenate([(o[1:] - o[:-1]) & np.uint64((1 << bits_c) - 1) for o, _ in csr])
        over = any(L > plan.cap for L in plan.labels)
        offs, labels, st = S.reassemble(segs, plan.rows, lab_off, plan.cap, bits_c, bits_l, total)
        assert st == (total, int(over))
        np.testing.assert_array_equal(offs, np.concatenate([[0], np.cumsum(cnt, dtype=np.uint64)]).astype(np.uint64))
        if not over:
            np.testing.assert_array_equal(labels, np.concatenate(want_l + [np.zeros(0, dtype=np.uint32)]))
        if total:
            _, l2, st2 = S.reassemble(segs, plan.rows, lab_off, plan.cap, bits_c, bits_l, total - 1)
            assert st2 == (total, 1) and len(l2) == 0
        for s, L in zip(segs, plan.labels):
            assert S.header(s) == L
            # zero pads: after the counts' and the labels' last words
            assert not s[lab_off + (min(L, plan.cap) * bits_l + 31) // 32 * 4:].any()


def test_shape_lists_cover_what_they_promise():
    assert len(S.WIDTHS) == 11 and {(13, 12), (12, 11), (12, 12), (1, 1), (32, 32)} <= set(S.WIDTHS)
    assert {len(p.labels) for p in S.SEGMENT_PLANS} >= {1, 2, 7, 8, 9, 63, 64}
    ends = set()
    for p in S.SEGMENT_PLANS:
        assert len(p.rows) == len(p.labels) <= 64
        ends |= set(np.cumsum([min(L, p.cap) for L in p.labels])[:-1].tolist())
    assert {8, 17, 47, 2048, 4096, 8191, 8192, 8193} <= ends
    assert any(p.labels[0] == 0 and sum(p.labels) for p in S.SEGMENT_PLANS)
    assert any(p.labels[-1] == 0 and sum(p.labels) for p in S.SEGMENT_PLANS)
    assert any(a == b == 0 and sum(p.labels) for p in S.SEGMENT_PLANS for a, b in zip(p.labels[1:], p.labels[2:]))
    assert any(p.cap in p.labels for p in S.SEGMENT_PLANS)
    assert {len(r) for r in S.OFFSET_PLANS} == set(range(1, 9))
    assert {n for r in S.OFFSET_PLANS for n in r} >= set(S.ROW_EDGES)
    for where in (0, 1, -1):
        assert any(len(r) > 2 and r[where] == 0 and sum(r) for r in S.OFFSET_PLANS)
    segs, lab_off, per, offs = S.count_segments([S.counts(n, 13) for n in (33, 0, 9)], 13)
    o2, _, st = S.reassemble(segs, (33, 0, 9), lab_off, 0, 13, 13, 0)
    np.testing.assert_array_equal(o2, offs)
    assert st == (0, 0) and len(offs) == 43 and all(len(s) == per for s in segs)
    cases = S.pack_cases()
    assert {c.n_rows for c in cases} >= set(S.ROW_EDGES) and {c.num_labels for c in cases} >= set(S.LABEL_EDGES)
    for cap in S.LABEL_CAPS:
        assert {c.num_labels - cap for c in cases if c.labels_cap == cap and c.cols_cap == cap + 1} == {-1, 0, 1, 2}
    assert S.BIG_CAP > 8192 and S.BIG_CAP % 8 and S.BIG_CAP % 32
