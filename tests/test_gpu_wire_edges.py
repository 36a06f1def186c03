"""GPU parity of the exchange's wire kernels (csrc/packids.hip) at bit-width,
chunk, tile and segment edges, against the numpy fixture tests/wire_shapes.py
(itself pinned by tests/test_wire_shapes.py).  The entry points take raw
device arrays, so no tree and no oracle is involved.

Every pack is compared byte for byte over the whole segment (prefilled with
0xAB, so the zero pads count); every unpack runs on a fixture-built wire
uploaded to the device, so a pack bug and an unpack bug cannot cancel; one
further test runs pack -> concatenate -> unpack.  Every device buffer lies
between two 64-byte canaries that are checked when it is read back: the wire
past wire_bytes, the labels past the total (all of them when the exchange is
flagged), the offsets past N + 1.

Not covered, out of reach by size: the 1 << 20 tile cap of
k_unpack_labels_dev (2^31 labels), the 1 << 24 workgroup limit of
k_unpack_labels12 (2^37 labels) and the 0x7FFFFFFF grid limits of the pack
and the offset scan."""
import ctypes as C

import numpy as np
import pytest

from conftest import gpu_available

import wire_shapes as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

CANARY = 0x5C
GUARD = 64


class Buf:
    """n device bytes between two canaries of GUARD bytes (the front one
    `shift` bytes longer: a pointer off 16-byte alignment); the bytes are
    `data`, or `fill`."""

    def __init__(self, nbytes=0, fill=CANARY, shift=0, data=None):
        import torch
        if data is not None:
            data = np.ascontiguousarray(data).view(np.uint8).ravel()
            nbytes = len(data)
        self.n, self.head = int(nbytes), GUARD + shift
        self.t = torch.full((self.head + self.n + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        if data is not None and self.n:
            self.t[self.head:self.head + self.n] = torch.from_numpy(data.copy()).cuda()
        elif fill != CANARY and self.n:
            self.t[self.head:self.head + self.n] = fill

    @property
    def ptr(self):
        return self.t.data_ptr() + self.head

    def read(self, dtype=np.uint8):
        a = self.t.cpu().numpy()
        assert (a[:self.head] == CANARY).all(), "bytes written before the buffer"
        assert (a[self.head + self.n:] == CANARY).all(), "bytes written past the buffer"
        return a[self.head:self.head + self.n].copy().view(dtype)

    def untouched(self):
        return bool((self.read() == CANARY).all())


def _lib():
    from genome_graph_annotation_amd import _lib as L
    return L, L.lib()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _u64s(xs):
    return (C.c_uint64 * max(1, len(xs)))(*[int(x) for x in xs])


def _pack(off, cols, L_, cols_cap, cap, bits_c, bits_l, lab_off, per, cols_shift=0, wire=None, at=0):
    """mbrwt_pack_csr_device into a fresh 0xAB segment (or at byte `at` of `wire`); the segment's bytes."""
    L, lib = _lib()
    d_off, d_cols = Buf(data=off), Buf(data=cols[:cols_cap], shift=cols_shift)
    d_num = Buf(data=np.array([L_], dtype=np.uint64))
    own = wire is None
    if own:
        wire = Buf(per, fill=0xAB)
    L.check(lib.mbrwt_pack_csr_device(d_off.ptr, len(off) - 1, d_cols.ptr, cols_cap, d_num.ptr, cap, bits_c, bits_l,
                                      lab_off, wire.ptr + at, per, _stream()), "pack")
    return wire.read() if own else None


def _pack_case(case, bits_c, bits_l, cols_shift=0):
    """Every (labels_offset, offsets base) form of a pack case: (what, got, want)."""
    cols = S.values(case.cols_cap, bits_l, seed=case.num_labels)
    cnt = S.counts(case.n_rows, bits_c, seed=case.labels_cap)
    for lab_off in (S.labels_offset(case.n_rows, bits_c), S.labels_offset(case.n_rows + 2049, bits_c)):
        per = S.segment_bytes(lab_off, case.labels_cap, bits_l)
        for base in (0, (1 << 32) + 5):
            off = S.offsets_of(cnt, base)
            want = S.wire_segment(off, cols, case.num_labels, case.cols_cap, case.labels_cap, bits_c, bits_l,
                                  lab_off, per)
            got = _pack(off, cols, case.num_labels, case.cols_cap, case.labels_cap, bits_c, bits_l, lab_off, per,
                        cols_shift)
            yield "%s labels at %d, offsets from %d" % (case, lab_off, base), got, want


@pytest.mark.parametrize("bits_c,bits_l", S.WIDTHS)
def test_pack_csr_bytes(bits_c, bits_l):
    for case in S.pack_cases():
        for what, got, want in _pack_case(case, bits_c, bits_l):
            assert S.header(want) == (S.LOST if case.num_labels > case.cols_cap else case.num_labels)
            np.testing.assert_array_equal(got, want, err_msg=what)


def test_pack_csr_unaligned_cols():
    # d_cols 4 bytes off a 16-byte boundary: k_pack_csr in place of k_pack_csr12
    for case in S.pack_cases():
        for (what, got, want), (_, aligned, _) in zip(_pack_case(case, 12, 12, cols_shift=4),
                                                      _pack_case(case, 12, 12)):
            np.testing.assert_array_equal(got, want, err_msg=what)
            np.testing.assert_array_equal(got, aligned, err_msg=what)


def _unpack_labels(recv, nseg, per, lab_off, cap, bits_l, total, values_cap, shift=0):
    """mbrwt_unpack_labels_device into a buffer of `total` labels: ((total, bad), labels or None when untouched)."""
    L, lib = _lib()
    out, st = Buf(4 * total, shift=shift), Buf(16)
    L.check(lib.mbrwt_unpack_labels_device(recv.ptr, nseg, per, lab_off, cap, bits_l, out.ptr, values_cap, st.ptr,
                                           _stream()), "unpack labels")
    status = tuple(int(x) for x in st.read(np.uint64))
    return status, (None if out.untouched() and total else out.read(np.uint32))


def _check_plan_labels(plan, bits_c, bits_l, shift=0):
    segs, _, lab_off, per = S.plan_segments(plan, bits_c, bits_l)
    recv = Buf(data=np.concatenate(segs))
    total = sum(min(x, plan.cap) for x in plan.labels)
    for values_cap in (total, total - 1) if total else (0,):
        _, want, want_st = S.reassemble(segs, plan.rows, lab_off, plan.cap, bits_c, bits_l, values_cap)
        assert want_st[1] == int(values_cap < total or max(plan.labels) > plan.cap)
        st, got = _unpack_labels(recv, len(segs), per, lab_off, plan.cap, bits_l, total, values_cap, shift)
        what = "%s at %d/%d bits, room for %d" % (plan.name, bits_c, bits_l, values_cap)
        assert st == want_st, what
        if want_st[1]:
            assert got is None, what + ": labels written by a flagged exchange"
        else:
            assert got is not None, what
            np.testing.assert_array_equal(got, want, err_msg=what)
    recv.read()


@pytest.mark.parametrize("bits_c,bits_l", S.WIDTHS)
def test_unpack_labels_plans(bits_c, bits_l):
    for plan in S.SEGMENT_PLANS:
        _check_plan_labels(plan, bits_c, bits_l)
    # a rank that lost its CSR (header 2^64 - 1) between two good ones
    L, lib = _lib()
    segs, _, lab_off, per = S.plan_segments(S.SEGMENT_PLANS[5], bits_c, bits_l)
    cap = S.SEGMENT_PLANS[5].cap
    segs[1] = S.wire_segment(np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32), 2, 1, cap, bits_c, bits_l,
                             lab_off, per)
    assert S.header(segs[1]) == S.LOST
    recv = Buf(data=np.concatenate(segs))
    total = S.header(segs[0]) + cap + S.header(segs[2])
    st, got = _unpack_labels(recv, 3, per, lab_off, cap, bits_l, total, total)
    assert st == (total, 1) and got is None
    # more segments than one launch's header scan takes
    out, stb = Buf(64), Buf(16)
    assert lib.mbrwt_unpack_labels_device(recv.ptr, 65, per, lab_off, cap, bits_l, out.ptr, 16, stb.ptr,
                                          _stream()) == L.MBRWT_ERR_INVALID
    assert out.untouched() and stb.untouched()


@pytest.mark.parametrize("bits_l", [7, 12])
def test_unpack_labels_unaligned_values(bits_l):
    # d_values 4 bytes off a 16-byte boundary: k_unpack_labels_dev at bits <= 12
    for plan in S.SEGMENT_PLANS:
        _check_plan_labels(plan, bits_l, bits_l, shift=4)


def _check_offsets(seg_counts, bits, what):
    L, lib = _lib()
    segs, _, per, want = S.count_segments(seg_counts, bits)
    rows = [len(c) for c in seg_counts]
    N, nseg = sum(rows), len(rows)
    recv, arr, s = Buf(data=np.concatenate(segs)), _u64s(rows), _stream()
    tb = C.c_uint64(0)
    L.check(lib.mbrwt_unpack_offsets_device(recv.ptr, nseg, per, arr, bits, None, None, C.byref(tb), s), "scratch size")
    need = int(tb.value)
    assert need == max(1, (N + 2047) // 2048) * 8, what
    tmp, offs = Buf(need), Buf(8 * (N + 1))
    short = C.c_uint64(need - 8)
    assert lib.mbrwt_unpack_offsets_device(recv.ptr, nseg, per, arr, bits, offs.ptr, tmp.ptr, C.byref(short),
                                           s) == L.MBRWT_ERR_INVALID, what
    assert offs.untouched() and tmp.untouched(), what
    L.check(lib.mbrwt_unpack_offsets_device(recv.ptr, nseg, per, arr, bits, offs.ptr, tmp.ptr, C.byref(tb), s), "offsets")
    got = offs.read(np.uint64)
    tmp.read()
    assert len(got) == N + 1 and len(want) == N + 1
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: offsets[%d] = %d, expected %d" % (what, i, got[i], want[i]))


@pytest.mark.parametrize("bits", sorted({c for c, _ in S.WIDTHS}))
def test_unpack_offsets_plans(bits):
    for k, rows in enumerate(S.OFFSET_PLANS):
        _check_offsets([S.counts(n, bits, seed=10 * k + r) for r, n in enumerate(rows)], bits,
                       "rows %s at %d bits" % (rows, bits))
    if bits < 32:
        return
    # block sums and prefixes above 2^32
    top = np.full(2048, 0xFFFFFFFF, dtype=np.uint32)
    _check_offsets([top], 32, "2,048 rows of 2^32 - 1")
    _check_offsets([top[:2], top[:1]], 32, "three rows of 2^32 - 1 over two segments")
    alt = np.zeros(4097, dtype=np.uint32)
    alt[1::2] = 1 << 31
    _check_offsets([alt], 32, "4,097 rows of 0 and 2^31 in turn")
    _check_offsets([alt[1:2500], alt[:1], alt[:1598]], 32, "the same from 2^31, over three segments")


@pytest.mark.parametrize("N", [2_097_152, 2_097_153, 2 * 2_097_152 + 2049])
def test_unpack_offsets_scan_carry(N):
    # k_off_scan_sums: one chunk of 1,024 block sums exactly; the first use of
    # its carry; the carry accumulated twice, the last block partial
    c = (np.arange(N, dtype=np.uint32) & 3).astype(np.uint32)
    a, b = N // 2 + 1, N // 2 + 6
    _check_offsets([c[:a], c[a:b], c[b:]], 2, "%d rows" % N)


@pytest.mark.parametrize("bits", [1, 12, 13, 32])
@pytest.mark.parametrize("nseg", [1, 64, 65, 130])
def test_unpack_segments_many(nseg, bits):
    L, lib = _lib()
    cyc = (5, 0, 1, 33, 0, 0, 8, 7, 64, 9, 31, 257, 32)
    cnts = [cyc[(r + nseg) % len(cyc)] for r in range(nseg)]
    vals = [S.values(n, bits, seed=r) for r, n in enumerate(cnts)]
    stride = (max(cnts) * bits + 31) // 32 * 4 + 4
    wire = np.full(nseg * stride, 0xAB, dtype=np.uint8)  # (what follows a segment's values is not read as one)
    for r, v in enumerate(vals):
        w = S.pack_bits(v, bits).view(np.uint8)
        wire[r * stride:r * stride + len(w)] = w
    total = sum(cnts)
    recv, out = Buf(data=wire), Buf(4 * total)
    L.check(lib.mbrwt_unpack_segments_device(recv.ptr, nseg, stride, _u64s(cnts), bits, out.ptr, _stream()), "unpack")
    want = np.concatenate(vals) & np.uint32((1 << bits) - 1)
    np.testing.assert_array_equal(out.read(np.uint32), want)


def _ids_round(n, bits, seed=0):
    """mbrwt_pack_ids_device of n values with bits above `bits`, and
    mbrwt_unpack_ids_device of the fixture's words."""
    L, lib = _lib()
    v = S.values(n, bits, seed)
    want = S.pack_bits(v, bits)
    d_in, d_words = Buf(data=v), Buf(4 * len(want))
    L.check(lib.mbrwt_pack_ids_device(d_in.ptr, n, bits, d_words.ptr, _stream()), "pack ids")
    got = d_words.read(np.uint32)
    assert np.array_equal(got, want), "pack of %d values at %d bits: word %d" % (
        n, bits, int(np.flatnonzero(got != want)[0]))
    d_w, d_out = Buf(data=want), Buf(4 * n)
    L.check(lib.mbrwt_unpack_ids_device(d_w.ptr, n, bits, d_out.ptr, _stream()), "unpack ids")
    got = d_out.read(np.uint32)
    back = v & np.uint32((1 << bits) - 1)
    assert np.array_equal(got, back), "unpack of %d values at %d bits: value %d" % (
        n, bits, int(np.flatnonzero(got != back)[0]))
    return v, want


@pytest.mark.parametrize("part", ["widths", "stride"])
def test_pack_unpack_ids_widths_and_stride(part):
    if part == "widths":
        for bits in range(1, 33):
            for n in (1, 31, 32, 33, 2049):
                _ids_round(n, bits, seed=bits)
        return
    # grids stop at 16,384 workgroups of 256: the grid-stride loops start above 4,194,304 items
    L, lib = _lib()
    bits, full = 31, 16384 * 256
    for nwords in (full, full + 1 + 256):   # k_pack_ids: one word per thread
        n = nwords * 32 // bits
        assert (n * bits + 31) // 32 == nwords
        _ids_round(n, bits)
    for n in (full, full + 257):            # k_unpack_ids: one value per thread
        v, words = _ids_round(n, bits, seed=1)
    # k_unpack_segments: the last n over two segments
    a = n // 2 + 100
    w0, w1 = S.pack_bits(v[:a], bits), S.pack_bits(v[a:], bits)
    stride = 4 * max(len(w0), len(w1))
    wire = np.full(2 * stride, 0xAB, dtype=np.uint8)
    wire[:4 * len(w0)] = w0.view(np.uint8)
    wire[stride:stride + 4 * len(w1)] = w1.view(np.uint8)
    recv, out = Buf(data=wire), Buf(4 * n)
    L.check(lib.mbrwt_unpack_segments_device(recv.ptr, 2, stride, _u64s([a, n - a]), bits, out.ptr, _stream()), "unpack")
    assert np.array_equal(out.read(np.uint32), v & np.uint32((1 << bits) - 1))


@pytest.mark.parametrize("bits_c,bits_l", [(12, 12), (13, 12), (7, 7)])
@pytest.mark.parametrize("ranks", [3, 8])
def test_wire_end_to_end_plans(ranks, bits_c, bits_l):
    L, lib = _lib()
    plans = [p for p in S.SEGMENT_PLANS if len(p.labels) == ranks]
    assert len(plans) >= 3
    for plan in plans:
        segs, csr, lab_off, per = S.plan_segments(plan, bits_c, bits_l)
        recv = Buf(ranks * per, fill=0xAB)
        for r, (off, cols) in enumerate(csr):
            _pack(off, cols, plan.labels[r], len(cols), plan.cap, bits_c, bits_l, lab_off, per, wire=recv, at=r * per)
        np.testing.assert_array_equal(recv.read(), np.concatenate(segs), err_msg=plan.name)
        total = sum(min(x, plan.cap) for x in plan.labels)
        offs, labels, want_st = S.reassemble(segs, plan.rows, lab_off, plan.cap, bits_c, bits_l, total)
        st, got = _unpack_labels(recv, ranks, per, lab_off, plan.cap, bits_l, total, total)
        assert st == want_st, plan.name
        if want_st[1]:
            assert got is None, plan.name
        else:
            np.testing.assert_array_equal(got, labels, err_msg=plan.name)
        N = sum(plan.rows)
        tb = C.c_uint64(0)
        arr, s = _u64s(plan.rows), _stream()
        L.check(lib.mbrwt_unpack_offsets_device(recv.ptr, ranks, per, arr, bits_c, None, None, C.byref(tb), s), "size")
        tmp, d_off = Buf(int(tb.value)), Buf(8 * (N + 1))
        L.check(lib.mbrwt_unpack_offsets_device(recv.ptr, ranks, per, arr, bits_c, d_off.ptr, tmp.ptr, C.byref(tb), s),
                "offsets")
        np.testing.assert_array_equal(d_off.read(np.uint64), offs, err_msg=plan.name)
