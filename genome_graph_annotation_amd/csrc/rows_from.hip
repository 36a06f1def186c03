// rows_from.hip -- ROW RECORDS straight from row-major data
// (mbrwt_create_from_rows).
//
// A row's record is a function of its label set and the tree's shape alone
// (§4f), so the records can be written from the rows themselves: no index
// column, no rank1, no node image, no dense column.  Per range of rows, on
// the build's stream:
//   upload       the range's offsets (rebased, u32) and column ids;
//   k_rows_keys  one thread per 8 labels: the column range-checked (a device
//                status word) and replaced by its pre-order leaf index (u16)
//                -- 16-byte loads and stores;
//   k_rows_order one lane per row: are the row's keys strictly ascending?
//                Only where some row is not, the range's rows are sorted --
//                hipcub's radix sort on (local row << 16 | key), whole rows in
//                chunks of at most kSortChunk labels -- and an adjacent-equal
//                pass flags a column listed twice;
//   the records  rows_build_range with the label source (rows_emit.hpp
//                emit_label_masks): measure, decide (first range), write, as
//                for a node image.
// The device holds the records plus ONE range's labels (6 bytes per label and
// 4 per row; the sort's scratch only when a range needs it).  Everything
// before the records is rows_from_load, which the per-node row counts
// (rows_counts.hip) run too.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <new>
#include <vector>

#include "device_access.hpp"
#include "mbrwt_internal.hpp"

namespace mbrwt {

namespace {

enum : uint32_t { kStatRange = 1, kStatOrder = 2, kStatDup = 4 };
constexpr uint64_t kSortChunk = 1ull << 25;  // labels per sort call (a row has < 2^16)

// keys[i] = inv[cols[i]] for the range's n labels, 8 per thread; a column
// >= m raises kStatRange (its key: 0)
__global__ __launch_bounds__(256) void k_rows_keys(const uint32_t *__restrict__ cols, uint64_t n, uint32_t m,
                                                   const uint16_t *__restrict__ inv, uint16_t *keys,
                                                   uint32_t *status) {
    const uint64_t groups = (n + 7) / 8;
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    auto key = [&](uint32_t c) -> uint32_t {
        if (c >= m) {
            bad = true;
            return 0u;
        }
        return gld(inv + c);
    };
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gs) {
        const uint64_t i = g * 8;
        if (i + 8 <= n) {  // (both buffers are 16-byte aligned allocations)
            const uint4 lo = gld(reinterpret_cast<const uint4 *>(cols + i));
            const uint4 hi = gld(reinterpret_cast<const uint4 *>(cols + i + 4));
            uint4 out;
            out.x = key(lo.x) | key(lo.y) << 16;
            out.y = key(lo.z) | key(lo.w) << 16;
            out.z = key(hi.x) | key(hi.y) << 16;
            out.w = key(hi.z) | key(hi.w) << 16;
            gst(reinterpret_cast<uint4 *>(keys + i), out);
        } else {
            for (uint64_t k = i; k < n; ++k) gst(keys + k, (uint16_t)key(gld(cols + k)));
        }
    }
    if (bad) atomicOr(status, (uint32_t)kStatRange);
}

// one lane per row: kStatOrder unless every row's keys ascend strictly
__global__ __launch_bounds__(256) void k_rows_order(const uint32_t *__restrict__ off, uint64_t nr,
                                                    const uint16_t *__restrict__ keys, uint32_t *status) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nr; r += gs) {
        const uint32_t a = gld(off + r), b = gld(off + r + 1);
        if (b - a < 2) continue;
        uint32_t prev = gld(keys + a);
        for (uint32_t p = a + 1; p < b; ++p) {
            const uint32_t k = gld(keys + p);
            bad |= k <= prev;
            prev = k;
        }
    }
    if (bad) atomicOr(status, (uint32_t)kStatOrder);
}

// rows [r0, r1) of the range, their labels from `base` on: (local row << 16 | key)
__global__ __launch_bounds__(256) void k_rows_compose(const uint32_t *__restrict__ off, uint64_t r0, uint64_t r1,
                                                      uint32_t base, const uint16_t *__restrict__ keys,
                                                      uint64_t *out) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = r0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < r1; r += gs) {
        const uint32_t a = gld(off + r), b = gld(off + r + 1);
        for (uint32_t p = a; p < b; ++p) gst(out + (p - base), (r - r0) << 16 | (uint64_t)gld(keys + p));
    }
}

// the sorted pairs back into the keys; equal neighbours (one row, one key
// twice) raise kStatDup
__global__ __launch_bounds__(256) void k_rows_sorted(const uint64_t *__restrict__ sorted, uint64_t n, uint16_t *keys,
                                                     uint32_t *status) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    bool dup = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {
        const uint64_t v = gld(sorted + i);
        if (i && gld(sorted + i - 1) == v) dup = true;
        gst(keys + i, (uint16_t)v);
    }
    if (dup) atomicOr(status, (uint32_t)kStatDup);
}

}  // namespace

void rows_from_end(RowsFrom *rf) {
    if (!rf) return;
    for (Workspace *w : {&rf->off, &rf->cols, &rf->keys, &rf->pairs, &rf->pairs2, &rf->sort, &rf->soff, &rf->work})
        if (w->buf) (void)hipFree(w->buf);
    if (rf->h_ids) (void)hipHostFree(rf->h_ids);
    if (rf->d_shape) (void)hipFree(rf->d_shape);
    if (rf->d_inv) (void)hipFree(rf->d_inv);
    if (rf->d_status) (void)hipFree(rf->d_status);
    delete rf;
}

uint64_t rows_from_range_bytes(uint64_t rows, uint64_t labels) {
    // offsets (u32) + columns (u32) + keys (u16), each padded; the sort of an
    // unordered range: two chunks of pairs and hipcub's scratch (about a third)
    const uint64_t sort = 3 * std::min<uint64_t>(labels, kSortChunk + 0x10000) * 8;
    return 4 * (rows + 1) + 6 * labels + sort + 1024;
}

int rows_from_begin(const Tree &shape, hipStream_t s, RowsFrom **out) {
    *out = nullptr;
    const size_t D = shape.nodes.size();
    const uint64_t m = shape.num_columns;
    if (D < 2 || m == 0 || m > 0x10000) {  // (keys are u16: the row records' own column limit)
        set_error(rows_limits_message());
        return MBRWT_ERR_UNSUPPORTED;
    }
    RowsFrom *rf = new (std::nothrow) RowsFrom();
    if (!rf) return MBRWT_ERR_NOMEM;
    struct Guard {
        RowsFrom *p;
        ~Guard() { rows_from_end(p); }
    } guard{rf};
    rf->s = s;
    rf->m = (uint32_t)m;
    rf->range.tree = shape;
    // per dnode the interval of pre-order leaf indices below it: children
    // follow their parent in BFS numbering, so one reverse pass folds them up
    std::vector<LabelNode> tab(D);
    for (size_t v = D; v-- > 0;) {
        const DevNode &dn = shape.nodes[v];
        LabelNode &t = tab[v];
        if (dn.kind == KIND_LEAF) {
            t = LabelNode{0u, kShapeLeaf, dn.label, dn.label + 1};
            continue;
        }
        if (dn.arity == 0 || (size_t)dn.first_child + dn.arity > D || dn.first_child <= v) {
            set_error("shape table: children out of order");
            return MBRWT_ERR_INVALID;
        }
        t = LabelNode{dn.first_child, dn.arity, tab[dn.first_child].lo, tab[dn.first_child + dn.arity - 1].hi};
    }
    std::vector<uint16_t> inv(m);
    rf->perm.resize(m);
    for (uint64_t k = 0; k < m; ++k) {
        rf->perm[k] = shape.label_perm.empty() ? (uint32_t)k : shape.label_perm[k];
        inv[rf->perm[k]] = (uint16_t)k;
    }
    MBRWT_HIP(hipMalloc(&rf->d_shape, D * sizeof(LabelNode)));
    MBRWT_HIP(hipMalloc(&rf->d_inv, m * 2));
    MBRWT_HIP(hipMalloc(&rf->d_status, 8));
    MBRWT_HIP(hipMemcpy(rf->d_shape, tab.data(), D * sizeof(LabelNode), hipMemcpyHostToDevice));
    MBRWT_HIP(hipMemcpy(rf->d_inv, inv.data(), m * 2, hipMemcpyHostToDevice));
    guard.p = nullptr;
    *out = rf;
    return MBRWT_OK;
}

// the rows of the range sorted by key, whole rows in chunks
static int sort_range(RowsFrom &rf, const uint64_t *offsets, uint64_t a, uint64_t b) {
    const uint32_t *d_off = reinterpret_cast<const uint32_t *>(rf.off.buf);
    uint16_t *d_keys = reinterpret_cast<uint16_t *>(rf.keys.buf);
    const uint64_t base0 = offsets[a];
    for (uint64_t r0 = a, r1; r0 < b; r0 = r1) {
        // [r0, r1): as many whole rows as kSortChunk labels hold (a row has at
        // most num_columns <= 2^16 labels: the caller checked)
        r1 = std::upper_bound(offsets + r0 + 1, offsets + b + 1, offsets[r0] + kSortChunk) - offsets - 1;
        r1 = std::max(r1, r0 + 1);
        const uint64_t n = offsets[r1] - offsets[r0];
        if (!n) continue;
        int rc;
        if ((rc = ensure(rf.pairs, n * 8)) || (rc = ensure(rf.pairs2, n * 8))) return rc;
        uint64_t *d_in = reinterpret_cast<uint64_t *>(rf.pairs.buf);
        uint64_t *d_out = reinterpret_cast<uint64_t *>(rf.pairs2.buf);
        const uint32_t base = (uint32_t)(offsets[r0] - base0);
        hipLaunchKernelGGL(k_rows_compose, dim3(grid256(r1 - r0)), dim3(256), 0, rf.s, d_off, r0 - a, r1 - a, base,
                           d_keys, d_in);
        MBRWT_HIP(hipGetLastError());
        int end_bit = 16;
        while (end_bit < 64 && ((r1 - r0 - 1) >> (end_bit - 16))) ++end_bit;
        size_t tb = 0;
        MBRWT_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, d_in, d_out, (int)n, 0, end_bit, rf.s));
        if ((rc = ensure(rf.sort, tb))) return rc;
        MBRWT_HIP(hipcub::DeviceRadixSort::SortKeys(rf.sort.buf, tb, d_in, d_out, (int)n, 0, end_bit, rf.s));
        hipLaunchKernelGGL(k_rows_sorted, dim3(grid256(n)), dim3(256), 0, rf.s, d_out, n, d_keys + base, rf.d_status);
        MBRWT_HIP(hipGetLastError());
    }
    return MBRWT_OK;
}

int rows_from_load(RowsFrom *rf, const uint64_t *offsets, const uint32_t *cols, uint64_t a, uint64_t b,
                   LabelRows *rows) {
    const uint64_t nr = b - a, L = offsets[b] - offsets[a];
    if (L > kRowsFromMaxLabels) {
        set_error("row records from rows: more than 2^31 - 1 labels in one range of rows");
        return MBRWT_ERR_UNSUPPORTED;
    }
    int rc;
    // (padded: k_rows_keys loads and stores whole 16-byte groups only inside n,
    // and an empty range still has non-null buffers)
    if ((rc = ensure(rf->off, (nr + 1) * 4)) || (rc = ensure(rf->cols, L * 4 + 16)) ||
        (rc = ensure(rf->keys, L * 2 + 16)))
        return rc;
    rf->h_off.resize(nr + 1);
    for (uint64_t r = 0; r <= nr; ++r) rf->h_off[r] = (uint32_t)(offsets[a + r] - offsets[a]);
    uint32_t *d_off = reinterpret_cast<uint32_t *>(rf->off.buf);
    uint32_t *d_cols = reinterpret_cast<uint32_t *>(rf->cols.buf);
    uint16_t *d_keys = reinterpret_cast<uint16_t *>(rf->keys.buf);
    MBRWT_HIP(hipMemsetAsync(rf->d_status, 0, 4, rf->s));
    MBRWT_HIP(hipMemcpyAsync(d_off, rf->h_off.data(), (nr + 1) * 4, hipMemcpyHostToDevice, rf->s));
    if (L) {
        MBRWT_HIP(hipMemcpyAsync(d_cols, cols + offsets[a], L * 4, hipMemcpyHostToDevice, rf->s));
        hipLaunchKernelGGL(k_rows_keys, dim3(grid256((L + 7) / 8)), dim3(256), 0, rf->s, d_cols, L, rf->m, rf->d_inv,
                           d_keys, rf->d_status);
        MBRWT_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_rows_order, dim3(grid256(nr)), dim3(256), 0, rf->s, d_off, nr, d_keys, rf->d_status);
        MBRWT_HIP(hipGetLastError());
    }
    uint32_t st = 0;
    MBRWT_HIP(hipMemcpyAsync(&st, rf->d_status, 4, hipMemcpyDeviceToHost, rf->s));
    MBRWT_HIP(hipStreamSynchronize(rf->s));
    if (st & kStatRange) {
        set_error("column id >= num_columns");
        return MBRWT_ERR_INVALID;
    }
    if (st & kStatOrder) {
        if ((rc = sort_range(*rf, offsets, a, b))) return rc;
        MBRWT_HIP(hipMemcpyAsync(&st, rf->d_status, 4, hipMemcpyDeviceToHost, rf->s));
        MBRWT_HIP(hipStreamSynchronize(rf->s));
        if (st & kStatDup) {
            set_error("a column listed twice in a row");
            return MBRWT_ERR_INVALID;
        }
    }
    *rows = LabelRows{rf->d_shape, d_off, d_keys};
    return MBRWT_OK;
}

int rows_from_range(RowsFrom *rf, RowsBuild *rb, const uint64_t *offsets, const uint32_t *cols, uint64_t a, uint64_t b,
                    uint64_t *labels) {
    Ctx &range = rf->range;
    if (int rc = rows_from_load(rf, offsets, cols, a, b, &range.label_rows)) return rc;
    range.tree.num_rows = b - a;
    range.tree.num_relations = offsets[b] - offsets[a];
    if (int rc = rows_build_range(rb, range, a)) return rc;
    *labels += offsets[b] - offsets[a];
    return MBRWT_OK;
}

}  // namespace mbrwt
