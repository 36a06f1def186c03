// rows_columns.hip -- mbrwt_get_columns: the sparse columns of a row window,
// for many columns at once -- the inverse of
// mbrwt_create_from_sparse_columns (rows_from_cols.hip).
//
// Row-record contexts (layout ROWS, and BOTH through its records): the
// records are swept a fixed number of times, whatever the number of columns.
//   slot map     column -> requested slot (u32, kNoSlot = not asked for)
//   count sweep  one lane per row of the window through the record form's
//                one-lane walker (rows_columns.hpp): the wanted labels per
//                slot -- privatised in LDS per workgroup up to kGcLdsSlots
//                slots -- and, when the window is one chunk, per row.  A scan
//                of the slot totals is the result's offsets: the sizing call
//                and the capacity refusal end here, no row written.
//   emit sweep   per chunk of rows: the per-row counts scanned (recounted
//                first when the window takes several chunks: 3 sweeps instead
//                of 2; a chunk is sized for twice the window's mean pairs per
//                row and halved where it counts more), the walk again writing (slot, row - chunk begin)
//                pairs in row order, a stable radix sort over the slot bits --
//                every slot's rows stay ascending -- and a scatter of the
//                sorted runs behind the per-slot cursors.
// Device bytes: 16 per pair of a chunk (u32 key and value, the two halves of
// the sort's DoubleBuffer -- that form of hipcub's sort keeps no further copy;
// 8 for a single column, which is not sorted) + the sort's histograms as
// queried, 4 per row of a chunk, 24 per slot and 4 per column of the matrix.
//
// Contexts without row records (node images, row shards): run_get_column per
// slot, staged and clipped to the window on the device -- the per-column cost,
// twice (sizes first: a refused call must not touch the rows).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "mbrwt_internal.hpp"
#include "rows_columns.hpp"
#include "rows_record.hpp"

namespace mbrwt {
namespace {

// block records in every code, and record classes through their dictionary
struct BlockRowLabels {
    RowsView v;  // (record classes: the dictionary's records)
    const uint32_t *table;
    const uint32_t *classes;
    uint32_t class_bits;
    template <class Leaf>
    __device__ bool operator()(uint64_t row, Leaf leaf) const {
        if (classes) row = class_field(classes, class_bits, row);
        if (row >= v.num_rows) return false;  // (a class the dictionary does not have)
        uint64_t masks;
        uint32_t count;
        rows_locate(v, row, masks, count);
        if (!count) return true;
        return record_walk(v, table, masks, count, leaf, [](uint32_t) {});
    }
};

// a per-row count as the u64 summand of a chunk's pair count
struct GcWiden {
    __device__ unsigned long long operator()(const uint32_t &v) const { return v; }
};

// the sorted pairs' runs: run_start[slot] = the first pair of the slot's run
__global__ __launch_bounds__(256) void k_gc_heads(const uint32_t *keys, uint64_t np, uint32_t *run_start) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gs) {
        const uint32_t k = gld(keys + i);
        if (i == 0 || gld(keys + i - 1) != k) gst(run_start + k, (uint32_t)i);
    }
}
// pair i of slot k's run -> d_rows[cursor[k] + rank in the run]
__global__ __launch_bounds__(256) void k_gc_scatter(const uint32_t *keys, const uint32_t *vals, uint64_t np,
                                                    const uint32_t *run_start, const unsigned long long *cursor,
                                                    uint32_t n_slots, uint64_t chunk_begin, uint64_t *d_rows,
                                                    uint64_t cap) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gs) {
        const uint32_t k = gld(keys + i);
        if (k >= n_slots) continue;
        const uint64_t at = gld(cursor + k) + (i - gld(run_start + k));
        if (at < cap) gst(d_rows + at, chunk_begin + gld(vals + i));
    }
}
// the cursors move past this chunk's runs (one lane per run: its last pair)
__global__ __launch_bounds__(256) void k_gc_advance(const uint32_t *keys, uint64_t np, const uint32_t *run_start,
                                                    unsigned long long *cursor, uint32_t n_slots) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gs) {
        const uint32_t k = gld(keys + i);
        if (k >= n_slots) continue;
        if (i + 1 == np || gld(keys + i + 1) != k) cursor[k] += i + 1 - gld(run_start + k);
    }
}

// the fallback's clip: bounds[0..1] = the staged column's [lo, hi) inside the
// window (two binary searches), *size = hi - lo
__global__ void k_gc_clip(const uint64_t *col, uint64_t n, uint64_t rb, uint64_t re, unsigned long long *bounds,
                          unsigned long long *size) {
    uint64_t lo[2];
    const uint64_t key[2] = {rb, re};
    for (int q = 0; q < 2; ++q) {  // the first id >= key[q]
        uint64_t a = 0, b = n;
        while (a < b) {
            const uint64_t mid = a + (b - a) / 2;
            if (gld(col + mid) < key[q]) a = mid + 1;
            else b = mid;
        }
        lo[q] = a;
    }
    bounds[0] = lo[0];
    bounds[1] = lo[1];
    if (size) *size = lo[1] - lo[0];
}
__global__ __launch_bounds__(256) void k_gc_copy(const uint64_t *col, const unsigned long long *bounds,
                                                 const uint64_t *dst_off, uint64_t *d_rows, uint64_t cap) {
    const uint64_t lo = bounds[0], n = bounds[1] - lo, at = gld(dst_off);
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs)
        if (at + i < cap) gst(d_rows + at + i, gld(col + lo + i));
}

constexpr uint64_t kGcMaxPairs = 0x7FFFFFFFull;   // (the device sort counts its items in an int)
constexpr uint64_t kGcMaxChunkRows = 1ull << 32;  // (values are u32 relative to the chunk)

// device bytes the call may take: the free memory less the 8 GiB reserve of the builds
uint64_t gc_budget() {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const uint64_t reserve = 8ull << 30;
    return std::max<uint64_t>(free_b > reserve ? free_b - reserve : 0, free_b / 8);
}

// the slot totals (zero-padded by one) scanned into the offsets; *total = the
// rows of the result; the capacity protocol.  One synchronisation.
int gc_offsets(Ctx &c, const unsigned long long *d_totals, uint64_t n_columns, uint64_t *d_offsets, bool have_rows,
               uint64_t rows_cap, uint64_t *rows_needed, const unsigned long long *d_status, uint64_t *total,
               hipStream_t s) {
    int rc;
    size_t sb = 0;
    MBRWT_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, sb, d_totals, d_offsets, n_columns + 1, s));
    if ((rc = ensure(c.ws_gc_tmp, sb))) return rc;
    MBRWT_HIP(hipcub::DeviceScan::ExclusiveSum(c.ws_gc_tmp.buf, sb, d_totals, d_offsets, n_columns + 1, s));
    MBRWT_HIP(hipMemcpyAsync(c.h_scalars, d_offsets + n_columns, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    c.h_scalars[1] = 0;
    if (d_status) MBRWT_HIP(hipMemcpyAsync(c.h_scalars + 1, d_status, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    MBRWT_HIP(hipStreamSynchronize(s));
    if (c.h_scalars[1]) {
        set_error("row-record walk failed (corrupt image)");
        return MBRWT_ERR_DEVICE;
    }
    *total = c.h_scalars[0];
    if (rows_needed) *rows_needed = *total;
    if (*total > rows_cap || (*total && !have_rows)) {
        set_error("row buffer too small (see rows_needed)");
        return MBRWT_ERR_CAPACITY;
    }
    return MBRWT_OK;
}

int records_get_columns(Ctx &c, const GcSweeps &sw, const std::vector<uint32_t> &slot_of, uint64_t n_columns,
                        uint64_t rb, uint64_t re, uint64_t *d_offsets, uint64_t *d_rows, uint64_t rows_cap,
                        uint64_t *rows_needed, Workspace *stage, hipStream_t s) {
    int rc;
    const uint64_t m = slot_of.size(), W = re - rb;
    // ws_gc_slots: [totals u64 x (n_columns + 1)][cursor u64 x n_columns][status u64 x 2]
    //              [run_start u32 x n_columns][slot map u32 x m]
    const uint64_t zero_bytes = (2 * n_columns + 3) * 8;
    if ((rc = ensure(c.ws_gc_slots, zero_bytes + (n_columns + m) * 4))) return rc;
    auto *d_totals = reinterpret_cast<unsigned long long *>(c.ws_gc_slots.buf);
    unsigned long long *d_cursor = d_totals + n_columns + 1, *d_status = d_cursor + n_columns;
    uint32_t *d_run = reinterpret_cast<uint32_t *>(d_status + 2), *d_slot_of = d_run + n_columns;
    MBRWT_HIP(hipMemsetAsync(d_totals, 0, zero_bytes, s));
    MBRWT_HIP(hipMemcpyAsync(d_slot_of, slot_of.data(), m * 4, hipMemcpyHostToDevice, s));

    // the chunk plan, part 1: one chunk when the window's per-row counts fit
    // (then the count sweep keeps them), or when the test hook says so
    const uint64_t budget = gc_budget();
    const bool try_single =
        c.columns_chunk ? c.columns_chunk >= W : (W <= kGcMaxChunkRows && 4 * (W + 1) <= budget / 2);
    if (try_single && (rc = ensure(c.ws_gc_rows, 4 * (W + 1)))) return rc;

    GcParams p{};
    p.slot_of = d_slot_of;
    p.num_columns = m;
    p.row0 = rb;
    p.n = W;
    p.row_cnt = try_single ? reinterpret_cast<uint32_t *>(c.ws_gc_rows.buf) : nullptr;
    p.totals = d_totals;
    p.lds_slots = n_columns <= kGcLdsSlots ? (uint32_t)n_columns : 0;
    p.status = d_status;
    if (W) {
        sw.count(p, s);
        MBRWT_HIP(hipGetLastError());
    }
    uint64_t total = 0;
    if ((rc = gc_offsets(c, d_totals, n_columns, d_offsets, d_rows || stage, rows_cap, rows_needed, d_status, &total,
                         s)))
        return rc;
    if (!total) return MBRWT_OK;
    if (stage) {
        if ((rc = ensure(*stage, total * sizeof(uint64_t)))) return rc;
        d_rows = reinterpret_cast<uint64_t *>(stage->buf);
    }

    // part 2: the pairs of a chunk.  One chunk holds the whole result when it
    // fits.  Else a chunk is sized for twice the window's mean pairs per row,
    // and a chunk that counts more pairs than the buffers hold is halved and
    // recounted (one row's pairs, at most n_columns, always fit).
    const bool sort = n_columns > 1;
    const uint64_t per_pair = sort ? 16 : 8;
    int bits = 1;
    while ((1ull << bits) < n_columns) ++bits;
    // the sort's own scratch for np pairs (the DoubleBuffer form: histograms and
    // look-back state only, no copy of the pairs)
    auto sort_bytes = [&](uint64_t np, size_t *bytes) -> hipError_t {
        hipcub::DoubleBuffer<uint32_t> kb(nullptr, nullptr), vb(nullptr, nullptr);
        *bytes = 0;
        return sort ? hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, kb, vb, (int)np, 0, bits, s) : hipSuccess;
    };
    const uint64_t rows_bytes = try_single ? 4 * (W + 1) : 0;
    const uint64_t room = budget > rows_bytes ? budget - rows_bytes : 0;
    size_t sort_b = 0;
    MBRWT_HIP(sort_bytes(std::max<uint64_t>(1, std::min(kGcMaxPairs, room / per_pair)), &sort_b));
    const uint64_t pair_cap = room > sort_b ? std::min(kGcMaxPairs, (room - sort_b) / per_pair) : 0;
    const bool single = try_single && (total <= pair_cap || c.columns_chunk);
    uint64_t R = W, pmax = total;
    if (!single) {
        const double mean2 = 2.0 * (double)total / (double)W;  // (total > 0)
        R = c.columns_chunk ? c.columns_chunk : (uint64_t)std::min((double)kGcMaxChunkRows, (double)pair_cap / mean2);
        R = std::max<uint64_t>(1, std::min(R, W));
        pmax = std::min(total, std::max(n_columns, (uint64_t)(mean2 * (double)R) + 1));
        if (!c.columns_chunk && pmax > pair_cap) {
            set_error("get_columns: no device memory for one row's pairs");
            return MBRWT_ERR_NOMEM;
        }
        if ((rc = ensure(c.ws_gc_rows, 4 * (R + 1)))) return rc;
    }
    if (pmax > kGcMaxPairs) {
        set_error("get_columns: more than 2^31 - 1 pairs in one chunk");
        return MBRWT_ERR_UNSUPPORTED;
    }
    if ((rc = ensure(c.ws_gc_pairs, pmax * per_pair))) return rc;
    uint32_t *d_keys = reinterpret_cast<uint32_t *>(c.ws_gc_pairs.buf), *d_vals = d_keys + pmax;
    uint32_t *d_keys2 = sort ? d_vals + pmax : d_keys, *d_vals2 = sort ? d_keys2 + pmax : d_vals;
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(c.ws_gc_rows.buf);
    unsigned long long *d_np = d_status + 1;  // a chunk's pair count
    hipcub::TransformInputIterator<unsigned long long, GcWiden, const uint32_t *> cnt64(d_cnt, GcWiden{});
    size_t scan_b = 0, red_b = 0;
    MBRWT_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, d_cnt, d_cnt, R + 1, s));
    MBRWT_HIP(hipcub::DeviceReduce::Sum(nullptr, red_b, cnt64, d_np, R, s));
    MBRWT_HIP(sort_bytes(pmax, &sort_b));
    if ((rc = ensure(c.ws_gc_tmp, std::max(std::max(scan_b, red_b), sort_b)))) return rc;
    MBRWT_HIP(hipMemcpyAsync(d_cursor, d_offsets, n_columns * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));

    p.totals = nullptr;
    p.lds_slots = 0;
    p.row_off = d_cnt;
    p.keys = d_keys;
    p.vals = d_vals;
    for (uint64_t cb = rb, nr; cb < re; cb += nr) {
        nr = std::min(R, re - cb);
        uint64_t np = total;
        p.row0 = cb;
        p.row_cnt = d_cnt;
        for (bool counted = single; !counted;) {  // this chunk's per-row counts and their sum
            p.n = nr;
            sw.count(p, s);
            MBRWT_HIP(hipGetLastError());
            MBRWT_HIP(hipcub::DeviceReduce::Sum(c.ws_gc_tmp.buf, red_b, cnt64, d_np, nr, s));
            MBRWT_HIP(hipMemcpyAsync(c.h_scalars, d_np, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            MBRWT_HIP(hipStreamSynchronize(s));  // (once per chunk, and once more per halving)
            np = c.h_scalars[0];
            counted = np <= pmax;
            if (!counted) {
                if (nr == 1) {
                    set_error("get_columns: one row's pairs exceed the number of columns");
                    return MBRWT_ERR_DEVICE;
                }
                nr /= 2;
            }
        }
        if (!np) continue;  // (no pair: the cursors stay)
        p.n = nr;
        MBRWT_HIP(hipMemsetAsync(d_cnt + nr, 0, 4, s));
        MBRWT_HIP(hipcub::DeviceScan::ExclusiveSum(c.ws_gc_tmp.buf, scan_b, d_cnt, d_cnt, nr + 1, s));
        sw.emit(p, s);
        MBRWT_HIP(hipGetLastError());
        hipcub::DoubleBuffer<uint32_t> kb(d_keys, d_keys2), vb(d_vals, d_vals2);
        if (sort) MBRWT_HIP(hipcub::DeviceRadixSort::SortPairs(c.ws_gc_tmp.buf, sort_b, kb, vb, (int)np, 0, bits, s));
        const uint32_t *sk = kb.Current(), *sv = vb.Current();
        const dim3 g(grid256(np));
        hipLaunchKernelGGL(k_gc_heads, g, dim3(256), 0, s, sk, np, d_run);
        hipLaunchKernelGGL(k_gc_scatter, g, dim3(256), 0, s, sk, sv, np, (const uint32_t *)d_run,
                           (const unsigned long long *)d_cursor, (uint32_t)n_columns, cb, d_rows, total);
        hipLaunchKernelGGL(k_gc_advance, g, dim3(256), 0, s, sk, np, (const uint32_t *)d_run, d_cursor,
                           (uint32_t)n_columns);
        MBRWT_HIP(hipGetLastError());
    }
    // (a walk that failed only in a recount is reported too)
    MBRWT_HIP(hipMemcpyAsync(c.h_scalars + 1, d_status, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    MBRWT_HIP(hipStreamSynchronize(s));
    if (c.h_scalars[1]) {
        set_error("row-record walk failed (corrupt image)");
        return MBRWT_ERR_DEVICE;
    }
    return MBRWT_OK;
}

// one column staged whole in ws_gc_pairs: *d_col, *need = its rows
int gc_stage_column(Ctx &c, uint64_t column, const uint64_t **d_col, uint64_t *need, hipStream_t s) {
    for (int attempt = 0;; ++attempt) {
        uint64_t *buf = reinterpret_cast<uint64_t *>(c.ws_gc_pairs.buf);
        int rc = run_get_column(c, column, buf, buf ? c.ws_gc_pairs.bytes / 8 : 0, need, s);
        if (rc == MBRWT_ERR_CAPACITY && attempt == 0) {
            if ((rc = ensure(c.ws_gc_pairs, *need * sizeof(uint64_t)))) return rc;
            continue;
        }
        *d_col = buf;
        return rc;
    }
}

int columns_get_columns(Ctx &c, const uint64_t *columns, uint64_t n_columns, uint64_t rb, uint64_t re,
                        uint64_t *d_offsets, uint64_t *d_rows, uint64_t rows_cap, uint64_t *rows_needed,
                        Workspace *stage, hipStream_t s) {
    int rc;
    // ws_gc_slots: [sizes u64 x (n_columns + 1)][bounds u64 x 2]
    if ((rc = ensure(c.ws_gc_slots, (n_columns + 3) * 8))) return rc;
    auto *d_sizes = reinterpret_cast<unsigned long long *>(c.ws_gc_slots.buf);
    unsigned long long *d_bounds = d_sizes + n_columns + 1;
    MBRWT_HIP(hipMemsetAsync(d_sizes, 0, (n_columns + 3) * 8, s));
    for (int pass = 0; pass < 2; ++pass) {
        for (uint64_t j = 0; j < n_columns; ++j) {
            const uint64_t *d_col = nullptr;
            uint64_t need = 0;
            if ((rc = gc_stage_column(c, columns ? columns[j] : j, &d_col, &need, s))) return rc;
            if (!need) continue;
            hipLaunchKernelGGL(k_gc_clip, dim3(1), dim3(1), 0, s, d_col, need, rb, re, d_bounds,
                               pass ? (unsigned long long *)nullptr : d_sizes + j);
            if (pass)
                hipLaunchKernelGGL(k_gc_copy, dim3(grid256(need)), dim3(256), 0, s, d_col,
                                   (const unsigned long long *)d_bounds, (const uint64_t *)(d_offsets + j), d_rows,
                                   rows_cap);
            MBRWT_HIP(hipGetLastError());
        }
        if (pass) break;
        uint64_t total = 0;
        if ((rc = gc_offsets(c, d_sizes, n_columns, d_offsets, d_rows || stage, rows_cap, rows_needed, nullptr, &total,
                             s)))
            return rc;
        if (!total) return MBRWT_OK;
        if (stage) {
            if ((rc = ensure(*stage, total * sizeof(uint64_t)))) return rc;
            d_rows = reinterpret_cast<uint64_t *>(stage->buf);
        }
        rows_cap = total;
    }
    MBRWT_HIP(hipStreamSynchronize(s));
    return MBRWT_OK;
}

}  // namespace

int run_get_columns(Ctx &c, const uint64_t *columns, uint64_t n_columns, uint64_t row_begin, uint64_t row_end,
                    uint64_t *d_offsets, uint64_t *d_rows, uint64_t rows_cap, uint64_t *rows_needed, Workspace *stage,
                    hipStream_t s) {
    if (rows_needed) *rows_needed = 0;
    if (!d_rows && !stage) rows_cap = 0;
    if (!n_columns) {
        MBRWT_HIP(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), s));
        MBRWT_HIP(hipStreamSynchronize(s));
        return MBRWT_OK;
    }
    if (!c.rows.ready || !c.shards.empty())
        return columns_get_columns(c, columns, n_columns, row_begin, row_end, d_offsets, d_rows, rows_cap, rows_needed,
                                   stage, s);
    std::vector<uint32_t> slot_of(c.tree.num_columns, kNoSlot);
    for (uint64_t j = 0; j < n_columns; ++j) slot_of[columns ? columns[j] : j] = (uint32_t)j;
    const RowsImage &im = c.rows;
    const GcSweeps sw =
        im.var ? var_gc_sweeps(c)
               : gc_sweeps(BlockRowLabels{rows_view(im, im.classes ? im.num_classes : c.tree.num_rows), walk_table(im),
                                          im.classes, im.class_bits});
    return records_get_columns(c, sw, slot_of, n_columns, row_begin, row_end, d_offsets, d_rows, rows_cap, rows_needed,
                               stage, s);
}

}  // namespace mbrwt
