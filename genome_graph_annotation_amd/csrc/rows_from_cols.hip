// rows_from_cols.hip -- ROW RECORDS from sparse columns
// (mbrwt_create_from_sparse_columns).
//
// The reference holds its data column-major before a BRWT conversion: per
// label the ascending ids of its set rows.  The record builders read rows
// (LabelRows: per row its pre-order keys, ascending), so a range of rows is
// TRANSPOSED on the device.  Per range [a, b), on the build's stream:
//   host          every column's slice of ids in [a, b) (cols_host.hpp) staged
//                 as u32 local rows into a pinned buffer, the slices in
//                 PRE-ORDER of their columns, with their offsets and a work
//                 list of (slice, chunk) pairs;
//   k_cols_compose  one workgroup per work item, consecutive lanes on
//                 consecutive staged ids: (local row << 16 | key) per label,
//                 the key being the slice's pre-order index; an id outside
//                 the range or not above its predecessor in the slice raises
//                 the status word; a histogram of the local rows;
//   the sort      ONE stable hipcub radix sort over the row bits alone: the
//                 composed pairs already ascend in key, so every row's keys
//                 come out strictly ascending (a range of one row is not
//                 sorted at all: the composed order is the row's);
//   the scan      the histogram's exclusive sum: the row offsets;
//   k_cols_rows   the u16 keys out of the sorted pairs, and the longest row.
// That is the LabelRows rows_from_load ends with; rows_build_range and
// rows_counts_range take it unchanged.  The slices of consecutive ranges tile
// every column (cols_host.hpp), so the two device checks prove the whole
// input valid without a host pass over the ids.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "device_access.hpp"
#include "mbrwt_internal.hpp"

namespace mbrwt {

namespace {

enum : uint32_t { kStatRange = 1, kStatOrder = 2 };

__global__ __launch_bounds__(256) void k_cols_compose(const uint32_t *__restrict__ ids,
                                                      const uint32_t *__restrict__ soff,
                                                      const ColsWork *__restrict__ work, uint32_t nr, uint64_t *pairs,
                                                      uint32_t *hist, uint32_t *status) {
    const ColsWork w = gld(work + blockIdx.x);
    const uint32_t s0 = gld(soff + w.key), s1 = gld(soff + w.key + 1);
    const uint32_t end = min(s1, w.begin + kColsChunk);  // (positions < 2^31: no wrap)
    uint32_t bad = 0;
    for (uint32_t i = w.begin + threadIdx.x; i < end; i += 256) {
        const uint32_t id = gld(ids + i);
        if (id >= nr) bad |= kStatRange;
        else atomicAdd(hist + id, 1u);
        if (i > s0 && gld(ids + i - 1) >= id) bad |= kStatOrder;
        gst(pairs + i, (uint64_t)id << 16 | w.key);
    }
    if (bad) atomicOr(status, bad);
}

// keys[i] = the key of sorted pair i; status[1] = the longest of the nr rows
__global__ __launch_bounds__(256) void k_cols_rows(const uint64_t *__restrict__ sorted, uint64_t n, uint16_t *keys,
                                                   const uint32_t *__restrict__ off, uint64_t nr, uint32_t *status) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = t; i < n; i += gs) gst(keys + i, (uint16_t)gld(sorted + i));
    uint32_t longest = 0;
    for (uint64_t r = t; r < nr; r += gs) longest = max(longest, gld(off + r + 1) - gld(off + r));
    for (int d = 32; d; d >>= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, d));
    if ((threadIdx.x & 63) == 0 && longest) atomicMax(status + 1, longest);
}

}  // namespace

int cols_from_load(RowsFrom *rf, const ColsView &v, const std::vector<uint64_t> &cur,
                   const std::vector<uint64_t> &ends, uint64_t a, uint64_t b, LabelRows *rows, uint64_t *labels) {
    const uint64_t nr = b - a;
    uint64_t L = 0;
    for (uint64_t c = 0; c < v.num_columns; ++c) L += ends[c] - cur[c];
    if (L > kColsMaxLabels) {
        set_error("row records from sparse columns: more than 2^31 - 1 labels in one range of rows");
        return MBRWT_ERR_UNSUPPORTED;
    }
    int rc;
    // (an empty range still has non-null buffers)
    if ((rc = ensure(rf->off, (nr + 1) * 4)) || (rc = ensure(rf->cols, L * 4 + 16)) ||
        (rc = ensure(rf->keys, L * 2 + 16)))
        return rc;
    uint32_t *d_off = reinterpret_cast<uint32_t *>(rf->off.buf);
    uint32_t *d_ids = reinterpret_cast<uint32_t *>(rf->cols.buf);
    uint16_t *d_keys = reinterpret_cast<uint16_t *>(rf->keys.buf);
    MBRWT_HIP(hipMemsetAsync(rf->d_status, 0, 8, rf->s));
    MBRWT_HIP(hipMemsetAsync(d_off, 0, (nr + 1) * 4, rf->s));  // the histogram; L == 0: the offsets
    if (L) {
        if (rf->h_ids_cap < L) {
            if (rf->h_ids) (void)hipHostFree(rf->h_ids);
            rf->h_ids = nullptr;
            rf->h_ids_cap = 0;
            MBRWT_HIP(hipHostMalloc(reinterpret_cast<void **>(&rf->h_ids), L * 4, hipHostMallocDefault));
            rf->h_ids_cap = L;
        }
        cols_stage_offsets(rf->perm, cur, ends, rf->h_soff);
        cols_stage(v, rf->perm, cur, rf->h_soff, a, rf->h_ids);
        cols_work_list(rf->h_soff, rf->h_work);
        const size_t W = rf->h_work.size();
        if ((rc = ensure(rf->soff, rf->h_soff.size() * 4)) || (rc = ensure(rf->work, W * sizeof(ColsWork))) ||
            (rc = ensure(rf->pairs, L * 8)) || (rc = ensure(rf->pairs2, L * 8)))
            return rc;
        uint32_t *d_soff = reinterpret_cast<uint32_t *>(rf->soff.buf);
        ColsWork *d_work = reinterpret_cast<ColsWork *>(rf->work.buf);
        uint64_t *d_pairs = reinterpret_cast<uint64_t *>(rf->pairs.buf);
        MBRWT_HIP(hipMemcpyAsync(d_ids, rf->h_ids, L * 4, hipMemcpyHostToDevice, rf->s));
        MBRWT_HIP(hipMemcpyAsync(d_soff, rf->h_soff.data(), rf->h_soff.size() * 4, hipMemcpyHostToDevice, rf->s));
        MBRWT_HIP(hipMemcpyAsync(d_work, rf->h_work.data(), W * sizeof(ColsWork), hipMemcpyHostToDevice, rf->s));
        hipLaunchKernelGGL(k_cols_compose, dim3((unsigned)W), dim3(256), 0, rf->s, d_ids, d_soff, d_work,
                           (uint32_t)nr, d_pairs, d_off, rf->d_status);
        MBRWT_HIP(hipGetLastError());
        const uint64_t *d_sorted = d_pairs;
        size_t tb = 0;
        if (nr > 1) {  // (one row: zero row bits, the composed order stands)
            int end_bit = 16;
            while ((nr - 1) >> (end_bit - 16)) ++end_bit;
            hipcub::DoubleBuffer<uint64_t> db(d_pairs, reinterpret_cast<uint64_t *>(rf->pairs2.buf));
            MBRWT_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, db, (int)L, 16, end_bit, rf->s));
            if ((rc = ensure(rf->sort, tb))) return rc;
            MBRWT_HIP(hipcub::DeviceRadixSort::SortKeys(rf->sort.buf, tb, db, (int)L, 16, end_bit, rf->s));
            d_sorted = db.Current();
        }
        tb = 0;
        MBRWT_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_off, d_off, (int)(nr + 1), rf->s));
        if ((rc = ensure(rf->sort, tb))) return rc;
        MBRWT_HIP(hipcub::DeviceScan::ExclusiveSum(rf->sort.buf, tb, d_off, d_off, (int)(nr + 1), rf->s));
        hipLaunchKernelGGL(k_cols_rows, dim3(grid256(std::max(L, nr))), dim3(256), 0, rf->s, d_sorted, L, d_keys,
                           d_off, nr, rf->d_status);
        MBRWT_HIP(hipGetLastError());
    }
    uint32_t st[2] = {0, 0};
    MBRWT_HIP(hipMemcpyAsync(st, rf->d_status, 8, hipMemcpyDeviceToHost, rf->s));
    MBRWT_HIP(hipStreamSynchronize(rf->s));
    if (st[0] & kStatRange) {
        set_error("sparse columns: a row id >= num_rows, or a column's row ids not ascending");
        return MBRWT_ERR_INVALID;
    }
    if (st[0] & kStatOrder) {
        set_error("sparse columns: a column's row ids do not ascend strictly");
        return MBRWT_ERR_INVALID;
    }
    if (st[1] > 0x7FFFu) {
        set_error("row record deeper than the build walker supports, or a row of more than 32,767 labels");
        return MBRWT_ERR_UNSUPPORTED;
    }
    *rows = LabelRows{rf->d_shape, d_off, d_keys};
    *labels = L;
    return MBRWT_OK;
}

int cols_from_range(RowsFrom *rf, RowsBuild *rb, const ColsView &v, const std::vector<uint64_t> &cur,
                    const std::vector<uint64_t> &ends, uint64_t a, uint64_t b, uint64_t *labels) {
    Ctx &range = rf->range;
    uint64_t L = 0;
    if (int rc = cols_from_load(rf, v, cur, ends, a, b, &range.label_rows, &L)) return rc;
    range.tree.num_rows = b - a;
    range.tree.num_relations = L;
    if (int rc = rows_build_range(rb, range, a)) return rc;
    *labels += L;
    return MBRWT_OK;
}

}  // namespace mbrwt
