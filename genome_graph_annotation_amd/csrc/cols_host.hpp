// cols_host.hpp -- the HOST side of the build from sparse columns
// (mbrwt_create_from_sparse_columns, rows_from_cols.hip):
// the slice cutter, the range sizing, the staging and the sample
// intersection.  Plain C++: nothing of HIP is included, so a stand-alone
// program tests it (tests/cpp/from_sparse_columns/cols_host.cpp).
//
// The matrix comes column-major: per column the ascending ids of its set rows
// (u64, or u32 where num_rows <= 2^32).  A range [a, b) of rows takes of every
// column the SLICE of ids in [a, b): one cursor per column walks the ranges, a
// binary search from the cursor finds the slice's end, and the last range
// ends every slice at the column's end -- so consecutive ranges' slices tile
// each column whatever the ids are, and "every staged id lies in its range
// and every slice ascends strictly" (checked on the device) is the whole
// input's validity.
#pragma once

#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

namespace mbrwt {

struct ColsView {
    uint64_t num_rows = 0, num_columns = 0;
    const uint64_t *offsets = nullptr;  // num_columns + 1
    const uint64_t *rows = nullptr;     // exactly one of rows / rows32
    const uint32_t *rows32 = nullptr;
    uint64_t id(uint64_t p) const { return rows ? rows[p] : rows32[p]; }
};

constexpr uint64_t kColsMaxLabels = 0x7FFFFFFFull;  // labels of one range (the device sort counts its items in an int)
constexpr uint32_t kColsBadRow = 0xFFFFFFFFu;       // a staged id outside [a, a + 2^32 - 1): never < the range's rows
constexpr uint32_t kColsChunk = 2048;               // staged ids per workgroup of k_cols_compose
constexpr unsigned kColsMaxThreads = 16;

// one workgroup's part of a staged slice: the ids [begin, begin + kColsChunk)
// of the slice of pre-order index `key`, cut at the slice's end
struct ColsWork {
    uint32_t key, begin;
};

// the first position of [lo, hi) whose id is >= x (none: hi).  A plain
// bisection: on ids that do not ascend it still returns a position of [lo, hi]
inline uint64_t cols_lower_bound(const ColsView &v, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v.id(mid) < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the slices of the rows [.., e) from the cursors on: ends[c] (ends may be
// null), and their labels.  e >= num_rows ends every slice at its column's end
inline uint64_t cols_cut_slices(const ColsView &v, const std::vector<uint64_t> &cur, uint64_t e,
                                std::vector<uint64_t> *ends) {
    uint64_t labels = 0;
    if (ends) ends->resize(v.num_columns);
    for (uint64_t c = 0; c < v.num_columns; ++c) {
        const uint64_t hi = v.offsets[c + 1];
        const uint64_t end = e >= v.num_rows ? hi : cols_lower_bound(v, cur[c], hi, e);
        labels += end - cur[c];
        if (ends) (*ends)[c] = end;
    }
    return labels;
}

// device bytes one range of `rows` rows and `labels` labels over m columns
// takes beside the records -- what rows_from_cols.hip allocates: the staged
// ids (u32), two buffers of pairs (u64), the keys (u16), the row offsets
// (u32), the slice offsets and the work list, the sort's and the scan's
// scratch (the look-back states: under 2 bytes per label)
inline uint64_t cols_range_bytes(uint64_t rows, uint64_t labels, uint64_t m) {
    const uint64_t work = labels / kColsChunk + m;
    return 4 * (rows + 1) + (4 + 16 + 2 + 2) * labels + 4 * (m + 1) + sizeof(ColsWork) * work + (4ull << 20);
}

// the largest range [a, a + k align), k align <= R, of n rows that `fits`
// (fits(e): the rows [a, e)); one multiple of align is taken whatever it costs
template <class Fits>
inline uint64_t cut_range_fit(uint64_t n, uint64_t a, uint64_t R, uint64_t align, Fits fits) {
    const uint64_t b = std::min(n, a + R);
    if (fits(b)) return b;
    uint64_t lo = 1, hi = (b - a + align - 1) / align;
    while (lo + 1 < hi) {
        const uint64_t mid = (lo + hi) / 2;
        (fits(a + mid * align) ? lo : hi) = mid;
    }
    return std::min(n, a + lo * align);
}

// RowsSource::cut (capi.cpp) for column-major data: labels(e) = the labels of the rows
// [a, e), from the per-column cursors; `budget` = the device bytes a range
// may take (capi.cpp: free less the reserve and the pending records, over
// 1.2); a fixed range size (MBRWT_BUILD_ROWS_RANGE) is taken as it is
template <class Labels>
inline uint64_t cut_cols_range(uint64_t n, uint64_t m, uint64_t a, uint64_t R, uint64_t align, bool fixed,
                               double budget, Labels labels) {
    if (fixed) return std::min(n, a + R);
    return cut_range_fit(n, a, R, align, [&](uint64_t e) {
        const uint64_t L = labels(e);
        return L <= kColsMaxLabels && (double)cols_range_bytes(e - a, L, m) <= budget;
    });
}

// a row id as a local row of the range starting at a
inline uint32_t cols_local_row(uint64_t id, uint64_t a) {
    return id < a || id - a >= kColsBadRow ? kColsBadRow : (uint32_t)(id - a);
}

// fn(t) for t in [0, threads) on that many host threads (the caller's included)
template <class Fn>
inline void cols_parallel(unsigned threads, Fn fn) {
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < threads; ++t) pool.emplace_back([&fn, t] { fn(t); });
    fn(0);
    for (std::thread &th : pool) th.join();
}
// host threads for `items` units of work: one per 2^20, at most 16
inline unsigned cols_threads(uint64_t items) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    return (unsigned)std::min<uint64_t>(std::min(hw, kColsMaxThreads), items / (1u << 20) + 1);
}

// The staged order: slice k is column perm[k]'s (perm: pre-order leaf index ->
// column), so the staged labels ascend in key and a stable sort by row leaves
// every row's keys ascending.  soff[k] = the staged position of slice k
// (m + 1 entries, the caller has checked the total against kColsMaxLabels)
inline void cols_stage_offsets(const std::vector<uint32_t> &perm, const std::vector<uint64_t> &cur,
                               const std::vector<uint64_t> &ends, std::vector<uint32_t> &soff) {
    const size_t m = perm.size();
    soff.resize(m + 1);
    uint64_t at = 0;
    for (size_t k = 0; k < m; ++k) {
        soff[k] = (uint32_t)at;
        at += ends[perm[k]] - cur[perm[k]];
    }
    soff[m] = (uint32_t)at;
}

// the staged positions [p0, p1): local rows (id - a) into out
inline void cols_stage_part(const ColsView &v, const std::vector<uint32_t> &perm, const std::vector<uint64_t> &cur,
                            const std::vector<uint32_t> &soff, uint64_t a, uint32_t p0, uint32_t p1, uint32_t *out) {
    size_t k = std::upper_bound(soff.begin(), soff.end(), p0) - soff.begin() - 1;
    for (uint32_t p = p0; p < p1; ++k) {
        const uint32_t stop = std::min(p1, soff[k + 1]);
        const uint64_t src = cur[perm[k]] + (p - soff[k]);
        if (v.rows32 && a == 0) {
            std::copy(v.rows32 + src, v.rows32 + src + (stop - p), out + p);
        } else {
            for (uint32_t i = 0; i < stop - p; ++i) out[p + i] = cols_local_row(v.id(src + i), a);
        }
        p = stop;
    }
}

// every slice staged, the positions split evenly over the host threads
inline void cols_stage(const ColsView &v, const std::vector<uint32_t> &perm, const std::vector<uint64_t> &cur,
                       const std::vector<uint32_t> &soff, uint64_t a, uint32_t *out) {
    const uint64_t L = soff.back();
    const unsigned T = cols_threads(L);
    cols_parallel(T, [&](unsigned t) {
        cols_stage_part(v, perm, cur, soff, a, (uint32_t)(L * t / T), (uint32_t)(L * (t + 1) / T), out);
    });
}

// the work list of k_cols_compose: per slice its chunks of kColsChunk ids
inline void cols_work_list(const std::vector<uint32_t> &soff, std::vector<ColsWork> &work) {
    work.clear();
    for (uint32_t k = 0; k + 1 < soff.size(); ++k)
        for (uint64_t p = soff[k]; p < soff[k + 1]; p += kColsChunk) work.push_back(ColsWork{k, (uint32_t)p});
}

// The greedy partitioner's sample of column c: the slots k (ascending) with
// sample[k] among the column's ids, appended to out.  sample == null: every
// row is its own slot (num_rows <= 10^6) and every id is checked -- false for
// an id >= num_rows or ids that do not ascend strictly.  With a sample, the
// shorter list is searched for in the longer, or both are merged.
inline bool cols_sample_slots(const ColsView &v, uint64_t c, const std::vector<uint64_t> *sample,
                              std::vector<uint32_t> &out) {
    const uint64_t lo = v.offsets[c], hi = v.offsets[c + 1];
    if (!sample) {
        for (uint64_t p = lo; p < hi; ++p) {
            const uint64_t id = v.id(p);
            if (id >= v.num_rows || (p > lo && v.id(p - 1) >= id)) return false;
            out.push_back((uint32_t)id);
        }
        return true;
    }
    const std::vector<uint64_t> &s = *sample;
    const uint64_t len = hi - lo, ns = s.size();
    if (len * 16 < ns) {  // few ids: each looked up in the sample
        for (uint64_t p = lo; p < hi; ++p) {
            const uint64_t id = v.id(p);
            const auto it = std::lower_bound(s.begin(), s.end(), id);
            if (it != s.end() && *it == id) out.push_back((uint32_t)(it - s.begin()));
        }
    } else if (ns * 16 < len) {  // a long column: each sampled row looked up in it, from the last hit on
        uint64_t p = lo;
        for (uint64_t k = 0; k < ns && p < hi; ++k) {
            p = cols_lower_bound(v, p, hi, s[k]);
            if (p < hi && v.id(p) == s[k]) out.push_back((uint32_t)k);
        }
    } else {
        uint64_t p = lo, k = 0;
        while (p < hi && k < ns) {
            const uint64_t id = v.id(p);
            if (id < s[k]) ++p;
            else if (id > s[k]) ++k;
            else {
                out.push_back((uint32_t)k);
                ++p;
                ++k;
            }
        }
    }
    return true;
}

}  // namespace mbrwt
