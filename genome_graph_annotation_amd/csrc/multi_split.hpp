// multi_split.hpp -- how the multi-device classify calls (multi.hip,
// include/mbrwt.h "multi-device") cut a batch of reads among k replicas, as
// pure host code: the validation of the read offsets and the split rule.
// Standard headers only, so the rule is testable without a device
// (tests/cpp/multi/test_multi_split.cpp); multi.hip's k_split_reads runs the
// same split_cut on the device.
//
// Reads, not rows, are cut: replica r gets the whole reads [b_r, b_{r+1}),
// b_0 = 0, b_k = n_reads, and for 0 < r < k
//     b_r = the first read whose starting row offset is >= ceil(r * n_rows / k)
// (n_reads when there is none).  Consequences:
//   - replica r's row count is below n_rows / k + the longest read;
//   - a replica may get no read at all (fewer reads than replicas, one long
//     read), and reads without rows anywhere;
//   - reads without rows at the front of the batch start at offset 0, below
//     every cut's target, and stay on replica 0; those at the back start at
//     n_rows and go to replica k - 1; a batch of empty reads only goes to
//     replica k - 1.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define MBRWT_SPLIT_HD __host__ __device__
#else
#define MBRWT_SPLIT_HD
#endif

namespace mbrwt {

// ceil(r * n_rows / k) for r <= k, without leaving 64 bits
MBRWT_SPLIT_HD inline uint64_t split_target(uint64_t n_rows, uint32_t k, uint32_t r) {
    return r * (n_rows / k) + (r * (n_rows % k) + k - 1) / k;
}

// b_r of the rule above; off(i) = read_offsets[i], i in [0, n_reads].  On
// offsets that do not ascend the result is still within [0, n_reads].
template <class Load>
MBRWT_SPLIT_HD inline uint64_t split_cut(Load off, uint64_t n_reads, uint64_t n_rows, uint32_t k, uint32_t r) {
    if (r == 0) return 0;
    if (r >= k) return n_reads;
    const uint64_t target = split_target(n_rows, k, r);
    uint64_t lo = 0, hi = n_reads;  // the first i in [0, n_reads] with off(i) >= target
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off(mid) < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// n_reads + 1 offsets: the first 0, ascending, the last n_rows (what one
// context's classify kernels check read by read; here over the whole batch,
// before any slice is cut: a descending pair astride a cut would otherwise
// become a negative slice length that no replica sees)
inline bool read_offsets_valid(const uint64_t *off, uint64_t n_reads, uint64_t n_rows) {
    if (off[0] != 0 || off[n_reads] != n_rows) return false;
    for (uint64_t i = 0; i < n_reads; ++i)
        if (off[i] > off[i + 1]) return false;
    return true;
}

// cut[0..k]: the read cuts of valid offsets
inline void split_reads(const uint64_t *off, uint64_t n_reads, uint64_t n_rows, uint32_t k,
                        std::vector<uint64_t> &cut) {
    cut.resize((size_t)k + 1);
    for (uint32_t r = 0; r <= k; ++r)
        cut[r] = split_cut([off](uint64_t i) { return off[i]; }, n_reads, n_rows, k, r);
}

}  // namespace mbrwt
