// rows_counts.hip -- PER-NODE ROW COUNTS straight from row-major data
// (mbrwt_rows_node_counts).
//
// cnt(u) = the rows with at least one label below node u of a tree shape is
// all BRWTOptimizer::relax needs of the matrix: a node's index column has
// cnt(parent) bits of which cnt(u) are set.  Per range of rows the labels are
// uploaded, keyed and ordered by rows_from_load (rows_from.hip); then one
// lane per row walks the row over the shape table (rows_emit.hpp
// emit_label_masks) and counts every child its masks name.
//
// The adds are skewed -- every non-empty row reaches the root, most reach the
// top levels -- so they are reduced on chip first: the root by a wave-wide
// ballot, every other node in a table of u32 counters in LDS (one per dnode),
// flushed with one 64-bit global atomic per non-zero counter per workgroup.
// A shape of more than kCountsLdsNodes dnodes adds straight to global memory.
// Integer adds: the result does not depend on their order.
#include <algorithm>

#include "device_access.hpp"
#include "mbrwt_internal.hpp"
#include "rows_emit.hpp"

namespace mbrwt {

namespace {

constexpr uint32_t kCountsLdsNodes = 12288;  // 48 KiB of u32 counters
constexpr unsigned kCountsMaxGrid = 2048;    // workgroups: few flushes, every CU busy

template <bool kLds>
__global__ __launch_bounds__(256) void k_rows_node_counts(LabelRows src, uint64_t nr, uint32_t D,
                                                          unsigned long long *counts) {
    extern __shared__ uint32_t tab[];  // [D] (kLds)
    if (kLds) {
        for (uint32_t i = threadIdx.x; i < D; i += 256) tab[i] = 0;
        __syncthreads();
    }
    uint32_t nonempty = 0;  // lane 0 of every wave: the wave's non-empty rows
    const uint64_t gs = (uint64_t)gridDim.x * 256;
    // (r0 is the same for the whole workgroup: the ballot sees every lane)
    for (uint64_t r0 = (uint64_t)blockIdx.x * 256; r0 < nr; r0 += gs) {
        const uint64_t r = r0 + threadIdx.x;
        bool any = false;
        if (r < nr) {
            any = emit_label_masks(src, (uint32_t)r, [&](uint64_t m, uint32_t, uint32_t v) {
                      const uint32_t fc = gld(src.shape + v).first_child;
                      for (; m; m &= m - 1) {
                          const uint32_t w = fc + (uint32_t)__builtin_ctzll(m);
                          if (kLds) atomicAdd(&tab[w], 1u);
                          else atomicAdd(counts + w, 1ull);
                      }
                  }) != 0;
        }
        nonempty += (uint32_t)__builtin_popcountll(__ballot(any));
    }
    if ((threadIdx.x & 63) == 0 && nonempty) {
        if (kLds) atomicAdd(&tab[1], nonempty);
        else atomicAdd(counts + 1, (unsigned long long)nonempty);
    }
    if (kLds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < D; i += 256)
            if (const uint32_t c = tab[i]) atomicAdd(counts + i, (unsigned long long)c);
    }
}

}  // namespace

int rows_counts_range(const LabelRows &rows, uint64_t num_rows, uint32_t num_dnodes, unsigned long long *d_counts,
                      hipStream_t s) {
    if (!num_rows) return MBRWT_OK;
    // (a workgroup's u32 counters: it sees fewer than 2^32 rows, as a range has)
    const unsigned grid = std::min(grid256(num_rows), kCountsMaxGrid);
    if (num_dnodes <= kCountsLdsNodes)
        hipLaunchKernelGGL(k_rows_node_counts<true>, dim3(grid), dim3(256), num_dnodes * sizeof(uint32_t), s, rows,
                           num_rows, num_dnodes, d_counts);
    else
        hipLaunchKernelGGL(k_rows_node_counts<false>, dim3(grid), dim3(256), 0, s, rows, num_rows, num_dnodes,
                           d_counts);
    MBRWT_HIP(hipGetLastError());
    return MBRWT_OK;
}

}  // namespace mbrwt
