// rows_columns.hpp -- the two record sweeps of mbrwt_get_columns
// (rows_columns.hip) over any record form.  A record form is
// a RowLabels functor: rl(row, leaf) calls leaf(column) for every label of
// `row` through the form's one-lane walker and returns false on a corrupt
// record.  The kernels are instantiated beside the walker they call
// (rows_columns.hip: block records and record classes; rows_var.hip: the
// variable-length records); the driver only sees the two launchers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>

#include "device_access.hpp"
#include "mbrwt_internal.hpp"

namespace mbrwt {

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;  // slot map: the column is not asked for
// per-slot totals are privatised in LDS (u32 per slot) up to this many slots
constexpr uint32_t kGcLdsSlots = 8192;

struct GcParams {
    const uint32_t *slot_of;     // num_columns entries: column -> slot, or kNoSlot
    uint64_t num_columns;
    uint64_t row0, n;            // the sweep's rows [row0, row0 + n)
    uint32_t *row_cnt;           // count sweep: wanted labels per row (null: not kept)
    unsigned long long *totals;  // count sweep: wanted labels per slot (null: not kept)
    uint32_t lds_slots;          // the slots when the totals are privatised in LDS, else 0
    const uint32_t *row_off;     // emit sweep: exclusive scan of row_cnt (n + 1)
    uint32_t *keys, *vals;       // emit sweep: (slot, row - row0) pairs in row order
    unsigned long long *status;  // [0] bit 0: a record walk failed
};

// count sweep: one lane per row
template <class RowLabels>
__global__ __launch_bounds__(256) void k_gc_count(RowLabels rl, GcParams p) {
    extern __shared__ uint32_t gc_lds[];
    const bool priv = p.lds_slots != 0;
    if (priv) {
        for (uint32_t k = threadIdx.x; k < p.lds_slots; k += blockDim.x) gc_lds[k] = 0;
        __syncthreads();
    }
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += gs) {
        uint32_t cnt = 0;
        bool ok = rl(p.row0 + i, [&](uint32_t col) {
            if (col >= p.num_columns) return;  // (a corrupt table entry: no read past the slot map)
            const uint32_t sl = gld(p.slot_of + col);
            if (sl == kNoSlot) return;
            ++cnt;
            if (priv) atomicAdd(&gc_lds[sl], 1u);
            else if (p.totals) atomicAdd(p.totals + sl, 1ull);
        });
        if (!ok) atomicOr(p.status, 1ull);
        if (p.row_cnt) gst(p.row_cnt + i, cnt);
    }
    if (priv) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < p.lds_slots; k += blockDim.x)
            if (const uint32_t t = gc_lds[k]) atomicAdd(p.totals + k, (unsigned long long)t);
    }
}

// emit sweep: the same walk, writing the row's pairs at its scanned offset
// (never past the row's counted share, whatever the walk yields)
template <class RowLabels>
__global__ __launch_bounds__(256) void k_gc_emit(RowLabels rl, GcParams p) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += gs) {
        uint32_t at = gld(p.row_off + i);
        const uint32_t end = gld(p.row_off + i + 1);
        if (at == end) continue;
        (void)rl(p.row0 + i, [&](uint32_t col) {
            if (col >= p.num_columns) return;
            const uint32_t sl = gld(p.slot_of + col);
            if (sl == kNoSlot || at >= end) return;
            gst(p.keys + at, sl);
            gst(p.vals + at, (uint32_t)i);
            ++at;
        });
    }
}

// the launchers of one record form
struct GcSweeps {
    std::function<void(const GcParams &, hipStream_t)> count, emit;
};
template <class RowLabels>
GcSweeps gc_sweeps(const RowLabels &rl) {
    GcSweeps sw;
    sw.count = [rl](const GcParams &p, hipStream_t s) {
        hipLaunchKernelGGL(k_gc_count<RowLabels>, dim3(grid256(p.n)), dim3(256), (size_t)p.lds_slots * 4, s, rl, p);
    };
    sw.emit = [rl](const GcParams &p, hipStream_t s) {
        hipLaunchKernelGGL(k_gc_emit<RowLabels>, dim3(grid256(p.n)), dim3(256), 0, s, rl, p);
    };
    return sw;
}
// the variable-length records' sweeps (rows_var.hip, beside var_row)
GcSweeps var_gc_sweeps(const Ctx &c);

}  // namespace mbrwt
