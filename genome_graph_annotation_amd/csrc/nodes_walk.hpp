// nodes_walk.hpp -- what the node-image kernel families share, and the small
// host interface each family shows the others.
//
// The per-node images (the NODES layout) answer get_rows through one of three
// kernel families, each in its own translation unit:
//   nodes_traverse.hip  k_traverse / k_traverse_group in the four modes below,
//                       k_compact, k_get -- the general kernels;
//   nodes_fast2.hip     k_traverse_fast2 + k_compact_chunks -- basic trees of
//                       arity <= 8;
//   nodes_rowblock.hip  k_traverse_p2w / k_traverse_ptw + k_compact_blocks and
//                       their driver -- 16-row rowblocks over a P2W / PTW table.
// query.hip routes a call to row records, row shards or one of these, and
// drives the slot path (nodes_traverse.hip, nodes_fast2.hip) itself.
#pragma once

#include <algorithm>

#include "device_access.hpp"
#include "mbrwt_internal.hpp"

namespace mbrwt {

// ---- device side: shared by more than one family ---------------------------

enum { MODE_SLOTS = 0, MODE_DIRECT = 1, MODE_WORK = 2, MODE_COUNT = 3 };

struct TravParams {
    const DevNode *nodes;
    const uint64_t *rows;
    uint64_t n;                  // number of slots processed by this launch
    uint64_t num_rows;
    const uint32_t *slot_list;   // MODE_DIRECT: batch indices of the slots
    const uint32_t *order;       // optional: slot s processes batch index order[s]
    uint32_t K;
    uint32_t *temp;              // MODE_SLOTS: [n_batch][K]
    uint32_t *counts;            // MODE_SLOTS: [n_batch]
    uint32_t *chunk_counts;      // k_traverse_fast2: labels per 8-row chunk [n_batch / 8]
    uint32_t *ovf_list;          // MODE_SLOTS
    unsigned long long *scalars; // [0] total, [1] overflow count, [2] error flags, [3] visits, [4] labels
    const uint64_t *offsets;     // MODE_DIRECT
    uint32_t *cols;              // MODE_DIRECT
    unsigned long long *label_counts;  // MODE_COUNT: [num_columns]
    const CNode *cnodes;         // compact node records (group kernel)
    uint32_t n_lds;              // records [0, n_lds) are staged in LDS
    uint32_t folded;             // root folded into the super-root (V accounting)
    const uint32_t *label_map;   // pre-order index -> global column (Tree::label_perm; null = identity)
};

// The compaction kernels stage the label map in LDS when it is small (one
// random 4-byte global read per label measured 2.3 ms per 8 M labels on a
// greedy tree): `lds_entries` > 0 = the first kernel arguments' map copied
// into the dynamic LDS of the workgroup.
constexpr uint32_t kMapLdsMax = 16384;  // entries (64 KiB)
struct LabelMap {
    const uint32_t *g;
    const AS_LDS uint32_t *l;
    __device__ __forceinline__ uint32_t operator()(uint32_t x) const { return l ? l[x] : g ? gld(g + x) : x; }
};
__device__ __forceinline__ LabelMap stage_label_map(const uint32_t *map, uint32_t lds_entries) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_label_map[];
    if (!map || !lds_entries) return LabelMap{map, nullptr};
    for (uint32_t i = threadIdx.x; i < lds_entries; i += blockDim.x) lds_label_map[i] = gld(map + i);
    __syncthreads();
    return LabelMap{map, (const AS_LDS uint32_t *)lds_label_map};
}

// labels of a row staged in LDS by the group kernels (k_traverse_group, k_traverse_fast2)
constexpr uint32_t kStageLabels = 32;

// Reductions over the 4 lanes of a group (lanes 4i..4i+3 = one DPP quad):
// quad_perm DPP moves, no LDS round trip.  All 4 lanes must be active.
__device__ __forceinline__ uint32_t quad_or(uint32_t v) {
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);  // quad_perm(1,0,3,2)
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);  // quad_perm(2,3,0,1)
    return v;
}
// exclusive prefix sum of v over the quad (lane order); `total` = quad sum
__device__ __forceinline__ uint32_t quad_exclusive_sum(uint32_t v, uint32_t c, uint32_t &total) {
    uint32_t incl = v;
    uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x90, 0xF, 0xF, false);  // quad_perm(0,0,1,2)
    incl += c >= 1 ? y : 0u;
    y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x40, 0xF, 0xF, false);  // quad_perm(0,0,0,1)
    incl += c >= 2 ? y : 0u;
    total = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0xFF, 0xF, 0xF, false);  // quad_perm(3,3,3,3)
    return incl - v;
}

// ---- host side (namespace nodes: the families' interface is not the library's) ----
namespace nodes {

using TravFn = void (*)(TravParams);
using GroupFn = void (*)(TravParams, uint32_t);

// A traversal launch: the lane-per-row kernel or the group kernel.
struct Trav {
    const void *fn = nullptr;
    TravFn lane_fn = nullptr;
    GroupFn group_fn = nullptr;
    uint32_t G = 1;  // lanes per row
    bool fast = false;
    const char *name = "k_traverse_group";
    explicit operator bool() const { return fn != nullptr; }
};

// non-temporal block reads on images larger than 1 GiB (k_traverse_fast2: +2.6 %)
inline bool nt_reads(const Ctx &c) { return c.tree.image_bytes > (1ull << 30); }

// label slots per row of the slot path (a rowblock's temp region: 16 of them)
inline uint32_t auto_slots(const Ctx &c) {
    if (c.slot_labels) return c.slot_labels;
    const double mean = c.tree.num_rows ? (double)c.tree.num_relations / (double)c.tree.num_rows : 0.0;
    uint32_t k = kStageLabels;  // >= the LDS stage of the group kernel
    while (k < 2.0 * mean + 8.0 && k < 1024) k <<= 1;
    return k;
}

// label-map entries the compaction kernels stage in LDS (0: identity or too
// large).  At kMapLdsMax entries k_compact asks for 64 KiB of dynamic LDS
// beside its 2,056 static bytes: gfx950 gives a workgroup up to 160 KiB with
// no function attribute (measured: the launch is accepted and exact,
// tests/test_gpu_node_edges.py test_label_map_limit).
inline uint32_t label_map_lds(const Ctx &c) {
    const size_t m = c.tree.label_perm.size();
    return (c.d_label_map && m <= kMapLdsMax) ? (uint32_t)m : 0u;
}

// nodes_traverse.hip: the general traversal of `mode` for this context (null:
// the tree is deeper than 32 levels of internal nodes); a launch over n slots
// (also of nodes_fast2.hip's Trav); the parameters every launch starts from;
// the slot path's compaction; the direct pass -- the rows ovf_list[0, ovf) of
// the batch re-traversed straight into the CSR (MODE_DIRECT)
Trav pick_traverse(const Ctx &c, int mode);
hipError_t launch(const Ctx &c, const Trav &t, uint64_t n, hipStream_t s, const TravParams &p);
TravParams base_params(const Ctx &c);
hipError_t compact_slots(const Ctx &c, const uint64_t *d_offsets, const uint32_t *temp, uint32_t K, uint32_t *d_cols,
                         uint64_t n, hipStream_t s);
hipError_t direct_pass(const Ctx &c, const Trav &fn_direct, const uint64_t *d_rows, const uint32_t *ovf_list,
                       uint64_t ovf, const uint64_t *d_offsets, uint32_t *d_cols, hipStream_t s);
hipError_t launch_get(const Ctx &c, const uint64_t *d_rows, const uint64_t *d_cols, uint64_t n, uint8_t *d_out,
                      hipStream_t s);  // k_get

// nodes_fast2.hip: k_traverse_fast2 for this context's slot path, or none; its compaction
Trav fast2_traverse(const Ctx &c);
hipError_t compact_chunks(const Ctx &c, const uint32_t *d_counts, const uint64_t *d_chunk_offsets, const uint32_t *temp,
                          uint32_t K, uint64_t *d_offsets, uint32_t *d_cols, uint64_t n, hipStream_t s);

// nodes_rowblock.hip: the rowblock kernel get_rows runs on this context
// ("k_traverse_ptw", "k_traverse_p2w"), or null; its driver -- *taken = the
// context has a rowblock kernel and the call was answered (else nothing is done)
const char *rowblock_kernel_name(const Ctx &c);
int run_get_rows_p2w(Ctx &c, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets, uint32_t *d_cols, uint64_t cap,
                     uint64_t *needed, hipStream_t s, bool *taken);

// query.hip: the counts workspace of both node drivers -- `rows` row counts |
// groups + 1 group counts (8-row chunks, 16-row rowblocks) | (8-byte aligned)
// groups + 1 group offsets -- and the widened exclusive scan over it: of the
// group counts into the group offsets, or (row_offsets != null) of `rows` row
// counts into row_offsets.  The scan's last input is no count: the driver
// clears it, and the last output is the batch's total.
struct CountsScan {
    uint32_t *counts = nullptr, *group_counts = nullptr;
    uint64_t *group_offsets = nullptr;
    uint32_t *in = nullptr;  // the scan: in[0, len) -> out[0, len)
    uint64_t *out = nullptr;
    uint64_t len = 0;
    size_t bytes = 0;  // of ws_scan
};
int counts_scan_prepare(Ctx &c, uint64_t rows, uint64_t groups, uint64_t *row_offsets, hipStream_t s, CountsScan *w);
hipError_t counts_scan_run(const Ctx &c, const CountsScan &w, hipStream_t s);

}  // namespace nodes
}  // namespace mbrwt
