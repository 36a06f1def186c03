// query.hip -- the router of the row queries (gfx950 / CDNA4).  Every entry
// point sends its call to the row records (rows.hip), the row shards
// (shards.hip) or the per-node images, whose kernels live in the nodes_*.hip
// families (nodes_walk.hpp):
//   run_get_rows      the checks, the routing, and the slot-path driver:
//                     MODE_SLOTS traversal (k_traverse_fast2 where the tree
//                     allows, else the general kernels) into K label slots per
//                     row, an exclusive scan for the CSR offsets, the
//                     compaction, and the direct pass over rows of more than K
//                     labels; rowblock trees go to nodes_rowblock.hip's driver;
//   run_get_rows16    u16 labels: the u32 call, then k_narrow_cols;
//   run_get_batch, run_count_labels, run_count_work
//                     the node-image point queries, ending in
//                     finish_node_point_call (calls.cpp);
//   traverse_kernel_name.
// Also the counts workspace and scan both node drivers use (CountsScan).
#include <hipcub/hipcub.hpp>

#include "nodes_walk.hpp"
#include "wave_scan.hpp"

namespace mbrwt {
using namespace nodes;

namespace nodes {

int counts_scan_prepare(Ctx &c, uint64_t rows, uint64_t groups, uint64_t *row_offsets, hipStream_t s, CountsScan *w) {
    const uint64_t go_off = ((rows + groups + 1) * sizeof(uint32_t) + 7) / 8 * 8;
    if (const int rc = ensure(c.ws_counts, go_off + (groups + 1) * sizeof(uint64_t))) return rc;
    w->counts = reinterpret_cast<uint32_t *>(c.ws_counts.buf);
    w->group_counts = w->counts + rows;
    w->group_offsets = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(c.ws_counts.buf) + go_off);
    w->in = row_offsets ? w->counts : w->group_counts;
    w->out = row_offsets ? row_offsets : w->group_offsets;
    w->len = row_offsets ? rows : groups + 1;
    hipcub::TransformInputIterator<uint64_t, Widen<uint32_t>, const uint32_t *> it(w->in, Widen<uint32_t>());
    MBRWT_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, w->bytes, it, w->out, w->len, s));
    return ensure(c.ws_scan, w->bytes);
}

hipError_t counts_scan_run(const Ctx &c, const CountsScan &w, hipStream_t s) {
    hipcub::TransformInputIterator<uint64_t, Widen<uint32_t>, const uint32_t *> it(w.in, Widen<uint32_t>());
    size_t bytes = w.bytes;
    return hipcub::DeviceScan::ExclusiveSum(c.ws_scan.buf, bytes, it, w.out, w.len, s);
}

}  // namespace nodes

// the MODE_SLOTS traversal of a context without a rowblock kernel
static Trav slots_traverse(const Ctx &c) {
    const Trav t = fast2_traverse(c);
    return t ? t : pick_traverse(c, MODE_SLOTS);
}

const char *traverse_kernel_name(const Ctx &c) {
    if (c.rows.ready && c.kernel_variant == 0) return c.rows.var ? "k_var_decode" : "k_traverse_rows";
    if (c.nodes_freed) return "";
    if (const char *name = rowblock_kernel_name(c)) return name;
    const Trav t = slots_traverse(c);
    return t ? t.name : "";
}

int run_get_rows(Ctx &c, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets, uint32_t *d_cols, uint64_t cap,
                 uint64_t *needed, hipStream_t s) {
    if (c.rows.ready && c.kernel_variant == 0) return rows_get_rows(c, d_rows, n, d_offsets, d_cols, cap, needed, s);
    if (c.nodes_freed) {
        set_error("kernel variant needs the node image (layout rows)");
        return MBRWT_ERR_UNSUPPORTED;
    }
    c.rows_sc_dirty = true;  // the node kernels reuse ws_counts
    if (!c.shards.empty()) return sharded_get_rows(c, d_rows, n, d_offsets, d_cols, cap, needed, s);
    if (n == 0) {
        MBRWT_HIP(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), s));
        MBRWT_HIP(hipStreamSynchronize(s));
        if (needed) *needed = 0;
        return MBRWT_OK;
    }
    if (c.tree.nodes.empty()) {  // BRWT(): every row is out of range
        set_error("query on an empty BRWT");
        return MBRWT_ERR_RANGE;
    }
    if (n > 0x7FFFFFF0ull) {  // u32 slot arithmetic in the kernels
        set_error("batch larger than 2^31 rows");
        return MBRWT_ERR_UNSUPPORTED;
    }
    int rc;
    bool taken = false;
    rc = run_get_rows_p2w(c, d_rows, n, d_offsets, d_cols, cap, needed, s, &taken);
    if (taken) return rc;
    const uint32_t K = auto_slots(c);
    const Trav fn = slots_traverse(c);
    const Trav fn_direct = pick_traverse(c, MODE_DIRECT);
    if (!fn || !fn_direct) {
        set_error("tree deeper than 32 levels of internal nodes");
        return MBRWT_ERR_UNSUPPORTED;
    }
    const uint64_t nch = (n + 7) / 8;
    if ((rc = ensure(c.ws_temp, n * K * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c.ws_ovf, n * sizeof(uint32_t)))) return rc;
    // n+1 row counts, nch+1 chunk counts; the scan runs over the row counts
    // (general kernels) or the chunk counts (fast2)
    CountsScan w;
    if ((rc = counts_scan_prepare(c, n + 1, nch, fn.fast ? nullptr : d_offsets, s, &w))) return rc;

    TravParams p = base_params(c);
    p.rows = d_rows;
    p.n = n;
    p.K = K;
    p.temp = reinterpret_cast<uint32_t *>(c.ws_temp.buf);
    p.counts = w.counts;
    p.chunk_counts = w.group_counts;
    p.ovf_list = reinterpret_cast<uint32_t *>(c.ws_ovf.buf);

    MBRWT_HIP(hipMemsetAsync(c.d_scalars, 0, 8 * sizeof(uint64_t), s));
    MBRWT_HIP(hipMemsetAsync(w.in + w.len - 1, 0, sizeof(uint32_t), s));
    if (c.timing) MBRWT_HIP(hipEventRecord(c.ev0, s));
    MBRWT_HIP(launch(c, fn, n, s, p));
    if (c.timing) MBRWT_HIP(hipEventRecord(c.ev1, s));
    MBRWT_HIP(counts_scan_run(c, w, s));
    MBRWT_HIP(hipMemcpyAsync(c.d_scalars, w.out + w.len - 1, sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    uint64_t ovf = 0;
    if ((rc = finish_nodes_call(c, cap, needed, &ovf, s))) return rc;
    if (fn.fast) MBRWT_HIP(compact_chunks(c, w.counts, w.group_offsets, p.temp, K, d_offsets, d_cols, n, s));
    else MBRWT_HIP(compact_slots(c, d_offsets, p.temp, K, d_cols, n, s));
    if (ovf) MBRWT_HIP(direct_pass(c, fn_direct, d_rows, p.ovf_list, ovf, d_offsets, d_cols, s));
    return MBRWT_OK;
}

// u16 labels ------------------------------------------------------------
namespace {
// (n <= cap: checked by the caller, so no element at or past cap is written)
__global__ __launch_bounds__(256) void k_narrow_cols(const uint32_t *src, uint16_t *dst, uint64_t n) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs)
        gst(dst + i, (uint16_t)gld(src + i));
}
}  // namespace

bool rows16_supported(const Ctx &c) {
    if (c.tree.num_columns <= 0x10000u) return true;
    set_error("u16 labels need a context of at most 65536 columns (this one has " +
              std::to_string(c.tree.num_columns) + ")");
    return false;
}

// Row records store u16 themselves (k_compact_tiles / k_var_decode).  Every
// other image (node layouts, row shards, a forced kernel variant) answers
// through its u32 path into ws_cols16 -- grown from the call's own total, as
// classify_batch grows its CSR, never sized by the caller's capacity -- and
// one narrowing pass into the caller's buffer: the u32 call's time plus 6
// bytes of traffic per label.
int run_get_rows16(Ctx &c, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets, uint16_t *d_cols, uint64_t cap,
                   uint64_t *needed, hipStream_t s) {
    if (c.rows.ready && c.kernel_variant == 0)
        return rows_get_rows(c, d_rows, n, d_offsets, d_cols, cap, needed, s, nullptr, 2);
    uint64_t need = 0;
    int rc;
    if (!d_cols || !cap) {  // count only
        rc = run_get_rows(c, d_rows, n, d_offsets, nullptr, 0, &need, s);
    } else {
        rc = run_get_rows(c, d_rows, n, d_offsets, reinterpret_cast<uint32_t *>(c.ws_cols16.buf),
                          c.ws_cols16.bytes / sizeof(uint32_t), &need, s);
        if (rc == MBRWT_ERR_CAPACITY && need <= cap) {
            if ((rc = ensure(c.ws_cols16, (need + need / 8 + 1024) * sizeof(uint32_t)))) return rc;
            rc = run_get_rows(c, d_rows, n, d_offsets, reinterpret_cast<uint32_t *>(c.ws_cols16.buf),
                              c.ws_cols16.bytes / sizeof(uint32_t), &need, s);
        }
    }
    if (needed) *needed = need;
    if (rc) return rc;
    if (need > cap) {  // (the workspace held what the caller's buffer does not)
        set_error("cols_cap too small");
        return MBRWT_ERR_CAPACITY;
    }
    if (need) {
        hipLaunchKernelGGL(k_narrow_cols, dim3(grid256(need)), dim3(256), 0, s,
                           reinterpret_cast<const uint32_t *>(c.ws_cols16.buf), d_cols, need);
        MBRWT_HIP(hipGetLastError());
    }
    return MBRWT_OK;
}

// the node-image point queries: a general traversal of `mode` over the n rows
// (none for n == 0), then the call's counters
static int run_point_traversal(Ctx &c, int mode, const uint64_t *d_rows, uint64_t n, uint64_t *d_counts,
                               uint64_t *visits, uint64_t *labels, hipStream_t s) {
    const Trav fn = pick_traverse(c, mode);
    if (!fn) return MBRWT_ERR_UNSUPPORTED;
    TravParams p = base_params(c);
    p.rows = d_rows;
    p.n = n;
    p.label_counts = reinterpret_cast<unsigned long long *>(d_counts);
    MBRWT_HIP(hipMemsetAsync(c.d_scalars, 0, 8 * sizeof(uint64_t), s));
    if (n) MBRWT_HIP(launch(c, fn, n, s, p));
    return finish_node_point_call(c, s, visits, labels);
}

int run_count_work(Ctx &c, const uint64_t *d_rows, uint64_t n, uint64_t *visits, uint64_t *labels, hipStream_t s) {
    if (c.nodes_freed) return rows_count_work(c, d_rows, n, visits, labels, s);
    if (!c.shards.empty()) return sharded_count_work(c, d_rows, n, visits, labels, s);
    if (c.tree.nodes.empty()) return n ? MBRWT_ERR_RANGE : MBRWT_OK;
    return run_point_traversal(c, MODE_WORK, d_rows, n, nullptr, visits, labels, s);
}

int run_count_labels(Ctx &c, const uint64_t *d_rows, uint64_t n, uint64_t *d_counts, hipStream_t s) {
    if (c.rows.ready) return rows_count_labels(c, d_rows, n, d_counts, s);
    if (!c.shards.empty()) return sharded_count_labels(c, d_rows, n, d_counts, s);
    if (c.tree.num_columns) MBRWT_HIP(hipMemsetAsync(d_counts, 0, c.tree.num_columns * sizeof(uint64_t), s));
    if (c.tree.nodes.empty()) return n ? MBRWT_ERR_RANGE : MBRWT_OK;
    return run_point_traversal(c, MODE_COUNT, d_rows, n, d_counts, nullptr, nullptr, s);
}

int run_get_batch(Ctx &c, const uint64_t *d_rows, const uint64_t *d_cols, uint64_t n, uint8_t *d_out, hipStream_t s) {
    if (c.nodes_freed) return rows_get_batch(c, d_rows, d_cols, n, d_out, s);
    if (!c.shards.empty()) return sharded_get_batch(c, d_rows, d_cols, n, d_out, s);
    if (n == 0) return MBRWT_OK;
    if (c.tree.nodes.empty()) return MBRWT_ERR_RANGE;
    MBRWT_HIP(hipMemsetAsync(c.d_scalars, 0, 8 * sizeof(uint64_t), s));
    MBRWT_HIP(launch_get(c, d_rows, d_cols, n, d_out, s));
    return finish_node_point_call(c, s);  // (k_get raises the range bit only)
}

}  // namespace mbrwt
