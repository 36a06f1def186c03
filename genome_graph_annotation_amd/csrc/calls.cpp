// calls.cpp -- the call plumbing every get_rows driver and point query shares
// (host only): workspace growth, the resident-workgroup count of a kernel,
// the timing events, and the end of a synchronous call -- the status block
// copied to the host, the stream synchronised, the status mapped to a return
// code and message.  Three status protocols end here: the row-record block
// {total, status}, the node-image block {total, overflow rows, error bits},
// and the point queries' counters ([2] error bits, [3] visits, [4] labels).
#include <algorithm>

#include "mbrwt_internal.hpp"

namespace mbrwt {

int ensure(Workspace &w, size_t bytes) {
    if (w.bytes >= bytes) return MBRWT_OK;
    if (w.buf) MBRWT_HIP(hipFree(w.buf));
    w.buf = nullptr;
    w.bytes = 0;
    size_t b = std::max<size_t>(bytes, 256);
    MBRWT_HIP(hipMalloc(&w.buf, b));
    w.bytes = b;
    return MBRWT_OK;
}

int resident_workgroups(Ctx &c, const void *fn, uint32_t threads, size_t lds, int occ_cap, uint64_t *blocks) {
    if (c.rb_fn != fn || c.rb_lds != lds || c.rb_threads != threads || c.rb_cap != occ_cap) {
        if (lds > 65536) MBRWT_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int dev_cus = 0, per_cu = 0;
        (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, c.device);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess || per_cu <= 0)
            per_cu = 1;
        if (occ_cap) per_cu = std::min(per_cu, occ_cap);
        c.rb_fn = fn;
        c.rb_lds = lds;
        c.rb_threads = threads;
        c.rb_cap = occ_cap;
        c.rb_blocks = std::max(1, dev_cus) * per_cu;
    }
    *blocks = (uint64_t)c.rb_blocks;
    return MBRWT_OK;
}

int timing_events(Ctx &c, bool async, hipEvent_t *e0, hipEvent_t *e1) {
    *e0 = c.ev0;
    *e1 = c.ev1;
    if (!c.timing || !async) return MBRWT_OK;
    if (c.async_ev.size() <= c.async_used) {
        hipEvent_t ea = nullptr, eb = nullptr;
        MBRWT_HIP(hipEventCreate(&ea));
        MBRWT_HIP(hipEventCreate(&eb));
        c.async_ev.push_back({ea, eb});
    }
    *e0 = c.async_ev[c.async_used].first;
    *e1 = c.async_ev[c.async_used].second;
    ++c.async_used;
    return MBRWT_OK;
}

// a synchronous call's status block on the host (`words` of d_scalars), and
// its kernel time between ev0 and ev1 into the context's timing
static int sync_status(Ctx &c, size_t words, hipStream_t s) {
    MBRWT_HIP(hipMemcpyAsync(c.h_scalars, c.d_scalars, words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    MBRWT_HIP(hipStreamSynchronize(s));
    if (c.timing) {
        float ms = 0;
        MBRWT_HIP(hipEventElapsedTime(&ms, c.ev0, c.ev1));
        c.timing_ms += ms;
        c.timing_launches += 1;
    }
    return MBRWT_OK;
}

int finish_rows_call(Ctx &c, uint64_t *needed, const char *fallback, hipStream_t s) {
    if (const int rc = sync_status(c, 2, s)) return rc;
    if (needed) *needed = c.h_scalars[0];
    switch (c.h_scalars[1]) {
        case MBRWT_OK: return MBRWT_OK;
        case MBRWT_ERR_RANGE: set_error("row out of range"); return MBRWT_ERR_RANGE;
        case MBRWT_ERR_CAPACITY: set_error("cols_cap too small"); return MBRWT_ERR_CAPACITY;
        default: set_error(fallback); return MBRWT_ERR_DEVICE;
    }
}

int node_error_code(uint64_t bits, const char **msg) {
    if (bits & 1) {
        if (msg) *msg = "row out of range";
        return MBRWT_ERR_RANGE;
    }
    if (bits & 2) {
        if (msg) *msg = "traversal stack overflow";
        return MBRWT_ERR_UNSUPPORTED;
    }
    return MBRWT_OK;
}

// a point query's counters: the launch check, d_scalars to the host, the
// stream synchronised, the bits of `error_mask` in [2] mapped to a return code
static int finish_point_call(Ctx &c, hipStream_t s, uint64_t error_mask, uint64_t *visits, uint64_t *labels) {
    MBRWT_HIP(hipGetLastError());
    MBRWT_HIP(hipMemcpyAsync(c.h_scalars, c.d_scalars, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    MBRWT_HIP(hipStreamSynchronize(s));
    if (const int rc = node_error_code(c.h_scalars[2] & error_mask)) return rc;
    if (visits) *visits = c.h_scalars[3];
    if (labels) *labels = c.h_scalars[4];
    return MBRWT_OK;
}

int finish_record_call(Ctx &c, hipStream_t s, uint64_t *visits, uint64_t *labels) {
    return finish_point_call(c, s, 1, visits, labels);  // (the record protocol has the range bit only)
}

int finish_node_point_call(Ctx &c, hipStream_t s, uint64_t *visits, uint64_t *labels) {
    return finish_point_call(c, s, 3, visits, labels);
}

int finish_nodes_call(Ctx &c, uint64_t cap, uint64_t *needed, uint64_t *overflow, hipStream_t s) {
    if (const int rc = sync_status(c, 4, s)) return rc;
    const char *msg = nullptr;
    if (const int rc = node_error_code(c.h_scalars[2], &msg)) {
        set_error(msg);
        return rc;
    }
    const uint64_t total = c.h_scalars[0];
    *overflow = c.overflow_rows = c.h_scalars[1];
    if (needed) *needed = total;
    if (total > cap) {
        set_error("cols_cap too small");
        return MBRWT_ERR_CAPACITY;
    }
    return MBRWT_OK;
}

}  // namespace mbrwt
