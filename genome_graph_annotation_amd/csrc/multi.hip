// multi.hip -- one process, N GPUs: a replica of the tree per device and
// get_rows over a batch cut into N contiguous slices, reassembled into the
// caller's ONE CSR (include/mbrwt.h "multi-device").  The reference's
// `annograph classify` is one process with a ThreadPool (main.cpp:462-497);
// this lets its C++ host drive every GPU of the node through the C ABI.
// What classify calls -- get_labels / get_top_labels over a batch of reads
// (main.cpp:177,193) -- runs end to end on every replica: the batch is cut
// between whole reads (multi_split.hpp), replica r classifies its reads with
// the device kernels of classify.hip, and only the reads' labels cross
// devices (classify_multi below).
//
// Reassembly: the replicas' slice CSRs go straight to their places in the
// caller's output -- host buffers by device-to-host copies at the slice's
// label offset, device buffers (on the first device) by peer copies over
// xGMI -- after one exchange of the slice label counts on the host.  A
// gather into one buffer is exactly a set of peer copies (no collective:
// RCCL has no gatherv and the sizes are host integers already).
#include <algorithm>
#include <cstring>
#include <exception>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "device_access.hpp"
#include "mbrwt_internal.hpp"
#include "multi_split.hpp"

namespace mbrwt {
namespace {

constexpr uint32_t kSplitThreads = 256;

// The device form of multi_split.hpp over read offsets on the first device:
// every adjacent pair of off[0..n_reads] checked grid-stride (out[2k + 2],
// zeroed by the caller, raised on offsets that do not ascend from 0 to
// n_rows), and, by block 0, the k + 1 read cuts (out[0..k], split_cut) with
// their row offsets (out[k + 1 .. 2k + 1]).  n_reads >= 1.
__global__ __launch_bounds__(kSplitThreads) void k_split_reads(const uint64_t *__restrict__ off, uint64_t n_reads,
                                                               uint64_t n_rows, uint32_t k,
                                                               uint64_t *__restrict__ out) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_reads; i += gs) {
        const uint64_t a = gld(off + i), b = gld(off + i + 1);
        bad |= a > b || (i == 0 && a != 0) || (i + 1 == n_reads && b != n_rows);
    }
    if (bad) gst(out + 2 * (uint64_t)k + 2, (uint64_t)1);
    if (blockIdx.x == 0)
        for (uint32_t r = threadIdx.x; r <= k; r += kSplitThreads) {
            const uint64_t b = split_cut([off](uint64_t i) { return gld(off + i); }, n_reads, n_rows, k, r);
            gst(out + r, b);
            gst(out + k + 1 + r, gld(off + b));
        }
}

__global__ __launch_bounds__(256) void k_rebase(uint64_t *off, uint64_t n, uint64_t add) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) gst(off + i, gld(off + i) + add);
}

}  // namespace
}  // namespace mbrwt

using namespace mbrwt;

struct mbrwt_multi {
    std::vector<mbrwt_ctx *> ctx;
    std::vector<int> dev;
    std::vector<hipStream_t> stream;
    std::vector<Workspace> rows, off, cols;  // per replica, on its device
    // classify: a replica's read offsets, then its result (label offsets, labels, counts)
    std::vector<Workspace> roff, loff, labs, cnts;
    Workspace split;  // k_split_reads' output, on the first device
    std::mutex mu;
};

namespace {

void slice(uint64_t n, uint32_t k, uint32_t r, uint64_t &lo, uint64_t &hi) {
    const uint64_t base = n / k, extra = n % k;
    lo = r * base + std::min<uint64_t>(r, extra);
    hi = lo + base + (r < extra ? 1 : 0);
}

void destroy(mbrwt_multi *m) {
    if (!m) return;
    for (size_t r = 0; r < m->ctx.size(); ++r) {
        if (hipSetDevice(m->dev[r]) != hipSuccess) {  // no such device: nothing was created there
            (void)hipGetLastError();                   // (and no sticky error left for the caller)
            continue;
        }
        for (Workspace *w : {&m->rows[r], &m->off[r], &m->cols[r], &m->roff[r], &m->loff[r], &m->labs[r], &m->cnts[r]})
            if (w->buf) (void)hipFree(w->buf);
        if (r == 0 && m->split.buf) (void)hipFree(m->split.buf);
        if (m->stream[r]) (void)hipStreamDestroy(m->stream[r]);
        mbrwt_destroy(m->ctx[r]);
    }
    delete m;
}

// one replica per device entry, built concurrently (one host thread each)
template <class Create>
int create_multi(const int *devices, int n, mbrwt_multi **out, Create &&create) {
    if (!out || !devices || n < 1) {
        set_error("invalid argument");
        return MBRWT_ERR_INVALID;
    }
    *out = nullptr;
    mbrwt_multi *m = new (std::nothrow) mbrwt_multi();
    if (!m) return MBRWT_ERR_NOMEM;
    m->dev.assign(devices, devices + n);
    m->ctx.assign(n, nullptr);
    m->stream.assign(n, nullptr);
    m->rows.resize(n);
    m->off.resize(n);
    m->cols.resize(n);
    m->roff.resize(n);
    m->loff.resize(n);
    m->labs.resize(n);
    m->cnts.resize(n);
    std::vector<int> rc(n, MBRWT_OK);
    std::vector<std::string> err(n);
    {
        std::vector<std::thread> pool;
        try {
            for (int r = 0; r < n; ++r)
                pool.emplace_back([&, r]() {
                    rc[r] = create(m->dev[r], &m->ctx[r]);
                    if (rc[r]) err[r] = mbrwt_last_error_message();
                    else if (hipSetDevice(m->dev[r]) != hipSuccess ||
                             hipStreamCreateWithFlags(&m->stream[r], hipStreamNonBlocking) != hipSuccess)
                        rc[r] = MBRWT_ERR_DEVICE;
                });
        } catch (...) {
            for (auto &t : pool) t.join();
            destroy(m);
            return MBRWT_ERR_NOMEM;
        }
        for (auto &t : pool) t.join();
    }
    for (int r = 0; r < n; ++r)
        if (rc[r]) {
            set_error("replica on device " + std::to_string(m->dev[r]) + ": " + err[r]);
            const int s = rc[r];
            destroy(m);
            return s;
        }
    *out = m;
    return MBRWT_OK;
}

// one(r) for every replica, each on a host thread of its own (replica 0 on
// the caller's); when several fail, the status and message of the lowest
template <class One>
int for_replicas(uint32_t k, One &&one) {
    std::vector<int> rc(k, MBRWT_OK);
    std::vector<std::string> err(k);
    std::vector<std::thread> pool;
    try {
        for (uint32_t r = 1; r < k; ++r)
            pool.emplace_back([&, r]() {
                rc[r] = one(r);
                if (rc[r]) err[r] = mbrwt_last_error_message();
            });
    } catch (...) {
        for (auto &t : pool) t.join();
        set_error("host thread creation failed");
        return MBRWT_ERR_NOMEM;
    }
    rc[0] = one(0);
    if (rc[0]) err[0] = mbrwt_last_error_message();
    for (auto &t : pool) t.join();
    for (uint32_t r = 0; r < k; ++r)
        if (rc[r]) {
            set_error(err[r]);
            return rc[r];
        }
    return MBRWT_OK;
}

// the caller's device buffers are on device 0, ordered on its stream s0: an
// event there for the replica streams to wait on
struct ReadyEvent {
    hipEvent_t ev = nullptr;
    int dev;
    explicit ReadyEvent(int dev0) : dev(dev0) {}
    int record(hipStream_t s0) {
        MBRWT_HIP(hipSetDevice(dev));
        MBRWT_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        MBRWT_HIP(hipEventRecord(ev, s0));
        return MBRWT_OK;
    }
    ~ReadyEvent() {
        if (!ev) return;
        (void)hipSetDevice(dev);
        (void)hipEventDestroy(ev);
    }
};

// the slices on every replica: slice r's CSR in replica r's workspaces, its
// label count in need[r]; MBRWT_ERR_CAPACITY never reaches the caller here
// (the workspaces grow to the slice's size)
int run_slices(mbrwt_multi &m, const uint64_t *rows, bool rows_on_host, uint64_t n, std::vector<uint64_t> &need,
               hipStream_t s0) {
    const uint32_t k = (uint32_t)m.ctx.size();
    need.assign(k, 0);
    ReadyEvent ready_ev(m.dev[0]);
    int rc0;
    if (!rows_on_host && (rc0 = ready_ev.record(s0))) return rc0;
    const hipEvent_t ready = ready_ev.ev;
    auto one = [&](uint32_t r) -> int {
        uint64_t lo, hi;
        slice(n, k, r, lo, hi);
        const uint64_t nr = hi - lo;
        MBRWT_HIP(hipSetDevice(m.dev[r]));
        int st;
        if ((st = ensure(m.rows[r], std::max<uint64_t>(nr, 1) * 8))) return st;
        if ((st = ensure(m.off[r], (nr + 1) * 8))) return st;
        if ((st = ensure(m.cols[r], 1024 * 4))) return st;
        uint64_t *d_rows = reinterpret_cast<uint64_t *>(m.rows[r].buf);
        if (nr) {
            if (rows_on_host) {
                MBRWT_HIP(hipMemcpyAsync(d_rows, rows + lo, nr * 8, hipMemcpyHostToDevice, m.stream[r]));
            } else {
                MBRWT_HIP(hipStreamWaitEvent(m.stream[r], ready, 0));
                MBRWT_HIP(hipMemcpyPeerAsync(d_rows, m.dev[r], rows + lo, m.dev[0], nr * 8, m.stream[r]));
            }
        }
        uint64_t nd = 0;
        st = mbrwt_get_rows_device(m.ctx[r], d_rows, nr, reinterpret_cast<uint64_t *>(m.off[r].buf),
                                   reinterpret_cast<uint32_t *>(m.cols[r].buf), m.cols[r].bytes / 4, &nd, m.stream[r]);
        if (st == MBRWT_ERR_CAPACITY) {  // grow to the slice's size and run again
            if ((st = ensure(m.cols[r], (nd + nd / 8 + 1024) * 4))) return st;
            st = mbrwt_get_rows_device(m.ctx[r], d_rows, nr, reinterpret_cast<uint64_t *>(m.off[r].buf),
                                       reinterpret_cast<uint32_t *>(m.cols[r].buf), m.cols[r].bytes / 4, &nd,
                                       m.stream[r]);
        }
        need[r] = nd;
        return st;
    };
    return for_replicas(k, one);
}

// ---- classify: get_labels / get_top_labels over a batch of reads -----------
// One driver for both calls and both buffer forms (the four entry points
// below).  The reads are cut among the replicas (multi_split.hpp); replica r
//   1. takes its row slice and its read offsets (host-to-device copies, or
//      peer copies once the caller's stream has reached the call), rebased
//      to start at 0,
//   2. runs its context's mbrwt_get[_top]_labels_batch_device into its own
//      result workspaces, grown once on MBRWT_ERR_CAPACITY,
// and, after the host has summed the replicas' label counts and checked the
// caller's capacity,
//   3. sends its label offsets, rebased by the counts before it, and its
//      labels (and counts) to their places in the caller's buffers.
// What crosses devices is the rows in and each read's labels out; the rows'
// own labels (the get_rows CSR, ~40 B per row) never leave the replica.
struct ClassifyCall {
    bool top;      // get_top_labels: counts beside the labels
    double ratio;  // get_labels
    uint64_t num_top;
    int run(mbrwt_ctx *c, const uint64_t *d_rows, uint64_t n_rows, const uint64_t *d_roff, uint64_t n_reads,
            uint64_t *d_loff, uint32_t *d_labs, uint64_t *d_cnts, uint64_t cap, uint64_t *need, hipStream_t s) const {
        return top ? mbrwt_get_top_labels_batch_device(c, d_rows, n_rows, d_roff, n_reads, num_top, d_loff, d_labs,
                                                       d_cnts, cap, need, s)
                   : mbrwt_get_labels_batch_device(c, d_rows, n_rows, d_roff, n_reads, ratio, d_loff, d_labs, cap,
                                                   need, s);
    }
};

void launch_rebase(uint64_t *off, uint64_t n, uint64_t add, hipStream_t s) {
    const uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_rebase, dim3((unsigned)g), dim3(256), 0, s, off, n, add);
}

// cut[0..k] and the row offsets there, of device offsets on the first device
// (k_split_reads; one small copy back, nothing of size n_reads on the host)
int split_on_device(mbrwt_multi &m, const uint64_t *d_read_off, uint64_t n_reads, uint64_t n_rows, hipStream_t s0,
                    std::vector<uint64_t> &cut, std::vector<uint64_t> &row_at, bool &valid) {
    const uint32_t k = (uint32_t)m.ctx.size();
    const size_t words = 2 * (size_t)k + 3;
    MBRWT_HIP(hipSetDevice(m.dev[0]));
    int rc;
    if ((rc = ensure(m.split, words * 8))) return rc;
    uint64_t *d_out = reinterpret_cast<uint64_t *>(m.split.buf);
    MBRWT_HIP(hipMemsetAsync(d_out + words - 1, 0, 8, s0));
    const uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>((n_reads + kSplitThreads - 1) / kSplitThreads, 1024));
    hipLaunchKernelGGL(k_split_reads, dim3((unsigned)g), dim3(kSplitThreads), 0, s0, d_read_off, n_reads, n_rows, k,
                       d_out);
    MBRWT_HIP(hipGetLastError());
    std::vector<uint64_t> out(words);
    MBRWT_HIP(hipMemcpyAsync(out.data(), d_out, words * 8, hipMemcpyDeviceToHost, s0));
    MBRWT_HIP(hipStreamSynchronize(s0));
    cut.assign(out.begin(), out.begin() + k + 1);
    row_at.assign(out.begin() + k + 1, out.begin() + 2 * (size_t)k + 2);
    valid = out[words - 1] == 0;
    return MBRWT_OK;
}

int classify_multi(mbrwt_multi &m, const ClassifyCall &call, bool on_host, const uint64_t *rows, uint64_t n_rows,
                   const uint64_t *read_off, uint64_t n_reads, uint64_t *label_offsets, uint32_t *labels,
                   uint64_t *counts, uint64_t cap, uint64_t *needed, hipStream_t s0) {
    const uint32_t k = (uint32_t)m.ctx.size();
    if (!n_reads && n_rows) {  // the one offset would have to be both 0 and n_rows
        set_error("read offsets must ascend from 0 to n_rows");
        return MBRWT_ERR_INVALID;
    }
    (void)hipGetLastError();  // a stale error of an unrelated call is not this call's
    // the cuts, from offsets validated as a whole
    std::vector<uint64_t> cut(k + 1, 0), row_at(k + 1, 0);
    int rc;
    if (n_reads) {
        bool valid;
        if (on_host) {
            if ((valid = read_offsets_valid(read_off, n_reads, n_rows))) {
                split_reads(read_off, n_reads, n_rows, k, cut);
                for (uint32_t r = 0; r <= k; ++r) row_at[r] = read_off[cut[r]];
            }
        } else if ((rc = split_on_device(m, read_off, n_reads, n_rows, s0, cut, row_at, valid))) {
            return rc;
        }
        if (!valid) {
            set_error("read offsets must ascend from 0 to n_rows");
            return MBRWT_ERR_INVALID;
        }
    }
    ReadyEvent ready(m.dev[0]);
    if (!on_host && (rc = ready.record(s0))) return rc;

    // 1, 2: every replica classifies its reads into its own workspaces
    std::vector<uint64_t> need(k, 0);
    rc = for_replicas(k, [&](uint32_t r) -> int {
        const uint64_t nr = row_at[r + 1] - row_at[r], nq = cut[r + 1] - cut[r];
        const hipStream_t s = m.stream[r];
        MBRWT_HIP(hipSetDevice(m.dev[r]));
        int st;
        if ((st = ensure(m.rows[r], std::max<uint64_t>(nr, 1) * 8))) return st;
        if ((st = ensure(m.roff[r], (nq + 1) * 8))) return st;
        if ((st = ensure(m.loff[r], (nq + 1) * 8))) return st;
        if ((st = ensure(m.labs[r], 1024 * 4))) return st;
        if (call.top && (st = ensure(m.cnts[r], 1024 * 8))) return st;
        uint64_t *d_rows = reinterpret_cast<uint64_t *>(m.rows[r].buf);
        uint64_t *d_roff = reinterpret_cast<uint64_t *>(m.roff[r].buf);
        if (on_host) {
            if (nr) MBRWT_HIP(hipMemcpyAsync(d_rows, rows + row_at[r], nr * 8, hipMemcpyHostToDevice, s));
            if (n_reads) MBRWT_HIP(hipMemcpyAsync(d_roff, read_off + cut[r], (nq + 1) * 8, hipMemcpyHostToDevice, s));
        } else {
            MBRWT_HIP(hipStreamWaitEvent(s, ready.ev, 0));
            if (nr) MBRWT_HIP(hipMemcpyPeerAsync(d_rows, m.dev[r], rows + row_at[r], m.dev[0], nr * 8, s));
            if (n_reads)
                MBRWT_HIP(hipMemcpyPeerAsync(d_roff, m.dev[r], read_off + cut[r], m.dev[0], (nq + 1) * 8, s));
        }
        if (row_at[r]) {  // the slice's offsets start at 0 (a wrapped add)
            launch_rebase(d_roff, nq + 1, 0 - row_at[r], s);
            MBRWT_HIP(hipGetLastError());
        }
        auto run = [&](uint64_t *nd) {
            const uint64_t c = call.top ? std::min<uint64_t>(m.labs[r].bytes / 4, m.cnts[r].bytes / 8) : m.labs[r].bytes / 4;
            return call.run(m.ctx[r], d_rows, nr, d_roff, nq, reinterpret_cast<uint64_t *>(m.loff[r].buf),
                            reinterpret_cast<uint32_t *>(m.labs[r].buf), reinterpret_cast<uint64_t *>(m.cnts[r].buf), c,
                            nd, s);
        };
        uint64_t nd = 0;
        st = run(&nd);
        if (st == MBRWT_ERR_CAPACITY) {  // grow to the replica's label count and run again
            const uint64_t c = nd + nd / 8 + 1024;
            if ((st = ensure(m.labs[r], c * 4))) return st;
            if (call.top && (st = ensure(m.cnts[r], c * 8))) return st;
            st = run(&nd);
        }
        need[r] = nd;
        return st;
    });
    if (rc) return rc;

    std::vector<uint64_t> pre(k + 1, 0);
    for (uint32_t r = 0; r < k; ++r) pre[r + 1] = pre[r] + need[r];
    if (needed) *needed = pre[k];
    if (pre[k] > cap || (pre[k] && !(labels && (counts || !call.top)))) {
        set_error("label buffer too small (see labels_needed)");
        return MBRWT_ERR_CAPACITY;
    }

    // 3: every replica's result to its place in the caller's buffers; the
    // last replica's final offset is the total (the single 0 without reads)
    rc = for_replicas(k, [&](uint32_t r) -> int {
        const uint64_t nq = cut[r + 1] - cut[r], n_off = nq + (r + 1 == k);
        const hipStream_t s = m.stream[r];
        uint64_t *d_loff = reinterpret_cast<uint64_t *>(m.loff[r].buf);
        MBRWT_HIP(hipSetDevice(m.dev[r]));
        if (on_host) {
            if (n_off) MBRWT_HIP(hipMemcpyAsync(label_offsets + cut[r], d_loff, n_off * 8, hipMemcpyDeviceToHost, s));
            if (need[r]) {
                MBRWT_HIP(hipMemcpyAsync(labels + pre[r], m.labs[r].buf, need[r] * 4, hipMemcpyDeviceToHost, s));
                if (call.top)
                    MBRWT_HIP(hipMemcpyAsync(counts + pre[r], m.cnts[r].buf, need[r] * 8, hipMemcpyDeviceToHost, s));
            }
            MBRWT_HIP(hipStreamSynchronize(s));
            for (uint64_t i = cut[r]; i < cut[r] + n_off; ++i) label_offsets[i] += pre[r];
            return MBRWT_OK;
        }
        if (n_off) {
            if (pre[r]) {
                launch_rebase(d_loff, n_off, pre[r], s);
                MBRWT_HIP(hipGetLastError());
            }
            MBRWT_HIP(hipMemcpyPeerAsync(label_offsets + cut[r], m.dev[0], d_loff, m.dev[r], n_off * 8, s));
        }
        if (need[r]) {
            MBRWT_HIP(hipMemcpyPeerAsync(labels + pre[r], m.dev[0], m.labs[r].buf, m.dev[r], need[r] * 4, s));
            if (call.top)
                MBRWT_HIP(hipMemcpyPeerAsync(counts + pre[r], m.dev[0], m.cnts[r].buf, m.dev[r], need[r] * 8, s));
        }
        MBRWT_HIP(hipStreamSynchronize(s));  // complete before the caller's stream continues
        return MBRWT_OK;
    });
    return rc;
}

// argument checks, the handle's mutex and the exception barrier of the four entry points
int classify_entry(const char *name, mbrwt_multi *m, const ClassifyCall &call, bool on_host, const uint64_t *rows,
                   uint64_t n_rows, const uint64_t *read_off, uint64_t n_reads, uint64_t *label_offsets,
                   uint32_t *labels, uint64_t *counts, uint64_t cap, uint64_t *needed, void *stream) {
    if (!m || !label_offsets || !read_off || (n_rows && !rows)) {
        set_error("invalid argument");
        return MBRWT_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(m->mu);
    try {
        return classify_multi(*m, call, on_host, rows, n_rows, read_off, n_reads, label_offsets, labels, counts, cap,
                              needed, reinterpret_cast<hipStream_t>(stream));
    } catch (const std::bad_alloc &) {
        set_error("host allocation failed");
        return MBRWT_ERR_NOMEM;
    } catch (...) {
        set_error(std::string("unexpected exception in ") + name);
        return MBRWT_ERR_INVALID;
    }
}

// the caller thread's build options (include/mbrwt.h mbrwt_set_build_option:
// thread-local), captured once and applied in every replica's worker thread
struct BuildOptions {
    int layout = build_layout(), footprint = rows_footprint(), partitioner = build_partitioner();
    BuildTuning tuning = build_tuning();
    void apply() const {
        set_build_layout(layout);
        set_rows_footprint(footprint);
        set_build_partitioner(partitioner);
        set_build_tuning(tuning);
    }
};

}  // namespace

extern "C" {

int mbrwt_multi_create(const mbrwt_tree_desc *desc, const int *devices, int n, mbrwt_multi **out) {
    if (!desc) {
        set_error("null tree description");
        return MBRWT_ERR_INVALID;
    }
    const BuildOptions opt;  // the caller thread's options, for every replica
    return create_multi(devices, n, out, [&](int d, mbrwt_ctx **c) {
        opt.apply();
        return mbrwt_create(desc, d, c);
    });
}

int mbrwt_multi_create_synthetic(const mbrwt_synth_desc *desc, const int *devices, int n, mbrwt_multi **out) {
    if (!desc) {
        set_error("null synthetic description");
        return MBRWT_ERR_INVALID;
    }
    const BuildOptions opt;
    return create_multi(devices, n, out, [&](int d, mbrwt_ctx **c) {
        opt.apply();
        return mbrwt_create_synthetic(desc, d, c);
    });
}

int mbrwt_multi_load(const uint8_t *bytes, uint64_t len, uint64_t *consumed, const int *devices, int n,
                     mbrwt_multi **out) {
    if (!bytes && len) {
        set_error("null stream");
        return MBRWT_ERR_INVALID;
    }
    mbrwt_tree *t = nullptr;  // parsed once, uploaded to every replica
    int rc = mbrwt_tree_parse(bytes, len, consumed, &t);
    if (rc) return rc;
    rc = mbrwt_multi_create(mbrwt_tree_get_desc(t), devices, n, out);
    mbrwt_tree_free(t);
    return rc;
}

void mbrwt_multi_destroy(mbrwt_multi *m) { destroy(m); }

int mbrwt_multi_size(const mbrwt_multi *m) { return m ? (int)m->ctx.size() : 0; }

mbrwt_ctx *mbrwt_multi_replica(mbrwt_multi *m, int i) {
    return (m && i >= 0 && i < (int)m->ctx.size()) ? m->ctx[i] : nullptr;
}

int mbrwt_multi_get_rows(mbrwt_multi *m, const uint64_t *rows, uint64_t n, uint64_t *offsets, uint32_t *cols,
                         uint64_t cols_cap, uint64_t *cols_needed) {
    if (!m || !offsets || (n && !rows)) {
        set_error("invalid argument");
        return MBRWT_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(m->mu);
    try {
        std::vector<uint64_t> need;
        int rc = run_slices(*m, rows, true, n, need, nullptr);
        if (rc) return rc;
        const uint32_t k = (uint32_t)m->ctx.size();
        std::vector<uint64_t> pre(k + 1, 0);
        for (uint32_t r = 0; r < k; ++r) pre[r + 1] = pre[r] + need[r];
        if (cols_needed) *cols_needed = pre[k];
        if (pre[k] > cols_cap || (pre[k] && !cols)) {
            set_error("cols_cap too small");
            return MBRWT_ERR_CAPACITY;
        }
        // each slice straight to its place: labels at the slice's label
        // offset, row offsets rebased on the host (one thread per replica)
        std::vector<int> st(k, MBRWT_OK);
        auto put = [&](uint32_t r) -> int {
            uint64_t lo, hi;
            slice(n, k, r, lo, hi);
            MBRWT_HIP(hipSetDevice(m->dev[r]));
            if (hi > lo)
                MBRWT_HIP(hipMemcpyAsync(offsets + lo, m->off[r].buf, (hi - lo) * 8, hipMemcpyDeviceToHost,
                                         m->stream[r]));
            if (need[r])
                MBRWT_HIP(hipMemcpyAsync(cols + pre[r], m->cols[r].buf, need[r] * 4, hipMemcpyDeviceToHost,
                                         m->stream[r]));
            MBRWT_HIP(hipStreamSynchronize(m->stream[r]));
            for (uint64_t i = lo; i < hi; ++i) offsets[i] += pre[r];
            return MBRWT_OK;
        };
        std::vector<std::thread> pool;
        for (uint32_t r = 1; r < k; ++r) pool.emplace_back([&, r]() { st[r] = put(r); });
        st[0] = put(0);
        for (auto &t : pool) t.join();
        for (uint32_t r = 0; r < k; ++r)
            if (st[r]) return st[r];
        offsets[n] = pre[k];
        return MBRWT_OK;
    } catch (const std::bad_alloc &) {
        set_error("host allocation failed");
        return MBRWT_ERR_NOMEM;
    } catch (...) {
        set_error("unexpected exception in mbrwt_multi_get_rows");
        return MBRWT_ERR_INVALID;
    }
}

int mbrwt_multi_get_rows_device(mbrwt_multi *m, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets,
                                uint32_t *d_cols, uint64_t cols_cap, uint64_t *cols_needed, void *stream) {
    if (!m || !d_offsets || (n && !d_rows)) {
        set_error("invalid argument");
        return MBRWT_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(m->mu);
    try {
        const hipStream_t s0 = reinterpret_cast<hipStream_t>(stream);
        std::vector<uint64_t> need;
        int rc = run_slices(*m, d_rows, false, n, need, s0);
        if (rc) return rc;
        const uint32_t k = (uint32_t)m->ctx.size();
        std::vector<uint64_t> pre(k + 1, 0);
        for (uint32_t r = 0; r < k; ++r) pre[r + 1] = pre[r] + need[r];
        if (cols_needed) *cols_needed = pre[k];
        if (pre[k] > cols_cap || (pre[k] && !d_cols)) {
            set_error("cols_cap too small");
            return MBRWT_ERR_CAPACITY;
        }
        // rebase each slice's offsets on its own device, then peer copies
        // into the caller's buffers on device 0 (xGMI; a plain copy for
        // replica 0), all ordered before the caller's stream continues
        for (uint32_t r = 0; r < k; ++r) {
            uint64_t lo, hi;
            slice(n, k, r, lo, hi);
            MBRWT_HIP(hipSetDevice(m->dev[r]));
            uint64_t *off = reinterpret_cast<uint64_t *>(m->off[r].buf);
            if (pre[r]) {
                const uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>((hi - lo + 256) / 256, 4096));
                hipLaunchKernelGGL(k_rebase, dim3((unsigned)g), dim3(256), 0, m->stream[r], off, hi - lo + 1, pre[r]);
                MBRWT_HIP(hipGetLastError());
            }
            MBRWT_HIP(hipMemcpyPeerAsync(d_offsets + lo, m->dev[0], off, m->dev[r], (hi - lo + (r + 1 == k)) * 8,
                                         m->stream[r]));
            if (need[r])
                MBRWT_HIP(hipMemcpyPeerAsync(d_cols + pre[r], m->dev[0], m->cols[r].buf, m->dev[r], need[r] * 4,
                                             m->stream[r]));
        }
        for (uint32_t r = 0; r < k; ++r) {
            MBRWT_HIP(hipSetDevice(m->dev[r]));
            MBRWT_HIP(hipStreamSynchronize(m->stream[r]));
        }
        MBRWT_HIP(hipSetDevice(m->dev[0]));
        if (n == 0) MBRWT_HIP(hipMemsetAsync(d_offsets, 0, 8, s0));
        return MBRWT_OK;
    } catch (const std::bad_alloc &) {
        set_error("host allocation failed");
        return MBRWT_ERR_NOMEM;
    } catch (...) {
        set_error("unexpected exception in mbrwt_multi_get_rows_device");
        return MBRWT_ERR_INVALID;
    }
}

int mbrwt_multi_get_labels_batch(mbrwt_multi *m, const uint64_t *rows, uint64_t n_rows, const uint64_t *read_offsets,
                                 uint64_t n_reads, double presence_ratio, uint64_t *label_offsets, uint32_t *labels,
                                 uint64_t labels_cap, uint64_t *labels_needed) {
    return classify_entry("mbrwt_multi_get_labels_batch", m, ClassifyCall{false, presence_ratio, 0}, true, rows, n_rows,
                          read_offsets, n_reads, label_offsets, labels, nullptr, labels_cap, labels_needed, nullptr);
}

int mbrwt_multi_get_labels_batch_device(mbrwt_multi *m, const uint64_t *d_rows, uint64_t n_rows,
                                        const uint64_t *d_read_offsets, uint64_t n_reads, double presence_ratio,
                                        uint64_t *d_label_offsets, uint32_t *d_labels, uint64_t labels_cap,
                                        uint64_t *labels_needed, void *stream) {
    return classify_entry("mbrwt_multi_get_labels_batch_device", m, ClassifyCall{false, presence_ratio, 0}, false,
                          d_rows, n_rows, d_read_offsets, n_reads, d_label_offsets, d_labels, nullptr, labels_cap,
                          labels_needed, stream);
}

int mbrwt_multi_get_top_labels_batch(mbrwt_multi *m, const uint64_t *rows, uint64_t n_rows,
                                     const uint64_t *read_offsets, uint64_t n_reads, uint64_t num_top,
                                     uint64_t *label_offsets, uint32_t *labels, uint64_t *counts, uint64_t labels_cap,
                                     uint64_t *labels_needed) {
    return classify_entry("mbrwt_multi_get_top_labels_batch", m, ClassifyCall{true, 0.0, num_top}, true, rows, n_rows,
                          read_offsets, n_reads, label_offsets, labels, counts, labels_cap, labels_needed, nullptr);
}

int mbrwt_multi_get_top_labels_batch_device(mbrwt_multi *m, const uint64_t *d_rows, uint64_t n_rows,
                                            const uint64_t *d_read_offsets, uint64_t n_reads, uint64_t num_top,
                                            uint64_t *d_label_offsets, uint32_t *d_labels, uint64_t *d_counts,
                                            uint64_t labels_cap, uint64_t *labels_needed, void *stream) {
    return classify_entry("mbrwt_multi_get_top_labels_batch_device", m, ClassifyCall{true, 0.0, num_top}, false, d_rows,
                          n_rows, d_read_offsets, n_reads, d_label_offsets, d_labels, d_counts, labels_cap,
                          labels_needed, stream);
}

}  // extern "C"
