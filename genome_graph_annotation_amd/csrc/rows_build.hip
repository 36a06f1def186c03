// rows_build.hip -- ROW RECORDS: building the row-record image from a node
// image (what a record is: rows.hip; layout in mbrwt_internal.hpp "ROW
// RECORDS"), and the calling thread's build options.
//
// Build (rows_build_*): rows_build_range takes one range of rows through
// named steps.  prepare_tables (once): the walk tables and the candidate
// record code.  measure_range: one thread per row walks the node image and
// measures its record (k_rows_measure).  On the first range, for the whole
// image: choose_code settles the record code and choose_layout the block
// size B and rows per block S from the records' sizes (k_rows_plan: spilled
// rows and spill bytes per candidate) or the variable-length records, and
// allocates the image; the rules and the cost model are pure host code in
// rows_plan.hpp.  write_range: one thread per block writes the block and its
// spill entries (k_rows_write).  RowsBuild's destructor is the one release.
//
// The kernels are generic over the rows' SOURCE (rows_emit.hpp): the node
// image of the range, or -- a range of mbrwt_create_from_rows, whose Ctx
// carries label_rows and the shape as its tree (rows_from.hip) -- the rows'
// labels walked over the shape; every step of the driver is the same.
#include <algorithm>
#include <memory>
#include <optional>

#include "device_access.hpp"
#include "mbrwt_internal.hpp"
#include "rows_emit.hpp"
#include "rows_plan.hpp"
#include "rows_record.hpp"

namespace mbrwt {

// ------------------------------------------------------------------------
// layout selection
// ------------------------------------------------------------------------
static thread_local int g_build_layout = LAYOUT_AUTO;  // AUTO: the automatic choice
static thread_local BuildTuning g_build_tuning;        // MBRWT_BUILD_ROWS_VAR .. _ROWS_WGS_PER_CU
BuildTuning &build_tuning() { return g_build_tuning; }
void set_build_tuning(const BuildTuning &t) { g_build_tuning = t; }

int build_layout() { return g_build_layout; }

void set_build_layout(int layout) { g_build_layout = layout; }
int thread_build_layout() { return g_build_layout; }
static thread_local int g_rows_footprint = 0;  // MBRWT_ROWS_FAST
void set_rows_footprint(int v) { g_rows_footprint = v; }
int rows_footprint() { return g_rows_footprint; }

namespace {

// the terminals of row r's descent in pre-order, term(id, children mask):
// the row's masks (emit_row_masks) walked over the build table BT
// (build_term_tables).  False when the row has more than kTermMaxMasks masks
// or its masks do not follow the table.
constexpr uint32_t kTermMaxMasks = 256;
template <class Src, class Term>
__device__ bool row_terms(const Src &src, uint32_t r, const uint32_t *bt, Term term, uint32_t &labels) {
    uint16_t mb[kTermMaxMasks];
    uint32_t nm = 0;
    labels = src.masks(r, [&](uint64_t mk, uint32_t, uint32_t) {
        if (nm < kTermMaxMasks) mb[nm] = (uint16_t)mk;
        ++nm;
    });
    if (labels == ~0u || nm > kTermMaxMasks) return false;
    if (!nm) return labels == 0;
    const uint32_t root = gld(bt);
    if ((root >> 30) == 3u) {  // a one-level tree
        term(gld(bt + 1), (uint32_t)mb[0]);
        return nm == 1;
    }
    const uint32_t nE = gld(bt + 2);
    const uint32_t *ent = bt + 4, *tid = bt + 4 + nE;
    uint32_t pos = 1, m = mb[0], f = root & 0xFFFFu;
    uint32_t sf[kRowsMaxHeight], sm[kRowsMaxHeight];
    int sp = 0;
    while (true) {
        if (!m) {
            if (!sp) break;
            --sp;
            f = sf[sp];
            m = sm[sp];
            continue;
        }
        const uint32_t c = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        const uint32_t sl = f + c;
        if (sl >= nE) return false;
        const uint32_t e = gld(ent + sl);
        if ((e >> 31) == 0u) {  // an internal node: its mask, one level down
            if (pos >= nm || (m && sp == (int)kRowsMaxHeight)) return false;
            if (m) {
                sf[sp] = f;
                sm[sp] = m;
                ++sp;
            }
            f = e & 0xFFFFu;
            m = mb[pos++];
        } else if ((e >> 30) == 3u) {  // a leaf parent: a terminal with its mask
            if (pos >= nm) return false;
            term(gld(tid + sl), (uint32_t)mb[pos++]);
        } else {  // a leaf: a terminal of its own
            term(gld(tid + sl), 0u);
        }
    }
    return pos == nm;
}
// row r's terminal fields (w bits: id | mask << ib) from byte p on; the
// bytes written, or ~0u
template <class Src>
__device__ __forceinline__ uint32_t write_row_terms(const Src &src, uint32_t r, uint8_t *p, const uint32_t *bt,
                                                    uint32_t w, uint32_t ib, uint32_t &labels) {
    uint64_t acc = 0;
    uint32_t nb = 0, wr = 0;
    const bool ok = row_terms(
        src, r, bt,
        [&](uint32_t id, uint32_t m) {
            acc |= (uint64_t)(id | (m << ib)) << nb;
            nb += w;
            while (nb >= 8u) {
                p[wr++] = (uint8_t)acc;
                acc >>= 8;
                nb -= 8u;
            }
        },
        labels);
    if (nb) p[wr++] = (uint8_t)acc;
    return ok ? wr : ~0u;
}

// per row of a range: record size (1 + mask bytes, < 2^15) | 0x8000 when the
// row has >= 255 labels (its count does not fit the inline byte)
// (nib: the masks as nibble codes, rows_record.hpp RecMasks)
// (Src: the rows' source, rows_emit.hpp -- a node image or the rows' labels)
template <class Src>
__global__ __launch_bounds__(256) void k_rows_measure(Src src, uint64_t n, uint16_t *sz, unsigned long long *acc,
                                                      uint32_t code, const uint32_t *bt, uint32_t w) {
    const bool nib = code == 1u;
    unsigned long long lab = 0, bytes = 0, bad = 0, bytes1 = 0;
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gs) {
        uint32_t b = 1, nn = 0, b1 = 1;
        uint32_t L = src.masks((uint32_t)r, [&](uint64_t mk, uint32_t a, uint32_t) {
            if (nib) nn += nib_codes((uint32_t)mk);
            else b += rec_mask_bytes(a);
            b1 += rec_mask_bytes(a);
        });
        b += (nn + 1) / 2;
        if (code == 2u && L != ~0u) {  // terminal records: the fields' bytes
            uint32_t nt = 0, L2 = 0;
            b = row_terms(src, (uint32_t)r, bt, [&](uint32_t, uint32_t) { ++nt; }, L2) && L2 == L
                    ? 1u + (nt * w + 7u) / 8u
                    : 0x8000u;  // (a row the fields cannot hold: bad)
        }
        bytes1 += b1;
        // (a row of >= 2^15 labels: the temp regions carry a row's count in
        // 15 bits beside the long-record flag, k_traverse_rows / k_compact_tiles)
        if (L == ~0u || b >= 0x8000 || L > 0x7FFFu) {
            ++bad;
            sz[r] = 0x7FFF;
            continue;
        }
        sz[r] = (uint16_t)(b | (L >= 255 ? 0x8000u : 0u));
        lab += L;
        bytes += b;
    }
    for (int off = 32; off > 0; off >>= 1) {
        lab += __shfl_down(lab, off);
        bytes += __shfl_down(bytes, off);
        bad += __shfl_down(bad, off);
        bytes1 += __shfl_down(bytes1, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (lab) atomicAdd(acc + 0, lab);
        if (bytes) atomicAdd(acc + 1, bytes);
        if (bad) atomicAdd(acc + 2, bad);
        if (bytes1) atomicAdd(acc + 3, bytes1);  // (the byte-coded size, beside a nibble measure)
    }
}

// which rows of a block spill: rows with >= 255 labels always; then, while
// the block overflows, the largest inline record (a spilled entry takes 5
// bytes in the block)
__device__ __forceinline__ uint32_t block_spills(const uint32_t *s, uint32_t nrows, uint32_t S, uint32_t B) {
    uint32_t used = S, spilled = 0;
    for (uint32_t t = 0; t < nrows; ++t) {
        if (s[t] & 0x8000u) {
            spilled |= 1u << t;
            used += 5;
        } else {
            used += s[t];
        }
    }
    while (used > B) {
        uint32_t best = 0, bt = 0;
        for (uint32_t t = 0; t < nrows; ++t)
            if (!((spilled >> t) & 1u) && s[t] >= best) {
                best = s[t];
                bt = t;
            }
        spilled |= 1u << bt;
        used = used - best + 5;
    }
    return spilled;
}
__device__ __forceinline__ uint32_t spill_units(uint32_t s) { return (8 + ((s & 0x7FFFu) - 1) + 15) / 16; }

// a candidate (B, S): spilled rows, spill units, rows whose spill entry is
// longer than a block (direct pass)
__global__ __launch_bounds__(256) void k_rows_plan(const uint16_t *sz, uint64_t n, uint32_t B, uint32_t S,
                                                   unsigned long long *acc) {
    unsigned long long sp = 0, units = 0, lng = 0;
    const uint64_t nb = (n + S - 1) / S;
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += gs) {
        uint32_t s[16];
        const uint32_t nr = (uint32_t)std::min<uint64_t>(S, n - b * S);
        for (uint32_t t = 0; t < nr; ++t) s[t] = gld(sz + b * S + t);
        const uint32_t m = block_spills(s, nr, S, B);
        for (uint32_t t = 0; t < nr; ++t)
            if ((m >> t) & 1u) {
                ++sp;
                units += spill_units(s[t]);
                lng += (8 + (s[t] & 0x7FFFu) - 1 > B) ? 1u : 0u;
            }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sp += __shfl_down(sp, off);
        units += __shfl_down(units, off);
        lng += __shfl_down(lng, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (sp) atomicAdd(acc + 0, sp);
        if (units) atomicAdd(acc + 1, units);
        if (lng) atomicAdd(acc + 2, lng);
    }
}

// the masks of row r written from byte p on (bytes, or nibble codes); the
// bytes written
template <class Src>
__device__ __forceinline__ uint32_t write_row_masks(const Src &src, uint32_t r, uint8_t *p, uint32_t nib,
                                                    uint32_t &labels) {
    uint32_t w = 0;
    auto put = [&](uint32_t v) {  // nibble w: byte w / 2, low half first
        if (w & 1u) p[w >> 1] |= (uint8_t)(v << 4);
        else p[w >> 1] = (uint8_t)v;
        ++w;
    };
    labels = src.masks(r, [&](uint64_t mk, uint32_t a, uint32_t) {
        if (nib) {  // (arity <= 8)
            if (nib_codes((uint32_t)mk) == 1u) {
                put((uint32_t)__builtin_ctzll(mk));
            } else {
                put(8u);
                put((uint32_t)mk & 15u);
                put((uint32_t)(mk >> 4) & 15u);
            }
        } else {  // one byte per 8 children, little-endian
            for (uint32_t k = 0; k < a; k += 8) p[w++] = (uint8_t)(mk >> k);
        }
    });
    return nib ? (w + 1) / 2 : w;
}

// one thread per block of the range: header, inline records, spill entries
template <class Src>
__global__ __launch_bounds__(256) void k_rows_write(Src src, uint64_t nr_range, const uint16_t *sz, uint32_t B,
                                                    uint32_t S, uint8_t *blocks, uint8_t *spill,
                                                    unsigned long long *spill_used, uint32_t code, const uint32_t *bt,
                                                    uint32_t w, uint32_t ib) {
    const uint32_t nib = code == 1u ? 1u : 0u;
    auto write = [&](uint32_t r, uint8_t *p, uint32_t &L) -> uint32_t {
        return code == 2u ? write_row_terms(src, r, p, bt, w, ib, L) : write_row_masks(src, r, p, nib, L);
    };
    const uint64_t nb = (nr_range + S - 1) / S;
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += gs) {
        uint32_t s[16];
        const uint32_t nr = (uint32_t)std::min<uint64_t>(S, nr_range - b * S);
        for (uint32_t t = 0; t < nr; ++t) s[t] = gld(sz + b * S + t);
        const uint32_t m = block_spills(s, nr, S, B);
        uint8_t *blk = blocks + b * B;
        uint32_t o = S;
        for (uint32_t t = 0; t < nr; ++t) {
            const uint32_t r = (uint32_t)(b * S + t);
            if ((m >> t) & 1u) {
                const uint64_t idx = atomicAdd(spill_used, (unsigned long long)spill_units(s[t]));
                uint8_t *se = spill + idx * 16;
                uint32_t L = 0;
                const uint32_t nw = write(r, se + 8, L);
                *reinterpret_cast<uint32_t *>(se) = L;
                *reinterpret_cast<uint32_t *>(se + 4) = nw;
                blk[t] = (uint8_t)(o | 0x80u);
                blk[o] = (uint8_t)std::min<uint32_t>(L, 255);
                for (uint32_t k = 0; k < 4; ++k) blk[o + 1 + k] = (uint8_t)(idx >> (8 * k));
                o += 5;
            } else {
                blk[t] = (uint8_t)o;
                uint32_t L = 0;
                const uint32_t nw = write(r, blk + o + 1, L);
                blk[o] = (uint8_t)L;
                o += 1 + nw;
            }
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------
// build driver
// ------------------------------------------------------------------------
// The layout of the whole image, chosen on the first range (choose_layout);
// every later range is written under it.
struct RowsPlan {
    bool var = false;              // variable-length records (rows_var.hip) instead of blocks
    BlockShape block{0, 0};        // blocks: their bytes and rows per block
    double var_bytes_per_row = 0;  // variable-length records: their size per row on the first range
};

struct RowsBuild {
    Ctx *top = nullptr;
    uint64_t n = 0, align = 1;
    std::optional<RowsPlan> plan;  // unset until the first range has decided (record code: img.term / img.nib)
    bool auto_layout = false;  // layout AUTO: decline records that cost more than kAutoMaxCost requests per row
    int footprint = 0;         // MBRWT_BUILD_ROWS_FOOTPRINT of the creating thread
    VarScratch vws;            // variable-length records (rows_var.hip)
    RowsImage img;
    unsigned long long *d_acc = nullptr;  // [0..3] measure, [4..7] plan
    uint16_t *d_sz = nullptr;
    uint64_t sz_cap = 0;
    hipStream_t s = nullptr;
    uint32_t *d_bt = nullptr;  // terminal records: the build table (build_term_tables)

    RowsBuild() = default;
    RowsBuild(const RowsBuild &) = delete;
    RowsBuild &operator=(const RowsBuild &) = delete;
    ~RowsBuild();  // the one release: scratch, and the image unless rows_build_finish moved it out
};

void free_rows(RowsImage &r) {
    for (void *p : r.var_chunks) (void)hipFree(p);
    if (r.var_lines) (void)hipFree(r.var_lines);
    if (r.d_var_units) (void)hipFree(r.d_var_units);
    if (r.d_var_anc) (void)hipFree(r.d_var_anc);
    if (r.d_unit_of) (void)hipFree(r.d_unit_of);
    if (r.blocks) (void)hipFree(r.blocks);
    if (r.spill) (void)hipFree(r.spill);
    if (r.d_spill_used) (void)hipFree(r.d_spill_used);
    if (r.d_table) (void)hipFree(r.d_table);
    if (r.d_table2) (void)hipFree(r.d_table2);
    if (r.d_table3) (void)hipFree(r.d_table3);
    if (r.d_table4) (void)hipFree(r.d_table4);
    if (r.classes) (void)hipFree(r.classes);
    r = RowsImage();
}

RowsBuild *rows_build_begin(Ctx &top, uint64_t num_rows, uint64_t align, bool auto_layout) {
    RowsBuild *rb = new (std::nothrow) RowsBuild();
    if (!rb) return nullptr;
    rb->top = &top;
    rb->auto_layout = auto_layout;
    rb->footprint = g_rows_footprint;
    rb->n = num_rows;
    rb->align = std::max<uint64_t>(1, align);
    rb->s = top.stream;
    if (hipMalloc(&rb->d_acc, 8 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&rb->img.d_spill_used, sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(rb->img.d_spill_used, 0, sizeof(unsigned long long)) != hipSuccess) {
        rows_build_abort(rb);
        return nullptr;
    }
    return rb;
}

RowsBuild::~RowsBuild() {
    if (d_acc) (void)hipFree(d_acc);
    if (d_sz) (void)hipFree(d_sz);
    if (d_bt) (void)hipFree(d_bt);
    var_free_scratch(vws);
    free_rows(img);
}

void rows_build_abort(RowsBuild *rb) { delete rb; }

const char *rows_limits_message() {
    return "tree shape outside the row-record limits (arity <= 64, columns < 2^16, height <= 16, a walk table of <= "
           "8192 words)";
}

static int read_acc(RowsBuild &rb, unsigned long long *h, int k) {
    MBRWT_HIP(hipMemcpyAsync(h, rb.d_acc, k * sizeof(unsigned long long), hipMemcpyDeviceToHost, rb.s));
    MBRWT_HIP(hipStreamSynchronize(rb.s));
    return MBRWT_OK;
}

// grow the spill area to hold `bytes` (entries keep their offsets: copy)
static int ensure_spill(RowsBuild &rb, uint64_t bytes) {
    RowsImage &im = rb.img;
    const uint64_t need = bytes + im.B + 256;
    if (need <= im.spill_cap) return MBRWT_OK;
    const uint64_t cap = std::max<uint64_t>(need, im.spill_cap + im.spill_cap / 4);
    uint8_t *p = nullptr;
    MBRWT_HIP(hipMalloc(&p, cap));
    MBRWT_HIP(hipMemsetAsync(p, 0, cap, rb.s));
    if (im.spill) {
        MBRWT_HIP(hipMemcpyAsync(p, im.spill, im.spill_cap, hipMemcpyDeviceToDevice, rb.s));
        MBRWT_HIP(hipStreamSynchronize(rb.s));
        MBRWT_HIP(hipFree(im.spill));
    }
    im.spill = p;
    im.spill_cap = cap;
    return MBRWT_OK;
}

// the record code the image stands at: prepare_tables' candidate, settled by
// choose_code on the first range (0 byte masks, 1 nibble codes, 2 terminal
// records), and the terminal fields' widths (word 0 of the TT table)
static uint32_t record_code(const RowsImage &im) { return im.term ? 2u : im.nib ? 1u : 0u; }
static uint32_t term_width(const RowsImage &im) { return im.term ? im.table3[0] & 0xFFu : 0u; }
static uint32_t term_id_bits(const RowsImage &im) { return im.term ? (im.table3[0] >> 8) & 0xFFu : 0u; }

// Prepare, once: the RWT / RWT2 / path tables of the tree's shape and, where
// the build options and the shape allow them, the nibble codes or the
// terminal records' tables (TT, work table, the build table on the device).
// Leaves the candidate record code in im.nib / im.term.
static int prepare_tables(RowsBuild &rb, Ctx &range) {
    RowsImage &im = rb.img;
    if (!build_rwt_table(range.tree, im.table, im.height, im.max_arity) ||
        !build_rwt2_table(range.tree, im.table2, im.frames, &im.slot_dnode)) {
        im.table.clear();
        set_error(rows_limits_message());
        return MBRWT_ERR_UNSUPPORTED;
    }
    // one-byte masks everywhere (rows_walk6): the root and every internal
    // or leaf-parent entry of arity <= 8
    auto ar8 = [](uint32_t e) { return (e >> 30) == 2u || ((e >> 16) & 0x7Fu) <= 8; };
    im.mask1 = ar8(im.table2[0]);
    for (size_t i = 4; i < 4 + (size_t)im.table2[1]; ++i) im.mask1 = im.mask1 && ar8(im.table2[i]);
    im.uni = im.mask1 ? rwt2_uniform_levels(im.table2) : 0u;
    if (im.uni) append_path_table(im.table2, im.uni);
    // masks wider than 16 bits (r06: arity up to 64) are read by the tree
    // odometer and the one-lane walks only: such a tree needs the tree
    // odometer's depth
    // (im.max_arity: over the nodes the walk reaches -- record-only
    // dnodes such as PACKT_IN carry other arities)
    if (im.max_arity > 16 && im.frames > kRowsOdoLevels) {
        im.table.clear();
        set_error("row records: a node wider than 16 children in a tree deeper than the tree odometer (8 levels)");
        return MBRWT_ERR_UNSUPPORTED;
    }
    // nibble-coded masks (MBRWT_BUILD_ROWS_CODE = 1, r06): read by the
    // path-table odometer and the one-lane walks, so uniform trees of
    // one-byte masks with a path table only (the others keep bytes)
    im.nib = build_tuning().rows_code == 1 && im.uni && im.table2.size() > 3 && im.table2[3] != 0;
    // terminal records (r06; MBRWT_BUILD_ROWS_CODE 0 = AUTO, the default,
    // or 2): trees of masks up to 16 bits whose terminals fit the fields
    im.term = false;
    // (AUTO, code 0: where they are smaller than byte masks -- decided on
    // the first range by choose_code; code 3 forces byte masks)
    const int code = build_tuning().rows_code;
    if ((code == 0 || code == 2) && im.max_arity <= 16) {
        std::vector<uint32_t> bt, term_slot;
        bool ok = build_term_tables(im.table2, im.table3, bt, term_slot);
        if (ok) {
            im.term_dnode.resize(term_slot.size());
            for (size_t i = 0; i < term_slot.size(); ++i)
                im.term_dnode[i] = term_slot[i] < im.slot_dnode.size() ? im.slot_dnode[term_slot[i]] : ~0u;
            ok = build_work_table(range.tree, im.term_dnode, im.table4);
        }
        if (ok) {
            if (!rb.d_bt) {
                if (hipMalloc(&rb.d_bt, bt.size() * 4) != hipSuccess) return hip_fail(hipGetLastError(), "build table");
                MBRWT_HIP(hipMemcpy(rb.d_bt, bt.data(), bt.size() * 4, hipMemcpyHostToDevice));
            }
            im.term = true;
        }
    }
    return MBRWT_OK;
}

// k_rows_measure's counters of one range
struct Measure {
    unsigned long long labels, bytes, bad, byte_coded;  // (bad: rows the code cannot hold)
};

// Measure, per range: every row's record size under the image's record code
// (into d_sz) and the range's counters
static int measure_range(RowsBuild &rb, Ctx &range, Measure &h) {
    const RowsImage &im = rb.img;
    const uint64_t nr = range.tree.num_rows;
    MBRWT_HIP(hipMemsetAsync(rb.d_acc, 0, 8 * sizeof(unsigned long long), rb.s));
    with_row_source(range, [&](auto src) {
        hipLaunchKernelGGL(k_rows_measure<decltype(src)>, dim3(grid256(nr)), dim3(256), 0, rb.s, src, nr, rb.d_sz,
                           rb.d_acc, record_code(im), (const uint32_t *)rb.d_bt, term_width(im));
    });
    MBRWT_HIP(hipGetLastError());
    unsigned long long a[4];
    if (int rc = read_acc(rb, a, 4)) return rc;
    h = Measure{a[0], a[1], a[2], a[3]};
    return MBRWT_OK;
}

// Decide, on the first range: the record code of the whole image (the rule:
// rows_plan.hpp); a code that gives way is measured again as what follows it
static int choose_code(RowsBuild &rb, Ctx &range, Measure &h) {
    RowsImage &im = rb.img;
    if (im.term && term_gives_way(h.bad, h.bytes, h.byte_coded)) {
        im.term = false;
        im.table3.clear();
        if (int rc = measure_range(rb, range, h)) return rc;
    }
    if (im.nib && nib_gives_way(h.bad, h.bytes, h.byte_coded)) {
        im.nib = false;
        if (int rc = measure_range(rb, range, h)) return rc;
    }
    return MBRWT_OK;
}

// k_rows_plan's counters of the measured range under one block shape
static int plan_range(RowsBuild &rb, Ctx &range, BlockShape bs, PlanCounts &out) {
    const uint64_t nr = range.tree.num_rows;
    MBRWT_HIP(hipMemsetAsync(rb.d_acc, 0, 8 * sizeof(unsigned long long), rb.s));
    hipLaunchKernelGGL(k_rows_plan, dim3(grid256((nr + bs.S - 1) / bs.S)), dim3(256), 0, rb.s, rb.d_sz, nr, bs.B, bs.S,
                       rb.d_acc);
    MBRWT_HIP(hipGetLastError());
    unsigned long long o[3];
    if (int rc = read_acc(rb, o, 3)) return rc;
    out = PlanCounts{o[0], o[1], o[2]};
    return MBRWT_OK;
}

// the variable-length records of the first range measured: whether they
// apply (ok), the whole image's bytes, the bytes per row into the plan
static int measure_var(RowsBuild &rb, Ctx &range, bool forced, RowsPlan &plan, bool &ok, double &image_bytes) {
    RowsImage &im = rb.img;
    const uint64_t nr = range.tree.num_rows;
    uint64_t vb = 0;
    const int rc = var_measure_range(im, range, rb.vws, &vb, rb.s);
    if (rc && rc != MBRWT_ERR_UNSUPPORTED) return rc;
    ok = rc == MBRWT_OK;
    image_bytes = var_image_bytes(vb, nr, rb.n, rb.align);
    plan.var_bytes_per_row = (double)vb / (double)nr;
    // a unit table so large that the decode's LDS cannot hold a mean
    // tile beside it: AUTO keeps the other layouts (forced: allowed,
    // every such tile then takes the decode's global path)
    if (ok && !forced &&
        !var_lds_fits(im, (double)range.tree.num_relations / std::max<double>(1.0, (double)range.tree.num_rows),
                      plan.var_bytes_per_row))
        ok = false;
    return MBRWT_OK;
}

// the image's device memory under the plan: directory lines or blocks
static int alloc_image(RowsBuild &rb, const RowsPlan &plan) {
    RowsImage &im = rb.img;
    if (plan.var) {
        im.var = true;
        const uint64_t nlines = (rb.n + kVarLineRows - 1) / kVarLineRows;
        MBRWT_HIP(hipMalloc(&im.var_lines, nlines * 64));
        MBRWT_HIP(hipMemsetAsync(im.var_lines, 0, nlines * 64, rb.s));
        return MBRWT_OK;
    }
    im.B = plan.block.B;
    im.S = plan.block.S;
    im.magic = div_magic(im.S);
    im.num_blocks = (rb.n + im.S - 1) / im.S;
    MBRWT_HIP(hipMalloc(&im.blocks, im.num_blocks * im.B));
    MBRWT_HIP(hipMemsetAsync(im.blocks, 0, im.num_blocks * im.B, rb.s));
    return MBRWT_OK;
}

// Decide, on the first range: the layout of the whole image -- every
// candidate (B, S) planned over the range and priced (the cost model and the
// choice: rows_plan.hpp), the variable-length records where the blocks cost
// too much or the build option forces them, the AUTO decline, the
// MBRWT_BUILD_ROWS_BLOCK override -- then the image's allocation.  Sets rb.plan.
static int choose_layout(RowsBuild &rb, Ctx &range) {
    RowsImage &im = rb.img;
    size_t free_b = 0, total_b = 0;
    MBRWT_HIP(hipMemGetInfo(&free_b, &total_b));
    const double budget = (double)free_b - 4.0 * (1ull << 30);
    std::vector<Cand> cands;
    for (BlockShape bs : block_candidates(rb.align)) {
        PlanCounts o;
        if (int rc = plan_range(rb, range, bs, o)) return rc;
        cands.push_back(price_candidate(bs, o, range.tree.num_rows, rb.n));
    }
    const Choice ch = choose_block(cands, budget, cost_tolerance(rb.footprint == 1, im.uni != 0));
    RowsPlan plan;
    const int force_var = build_tuning().rows_var;
    const bool want_var = force_var == 1 || ch.tmin > kAutoMaxCost;
    bool var_ok = force_var != 0 && rb.align % kVarLineRows == 0 && var_prepare(range.tree, im);
    // the lanes per row the decode will run with (the build option, else
    // automatic): the LDS gate (measure_var) must judge that geometry
    uint32_t var_G = build_tuning().var_lanes;
    if (var_G & (var_G - 1) || var_G > 16) var_G = 0;  // (1, 2, 4, 8 or 16; 0: automatic)
    im.var_G = var_G;
    double var_mem = kNoFit;
    if (var_ok && want_var)
        if (int rc = measure_var(rb, range, force_var == 1, plan, var_ok, var_mem)) return rc;
    if (var_ok && var_mem <= budget && want_var) {
        plan.var = true;
    } else {
        if (!ch.best) {
            set_error("row-record image does not fit the device");
            return MBRWT_ERR_NOMEM;
        }
        if (rb.auto_layout && ch.tmin > kAutoMaxCost) {  // (kAutoMaxCost, rows_plan.hpp)
            set_error("row records too long for the block layout");
            return MBRWT_ERR_UNSUPPORTED;
        }
        plan.block = {ch.best->B, ch.best->S};
        (void)block_override(build_tuning().rows_block, rb.align, plan.block);  // MBRWT_BUILD_ROWS_BLOCK
    }
    if (int rc = alloc_image(rb, plan)) return rc;
    rb.plan = plan;
    return MBRWT_OK;
}

// Write, per range: the range's records into the image under the plan --
// blocks with their spill entries (the spill area planned and grown first),
// or the variable-length records (rows_var.hip)
static int write_range(RowsBuild &rb, Ctx &range, uint64_t row0) {
    RowsImage &im = rb.img;
    const uint64_t nr = range.tree.num_rows;
    if (rb.plan->var) return var_build_range(im, range, row0, rb.vws, rb.s);
    PlanCounts pc;
    if (int rc = plan_range(rb, range, rb.plan->block, pc)) return rc;
    unsigned long long used = 0;
    MBRWT_HIP(hipMemcpyAsync(&used, im.d_spill_used, sizeof(used), hipMemcpyDeviceToHost, rb.s));
    MBRWT_HIP(hipStreamSynchronize(rb.s));
    // a spilled entry stores its offset as u32 16-byte units: the spill area
    // addresses 64 GiB
    if (used + pc.units >= (1ull << 32)) {
        set_error("row-record spill area beyond 64 GiB");
        return MBRWT_ERR_UNSUPPORTED;
    }
    // the first range sizes the area for the whole image (extrapolated)
    const double scale = row0 == 0 ? (double)rb.n / (double)nr : 1.0;
    if (int rc = ensure_spill(
            rb, (uint64_t)(used * 16 + pc.units * 16 * scale * (row0 == 0 ? 1.05 : 1.0)) + 16 * pc.units))
        return rc;
    im.spilled_rows += pc.spilled;
    im.long_rows += pc.long_rows;
    im.spill_bytes += pc.units * 16;
    with_row_source(range, [&](auto src) {
        hipLaunchKernelGGL(k_rows_write<decltype(src)>, dim3(grid256((nr + im.S - 1) / im.S)), dim3(256), 0, rb.s, src,
                           nr, rb.d_sz, im.B, im.S, im.blocks + (row0 / im.S) * im.B, im.spill, im.d_spill_used,
                           record_code(im), (const uint32_t *)rb.d_bt, term_width(im), term_id_bits(im));
    });
    MBRWT_HIP(hipGetLastError());
    MBRWT_HIP(hipStreamSynchronize(rb.s));
    return MBRWT_OK;
}

// Records of one range: prepare (once), measure, decide (the first range, for
// the whole image: record code, then layout), write.
int rows_build_range(RowsBuild *rbp, Ctx &range, uint64_t row0) {
    if (!rbp) return MBRWT_ERR_NOMEM;
    RowsBuild &rb = *rbp;
    RowsImage &im = rb.img;
    const uint64_t nr = range.tree.num_rows;
    if (!nr) return MBRWT_OK;
    // (a range of a build from rows brings its labels instead, rows_from.hip)
    if ((!range.d_nodes && !range.label_rows.shape) || range.tree.nodes.empty()) {
        set_error("row records need a node image");
        return MBRWT_ERR_UNSUPPORTED;
    }
    if (row0 % rb.align) {
        set_error("row-record range not aligned");
        return MBRWT_ERR_INVALID;
    }
    if (im.table.empty())
        if (int rc = prepare_tables(rb, range)) return rc;
    if (nr > rb.sz_cap) {
        if (rb.d_sz) MBRWT_HIP(hipFree(rb.d_sz));
        rb.d_sz = nullptr;
        MBRWT_HIP(hipMalloc(&rb.d_sz, nr * sizeof(uint16_t)));
        rb.sz_cap = nr;
    }
    Measure h;
    if (int rc = measure_range(rb, range, h)) return rc;
    const bool first = !rb.plan;  // the first range decides for the whole image
    if (first)
        if (int rc = choose_code(rb, range, h)) return rc;
    if (h.bad) {
        set_error("row record deeper than the build walker supports, or a row of more than 32,767 labels");
        return MBRWT_ERR_UNSUPPORTED;
    }
    if (h.labels != range.tree.num_relations) {
        set_error("row records: label count differs from the node image");
        return MBRWT_ERR_DEVICE;
    }
    if (!im.var) im.record_bytes += h.bytes;
    if (first)
        if (int rc = choose_layout(rb, range)) return rc;
    return write_range(rb, range, row0);
}

// device bytes the records of `rows` more rows will still allocate (the
// variable-length records are allocated per range; blocks up front)
uint64_t rows_build_pending_bytes(const RowsBuild *rb, uint64_t rows) {
    return rb && rb->plan && rb->plan->var ? var_pending_bytes(rb->plan->var_bytes_per_row, rows) : 0;
}

// the finished image's tables on the device, its size, its record classes
static int finish_image(RowsBuild &rb) {
    RowsImage &im = rb.img;
    if (!rb.plan) {  // no rows
        set_error("row records of an empty matrix");
        return MBRWT_ERR_UNSUPPORTED;
    }
    if (hipMalloc(&im.d_table, im.table.size() * 4) != hipSuccess ||
        hipMemcpy(im.d_table, im.table.data(), im.table.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(&im.d_table2, im.table2.size() * 4) != hipSuccess ||
        hipMemcpy(im.d_table2, im.table2.data(), im.table2.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return hip_fail(hipGetLastError(), "row-record table upload");
    if (im.term &&
        (hipMalloc(&im.d_table3, im.table3.size() * 4) != hipSuccess ||
         hipMemcpy(im.d_table3, im.table3.data(), im.table3.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
         hipMalloc(&im.d_table4, im.table4.size() * 4) != hipSuccess ||
         hipMemcpy(im.d_table4, im.table4.data(), im.table4.size() * 4, hipMemcpyHostToDevice) != hipSuccess))
        return hip_fail(hipGetLastError(), "terminal table upload");
    if (im.var) {
        // (+32 zero entries: the decoder's speculative unit reads past the last word)
        if (hipMalloc(&im.d_var_units, (im.var_units.size() + 32) * 4) != hipSuccess ||
            hipMemset(im.d_var_units, 0, (im.var_units.size() + 32) * 4) != hipSuccess ||
            hipMemcpy(im.d_var_units, im.var_units.data(), im.var_units.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMalloc(&im.d_var_anc, std::max<size_t>(1, im.var_anc.size()) * 4) != hipSuccess ||
            hipMemcpy(im.d_var_anc, im.var_anc.data(), im.var_anc.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return hip_fail(hipGetLastError(), "variable-length record tables");
        im.bytes = (rb.n + kVarLineRows - 1) / kVarLineRows * 64 + im.var_rec_bytes;
        return MBRWT_OK;
    }
    if (!im.spill && ensure_spill(rb, 0)) return MBRWT_ERR_NOMEM;
    im.bytes = im.num_blocks * im.B + im.spill_bytes;
    // record classes where rows repeat few distinct records (rows_class.hip)
    return rows_classes_build(im, rb.n, build_tuning().rows_classes, &im.class_sample_distinct, rb.s);
}

// uploads the tables, moves the image into the context; frees the build
// whether it succeeds or not
int rows_build_finish(RowsBuild *rbp) {
    if (!rbp) return MBRWT_ERR_NOMEM;
    std::unique_ptr<RowsBuild> rb(rbp);
    if (int rc = finish_image(*rb)) return rc;
    RowsImage &im = rb->img;
    im.occ_cap = build_tuning().rows_wgs_per_cu;  // (MBRWT_BUILD_ROWS_WGS_PER_CU: occupancy sweeps)
    im.ready = true;
    free_rows(rb->top->rows);
    rb->top->rows = im;
    im = RowsImage();  // ownership moved
    return MBRWT_OK;
}

}  // namespace mbrwt
