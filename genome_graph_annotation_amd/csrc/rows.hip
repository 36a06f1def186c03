// rows.hip -- ROW RECORDS: the BRWT's index bits regrouped by row, and the
// row-record query kernels (layout in mbrwt_internal.hpp "ROW RECORDS",
// DESIGN.md §4/§5; the image is built in rows_build.hip from the walk tables
// of rows_tables.cpp).
//
// The reference answers get_row(r) (BRWT.cpp:26-53) by a descent that reads,
// at every internal node u it reaches, the index bits of u's children at
// j = rank1(u, i) - 1 (BRWT.cpp:30, :43).  Those bits -- the children mask of
// u at the row's position -- belong to row r alone: every bit of every index
// column is reached by exactly one row.  A row's RECORD is the masks of its
// descent in DFS pre-order (the order the reference visits them, BRWT.cpp:
// 45-51), so the records of all rows are a permutation of the tree's index
// bits, and get_row is one 64- or 128-byte block read plus a walk of the
// record over the tree's shape (the RWT table, in LDS): the rank1 remaps are
// resolved once, when the image is built from a node image (any of its
// layouts), not per query.
//
// Query (rows_get_rows): k_traverse_rows -- one wave per tile of 64 query
// rows: the 64 blocks are read as coalesced 16-byte quarters (one request per
// block) into LDS, a wave scan of the records' label counts places every
// row's labels, the 64 lanes walk their records in lockstep over the RWT table
// writing u16 labels into an LDS stage, which leaves as full-line stores into
// the tile's temp region; one scan over the tile totals and k_compact_tiles
// (u16 -> the caller's u32 CSR, the call's status) follow.  Tiles with more
// labels than their region, or with a record longer than a block, are walked
// by k_compact_tiles itself from the records in global memory.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "device_access.hpp"
#include "mbrwt_internal.hpp"
#include "pack_block.hpp"
#include "rows_record.hpp"
#include "rows_select.hpp"
#include "wave_scan.hpp"

namespace mbrwt {

// ------------------------------------------------------------------------
// queries
// ------------------------------------------------------------------------
namespace {

// rwt_walk with its pending frames {first entry, mask} in a per-lane LDS
// stack (stk[128 k], stk[128 k + 64], k < lim <= kRowsMaxHeight: the tree's
// height) instead
// of registers: the compaction kernel walks direct tiles with it, so its
// register budget (and occupancy) stays that of its copy loop
template <class MaskFn, class LeafFn>
__device__ bool rwt_walk_lds(const uint32_t *table, MaskFn mask, LeafFn leaf, AS_LDS uint32_t *stk, uint32_t lim) {
    const uint32_t nI = table[0], nE = table[1];
    const uint32_t *ntab = table + 4;
    const uint32_t *etab = ntab + nI;
    uint32_t nw = ntab[0];
    uint32_t a = nw >> 24;
    uint32_t m = (uint32_t)mask(a);  // (arity <= 16 here: wide trees take rwt_walk)
    uint32_t first = nw & 0xFFFFFFu;
    uint32_t sp = 0;
    bool ok = true;
    while (true) {
        if (!m) {
            if (!sp) break;
            --sp;
            first = stk[128 * sp];
            m = stk[128 * sp + 64];
            continue;
        }
        const uint32_t c = (uint32_t)__builtin_ctz(m);
        m &= m - 1;
        if (first + c >= nE) {
            ok = false;
            break;
        }
        const uint32_t e = etab[first + c];
        if (e & 0x80000000u) {
            leaf(e & 0x7FFFFFFFu);
            continue;
        }
        if (e >= nI || (m && sp == lim)) {
            ok = false;
            break;
        }
        if (m) {  // (the push before the child's mask read: rwt_walk)
            stk[128 * sp] = first;
            stk[128 * sp + 64] = m;
            ++sp;
        }
        nw = ntab[e];
        a = nw >> 24;
        m = (uint32_t)mask(a);
        first = nw & 0xFFFFFFu;
    }
    return ok;
}

// walk families of k_traverse_rows (RowsImage::walk)
enum : uint32_t { WALK_GENERAL = 0, WALK_MASK1 = 1, WALK_ODOMETER = 2, WALK_TREE_ODOMETER = 3 };

struct RowsParams {
    const uint64_t *rows;
    uint64_t n;
    uint64_t num_rows;
    uint64_t blocks, spill, magic;
    uint32_t S;
    uint32_t table_words;
    const uint32_t *table;        // RWT2
    uint32_t C;                   // labels per tile region (multiple of 64)
    uint8_t *temp;                // tiles x (128 + 2 C) bytes: u16 counts[64], u16 labels[C]
    uint32_t *tile_counts;        // [tiles] labels (bit 31: the tile goes to the direct pass)
    unsigned long long *scalars;  // the kernel's counters: [2] error flags (bit 0: row out of range)
    unsigned long long *status;   // the call's {needed, status, sticky}: status is reset here
    uint32_t uni;                 // the odometer: the tree's internal levels K (1..5)
    uint32_t path_walk;           // the odometer over the path table when the tree has one
    uint32_t stk_words;           // per-lane LDS stack slots (general walks)
    uint32_t frames;              // the tree odometer: internal levels on the longest path (1..kRowsOdoLevels)
    uint32_t mask1;               // every mask one byte
    const uint32_t *classes;      // record classes: the packed class index (null: none; rows_class.hip)
    uint32_t class_bits;
};

// a u16 store at a 32-bit byte offset from a wave-uniform base (the saddr +
// 32-bit voffset form of global_store_short: no 64-bit address arithmetic)
__device__ __forceinline__ void st16(uint16_t *base, uint32_t idx, uint32_t v) {
    *(AS_GLOBAL uint16_t *)((uintptr_t)base + (uint64_t)(idx * 2u)) = (uint16_t)v;
}

// The general walk (masks of 1 or 2 bytes: arity <= 16): one lock-step
// iteration per reached child, the top frame in two registers, the pending
// frames in a per-lane LDS stack (one write / one read per push / pop), one
// emission loop for leaves and leaf parents, mask bytes read as two bytes
// masked by the arity.
// a terminal entry's label for bit `bit` of its mask: a leaf's column (bit
// 0), a leaf parent's first column + bit, or entry `bit` of its column list
__device__ __forceinline__ uint32_t term_label(uint32_t e, const AS_LDS uint16_t *lst, uint32_t bit) {
    const uint32_t i = (e & 0xFFFFu) + bit;
    return ((e >> 29) & 1u) ? (uint32_t)lst[i] : i;
}

__device__ __forceinline__ void rows_walk4(const AS_LDS uint8_t *pb, uint32_t o, bool live, uint32_t root,
                                           const AS_LDS uint32_t *ent, const AS_LDS uint16_t *lst,
                                           AS_LDS uint32_t *stk, uint16_t *out, uint32_t pos) {
    const uint32_t ra = (root >> 16) & 0x7Fu;
    const uint32_t rm = ((uint32_t)pb[o] | ((uint32_t)pb[o + 1] << 8)) & ((1u << ra) - 1u);
    o += ra > 8 ? 2u : 1u;
    if ((root >> 30) == 3u) {  // a one-level tree: the root is a leaf parent
        if (live)
            for (uint32_t x = rm; x; x &= x - 1) st16(out, pos++, (root & 0xFFFFu) + (uint32_t)__builtin_ctz(x));
        return;
    }
    uint32_t f = root & 0xFFFFu, m = live ? rm : 0u;
    uint32_t sp = 0;
    while (__any(m != 0)) {
        const bool act = m != 0;
        const uint32_t c = (uint32_t)__builtin_ctz(m | 0x10000u);
        m &= m - 1;
        const uint32_t e = ent[act ? f + c : 0u];
        const uint32_t a = act ? (e >> 16) & 0x7Fu : 0u;  // leaf: 0
        const uint32_t mw = ((uint32_t)pb[o] | ((uint32_t)pb[o + 1] << 8)) & ((1u << a) - 1u);
        o += a ? (a > 8 ? 2u : 1u) : 0u;
        const bool inner = act && (e >> 31) == 0u;
        uint32_t x = (act && (e >> 31)) ? (a ? mw : 1u) : 0u;  // a leaf: its column; a leaf parent: its set children
        const uint32_t base = e & 0xFFFFu;
        for (; x; x &= x - 1) st16(out, pos++, term_label(e, lst, (uint32_t)__builtin_ctz(x)));
        if (inner && m) {
            stk[sp * 64] = f | (m << 16);
            ++sp;
        }
        if (inner) {
            f = base;
            m = mw;
        }
        if (act && !m && sp) {
            --sp;
            const uint32_t w = stk[sp * 64];
            f = w & 0xFFFFu;
            m = w >> 16;
        }
    }
}

// The walk when every mask is one byte (arity <= 8 everywhere): rows_walk4's
// steps in about half the vector instructions -- the record cursor is an LDS
// byte address, the stack pointer a per-lane LDS address (slot stride 256
// bytes), finished lanes leave the loop (exec mask) instead of being carried
// by selects, and leaves / leaf parents and internal children take
// exec-masked branches.  Labels are stored one by one into the tile's temp
// region (global u16).
__device__ __forceinline__ void rows_walk6(const AS_LDS uint8_t *pb, uint32_t o, bool live, uint32_t root,
                                           const AS_LDS uint32_t *ent, const AS_LDS uint16_t *lst,
                                           AS_LDS uint32_t *stk, AS_GLOBAL uint16_t *out, uint32_t pos) {
    const AS_LDS uint8_t *rc = pb + o;  // record cursor
    const uint32_t rm = rc[0];
    ++rc;
    if ((root >> 30) == 3u) {  // a one-level tree: the root is a leaf parent
        if (live)
            for (uint32_t x = rm; x; x &= x - 1) out[pos++] = (uint16_t)((root & 0xFFFFu) + (uint32_t)__builtin_ctz(x));
        return;
    }
    if (!live) return;
    uint32_t f = root & 0xFFFFu, m = rm;
    AS_LDS uint32_t *sp = stk;
    uint32_t ob = pos * 2u;  // byte offset of the next label
    while (m != 0u) {
        const uint32_t c = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        const uint32_t e = ent[f + c];
        const uint32_t mw = *rc;
        if ((int32_t)e < 0) {  // a leaf (its column) or a leaf parent (its set children)
            const bool lp = (e >> 30) & 1u;
            uint32_t x = lp ? mw : 1u;
            rc += lp ? 1 : 0;
            do {
                *(AS_GLOBAL uint16_t *)((uintptr_t)out + ob) = (uint16_t)term_label(e, lst, (uint32_t)__builtin_ctz(x));
                ob += 2u;
                x &= x - 1u;
            } while (x);
        } else {  // an internal child: push the rest of this frame, descend
            if (m) {
                *sp = f | (m << 16);
                sp += 64;
            }
            f = e & 0xFFFFu;
            m = mw;
            ++rc;
        }
        if (m == 0u && sp != stk) {
            sp -= 64;
            const uint32_t w = *sp;
            f = w & 0xFFFFu;
            m = w >> 16;
        }
    }
}

// The odometer walk (uniform trees: every root-to-leaf path crosses K
// internal levels and then a leaf parent with consecutive columns, one-byte
// masks -- the basic partitioner's trees without singleton groups, i.e.
// C2-C4).  rows_walk6 spends one lock-step iteration per reached node (19.3
// per C4 row, 34 per 64-row tile in lock step); here one iteration reaches
// the NEXT LEAF PARENT of the row in pre-order (7.9 per C4 row, 15 per tile):
// the remaining-children masks r[0..K-1] of the current path form an
// odometer -- level k takes its next child when every level below it is
// exhausted (top-down, so a level refilled in this iteration feeds the level
// under it), reading that child's mask as the record's next byte, which is
// exactly BRWT::get_row's pre-order (BRWT.cpp:43-51); the leaf-parent step
// then reads the leaf mask and stores base + bit for its set bits into the
// wave's LDS label stage.  No stack, no per-lane frame state beyond 2K
// registers.
template <int K>
__device__ __forceinline__ void rows_walk_uni(const AS_LDS uint8_t *pb, uint32_t o, bool live, uint32_t root,
                                              const AS_LDS uint32_t *ent, AS_LDS uint16_t *out, uint32_t pos) {
    const AS_LDS uint8_t *rc = pb + o;  // record cursor
    uint32_t r[K], f[K];
    f[0] = root & 0xFFFFu;
    r[0] = live ? (uint32_t)rc[0] : 0u;
    ++rc;
#pragma unroll
    for (int k = 1; k < K; ++k) r[k] = f[k] = 0u;
    uint32_t ob = pos * 2u;  // byte offset of the next label
    while (true) {
        uint32_t any = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) any |= r[k];
        if (!any) break;
        bool nd[K];  // nd[k]: levels k..K-1 are exhausted
        nd[K - 1] = r[K - 1] == 0u;
#pragma unroll
        for (int k = K - 2; k >= 1; --k) nd[k] = nd[k + 1] && r[k] == 0u;
#pragma unroll
        for (int k = 1; k < K; ++k) {
            if (nd[k]) {
                const uint32_t c = (uint32_t)__builtin_ctz(r[k - 1]);
                r[k - 1] &= r[k - 1] - 1u;
                f[k] = ent[f[k - 1] + c] & 0xFFFFu;
                r[k] = *rc;
                ++rc;
            }
        }
        const uint32_t c = (uint32_t)__builtin_ctz(r[K - 1]);
        r[K - 1] &= r[K - 1] - 1u;
        const uint32_t base = ent[f[K - 1] + c] & 0xFFFFu;  // a leaf parent: its first column
        uint32_t x = *rc;
        ++rc;
        do {
            *(AS_LDS uint16_t *)((uintptr_t)out + ob) = (uint16_t)(base + (uint32_t)__builtin_ctz(x));
            ob += 2u;
            x &= x - 1u;
        } while (x);
    }
}

// The odometer over the PATH TABLE (append_path_table): the same lock-step
// iteration per reached leaf parent as rows_walk_uni, but a level keeps the
// path index of its node instead of its table entry, so refilling a level is
// register arithmetic (no dependent LDS read per level) and the leaf
// parent's first column is ONE LDS read; the level refills are selects (at
// the Kingsford shape nearly every iteration refills the level above the
// leaf parents in some lane, so branches only added exec-mask work), and a
// leaf parent's first label is stored unconditionally (1.01 labels per leaf
// parent at C4), the loop only for the rest.
// a * b + c in one full-rate v_mad_u32_u24 (a, b < 2^24; b wave-uniform):
// the compiler folds __umul24(a, b) + c into the quarter-rate 64-bit
// v_mad_u64_u32, so the instruction is named here
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}

// a record's next mask at cursor c (bytes: byte c; nibble codes, r06:
// nibble c, rows_record.hpp RecMasks) and the cursor's advance.  The nibble
// form reads the two bytes the code can span (LDS: a read past the record
// stays inside the wave's slots)
struct MaskAt {
    uint32_t m, adv;
};
template <bool NIB>
__device__ __forceinline__ MaskAt rec_mask_at(const AS_LDS uint8_t *rec, uint32_t c) {
    if constexpr (!NIB) {
        return MaskAt{(uint32_t)rec[c], 1u};
    } else {
        // (two byte reads: one unaligned 4-byte ds_read_b32 instead took the
        // C4 kernel from 0.30 to 0.43 ms, profiles/r06/v04_nibble_codes)
        const uint32_t i = c >> 1;
        const uint32_t w = ((uint32_t)rec[i] | ((uint32_t)rec[i + 1] << 8)) >> ((c & 1u) * 4u);
        const uint32_t v = w & 15u;
        return v < 8u ? MaskAt{1u << v, 1u} : MaskAt{(w >> 4) & 0xFFu, 3u};
    }
}

template <int K, bool LIN, bool NIB>
__device__ __forceinline__ void rows_walk_path(const AS_LDS uint8_t *pb, uint32_t o, bool live,
                                               const AS_LDS uint16_t *ptab, uint32_t A, AS_LDS uint16_t *out,
                                               uint32_t pos) {
    const AS_LDS uint8_t *rec = pb + o;  // the record's masks
    uint32_t rc = 0;                     // cursor (bytes or nibbles)
    uint32_t r[K], idx[K];
    {
        const MaskAt m0 = rec_mask_at<NIB>(rec, 0);
        r[0] = live ? m0.m : 0u;
        rc = m0.adv;
    }
    idx[0] = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) r[k] = idx[k] = 0u;
    uint32_t ob = pos * 2u;  // byte offset of the next label
    while (true) {
        uint32_t any = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) any |= r[k];
        if (!any) break;
        bool nd[K];  // nd[k]: levels k..K-1 are exhausted
        nd[K - 1] = r[K - 1] == 0u;
#pragma unroll
        for (int k = K - 2; k >= 1; --k) nd[k] = nd[k + 1] && r[k] == 0u;
#pragma unroll
        for (int k = 1; k < K; ++k) {
            const uint32_t c = (uint32_t)__builtin_ctz(r[k - 1]);
            const MaskAt bm = rec_mask_at<NIB>(rec, rc);
            const uint32_t b = bm.m;
            // the node at level k is child c of the level-(k-1) node: A_{k-1}
            // (the largest arity at level k-1) scales the parent's index
            const uint32_t Ak = k >= 2 ? (A >> (4 * (k - 2))) & 0xFu : 0u;  // (wave-uniform)
            // (24-bit multiplies: v_mad_u32_u24 issues at full rate, the
            // 32-bit v_mad_u64_u32 the compiler picks otherwise does not)
            const uint32_t ni = k == 1 ? c : mad_u24(idx[k - 1], Ak, c);
            idx[k] = nd[k] ? ni : idx[k];
            r[k - 1] = nd[k] ? (r[k - 1] & (r[k - 1] - 1u)) : r[k - 1];
            r[k] = nd[k] ? b : r[k];
            rc += nd[k] ? bm.adv : 0u;
        }
        const uint32_t c = (uint32_t)__builtin_ctz(r[K - 1]);
        r[K - 1] &= r[K - 1] - 1u;
        const uint32_t AK = K > 1 ? (A >> (4 * (K > 1 ? K - 2 : 0))) & 0xFu : 0u;
        const uint32_t pidx = K > 1 ? mad_u24(idx[K - 1], AK, c) : c;
        // the leaf parent's first column: computed on a linear path table (no
        // LDS round trip per iteration), else read
        const uint32_t base = LIN ? pidx << ((A >> 24) & 0x1Fu) : (uint32_t)ptab[pidx];
        const MaskAt xm = rec_mask_at<NIB>(rec, rc);
        uint32_t x = xm.m;
        rc += xm.adv;
        *(AS_LDS uint16_t *)((uintptr_t)out + ob) = (uint16_t)(base + (uint32_t)__builtin_ctz(x));
        ob += 2u;
        x &= x - 1u;
        while (x) {
            *(AS_LDS uint16_t *)((uintptr_t)out + ob) = (uint16_t)(base + (uint32_t)__builtin_ctz(x));
            ob += 2u;
            x &= x - 1u;
        }
    }
}

// The odometer for ANY tree shape (r04; the greedy + relax trees of the
// reference's production build: leaf parents at different depths, leaf
// parents whose columns are not consecutive -- walked as internal nodes with
// leaf children -- and masks of up to 16 bits).  As in rows_walk_uni one
// lock-step iteration reaches the row's next TERMINAL in pre-order (a leaf
// parent with consecutive columns, or a leaf): the deepest level with a
// remaining child takes it, and while that child is internal the walk
// descends in the same iteration, each level reading its node's mask as the
// record's next byte(s) -- BRWT::get_row's pre-order (BRWT.cpp:43-51), the
// record format unchanged.  Levels are unrolled and predicated: a level no
// lane of the wave needs costs a skipped branch.  State: 2 KM registers.
template <int KM, bool M1, bool WIDE = false>
__device__ __forceinline__ void rows_walk_tree(const AS_LDS uint8_t *pb, uint32_t o, bool live, uint32_t root,
                                               const AS_LDS uint32_t *ent, const AS_LDS uint16_t *lst,
                                               AS_LDS uint16_t *out, uint32_t pos) {
    // masks: one byte (M1), up to two (arity <= 16), or (WIDE, r06) up to
    // eight -- arity <= 64, one byte per 8 children
    using MT = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
    const AS_LDS uint8_t *rc = pb + o;  // record cursor
    // a node's mask of arity a at the cursor; its width in bytes
    auto mask_at = [&](uint32_t a) -> MT {
        MT m = rc[0];
        if constexpr (WIDE) {
            for (uint32_t k = 8; k < a; k += 8) m |= (MT)rc[k >> 3] << k;  // (rare: a loop, not reads in every lane)
            return a >= 64 ? m : (m & (((MT)1 << a) - 1u));
        } else {
            if (!M1 && a > 8) m |= (uint32_t)rc[1] << 8;  // (rare: a branch, not a read in every lane)
            return m & ((1u << a) - 1u);
        }
    };
    auto width = [](uint32_t a) -> uint32_t { return WIDE ? (a + 7u) >> 3 : (M1 || a <= 8) ? 1u : 2u; };
    uint32_t ob = pos * 2u;  // byte offset of the next label
    auto ctz = [](MT x) -> uint32_t { return WIDE ? (uint32_t)__builtin_ctzll((uint64_t)x) : (uint32_t)__builtin_ctz((uint32_t)x); };
    auto emit = [&](uint32_t e, MT x) {
        *(AS_LDS uint16_t *)((uintptr_t)out + ob) = (uint16_t)term_label(e, lst, ctz(x));
        ob += 2u;
        x &= x - 1u;
        while (x) {
            *(AS_LDS uint16_t *)((uintptr_t)out + ob) = (uint16_t)term_label(e, lst, ctz(x));
            ob += 2u;
            x &= x - 1u;
        }
    };
    const uint32_t ra = (root >> 16) & 0x7Fu;
    if ((root >> 30) == 3u) {  // a one-level tree: the root is a leaf parent
        if (live) {
            const MT x = mask_at(ra);
            if (x) emit(root, x);
        }
        return;
    }
    MT r[KM];
    uint32_t f[KM];
    r[0] = live ? mask_at(ra) : (MT)0;
    f[0] = root & 0xFFFFu;
    rc += width(ra);
#pragma unroll
    for (int k = 1; k < KM; ++k) {
        r[k] = 0;
        f[k] = 0u;
    }
    while (true) {
        uint32_t nz = 0;
#pragma unroll
        for (int k = 0; k < KM; ++k) nz |= (r[k] != 0 ? 1u : 0u) << k;
        if (!nz) break;
        const uint32_t ks = 31u - (uint32_t)__builtin_clz(nz);  // the deepest level with a child left
        bool go = true;
        uint32_t term = 0;
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (go && (uint32_t)k >= ks) {
                const uint32_t c = ctz(r[k]);
                r[k] &= r[k] - 1u;
                const uint32_t e = ent[f[k] + c];
                if ((int32_t)e >= 0) {  // an internal child: its mask, one level down
                    const uint32_t a = (e >> 16) & 0x7Fu;
                    const MT m = mask_at(a);
                    rc += width(a);
                    if (k + 1 < KM) {
                        r[k + 1] = m;
                        f[k + 1] = e & 0xFFFFu;
                    }
                } else {
                    term = e;
                    go = false;
                }
            }
        }
        // the terminal: a leaf parent (its set children) or a leaf (its column)
        MT x = 1u;
        if ((term >> 30) == 3u) {
            const uint32_t a = (term >> 16) & 0x7Fu;
            x = mask_at(a);
            rc += width(a);
        }
        emit(term, x);
    }
}

// The walk of a TERMINAL record (r06, rows_record.hpp term_walk): no tree
// to walk -- each field names a leaf parent (its children mask beside) or a
// leaf, in pre-order, so a lane reads its fields one after the other (two
// aligned LDS words and a funnel shift per field) until its row's count of
// labels is out.  The TT table is in LDS: hdr = its word 0, ent its entries,
// lst its column lists.
__device__ __forceinline__ void rows_walk_terms(const AS_LDS uint8_t *pb, uint32_t o, bool live, uint32_t cnt,
                                                uint32_t hdr, const AS_LDS uint32_t *ent, const AS_LDS uint16_t *lst,
                                                AS_LDS uint16_t *out, uint32_t pos) {
    const uint32_t w = hdr & 0xFFu, ib = (hdr >> 8) & 0xFFu;
    const uint32_t fmask = (1u << w) - 1u, imask = (1u << ib) - 1u;
    const uint32_t a0 = (uint32_t)(uintptr_t)(pb + o);
    const AS_LDS uint32_t *wp = (const AS_LDS uint32_t *)(uintptr_t)(a0 & ~3u);
    uint32_t bit = 8u * (a0 & 3u);
    uint32_t left = live ? cnt : 0u;
    uint32_t ob = pos * 2u;  // byte offset of the next label
    // (fixed-width fields: the next field's words are read before this
    // field's entry and labels, off the dependency chain)
    uint32_t lo = 0, hi = 0;
    if (left) {
        lo = wp[bit >> 5];
        hi = wp[(bit >> 5) + 1];
    }
    while (left) {
        const uint32_t f = __builtin_amdgcn_alignbit(hi, lo, bit & 31u) & fmask;
        bit += w;
        lo = wp[bit >> 5];
        hi = wp[(bit >> 5) + 1];
        const uint32_t e = ent[f & imask];
        uint32_t x = (e >> 30) == 3u ? (f >> ib) : 1u;  // a leaf parent: its set children; a leaf: itself
        x = x ? x : 1u;  // (a corrupt field: one label, so the loop still ends)
        do {
            *(AS_LDS uint16_t *)((uintptr_t)out + ob) = (uint16_t)term_label(e, lst, (uint32_t)__builtin_ctz(x));
            ob += 2u;
            x &= x - 1u;
            --left;
        } while (x && left);
    }
}

// Tiles per wave (r05).  A persistent grid (every wave a fixed share of the
// tiles) lasts as long as its slowest wave, and its waves are not equally
// fast: the workgroups dispatched last lose issue arbitration by age (per-wave
// phase stamps at C4: the third workgroup of each CU took 27.5k cycles per
// tile against 22.3k for the first, lifetimes 396k..623k cycles around a mean
// of 507k; profiles/r05/v03_balance).  A grid of one tile per wave lets the
// dispatcher refill each CU as its waves finish: 0.263-0.271 ms against
// 0.280-0.284 ms per 8 M rows on the same boxes.  Rejected (same boxes):
// claiming the second half of the tiles from per-XCD atomic counters (0.316:
// the claims' returns sit in the waves' vmcnt queue ahead of their block
// loads), s_setprio for the later workgroups (0.2855), and requesting the
// next tile's blocks before walking this one (register prefetch with the
// spill reloads issued first: 0.2865 persistent, 0.2775 at 4 tiles per wave).
// (The r05 A/B variants of this kernel -- phase stamps, gather-only, no-walk,
// no-store, cache-resident blocks -- were retired in r06; their results are
// in profiles/r05 and DESIGN.md §16.)
constexpr uint32_t kRowsTilesPerWave = 1;

// k_traverse_rows: one wave per tile of 64 query rows (file comment).
// B: block bytes; WPB: waves per workgroup (the RWT2 table is staged once per
// workgroup); WALK: the walk family.  (r06: a one-pass form that wrote the
// CSR itself, its place found by a decoupled look-back, measured 0.44-0.48
// against 0.33 ms per C4 step and was retired: profiles/r06/v01_one_pass.)
// VAR: the record variant -- 0 byte masks, VAR_NIB nibble codes (the path
// odometer), VAR_WIDE masks of up to 64 bits (the tree odometer, r06)
enum : uint32_t { VAR_BYTE = 0, VAR_NIB = 1, VAR_WIDE = 2, VAR_TERM = 3 };
template <int B, int WPB, bool NT, uint32_t WALK, uint32_t VAR = VAR_BYTE>
__global__ __launch_bounds__(64 * WPB) void k_traverse_rows(RowsParams p) {
    constexpr bool NIB = VAR == VAR_NIB;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_rows[];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t ntiles = (p.n + 63) / 64;
    const uint64_t tstride = (uint64_t)gridDim.x * WPB;  // (one tile per wave unless the grid is capped)
    uint64_t t = (uint64_t)blockIdx.x * WPB + wv;
    uint64_t row_n = 0;  // the row of this lane in the wave's next tile (its load overlaps the table's)
    if (t < ntiles && t * 64 + lane < p.n) row_n = gld(p.rows + t * 64 + lane);
    for (uint32_t i = threadIdx.x; i < p.table_words; i += blockDim.x) lds_rows[i] = gld(p.table + i);
    if (blockIdx.x == 0 && threadIdx.x == 0) p.status[1] = MBRWT_OK;  // k_compact_tiles raises it
    __syncthreads();
    const uint32_t root = __builtin_amdgcn_readfirstlane(lds_rows[0]);
    const AS_LDS uint32_t *ent = (const AS_LDS uint32_t *)lds_rows + 4;
    // the leaf parents' column lists after the entries
    const AS_LDS uint16_t *lst = (const AS_LDS uint16_t *)(ent + __builtin_amdgcn_readfirstlane(lds_rows[1]));
    // the path table of a uniform tree (append_path_table; 0: none)
    const uint32_t ptw = p.path_walk ? __builtin_amdgcn_readfirstlane(lds_rows[3]) : 0u;
    const uint32_t pA = ptw ? __builtin_amdgcn_readfirstlane(lds_rows[ptw]) : 0u;
    const uint32_t C = p.C;
    // a row's block at a stride of B + 4 bytes: lanes reading their records
    // at similar offsets hit different LDS banks (a B-byte stride puts every
    // other lane in the same bank)
    constexpr uint32_t PB = B + 4;
    AS_LDS uint8_t *wb = (AS_LDS uint8_t *)(lds_rows + ((p.table_words + 3) & ~3u)) +
                         wv * (64u * PB + 256u * p.stk_words + (WALK >= WALK_ODOMETER ? 2u * C : 0u));
    AS_LDS uint8_t *mine = wb + lane * PB;
    AS_LDS uint32_t *stk = (AS_LDS uint32_t *)(wb + 64u * PB) + lane;
    constexpr uint32_t LPB = B / 16, RPI = 64 / LPB;
    const uint32_t S = p.S;
    // a tile's 64 blocks as coalesced quarters: load k brings rows RPI k ..
    // RPI k + RPI - 1, lane L its 16 bytes L % LPB (row addresses by __shfl)
    auto issue_blocks = [&](uint64_t addr, u32x4_t (&qq)[LPB]) {
#pragma unroll
        for (uint32_t k = 0; k < LPB; ++k) {
            const int src = (int)(RPI * k + lane / LPB);
            const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)addr, src, 64);
            const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(addr >> 32), src, 64);
            qq[k] = gld_at_nt<u32x4_t, NT>((((uint64_t)hi << 32) | lo) + 16u * (lane % LPB));
        }
    };
    auto block_of = [&](uint64_t row, bool ok) -> uint64_t { return ok ? rows_block(row, S, p.magic) : 0; };
    u32x4_t q[LPB];
    for (uint64_t tn; t < ntiles; t = tn) {
        const uint64_t r0 = t * 64;
        const uint32_t nr = (uint32_t)(p.n - r0 < 64 ? p.n - r0 : 64);
        const uint64_t row = row_n;
        tn = t + tstride;
        if (tn < ntiles && tn * 64 + lane < p.n) row_n = gld(p.rows + tn * 64 + lane);
        const bool valid = lane < nr && row < p.num_rows;
        if (lane < nr && !valid) atomicOr(&p.scalars[2], 1ull);
        // record classes: the row's class is its record's row in the
        // dictionary (S = 1); the class index is the random HBM read, the
        // dictionary's blocks mostly cache hits
        const uint64_t rec_row = (p.classes && valid) ? class_field(p.classes, p.class_bits, row) : row;
        const uint64_t b = block_of(rec_row, valid);
        const uint32_t sub = (uint32_t)(rec_row - b * S);
        issue_blocks(p.blocks + b * B, q);
#pragma unroll
        for (uint32_t k = 0; k < LPB; ++k) {
            AS_LDS uint32_t *d = (AS_LDS uint32_t *)(wb + (RPI * k + lane / LPB) * PB + 16u * (lane % LPB));
            d[0] = q[k].x;
            d[1] = q[k].y;
            d[2] = q[k].z;
            d[3] = q[k].w;
        }
        wave_sync();
        uint32_t cnt = 0, o = 0;
        bool spl = false;
        if (valid) {
            const uint32_t e = mine[sub];
            o = e & 0x7Fu;
            spl = (e & 0x80u) != 0;
            cnt = mine[o];
            ++o;
        }
        bool lng = false;
        // spilled rows: the entry (<= B bytes of it) replaces the block in
        // the lane's own slot; masks from byte 8
        const bool any_spl = __any(spl);
        u32x4_t sq[LPB];
        if (any_spl && spl) {
            const uint32_t idx = (uint32_t)mine[o] | ((uint32_t)mine[o + 1] << 8) | ((uint32_t)mine[o + 2] << 16) |
                                 ((uint32_t)mine[o + 3] << 24);
            const uint64_t sa = p.spill + (uint64_t)idx * 16;
            *(AS_LDS uint32_t *)(mine + B) = idx;  // (the slot's pad word: a long record's copy below)
#pragma unroll
            for (uint32_t k = 0; k < LPB; ++k) sq[k] = gld_at<u32x4_t>(sa + 16u * k);
        }
        if (any_spl && spl) {
#pragma unroll
            for (uint32_t k = 0; k < LPB; ++k) {
                AS_LDS uint32_t *d = (AS_LDS uint32_t *)mine + 4 * k;
                d[0] = sq[k].x;
                d[1] = sq[k].y;
                d[2] = sq[k].z;
                d[3] = sq[k].w;
            }
            cnt = sq[0].x;
            lng = 8 + sq[0].y > B;
            o = 8;
        }
        const uint32_t x = wave_incl_sum(cnt);
        const uint32_t total = __builtin_amdgcn_readlane(x, 63);
        const uint32_t pos = x - cnt;
        // a tile whose labels exceed its region is walked by k_compact_tiles
        // from global memory; so is a record longer than a block (its count
        // flagged with bit 15; its labels' places in the tile are kept)
        const bool direct = total > C;
        // the lane's record in LDS: its block slot, or (r05) for a record
        // longer than a block, a copy of its whole spill entry in the free tail
        // of the wave's label stage (the tile's labels take its first 2 total
        // bytes), so the odometers walk it here instead of walking it byte by
        // byte from global memory (the greedy + relax shape: 0.13 % of rows,
        // 8 % of tiles; its compaction took 266 us of a 0.76 ms step,
        // profiles/r05)
        const AS_LDS uint8_t *rec = mine;
        AS_LDS uint16_t *stage = (AS_LDS uint16_t *)(wb + 64u * PB + 256u * p.stk_words);
        if constexpr (WALK == WALK_ODOMETER || WALK == WALK_TREE_ODOMETER) {
            if (!direct && __any(lng)) {
                // each long row's entry (16-byte chunks) below the previous
                // one's from the stage's end; all of them, or none
                // (the entry's mask bytes and index from the lane's slot)
                const uint32_t need = lng ? ((8u + *(const AS_LDS uint32_t *)(mine + 4) + 15u) & ~15u) : 0u;
                const uint32_t incl = wave_incl_sum(need);
                if (2u * total + __builtin_amdgcn_readlane(incl, 63) <= 2u * C) {
                    AS_LDS uint8_t *stg = (AS_LDS uint8_t *)stage + 2u * C - incl;
                    if (lng) {
                        const uint64_t sa = p.spill + (uint64_t)*(const AS_LDS uint32_t *)(mine + B) * 16;
#pragma unroll 1
                        for (uint32_t b = 0; b < need; b += 16u) *(AS_LDS u32x4_t *)(stg + b) = gld_at<u32x4_t>(sa + b);
                        rec = stg;  // masks from byte 8, as in a spilled row's slot
                        lng = false;
                    }
                    wave_sync();
                }
            }
        }
        const bool has_long = __any(lng);
        uint8_t *treg = p.temp + t * (uint64_t)(128 + 2 * C);
        // (non-temporal: the temp region is read once, by k_compact_tiles;
        // the stores then disturb the random block reads less -- C4 kernel
        // 0.262 -> 0.255 ms, step 0.348 -> 0.333 ms; the same hint on the
        // compaction's CSR stores made the two-stream step slower again,
        // 0.344 ms: profiles/r05/v21_temp_stores)
        if (lane < nr)
            __builtin_nontemporal_store((uint16_t)(cnt | (lng ? 0x8000u : 0u)),
                                        (AS_GLOBAL uint16_t *)(uintptr_t)(reinterpret_cast<uint16_t *>(treg) + lane));
        if (!direct) {
            const bool live = valid && cnt > 0 && !lng;
            if constexpr (WALK == WALK_ODOMETER || WALK == WALK_TREE_ODOMETER) {
                // the odometer into the wave's LDS label stage, then the
                // tile's labels as 16-byte vector stores (a few wide stores
                // instead of one scattered 2-byte store per label: the r03
                // SQ/TA counters showed the texture-address unit as the
                // busiest unit)
                if constexpr (WALK == WALK_TREE_ODOMETER && VAR == VAR_TERM) {
                    rows_walk_terms(rec, o, live, cnt, root, ent, lst, stage, pos);
                } else if constexpr (WALK == WALK_TREE_ODOMETER) {
#define MBRWT_TREE_CASE(K)                                                              \
    case K:                                                                             \
        if constexpr (VAR == VAR_WIDE)                                                  \
            rows_walk_tree<K, false, true>(rec, o, live, root, ent, lst, stage, pos);   \
        else if (p.mask1)                                                               \
            rows_walk_tree<K, true>(rec, o, live, root, ent, lst, stage, pos);          \
        else                                                                            \
            rows_walk_tree<K, false>(rec, o, live, root, ent, lst, stage, pos);         \
        break;
                    switch (p.frames) {
                        MBRWT_TREE_CASE(1)
                        MBRWT_TREE_CASE(2)
                        MBRWT_TREE_CASE(3)
                        MBRWT_TREE_CASE(4)
                        MBRWT_TREE_CASE(5)
                        MBRWT_TREE_CASE(6)
                        MBRWT_TREE_CASE(7)
                        default:
                            if constexpr (VAR == VAR_WIDE)
                                rows_walk_tree<8, false, true>(rec, o, live, root, ent, lst, stage, pos);
                            else
                                rows_walk_tree<8, false>(rec, o, live, root, ent, lst, stage, pos);
                            break;
                    }
#undef MBRWT_TREE_CASE
                } else if (ptw) {
                    const AS_LDS uint16_t *ptab = (const AS_LDS uint16_t *)((const AS_LDS uint32_t *)lds_rows + ptw + 1);
                    const bool lin = (pA >> 31) != 0u;
#define MBRWT_PATH_CASE(K)                                                      \
    case K:                                                                     \
        if (lin)                                                                \
            rows_walk_path<K, true, NIB>(rec, o, live, ptab, pA, stage, pos);   \
        else                                                                    \
            rows_walk_path<K, false, NIB>(rec, o, live, ptab, pA, stage, pos);  \
        break;
                    switch (p.uni) {
                        MBRWT_PATH_CASE(1)
                        MBRWT_PATH_CASE(2)
                        MBRWT_PATH_CASE(3)
                        MBRWT_PATH_CASE(4)
                        default:
                        MBRWT_PATH_CASE(5)
                    }
#undef MBRWT_PATH_CASE
                } else {
                    switch (p.uni) {
                        case 1: rows_walk_uni<1>(rec, o, live, root, ent, stage, pos); break;
                        case 2: rows_walk_uni<2>(rec, o, live, root, ent, stage, pos); break;
                        case 3: rows_walk_uni<3>(rec, o, live, root, ent, stage, pos); break;
                        case 4: rows_walk_uni<4>(rec, o, live, root, ent, stage, pos); break;
                        default: rows_walk_uni<5>(rec, o, live, root, ent, stage, pos); break;
                    }
                }
                wave_sync();
                // (r05: rounding the copy up to whole 128-byte lines helped
                // plain stores by 1.5 % and non-temporal ones not at all)
                const uint32_t nbytes = total * 2;
                for (uint32_t q2 = lane * 16; q2 < nbytes; q2 += 1024)
                    __builtin_nontemporal_store(*(const AS_LDS u32x4_t *)((const AS_LDS uint8_t *)stage + q2),
                                                (AS_GLOBAL u32x4_t *)(uintptr_t)(treg + 128 + q2));
            } else if constexpr (WALK == WALK_MASK1) {
                rows_walk6(mine, o, live, root, ent, lst, stk,
                           (AS_GLOBAL uint16_t *)reinterpret_cast<uint16_t *>(treg + 128), pos);
            } else {
                rows_walk4(mine, o, live, root, ent, lst, stk, reinterpret_cast<uint16_t *>(treg + 128), pos);
            }
        }
        if (lane == 0) gst(p.tile_counts + t, total | (direct ? 0x80000000u : 0u) | (has_long ? 0x40000000u : 0u));
        wave_sync();  // the slots are reused
    }
}

// tile regions -> CSR: one wave per TPW consecutive tiles (every load of
// the group -- counts, the tile offsets, the first 512 labels of each tile --
// issued before any store, so a wave pays one memory latency for TPW tiles);
// offsets by a wave scan of each tile's counts, labels u16 -> u32.  A direct
// tile (bit 31 of its count: more labels than its region, or a record longer
// than a block) is walked here, one lane per row, from the records in global
// memory straight into the CSR.  Launched before the host knows the total:
// over the capacity it writes no CSR.  The scan is exclusive over the tiles,
// so the batch total is offset + count of the last tile; workgroup 0
// publishes the call's {total, status, sticky bits} (the traversal reset the
// status word; a failed record walk raises it to MBRWT_ERR_DEVICE) and
// clears the traversal's error flags for the next call.
constexpr uint32_t kCompactTpw = 4;
struct CompactParams {
    const uint8_t *temp;
    uint32_t C;
    const uint32_t *tile_counts;
    const uint64_t *tile_offsets;
    uint64_t *offsets;
    void *cols;                   // the CSR's labels: u32, or u16 (k_compact_tiles<WIDE, uint16_t>)
    uint64_t n, cap;
    unsigned long long *scalars;  // the traversal's counters ([2] error flags)
    unsigned long long *status;   // {total, status, sticky}
    const uint64_t *rows;         // the batch (direct tiles)
    const uint32_t *classes;      // record classes (null: none)
    uint32_t class_bits;
    RowsView v;
    const uint32_t *table;        // RWT (direct tiles)
    uint32_t stk_lim;             // walk stack frames (the tree's height; dynamic LDS)
};
// OUT = uint16_t (mbrwt_get_rows16*): the same labels stored as they lie in
// the region, one u16 per lane and store -- a tile's offset has any parity,
// so its destination is aligned to 2 bytes only, and a wider store at either
// end would reach into the neighbouring tile, which another wave writes.
template <bool WIDE, class OUT>
__global__ __launch_bounds__(256) void k_compact_tiles(CompactParams p) {
    extern __shared__ uint32_t cstk[];  // the direct walks' stacks: 4 x 128 x stk_lim words (two per lane and frame)
    const uint64_t n = p.n;
    const uint64_t ntiles = (n + 63) / 64;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t total = gld(p.tile_offsets + ntiles - 1) + (gld(p.tile_counts + ntiles - 1) & 0x3FFFFFFFu);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t err = p.scalars[2];
        p.scalars[2] = 0;
        p.status[0] = total;
        publish_status(p.status, (err & 1) ? MBRWT_ERR_RANGE : total > p.cap ? MBRWT_ERR_CAPACITY : MBRWT_OK);
    }
    if (total > p.cap) return;
    const uint64_t t0 = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * kCompactTpw;
    if (t0 >= ntiles) return;
    const uint32_t C = p.C;
    const uint32_t region = 128 + 2 * C;
    uint32_t tc[kCompactTpw], cnt[kCompactTpw], v[kCompactTpw][8];
    uint64_t base[kCompactTpw];
#pragma unroll
    for (uint32_t k = 0; k < kCompactTpw; ++k) {
        const uint64_t t = t0 + k;
        const bool in = t < ntiles;
        const uint8_t *treg = p.temp + (in ? t : 0) * (uint64_t)region;
        const uint64_t r0 = t * 64;
        tc[k] = in ? gld(p.tile_counts + t) : 0x80000000u;
        base[k] = in ? gld(p.tile_offsets + t) : 0;
        cnt[k] = (in && r0 + lane < n) ? (uint32_t)gld(reinterpret_cast<const uint16_t *>(treg) + lane) : 0u;  // (bit 15: long)
        const uint16_t *lab = reinterpret_cast<const uint16_t *>(treg + 128);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) v[k][j] = gld(lab + lane + 64 * j);  // (C >= 1024: inside the region)
    }
#pragma unroll
    for (uint32_t k = 0; k < kCompactTpw; ++k) {
        const uint64_t t = t0 + k;
        if (t >= ntiles) break;
        const uint64_t r0 = t * 64;
        const uint32_t nr = (uint32_t)(n - r0 < 64 ? n - r0 : 64);
        const uint32_t c = cnt[k] & 0x7FFFu;
        const uint32_t x = wave_incl_sum(c);
        const uint64_t rbase = base[k] + (x - c);
        if (lane < nr) gst(p.offsets + r0 + lane, rbase);
        if (t == ntiles - 1 && lane == nr - 1) gst(p.offsets + n, base[k] + x);
        const uint32_t tot = tc[k] & 0x3FFFFFFFu;
        const uint64_t tb = base[k];
        base[k] = rbase;  // (the walks below: each row's own offset)
        if (tc[k] >> 31) continue;  // a direct tile: walked below, once the copies' registers are free
        OUT *dst = static_cast<OUT *>(p.cols) + tb;
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t i = lane + 64 * j;
            if (i < tot) gst(dst + i, (OUT)v[k][j]);
        }
        const uint16_t *lab = reinterpret_cast<const uint16_t *>(p.temp + t * (uint64_t)region + 128);
        for (uint32_t i0 = 512; i0 < tot; i0 += 512) {
            uint32_t w[8];
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t i = i0 + lane + 64 * j;
                w[j] = i < tot ? (uint32_t)gld(lab + i) : 0u;
            }
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t i = i0 + lane + 64 * j;
                if (i < tot) gst(dst + i, (OUT)w[j]);
            }
        }
    }
    // direct tiles and records longer than a block (rare): one lane per row,
    // the record walked from global memory straight into the CSR at the
    // row's offset (base[k] now) -- over the places the copy above filled
    // for a long record, hence the fence
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
#pragma unroll 1
    for (uint32_t k = 0; k < kCompactTpw; ++k) {
        const uint64_t t = t0 + k;
        if (t >= ntiles || !(tc[k] >> 30)) continue;
        const uint64_t r0 = t * 64;
        const uint32_t nr = (uint32_t)(n - r0 < 64 ? n - r0 : 64);
        const bool walk = (tc[k] >> 31) ? (cnt[k] & 0x7FFFu) != 0 : (cnt[k] >> 15) != 0;
        if (lane < nr && walk) {
            uint64_t row = gld(p.rows + r0 + lane);
            if (p.classes) row = class_field(p.classes, p.class_bits, row);
            uint64_t masks;
            uint32_t count;
            rows_locate(p.v, row, masks, count);  // (count = cnt: rows out of range have none)
            OUT *dst = static_cast<OUT *>(p.cols) + base[k];
            uint32_t j = 0;
            auto put = [&](uint32_t col) {
                if (j < count) gst(dst + j, (OUT)col);
                ++j;
            };
            auto byte = [&](uint32_t o) { return (uint32_t)gld_at<uint8_t>(masks + o); };
            const auto mk = rec_masks(byte, p.v.nib);
            // (masks beyond 16 bits: the frames in registers, not packed in
            // LDS; terminal records: no frames)
            const bool ok = p.v.term ? term_walk(p.table, byte, count, put)
                            : WIDE   ? rwt_walk(p.table, mk, put, [](uint32_t) {})
                                     : rwt_walk_lds(p.table, mk, put,
                                                (AS_LDS uint32_t *)cstk + (threadIdx.x >> 6) * 128 * p.stk_lim + lane,
                                                p.stk_lim);
            if (!ok || j != count) publish_status(p.status, MBRWT_ERR_DEVICE);
        }
    }
}

// point queries: the column among the row's labels (BRWT::get, BRWT.cpp:9-24)
__global__ __launch_bounds__(256) void k_rows_get(RowsView v, const uint32_t *table, const uint64_t *rows,
                                                  const uint64_t *qcols, uint64_t n, uint64_t num_cols, uint8_t *out,
                                                  unsigned long long *scalars) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {
        const uint64_t row = gld(rows + i), col = gld(qcols + i);
        if (row >= v.num_rows || col >= num_cols) {
            atomicOr(&scalars[2], 1ull);
            gst(out + i, (uint8_t)0);
            continue;
        }
        uint64_t masks;
        uint32_t count;
        rows_locate(v, row, masks, count);
        uint32_t hit = 0;
        if (count) (void)record_walk(v, table, masks, count, [&](uint32_t c) { hit |= c == col; }, [](uint32_t) {});
        gst(out + i, (uint8_t)hit);
    }
}

// count_labels (annotate_static.cpp:149-162) and the V / L accounting
// (V = 1 + the arities of the internal nodes the descent
// reaches, i.e. of the record's masks)
template <bool WORK>
__global__ __launch_bounds__(256) void k_rows_count(RowsView v, const uint32_t *table, const uint64_t *rows,
                                                    uint64_t n, unsigned long long *counts,
                                                    unsigned long long *scalars, const uint32_t *wt) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long vis = 0, lab = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {
        const uint64_t row = gld(rows + i);
        if (row >= v.num_rows) {
            atomicOr(&scalars[2], 1ull);
            continue;
        }
        uint64_t masks;
        uint32_t count;
        rows_locate(v, row, masks, count);
        vis += 1;
        if (!count) continue;
        if (WORK && v.term) {  // terminal records: V from the terminals' ancestor chains (WT)
            const uint32_t D = wt[0], nT = wt[1];
            const uint32_t *ids = wt + 4, *ars = ids + (size_t)nT * D, *len = ars + (size_t)nT * D, *own = len + nT;
            uint32_t prev = ~0u;
            (void)term_walk(
                table, [&](uint32_t o) { return (uint32_t)gld_at<uint8_t>(masks + o); }, count,
                [&](uint32_t) { ++lab; },
                [&](uint32_t id) {
                    const uint32_t l = len[id];
                    uint32_t k = 0;
                    if (prev != ~0u) {  // (the chain shared with the previous terminal: counted already)
                        const uint32_t lp = len[prev];
                        while (k < l && k < lp && ids[(size_t)id * D + k] == ids[(size_t)prev * D + k]) ++k;
                    }
                    for (; k < l; ++k) vis += ars[(size_t)id * D + k];
                    vis += own[id];
                    prev = id;
                });
            continue;
        }
        (void)record_walk(
            v, table, masks, count,
            [&](uint32_t c) {
                if constexpr (WORK) ++lab;
                else atomicAdd(counts + c, 1ull);
            },
            [&](uint32_t a) {
                if constexpr (WORK) vis += a;
            });
    }
    if constexpr (WORK) {
        for (int off = 32; off > 0; off >>= 1) {
            vis += __shfl_down(vis, off);
            lab += __shfl_down(lab, off);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&scalars[3], vis);
            atomicAdd(&scalars[4], lab);
        }
    }
}

// get_column over row records: every row whose record holds the column,
// ascending (a select over the row ids; BRWT::get_column, BRWT.cpp:55-85)
struct RowHasColumn {
    RowsView v;
    const uint32_t *table;
    uint32_t col;
    __device__ bool operator()(const uint64_t &row) const {
        uint64_t masks;
        uint32_t count;
        rows_locate(v, row, masks, count);
        if (!count) return false;
        bool hit = false;
        (void)record_walk(v, table, masks, count, [&](uint32_t c) { hit |= c == col; }, [](uint32_t) {});
        return hit;
    }
};


// the context's records (record classes: the dictionary's)
RowsView view_of(const Ctx &c) {
    return rows_view(c.rows, c.rows.classes ? c.rows.num_classes : c.tree.num_rows);
}

using RowsFn = void (*)(RowsParams);
constexpr uint32_t kRowsWpb = 8;
// the tree odometer's wide workgroups: a large walk table (the greedy +
// relax shape's 8.8 KB, staged once per workgroup) leaves room for only two
// 8-wave workgroups per CU (16 waves); two of 11 waves fit (22)
constexpr uint32_t kRowsWpbWide = 11;
template <int B, bool NT>
RowsFn rows_fn_b(uint32_t walk, uint32_t wpb, bool nib, bool wide, bool term) {
    if (term) return k_traverse_rows<B, kRowsWpb, NT, WALK_TREE_ODOMETER, VAR_TERM>;  // (terminal records)
    if (nib) return k_traverse_rows<B, kRowsWpb, NT, WALK_ODOMETER, VAR_NIB>;  // (nibble codes: the path odometer)
    if (wide)  // (masks beyond 16 bits: the tree odometer)
        return wpb == kRowsWpbWide ? k_traverse_rows<B, kRowsWpbWide, NT, WALK_TREE_ODOMETER, VAR_WIDE>
                                   : k_traverse_rows<B, kRowsWpb, NT, WALK_TREE_ODOMETER, VAR_WIDE>;
    if (wpb == kRowsWpbWide) return k_traverse_rows<B, kRowsWpbWide, NT, WALK_TREE_ODOMETER>;
    return walk == WALK_ODOMETER        ? k_traverse_rows<B, kRowsWpb, NT, WALK_ODOMETER>
           : walk == WALK_TREE_ODOMETER ? k_traverse_rows<B, kRowsWpb, NT, WALK_TREE_ODOMETER>
           : walk == WALK_MASK1         ? k_traverse_rows<B, kRowsWpb, NT, WALK_MASK1>
                                        : k_traverse_rows<B, kRowsWpb, NT, WALK_GENERAL>;
}
RowsFn rows_fn(const RowsImage &im, uint32_t walk, uint32_t wpb) {
    const bool nt = im.bytes > (1ull << 30);  // non-temporal block reads for images beyond the caches
    const bool wide = im.max_arity > 16, term = im.term;
    if (im.B == 64)
        return nt ? rows_fn_b<64, true>(walk, wpb, im.nib, wide, term)
                  : rows_fn_b<64, false>(walk, wpb, im.nib, wide, term);
    return nt ? rows_fn_b<128, true>(walk, wpb, im.nib, wide, term)
              : rows_fn_b<128, false>(walk, wpb, im.nib, wide, term);
}
// resident waves per CU with workgroups of w waves: the LDS (160 KiB per CU:
// the table once per workgroup + per_wave bytes per wave) within the 24-wave cap
uint32_t rows_waves_per_cu(size_t table_bytes, size_t per_wave, uint32_t w) {
    const size_t lds = table_bytes + w * per_wave;
    const uint32_t wgs = std::min<uint32_t>((uint32_t)((160u << 10) / std::max<size_t>(1, lds)), 24u / w);
    return wgs * w;
}
// per-lane stack slots of the general walks: the current frame is held in
// registers and only a descent pushes, so at most frames - 1 are pending.
// Exact sizing keeps a workgroup of 8 waves within a quarter of the CU's LDS
// at the Kingsford shape (3 frames: 8 x (4096 + 512) B + the table).
uint32_t rows_stack_words(const RowsImage &im) { return std::max(1u, im.frames ? im.frames - 1 : 1u); }

// labels per tile region: room for the tile's mean + 8 sigma
uint32_t rows_tile_labels(const Ctx &c) {
    const double mean = c.tree.num_rows ? (double)c.tree.num_relations / (double)c.tree.num_rows : 0.0;
    const double need = 64.0 * mean + 8.0 * std::sqrt(64.0 * mean + 1.0) + 64.0;
    uint32_t C = 1024;
    while (C < need && C < 4096) C <<= 1;
    return C;
}

struct MaskTile {
    __host__ __device__ __forceinline__ uint64_t operator()(const uint32_t &x) const { return x & 0x3FFFFFFFu; }
};

}  // namespace

// the walk family of a context's get_rows: the odometer on uniform trees,
// the one-byte-mask walk where every mask is one byte, else the general walk
// (MBRWT_OPT_ROWS_WALK = 6 forces the non-odometer walk: tests)
static uint32_t rows_walk_of(const Ctx &c) {
    const RowsImage &im = c.rows;
    if (im.term) return WALK_TREE_ODOMETER;  // (terminal records: their own walk, in the tree odometer's slot)
    if (im.nib) return WALK_ODOMETER;       // (nibble codes: only the path odometer reads them)
    if (im.max_arity > 16) return WALK_TREE_ODOMETER;  // (masks beyond 16 bits: the tree odometer only)
    if (im.uni && c.rows_walk != 6 && c.rows_walk != 4 && c.rows_walk != 3)
        return WALK_ODOMETER;  // (7: without the path table)
    // (A/B: 6 = rows_walk6 where every mask is one byte, 4 = rows_walk4)
    if (c.rows_walk == 6 && im.mask1) return WALK_MASK1;
    if (c.rows_walk == 4) return WALK_GENERAL;
    if (im.frames >= 1 && im.frames <= kRowsOdoLevels) return WALK_TREE_ODOMETER;
    return im.mask1 ? WALK_MASK1 : WALK_GENERAL;
}

int rows_get_rows(Ctx &c, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets, void *d_cols, uint64_t cap,
                  uint64_t *needed, hipStream_t s, uint64_t *d_status, uint32_t width) {
    const RowsImage &im = c.rows;
    if (n == 0 && d_status) return MBRWT_ERR_UNSUPPORTED;  // (the caller's generic path handles it)
    if (n == 0) {
        MBRWT_HIP(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), s));
        MBRWT_HIP(hipStreamSynchronize(s));
        if (needed) *needed = 0;
        return MBRWT_OK;
    }
    if (im.var) return var_get_rows(c, d_rows, n, d_offsets, d_cols, cap, needed, s, d_status, width);
    if (n > 0x7FFFFFF0ull) {
        set_error("batch larger than 2^31 rows");
        return MBRWT_ERR_UNSUPPORTED;
    }
    int rc;
    const uint32_t C = rows_tile_labels(c);
    const uint64_t nt = (n + 63) / 64;
    const uint64_t region = 128 + 2ull * C;
    const uint32_t walk = rows_walk_of(c);
    const uint32_t stk_lim = std::max(1u, std::min(im.height, kRowsMaxHeight));
    // counts workspace: nt+1 tile counts | (8-byte aligned) nt+1 tile offsets
    const uint64_t to_off = ((nt + 1) * sizeof(uint32_t) + 7) / 8 * 8;
    if ((rc = ensure(c.ws_temp, nt * region))) return rc;
    // [tile counts | tile offsets | the kernel's own counters (4 x u64)]
    const uint64_t sc_off = to_off + (nt + 1) * sizeof(uint64_t);
    const bool fresh = c.ws_counts.bytes < sc_off + 32;
    if ((rc = ensure(c.ws_counts, sc_off + 32))) return rc;
    unsigned long long *d_sc = reinterpret_cast<unsigned long long *>(reinterpret_cast<uint8_t *>(c.ws_counts.buf) + sc_off);
    if (fresh || c.rows_sc_dirty || c.rows_sc_at != sc_off) {  // the counters are cleared by k_compact_tiles
        MBRWT_HIP(hipMemsetAsync(d_sc, 0, 32, s));
        c.rows_sc_dirty = false;
        c.rows_sc_at = sc_off;
    }
    uint32_t *d_tc = reinterpret_cast<uint32_t *>(c.ws_counts.buf);
    uint64_t *d_to = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(c.ws_counts.buf) + to_off);
    hipcub::TransformInputIterator<uint64_t, MaskTile, const uint32_t *> it(d_tc, MaskTile());
    size_t scan_bytes = 0;
    MBRWT_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, it, d_to, nt, s));
    if ((rc = ensure(c.ws_scan, scan_bytes))) return rc;
    // the call's status block: the caller's (asynchronous) or the context's
    unsigned long long *st_blk =
        reinterpret_cast<unsigned long long *>(d_status ? d_status : c.d_scalars);

    RowsParams p{};
    p.rows = d_rows;
    p.n = n;
    p.num_rows = c.tree.num_rows;  // (record classes: mapped inside the traversal)
    p.classes = im.classes;
    p.class_bits = im.class_bits;
    p.blocks = (uint64_t)(uintptr_t)im.blocks;
    p.spill = (uint64_t)(uintptr_t)im.spill;
    p.magic = im.magic;
    p.S = im.S;
    const std::vector<uint32_t> &tab = im.term ? im.table3 : im.table2;  // (terminal records: the TT table)
    p.table_words = (uint32_t)tab.size();
    p.table = im.term ? im.d_table3 : im.d_table2;
    p.C = C;
    p.temp = reinterpret_cast<uint8_t *>(c.ws_temp.buf);
    p.tile_counts = d_tc;
    p.scalars = d_sc;
    p.status = st_blk;
    p.uni = im.uni;
    p.path_walk = (c.rows_walk == 7 && !im.nib) ? 0u : 1u;  // (7: the r03 odometer, A/B)
    p.stk_words = walk >= WALK_ODOMETER ? 0u : rows_stack_words(im);  // (the odometers keep no stack)
    p.frames = im.frames;
    p.mask1 = im.mask1 ? 1u : 0u;

    const size_t table_bytes = ((tab.size() + 3) & ~size_t(3)) * 4;
    const size_t per_wave = 64ull * (im.B + 4) + 256ull * p.stk_words + (walk >= WALK_ODOMETER ? 2ull * C : 0ull);
    const uint32_t wpb = (walk == WALK_TREE_ODOMETER && !im.term && !im.occ_cap &&
                          rows_waves_per_cu(table_bytes, per_wave, kRowsWpbWide) >
                              rows_waves_per_cu(table_bytes, per_wave, kRowsWpb))
                             ? kRowsWpbWide
                             : kRowsWpb;
    const RowsFn kfn = rows_fn(im, walk, wpb);
    // (terminal records: a field's second word may lie past the last wave's stage)
    const size_t lds = table_bytes + wpb * per_wave + (im.term ? 16 : 0);
    const uint32_t threads = 64 * wpb;
    // at most 24 waves (3 workgroups of 8) per CU: more waves make the walk phase
    // slower than the extra loads in flight gain (C4 0.426 ms at 3 against
    // 0.456 at 4, C2 0.068 against 0.073: profiles/r03/v06_rows_occupancy_*);
    // MBRWT_BUILD_ROWS_WGS_PER_CU (when the image is built) overrides
    const int occ_cap = im.occ_cap ? (int)im.occ_cap : (int)std::max(1u, 24u / wpb);
    uint64_t resident = 0;
    if ((rc = resident_workgroups(c, reinterpret_cast<const void *>(kfn), threads, lds, occ_cap, &resident))) return rc;

    c.rows_sc_dirty = true;  // until k_compact_tiles has run
    hipEvent_t e0, e1;
    if ((rc = timing_events(c, d_status != nullptr, &e0, &e1))) return rc;
    if (c.timing) MBRWT_HIP(hipEventRecord(e0, s));
    {
        // the odometer: kRowsTilesPerWave tiles per wave, the dispatcher
        // refilling each CU; the other walks keep the persistent grid (the
        // tree odometer's table -- 8.8 KB at the greedy + relax shape -- is
        // staged once per workgroup: one tile per wave took 0.518 against
        // 0.458 ms there, profiles/r05)
        const bool persistent = walk != WALK_ODOMETER && !im.term;  // (terminal records: a small table)
        const uint64_t per_wg = (uint64_t)wpb * kRowsTilesPerWave;
        const uint64_t g = persistent
                               ? std::max<uint64_t>(1, std::min<uint64_t>((nt + wpb - 1) / wpb, resident))
                               : std::max<uint64_t>(1, std::min<uint64_t>((nt + per_wg - 1) / per_wg, 1ull << 30));
        hipLaunchKernelGGL(kfn, dim3((unsigned)g), dim3(threads), lds, s, p);
        MBRWT_HIP(hipGetLastError());
    }
    if (c.timing) MBRWT_HIP(hipEventRecord(e1, s));
    MBRWT_HIP(hipcub::DeviceScan::ExclusiveSum(c.ws_scan.buf, scan_bytes, it, d_to, nt, s));
    {
        CompactParams cp{};
        cp.temp = p.temp;
        cp.C = C;
        cp.tile_counts = d_tc;
        cp.tile_offsets = d_to;
        cp.offsets = d_offsets;
        cp.cols = d_cols;
        cp.n = n;
        cp.cap = cap;
        cp.scalars = d_sc;
        cp.status = st_blk;
        cp.rows = d_rows;
        cp.classes = im.classes;
        cp.class_bits = im.class_bits;
        cp.v = view_of(c);
        cp.table = im.term ? im.d_table3 : im.d_table;
        const uint64_t waves = (nt + kCompactTpw - 1) / kCompactTpw;
        cp.stk_lim = stk_lim;
        // (MBRWT_OPT_COMPACT_CUS: on the CU-masked stream, between two events)
        hipStream_t sc = s;
        if (c.compact_cus && c.s_compact) {
            MBRWT_HIP(hipEventRecord(c.ev_trav, s));
            MBRWT_HIP(hipStreamWaitEvent(c.s_compact, c.ev_trav, 0));
            sc = c.s_compact;
        }
        using CompactFn = void (*)(CompactParams);
        const bool wide = im.max_arity > 16, narrow = width == 2;
        const CompactFn cfn = wide ? (narrow ? k_compact_tiles<true, uint16_t> : k_compact_tiles<true, uint32_t>)
                                   : (narrow ? k_compact_tiles<false, uint16_t> : k_compact_tiles<false, uint32_t>);
        hipLaunchKernelGGL(cfn, dim3((unsigned)((waves + 3) / 4)), dim3(256),
                           wide ? (size_t)0 : (size_t)256 * cp.stk_lim * 8, sc, cp);
        MBRWT_HIP(hipGetLastError());
        if (sc != s) {
            MBRWT_HIP(hipEventRecord(c.ev_comp, sc));
            MBRWT_HIP(hipStreamWaitEvent(s, c.ev_comp, 0));
        }
        c.rows_sc_dirty = false;
    }
    if (d_status) return MBRWT_OK;  // no host synchronisation: the status lands on the stream
    return finish_rows_call(c, needed, "row-record walk failed (corrupt image)", s);
}

namespace {
__global__ void k_set_status(unsigned long long *status, uint64_t need, uint64_t st) {
    status[0] = need;
    status[1] = st;
    status[2] |= 1ull << st;
}
}  // namespace

int rows_set_status(uint64_t *d_status, uint64_t need, int rc, hipStream_t s) {
    hipLaunchKernelGGL(k_set_status, dim3(1), dim3(1), 0, s, reinterpret_cast<unsigned long long *>(d_status), need,
                       (uint64_t)rc);
    MBRWT_HIP(hipGetLastError());
    return MBRWT_OK;
}

int rows_get_batch(Ctx &c, const uint64_t *d_rows, const uint64_t *d_cols, uint64_t n, uint8_t *d_out, hipStream_t s) {
    if (n == 0) return MBRWT_OK;
    if (c.rows.var) return var_get_batch(c, d_rows, d_cols, n, d_out, s);
    if (c.rows.classes)
        if (int rc = rows_class_map(c, d_rows, n, &d_rows, s)) return rc;
    MBRWT_HIP(hipMemsetAsync(c.d_scalars, 0, 8 * sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_rows_get, dim3(grid256(n)), dim3(256), 0, s, view_of(c),
                       (const uint32_t *)walk_table(c.rows), d_rows, d_cols, n, c.tree.num_columns, d_out,
                       reinterpret_cast<unsigned long long *>(c.d_scalars));
    return finish_record_call(c, s);
}

int rows_count_labels(Ctx &c, const uint64_t *d_rows, uint64_t n, uint64_t *d_counts, hipStream_t s) {
    if (c.rows.var) return var_count(c, d_rows, n, d_counts, nullptr, nullptr, s);
    if (c.rows.classes)
        if (int rc = rows_class_map(c, d_rows, n, &d_rows, s)) return rc;
    if (c.tree.num_columns) MBRWT_HIP(hipMemsetAsync(d_counts, 0, c.tree.num_columns * sizeof(uint64_t), s));
    MBRWT_HIP(hipMemsetAsync(c.d_scalars, 0, 8 * sizeof(uint64_t), s));
    if (n)
        hipLaunchKernelGGL(k_rows_count<false>, dim3(grid256(n)), dim3(256), 0, s, view_of(c),
                           (const uint32_t *)walk_table(c.rows), d_rows, n, reinterpret_cast<unsigned long long *>(d_counts),
                           reinterpret_cast<unsigned long long *>(c.d_scalars), (const uint32_t *)c.rows.d_table4);
    return finish_record_call(c, s);
}

int rows_count_work(Ctx &c, const uint64_t *d_rows, uint64_t n, uint64_t *visits, uint64_t *labels, hipStream_t s) {
    if (c.rows.var) return var_count(c, d_rows, n, nullptr, visits, labels, s);

    if (c.rows.classes)
        if (int rc = rows_class_map(c, d_rows, n, &d_rows, s)) return rc;
    MBRWT_HIP(hipMemsetAsync(c.d_scalars, 0, 8 * sizeof(uint64_t), s));
    if (n)
        hipLaunchKernelGGL(k_rows_count<true>, dim3(grid256(n)), dim3(256), 0, s, view_of(c),
                           (const uint32_t *)walk_table(c.rows), d_rows, n, nullptr,
                           reinterpret_cast<unsigned long long *>(c.d_scalars), (const uint32_t *)c.rows.d_table4);
    return finish_record_call(c, s, visits, labels);
}

int rows_get_column(Ctx &c, uint64_t column, uint64_t *d_rows, uint64_t rows_cap, uint64_t *rows_needed,
                    hipStream_t s) {
    if (c.rows.var) return var_get_column(c, column, d_rows, rows_cap, rows_needed, s);
    if (column >= c.tree.num_columns) {
        set_error("column out of range");
        return MBRWT_ERR_RANGE;
    }
    if (c.rows.classes) return rows_class_get_column(c, column, d_rows, rows_cap, rows_needed, s);
    const uint64_t n = c.tree.num_rows;
    const RowHasColumn f{view_of(c), walk_table(c.rows), (uint32_t)column};
    return select_rows(c, n, f, d_rows, rows_cap, rows_needed, s);
}

}  // namespace mbrwt
