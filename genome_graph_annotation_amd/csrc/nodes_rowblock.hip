// nodes_rowblock.hip -- the rowblock kernels of the per-node images (gfx950 /
// CDNA4) and their get_rows driver: k_traverse_p2w (trees with a P2W table),
// k_traverse_ptw (trees with a PTW table), k_compact_blocks.  A wave resolves
// 16 consecutive query rows into the rowblock's own temp region; one scan over
// the rowblock totals; the compaction; nodes_traverse.hip's direct pass for
// the rows of overflowing rowblocks.
#include "nodes_walk.hpp"
#include "pack_block.hpp"
#include "wave_scan.hpp"

namespace mbrwt {

// ------------------------------------------------------------------------
// k_traverse_p2w: the traversal kernel for trees whose super-root's children
// are all KIND_PACK2 nodes (the basic arity-8 trees at the Kingsford and
// RefSeq shapes).  A wave resolves a ROWBLOCK of 16 consecutive query rows in
// wave-uniform phases, so every iteration runs ONE code path for all 16 of
// its 4-lane groups (k_traverse_fast2 runs the row flush, the root visit and
// the PACK2 visit in nearly every iteration, for groups at different places):
//   root phase -- group g reads the super-root's 64-byte block at its row
//                 (BRWT.cpp:30 + :43 for every child of the root at once);
//                 its child mask P_g and the children's positions j_k;
//   items      -- the set (row, child) pairs of the rowblock, numbered in
//                 (row, child) order = the reference's output order
//                 (BRWT.cpp:45-51), listed in LDS (prefix of popc(P_g) over
//                 the groups by 4 ballots);
//   rounds     -- group g resolves item 16r + g: ONE 64-byte PACK2 block read
//                 (the child's whole 3-level subtree at j_k), the record walk
//                 counts the item's labels (quad scans), a wave scan over the
//                 round's items places them after all earlier items, and the
//                 labels go to the wave's LDS ring;
//   flush      -- complete 64-label units of the ring are stored as 256-byte
//                 wave-wide stores into the rowblock's temp region (full
//                 lines: no partial-line write amplification), the rest at
//                 the rowblock's end.
// Row counts come from the items' label positions; a rowblock with more than
// C labels stores none and lists its rows for the direct pass.
// ------------------------------------------------------------------------
constexpr uint32_t kP2wItems = 128;                      // <= 16 rows x 8 children
constexpr uint32_t kP2wWaveWords = kP2wItems + 32 + 132 + 20 + 16 * 16;  // + ring: items j | k | ipos | gfirst | blocks

struct P2wParams {
    const uint64_t *rows;
    uint64_t n;
    uint64_t num_rows;
    uint64_t root_base;       // dnode 0's PLANE image
    uint32_t root_stride;     // its bytes per 32-position block
    uint32_t table_words;     // Tree::p2w_table
    const uint32_t *table;
    uint32_t C;               // label capacity of a rowblock's temp region
    uint32_t S;               // LDS ring labels per wave (power of two >= 128)
    uint32_t *temp;           // [n_blocks][C]
    uint32_t *counts;         // [n] labels per row
    uint32_t *block_counts;   // [n_blocks] labels per rowblock
    uint32_t *ovf_list;       // rows of overflowing rowblocks
    unsigned long long *scalars;  // [1] overflow rows, [2] error flags
};

// (A register prefetch of a group's next block measured +1 % at 8 waves per
// SIMD and -7 % at 6: removed)
template <bool NT, typename LT = uint32_t>
__global__ __launch_bounds__(256, 8) void k_traverse_p2w(P2wParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_p2w[];
    const uint32_t lane = threadIdx.x & 63, c = lane & 3, g = lane >> 2, gb = lane & ~3u;
    // wave-uniform values are made scalar (SGPRs): VGPRs are the occupancy limit
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t i = threadIdx.x; i < p.table_words; i += blockDim.x) lds_p2w[i] = gld(p.table + i);
    __syncthreads();
    const AS_LDS uint32_t *tab = (const AS_LDS uint32_t *)lds_p2w;
    const uint32_t R = __builtin_amdgcn_readfirstlane(tab[0]), nA = __builtin_amdgcn_readfirstlane(tab[1]);
    const AS_LDS uint32_t *roots = tab + 4;
    const AS_LDS uint32_t *afc = roots + 4 * R;
    const AS_LDS uint32_t *blab = afc + nA;
    AS_LDS uint32_t *wbase = (AS_LDS uint32_t *)lds_p2w + ((p.table_words + 3) & ~3u) + wv * (kP2wWaveWords + p.S);
    AS_LDS uint32_t *items_j = wbase;                                 // [128] item position j
    AS_LDS uint8_t *items_k = (AS_LDS uint8_t *)(wbase + kP2wItems);  // [128] item child k
    AS_LDS uint32_t *ipos = wbase + kP2wItems + 32;                   // [129] item's first label; [T] = total
    AS_LDS uint32_t *gfirst = ipos + 132;                             // [17] group's first item; [16] = T
    AS_LDS uint32_t *pk = gfirst + 20 + 16 * g;                       // the group's staged 64-byte block
    AS_LDS uint32_t *ring = gfirst + 20 + 256;                        // S labels
    const AS_LDS uint8_t *pb = (const AS_LDS uint8_t *)pk;
    const uint32_t smask = p.S - 1;
    constexpr uint32_t kNone = 0xFFFFFFFFu;  // no row (ids are < num_rows <= 2^32 - 1)

    const uint64_t nblocks = (p.n + 15) / 16;
    const uint64_t wstride = (uint64_t)gridDim.x * 4;
    // the row of group g in rowblock b (out-of-range ids raise the error flag)
    auto load_row = [&](uint64_t b) -> uint32_t {
        const uint64_t r0 = b * 16;
        if (b >= nblocks || r0 + g >= p.n) return kNone;
        const uint64_t r = gld(p.rows + r0 + g);
        if (r < p.num_rows) return (uint32_t)r;
        if (c == 0) atomicOr(&p.scalars[2], 1ull);
        return kNone;
    };
    // the super-root's 64-byte block at `row` (16 bytes per lane: {rank, bits} of children 2c, 2c+1)
    auto root_load = [&](uint32_t row) -> uint4 {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (row != kNone && 2 * c < R)
            q = gld_at_nt<uint4, NT>(p.root_base + (uint64_t)(row >> 5) * p.root_stride + 16u * c);
        return q;
    };
    // the PACK2 block of item i (the child's whole 3-level subtree at j)
    auto item_load = [&](uint32_t i, uint32_t T) -> uint4 {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (i < T) {
            const uint32_t j = items_j[i], k = items_k[i];
            const uint64_t ubase = (uint64_t)roots[4 * k] | ((uint64_t)roots[4 * k + 1] << 32);
            q = gld_at_nt<uint4, NT>(ubase + (uint64_t)(j >> roots[4 * k + 2]) * kPack2Block + 16u * c);
        }
        return q;
    };

    uint64_t rb = (uint64_t)blockIdx.x * 4 + wv;
    for (; rb < nblocks; rb += wstride) {
        const uint64_t r0 = rb * 16;
        const uint32_t nr = (uint32_t)(p.n - r0 < 16 ? p.n - r0 : 16);
        // LT: the temp region's label type (u16 when every label is < 2^16:
        // half the traversal's writes and the compaction's reads)
        LT *const out = reinterpret_cast<LT *>(p.temp) + rb * (uint64_t)p.C;

        // ---- root phase: the super-root's block at group g's row ----
        const uint32_t row = load_row(rb);
        const uint4 qr = root_load(row);
        uint32_t P = 0, j0 = 0, j1 = 0;
        if (row != kNone && 2 * c < R) {
            const uint32_t t = row & 31, below = (1u << t) - 1u;
            const uint32_t b0 = (qr.y >> t) & 1u, b1 = (2 * c + 1 < R) ? (qr.w >> t) & 1u : 0u;
            j0 = qr.x + (uint32_t)__builtin_popcount(qr.y & below);
            j1 = qr.z + (uint32_t)__builtin_popcount(qr.w & below);
            P = (b0 | (b1 << 1)) << (2 * c);
        }
        P = quad_or(P);
        // ---- items in (row, child) order ----
        {
            const uint32_t ng = (uint32_t)__builtin_popcount(P);
            uint32_t pre = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                const uint64_t M = __ballot(c == 0 && ((ng >> b) & 1u));
                pre += (uint32_t)__popcll(M & ((1ull << gb) - 1ull)) << b;
            }
#pragma unroll
            for (uint32_t h = 0; h < 2; ++h) {
                const uint32_t k = 2 * c + h;
                if ((P >> k) & 1u) {
                    const uint32_t idx = pre + (uint32_t)__builtin_popcount(P & ((1u << k) - 1u));
                    items_j[idx] = h ? j1 : j0;
                    items_k[idx] = (uint8_t)k;
                }
            }
            if (c == 0) gfirst[g] = pre;
            if (lane == 60) gfirst[16] = pre + ng;
        }
        wave_sync();
        const uint32_t T = __builtin_amdgcn_readfirstlane(gfirst[16]);

        // ---- rounds: group g resolves item ib + g ----
        uint32_t running = 0, flushed = 0;  // wave-uniform label positions in the rowblock
        for (uint32_t ib = 0; ib < T; ib += 16) {
            const uint32_t i = ib + g;
            const bool act = i < T;
            const uint4 q = item_load(i, T);
            uint32_t j = 0, k = 0;
            if (act) {
                j = items_j[i];
                k = items_k[i];
            }
            const uint32_t lgs = roots[4 * k + 2], aidx = roots[4 * k + 3];
            const uint32_t t = j & ((1u << lgs) - 1u);
            if (act) ((AS_LDS u32x4_t *)pk)[c] = u32x4_t{q.x, q.y, q.z, q.w};
            wave_sync();
            uint32_t s = act ? pb[t] : 0u;
            if (act && pb[0] == 0) {
                // spilled block: copy the position's record into the group's
                // slot (list = u16 start[S+1], then the records; <= 64 bytes)
                const uint64_t la = ((uint64_t)pk[3] << 32) | pk[2];
                const uint32_t s0 = gld_at<uint16_t>(la + 2ull * t), len = gld_at<uint16_t>(la + 2ull * t + 2) - s0;
                wave_sync();  // every lane has read the list address
                AS_LDS uint8_t *pw = (AS_LDS uint8_t *)pk;
                for (uint32_t o = c; o < len; o += 4) pw[o] = gld_at<uint8_t>(la + s0 + o);
                wave_sync();
                s = 0;
            }
            // record walk, part 1: this lane's children A = 2c, 2c+1 of the
            // PACK2 node, their m1 bytes, the count of their labels
            const uint32_t m2 = act ? pb[s] : 0u;
            const uint32_t A0 = 2 * c;
            const uint32_t bA0 = (m2 >> A0) & 1u, bA1 = (m2 >> (A0 + 1)) & 1u;
            const uint32_t i0 = s + 1 + (uint32_t)__builtin_popcount(m2 & ((1u << A0) - 1u));
            const uint32_t m10 = bA0 ? pb[i0] : 0u;
            const uint32_t m11 = bA1 ? pb[i0 + bA0] : 0u;
            const uint32_t n1 = (uint32_t)__builtin_popcount(m10) + (uint32_t)__builtin_popcount(m11);
            uint32_t n1_tot;
            const uint32_t o2 = s + 1 + (uint32_t)__builtin_popcount(m2) + quad_exclusive_sum(n1, c, n1_tot);
            uint32_t nl = 0;
#pragma nounroll
            for (uint32_t e = 0; e < n1; ++e) nl += (uint32_t)__builtin_popcount(pb[o2 + e]);
            uint32_t ltot;
            const uint32_t lofs = quad_exclusive_sum(nl, c, ltot);
            // the item's first label: a wave scan of the items' totals (lanes of
            // a group hold the same total; groups are in item order)
            uint32_t x = ltot;
#pragma unroll
            for (uint32_t d = 4; d < 64; d <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
                if (lane >= d) x += y;
            }
            const uint32_t rtot = __builtin_amdgcn_readlane(x, 63);
            const uint32_t ibase = running + x - ltot;
            if (act && c == 0) ipos[i] = ibase;
            // a round that does not fit the ring (rare): pending ring labels
            // first, then this round's labels straight to the temp region
            const bool direct = rtot + (running - flushed) > p.S;
            if (direct) {
                for (uint32_t q2 = flushed + lane; q2 < running; q2 += 64)
                    if (q2 < p.C) gst(out + q2, (LT)ring[q2 & smask]);
                wave_sync();
            }
            // part 2: the labels, in the record's (pre-)order
            uint32_t pos = ibase + lofs;
            uint32_t o = o2;
#pragma unroll
            for (uint32_t h = 0; h < 2; ++h) {
                uint32_t xm = h ? m11 : m10;
                if (!xm) continue;
                const uint32_t fb = afc[aidx + A0 + h];  // first B of this A (index into blab)
                for (; xm; xm &= xm - 1) {
                    const uint32_t l = blab[fb + (uint32_t)__builtin_ctz(xm)];
                    for (uint32_t lm = pb[o++]; lm; lm &= lm - 1, ++pos) {
                        const uint32_t label = l + (uint32_t)__builtin_ctz(lm);
                        if (!direct) ring[pos & smask] = label;
                        else if (pos < p.C) gst(out + pos, (LT)label);
                    }
                }
            }
            running += rtot;
            if (direct) {
                flushed = running;
            } else {
                const uint32_t F = running & ~63u;  // complete 64-label units
                if (F > flushed) {
                    wave_sync();
                    for (uint32_t q2 = flushed + lane; q2 < F; q2 += 64)
                        if (q2 < p.C) gst(out + q2, (LT)ring[q2 & smask]);
                    flushed = F;
                }
            }
            wave_sync();  // the group's block slot and the ring are reused
        }
        if (lane == 0) ipos[T] = running;
        wave_sync();
        for (uint32_t q2 = flushed + lane; q2 < running; q2 += 64)
            if (q2 < p.C) gst(out + q2, (LT)ring[q2 & smask]);
        if (c == 0 && g < nr) gst(p.counts + r0 + g, (uint32_t)(ipos[gfirst[g + 1]] - ipos[gfirst[g]]));
        if (lane == 0) gst(p.block_counts + rb, running);
        if (running > p.C) {  // rowblock overflow: its rows go to the direct pass
            unsigned long long k0 = 0;
            if (lane == 0) k0 = atomicAdd(&p.scalars[1], (unsigned long long)nr);
            k0 = (unsigned long long)__shfl((long long)k0, 0, 64);
            if (c == 0 && g < nr) gst(p.ovf_list + k0 + g, (uint32_t)(r0 + g));
        }
        wave_sync();
    }
}

// ------------------------------------------------------------------------
// k_traverse_ptw: the traversal kernel for trees whose folded root's
// children are leaves or KIND_PACKT nodes -- any partitioner's shape (the
// greedy + relaxed trees of the reference's build scripts).  The rowblock
// phases of k_traverse_p2w, with one LANE per item in the rounds:
//   root phase -- group g reads the super-root's block at its row: up to 16
//                 children (WIDE: a second 64-byte half), their bits and
//                 positions (BRWT.cpp:30 + :43 for every child of the root);
//   items      -- the set (row, child) pairs in (row, child) order; a leaf
//                 child is an item of one label and no block;
//   rounds     -- lane L resolves item 64r + L: the 4 lanes of a group read
//                 the 64-byte KIND_PACKT blocks of the group's 4 items
//                 together (16 bytes each, one request per block), staged in
//                 LDS; the record's count byte places the item's labels (a
//                 wave scan), then the lane walks the DFS record over the PTW
//                 table in LDS and writes the labels -- in pre-order, the
//                 reference's order -- into the wave's ring;
//   flush      -- p2w's: 64-label units as full-line stores.
// MAXD: stack levels of the walk (>= the PACKT subtrees' height).  The temp
// labels are u16 (PTW columns are < 2^15).
// ------------------------------------------------------------------------
// waves per workgroup (one staged PTW table each): 3 x 7 per CU, 2.27 against 2.47 ms at 4 x 4
// (profiles/r02/v42_bench_greedy_ptw_wpb7.log)
constexpr uint32_t kPtwWpb = 7;
// labels of a wave's ring: the size at which 21 waves' LDS fits a CU (the same profile; 512 with 4-wave workgroups)
constexpr uint32_t kPtwRing = 256;
using PtwLabel = uint16_t;  // the temp region's labels

template <bool WIDE>
struct PtwLayout {
    static constexpr uint32_t kItems = WIDE ? 256 : 128;  // 16 rows x R children
    static constexpr uint32_t kRing = kPtwRing;           // labels
    // items j | items k | row counts | group's first item | blocks (64 x 64 B) | ring
    static constexpr uint32_t kWords = kItems + kItems / 4 + 16 + 20 + 1024 + kRing;
};

// the labels of a KIND_PACKT record (masks from byte o on) into the ring
// (or, `direct`, the rowblock's temp region) from label position pos on
template <int MAXD>
__device__ __forceinline__ void ptw_walk(const AS_LDS uint8_t *pb, uint32_t o, uint32_t node,
                                         const AS_LDS uint32_t *ntab, const AS_LDS uint16_t *etab,
                                         AS_LDS uint32_t *ring, uint32_t smask, uint32_t pos, bool direct,
                                         PtwLabel *out, uint32_t C, bool &overflow) {
    uint32_t nw = ntab[node];
    uint32_t m = pb[o++];
    if ((nw >> 24) > 8) m |= (uint32_t)pb[o++] << 8;
    uint32_t top = (nw & 0xFFFFu) | (m << 16);  // {first entry, children still to visit}
    uint32_t st[MAXD - 1];
#pragma unroll
    for (int k = 0; k < MAXD - 1; ++k) st[k] = 0;
    int sp = 0;
    while (true) {
        if ((top >> 16) == 0) {
            if (sp == 0) break;
            top = st[0];
#pragma unroll
            for (int k = 0; k < MAXD - 2; ++k) st[k] = st[k + 1];
            --sp;
            continue;
        }
        const uint32_t c = (uint32_t)__builtin_ctz(top >> 16);
        top &= ~(0x10000u << c);
        const uint32_t e = etab[(top & 0xFFFFu) + c];
        if (e & 0x8000u) {
            const uint32_t label = e & 0x7FFFu;
            if (!direct) ring[pos & smask] = label;
            else if (pos < C) gst(out + pos, (PtwLabel)label);
            ++pos;
            continue;
        }
        nw = ntab[e];
        uint32_t mw = pb[o++];
        if ((nw >> 24) > 8) mw |= (uint32_t)pb[o++] << 8;
        if (top >> 16) {  // the parent still has children to visit
            if (sp == MAXD - 1) {
                overflow = true;
                break;
            }
#pragma unroll
            for (int k = MAXD - 2; k > 0; --k) st[k] = st[k - 1];
            st[0] = top;
            ++sp;
        }
        top = (nw & 0xFFFFu) | (mw << 16);
    }
}

// The same walk for all 64 lanes of the wave at once, in lockstep and
// without per-lane branches (the branchy walk's exec-mask and loop handling
// measured more scalar than vector instructions per launch): each iteration
// takes one child of every lane's top frame; a leaf stores its column, an
// internal child pushes its frame (selects over the register stack) and an
// emptied frame is popped at the end of the iteration.  Lanes with no record
// (`live` false) idle.  Ring only (the `direct` rounds use ptw_walk).
template <int MAXD>
__device__ __forceinline__ void ptw_walk_wave(const AS_LDS uint8_t *pb, uint32_t o, uint32_t node, bool live,
                                              const AS_LDS uint32_t *ntab, const AS_LDS uint16_t *etab,
                                              AS_LDS uint32_t *ring, uint32_t smask, uint32_t pos, bool &overflow) {
    uint32_t nw = ntab[live ? node : 0u];
    uint32_t m = pb[o];
    const uint32_t w0 = (nw >> 24) > 8 ? 1u : 0u;
    m |= w0 ? (uint32_t)pb[o + 1] << 8 : 0u;
    o += 1 + w0;
    uint32_t top = live ? ((nw & 0xFFFFu) | (m << 16)) : 0u;
    uint32_t st[MAXD - 1];
#pragma unroll
    for (int k = 0; k < MAXD - 1; ++k) st[k] = 0;
    uint32_t sp = 0;
    bool done = !live || (top >> 16) == 0;
    while (__any(!done)) {
        const uint32_t mm = top >> 16;
        const uint32_t c = (uint32_t)__builtin_ctz(mm | 0x10000u);
        top &= ~(0x10000u << c);
        const uint32_t e = etab[done ? 0u : (top & 0xFFFFu) + c];
        const bool leaf = (e & 0x8000u) != 0;
        if (!done && leaf) ring[pos & smask] = e & 0x7FFFu;
        pos += (!done && leaf) ? 1u : 0u;
        const bool inner = !done && !leaf;
        const uint32_t nw2 = ntab[inner ? e : 0u];
        const uint32_t w2 = (nw2 >> 24) > 8 ? 1u : 0u;
        const uint32_t mw = (uint32_t)pb[o] | (w2 ? (uint32_t)pb[o + 1] << 8 : 0u);
        o += inner ? 1u + w2 : 0u;
        const bool push = inner && (top >> 16) != 0;
        overflow |= push && sp == (uint32_t)(MAXD - 1);
#pragma unroll
        for (int k = MAXD - 2; k > 0; --k) st[k] = push ? st[k - 1] : st[k];
        st[0] = push ? top : st[0];
        sp += push ? 1u : 0u;
        top = inner ? ((nw2 & 0xFFFFu) | (mw << 16)) : top;
        const bool pop = !done && (top >> 16) == 0 && sp > 0;  // (pushed frames are never empty)
        top = pop ? st[0] : top;
#pragma unroll
        for (int k = 0; k < MAXD - 2; ++k) st[k] = pop ? st[k + 1] : st[k];
        sp -= pop ? 1u : 0u;
        done = done || (top >> 16) == 0;
    }
}

template <bool NT, bool WIDE, int MAXD>
__global__ __launch_bounds__(64 * kPtwWpb) void k_traverse_ptw(P2wParams p) {
    using Lay = PtwLayout<WIDE>;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_ptw[];
    const uint32_t lane = threadIdx.x & 63, c = lane & 3, g = lane >> 2, gb = lane & ~3u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t i = threadIdx.x; i < p.table_words; i += blockDim.x) lds_ptw[i] = gld(p.table + i);
    __syncthreads();
    const AS_LDS uint32_t *tab = (const AS_LDS uint32_t *)lds_ptw;
    const uint32_t R = __builtin_amdgcn_readfirstlane(tab[0]), nI = __builtin_amdgcn_readfirstlane(tab[1]);
    const AS_LDS uint32_t *roots = tab + 4;
    const AS_LDS uint32_t *ntab = roots + 4 * R;
    const AS_LDS uint16_t *etab = (const AS_LDS uint16_t *)(ntab + nI);
    AS_LDS uint32_t *wbase = (AS_LDS uint32_t *)lds_ptw + ((p.table_words + 3) & ~3u) + wv * Lay::kWords;
    AS_LDS uint32_t *items_j = wbase;                                    // item position j
    AS_LDS uint8_t *items_k = (AS_LDS uint8_t *)(wbase + Lay::kItems);   // item child k
    AS_LDS uint32_t *rowcnt = wbase + Lay::kItems + Lay::kItems / 4;      // [16] labels per row
    AS_LDS uint32_t *gfirst = rowcnt + 16;                               // [17] group's first item; [16] = T
    AS_LDS uint32_t *slots = gfirst + 20;                                // lane L's 64-byte block: [16 L, 16 L + 16)
    AS_LDS uint32_t *ring = slots + 1024;                                // kRing labels
    AS_LDS uint32_t *mine = slots + 16 * lane;
    const AS_LDS uint8_t *pb = (const AS_LDS uint8_t *)mine;
    constexpr uint32_t smask = Lay::kRing - 1;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    bool overflow = false;

    const uint64_t nblocks = (p.n + 15) / 16;
    const uint64_t wstride = (uint64_t)gridDim.x * kPtwWpb;
    for (uint64_t rb = (uint64_t)blockIdx.x * kPtwWpb + wv; rb < nblocks; rb += wstride) {
        const uint64_t r0 = rb * 16;
        const uint32_t nr = (uint32_t)(p.n - r0 < 16 ? p.n - r0 : 16);
        // u16 temp labels: half the traversal's writes and the compaction's reads
        PtwLabel *const out = reinterpret_cast<PtwLabel *>(p.temp) + rb * (uint64_t)p.C;

        // ---- root phase: the super-root's block at group g's row ----
        uint32_t row = kNone;
        if (r0 + g < p.n) {
            const uint64_t r = gld(p.rows + r0 + g);
            if (r < p.num_rows) row = (uint32_t)r;
            else if (c == 0) atomicOr(&p.scalars[2], 1ull);
        }
        uint4 qa = make_uint4(0, 0, 0, 0), qb = make_uint4(0, 0, 0, 0);
        const uint64_t rblk = p.root_base + (uint64_t)(row >> 5) * p.root_stride;
        if (row != kNone && 2 * c < R) qa = gld_at_nt<uint4, NT>(rblk + 16u * c);
        if (WIDE && row != kNone && 8 + 2 * c < R) qb = gld_at_nt<uint4, NT>(rblk + 64u + 16u * c);
        uint32_t P = 0, jj[4] = {0, 0, 0, 0};
        if (row != kNone) {
            const uint32_t t = row & 31, below = (1u << t) - 1u;
            const uint32_t k0 = 2 * c;
            const uint32_t b0 = k0 < R ? (qa.y >> t) & 1u : 0u, b1 = k0 + 1 < R ? (qa.w >> t) & 1u : 0u;
            jj[0] = qa.x + (uint32_t)__builtin_popcount(qa.y & below);
            jj[1] = qa.z + (uint32_t)__builtin_popcount(qa.w & below);
            P = (b0 | (b1 << 1)) << k0;
            if (WIDE) {
                const uint32_t b2 = 8 + k0 < R ? (qb.y >> t) & 1u : 0u, b3 = 9 + k0 < R ? (qb.w >> t) & 1u : 0u;
                jj[2] = qb.x + (uint32_t)__builtin_popcount(qb.y & below);
                jj[3] = qb.z + (uint32_t)__builtin_popcount(qb.w & below);
                P |= (b2 | (b3 << 1)) << (8 + k0);
            }
        }
        P = quad_or(P);
        // ---- items in (row, child) order ----
        {
            const uint32_t ng = (uint32_t)__builtin_popcount(P);
            uint32_t pre = 0;
#pragma unroll
            for (uint32_t b = 0; b < (WIDE ? 5u : 4u); ++b) {
                const uint64_t M = __ballot(c == 0 && ((ng >> b) & 1u));
                pre += (uint32_t)__popcll(M & ((1ull << gb) - 1ull)) << b;
            }
#pragma unroll
            for (uint32_t h = 0; h < (WIDE ? 4u : 2u); ++h) {
                const uint32_t k = (h < 2 ? 0u : 8u) + 2 * c + (h & 1u);
                if ((P >> k) & 1u) {
                    const uint32_t idx = pre + (uint32_t)__builtin_popcount(P & ((1u << k) - 1u));
                    items_j[idx] = jj[h];
                    items_k[idx] = (uint8_t)k;
                }
            }
            if (c == 0) {
                gfirst[g] = pre;
                rowcnt[g] = 0;
            }
            if (lane == 60) gfirst[16] = pre + ng;
        }
        wave_sync();
        const uint32_t T = __builtin_amdgcn_readfirstlane(gfirst[16]);

        // ---- rounds: lane L resolves item ib + L ----
        uint32_t running = 0, flushed = 0;
        for (uint32_t ib = 0; ib < T; ib += 64) {
            // the group's 4 blocks, quarter c each (all 4 requests in flight together)
            uint4 q[4];
#pragma unroll
            for (uint32_t h = 0; h < 4; ++h) {
                q[h] = make_uint4(0, 0, 0, 0);
                const uint32_t ih = ib + 4 * g + h;
                if (ih < T) {
                    const uint32_t k = items_k[ih];
                    if (!(roots[4 * k + 3] >> 31)) {
                        const uint64_t ubase = (uint64_t)roots[4 * k] | ((uint64_t)roots[4 * k + 1] << 32);
                        q[h] = gld_at_nt<uint4, NT>(ubase + (uint64_t)(items_j[ih] / roots[4 * k + 2]) * kPack2Block +
                                                    16u * c);
                    }
                }
            }
#pragma unroll
            for (uint32_t h = 0; h < 4; ++h)
                ((AS_LDS u32x4_t *)(slots + 16 * (4 * g + h)))[c] = u32x4_t{q[h].x, q[h].y, q[h].z, q[h].w};
            wave_sync();
            const uint32_t i = ib + lane;
            const bool act = i < T;
            uint32_t j = 0, k = 0;
            if (act) {
                j = items_j[i];
                k = items_k[i];
            }
            const uint32_t ent = roots[4 * k + 3];
            const bool blk = act && !(ent >> 31);
            uint32_t s = 0;
            if (blk) {
                const uint32_t t = j % roots[4 * k + 2];
                s = pb[t];
                if (pb[0] == 0) {
                    // spilled block: copy the position's record into the lane's
                    // slot (list = u16 start[S+1], then the records; <= 64 bytes)
                    const uint64_t la = ((uint64_t)mine[3] << 32) | mine[2];
                    const uint32_t s0 = gld_at<uint16_t>(la + 2ull * t), len = gld_at<uint16_t>(la + 2ull * t + 2) - s0;
                    AS_LDS uint8_t *pw = (AS_LDS uint8_t *)mine;
                    for (uint32_t o = 0; o < len; o += 4) {
                        uint8_t b4[4];
#pragma unroll
                        for (uint32_t e = 0; e < 4; ++e) b4[e] = o + e < len ? gld_at<uint8_t>(la + s0 + o + e) : 0;
#pragma unroll
                        for (uint32_t e = 0; e < 4; ++e)
                            if (o + e < len) pw[o + e] = b4[e];
                    }
                    s = 0;
                }
            }
            const uint32_t nl = blk ? (uint32_t)pb[s] : act ? 1u : 0u;  // the record's label count
            // the item's first label: a wave scan of the counts (lanes are in item order)
            uint32_t x = nl;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
                if (lane >= d) x += y;
            }
            const uint32_t rtot = __builtin_amdgcn_readlane(x, 63);
            const uint32_t ibase = running + x - nl;
            if (act) {  // the item's row: the last group whose first item is <= i
                uint32_t gr = 0;
#pragma unroll
                for (uint32_t q2 = 1; q2 < 16; ++q2) gr = gfirst[q2] <= i ? q2 : gr;
                __hip_atomic_fetch_add((uint32_t *)(rowcnt + gr), nl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
            const bool direct = rtot + (running - flushed) > Lay::kRing;
            if (direct) {
                for (uint32_t q2 = flushed + lane; q2 < running; q2 += 64)
                    if (q2 < p.C) gst(out + q2, (PtwLabel)ring[q2 & smask]);
                wave_sync();
            }
            if (!direct) {
                ptw_walk_wave<MAXD>(pb, s + 1, ent, blk, ntab, etab, ring, smask, ibase, overflow);
                if (act && !blk) ring[ibase & smask] = ent & 0x7FFFFFFFu;
            } else if (blk) {
                ptw_walk<MAXD>(pb, s + 1, ent, ntab, etab, ring, smask, ibase, direct, out, p.C, overflow);
            } else if (act && ibase < p.C) {
                gst(out + ibase, (PtwLabel)(ent & 0x7FFFFFFFu));
            }
            running += rtot;
            if (direct) {
                flushed = running;
            } else {
                const uint32_t F = running & ~63u;  // complete 64-label units
                if (F > flushed) {
                    wave_sync();
                    for (uint32_t q2 = flushed + lane; q2 < F; q2 += 64)
                        if (q2 < p.C) gst(out + q2, (PtwLabel)ring[q2 & smask]);
                    flushed = F;
                }
            }
            wave_sync();  // the slots and the ring are reused
        }
        for (uint32_t q2 = flushed + lane; q2 < running; q2 += 64)
            if (q2 < p.C) gst(out + q2, (PtwLabel)ring[q2 & smask]);
        if (lane < nr) gst(p.counts + r0 + lane, rowcnt[lane]);
        if (lane == 0) gst(p.block_counts + rb, running);
        if (running > p.C) {  // rowblock overflow: its rows go to the direct pass
            unsigned long long k0 = 0;
            if (lane == 0) k0 = atomicAdd(&p.scalars[1], (unsigned long long)nr);
            k0 = (unsigned long long)__shfl((long long)k0, 0, 64);
            if (lane < nr) gst(p.ovf_list + k0 + lane, (uint32_t)(r0 + lane));
        }
        wave_sync();
    }
    if (overflow) atomicOr(&p.scalars[2], 2ull);
}

// k_compact_blocks: output of k_traverse_p2w -> CSR.  16 lanes per 16-row
// block (4 blocks per wave): the rows' offsets (block offset + in-block
// prefix) and a contiguous copy of the block's labels, each lane's (up to 8)
// label reads issued before its stores.  Overflowing blocks (> C labels) are
// left to the direct pass.
template <bool BIG, typename LT = uint32_t>
__global__ __launch_bounds__(256) void k_compact_blocks(const uint32_t *__restrict__ counts,
                                                        const uint64_t *__restrict__ block_offsets,
                                                        const LT *__restrict__ temp, uint32_t C,
                                                        uint64_t *__restrict__ offsets, uint32_t *__restrict__ cols,
                                                        uint64_t n, const uint32_t *__restrict__ label_map,
                                                        uint32_t map_lds, uint64_t cap) {
    const LabelMap lmap = stage_label_map(label_map, map_lds);
    const uint32_t lane = threadIdx.x & 63, sub = lane & 15;
    const uint64_t nb = (n + 15) / 16;
    // launched before the host knows the total: a batch over the caller's
    // capacity writes nothing (the host then returns MBRWT_ERR_CAPACITY)
    if (gld(block_offsets + nb) > cap) return;
    const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) >> 4;
    for (uint64_t b = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; b < nb; b += stride) {
        const uint64_t r0 = b * 16;
        const uint32_t nr = (uint32_t)(n - r0 < 16 ? n - r0 : 16);
        const uint64_t base = gld(block_offsets + b);
        const uint32_t mine = sub < nr ? gld(counts + r0 + sub) : 0u;
        // the first 128 labels are read before the block's total is known
        // (when the temp region holds C >= 128 words; always at the default
        // slot sizes): the label reads overlap the offset reads instead of
        // waiting behind them
        const LT *src = temp + b * (uint64_t)C;
        uint32_t v0[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) v0[k] = C >= 128 ? (uint32_t)gld(src + sub + 16 * k) : 0u;
        uint32_t x = mine;
#pragma unroll
        for (uint32_t d = 1; d < 16; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, d, 16);
            if (sub >= d) x += y;
        }
        const uint32_t total = (uint32_t)__shfl((int)x, 15, 16);
        if (sub < nr) gst(offsets + r0 + sub, base + (x - mine));
        if (sub == 0 && r0 + nr == n) gst(offsets + n, base + total);
        if (total > C) continue;
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {  // the first 128 labels
            const uint32_t i = sub + 16 * k;
            if (i < total) gst(cols + base + i, lmap(C < 128 ? (uint32_t)gld(src + i) : v0[k]));
        }
        // the rest, U labels per lane and round, every lane's reads issued
        // before its stores: U = 32 for large rows (BIG: e.g. 120 labels per
        // row at the RefSeq shape, 2.7 -> 2.1 ms per 10 M rows), 8 otherwise
        // (32 registers cost occupancy: 0.146 -> 0.201 ms at 8 labels per row)
        constexpr uint32_t U = BIG ? 32 : 8;
        for (uint32_t i0 = 128; i0 < total; i0 += 16 * U) {
            uint32_t v[U];
#pragma unroll
            for (uint32_t k = 0; k < U; ++k) {
                const uint32_t i = i0 + sub + 16 * k;
                v[k] = i < total ? (uint32_t)gld(src + i) : 0u;
            }
#pragma unroll
            for (uint32_t k = 0; k < U; ++k) {
                const uint32_t i = i0 + sub + 16 * k;
                if (i < total) gst(cols + base + i, lmap(v[k]));
            }
        }
    }
}
namespace nodes {
namespace {

using P2wFn = void (*)(P2wParams);

// labels of a wave's LDS ring in k_traverse_p2w (profiles/r02/v32_p2w_c4_sweep.log)
constexpr uint32_t kP2wRing = 512;
constexpr uint32_t kP2wWpb = 4;  // waves per workgroup (its __launch_bounds__)

// the p2w kernel stores u16 temp labels when they fit (label indices < num_columns)
bool p2w_label16(const Ctx &c) { return c.tree.num_columns <= 0x10000u; }

// k_traverse_p2w for this context?  Default for trees with a P2W table.
P2wFn p2w_kernel(const Ctx &c) {
    if (c.tree.p2w_table.empty() || !c.d_p2w || c.kernel_variant != 0) return nullptr;
    const bool big = nt_reads(c);
    if (p2w_label16(c)) return big ? k_traverse_p2w<true, uint16_t> : k_traverse_p2w<false, uint16_t>;
    return big ? k_traverse_p2w<true> : k_traverse_p2w<false>;
}

size_t p2w_lds_bytes(const Ctx &c) {
    return ((c.tree.p2w_table.size() + 3) & ~size_t(3)) * 4 + kP2wWpb * (size_t)(kP2wWaveWords + kP2wRing) * 4;
}

// k_traverse_ptw for this context?  Default for trees with a PTW table.
bool ptw_wide(const Ctx &c) { return c.tree.ptw_table[0] > 8; }  // a second 64-byte half of root children
P2wFn ptw_kernel(const Ctx &c) {
    const auto &t = c.tree.ptw_table;
    if (t.empty() || !c.d_ptw || c.kernel_variant != 0) return nullptr;
    const bool nt = nt_reads(c), wide = ptw_wide(c), deep = t[3] > 4;
#define PTW(NTV, W, D) if (nt == NTV && wide == W && deep == D) return k_traverse_ptw<NTV, W, D ? 8 : 4>;
    PTW(false, false, false) PTW(false, false, true) PTW(false, true, false) PTW(false, true, true)
    PTW(true, false, false) PTW(true, false, true) PTW(true, true, false) PTW(true, true, true)
#undef PTW
    return nullptr;
}

size_t ptw_lds_bytes(const Ctx &c) {
    const size_t per_wave = ptw_wide(c) ? PtwLayout<true>::kWords : PtwLayout<false>::kWords;
    return ((c.tree.ptw_table.size() + 3) & ~size_t(3)) * 4 + kPtwWpb * per_wave * 4;
}

// the rowblock kernel of a context (fn null: none) -- k_traverse_ptw before k_traverse_p2w
struct RowblockKernel {
    P2wFn fn;
    const uint32_t *table;
    uint32_t table_words;
    size_t lds;
    uint32_t wpb;
    bool final_columns;  // the kernel emits global columns (k_traverse_ptw): no label map afterwards
    bool label16;        // u16 temp labels
    const char *name;
};
RowblockKernel rowblock_kernel(const Ctx &c) {
    if (const P2wFn kfn = ptw_kernel(c))
        return {kfn, c.d_ptw, (uint32_t)c.tree.ptw_table.size(), ptw_lds_bytes(c), kPtwWpb, true, sizeof(PtwLabel) == 2,
                "k_traverse_ptw"};
    if (const P2wFn kfn = p2w_kernel(c))
        return {kfn, c.d_p2w, (uint32_t)c.tree.p2w_table.size(), p2w_lds_bytes(c), kP2wWpb, false, p2w_label16(c),
                "k_traverse_p2w"};
    return {};
}

}  // namespace

const char *rowblock_kernel_name(const Ctx &c) { return rowblock_kernel(c).name; }

// get_rows through k_traverse_p2w: rowblocks of 16 rows, each written to its
// own temp region of C = 16 K labels; one scan over the rowblock totals; the
// compaction; the direct pass for overflowing rowblocks.
// (k_traverse_ptw: the same driver over the PTW table)
int run_get_rows_p2w(Ctx &c, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets, uint32_t *d_cols, uint64_t cap,
                     uint64_t *needed, hipStream_t s, bool *taken) {
    const RowblockKernel kr = rowblock_kernel(c);
    *taken = kr.fn != nullptr;
    if (!kr.fn) return MBRWT_OK;
    const P2wFn kfn = kr.fn;
    const uint32_t K = auto_slots(c);
    const uint32_t C = 16 * K;
    const Trav fn_direct = pick_traverse(c, MODE_DIRECT);
    if (!fn_direct) {
        set_error("tree deeper than 32 levels of internal nodes");
        return MBRWT_ERR_UNSUPPORTED;
    }
    int rc;
    const uint64_t nb = (n + 15) / 16;
    if ((rc = ensure(c.ws_temp, nb * (uint64_t)C * (kr.label16 ? 2u : 4u)))) return rc;
    if ((rc = ensure(c.ws_ovf, n * sizeof(uint32_t)))) return rc;
    CountsScan w;  // n row counts, the scan over the nb + 1 block counts
    if ((rc = counts_scan_prepare(c, n, nb, nullptr, s, &w))) return rc;

    const DevNode &root = c.tree.nodes[0];
    P2wParams p{};
    p.rows = d_rows;
    p.n = n;
    p.num_rows = c.tree.num_rows;
    p.root_base = root.base;
    p.root_stride = root.stride;
    p.table_words = kr.table_words;
    p.table = kr.table;
    p.C = C;
    p.S = kP2wRing;  // (k_traverse_ptw: its ring is a compile-time constant)
    p.temp = reinterpret_cast<uint32_t *>(c.ws_temp.buf);
    p.counts = w.counts;
    p.block_counts = w.group_counts;
    p.ovf_list = reinterpret_cast<uint32_t *>(c.ws_ovf.buf);
    p.scalars = reinterpret_cast<unsigned long long *>(c.d_scalars);

    const size_t lds = kr.lds;
    const uint32_t threads = 64 * kr.wpb;
    uint64_t resident = 0;
    if ((rc = resident_workgroups(c, reinterpret_cast<const void *>(kfn), threads, lds, 0, &resident))) return rc;
    const uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>((nb + kr.wpb - 1) / kr.wpb, resident));

    MBRWT_HIP(hipMemsetAsync(c.d_scalars, 0, 8 * sizeof(uint64_t), s));
    MBRWT_HIP(hipMemsetAsync(w.in + w.len - 1, 0, sizeof(uint32_t), s));
    if (c.timing) MBRWT_HIP(hipEventRecord(c.ev0, s));
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(threads), lds, s, p);
    MBRWT_HIP(hipGetLastError());
    if (c.timing) MBRWT_HIP(hipEventRecord(c.ev1, s));
    MBRWT_HIP(counts_scan_run(c, w, s));
    // the compaction is queued right behind the scan, before the host learns
    // the total (one synchronisation per call, after it; the kernel checks
    // the capacity itself)
    const uint32_t map_lds = kr.final_columns ? 0u : label_map_lds(c);
    // one 16-lane group per rowblock and no grid-stride rounds: with 8192
    // workgroups each wave walked ~15 rowblocks through two dependent memory
    // latencies each
    const uint64_t g = std::min<uint64_t>((nb + 15) / 16, 1u << 20);
    const bool big = c.tree.num_rows && (double)c.tree.num_relations > 32.0 * (double)c.tree.num_rows;
    const uint32_t *lm = kr.final_columns ? nullptr : (const uint32_t *)c.d_label_map;
    if (kr.label16) {
        auto *cfn = big ? k_compact_blocks<true, uint16_t> : k_compact_blocks<false, uint16_t>;
        hipLaunchKernelGGL(cfn, dim3((unsigned)g), dim3(256), map_lds * 4, s, w.counts, w.group_offsets,
                           reinterpret_cast<const uint16_t *>(p.temp), C, d_offsets, d_cols, n, lm, map_lds, cap);
    } else
        hipLaunchKernelGGL(big ? k_compact_blocks<true> : k_compact_blocks<false>, dim3((unsigned)g), dim3(256),
                           map_lds * 4, s, w.counts, w.group_offsets, (const uint32_t *)p.temp, C, d_offsets, d_cols, n,
                           lm, map_lds, cap);
    MBRWT_HIP(hipGetLastError());
    MBRWT_HIP(hipMemcpyAsync(c.d_scalars, w.out + w.len - 1, sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    uint64_t ovf = 0;
    if ((rc = finish_nodes_call(c, cap, needed, &ovf, s))) return rc;
    if (ovf) MBRWT_HIP(direct_pass(c, fn_direct, d_rows, p.ovf_list, ovf, d_offsets, d_cols, s));
    return MBRWT_OK;
}

}  // namespace nodes
}  // namespace mbrwt
