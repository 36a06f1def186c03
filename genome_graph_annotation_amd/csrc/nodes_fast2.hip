// nodes_fast2.hip -- k_traverse_fast2 and k_compact_chunks: the slot path of
// the basic arity-<=8 trees on the per-node images (gfx950 / CDNA4).  The
// launch goes through nodes_traverse.hip's launch(); query.hip drives it.
#include "nodes_walk.hpp"
#include "pack_block.hpp"

namespace mbrwt {

constexpr uint32_t kFastMaxd = 4;  // stack frames of k_traverse_fast2 (finalize_tree: fast_shape)

// ------------------------------------------------------------------------
// k_traverse_fast2: the traversal kernel for the basic arity-<=8 trees
// (every internal node PLANE, MASK8 or PACK with arity <= 8, MASK8 labels
// consecutive, <= kFastMaxd stack frames, every non-leaf record in the LDS
// table -- Tree::fast_shape && lds_complete).  A group of 4 lanes answers a
// row (2 children per lane, 16 rows per wave).  Every iteration of the wave
// runs ONE inlined visit (a group starting a row visits the root in the same
// code as a group visiting a popped child): with 16 groups per wave at
// different places of their trees, every extra code path in the loop body
// is paid by the whole wave.  Visits:
//   PLANE -- one coalesced 64-byte block read (16 B per lane = {rank, bits}
//            of two children); child mask OR-reduced over the quad by DPP;
//            a stack frame (3 registers per lane) is pushed;
//   PACK  -- the same block read gives the children bits AND their MASK8
//            masks; the block is staged in LDS and each lane picks the masks
//            of its two children: a level costs no second dependent read;
//   PLANE with FLAG_MASK_CHILDREN (node kinds without MBRWT_KIND_PACK) -- block read, then
//            the (independent) mask reads of the set MASK8 children;
//   MASK8 -- leaf labels from one byte (only as the root's child).
// Labels are staged in LDS (32 per row) and flushed as 16-byte vectors when
// the row ends (vmcnt counts stores on CDNA4: no stores inside the descent).
// ------------------------------------------------------------------------
template <bool NT, bool SMALLK, bool P2>
__global__ __launch_bounds__(256, 8) void k_traverse_fast2(TravParams p) {
    // P2: trees with KIND_PACK2 nodes (one stack frame, no FLAG_MASK_CHILDREN
    // nodes): the PACK2 visit replaces the MASK_CHILDREN one, a shorter stack
    constexpr int kFastMaxd = P2 ? 1 : (int)mbrwt::kFastMaxd;
    constexpr uint64_t M48 = (1ull << 48) - 1;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t c = lane & 3;
    const uint32_t gbase = lane & ~3u;
    const uint64_t gid = (uint64_t)blockIdx.x * 64 + threadIdx.x / 4;
    const uint64_t ngroups = (uint64_t)gridDim.x * 64;

    // LDS: 64 groups x kStageLabels labels | 64 groups x one 64-byte PACK block | node records
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stage[];
    AS_LDS uint32_t *stage = (AS_LDS uint32_t *)lds_stage + (threadIdx.x / 4) * kStageLabels;
    AS_LDS uint32_t *pk = (AS_LDS uint32_t *)lds_stage + 64 * kStageLabels + (threadIdx.x / 4) * 16;
    AS_LDS uint64_t *lds_nodes = (AS_LDS uint64_t *)((AS_LDS uint32_t *)lds_stage + 64 * kStageLabels + 64 * 16);
    const uint64_t *gnodes = reinterpret_cast<const uint64_t *>(p.cnodes);
    for (uint32_t i = threadIdx.x; i < 2 * p.n_lds; i += blockDim.x) lds_nodes[i] = gld(gnodes + i);
    __syncthreads();

    uint32_t jc0[kFastMaxd], jc1[kFastMaxd], fp[kFastMaxd];  // fp = first_child << 8 | pending mask
#pragma unroll
    for (int k = 0; k < (int)kFastMaxd; ++k) jc0[k] = jc1[k] = fp[k] = 0;
    int sp = 0;
    uint32_t cnt = 0;
    // u32 chunk / slot indices: run_get_rows keeps batches below 2^31 rows
    uint32_t chunk = (uint32_t)gid;
    uint32_t ri = 0;
    uint32_t slot = chunk * 8;
    // output: the labels of a chunk's rows are packed back to back in the
    // chunk's 8*K-label region (rows with > K labels are left out for the
    // overflow pass), so the compaction is a contiguous copy per chunk
    uint32_t running = 0, chunk_total = 0;
    // the current row's first label in its chunk's region (recomputed, not held)
    auto slot_ptr = [&]() -> uint32_t * { return p.temp + (uint64_t)chunk * 8 * p.K + running; };

    // SMALLK: K == kStageLabels, every kept label fits the stage
    auto emit = [&](uint32_t pos, uint32_t label) {
        if (pos < kStageLabels) stage[pos] = label;
        else if (!SMALLK && pos < p.K) gst(slot_ptr() + pos, label);  // past the LDS stage
    };

    // rows: chunks of 8 consecutive slots per group, ids preloaded 2 per lane as
    // u32 (ids >= num_rows clamp to 0xFFFFFFFF >= num_rows)
    uint32_t r0 = 0, r1 = 0;
    auto clamp_row = [&](uint64_t r) -> uint32_t { return r < p.num_rows ? (uint32_t)r : 0xFFFFFFFFu; };
    auto load_chunk = [&]() {
        const uint64_t sb = (uint64_t)chunk * 8 + 2 * c;
        r0 = sb < p.n ? clamp_row(gld(p.rows + sb)) : 0u;
        r1 = sb + 1 < p.n ? clamp_row(gld(p.rows + sb + 1)) : 0u;
    };
    bool active = (uint64_t)slot < p.n, fresh = active;  // fresh: the slot's row has not been started
    if (active) load_chunk();

    while (true) {
        if (active && !fresh && sp == 0) {  // row done: flush its stage, count, next slot
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // a row of more than K labels stores nothing (the direct pass writes
            // it): with K < kStageLabels its stage would run past the chunk's region
            const uint32_t lim = cnt > p.K ? 0u : cnt < kStageLabels ? cnt : kStageLabels;
            uint32_t *const dst = slot_ptr();
            for (uint32_t q = c; q < lim; q += 4) gst(dst + q, (uint32_t)stage[q]);
            if (c == 0) {
                gst(p.counts + slot, cnt);
                if (cnt > p.K) {
                    const unsigned long long k = atomicAdd(&p.scalars[1], 1ull);
                    gst(p.ovf_list + k, slot);
                }
            }
            if (cnt <= p.K) running += cnt;
            chunk_total += cnt;
            if ((ri == 7 || slot + 1 == p.n) && c == 0) gst(p.chunk_counts + chunk, chunk_total);
            if (++ri == 8) {
                ri = 0;
                running = 0;
                chunk_total = 0;
                chunk += (uint32_t)ngroups;
                if ((uint64_t)chunk * 8 < p.n) load_chunk();
            }
            slot = chunk * 8 + ri;
            active = (uint64_t)chunk * 8 + ri < p.n;
            fresh = active;
        }
        if (!__any(active)) break;
        if (!active) continue;

        // the node to visit: the root for a fresh row, else the next pending child
        uint64_t w0, w1;
        uint32_t j;
        bool go = true;
        if (fresh) {
            fresh = false;
            cnt = 0;
            const uint32_t mine = (ri & 1) ? r1 : r0;
            j = (uint32_t)__shfl((int)mine, (int)(gbase + (ri >> 1)), 64);
            w0 = lds_nodes[0];
            w1 = lds_nodes[1];
            if ((uint64_t)j >= p.num_rows) {
                if (c == 0) atomicOr(&p.scalars[2], 1ull);
                go = false;
            }
        } else {
            uint32_t top = fp[0];
            const uint32_t cs = (uint32_t)__builtin_ctz(top & 0xFFu);
            top &= top - 1;
            fp[0] = top;
            const uint32_t w = (top >> 8) + cs;
            const uint32_t jsel = (cs & 1) ? jc1[0] : jc0[0];
            j = (uint32_t)__shfl((int)jsel, (int)(gbase + (cs >> 1)), 64);
            if ((top & 0xFFu) == 0) {
#pragma unroll
                for (int k = 0; k < (int)kFastMaxd - 1; ++k) {
                    jc0[k] = jc0[k + 1];
                    jc1[k] = jc1[k + 1];
                    fp[k] = fp[k + 1];
                }
                --sp;
            }
            w0 = lds_nodes[2 * w];
            w1 = lds_nodes[2 * w + 1];
        }
        if (!go) continue;

        const uint64_t base = w0 & M48;
        const uint32_t a = (uint32_t)(w0 >> 56);
        const uint32_t kind = (uint32_t)(w0 >> 48) & 7u;
        // the labels of this lane's two MASK8 children (masks m0, m1 with leaf
        // labels l0.., l1..) at their place among the node's labels
        auto emit_children = [&](uint32_t m0, uint32_t m1, uint32_t l0, uint32_t l1) {
            const uint32_t s0 = (uint32_t)__builtin_popcount(m0) + (uint32_t)__builtin_popcount(m1);
            uint32_t total;
            uint32_t pos = cnt + quad_exclusive_sum(s0, c, total);
            for (; m0; m0 &= m0 - 1) emit(pos++, l0 + (uint32_t)__builtin_ctz(m0));
            for (; m1; m1 &= m1 - 1) emit(pos++, l1 + (uint32_t)__builtin_ctz(m1));
            cnt += total;
        };
        if (P2 && ((w0 >> 48) & 15u) == 15u) {  // KIND_PACK2 (kind PACK + flag): the subtree below at j
            // one coalesced 64-byte block read; staged in LDS, each lane takes
            // children 2c, 2c+1 of the node: their m1 bytes, then the leaf
            // masks of their set children (offsets by quad scans)
            const uint32_t lgs = (uint32_t)(w0 >> 52) & 15u;  // log2(span)
            const uint32_t t = j & ((1u << lgs) - 1u);
            const uint4 q = gld_at_nt<uint4, NT>(base + (uint64_t)(j >> lgs) * kPack2Block + 16u * c);
            ((AS_LDS u32x4_t *)pk)[c] = u32x4_t{q.x, q.y, q.z, q.w};
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const AS_LDS uint8_t *pb = (const AS_LDS uint8_t *)pk;
            uint32_t s = pb[t];
            if (pb[0] == 0) {
                // rare (spilled block): the position's record is copied into the
                // group's LDS slot -- list = u16 start[S+1], then the records;
                // builders keep every record <= 64 bytes (mbrwt_internal.hpp)
                const uint64_t la = ((uint64_t)pk[3] << 32) | pk[2];
                const uint32_t s0 = gld_at<uint16_t>(la + 2ull * t), len = gld_at<uint16_t>(la + 2ull * t + 2) - s0;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();  // every lane has read the list address
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                AS_LDS uint8_t *pw = (AS_LDS uint8_t *)pk;
                for (uint32_t o = c; o < len; o += 4) pw[o] = gld_at<uint8_t>(la + s0 + o);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                s = 0;
            }
            const uint32_t fc = (uint32_t)w1;
            // the record walk: lane c takes children 2c, 2c+1 of the node
            auto walk = [&](auto rd) {
                const uint32_t m2 = rd(s);
                const uint32_t A0 = 2 * c;
                const uint32_t bA0 = (m2 >> A0) & 1u, bA1 = (m2 >> (A0 + 1)) & 1u;
                const uint32_t i0 = s + 1 + (uint32_t)__builtin_popcount(m2 & ((1u << A0) - 1u));
                const uint32_t m10 = bA0 ? rd(i0) : 0u;
                const uint32_t m11 = bA1 ? rd(i0 + bA0) : 0u;
                const uint32_t n1 = (uint32_t)__builtin_popcount(m10) + (uint32_t)__builtin_popcount(m11);
                uint32_t n1_tot;
                const uint32_t o2 = s + 1 + (uint32_t)__builtin_popcount(m2) + quad_exclusive_sum(n1, c, n1_tot);
                uint32_t nl = 0;
#pragma nounroll
                for (uint32_t k = 0; k < n1; ++k) nl += (uint32_t)__builtin_popcount(rd(o2 + k));
                uint32_t ltot;
                uint32_t pos = cnt + quad_exclusive_sum(nl, c, ltot);
                uint32_t o = o2;
#pragma unroll
                for (uint32_t h = 0; h < 2; ++h) {
                    uint32_t x = h ? m11 : m10;
                    if (!x) continue;
                    const uint32_t fa = (uint32_t)lds_nodes[2 * (fc + A0 + h) + 1];  // first MASK8 child of A
                    for (; x; x &= x - 1) {
                        const uint32_t l = (uint32_t)(lds_nodes[2 * (fa + (uint32_t)__builtin_ctz(x)) + 1] >> 32);
                        for (uint32_t lm = rd(o++); lm; lm &= lm - 1) emit(pos++, l + (uint32_t)__builtin_ctz(lm));
                    }
                }
                return ltot;
            };
            const uint32_t ltot = walk([&](uint32_t o) -> uint32_t { return pb[o]; });
            cnt += ltot;
            continue;
        }
        if (kind == KIND_PACK) {
            const uint32_t t = j % kPackSpan, below = (1u << t) - 1u;
            const uint4 q = gld_at_nt<uint4, NT>(base + (uint64_t)(j / kPackSpan) * kPackBlock + 16u * c);
            const uint32_t lo = q.x & 0xFFFFu, hi = q.x >> 16;  // bits of children 2c, 2c+1
            const uint32_t b0 = (lo >> t) & 1u, b1 = (hi >> t) & 1u;
            uint32_t pairs;
            const uint32_t pre = quad_exclusive_sum((uint32_t)__builtin_popcount(q.x), c, pairs);
            ((AS_LDS u32x4_t *)pk)[c] = u32x4_t{q.x, q.y, q.z, q.w};
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t o0 = pre + (uint32_t)__builtin_popcount(lo & below);
            const uint32_t o1 = pre + (uint32_t)__builtin_popcount(lo) + (uint32_t)__builtin_popcount(hi & below);
            uint32_t m0 = 0, m1 = 0, l0 = 0, l1 = 0;
            const uint32_t fc = (uint32_t)w1;
            if (pairs <= kPackArea) {
                const AS_LDS uint8_t *pb = (const AS_LDS uint8_t *)pk;
                if (b0) m0 = pb[pack_area_byte(o0)];
                if (b1) m1 = pb[pack_area_byte(o1)];
            } else {  // spilled block: area bytes 0..7 hold the list's address
                const uint64_t sa = ((uint64_t)pk[2] << 32) | pk[1];
                if (b0) m0 = gld_at_nt<uint8_t, NT>(sa + o0);
                if (b1) m1 = gld_at_nt<uint8_t, NT>(sa + o1);
            }
            if (b0) l0 = (uint32_t)(lds_nodes[2 * (fc + 2 * c) + 1] >> 32);
            if (b1) l1 = (uint32_t)(lds_nodes[2 * (fc + 2 * c + 1) + 1] >> 32);
            emit_children(m0, m1, l0, l1);
            continue;
        }
        if (kind == KIND_MASK8) {  // leaves below: labels from the mask
            const uint32_t m = gld_at_nt<uint8_t, NT>(base + j);
            const uint32_t l0 = (uint32_t)(w1 >> 32);
#pragma unroll
            for (uint32_t q = 0; q < 2; ++q) {
                const uint32_t cc = 2 * c + q;
                if ((m >> cc) & 1u) emit(cnt + (uint32_t)__builtin_popcount(m & ((1u << cc) - 1u)), l0 + cc);
            }
            cnt += (uint32_t)__builtin_popcount(m);
            continue;
        }
        // KIND_PLANE: one coalesced 64-byte block read, 2 children per lane
        const uint32_t stride = 1u << ((uint32_t)(w0 >> 52) & 15u);
        const uint32_t t = j & 31, below = (1u << t) - 1u;
        uint32_t b0 = 0, b1 = 0, j0 = 0, j1 = 0;
        if (2 * c < a) {
            const uint4 q = gld_at_nt<uint4, NT>(base + (uint64_t)(j >> 5) * stride + 16u * c);
            b0 = (q.y >> t) & 1u;
            b1 = (2 * c + 1 < a) ? (q.w >> t) & 1u : 0u;
            j0 = q.x + (uint32_t)__builtin_popcount(q.y & below);
            j1 = q.z + (uint32_t)__builtin_popcount(q.w & below);
        }
        const uint32_t fc = (uint32_t)w1;
        if (!P2 && ((w0 >> 51) & 1u)) {  // FLAG_MASK_CHILDREN: the set children's mask reads, together
            uint32_t m0 = 0, m1 = 0, l0 = 0, l1 = 0;
            if (b0) {
                const uint32_t w = fc + 2 * c;
                m0 = gld_at_nt<uint8_t, NT>((lds_nodes[2 * w] & M48) + j0);
                l0 = (uint32_t)(lds_nodes[2 * w + 1] >> 32);
            }
            if (b1) {
                const uint32_t w = fc + 2 * c + 1;
                m1 = gld_at_nt<uint8_t, NT>((lds_nodes[2 * w] & M48) + j1);
                l1 = (uint32_t)(lds_nodes[2 * w + 1] >> 32);
            }
            emit_children(m0, m1, l0, l1);
            continue;
        }
        const uint32_t P = quad_or((b0 | (b1 << 1)) << (2 * c));  // child k <- bit k
        if (P) {
            if (sp >= (int)kFastMaxd) {
                if (c == 0) atomicOr(&p.scalars[2], 2ull);
                continue;
            }
#pragma unroll
            for (int k = kFastMaxd - 1; k > 0; --k) {
                jc0[k] = jc0[k - 1];
                jc1[k] = jc1[k - 1];
                fp[k] = fp[k - 1];
            }
            jc0[0] = j0;
            jc1[0] = j1;
            fp[0] = (fc << 8) | P;
            ++sp;
        }
    }
}

// k_compact_chunks: output of k_traverse_fast2 -> CSR.  The traversal packs
// the labels of the 8 rows of chunk ch back to back at temp + ch*8*K (rows
// with more than K labels left out for the overflow pass) and counts labels
// per row and per chunk; the scan runs over the chunk counts only.  Here 8
// lanes per chunk (8 chunks per wave) write the chunk's 8 row offsets (chunk
// offset + in-chunk prefix) and copy the packed labels; each lane issues its
// (up to 8) label reads before any store.  Contiguous reads and writes.
__global__ __launch_bounds__(256) void k_compact_chunks(const uint32_t *__restrict__ counts,
                                                        const uint64_t *__restrict__ chunk_offsets,
                                                        const uint32_t *__restrict__ temp, uint32_t K,
                                                        uint64_t *__restrict__ offsets, uint32_t *__restrict__ cols,
                                                        uint64_t n, const uint32_t *__restrict__ label_map,
                                                        uint32_t map_lds) {
    const LabelMap lmap = stage_label_map(label_map, map_lds);
    const uint32_t lane = threadIdx.x & 63, sub = lane & 7, gb = lane & ~7u;
    const uint64_t nch = (n + 7) / 8;
    const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) >> 3;
    for (uint64_t ch = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; ch < nch; ch += stride) {
        const uint64_t r0 = ch * 8;
        const uint32_t nr = (uint32_t)(n - r0 < 8 ? n - r0 : 8);
        const uint64_t base = gld(chunk_offsets + ch);
        const uint32_t mine = sub < nr ? gld(counts + r0 + sub) : 0u;
        uint32_t cr[8];
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) cr[r] = (uint32_t)__shfl((int)mine, (int)(gb + r), 64);
        uint32_t pre[9], buf[9];
        pre[0] = buf[0] = 0;
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) {
            pre[r + 1] = pre[r] + cr[r];
            buf[r + 1] = buf[r] + (cr[r] <= K ? cr[r] : 0u);  // overflow rows hold no labels here
        }
        if (sub < nr) gst(offsets + r0 + sub, base + pre[sub]);
        if (sub == 0 && r0 + nr == n) gst(offsets + n, base + pre[nr]);
        const uint32_t stored = buf[nr];
        const uint32_t *src = temp + ch * 8 * K;
        if (stored == pre[nr]) {  // no overflow row in the chunk: packed label i is output label base + i
            for (uint32_t i0 = 0; i0 < stored; i0 += 64) {
                uint32_t v[8];
#pragma unroll
                for (uint32_t k = 0; k < 8; ++k) {
                    const uint32_t i = i0 + sub + 8 * k;
                    v[k] = i < stored ? lmap(gld(src + i)) : 0u;
                }
#pragma unroll
                for (uint32_t k = 0; k < 8; ++k) {
                    const uint32_t i = i0 + sub + 8 * k;
                    if (i < stored) gst(cols + base + i, v[k]);
                }
            }
            continue;
        }
        for (uint32_t i0 = 0; i0 < stored; i0 += 64) {
            uint32_t v[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                const uint32_t i = i0 + sub + 8 * k;
                v[k] = i < stored ? lmap(gld(src + i)) : 0u;
            }
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                const uint32_t i = i0 + sub + 8 * k;
                if (i >= stored) continue;
                // the row owning packed label i (empty rows before it share its buf value)
                uint32_t prow = pre[0], brow = buf[0];
#pragma unroll
                for (uint32_t r = 1; r < 8; ++r)
                    if (r < nr && buf[r] <= i) {
                        prow = pre[r];
                        brow = buf[r];
                    }
                gst(cols + base + prow + (i - brow), v[k]);
            }
        }
    }
}
namespace nodes {

Trav fast2_traverse(const Ctx &c) {
    Trav t;
    const bool p2 = c.tree.has_pack2;
    if (!(c.tree.fast_shape && c.tree.lds_complete && c.kernel_variant == 0 &&
          (!p2 || (c.tree.push_frames <= 1 && !c.tree.has_mask_children))))
        return t;
    const bool nt = nt_reads(c);
    const bool smallk = auto_slots(c) == kStageLabels;
    t.G = 4;
    t.fast = true;
    t.name = p2 ? "k_traverse_fast2/pack2" : "k_traverse_fast2";
#define FAST2(P)                                                                                          \
    if (smallk) t.lane_fn = nt ? (TravFn)k_traverse_fast2<true, true, P> : (TravFn)k_traverse_fast2<false, true, P>; \
    else t.lane_fn = nt ? (TravFn)k_traverse_fast2<true, false, P> : (TravFn)k_traverse_fast2<false, false, P>;
    if (p2) {
        FAST2(true)
    } else {
        FAST2(false)
    }
#undef FAST2
    t.fn = reinterpret_cast<const void *>(t.lane_fn);
    return t;
}

hipError_t compact_chunks(const Ctx &c, const uint32_t *d_counts, const uint64_t *d_chunk_offsets, const uint32_t *temp,
                          uint32_t K, uint64_t *d_offsets, uint32_t *d_cols, uint64_t n, hipStream_t s) {
    const uint32_t map_lds = label_map_lds(c);
    const uint64_t g = std::min<uint64_t>(((n + 7) / 8 + 31) / 32, 1u << 20);  // no grid-stride rounds
    hipLaunchKernelGGL(k_compact_chunks, dim3((unsigned)g), dim3(256), map_lds * 4, s, d_counts, d_chunk_offsets, temp, K,
                       d_offsets, d_cols, n, (const uint32_t *)c.d_label_map, map_lds);
    return hipGetLastError();
}

}  // namespace nodes
}  // namespace mbrwt
