// nodes_traverse.hip -- the general kernels of the per-node images (gfx950 /
// CDNA4): k_traverse and k_traverse_group in four modes, k_compact, k_get.
//
// Hot path: BRWT::get_row (BRWT.cpp:26-53) and the bit_vector_rrr<63>
// operator[] / rank1 it rides on (bit_vector.cpp:857-888), restated over the
// sibling-interleaved device image (mbrwt_internal.hpp).
//
// k_traverse: one lane per query row, depth-first over the tree in the
// reference's child order, with the pending frames of the descent in a
// register shift-stack (static register indices only, no scratch).  Lanes
// refill themselves with the next row of their grid-stride sequence as soon
// as their row finishes, so a wave stays full while rows of different
// lengths are in flight.  Every visit of an internal node at position j is
// ONE block read (64 B for arity 8) that yields the index bit and rank of all
// children at j; the rank of child c is rank_c(block) + popc(bits_c & below).
//
// Output: pass 1 (MODE_SLOTS) writes each row's labels into a fixed slot of K
// labels and its count; an exclusive scan gives CSR offsets; k_compact copies
// slots to the CSR; rows with more than K labels are re-traversed straight
// into the CSR (MODE_DIRECT over the overflow list only).  MODE_WORK counts
// visits and labels, MODE_COUNT labels per column (query.hip drives them all).
#include "nodes_walk.hpp"
#include "pack_block.hpp"

namespace mbrwt {

// MODE_DIRECT / MODE_COUNT write final columns; the slot modes keep pre-order
// indices and the compaction maps them
__device__ __forceinline__ uint32_t final_label(const uint32_t *map, uint32_t label) {
    return map ? gld(map + label) : label;
}

// decoded node record
struct NodeInfo {
    uint64_t base;
    uint32_t first_child;
    uint32_t label;
    uint32_t stride;
    uint32_t arity;
    uint32_t kind;
    uint32_t flags;
};
__device__ __forceinline__ NodeInfo decode(uint64_t w0, uint64_t w1) {
    NodeInfo n;
    n.base = w0 & ((1ull << 48) - 1);
    n.kind = (uint32_t)(w0 >> 48) & 7u;
    n.flags = (uint32_t)(w0 >> 51) & 1u;
    if (n.kind == KIND_PACK && n.flags) n.kind = KIND_PACK2;  // CNode encoding (mbrwt_internal.hpp)
    n.stride = 1u << ((uint32_t)(w0 >> 52) & 15u);
    n.arity = (uint32_t)(w0 >> 56);
    n.first_child = (uint32_t)w1;
    n.label = (uint32_t)(w1 >> 32);
    return n;
}

template <typename MaskT>
__device__ __forceinline__ int ctz_m(MaskT m) {
    if constexpr (sizeof(MaskT) == 8) return __builtin_ctzll(m);
    else return __builtin_ctz(m);
}

template <int MAXD, typename MaskT>
struct Frames {
    uint32_t node[MAXD];
    uint32_t pos[MAXD];
    MaskT rem[MAXD];
    int sp;
    __device__ __forceinline__ void push(uint32_t v, uint32_t j, MaskT m) {
#pragma unroll
        for (int k = MAXD - 1; k > 0; --k) {
            node[k] = node[k - 1];
            pos[k] = pos[k - 1];
            rem[k] = rem[k - 1];
        }
        node[0] = v;
        pos[0] = j;
        rem[0] = m;
        ++sp;
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int k = 0; k < MAXD - 1; ++k) {
            node[k] = node[k + 1];
            pos[k] = pos[k + 1];
            rem[k] = rem[k + 1];
        }
        --sp;
    }
};

// Per-lane sink for the labels of the current row.
template <int MODE>
struct Sink {
    uint32_t cnt;
    uint64_t slot_base;  // MODE_SLOTS: bi*K ; MODE_DIRECT: offsets[bi]
    uint64_t visits;
    __device__ __forceinline__ void emit(const TravParams &p, uint32_t label) {
        if constexpr (MODE == MODE_SLOTS) {
            if (cnt < p.K) gst(p.temp + slot_base + cnt, label);
        } else if constexpr (MODE == MODE_DIRECT) {
            gst(p.cols + slot_base + cnt, final_label(p.label_map, label));
        } else if constexpr (MODE == MODE_COUNT) {
            atomicAdd(&p.label_counts[final_label(p.label_map, label)], 1ull);
        }
        ++cnt;
    }
};

template <typename MaskT>
__device__ __forceinline__ MaskT arity_mask(uint32_t a) {
    return a >= 8 * sizeof(MaskT) ? ~(MaskT)0 : (((MaskT)1 << a) - 1);
}

// Enter dnode v at position j of its children image (v's own index bit at
// this position is known to be set, or v is the super-root).
template <int MAXD, typename MaskT, int MODE>
__device__ __forceinline__ void enter(const TravParams &p, Frames<MAXD, MaskT> &st, Sink<MODE> &sk, uint32_t v,
                                      uint32_t j) {
    const DevNode nd = gld(p.nodes + v);
    const uint8_t kind = nd.kind;
    const uint32_t a = nd.arity;
    const uint64_t base = nd.base;
    if constexpr (MODE == MODE_WORK) sk.visits += a;  // operator[] on every child (BRWT.cpp:30)
    if (kind == KIND_PACKT) {  // the whole subtree below v at j, DFS pre-order
        Pack2Block pb;
        pb.load(base, j, nd.stride);
        const bool ok = packt_walk(
            p.nodes, v, [&](uint32_t o) { return pb.byte(o); }, pb.start(j % nd.stride),
            [&](uint32_t label) { sk.emit(p, label); },
            [&](uint32_t ar) {
                if constexpr (MODE == MODE_WORK) sk.visits += ar;
            });
        if (!ok) atomicOr(&p.scalars[2], 2ull);
        return;
    }
    if (kind == KIND_PACK2) {  // the whole subtree below v at j, in pre-order
        Pack2Block pb;
        pb.load(base, j, nd.stride);
        const uint32_t s = pb.start(j % nd.stride);
        const uint32_t m2 = pb.byte(s);
        uint32_t o1 = s + 1, o2 = s + 1 + (uint32_t)__builtin_popcount(m2);
        for (uint32_t A = 0; A < a; ++A) {
            if (!((m2 >> A) & 1u)) continue;
            const DevNode na = gld(p.nodes + nd.first_child + A);
            if constexpr (MODE == MODE_WORK) sk.visits += na.arity;
            for (uint32_t x = pb.byte(o1++); x; x &= x - 1) {
                const DevNode nb = gld(p.nodes + na.first_child + (uint32_t)__builtin_ctz(x));
                if constexpr (MODE == MODE_WORK) sk.visits += nb.arity;
                for (uint32_t m = pb.byte(o2++); m; m &= m - 1) sk.emit(p, nb.label + (uint32_t)__builtin_ctz(m));
            }
        }
        return;
    }
    if (kind == KIND_PACK) {  // children are MASK8 nodes: resolve them here, in child order
        PackBlock pb;
        pb.load(base, j);
        const uint32_t t = j % kPackSpan;
        uint32_t o = 0;
        for (uint32_t k = 0; k < a; ++k) {
            const uint32_t bk = pb.bits(k);
            if ((bk >> t) & 1u) {
                const DevNode ch = gld(p.nodes + nd.first_child + k);
                if constexpr (MODE == MODE_WORK) sk.visits += ch.arity;
                uint32_t m = pb.mask(o + (uint32_t)__builtin_popcount(bk & ((1u << t) - 1u)));
                while (m) {
                    sk.emit(p, ch.label + (uint32_t)__builtin_ctz(m));
                    m &= m - 1;
                }
            }
            o += (uint32_t)__builtin_popcount(bk);
        }
        return;
    }
    if (kind == KIND_PLANE) {
        const uint64_t blk = base + (uint64_t)(j >> 5) * nd.stride;
        const uint32_t t = j & 31;
        MaskT m = 0;
        for (uint32_t c = 0; c < a; c += 2) {
            const uint4 q = gld_at<uint4>(blk + 8u * c);
            m |= (MaskT)((q.y >> t) & 1u) << c;
            m |= (MaskT)((q.w >> t) & 1u) << (c + 1);
        }
        m &= arity_mask<MaskT>(a);
        if (m) {
            if (st.sp >= MAXD) {
                atomicOr(&p.scalars[2], 2ull);  // stack overflow: host picked MAXD too small
                return;
            }
            st.push(v, j, m);
        }
        return;
    }
    // all children are leaves: one mask per position
    uint64_t m;
    if (kind == KIND_MASK8) m = gld_at<uint8_t>(base + j);
    else if (kind == KIND_MASK16) m = gld_at<uint16_t>(base + 2ull * j);
    else if (kind == KIND_MASK32) m = gld_at<uint32_t>(base + 4ull * j);
    else m = gld_at<uint64_t>(base + 8ull * j);
    if (nd.flags & FLAG_CONSEC_LABELS) {
        const uint32_t l0 = nd.label;
        while (m) {
            sk.emit(p, l0 + (uint32_t)__builtin_ctzll(m));
            m &= m - 1;
        }
    } else {
        const uint32_t fc = nd.first_child;
        while (m) {
            sk.emit(p, gld(p.nodes + fc + __builtin_ctzll(m)).label);
            m &= m - 1;
        }
    }
}

// One step: take the next set child of the top frame and descend into it.
template <int MAXD, typename MaskT, int MODE>
__device__ __forceinline__ void step(const TravParams &p, Frames<MAXD, MaskT> &st, Sink<MODE> &sk) {
    const uint32_t u = st.node[0];
    const uint32_t j = st.pos[0];
    MaskT m = st.rem[0];
    const int c = ctz_m(m);
    m &= m - 1;
    st.rem[0] = m;
    const DevNode nu = gld(p.nodes + u);
    const uint32_t v = nu.first_child + (uint32_t)c;
    const uint64_t blk = nu.base + (uint64_t)(j >> 5) * nu.stride + 8u * c;
    if (m == 0) st.pop();  // the frame has no children left: drop it before descending
    const DevNode nv = gld(p.nodes + v);
    if (nv.kind == KIND_LEAF) {
        sk.emit(p, nv.label);
        return;
    }
    const uint2 rb = gld_at<uint2>(blk);  // {rank before block, bits}
    const uint32_t below = (1u << (j & 31)) - 1u;
    const uint32_t jv = rb.x + (uint32_t)__builtin_popcount(rb.y & below);  // rank1(j) - 1
    enter<MAXD, MaskT, MODE>(p, st, sk, v, jv);
}

template <int MAXD, typename MaskT, int MODE>
__global__ __launch_bounds__(256) void k_traverse(TravParams p) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    Frames<MAXD, MaskT> st;
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {
        st.node[k] = 0;
        st.pos[k] = 0;
        st.rem[k] = 0;
    }
    st.sp = 0;
    Sink<MODE> sk;
    sk.cnt = 0;
    sk.visits = 0;
    sk.slot_base = 0;
    uint64_t bi = 0;
    unsigned long long acc_visits = 0, acc_labels = 0;

    auto begin_row = [&]() {
        bi = (MODE == MODE_DIRECT) ? (uint64_t)gld(p.slot_list + s) : (p.order ? (uint64_t)gld(p.order + s) : s);
        const uint64_t row = gld(p.rows + bi);
        sk.cnt = 0;
        sk.visits = 0;
        if constexpr (MODE == MODE_SLOTS) sk.slot_base = bi * p.K;
        if constexpr (MODE == MODE_DIRECT) sk.slot_base = gld(p.offsets + bi);
        if (row >= p.num_rows) {
            atomicOr(&p.scalars[2], 1ull);
            return;
        }
        enter<MAXD, MaskT, MODE>(p, st, sk, 0u, (uint32_t)row);
        if constexpr (MODE == MODE_WORK) {
            // folded root: its own probe counts once, its children's only if its bit is set
            if (p.folded) sk.visits = sk.visits + 1 - ((st.sp == 0 && sk.cnt == 0) ? (uint64_t)gld(p.nodes).arity : 0ull);
        }
    };
    auto end_row = [&]() {
        if constexpr (MODE == MODE_SLOTS) {
            gst(p.counts + bi, sk.cnt);
            if (sk.cnt > p.K) {
                const unsigned long long k = atomicAdd(&p.scalars[1], 1ull);
                gst(p.ovf_list + k, (uint32_t)bi);
            }
        }
        if constexpr (MODE == MODE_WORK) {
            acc_visits += sk.visits;
            acc_labels += sk.cnt;
        }
    };

    bool active = s < p.n;
    if (active) begin_row();
    while (true) {
        if (active && st.sp == 0) {
            end_row();
            s += gstride;
            active = s < p.n;
            if (active) begin_row();
        }
        if (!__any(active)) break;
        if (active && st.sp > 0) step<MAXD, MaskT, MODE>(p, st, sk);
    }
    if constexpr (MODE == MODE_WORK) {
        if (acc_visits) atomicAdd(&p.scalars[3], acc_visits);
        if (acc_labels) atomicAdd(&p.scalars[4], acc_labels);
    }
}

// ------------------------------------------------------------------------
// k_traverse_group: G lanes cooperate on one row (G = pow2ceil(max arity)).
// Visiting node u at position j, lane c of the group reads child c's
// {rank, bits} pair: the G 8-byte reads of one block are adjacent, so the
// memory pipeline sees ONE coalesced request per visit instead of one per
// lane-load (random requests, not bytes, bound this path: tools/
// gather_probe.hip).  Each stack level holds, per lane, the child index j_c
// of child c and, uniform in the group, the parent's first child and the
// mask of children still to visit.  Children are taken in order (DFS, the
// reference's output order); the index of the next child comes from lane
// c's register through a cross-lane shuffle.
// ------------------------------------------------------------------------
// children per lane, one 16-byte read per visit (4: 12.1 against 11.1 ms, profiles/r01/exp_c3_refseq_sweep.log)
constexpr int kGroupCpl = 2;
// waves per SIMD asked of the register allocator (none: 11.5 against 11.1 ms, profiles/r01/exp_c3_refseq_sweep.log)
constexpr int kGroupWpe = 8;

template <int MAXD, typename MaskT>
struct GroupFrames {
    uint32_t jc[MAXD][kGroupCpl];  // per lane: position of child c*kGroupCpl+k in its own image
    uint32_t fc[MAXD];       // uniform: dnode of child 0
    MaskT pend[MAXD];        // uniform: children still to take (bit i = child i)
    int sp;
    __device__ __forceinline__ void push(const uint32_t (&j)[kGroupCpl], uint32_t f, MaskT p) {
#pragma unroll
        for (int k = MAXD - 1; k > 0; --k) {
#pragma unroll
            for (int q = 0; q < kGroupCpl; ++q) jc[k][q] = jc[k - 1][q];
            fc[k] = fc[k - 1];
            pend[k] = pend[k - 1];
        }
#pragma unroll
        for (int q = 0; q < kGroupCpl; ++q) jc[0][q] = j[q];
        fc[0] = f;
        pend[0] = p;
        ++sp;
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int k = 0; k < MAXD - 1; ++k) {
#pragma unroll
            for (int q = 0; q < kGroupCpl; ++q) jc[k][q] = jc[k + 1][q];
            fc[k] = fc[k + 1];
            pend[k] = pend[k + 1];
        }
        --sp;
    }
};

// Per-group label sink: the labels of the current row are staged in LDS
// (kStageLabels per group) and written out once, contiguously, when the row
// ends.  Stores count in vmcnt on CDNA4, so a store issued inside the
// descent would hold up the wait of the next dependent block load; staging
// keeps the descent free of global stores.  Labels past the stage go
// straight to global memory (rare: rows with > kStageLabels labels).

template <int MODE>
struct GroupSink {
    uint32_t cnt;        // labels emitted so far (uniform)
    uint64_t slot_base;  // MODE_SLOTS: bi*K ; MODE_DIRECT: offsets[bi]
    uint64_t visits;
    AS_LDS uint32_t *stage;  // this group's LDS stage
    // lane-parallel emission: `label` goes to position cnt + rank
    __device__ __forceinline__ void put(const TravParams &p, uint32_t rank, uint32_t label) {
        const uint32_t pos = cnt + rank;
        if constexpr (MODE == MODE_DIRECT || MODE == MODE_COUNT) label = final_label(p.label_map, label);
        if constexpr (MODE == MODE_SLOTS || MODE == MODE_DIRECT) {
            if (pos < kStageLabels) {
                stage[pos] = label;
                return;
            }
        }
        if constexpr (MODE == MODE_SLOTS) {
            if (pos < p.K) gst(p.temp + slot_base + pos, label);
        } else if constexpr (MODE == MODE_DIRECT) {
            gst(p.cols + slot_base + pos, label);
        } else if constexpr (MODE == MODE_COUNT) {
            atomicAdd(&p.label_counts[label], 1ull);
        }
    }
    // end of row: the group's lanes copy the stage out, contiguously
    __device__ __forceinline__ void flush(const TravParams &p, uint32_t c, uint32_t G) {
        if constexpr (MODE == MODE_SLOTS || MODE == MODE_DIRECT) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            uint32_t lim = cnt < kStageLabels ? cnt : kStageLabels;
            if constexpr (MODE == MODE_SLOTS) lim = lim < p.K ? lim : p.K;
            for (uint32_t pos = c; pos < lim; pos += G) {
                if constexpr (MODE == MODE_SLOTS) gst(p.temp + slot_base + pos, (uint32_t)stage[pos]);
                else gst(p.cols + slot_base + pos, (uint32_t)stage[pos]);
            }
        }
    }
};

// spread the low G bits of x to every kGroupCpl-th bit position
__device__ __forceinline__ uint64_t spread_bits(uint64_t x, uint32_t G) {
    uint64_t r = 0;
    for (uint32_t i = 0; i < G; ++i) r |= ((x >> i) & 1ull) << (i * kGroupCpl);
    return r;
}

template <int MAXD, typename MaskT, int MODE>
__device__ __forceinline__ void group_visit(const TravParams &p, GroupFrames<MAXD, MaskT> &st, GroupSink<MODE> &sk,
                                            const NodeInfo &nd, uint32_t j, uint32_t c, uint32_t gbase,
                                            uint64_t gmask, uint32_t G) {
    const uint32_t a = nd.arity;
    const uint64_t base = nd.base;
    if constexpr (MODE == MODE_WORK) sk.visits += a;  // operator[] on every child (BRWT.cpp:30)
    if (nd.kind == KIND_PACK2) {
        // every lane walks the whole record; each emits the labels below its
        // own children at their rank among the node's labels (pre-order)
        Pack2Block pb;
        pb.load(base, j, nd.stride);
        const uint32_t s = pb.start(j % nd.stride);
        const uint32_t m2 = pb.byte(s);
        uint32_t o1 = s + 1, o2 = s + 1 + (uint32_t)__builtin_popcount(m2), total = 0;
        const uint64_t *cn = reinterpret_cast<const uint64_t *>(p.cnodes);
        for (uint32_t A = 0; A < a; ++A) {
            if (!((m2 >> A) & 1u)) continue;
            const uint32_t wa = nd.first_child + A;
            const NodeInfo na = decode(gld(cn + 2 * wa), gld(cn + 2 * wa + 1));
            if constexpr (MODE == MODE_WORK) sk.visits += na.arity;
            for (uint32_t x = pb.byte(o1++); x; x &= x - 1) {
                const uint32_t wb = na.first_child + (uint32_t)__builtin_ctz(x);
                const NodeInfo nb = decode(gld(cn + 2 * wb), gld(cn + 2 * wb + 1));
                if constexpr (MODE == MODE_WORK) sk.visits += nb.arity;
                const uint32_t lm = pb.byte(o2++);
                if (A / kGroupCpl == c) {
                    uint32_t r = total;
                    for (uint32_t mm = lm; mm; mm &= mm - 1) sk.put(p, r++, nb.label + (uint32_t)__builtin_ctz(mm));
                }
                total += (uint32_t)__builtin_popcount(lm);
            }
        }
        sk.cnt += total;
        return;
    }
    if (nd.kind == KIND_PACK) {
        // every lane holds the whole block; each emits the labels of its own
        // children at their rank among the node's labels (child order)
        PackBlock pb;
        pb.load(base, j);
        const uint32_t t = j % kPackSpan, below = (1u << t) - 1u;
        uint32_t o = 0, before = 0, total = 0;
        for (uint32_t k = 0; k < a; ++k) {
            const uint32_t bk = pb.bits(k);
            if ((bk >> t) & 1u) {
                const uint32_t m = pb.mask(o + (uint32_t)__builtin_popcount(bk & below));
                const NodeInfo ch = decode(gld(reinterpret_cast<const uint64_t *>(p.cnodes) + 2 * (nd.first_child + k)),
                                           gld(reinterpret_cast<const uint64_t *>(p.cnodes) + 2 * (nd.first_child + k) + 1));
                if constexpr (MODE == MODE_WORK) sk.visits += ch.arity;
                if (k / kGroupCpl == c) {
                    uint32_t mm = m, r = before;
                    for (; mm; mm &= mm - 1) sk.put(p, r++, ch.label + (uint32_t)__builtin_ctz(mm));
                }
                before += (uint32_t)__builtin_popcount(m);
                total += (uint32_t)__builtin_popcount(m);
            }
            o += (uint32_t)__builtin_popcount(bk);
        }
        sk.cnt += total;
        return;
    }
    if (nd.kind == KIND_PLANE) {
        const uint32_t t = j & 31;
        const uint32_t below = (1u << t) - 1u;
        uint32_t bit[kGroupCpl], jc[kGroupCpl];
#pragma unroll
        for (int q = 0; q < kGroupCpl; ++q) {
            bit[q] = 0;
            jc[q] = 0;
        }
        if (c * kGroupCpl < a) {
            const uint64_t blk = base + (uint64_t)(j >> 5) * nd.stride + 8u * kGroupCpl * c;
            uint32_t rk[kGroupCpl], bw[kGroupCpl];
#pragma unroll
            for (int h = 0; h < kGroupCpl / 2; ++h) {
                const uint4 q4 = gld_at<uint4>(blk + 16 * h);
                rk[2 * h] = q4.x;
                bw[2 * h] = q4.y;
                rk[2 * h + 1] = q4.z;
                bw[2 * h + 1] = q4.w;
            }
#pragma unroll
            for (int q = 0; q < kGroupCpl; ++q) {
                if (c * kGroupCpl + q < a) {
                    bit[q] = (bw[q] >> t) & 1u;
                    jc[q] = rk[q] + (uint32_t)__builtin_popcount(bw[q] & below);  // rank1(j) - 1
                }
            }
        }
        uint64_t P = 0;
#pragma unroll
        for (int q = 0; q < kGroupCpl; ++q) P |= spread_bits((__ballot(bit[q]) >> gbase) & gmask, G) << q;
        if (P) {
            if (st.sp >= MAXD) {
                if (c == 0) atomicOr(&p.scalars[2], 2ull);
                return;
            }
            st.push(jc, nd.first_child, (MaskT)P);
        }
        return;
    }
    uint64_t m;  // all children are leaves: one mask per position (uniform load)
    if (nd.kind == KIND_MASK8) m = gld_at<uint8_t>(base + j);
    else if (nd.kind == KIND_MASK16) m = gld_at<uint16_t>(base + 2ull * j);
    else if (nd.kind == KIND_MASK32) m = gld_at<uint32_t>(base + 4ull * j);
    else m = gld_at<uint64_t>(base + 8ull * j);
#pragma unroll
    for (int q = 0; q < kGroupCpl; ++q) {
        const uint32_t cc = c * kGroupCpl + q;
        if (cc < a && ((m >> cc) & 1u)) {
            const uint32_t label =
                (nd.flags & FLAG_CONSEC_LABELS) ? nd.label + cc
                                                 : (uint32_t)(gld(reinterpret_cast<const uint64_t *>(p.cnodes) +
                                                                  2 * (nd.first_child + cc) + 1) >> 32);
            sk.put(p, (uint32_t)__builtin_popcountll(m & ((1ull << cc) - 1ull)), label);
        }
    }
    sk.cnt += (uint32_t)__builtin_popcountll(m);
}

template <int MAXD, typename MaskT, int MODE>
__global__ __launch_bounds__(256, kGroupWpe) void k_traverse_group(TravParams p, uint32_t G) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t c = lane & (G - 1);
    const uint32_t gbase = lane & ~(G - 1);
    const uint64_t gmask = G >= 64 ? ~0ull : ((1ull << G) - 1ull);
    const uint64_t groups_per_block = blockDim.x / G;
    const uint64_t gstride = (uint64_t)gridDim.x * groups_per_block;
    uint64_t s = (uint64_t)blockIdx.x * groups_per_block + threadIdx.x / G;

    GroupFrames<MAXD, MaskT> st;
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {
#pragma unroll
        for (int q = 0; q < kGroupCpl; ++q) st.jc[k][q] = 0;
        st.fc[k] = 0;
        st.pend[k] = 0;
    }
    st.sp = 0;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stage[];  // (256 / G) * kStageLabels
    // node records [0, n_lds) after the label stages
    AS_LDS uint64_t *lds_nodes = (AS_LDS uint64_t *)((AS_LDS uint32_t *)lds_stage + (blockDim.x / G) * kStageLabels);
    const uint64_t *gnodes = reinterpret_cast<const uint64_t *>(p.cnodes);
    for (uint32_t i = threadIdx.x; i < 2 * p.n_lds; i += blockDim.x) lds_nodes[i] = gld(gnodes + i);
    __syncthreads();
    auto node_info = [&](uint32_t w) -> NodeInfo {
        if (w < p.n_lds) return decode(lds_nodes[2 * w], lds_nodes[2 * w + 1]);
        return decode(gld(gnodes + 2 * w), gld(gnodes + 2 * w + 1));
    };
    GroupSink<MODE> sk;
    sk.cnt = 0;
    sk.visits = 0;
    sk.slot_base = 0;
    sk.stage = (AS_LDS uint32_t *)lds_stage + (threadIdx.x / G) * kStageLabels;
    uint64_t bi = 0;
    unsigned long long acc_visits = 0, acc_labels = 0;

    auto begin_row = [&]() {
        bi = (MODE == MODE_DIRECT) ? (uint64_t)gld(p.slot_list + s) : (p.order ? (uint64_t)gld(p.order + s) : s);
        const uint64_t row = gld(p.rows + bi);
        sk.cnt = 0;
        sk.visits = 0;
        if constexpr (MODE == MODE_SLOTS) sk.slot_base = bi * p.K;
        if constexpr (MODE == MODE_DIRECT) sk.slot_base = gld(p.offsets + bi);
        if (row >= p.num_rows) {
            if (c == 0) atomicOr(&p.scalars[2], 1ull);
            return;
        }
        const NodeInfo nd = node_info(0);
        group_visit<MAXD, MaskT, MODE>(p, st, sk, nd, (uint32_t)row, c, gbase, gmask, G);
        if constexpr (MODE == MODE_WORK) {
            // folded root: its own probe counts once, its children's only if its bit is set
            if (p.folded) sk.visits = sk.visits + 1 - ((st.sp == 0 && sk.cnt == 0) ? (uint64_t)nd.arity : 0ull);
        }
    };
    auto end_row = [&]() {
        sk.flush(p, c, G);
        if constexpr (MODE == MODE_SLOTS) {
            if (c == 0) {
                gst(p.counts + bi, sk.cnt);
                if (sk.cnt > p.K) {
                    const unsigned long long k = atomicAdd(&p.scalars[1], 1ull);
                    gst(p.ovf_list + k, (uint32_t)bi);
                }
            }
        }
        if constexpr (MODE == MODE_WORK) {
            if (c == 0) {
                acc_visits += sk.visits;
                acc_labels += sk.cnt;
            }
        }
    };

    bool active = s < p.n;
    if (active) begin_row();
    while (true) {
        if (active && st.sp == 0) {
            end_row();
            s += gstride;
            active = s < p.n;
            if (active) begin_row();
        }
        if (!__any(active)) break;
        if (active && st.sp > 0) {
            MaskT P = st.pend[0];
            const uint32_t cs = (uint32_t)__builtin_ctzll((uint64_t)P);
            P &= P - 1;
            st.pend[0] = P;
            const uint32_t w = st.fc[0] + cs;
            uint32_t mine = st.jc[0][0];
#pragma unroll
            for (int q = 1; q < kGroupCpl; ++q)
                if ((cs % kGroupCpl) == (uint32_t)q) mine = st.jc[0][q];
            const uint32_t jw = (uint32_t)__shfl((int)mine, (int)(gbase + cs / kGroupCpl), 64);
            if (P == 0) st.pop();  // no children left at this level: drop it before descending
            const NodeInfo nd = node_info(w);
            if (nd.kind == KIND_LEAF) {
                if (c == 0) sk.put(p, 0, nd.label);
                sk.cnt += 1;
            } else {
                group_visit<MAXD, MaskT, MODE>(p, st, sk, nd, jw, c, gbase, gmask, G);
            }
        }
    }
    if constexpr (MODE == MODE_WORK) {
        if (acc_visits) atomicAdd(&p.scalars[3], acc_visits);
        if (acc_labels) atomicAdd(&p.scalars[4], acc_labels);
    }
}

// CSR compaction of the label slots (rows with <= K labels).  A workgroup
// takes 256 consecutive rows; its threads walk the tile's contiguous output
// range [offsets[r0], offsets[r0+256]) so the stores are fully coalesced,
// find each position's row by a binary search over the tile's offsets in
// LDS, and read the slot labels (a row's labels are adjacent in its slot).
constexpr int kCompactTile = 256;
__global__ __launch_bounds__(kCompactTile) void k_compact(const uint64_t *__restrict__ offsets,
                                                          const uint32_t *__restrict__ temp, uint32_t K,
                                                          uint32_t *__restrict__ cols, uint64_t n,
                                                          const uint32_t *__restrict__ label_map, uint32_t map_lds) {
    __shared__ uint64_t soff[kCompactTile + 1];
    const LabelMap lmap = stage_label_map(label_map, map_lds);
    const uint32_t t = threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile * kCompactTile < n; tile += gridDim.x) {
        const uint64_t r0 = tile * kCompactTile;
        const uint32_t rn = (uint32_t)((n - r0) < kCompactTile ? (n - r0) : kCompactTile);
        for (uint32_t i = t; i <= rn; i += kCompactTile) soff[i] = gld(offsets + r0 + i);
        __syncthreads();
        const uint64_t q0 = soff[0], q1 = soff[rn];
        for (uint64_t q = q0 + t; q < q1; q += kCompactTile) {
            uint32_t lo = 0, hi = rn;  // largest r with soff[r] <= q
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (soff[mid] <= q) lo = mid;
                else hi = mid;
            }
            const uint64_t c = soff[lo + 1] - soff[lo];
            if (c <= K) gst(cols + q, lmap(gld(temp + (r0 + lo) * K + (q - soff[lo]))));
        }
        __syncthreads();
    }
}

// Point queries: walk the column's root-to-leaf path (BRWT::get, BRWT.cpp:9-24).
__global__ __launch_bounds__(256) void k_get(const DevNode *__restrict__ nodes, const uint8_t *__restrict__ col_path,
                                             uint32_t path_len, const uint64_t *__restrict__ rows,
                                             const uint64_t *__restrict__ cols, uint64_t n, uint64_t num_rows,
                                             uint64_t num_cols, uint8_t *__restrict__ out,
                                             unsigned long long *scalars) {
    const uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gstride) {
        const uint64_t row = rows[i], col = cols[i];
        if (row >= num_rows || col >= num_cols) {
            atomicOr(&scalars[2], 1ull);
            out[i] = 0;
            continue;
        }
        uint32_t v = 0, j = (uint32_t)row;
        uint8_t bit = 0;
        for (uint32_t k = 0; k < path_len; ++k) {
            const DevNode ndv = gld(nodes + v);
            const DevNode *nd = &ndv;
            const uint32_t c = col_path[col * path_len + k];
            const uint64_t base = nd->base;
            if (nd->kind == KIND_PACKT) {  // the column's leaf below v (pre-order label), then one record walk
                uint32_t w = v;
                for (uint32_t kk = k; kk < path_len; ++kk) {
                    w = gld(nodes + w).first_child + col_path[col * path_len + kk];
                    if (gld(nodes + w).kind == KIND_LEAF) break;
                }
                const uint32_t want = gld(nodes + w).label;
                Pack2Block pb;
                pb.load(base, j, nd->stride);
                uint32_t hit = 0;
                (void)packt_walk(
                    nodes, v, [&](uint32_t o) { return pb.byte(o); }, pb.start(j % nd->stride),
                    [&](uint32_t label) { hit |= label == want; }, [](uint32_t) {});
                bit = (uint8_t)hit;
                break;
            }
            if (nd->kind == KIND_PACK2) {  // child c, its child c2, leaf c3: one record walk
                Pack2Block pb;
                pb.load(base, j, nd->stride);
                const uint32_t s = pb.start(j % nd->stride);
                const uint32_t m2 = pb.byte(s);
                if ((m2 >> c) & 1u) {
                    const uint32_t c2 = col_path[col * path_len + k + 1], c3 = col_path[col * path_len + k + 2];
                    const uint32_t i = (uint32_t)__builtin_popcount(m2 & ((1u << c) - 1u));
                    const uint32_t m1 = pb.byte(s + 1 + i);
                    if ((m1 >> c2) & 1u) {
                        uint32_t o = s + 1 + (uint32_t)__builtin_popcount(m2);  // leaf masks of earlier children
                        for (uint32_t q = 0; q < i; ++q) o += (uint32_t)__builtin_popcount(pb.byte(s + 1 + q));
                        o += (uint32_t)__builtin_popcount(m1 & ((1u << c2) - 1u));
                        bit = (uint8_t)((pb.byte(o) >> c3) & 1u);
                    }
                }
                break;
            }
            if (nd->kind == KIND_PACK) {  // child c is a MASK8 node: its bit, then its mask
                PackBlock pb;
                pb.load(base, j);
                const uint32_t t = j % kPackSpan;
                uint32_t o = 0;
                for (uint32_t q = 0; q < c; ++q) o += (uint32_t)__builtin_popcount(pb.bits(q));
                const uint32_t bc = pb.bits(c);
                if ((bc >> t) & 1u) {
                    const uint32_t m = pb.mask(o + (uint32_t)__builtin_popcount(bc & ((1u << t) - 1u)));
                    bit = (uint8_t)((m >> col_path[col * path_len + k + 1]) & 1u);
                }
                break;
            }
            if (nd->kind == KIND_PLANE) {
                const uint2 rb = gld_at<uint2>(base + (uint64_t)(j >> 5) * nd->stride + 8u * c);
                const uint32_t t = j & 31;
                if (!((rb.y >> t) & 1u)) break;
                j = rb.x + (uint32_t)__builtin_popcount(rb.y & ((1u << t) - 1u));
                v = nd->first_child + c;
                if (nodes[v].kind == KIND_LEAF) {
                    bit = 1;
                    break;
                }
            } else {
                uint64_t m;
                if (nd->kind == KIND_MASK8) m = gld_at<uint8_t>(base + j);
                else if (nd->kind == KIND_MASK16) m = gld_at<uint16_t>(base + 2ull * j);
                else if (nd->kind == KIND_MASK32) m = gld_at<uint32_t>(base + 4ull * j);
                else m = gld_at<uint64_t>(base + 8ull * j);
                bit = (uint8_t)((m >> c) & 1u);
                break;
            }
        }
        out[i] = bit;
    }
}
// ------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------
namespace nodes {
namespace {

template <int MODE>
Trav pick_traverse_mode(const Ctx &c) {
    const uint32_t depth = c.tree.stack_depth, max_arity = c.tree.max_arity;
    Trav t;
    if (c.kernel_variant == 1 || c.tree.has_packt) {  // lane-per-row kernel (A/B; the general kernel of KIND_PACKT trees)
        const bool wide = max_arity > 32;
        t.name = "k_traverse";
#define PICK(D)                                                                                      \
    if (depth <= D) {                                                                                \
        t.lane_fn = wide ? (TravFn)k_traverse<D, uint64_t, MODE> : (TravFn)k_traverse<D, uint32_t, MODE>; \
        t.fn = reinterpret_cast<const void *>(t.lane_fn);                                            \
        return t;                                                                                    \
    }
        PICK(4)
        PICK(8)
        PICK(16)
        PICK(32)
#undef PICK
        return t;
    }
    // group kernel (also the other modes of fast2's trees): G = pow2ceil(ceil(max_arity / kGroupCpl)) lanes per row
    const uint32_t need = (max_arity + kGroupCpl - 1) / kGroupCpl;
    uint32_t G = 1;
    while (G < need) G <<= 1;
    t.G = G;
#define PICKG(D)                                                                                   \
    if (depth <= D) {                                                                              \
        t.group_fn = max_arity <= 32 ? (GroupFn)k_traverse_group<D, uint32_t, MODE>                \
                                     : (GroupFn)k_traverse_group<D, uint64_t, MODE>;               \
        t.fn = reinterpret_cast<const void *>(t.group_fn);                                         \
        return t;                                                                                  \
    }
    PICKG(4)
    PICKG(8)
    PICKG(16)
    PICKG(32)
#undef PICKG
    return t;
}

// node records staged in LDS: the first min(kLdsNodes, last non-leaf + 1)
uint32_t lds_node_count(const Ctx &c) {
    return (uint32_t)std::min<size_t>({c.tree.nodes.size(), (size_t)kLdsNodes, (size_t)c.tree.lds_records});
}

size_t lds_bytes(const Ctx &c, const Trav &t) {
    if (!t.group_fn && !t.fast) return 0;
    // label stages (+ one 64-byte PACK block per group for fast2) + node records
    return (size_t)(256 / t.G) * kStageLabels * sizeof(uint32_t) + (t.fast ? 64 * kPackBlock : 0) +
           (size_t)lds_node_count(c) * sizeof(CNode);
}

int grid_for(const Ctx &c, const Trav &t, uint64_t n) {
    int dev_cus = 0;
    (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, c.device);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, t.fn, 256, lds_bytes(c, t)) != hipSuccess || per_cu <= 0)
        per_cu = 4;
    const uint64_t resident = (uint64_t)std::max(1, dev_cus) * (uint64_t)per_cu;
    // fast: 64 groups x 8-row chunks
    const uint64_t rows_per_block = t.fast ? 512 : 256 / t.G;
    const uint64_t need = (n + rows_per_block - 1) / rows_per_block;
    return (int)std::max<uint64_t>(1, std::min(need, resident));
}

}  // namespace

Trav pick_traverse(const Ctx &c, int mode) {
    switch (mode) {
        case MODE_SLOTS: return pick_traverse_mode<MODE_SLOTS>(c);
        case MODE_DIRECT: return pick_traverse_mode<MODE_DIRECT>(c);
        case MODE_WORK: return pick_traverse_mode<MODE_WORK>(c);
        default: return pick_traverse_mode<MODE_COUNT>(c);
    }
}

hipError_t launch(const Ctx &c, const Trav &t, uint64_t n, hipStream_t s, const TravParams &p) {
    const int grid = grid_for(c, t, n);
    if (t.group_fn) hipLaunchKernelGGL(t.group_fn, dim3(grid), dim3(256), lds_bytes(c, t), s, p, t.G);
    else hipLaunchKernelGGL(t.lane_fn, dim3(grid), dim3(256), lds_bytes(c, t), s, p);
    return hipGetLastError();
}

TravParams base_params(const Ctx &c) {
    TravParams p{};
    p.nodes = c.d_nodes;
    p.cnodes = c.d_cnodes;
    p.n_lds = lds_node_count(c);
    p.folded = c.tree.folded ? 1u : 0u;
    p.num_rows = c.tree.num_rows;
    p.scalars = reinterpret_cast<unsigned long long *>(c.d_scalars);
    p.label_map = c.d_label_map;
    return p;
}

hipError_t compact_slots(const Ctx &c, const uint64_t *d_offsets, const uint32_t *temp, uint32_t K, uint32_t *d_cols,
                         uint64_t n, hipStream_t s) {
    const uint32_t map_lds = label_map_lds(c);
    const uint64_t g = std::min<uint64_t>((n + kCompactTile - 1) / kCompactTile, 16384);
    hipLaunchKernelGGL(k_compact, dim3((unsigned)g), dim3(kCompactTile), map_lds * 4, s, d_offsets, temp, K, d_cols, n,
                       (const uint32_t *)c.d_label_map, map_lds);
    return hipGetLastError();
}

hipError_t direct_pass(const Ctx &c, const Trav &fn_direct, const uint64_t *d_rows, const uint32_t *ovf_list,
                       uint64_t ovf, const uint64_t *d_offsets, uint32_t *d_cols, hipStream_t s) {
    TravParams q = base_params(c);
    q.rows = d_rows;
    q.n = ovf;
    q.slot_list = ovf_list;
    q.offsets = d_offsets;
    q.cols = d_cols;
    return launch(c, fn_direct, ovf, s, q);
}

hipError_t launch_get(const Ctx &c, const uint64_t *d_rows, const uint64_t *d_cols, uint64_t n, uint8_t *d_out,
                      hipStream_t s) {
    const uint64_t g = std::min<uint64_t>((n + 255) / 256, 16384);
    hipLaunchKernelGGL(k_get, dim3((unsigned)g), dim3(256), 0, s, c.d_nodes, c.d_col_path, c.tree.path_len, d_rows,
                       d_cols, n, c.tree.num_rows, c.tree.num_columns, d_out,
                       reinterpret_cast<unsigned long long *>(c.d_scalars));
    return hipGetLastError();
}

}  // namespace nodes
}  // namespace mbrwt
