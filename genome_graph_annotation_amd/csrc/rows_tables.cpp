// rows_tables.cpp -- the WALK TABLES of the row records: pure host code that
// turns a finished node tree's shape into the tables the row-record kernels
// walk (rows.hip the queries, rows_build.hip the image build; layout of the
// RWT table in mbrwt_internal.hpp "ROW RECORDS", of the others below).
#include <algorithm>
#include <cstring>
#include <vector>

#include "mbrwt_internal.hpp"

namespace mbrwt {

// ------------------------------------------------------------------------
// RWT table
// ------------------------------------------------------------------------
bool build_rwt_table(const Tree &tree, std::vector<uint32_t> &table, uint32_t &height, uint32_t &max_arity) {
    table.clear();
    height = 0;
    max_arity = 0;
    const auto &N = tree.nodes;
    if (N.size() < 2) return false;
    // the logical root: the folded root's children hang off dnode 0
    const bool folded = tree.folded;
    const uint32_t root = folded ? 0u : 1u;
    if (!folded && N[0].arity != 1) return false;
    if (N[root].kind == KIND_LEAF || N[root].arity == 0) return false;  // one-column tree
    auto column_of = [&](const DevNode &d) { return tree.label_perm.empty() ? d.label : tree.label_perm[d.label]; };
    std::vector<uint32_t> inner{root}, level{1};
    std::vector<uint32_t> local(N.size(), UINT32_MAX);
    local[root] = 0;
    for (size_t h = 0; h < inner.size(); ++h) {
        const DevNode &v = N[inner[h]];
        height = std::max(height, level[h]);
        if (v.arity == 0 || v.arity > kRowsMaxArity) return false;
        max_arity = std::max<uint32_t>(max_arity, v.arity);
        for (uint32_t c = 0; c < v.arity; ++c) {
            const uint32_t w = v.first_child + c;
            if (w >= N.size()) return false;
            if (N[w].kind != KIND_LEAF) {
                local[w] = (uint32_t)inner.size();
                inner.push_back(w);
                level.push_back(level[h] + 1);
            }
        }
    }
    if (height > kRowsMaxHeight || inner.size() >= 0x8000) return false;
    std::vector<uint32_t> nodew(inner.size());
    std::vector<uint32_t> ent;  // (r06: u32 entries -- columns up to 2^16; u16 with 15-bit columns before)
    for (size_t i = 0; i < inner.size(); ++i) {
        const DevNode &v = N[inner[i]];
        if (ent.size() + v.arity > 0xFFFFFF) return false;
        nodew[i] = (uint32_t)ent.size() | ((uint32_t)v.arity << 24);
        for (uint32_t c = 0; c < v.arity; ++c) {
            const DevNode &w = N[v.first_child + c];
            if (w.kind == KIND_LEAF) {
                const uint32_t col = column_of(w);
                if (col >= 0x10000) return false;  // (the label stage and temp regions hold u16 labels)
                ent.push_back(0x80000000u | col);
            } else {
                ent.push_back(local[v.first_child + c]);
            }
        }
    }
    const size_t nI = inner.size(), nE = ent.size();
    const size_t words = 4 + nI + nE;
    // (the RWT table stays in global memory -- the one-lane walks read it
    // there -- so only the LDS-staged RWT2 table has kRowsMaxTableWords)
    if (words > (1u << 22)) return false;
    table.assign(words, 0);
    table[0] = (uint32_t)nI;
    table[1] = (uint32_t)nE;
    table[2] = height;
    std::memcpy(&table[4], nodew.data(), nI * 4);
    std::memcpy(&table[4 + nI], ent.data(), nE * 4);
    return true;
}

// RWT2 table (k_traverse_rows): one u32 ENTRY per child of every internal
// node that is not a leaf parent ("LP" nodes, whose labels are base column +
// bit, or entry bit of a column list: no entries, no frame), u32 words
//   [0] the root's entry, [1] nE, [2] frames (non-LP internal levels on a
//   path), [3] 0 (or the path table's offset, append_path_table), nE
//   entries, then the column lists (u16) of the leaf parents whose columns
//   are not consecutive (the greedy partitioner's groups); an entry is
//     leaf      0x80000000 | column
//     LP node   0xC0000000 | arity << 16 | first column
//     LP list   0xE0000000 | arity << 16 | first u16 of its column list
//     internal  arity << 16 | first entry of its children
// so the walk reads ONE table word per visited child.
bool build_rwt2_table(const Tree &tree, std::vector<uint32_t> &t2, uint32_t &frames, std::vector<uint32_t> *slot_dnode) {
    t2.clear();
    frames = 0;
    const auto &N = tree.nodes;
    if (N.size() < 2) return false;
    const bool folded = tree.folded;
    const uint32_t root = folded ? 0u : 1u;
    if (N[root].kind == KIND_LEAF || N[root].arity == 0) return false;
    auto column_of = [&](const DevNode &d) { return tree.label_perm.empty() ? d.label : tree.label_perm[d.label]; };
    // a leaf parent: base = its first column (consecutive: cons) 
    auto is_lp2 = [&](uint32_t v, uint32_t &base, bool &cons) {
        const DevNode &d = N[v];
        cons = true;
        for (uint32_t c = 0; c < d.arity; ++c) {
            const DevNode &w = N[d.first_child + c];
            if (w.kind != KIND_LEAF) return false;
            if (c == 0) base = column_of(w);
            else if (column_of(w) != base + c) cons = false;
        }
        return d.arity > 0;
    };
    auto is_lp = [&](uint32_t v, uint32_t &base) {
        bool cons;
        return is_lp2(v, base, cons);
    };
    std::vector<uint16_t> lists;  // the column lists of non-consecutive leaf parents
    // non-LP internal nodes in BFS order, each with its first entry
    std::vector<uint32_t> order{root}, depth{1}, first;
    uint32_t nE = 0;
    std::vector<uint32_t> first_of(N.size(), 0);
    uint32_t rb = 0;
    bool root_cons = false;
    const bool root_lp = is_lp2(root, rb, root_cons) && root_cons;  // (a listed root: an internal node)
    if (!root_lp) {
        for (size_t h = 0; h < order.size(); ++h) {
            const uint32_t v = order[h];
            const DevNode &d = N[v];
            if (d.arity == 0 || d.arity > kRowsMaxArity) return false;
            frames = std::max(frames, depth[h]);
            first_of[v] = nE;
            nE += d.arity;
            for (uint32_t c = 0; c < d.arity; ++c) {
                const uint32_t w = d.first_child + c;
                uint32_t b;
                if (N[w].kind == KIND_LEAF || is_lp(w, b)) continue;
                order.push_back(w);
                depth.push_back(depth[h] + 1);
            }
        }
    } else if (N[root].arity > kRowsMaxArity) {
        return false;
    }
    if (nE >= 0x10000 || 4 + (size_t)nE > kRowsMaxTableWords) return false;
    auto entry = [&](uint32_t w, uint32_t &out) -> bool {
        const DevNode &d = N[w];
        if (d.kind == KIND_LEAF) {
            const uint32_t col = column_of(d);
            if (col >= 0x10000) return false;
            out = 0x80000000u | col;
            return true;
        }
        if (d.arity == 0 || d.arity > kRowsMaxArity) return false;
        uint32_t b;
        bool cons;
        if (is_lp2(w, b, cons)) {
            if (cons) {
                if (b + d.arity > 0x10000) return false;
                out = 0xC0000000u | ((uint32_t)d.arity << 16) | b;
                return true;
            }
            if (lists.size() + d.arity > 0x10000) return false;
            out = 0xE0000000u | ((uint32_t)d.arity << 16) | (uint32_t)lists.size();
            for (uint32_t c = 0; c < d.arity; ++c) {
                const uint32_t col = column_of(N[d.first_child + c]);
                if (col >= 0x10000) return false;
                lists.push_back((uint16_t)col);
            }
            return true;
        }
        out = ((uint32_t)d.arity << 16) | first_of[w];
        return true;
    };
    t2.assign(4 + nE, 0);
    if (slot_dnode) {  // (terminal records: the dnode of every entry; slot nE = the root)
        slot_dnode->assign(nE + 1, ~0u);
        (*slot_dnode)[nE] = root;
        if (!root_lp)
            for (const uint32_t v : order)
                for (uint32_t c = 0; c < N[v].arity; ++c) (*slot_dnode)[first_of[v] + c] = N[v].first_child + c;
    }
    if (!entry(root, t2[0])) return false;
    t2[1] = nE;
    t2[2] = frames;
    if (!root_lp)
        for (const uint32_t v : order) {
            const DevNode &d = N[v];
            for (uint32_t c = 0; c < d.arity; ++c)
                if (!entry(d.first_child + c, t2[4 + first_of[v] + c])) return false;
        }
    for (size_t i = 0; i < lists.size(); i += 2)
        t2.push_back((uint32_t)lists[i] | (i + 1 < lists.size() ? (uint32_t)lists[i + 1] << 16 : 0u));
    return t2.size() <= kRowsMaxTableWords;
}

// K when every root-to-leaf path of the RWT2 table crosses exactly K internal
// entries (the root included) and then a leaf parent (rows_walk_uni), else 0
uint32_t rwt2_uniform_levels(const std::vector<uint32_t> &t2) {
    if (t2.size() < 4 || (t2[0] >> 30) != 0u) return 0;  // the root is a leaf parent (or a leaf)
    const uint32_t K = t2[2];
    if (K < 1 || K > 5) return 0;
    std::vector<uint32_t> lev{t2[0]};
    for (uint32_t d = 1; d <= K; ++d) {
        std::vector<uint32_t> next;
        for (const uint32_t w : lev) {
            const uint32_t a = (w >> 16) & 0x7Fu, f = w & 0xFFFFu;
            for (uint32_t c = 0; c < a; ++c) {
                if (4 + (size_t)f + c >= t2.size()) return 0;
                const uint32_t e = t2[4 + f + c];
                if ((e >> 29) != (d == K ? 6u : 0u)) return 0;  // consecutive leaf parents exactly at depth K + 1
                if (d < K) next.push_back(e);
            }
        }
        lev.swap(next);
    }
    return K;
}

// The PATH TABLE of a uniform tree (rows_walk_path): every leaf parent's
// first column indexed by the child indices on its path from the root,
// idx = ((c_0 A_1 + c_1) A_2 + ...) A_{K-1} + c_{K-1}, A_k = the largest
// arity at level k (level 0 = the root).  Appended to the RWT2 table: t2[3]
// = its word offset, word 0 = A_1..A_{K-1} (4 bits each), then the u16
// columns.  The odometer then never reads the table to follow a level: it
// keeps the path index, and the leaf parent's column is one LDS read.
// Empty (t2[3] = 0) when the table would exceed kRowsMaxPathEntries.
constexpr uint32_t kRowsMaxPathEntries = 4096;
void append_path_table(std::vector<uint32_t> &t2, uint32_t K) {
    if (!K || t2.size() < 4) return;
    std::vector<uint32_t> A(K, 0);
    std::vector<uint32_t> lev{t2[0]};
    for (uint32_t d = 0; d < K; ++d) {  // A[d] = the largest arity at level d
        std::vector<uint32_t> next;
        for (const uint32_t w : lev) {
            const uint32_t a = (w >> 16) & 0x7Fu, f = w & 0xFFFFu;
            A[d] = std::max(A[d], a);
            if (d + 1 < K)
                for (uint32_t c = 0; c < a; ++c) next.push_back(t2[4 + f + c]);
        }
        lev.swap(next);
    }
    uint64_t entries = 1;
    for (uint32_t d = 0; d < K; ++d) entries *= A[d];
    if (entries > kRowsMaxPathEntries || entries == 0) return;
    std::vector<uint16_t> col(entries, 0);
    std::vector<uint8_t> set(entries, 0);
    // depth-first over the paths
    struct F {
        uint32_t w, idx, d;
    };
    std::vector<F> st{{t2[0], 0, 0}};
    while (!st.empty()) {
        const F fr = st.back();
        st.pop_back();
        const uint32_t a = (fr.w >> 16) & 0x7Fu, f = fr.w & 0xFFFFu;
        for (uint32_t c = 0; c < a; ++c) {
            const uint32_t e = t2[4 + f + c];
            const uint32_t idx = fr.idx * A[fr.d] + c;
            if (fr.d + 1 == K) {  // a leaf parent: its first column
                col[idx] = (uint16_t)(e & 0xFFFFu);
                set[idx] = 1;
            }
            else st.push_back(F{e, idx, fr.d + 1});
        }
    }
    uint32_t packed = 0;
    for (uint32_t d = 1; d < K; ++d) packed |= A[d] << (4 * (d - 1));
    // a LINEAR path table (every leaf parent's first column = its path index
    // << s: the basic partitioner's trees, whose only incomplete nodes are the
    // last of their level -- C2-C4 with s = 3) is flagged in bit 31, s in bits
    // 24..28: the walk then computes the column instead of reading it
    for (uint32_t sh = 0; sh < 16; ++sh) {
        bool lin = true;
        for (uint64_t i = 0; i < entries && lin; ++i) lin = !set[i] || col[i] == (uint32_t)(i << sh);
        if (lin) {
            packed |= 0x80000000u | sh << 24;
            break;
        }
    }
    t2[3] = (uint32_t)t2.size();
    t2.push_back(packed);
    for (size_t i = 0; i < col.size(); i += 2)
        t2.push_back((uint32_t)col[i] | (i + 1 < col.size() ? (uint32_t)col[i + 1] << 16 : 0u));
}

// TERMINAL records (r06, MBRWT_BUILD_ROWS_CODE = 2; rows_record.hpp
// term_walk): every RWT2 entry that is a leaf or a leaf parent is a
// terminal.  TT = [w | ib << 8, nT, 0, 0, nT entry words, the RWT2 column
// lists]; the build table BT = [root entry, the root's terminal id (a
// one-level tree), nE, 0, nE entries, nE terminal ids (internal: ~0)] for
// the build's walk.  False when the fields would not fit 28 bits (more than
// 4,096 terminals or a leaf parent wider than 16).
bool build_term_tables(const std::vector<uint32_t> &t2, std::vector<uint32_t> &tt, std::vector<uint32_t> &bt,
                       std::vector<uint32_t> &term_slot) {
    tt.clear();
    bt.clear();
    term_slot.clear();
    if (t2.size() < 4) return false;
    const uint32_t root = t2[0], nE = t2[1];
    const size_t lists_end = t2[3] ? (size_t)t2[3] : t2.size();
    if (4 + (size_t)nE > lists_end) return false;
    std::vector<uint32_t> ent, tid(nE, ~0u);
    uint32_t mbits = 0;
    auto is_term = [](uint32_t e) { return (e >> 31) != 0u; };
    auto lp_arity = [](uint32_t e) { return (e >> 30) == 3u ? (e >> 16) & 0x7Fu : 0u; };
    if ((root >> 30) == 3u) {  // a one-level tree: the root is the only terminal
        ent.push_back(root);
        term_slot.push_back(nE);
        mbits = lp_arity(root);
    } else {
        for (uint32_t i = 0; i < nE; ++i) {
            const uint32_t e = t2[4 + i];
            if (!is_term(e)) continue;
            tid[i] = (uint32_t)ent.size();
            ent.push_back(e);
            term_slot.push_back(i);
            mbits = std::max(mbits, lp_arity(e));
        }
    }
    const uint32_t nT = (uint32_t)ent.size();
    uint32_t ib = 1;
    while ((1u << ib) < nT) ++ib;
    if (nT == 0 || nT > 4096 || mbits > 16 || ib + mbits > 28) return false;
    const uint32_t w = ib + mbits;
    tt = {w | ib << 8, nT, 0u, 0u};
    tt.insert(tt.end(), ent.begin(), ent.end());
    tt.insert(tt.end(), t2.begin() + 4 + nE, t2.begin() + lists_end);
    bt = {root, 0u, nE, 0u};
    bt.insert(bt.end(), t2.begin() + 4, t2.begin() + 4 + nE);
    bt.insert(bt.end(), tid.begin(), tid.end());
    return tt.size() <= kRowsMaxTableWords;
}

// WT (terminal records' V accounting): every terminal's chain of ancestor
// dnodes from the root down, their arities, the chain's length and the
// terminal's own arity (a leaf parent's; 0 for a leaf).  The parents come
// from the logical tree below the root (as build_rwt_table walks it).
bool build_work_table(const Tree &tree, const std::vector<uint32_t> &term_dnode, std::vector<uint32_t> &wt) {
    const auto &N = tree.nodes;
    const uint32_t root = tree.folded ? 0u : 1u;
    std::vector<uint32_t> parent(N.size(), ~0u), q{root};
    for (size_t h = 0; h < q.size(); ++h) {
        const DevNode &v = N[q[h]];
        if (v.kind == KIND_LEAF) continue;
        for (uint32_t c = 0; c < v.arity; ++c) {
            const uint32_t w = v.first_child + c;
            if (w >= N.size()) return false;
            parent[w] = q[h];
            if (N[w].kind != KIND_LEAF) q.push_back(w);
        }
    }
    const uint32_t nT = (uint32_t)term_dnode.size();
    std::vector<std::vector<uint32_t>> chains(nT);
    uint32_t D = 1;
    for (uint32_t t = 0; t < nT; ++t) {
        const uint32_t u = term_dnode[t];
        if (u >= N.size()) return false;
        for (uint32_t a = u == root ? ~0u : parent[u]; a != ~0u; a = a == root ? ~0u : parent[a]) {
            chains[t].push_back(a);
            if (chains[t].size() > 32) return false;
        }
        std::reverse(chains[t].begin(), chains[t].end());
        D = std::max<uint32_t>(D, (uint32_t)chains[t].size());
    }
    wt.assign(4 + (size_t)nT * (2 * D + 2), 0u);
    wt[0] = D;
    wt[1] = nT;
    for (uint32_t t = 0; t < nT; ++t) {
        const uint32_t u = term_dnode[t];
        for (uint32_t k = 0; k < chains[t].size(); ++k) {
            wt[4 + (size_t)t * D + k] = chains[t][k];
            wt[4 + (size_t)nT * D + (size_t)t * D + k] = N[chains[t][k]].arity;
        }
        wt[4 + (size_t)2 * nT * D + t] = (uint32_t)chains[t].size();
        wt[4 + (size_t)2 * nT * D + nT + t] = N[u].kind == KIND_LEAF ? 0u : N[u].arity;
    }
    return true;
}

}  // namespace mbrwt
