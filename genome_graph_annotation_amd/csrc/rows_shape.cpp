// rows_shape.cpp -- tree SHAPES without data: pure host code behind
// mbrwt_tree_basic_shape and mbrwt_create_from_rows (rows_from.hip).  A
// row's record depends on its label set and the tree's shape alone
// (DESIGN.md §4f, §11b), so a build from rows needs the shape as a Tree --
// the dnode table the walk tables are made from (rows_tables.cpp) -- and
// nothing of a node image.
#include <algorithm>
#include <vector>

#include "mbrwt_internal.hpp"

namespace mbrwt {

// BRWTBottomUpBuilder::build with get_basic_partitioner(arity)
// (BRWT_builders.cpp:20-31, :119-163): level by level, groups of `arity`
// consecutive nodes get a parent; a group of one passes through (merge of
// one node, :74-76), so leaves may sit at mixed depths.  BFS arrays as
// mbrwt_shape_desc; m == 0 gives no node, m == 1 the single leaf.
int basic_shape(uint64_t m, uint32_t arity, std::vector<uint32_t> &num_children, std::vector<uint32_t> &first_child,
                std::vector<uint32_t> &leaf_column) {
    num_children.clear();
    first_child.clear();
    leaf_column.clear();
    if (arity < 2 || arity > kMaxArity) {
        set_error("arity must be in [2, 64]");
        return MBRWT_ERR_INVALID;
    }
    if (m > 0x7FFFFFFFull) {
        set_error("num_columns >= 2^31 is not supported by this build");
        return MBRWT_ERR_UNSUPPORTED;
    }
    if (m == 0) return MBRWT_OK;
    // build order: node i < m is the leaf of column i; parents follow
    std::vector<uint32_t> kid_first, kid_count;  // per build node: its children in `kids`
    std::vector<uint32_t> kids;
    kid_first.assign(m, 0);
    kid_count.assign(m, 0);
    std::vector<uint32_t> level(m);
    for (uint32_t i = 0; i < m; ++i) level[i] = i;
    while (level.size() > 1) {
        std::vector<uint32_t> next;
        for (size_t g = 0; g < level.size(); g += arity) {
            const size_t e = std::min(level.size(), g + arity);
            if (e - g == 1) {
                next.push_back(level[g]);
                continue;
            }
            next.push_back((uint32_t)kid_first.size());
            kid_first.push_back((uint32_t)kids.size());
            kid_count.push_back((uint32_t)(e - g));
            kids.insert(kids.end(), level.begin() + g, level.begin() + e);
        }
        level.swap(next);
    }
    // BFS numbering from the root: children contiguous, in child order
    std::vector<uint32_t> order{level[0]};
    for (size_t h = 0; h < order.size(); ++h) {
        const uint32_t v = order[h];
        num_children.push_back(kid_count[v]);
        first_child.push_back(kid_count[v] ? (uint32_t)order.size() : 0u);
        leaf_column.push_back(kid_count[v] ? UINT32_MAX : v);
        for (uint32_t c = 0; c < kid_count[v]; ++c) order.push_back(kids[kid_first[v] + c]);
    }
    return MBRWT_OK;
}

// The Tree of a shape alone: the dnode table (super-root + nodes) with the
// leaves labelled by pre-order index and label_perm, max_arity, num_nodes,
// folded = false; no image (every base 0).  The leaves' columns must be a
// permutation of 0..num_columns-1.
int shape_tree(const mbrwt_shape_desc &sh, uint64_t num_columns, Tree &tree) {
    tree = Tree();
    tree.num_columns = num_columns;
    const uint32_t N = sh.num_nodes;
    tree.num_nodes = N;
    if (N == 0 || !sh.num_children || !sh.first_child || !sh.leaf_column) {
        set_error("empty shape or null array in shape description");
        return MBRWT_ERR_INVALID;
    }
    std::vector<uint8_t> seen(N, 0), col_seen(num_columns, 0);
    uint64_t leaves = 0;
    tree.nodes.assign((size_t)N + 1, DevNode{});
    for (uint32_t u = 0; u < N; ++u) {
        DevNode &dn = tree.nodes[u + 1];
        const uint32_t a = sh.num_children[u];
        if (a == 0) {
            const uint32_t col = sh.leaf_column[u];
            if (col >= num_columns || col_seen[col]) {
                set_error("leaf column out of range or duplicated");
                return MBRWT_ERR_INVALID;
            }
            col_seen[col] = 1;
            ++leaves;
            dn.kind = KIND_LEAF;
            dn.label = col;
            continue;
        }
        if (a > kMaxArity) {
            set_error("node arity > 64 is not supported by this build");
            return MBRWT_ERR_UNSUPPORTED;
        }
        const uint64_t fc = sh.first_child[u];
        if (fc <= u || fc + a > N) {
            set_error("children not in BFS order");
            return MBRWT_ERR_INVALID;
        }
        for (uint32_t c = 0; c < a; ++c)
            if (seen[fc + c]++) {
                set_error("node has two parents");
                return MBRWT_ERR_INVALID;
            }
        dn.kind = KIND_PLANE;  // (an internal node: the walk tables tell leaves from the rest only)
        dn.arity = (uint16_t)a;
        dn.first_child = (uint32_t)fc + 1;
        dn.label = UINT32_MAX;
        tree.max_arity = std::max(tree.max_arity, a);
    }
    for (uint32_t u = 1; u < N; ++u)
        if (!seen[u]) {
            set_error("node without a parent");
            return MBRWT_ERR_INVALID;
        }
    if (leaves != num_columns) {
        set_error("number of leaves != num_columns");
        return MBRWT_ERR_INVALID;
    }
    DevNode &sr = tree.nodes[0];  // the super-root: one child, the root
    sr.kind = KIND_PLANE;
    sr.arity = 1;
    sr.first_child = 1;
    sr.label = UINT32_MAX;
    // leaves by pre-order index (as finalize_tree labels them)
    std::vector<uint32_t> perm, st{1};
    bool identity = true;
    while (!st.empty()) {
        const uint32_t v = st.back();
        st.pop_back();
        DevNode &dn = tree.nodes[v];
        if (dn.kind == KIND_LEAF) {
            identity &= dn.label == (uint32_t)perm.size();
            const uint32_t col = dn.label;
            dn.label = (uint32_t)perm.size();
            perm.push_back(col);
            continue;
        }
        for (uint32_t c = dn.arity; c-- > 0;) st.push_back(dn.first_child + c);
    }
    if (!identity) tree.label_perm = std::move(perm);
    return MBRWT_OK;
}

}  // namespace mbrwt
