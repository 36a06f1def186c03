// mbrwt_tree_relax_shape on a handful of shapes, host only: a stand-alone
// program for a sanitizer build of the library's host code (`make sanitize`
// here; no GPU is touched).  Basic shapes of several arities and sizes, a
// hand-made mixed-depth shape, every max_arity class, counts all zero, all
// equal and halving per level; the result must stay a tree over the same
// leaves.  Exit status 0 and "relax_shape_host ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../../include/mbrwt.h"

namespace {

int failures = 0;
#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            ++failures;                                                  \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
        }                                                                \
    } while (0)

struct Shape {
    std::vector<uint32_t> nc, fc, lc;
    mbrwt_shape_desc desc() const { return mbrwt_shape_desc{(uint32_t)nc.size(), nc.data(), fc.data(), lc.data()}; }
};

Shape basic(uint64_t m, uint32_t arity) {
    mbrwt_tree *t = nullptr;
    CHECK(mbrwt_tree_basic_shape(m, arity, &t) == MBRWT_OK);
    const mbrwt_tree_desc *d = mbrwt_tree_get_desc(t);
    Shape s;
    s.nc.assign(d->num_children, d->num_children + d->num_nodes);
    s.fc.assign(d->first_child, d->first_child + d->num_nodes);
    s.lc.assign(d->leaf_column, d->leaf_column + d->num_nodes);
    mbrwt_tree_free(t);
    return s;
}

// counts that a matrix could have: a leaf's own, a parent at most the sum and
// at least the largest of its children's
std::vector<uint64_t> counts_of(const Shape &s, int law) {
    const size_t N = s.nc.size();
    std::vector<uint64_t> c(N, 0);
    for (size_t u = N; u-- > 0;) {
        if (!s.nc[u]) {
            c[u] = law == 0 ? 0 : law == 1 ? 1000 : 1 + (s.lc[u] * 2654435761u) % 997;
            continue;
        }
        uint64_t sum = 0, mx = 0;
        for (uint32_t k = 0; k < s.nc[u]; ++k) {
            sum += c[s.fc[u] + k];
            mx = mx > c[s.fc[u] + k] ? mx : c[s.fc[u] + k];
        }
        c[u] = law == 1 ? mx : law == 2 ? sum : (sum + mx) / 2;
    }
    return c;
}

void relax_all(const Shape &s) {
    const mbrwt_shape_desc sd = s.desc();
    size_t leaves = 0;
    for (const uint32_t k : s.nc) leaves += k == 0;
    for (int law = 0; law < 4; ++law) {
        const std::vector<uint64_t> counts = counts_of(s, law);
        for (const uint64_t max_arity : {0ull, 1ull, 2ull, 3ull, 10ull, 64ull, ~0ull}) {
            mbrwt_tree *t = nullptr;
            CHECK(mbrwt_tree_relax_shape(&sd, counts.data(), max_arity, &t) == MBRWT_OK);
            if (!t) continue;
            const mbrwt_tree_desc *d = mbrwt_tree_get_desc(t);
            CHECK(d->num_nodes <= s.nc.size() && d->num_rows == 0);
            size_t got_leaves = 0, edges = 0;
            std::vector<uint8_t> seen(leaves, 0);
            for (uint32_t u = 0; u < d->num_nodes; ++u) {
                CHECK(d->vec_size[u] == 0);
                if (d->num_children[u]) {
                    CHECK(d->first_child[u] > u && (uint64_t)d->first_child[u] + d->num_children[u] <= d->num_nodes);
                    edges += d->num_children[u];
                } else {
                    ++got_leaves;
                    CHECK(d->leaf_column[u] < leaves && !seen[d->leaf_column[u]]);
                    if (d->leaf_column[u] < leaves) seen[d->leaf_column[u]] = 1;
                }
            }
            CHECK(got_leaves == leaves);
            CHECK(d->num_nodes == 0 || edges + 1 == d->num_nodes);
            if (max_arity <= 1) CHECK(d->num_nodes == s.nc.size());
            mbrwt_tree_free(t);
        }
    }
}

}  // namespace

int main() {
    for (const uint64_t m : {1ull, 2ull, 3ull, 17ull, 64ull, 65ull, 300ull, 2652ull})
        for (const uint32_t arity : {2u, 3u, 8u, 64u}) relax_all(basic(m, arity));
    // leaves at mixed depths: root(3) -> leaf 4, node(2) -> leaf 0, node(3) -> leaves 3 1 2; leaf 5
    Shape mixed;
    mixed.nc = {3, 0, 2, 0, 0, 3, 0, 0, 0};
    mixed.fc = {1, 0, 4, 0, 0, 6, 0, 0, 0};
    mixed.lc = {~0u, 4, ~0u, 5, 0, ~0u, 3, 1, 2};
    relax_all(mixed);
    // rejected arguments allocate nothing that leaks
    const mbrwt_shape_desc sd = mixed.desc();
    const std::vector<uint64_t> counts(mixed.nc.size(), 1);
    mbrwt_tree *t = nullptr;
    CHECK(mbrwt_tree_relax_shape(nullptr, counts.data(), 10, &t) == MBRWT_ERR_INVALID);
    CHECK(mbrwt_tree_relax_shape(&sd, nullptr, 10, &t) == MBRWT_ERR_INVALID);
    CHECK(mbrwt_tree_relax_shape(&sd, counts.data(), 10, nullptr) == MBRWT_ERR_INVALID);
    Shape bad = mixed;
    bad.fc[5] = 7;  // children past the last node
    const mbrwt_shape_desc bd = bad.desc();
    CHECK(mbrwt_tree_relax_shape(&bd, counts.data(), 10, &t) == MBRWT_ERR_INVALID && t == nullptr);
    std::printf(failures ? "relax_shape_host: %d failed checks\n" : "relax_shape_host ok\n", failures);
    return failures ? 1 : 0;
}
