// BRWTDevice::build_from_sparse_columns[_greedy] (csrc/brwt_device.hpp over
// mbrwt_create_from_sparse_columns + mbrwt_tree_shape_from_sparse_columns):
// the columns of a matrix as ascending row ids; the greedy (+ relaxed) shape
// from them is the oracle's tree of the dense matrix, node for node, and the
// context under it answers every row like the oracle.  Needs a GPU.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../backends.hpp"
#include "../minitest.hpp"

namespace {

struct Fixture {
    uint64_t n = 1000, m = 37;
    std::vector<std::vector<bool>> cols;
    std::vector<uint64_t> offsets{0}, ids;
};

Fixture make() {
    Fixture f;
    uint64_t s = 7;
    auto next = [&]() { return (s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33; };
    f.cols.assign(f.m, std::vector<bool>(f.n, false));
    for (uint64_t j = 0; j < f.m; ++j) {
        for (uint64_t i = 0; i < f.n; ++i)
            if ((f.cols[j][i] = next() % 100 < 12)) f.ids.push_back(i);
        f.offsets.push_back(f.ids.size());
    }
    return f;
}

void answers_like(const mbrwt_host::BRWTDevice &dev, const Fixture &f, const OracleMatrix &om, uint32_t nodes) {
    ASSERT_EQ(dev.num_rows(), f.n);
    ASSERT_EQ(dev.num_columns(), f.m);
    ASSERT_EQ(dev.num_relations(), om.num_relations());
    ASSERT_EQ(dev.num_nodes(), (uint64_t)nodes);
    std::vector<uint64_t> rows(f.n);
    for (uint64_t i = 0; i < f.n; ++i) rows[i] = i;
    const auto rws = dev.get_rows(rows);
    for (uint64_t i = 0; i < f.n; ++i) ASSERT_TRUE(rws[i] == om.get_row(i));
}

void greedy_is_the_oracles(uint64_t relax) {
    const Fixture f = make();
    const OracleMatrix om(build_oracle(f.cols, f.n, 1, 2, relax));
    DescStorage st;
    const mbrwt_tree_desc want = oracle_desc(om, st);
    const mbrwt_sparse_columns_desc cd{f.n, f.m, f.offsets.data(), f.ids.data(), nullptr};
    mbrwt_tree *t = nullptr;
    ASSERT_EQ(mbrwt_tree_shape_from_sparse_columns(&cd, MBRWT_PARTITIONER_GREEDY, 0, relax, 0, &t), (int)MBRWT_OK);
    const mbrwt_tree_desc *got = mbrwt_tree_get_desc(t);
    ASSERT_EQ(got->num_nodes, want.num_nodes);
    for (uint32_t u = 0; u < want.num_nodes; ++u) {
        ASSERT_EQ(got->num_children[u], want.num_children[u]);
        if (want.num_children[u]) ASSERT_EQ(got->first_child[u], want.first_child[u]);
        else ASSERT_EQ(got->leaf_column[u], want.leaf_column[u]);
    }
    mbrwt_tree_free(t);
    answers_like(mbrwt_host::BRWTDevice::build_from_sparse_columns_greedy(f.offsets, f.ids, f.n, relax), f, om,
                 want.num_nodes);
}

}  // namespace

TEST(FromSparseColumns, Basic) {
    const Fixture f = make();
    const OracleMatrix om(build_oracle(f.cols, f.n, 0, 4, 0));
    DescStorage st;
    const mbrwt_tree_desc want = oracle_desc(om, st);
    answers_like(mbrwt_host::BRWTDevice::build_from_sparse_columns(f.offsets, f.ids, f.n, 4), f, om, want.num_nodes);
}

TEST(FromSparseColumns, Greedy) { greedy_is_the_oracles(0); }

TEST(FromSparseColumns, GreedyRelaxed) { greedy_is_the_oracles(10); }

TEST(FromSparseColumns, RowOutOfRangeThrows) {
    Fixture f = make();
    f.ids[f.offsets[3] - 1] = f.n;
    EXPECT_THROW(mbrwt_host::BRWTDevice::build_from_sparse_columns(f.offsets, f.ids, f.n, 4),
                 mbrwt_host::MBRWTException);
    EXPECT_THROW(mbrwt_host::BRWTDevice::build_from_sparse_columns_greedy(f.offsets, f.ids, f.n, 10),
                 mbrwt_host::MBRWTException);
}

int main() { return minitest::run_all(); }
