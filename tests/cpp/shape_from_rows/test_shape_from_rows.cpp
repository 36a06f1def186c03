// BRWTDevice::build_from_rows_greedy (csrc/brwt_device.hpp over
// mbrwt_tree_shape_from_rows + mbrwt_create_from_rows): the rows of a matrix
// as a CSR, columns descending per row; the shape from the rows is the
// oracle's greedy (+ relaxed) tree of the dense matrix, node for node, and the
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
    std::vector<uint64_t> offsets{0};
    std::vector<uint32_t> labels;
};

Fixture make() {
    Fixture f;
    uint64_t s = 7;
    auto next = [&]() { return (s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33; };
    f.cols.assign(f.m, std::vector<bool>(f.n, false));
    for (uint64_t j = 0; j < f.m; ++j)
        for (uint64_t i = 0; i < f.n; ++i) f.cols[j][i] = next() % 100 < 12;
    for (uint64_t i = 0; i < f.n; ++i) {
        for (uint64_t j = f.m; j-- > 0;)
            if (f.cols[j][i]) f.labels.push_back((uint32_t)j);
        f.offsets.push_back(f.labels.size());
    }
    return f;
}

void greedy_is_the_oracles(uint64_t relax) {
    const Fixture f = make();
    const OracleMatrix om(build_oracle(f.cols, f.n, 1, 2, relax));
    DescStorage st;
    const mbrwt_tree_desc want = oracle_desc(om, st);
    // the shape alone
    const mbrwt_rows_desc rd{f.n, f.m, f.offsets.data(), f.labels.data()};
    mbrwt_tree *t = nullptr;
    ASSERT_EQ(mbrwt_tree_shape_from_rows(&rd, MBRWT_PARTITIONER_GREEDY, 0, relax, 0, &t), (int)MBRWT_OK);
    const mbrwt_tree_desc *got = mbrwt_tree_get_desc(t);
    ASSERT_EQ(got->num_nodes, want.num_nodes);
    for (uint32_t u = 0; u < want.num_nodes; ++u) {
        ASSERT_EQ(got->num_children[u], want.num_children[u]);
        if (want.num_children[u]) ASSERT_EQ(got->first_child[u], want.first_child[u]);
        else ASSERT_EQ(got->leaf_column[u], want.leaf_column[u]);
    }
    mbrwt_tree_free(t);
    // the context under it
    const auto dev = mbrwt_host::BRWTDevice::build_from_rows_greedy(f.offsets, f.labels, f.m, relax);
    ASSERT_EQ(dev.num_rows(), f.n);
    ASSERT_EQ(dev.num_columns(), f.m);
    ASSERT_EQ(dev.num_relations(), om.num_relations());
    ASSERT_EQ(dev.num_nodes(), (uint64_t)want.num_nodes);
    std::vector<uint64_t> rows(f.n);
    for (uint64_t i = 0; i < f.n; ++i) rows[i] = i;
    const auto rws = dev.get_rows(rows);
    for (uint64_t i = 0; i < f.n; ++i) ASSERT_TRUE(rws[i] == om.get_row(i));
}

}  // namespace

TEST(ShapeFromRows, Greedy) { greedy_is_the_oracles(0); }

TEST(ShapeFromRows, GreedyRelaxed) { greedy_is_the_oracles(10); }

TEST(ShapeFromRows, ColumnOutOfRangeThrows) {
    Fixture f = make();
    f.labels[f.labels.size() / 2] = (uint32_t)f.m;
    EXPECT_THROW(mbrwt_host::BRWTDevice::build_from_rows_greedy(f.offsets, f.labels, f.m, 10),
                 mbrwt_host::MBRWTException);
}

int main() { return minitest::run_all(); }
