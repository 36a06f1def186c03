// BRWTDevice::build_from_rows (csrc/brwt_device.hpp over
// mbrwt_create_from_rows): the rows of a matrix as a CSR, columns descending
// per row, under the basic partitioner's shape and under the shape of the
// oracle's greedy tree; every row, the properties and the exported tree
// against the oracle.  Needs a GPU.
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

void same_as_oracle(const mbrwt_host::BRWTDevice &dev, const OracleMatrix &om, const Fixture &f) {
    ASSERT_EQ(dev.num_rows(), f.n);
    ASSERT_EQ(dev.num_columns(), f.m);
    ASSERT_EQ(dev.num_relations(), om.num_relations());
    std::vector<uint64_t> rows(f.n);
    for (uint64_t i = 0; i < f.n; ++i) rows[i] = i;
    const auto got = dev.get_rows(rows);
    for (uint64_t i = 0; i < f.n; ++i) ASSERT_TRUE(got[i] == om.get_row(i));
}

}  // namespace

TEST(FromRows, BasicShape) {
    const Fixture f = make();
    const OracleMatrix om(build_oracle(f.cols, f.n, 0, 4, 0));
    const auto dev = mbrwt_host::BRWTDevice::build_from_rows(f.offsets, f.labels, f.m, 4);
    same_as_oracle(dev, om, f);
    DescStorage st;
    const mbrwt_tree_desc d = oracle_desc(om, st);
    ASSERT_EQ(dev.num_nodes(), (uint64_t)d.num_nodes);
}

TEST(FromRows, GivenGreedyShape) {
    const Fixture f = make();
    const OracleMatrix om(build_oracle(f.cols, f.n, 1, 2, 0));
    DescStorage st;
    const mbrwt_tree_desc d = oracle_desc(om, st);
    const mbrwt_shape_desc shape{d.num_nodes, d.num_children, d.first_child, d.leaf_column};
    const auto dev = mbrwt_host::BRWTDevice::build_from_rows(f.offsets, f.labels, f.m, 0, &shape);
    same_as_oracle(dev, om, f);
}

TEST(FromRows, DuplicateColumnThrows) {
    Fixture f = make();
    uint64_t r = 0;
    while (f.offsets[r + 1] - f.offsets[r] < 2) ++r;
    f.labels[f.offsets[r] + 1] = f.labels[f.offsets[r]];
    EXPECT_THROW(mbrwt_host::BRWTDevice::build_from_rows(f.offsets, f.labels, f.m, 4), mbrwt_host::MBRWTException);
}

int main() { return minitest::run_all(); }
