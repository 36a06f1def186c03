// BRWTDevice::get_columns (csrc/brwt_device.hpp over mbrwt_get_columns): the
// sparse columns of a row window, in the caller's order of columns, against
// the matrix the context was built from.  One 65 x 17 matrix: all columns,
// then a window with a reversed list.  Needs a GPU.
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../../../genome_graph_annotation_amd/csrc/brwt_device.hpp"
#include "../minitest.hpp"

namespace {

struct Fixture {
    uint64_t n = 65, m = 17;
    std::vector<std::vector<bool>> cols;
    std::vector<uint64_t> offsets{0}, ids;
};

Fixture make() {
    Fixture f;
    uint64_t s = 11;
    auto next = [&]() { return (s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33; };
    f.cols.assign(f.m, std::vector<bool>(f.n, false));
    for (uint64_t j = 0; j < f.m; ++j) {
        for (uint64_t i = 0; i < f.n; ++i)
            if ((f.cols[j][i] = j != 5 && next() % 100 < 30)) f.ids.push_back(i);  // (column 5 is empty)
        f.offsets.push_back(f.ids.size());
    }
    return f;
}

std::vector<uint64_t> expect(const Fixture &f, uint64_t column, uint64_t begin, uint64_t end) {
    std::vector<uint64_t> rows;
    for (uint64_t i = begin; i < end; ++i)
        if (f.cols[column][i]) rows.push_back(i);
    return rows;
}

}  // namespace

TEST(GetColumns, AllColumns) {
    const Fixture f = make();
    const auto dev = mbrwt_host::BRWTDevice::build_from_sparse_columns(f.offsets, f.ids, f.n, 4);
    std::vector<uint64_t> columns(f.m);
    for (uint64_t j = 0; j < f.m; ++j) columns[j] = j;
    const auto got = dev.get_columns(columns, 0, f.n);
    ASSERT_EQ(got.size(), (size_t)f.m);
    for (uint64_t j = 0; j < f.m; ++j) {
        ASSERT_TRUE(got[j] == expect(f, j, 0, f.n));
        ASSERT_TRUE(got[j] == dev.get_column(j));
    }
    ASSERT_TRUE(got[5].empty());
}

TEST(GetColumns, WindowInTheCallersOrder) {
    const Fixture f = make();
    const auto dev = mbrwt_host::BRWTDevice::build_from_sparse_columns(f.offsets, f.ids, f.n, 4);
    const std::vector<uint64_t> columns{16, 5, 0, 9};
    const auto got = dev.get_columns(columns, 3, 64);
    ASSERT_EQ(got.size(), columns.size());
    for (size_t j = 0; j < columns.size(); ++j) ASSERT_TRUE(got[j] == expect(f, columns[j], 3, 64));
    ASSERT_TRUE(dev.get_columns({}, 0, f.n).empty());
    EXPECT_THROW(dev.get_columns({17}, 0, f.n), std::out_of_range);
    EXPECT_THROW(dev.get_columns({1, 1}, 0, f.n), mbrwt_host::MBRWTException);
}

int main() { return minitest::run_all(); }
