// The read split of the multi-device classify calls (csrc/multi_split.hpp) as
// pure host code: cut invariants, the rule itself against a linear scan, every
// replica's slice valid again after the rebase, the balance bound, where
// reads without rows go, and the malformed offsets the calls must refuse.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../minitest.hpp"
#include "multi_split.hpp"

using mbrwt::read_offsets_valid;
using mbrwt::split_reads;
using mbrwt::split_target;

namespace {

typedef std::vector<uint64_t> Offsets;

// every property of the cuts of valid offsets, for k = 1..4
void check_split(const Offsets &off) {
    const uint64_t n_reads = off.size() - 1, n_rows = off.back();
    ASSERT_TRUE(read_offsets_valid(off.data(), n_reads, n_rows));
    uint64_t longest = 0;
    for (uint64_t i = 0; i < n_reads; ++i) longest = std::max(longest, off[i + 1] - off[i]);
    for (uint32_t k = 1; k <= 4; ++k) {
        std::vector<uint64_t> cut;
        split_reads(off.data(), n_reads, n_rows, k, cut);
        ASSERT_EQ(cut.size(), (size_t)k + 1);
        EXPECT_EQ(cut[0], 0u);
        EXPECT_EQ(cut[k], n_reads);
        uint64_t rows_seen = 0;
        for (uint32_t r = 0; r < k; ++r) {
            ASSERT_TRUE(cut[r] <= cut[r + 1] && cut[r + 1] <= n_reads);
            // the rule: the first read starting at or after ceil(r * n_rows / k)
            if (r > 0) {
                const uint64_t target = split_target(n_rows, k, r);
                EXPECT_TRUE(target * k >= (uint64_t)r * n_rows && target * k < (uint64_t)r * n_rows + k);
                uint64_t first = 0;
                while (first < n_reads && off[first] < target) ++first;
                EXPECT_EQ(cut[r], first);
            }
            // the replica's slice, rebased, is a valid batch of its own
            const uint64_t nr = off[cut[r + 1]] - off[cut[r]], nq = cut[r + 1] - cut[r];
            Offsets mine(off.begin() + cut[r], off.begin() + cut[r + 1] + 1);
            for (auto &o : mine) o -= off[cut[r]];
            EXPECT_TRUE(read_offsets_valid(mine.data(), nq, nr));
            rows_seen += nr;
            // balance: no more than n_rows / k rows plus the longest read
            EXPECT_TRUE(nr * k <= n_rows + (uint64_t)k * longest);
        }
        EXPECT_EQ(rows_seen, n_rows);
        if (n_rows && k > 1) {
            // reads without rows at the front stay on the first replica, at the back on the last
            uint64_t lead = 0, trail = n_reads;
            while (off[lead + 1] == 0) ++lead;
            while (off[trail - 1] == n_rows) --trail;
            EXPECT_TRUE(cut[1] >= lead);
            EXPECT_TRUE(cut[k - 1] <= trail);
        }
    }
}

}  // namespace

TEST(MultiSplit, ZeroReads) {
    const Offsets off{0};
    check_split(off);
    std::vector<uint64_t> cut;
    split_reads(off.data(), 0, 0, 3, cut);
    EXPECT_EQ(cut, (std::vector<uint64_t>{0, 0, 0, 0}));
}

TEST(MultiSplit, FewerReadsThanReplicas) {
    check_split({0, 7});
    check_split({0, 3, 10});
    std::vector<uint64_t> cut;
    const Offsets off{0, 3, 10};
    split_reads(off.data(), 2, 10, 4, cut);  // targets 3, 5, 8: replicas 2 and 3 get no read
    EXPECT_EQ(cut, (std::vector<uint64_t>{0, 1, 2, 2, 2}));
}

TEST(MultiSplit, OneReadBetweenEmptyReads) {
    const Offsets off{0, 0, 0, 10, 10, 10};
    check_split(off);
    std::vector<uint64_t> cut;
    split_reads(off.data(), 5, 10, 3, cut);  // the first two empty reads with the rows, the others last
    EXPECT_EQ(cut, (std::vector<uint64_t>{0, 3, 3, 5}));
}

TEST(MultiSplit, EmptyReadsAtBothEnds) {
    check_split({0, 0, 3, 7, 7, 12, 12, 12});
    check_split({0, 0, 1, 1});  // one row: every target is 1
}

TEST(MultiSplit, OnlyEmptyReads) {
    const Offsets off{0, 0, 0};
    check_split(off);
    std::vector<uint64_t> cut;
    split_reads(off.data(), 2, 0, 3, cut);  // no rows: all on the last replica
    EXPECT_EQ(cut, (std::vector<uint64_t>{0, 0, 0, 2}));
}

TEST(MultiSplit, EqualLengthReads) {
    Offsets off;
    for (uint64_t i = 0; i <= 12; ++i) off.push_back(5 * i);
    check_split(off);
    std::vector<uint64_t> cut;
    split_reads(off.data(), 12, 60, 4, cut);
    EXPECT_EQ(cut, (std::vector<uint64_t>{0, 3, 6, 9, 12}));
    split_reads(off.data(), 12, 60, 3, cut);
    EXPECT_EQ(cut, (std::vector<uint64_t>{0, 4, 8, 12}));
}

TEST(MultiSplit, RandomReads) {
    uint64_t s = 12345;
    auto next = [&]() { return (s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33; };
    for (int rep = 0; rep < 200; ++rep) {
        Offsets off{0};
        const uint64_t n_reads = next() % 40;
        for (uint64_t i = 0; i < n_reads; ++i) off.push_back(off.back() + (next() % 3 ? next() % 60 : 0));
        check_split(off);
    }
}

TEST(MultiSplit, TargetDoesNotOverflow) {
    const uint64_t n = ~0ull;
    EXPECT_EQ(split_target(n, 4, 4), n);
    EXPECT_EQ(split_target(n, 4, 2), n / 2 + 1);  // ceil
    EXPECT_EQ(split_target(10, 4, 1), 3u);
    EXPECT_EQ(split_target(0, 3, 2), 0u);
}

// the malformed offsets of the single-context calls' tests, for 10 rows: past
// n_rows, not from 0, descending, short
TEST(MultiSplit, MalformedOffsets) {
    const std::vector<Offsets> bad{{0, 11}, {1, 10}, {0, 6, 4, 10}, {0, 5, 9}};
    for (const auto &off : bad) {
        const uint64_t n_reads = off.size() - 1;
        EXPECT_FALSE(read_offsets_valid(off.data(), n_reads, 10));
        for (uint32_t k = 1; k <= 4; ++k)  // the search stays inside the array whatever it holds
            for (uint32_t r = 0; r <= k; ++r)
                EXPECT_TRUE(mbrwt::split_cut([&](uint64_t i) { return off.at(i); }, n_reads, 10, k, r) <= n_reads);
    }
    // a descending pair exactly on a cut: with two replicas the target is row
    // 5 and the cut falls on read 1, between the 6 and the 4
    const Offsets on_cut{0, 6, 4, 10};
    EXPECT_EQ(mbrwt::split_cut([&](uint64_t i) { return on_cut.at(i); }, 3, 10, 2, 1), 1u);
    EXPECT_FALSE(read_offsets_valid(on_cut.data(), 3, 10));
    // descending at the very end, and a single offset that is not n_rows
    EXPECT_FALSE(read_offsets_valid(Offsets{0, 12, 10}.data(), 2, 10));
    EXPECT_FALSE(read_offsets_valid(Offsets{0}.data(), 0, 10));
    EXPECT_TRUE(read_offsets_valid(Offsets{0, 10}.data(), 1, 10));
}

int main() { return minitest::run_all(); }
