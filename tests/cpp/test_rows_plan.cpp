// test_rows_plan.cpp -- the row-record build's decisions (csrc/rows_plan.hpp)
// as pure host code: candidate list, candidate cost, the choice, the block
// override, the row / S magic number and the record-code rule.  Stand-alone:
// links neither libmbrwt nor the oracle.
#include <cmath>
#include <cstdint>
#include <vector>

#include "minitest.hpp"
#include "rows_plan.hpp"

using namespace mbrwt;

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::max(1.0, std::fabs(b)); }

// candidates A (1.00, 100), B (1.10, 80), C (1.12, 60), D (1.50, 10), in order
static std::vector<Cand> abcd() {
    return {{64, 1, 1.00, 100.0}, {64, 2, 1.10, 80.0}, {64, 3, 1.12, 60.0}, {64, 4, 1.50, 10.0}};
}

TEST(Choice, table) {
    const std::vector<Cand> c = abcd();
    const Cand *A = &c[0], *C = &c[2];
    // A does not fit; tmin 1.10, limit 1.122: B and C qualify, C is smaller
    Choice ch = choose_block(c, 90.0, 1.02);
    EXPECT_TRUE(near(ch.tmin, 1.10));
    EXPECT_TRUE(ch.best == C);
    // limit 1.43: D is out
    EXPECT_TRUE(choose_block(c, 90.0, 1.30).best == C);
    // only A qualifies
    ch = choose_block(c, 200.0, 1.02);
    EXPECT_TRUE(near(ch.tmin, 1.00));
    EXPECT_TRUE(ch.best == A);
    EXPECT_TRUE(choose_block(c, 200.0, 1.30).best == C);
}

TEST(Choice, nothing_fits) {
    const std::vector<Cand> c = abcd();
    for (double tol : {1.0, 1.02, 1.30, 100.0}) {
        const Choice ch = choose_block(c, 5.0, tol);
        EXPECT_TRUE(ch.best == nullptr);
        EXPECT_EQ(ch.tmin, kNoFit);
    }
    EXPECT_TRUE(choose_block({}, 1e9, 1.02).best == nullptr);
}

TEST(Choice, tie_takes_the_earlier) {
    const std::vector<Cand> c = {{64, 1, 1.00, 50.0}, {64, 2, 1.01, 40.0}, {128, 3, 1.015, 40.0}, {128, 5, 1.5, 5.0}};
    const Choice ch = choose_block(c, 100.0, 1.02);
    EXPECT_TRUE(ch.best == &c[1]);
}

TEST(Tolerance, rule) {
    EXPECT_EQ(cost_tolerance(false, true), 1.02);
    EXPECT_EQ(cost_tolerance(true, true), 1.30);
    EXPECT_EQ(cost_tolerance(false, false), 1.30);
    EXPECT_EQ(cost_tolerance(true, false), 1.30);
    EXPECT_EQ(kAutoMaxCost, 1.25);
    EXPECT_EQ(kCost128, 1.6);
}

TEST(Cost, requests_and_bytes) {
    const PlanCounts o{200, 50, 2};  // nr = 1000: 200 spilled, 2 long
    EXPECT_TRUE(near(price_candidate({64, 3}, o, 1000, 10000).t, 1.3));
    EXPECT_TRUE(near(price_candidate({128, 3}, o, 1000, 10000).t, 2.08));
    // ceil(10000 / 3) * 64 + 50 * 16 * 10
    const Cand c = price_candidate({64, 3}, o, 1000, 10000);
    EXPECT_EQ(c.mem, 221376.0);
    EXPECT_EQ(c.B, 64u);
    EXPECT_EQ(c.S, 3u);
    EXPECT_EQ(3334.0 * 64 + 50 * 16 * 10, 221376.0);
}

TEST(Candidates, list) {
    const std::vector<BlockShape> all = block_candidates(360360);
    ASSERT_EQ(all.size(), (size_t)23);
    for (size_t i = 0; i < 8; ++i) {  // B = 64, S = 1..8, then B = 128, S = 1..15
        EXPECT_EQ(all[i].B, 64u);
        EXPECT_EQ(all[i].S, (uint32_t)i + 1);
    }
    for (size_t i = 8; i < 23; ++i) {
        EXPECT_EQ(all[i].B, 128u);
        EXPECT_EQ(all[i].S, (uint32_t)i - 7);
    }
    const std::vector<BlockShape> p = block_candidates(13);
    ASSERT_EQ(p.size(), (size_t)3);
    EXPECT_TRUE(p[0].B == 64 && p[0].S == 1);
    EXPECT_TRUE(p[1].B == 128 && p[1].S == 1);
    EXPECT_TRUE(p[2].B == 128 && p[2].S == 13);
}

TEST(Override, accepted_and_ignored) {
    const uint64_t align = 360360;
    BlockShape bs{0, 0};
    EXPECT_TRUE(block_override(64u << 8 | 8, align, bs));
    EXPECT_TRUE(bs.B == 64 && bs.S == 8);
    EXPECT_TRUE(block_override(128u << 8 | 15, align, bs));
    EXPECT_TRUE(bs.B == 128 && bs.S == 15);
    bs = {7, 7};
    EXPECT_FALSE(block_override(64u << 8 | 9, align, bs));
    EXPECT_FALSE(block_override(96u << 8 | 1, align, bs));
    EXPECT_FALSE(block_override(128u << 8 | 0, align, bs));
    EXPECT_FALSE(block_override(128u << 8 | 3, 13, bs));  // S does not divide the alignment
    EXPECT_FALSE(block_override(64u << 8 | 7, 360360 / 7, bs));
    EXPECT_TRUE(bs.B == 7 && bs.S == 7);  // an ignored override leaves the choice alone
    EXPECT_TRUE(block_override(128u << 8 | 13, 13, bs));
}

TEST(Magic, exact_division) {
    EXPECT_EQ(div_magic(1), (uint64_t)0);
    for (uint32_t S = 2; S <= 15; ++S) {
        const uint64_t magic = div_magic(S);
        const uint64_t rows[] = {0, 1, S - 1, S, (1ull << 32) - 1, (1ull << 32) + 1, (1ull << 59) - 1};
        for (uint64_t row : rows) {
            const uint64_t hi = (uint64_t)(((unsigned __int128)row * magic) >> 64);  // umulhi
            EXPECT_EQ(hi, row / S);
        }
    }
}

TEST(CodeRule, terminal_records) {
    EXPECT_FALSE(term_gives_way(0, 90, 100));  // keeps
    EXPECT_TRUE(term_gives_way(0, 100, 100));  // no smaller: drops
    EXPECT_TRUE(term_gives_way(1, 50, 100));   // a row the fields cannot hold: drops
}

TEST(CodeRule, nibble_codes) {
    EXPECT_TRUE(nib_gives_way(0, 100, 100));   // drops
    EXPECT_FALSE(nib_gives_way(1, 100, 100));  // keeps: the caller then reports the bad row
    EXPECT_FALSE(nib_gives_way(0, 90, 100));
}

TEST(VarBytes, estimates) {
    // 1000 record bytes over 100 of 1300 rows, ranges of 650 rows:
    // 1000 * 13 * 1.02 + 100 lines * 64 + 64 * (1 + 2)
    EXPECT_TRUE(near(var_image_bytes(1000, 100, 1300, 650), 13260.0 + 6400.0 + 192.0));
    EXPECT_EQ(var_pending_bytes(10.0, 1000), (uint64_t)10200 + (64ull << 20));
    EXPECT_EQ(var_pending_bytes(0.0, 0), 64ull << 20);
}

int main(int argc, char **argv) { return minitest::run_all(argc > 1 ? argv[1] : nullptr); }
