// BRWTMultiDevice's batched classify (csrc/brwt_device.hpp labels_batch_csr,
// top_labels_batch_csr over mbrwt_multi_get[_top]_labels_batch) on two
// replicas of device 0, against StaticBinRelAnnotator's per-read count_labels
// semantics (annotate_static.cpp:71-94, :149-162; annotate.cpp:57-83)
// computed over the oracle matrix.  Needs a GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../backends.hpp"
#include "../minitest.hpp"

namespace {

struct Fixture {
    OracleMatrix oracle;
    mbrwt_host::BRWTMultiDevice multi;
    std::vector<uint64_t> rows, read_off;
};

Fixture make() {
    const uint64_t n = 3000, m = 40;
    uint64_t s = 99;
    auto next = [&]() { return (s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33; };
    std::vector<std::vector<bool>> cols(m, std::vector<bool>(n, false));
    for (uint64_t j = 0; j < m; ++j)
        for (uint64_t i = 0; i < n; ++i) cols[j][i] = next() % 100 < 8;
    OracleMatrix om(build_oracle(cols, n, 0, 4, 0));
    DescStorage st;
    const mbrwt_tree_desc d = oracle_desc(om, st);
    Fixture f{om, mbrwt_host::BRWTMultiDevice(d, {0, 0}), {}, {0}};
    for (int r = 0; r < 150; ++r) {  // reads of 0..29 rows around an anchor
        const uint64_t len = next() % 30, anchor = next() % (n - 64);
        for (uint64_t i = 0; i < len; ++i) f.rows.push_back(anchor + next() % 64);
        f.read_off.push_back(f.rows.size());
    }
    return f;
}

// count_labels of one read over the oracle (annotate_static.cpp:149-162)
std::vector<uint64_t> count_labels(const Fixture &f, uint64_t r) {
    std::vector<uint64_t> counts(f.oracle.num_columns(), 0);
    for (uint64_t i = f.read_off[r]; i < f.read_off[r + 1]; ++i)
        for (auto c : f.oracle.get_row(f.rows[i])) ++counts[c];
    return counts;
}

}  // namespace

TEST(MultiMirror, LabelsBatchOnEveryReplica) {
    const Fixture f = make();
    ASSERT_EQ(f.multi.replicas(), 2);
    const uint64_t n_reads = f.read_off.size() - 1;
    for (double ratio : {0.0, 0.3, 1.0}) {
        std::vector<uint64_t> lab_off;
        std::vector<uint32_t> labels;
        // true: answered by the device call, not left to the per-read host fallback
        ASSERT_TRUE(f.multi.labels_batch_csr(f.rows, f.read_off, ratio, &lab_off, &labels));
        ASSERT_EQ(lab_off.size(), n_reads + 1);
        std::vector<uint64_t> want_off{0};
        std::vector<uint32_t> want;
        for (uint64_t r = 0; r < n_reads; ++r) {
            const uint64_t len = f.read_off[r + 1] - f.read_off[r];
            const uint64_t thr = ratio == 0 ? 1 : (uint64_t)std::ceil(len * ratio);
            const auto counts = count_labels(f, r);
            for (size_t c = 0; c < counts.size(); ++c)
                if (counts[c] && counts[c] >= thr) want.push_back((uint32_t)c);
            want_off.push_back(want.size());
        }
        EXPECT_EQ(lab_off, want_off);
        EXPECT_EQ(labels, want);
    }
}

TEST(MultiMirror, TopLabelsBatchOnEveryReplica) {
    const Fixture f = make();
    const uint64_t n_reads = f.read_off.size() - 1;
    for (uint64_t num_top : {(uint64_t)-1, (uint64_t)3, (uint64_t)0}) {
        std::vector<uint64_t> lab_off, counts;
        std::vector<uint32_t> labels;
        ASSERT_TRUE(f.multi.top_labels_batch_csr(f.rows, f.read_off, num_top, &lab_off, &labels, &counts));
        std::vector<uint64_t> want_off{0}, want_c;
        std::vector<uint32_t> want_l;
        for (uint64_t r = 0; r < n_reads; ++r) {
            const auto cnt = count_labels(f, r);
            std::vector<std::pair<uint64_t, uint32_t>> top;  // by count descending, then label ascending
            for (size_t c = 0; c < cnt.size(); ++c)
                if (cnt[c]) top.emplace_back(cnt[c], (uint32_t)c);
            std::sort(top.begin(), top.end(),
                      [](const auto &a, const auto &b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
            top.resize(std::min<uint64_t>(top.size(), num_top));
            for (const auto &p : top) {
                want_l.push_back(p.second);
                want_c.push_back(p.first);
            }
            want_off.push_back(want_l.size());
        }
        EXPECT_EQ(lab_off, want_off);
        EXPECT_EQ(labels, want_l);
        EXPECT_EQ(counts, want_c);
    }
}

// the annotator over the multi-device matrix takes the batched path and
// answers as it does read by read
TEST(MultiMirror, AnnotatorBatchEqualsPerRead) {
    const Fixture f = make();
    mbrwt_host::LabelEncoder<std::string> enc;
    for (uint64_t c = 0; c < f.oracle.num_columns(); ++c) enc.insert_and_encode("label" + std::to_string(c));
    mbrwt_host::StaticBinRelAnnotator<mbrwt_host::BRWTMultiDevice> anno(
        std::make_shared<mbrwt_host::BRWTMultiDevice>(f.multi), enc);
    std::vector<std::vector<uint64_t>> reads;
    for (size_t r = 0; r + 1 < f.read_off.size() && r < 20; ++r)
        reads.emplace_back(f.rows.begin() + f.read_off[r], f.rows.begin() + f.read_off[r + 1]);
    const auto got = anno.get_labels_batch(reads, 0.5);
    ASSERT_EQ(got.size(), reads.size());
    for (size_t r = 0; r < reads.size(); ++r) EXPECT_EQ(got[r], anno.get_labels(reads[r], 0.5));
}

int main() { return minitest::run_all(); }
