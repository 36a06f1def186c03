// The host side of the build from sparse columns (csrc/cols_host.hpp: no
// HIP), stand-alone: the slice cutter, the staging, the work list, the sample
// intersection and the range sizing; then the null-argument statuses of the
// three entry points, which need no GPU.  Also built with the sanitizers
// (`make sanitize` here).  Exit status 0 and "cols_host ok" on success.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "../../../genome_graph_annotation_amd/csrc/cols_host.hpp"
#include "../../../include/mbrwt.h"

namespace {

using namespace mbrwt;

int failures = 0;
#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            ++failures;                                                  \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
        }                                                                \
    } while (0)

uint64_t rng_state = 12345;
uint64_t rnd() { return (rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull) >> 17; }

struct Cols {
    uint64_t n = 0;
    std::vector<uint64_t> off{0}, ids;
    std::vector<uint32_t> ids32;
    void add(const std::set<uint64_t> &s) {
        ids.insert(ids.end(), s.begin(), s.end());
        off.push_back(ids.size());
    }
    ColsView view(bool narrow = false) {
        ColsView v;
        v.num_rows = n;
        v.num_columns = off.size() - 1;
        v.offsets = off.data();
        if (narrow) {
            ids32.assign(ids.begin(), ids.end());
            v.rows32 = ids32.data();
        } else {
            v.rows = ids.data();
        }
        return v;
    }
};

// walks `bounds` (0 = bounds[0] < ... < bounds.back() = n) with one cursor per
// column: the slices tile every column, hold exactly the ids of their range,
// and are staged in perm order as id - a
void walk(Cols &c, const std::vector<uint64_t> &bounds, bool narrow) {
    const ColsView v = c.view(narrow);
    const uint64_t m = v.num_columns;
    std::vector<uint32_t> perm(m);
    for (uint64_t k = 0; k < m; ++k) perm[k] = (uint32_t)((k * 7 + 3) % m);  // (m not a multiple of 7)
    std::vector<uint64_t> cur(c.off.begin(), c.off.end() - 1), ends;
    uint64_t total = 0;
    for (size_t i = 0; i + 1 < bounds.size(); ++i) {
        const uint64_t a = bounds[i], b = bounds[i + 1];
        const uint64_t L = cols_cut_slices(v, cur, b, &ends);
        CHECK(L == cols_cut_slices(v, cur, b, nullptr));
        for (uint64_t col = 0; col < m; ++col) {
            CHECK(cur[col] <= ends[col] && ends[col] <= c.off[col + 1]);
            for (uint64_t p = cur[col]; p < ends[col]; ++p) CHECK(v.id(p) >= a && v.id(p) < b);
            if (ends[col] < c.off[col + 1]) CHECK(v.id(ends[col]) >= b);
        }
        std::vector<uint32_t> soff, out(L + 1, 0xABCDABCDu);
        cols_stage_offsets(perm, cur, ends, soff);
        CHECK(soff.size() == m + 1 && soff[0] == 0 && soff[m] == L);
        cols_stage(v, perm, cur, soff, a, out.data());
        CHECK(out[L] == 0xABCDABCDu);
        for (uint64_t k = 0; k < m; ++k) {
            CHECK(soff[k + 1] - soff[k] == ends[perm[k]] - cur[perm[k]]);
            for (uint32_t p = soff[k]; p < soff[k + 1]; ++p) CHECK(out[p] == v.id(cur[perm[k]] + (p - soff[k])) - a);
        }
        // staged in parts that split slices anywhere
        std::vector<uint32_t> parts(L, 0);
        for (uint32_t p0 = 0; p0 < L; p0 += 3)
            cols_stage_part(v, perm, cur, soff, a, p0, (uint32_t)std::min<uint64_t>(L, p0 + 3), parts.data());
        for (uint64_t p = 0; p < L; ++p) CHECK(parts[p] == out[p]);
        std::vector<ColsWork> work;
        cols_work_list(soff, work);
        uint64_t covered = 0;
        for (size_t w = 0; w < work.size(); ++w) {
            const uint32_t k = work[w].key;
            CHECK(k < m && work[w].begin >= soff[k] && work[w].begin < soff[k + 1]);
            CHECK((work[w].begin - soff[k]) % kColsChunk == 0);
            covered += std::min<uint64_t>(soff[k + 1], (uint64_t)work[w].begin + kColsChunk) - work[w].begin;
            if (w) CHECK(work[w - 1].key < k || (work[w - 1].key == k && work[w - 1].begin + kColsChunk == work[w].begin));
        }
        CHECK(covered == L);
        total += L;
        cur.swap(ends);
    }
    for (uint64_t col = 0; col < m; ++col) CHECK(cur[col] == c.off[col + 1]);  // the slices tiled every column
    CHECK(total == c.ids.size());
}

void slices() {
    // ids at the edges of the ranges, empty columns, a column inside one range,
    // a column of every row of a range (more than one chunk of the work list)
    Cols c;
    c.n = 10000;
    const std::vector<uint64_t> bounds{0, 3000, 3001, 7000, 10000};
    c.add({});
    c.add({0, 2999, 3000, 3001, 6999, 7000, 9999});
    c.add({2999});
    c.add({3000});
    c.add({});
    std::set<uint64_t> mid, all;
    for (uint64_t r = 3001; r < 7000; ++r) mid.insert(r);
    for (uint64_t r = 0; r < c.n; ++r) all.insert(r);
    c.add(mid);
    c.add(all);
    for (int j = 0; j < 4; ++j) {
        std::set<uint64_t> s;
        for (int i = 0; i < 500; ++i) s.insert(rnd() % c.n);
        c.add(s);
    }
    c.add({9999});
    c.add({});
    walk(c, bounds, false);
    walk(c, bounds, true);
    walk(c, {0, c.n}, true);  // one range from row 0: the u32 ids copied as they are
    // u64 ids above 2^32, ranges that begin beyond 2^32: the u32 rebasing
    Cols big;
    const uint64_t G = 1ull << 32;
    big.n = 2 * G + 1000;
    const std::vector<uint64_t> bb{0, G - 10, G + 5, 2 * G, big.n};  // (a range holds fewer than 2^32 - 1 rows)
    big.add({0, 7, G - 1, G, G + 4, G + 5, G + 6, 2 * G - 1, 2 * G, 2 * G + 999});
    big.add({});
    big.add({G + 5, 2 * G - 1});
    big.add({2 * G + 1});
    for (int j = 0; j < 5; ++j) {
        std::set<uint64_t> s;
        for (int i = 0; i < 300; ++i) s.insert(rnd() % big.n);
        big.add(s);
    }
    walk(big, bb, false);
    // the local row of an id outside [a, a + 2^32 - 1) is the bad row
    CHECK(cols_local_row(G + 5, G + 5) == 0);
    CHECK(cols_local_row(2 * G + 3, G + 5) == G - 2);
    CHECK(cols_local_row(G + 4, G + 5) == kColsBadRow);
    CHECK(cols_local_row(2 * G + 4, G + 5) == kColsBadRow);
    CHECK(cols_local_row(~0ull, 0) == kColsBadRow);
    // ids that do not ascend: the bisection still answers inside the column,
    // so the slices tile it and the misplaced id is staged as out of range
    Cols bad;
    bad.n = 1000;
    bad.off = {0, 6};
    bad.ids = {10, 600, 20, 700, 30, 800};
    const ColsView v = bad.view();
    std::vector<uint64_t> cur{0}, ends;
    uint64_t seen = 0;
    bool flagged = false;
    for (const uint64_t a : {0ull, 500ull}) {
        const uint64_t b = a + 500;
        seen += cols_cut_slices(v, cur, b, &ends);
        for (uint64_t p = cur[0]; p < ends[0]; ++p) flagged |= cols_local_row(v.id(p), a) >= 500;
        cur.swap(ends);
    }
    CHECK(seen == 6 && cur[0] == 6 && flagged);
}

void sample() {
    Cols c;
    c.n = 200000;
    std::vector<uint64_t> s;
    {
        std::set<uint64_t> pick;
        while (pick.size() < 5000) pick.insert(rnd() % c.n);
        s.assign(pick.begin(), pick.end());
    }
    std::set<uint64_t> few, many, some;
    for (int i = 0; i < 100; ++i) few.insert(i % 2 ? s[rnd() % s.size()] : rnd() % c.n);   // len * 16 < ns
    for (uint64_t r = 0; r < c.n; ++r)
        if (rnd() % 10 < 7) many.insert(r);                                               // ns * 16 < len
    for (int i = 0; i < 6000; ++i) some.insert(i % 3 ? rnd() % c.n : s[rnd() % s.size()]);  // the merge
    c.add(few);
    c.add(many);
    c.add(some);
    c.add({});
    c.add({s.front()});
    c.add({s.back()});
    const ColsView v = c.view();
    const std::set<uint64_t> *sets[] = {&few, &many, &some};
    for (uint64_t col = 0; col < v.num_columns; ++col) {
        std::vector<uint32_t> got{77}, want{77};  // (appended to what is there)
        CHECK(cols_sample_slots(v, col, &s, got));
        for (uint32_t k = 0; k < s.size(); ++k) {
            bool in = false;
            if (col < 3) in = sets[col]->count(s[k]) != 0;
            else if (col == 4) in = k == 0;
            else if (col == 5) in = k + 1 == s.size();
            if (in) want.push_back(k);
        }
        CHECK(got == want);
    }
    // every row its own slot: the ids themselves, checked
    Cols d;
    d.n = 100;
    d.add({0, 5, 99});
    d.add({});
    d.off.push_back(d.ids.size() + 2);
    d.ids.insert(d.ids.end(), {7, 7});  // a row twice
    d.off.push_back(d.ids.size() + 2);
    d.ids.insert(d.ids.end(), {9, 8});  // descending
    d.off.push_back(d.ids.size() + 1);
    d.ids.push_back(100);  // == num_rows
    const ColsView w = d.view();
    std::vector<uint32_t> out;
    CHECK(cols_sample_slots(w, 0, nullptr, out) && out == (std::vector<uint32_t>{0, 5, 99}));
    CHECK(cols_sample_slots(w, 1, nullptr, out) && out.size() == 3);
    for (uint64_t col = 2; col < 5; ++col) {
        std::vector<uint32_t> o;
        CHECK(!cols_sample_slots(w, col, nullptr, o));
    }
}

void sizing() {
    const uint64_t align = 360360, n = 100 * align + 17, a = 3 * align;
    const double roomy = 1e18;
    // a label count of exactly 2^31 - 1 is taken, one more is not (synthetic
    // cursors: the labels of [a, a + j align))
    for (const uint64_t at5 : {kColsMaxLabels, kColsMaxLabels + 1}) {
        auto labels = [&](uint64_t e) {
            const uint64_t j = (e - a + align - 1) / align;
            return j < 5 ? j * 1000 : j == 5 ? at5 : at5 + (j - 5) * 1000 + 1;
        };
        const uint64_t b = cut_cols_range(n, 16, a, 64 * align, align, false, roomy, labels);
        CHECK(b == a + (at5 == kColsMaxLabels ? 5 : 4) * align);
    }
    // everything fits: the whole R, or the rest of the rows
    auto none = [](uint64_t) { return (uint64_t)0; };
    CHECK(cut_cols_range(n, 16, a, 64 * align, align, false, roomy, none) == a + 64 * align);
    CHECK(cut_cols_range(n, 16, 99 * align, 64 * align, align, false, roomy, none) == n);
    // the budget: the bytes of j multiples fit exactly, one byte less does not
    auto per_row = [&](uint64_t e) { return (e - a) * 3; };
    const double seven = (double)cols_range_bytes(7 * align, 7 * align * 3, 16);
    CHECK(cut_cols_range(n, 16, a, 64 * align, align, false, seven, per_row) == a + 7 * align);
    CHECK(cut_cols_range(n, 16, a, 64 * align, align, false, seven - 1, per_row) == a + 6 * align);
    // nothing fits: one multiple is taken whatever it costs
    CHECK(cut_cols_range(n, 16, a, 64 * align, align, false, 0.0, per_row) == a + align);
    // a fixed range size is taken as it is
    auto huge = [](uint64_t) { return ~0ull; };
    CHECK(cut_cols_range(n, 16, a, 2 * align, align, true, 0.0, huge) == a + 2 * align);
    CHECK(cut_cols_range(n, 16, 99 * align, 2 * align, align, true, 0.0, huge) == n);
    // what a range allocates grows with every term
    CHECK(cols_range_bytes(10, 100, 4) < cols_range_bytes(11, 100, 4));
    CHECK(cols_range_bytes(10, 100, 4) < cols_range_bytes(10, 101, 4));
    CHECK(cols_range_bytes(10, 100, 4) < cols_range_bytes(10, 100, 5));
    CHECK(cols_threads(0) == 1 && cols_threads(~0ull >> 1) <= kColsMaxThreads);
}

void null_arguments() {
    const uint64_t off[3] = {0, 1, 2}, rows[2] = {0, 1};
    const mbrwt_sparse_columns_desc d{4, 2, off, rows, nullptr};
    mbrwt_ctx *ctx = nullptr;
    mbrwt_tree *tree = nullptr;
    uint64_t counts[8] = {0};
    CHECK(mbrwt_create_from_sparse_columns(nullptr, nullptr, 8, 0, &ctx) == MBRWT_ERR_INVALID);
    CHECK(mbrwt_last_error_message() && mbrwt_last_error_message()[0]);
    CHECK(mbrwt_create_from_sparse_columns(&d, nullptr, 8, 0, nullptr) == MBRWT_ERR_INVALID);
    CHECK(mbrwt_sparse_columns_node_counts(nullptr, nullptr, 8, 0, counts) == MBRWT_ERR_INVALID);
    CHECK(mbrwt_sparse_columns_node_counts(&d, nullptr, 8, 0, nullptr) == MBRWT_ERR_INVALID);
    CHECK(mbrwt_tree_shape_from_sparse_columns(nullptr, MBRWT_PARTITIONER_BASIC, 8, 0, 0, &tree) ==
          MBRWT_ERR_INVALID);
    CHECK(mbrwt_tree_shape_from_sparse_columns(&d, MBRWT_PARTITIONER_BASIC, 8, 0, 0, nullptr) == MBRWT_ERR_INVALID);
    CHECK(ctx == nullptr && tree == nullptr);
    // the descriptor's own checks come before any device call
    const mbrwt_sparse_columns_desc no_off{4, 2, nullptr, rows, nullptr};
    CHECK(mbrwt_sparse_columns_node_counts(&no_off, nullptr, 8, 0, counts) == MBRWT_ERR_INVALID);
    const uint32_t rows32[2] = {0, 1};
    const mbrwt_sparse_columns_desc both{4, 2, off, rows, rows32};
    CHECK(mbrwt_tree_shape_from_sparse_columns(&both, MBRWT_PARTITIONER_GREEDY, 8, 0, 0, &tree) == MBRWT_ERR_INVALID);
    // the basic shape reads no id and needs no device
    CHECK(mbrwt_tree_shape_from_sparse_columns(&d, MBRWT_PARTITIONER_BASIC, 8, 0, 0, &tree) == MBRWT_OK);
    CHECK(tree && mbrwt_tree_get_desc(tree)->num_nodes == 3);
    mbrwt_tree_free(tree);
}

}  // namespace

int main() {
    slices();
    sample();
    sizing();
    null_arguments();
    if (failures) {
        std::printf("cols_host: %d failed checks\n", failures);
        return 1;
    }
    std::printf("cols_host ok\n");
    return 0;
}
