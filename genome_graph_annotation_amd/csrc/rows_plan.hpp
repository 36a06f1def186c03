// rows_plan.hpp -- the decisions of the row-record build (rows_build.hip
// rows_build_range: choose_code, choose_layout) as pure host code: the
// candidate block shapes, their cost model, the choice among them, the
// record-code rule and the variable-length byte estimates.  Standard headers
// only, so the rules are testable without a device (tests/cpp/test_rows_plan.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace mbrwt {

// ------------------------------------------------------------------------
// block shapes
// ------------------------------------------------------------------------
struct BlockShape {
    uint32_t B, S;  // block bytes (64 or 128), rows per block
};
inline uint32_t max_rows_per_block(uint32_t B) { return B == 64 ? 8u : 15u; }

// the candidates, in the order the choice breaks its ties by: S must divide
// `align` (every range of a build starts at a multiple of it)
inline std::vector<BlockShape> block_candidates(uint64_t align) {
    std::vector<BlockShape> out;
    for (uint32_t B : {64u, 128u})
        for (uint32_t S = 1; S <= max_rows_per_block(B); ++S)
            if (align % S == 0) out.push_back({B, S});
    return out;
}

// MBRWT_BUILD_ROWS_BLOCK: B << 8 | S; a value outside the candidates is ignored
inline bool block_override(uint32_t bs, uint64_t align, BlockShape &out) {
    const uint32_t Bv = bs >> 8, Sv = bs & 0xFFu;
    if (!((Bv == 64 || Bv == 128) && Sv >= 1 && Sv <= max_rows_per_block(Bv) && align % Sv == 0)) return false;
    out = {Bv, Sv};
    return true;
}

// row / S = umulhi(row, floor(2^64 / S) + 1), exact for rows < 2^59 and S <= 16
inline uint64_t div_magic(uint32_t S) { return S > 1 ? ((uint64_t)((((unsigned __int128)1) << 64) / S) + 1) : 0; }

// ------------------------------------------------------------------------
// cost model
// ------------------------------------------------------------------------
// (B, S): the fewest requests per row -- one block read plus one per
// spilled row, a 128-byte block costing kCost128 of a 64-byte one
// (measured ceilings), a record longer than a block a
// direct-pass row (x50) -- among the images that fit the device,
// then the smallest within 2 % of that
// a 128-byte block costs more than its request (random 128-byte reads
// run at 52.6 vs 53.7 G/s, profiles/r03/v01_probe_sweep.json): its
// LDS slots halve the traversal's resident waves -- the greedy +
// relax shape at 3.7 B rows took 0.859 ms with 128-byte blocks of 3
// rows against 0.522 ms with 64-byte blocks of one row
// (profiles/r04/v09_tree_odometer/)
constexpr double kCost128 = 1.6;

// the variable-length records (rows_var.hip: uniform trees, ranges
// on directory lines): for rows too long for the blocks -- a block
// layout costing more than kAutoMaxCost requests per row (most rows
// spilled, or records longer than a block) or none that fits.
// The build option MBRWT_BUILD_ROWS_VAR = 1 / 0 forces / forbids them.
// layout AUTO keeps the per-node images when the records are long
// enough that most rows would take a second (spill) request or the
// direct pass and no variable-length layout applies
constexpr double kAutoMaxCost = 1.25;

constexpr double kNoFit = 1e300;  // the fewest requests when no candidate fits the budget

// k_rows_plan's counters of one range under one (B, S)
struct PlanCounts {
    unsigned long long spilled, units, long_rows;  // rows, 16-byte spill units, rows longer than a block
};

struct Cand {
    uint32_t B, S;
    double t, mem;  // modelled requests per row, device bytes of the whole image
};

// a candidate priced from the counters of a range of nr rows, for an image of n rows
inline Cand price_candidate(BlockShape bs, const PlanCounts &o, uint64_t nr, uint64_t n) {
    const double scale = (double)n / (double)nr;
    const double fs = (double)o.spilled / nr, fl = (double)o.long_rows / nr;
    return Cand{bs.B, bs.S, (bs.B == 128 ? kCost128 : 1.0) * (1.0 + fs + 50.0 * fl),
                (double)((n + bs.S - 1) / bs.S) * bs.B + (double)o.units * 16.0 * scale};
}

// The smallest image within `tol` of the fewest modelled requests.
// The model prices a spilled row as a whole second request, which
// holds on the odometer's uniform trees (request-bound: C4 with
// three rows per block, 0.321 against 0.268 ms, profiles/r05), so
// there FAST keeps within 2 %.  Under the tree odometer (greedy +
// relax, non-uniform) the reloads overlap the other waves' walks
// (20 % of the rows spilled: +2 % kernel time, profiles/r04/v15_*),
// so from r05 such trees take the COMPACT tolerance (30 %) by
// default: two rows per block, 158.9 GB instead of 236.9 GB at
// 3.7 B rows.  MBRWT_BUILD_ROWS_FOOTPRINT = COMPACT takes 30 % always.
inline double cost_tolerance(bool compact_footprint, bool uniform_tree) {
    return compact_footprint || !uniform_tree ? 1.30 : 1.02;
}

struct Choice {
    double tmin;       // the fewest requests among the candidates that fit (kNoFit: none does)
    const Cand *best;  // the smallest of them within tmin * tol, the first on a tie (null: none fits)
};
inline Choice choose_block(const std::vector<Cand> &cands, double budget, double tol) {
    Choice ch{kNoFit, nullptr};
    for (const Cand &c : cands)
        if (c.mem <= budget) ch.tmin = std::min(ch.tmin, c.t);
    for (const Cand &c : cands)
        if (c.mem <= budget && c.t <= ch.tmin * tol && (!ch.best || c.mem < ch.best->mem)) ch.best = &c;
    return ch;
}

// ------------------------------------------------------------------------
// record code
// ------------------------------------------------------------------------
// nibble codes or terminal records that do not shrink the first range's
// records (dense rows: most masks hold several bits), or terminal
// fields a row of the range cannot take, give way to bytes for the
// whole image
// (k_rows_measure's counters: rows the code cannot hold, the records' bytes
// under the code, their bytes as byte masks)
inline bool term_gives_way(unsigned long long bad, unsigned long long bytes, unsigned long long byte_coded) {
    return bad || bytes >= byte_coded;
}
// (a bad row is not the nibble codes' doing: the caller reports it)
inline bool nib_gives_way(unsigned long long bad, unsigned long long bytes, unsigned long long byte_coded) {
    return bad == 0 && bytes >= byte_coded;
}

// ------------------------------------------------------------------------
// variable-length records: byte estimates
// ------------------------------------------------------------------------
constexpr uint64_t kVarLineRows = 13;  // rows per 64-byte directory line (rows_var.hip)
constexpr double kVarSlack = 1.02;     // over the first range's bytes per row

// the whole image of n rows (`align` rows per range at most), from the
// record bytes vb of a range of nr rows: records, directory lines, a line of
// padding per range
inline double var_image_bytes(uint64_t vb, uint64_t nr, uint64_t n, uint64_t align) {
    const double scale = (double)n / (double)nr;
    return (double)vb * scale * kVarSlack + (double)((n + kVarLineRows - 1) / kVarLineRows) * 64.0 +
           64.0 * (1 + n / align);
}
// what `rows` more rows will still allocate (one allocation per range)
inline uint64_t var_pending_bytes(double bytes_per_row, uint64_t rows) {
    return (uint64_t)(bytes_per_row * kVarSlack * (double)rows) + (64ull << 20);
}

}  // namespace mbrwt
