// rows_select.hpp -- get_column by predicate over the row ids, for every
// record form (rows.hip, rows_var.hip, rows_class.hip): the rows whose record
// holds the column, ascending (BRWT::get_column, BRWT.cpp:55-85), under the
// capacity protocol of mbrwt_get_column.
#pragma once

#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "mbrwt_internal.hpp"

namespace mbrwt {

// a predicate over row ids as the 0 / 1 summand of a reduce
template <class Pred>
struct CountIf {
    Pred f;
    __device__ uint64_t operator()(const uint64_t &row) const { return f(row) ? 1u : 0u; }
};

// The rows of [0, n) that satisfy `f`: the column's size first (a reduce over
// the rows, into *rows_needed), then the rows (a select) into d_rows when it
// is given and holds them -- a null buffer only asks for the size.
template <class Pred>
int select_rows(Ctx &c, uint64_t n, const Pred &f, uint64_t *d_rows, uint64_t rows_cap, uint64_t *rows_needed,
                hipStream_t s) {
    hipcub::CountingInputIterator<uint64_t> rows_it(0);
    hipcub::TransformInputIterator<uint64_t, CountIf<Pred>, hipcub::CountingInputIterator<uint64_t>> cnt_it(
        rows_it, CountIf<Pred>{f});
    int rc;
    size_t red_bytes = 0, sel_bytes = 0;
    uint64_t *d_num = reinterpret_cast<uint64_t *>(c.d_scalars);
    MBRWT_HIP(hipcub::DeviceReduce::Sum(nullptr, red_bytes, cnt_it, d_num, n, s));
    if ((rc = ensure(c.ws_scan, std::max<size_t>(red_bytes, 256)))) return rc;
    MBRWT_HIP(hipcub::DeviceReduce::Sum(c.ws_scan.buf, red_bytes, cnt_it, d_num, n, s));
    MBRWT_HIP(hipMemcpyAsync(c.h_scalars, c.d_scalars, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    MBRWT_HIP(hipStreamSynchronize(s));
    const uint64_t need = c.h_scalars[0];
    if (rows_needed) *rows_needed = need;
    if (!d_rows || need > rows_cap) {
        if (need > rows_cap) {
            set_error("rows_cap too small");
            return MBRWT_ERR_CAPACITY;
        }
        return MBRWT_OK;
    }
    if (!need) return MBRWT_OK;
    MBRWT_HIP(hipcub::DeviceSelect::If(nullptr, sel_bytes, rows_it, d_rows, d_num, n, f, s));
    if ((rc = ensure(c.ws_scan, sel_bytes))) return rc;
    MBRWT_HIP(hipcub::DeviceSelect::If(c.ws_scan.buf, sel_bytes, rows_it, d_rows, d_num, n, f, s));
    MBRWT_HIP(hipStreamSynchronize(s));
    return MBRWT_OK;
}

}  // namespace mbrwt
