// The host-side argument checks of mbrwt_get_columns / mbrwt_get_columns_device
// that need no context: a null ctx or null offsets is MBRWT_ERR_INVALID before
// any HIP call, and no output buffer is written.  Stand-alone (no GPU); `make
// sanitize` builds it with AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../../include/mbrwt.h"

int main() {
    int failed = 0;
    auto expect = [&](bool ok, const char *what) {
        if (!ok) {
            std::printf("FAILED: %s\n", what);
            ++failed;
        }
    };
    std::vector<uint64_t> columns{3, 3, 1ull << 40}, offsets(4, 77), rows(8, 88);
    uint64_t need = 99;
    expect(mbrwt_get_columns(nullptr, columns.data(), columns.size(), 0, 10, offsets.data(), rows.data(), rows.size(),
                             &need) == MBRWT_ERR_INVALID,
           "host form, null ctx");
    expect(mbrwt_get_columns(nullptr, nullptr, 0, 5, 4, nullptr, nullptr, 0, nullptr) == MBRWT_ERR_INVALID,
           "host form, everything null");
    expect(mbrwt_get_columns_device(nullptr, columns.data(), columns.size(), 0, 10, offsets.data(), rows.data(),
                                    rows.size(), &need, nullptr) == MBRWT_ERR_INVALID,
           "device form, null ctx");
    expect(mbrwt_get_columns_device(nullptr, nullptr, ~0ull, ~0ull, 0, nullptr, nullptr, ~0ull, nullptr, nullptr) ==
               MBRWT_ERR_INVALID,
           "device form, everything null");
    expect(need == 99, "rows_needed untouched");
    for (uint64_t v : offsets) expect(v == 77, "offsets untouched");
    for (uint64_t v : rows) expect(v == 88, "rows untouched");
    expect(mbrwt_set_option(nullptr, MBRWT_OPT_COLUMNS_CHUNK, 5) == MBRWT_ERR_INVALID, "option on a null ctx");
    std::printf("get_columns argument checks: %d failed\n", failed);
    return failed ? 1 : 0;
}
