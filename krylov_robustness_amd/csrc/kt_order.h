// kt_order.h -- the row order of the relabelled (hub) CSR copy.  Host only, no
// HIP: tests/native/hub_order builds it into a stand-alone check program.
//
// Hubs first, as before: rows in descending degree class.  Rows up to
// long_thresh fall into classes of ceil(deg / 4) -- equal trips of the 4-deep
// gather loop, so the lanes of a wave still finish together -- and longer rows
// into exact-degree classes.  Inside a class the rows are ordered by their
// highest-degree neighbour outside the top kOrderHubRanks rows (the hubs stay
// L2-resident whatever the order), so that rows gathering the same mid-degree
// row run near each other and its lines are still in L2 at the next use; rows
// with no such neighbour go last.  Ties keep the original order, so equal
// inputs give equal orders.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace kt {

constexpr int64_t kOrderHubRanks = 4096;

inline int64_t order_class(int64_t deg, int long_thresh) { return deg > long_thresh ? deg : (deg + 3) / 4; }

// out = idx stably sorted by key (0 <= key < nkeys), ascending
inline void order_counting_sort(const std::vector<int32_t>& idx, const std::vector<int64_t>& key, int64_t nkeys,
                                std::vector<int32_t>& out) {
    std::vector<int64_t> cnt((size_t)nkeys + 1, 0);
    for (int32_t i : idx) cnt[(size_t)key[i] + 1]++;
    for (int64_t k = 0; k < nkeys; ++k) cnt[(size_t)k + 1] += cnt[(size_t)k];
    out.resize(idx.size());
    for (int32_t i : idx) out[(size_t)cnt[(size_t)key[i]]++] = i;
}

// new2old[r] = the original row at position r (n rows; rowptr, col: CSR of A
// in the original labels)
inline void hub_order(int64_t n, const int64_t* rowptr, const int32_t* col, int long_thresh,
                      std::vector<int32_t>& new2old) {
    std::vector<int32_t> ident((size_t)n), byrank;
    std::vector<int64_t> key((size_t)n);
    int64_t dmax = 0;
    for (int64_t i = 0; i < n; ++i) {
        ident[(size_t)i] = (int32_t)i;
        dmax = std::max(dmax, rowptr[i + 1] - rowptr[i]);
    }
    // degree rank: position in the stable descending-degree order
    for (int64_t i = 0; i < n; ++i) key[(size_t)i] = dmax - (rowptr[i + 1] - rowptr[i]);
    order_counting_sort(ident, key, dmax + 1, byrank);
    std::vector<int32_t> rank((size_t)n);
    for (int64_t r = 0; r < n; ++r) rank[(size_t)byrank[(size_t)r]] = (int32_t)r;
    // the neighbour key, then (stable) the class on top of it
    for (int64_t i = 0; i < n; ++i) {
        int64_t p = n;
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            const int64_t rc = rank[(size_t)col[k]];
            if (rc >= kOrderHubRanks && rc < p) p = rc;
        }
        key[(size_t)i] = p;
    }
    order_counting_sort(ident, key, n + 1, byrank);
    const int64_t cmax = order_class(dmax, long_thresh);
    for (int64_t i = 0; i < n; ++i) key[(size_t)i] = cmax - order_class(rowptr[i + 1] - rowptr[i], long_thresh);
    order_counting_sort(byrank, key, cmax + 1, new2old);
}

}  // namespace kt
