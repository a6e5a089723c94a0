// kt_order.h -- the row order of the relabelled (hub) CSR copy.  Host only, no
// HIP: tests/native/hub_order and tests/native/chain_order build it into
// stand-alone check programs.  hub_order is the base order described next;
// chain_order, further down, is what the copy is built in.
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

// hub_order with same-class neighbours chained: the base order is walked, and
// from each row not yet placed a run starts -- the row is placed, then, among
// its neighbours not yet placed and of the same class, the one of smallest
// degree rank, then one of that row's, until there is none.  Two adjacent rows
// of one run are processed by one row group in the same trip, so each one's
// gather of the other finds the line that the other's own-row read brings in.
// Rows longer than long_thresh (a whole wave each, exact-degree classes) are
// not chained; they lead the base order and keep their positions.  A run never
// leaves its class and the base order is class-major, so the classes stay
// contiguous and non-increasing.  Self loops are skipped.  Every row is
// scanned once, when it is placed: O(n + nnz) on top of hub_order.
inline void chain_order(int64_t n, const int64_t* rowptr, const int32_t* col, int long_thresh,
                        std::vector<int32_t>& new2old) {
    std::vector<int32_t> base, ident((size_t)n), byrank;
    hub_order(n, rowptr, col, long_thresh, base);
    std::vector<int64_t> key((size_t)n);
    int64_t dmax = 0;
    for (int64_t i = 0; i < n; ++i) {
        ident[(size_t)i] = (int32_t)i;
        dmax = std::max(dmax, rowptr[i + 1] - rowptr[i]);
    }
    // degree rank, as in hub_order
    for (int64_t i = 0; i < n; ++i) key[(size_t)i] = dmax - (rowptr[i + 1] - rowptr[i]);
    order_counting_sort(ident, key, dmax + 1, byrank);
    std::vector<int32_t> rank((size_t)n);
    for (int64_t r = 0; r < n; ++r) rank[(size_t)byrank[(size_t)r]] = (int32_t)r;
    std::vector<char> placed((size_t)n, 0);
    new2old.clear();
    new2old.reserve((size_t)n);
    for (int32_t start : base) {
        if (placed[(size_t)start]) continue;
        placed[(size_t)start] = 1;
        new2old.push_back(start);
        const int64_t deg = rowptr[start + 1] - rowptr[start];
        if (deg > long_thresh) continue;
        const int64_t cls = order_class(deg, long_thresh);
        for (int32_t cur = start;;) {
            int32_t next = -1;
            for (int64_t k = rowptr[cur]; k < rowptr[cur + 1]; ++k) {
                const int32_t c = col[k];
                if (c == cur || placed[(size_t)c]) continue;
                const int64_t dc = rowptr[c + 1] - rowptr[c];
                if (dc > long_thresh || order_class(dc, long_thresh) != cls) continue;
                if (next < 0 || rank[(size_t)c] < rank[(size_t)next]) next = c;
            }
            if (next < 0) break;
            placed[(size_t)next] = 1;
            new2old.push_back(next);
            cur = next;
        }
    }
}

}  // namespace kt
