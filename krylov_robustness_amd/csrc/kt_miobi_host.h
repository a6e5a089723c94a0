// kt_miobi_host.h -- the host-only parts of the MIOBI drivers (kt_miobi.cpp):
// of their shared window loop, the edge window length and the step-count
// check; of kt_miobi_make's: the candidate ranking, the adjacency
// bitmask of the candidate block and the bookkeeping of the candidate count m;
// and of kt_miobi_break_node's (§4.2g): the argument scan, the window length,
// the removed-entry count replayed, the long-row list and the row / column
// removal.  Plain C++ with no device call, so that a stand-alone host program
// can run them under a sanitizer (tests/native/miobi_make_check/host_san.cpp,
// tests/native/miobi_node_check/host_san.cpp,
// tests/native/miobi_window_check/host_san.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace kt {

// ---- the window loop all three drivers share -------------------------------

// the steps to queue for one window of the edge drivers (kt_miobi_break,
// kt_miobi_make): up to the next multiple of `refresh` steps, where the
// eigenpairs are recomputed (MIOBIBreakEdge2.m:255, MIOBIMakeEdge.m:326);
// refresh <= 0: all that remain
inline int miobi_edge_window(int remaining, int done, int refresh) {
    return refresh > 0 ? std::min(remaining, refresh - done % refresh) : remaining;
}

// whether the device's step count after a window of w queued steps can be
// right: it started at `done` and every step adds one or, past a stop, nothing
inline bool miobi_step_in_window(int now, int done, int w) { return now >= done && now <= done + w; }

// ---- make (kt_miobi_make, MIOBIMakeEdge.m) ---------------------------------

// max(sum(A, 2)) of a unit-weight matrix: the longest row (MIOBIMakeEdge.m:60-61)
inline int miobi_max_degree(int64_t n, const int64_t* rowptr) {
    int64_t d = 0;
    for (int64_t i = 0; i < n; ++i) d = std::max(d, rowptr[i + 1] - rowptr[i]);
    return (int)d;
}

// m = min(maxDegree + k, N) with k the WHOLE budget (:63)
inline int miobi_live_m(int maxdeg, int k, int64_t n) { return (int)std::min<int64_t>((int64_t)maxdeg + k, n); }

// the ranks a window of w steps can reach: m grows by at most one per step
inline int miobi_cap_m(int maxdeg, int k, int w, int64_t n) {
    return (int)std::min<int64_t>((int64_t)maxdeg + k + w, n);
}

// node[r] = the node at rank r < mcap of sort(v0, 'descend') (:62): the value
// descending, equal values by ascending index -- what a stable sort gives.  The
// comparison is a strict total order, so the first mcap of it need no full sort.
inline void miobi_rank(int64_t n, const double* v0, int mcap, std::vector<int>& node) {
    std::vector<int> idx((size_t)n);
    for (int64_t i = 0; i < n; ++i) idx[(size_t)i] = (int)i;
    const auto first = [v0](int x, int y) { return v0[x] != v0[y] ? v0[x] > v0[y] : x < y; };
    std::partial_sort(idx.begin(), idx.begin() + mcap, idx.end(), first);
    node.assign(idx.begin(), idx.begin() + mcap);
}

// rank_of[node[a]] = a for the candidates (set), or back to -1 (clear); the
// other entries of the n-vector stay -1
inline void miobi_set_ranks(const std::vector<int>& node, std::vector<int>& rank_of, bool set) {
    for (size_t a = 0; a < node.size(); ++a) rank_of[(size_t)node[a]] = set ? (int)a : -1;
}

// rank_of: as miobi_set_ranks(node, rank_of, true) leaves it.
// mask: mcap rows of words = ceil(mcap / 64) 64-bit words, bit (a, b) set when
// node[a] and node[b] are adjacent in the CSR (both halves of a symmetric
// matrix; a diagonal entry sets (a, a), which no pair reads).  deg[a] = the
// row length of node[a].
inline void miobi_build_mask(const int64_t* rowptr, const int32_t* col, const std::vector<int>& node,
                             const std::vector<int>& rank_of, std::vector<uint64_t>& mask,
                             std::vector<int>& deg) {
    const int mcap = (int)node.size(), words = (mcap + 63) / 64;
    mask.assign((size_t)mcap * words, 0);
    deg.assign((size_t)mcap, 0);
    for (int a = 0; a < mcap; ++a) {
        const int64_t beg = rowptr[node[a]], end = rowptr[node[a] + 1];
        deg[a] = (int)(end - beg);
        for (int64_t q = beg; q < end; ++q) {
            const int b = rank_of[(size_t)col[q]];
            if (b >= 0) mask[(size_t)a * words + (b >> 6)] |= 1ull << (b & 63);
        }
    }
}

// The device's bookkeeping replayed: the pair of ranks (a, b) gains an edge.
// Returns the m of the NEXT step; deg, maxdeg are updated in place.
inline int miobi_book_step(std::vector<int>& deg, int& maxdeg, int a, int b, int k, int64_t n) {
    maxdeg = std::max(maxdeg, std::max(++deg[(size_t)a], ++deg[(size_t)b]));
    return miobi_live_m(maxdeg, k, n);
}

// ---- break-node (kt_miobi_break_node, MIOBIBreakNode.m) --------------------

// whether the CSR holds an entry (i, i)
inline bool miobi_has_diagonal(int64_t n, const int64_t* rowptr, const int32_t* col) {
    for (int64_t i = 0; i < n; ++i)
        for (int64_t q = rowptr[i]; q < rowptr[i + 1]; ++q)
            if (col[q] == i) return true;
    return false;
}

// the steps to queue for one window: a selected node has degree >= 1 and so
// adds at least 2 to the removed-entry count, which reaches `refresh` within
// ceil(refresh / 2) steps (MIOBIBreakNode.m:208, :283-286); refresh <= 0: all
inline int miobi_node_window(int remaining, int refresh) {
    return refresh > 0 ? std::min(remaining, (refresh + 1) / 2) : remaining;
}

// the device's count replayed for one step: acc += 2 deg; at or beyond refresh
// (> 0) the window ends and acc %= refresh (:283-292).  Returns whether it ends.
inline bool miobi_node_book(int& acc, int deg, int refresh) {
    if (refresh <= 0) return false;
    const int64_t a = (int64_t)acc + 2 * (int64_t)deg;
    acc = (int)(a >= refresh ? a % refresh : a);
    return a >= refresh;
}

// the rows longer than thresh, ascending
inline void miobi_long_rows(int64_t n, const int64_t* rowptr, int thresh, std::vector<int>& rows) {
    rows.clear();
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] - rowptr[i] > thresh) rows.push_back((int)i);
}

// A(r, :) = 0, A(:, r) = 0 for every r with dead[r] (:211-212) in one pass over
// the CSR; val may be empty (no values kept).  Returns the entries removed.
inline int64_t miobi_clear_nodes(int64_t n, const std::vector<unsigned char>& dead, std::vector<int64_t>& rowptr,
                                 std::vector<int32_t>& col, std::vector<double>& val) {
    int64_t w = 0, beg = 0;
    const bool vals = !val.empty();
    for (int64_t i = 0; i < n; ++i) {
        const int64_t end = rowptr[i + 1];
        if (!dead[(size_t)i])
            for (int64_t q = beg; q < end; ++q)
                if (!dead[(size_t)col[q]]) {
                    col[(size_t)w] = col[q];
                    if (vals) val[(size_t)w] = val[q];
                    ++w;
                }
        beg = end;
        rowptr[i + 1] = w;
    }
    const int64_t removed = (int64_t)col.size() - w;
    col.resize((size_t)w);
    if (vals) val.resize((size_t)w);
    return removed;
}

}  // namespace kt
