// kt_miobi_host.h -- the host-only parts of kt_miobi_make's driver
// (kt_miobi.cpp): the candidate ranking, the adjacency
// bitmask of the candidate block and the bookkeeping of the candidate count m.
// Plain C++ with no device call, so that a stand-alone host program can run
// them under a sanitizer (tests/native/miobi_make_check/host_san.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace kt {

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

}  // namespace kt
