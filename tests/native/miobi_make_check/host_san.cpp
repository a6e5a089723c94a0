// host_san -- TEST INFRASTRUCTURE: the host-only parts of kt_miobi_make's driver
// (kt_miobi_host.h: ranking, adjacency mask, m bookkeeping) on a 200-node
// graph against brute-force loops; built by `make host_san` with
// -fsanitize=address,undefined and run on the CPU.  Exit status 0: all agree.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kt_miobi_host.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

static int check(bool ok, const char* what) {
    if (!ok) printf("FAILED: %s\n", what);
    return ok ? 0 : 1;
}

int main() {
    const int n = 200, k = 12;
    // a symmetric 0/1 graph with a hub (node 17) and a few twins; dense copy for the brute force
    std::vector<char> D((size_t)n * n, 0);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (i == 17 || j == 17 ? rnd() % 3 == 0 : rnd() % 40 == 0) D[(size_t)i * n + j] = D[(size_t)j * n + i] = 1;
    std::vector<int64_t> rowptr(n + 1, 0);
    std::vector<int32_t> col;
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j)
            if (D[(size_t)i * n + j]) col.push_back(j);
        rowptr[i + 1] = (int64_t)col.size();
    }
    int bad = 0;
    int maxdeg = kt::miobi_max_degree(n, rowptr.data());
    int brute = 0;
    for (int i = 0; i < n; ++i) {
        int d = 0;
        for (int j = 0; j < n; ++j) d += D[(size_t)i * n + j];
        brute = std::max(brute, d);
    }
    bad += check(maxdeg == brute, "miobi_max_degree");
    bad += check(kt::miobi_live_m(maxdeg, k, n) == std::min(maxdeg + k, n), "miobi_live_m");
    bad += check(kt::miobi_live_m(n - 3, k, n) == n && kt::miobi_cap_m(n - 30, k, 50, n) == n, "the clamp at n");

    // values with exact ties (quantised), so that the index order decides
    std::vector<double> v0(n);
    for (int i = 0; i < n; ++i) v0[i] = (double)(rnd() % 23) / 23.0;
    for (int w : {1, 5, k}) {
        const int mcap = kt::miobi_cap_m(maxdeg, k, w, n);
        std::vector<int> node;
        kt::miobi_rank(n, v0.data(), mcap, node);
        // brute force: a stable insertion sort, descending
        std::vector<int> idx;
        for (int i = 0; i < n; ++i) {
            size_t p = idx.size();
            while (p > 0 && v0[idx[p - 1]] < v0[i]) --p;
            idx.insert(idx.begin() + (long)p, i);
        }
        bool same = (int)node.size() == mcap;
        for (int a = 0; a < mcap && same; ++a) same = node[a] == idx[a];
        bad += check(same, "miobi_rank against a stable descending sort");

        std::vector<int> rank_of(n, -1), deg;
        std::vector<uint64_t> mask;
        kt::miobi_set_ranks(node, rank_of, true);
        kt::miobi_build_mask(rowptr.data(), col.data(), node, rank_of, mask, deg);
        const int words = (mcap + 63) / 64;
        bool ok = (int)mask.size() == mcap * words && (int)deg.size() == mcap;
        for (int a = 0; a < mcap && ok; ++a) {
            int d = 0;
            for (int j = 0; j < n; ++j) d += D[(size_t)node[a] * n + j];
            ok = deg[a] == d;
            for (int b = 0; b < words * 64 && ok; ++b) {
                const bool got = (mask[(size_t)a * words + (b >> 6)] >> (b & 63)) & 1ull;
                ok = got == (b < mcap && D[(size_t)node[a] * n + node[b]]);
            }
        }
        bad += check(ok, "miobi_build_mask against the dense matrix");

        // bookkeeping: add w edges at the top ranks and compare with the degrees of the edited dense copy
        std::vector<char> E = D;
        int hmax = maxdeg, m = kt::miobi_live_m(maxdeg, k, n);
        ok = true;
        for (int s = 0, a = 0; s < w && ok; ++a)
            for (int b = a + 1; b < m && s < w && ok; ++b) {
                if (E[(size_t)node[a] * n + node[b]]) continue;
                E[(size_t)node[a] * n + node[b]] = E[(size_t)node[b] * n + node[a]] = 1;
                m = kt::miobi_book_step(deg, hmax, a, b, k, n);
                int bm = 0;
                for (int i = 0; i < n; ++i) {
                    int d = 0;
                    for (int j = 0; j < n; ++j) d += E[(size_t)i * n + j];
                    bm = std::max(bm, d);
                }
                ok = hmax == bm && m == std::min(bm + k, n) && m <= mcap;
                ++s;
            }
        bad += check(ok, "miobi_book_step against the edited dense matrix, m within mcap");
        kt::miobi_set_ranks(node, rank_of, false);
        ok = true;
        for (int i = 0; i < n; ++i) ok = ok && rank_of[i] == -1;
        bad += check(ok, "miobi_set_ranks clears what it set");
    }
    printf("%s\n", bad ? "host_san: FAILED" : "host_san: ok");
    return bad ? 1 : 0;
}
