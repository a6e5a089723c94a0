// host_san -- TEST INFRASTRUCTURE: the host-only parts of kt_miobi_break_node's
// driver (kt_miobi_host.h: the diagonal scan, the window length, the
// removed-entry count, the long-row list and the row / column removal) on a
// 200-node graph against brute-force loops; built by `make host_san` with
// -fsanitize=address,undefined and run on the CPU.  Exit status 0: all agree.
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

static void to_csr(int n, const std::vector<char>& D, std::vector<int64_t>& rowptr, std::vector<int32_t>& col) {
    rowptr.assign((size_t)n + 1, 0);
    col.clear();
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j)
            if (D[(size_t)i * n + j]) col.push_back(j);
        rowptr[(size_t)i + 1] = (int64_t)col.size();
    }
}

int main() {
    const int n = 200;
    // a symmetric 0/1 graph with a hub (node 17, the last node too) and isolated nodes; dense copy for the brute force
    std::vector<char> D((size_t)n * n, 0);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (i % 41 != 3 && j % 41 != 3 && (i == 17 || j == 17 || j == n - 1 ? rnd() % 2 == 0 : rnd() % 40 == 0))
                D[(size_t)i * n + j] = D[(size_t)j * n + i] = 1;
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col;
    to_csr(n, D, rowptr, col);
    int bad = 0;

    bad += check(!kt::miobi_has_diagonal(n, rowptr.data(), col.data()), "miobi_has_diagonal on a zero diagonal");
    for (int d : {0, 77, n - 1}) {
        std::vector<char> E = D;
        E[(size_t)d * n + d] = 1;
        std::vector<int64_t> rp;
        std::vector<int32_t> cl;
        to_csr(n, E, rp, cl);
        bad += check(kt::miobi_has_diagonal(n, rp.data(), cl.data()), "miobi_has_diagonal finds the entry");
    }

    bad += check(kt::miobi_node_window(100, 50) == 25 && kt::miobi_node_window(100, 49) == 25 &&
                     kt::miobi_node_window(7, 50) == 7 && kt::miobi_node_window(100, 1) == 1 &&
                     kt::miobi_node_window(100, 0) == 100 && kt::miobi_node_window(100, -3) == 100,
                 "miobi_node_window");

    // the count: degrees 30, 30, 2, 1 with refresh 50 -> ends at steps 1 and 2, carries 10, 20, then 24, 26
    {
        int acc = 0;
        const int degs[] = {30, 30, 2, 1}, carry[] = {10, 20, 24, 26};
        const bool ends[] = {true, true, false, false};
        bool ok = true;
        for (int s = 0; s < 4; ++s) ok = ok && kt::miobi_node_book(acc, degs[s], 50) == ends[s] && acc == carry[s];
        int big = 49;
        ok = ok && kt::miobi_node_book(big, 2147483647, 50) && big == (int)((49 + 2LL * 2147483647) % 50);
        int off = 5;
        ok = ok && !kt::miobi_node_book(off, 1000, 0) && off == 5;
        // a window of miobi_node_window steps always reaches its end with degrees >= 1
        for (int refresh : {1, 2, 3, 49, 50, 51}) {
            int a = refresh - 1, steps = 0;
            bool ended = false;
            while (!ended) ended = kt::miobi_node_book(a, 1, refresh), ++steps;
            ok = ok && steps <= kt::miobi_node_window(1000, refresh);
            a = 0, steps = 0, ended = false;
            while (!ended) ended = kt::miobi_node_book(a, 1, refresh), ++steps;
            ok = ok && steps == kt::miobi_node_window(1000, refresh);
        }
        bad += check(ok, "miobi_node_book");
    }

    for (int thresh : {0, 5, 90, 1000}) {
        std::vector<int> rows;
        kt::miobi_long_rows(n, rowptr.data(), thresh, rows);
        std::vector<int> brute;
        for (int i = 0; i < n; ++i) {
            int d = 0;
            for (int j = 0; j < n; ++j) d += D[(size_t)i * n + j];
            if (d > thresh) brute.push_back(i);
        }
        bad += check(rows == brute, "miobi_long_rows against the dense degrees");
    }

    // removal: none, the hub, the first and last node, a few at once, an isolated node, all; with and without values
    const std::vector<std::vector<int>> sets = {{}, {17}, {0, n - 1}, {17, 18, 60, 61, 199}, {3}, {}};
    for (size_t q = 0; q < sets.size(); ++q)
        for (int with_val = 0; with_val < 2; ++with_val) {
            std::vector<unsigned char> dead((size_t)n, q + 1 == sets.size() ? 1 : 0);
            for (int r : sets[q]) dead[(size_t)r] = 1;
            std::vector<int64_t> rp = rowptr;
            std::vector<int32_t> cl = col;
            std::vector<double> vl;
            if (with_val) vl.assign(col.size(), 1.0);
            const int64_t removed = kt::miobi_clear_nodes(n, dead, rp, cl, vl);
            std::vector<char> E = D;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                    if (dead[(size_t)i] || dead[(size_t)j]) E[(size_t)i * n + j] = 0;
            std::vector<int64_t> rp2;
            std::vector<int32_t> cl2;
            to_csr(n, E, rp2, cl2);
            bool ok = rp == rp2 && cl == cl2 && removed == (int64_t)col.size() - (int64_t)cl2.size() &&
                      vl.size() == (with_val ? cl2.size() : 0);
            for (double x : vl) ok = ok && x == 1.0;
            bad += check(ok, "miobi_clear_nodes against the dense matrix");
        }
    printf("%s\n", bad ? "host_san: FAILED" : "host_san: ok");
    return bad ? 1 : 0;
}
