// chain_order_check -- kt_order.h's chained row order on the host, without a
// device (TEST INFRASTRUCTURE: tests/test_chain_order.py runs it).  For each
// graph: new2old is a bijection, degree classes are non-increasing along it,
// an equal input in other storage gives the same order, rows longer than
// long_thresh sit at their hub_order positions, the run property holds, and
// the order equals an independent implementation of the rule.
//
// The run property, read off the order alone: a short row at position p either
// is adjacent in the graph to the row at p - 1, of the same class, and has the
// smallest degree rank among that row's same-class neighbours at positions
// >= p (it continues the run); or the row at p - 1, the end of the run before
// it, has no same-class short neighbour at a position >= p (the run stopped
// because nothing eligible was left), and the row is the earliest in the base
// order among the rows at positions >= p (runs start along the base order).
//
// Prints one JSON line; exit status 0 when every check holds.
//   chain_order_check            the checks
//   chain_order_check time N D   seconds of one chain_order call, and of one
//                                hub_order call, on a random graph of N rows,
//                                D entries per row on average
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "kt_order.h"

namespace {

struct Graph {
    std::string name;
    int64_t n = 0;
    std::vector<int64_t> rp;
    std::vector<int32_t> col;
};

uint64_t g_state = 0x13198A2E03707344ULL;
uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

Graph from_edges(const std::string& name, int64_t n, std::vector<std::pair<int32_t, int32_t>> e) {
    const size_t m = e.size();
    for (size_t i = 0; i < m; ++i)
        if (e[i].first != e[i].second) e.push_back({e[i].second, e[i].first});
    std::sort(e.begin(), e.end());
    e.erase(std::unique(e.begin(), e.end()), e.end());
    Graph g;
    g.name = name;
    g.n = n;
    g.rp.assign((size_t)n + 1, 0);
    for (auto& x : e) g.rp[(size_t)x.first + 1]++;
    for (int64_t i = 0; i < n; ++i) g.rp[(size_t)i + 1] += g.rp[(size_t)i];
    for (auto& x : e) g.col.push_back(x.second);
    return g;
}

// endpoints drawn with probability ~ (i + 1)^-0.5: a heavy tail with hubs past
// every threshold (long rows, more than kOrderHubRanks rows above the tail)
Graph heavy_tail(const std::string& name, int64_t n, int64_t edges, bool loops) {
    std::vector<double> cum((size_t)n);
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) cum[(size_t)i] = (s += 1.0 / std::sqrt((double)(i + 1)));
    auto draw = [&]() {
        const double u = (double)(rnd() >> 11) / 9007199254740992.0 * s;
        const int64_t i = std::lower_bound(cum.begin(), cum.end(), u) - cum.begin();
        // scatter the labels so that degree and index are unrelated
        return (int32_t)(((uint64_t)std::min(i, n - 1) * 7919u + 13u) % (uint64_t)n);
    };
    std::vector<std::pair<int32_t, int32_t>> e;
    for (int64_t k = 0; k < edges; ++k) {
        const int32_t a = draw(), b = draw();
        if (a != b || loops) e.push_back({a, b});
    }
    return from_edges(name, n, e);
}

// The rule, written from its statement: ranks from a comparison sort, the
// candidates of each step collected and the least taken, placement kept as
// positions.
std::vector<int32_t> reference_order(const Graph& g, int long_thresh, const std::vector<int32_t>& base) {
    const int64_t n = g.n;
    auto deg = [&](int64_t i) { return g.rp[(size_t)i + 1] - g.rp[(size_t)i]; };
    std::vector<int32_t> byd((size_t)n), rank((size_t)n);
    for (int64_t i = 0; i < n; ++i) byd[(size_t)i] = (int32_t)i;
    std::stable_sort(byd.begin(), byd.end(), [&](int32_t x, int32_t y) { return deg(x) > deg(y); });
    for (int64_t r = 0; r < n; ++r) rank[(size_t)byd[(size_t)r]] = (int32_t)r;
    std::vector<int64_t> pos((size_t)n, -1);
    std::vector<int32_t> out;
    for (int64_t b = 0; b < n; ++b) {
        int32_t row = base[(size_t)b];
        if (pos[(size_t)row] >= 0) continue;
        while (row >= 0) {
            pos[(size_t)row] = (int64_t)out.size();
            out.push_back(row);
            if (deg(row) > long_thresh) break;
            std::vector<std::pair<int32_t, int32_t>> cand;  // (rank, row)
            for (int64_t k = g.rp[(size_t)row]; k < g.rp[(size_t)row + 1]; ++k) {
                const int32_t c = g.col[(size_t)k];
                if (c != row && pos[(size_t)c] < 0 && deg(c) <= long_thresh &&
                    kt::order_class(deg(c), long_thresh) == kt::order_class(deg(row), long_thresh))
                    cand.push_back({rank[(size_t)c], c});
            }
            row = cand.empty() ? -1 : std::min_element(cand.begin(), cand.end())->second;
        }
    }
    return out;
}

bool check(const Graph& g, int long_thresh, std::string& why, int64_t& chained) {
    const int64_t n = g.n;
    std::vector<int32_t> a, b, base;
    kt::chain_order(n, g.rp.data(), g.col.data(), long_thresh, a);
    const Graph copy = g;  // equal input in other storage
    kt::chain_order(n, copy.rp.data(), copy.col.data(), long_thresh, b);
    if (a != b) return why = "two runs differ", false;
    if ((int64_t)a.size() != n) return why = "wrong length", false;
    std::vector<int64_t> pos((size_t)n, -1);
    for (int64_t r = 0; r < n; ++r) {
        const int32_t v = a[(size_t)r];
        if (v < 0 || v >= n || pos[(size_t)v] >= 0) return why = "not a bijection", false;
        pos[(size_t)v] = r;
    }
    auto deg = [&](int64_t i) { return g.rp[(size_t)i + 1] - g.rp[(size_t)i]; };
    auto cls = [&](int64_t i) { return kt::order_class(deg(i), long_thresh); };
    for (int64_t r = 1; r < n; ++r)
        if (cls(a[(size_t)r - 1]) < cls(a[(size_t)r])) return why = "degree class increases", false;
    kt::hub_order(n, g.rp.data(), g.col.data(), long_thresh, base);
    std::vector<int64_t> bpos((size_t)n);
    for (int64_t r = 0; r < n; ++r) bpos[(size_t)base[(size_t)r]] = r;
    for (int64_t r = 0; r < n; ++r)
        if (deg(base[(size_t)r]) > long_thresh && a[(size_t)r] != base[(size_t)r])
            return why = "a long row left its hub_order position", false;
    // the run property (see the head of this file)
    std::vector<int32_t> rank((size_t)n), byd((size_t)n);
    for (int64_t i = 0; i < n; ++i) byd[(size_t)i] = (int32_t)i;
    std::stable_sort(byd.begin(), byd.end(), [&](int32_t x, int32_t y) { return deg(x) > deg(y); });
    for (int64_t r = 0; r < n; ++r) rank[(size_t)byd[(size_t)r]] = (int32_t)r;
    // sufmin[p] = the least base position among the rows at positions >= p
    std::vector<int64_t> sufmin((size_t)n + 1, n);
    for (int64_t p = n - 1; p >= 0; --p) sufmin[(size_t)p] = std::min(sufmin[(size_t)p + 1], bpos[(size_t)a[(size_t)p]]);
    chained = 0;
    for (int64_t p = 0; p < n; ++p) {
        const int32_t row = a[(size_t)p];
        if (deg(row) > long_thresh) continue;
        // what the row before had left when this one was placed
        int32_t least = -1;
        bool adjacent = false;
        if (p > 0 && deg(a[(size_t)p - 1]) <= long_thresh) {
            const int32_t prev = a[(size_t)p - 1];
            for (int64_t k = g.rp[(size_t)prev]; k < g.rp[(size_t)prev + 1]; ++k) {
                const int32_t c = g.col[(size_t)k];
                if (c == prev || pos[(size_t)c] < p || deg(c) > long_thresh || cls(c) != cls(prev)) continue;
                if (c == row) adjacent = true;
                if (least < 0 || rank[(size_t)c] < rank[(size_t)least]) least = c;
            }
        }
        if (adjacent) {
            if (least != row) return why = "a run did not take the neighbour of smallest degree rank", false;
            ++chained;
        } else {
            if (least >= 0) return why = "a run stopped with an eligible neighbour left", false;
            if (bpos[(size_t)row] != sufmin[(size_t)p]) return why = "a run did not start along the base order", false;
        }
    }
    if (a != reference_order(g, long_thresh, base)) return why = "differs from the independent implementation", false;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "time")) {
        const int64_t n = std::atoll(argv[2]), d = std::atoll(argv[3]);
        const Graph g = heavy_tail("time", n, n * d / 2, false);
        std::vector<int32_t> o;
        double chain = 1e30, hub = 1e30;
        for (int rep = 0; rep < 3; ++rep) {
            auto t0 = std::chrono::steady_clock::now();
            kt::chain_order(n, g.rp.data(), g.col.data(), 64, o);
            chain = std::min(chain, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
            t0 = std::chrono::steady_clock::now();
            kt::hub_order(n, g.rp.data(), g.col.data(), 64, o);
            hub = std::min(hub, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        std::printf("{\"n\": %lld, \"nnz\": %lld, \"chain_order_seconds\": %.4f, \"hub_order_seconds\": %.4f}\n",
                    (long long)n, (long long)g.col.size(), chain, hub);
        return 0;
    }
    std::vector<Graph> gs;
    gs.push_back(heavy_tail("heavy_tail_20k", 20000, 150000, false));
    gs.push_back(heavy_tail("heavy_tail_loops_6k", 6000, 40000, true));
    {
        std::vector<std::pair<int32_t, int32_t>> e;
        for (int32_t i = 1; i < 300; ++i) e.push_back({0, i});
        gs.push_back(from_edges("star_300", 300, e));
        e.clear();
        for (int32_t i = 1; i < 301; ++i) e.push_back({i - 1, i});
        gs.push_back(from_edges("path_301", 301, e));
        e.clear();
        // labels scattered along the cycle, chords of two lengths on part of it
        for (int32_t i = 0; i < 211; ++i) e.push_back({(int32_t)(i * 89 % 211), (int32_t)((i + 1) * 89 % 211)});
        for (int32_t i = 0; i < 211; i += 3) e.push_back({i, (i + 40) % 211});
        for (int32_t i = 0; i < 100; i += 5) e.push_back({i, (i + 17) % 211});
        gs.push_back(from_edges("cycle_chords_211", 211, e));
        e.clear();
        for (int32_t i = 0; i < 100; i += 2) e.push_back({i, (i + 7) % 100});
        gs.push_back(from_edges("isolated_rows_257", 257, e));  // rows 100.. have degree 0
        gs.push_back(from_edges("empty_0", 0, {}));
        gs.push_back(from_edges("single_1", 1, {}));
    }
    int failed = 0;
    std::string out = "{\"graphs\": [";
    for (size_t i = 0; i < gs.size(); ++i) {
        for (int lt : {64, 8}) {
            std::string why = "ok";
            int64_t chained = 0;
            if (!check(gs[i], lt, why, chained)) ++failed;
            int64_t n_long = 0;
            for (int64_t r = 0; r < gs[i].n; ++r) n_long += gs[i].rp[(size_t)r + 1] - gs[i].rp[(size_t)r] > lt;
            out += std::string(i || lt != 64 ? ", " : "") + "{\"name\": \"" + gs[i].name +
                   "\", \"long_thresh\": " + std::to_string(lt) + ", \"n\": " + std::to_string(gs[i].n) +
                   ", \"nnz\": " + std::to_string(gs[i].col.size()) + ", \"long_rows\": " + std::to_string(n_long) +
                   ", \"chained\": " + std::to_string(chained) + ", \"result\": \"" + why + "\"}";
        }
    }
    out += "], \"failed\": " + std::to_string(failed) + "}";
    std::printf("%s\n", out.c_str());
    return failed ? 1 : 0;
}
