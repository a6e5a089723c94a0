// hub_order_check -- kt_order.h's row order on the host, without a device
// (TEST INFRASTRUCTURE: tests/test_hub_order.py runs it).  For each graph:
// new2old is a bijection, degree classes are non-increasing along it, equal
// inputs give equal orders, and the order equals an independent comparison
// sort by (class descending, neighbour key ascending, original index).
// Prints one JSON line; exit status 0 when every check holds.
//   hub_order_check            the checks
//   hub_order_check time N D   seconds of one hub_order call on a random graph
//                              of N rows, D entries per row on average
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

uint64_t g_state = 0x243F6A8885A308D3ULL;
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

bool check(const Graph& g, int long_thresh, std::string& why) {
    const int64_t n = g.n;
    std::vector<int32_t> a, b;
    kt::hub_order(n, g.rp.data(), g.col.data(), long_thresh, a);
    const Graph copy = g;  // equal input in other storage
    kt::hub_order(n, copy.rp.data(), copy.col.data(), long_thresh, b);
    if (a != b) return why = "two runs differ", false;
    if ((int64_t)a.size() != n) return why = "wrong length", false;
    std::vector<char> seen((size_t)n, 0);
    for (int32_t v : a) {
        if (v < 0 || v >= n || seen[(size_t)v]) return why = "not a bijection", false;
        seen[(size_t)v] = 1;
    }
    auto deg = [&](int64_t i) { return g.rp[(size_t)i + 1] - g.rp[(size_t)i]; };
    for (int64_t r = 1; r < n; ++r)
        if (kt::order_class(deg(a[(size_t)r - 1]), long_thresh) < kt::order_class(deg(a[(size_t)r]), long_thresh))
            return why = "degree class increases", false;
    // the independent order
    std::vector<int32_t> byd((size_t)n), rank((size_t)n), ref((size_t)n);
    std::vector<int64_t> prim((size_t)n);
    for (int64_t i = 0; i < n; ++i) byd[(size_t)i] = ref[(size_t)i] = (int32_t)i;
    std::stable_sort(byd.begin(), byd.end(), [&](int32_t x, int32_t y) { return deg(x) > deg(y); });
    for (int64_t r = 0; r < n; ++r) rank[(size_t)byd[(size_t)r]] = (int32_t)r;
    for (int64_t i = 0; i < n; ++i) {
        int64_t p = n;
        for (int64_t k = g.rp[(size_t)i]; k < g.rp[(size_t)i + 1]; ++k) {
            const int64_t rc = rank[(size_t)g.col[(size_t)k]];
            if (rc >= kt::kOrderHubRanks) p = std::min(p, rc);
        }
        prim[(size_t)i] = p;
    }
    std::sort(ref.begin(), ref.end(), [&](int32_t x, int32_t y) {
        const int64_t cx = kt::order_class(deg(x), long_thresh), cy = kt::order_class(deg(y), long_thresh);
        if (cx != cy) return cx > cy;
        if (prim[(size_t)x] != prim[(size_t)y]) return prim[(size_t)x] < prim[(size_t)y];
        return x < y;
    });
    if (a != ref) return why = "differs from the comparison sort", false;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "time")) {
        const int64_t n = std::atoll(argv[2]), d = std::atoll(argv[3]);
        const Graph g = heavy_tail("time", n, n * d / 2, false);
        std::vector<int32_t> o;
        double best = 1e30;
        for (int rep = 0; rep < 3; ++rep) {
            const auto t0 = std::chrono::steady_clock::now();
            kt::hub_order(n, g.rp.data(), g.col.data(), 64, o);
            best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        // the order it replaced: a stable comparison sort by degree alone
        double plain = 1e30;
        for (int rep = 0; rep < 3; ++rep) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int64_t i = 0; i < n; ++i) o[(size_t)i] = (int32_t)i;
            std::stable_sort(o.begin(), o.end(), [&](int32_t x, int32_t y) {
                return g.rp[(size_t)x + 1] - g.rp[(size_t)x] > g.rp[(size_t)y + 1] - g.rp[(size_t)y];
            });
            plain = std::min(plain, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        std::printf("{\"n\": %lld, \"nnz\": %lld, \"hub_order_seconds\": %.4f, \"degree_sort_seconds\": %.4f}\n",
                    (long long)n, (long long)g.col.size(), best, plain);
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
        for (int32_t i = 0; i < 100; i += 2) e.push_back({i, (i + 7) % 100});
        gs.push_back(from_edges("isolated_rows_257", 257, e));  // rows 100.. have degree 0
        gs.push_back(from_edges("empty_5", 5, {}));
        gs.push_back(from_edges("single_1", 1, {}));
    }
    int failed = 0;
    std::string out = "{\"graphs\": [";
    for (size_t i = 0; i < gs.size(); ++i) {
        for (int lt : {64, 8}) {
            std::string why = "ok";
            if (!check(gs[i], lt, why)) ++failed;
            out += std::string(i || lt != 64 ? ", " : "") + "{\"name\": \"" + gs[i].name +
                   "\", \"long_thresh\": " + std::to_string(lt) + ", \"n\": " + std::to_string(gs[i].n) +
                   ", \"nnz\": " + std::to_string(gs[i].col.size()) + ", \"result\": \"" + why + "\"}";
        }
    }
    out += "], \"failed\": " + std::to_string(failed) + "}";
    std::printf("%s\n", out.c_str());
    return failed ? 1 : 0;
}
