// node_check -- k_node_check (kt_adapt.hip), the device stopping test of the
// node-removal columns, on synthetic sweep records against
// the host value function (kt_dense.cpp node_update_value) and the lag-2 rule
// of trace_fun_update.m:104-124 restated here.  TEST INFRASTRUCTURE: built by
// __graft_entry__.build(), run by tests/test_gpu_node_check.py, which holds the
// printed figures to its tolerances.  One JSON line on stdout.
//
// Shapes: P in {1, 4, 16} x mcap in {128, 256}, and P = 16 with 5 live columns
// over a sentinel-filled state.  Per shape one run from a zeroed state through
// depths 1 .. 16, read back at 1, 2, 3, 8 and 16, and one run for each of the
// depths j = 31, 32 and mcap: the state is seeded with the host rule's state
// after depth j - 3 and the checks of j - 2, j - 1, j follow, as a sweep
// queues them (a QL of depth 256 on one lane takes milliseconds; running every
// depth up to it would take the suite half a minute).  P = 16 takes the
// launcher's 8-lane groups from depth 128 and its 4-lane groups at depth 256.
// Column kinds by (lane + the shape's first kind) % 6: 0 ordinary (converges
// within a dozen steps), 1 beta_1 = 0 (stops at depth 1, lucky), 2 a breakdown
// at step 5, 3 already stopped (its state must stay as it is), 4 a spectrum
// reaching ~690 (fun = exp stays finite; never converges at this tol), 5 a
// spectrum of width ~65 (X ~ 1e14, whose rounding noise alone is far above
// this tol, so the deep depths are checked on a running column at an ordinary
// scale).  A seeded run seeds kinds 0, 4 and 5 as running with the pair
// (X_{j-4}, X_{j-3}) -- kind 0 then meets the rule's stop at depth j - 2 -- and
// kinds 1 and 2 as the stopped columns they are by then.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "kt_internal.h"
#include "kt_launch.h"

namespace kt {
void set_error(const std::string&) {}  // kt_dense.o's ABI edge; unused here
}

#define CK(x)                                                                         \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            printf("{\"hip_error\": \"%s: %s\"}\n", #x, hipGetErrorString(e_));       \
            return 2;                                                                 \
        }                                                                             \
    } while (0)

static const double kTol = 1e-9;
static const double kSentinel = -12345.5;

// column `kind`: alpha[k], low[k] (= the off-diagonal below row k), k < mcap
static void make_column(int kind, int lane, int mcap, std::vector<double>& al, std::vector<double>& lo) {
    al.assign(mcap, 0.0);
    lo.assign(mcap, 0.0);
    for (int k = 0; k < mcap; ++k) {
        al[k] = 0.3 * std::cos(0.7 * k + lane);
        lo[k] = 1.0 + 0.3 * std::sin(1.3 * k + 0.5 * lane);
    }
    if (kind == 1) lo[0] = 0.0;
    if (kind == 2) lo[4] = 1e-12;
    if (kind == 4)
        for (int k = 0; k < mcap; ++k) {
            al[k] = 380.0 + 3.0 * std::cos(0.9 * k + lane);
            lo[k] = 150.0 + 2.0 * std::sin(0.4 * k);
        }
    if (kind == 5)
        for (int k = 0; k < mcap; ++k) lo[k] = 16.0 + 0.5 * std::sin(1.3 * k + 0.5 * lane);
}

// one column on the host: its values by depth and the rule's state
struct HostCol {
    const std::vector<double>*al = nullptr, *lo = nullptr;
    std::vector<double> x, scale, tm;  // X_k, sum |f(eig(T_k))|, theta_max at index k (1-based)
    std::vector<char> have;
    double xstop[2] = {0.0, 0.0};
    int depth = 0, stopped = 0, lucky = 0;
    void value(int k) {
        if ((int)have.size() <= k) {
            x.resize(k + 1, 0.0);
            scale.resize(k + 1, 0.0);
            tm.resize(k + 1, 0.0);
            have.resize(k + 1, 0);
        }
        if (have[k]) return;
        x[k] = kt::node_update_value(k, al->data(), lo->data(), KT_FUN_EXP, &scale[k], &tm[k]);
        have[k] = 1;
    }
    void step(int k) {
        if (stopped) return;
        value(k);
        bool stop = false;
        if (k <= 2) {
            xstop[k - 1] = x[k];
        } else if (std::fabs(x[k] - xstop[0]) < kTol) {
            stop = true;
        } else {
            xstop[0] = xstop[1];
            xstop[1] = x[k];
        }
        const bool lk = (*lo)[k - 1] < 1e-8;
        if (!stop && lk) stop = true;
        if (stop) {
            stopped = 1;
            depth = k;
            lucky = lk ? 1 : 0;
        }
    }
};

int main() {
    // P, mcap, live columns, the first lane's kind
    const int shapes[7][4] = {{1, 128, 1, 5}, {4, 128, 4, 0}, {16, 128, 16, 2}, {1, 256, 1, 4},
                              {4, 256, 4, 2}, {16, 256, 16, 0}, {16, 128, 5, 1}};
    std::string out = "{\"tol\": 1e-9, \"cases\": [";
    bool first = true;
    for (int si = 0; si < 7; ++si) {
        const int P = shapes[si][0], mcap = shapes[si][1], live = shapes[si][2];
        const bool sentinel_case = live < P;
        std::vector<double> rec((size_t)3 * mcap * P, 0.0);
        std::vector<std::vector<double>> als(P), los(P);
        std::vector<int> kinds(P, 0);
        for (int c = 0; c < P; ++c) {
            kinds[c] = (c + shapes[si][3]) % 6;
            make_column(kinds[c], c, mcap, als[c], los[c]);
            for (int k = 0; k < mcap; ++k) {
                rec[(size_t)(0 * mcap + k) * P + c] = als[c][k];
                rec[(size_t)(2 * mcap + k) * P + c] = los[c][k];
                if (k + 1 < mcap) rec[(size_t)(1 * mcap + k + 1) * P + c] = los[c][k];  // up[k+1] = low[k]
            }
        }
        double *drec, *dst;
        int* dact;
        CK(hipMalloc(&drec, rec.size() * 8));
        CK(hipMalloc(&dst, (size_t)P * kt::kAdaptState * 8));
        CK(hipMalloc(&dact, 4));
        CK(hipMemcpy(drec, rec.data(), rec.size() * 8, hipMemcpyHostToDevice));
        // run 0: depths 1 .. 16 from a zeroed state; runs 1 .. 3: seeded at j - 3, depths j - 2 .. j
        const int ends[4] = {16, 31, 32, mcap};
        for (int run = 0; run < 4; ++run) {
            const int j1 = ends[run], j0 = run ? j1 - 2 : 1, seed = j0 - 1;
            std::vector<double> st((size_t)P * kt::kAdaptState, 0.0);
            std::vector<HostCol> hc(P);
            std::vector<char> frozen(P, 0);  // columns whose state must stay as it starts
            for (int c = 0; c < P; ++c) {
                double* s = &st[(size_t)c * kt::kAdaptState];
                HostCol& h = hc[c];
                h.al = &als[c];
                h.lo = &los[c];
                if (c >= live) {
                    for (int q = 0; q < kt::kAdaptState; ++q) s[q] = kSentinel;
                    frozen[c] = 1;
                } else if (kinds[c] == 3) {  // stopped before this sweep's first check
                    s[0] = kSentinel;
                    s[3] = 2.0;
                    s[4] = 1.0;
                    frozen[c] = 1;
                } else if (run && (kinds[c] == 1 || kinds[c] == 2)) {  // stopped long before the seed depth
                    const int d = kinds[c] == 1 ? 1 : 5;
                    h.value(d);
                    h.stopped = h.lucky = 1;
                    h.depth = d;
                    s[0] = h.x[d] * std::exp(-h.tm[d]);
                    s[3] = (double)d;
                    s[4] = s[6] = 1.0;
                    s[5] = h.tm[d];
                    s[7] = (double)d;
                    frozen[c] = 1;
                } else if (run) {  // running, the stored pair (X_{seed-1}, X_seed)
                    h.value(seed - 1);
                    h.value(seed);
                    h.xstop[0] = h.x[seed - 1];
                    h.xstop[1] = h.x[seed];
                    const double sc = std::exp(-h.tm[seed]);
                    s[0] = s[2] = h.x[seed] * sc;
                    s[1] = h.x[seed - 1] * sc;
                    s[5] = h.tm[seed];
                    s[7] = (double)seed;
                }
            }
            const std::vector<double> st0 = st;
            CK(hipMemcpy(dst, st.data(), st.size() * 8, hipMemcpyHostToDevice));
            CK(hipMemset(dact, 0xff, 4));
            for (int j = j0; j <= j1; ++j) {
                CK(kt::launch_node_check(drec, mcap, P, j, live, KT_FUN_EXP, kTol, dst, dact, nullptr));
                for (int c = 0; c < live; ++c)
                    if (!frozen[c]) hc[c].step(j);
                const bool snap = run ? j == j1 : (j == 1 || j == 2 || j == 3 || j == 8 || j == 16);
                if (!snap) continue;
                CK(hipDeviceSynchronize());
                int act = -1;
                CK(hipMemcpy(st.data(), dst, st.size() * 8, hipMemcpyDeviceToHost));
                CK(hipMemcpy(&act, dact, 4, hipMemcpyDeviceToHost));
                int untouched = 1;
                for (int c = 0; c < P; ++c)
                    if (frozen[c])
                        for (int q = 0; q < kt::kAdaptState; ++q)
                            if (st[(size_t)c * kt::kAdaptState + q] != st0[(size_t)c * kt::kAdaptState + q])
                                untouched = 0;
                char buf[640];
                snprintf(buf, sizeof buf, "%s{\"P\": %d, \"mcap\": %d, \"j\": %d, \"live\": %d, \"sentinel\": %d, "
                         "\"seeded\": %d, \"active\": %d, \"untouched\": %d, \"cols\": [", first ? "" : ", ", P, mcap,
                         j, live, (int)sentinel_case, run ? 1 : 0, act, untouched);
                out += buf;
                first = false;
                for (int c = 0; c < live; ++c) {
                    const double* s = &st[(size_t)c * kt::kAdaptState];
                    HostCol& h = hc[c];
                    const int sd = s[4] != 0.0, dd = sd ? (int)s[3] : j;
                    double xh = 0.0, sc = 1.0, margin = 1e300;
                    if (kinds[c] != 3) {
                        // the host's value at the depth the device holds, and how close
                        // any decision of this run up to there came to the threshold
                        const int upto = std::min(j, std::max(dd, h.stopped ? h.depth : j));
                        if (!frozen[c])
                            for (int k = std::max(3, j0); k <= upto; ++k) {
                                h.value(k);
                                h.value(k - 2);
                                margin = std::min(margin, std::fabs(std::fabs(h.x[k] - h.x[k - 2]) - kTol) / h.scale[k]);
                            }
                        h.value(dd);
                        xh = h.x[dd];
                        sc = h.scale[dd];
                    }
                    auto fin = [](double v) { return std::isfinite(v) ? v : 1e300; };
                    snprintf(buf, sizeof buf,
                             "%s{\"c\": %d, \"kind\": %d, \"x_dev\": %.17g, \"x_host\": %.17g, \"scale\": %.17g, "
                             "\"theta\": %.17g, \"stopped_dev\": %d, \"depth_dev\": %d, \"lucky_dev\": %d, "
                             "\"stopped_host\": %d, \"depth_host\": %d, \"lucky_host\": %d, \"margin\": %.6e}",
                             c ? ", " : "", c, kinds[c], fin(s[0] * std::exp(s[5])), fin(xh), fin(sc), s[5], sd,
                             (int)s[3], (int)s[6], h.stopped, h.depth, h.lucky, fin(margin));
                    out += buf;
                }
                out += "]}";
            }
        }
        CK(hipFree(drec));
        CK(hipFree(dst));
        CK(hipFree(dact));
    }
    out += "]}";
    printf("%s\n", out.c_str());
    return 0;
}
