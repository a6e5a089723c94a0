// bracket_check -- k_bracket_check (kt_adapt.hip), the device stopping test of
// the bracket columns, on synthetic sweep records against the
// host rule (kt_dense.cpp gauss_radau_sums) and the stop rule restated here.
// TEST INFRASTRUCTURE: built by __graft_entry__.build(), run by
// tests/test_gpu_bracket_check.py, which holds the printed figures to its
// tolerances.  One JSON line on stdout.
//
// Shapes: P = 16 with 16, 15 and 1 live columns at mcap = 256, and 16 live
// columns at mcap = 128; the columns past `live` and the columns seeded as
// stopped hold a sentinel state that must stay as it is.  Per shape two runs
// from a zeroed state:
//   run 0, rtol = 1e-10: depths 1 .. 16 consecutively, read back at 1, 2, 3, 5,
//     8, 12 and 16 -- the stop decisions;
//   run 1, rtol = -1 (no gap can satisfy it, so a column runs until a flag 1, 2
//     or the cap ends it): the depths around the launcher's switch from one
//     16-lane launch to 8-lane groups (24 (j + 1) 16 bytes pass 64 KB less the
//     static words after j = 168: depths 167 .. 170) and the last two depths,
//     mcap - 1 and mcap (flag 3), each read back.  The state carries no lag, so
//     a run may start at any depth; the columns that stop long before these
//     depths (kinds 1, 2) are seeded as the stopped columns they are by then.
// Column kinds by (lane + the shape's first kind) % 5, the Radau node mu per
// kind: 0 the path graph (alpha = 0, beta = 1; mu = 2.5: converges within a
// dozen steps), 1 a random tridiagonal with a breakdown at step 5 (flag 1),
// 2 alpha = 0, beta = 1.5 under mu = 2.5: theta_max = 3 cos(pi / (j + 1))
// passes mu at depth 5 (flag 2), 3 a spectrum of half-width ~300 under mu = 640
// (every term near exp's lower range, U_j made of one weight of ~1e-12 next to
// L_j ~ 1e-150; does not converge by depth 256), 4 a random tridiagonal of
// half-width ~32 under mu = 40.  One launch takes one mu,
// as a call has one lam_hi, so each kind's columns are checked in a launch
// sequence of their own record: a shape is run once per kind present, with the
// other kinds' columns seeded stopped.
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

static const double kSentinel = -12345.5;
static const double kMu[5] = {2.5, 2.5, 2.5, 640.0, 40.0};

// column `kind`: alpha[k], low[k] (= the off-diagonal below row k), k < mcap
static void make_column(int kind, int lane, int mcap, std::vector<double>& al, std::vector<double>& lo) {
    al.assign(mcap, 0.0);
    lo.assign(mcap, 1.0);
    if (kind == 1) {
        for (int k = 0; k < mcap; ++k) {
            al[k] = 0.3 * std::cos(0.7 * k + lane);
            lo[k] = 0.8 + 0.2 * std::sin(1.3 * k + 0.5 * lane);
        }
        lo[4] = 1e-12;
    }
    if (kind == 2) lo.assign(mcap, 1.5);
    if (kind == 3)
        for (int k = 0; k < mcap; ++k) {
            al[k] = 3.0 * std::cos(0.9 * k + lane);
            lo[k] = 150.0 + 2.0 * std::sin(0.4 * k);
        }
    if (kind == 4)
        for (int k = 0; k < mcap; ++k) {
            al[k] = 0.3 * std::cos(0.7 * k + lane);
            lo[k] = 16.0 + 0.5 * std::sin(1.3 * k + 0.5 * lane);
        }
}

// the stop rule on the host rule's sums
struct HostCol {
    const std::vector<double>*al = nullptr, *lo = nullptr;
    double mu = 0.0, l = 0.0, h = 0.0, margin = 1e300;
    int depth = 0, stopped = 0, flag = 0;
    void sums(int j, double* pl, double* ph, int* pf, double* scales = nullptr) const {
        *pf = kt::gauss_radau_sums(j, al->data(), lo->data(), (*lo)[j - 1], mu, pl, ph, scales);
    }
    void step(int j, int mcap, double rtol) {
        if (stopped) return;
        int f;
        sums(j, &l, &h, &f);
        if (f == 0) {
            margin = std::min(margin, std::fabs((h - l) - rtol * l) / l);
            f = (h - l <= rtol * l) ? 0 : (j == mcap ? 3 : -1);
        }
        if (f >= 0) {
            stopped = 1;
            depth = j;
            flag = f;
        }
    }
};

int main() {
    // P, mcap, live columns, the first lane's kind
    const int shapes[4][4] = {{16, 256, 16, 0}, {16, 256, 15, 3}, {16, 256, 1, 4}, {16, 128, 16, 2}};
    std::string out = "{\"cases\": [";
    bool first = true;
    for (int si = 0; si < 4; ++si) {
        const int P = shapes[si][0], mcap = shapes[si][1], live = shapes[si][2];
        std::vector<double> rec((size_t)3 * mcap * P, 0.0);
        std::vector<std::vector<double>> als(P), los(P);
        std::vector<int> kinds(P, 0);
        for (int c = 0; c < P; ++c) {
            kinds[c] = (c + shapes[si][3]) % 5;
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
        for (int kind = 0; kind < 5; ++kind) {
            bool present = false;
            for (int c = 0; c < live; ++c) present = present || kinds[c] == kind;
            if (!present) continue;
            const double mu = kMu[kind];
            for (int run = 0; run < 2; ++run) {
                if (run == 1 && (kind == 1 || kind == 2)) continue;  // stopped long before the deep depths
                const double rtol = run ? -1.0 : 1e-10;
                std::vector<int> depths, snaps;
                if (run == 0) {
                    for (int j = 1; j <= 16; ++j) depths.push_back(j);
                    snaps = {1, 2, 3, 5, 8, 12, 16};
                } else {
                    if (mcap > 170) depths = {167, 168, 169, 170};
                    depths.push_back(mcap - 1);
                    depths.push_back(mcap);
                    snaps = depths;
                }
                std::vector<double> st((size_t)P * kt::kAdaptState, 0.0);
                std::vector<HostCol> hc(P);
                std::vector<char> frozen(P, 0);  // columns whose state must stay as it starts
                for (int c = 0; c < P; ++c) {
                    double* s = &st[(size_t)c * kt::kAdaptState];
                    hc[c].al = &als[c];
                    hc[c].lo = &los[c];
                    hc[c].mu = mu;
                    if (c >= live) {
                        for (int q = 0; q < kt::kAdaptState; ++q) s[q] = kSentinel;
                        frozen[c] = 1;
                    } else if (kinds[c] != kind) {  // another launch sequence's column: stopped here
                        s[0] = s[1] = kSentinel;
                        s[3] = 2.0;
                        s[4] = 1.0;
                        frozen[c] = 1;
                    }
                }
                const std::vector<double> st0 = st;
                CK(hipMemcpy(dst, st.data(), st.size() * 8, hipMemcpyHostToDevice));
                CK(hipMemset(dact, 0xff, 4));
                for (int j : depths) {
                    CK(kt::launch_bracket_check(drec, mcap, P, j, live, mu, rtol, dst, dact, nullptr));
                    for (int c = 0; c < live; ++c)
                        if (!frozen[c]) hc[c].step(j, mcap, rtol);
                    if (std::find(snaps.begin(), snaps.end(), j) == snaps.end()) continue;
                    CK(hipDeviceSynchronize());
                    int act = -1;
                    CK(hipMemcpy(st.data(), dst, st.size() * 8, hipMemcpyDeviceToHost));
                    CK(hipMemcpy(&act, dact, 4, hipMemcpyDeviceToHost));
                    int untouched = 1, running = 0;
                    for (int c = 0; c < P; ++c) {
                        if (c < live && st[(size_t)c * kt::kAdaptState + 4] == 0.0) ++running;
                        if (frozen[c])
                            for (int q = 0; q < kt::kAdaptState; ++q)
                                if (st[(size_t)c * kt::kAdaptState + q] != st0[(size_t)c * kt::kAdaptState + q])
                                    untouched = 0;
                    }
                    char buf[800];
                    snprintf(buf, sizeof buf, "%s{\"P\": %d, \"mcap\": %d, \"j\": %d, \"live\": %d, \"kind\": %d, "
                             "\"run\": %d, \"rtol\": %.3e, \"active\": %d, \"running\": %d, \"untouched\": %d, "
                             "\"cols\": [", first ? "" : ", ", P, mcap, j, live, kind, run, rtol, act, running,
                             untouched);
                    out += buf;
                    first = false;
                    bool firstc = true;
                    for (int c = 0; c < live; ++c) {
                        if (frozen[c]) continue;
                        const double* s = &st[(size_t)c * kt::kAdaptState];
                        const HostCol& h = hc[c];
                        const int sd = s[4] != 0.0, dd = sd ? (int)s[3] : j;
                        // the host rule at the depth the device holds
                        double hl = 0.0, hh = 0.0, sc[2] = {0.0, 0.0};
                        int hf = 0;
                        if (dd >= 1 && dd <= mcap) h.sums(dd, &hl, &hh, &hf, sc);
                        auto fin = [](double v) { return std::isfinite(v) ? v : -1.0; };
                        snprintf(buf, sizeof buf,
                                 "%s{\"c\": %d, \"lo_dev\": %.17g, \"hi_dev\": %.17g, \"lo_host\": %.17g, "
                                 "\"hi_host\": %.17g, \"scale_lo\": %.17g, \"scale_hi\": %.17g, \"hi_nan_dev\": %d, \"hi_nan_host\": %d, \"stopped_dev\": %d, "
                                 "\"depth_dev\": %d, \"flag_dev\": %d, \"last_dev\": %d, \"stopped_host\": %d, "
                                 "\"depth_host\": %d, \"flag_host\": %d, \"margin\": %.6e}",
                                 firstc ? "" : ", ", c, fin(s[0]), fin(s[1]), fin(hl), fin(hh), sc[0], sc[1], (int)std::isnan(s[1]),
                                 (int)std::isnan(hh), sd, (int)s[3], (int)s[6], (int)s[7], h.stopped, h.depth, h.flag,
                                 std::min(h.margin, 1e300));
                        out += buf;
                        firstc = false;
                    }
                    out += "]}";
                }
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
