// pair_bracket_check -- k_pair_bracket_check (kt_adapt.hip), the device stopping
// test of the pair columns, on synthetic sweep records against
// the host rule (kt_dense.cpp gauss_radau_sums, pair_bracket_combine) driven by
// the stop rule restated here.  TEST INFRASTRUCTURE: built by
// __graft_entry__.build(), run by tests/test_gpu_pair_bracket_check.py, which
// holds the printed figures to its tolerances.  `pair_bracket_check TOL`: one
// JSON line on stdout; a pair is "robust" while none of the decisions taken on
// it changes when lo and hi move by TOL times the unit of the sums' errors (sum
// exp(theta_k - mu) over the eigenvalues the four sums take).  With --host
// behind TOL it prints the host rule's decisions alone and touches no device.
//
// Shapes: P = 16 with 16, 14 and 2 live columns at mcap = 256, and 16 live
// columns at mcap = 128; the columns past `live` and the pairs seeded as decided
// hold a sentinel state that must stay as it is.  mu = 2.5 throughout.  Per
// shape two runs:
//   run 0, rtol = 1e-6, ftol = 1e-9 (both far above the sums' rounding, so that
//     the decisions are comparable): depths 1 .. 16 consecutively from a zeroed
//     state, read back at 1, 2, 3, 4, 5, 6, 8, 12 and 16 -- the stop decisions;
//   run 1, rtol = ftol = -1 (no gap can satisfy either, so a pair runs until a
//     flag 1, 2 or the cap ends it): the depths around the launcher's switch
//     from one 16-lane launch to 8-lane groups (167 .. 170) and the last two
//     depths, mcap - 1 and mcap (flag 3), each read back.  The state carries no
//     lag, so a run may start at any depth: the pairs decided long before
//     (kinds 2, 3) are seeded decided, and kind 1's frozen column as the frozen
//     column it is by then.
// Pair kinds by (pair + the shape's first kind) % 5, columns (+, -):
//   0 both running, a closing bracket: the path graphs alpha = 0, beta = 1 and
//     beta = 0.5 (flag 0 within a dozen steps);
//   1 the path graph and a random tridiagonal that breaks down at step 3: the
//     - column is frozen there, the + column runs on until the pair's flag 0;
//   2 both broken: random tridiagonals with breakdowns at steps 3 (+) and 5 (-),
//     flag 1 at depth 5;
//   3 mu too small: alpha = 0, beta = 1.5, whose theta_max = 3 cos(pi / (j + 1))
//     passes mu at depth 5 (flag 2), beside the path graph;
//   4 the floor: the same path graph in both columns -- the entry is 0, lo =
//     -hi, never of one sign, and the pair stops by flag 4.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static const double kMu = 2.5;

// column `c` of pair kind `kind`: alpha[k], low[k] (= the off-diagonal below row k)
static void make_column(int kind, int c, int mcap, std::vector<double>& al, std::vector<double>& lo) {
    const int minus = c & 1;
    al.assign(mcap, 0.0);
    lo.assign(mcap, 1.0);
    const bool random = (kind == 1 && minus) || kind == 2;
    if (random) {
        for (int k = 0; k < mcap; ++k) {
            al[k] = 0.3 * std::cos(0.7 * k + c);
            lo[k] = 0.8 + 0.2 * std::sin(1.3 * k + 0.5 * c);
        }
        lo[(kind == 2 && minus) ? 4 : 2] = 1e-12;
    }
    if (kind == 0 && minus) lo.assign(mcap, 0.5);
    if (kind == 3 && !minus) lo.assign(mcap, 1.5);
}

struct HostCol {
    const std::vector<double>*al = nullptr, *lo = nullptr;
    double L = 0.0, U = 0.0, sc[2] = {0.0, 0.0};
    int k = 0, frozen = 0, last = 0;  // frozen: the depth of the breakdown
    int sums(int j, double* pl, double* ph, double* scales) const {
        return kt::gauss_radau_sums(j, al->data(), lo->data(), (*lo)[j - 1], kMu, pl, ph, scales);
    }
};

// the stop rule on the host rule's sums
struct HostPair {
    HostCol c[2];
    int decided = 0, flag = -1, depth = 0;
    // whether every decision so far stays the same when lo and hi move by tol times the sums' unit, sum
    // exp(theta - mu) over the eigenvalues the four sums take
    int robust = 1;
    static int gap_flag(double lo, double hi, double floor_, double rtol) {
        const double gap = hi - lo;
        if (lo * hi > 0.0 && gap >= 0.0 && gap <= rtol * std::min(std::fabs(lo), std::fabs(hi))) return 0;
        return gap <= floor_ ? 4 : 3;
    }
    void step(int j, int mcap, double rtol, double ftol, double tol) {
        if (decided) return;
        for (HostCol& q : c)
            if (!q.frozen) {
                q.k = q.sums(j, &q.L, &q.U, q.sc);
                q.last = j;
                if (q.k == 1) q.frozen = j;
            }
        double lo, hi;
        int f = kt::pair_bracket_combine(c[0].L, c[0].U, c[0].k, c[1].L, c[1].U, c[1].k, rtol, ftol, &lo, &hi);
        if (f == 0 || f == 3 || f == 4) {
            const double d = tol * (c[0].sc[0] + c[0].sc[1] + c[1].sc[0] + c[1].sc[1]);
            const double floor_ = ftol * (0.5 * (c[0].U + c[1].U));
            for (int s = 0; s < 4; ++s)
                if (gap_flag(lo + ((s & 1) ? d : -d), hi + ((s & 2) ? d : -d), floor_, rtol) != f) robust = 0;
        }
        if (f == 3 && j < mcap) f = -1;
        if (f >= 0) {
            decided = 1;
            flag = f;
            depth = j;
        }
    }
};

int main(int argc, char** argv) {
    if (argc < 2) {
        printf("usage: pair_bracket_check TOL [--host]\n");
        return 2;
    }
    const double tol = std::atof(argv[1]);
    const bool host_only = argc > 2 && !std::strcmp(argv[2], "--host");
    // P, mcap, live columns, the first pair's kind
    const int shapes[4][4] = {{16, 256, 16, 0}, {16, 256, 14, 2}, {16, 256, 2, 1}, {16, 128, 16, 3}};
    std::string out = "{\"cases\": [";
    bool first = true;
    for (int si = 0; si < 4; ++si) {
        const int P = shapes[si][0], mcap = shapes[si][1], live = shapes[si][2];
        std::vector<double> rec((size_t)3 * mcap * P, 0.0);
        std::vector<std::vector<double>> als(P), los(P);
        std::vector<int> kinds(P / 2, 0);
        for (int c = 0; c < P; ++c) {
            kinds[c / 2] = (c / 2 + shapes[si][3]) % 5;
            make_column(kinds[c / 2], c, mcap, als[c], los[c]);
            for (int k = 0; k < mcap; ++k) {
                rec[(size_t)(0 * mcap + k) * P + c] = als[c][k];
                rec[(size_t)(2 * mcap + k) * P + c] = los[c][k];
                if (k + 1 < mcap) rec[(size_t)(1 * mcap + k + 1) * P + c] = los[c][k];  // up[k+1] = low[k]
            }
        }
        double *drec = nullptr, *dst = nullptr;
        int* dact = nullptr;
        if (!host_only) {
            CK(hipMalloc(&drec, rec.size() * 8));
            CK(hipMalloc(&dst, (size_t)P * kt::kAdaptState * 8));
            CK(hipMalloc(&dact, 4));
            CK(hipMemcpy(drec, rec.data(), rec.size() * 8, hipMemcpyHostToDevice));
        }
        for (int run = 0; run < 2; ++run) {
            const double rtol = run ? -1.0 : 1e-6, ftol = run ? -1.0 : 1e-9;
            std::vector<int> depths, snaps;
            if (run == 0) {
                for (int j = 1; j <= 16; ++j) depths.push_back(j);
                snaps = {1, 2, 3, 4, 5, 6, 8, 12, 16};
            } else {
                if (mcap > 170) depths = {167, 168, 169, 170};
                depths.push_back(mcap - 1);
                depths.push_back(mcap);
                snaps = depths;
            }
            std::vector<double> st((size_t)P * kt::kAdaptState, 0.0);
            std::vector<HostPair> hp(P / 2);
            // per column and state word: whether it must stay as it starts (2: until the pair is decided)
            std::vector<char> keep((size_t)P * kt::kAdaptState, 0);
            std::vector<char> seeded(P / 2, 0);
            for (int c = 0; c < P; ++c) {
                double* s = &st[(size_t)c * kt::kAdaptState];
                char* kp = &keep[(size_t)c * kt::kAdaptState];
                HostCol& h = hp[c / 2].c[c & 1];
                h.al = &als[c];
                h.lo = &los[c];
                const int kind = kinds[c / 2];
                if (c >= live) {
                    for (int q = 0; q < kt::kAdaptState; ++q) s[q] = kSentinel, kp[q] = 1;
                    seeded[c / 2] = 1;
                } else if (run == 1 && (kind == 2 || kind == 3)) {  // decided at depth 5
                    for (int q = 0; q < kt::kAdaptState; ++q) s[q] = kSentinel, kp[q] = 1;
                    s[3] = 5.0;
                    s[4] = s[5] = 1.0;
                    seeded[c / 2] = 1;
                } else if (run == 1 && kind == 1 && (c & 1)) {  // frozen at depth 3
                    h.k = h.sums(3, &h.L, &h.U, h.sc);
                    h.frozen = h.last = 3;
                    s[0] = h.L;
                    s[1] = h.U;
                    s[3] = s[7] = 3.0;
                    s[4] = s[6] = 1.0;
                    for (int q : {0, 1, 2, 3, 4, 7}) kp[q] = 1;
                    kp[5] = kp[6] = 2;
                }
            }
            const std::vector<double> st0 = st;
            if (!host_only) {
                CK(hipMemcpy(dst, st.data(), st.size() * 8, hipMemcpyHostToDevice));
                CK(hipMemset(dact, 0xff, 4));
            }
            for (int j : depths) {
                if (!host_only)
                    CK(kt::launch_pair_bracket_check(drec, mcap, P, j, live, kMu, rtol, ftol, dst, dact, nullptr));
                for (int p = 0; p < live / 2; ++p)
                    if (!seeded[p]) hp[p].step(j, mcap, rtol, ftol, tol);
                if (std::find(snaps.begin(), snaps.end(), j) == snaps.end()) continue;
                int act = -1;
                if (!host_only) {
                    CK(hipDeviceSynchronize());
                    CK(hipMemcpy(st.data(), dst, st.size() * 8, hipMemcpyDeviceToHost));
                    CK(hipMemcpy(&act, dact, 4, hipMemcpyDeviceToHost));
                }
                int untouched = 1, running = 0;
                for (int c = 0; c < P; ++c) {
                    const double* s = &st[(size_t)c * kt::kAdaptState];
                    if (c < live && s[4] == 0.0) ++running;
                    for (int q = 0; q < kt::kAdaptState; ++q) {
                        const char kq = keep[(size_t)c * kt::kAdaptState + q];
                        if ((kq == 1 || (kq == 2 && s[5] == 0.0)) && s[q] != st0[(size_t)c * kt::kAdaptState + q])
                            untouched = 0;
                    }
                }
                char buf[900];
                snprintf(buf, sizeof buf, "%s{\"P\": %d, \"mcap\": %d, \"j\": %d, \"live\": %d, \"run\": %d, "
                         "\"rtol\": %.3e, \"ftol\": %.3e, \"active\": %d, \"running\": %d, \"untouched\": %d, "
                         "\"pairs\": [", first ? "" : ", ", P, mcap, j, live, run, rtol, ftol, act, running, untouched);
                out += buf;
                first = false;
                bool firstp = true;
                for (int p = 0; p < live / 2; ++p) {
                    if (seeded[p]) continue;
                    const HostPair& h = hp[p];
                    snprintf(buf, sizeof buf, "%s{\"p\": %d, \"kind\": %d, \"decided_host\": %d, \"depth_host\": %d, "
                             "\"flag_host\": %d, \"robust\": %d, \"cols\": [", firstp ? "" : ", ", p, kinds[p],
                             h.decided, h.depth, h.flag, h.robust);
                    out += buf;
                    firstp = false;
                    for (int q = 0; q < 2; ++q) {
                        const double* s = &st[(size_t)(2 * p + q) * kt::kAdaptState];
                        const HostCol& hc = h.c[q];
                        const int sd = s[4] != 0.0, dd = sd ? (int)s[3] : j;
                        // the host rule at the depth the device holds
                        double hl = 0.0, hh = 0.0, sc[2] = {0.0, 0.0};
                        if (dd >= 1 && dd <= mcap) hc.sums(dd, &hl, &hh, sc);
                        auto fin = [](double v) { return std::isfinite(v) ? v : -1.0; };
                        snprintf(buf, sizeof buf,
                                 "%s{\"lo_dev\": %.17g, \"hi_dev\": %.17g, \"lo_host\": %.17g, \"hi_host\": %.17g, "
                                 "\"scale_lo\": %.17g, \"scale_hi\": %.17g, \"hi_nan_dev\": %d, \"hi_nan_host\": %d, "
                                 "\"stopped_dev\": %d, \"depth_dev\": %d, \"decided_dev\": %d, \"flag_dev\": %d, "
                                 "\"last_dev\": %d, \"frozen_host\": %d, \"last_host\": %d}",
                                 q ? ", " : "", fin(s[0]), fin(s[1]), fin(hl), fin(hh), sc[0], sc[1],
                                 (int)std::isnan(s[1]), (int)std::isnan(hh), sd, (int)s[3], (int)s[5], (int)s[6],
                                 (int)s[7], hc.frozen, hc.last);
                        out += buf;
                    }
                    out += "]}";
                }
                out += "]}";
            }
        }
        if (!host_only) {
            CK(hipFree(drec));
            CK(hipFree(dst));
            CK(hipFree(dact));
        }
    }
    out += "]}";
    printf("%s\n", out.c_str());
    return 0;
}
