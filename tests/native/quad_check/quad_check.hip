// quad_check -- k_quad_check (kt_adapt.hip), the adaptive Lanczos depth's
// device stopping test, on synthetic sweep records against the host rule
// (kt_dense.cpp tridiag_depth_test).  TEST INFRASTRUCTURE: built by
// __graft_entry__.build(), run by tests/test_gpu_quad_check.py, which holds
// the printed figures to its tolerances.  One JSON line on stdout.
//
// Cases: (P, mcap) = (1, 256), (4, 256), (16, 128), (16, 256), each at depths
// j = 3, 8, 31, 32 and mcap (the checks of depths j - 2, j - 1, j in turn, as
// a sweep queues them); (16, 256) at j > 128 takes the launcher's 8-lane
// groups.  Column kinds by (lane + case) % 5: a Jacobi matrix whose
// quadrature converges, a zero column, a breakdown at step 2, a cluster of 20
// equal alphas with offs of 1e-6, a spectrum near 900.  The first half of the
// live columns take the f(A) x test.  A last case runs P = 16 with 5 live
// columns over a sentinel-filled state.
#include <hip/hip_runtime.h>

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

static const double kRtol = 1e-9;
static const double kSentinel = -12345.5;

// column `kind`: alpha[k], low[k] (= the off-diagonal below row k), k < mcap
static void make_column(int kind, int lane, int mcap, std::vector<double>& al, std::vector<double>& lo, double* n2) {
    al.assign(mcap, 0.0);
    lo.assign(mcap, 0.0);
    *n2 = 3.0 + lane;
    for (int k = 0; k < mcap; ++k) {
        al[k] = 2.0 + 0.5 * std::cos(0.7 * k + lane);
        lo[k] = 1.0 + 0.3 * std::sin(1.3 * k + 0.5 * lane);
    }
    if (kind == 1) *n2 = 0.0;
    if (kind == 2) lo[1] = 1e-12;
    if (kind == 3)
        for (int k = 0; k < 20 && k < mcap; ++k) {
            al[k] = 1.5;
            lo[k] = 1e-6;
        }
    if (kind == 4)
        for (int k = 0; k < mcap; ++k) {
            al[k] = 600.0 + 20.0 * std::cos(0.9 * k + lane);
            lo[k] = 150.0 + 10.0 * std::sin(0.4 * k);
        }
}

int main() {
    const int shapes[4][2] = {{1, 256}, {4, 256}, {16, 128}, {16, 256}};
    std::string out = "{\"rtol\": 1e-9, \"cases\": [";
    bool first = true;
    int ncase = 0;
    for (int si = 0; si < 5; ++si) {
        const bool sentinel_case = si == 4;
        const int P = sentinel_case ? 16 : shapes[si][0], mcap = sentinel_case ? 128 : shapes[si][1];
        const int live = sentinel_case ? 5 : P, nfe = (live + 1) / 2;
        const int depths[5] = {3, 8, 31, 32, mcap};
        for (int di = 0; di < (sentinel_case ? 1 : 5); ++di, ++ncase) {
            const int j = sentinel_case ? 31 : depths[di];
            std::vector<double> rec((size_t)3 * mcap * P, 0.0), n2(P, 1.0);
            std::vector<std::vector<double>> als(P), los(P);
            std::vector<int> kinds(P, 0);
            for (int c = 0; c < P; ++c) {
                kinds[c] = (c + ncase) % 5;
                make_column(kinds[c], c, mcap, als[c], los[c], &n2[c]);
                for (int k = 0; k < mcap; ++k) {
                    rec[(size_t)(0 * mcap + k) * P + c] = als[c][k];
                    rec[(size_t)(2 * mcap + k) * P + c] = los[c][k];
                    if (k + 1 < mcap) rec[(size_t)(1 * mcap + k + 1) * P + c] = los[c][k];  // up[k+1] = low[k]
                }
            }
            std::vector<double> st((size_t)P * kt::kAdaptState, 0.0);
            if (sentinel_case)
                for (int c = live; c < P; ++c)
                    for (int q = 0; q < kt::kAdaptState; ++q) st[(size_t)c * kt::kAdaptState + q] = kSentinel;
            double *drec, *dn2, *dst;
            int* dact;
            CK(hipMalloc(&drec, rec.size() * 8));
            CK(hipMalloc(&dn2, P * 8));
            CK(hipMalloc(&dst, st.size() * 8));
            CK(hipMalloc(&dact, 4));
            CK(hipMemcpy(drec, rec.data(), rec.size() * 8, hipMemcpyHostToDevice));
            CK(hipMemcpy(dn2, n2.data(), P * 8, hipMemcpyHostToDevice));
            CK(hipMemcpy(dst, st.data(), st.size() * 8, hipMemcpyHostToDevice));
            CK(hipMemset(dact, 0xff, 4));
            for (int jj = std::max(1, j - 2); jj <= j; ++jj)
                CK(kt::launch_quad_check(drec, mcap, P, jj, live, nfe, dn2, KT_FUN_EXP, kRtol, dst, dact, nullptr));
            CK(hipDeviceSynchronize());
            int act = -1;
            CK(hipMemcpy(st.data(), dst, st.size() * 8, hipMemcpyDeviceToHost));
            CK(hipMemcpy(&act, dact, 4, hipMemcpyDeviceToHost));
            CK(hipFree(drec));
            CK(hipFree(dn2));
            CK(hipFree(dst));
            CK(hipFree(dact));
            int untouched = 1;
            for (int c = live; c < P; ++c)
                for (int q = 0; q < kt::kAdaptState; ++q)
                    if (sentinel_case && st[(size_t)c * kt::kAdaptState + q] != kSentinel) untouched = 0;
            char buf[512];
            snprintf(buf, sizeof buf, "%s{\"P\": %d, \"mcap\": %d, \"j\": %d, \"live\": %d, \"active\": %d, "
                     "\"untouched\": %d, \"cols\": [", first ? "" : ", ", P, mcap, j, live, act, untouched);
            out += buf;
            first = false;
            for (int c = 0; c < live; ++c) {
                const double* s = &st[(size_t)c * kt::kAdaptState];
                const int want = c < nfe;
                kt::DepthTest h;
                if (n2[c] == 0.0) {
                    h.converged = true;
                } else {
                    h = kt::tridiag_depth_test(j, als[c].data(), los[c].data(), KT_FUN_EXP, want, kRtol);
                }
                auto fin = [](double v) { return std::isfinite(v) ? v : 1e300; };
                snprintf(buf, sizeof buf,
                         "%s{\"c\": %d, \"kind\": %d, \"fe1\": %d, \"q_dev\": %.17g, \"q_host\": %.17g, \"depth_dev\": %d, "
                         "\"stopped_dev\": %d, \"steps_host\": %d, \"conv_host\": %d, \"r1\": %.6e, \"r2\": %.6e, "
                         "\"r3\": %.6e}",
                         c ? ", " : "", c, kinds[c], want, fin(s[0]), fin(h.q), (int)s[3], (int)s[4], h.steps,
                         (int)h.converged, fin(h.r1), fin(h.r2), fin(h.r3));
                out += buf;
            }
            out += "]}";
        }
    }
    out += "]}";
    printf("%s\n", out.c_str());
    return 0;
}
