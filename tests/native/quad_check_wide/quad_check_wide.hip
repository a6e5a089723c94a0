// quad_check_wide -- the device side of the error-controlled probe sweeps
// (kt_slq_trace_auto) below the driver: k_quad_check_wide (kt_adapt.hip), the
// stopping test for any sweep width, on synthetic sweep records against the
// host rule (kt_dense.cpp tridiag_depth_test), and the gated forms of the
// y-form step launches (kt_kernels.hip) on a tiny CSR.  TEST INFRASTRUCTURE:
// built by __graft_entry__.build(), run by tests/test_gpu_quad_check_wide.py,
// which holds the printed figures to its tolerances.  One JSON line on stdout.
//
// Check cases: (P, live) = (1, 1), (16, 16), (64, 48), (128, 128) at record
// capacity 256, each at depths j = 3, 8, 31, 32, 128, 129, 200, 256 (the
// checks of depths j - 2, j - 1, j in turn, as a sweep queues them; 512 j
// bytes of LDS, so j > 128 takes the large dynamic LDS).  Column kinds by
// (column + case) % 5 as in quad_check: a Jacobi matrix whose quadrature
// converges, a zero column, a breakdown at step 2, a cluster of 20 equal
// alphas with offs of 1e-6, a spectrum near 900.  The first half of the live
// columns take the f(A) x test.  State rows past `live` and the running words
// start sentinel-filled: the kernel must leave the former alone and write
// exactly ceil(live / 16) of the latter.
//
// Gate cases: the ordinary pass (weighted), a compact sweep's second step
// (int16 Yold) and first step (int16 X), and k_ycoef, at P = 16 (one running
// word) and P = 128 (eight words, only the last one non-zero when open): with
// every word zero the launch leaves sentinel-filled outputs untouched, with a
// word non-zero it writes the bits of the ungated launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
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

static const double kRtol = 1e-9;
static const double kSentinel = -12345.5;
static const int kSentinelWord = -77;

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

template <class T>
static hipError_t to_dev(T** d, const std::vector<T>& h) {
    hipError_t e = hipMalloc(d, h.size() * sizeof(T));
    if (e != hipSuccess) return e;
    return hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

template <class T>
static hipError_t from_dev(std::vector<T>& h, const T* d) {
    return hipMemcpy(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost);
}

static double unit_rand(uint64_t& s) {  // (0, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return ((s >> 11) + 0.5) / 9007199254740992.0;
}

static int check_cases(std::string& out) {
    const int shapes[4][2] = {{1, 1}, {16, 16}, {64, 48}, {128, 128}};
    const int depths[8] = {3, 8, 31, 32, 128, 129, 200, 256};
    const int mcap = 256;
    out += "\"cases\": [";
    bool first = true;
    int ncase = 0;
    for (int si = 0; si < 4; ++si)
        for (int di = 0; di < 8; ++di, ++ncase) {
            const int P = shapes[si][0], live = shapes[si][1], nfe = (live + 1) / 2, j = depths[di];
            const int ng = (live + kt::kWideCheckCols - 1) / kt::kWideCheckCols;
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
            for (int c = live; c < P; ++c)
                for (int q = 0; q < kt::kAdaptState; ++q) st[(size_t)c * kt::kAdaptState + q] = kSentinel;
            std::vector<int> words(kt::kGateWordsMax, kSentinelWord);
            double *drec, *dn2, *dst;
            int* dw;
            CK(to_dev(&drec, rec));
            CK(to_dev(&dn2, n2));
            CK(to_dev(&dst, st));
            CK(to_dev(&dw, words));
            for (int jj = std::max(1, j - 2); jj <= j; ++jj)
                CK(kt::launch_quad_check_wide(drec, mcap, P, jj, live, nfe, dn2, KT_FUN_EXP, kRtol, dst, dw, nullptr));
            CK(hipDeviceSynchronize());
            CK(from_dev(st, dst));
            CK(from_dev(words, dw));
            CK(hipFree(drec));
            CK(hipFree(dn2));
            CK(hipFree(dst));
            CK(hipFree(dw));
            int untouched = 1;
            for (int c = live; c < P; ++c)
                for (int q = 0; q < kt::kAdaptState; ++q)
                    if (st[(size_t)c * kt::kAdaptState + q] != kSentinel) untouched = 0;
            for (int b = ng; b < kt::kGateWordsMax; ++b)
                if (words[b] != kSentinelWord) untouched = 0;
            char buf[640];
            snprintf(buf, sizeof buf, "%s{\"P\": %d, \"mcap\": %d, \"j\": %d, \"live\": %d, \"untouched\": %d, \"running\": [",
                     first ? "" : ", ", P, mcap, j, live, untouched);
            out += buf;
            first = false;
            for (int b = 0; b < ng; ++b) {
                snprintf(buf, sizeof buf, "%s%d", b ? ", " : "", words[b]);
                out += buf;
            }
            out += "], \"cols\": [";
            for (int c = 0; c < live; ++c) {
                const double* s = &st[(size_t)c * kt::kAdaptState];
                const int want = c < nfe;
                kt::DepthTest h;
                if (n2[c] == 0.0)
                    h.converged = true;
                else
                    h = kt::tridiag_depth_test(j, als[c].data(), los[c].data(), KT_FUN_EXP, want, kRtol);
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
    out += "]";
    return 0;
}

// The guard argument: a running column whose guard value is below gmin stops
// at once, and every stopping column leaves its guard value in gsnap.
static int guard_case(std::string& out) {
    const int P = 16, mcap = 32, j = 12;
    std::vector<double> rec((size_t)3 * mcap * P, 0.0), al, lo;
    for (int c = 0; c < P; ++c) {
        double n2;
        make_column(0, c, mcap, al, lo, &n2);
        for (int k = 0; k < mcap; ++k) {
            rec[(size_t)(0 * mcap + k) * P + c] = al[k];
            rec[(size_t)(2 * mcap + k) * P + c] = lo[k];
            if (k + 1 < mcap) rec[(size_t)(1 * mcap + k + 1) * P + c] = lo[k];
        }
    }
    std::vector<double> st((size_t)P * kt::kAdaptState, 0.0), guard(P, 0.5), gsnap(P, kSentinel);
    guard[3] = 1e-6;
    guard[9] = NAN;
    std::vector<int> words(kt::kGateWordsMax, kSentinelWord);
    double *drec, *dst, *dg, *dgs;
    int* dw;
    CK(to_dev(&drec, rec));
    CK(to_dev(&dst, st));
    CK(to_dev(&dg, guard));
    CK(to_dev(&dgs, gsnap));
    CK(to_dev(&dw, words));
    CK(kt::launch_quad_check_wide(drec, mcap, P, j, P, 0, nullptr, KT_FUN_EXP, kRtol, dst, dw, nullptr, dg, 1e-4, dgs));
    CK(hipDeviceSynchronize());
    CK(from_dev(st, dst));
    CK(from_dev(gsnap, dgs));
    CK(from_dev(words, dw));
    CK(hipFree(drec));
    CK(hipFree(dst));
    CK(hipFree(dg));
    CK(hipFree(dgs));
    CK(hipFree(dw));
    int ok = words[0] == P - 2;
    for (int c = 0; c < P; ++c) {
        const double* s = &st[(size_t)c * kt::kAdaptState];
        const bool tripped = c == 3 || c == 9;
        if (tripped) {
            ok &= s[4] == 1.0 && (int)s[3] == j;
            ok &= c == 3 ? gsnap[c] == 1e-6 : std::isnan(gsnap[c]);
        } else {
            ok &= s[4] == 0.0 && gsnap[c] == kSentinel && s[7] == (double)j;
        }
    }
    char buf[64];
    snprintf(buf, sizeof buf, "\"guard_ok\": %d", ok);
    out += buf;
    return 0;
}

// The check's device time at P = 16 (one workgroup, every column running, so
// each lane runs its whole QL) at depths 8, 16, 32, 64: the figure DESIGN.md
// §4.2a sets beside the step pass.  Reported, not asserted.
static int check_timing(std::string& out) {
    const int P = 16, mcap = 128, reps = 20;
    std::vector<double> rec((size_t)3 * mcap * P, 0.0), al, lo;
    for (int c = 0; c < P; ++c) {
        double n2;
        make_column(0, c, mcap, al, lo, &n2);
        for (int k = 0; k < mcap; ++k) {
            rec[(size_t)(0 * mcap + k) * P + c] = al[k];
            rec[(size_t)(2 * mcap + k) * P + c] = lo[k];
            if (k + 1 < mcap) rec[(size_t)(1 * mcap + k + 1) * P + c] = lo[k];
        }
    }
    double *drec, *dst;
    int* dw;
    CK(to_dev(&drec, rec));
    CK(hipMalloc(&dst, sizeof(double) * P * kt::kAdaptState));
    CK(hipMalloc(&dw, sizeof(int) * kt::kGateWordsMax));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    out += "\"check_us\": {";
    const int depths[4] = {8, 16, 32, 64};
    for (int di = 0; di < 4; ++di) {
        const int j = depths[di];
        double total = 0.0;
        for (int r = -3; r < reps; ++r) {  // three warm-up launches; a zeroed state stops no column
            CK(hipMemsetAsync(dst, 0, sizeof(double) * P * kt::kAdaptState, nullptr));
            CK(hipEventRecord(e0, nullptr));
            CK(kt::launch_quad_check_wide(drec, mcap, P, j, P, 0, nullptr, KT_FUN_EXP, 1e-12, dst, dw, nullptr));
            CK(hipEventRecord(e1, nullptr));
            CK(hipEventSynchronize(e1));
            float ms = 0.f;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 0) total += ms;
        }
        char buf[64];
        snprintf(buf, sizeof buf, "%s\"%d\": %.2f", di ? ", " : "", j, 1e3 * total / reps);
        out += buf;
    }
    out += "}";
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    CK(hipFree(drec));
    CK(hipFree(dst));
    CK(hipFree(dw));
    return 0;
}

struct TinyCsr {
    int n = 0, n_long = 0, long_thresh = 64;
    std::vector<int> rp, ci, long_rows;
    std::vector<double> va;
};

// a ring with a few chords, row 0 with 150 entries (a long-row wave)
static TinyCsr tiny_csr(int n) {
    TinyCsr g;
    g.n = n;
    g.rp.push_back(0);
    uint64_t s = 7;
    for (int r = 0; r < n; ++r) {
        if (r == 0) {
            for (int c = 1; c <= 150; ++c) g.ci.push_back(c);
        } else {
            const int off[6] = {1, 7, 31, n - 31, n - 7, n - 1};
            std::vector<int> cs;
            for (int o : off) cs.push_back((r + o) % n);
            std::sort(cs.begin(), cs.end());
            for (int c : cs) g.ci.push_back(c);
        }
        g.rp.push_back((int)g.ci.size());
    }
    for (size_t k = 0; k < g.ci.size(); ++k) g.va.push_back(0.5 + unit_rand(s));
    g.long_rows.push_back(0);
    g.n_long = 1;
    return g;
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

static bool all_sentinel(const std::vector<double>& a) {
    for (double v : a)
        if (v != kSentinel) return false;
    return true;
}

static int gate_cases(std::string& out) {
    const TinyCsr g = tiny_csr(700);
    int *drp, *dci, *dlr;
    double* dva;
    CK(to_dev(&drp, g.rp));
    CK(to_dev(&dci, g.ci));
    CK(to_dev(&dlr, g.long_rows));
    CK(to_dev(&dva, g.va));
    out += "\"gate\": [";
    bool first = true;
    for (int P : {16, 128}) {
        const int n = g.n, ng = P / kt::kWideCheckCols;
        const int grid = kt::spmm_grid(n, P, 1024), lblocks = kt::long_blocks_for(g.n_long, 512), grid1 = grid + lblocks;
        uint64_t s = 11 + P;
        std::vector<double> X((size_t)n * P), Yold((size_t)n * P), coef(3 * P), sent((size_t)n * P, kSentinel);
        std::vector<double> psent((size_t)3 * P * grid1, kSentinel);
        std::vector<int16_t> T((size_t)n * P);
        for (auto& v : X) v = unit_rand(s) - 0.5;
        for (auto& v : Yold) v = unit_rand(s) - 0.5;
        for (auto& v : coef) v = 0.25 + unit_rand(s);
        for (auto& v : T) v = (int16_t)((int)(unit_rand(s) * 11.0) - 5);
        const double s0 = 1.0 / std::sqrt((double)n);
        std::vector<int> open(ng, 0), closed(ng, 0);
        open[ng - 1] = 3;  // only the last word running
        double *dX, *dY, *dcoef, *dOut, *dpart;
        int16_t* dT;
        int *dopen, *dclosed;
        CK(to_dev(&dX, X));
        CK(to_dev(&dY, Yold));
        CK(to_dev(&dcoef, coef));
        CK(to_dev(&dT, T));
        CK(to_dev(&dOut, sent));
        CK(to_dev(&dpart, psent));
        CK(to_dev(&dopen, open));
        CK(to_dev(&dclosed, closed));
        // kernel 0: the ordinary pass (weighted); 1: a compact sweep's second
        // step (int16 Yold); 2: its first step (int16 X)
        for (int kern = 0; kern < 3; ++kern) {
            std::vector<double> o_ref(sent.size()), p_ref(psent.size()), o(sent.size()), p(psent.size());
            int open_equal = 0, closed_untouched = 0;
            for (int run = 0; run < 3; ++run) {  // ungated, gated open, gated closed
                const int* gate = run == 0 ? nullptr : run == 1 ? dopen : dclosed;
                CK(hipMemcpy(dOut, sent.data(), sent.size() * 8, hipMemcpyHostToDevice));
                CK(hipMemcpy(dpart, psent.data(), psent.size() * 8, hipMemcpyHostToDevice));
                if (kern == 0)
                    CK(kt::launch_spmm_lanczos(P, 8, grid1, drp, dci, dva, n, dX, dY, dOut, dcoef, dpart, dlr, g.n_long,
                                               g.long_thresh, lblocks, nullptr, nullptr, nullptr, nullptr, 0, 0.0, gate,
                                               ng));
                else if (kern == 1)
                    CK(kt::launch_spmm_lanczos(P, 2 | 8 | 128, grid1, drp, dci, dva, n, dX,
                                               reinterpret_cast<const double*>(dT), dOut, dcoef, dpart, dlr, g.n_long,
                                               g.long_thresh, lblocks, nullptr, nullptr, nullptr, nullptr, 0, s0, gate,
                                               ng));
                else
                    CK(kt::launch_spmm_lanczos_first(P, 2 | 8, grid1, drp, dci, n, dT, s0, dOut, dcoef, dpart, dlr,
                                                     g.n_long, g.long_thresh, lblocks, nullptr, gate, ng));
                CK(hipDeviceSynchronize());
                CK(from_dev(run == 0 ? o_ref : o, dOut));
                CK(from_dev(run == 0 ? p_ref : p, dpart));
                if (run == 1) open_equal = same_bits(o, o_ref) && same_bits(p, p_ref) && !all_sentinel(o);
                if (run == 2) closed_untouched = all_sentinel(o) && all_sentinel(p);
            }
            char buf[200];
            snprintf(buf, sizeof buf, "%s{\"kernel\": \"%s\", \"P\": %d, \"open_equal\": %d, \"closed_untouched\": %d}",
                     first ? "" : ", ", kern == 0 ? "pass" : kern == 1 ? "pass_i16" : "first", P, open_equal,
                     closed_untouched);
            out += buf;
            first = false;
        }
        // k_ycoef: state ys (9 P), one record row (3 P) and the guard (P) in one block
        {
            std::vector<double> part((size_t)3 * P * grid1), blk((size_t)13 * P), ref(blk.size()), got(blk.size());
            for (auto& v : part) v = unit_rand(s);
            for (auto& v : blk) v = 0.5 + unit_rand(s);
            double *dp2, *dblk;
            CK(to_dev(&dp2, part));
            CK(to_dev(&dblk, blk));
            int open_equal = 0, closed_untouched = 0;
            for (int run = 0; run < 3; ++run) {
                const int* gate = run == 0 ? nullptr : run == 1 ? dopen : dclosed;
                CK(hipMemcpy(dblk, blk.data(), blk.size() * 8, hipMemcpyHostToDevice));
                CK(kt::launch_ycoef(P, dp2, grid1, 0, 0, 0.0, dblk, dblk + 9 * P, dblk + 10 * P, dblk + 11 * P,
                                    dblk + 12 * P, nullptr, gate, ng));
                CK(hipDeviceSynchronize());
                CK(from_dev(run == 0 ? ref : got, dblk));
                if (run == 1) open_equal = same_bits(got, ref) && !same_bits(got, blk);
                if (run == 2) closed_untouched = same_bits(got, blk);
            }
            CK(hipFree(dp2));
            CK(hipFree(dblk));
            char buf[200];
            snprintf(buf, sizeof buf, ", {\"kernel\": \"ycoef\", \"P\": %d, \"open_equal\": %d, \"closed_untouched\": %d}", P,
                     open_equal, closed_untouched);
            out += buf;
        }
        CK(hipFree(dX));
        CK(hipFree(dY));
        CK(hipFree(dcoef));
        CK(hipFree(dT));
        CK(hipFree(dOut));
        CK(hipFree(dpart));
        CK(hipFree(dopen));
        CK(hipFree(dclosed));
    }
    out += "]";
    CK(hipFree(drp));
    CK(hipFree(dci));
    CK(hipFree(dlr));
    CK(hipFree(dva));
    return 0;
}

int main() {
    std::string out = "{\"rtol\": 1e-9, ";
    if (int e = check_cases(out)) return e;
    out += ", ";
    if (int e = guard_case(out)) return e;
    out += ", ";
    if (int e = gate_cases(out)) return e;
    out += ", ";
    if (int e = check_timing(out)) return e;
    out += "}";
    printf("%s\n", out.c_str());
    return 0;
}
