// kt_adapt.hip -- device side of the adaptive Lanczos depth (kt_slq.cpp
// lanczos_columns_adaptive): the per-column stopping test on a sweep's device
// record, and the back-projection over a basis kept in growth chunks.
//
// k_quad_check decides depths only; the values a call returns are formed on
// the host from the record truncated at the depth chosen here.
// k_node_check is the same for the node-removal columns of
// lanczos_nodes_adaptive (§4.2h), k_unit_start their sweeps' start block, and
// k_bracket_check the test of lanczos_nodes_bracket's columns (§4.2i);
// k_pair_bracket_check and k_pair_start are the same for the column pairs of
// lanczos_pairs_bracket (§4.2j).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "kt_internal.h"
#include "kt_launch.h"

namespace kt {

namespace {

__device__ __forceinline__ double dev_fscalar(int fun, double x) {
    switch (fun) {
    case KT_FUN_EXP: return exp(x);
    case KT_FUN_SINH: return sinh(x);
    case KT_FUN_COSH: return cosh(x);
    case KT_FUN_SIN: return sin(x);
    case KT_FUN_COS: return cos(x);
    case KT_FUN_LOG: return log(x);
    case KT_FUN_SQRT: return sqrt(x);
    default: return NAN;
    }
}

__device__ __forceinline__ double dev_rot_radius(double f, double g) {
    const double af = fabs(f), ag = fabs(g);
    const double mx = af > ag ? af : ag;
    if (mx > 1e150 || (mx < 1e-150 && mx > 0.0)) return hypot(f, g);
    return sqrt(f * f + g * g);
}

// The host's implicit-shift QL (kt_dense.cpp ql_rows; EISPACK IMTQL2) on one
// lane's m x m tridiagonal, arrays strided by G in LDS ([k][lane]); z carries
// the first row of the eigenvector matrix, zl (LAST) the last row.
template <bool LAST>
__device__ void dev_ql_rows(int m, int G, double* d, double* e, double* z, double* zl) {
    e[(m - 1) * G] = 0.0;
    for (int i = 0; i < m; ++i) {
        z[i * G] = (i == 0) ? 1.0 : 0.0;
        if (LAST) zl[i * G] = (i == m - 1) ? 1.0 : 0.0;
    }
    for (int l = 0; l < m; ++l) {
        int iter = 0;
        for (;;) {
            int mm = l;
            for (; mm < m - 1; ++mm) {
                const double dd = fabs(d[mm * G]) + fabs(d[(mm + 1) * G]);
                if (fabs(e[mm * G]) <= 2.220446049250313e-16 * dd) break;
            }
            if (mm == l || iter++ == 100) break;
            double g = (d[(l + 1) * G] - d[l * G]) / (2.0 * e[l * G]);
            double r = dev_rot_radius(g, 1.0);
            g = d[mm * G] - d[l * G] + e[l * G] / (g + copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            bool deflated = false;
            for (int i = mm - 1; i >= l; --i) {
                const double f = s * e[i * G], b = c * e[i * G];
                r = dev_rot_radius(f, g);
                e[(i + 1) * G] = r;
                if (r == 0.0) {
                    d[(i + 1) * G] -= p;
                    e[mm * G] = 0.0;
                    deflated = true;
                    break;
                }
                s = f / r;
                c = g / r;
                g = d[(i + 1) * G] - p;
                r = (d[i * G] - g) * s + 2.0 * c * b;
                p = s * r;
                d[(i + 1) * G] = g + p;
                g = c * r - b;
                const double zf = z[(i + 1) * G];
                z[(i + 1) * G] = s * z[i * G] + c * zf;
                z[i * G] = c * z[i * G] - s * zf;
                if (LAST) {
                    const double lf = zl[(i + 1) * G];
                    zl[(i + 1) * G] = s * zl[i * G] + c * lf;
                    zl[i * G] = c * zl[i * G] - s * lf;
                }
            }
            if (deflated) continue;
            d[l * G] -= p;
            e[l * G] = g;
            e[mm * G] = 0.0;
        }
    }
}

// One column's stopping test at depth j (lane t of G owns column c; the LDS
// arrays sm are [k][lane] with stride G): the body of k_quad_check and
// k_quad_check_wide.  Returns whether the column is stopped after it.
// guard / gmin / gsnap: k_quad_check_wide's guard argument (nullptr: none).
__device__ __forceinline__ int dev_check_column(const double* __restrict__ trec, int mcap, int P, int j, int c,
                                                int t, int G, int nfe, const double* __restrict__ n2, int fun,
                                                double rtol, double* __restrict__ state, double* sm,
                                                const double* __restrict__ guard, double gmin,
                                                double* __restrict__ gsnap) {
    int stopped;
    double* st = state + (size_t)c * kAdaptState;
    stopped = st[4] != 0.0;
    if (!stopped && n2 && !(n2[c] > 0.0)) {
        st[0] = 0.0;
        st[3] = 0.0;
        st[4] = 1.0;
        stopped = 1;
        if (guard) gsnap[c] = 1.0;
    } else if (!stopped && guard && !(guard[c] >= gmin)) {
        st[3] = (double)j;
        st[4] = 1.0;
        stopped = 1;
        gsnap[c] = guard[c];
    } else if (!stopped) {
        const double* al = trec + c;
        const double* up = trec + (size_t)mcap * P + c;
        const double* low = trec + (size_t)2 * mcap * P + c;
        int steps = j;
        bool broke = false;
        for (int k = 0; k < j; ++k)
            if (low[(size_t)k * P] < 1e-8) {
                steps = k + 1;
                broke = true;
                break;
            }
        double* d = sm + t;
        double* e = sm + (size_t)j * G + t;
        double* z = sm + (size_t)2 * j * G + t;
        double* zl = sm + (size_t)3 * j * G + t;
        for (int k = 0; k < steps; ++k) d[k * G] = al[(size_t)k * P];
        for (int k = 0; k + 1 < steps; ++k) e[k * G] = 0.5 * (low[(size_t)k * P] + up[(size_t)(k + 1) * P]);
        const bool wf = c < nfe && !broke;
        if (wf)
            dev_ql_rows<true>(steps, G, d, e, z, zl);
        else
            dev_ql_rows<false>(steps, G, d, e, z, zl);
        double tm = d[0];
        for (int k = 1; k < steps; ++k) tm = fmax(tm, d[k * G]);
        const double shift = (fun == KT_FUN_EXP) ? tm : 0.0;
        double q = 0.0, lastc = 0.0, nrm2 = 0.0;
        for (int k = 0; k < steps; ++k) {
            const double w = dev_fscalar(fun, d[k * G] - shift), z1 = z[k * G];
            q += z1 * z1 * w;
            if (wf) lastc += zl[k * G] * z1 * w;
            nrm2 += z1 * z1 * w * w;
        }
        const bool hist = st[7] == (double)(j - 1);
        const double q1 = st[0];
        // theta_max grows with the depth: the shallower sum at this depth's scale
        const double q1s = (fun == KT_FUN_EXP) ? q1 * exp(st[5] - tm) : q1;
        const bool agree1 = hist && fabs(q - q1s) <= rtol * fabs(q);
        const bool agree2 = hist && st[6] != 0.0;
        bool stop = broke;
        if (!stop && j >= kAdaptMinDepth && agree1 && agree2)
            stop = !wf || low[(size_t)(j - 1) * P] * fabs(lastc) <= rtol * sqrt(nrm2);
        st[2] = st[1];
        st[1] = q1;
        st[0] = q;
        st[5] = tm;
        st[6] = agree1 ? 1.0 : 0.0;
        st[7] = (double)j;
        if (stop) {
            st[3] = (double)steps;
            st[4] = 1.0;
            stopped = 1;
            if (guard) gsnap[c] = guard[c];
        }
    }
    return stopped;
}

}  // namespace

// The stopping test of the adaptive depth at depth j: one workgroup of one
// wavefront, lane t owns column c = g0 + t (t < G, c < live).  trec: the
// sweep's device record [alpha | up | low][mcap][P].  state: kAdaptState
// doubles per column,
//   [0] q_j  [1] q_{j-1}  [2] q_{j-2}  [3] depth  [4] stopped  [5] theta_max_j
//   [6] q_j agreed with q_{j-1}  [7] the depth of the last check
// (fun = exp: each q scaled by exp(-theta_max) of its own depth).  The two
// quadrature agreements come from consecutive launches (j - 2, j - 1, j), so
// a column's decision needs the checks of the two depths before it; a stopped
// column is left as it is.  Columns < nfe also take the f(A) x residual test
// (beta_j = low[j-1]).  n2 (nullable): squared column norms, a zero column
// stops at once with depth 0.  active[0]: the live columns still running, an
// ordinary store by lane 0 after the barrier.  No cross-lane operation: the
// lanes' QL loops diverge freely.
__global__ __launch_bounds__(64) void k_quad_check(const double* __restrict__ trec, int mcap, int P, int j, int live,
                                                   int g0, int G, int nfe, const double* __restrict__ n2, int fun,
                                                   double rtol, double* __restrict__ state,
                                                   int* __restrict__ active) {
    extern __shared__ double sm[];
    __shared__ int stopped_l[64];
    const int t = threadIdx.x, c = g0 + t;
    const bool mine = t < G && c < live;
    int stopped = -1;
    if (mine)
        stopped = dev_check_column(trec, mcap, P, j, c, t, G, nfe, n2, fun, rtol, state, sm, nullptr, 0.0, nullptr);
    stopped_l[t] = stopped;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < live; ++k) {
            const bool here = k >= g0 && k < g0 + G;  // another group's columns: an earlier launch wrote them
            run += here ? (stopped_l[k - g0] == 0) : (state[(size_t)k * kAdaptState + 4] == 0.0);
        }
        active[0] = run;
    }
}

// P <= 32 columns, 1 <= j <= mcap <= 256.  The four LDS arrays of depth j
// take 32 j G bytes: every live column in one launch while that fits 64 KB
// (P = 16 up to depth 128), else column groups of 8 lanes per launch (64 KB
// at depth 256), each group's count taken over all live columns.
hipError_t launch_quad_check(const double* trec, int mcap, int P, int j, int live, int nfe, const double* n2,
                             int fun, double rtol, double* state, int* active, hipStream_t st) {
    if (P < 1 || P > 32 || live < 1 || live > P || j < 1 || j > mcap || mcap > 256) return hipErrorInvalidValue;
    const int G = ((size_t)32 * j * P <= (size_t)65536) ? P : 8;
    for (int g0 = 0; g0 < live; g0 += G) {
        k_quad_check<<<1, 64, sizeof(double) * 4 * j * G, st>>>(trec, mcap, P, j, live, g0, G, nfe, n2, fun, rtol,
                                                                 state, active);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// k_quad_check for any sweep width (the SLQ sweeps, kt_slq.cpp
// slq_trace_auto): workgroup b owns columns [16 b, 16 b + 16), lane t column
// 16 b + t, with the same per-column test, state layout and [k][lane] LDS
// arrays (G = 16: 512 j bytes).  running[b]: workgroup b's columns still
// running -- its own columns only, an ordinary store by lane 0, so no
// workgroup reads another's state and the sweep's running words are the
// grid's ceil(live / 16) counts (the gate of the step launches ORs them).
// guard (nullable; the y-form sweep's running guard value per column): a
// running column whose guard is not >= gmin stops at once, flagged with its
// depth (its sweep is redone by the explicit sweep whatever it decides); a
// column that stops leaves the guard it stopped with in gsnap[c], the value
// the host judges the sweep by, so the verdict does not depend on how many
// steps ran past the column's depth.
__global__ __launch_bounds__(64) void k_quad_check_wide(const double* __restrict__ trec, int mcap, int P, int j,
                                                        int live, int nfe, const double* __restrict__ n2, int fun,
                                                        double rtol, double* __restrict__ state,
                                                        int* __restrict__ running,
                                                        const double* __restrict__ guard, double gmin,
                                                        double* __restrict__ gsnap) {
    extern __shared__ double sm[];
    __shared__ int stopped_l[kWideCheckCols];
    constexpr int G = kWideCheckCols;
    const int t = threadIdx.x, c = blockIdx.x * G + t;
    const bool mine = t < G && c < live;
    int stopped = -1;
    if (mine) stopped = dev_check_column(trec, mcap, P, j, c, t, G, nfe, n2, fun, rtol, state, sm, guard, gmin, gsnap);
    if (t < G) stopped_l[t] = stopped;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < G; ++k) run += stopped_l[k] == 0;
        running[blockIdx.x] = run;
    }
}

// 1 <= live <= P <= 128, 1 <= j <= mcap <= 256: one launch of ceil(live / 16)
// workgroups per check.  512 j bytes of LDS per workgroup: from 64 KB on (j >= 128)
// the kernel opts in to the large dynamic LDS (128 KB at j = 256 of the 160 KB
// a gfx950 workgroup may declare).
hipError_t launch_quad_check_wide(const double* trec, int mcap, int P, int j, int live, int nfe, const double* n2,
                                  int fun, double rtol, double* state, int* running, hipStream_t st,
                                  const double* guard, double gmin, double* gsnap) {
    if (P < 1 || P > 128 || live < 1 || live > P || j < 1 || j > mcap || mcap > 256) return hipErrorInvalidValue;
    if (guard && !gsnap) return hipErrorInvalidValue;
    const size_t lds = sizeof(double) * 4 * (size_t)j * kWideCheckCols;
    // with the kernel's static stopped_l the workgroup passes 64 KB from j = 128 on;
    // the opt-in is per device and made once for each
    if (lds + sizeof(int) * kWideCheckCols > (size_t)65536) {
        static std::atomic<uint64_t> opted{0};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const uint64_t bit = (dev >= 0 && dev < 64) ? (uint64_t)1 << dev : 0;
        if (!bit || !(opted.load(std::memory_order_acquire) & bit)) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_quad_check_wide),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(double) * 4 * 256 * kWideCheckCols));
            if (e != hipSuccess) return e;
            opted.fetch_or(bit, std::memory_order_release);
        }
    }
    const int grid = (live + kWideCheckCols - 1) / kWideCheckCols;
    k_quad_check_wide<<<grid, 64, lds, st>>>(trec, mcap, P, j, live, nfe, n2, fun, rtol, state, running, guard,
                                             gmin, gsnap);
    return hipGetLastError();
}

namespace {

// ascending insertion sort of one lane's m values (stride G in LDS)
__device__ __forceinline__ void dev_sort_strided(int m, int G, double* d) {
    for (int i = 1; i < m; ++i) {
        const double v = d[i * G];
        int k = i - 1;
        for (; k >= 0 && d[k * G] > v; --k) d[(k + 1) * G] = d[k * G];
        d[(k + 1) * G] = v;
    }
}

}  // namespace

// The stopping test of a node-removal column at depth j (DESIGN.md §4.2h;
// kt_slq.cpp lanczos_nodes_adaptive): k_quad_check's launch shape -- one
// wavefront, lane t owns column c = g0 + t (t < G, c < live), LDS arrays
// [k][lane] with stride G.  The column's sweep started at a unit vector e_i, so
// with T_j the record's leading j x j tridiagonal
//   X_j = trace_diff(sort({0} + eig(T_j[2:, 2:])), sort(eig(T_j)))
// (two value-only QL runs) approximates tr f(A_{-i}) - tr f(A).  state:
// kAdaptState doubles per column, zeroed before the sweep's first check,
//   [0] X_j  [1] Xstop[0]  [2] Xstop[1]  [3] depth  [4] stopped  [5] theta_max_j
//   [6] lucky  [7] the depth of the last check
// fun = exp: the three X scaled by exp(-theta_max_j) (the stored two are
// brought to each new depth's scale; theta_max grows with the depth), and tol
// scaled the same way in the comparison, so nothing overflows below exp's own
// range.  The rule is trace_fun_update.m:104-124: X_1 and X_2 are stored; for
// j > 2 the column stops when |X_j - X_{j-2}| < tol, else the stored pair
// moves up; a column that did not stop stops with lucky = 1 when the record's
// beta_j (low[j-1]) < 1e-8.  The checks of a sweep run at consecutive depths
// from 1; a stopped column is left as it is.  active[0]: as k_quad_check's.
__global__ __launch_bounds__(64) void k_node_check(const double* __restrict__ trec, int mcap, int P, int j, int live,
                                                   int g0, int G, int fun, double tol, double* __restrict__ state,
                                                   int* __restrict__ active) {
    extern __shared__ double sm[];
    __shared__ int stopped_l[64];
    const int t = threadIdx.x, c = g0 + t;
    const bool mine = t < G && c < live;
    int stopped = -1;
    if (mine) {
        double* st = state + (size_t)c * kAdaptState;
        stopped = st[4] != 0.0;
        if (!stopped) {
            const double* al = trec + c;
            const double* up = trec + (size_t)mcap * P + c;
            const double* low = trec + (size_t)2 * mcap * P + c;
            double* d2 = sm + t;
            double* d1 = sm + (size_t)j * G + t;
            double* e = sm + (size_t)2 * j * G + t;
            double* z = sm + (size_t)3 * j * G + t;
            for (int k = 0; k < j; ++k) d2[k * G] = al[(size_t)k * P];
            for (int k = 0; k + 1 < j; ++k) e[k * G] = 0.5 * (low[(size_t)k * P] + up[(size_t)(k + 1) * P]);
            dev_ql_rows<false>(j, G, d2, e, z, nullptr);
            if (j > 1) {
                for (int k = 0; k + 1 < j; ++k) d1[k * G] = al[(size_t)(k + 1) * P];
                for (int k = 0; k + 2 < j; ++k)
                    e[k * G] = 0.5 * (low[(size_t)(k + 1) * P] + up[(size_t)(k + 2) * P]);
                dev_ql_rows<false>(j - 1, G, d1, e, z, nullptr);
            }
            d1[(j - 1) * G] = 0.0;  // the removed node stays as an isolated vertex: f(0)
            dev_sort_strided(j, G, d1);
            dev_sort_strided(j, G, d2);
            const double tm = fmax(d1[(j - 1) * G], d2[(j - 1) * G]);
            double x = 0.0;
            if (fun == KT_FUN_EXP) {
                for (int k = 0; k < j; ++k) x += exp(d1[k * G] - tm) * (1.0 - exp(d2[k * G] - d1[k * G]));
            } else {
                for (int k = 0; k < j; ++k) x += dev_fscalar(fun, d1[k * G]) - dev_fscalar(fun, d2[k * G]);
            }
            const bool ex = fun == KT_FUN_EXP;
            const double r = (ex && j > 1) ? exp(st[5] - tm) : 1.0;  // the stored pair at this depth's scale
            double x0 = st[1] * r, x1 = st[2] * r;
            bool stop = false;
            if (j == 1) {
                x0 = x;
            } else if (j == 2) {
                x1 = x;
            } else if (fabs(x - x0) < (ex ? tol * exp(-tm) : tol)) {
                stop = true;
            } else {
                x0 = x1;
                x1 = x;
            }
            const bool lucky = low[(size_t)(j - 1) * P] < 1e-8;
            if (!stop && lucky) stop = true;
            st[0] = x;
            st[1] = x0;
            st[2] = x1;
            st[5] = ex ? tm : 0.0;
            st[7] = (double)j;
            if (stop) {
                st[3] = (double)j;
                st[4] = 1.0;
                st[6] = lucky ? 1.0 : 0.0;
                stopped = 1;
            }
        }
    }
    stopped_l[t] = stopped;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < live; ++k) {
            const bool here = k >= g0 && k < g0 + G;  // another group's columns: an earlier launch wrote them
            run += here ? (stopped_l[k - g0] == 0) : (state[(size_t)k * kAdaptState + 4] == 0.0);
        }
        active[0] = run;
    }
}

// P <= 32 columns, 1 <= j <= mcap <= 256.  The four LDS arrays of depth j take
// 32 j G bytes: every live column in one launch while they fit 64 KB together
// with the kernel's static words (P = 16 up to depth 127), else column groups
// of 8 lanes per launch, and of 4 at the depths where 8 lanes' arrays alone
// are 64 KB (j = 256); each group's count is taken over all live columns.
hipError_t launch_node_check(const double* trec, int mcap, int P, int j, int live, int fun, double tol, double* state,
                             int* active, hipStream_t st) {
    if (P < 1 || P > 32 || live < 1 || live > P || j < 1 || j > mcap || mcap > 256) return hipErrorInvalidValue;
    const size_t room = (size_t)65536 - 512;
    int G = P;
    if ((size_t)32 * j * G > room) G = 8;
    if ((size_t)32 * j * G > room) G = 4;
    for (int g0 = 0; g0 < live; g0 += G) {
        k_node_check<<<1, 64, sizeof(double) * 4 * j * G, st>>>(trec, mcap, P, j, live, g0, G, fun, tol, state, active);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// One column's Gauss / Gauss-Radau sums at depth j, the body k_bracket_check and
// k_pair_bracket_check share (lane t of G owns column c; sm: the three LDS
// arrays): *lo = L_j, *hi = U_j.  Returns 1 when beta_j < 1e-8 (*hi = *lo), 2
// when a pivot is not negative or a Ritz value lies above mu (*hi = NaN), else 0.
__device__ __forceinline__ int dev_bracket_column(const double* __restrict__ trec, int mcap, int P, int j, int c,
                                                  int t, int G, double mu, double* sm, double* plo, double* phi) {
    const double* al = trec + c;
    const double* up = trec + (size_t)mcap * P + c;
    const double* low = trec + (size_t)2 * mcap * P + c;
    double* d = sm + t;
    double* e = sm + (size_t)(j + 1) * G + t;
    double* z = sm + (size_t)2 * (j + 1) * G + t;
    double dk = al[0] - mu;
    bool bad = !(dk < 0.0);
    d[0] = al[0];
    for (int k = 1; k < j; ++k) {
        const double b = 0.5 * (low[(size_t)(k - 1) * P] + up[(size_t)k * P]);
        e[(k - 1) * G] = b;
        d[k * G] = al[(size_t)k * P];
        dk = al[(size_t)k * P] - mu - b * b / dk;
        bad = bad || !(dk < 0.0);
    }
    dev_ql_rows<false>(j, G, d, e, z, nullptr);
    double tm = d[0], lo = 0.0;
    for (int k = 0; k < j; ++k) {
        tm = fmax(tm, d[k * G]);
        lo += z[k * G] * z[k * G] * exp(d[k * G] - mu);
    }
    const double bj = low[(size_t)(j - 1) * P];
    double hi = lo;
    int kind = 0;
    if (bj < 1e-8) {
        kind = 1;
    } else if (bad || tm > mu) {
        kind = 2;
        hi = NAN;
    } else {
        d[0] = al[0];
        for (int k = 1; k < j; ++k) {
            e[(k - 1) * G] = 0.5 * (low[(size_t)(k - 1) * P] + up[(size_t)k * P]);
            d[k * G] = al[(size_t)k * P];
        }
        e[(j - 1) * G] = bj;
        d[j * G] = mu + bj * bj / dk;
        dev_ql_rows<false>(j + 1, G, d, e, z, nullptr);
        hi = 0.0;
        for (int k = 0; k <= j; ++k) hi += z[k * G] * z[k * G] * exp(d[k * G] - mu);
    }
    *plo = lo;
    *phi = hi;
    return kind;
}

// The stopping test of a bracket column at depth j (kt_slq.cpp
// lanczos_nodes_bracket): k_node_check's launch shape and state block -- one
// wavefront, lane t owns column c = g0 + t (t < G, c < live), LDS arrays
// [k][lane] with stride G.  With T_j the record's leading j x j tridiagonal of
// the sweep started at e_i, beta_j = low[j-1] and mu >= lambda_max(A):
//   L_j = sum z_k^2 exp(theta_k - mu) over the eigenpairs of T_j (Gauss),
//   U_j = the same sum over T_j bordered by beta_j with last diagonal entry
//         mu + beta_j^2 / d_j (Gauss-Radau, a node at mu),
// d the pivots of T_j - mu I, run in registers.  Two dev_ql_rows<false> runs on
// three LDS arrays of depth j + 1 (d, e, z).  state: kAdaptState doubles per
// column, zeroed before the sweep's first check,
//   [0] L_j  [1] U_j (both scaled by exp(-mu))  [3] depth  [4] stopped
//   [6] flag  [7] the depth of the last check
// The column stops with flag 1 when beta_j < 1e-8 (U := L), else with flag 2
// when a pivot is not negative or a Ritz value lies above mu (U := NaN), else
// with flag 0 when U_j - L_j <= rtol L_j, else with flag 3 at j = mcap.  A
// stopped column is left as it is.  active[0]: as k_quad_check's.
__global__ __launch_bounds__(64) void k_bracket_check(const double* __restrict__ trec, int mcap, int P, int j,
                                                      int live, int g0, int G, double mu, double rtol,
                                                      double* __restrict__ state, int* __restrict__ active) {
    extern __shared__ double sm[];
    __shared__ int stopped_l[64];
    const int t = threadIdx.x, c = g0 + t;
    const bool mine = t < G && c < live;
    int stopped = -1;
    if (mine) {
        double* st = state + (size_t)c * kAdaptState;
        stopped = st[4] != 0.0;
        if (!stopped) {
            double lo, hi;
            const int kind = dev_bracket_column(trec, mcap, P, j, c, t, G, mu, sm, &lo, &hi);
            int flag = kind ? kind : -1;
            if (!kind) {
                if (hi - lo <= rtol * lo)
                    flag = 0;
                else if (j == mcap)
                    flag = 3;
            }
            st[0] = lo;
            st[1] = hi;
            st[7] = (double)j;
            if (flag >= 0) {
                st[3] = (double)j;
                st[4] = 1.0;
                st[6] = (double)flag;
                stopped = 1;
            }
        }
    }
    stopped_l[t] = stopped;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < live; ++k) {
            const bool here = k >= g0 && k < g0 + G;  // another group's columns: an earlier launch wrote them
            run += here ? (stopped_l[k - g0] == 0) : (state[(size_t)k * kAdaptState + 4] == 0.0);
        }
        active[0] = run;
    }
}

// P <= 32 columns, 1 <= j <= mcap <= 256.  The three LDS arrays of depth j + 1
// take 24 (j + 1) G bytes: every live column in one launch while they fit 64 KB
// together with the kernel's static words (P = 16 up to depth 168), else column
// groups of 8 lanes per launch (48.2 KB at depth 256); each group's count is
// taken over all live columns.
hipError_t launch_bracket_check(const double* trec, int mcap, int P, int j, int live, double mu, double rtol,
                                double* state, int* active, hipStream_t st) {
    if (P < 1 || P > 32 || live < 1 || live > P || j < 1 || j > mcap || mcap > 256) return hipErrorInvalidValue;
    const size_t room = (size_t)65536 - 512;
    const size_t per_lane = sizeof(double) * 3 * (size_t)(j + 1);
    const int G = (per_lane * P <= room) ? P : 8;
    if (per_lane * G > room) return hipErrorInvalidValue;
    for (int g0 = 0; g0 < live; g0 += G) {
        k_bracket_check<<<1, 64, per_lane * G, st>>>(trec, mcap, P, j, live, g0, G, mu, rtol, state, active);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The stopping test of a pair's two bracket columns at depth j (DESIGN.md §4.2j;
// kt_slq.cpp lanczos_pairs_bracket): k_bracket_check's launch shape, LDS layout
// and state block.  Columns 2p and 2p + 1 are the Lanczos runs started at
// (e_i + e_j) / sqrt 2 and (e_i - e_j) / sqrt 2 of pair p; live, g0 and G are
// even, so both sit in one launch, in neighbouring lanes.  With L, U the Gauss
// and Gauss-Radau sums of the two columns (dev_bracket_column, scaled by
// exp(-mu)), lo = (L+ - U-) / 2 <= exp(A)_ij exp(-mu) <= hi = (U+ - L-) / 2.
// state per column:
//   [0] L  [1] U  [3] depth  [4] stopped  [5] the pair is decided
//   [6] flag: 1 while the column is frozen and its pair undecided, then the pair's
//   [7] the depth of the column's last check
// A column whose beta_j < 1e-8 is frozen at j (stopped, U := L, its depth and
// sums kept) while the other one runs on.  Then, in this order: flag 2 when a
// running column proves mu below lambda_max, 1 when both are frozen, 0 when
// lo hi > 0 and 0 <= hi - lo <= rtol min(|lo|, |hi|), 4 when hi - lo <= ftol
// (U+ + U-) / 2, the rounding level of the two sums (an inverted bracket too), 3
// at j = mcap.  A decided pair stops its running columns at j and is left as it
// is from then on.  The lanes hand their sums over through the QL arrays'
// first 3 G words once every lane is done with them.  active[0]: as
// k_quad_check's.
__global__ __launch_bounds__(64) void k_pair_bracket_check(const double* __restrict__ trec, int mcap, int P, int j,
                                                           int live, int g0, int G, double mu, double rtol,
                                                           double ftol, double* __restrict__ state,
                                                           int* __restrict__ active) {
    extern __shared__ double sm[];
    __shared__ int stopped_l[64];
    const int t = threadIdx.x, c = g0 + t;
    const bool mine = t < G && c < live;
    double* st = state + (size_t)(mine ? c : 0) * kAdaptState;
    int kind = -1;  // -1: no column here, or its pair is decided; 0 a bracket; 1 frozen; 2 mu too small
    double lo = 0.0, hi = 0.0;
    if (mine && st[5] == 0.0) {
        if (st[4] != 0.0) {
            kind = 1;
            lo = st[0];
            hi = st[1];
        } else {
            kind = dev_bracket_column(trec, mcap, P, j, c, t, G, mu, sm, &lo, &hi);
            st[0] = lo;
            st[1] = hi;
            st[7] = (double)j;
            if (kind == 1) {
                st[3] = (double)j;
                st[4] = 1.0;
                st[6] = 1.0;
            }
        }
    }
    __syncthreads();  // every lane is done with its QL arrays
    if (t < G) {
        sm[t] = lo;
        sm[G + t] = hi;
        sm[2 * G + t] = (double)kind;
    }
    __syncthreads();
    int stopped = -1;
    if (mine) {
        if (kind >= 0) {
            const int a = t & ~1;  // the pair's + column; a + 1 < G: g0, G and live are even
            const double Lp = sm[a], Up = sm[G + a], Lm = sm[a + 1], Um = sm[G + a + 1];
            const int kp = (int)sm[2 * G + a], km = (int)sm[2 * G + a + 1];
            int flag = -1;
            if (kp == 2 || km == 2) {
                flag = 2;
            } else if (kp == 1 && km == 1) {
                flag = 1;
            } else {
                const double plo = 0.5 * (Lp - Um), phi = 0.5 * (Up - Lm), gap = phi - plo;
                if (plo * phi > 0.0 && gap >= 0.0 && gap <= rtol * fmin(fabs(plo), fabs(phi)))
                    flag = 0;
                else if (gap <= ftol * (0.5 * (Up + Um)))
                    flag = 4;
                else if (j == mcap)
                    flag = 3;
            }
            if (flag >= 0) {
                st[5] = 1.0;
                st[6] = (double)flag;
                if (st[4] == 0.0) {
                    st[3] = (double)j;
                    st[4] = 1.0;
                }
            }
        }
        stopped = st[4] != 0.0;
    }
    stopped_l[t] = stopped;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < live; ++k) {
            const bool here = k >= g0 && k < g0 + G;  // another group's columns: an earlier launch wrote them
            run += here ? (stopped_l[k - g0] == 0) : (state[(size_t)k * kAdaptState + 4] == 0.0);
        }
        active[0] = run;
    }
}

// launch_bracket_check's shapes and groups, P and live even: G = P or 8, so a
// group holds whole pairs.
hipError_t launch_pair_bracket_check(const double* trec, int mcap, int P, int j, int live, double mu, double rtol,
                                     double ftol, double* state, int* active, hipStream_t st) {
    if (P < 2 || P > 32 || (P & 1) || live < 2 || live > P || (live & 1) || j < 1 || j > mcap || mcap > 256)
        return hipErrorInvalidValue;
    const size_t room = (size_t)65536 - 512;
    const size_t per_lane = sizeof(double) * 3 * (size_t)(j + 1);
    const int G = (per_lane * P <= room) ? P : 8;
    if (per_lane * G > room) return hipErrorInvalidValue;
    for (int g0 = 0; g0 < live; g0 += G) {
        k_pair_bracket_check<<<1, 64, per_lane * G, st>>>(trec, mcap, P, j, live, g0, G, mu, rtol, ftol, state,
                                                          active);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The start of a node-removal sweep: column c < nc of the zeroed n x P block X
// gets 1 at row pos[c] (the candidate's row in the sweep's row order; duplicate
// rows are legal, each in its own column), and the sweep's start scale and
// squared norm (sc, k2s: P each) are 1 for those columns, 0 for the padding.
__global__ __launch_bounds__(64) void k_unit_start(int n, int P, int nc, const int* __restrict__ pos,
                                                   double* __restrict__ X, double* __restrict__ sc,
                                                   double* __restrict__ k2s) {
    const int c = threadIdx.x;
    if (c >= P) return;
    const int r = c < nc ? pos[c] : -1;
    const bool ok = r >= 0 && r < n;
    if (ok) X[(size_t)r * P + c] = 1.0;
    sc[c] = ok ? 1.0 : 0.0;
    k2s[c] = ok ? 1.0 : 0.0;
}

hipError_t launch_unit_start(int n, int P, int nc, const int* pos, double* X, double* sc, double* k2s,
                             hipStream_t st) {
    if (n < 1 || P < 1 || P > 64 || nc < 0 || nc > P) return hipErrorInvalidValue;
    k_unit_start<<<1, 64, 0, st>>>(n, P, nc, pos, X, sc, k2s);
    return hipGetLastError();
}

// The start of a pair sweep: pair p < np of the zeroed n x P
// block X gets e_i + e_j in column 2p and e_i - e_j in column 2p + 1, i =
// pos[2p], j = pos[2p + 1] the pair's rows in the sweep's row order (i != j;
// repeated pairs are legal, each in its own two columns).  The start scale is
// 1 / sqrt 2 and the squared norm 2 for those columns, 0 for the padding.
__global__ __launch_bounds__(64) void k_pair_start(int n, int P, int np, const int* __restrict__ pos,
                                                   double* __restrict__ X, double* __restrict__ sc,
                                                   double* __restrict__ k2s) {
    const int c = threadIdx.x;
    if (c >= P) return;
    const int p = c >> 1;
    const int ri = p < np ? pos[2 * p] : -1, rj = p < np ? pos[2 * p + 1] : -1;
    const bool ok = ri >= 0 && ri < n && rj >= 0 && rj < n && ri != rj;
    if (ok) {
        X[(size_t)ri * P + c] = 1.0;
        X[(size_t)rj * P + c] = (c & 1) ? -1.0 : 1.0;
    }
    sc[c] = ok ? 0.70710678118654752440 : 0.0;
    k2s[c] = ok ? 2.0 : 0.0;
}

hipError_t launch_pair_start(int n, int P, int np, const int* pos, double* X, double* sc, double* k2s,
                             hipStream_t st) {
    if (n < 2 || P < 2 || P > 64 || (P & 1) || np < 0 || 2 * np > P) return hipErrorInvalidValue;
    k_pair_start<<<1, 64, 0, st>>>(n, P, np, pos, X, sc, k2s);
    return hipGetLastError();
}

// Y[r, c] = sum_{j < m} U_j[r * nc + c] W[j * nc + c], slot j (n x nc,
// row-major) at tab.chunk[j / spc] + (j % spc) n nc: k_weighted_sum over a
// basis allocated in growth chunks of spc slots.
__global__ __launch_bounds__(256) void k_weighted_sum_tab(int n, int m, int nc, SlotTab tab, int spc,
                                                          const double* __restrict__ W, double* __restrict__ Y,
                                                          int ldy) {
    const int64_t total = (int64_t)n * nc;
    const int64_t sstride = (int64_t)n * nc;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / nc;
        const int c = (int)(t % nc);
        double s = 0.0;
        for (int j = 0; j < m; ++j) {
            const double* u = tab.chunk[j / spc] + (int64_t)(j % spc) * sstride + t;
            s = fma(__builtin_nontemporal_load(u), W[j * nc + c], s);
        }
        Y[r * ldy + c] = s;
    }
}

hipError_t launch_weighted_sum_tab(int n, int m, int nc, const SlotTab& tab, int spc, const double* W, double* Y,
                                   int ldy, hipStream_t st) {
    if (spc < 1 || m < 1 || (m + spc - 1) / spc > kSlotTabChunks) return hipErrorInvalidValue;
    const int64_t total = (int64_t)n * nc;
    int grid = (int)std::min<int64_t>((total + 255) / 256, 4096);
    if (grid < 1) grid = 1;
    k_weighted_sum_tab<<<grid, 256, 0, st>>>(n, m, nc, tab, spc, W, Y, ldy);
    return hipGetLastError();
}

}  // namespace kt
