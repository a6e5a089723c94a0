// miobi_node_check -- TEST INFRASTRUCTURE: the break-node launchers of
// kt_miobi.hip (kt_miobi_break_node's kernels) called one by one against host
// loops.  Prints one JSON line:
//   {"mode": "device"|"host", "max_score_err_over_bound": x, "groups": {"score":
//    {"cases": N, "failed_count": F, "failed": ["..."]}, "pick": ..., "apply":
//    ..., "colsum": ...}, "wall_s": s}
// plus "hip_error" when a HIP call failed (the run stops there).  Exit status
// 0: no failed case, 1: some, 2: HIP error.
//
//   miobi_node_check          the cases on the device
//   miobi_node_check --host   the same enumeration with plain host loops in
//                             place of the launches (the device test holds its
//                             case counts to this run's)
//
// A case is one score launch and one pick launch on a random CSR (rows of
// chosen lengths, no diagonal entry), a block V whose columns >= t are NaN
// (they must not reach a sum), alive bytes and a state {steps, stop, acc,
// window end}; where the pick sets the stop or the window-end word, a second
// pair of launches must write nothing.
// score   every row against long double sums; a dead row and a row without a
//         live neighbour +Inf exactly; the slot past the output keeps its
//         sentinel.  Within a column every entry of V has one sign, so a row's
//         sum W has no cancellation and the bound is rigorous: with x = -2 v W
//         the exp argument, relative error <= (max_k |x_k| (len + 3) + t + 8)
//         2^-53 per row -- len + 3 roundings of relative size 2^-53 reach x
//         (the len - 1 adds of W, the products v W and 2 v W, one spare), and
//         exp, the product with c and the five butterfly adds stay within t +
//         8.  Cases marked `grids` run under grids of 1, 2 and the maximum and
//         must give the same bits.
// pick    the selection is the first of (score ascending, node ascending) over
//         the finite scores, found on the host from the launch's own scores;
//         equal bits in different workgroups (short rows, and rows split over
//         a workgroup) go to the lower node under every grid; no finite score:
//         the stop word is set and nothing else changes
// apply   the selection record with the live degree, the alive byte (and no
//         other), the eigenvalue shift in either mode, c = exp(e), the track
//         row, the step count, the removed-entry count with its carry and the
//         window-end word; the no-op launches after either word
// colsum  the column sums of V over all rows against long double sums
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../../krylov_robustness_amd/csrc/kt_launch.h"

static const int LD = kt::kMiobiLd;

static bool g_host = false;
static const char* g_hip_err = nullptr;
static double g_max_ratio = 0.0;
static const double SENT = -7.7777e77;
static const double U53 = 1.1102230246251565e-16;  // 2^-53

struct Group {
    const char* name;
    int cases;
    std::vector<std::string> failed;
};
static Group g_groups[4] = {{"score", 0, {}}, {"pick", 0, {}}, {"apply", 0, {}}, {"colsum", 0, {}}};

static uint64_t g_rng = 88172645463325252ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static double runif(double a, double b) { return a + (b - a) * (double)(rnd() >> 11) / 9007199254740992.0; }

static bool hip_ok(hipError_t e) {
    if (e == hipSuccess) return true;
    if (!g_hip_err) g_hip_err = hipGetErrorString(e);
    return false;
}

// device copy of a host vector (host mode: the vector itself)
template <class T>
struct Buf {
    std::vector<T> h;
    T* d = nullptr;
    bool up() {
        if (g_host) {
            d = h.data();
            return true;
        }
        if (!d && !hip_ok(hipMalloc((void**)&d, sizeof(T) * h.size()))) return false;
        return hip_ok(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    }
    bool down() {
        if (g_host) return true;
        return hip_ok(hipDeviceSynchronize()) &&
               hip_ok(hipMemcpy(h.data(), d, sizeof(T) * h.size(), hipMemcpyDeviceToHost));
    }
    ~Buf() {
        if (!g_host && d) (void)hipFree(d);
    }
};

static bool before(double s1, int i1, double s2, int i2) {
    if (i1 < 0) return false;
    if (i2 < 0) return true;
    if (s1 != s2) return s1 < s2 || (s2 != s2 && s1 == s1);
    return i1 < i2;
}

// ---- host stand-ins -------------------------------------------------------
static hipError_t op_score(int n, int t, const double* V, const double* c, const int* rowptr, const int* col,
                           const unsigned char* alive, const int* long_rows, int n_long, double* score, int nblocks,
                           double* ps, int* pn, int* pd, const int* state) {
    if (!g_host)
        return kt::launch_miobi_node_score(n, t, V, c, rowptr, col, alive, long_rows, n_long, score, nblocks, ps, pn, pd,
                                           state, nullptr);
    if (state && (state[1] || state[3])) return hipSuccess;
    for (int b = 0; b < nblocks; ++b) ps[b] = 0.0, pn[b] = -1, pd[b] = 0;
    for (int r = 0; r < n; ++r) {
        int cnt = 0;
        double s = 0.0;
        if (alive[r]) {
            double w[32] = {0.0};
            for (int q = rowptr[r]; q < rowptr[r + 1]; ++q)
                if (alive[col[q]]) {
                    ++cnt;
                    for (int k = 0; k < t; ++k) w[k] += V[(size_t)col[q] * LD + k];
                }
            for (int k = 0; k < t; ++k) s += c[k] * exp(-2.0 * (V[(size_t)r * LD + k] * w[k]));
        }
        if (cnt == 0) s = std::numeric_limits<double>::infinity();
        if (score) score[r] = s;
        if (cnt > 0 && !std::isinf(s) && before(s, r, ps[0], pn[0])) ps[0] = s, pn[0] = r, pd[0] = cnt;
    }
    return hipSuccess;
}

static hipError_t op_pick(int nparts, const double* ps, const int* pn, const int* pd, int t, int shift, int refresh,
                          const double* V, const int* rowptr, const int* col, unsigned char* alive, double* e,
                          double* c, const double* colsum, int* sn, double* ss, int* sd, double* track, int* state) {
    if (!g_host)
        return kt::launch_miobi_node_pick(nparts, ps, pn, pd, t, shift, refresh, V, rowptr, col, alive, e, c, colsum, sn,
                                          ss, sd, track, state, nullptr);
    if (state[1] || state[3]) return hipSuccess;
    double bs = 0.0;
    int bi = -1, bd = 0;
    for (int b = 0; b < nparts; ++b)
        if (before(ps[b], pn[b], bs, bi)) bs = ps[b], bi = pn[b], bd = pd[b];
    if (bi < 0) {
        state[1] = 1;
        return hipSuccess;
    }
    const int step = state[0];
    for (int k = 0; k < t; ++k) {
        const double v = V[(size_t)bi * LD + k];
        double de;
        if (shift) {
            double w = 0.0;
            for (int q = rowptr[bi]; q < rowptr[bi + 1]; ++q)
                if (alive[col[q]]) w += V[(size_t)col[q] * LD + k];
            de = -2.0 * (v * w);
        } else {
            de = -(2.0 * v * colsum[k] - v * v);
        }
        e[k] += de;
        c[k] = exp(e[k]);
        track[(size_t)(step + 1) * LD + k] = e[k];
    }
    sn[step] = bi;
    ss[step] = bs;
    sd[step] = bd;
    alive[bi] = 0;
    if (refresh > 0) {
        long long a = (long long)state[2] + 2LL * bd;
        if (a >= refresh) a %= refresh, state[3] = 1;
        state[2] = (int)a;
    }
    state[0] = step + 1;
    return hipSuccess;
}

static hipError_t op_colsum(int64_t n, const double* V, double* part, double* s) {
    if (!g_host) return kt::launch_miobi_colsum(n, V, part, s, nullptr);
    for (int k = 0; k < LD; ++k) {
        double a = 0.0;
        for (int64_t r = 0; r < n; ++r) a += V[(size_t)r * LD + k];
        s[k] = a;
    }
    return hipSuccess;
}

// ---- cases ----------------------------------------------------------------
static void report(int g, bool ok, const std::string& what) {
    g_groups[g].cases += 1;
    if (!ok) g_groups[g].failed.push_back(what);
}

enum { G_SMALL = 0, G_BIG = 1 };
enum { DEAD_NONE = 0, DEAD_SOME = 1, DEAD_ALL = 2 };
// ties: 0 none; 1: the short rows 40 and 340 carry the same neighbours and the same bits of V, below every other
// score; 2: the same for the split rows 8 and 350 (600 entries each)
struct Spec {
    int t, n, graph, dead, max_blocks, ties, shift, refresh, acc0;
    bool grids;
};

static const int kBigN = 700;
static const int kLens[] = {0, 1, kt::kMiobiNodeBatch - 1, kt::kMiobiNodeBatch, kt::kMiobiNodeBatch + 1,
                            kt::kMiobiNodeLong - 1, kt::kMiobiNodeLong, kt::kMiobiNodeLong + 1, 600,
                            8 * kt::kMiobiNodeChunk, 8 * kt::kMiobiNodeChunk + 1, 16};

// scores and the reduced selection of the first grid of a `grids` / ties family, for the bit comparison
static std::vector<double> g_ref_score;
static double g_ref_sel_s = 0.0;
static int g_ref_sel_n = -2;

static void random_row(int n, int r, int len, const std::vector<int>& avoid, std::vector<int>& out) {
    std::vector<char> used((size_t)n, 0);
    used[(size_t)r] = 1;
    for (int a : avoid) used[(size_t)a] = 1;
    out.clear();
    while ((int)out.size() < len) {
        const int c = (int)(rnd() % (uint64_t)n);
        if (used[(size_t)c]) continue;
        used[(size_t)c] = 1;
        out.push_back(c);
    }
    std::sort(out.begin(), out.end());
}

static bool run_case(const Spec& S, bool first_of_family) {
    const int t = S.t, n = S.n;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    Buf<double> V, E, Cc, Cs, Score, Ps, SelS, Track;
    Buf<int> Rp, Col, Lr, Pn, Pd, SelN, SelD, State;
    Buf<unsigned char> Al;
    // the graph
    const int ta = S.ties == 2 ? 8 : 40, tb = S.ties == 2 ? 350 : 340;
    std::vector<int> row, tie_row;
    Rp.h.assign((size_t)n + 1, 0);
    for (int r = 0; r < n; ++r) {
        int len = S.graph == G_SMALL ? (n > 1 ? (r * 7 + 3) % n : 0)
                                     : r < (int)(sizeof kLens / sizeof kLens[0]) ? kLens[r] : (int)(rnd() % 24);
        if (S.graph == G_BIG && r == 20) len = 5;
        if (S.ties && (r == ta || r == tb)) {
            if (r == ta) random_row(n, ta, S.ties == 2 ? 600 : 40, {tb, 20}, tie_row);
            row = tie_row;
        } else {
            random_row(n, r, len, S.ties ? std::vector<int>{ta, tb} : std::vector<int>{}, row);
        }
        Col.h.insert(Col.h.end(), row.begin(), row.end());
        Rp.h[(size_t)r + 1] = (int)Col.h.size();
    }
    if (Col.h.empty()) Col.h.push_back(0);  // (never read: every row is empty)
    for (int r = 0; r < n; ++r)
        if (Rp.h[(size_t)r + 1] - Rp.h[(size_t)r] > kt::kMiobiNodeLong) Lr.h.push_back(r);
    const int n_long = (int)Lr.h.size();
    if (Lr.h.empty()) Lr.h.push_back(0);
    // V: one sign per column, magnitudes in (0, 0.1); columns >= t NaN
    V.h.assign((size_t)n * LD, nan);
    for (int r = 0; r < n; ++r)
        for (int k = 0; k < t; ++k) V.h[(size_t)r * LD + k] = (k % 3 == 1 ? -1.0 : 1.0) * runif(1e-3, 0.1);
    if (S.ties) {
        for (int k = 0; k < t; ++k) V.h[(size_t)ta * LD + k] = V.h[(size_t)tb * LD + k] = (k % 3 == 1 ? -3.0 : 3.0) - 0.01 * k;
        for (int c : tie_row)
            for (int k = 0; k < t; ++k) V.h[(size_t)c * LD + k] = (k % 3 == 1 ? -0.1 : 0.1);
    }
    Al.h.assign((size_t)n, 1);
    if (S.dead == DEAD_ALL) std::fill(Al.h.begin(), Al.h.end(), 0);
    if (S.dead == DEAD_SOME) {
        for (int r = 0; r < n; ++r)
            if (rnd() % 4 == 0 && !(S.ties && (r == ta || r == tb))) Al.h[(size_t)r] = 0;
        if (S.graph == G_BIG) {  // row 20 stays alive, every neighbour of it dies: +Inf
            Al.h[20] = 1;
            for (int q = Rp.h[20]; q < Rp.h[21]; ++q) Al.h[(size_t)Col.h[(size_t)q]] = 0;
        }
    }
    E.h.assign(LD, 0.0);
    Cc.h.assign(LD, 0.0);
    Cs.h.assign(LD, nan);
    for (int k = 0; k < t; ++k) {
        E.h[k] = runif(-1.0, 4.0) - 0.07 * k;
        Cc.h[k] = exp(E.h[k]);
        Cs.h[k] = runif(-30.0, 30.0);
    }
    const int nblocks = kt::miobi_node_blocks(n, S.max_blocks);
    Score.h.assign((size_t)n + 1, SENT);
    Ps.h.assign((size_t)nblocks, SENT);
    Pn.h.assign((size_t)nblocks, -7);
    Pd.h.assign((size_t)nblocks, -7);
    SelN.h.assign(4, -1);
    SelD.h.assign(4, -1);
    SelS.h.assign(4, SENT);
    Track.h.assign((size_t)LD * 5, SENT);
    const int step0 = 2;
    State.h = {step0, 0, S.acc0, 0};
    const std::vector<double> e0 = E.h, c0 = Cc.h;
    const std::vector<unsigned char> al0 = Al.h;
    if (!V.up() || !E.up() || !Cc.up() || !Cs.up() || !Score.up() || !Ps.up() || !SelS.up() || !Track.up() || !Rp.up() ||
        !Col.up() || !Lr.up() || !Pn.up() || !Pd.up() || !SelN.up() || !SelD.up() || !State.up() || !Al.up())
        return false;
    if (!hip_ok(op_score(n, t, V.d, Cc.d, Rp.d, Col.d, Al.d, Lr.d, n_long, Score.d, nblocks, Ps.d, Pn.d, Pd.d, State.d)))
        return false;
    if (!hip_ok(op_pick(nblocks, Ps.d, Pn.d, Pd.d, t, S.shift, S.refresh, V.d, Rp.d, Col.d, Al.d, E.d, Cc.d, Cs.d, SelN.d,
                        SelS.d, SelD.d, Track.d, State.d)))
        return false;
    if (!Score.down() || !E.down() || !Cc.down() || !SelS.down() || !Track.down() || !SelN.down() || !SelD.down() ||
        !State.down() || !Al.down())
        return false;
    char tag[240];
    snprintf(tag, sizeof tag, "t=%d n=%d graph=%d dead=%d max_blocks=%d ties=%d shift=%d refresh=%d acc0=%d", t, n,
             S.graph, S.dead, S.max_blocks, S.ties, S.shift, S.refresh, S.acc0);

    // score
    bool ok = Score.h[(size_t)n] == SENT;
    double bs = 0.0;
    int bi = -1;
    std::vector<int> live_deg((size_t)n, 0);
    for (int r = 0; r < n; ++r) {
        const double got = Score.h[(size_t)r];
        const int len = Rp.h[(size_t)r + 1] - Rp.h[(size_t)r];
        long double w[32] = {0.0L};
        int cnt = 0;
        if (al0[(size_t)r])
            for (int q = Rp.h[(size_t)r]; q < Rp.h[(size_t)r + 1]; ++q) {
                const int c = Col.h[(size_t)q];
                if (!al0[(size_t)c]) continue;
                ++cnt;
                for (int k = 0; k < t; ++k) w[k] += (long double)V.h[(size_t)c * LD + k];
            }
        live_deg[(size_t)r] = cnt;
        if (cnt == 0) {
            ok = ok && got == inf;
            continue;
        }
        long double s = 0.0L, xmax = 0.0L;
        for (int k = 0; k < t; ++k) {
            const long double x = -2.0L * (long double)V.h[(size_t)r * LD + k] * w[k];
            xmax = std::max(xmax, fabsl(x));
            s += (long double)c0[k] * expl(x);
        }
        const double bound = ((double)xmax * (len + 3) + t + 8) * U53;
        const double rel = (double)(fabsl((long double)got - s) / fabsl(s));
        if (!(rel <= bound)) ok = false;
        const double ratio = rel == rel ? rel / bound : inf;
        if (ratio > g_max_ratio) g_max_ratio = ratio;
        if (!std::isinf(got) && before(got, r, bs, bi)) bs = got, bi = r;
    }
    if (S.graph == G_BIG && S.dead == DEAD_SOME) ok = ok && Score.h[20] == inf && al0[20] == 1;
    if (S.grids || S.ties) {  // the same bits under every grid
        if (first_of_family) {
            g_ref_score = Score.h;
            g_ref_sel_s = bs;
            g_ref_sel_n = bi;
        } else {
            ok = ok && g_ref_score.size() == Score.h.size() &&
                 !memcmp(g_ref_score.data(), Score.h.data(), sizeof(double) * Score.h.size()) && g_ref_sel_n == bi &&
                 !memcmp(&g_ref_sel_s, &bs, sizeof bs);
        }
    }
    report(0, ok, std::string("score ") + tag);

    // pick
    const bool stopped = bi < 0;
    if (stopped) {
        ok = State.h[1] == 1 && State.h[0] == step0 && State.h[2] == S.acc0 && State.h[3] == 0 && SelN.h[step0] == -1 &&
             SelS.h[step0] == SENT && SelD.h[step0] == -1 && E.h == e0 && Cc.h == c0 && Al.h == al0 &&
             Track.h[(size_t)LD * (step0 + 1)] == SENT;
        report(1, ok, std::string("pick (stop) ") + tag);
    } else {
        ok = State.h[1] == 0 && SelN.h[step0] == bi && SelS.h[step0] == Score.h[(size_t)bi] &&
             SelD.h[step0] == live_deg[(size_t)bi];
        if (S.ties) ok = ok && bi == ta && Score.h[(size_t)ta] == Score.h[(size_t)tb];
        report(1, ok, std::string("pick ") + tag);

        // apply
        ok = State.h[0] == step0 + 1 && SelN.h[step0 + 1] == -1 && SelN.h[step0 - 1] == -1 && SelD.h[step0 + 1] == -1 &&
             SelS.h[step0 + 1] == SENT;
        std::vector<unsigned char> al1 = al0;
        al1[(size_t)bi] = 0;
        ok = ok && Al.h == al1;
        const int deg = live_deg[(size_t)bi], len = Rp.h[(size_t)bi + 1] - Rp.h[(size_t)bi];
        int want_acc = S.acc0, want_end = 0;
        if (S.refresh > 0) {
            long long a = (long long)S.acc0 + 2LL * deg;
            if (a >= S.refresh) a %= S.refresh, want_end = 1;
            want_acc = (int)a;
        }
        ok = ok && State.h[2] == want_acc && State.h[3] == want_end;
        for (int q = 0; q < LD; ++q) {
            if (q < t) {
                const long double v = V.h[(size_t)bi * LD + q];
                long double de, mag;
                if (S.shift) {
                    long double w = 0.0L;
                    for (int p = Rp.h[(size_t)bi]; p < Rp.h[(size_t)bi + 1]; ++p)
                        if (al0[(size_t)Col.h[(size_t)p]]) w += (long double)V.h[(size_t)Col.h[(size_t)p] * LD + q];
                    de = -2.0L * v * w;
                    mag = fabsl(de) * (len + 3);
                } else {
                    de = -(2.0L * v * (long double)Cs.h[q] - v * v);
                    mag = 4.0L * (fabsl(2.0L * v * (long double)Cs.h[q]) + v * v);
                }
                const double tol = (double)(mag + 2.0L * (fabsl((long double)e0[q]) + fabsl(de))) * U53;
                ok = ok && fabs(E.h[q] - (double)((long double)e0[q] + de)) <= tol &&
                     fabs(Cc.h[q] - exp(E.h[q])) <= 1e-14 * exp(E.h[q]) && Track.h[(size_t)LD * (step0 + 1) + q] == E.h[q];
            } else {
                ok = ok && E.h[q] == 0.0 && Cc.h[q] == 0.0 && Track.h[(size_t)LD * (step0 + 1) + q] == SENT;
            }
        }
        ok = ok && Track.h[(size_t)LD * step0] == SENT && Track.h[(size_t)LD * (step0 + 2)] == SENT;
        report(2, ok, std::string("apply ") + tag);
    }

    // after the stop or the window-end word a further score + pick writes nothing
    if (State.h[1] || State.h[3]) {
        const std::vector<int> st1 = State.h, sn1 = SelN.h;
        const std::vector<double> e1 = E.h, c1 = Cc.h, tr1 = Track.h;
        const std::vector<unsigned char> al1 = Al.h;
        std::fill(Ps.h.begin(), Ps.h.end(), SENT);
        std::fill(Pn.h.begin(), Pn.h.end(), -7);
        std::fill(Pd.h.begin(), Pd.h.end(), -7);
        std::fill(Score.h.begin(), Score.h.end(), SENT);
        if (!Ps.up() || !Pn.up() || !Pd.up() || !Score.up()) return false;
        if (!hip_ok(op_score(n, t, V.d, Cc.d, Rp.d, Col.d, Al.d, Lr.d, n_long, Score.d, nblocks, Ps.d, Pn.d, Pd.d, State.d)))
            return false;
        if (!hip_ok(op_pick(nblocks, Ps.d, Pn.d, Pd.d, t, S.shift, S.refresh, V.d, Rp.d, Col.d, Al.d, E.d, Cc.d, Cs.d,
                            SelN.d, SelS.d, SelD.d, Track.d, State.d)))
            return false;
        if (!Score.down() || !Ps.down() || !Pn.down() || !Pd.down() || !E.down() || !Cc.down() || !Track.down() ||
            !SelN.down() || !State.down() || !Al.down())
            return false;
        ok = State.h == st1 && SelN.h == sn1 && E.h == e1 && Cc.h == c1 && Track.h == tr1 && Al.h == al1;
        for (double x : Ps.h) ok = ok && x == SENT;
        for (int x : Pn.h) ok = ok && x == -7;
        for (double x : Score.h) ok = ok && x == SENT;
        report(2, ok, std::string("apply (no-op after a word) ") + tag);
    }
    return true;
}

static bool run_colsum(int64_t n) {
    Buf<double> V, Part, S;
    V.h.resize((size_t)n * LD);
    for (double& x : V.h) x = runif(-1.0, 1.0);
    Part.h.assign((size_t)LD * 256, SENT);
    S.h.assign((size_t)LD + 1, SENT);
    if (!V.up() || !Part.up() || !S.up()) return false;
    if (!hip_ok(op_colsum(n, V.d, Part.d, S.d))) return false;
    if (!S.down()) return false;
    bool ok = S.h[(size_t)LD] == SENT;
    for (int k = 0; k < LD; ++k) {
        long double s = 0.0L, a = 0.0L;
        for (int64_t r = 0; r < n; ++r) s += (long double)V.h[(size_t)r * LD + k], a += fabsl((long double)V.h[(size_t)r * LD + k]);
        ok = ok && fabs(S.h[(size_t)k] - (double)s) <= (double)(a * (long double)n) * U53 + 1e-300;
    }
    char tag[64];
    snprintf(tag, sizeof tag, "colsum n=%lld", (long long)n);
    report(3, ok, tag);
    return true;
}

static bool run_all() {
    const int ts[] = {2, 3, 16, 17, 31, 32};
    const int ns[] = {1, 63, 64, 65};
    int q = 0;
    for (int t : ts)
        for (int n : ns) {
            Spec S = {t, n, G_SMALL, q % 3 == 1 ? DEAD_SOME : DEAD_NONE, q % 5 == 4 ? 2 : 0, 0, q % 2, q % 4 == 3 ? 0 : 50,
                      q % 7, false};
            if (!run_case(S, false)) return false;
            ++q;
        }
    const int B = kBigN;
    const Spec extra[] = {
        // rows of 0, 1, batch - 1 / batch / batch + 1, threshold - 1 / threshold / threshold + 1, 600 (more than a
        // workgroup's trip of 512), 512 and 513 entries; no dead node, then dead neighbours and an all-dead row
        {25, B, G_BIG, DEAD_NONE, 0, 0, 0, 50, 0, false},
        {25, B, G_BIG, DEAD_SOME, 0, 0, 1, 50, 48, false},
        {17, B, G_BIG, DEAD_SOME, 2, 0, 0, 0, 7, false},
        {32, B, G_BIG, DEAD_SOME, 1, 0, 1, 1000000, 5, false},
        {2, B, G_BIG, DEAD_NONE, 0, 0, 1, 3, 2, false},
        {31, B, G_BIG, DEAD_SOME, 3, 0, 0, 50, 49, false},
    };
    for (const Spec& S : extra)
        if (!run_case(S, false)) return false;
    // grids of 1, 2 and the maximum: the same bits (each family restarts the generator, so its cases share their data)
    const Spec fam[][3] = {
        {{25, B, G_BIG, DEAD_SOME, 1, 0, 1, 50, 0, true}, {25, B, G_BIG, DEAD_SOME, 2, 0, 1, 50, 0, true},
         {25, B, G_BIG, DEAD_SOME, 0, 0, 1, 50, 0, true}},
        // equal scores in different workgroups: short rows, then rows split over a workgroup; the carry of acc
        {{25, B, G_BIG, DEAD_SOME, 1, 1, 0, 50, 49, false}, {25, B, G_BIG, DEAD_SOME, 2, 1, 0, 50, 49, false},
         {25, B, G_BIG, DEAD_SOME, 0, 1, 0, 50, 49, false}},
        {{17, B, G_BIG, DEAD_NONE, 1, 2, 1, 50, 0, false}, {17, B, G_BIG, DEAD_NONE, 2, 2, 1, 50, 0, false},
         {17, B, G_BIG, DEAD_NONE, 0, 2, 1, 50, 0, false}},
    };
    for (const auto& f : fam) {
        const uint64_t seed = g_rng;
        for (int i = 0; i < 3; ++i) {
            g_rng = seed;
            if (!run_case(f[i], i == 0)) return false;
        }
    }
    // every node dead: the stop word and nothing else, then no-op launches
    const Spec dead[] = {{25, B, G_BIG, DEAD_ALL, 0, 0, 0, 50, 3, false}, {2, B, G_BIG, DEAD_ALL, 2, 0, 1, 50, 3, false},
                         {16, 65, G_SMALL, DEAD_ALL, 0, 0, 0, 0, 0, false}};
    for (const Spec& S : dead)
        if (!run_case(S, false)) return false;
    for (int64_t n : {1, 63, 64, 65, 700, 20000})
        if (!run_colsum(n)) return false;
    return true;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--host")) g_host = true;
        else {
            fprintf(stderr, "usage: miobi_node_check [--host]\n");
            return 64;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    run_all();
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"mode\": \"%s\", ", g_host ? "host" : "device");
    if (g_hip_err) printf("\"hip_error\": \"%s\", ", g_hip_err);
    printf("\"max_score_err_over_bound\": %.3e, \"groups\": {", g_max_ratio);
    bool any = false;
    for (int g = 0; g < 4; ++g) {
        const Group& G = g_groups[g];
        printf("%s\"%s\": {\"cases\": %d, \"failed_count\": %d, \"failed\": [", g ? ", " : "", G.name, G.cases,
               (int)G.failed.size());
        for (size_t i = 0; i < G.failed.size() && i < 8; ++i) printf("%s\"%s\"", i ? ", " : "", G.failed[i].c_str());
        printf("]}");
        any = any || !G.failed.empty();
    }
    printf("}, \"wall_s\": %.3f}\n", wall);
    return g_hip_err ? 2 : any ? 1 : 0;
}
