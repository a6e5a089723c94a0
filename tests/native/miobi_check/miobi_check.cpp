// miobi_check -- TEST INFRASTRUCTURE: the launchers of kt_miobi.hip
// (kt_miobi_break's kernels) called one by one against host loops.  Prints one
// JSON line:
//   {"mode": "device"|"host", "max_score_rel_err": x, "groups": {"score":
//    {"cases": N, "failed_count": F, "failed": ["..."]}, "pick": ..., "apply":
//    ..., "norm": ...}, "wall_s": s}
// plus "hip_error" when a HIP call failed (the run stops there).  Exit status
// 0: no failed case, 1: some, 2: HIP error.
//
//   miobi_check          the cases on the device
//   miobi_check --host   the same enumeration with plain host loops in place of
//                        the launches (the device test holds its case counts
//                        to this run's)
//
// A case is one score launch and one pick launch on a random V (columns >= t
// NaN: they must not reach a sum), random dead pairs and, where asked, weights.
// score   every live pair's score against a long double sum to 1e-12 relative;
//         dead pairs and the slot past the list keep their sentinel
// pick    the selection is the minimum of (score, key (max, min), list index)
//         over the live pairs, found on the host from the launch's own scores;
//         all pairs dead: the stop word is set, nothing else changes, and a
//         further score + pick pair is a no-op
// apply   the selection record, alive byte, step count, e, c = exp(e), the
//         track row and (paper) M = I + S against the host formulas
// norm    launch_miobi_normalise: unit columns, column 0 non-negative, zero
//         columns stay zero, rows past n untouched, no-op under the stop word
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../../krylov_robustness_amd/csrc/kt_launch.h"

typedef unsigned long long u64;
static const int LD = kt::kMiobiLd;

static bool g_host = false;
static const char* g_hip_err = nullptr;
static double g_max_rel = 0.0;
static const double SENT = -7.7777e77;

struct Group {
    const char* name;
    int cases;
    std::vector<std::string> failed;
};
static Group g_groups[4] = {{"score", 0, {}}, {"pick", 0, {}}, {"apply", 0, {}}, {"norm", 0, {}}};

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
        return hip_ok(hipMalloc((void**)&d, sizeof(T) * h.size())) &&
               hip_ok(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
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

static u64 key_of(int i, int j) { return ((u64)(unsigned)std::max(i, j) << 32) | (unsigned)std::min(i, j); }

static bool before(double s1, u64 k1, int i1, double s2, u64 k2, int i2) {
    if (i1 < 0) return false;
    if (i2 < 0) return true;
    if (s1 != s2) return s1 < s2;
    if (k1 != k2) return k1 < k2;
    return i1 < i2;
}

// ---- host stand-ins -------------------------------------------------------
static hipError_t op_score(int64_t np, int t, const double* V, const double* c, const int* pi, const int* pj,
                           const unsigned char* alive, double sign, double* score, int nblocks, double* ps, u64* pk,
                           int* pidx, const int* stop) {
    if (!g_host) return kt::launch_miobi_score(np, t, V, c, pi, pj, alive, sign, score, nblocks, ps, pk, pidx, stop, nullptr);
    if (stop && *stop) return hipSuccess;
    for (int b = 0; b < nblocks; ++b) pidx[b] = -1, ps[b] = 0.0, pk[b] = 0;
    for (int64_t p = 0; p < np; ++p) {
        if (alive && !alive[p]) continue;
        double s = 0.0;
        for (int k = 0; k < t; ++k) s += c[k] * exp(sign * (V[(size_t)pi[p] * LD + k] * V[(size_t)pj[p] * LD + k]));
        if (score) score[p] = s;
        const int b = (int)((p / kt::kMiobiTilePairs) % nblocks);
        if (before(s, key_of(pi[p], pj[p]), (int)p, ps[b], pk[b], pidx[b])) ps[b] = s, pk[b] = key_of(pi[p], pj[p]), pidx[b] = (int)p;
    }
    return hipSuccess;
}

static hipError_t op_pick(int nparts, const double* ps, const u64* pk, const int* pidx, int t, int paper, double gap_rel,
                          const double* V, double* e, double* c, const int* pi, const int* pj, const double* wt,
                          unsigned char* alive, int* si, int* sj, double* ss, double* track, double* M, int* state) {
    if (!g_host)
        return kt::launch_miobi_pick(nparts, ps, pk, pidx, t, paper, gap_rel, V, e, c, pi, pj, wt, alive, si, sj, ss,
                                     track, M, state, nullptr);
    if (state[1]) return hipSuccess;
    double bs = 0.0;
    u64 bk = 0;
    int bi = -1;
    for (int b = 0; b < nparts; ++b)
        if (before(ps[b], pk[b], pidx[b], bs, bk, bi)) bs = ps[b], bk = pk[b], bi = pidx[b];
    if (bi < 0) {
        state[1] = 1;
        if (paper)
            for (int q = 0; q < LD * LD; ++q) M[q] = (q / LD == q % LD && q % LD < t) ? 1.0 : 0.0;
        return hipSuccess;
    }
    const int i = pi[bi], j = pj[bi], step = state[0];
    const double a = wt ? wt[bi] : 1.0;
    double eo[32], u[32], v[32];
    for (int k = 0; k < LD; ++k) {
        u[k] = k < t ? V[(size_t)i * LD + k] : 0.0;
        v[k] = k < t ? V[(size_t)j * LD + k] : 0.0;
        eo[k] = k < t ? e[k] : 0.0;
    }
    for (int k = 0; k < t; ++k) {
        e[k] = eo[k] + (-2.0 * a) * (u[k] * v[k]);
        c[k] = exp(e[k]);
        track[(size_t)(step + 1) * LD + k] = e[k];
    }
    si[step] = std::max(i, j);
    sj[step] = std::min(i, j);
    ss[step] = bs;
    alive[bi] = 0;
    state[0] = step + 1;
    if (paper)
        for (int r = 0; r < LD; ++r)
            for (int cc = 0; cc < LD; ++cc) {
                double m = 0.0;
                if (r < t && cc < t) {
                    const double d = eo[cc] - eo[r];
                    m = r == cc ? 1.0
                                : (d == 0.0 || fabs(d) <= gap_rel * fabs(eo[0])) ? 0.0
                                                                               : -a * (u[r] * v[cc] + v[r] * u[cc]) / d;
                }
                M[r * LD + cc] = m;
            }
    return hipSuccess;
}

static hipError_t op_norm(int64_t n, double* V, double* part, const int* state) {
    if (!g_host) return kt::launch_miobi_normalise(n, V, part, state, nullptr);
    if (state[1]) return hipSuccess;
    for (int k = 0; k < LD; ++k) {
        double s = 0.0;
        for (int64_t r = 0; r < n; ++r) s += V[r * LD + k] * V[r * LD + k];
        const double f = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
        for (int64_t r = 0; r < n; ++r) V[r * LD + k] = k == 0 ? fabs(V[r * LD + k] * f) : V[r * LD + k] * f;
    }
    return hipSuccess;
}

// ---- cases ----------------------------------------------------------------
static void report(int g, bool ok, const std::string& what) {
    g_groups[g].cases += 1;
    if (!ok) g_groups[g].failed.push_back(what);
}

enum { PLAIN = 0, ALL_DEAD = 1, TIES = 2, TIES_SWAPPED = 3 };

struct Spec {
    int t, npairs, kind, max_blocks;
    bool weights, paper, dead;
    double sign, gap_rel;
};

static bool close_rel(double a, double b, double tol) { return fabs(a - b) <= tol * std::max(fabs(a), fabs(b)); }

static bool run_case(const Spec& S) {
    const int n = 97, t = S.t, np = S.npairs;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Buf<double> V, E, Cc, W, Score, Ps, SelS, Track, M;
    Buf<int> Pi, Pj, Pidx, SelI, SelJ, State;
    Buf<u64> Pk;
    Buf<unsigned char> Alive;
    V.h.assign((size_t)n * LD, nan);
    for (int r = 0; r < n; ++r)
        for (int k = 0; k < t; ++k) V.h[(size_t)r * LD + k] = runif(-0.4, 0.4);
    E.h.assign(LD, 0.0);
    Cc.h.assign(LD, 0.0);
    for (int k = 0; k < t; ++k) {
        E.h[k] = runif(-1.0, 4.0) - 0.07 * k;
        Cc.h[k] = exp(E.h[k]);
    }
    Pi.h.resize(np + 1);
    Pj.h.resize(np + 1);
    W.h.resize(np + 1);
    Alive.h.assign(np + 1, 1);
    for (int p = 0; p <= np; ++p) {
        int i = 8 + (int)(rnd() % (uint64_t)(n - 8)), j = 8 + (int)(rnd() % (uint64_t)(n - 8));
        if (i == j) j = i == n - 1 ? 8 : i + 1;
        Pi.h[p] = i;
        Pj.h[p] = j;
        W.h[p] = S.weights ? runif(0.5, 1.5) : 1.0;
        if (S.dead && rnd() % 5 == 0) Alive.h[p] = 0;
    }
    if (S.kind == ALL_DEAD) std::fill(Alive.h.begin(), Alive.h.end(), (unsigned char)0);
    int want_i = -1, want_j = -1;
    if (S.kind == TIES || S.kind == TIES_SWAPPED) {
        // nodes 0..3 carry the two largest products: rows 2, 3 copy rows 0, 1, so the
        // pairs {0, 1} and {2, 3} score the same bits and below every other pair
        for (int k = 0; k < t; ++k) {
            V.h[0 * LD + k] = V.h[2 * LD + k] = 0.9;
            V.h[1 * LD + k] = V.h[3 * LD + k] = 0.8;
        }
        const int first = 0, last = np - 1;  // different workgroups once np > 64
        const int a = S.kind == TIES ? first : last, b = S.kind == TIES ? last : first;
        Pi.h[a] = 3, Pj.h[a] = 2;  // the larger key, stored (max, min)
        Pi.h[b] = 0, Pj.h[b] = 1;  // the smaller key, stored (min, max)
        Alive.h[a] = Alive.h[b] = 1;
        want_i = 1, want_j = 0;
    }
    const int nblocks = kt::miobi_score_blocks(np, S.max_blocks);
    Score.h.assign(np + 1, SENT);
    Ps.h.assign(nblocks, SENT);
    Pk.h.assign(nblocks, 0);
    Pidx.h.assign(nblocks, -7);
    SelI.h.assign(4, -1);
    SelJ.h.assign(4, -1);
    SelS.h.assign(4, SENT);
    Track.h.assign((size_t)LD * 5, SENT);
    M.h.assign((size_t)LD * LD, SENT);
    const int step0 = 2;
    State.h = {step0, 0};
    const std::vector<double> e0 = E.h, c0 = Cc.h;
    const std::vector<unsigned char> alive0 = Alive.h;
    if (!V.up() || !E.up() || !Cc.up() || !W.up() || !Score.up() || !Ps.up() || !SelS.up() || !Track.up() || !M.up() ||
        !Pi.up() || !Pj.up() || !Pidx.up() || !SelI.up() || !SelJ.up() || !State.up() || !Pk.up() || !Alive.up())
        return false;
    const double* wt = S.weights ? W.d : nullptr;
    const int rounds = S.kind == ALL_DEAD ? 2 : 1;  // the second pair must find the stop word and do nothing
    for (int rd = 0; rd < rounds; ++rd) {
        if (!hip_ok(op_score(np, t, V.d, Cc.d, Pi.d, Pj.d, Alive.d, S.sign, Score.d, nblocks, Ps.d, Pk.d, Pidx.d,
                             State.d + 1)))
            return false;
        if (!hip_ok(op_pick(nblocks, Ps.d, Pk.d, Pidx.d, t, S.paper ? 1 : 0, S.gap_rel, V.d, E.d, Cc.d, Pi.d, Pj.d, wt,
                            Alive.d, SelI.d, SelJ.d, SelS.d, Track.d, M.d, State.d)))
            return false;
    }
    if (!Score.down() || !E.down() || !Cc.down() || !SelS.down() || !Track.down() || !M.down() || !SelI.down() ||
        !SelJ.down() || !State.down() || !Alive.down())
        return false;
    char tag[200];
    snprintf(tag, sizeof tag, "t=%d npairs=%d kind=%d max_blocks=%d weights=%d paper=%d dead=%d sign=%g", t, np, S.kind,
             S.max_blocks, (int)S.weights, (int)S.paper, (int)S.dead, S.sign);

    // score
    bool ok = Score.h[np] == SENT;
    double bs = 0.0;
    u64 bk = 0;
    int bi = -1;
    for (int p = 0; p < np; ++p) {
        if (!alive0[p]) {
            ok = ok && Score.h[p] == SENT;
            continue;
        }
        long double s = 0.0L;
        for (int k = 0; k < t; ++k)
            s += expl((long double)e0[k]) *
                 expl((long double)S.sign * ((long double)V.h[(size_t)Pi.h[p] * LD + k] * (long double)V.h[(size_t)Pj.h[p] * LD + k]));
        const double rel = (double)(fabsl((long double)Score.h[p] - s) / fabsl(s));
        if (!(rel <= 1e-12)) ok = false;
        if (rel > g_max_rel || rel != rel) g_max_rel = rel;
        if (before(Score.h[p], key_of(Pi.h[p], Pj.h[p]), p, bs, bk, bi)) bs = Score.h[p], bk = key_of(Pi.h[p], Pj.h[p]), bi = p;
    }
    report(0, ok, std::string("score ") + tag);

    // pick
    if (bi < 0) {
        ok = State.h[1] == 1 && State.h[0] == step0 && SelI.h[step0] == -1 && SelS.h[step0] == SENT && E.h == e0 &&
             Cc.h == c0 && Alive.h == alive0 && Track.h[(size_t)LD * (step0 + 1)] == SENT;
        if (S.paper)
            for (int q = 0; q < LD * LD; ++q) ok = ok && M.h[q] == ((q / LD == q % LD && q % LD < t) ? 1.0 : 0.0);
        report(1, ok, std::string("pick (stop) ") + tag);
        return true;
    }
    ok = State.h[1] == 0 && SelI.h[step0] == std::max(Pi.h[bi], Pj.h[bi]) && SelJ.h[step0] == std::min(Pi.h[bi], Pj.h[bi]) &&
         SelS.h[step0] == Score.h[bi];
    if (want_i >= 0) ok = ok && SelI.h[step0] == want_i && SelJ.h[step0] == want_j;
    report(1, ok, std::string("pick ") + tag);

    // apply
    ok = State.h[0] == step0 + 1 && SelI.h[step0 + 1] == -1 && SelI.h[step0 - 1] == -1;
    for (int p = 0; p <= np; ++p) ok = ok && Alive.h[p] == (p == bi ? 0 : alive0[p]);
    const int i = Pi.h[bi], j = Pj.h[bi];
    const double a = S.weights ? W.h[bi] : 1.0;
    const double scale = fabs(e0[0]) + 2.0;
    for (int k = 0; k < LD; ++k) {
        if (k < t) {
            const double en = e0[k] - 2.0 * a * V.h[(size_t)i * LD + k] * V.h[(size_t)j * LD + k];
            ok = ok && fabs(E.h[k] - en) <= 4e-16 * scale && close_rel(Cc.h[k], exp(E.h[k]), 1e-14) &&
                 Track.h[(size_t)LD * (step0 + 1) + k] == E.h[k];
        } else {
            ok = ok && E.h[k] == 0.0 && Cc.h[k] == 0.0 && Track.h[(size_t)LD * (step0 + 1) + k] == SENT;
        }
    }
    ok = ok && Track.h[(size_t)LD * step0] == SENT && Track.h[(size_t)LD * (step0 + 2)] == SENT;
    if (S.paper) {
        for (int r = 0; r < LD; ++r)
            for (int cc = 0; cc < LD; ++cc) {
                double m = 0.0;
                if (r < t && cc < t) {
                    const double d = e0[cc] - e0[r];
                    const double dh = -a * (V.h[(size_t)i * LD + r] * V.h[(size_t)j * LD + cc] +
                                            V.h[(size_t)j * LD + r] * V.h[(size_t)i * LD + cc]);
                    m = r == cc ? 1.0 : (d == 0.0 || fabs(d) <= S.gap_rel * fabs(e0[0])) ? 0.0 : dh / d;
                }
                const double got = M.h[r * LD + cc];
                ok = ok && (m == 0.0 || m == 1.0 ? got == m : fabs(got - m) <= 1e-14 * fabs(m) + 1e-300);
            }
    } else {
        ok = ok && M.h[0] == SENT;
    }
    report(2, ok, std::string("apply ") + tag);
    return true;
}

static bool norm_case(int n, int t, int stop) {
    const int guard = 3;
    Buf<double> V, Part;
    Buf<int> State;
    V.h.assign((size_t)(n + guard) * LD, SENT);
    for (int r = 0; r < n; ++r)
        for (int k = 0; k < LD; ++k) V.h[(size_t)r * LD + k] = k < t ? runif(-1.0, 1.0) : 0.0;
    const std::vector<double> v0 = V.h;
    Part.h.assign((size_t)LD * kt::miobi_norm_blocks(n), SENT);
    State.h = {0, stop};
    if (!V.up() || !Part.up() || !State.up()) return false;
    if (!hip_ok(op_norm(n, V.d, Part.d, State.d)) || !V.down()) return false;
    bool ok = true;
    if (stop) {
        ok = V.h == v0;
    } else {
        for (int k = 0; k < LD; ++k) {
            long double s0 = 0.0L, s1 = 0.0L;
            for (int r = 0; r < n; ++r) s0 += (long double)v0[(size_t)r * LD + k] * v0[(size_t)r * LD + k];
            for (int r = 0; r < n; ++r) {
                const double x = V.h[(size_t)r * LD + k];
                s1 += (long double)x * x;
                const double want = k < t ? (double)(v0[(size_t)r * LD + k] / sqrtl(s0)) : 0.0;
                ok = ok && fabs(x - (k == 0 ? fabs(want) : want)) <= 1e-15;
            }
            ok = ok && (k < t ? fabsl(sqrtl(s1) - 1.0L) <= 1e-14L : s1 == 0.0L);
        }
        for (size_t q = (size_t)n * LD; q < V.h.size(); ++q) ok = ok && V.h[q] == SENT;
    }
    char buf[96];
    snprintf(buf, sizeof buf, "norm n=%d t=%d stop=%d", n, t, stop);
    report(3, ok, buf);
    return true;
}

static bool run_all() {
    const int ts[] = {2, 3, 16, 17, 31, 32};
    const int nps[] = {1, 2, 63, 64, 65, 40 * kt::kMiobiTilePairs};
    int q = 0;
    for (int t : ts)
        for (int np : nps) {
            Spec S = {t, np, PLAIN, 0, q % 2 == 1, q % 3 == 0, np > 2, q % 4 == 3 ? 2.0 : -2.0, q % 6 == 0 ? 0.05 : 0.0};
            if (!run_case(S)) return false;
            ++q;
        }
    // the grid-stride loop (7 workgroups over 40 tiles), all pairs dead, exact ties across workgroups
    const Spec extra[] = {
        {25, 40 * kt::kMiobiTilePairs, PLAIN, 7, true, true, true, -2.0, 0.0},
        {25, 40 * kt::kMiobiTilePairs + 1, PLAIN, 7, false, false, true, -2.0, 0.0},
        {25, 65, ALL_DEAD, 0, false, true, false, -2.0, 0.0},
        {3, 40 * kt::kMiobiTilePairs, ALL_DEAD, 0, true, false, false, -2.0, 0.0},
        {25, 40 * kt::kMiobiTilePairs, TIES, 0, false, false, true, -2.0, 0.0},
        {25, 40 * kt::kMiobiTilePairs, TIES_SWAPPED, 0, false, false, true, -2.0, 0.0},
        {17, 65, TIES, 0, true, true, false, -2.0, 0.0},
        {17, 2, TIES_SWAPPED, 0, false, false, false, -2.0, 0.0},
        {32, 40 * kt::kMiobiTilePairs, TIES_SWAPPED, 7, false, false, true, -2.0, 0.0},
    };
    for (const Spec& S : extra)
        if (!run_case(S)) return false;
    const int nn[] = {1, 63, 64, 65, 20000};
    for (int n : nn)
        if (!norm_case(n, n % 2 ? 25 : 32, 0)) return false;
    return norm_case(1000, 25, 1);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--host")) g_host = true;
        else {
            fprintf(stderr, "usage: miobi_check [--host]\n");
            return 64;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    run_all();
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"mode\": \"%s\", ", g_host ? "host" : "device");
    if (g_hip_err) printf("\"hip_error\": \"%s\", ", g_hip_err);
    printf("\"max_score_rel_err\": %.3e, \"groups\": {", g_max_rel);
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
