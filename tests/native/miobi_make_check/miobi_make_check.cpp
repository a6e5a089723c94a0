// miobi_make_check -- TEST INFRASTRUCTURE: the make-edge launchers of
// kt_miobi.hip (kt_miobi_make's kernels) called one by one against host loops.
// Prints one JSON line:
//   {"mode": "device"|"host", "max_score_rel_err": x, "groups": {"score":
//    {"cases": N, "failed_count": F, "failed": ["..."]}, "pick": ..., "apply":
//    ...}, "wall_s": s}
// plus "hip_error" when a HIP call failed (the run stops there).  Exit status
// 0: no failed case, 1: some, 2: HIP error.
//
//   miobi_make_check          the cases on the device
//   miobi_make_check --host   the same enumeration with plain host loops in
//                             place of the launches (the device test holds its
//                             case counts to this run's)
//
// A case is one score launch and one pick launch on a random candidate block W
// (columns >= t NaN: they must not reach a sum; rows at or beyond the live m
// carry the largest values of all: they must not be scored), a mask and a
// state {steps, stop, maxdeg, live m}.
// score   every pair a < b < m with a clear mask bit against a long double sum
//         to 1e-12 relative; every other slot of the m x m output, and the slot
//         past it, keeps its sentinel
// pick    the selection is the first of (score descending, key (a << 32) | b
//         ascending) over the scored pairs, found on the host from the launch's
//         own scores; where rows of W are bit-identical across tiles the
//         smaller (a, b) must win under every grid; no free pair: the stop word
//         is set, nothing else changes, and a further score + pick is a no-op
// apply   the selection record, both mask bits (and no other), degrees, maxdeg,
//         the next m (grown by one, unchanged, clamped at n), the m recorded
//         for the step, step count, e, c = exp(e) and the track row
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
static Group g_groups[3] = {{"score", 0, {}}, {"pick", 0, {}}, {"apply", 0, {}}};

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

static u64 key_of(int a, int b) { return ((u64)(unsigned)a << 32) | (unsigned)b; }

static bool before(double s1, u64 k1, int ok1, double s2, u64 k2, int ok2) {
    if (!ok1) return false;
    if (!ok2) return true;
    if (s1 != s2) return s1 > s2;
    return k1 < k2;
}

static bool bit(const std::vector<u64>& mask, int words, int a, int b) {
    return (mask[(size_t)a * words + (b >> 6)] >> (b & 63)) & 1ull;
}
static void set_bit(std::vector<u64>& mask, int words, int a, int b) {
    mask[(size_t)a * words + (b >> 6)] |= 1ull << (b & 63);
}

// ---- host stand-ins -------------------------------------------------------
static hipError_t op_score(int mcap, int t, const double* W, const double* c, const u64* mask, const int* state,
                           double* score, int nblocks, double* ps, u64* pk, int* po) {
    if (!g_host) return kt::launch_miobi_make_score(mcap, t, W, c, mask, state, score, nblocks, ps, pk, po, nullptr);
    if (state[1]) return hipSuccess;
    const int words = kt::miobi_make_words(mcap), m = std::min(state[3], mcap);
    for (int b = 0; b < nblocks; ++b) po[b] = 0, ps[b] = 0.0, pk[b] = 0;
    for (int a = 0; a < m; ++a)
        for (int b = a + 1; b < m; ++b) {
            if ((mask[(size_t)a * words + (b >> 6)] >> (b & 63)) & 1ull) continue;
            double s = 0.0;
            for (int k = 0; k < t; ++k) s = fma(c[k], exp(2.0 * (W[(size_t)a * LD + k] * W[(size_t)b * LD + k])), s);
            if (score) score[(size_t)a * mcap + b] = s;
            const int tr = a / kt::kMiobiMakeTile, tc = b / kt::kMiobiMakeTile, blk = (tc * (tc + 1) / 2 + tr) % nblocks;
            if (before(s, key_of(a, b), 1, ps[blk], pk[blk], po[blk])) ps[blk] = s, pk[blk] = key_of(a, b), po[blk] = 1;
        }
    return hipSuccess;
}

static hipError_t op_pick(int nparts, const double* ps, const u64* pk, const int* po, int mcap, int t, int k, int n,
                          const double* W, const int* node, double* e, double* c, u64* mask, int* deg, int* si,
                          int* sj, double* ss, double* track, int* cm, int* state) {
    if (!g_host)
        return kt::launch_miobi_make_pick(nparts, ps, pk, po, mcap, t, k, n, W, node, e, c, mask, deg, si, sj, ss,
                                          track, cm, state, nullptr);
    if (state[1]) return hipSuccess;
    double bs = 0.0;
    u64 bk = 0;
    int bo = 0;
    for (int b = 0; b < nparts; ++b)
        if (before(ps[b], pk[b], po[b], bs, bk, bo)) bs = ps[b], bk = pk[b], bo = 1;
    if (!bo) {
        state[1] = 1;
        return hipSuccess;
    }
    const int a = (int)(bk >> 32), b = (int)(bk & 0xffffffffull), step = state[0], words = kt::miobi_make_words(mcap);
    for (int q = 0; q < t; ++q) {
        e[q] = e[q] + 2.0 * (W[(size_t)a * LD + q] * W[(size_t)b * LD + q]);
        c[q] = exp(e[q]);
        track[(size_t)(step + 1) * LD + q] = e[q];
    }
    si[step] = std::max(node[a], node[b]);
    sj[step] = std::min(node[a], node[b]);
    ss[step] = bs;
    cm[step] = state[3];
    mask[(size_t)a * words + (b >> 6)] |= 1ull << (b & 63);
    mask[(size_t)b * words + (a >> 6)] |= 1ull << (a & 63);
    const int md = std::max(state[2], std::max(++deg[a], ++deg[b]));
    state[2] = md;
    state[3] = std::min(mcap, std::min(md + k, n));
    state[0] = step + 1;
    return hipSuccess;
}

// ---- cases ----------------------------------------------------------------
static void report(int g, bool ok, const std::string& what) {
    g_groups[g].cases += 1;
    if (!ok) g_groups[g].failed.push_back(what);
}

enum { M_EMPTY = 0, M_FULL = 1, M_RANDOM = 2, M_ONLY_FIRST = 3, M_ONLY_CORNER = 4 };
enum { D_PLAIN = 0, D_GROW = 1, D_CLAMP = 2 };  // what the pick does to m
// ties: 0 none; 1..4: ranks 69 and 73 carry the bits of ranks 0 and 1, so the pairs (0, 1), (0, 73), (1, 69)
// and (69, 73) score the same bits, above every other pair; the first ties - 1 of them are masked out
struct Spec {
    int t, mcap, m, mask_kind, max_blocks, ties, deg_kind;
};

static bool run_case(const Spec& S) {
    const int t = S.t, mcap = S.mcap, m = S.m, words = kt::miobi_make_words(mcap);
    const int n = S.deg_kind == D_CLAMP ? mcap : 211;  // 37 is coprime to both choices used here
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Buf<double> W, E, Cc, Score, Ps, SelS, Track;
    Buf<int> Node, Deg, Po, SelI, SelJ, Cm, State;
    Buf<u64> Pk, Mask;
    W.h.assign((size_t)mcap * LD, nan);
    for (int r = 0; r < mcap; ++r)
        for (int k = 0; k < t; ++k) W.h[(size_t)r * LD + k] = r < m ? runif(-0.4, 0.4) : 0.95;
    if (S.ties)
        for (int k = 0; k < t; ++k) {
            W.h[0 * LD + k] = W.h[69 * LD + k] = 0.9 - 0.001 * k;
            W.h[1 * LD + k] = W.h[73 * LD + k] = 0.8 + 0.002 * k;
        }
    E.h.assign(LD, 0.0);
    Cc.h.assign(LD, 0.0);
    for (int k = 0; k < t; ++k) {
        E.h[k] = runif(-1.0, 4.0) - 0.07 * k;
        Cc.h[k] = exp(E.h[k]);
    }
    Node.h.resize(mcap);
    for (int r = 0; r < mcap; ++r) Node.h[r] = (r * 37 + 11) % n;
    Mask.h.assign((size_t)mcap * words, 0);
    for (int a = 0; a < mcap; ++a)
        for (int b = a + 1; b < mcap; ++b) {
            bool adj = false;
            if (S.mask_kind == M_FULL) adj = true;
            if (S.mask_kind == M_RANDOM) adj = rnd() % 3 == 0;
            if (S.mask_kind == M_ONLY_FIRST) adj = !(a == 0 && b == 1);
            if (S.mask_kind == M_ONLY_CORNER) adj = !(a == m - 2 && b == m - 1);
            if (S.ties && (a == 0 || a == 1 || a == 69) && (b == 1 || b == 69 || b == 73))
                adj = (a == 0 && b == 69) || (a == 1 && b == 73);  // (these two score other bits, one of them more)
            if (adj) set_bit(Mask.h, words, a, b), set_bit(Mask.h, words, b, a);
        }
    int want_a = -1, want_b = -1;
    if (S.ties) {
        const int ta[] = {0, 0, 1, 69}, tb[] = {1, 73, 69, 73};
        for (int q = 0; q < S.ties - 1; ++q) set_bit(Mask.h, words, ta[q], tb[q]), set_bit(Mask.h, words, tb[q], ta[q]);
        want_a = ta[S.ties - 1], want_b = tb[S.ties - 1];
    }
    // the budget k makes maxdeg + k the live m; D_GROW: every degree is at the maximum, so the pick raises it
    const int maxdeg = m > 8 ? 7 : 1, k = m - maxdeg;
    Deg.h.resize(mcap);
    for (int r = 0; r < mcap; ++r) Deg.h[r] = S.deg_kind != D_PLAIN ? maxdeg : maxdeg == 7 ? 1 + (int)(rnd() % 5) : 0;
    const int nblocks = kt::miobi_make_blocks(mcap, S.max_blocks);
    Score.h.assign((size_t)mcap * mcap + 1, SENT);
    Ps.h.assign(nblocks, SENT);
    Pk.h.assign(nblocks, 0);
    Po.h.assign(nblocks, -7);
    SelI.h.assign(4, -1);
    SelJ.h.assign(4, -1);
    Cm.h.assign(4, -1);
    SelS.h.assign(4, SENT);
    Track.h.assign((size_t)LD * 5, SENT);
    const int step0 = 2;
    State.h = {step0, 0, maxdeg, m};
    const std::vector<double> e0 = E.h, c0 = Cc.h;
    const std::vector<u64> mask0 = Mask.h;
    const std::vector<int> deg0 = Deg.h;
    if (!W.up() || !E.up() || !Cc.up() || !Score.up() || !Ps.up() || !SelS.up() || !Track.up() || !Node.up() ||
        !Deg.up() || !Po.up() || !SelI.up() || !SelJ.up() || !Cm.up() || !State.up() || !Pk.up() || !Mask.up())
        return false;
    const int rounds = S.mask_kind == M_FULL ? 2 : 1;  // the second pair must find the stop word and do nothing
    for (int rd = 0; rd < rounds; ++rd) {
        if (!hip_ok(op_score(mcap, t, W.d, Cc.d, Mask.d, State.d, Score.d, nblocks, Ps.d, Pk.d, Po.d))) return false;
        if (!hip_ok(op_pick(nblocks, Ps.d, Pk.d, Po.d, mcap, t, k, n, W.d, Node.d, E.d, Cc.d, Mask.d, Deg.d, SelI.d,
                            SelJ.d, SelS.d, Track.d, Cm.d, State.d)))
            return false;
    }
    if (!Score.down() || !E.down() || !Cc.down() || !SelS.down() || !Track.down() || !SelI.down() || !SelJ.down() ||
        !Cm.down() || !State.down() || !Mask.down() || !Deg.down())
        return false;
    char tag[200];
    snprintf(tag, sizeof tag, "t=%d mcap=%d m=%d mask=%d max_blocks=%d ties=%d deg=%d", t, mcap, m, S.mask_kind,
             S.max_blocks, S.ties, S.deg_kind);

    // score
    bool ok = Score.h[(size_t)mcap * mcap] == SENT;
    double bs = 0.0;
    u64 bk = 0;
    int bo = 0;
    for (int a = 0; a < mcap; ++a)
        for (int b = 0; b < mcap; ++b) {
            const double got = Score.h[(size_t)a * mcap + b];
            if (!(a < b && b < m && !bit(mask0, words, a, b))) {
                ok = ok && got == SENT;
                continue;
            }
            long double s = 0.0L;
            for (int q = 0; q < t; ++q)
                s += expl((long double)e0[q]) *
                     expl(2.0L * ((long double)W.h[(size_t)a * LD + q] * (long double)W.h[(size_t)b * LD + q]));
            const double rel = (double)(fabsl((long double)got - s) / fabsl(s));
            if (!(rel <= 1e-12)) ok = false;
            if (rel > g_max_rel || rel != rel) g_max_rel = rel;
            if (before(got, key_of(a, b), 1, bs, bk, bo)) bs = got, bk = key_of(a, b), bo = 1;
        }
    report(0, ok, std::string("score ") + tag);

    // pick
    if (!bo) {
        ok = State.h[1] == 1 && State.h[0] == step0 && State.h[2] == maxdeg && State.h[3] == m && SelI.h[step0] == -1 &&
             SelS.h[step0] == SENT && Cm.h[step0] == -1 && E.h == e0 && Cc.h == c0 && Mask.h == mask0 && Deg.h == deg0 &&
             Track.h[(size_t)LD * (step0 + 1)] == SENT;
        report(1, ok, std::string("pick (stop) ") + tag);
        return true;
    }
    const int a = (int)(bk >> 32), b = (int)(bk & 0xffffffffull);
    ok = State.h[1] == 0 && SelI.h[step0] == std::max(Node.h[a], Node.h[b]) &&
         SelJ.h[step0] == std::min(Node.h[a], Node.h[b]) && SelS.h[step0] == Score.h[(size_t)a * mcap + b];
    if (want_a >= 0) ok = ok && a == want_a && b == want_b;
    if (S.mask_kind == M_ONLY_FIRST) ok = ok && a == 0 && b == 1;
    if (S.mask_kind == M_ONLY_CORNER) ok = ok && a == m - 2 && b == m - 1;
    report(1, ok, std::string("pick ") + tag);

    // apply
    ok = State.h[0] == step0 + 1 && SelI.h[step0 + 1] == -1 && SelI.h[step0 - 1] == -1 && Cm.h[step0] == m &&
         Cm.h[step0 + 1] == -1 && Cm.h[step0 - 1] == -1;
    std::vector<u64> mask1 = mask0;
    set_bit(mask1, words, a, b);
    set_bit(mask1, words, b, a);
    ok = ok && Mask.h == mask1 && bit(Mask.h, words, a, b) && bit(Mask.h, words, b, a);
    std::vector<int> deg1 = deg0;
    const int md = std::max(maxdeg, std::max(++deg1[a], ++deg1[b]));
    ok = ok && Deg.h == deg1 && State.h[2] == md && State.h[3] == std::min(mcap, std::min(md + k, n));
    if (S.deg_kind == D_PLAIN) ok = ok && State.h[3] == m;
    if (S.deg_kind == D_GROW) ok = ok && State.h[2] == maxdeg + 1 && State.h[3] == m + 1;
    if (S.deg_kind == D_CLAMP) ok = ok && State.h[2] == maxdeg + 1 && State.h[3] == m && m == n;
    const double scale = fabs(e0[0]) + 2.0;
    for (int q = 0; q < LD; ++q) {
        if (q < t) {
            const double en = e0[q] + 2.0 * W.h[(size_t)a * LD + q] * W.h[(size_t)b * LD + q];
            ok = ok && fabs(E.h[q] - en) <= 4e-16 * scale && fabs(Cc.h[q] - exp(E.h[q])) <= 1e-14 * exp(E.h[q]) &&
                 Track.h[(size_t)LD * (step0 + 1) + q] == E.h[q];
        } else {
            ok = ok && E.h[q] == 0.0 && Cc.h[q] == 0.0 && Track.h[(size_t)LD * (step0 + 1) + q] == SENT;
        }
    }
    ok = ok && Track.h[(size_t)LD * step0] == SENT && Track.h[(size_t)LD * (step0 + 2)] == SENT;
    report(2, ok, std::string("apply ") + tag);
    return true;
}

static bool run_all() {
    const int ts[] = {2, 3, 16, 17, 31, 32};
    const int mcaps[] = {2, 63, 64, 65, 129, 200};
    int q = 0;
    for (int t : ts)
        for (int mcap : mcaps) {
            // a live m below mcap wherever mcap leaves room (mcap = 2 has one pair)
            const int m = mcap <= 2 ? mcap : mcap - 1 - q % 3;
            Spec S = {t, mcap, m, q % 2 ? M_RANDOM : M_EMPTY, q % 5 == 4 ? 2 : 0, 0, D_PLAIN};
            if (!run_case(S)) return false;
            ++q;
        }
    const Spec extra[] = {
        // no free pair: the stop word and nothing else
        {25, 65, 64, M_FULL, 0, 0, D_PLAIN},
        {3, 200, 190, M_FULL, 2, 0, D_PLAIN},
        {2, 2, 2, M_FULL, 0, 0, D_PLAIN},
        // one free pair: the first position; the ragged corner of the last tile
        {25, 200, 197, M_ONLY_FIRST, 0, 0, D_PLAIN},
        {17, 65, 65, M_ONLY_FIRST, 0, 0, D_PLAIN},
        {25, 200, 197, M_ONLY_CORNER, 0, 0, D_PLAIN},
        {32, 130, 129, M_ONLY_CORNER, 1, 0, D_PLAIN},
        {16, 65, 65, M_ONLY_CORNER, 0, 0, D_PLAIN},
        // bit-identical rows in different tiles, grids of 1, 2 and the maximum
        {25, 200, 190, M_RANDOM, 1, 1, D_PLAIN},
        {25, 200, 190, M_RANDOM, 2, 1, D_PLAIN},
        {25, 200, 190, M_RANDOM, 0, 1, D_PLAIN},
        {17, 200, 200, M_EMPTY, 1, 2, D_PLAIN},
        {17, 200, 200, M_EMPTY, 2, 2, D_PLAIN},
        {17, 200, 200, M_EMPTY, 0, 2, D_PLAIN},
        {32, 129, 120, M_RANDOM, 1, 3, D_PLAIN},
        {32, 129, 120, M_RANDOM, 2, 3, D_PLAIN},
        {32, 129, 120, M_RANDOM, 0, 3, D_PLAIN},
        {2, 200, 199, M_EMPTY, 0, 4, D_PLAIN},
        // the pick raises the maximum degree: m grows by one; m clamps at n
        {25, 200, 150, M_RANDOM, 0, 0, D_GROW},
        {25, 65, 64, M_EMPTY, 0, 0, D_GROW},
        {25, 65, 65, M_RANDOM, 0, 0, D_CLAMP},
        {3, 200, 200, M_EMPTY, 2, 0, D_CLAMP},
    };
    for (const Spec& S : extra)
        if (!run_case(S)) return false;
    return true;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--host")) g_host = true;
        else {
            fprintf(stderr, "usage: miobi_make_check [--host]\n");
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
    for (int g = 0; g < 3; ++g) {
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
