// pairs_check -- the greedy candidate kernels of kt_pairs.hip called one by
// one through their kt::launch_* entry points (kt_launch.h), each result
// compared with a host reference in long double (or in exact integers).
//
// Groups: select (launch_pair_select), orth (launch_pairs_orth), eig
// (launch_pair_eig in its three forms), edit (launch_greedy_edit), whole
// (launch_pair_fused in three forms, launch_pair_reg_dyn).
// Not covered here: the fused and dense paths past 2j = 56 with global scratch
// (they stay with test_pairs_fused_matches_batched), log and sqrt in `whole`
// (the graphs' adjacency matrices are indefinite; `eig` covers them).
//
// Conventions (as sweep_check): long double references; every output
// pre-filled with a sentinel and followed by a guard region that must come
// back unchanged; NaN in inputs that must not be read (window columns past 2C,
// record 0's window entries, the weights of unit graphs, CSR capacity past
// dyn[0], the state slots a kernel does not own); on the device every case
// runs twice and the two outputs must agree bit for bit (the source claims
// fixed-order sums); failures carry name, shape, what, index, got, expected,
// bound.  KT_PAIRS_DENSE_EIG and KT_PAIRS_REG are flipped with setenv inside
// the one process (the library reads them per call).
// u = 2^-53, gamma_k = k u / (1 - k u).  Bounds are first order (terms in u^2
// dropped) with the magnitudes taken from the long double reference; each
// group reports max_ratio, the largest error / bound it saw.
//
// ---- select ---------------------------------------------------------------
// C = 1, 3, 63, 64, 65, 130; n = 2, 3, 17, 300; ld = 2C, 2C + 6.  X zero in
// the candidate columns, sentinels past them; ii / jj random, every fifth
// candidate with i == j, ii[0] the last row.  Exactly the 2C selected entries
// become 1.0, everything else keeps its bits.
//
// ---- orth -----------------------------------------------------------------
// Entry forms: start (cur == nullptr: sweeps C0-D-E), step1 (prev == nullptr),
// full.  C, n, ld as select, plus (n = 1100, C = 5, num_cu = 256) whose
// nrb = 69 > 64 sends wave_sum_parts on a second trip; skip null everywhere,
// pointing at 1 and at 0 at (C = 65, n = 17) and (C = 3, n = 300, num_cu = 8):
// with 0, W, coef, part and hr are bit-unchanged.  Columns >= 2C of W carry
// sentinels that must survive; those of prev / cur are NaN.
// Kinds (a kind needs n >= window + 2 rows for a remainder of full rank):
//   exact    the window is distinct unit vectors, W small integers, the
//            remainder's column 1 is (3, 4) on two free rows: h equals the
//            selected entries of W by bits, g2 = 0 by bits, R11 = -5 by bits;
//            R12, R22 and Q as in `bounded`
//   bounded  standard-normal W, a window orthonormalised in long double and
//            rounded; h, R against the long double reference of the same
//            algorithm (CGS2, then dgeqr2 / dorg2r), Q by three residuals
//   exactly rank-deficient blocks, all in exactly representable arithmetic
//   (norms are powers of two or the entry itself), compared componentwise
//   (h, R, Q) with the long double dgeqr2 / dorg2r, tau = 0 branch included:
//     selectors       W = [e_i e_j] written by launch_pair_select, i != j
//     rank_i_eq_j     the same with i == j
//     rank_zero_col2  column 2 inside the window's span, column 1 leaves +-4
//     rank_in_span    both columns inside the window's span (Q = [e_1 e_2])
//     rank_zero_tail  column 1 = (a, 0, ...), a = +-3: beta1 = a, not -|a|
// Bounds, for candidate columns s = 1, 2, window vectors P_k (k <= 4), w the
// input, w' / w'' the remainder after pass 1 / 2, g1, g2 the passes' dots:
//   a dot of n terms in any order (per-thread chains, LDS, wave_sum_parts):
//     gamma_(n+1) sum |P_rk| |w_r|
//   one update w_r - sum_k P_rk g_k (4 products, 3 additions, 1 subtraction):
//     upd_r = gamma_6 (|w_r| + sum_k |P_rk| |g_k|)
//   h = fl(g1 + g2); with E = |I - P'P| (long double, exact for the data):
//     |h - h_ref|_k <= sum_k' E_kk' gamma_(n+1) sum_r |P_rk'| |w_r|   (pass 1's error, seen through E only)
//                      + gamma_(n+1) sum_r |P_rk| |w'_r| + sum_r |P_rk| upd1_r  (pass 2)
//                      + u |h_k|
//   Delta_r = sum_k |P_rk| bound_h_k + upd1_r + upd2_r bounds the error of w''.
//   R (forward, from the perturbation of a 2-column QR; c = gamma_(n+16): the
//   n-term sum of squares or products plus at most 16 scalar roundings in
//   hypot, sqrt, tau, scal, t, kappa):
//     R11: |Delta_1|_2 + c |R11|
//     dq = 2 |Delta_1|_2 / |R11|   (the change of q1)
//     et = c (|w''_02| + sum_(r>=1) |w''_r1 w''_r2| / |alpha1 - beta1|)   (the error of t)
//     R12: |Delta_2|_2 + dq |w''_2|_2 + 2 et + gamma_16 (|w''_02| + |tau1 t|)
//     R22: |Delta_2|_2 + 2 dq |w''_2|_2 + (|tau1| et / |alpha1 - beta1| + gamma_8 |kappa|) |w''_1|_2
//          + gamma_4 (|w''_2|_2 + |kappa| |w''_1|_2) + c |R22|
//     R22's sign is rounding's choice where z_1, or an existing tail of z, is
//     zero to within that bound (beta2 = -sign(z_1)|z| but beta2 = z_1 at an
//     exactly zero tail): |R22| is compared there.
//   Q (backward form): |Q'Q - I| <= 24 c (tau v'v / 2 = 1 to 2 gamma_(n+8) per
//     reflector, d = v1'v2 to 2 gamma_(n+4), |tau| <= 2, |v|^2 <= 2);
//     |P_k' q1| <= rho_k1 / |R11| + 24 c |P_k|,
//     |P_k' q2| <= (rho_k2 + |R12| rho_k1 / |R11|) / |R22| + 24 c |P_k|, with
//     rho_ks = gamma_(n+1) sum_r |P_rk| |w'_rs| + sum_k' E_kk' |g2_k's| + sum_r |P_rk| upd2_rs
//     (what CGS2's second pass leaves of P'w'');
//     |W_in - [p c] h - Q R|_rs <= sum_k |P_rk| u |h_ks| + upd1_rs + upd2_rs + 8 c |w''_s|_2.
// The --host stand-in meets all of them with max_ratio 0.10.
//
// ---- eig ------------------------------------------------------------------
// Forms and depths j (the edges of xm_waves, group_lanes and the
// 64-eigenvalues-at-a-time loop of fused_xm_blk):
//   blk   k_pair_eig_blk (default)                 j = 1 2 3 8 16 17 28 29 32 33 64 65 129
//   wave  k_pair_eig_wave<1,4> (dense, 2j <= 56)   j = 1 2 3 8 16 17 28
//   one   k_pair_eig (dense, 2j > 56, scratch)     j = 29 33
// with it = j + 3: blk and wave at every C = 1, 63, 64, 65, 257 times every
// fun = 0 .. 6; the one-thread form at every C with fun = 0 and at every fun
// with C = 65 (22 of the 70 launches per depth: a dense solve per thread takes
// tens of milliseconds a launch, and the full product was measured at 10.6 s
// for the whole program on the device against 6 s this way; fun only enters
// after the eigenvalues, C only sets how many threads run the same solve);
// each depth once more (C = 65, fun = 0) with it = j.  Candidate c of a launch takes record variant c % nv
// and state mode c % 5.
// Record variants hist[step][C][11] (record 0's window entries h[0,1,4,5] are
// NaN: never read):
//   lanczos  a long double block-2 Lanczos (full reorthogonalisation) on a
//            random symmetric matrix of order 2j + 6, rounded to double
//   midzero  a zero R block in the middle, the second half a copy of the
//            first (decoupled halves, equal eigenvalues across them)
//   zerolead zero leading diagonal block, decoupled from a positive definite
//            rest: two zero eigenvalues at the spectrum's lower edge
//   cluster  constant diagonal, couplings of 1e-9
//   wide     diagonal log-spaced over 1e-8 .. 1e2, couplings 5 % of the
//            smaller neighbour (positive definite by diagonal dominance)
//   asym     random, the mirrored entries (h[8] and the next h[0], h[9] / h[1],
//            h[10] / h[5], h[3] / h[6], 0 / h[4]) differ at 1e-6: the
//            (X + X')/2 step matters
//   lanczos0 the lanczos records with Cm = 0 (contract: Xm == +0.0 by bits in
//            every form, both projections run identical arithmetic)
// Every variant runs at every depth.  For log and sqrt the diagonal is shifted
// so that Gershgorin's lower bound is 0.25 rho (`wide` is positive as built
// and is not shifted); the other functions see the records unshifted.
// Reference: the matrix exactly as k_pair_eig places it, Cm added and
// (X + X')/2 formed in fp64 (these steps are defined by bits), then cyclic
// Jacobi in long double, Xm = sum_k f(l1_k) - f(l2_k) in long double.
// Bound on Xm:
//   K_eig u rho sum_k (|f'(l1_k)| + |f'(l2_k)|) + gamma_(nn+8) sum_k (|f(l1_k)| + |f(l2_k)|)
// rho: Gershgorin radius of both projections in long double; the first term
// is an eigenvalue error of K_eig u rho carried through f, the second the
// rounding of f itself (a few ulp), of exp(l1)(1 - exp(l2 - l1)) and of the
// nn-term sum in any order.
//   K_eig = max(18, 4 r_host) rounded up to a power of two; 18 u rho is the
//   source's statement for the block Sturm path (4e-15 rho).
//   r_host = the largest |lambda - lambda_ref| / (u rho) of the --host
//   stand-in (fp64 cyclic Jacobi) over every eig case; --host prints it on
//   stderr.  Measured: r_host = 47.3 (17.7 up to j = 33; the fp64 Jacobi
//   error grows with the order), so K_eig = 256.
// Structural checks (exact): the stop decision (state prepared so that
// |Xm_ref - X0| is tol / 5 or 5 tol, tol = 64 x the launch's largest bound;
// X1 set so that a lag-1 test decides the other way), the lucky flag at
// |R| = 0.9e-8 and 1.1e-8 (R22 far below both), j == it, the X0/X1 shift by
// bits, done candidates bit-unchanged, slots 6-7 untouched, active[0].
//
// ---- edit -----------------------------------------------------------------
// One graph: n = 1500 (n + 1 > 1024), a ring plus chords, weights distinct by
// position, nnz > 1024, self loops, long_thresh = 8 with the long rows (40:
// 20 entries, 10: 12, 700: 9, 1200: 9) listed heaviest first; CSR buffers of
// capacity nnz + 37 with dyn[0] = nnz.  Everything is compared exactly with
// an edit done on (row, column, weight) triples: sel, selv, the ranking
// [0, nT - 1) (the kernel leaves slot nT - 1 as it was), rp2, ci2, va2 up to
// dyn2[0] and their sentinel tails, lr2, dyn2, the inputs unchanged.
// Cases: C = 1, 5, 1024, 1025, 2500; nT = C and 4096; ties within a thread
// (c, c + 1024), across lanes, across waves, and the later index in the lower
// lane / wave; NaN scores (also at 0 and C - 1) beside the minimum; all NaN /
// +inf (sel = -1, selv = +inf, CSR and ranking copied unchanged); the best
// candidate at rank 0, in the middle, at nT - 1; an ordinary edge, a self
// loop, an absent edge, an edge of a long row at long_thresh + 1 (it leaves
// lr2, the others keep their order), an edge between two such rows; step 0
// and 3; nT = 4097 returns hipErrorInvalidValue with nothing written.
//
// ---- whole ----------------------------------------------------------------
// Fifteen graphs built here (make_wgraph; --count prints the table, the host
// test pins it): n = 2, 3, 511, 512, 513, 1024 (R = 2), 1025 (4), 2049 (6),
// 3073 (7), 3585, 4096 (8), 4097 (past 8 * 512: k_pair_fused); unit (weights
// passed as NaN: never read) and weighted; rows r % 11 == 5 empty, short
// degrees 1 .. 14 (every one of 3, 4, 5, 7, 8, 9, around the 4-deep gather, on
// the graphs with at most 3 long rows; make_wgraph checks), long_thresh = 16
// with one row at 16, long rows of 17 .. 20, 33 and 70 entries, n_long = 0, 3
// and 300 > kRegLongCap; at n = 4096 nnz = 7.4k, 20k and 46k so that
// kt::pair_reg_form gives csr 2, 1 and 0 and spec 0 and 1.
// Per graph C = 3 candidates (an edge of the heaviest row, two more edges; on
// some graphs the third is a pair i == i, whose start is rank deficient and
// whose Cm needs R12), B = [0.3 -1; -1 -0.2], fun = exp, cosh or cos, it = 6
// (n = 2, 3: it = 1, the Krylov space ends there); forms default (k_pair_reg,
// or k_pair_fused at 4097), KT_PAIRS_REG=0 (k_pair_fused, block Sturm) and
// with KT_PAIRS_DENSE_EIG=1 (dense, 2 it <= 56); tolerances never (0), always
// (1e300: stops at step 3) and, on the graphs that have one, mid (4 x one
// candidate's lag-2 difference at a step 4 <= J < it where that candidate
// stops at J and every candidate's decisions keep their margins).  That
// needs lag-2 differences a factor 16 apart from step to step; with the
// heavier weights and on most unit graphs Xm converges by about a factor 8
// per step, so n1025, n2049 and n3073 carry lighter weights (/ 16 instead of
// / 4).  n511, n513, n1024, n1025, n2049, n3073 and n4096a have a mid
// tolerance -- every R = 2, 4, 6, 7, 8; --count marks them, the host test pins
// them -- and the other graphs have no mid cases.
// Reference: the whole run in long double (3-term block Lanczos with CGS2
// against the window, Gram-Schmidt QR -- Xm does not depend on the basis's
// signs --, Jacobi).  Kept cases only: wherever a record enters a projection
// min(R11, R22) >= 1e-3 rho(A), every stop decision a factor 4 from tol, |R|
// a factor 4 from 1e-8; --host fails a case that is not.
// Bound on Xm: K_whole u rho sum (|f'|) + gamma_(nn+8) sum (|f|) at the final
// step, K_whole = max(K_eig, 8 r_whole); r_whole = the worst (error - gamma
// term) / (u rho sum |f'|) of the fp64 --host restatement (CGS2 + Householder
// + Jacobi) over the whole cases.  Measured: r_whole = 0.84, so K_whole = 256.
// iter, lucky, done exact; slots 0, 1, 6, 7 untouched.
// Contract: launch_pair_reg_dyn on a CSR with candidate 1's edge deleted, in
// buffers of the first matrix's capacity with dyn = {nnz, n_long} of the
// edited one, equals launch_pair_fused on that CSR by bits.
//
//   pairs_check                     run on the GPU
//   pairs_check --host              every launcher replaced by a plain fp64
//                                   stand-in written from the contract (no GPU)
//   pairs_check --host --mutate=M   one deliberate defect in that stand-in
//   pairs_check --count             the case counts and the form tables alone
//   --group=NAME runs one group; --small thins the shapes (C = 3 and 65 for
//   select / orth; C = 65, fun = 0 and 5, j <= 33 for eig; four graphs)
//
// Prints one JSON line; exit status 0 iff no case failed, 1 on failures, 3 on
// a HIP error (nothing is launched after it), 2 on bad usage.
// Build: make -C tests/native/pairs_check (links the library's own kt_pairs.o).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../../krylov_robustness_amd/csrc/kt_launch.h"

typedef long double ld_t;
typedef std::vector<double> dvec;
typedef std::vector<ld_t> lvec;
typedef std::vector<int> ivec;

static const double K_EIG = 256.0;  // max(18, 4 r_host) -> power of two; r_host = 47.3 measured (--host)

static bool g_host = false;
static bool g_list = false;
static bool g_small = false;
static int g_only = -1;
static std::string g_mut;
// inside the whole-run stand-in only the whole_* defects apply (it reuses the orth stand-in)
static bool g_whole_scope = false;
static bool mut(const char* s) { return g_mut == s && (!g_whole_scope || !strncmp(s, "whole_", 6)); }

// ---------------------------------------------------------------------------
// report
// ---------------------------------------------------------------------------
struct Fail {
    std::string name, shape, what;
    long idx;
    double got, exp, bound;
};
struct Group {
    const char* name;
    long cases = 0, nfail = 0;
    std::vector<Fail> fails;
    double seconds = 0.0, max_ratio = 0.0;
};
enum { G_SELECT, G_ORTH, G_EIG, G_EDIT, G_WHOLE, NG };
static Group g_groups[NG] = {{"select"}, {"orth"}, {"eig"}, {"edit"}, {"whole"}};
static std::chrono::steady_clock::time_point g_t0;

static std::string fmt(const char* f, ...) {
    char buf[320];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

static std::string jnum(double x) {
    if (std::isnan(x)) return "\"nan\"";
    if (std::isinf(x)) return x > 0 ? "\"inf\"" : "\"-inf\"";
    return fmt("%.17g", x);
}

struct EigForm {
    const char* name;
    int dense;
    const char* reaches;
    std::vector<int> depths;
};
static const std::vector<EigForm> kEigForms = {
    {"blk", 0, "k_pair_eig_blk", {1, 2, 3, 8, 16, 17, 28, 29, 32, 33, 64, 65, 129}},
    {"wave", 1, "k_pair_eig_wave<1,4>", {1, 2, 3, 8, 16, 17, 28}},
    {"one", 1, "k_pair_eig", {29, 33}},
};

static void wgraphs_print();
static void print_report(const char* hip_err) {
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - g_t0).count();
    long nfail = 0;
    for (int g = 0; g < NG; ++g) nfail += g_groups[g].nfail;
    printf("{\"pairs_check\": \"%s\", \"mode\": \"%s\", \"mutate\": \"%s\", \"wall_s\": %.3f, ",
           hip_err ? "HIP_ERROR" : (nfail ? "FAIL" : "ok"), g_list ? "count" : (g_host ? "host" : "device"),
           g_mut.c_str(), wall);
    if (hip_err) printf("\"hip_error\": \"%s\", ", hip_err);
    if (g_list) {
        printf("\"forms\": {\"pair_eig\": [");
        for (size_t i = 0; i < kEigForms.size(); ++i) {
            const EigForm& f = kEigForms[i];
            printf("%s{\"form\": \"%s\", \"dense\": %d, \"reaches\": \"%s\", \"depths\": [", i ? ", " : "", f.name,
                   f.dense, f.reaches);
            for (size_t k = 0; k < f.depths.size(); ++k) printf("%s%d", k ? ", " : "", f.depths[k]);
            printf("]}");
        }
        printf("], \"pair_reg\": [");
        wgraphs_print();
        printf("]}, ");
    }
    printf("\"groups\": {");
    for (int g = 0; g < NG; ++g) {
        const Group& G = g_groups[g];
        printf("%s\"%s\": {\"cases\": %ld, \"seconds\": %.3f, \"max_ratio\": %.4g, \"failed_count\": %ld, \"failed\": [",
               g ? ", " : "", G.name, G.cases, G.seconds, G.max_ratio, G.nfail);
        for (size_t i = 0; i < G.fails.size(); ++i) {
            const Fail& f = G.fails[i];
            printf("%s{\"name\": \"%s\", \"shape\": \"%s\", \"what\": \"%s\", \"index\": %ld, \"got\": %s, "
                   "\"expected\": %s, \"bound\": %s}",
                   i ? ", " : "", f.name.c_str(), f.shape.c_str(), f.what.c_str(), f.idx, jnum(f.got).c_str(),
                   jnum(f.exp).c_str(), jnum(f.bound).c_str());
        }
        printf("]}");
    }
    printf("}}\n");
    fflush(stdout);
}

[[noreturn]] static void hip_die(const char* what, hipError_t e) {
    const std::string msg = fmt("%s: %s", what, hipGetErrorString(e));
    print_report(msg.c_str());
    exit(3);
}
#define HC(x)                                  \
    do {                                       \
        hipError_t e_ = (x);                   \
        if (e_ != hipSuccess) hip_die(#x, e_); \
    } while (0)
// a launcher call, then (device) the stream drained so that an error belongs to this case
#define LAUNCH(x)                                \
    do {                                         \
        HC(x);                                   \
        if (!g_host) HC(hipDeviceSynchronize()); \
    } while (0)

[[noreturn]] static void setup_die(const std::string& msg) {
    fprintf(stderr, "pairs_check: test setup: %s\n", msg.c_str());
    exit(2);
}

static uint64_t bits_of(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}

static const double SENT = -7.7777e77;
static const int ISENT = -77777777;
static const size_t GUARD = 67;
static const ld_t U = ldexpl(1.0L, -53);
static ld_t gam(ld_t k) { return k * U / (1.0L - k * U); }

// One case: keeps its worst failing element (largest error / bound).
struct Case {
    Group& g;
    std::string name, shape;
    bool bad = false;
    double score = -1.0;
    Fail worst;
    Case(int gi, const std::string& n, const std::string& s) : g(g_groups[gi]), name(n), shape(s) {}
    ~Case() {
        g.cases++;
        if (bad) {
            g.nfail++;
            if (g.fails.size() < 12) g.fails.push_back(worst);
        }
    }
    void fail(const char* what, long idx, double got, double exp, double bound, double sc = 0.0) {
        if (std::isnan(sc)) sc = INFINITY;
        if (!bad || sc > score) {
            worst = Fail{name, shape, what, idx, got, exp, bound};
            score = sc;
        }
        bad = true;
    }
    void exact(const char* what, long idx, double got, double exp) {
        if (!(got == exp)) fail(what, idx, got, exp, 0.0, fabs(got - exp));
    }
    void same(const char* what, long idx, double got, double exp) {
        if (bits_of(got) != bits_of(exp)) fail(what, idx, got, exp, 0.0, INFINITY);
    }
    void bounded(const char* what, long idx, ld_t got, ld_t ref, ld_t bound) {
        if (!std::isfinite((double)bound)) setup_die(fmt("%s %s: the bound of '%s' is not finite", name.c_str(), shape.c_str(), what));
        const ld_t e = fabsl(got - ref);
        if (!(e <= bound)) {
            fail(what, idx, (double)got, (double)ref, (double)bound, (double)(e / bound));
        } else if (bound > 0.0L) {
            g.max_ratio = std::max(g.max_ratio, (double)(e / bound));
        }
    }
    void unchanged(const char* what, const dvec& before, const dvec& after, size_t from = 0) {
        for (size_t t = from; t < before.size(); ++t) same(what, (long)t, after[t], before[t]);
    }
    void iunchanged(const char* what, const ivec& before, const ivec& after, size_t from = 0) {
        for (size_t t = from; t < before.size(); ++t)
            if (after[t] != before[t]) fail(what, (long)t, after[t], before[t], 0.0, INFINITY);
    }
    void ieq(const char* what, long idx, int got, int exp) {
        if (got != exp) fail(what, idx, got, exp, 0.0, INFINITY);
    }
};

// ---------------------------------------------------------------------------
// memory: a per-case stack (device memory, or host memory with --host)
// ---------------------------------------------------------------------------
struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
    void init(size_t c) {
        cap = c;
        if (g_host) {
            base = (char*)malloc(c);
            if (!base) exit(2);
        } else {
            HC(hipMalloc((void**)&base, c));
        }
    }
    template <class T>
    T* up(const std::vector<T>& h) {
        const size_t b = h.size() * sizeof(T);
        T* p = (T*)(base + off);
        if (off + b > cap) setup_die("arena too small");
        off += (b + 255) / 256 * 256;
        if (b) {
            if (g_host) memcpy(p, h.data(), b);
            else HC(hipMemcpy(p, h.data(), b, hipMemcpyHostToDevice));
        }
        return p;
    }
};
static Arena g_work;
template <class T>
static T* up(const std::vector<T>& h) {
    return g_work.up(h);
}
template <class T>
static std::vector<T> down(const T* p, size_t n) {
    std::vector<T> h(n);
    if (n) {
        if (g_host) memcpy(h.data(), p, n * sizeof(T));
        else HC(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    }
    return h;
}

static uint64_t g_rng = 88172645463325252ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static double runif() { return (rnd() >> 11) * (1.0 / 9007199254740992.0); }
static double rnormal() {
    const double u1 = ((rnd() >> 11) + 1.0) * (1.0 / 9007199254740993.0);
    const double u2 = (rnd() >> 11) * (1.0 / 9007199254740992.0);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// state per candidate (kt_pairs.hip): [0] X0 [1] X1 [2] Xm [3] iter [4] lucky [5] done, 8 doubles
enum : int { PS_X0 = 0, PS_X1 = 1, PS_XM = 2, PS_ITER = 3, PS_LUCKY = 4, PS_DONE = 5, PS_N = 8 };

// ---------------------------------------------------------------------------
// eigenvalues: cyclic Jacobi (Rutishauser's rotation), ascending.  Rotations
// on entries below eps |A|_F / (64 n) are skipped: all skipped entries
// together move an eigenvalue by less than eps |A|_F / 64.
// ---------------------------------------------------------------------------
template <class T>
static std::vector<T> jacobi_eig(int n, std::vector<T> a /* row-major, symmetric */) {
    T fro = 0;
    for (const T& x : a) fro += x * x;
    fro = std::sqrt(fro);
    const T tiny = std::numeric_limits<T>::epsilon() * fro / (T)(64 * n);
    for (int sweep = 0; sweep < 100; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const T apq = a[(size_t)p * n + q];
                if (!(std::fabs(apq) > tiny)) continue;
                rotated = true;
                const T theta = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2 * apq);
                const T t = std::fabs(theta) > (T)1e12 ? 1 / (2 * theta)
                                                       : (theta >= 0 ? 1 : -1) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
                const T c = 1 / std::sqrt(t * t + 1), s = t * c;
                a[(size_t)p * n + p] -= t * apq;
                a[(size_t)q * n + q] += t * apq;
                a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0;
                T* rp = &a[(size_t)p * n];
                T* rq = &a[(size_t)q * n];
                for (int k = 0; k < n; ++k) {
                    if (k == p || k == q) continue;
                    const T x = rp[k], y = rq[k];
                    rp[k] = c * x - s * y;
                    rq[k] = s * x + c * y;
                    a[(size_t)k * n + p] = rp[k];
                    a[(size_t)k * n + q] = rq[k];
                }
            }
        if (!rotated) break;
        if (sweep == 99) setup_die(fmt("jacobi_eig: no convergence at n = %d", n));
    }
    std::vector<T> d(n);
    for (int i = 0; i < n; ++i) d[i] = a[(size_t)i * n + i];
    std::sort(d.begin(), d.end());
    return d;
}

// the two projections of one candidate exactly as k_pair_eig forms them (fp64,
// row-major): G from the records (lanczos_krylov.m:85-90 block placement),
// T = G + Cm (column-major 2 x 2) at the leading block, both (X + X')/2.
// rec: record b at rec + b * stride.
static void place_projections(int j, const double* rec, size_t stride, const double* cm, bool symmetrise, dvec& G,
                              dvec& T) {
    const int nn = 2 * j;
    G.assign((size_t)nn * nn, 0.0);
    auto at = [&](int r, int c) -> double& { return G[(size_t)r * nn + c]; };
    for (int b = 0; b < j; ++b) {
        const double* h = rec + b * stride;
        at(2 * b, 2 * b) = h[2];
        at(2 * b + 1, 2 * b) = h[3];
        at(2 * b, 2 * b + 1) = h[6];
        at(2 * b + 1, 2 * b + 1) = h[7];
        if (b >= 1) {
            at(2 * b - 2, 2 * b) = h[0];
            at(2 * b - 1, 2 * b) = h[1];
            at(2 * b - 2, 2 * b + 1) = h[4];
            at(2 * b - 1, 2 * b + 1) = h[5];
        }
        if (b + 1 < j) {
            at(2 * b + 2, 2 * b) = h[8];
            at(2 * b + 2, 2 * b + 1) = h[9];
            at(2 * b + 3, 2 * b + 1) = h[10];
        }
    }
    T = G;
    T[0] += cm[0];
    T[nn] += cm[1];
    T[1] += cm[2];
    T[nn + 1] += cm[3];
    for (dvec* X : {&G, &T})
        for (int r = 0; r < nn; ++r)
            for (int q = 0; q < r; ++q) {
                // without the step: the lower triangle alone (a defect)
                const double x = symmetrise ? 0.5 * ((*X)[(size_t)r * nn + q] + (*X)[(size_t)q * nn + r])
                                            : (*X)[(size_t)r * nn + q];
                (*X)[(size_t)r * nn + q] = (*X)[(size_t)q * nn + r] = x;
            }
}

template <class T>
static T fscalar(int fun, T x) {
    switch (fun) {
    case 0: return std::exp(x);
    case 1: return std::sinh(x);
    case 2: return std::cosh(x);
    case 3: return std::sin(x);
    case 4: return std::cos(x);
    case 5: return std::log(x);
    case 6: return std::sqrt(x);
    }
    return 0;
}
static ld_t fprime(int fun, ld_t x) {
    switch (fun) {
    case 0: return expl(x);
    case 1: return coshl(x);
    case 2: return sinhl(x);
    case 3: return cosl(x);
    case 4: return -sinl(x);
    case 5: return 1.0L / x;
    case 6: return 0.5L / sqrtl(x);
    }
    return 0;
}

// ---------------------------------------------------------------------------
// the --host stand-in of launch_pair_eig: fp64 Jacobi, written from the
// contract (kt_launch.h, the state layout and the stop rule of
// trace_fun_update.m:85-118).  Eigenvalues are memoised on the candidate's
// record bytes (the launches repeat a few record variants many times).
// ---------------------------------------------------------------------------
namespace host {
static std::map<std::string, std::pair<dvec, dvec>> g_memo;

static const std::pair<dvec, dvec>& projections_eig(int j, const double* rec, size_t stride, const double* cm) {
    std::string key((size_t)(j * 11 + 4) * 8, '\0');
    for (int b = 0; b < j; ++b) memcpy(&key[(size_t)b * 88], rec + b * stride, 88);
    memset(&key[(size_t)(j - 1) * 88 + 64], 0, 24);  // the last record's R is not part of the projections
    memcpy(&key[(size_t)j * 88], cm, 32);
    auto it = g_memo.find(key);
    if (it != g_memo.end()) return it->second;
    dvec G, T;
    double cmz[4] = {cm[0], cm[1], cm[2], cm[3]};
    place_projections(j, rec, stride, cmz, !mut("eig_no_symmetrise"), G, T);
    if (mut("eig_cm_on_both")) G = T;
    std::pair<dvec, dvec> v;
    v.first = jacobi_eig<double>(2 * j, T);
    v.second = jacobi_eig<double>(2 * j, G);
    return g_memo.emplace(key, std::move(v)).first->second;
}

static hipError_t pair_eig(int C, int j, int it, int fun, double tol, const double* hist, const double* Cm,
                           double* state, int* active) {
    const int nn = 2 * j;
    for (int c = 0; c < C; ++c) {
        double* st = state + (size_t)c * PS_N;
        if (st[PS_DONE] != 0.0 && !mut("eig_done_not_frozen")) continue;
        const auto& ev = projections_eig(j, hist + (size_t)c * 11, (size_t)C * 11, Cm + (size_t)c * 4);
        double xm = 0.0;
        const int ne = mut("eig_drop_last_eigenvalue") ? nn - 1 : nn;
        for (int k = 0; k < ne; ++k) xm += fscalar<double>(fun, ev.first[k]) - fscalar<double>(fun, ev.second[k]);
        const double* hj = hist + ((size_t)(j - 1) * C + c) * 11;
        const bool lucky = mut("eig_lucky_r22_only") ? fabs(hj[10]) < 1e-8
                                                     : sqrt(hj[8] * hj[8] + hj[9] * hj[9] + hj[10] * hj[10]) < 1e-8;
        st[PS_XM] = xm;
        st[PS_LUCKY] = lucky ? 1.0 : 0.0;
        bool stop = false;
        if (j <= 2) {
            st[PS_X0 + j - 1] = xm;
        } else if (fabs(xm - st[mut("eig_stop_lag1") ? PS_X1 : PS_X0]) < tol) {
            stop = true;
        } else {
            st[PS_X0] = st[PS_X1];
            st[PS_X1] = xm;
        }
        if (stop || lucky || j == it) {
            st[PS_DONE] = 1.0;
            st[PS_ITER] = j;
        }
    }
    int cnt = 0;
    for (int c = 0; c < C; ++c) cnt += mut("active_counts_done") ? state[(size_t)c * PS_N + PS_DONE] != 0.0
                                                                 : state[(size_t)c * PS_N + PS_DONE] == 0.0;
    active[0] = cnt;
    return hipSuccess;
}

// launch_greedy_edit: the smallest score (first on ties, NaN never), its pair
// dropped from the ranking, the edge deleted from both triangles into the
// other CSR buffer, the long rows that stay long in their order
static hipError_t greedy_edit(int C, const double* state, int* Ti, int* Tj, int nT, int n, int long_thresh,
                              const int* rp, const int* ci, const double* va, const int* lr, const int* dyn, int* rp2,
                              int* ci2, double* va2, int* lr2, int* dyn2, int step, int* sel, double* selv) {
    if (nT > 4096) return hipErrorInvalidValue;
    double v = INFINITY;
    int best = -1;
    for (int c = 0; c < C; ++c) {
        const double x = state[(size_t)c * PS_N + PS_XM];
        if (mut("edit_nan_wins") && std::isnan(x) && !std::isnan(v)) {
            v = x;
            best = c;
        } else if (x < v || (mut("edit_tie_takes_last") && x == v && best >= 0)) {
            v = x;
            best = c;
        }
    }
    const int r1 = best >= 0 ? Ti[best] : -1, r2 = best >= 0 ? Tj[best] : -1;
    sel[2 * step] = r1;
    sel[2 * step + 1] = r2;
    selv[step] = v;
    int k1 = -1, k2 = -1;
    if (best >= 0) {
        for (int k = rp[r1]; k < rp[r1 + 1]; ++k)
            if (ci[k] == r2) k1 = k;
        if (r1 != r2)
            for (int k = rp[r2]; k < rp[r2 + 1]; ++k)
                if (ci[k] == r1) k2 = k;
        const int last = mut("edit_ranking_last_entry_lost") ? nT - 1 : nT;
        for (int t = best + 1; t < last; ++t) {
            Ti[t - 1] = Ti[t];
            Tj[t - 1] = Tj[t];
        }
    }
    const int nnz = dyn[0];
    int d = 0;
    for (int t = 0; t < nnz; ++t) {
        if (t == k1 || t == k2) continue;
        ci2[d] = ci[t];
        va2[d] = va[t];
        ++d;
    }
    for (int r = 0; r <= n; ++r) {
        const bool s1 = mut("edit_rp_shift_from_r1") ? r >= r1 : r > r1;
        rp2[r] = rp[r] - (k1 >= 0 && s1) - (k2 >= 0 && r > r2);
    }
    int m = 0;
    for (int l = 0; l < dyn[1]; ++l) {
        const int r = lr[l];
        if (rp2[r + 1] - rp2[r] > long_thresh || mut("edit_keeps_shortened_long_row")) lr2[m++] = r;
    }
    dyn2[0] = d;
    dyn2[1] = m;
    return hipSuccess;
}
}  // namespace host

// ---------------------------------------------------------------------------
// select / orth
// ---------------------------------------------------------------------------
// per-candidate coefficient record of launch_pairs_orth (kt_pairs.hip)
enum : int { CF_G1 = 0, CF_G2 = 8, CF_NCOEF = 25 };

namespace host {
static hipError_t pair_select(int C, const int* ii, const int* jj, double* X, int ld) {
    for (int c = 0; c < C; ++c) {
        X[(size_t)ii[c] * ld + 2 * c] = 1.0;
        X[(size_t)jj[c] * ld + 2 * c + 1] = 1.0;
    }
    return hipSuccess;
}

static void larfg(double alpha, double xx, double& beta, double& tau, double& scal) {
    if (xx == 0.0 && !mut("orth_no_tau0_branch")) {  // H = I
        beta = alpha;
        tau = 0.0;
        scal = 1.0;
        return;
    }
    beta = -copysign(hypot(alpha, sqrt(xx)), alpha);
    tau = (beta - alpha) / beta;
    scal = 1.0 / (alpha - beta);
}

// CGS2 of each candidate's two columns against [prev cur] and the thin
// Householder QR of the remainder (LAPACK's conventions); the row sums are
// formed per row block and the blocks summed, as the launcher's geometry has it
static hipError_t pairs_orth(int C, int n, int num_cu, const double* prev, const double* cur, double* W, int ld,
                             double* coef, double* part, double* hr, const int* skip) {
    (void)part;
    if (skip && *skip == 0 && !mut("orth_ignores_skip")) return hipSuccess;
    const int nrb = (int)(kt::pairs_part_doubles(n, C, num_cu) / ((size_t)8 * C));
    const int rpb = (n + nrb - 1) / nrb;
    const int nend = mut("orth_drop_last_row") ? n - 1 : n;
    const int nsum = mut("orth_partials_stop_at_64") ? std::min(nrb, 64) : nrb;
    auto bsum = [&](int from, auto term) {
        double s = 0.0;
        for (int b = 0; b < nsum; ++b) {
            double sb = 0.0;
            for (int r = std::max(from, b * rpb); r < std::min(nend, (b + 1) * rpb); ++r) sb += term(r);
            s += sb;
        }
        return s;
    };
    for (int c = 0; c < C; ++c) {
        const size_t off = 2 * (size_t)c;
        auto w = [&](int r, int s) -> double& { return W[(size_t)r * ld + off + s]; };
        double* cf = coef + (size_t)c * CF_NCOEF;
        for (int k = 0; k < 16; ++k) cf[k] = 0.0;
        if (cur) {
            const double* basis[4] = {prev, prev, cur, cur};
            for (int pass = 0; pass < 2; ++pass) {
                double* g = cf + (pass ? CF_G2 : CF_G1);
                for (int s = 0; s < 2; ++s)
                    for (int k = 0; k < 4; ++k)
                        g[4 * s + k] = basis[k] ? bsum(0, [&](int r) { return basis[k][(size_t)r * ld + off + (k & 1)] * w(r, s); }) : 0.0;
                for (int r = 0; r < nend; ++r)
                    for (int s = 0; s < 2; ++s) {
                        double acc = 0.0;
                        for (int k = 0; k < 4; ++k)
                            if (basis[k]) acc += basis[k][(size_t)r * ld + off + (k & 1)] * g[4 * s + k];
                        w(r, s) -= acc;
                    }
            }
        }
        const double s1 = bsum(mut("orth_row0_in_s1") ? 0 : 1, [&](int r) { return w(r, 0) * w(r, 0); });
        const double ab = bsum(1, [&](int r) { return w(r, 0) * w(r, 1); });
        double beta1, tau1, scal1, beta2, tau2, scal2;
        larfg(w(0, 0), s1, beta1, tau1, scal1);
        const double t = w(0, 1) + scal1 * ab;
        const double kappa = tau1 * t * scal1;
        const double r12 = w(0, 1) - tau1 * t;
        const double v11 = w(1, 0) * scal1;
        auto z = [&](int r) { return w(r, 1) - kappa * w(r, 0); };
        const double s2 = bsum(mut("orth_row1_in_s2") ? 1 : 2, [&](int r) { return z(r) * z(r); });
        const double dz = bsum(2, [&](int r) { return w(r, 0) * z(r); });
        larfg(z(1), s2, beta2, tau2, scal2);
        const double d = v11 + scal1 * scal2 * dz;
        const double k2 = tau1 * (v11 - tau2 * d);
        double* o = hr + (size_t)c * 11;
        for (int k = 0; k < 8; ++k) o[k] = cf[CF_G1 + k] + cf[CF_G2 + k];
        o[8] = beta1;
        o[9] = r12;
        o[10] = beta2;
        for (int r = 0; r < nend; ++r) {
            const double v1 = r == 0 ? 1.0 : r == 1 ? v11 : w(r, 0) * scal1;
            const double v2 = r == 0 ? 0.0 : r == 1 ? 1.0 : z(r) * scal2;
            const double q0 = (r == 0 ? 1.0 : 0.0) - tau1 * v1;
            const double q1 = (r == 1 ? 1.0 : 0.0) - tau2 * v2 - k2 * v1;
            w(r, 0) = q0;
            w(r, 1) = q1;
            if (mut("orth_store_invalid_lane") && c == C - 1)  // the lanes past C store too, at their own columns
                for (int cc = C; cc < (C + 63) / 64 * 64 && 2 * cc + 1 < ld; ++cc) {
                    W[(size_t)r * ld + 2 * cc] = q0;
                    W[(size_t)r * ld + 2 * cc + 1] = q1;
                }
        }
    }
    return hipSuccess;
}
}  // namespace host

static void grp_select() {
    const std::vector<int> Cs = g_small ? std::vector<int>{3, 65} : std::vector<int>{1, 3, 63, 64, 65, 130};
    for (int C : Cs)
        for (int n : {2, 3, 17, 300})
            for (int pad : {0, 6}) {
                const int ld = 2 * C + pad;
                Case cs(G_SELECT, "select", fmt("C=%d n=%d ld=%d", C, n, ld));
                if (g_list) continue;
                g_rng = 0xD1B54A32D192ED03ull + (uint64_t)C * 1000 + n * 7 + pad;
                dvec X((size_t)n * ld + GUARD, SENT);
                for (int r = 0; r < n; ++r)
                    for (int q = 0; q < 2 * C; ++q) X[(size_t)r * ld + q] = 0.0;
                ivec ii(C), jj(C);
                for (int c = 0; c < C; ++c) {
                    ii[c] = (int)(rnd() % n);
                    jj[c] = c % 5 == 2 ? ii[c] : (int)(rnd() % n);
                }
                ii[0] = n - 1;
                dvec want = X;
                for (int c = 0; c < C; ++c) {
                    want[(size_t)ii[c] * ld + 2 * c] = 1.0;
                    want[(size_t)jj[c] * ld + 2 * c + 1] = 1.0;
                }
                dvec got[2];
                for (int run = 0; run < (g_host ? 1 : 2); ++run) {
                    g_work.off = 0;
                    double* dX = up(X);
                    const int* dii = up(ii);
                    const int* djj = up(jj);
                    if (g_host) LAUNCH(host::pair_select(C, dii, djj, dX, ld));
                    else LAUNCH(kt::launch_pair_select(C, dii, djj, dX, ld, nullptr));
                    got[run] = down(dX, X.size());
                    cs.unchanged(run ? "X (second run)" : "X", want, got[run]);
                }
            }
}

// ---- the long double reference: CGS2, then dgeqr2 / dorg2r on the n x 2 remainder
struct OrthRef {
    ld_t h[8], g1[8], g2[8], R[3];
    lvec w1[2], w2[2], q[2];  // after pass 1, after pass 2, Q
    ld_t tau1, tau2, t, kappa, amb;  // amb = alpha1 - beta1
    ld_t z1, ztail;                  // the second reflector's alpha and the norm of its tail
};

static void dlarfg_ld(int m, ld_t& alpha, ld_t* x, ld_t& tau) {  // x: m - 1 entries
    ld_t xx = 0;
    for (int i = 0; i < m - 1; ++i) xx += x[i] * x[i];
    if (xx == 0) {
        tau = 0;
        return;
    }
    const ld_t nrm = sqrtl(alpha * alpha + xx);
    const ld_t beta = alpha >= 0 ? -nrm : nrm;
    tau = (beta - alpha) / beta;
    for (int i = 0; i < m - 1; ++i) x[i] /= (alpha - beta);
    alpha = beta;
}

static void orth_ref(int n, const lvec* P /* [4], empty = absent */, const lvec& a0, const lvec& a1, OrthRef& o) {
    lvec w[2] = {a0, a1};
    auto dot = [&](const lvec& x, const lvec& y) {
        ld_t s = 0;
        for (int r = 0; r < n; ++r) s += x[r] * y[r];
        return s;
    };
    for (int pass = 0; pass < 2; ++pass) {
        ld_t* g = pass ? o.g2 : o.g1;
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 4; ++k) g[4 * s + k] = P[k].empty() ? 0.0L : dot(P[k], w[s]);
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 4; ++k)
                if (!P[k].empty())
                    for (int r = 0; r < n; ++r) w[s][r] -= P[k][r] * g[4 * s + k];
        (pass ? o.w2 : o.w1)[0] = w[0];
        (pass ? o.w2 : o.w1)[1] = w[1];
    }
    for (int k = 0; k < 8; ++k) o.h[k] = o.g1[k] + o.g2[k];
    // dgeqr2
    const ld_t alpha1 = w[0][0];
    ld_t a = alpha1;
    dlarfg_ld(n, a, w[0].data() + 1, o.tau1);
    o.amb = alpha1 - a;
    o.R[0] = a;
    ld_t vw = w[1][0];  // v1' w(:, 2), v1 = [1; w0(2:n)]
    for (int r = 1; r < n; ++r) vw += w[0][r] * w[1][r];
    o.t = vw;
    w[1][0] -= o.tau1 * vw;
    for (int r = 1; r < n; ++r) w[1][r] -= o.tau1 * vw * w[0][r];
    o.R[1] = w[1][0];
    o.kappa = o.amb != 0 ? o.tau1 * vw / o.amb : 0.0L;
    ld_t b = w[1][1];
    o.z1 = b;
    o.ztail = 0;
    for (int r = 2; r < n; ++r) o.ztail += w[1][r] * w[1][r];
    o.ztail = sqrtl(o.ztail);
    dlarfg_ld(n - 1, b, w[1].data() + 2, o.tau2);
    o.R[2] = b;
    // dorg2r: Q = H1 H2 [e1 e2]
    lvec v1(n, 0), v2(n, 0);
    v1[0] = 1;
    for (int r = 1; r < n; ++r) v1[r] = w[0][r];
    v2[1] = 1;
    for (int r = 2; r < n; ++r) v2[r] = w[1][r];
    for (int s = 0; s < 2; ++s) {
        lvec q(n, 0);
        q[s] = 1;
        const ld_t c2 = o.tau2 * dot(v2, q);
        for (int r = 0; r < n; ++r) q[r] -= c2 * v2[r];
        const ld_t c1 = o.tau1 * dot(v1, q);
        for (int r = 0; r < n; ++r) q[r] -= c1 * v1[r];
        o.q[s] = q;
    }
}

enum { OF_START, OF_STEP1, OF_FULL };
static const char* kOrthForm[3] = {"start", "step1", "full"};
enum { OK_EXACT, OK_BOUNDED, OK_SELECT, OK_SELECT_EQ, OK_ZERO_COL2, OK_IN_SPAN, OK_ZERO_TAIL };
static const char* kOrthKind[] = {"exact", "bounded", "selectors", "rank_i_eq_j", "rank_zero_col2", "rank_in_span", "rank_zero_tail"};

// skipmode: 0 null, 1 points at 1, 2 points at 0
static void orth_case(int form, int kind, int C, int n, int pad, int num_cu, int skipmode) {
    const int ld = 2 * C + pad;
    Case cs(G_ORTH, kOrthKind[kind], fmt("form=%s C=%d n=%d ld=%d num_cu=%d skip=%d", kOrthForm[form], C, n, ld, num_cu, skipmode));
    if (g_list) return;
    g_rng = 0xA0761D6478BD642Full + (uint64_t)C * 977 + (uint64_t)n * 31 + pad + 7 * form + 101 * kind;
    const int nwin = form == OF_START ? 0 : form == OF_STEP1 ? 2 : 4;
    const size_t blk = (size_t)n * ld;
    dvec W(blk + GUARD, SENT), prev(blk, NAN), cur(blk, NAN);
    std::vector<std::vector<lvec>> Pc(C, std::vector<lvec>(4));
    std::vector<lvec> A0(C), A1(C);
    for (int c = 0; c < C; ++c) {
        lvec win[4];  // p0 p1 c0 c1 (absent: empty)
        lvec a0(n, 0), a1(n, 0);
        ivec rows;  // window rows of the unit-vector kinds
        if (kind == OK_BOUNDED) {
            for (int k = 4 - nwin; k < 4; ++k) {
                win[k].resize(n);
                for (ld_t& x : win[k]) x = rnormal();
                for (int pass = 0; pass < 2; ++pass)
                    for (int k2 = 4 - nwin; k2 < k; ++k2) {
                        ld_t g = 0;
                        for (int r = 0; r < n; ++r) g += win[k2][r] * win[k][r];
                        for (int r = 0; r < n; ++r) win[k][r] -= g * win[k2][r];
                    }
                ld_t nn = 0;
                for (ld_t x : win[k]) nn += x * x;
                for (ld_t& x : win[k]) x = (double)(x / sqrtl(nn));  // orthonormal to rounding
            }
            for (int r = 0; r < n; ++r) {
                a0[r] = rnormal();
                a1[r] = rnormal();
            }
        } else {
            while ((int)rows.size() < nwin) {
                const int r = (int)(rnd() % n);
                if (std::find(rows.begin(), rows.end(), r) == rows.end()) rows.push_back(r);
            }
            for (int k = 0; k < nwin; ++k) {
                win[4 - nwin + k].assign(n, 0);
                win[4 - nwin + k][rows[k]] = 1;
            }
            ivec freer;
            for (int r = 0; r < n; ++r)
                if (std::find(rows.begin(), rows.end(), r) == rows.end()) freer.push_back(r);
            auto ri = [&]() { return (ld_t)((int)(rnd() % 17) - 8); };
            for (int r = 0; r < n; ++r) {
                a0[r] = ri();
                a1[r] = ri();
            }
            switch (kind) {
            case OK_EXACT:  // the remainder's column 1 is (3, 4): beta1 = -5
                for (int r : freer) a0[r] = 0;
                {
                    const int rA = freer[c % 2 ? 0 : freer.size() - 2], rB = freer[freer.size() - 1];
                    a0[rA] = 3;
                    a0[rB] = 4;
                    // column 2 independent of it on the free rows (R22 != 0)
                    bool other = false;
                    for (int r : freer) other = other || (r != rA && r != rB && a1[r] != 0);
                    if (!other && 3 * a1[rB] == 4 * a1[rA]) a1[rB] += 1;
                }
                break;
            case OK_SELECT:
            case OK_SELECT_EQ: {
                const int i = c % 3 == 0 ? 0 : c % 3 == 1 ? 1 % n : n - 1;
                int j = kind == OK_SELECT_EQ ? i : (int)(rnd() % n);
                if (kind == OK_SELECT && j == i) j = (i + 1) % n;
                a0.assign(n, 0);
                a1.assign(n, 0);
                a0[i] = 1;
                a1[j] = 1;
                break;
            }
            case OK_ZERO_COL2:  // column 2 lies in the window's span; column 1 leaves one entry 4 (or -4)
                for (int r : freer) a0[r] = a1[r] = 0;
                a0[freer[c % freer.size()]] = c % 2 ? 4 : -4;
                break;
            case OK_IN_SPAN:
                for (int r : freer) a0[r] = a1[r] = 0;
                break;
            case OK_ZERO_TAIL:  // column 1 = (a, 0, ...), a != 0; column 2 leaves (x, 0, 4, 0 ...) or (x, y)
                a0.assign(n, 0);
                a0[0] = c % 2 ? 3 : -3;
                for (int r = 1; r < n; ++r) a1[r] = 0;
                if (n > 2 && c % 3) a1[2 + c % (n - 2)] = 4;
                else a1[1] = c % 3 ? 0 : 5;
                break;
            }
        }
        for (int r = 0; r < n; ++r) {
            W[(size_t)r * ld + 2 * c] = (double)a0[r];
            W[(size_t)r * ld + 2 * c + 1] = (double)a1[r];
            for (int s = 0; s < 2; ++s) {
                prev[(size_t)r * ld + 2 * c + s] = win[s].empty() ? 0.0 : (double)win[s][r];
                cur[(size_t)r * ld + 2 * c + s] = win[2 + s].empty() ? 0.0 : (double)win[2 + s][r];
            }
        }
        for (int k = 0; k < 4; ++k) Pc[c][k] = win[k];
        A0[c] = a0;
        A1[c] = a1;
    }
    const size_t npart = kt::pairs_part_doubles(n, C, num_cu);
    dvec coef((size_t)CF_NCOEF * C + GUARD, SENT), part(npart + GUARD, SENT), hr((size_t)11 * C + GUARD, SENT);
    if (kind == OK_SELECT || kind == OK_SELECT_EQ) {  // W through launch_pair_select, as the start does
        for (int r = 0; r < n; ++r)
            for (int q = 0; q < 2 * C; ++q) W[(size_t)r * ld + q] = 0.0;
    }
    dvec oW[2], ocoef[2], opart[2], ohr[2];
    for (int run = 0; run < (g_host ? 1 : 2); ++run) {
        g_work.off = 0;
        double* dW = up(W);
        const double* dprev = form == OF_FULL ? up(prev) : nullptr;
        const double* dcur = form != OF_START ? up(cur) : nullptr;
        double *dcoef = up(coef), *dpart = up(part), *dhr = up(hr);
        const int* dskip = skipmode ? up(ivec{skipmode == 1 ? 1 : 0}) : nullptr;
        if (kind == OK_SELECT || kind == OK_SELECT_EQ) {
            ivec ii(C), jj(C);
            for (int c = 0; c < C; ++c)
                for (int r = 0; r < n; ++r) {
                    if (A0[c][r] != 0) ii[c] = r;
                    if (A1[c][r] != 0) jj[c] = r;
                }
            const int* dii = up(ii);
            const int* djj = up(jj);
            if (g_host) LAUNCH(host::pair_select(C, dii, djj, dW, ld));
            else LAUNCH(kt::launch_pair_select(C, dii, djj, dW, ld, nullptr));
        }
        if (g_host) LAUNCH(host::pairs_orth(C, n, num_cu, dprev, dcur, dW, ld, dcoef, dpart, dhr, dskip));
        else LAUNCH(kt::launch_pairs_orth(C, n, num_cu, dprev, dcur, dW, ld, dcoef, dpart, dhr, nullptr, dskip));
        oW[run] = down(dW, W.size());
        ocoef[run] = down(dcoef, coef.size());
        opart[run] = down(dpart, part.size());
        ohr[run] = down(dhr, hr.size());
    }
    if (!g_host) {
        cs.unchanged("second run differs (W)", oW[0], oW[1]);
        cs.unchanged("second run differs (coef)", ocoef[0], ocoef[1]);
        cs.unchanged("second run differs (part)", opart[0], opart[1]);
        cs.unchanged("second run differs (hr)", ohr[0], ohr[1]);
    }
    if (skipmode == 2) {  // nothing may be written
        cs.unchanged("W with skip -> 0", W, oW[0]);
        cs.unchanged("coef with skip -> 0", coef, ocoef[0]);
        cs.unchanged("part with skip -> 0", part, opart[0]);
        cs.unchanged("hr with skip -> 0", hr, ohr[0]);
        return;
    }
    const dvec& Q = oW[0];
    for (int r = 0; r < n; ++r)
        for (int q = 2 * C; q < ld; ++q) cs.same("sentinel column", (long)((size_t)r * ld + q), Q[(size_t)r * ld + q], SENT);
    cs.unchanged("W guard", W, Q, blk);
    cs.unchanged("coef guard", coef, ocoef[0], (size_t)CF_NCOEF * C);
    cs.unchanged("part guard", part, opart[0], npart);
    cs.unchanged("hr guard", hr, ohr[0], (size_t)11 * C);
    const ld_t gn1 = gam(n + 1), g6 = gam(6), gq = gam(n + 16);
    for (int c = 0; c < C; ++c) {
        OrthRef R;
        orth_ref(n, Pc[c].data(), A0[c], A1[c], R);
        const double* o = &ohr[0][(size_t)c * 11];
        const long ix = (long)c * 11;
        auto qd = [&](int r, int s) { return (ld_t)Q[(size_t)r * ld + 2 * c + s]; };
        for (int r = 0; r < n; ++r)
            for (int s = 0; s < 2; ++s)
                if (bits_of((double)qd(r, s)) == bits_of(SENT)) cs.fail("Q not written", (long)((size_t)r * ld + 2 * c + s), SENT, (double)R.q[s][r], 0.0, INFINITY);
        if (kind != OK_BOUNDED && kind != OK_EXACT) {  // exact arithmetic throughout: LAPACK's result, componentwise
            for (int k = 0; k < 8; ++k) cs.exact("h (rank-deficient)", ix + k, o[k], (double)R.h[k]);
            for (int k = 0; k < 3; ++k) cs.exact("R (rank-deficient)", ix + 8 + k, o[8 + k], (double)R.R[k]);
            for (int r = 0; r < n; ++r)
                for (int s = 0; s < 2; ++s) cs.exact("Q (rank-deficient)", (long)((size_t)r * ld + 2 * c + s), (double)qd(r, s), (double)R.q[s][r]);
            continue;
        }
        if (kind == OK_EXACT) {
            for (int k = 0; k < 8; ++k) {
                cs.same("h = selected entries of W", ix + k, o[k], (double)R.h[k] + 0.0);
                cs.same("g2 = 0", (long)c * CF_NCOEF + CF_G2 + k, ocoef[0][(size_t)c * CF_NCOEF + CF_G2 + k], 0.0);
            }
            cs.same("R11 = -5", ix + 8, o[8], -5.0);
        }
        // ---- bounds (see the header)
        const lvec* P = Pc[c].data();
        ld_t E[4][4], bh[8], rho[8], dabs1[8], dabs2[8];
        for (int k = 0; k < 4; ++k)
            for (int k2 = 0; k2 < 4; ++k2) {
                E[k][k2] = 0;
                if (P[k].empty() || P[k2].empty()) continue;
                ld_t d = 0;
                for (int r = 0; r < n; ++r) d += P[k][r] * P[k2][r];
                E[k][k2] = fabsl((k == k2 ? 1.0L : 0.0L) - d);
            }
        const lvec* win_in[2] = {&A0[c], &A1[c]};
        std::vector<lvec> upd1(2, lvec(n, 0)), upd2(2, lvec(n, 0));
        for (int s = 0; s < 2; ++s) {
            for (int r = 0; r < n; ++r) {
                ld_t m1 = fabsl((*win_in[s])[r]), m2 = fabsl(R.w1[s][r]);
                for (int k = 0; k < 4; ++k)
                    if (!P[k].empty()) {
                        m1 += fabsl(P[k][r] * R.g1[4 * s + k]);
                        m2 += fabsl(P[k][r] * R.g2[4 * s + k]);
                    }
                upd1[s][r] = nwin ? g6 * m1 : 0.0L;
                upd2[s][r] = nwin ? g6 * m2 : 0.0L;
            }
            for (int k = 0; k < 4; ++k) {
                ld_t d1 = 0, d2 = 0;
                if (!P[k].empty())
                    for (int r = 0; r < n; ++r) {
                        d1 += fabsl(P[k][r] * (*win_in[s])[r]);
                        d2 += fabsl(P[k][r] * R.w1[s][r]);
                    }
                dabs1[4 * s + k] = d1;
                dabs2[4 * s + k] = d2;
            }
            for (int k = 0; k < 4; ++k) {
                ld_t b = 0, rh = 0;
                if (!P[k].empty()) {
                    for (int k2 = 0; k2 < 4; ++k2) {
                        b += E[k][k2] * gn1 * dabs1[4 * s + k2];
                        rh += E[k][k2] * fabsl(R.g2[4 * s + k2]);
                    }
                    b += gn1 * dabs2[4 * s + k] + U * fabsl(R.h[4 * s + k]);
                    rh += gn1 * dabs2[4 * s + k];
                    for (int r = 0; r < n; ++r) {
                        b += fabsl(P[k][r]) * upd1[s][r];
                        rh += fabsl(P[k][r]) * upd2[s][r];
                    }
                }
                bh[4 * s + k] = b;
                rho[4 * s + k] = rh;
            }
        }
        ld_t nD[2], nw[2];
        for (int s = 0; s < 2; ++s) {
            ld_t a = 0, b = 0;
            for (int r = 0; r < n; ++r) {
                ld_t d = upd1[s][r] + upd2[s][r];
                for (int k = 0; k < 4; ++k)
                    if (!P[k].empty()) d += fabsl(P[k][r]) * bh[4 * s + k];
                a += d * d;
                b += R.w2[s][r] * R.w2[s][r];
            }
            nD[s] = sqrtl(a);
            nw[s] = sqrtl(b);
        }
        if (kind == OK_BOUNDED)
            for (int k = 0; k < 8; ++k) cs.bounded("h", ix + k, o[k], R.h[k], bh[k]);
        const ld_t aR11 = fabsl(R.R[0]), aR22 = fabsl(R.R[2]);
        ld_t sab = 0;
        for (int r = 1; r < n; ++r) sab += fabsl(R.w2[0][r] * R.w2[1][r]);
        const ld_t iamb = R.amb != 0 ? 1.0L / fabsl(R.amb) : 0.0L;
        const ld_t dq1 = aR11 > 0 ? 2 * nD[0] / aR11 : 0.0L;
        const ld_t et = gq * (fabsl(R.w2[1][0]) + sab * iamb);
        const ld_t bR11 = nD[0] + gq * aR11;
        const ld_t bR12 = nD[1] + dq1 * nw[1] + 2 * et + gam(16) * (fabsl(R.w2[1][0]) + fabsl(R.tau1 * R.t));
        const ld_t bR22 = nD[1] + 2 * dq1 * nw[1] + (fabsl(R.tau1) * iamb * et + gam(8) * fabsl(R.kappa)) * nw[0] +
                          gam(4) * (nw[1] + fabsl(R.kappa) * nw[0]) + gq * aR22;
        if (kind == OK_BOUNDED) cs.bounded("R11", ix + 8, o[8], R.R[0], bR11);
        cs.bounded("R12", ix + 9, o[9], R.R[1], bR12);
        // beta2 = -sign(z1) |z|, but beta2 = z1 where z's tail is exactly zero: where z1, or a
        // tail that exists (n > 2), is zero to within the error bound, the sign is rounding's
        // choice (either is a valid QR; the residuals below hold for both), so |R22| is compared
        if ((R.tau2 != 0 && fabsl(R.z1) <= bR22) || (n > 2 && R.ztail <= bR22)) cs.bounded("|R22|", ix + 10, fabs(o[10]), aR22, bR22);
        else cs.bounded("R22", ix + 10, o[10], R.R[2], bR22);
        // Q by its three residuals
        for (int s = 0; s < 2; ++s)
            for (int s2 = 0; s2 <= s; ++s2) {
                ld_t d = 0;
                for (int r = 0; r < n; ++r) d += qd(r, s) * qd(r, s2);
                cs.bounded("Q'Q - I", 2 * c + s, d, s == s2 ? 1.0L : 0.0L, 24 * gq);
            }
        for (int k = 0; k < 4; ++k) {
            if (P[k].empty()) continue;
            ld_t np = 0;
            for (int r = 0; r < n; ++r) np += P[k][r] * P[k][r];
            np = sqrtl(np);
            for (int s = 0; s < 2; ++s) {
                ld_t d = 0;
                for (int r = 0; r < n; ++r) d += P[k][r] * qd(r, s);
                const ld_t b = s == 0 ? rho[k] / aR11 : (rho[4 + k] + fabsl(R.R[1]) * rho[k] / aR11) / aR22;
                cs.bounded("[p c]'Q", (long)(c * 8 + 4 * s + k), d, 0.0L, b + np * 24 * gq);
            }
        }
        for (int r = 0; r < n; ++r)
            for (int s = 0; s < 2; ++s) {
                ld_t res = (*win_in[s])[r], b = upd1[s][r] + upd2[s][r] + 8 * gq * nw[s];
                for (int k = 0; k < 4; ++k)
                    if (!P[k].empty()) {
                        res -= P[k][r] * (ld_t)o[4 * s + k];
                        b += fabsl(P[k][r]) * U * fabsl(R.h[4 * s + k]);
                    }
                res -= qd(r, 0) * (ld_t)o[8 + s];
                if (s == 1) res -= qd(r, 1) * (ld_t)o[10];
                cs.bounded("W - [p c] h - Q R", (long)((size_t)r * ld + 2 * c + s), res, 0.0L, b);
            }
    }
}

static void grp_orth() {
    const std::vector<int> Cs = g_small ? std::vector<int>{3, 65} : std::vector<int>{1, 3, 63, 64, 65, 130};
    for (int form : {OF_START, OF_STEP1, OF_FULL}) {
        const int nwin = form == OF_START ? 0 : form == OF_STEP1 ? 2 : 4;
        for (int C : Cs)
            for (int n : {2, 3, 17, 300})
                for (int pad : {0, 6}) {
                    // the remainder needs two rows of its own (two free unit vectors / full column rank)
                    if (n >= nwin + 2) {
                        orth_case(form, OK_EXACT, C, n, pad, 256, 0);
                        orth_case(form, OK_BOUNDED, C, n, pad, 256, 0);
                    }
                    if (form == OF_START) {
                        orth_case(form, OK_SELECT, C, n, pad, 256, 0);
                        orth_case(form, OK_SELECT_EQ, C, n, pad, 256, 0);
                        orth_case(form, OK_ZERO_TAIL, C, n, pad, 256, 0);
                    } else if (n > nwin) {
                        orth_case(form, OK_ZERO_COL2, C, n, pad, 256, 0);
                        orth_case(form, OK_IN_SPAN, C, n, pad, 256, 0);
                    }
                }
        // nrb = 69 > 64: the partial sums take a second trip
        orth_case(form, OK_EXACT, 5, 1100, 6, 256, 0);
        orth_case(form, OK_BOUNDED, 5, 1100, 6, 256, 0);
        for (int skipmode : {1, 2})
            for (int pad : {0, 6}) {
                orth_case(form, OK_BOUNDED, 65, 17, pad, 256, skipmode);
                orth_case(form, OK_EXACT, 3, 300, pad, 8, skipmode);
            }
    }
}

// ---------------------------------------------------------------------------
// eig: record variants
// ---------------------------------------------------------------------------
enum { V_LANCZOS, V_MIDZERO, V_ZEROLEAD, V_CLUSTER, V_WIDE, V_ASYM, V_LANCZOS0, NVAR };
static const char* kVarName[NVAR] = {"lanczos", "midzero", "zerolead", "cluster", "wide", "asym", "lanczos0"};

struct Variant {  // records [j][11], Cm, and the reference spectra
    dvec rec;
    double cm[4];
    lvec l1, l2;
    ld_t rho = 0;
    dvec G, T;  // the fp64 projections until the spectra are solved
    int j = 0, var = 0;
    bool pos = false;
};

// block-2 Lanczos with full reorthogonalisation in long double on a random
// symmetric matrix of order 2j + 6; the records rounded to double
static dvec lanczos_records(int j) {
    static std::map<int, dvec> cache;
    if (cache.count(j)) return cache[j];
    const int N = 2 * j + 6;
    std::vector<ld_t> A((size_t)N * N);
    for (int r = 0; r < N; ++r)
        for (int c = 0; c <= r; ++c) A[(size_t)r * N + c] = A[(size_t)c * N + r] = (ld_t)rnormal() / sqrtl((ld_t)N);
    std::vector<lvec> V;  // orthonormal columns so far
    auto dot = [&](const lvec& a, const lvec& b) {
        ld_t s = 0;
        for (int i = 0; i < N; ++i) s += a[i] * b[i];
        return s;
    };
    lvec e0(N, 0), e1(N, 0);
    e0[0] = 1;
    e1[1] = 1;
    V.push_back(e0);
    V.push_back(e1);
    dvec rec((size_t)j * 11, NAN);
    for (int b = 0; b < j; ++b) {
        lvec w[2];
        for (int s = 0; s < 2; ++s) {
            w[s].assign(N, 0);
            const lvec& x = V[2 * b + s];
            for (int r = 0; r < N; ++r) {
                ld_t acc = 0;
                for (int c = 0; c < N; ++c) acc += A[(size_t)r * N + c] * x[c];
                w[s][r] = acc;
            }
        }
        double* h = &rec[(size_t)b * 11];
        for (int s = 0; s < 2; ++s) {
            if (b >= 1) {
                h[4 * s + 0] = (double)dot(V[2 * b - 2], w[s]);
                h[4 * s + 1] = (double)dot(V[2 * b - 1], w[s]);
            }
            h[4 * s + 2] = (double)dot(V[2 * b], w[s]);
            h[4 * s + 3] = (double)dot(V[2 * b + 1], w[s]);
        }
        for (int pass = 0; pass < 2; ++pass)
            for (int s = 0; s < 2; ++s)
                for (const lvec& v : V) {
                    const ld_t g = dot(v, w[s]);
                    for (int i = 0; i < N; ++i) w[s][i] -= g * v[i];
                }
        const ld_t r11 = sqrtl(dot(w[0], w[0]));
        for (ld_t& x : w[0]) x /= r11;
        const ld_t r12 = dot(w[0], w[1]);
        for (int i = 0; i < N; ++i) w[1][i] -= r12 * w[0][i];
        const ld_t r22 = sqrtl(dot(w[1], w[1]));
        for (ld_t& x : w[1]) x /= r22;
        h[8] = (double)r11;
        h[9] = (double)r12;
        h[10] = (double)r22;
        V.push_back(w[0]);
        V.push_back(w[1]);
    }
    cache[j] = rec;
    return rec;
}

// records from diagonal blocks D_b = [a b; b c] and couplings R_b = [r11 r12; 0 r22];
// asym: the mirrored entries differ at 1e-6 (relative; 1e-6 for the zero)
static dvec block_records(int j, const dvec& D, const dvec& R, bool asym) {
    dvec rec((size_t)j * 11, NAN);
    const double e = asym ? 1e-6 : 0.0;
    for (int b = 0; b < j; ++b) {
        double* h = &rec[(size_t)b * 11];
        h[2] = D[3 * b];
        h[3] = D[3 * b + 1] * (1 + e);
        h[6] = D[3 * b + 1] * (1 - e);
        h[7] = D[3 * b + 2];
        if (b >= 1) {  // the window block: R_{b-1}'
            h[0] = R[3 * (b - 1)] * (1 + e);
            h[1] = R[3 * (b - 1) + 1] * (1 - e);
            h[4] = e;
            h[5] = R[3 * (b - 1) + 2] * (1 + 2 * e);
        }
        h[8] = R[3 * b] * (1 - e);
        h[9] = R[3 * b + 1] * (1 + e);
        h[10] = R[3 * b + 2];
    }
    return rec;
}

static void build_variant(int j, int var, bool pos, Variant& v) {
    const int nn = 2 * j;
    g_rng = 0x2545F4914F6CDD1Dull + (uint64_t)j * 131 + var;
    dvec D(3 * j), R(3 * j);
    double cscale = 0.3;
    for (int b = 0; b < j; ++b) {
        D[3 * b] = rnormal();
        D[3 * b + 1] = rnormal();
        D[3 * b + 2] = rnormal();
        R[3 * b] = 0.5 + runif();
        R[3 * b + 1] = rnormal();
        R[3 * b + 2] = 0.5 + runif();
    }
    switch (var) {
    case V_LANCZOS:
    case V_LANCZOS0:
        g_rng = 0x2545F4914F6CDD1Dull + (uint64_t)j * 131;  // the same records for both
        v.rec = lanczos_records(j);
        break;
    case V_MIDZERO: {
        const int m = j / 2;  // blocks [0, m) and [m, j): R_{m-1} = 0
        for (int b = m; b < j && m > 0; ++b)
            for (int t = 0; t < 3; ++t) {
                D[3 * b + t] = D[3 * (b - m) + t];
                R[3 * b + t] = R[3 * (b - m) + t];
            }
        if (m > 0) {
            R[3 * (m - 1)] = R[3 * (m - 1) + 1] = R[3 * (m - 1) + 2] = 0.0;
            if (2 * m == j) R[3 * (j - 1)] = R[3 * (j - 1) + 1] = R[3 * (j - 1) + 2] = 0.0;
        }
        v.rec = block_records(j, D, R, false);
        break;
    }
    case V_ZEROLEAD:
        for (int b = 0; b < j; ++b) {
            D[3 * b] = 3.0 + runif();
            D[3 * b + 1] = 0.3 * rnormal();
            D[3 * b + 2] = 3.0 + runif();
            R[3 * b] = 0.4 * runif();
            R[3 * b + 1] = 0.2 * runif();
            R[3 * b + 2] = 0.4 * runif();
        }
        D[0] = D[1] = D[2] = 0.0;
        R[0] = R[1] = R[2] = 0.0;
        v.rec = block_records(j, D, R, false);
        break;
    case V_CLUSTER:
        for (int b = 0; b < j; ++b) {
            D[3 * b] = D[3 * b + 2] = 1.0;
            D[3 * b + 1] = 1e-9 * rnormal();
            for (int t = 0; t < 3; ++t) R[3 * b + t] = 1e-9 * rnormal();
        }
        v.rec = block_records(j, D, R, false);
        break;
    case V_WIDE: {
        auto dg = [&](int i) { return pow(10.0, -8.0 + 10.0 * i / (double)(nn > 1 ? nn - 1 : 1)); };
        for (int b = 0; b < j; ++b) {
            D[3 * b] = dg(2 * b);
            D[3 * b + 2] = dg(2 * b + 1);
            D[3 * b + 1] = 0.05 * dg(2 * b);
            for (int t = 0; t < 3; ++t) R[3 * b + t] = 0.05 * dg(2 * b);
        }
        v.rec = block_records(j, D, R, false);
        break;
    }
    case V_ASYM: v.rec = block_records(j, D, R, true); break;
    }
    double dmax = 0.0;
    for (int b = 0; b < j; ++b) dmax = std::max(dmax, std::max(fabs(v.rec[11 * b + 2]), fabs(v.rec[11 * b + 7])));
    cscale *= std::max(dmax, 0.5);
    v.cm[0] = cscale * rnormal();
    v.cm[1] = cscale * rnormal();
    v.cm[2] = v.cm[1] * (1 + 1e-6) + (var == V_ASYM ? 1e-6 : 0.0);
    v.cm[3] = cscale * rnormal();
    if (var == V_WIDE) {
        v.cm[0] = 0.3 * v.rec[2];
        v.cm[1] = v.cm[2] = 0.01 * v.rec[2];
        v.cm[3] = 0.3 * v.rec[7];
    }
    if (var == V_LANCZOS0) v.cm[0] = v.cm[1] = v.cm[2] = v.cm[3] = 0.0;
    // the last record's R is not part of the projection: set per candidate (lucky test)
    v.rec[11 * (j - 1) + 8] = 0.5;
    v.rec[11 * (j - 1) + 9] = 0.25;
    v.rec[11 * (j - 1) + 10] = 0.75;
    dvec G, T;
    auto gersh = [&](ld_t& lo, ld_t& rho) {
        place_projections(j, v.rec.data(), 11, v.cm, true, G, T);
        lo = INFINITY;
        rho = 0;
        for (const dvec* X : {&G, &T})
            for (int r = 0; r < nn; ++r) {
                ld_t off = 0;
                for (int q = 0; q < nn; ++q)
                    if (q != r) off += fabsl((ld_t)(*X)[(size_t)r * nn + q]);
                const ld_t d = (*X)[(size_t)r * nn + r];
                lo = std::min(lo, d - off);
                rho = std::max(rho, fabsl(d) + off);
            }
    };
    ld_t lo, rho;
    gersh(lo, rho);
    if (pos && var != V_WIDE && lo < 0.25L * rho) {
        const double s = (double)(0.25L * rho - lo);
        for (int b = 0; b < j; ++b) {
            v.rec[11 * b + 2] += s;
            v.rec[11 * b + 7] += s;
        }
        gersh(lo, rho);
    }
    v.rho = rho;
    v.G = G;
    v.T = T;
    v.j = j;
    v.var = var;
    v.pos = pos;
}

static double g_r_host = 0.0;  // --host: the stand-in's largest eigenvalue error / (u rho)
static std::map<std::tuple<int, int, bool>, Variant> g_variants;

// the long double spectra of prepared variants, one Jacobi run per task on up
// to 16 threads (the runs are independent; largest first)
static void solve_variants(const std::vector<Variant*>& vs) {
    struct Task {
        Variant* v;
        int mat;  // 0: T -> l1, 1: G -> l2
    };
    std::vector<Task> tasks;
    for (Variant* v : vs) {
        tasks.push_back({v, 1});
        if (v->var != V_LANCZOS0) tasks.push_back({v, 0});
    }
    std::stable_sort(tasks.begin(), tasks.end(), [](const Task& a, const Task& b) { return a.v->j > b.v->j; });
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t t; (t = next.fetch_add(1)) < tasks.size();) {
            Variant& v = *tasks[t].v;
            const dvec& X = tasks[t].mat ? v.G : v.T;
            (tasks[t].mat ? v.l2 : v.l1) = jacobi_eig<ld_t>(2 * v.j, lvec(X.begin(), X.end()));
        }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nth = std::min<size_t>({(size_t)16, (size_t)(hw ? hw : 1), tasks.size()});
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nth; ++t) pool.emplace_back(work);
    work();
    for (std::thread& th : pool) th.join();
    for (Variant* v : vs) {
        if (v->var == V_LANCZOS0) v->l1 = v->l2;
        if (v->pos && !(v->l1[0] > 0 && v->l2[0] > 0)) setup_die(fmt("variant %s j=%d is not positive", kVarName[v->var], v->j));
        dvec().swap(v->G);
        dvec().swap(v->T);
        if (g_host && g_mut.empty()) {
            const auto& ev = host::projections_eig(v->j, v->rec.data(), 11, v->cm);
            for (int k = 0; k < 2 * v->j; ++k) {
                g_r_host = std::max(g_r_host, (double)(fabsl(ev.first[k] - v->l1[k]) / (U * v->rho)));
                g_r_host = std::max(g_r_host, (double)(fabsl(ev.second[k] - v->l2[k]) / (U * v->rho)));
            }
        }
    }
}

// prepared (not yet solved) on first use; variants_prefetch solves a whole list at once
static Variant* variant_slot(int j, int var, bool pos, bool* fresh) {
    const auto key = std::make_tuple(j, var, pos);
    auto it = g_variants.find(key);
    *fresh = it == g_variants.end();
    if (!*fresh) return &it->second;
    Variant& v = g_variants[key];
    build_variant(j, var, pos, v);
    return &v;
}
static const Variant& variant(int j, int var, bool pos) {
    bool fresh;
    Variant* v = variant_slot(j, var, pos, &fresh);
    if (fresh) solve_variants({v});
    return *v;
}

static std::vector<int> variants_of(int) {  // every variant at every depth
    return {V_LANCZOS, V_MIDZERO, V_ZEROLEAD, V_CLUSTER, V_WIDE, V_ASYM, V_LANCZOS0};
}

// state modes of a candidate
enum { M_GO, M_STOP, M_DONE, M_LUCKY, M_NOTLUCKY, NMODE };

static void eig_case(const EigForm& F, int j, int C, int fun, int it) {
    Case cs(G_EIG, fmt("%s_%s", F.name, it == j ? "last" : "step"), fmt("form=%s j=%d C=%d fun=%d it=%d", F.name, j, C, fun, it));
    if (g_list) return;
    const int nn = 2 * j;
    const bool pos = fun >= 5;
    const std::vector<int> vars = variants_of(j);
    const int nv = (int)vars.size();
    // per variant: reference Xm and its bound
    std::vector<ld_t> xref(nv), xbound(nv);
    ld_t tol_l = 1e-30L;
    for (int k = 0; k < nv; ++k) {
        const Variant& v = variant(j, vars[k], pos);
        ld_t x = 0, sf = 0, sfp = 0;
        for (int i = 0; i < nn; ++i) {
            const ld_t f1 = fscalar<ld_t>(fun, v.l1[i]), f2 = fscalar<ld_t>(fun, v.l2[i]);
            x += f1 - f2;
            sf += fabsl(f1) + fabsl(f2);
            sfp += fabsl(fprime(fun, v.l1[i])) + fabsl(fprime(fun, v.l2[i]));
        }
        xref[k] = vars[k] == V_LANCZOS0 ? 0.0L : x;
        xbound[k] = vars[k] == V_LANCZOS0 ? 0.0L : (ld_t)K_EIG * U * v.rho * sfp + gam(nn + 8) * sf;
        tol_l = std::max(tol_l, 64 * xbound[k]);
    }
    const double tol = (double)tol_l;
    dvec hist((size_t)j * C * 11), Cm((size_t)C * 4), state((size_t)C * PS_N + GUARD, SENT);
    for (int c = 0; c < C; ++c) {
        const int k = c % nv, mode = c % NMODE;
        const Variant& v = variant(j, vars[k], pos);
        for (int b = 0; b < j; ++b) memcpy(&hist[((size_t)b * C + c) * 11], &v.rec[(size_t)b * 11], 88);
        double* hj = &hist[((size_t)(j - 1) * C + c) * 11];
        if (mode == M_LUCKY || mode == M_NOTLUCKY) {
            const double r = mode == M_LUCKY ? 0.9e-8 : 1.1e-8;
            hj[8] = 0.6 * r;
            hj[9] = -0.8 * r;
            hj[10] = 1e-11;
        }
        memcpy(&Cm[(size_t)c * 4], v.cm, 32);
        double* st = &state[(size_t)c * PS_N];
        st[PS_DONE] = mode == M_DONE ? 1.0 : 0.0;
        const double xr = (double)xref[k];
        if (mode == M_STOP) {
            st[PS_X0] = xr + 0.2 * tol;
            st[PS_X1] = xr + 100.0 * tol;
        } else {
            st[PS_X0] = xr + 5.0 * tol;
            st[PS_X1] = xr - 0.125 * tol;
        }
        if (j > 2 && mode != M_DONE) {  // the reference decision is a factor 4 from tol
            const double dist = fabs(xr - st[PS_X0]);
            if (mode == M_STOP ? !(dist <= 0.25 * tol) : !(dist >= 4.0 * tol)) setup_die("stop margin");
        }
    }
    ivec active(1 + GUARD, ISENT);
    setenv("KT_PAIRS_DENSE_EIG", F.dense ? "1" : "0", 1);
    const bool one = F.dense && nn > 56;
    const size_t sstride = one ? (size_t)2 * nn * nn + 3 * nn + 5 : 0;
    dvec scratch(one ? sstride * C + GUARD : 0, SENT);
    dvec out[2];
    ivec aout[2];
    dvec sout;
    for (int run = 0; run < (g_host ? 1 : 2); ++run) {
        g_work.off = 0;
        const double* dh = up(hist);
        const double* dcm = up(Cm);
        double* dst = up(state);
        int* dact = up(active);
        double* dscr = one ? up(scratch) : nullptr;
        if (g_host) LAUNCH(host::pair_eig(C, j, it, fun, tol, dh, dcm, dst, dact));
        else LAUNCH(kt::launch_pair_eig(C, j, it, fun, tol, dh, dcm, dscr, (int64_t)sstride, dst, dact, nullptr));
        out[run] = down(dst, state.size());
        aout[run] = down(dact, active.size());
        if (one && run == 0) sout = down(dscr, scratch.size());
    }
    if (!g_host) {
        for (size_t t = 0; t < state.size(); ++t)
            if (bits_of(out[0][t]) != bits_of(out[1][t])) cs.fail("second run differs", (long)t, out[1][t], out[0][t], 0.0, INFINITY);
        cs.iunchanged("second run differs (active)", aout[0], aout[1]);
    }
    const dvec& o = out[0];
    int live = 0;
    for (int c = 0; c < C; ++c) {
        const int k = c % nv, mode = c % NMODE;
        const double* s0 = &state[(size_t)c * PS_N];
        const double* s1 = &o[(size_t)c * PS_N];
        const long ix = (long)c * PS_N;
        if (mode == M_DONE) {
            for (int t = 0; t < PS_N; ++t) cs.same("done candidate changed", ix + t, s1[t], s0[t]);
            continue;
        }
        if (vars[k] == V_LANCZOS0) cs.same("Xm with Cm = 0", ix + PS_XM, s1[PS_XM], 0.0);
        else cs.bounded(fmt("Xm (%s)", kVarName[vars[k]]).c_str(), ix + PS_XM, s1[PS_XM], xref[k], xbound[k]);
        const bool lucky = mode == M_LUCKY;
        cs.same("lucky", ix + PS_LUCKY, s1[PS_LUCKY], lucky ? 1.0 : 0.0);
        bool stop = false;
        if (j <= 2) {
            cs.same("X[j-1] = Xm", ix + j - 1, s1[PS_X0 + j - 1], s1[PS_XM]);
            cs.same("other X slot", ix + 2 - j, s1[PS_X0 + 2 - j], s0[PS_X0 + 2 - j]);
        } else if (mode == M_STOP) {
            stop = true;
            cs.same("X0 on stop", ix, s1[PS_X0], s0[PS_X0]);
            cs.same("X1 on stop", ix + 1, s1[PS_X1], s0[PS_X1]);
        } else {
            cs.same("X0 <- X1", ix, s1[PS_X0], s0[PS_X1]);
            cs.same("X1 <- Xm", ix + 1, s1[PS_X1], s1[PS_XM]);
        }
        const bool done = stop || lucky || j == it;
        cs.same("done", ix + PS_DONE, s1[PS_DONE], done ? 1.0 : 0.0);
        cs.same("iter", ix + PS_ITER, s1[PS_ITER], done ? (double)j : s0[PS_ITER]);
        cs.same("slot 6", ix + 6, s1[6], s0[6]);
        cs.same("slot 7", ix + 7, s1[7], s0[7]);
        live += !done;
    }
    cs.unchanged("guard", state, o, (size_t)C * PS_N);
    cs.ieq("active[0]", 0, aout[0][0], live);
    cs.iunchanged("active guard", active, aout[0], 1);
    if (one) {
        for (int c = 0; c < C; ++c)
            for (size_t t = sstride - 5; t < sstride; ++t) cs.same("scratch pad", (long)(c * sstride + t), sout[c * sstride + t], SENT);
        cs.unchanged("scratch guard", scratch, sout, sstride * C);
    }
}

static void grp_eig() {
    const std::vector<int> Cs = g_small ? std::vector<int>{65} : std::vector<int>{1, 63, 64, 65, 257};
    const std::vector<int> funs = g_small ? std::vector<int>{0, 5} : std::vector<int>{0, 1, 2, 3, 4, 5, 6};
    if (!g_list) {  // every reference spectrum the cases below use, solved together
        std::vector<Variant*> fresh;
        for (const EigForm& F : kEigForms)
            for (int j : F.depths) {
                if (g_small && j > 33) continue;
                for (int var : variants_of(j))
                    for (int fun : funs) {
                        bool f;
                        Variant* v = variant_slot(j, var, fun >= 5, &f);
                        if (f) fresh.push_back(v);
                    }
            }
        const auto t0 = std::chrono::steady_clock::now();
        solve_variants(fresh);
        fprintf(stderr, "pairs_check: reference spectra in %.2f s\n",
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    for (const EigForm& F : kEigForms)
        for (int j : F.depths) {
            if (g_small && j > 33) continue;
            for (int C : Cs)
                for (int fun : funs)
                    if (strcmp(F.name, "one") || fun == 0 || C == 65) eig_case(F, j, C, fun, j + 3);
            eig_case(F, j, 65, 0, j);
        }
    setenv("KT_PAIRS_DENSE_EIG", "0", 1);
    if (g_host && !g_list && g_mut.empty()) fprintf(stderr, "pairs_check: r_host = %.3f (K_eig = %g)\n", g_r_host, K_EIG);
}

// ---------------------------------------------------------------------------
// edit
// ---------------------------------------------------------------------------
struct EditGraph {
    int n = 0, lt = 8;
    ivec rp, ci, lr;
    dvec va;
    int deg(int r) const { return rp[r + 1] - rp[r]; }
    bool has(int r, int c) const {
        for (int k = rp[r]; k < rp[r + 1]; ++k)
            if (ci[k] == c) return true;
        return false;
    }
};
static EditGraph g_eg;

static void edit_graph_init() {
    EditGraph& G = g_eg;
    const int n = G.n = 1500;
    std::vector<std::vector<int>> adj(n);
    auto add = [&](int a, int b) {
        if (std::find(adj[a].begin(), adj[a].end(), b) != adj[a].end()) return;
        adj[a].push_back(b);
        if (a != b) adj[b].push_back(a);
    };
    for (int r = 0; r < n; ++r) add(r, (r + 1) % n);
    for (int r = 0; r < n; r += 3) add(r, (r + 701) % n);
    for (int r : {5, 700, 999, 1499}) add(r, r);  // self loops
    auto grow = [&](int hub, int want, int stride) {
        for (int t = 1; (int)adj[hub].size() < want; ++t) {
            const int c = (hub + 13 + t * stride) % n;
            if (c == 40 || c == 10 || c == 700 || c == 1200) continue;
            add(hub, c);
        }
    };
    add(700, 1200);  // an edge between two rows at long_thresh + 1
    grow(40, 20, 37);
    grow(10, 12, 41);
    grow(700, 9, 43);
    grow(1200, 9, 47);
    G.rp.assign(n + 1, 0);
    for (int r = 0; r < n; ++r) {
        std::sort(adj[r].begin(), adj[r].end());
        G.rp[r + 1] = G.rp[r] + (int)adj[r].size();
        for (int c : adj[r]) {
            G.ci.push_back(c);
            const int a = std::min(r, c), b = std::max(r, c);
            G.va.push_back(1.0 + a * 0.001 + b * 1e-7);  // symmetric, distinct by position
        }
    }
    for (int r = 0; r < n; ++r)
        if (G.deg(r) > G.lt) G.lr.push_back(r);
    std::stable_sort(G.lr.begin(), G.lr.end(), [&](int a, int b) { return G.deg(a) > G.deg(b); });
    if (G.lr != ivec{40, 10, 700, 1200} || G.deg(700) != 9 || G.deg(1200) != 9 || G.deg(40) != 20 || G.deg(10) != 12)
        setup_die("edit graph long rows");
}

struct EditSpec {
    const char* name;
    int C, nT;
    ivec minima;       // candidates holding the smallest score (ties); empty: none finite
    ivec nans;         // candidates holding NaN
    const char* edge;  // ordinary, self, absent, long, twolong
    int step;
    bool none_inf;     // with empty minima: +inf scores (else NaN)
};

static void edit_case(const EditSpec& S) {
    Case cs(G_EDIT, S.name, fmt("C=%d nT=%d edge=%s step=%d ties=%d nan=%d", S.C, S.nT, S.edge, S.step,
                                (int)S.minima.size(), (int)S.nans.size()));
    if (g_list) return;
    const EditGraph& G = g_eg;
    const int n = G.n, nnz = (int)G.ci.size(), C = S.C, nT = S.nT;
    const int cap = nnz + 37;
    g_rng = 0x9E3779B97F4A7C15ull + (uint64_t)C * 7 + nT;
    dvec state((size_t)C * PS_N + GUARD, NAN);
    for (int c = 0; c < C; ++c) state[(size_t)c * PS_N + PS_XM] = 5.0 + (double)(rnd() % 1000);
    for (int c : S.minima) state[(size_t)c * PS_N + PS_XM] = -2.5;
    for (int c : S.nans) state[(size_t)c * PS_N + PS_XM] = NAN;
    if (S.minima.empty())
        for (int c = 0; c < C; ++c) state[(size_t)c * PS_N + PS_XM] = (S.none_inf && !(c & 1)) ? INFINITY : NAN;
    const int best = S.minima.empty() ? -1 : *std::min_element(S.minima.begin(), S.minima.end());
    // the ranking: existing ordinary edges (both orders), the selected entry by kind
    ivec Ti(nT + GUARD, ISENT), Tj(nT + GUARD, ISENT);
    for (int t = 0; t < nT; ++t) {
        const int r = (int)(rnd() % n);
        Ti[t] = r;
        Tj[t] = G.ci[G.rp[r] + (int)(rnd() % G.deg(r))];
    }
    // every tied candidate other than the first names an edge that must stay
    for (int c : S.minima) {
        Ti[c] = 300 + 3 * (c % 50);
        Tj[c] = Ti[c] + 1;
    }
    int e1 = -1, e2 = -1;
    if (!strcmp(S.edge, "ordinary")) e1 = 601, e2 = 600;
    else if (!strcmp(S.edge, "self")) e1 = e2 = 999;
    else if (!strcmp(S.edge, "absent")) e1 = 2, e2 = 900;
    else if (!strcmp(S.edge, "long")) e1 = 1200, e2 = G.ci[G.rp[1200]];
    else if (!strcmp(S.edge, "twolong")) e1 = 700, e2 = 1200;
    else setup_die("edge kind");
    const bool present = G.has(e1, e2);
    if (present != (strcmp(S.edge, "absent") != 0) || G.has(e1, e2) != G.has(e2, e1)) setup_die("edit edge");
    if (best >= 0) {
        Ti[best] = e1;
        Tj[best] = e2;
    }
    ivec rp = G.rp, ci = G.ci, lr = G.lr, dyn = {nnz, (int)G.lr.size()};
    dvec va = G.va;
    ci.resize(cap, ISENT);  // beyond dyn[0]: must not be copied
    va.resize(cap, NAN);
    lr.resize(lr.size() + 3, ISENT);
    ivec rp2(n + 1 + GUARD, ISENT), ci2(cap + GUARD, ISENT), lr2(G.lr.size() + GUARD, ISENT), dyn2(2 + GUARD, ISENT);
    dvec va2(cap + GUARD, SENT), selv(S.step + 1 + GUARD, SENT);
    ivec sel(2 * (S.step + 1) + GUARD, ISENT);
    // ---- reference: the edit on (row, column, weight) triples
    ivec xTi = Ti, xTj = Tj, xrp2 = rp2, xci2 = ci2, xlr2 = lr2, xdyn2 = dyn2, xsel = sel;
    dvec xva2 = va2, xselv = selv;
    const bool refuse = nT > 4096;
    if (!refuse) {
        xsel[2 * S.step] = best >= 0 ? e1 : -1;
        xsel[2 * S.step + 1] = best >= 0 ? e2 : -1;
        xselv[S.step] = best >= 0 ? -2.5 : INFINITY;
        if (best >= 0) {
            xTi.erase(xTi.begin() + best);
            xTj.erase(xTj.begin() + best);
            xTi.insert(xTi.begin() + nT - 1, Ti[nT - 1]);  // slot nT - 1 keeps its value
            xTj.insert(xTj.begin() + nT - 1, Tj[nT - 1]);
        }
        ivec cnt(n, 0);
        int d = 0;
        for (int r = 0; r < n; ++r)
            for (int k = G.rp[r]; k < G.rp[r + 1]; ++k) {
                const int c = G.ci[k];
                if (best >= 0 && ((r == e1 && c == e2) || (r == e2 && c == e1))) continue;
                xci2[d] = c;
                xva2[d] = G.va[k];
                ++d;
                ++cnt[r];
            }
        xrp2[0] = 0;
        for (int r = 0; r < n; ++r) xrp2[r + 1] = xrp2[r] + cnt[r];
        int m = 0;
        for (int r : G.lr)
            if (cnt[r] > G.lt) xlr2[m++] = r;
        xdyn2[0] = d;
        xdyn2[1] = m;
        if (!strcmp(S.edge, "long") && best >= 0 && (m != 3 || xlr2[2] != 700)) setup_die("long row case");
        if (!strcmp(S.edge, "twolong") && best >= 0 && m != 2) setup_die("two long rows case");
    }
    // ---- run (twice on the device)
    struct Out {
        ivec Ti, Tj, rp2, ci2, lr2, dyn2, sel, rp, ci, lr, dyn;
        dvec va2, selv, state, va;
    } o[2];
    for (int run = 0; run < (g_host ? 1 : 2); ++run) {
        g_work.off = 0;
        const double* dstate = up(state);
        int *dTi = up(Ti), *dTj = up(Tj);
        int *drp = up(rp), *dci = up(ci), *dlr = up(lr), *ddyn = up(dyn);
        double* dva = up(va);
        int *drp2 = up(rp2), *dci2 = up(ci2), *dlr2 = up(lr2), *ddyn2 = up(dyn2), *dsel = up(sel);
        double *dva2 = up(va2), *dselv = up(selv);
        const hipError_t e =
            g_host ? host::greedy_edit(C, dstate, dTi, dTj, nT, n, G.lt, drp, dci, dva, dlr, ddyn, drp2, dci2, dva2, dlr2,
                                       ddyn2, S.step, dsel, dselv)
                   : kt::launch_greedy_edit(C, dstate, dTi, dTj, nT, n, G.lt, drp, dci, dva, dlr, ddyn, drp2, dci2, dva2,
                                            dlr2, ddyn2, S.step, dsel, dselv, nullptr);
        if (refuse) {
            if (e != hipErrorInvalidValue) cs.fail("nT > 4096 must return hipErrorInvalidValue", 0, (double)e, (double)hipErrorInvalidValue, 0.0, INFINITY);
            if (e != hipSuccess) (void)hipGetLastError();
        } else {
            HC(e);
        }
        if (!g_host) HC(hipDeviceSynchronize());
        Out& O = o[run];
        O.Ti = down(dTi, Ti.size());
        O.Tj = down(dTj, Tj.size());
        O.rp2 = down(drp2, rp2.size());
        O.ci2 = down(dci2, ci2.size());
        O.lr2 = down(dlr2, lr2.size());
        O.dyn2 = down(ddyn2, dyn2.size());
        O.sel = down(dsel, sel.size());
        O.va2 = down(dva2, va2.size());
        O.selv = down(dselv, selv.size());
        O.state = down(dstate, state.size());
        O.rp = down(drp, rp.size());
        O.ci = down(dci, ci.size());
        O.lr = down(dlr, lr.size());
        O.dyn = down(ddyn, dyn.size());
        O.va = down(dva, va.size());
    }
    for (int run = 0; run < (g_host ? 1 : 2); ++run) {
        const Out& O = o[run];
        const char* sfx = run ? " (second run)" : "";
        auto w = [&](const char* s) { return std::string(s) + sfx; };
        // slot nT - 1 of the ranking is left to the kernel (it keeps the old value)
        cs.iunchanged(w("Ti").c_str(), xTi, O.Ti);
        cs.iunchanged(w("Tj").c_str(), xTj, O.Tj);
        cs.iunchanged(w("rp2").c_str(), xrp2, O.rp2);
        cs.iunchanged(w("ci2").c_str(), xci2, O.ci2);
        cs.iunchanged(w("lr2").c_str(), xlr2, O.lr2);
        cs.iunchanged(w("dyn2").c_str(), xdyn2, O.dyn2);
        cs.iunchanged(w("sel").c_str(), xsel, O.sel);
        cs.unchanged(w("va2").c_str(), xva2, O.va2);
        cs.unchanged(w("selv").c_str(), xselv, O.selv);
        cs.unchanged(w("state (input)").c_str(), state, O.state);
        cs.iunchanged(w("rp (input)").c_str(), rp, O.rp);
        cs.iunchanged(w("ci (input)").c_str(), ci, O.ci);
        cs.iunchanged(w("lr (input)").c_str(), lr, O.lr);
        cs.iunchanged(w("dyn (input)").c_str(), dyn, O.dyn);
        cs.unchanged(w("va (input)").c_str(), va, O.va);
    }
}

static void grp_edit() {
    const std::vector<EditSpec> specs = {
        {"one_candidate", 1, 1, {0}, {}, "ordinary", 0, false},
        {"one_candidate_nT4096", 1, 4096, {0}, {}, "self", 3, false},
        {"rank0", 5, 5, {0}, {}, "ordinary", 0, false},
        {"middle", 5, 5, {2}, {4}, "self", 0, false},
        {"last_of_nT", 5, 5, {4}, {0}, "absent", 3, false},
        {"tie_lanes", 1024, 1024, {40, 3}, {}, "ordinary", 0, false},
        {"tie_waves", 1024, 4096, {900, 100, 515}, {0, 1023}, "long", 0, false},
        {"last_of_nT_1024", 1024, 1024, {1023}, {5}, "twolong", 3, false},
        {"tie_in_thread", 1025, 1025, {1024, 0}, {}, "ordinary", 0, false},
        {"tie_in_thread_mid", 2500, 2500, {2071, 1047, 23}, {22, 24}, "self", 0, false},
        {"tie_later_index_lower_lane", 2500, 4096, {1030, 10}, {}, "long", 3, false},
        {"tie_wave_later_index_lower_wave", 2500, 2500, {1025 + 1024, 70}, {1}, "absent", 0, false},
        {"last_of_nT_2500", 2500, 2500, {2499}, {0, 2498}, "ordinary", 0, false},
        {"middle_nT4096", 1025, 4096, {600}, {}, "twolong", 0, false},
        {"all_nan", 5, 5, {}, {}, "ordinary", 0, false},
        {"all_nan_or_inf", 2500, 4096, {}, {}, "ordinary", 3, true},
        {"all_inf_one", 1, 1, {}, {}, "ordinary", 0, true},
        {"nT_4097_refused", 5, 4097, {2}, {}, "ordinary", 0, false},
    };
    for (const EditSpec& S : specs) edit_case(S);
}

// ---------------------------------------------------------------------------
// whole: launch_pair_fused / launch_pair_reg_dyn
// ---------------------------------------------------------------------------
static const double K_WHOLE = 256.0;  // max(K_eig, 8 r_whole); r_whole = 0.84 measured (--host)
static const int kLongThresh = 16;

struct WGraph {
    std::string name;
    int n = 0, it = 6;
    bool unit = false, self_pair = false;
    double wdiv = 4.0;  // the weights are (0.25 .. 1.75) / wdiv
    ivec rp, ci, lr;
    dvec va;       // the weights (the reference's; all 1 for unit)
    dvec va_dev;   // what the launcher gets: NaN for unit weights (never read)
    int cand[3][2];
    ld_t rhoA = 0;
    int rows = 0, csr = 0, spec = 0;  // pair_reg_form
    bool applies = false;
    int nnz() const { return (int)ci.size(); }
    int deg(int r) const { return rp[r + 1] - rp[r]; }
};

static void wgraph_finish(WGraph& G, std::vector<ivec>& adj) {
    const int n = G.n;
    G.rp.assign(n + 1, 0);
    for (int r = 0; r < n; ++r) {
        std::sort(adj[r].begin(), adj[r].end());
        G.rp[r + 1] = G.rp[r] + (int)adj[r].size();
        ld_t rs = 0;
        for (int c : adj[r]) {
            G.ci.push_back(c);
            const int a = std::min(r, c), b = std::max(r, c);
            const double w = G.unit ? 1.0 : (0.25 + ((a * 31 + b * 17) % 13) / 8.0) / G.wdiv;
            G.va.push_back(w);
            rs += w;
        }
        G.rhoA = std::max(G.rhoA, rs);
    }
    G.va_dev = G.unit ? dvec(G.va.size(), NAN) : G.va;
    for (int r = 0; r < n; ++r)
        if (G.deg(r) > kLongThresh) G.lr.push_back(r);
    std::stable_sort(G.lr.begin(), G.lr.end(), [&](int a, int b) { return G.deg(a) > G.deg(b); });
    setenv("KT_PAIRS_DENSE_EIG", "0", 1);
    setenv("KT_PAIRS_REG", "1", 1);
    G.applies = kt::pair_reg_form(n, G.nnz(), G.it, (int)G.lr.size(), G.unit, &G.rows, &G.csr, &G.spec);
}

// n rows, about target nonzeros, nlong designed long rows (70, 33, then 17 ..
// 20 entries) and one row at long_thresh; rows r % 11 == 5 stay empty
static WGraph make_wgraph(const char* name, int n, int target, int nlong, bool unit, bool self_pair, double wdiv) {
    WGraph G;
    G.wdiv = wdiv;
    G.name = name;
    G.n = n;
    G.unit = unit;
    G.self_pair = self_pair;
    uint64_t rng = 0x632BE59BD9B4E019ull + (uint64_t)n * 2654435761u + target;
    auto rnd_l = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    std::vector<ivec> adj(n);
    int nnz = 0;
    auto allowed = [&](int r) { return !(n >= 50 && r % 11 == 5); };
    auto add = [&](int a, int b) {
        if (std::find(adj[a].begin(), adj[a].end(), b) != adj[a].end()) return false;
        adj[a].push_back(b);
        ++nnz;
        if (a != b) {
            adj[b].push_back(a);
            ++nnz;
        }
        return true;
    };
    if (n < 50) {  // tiny: a path and one self loop; one Lanczos step
        for (int r = 0; r + 1 < n; ++r) add(r, r + 1);
        add(0, 0);
        G.it = 1;
        for (int c = 0; c < 3; ++c) {
            G.cand[c][0] = c % n;
            G.cand[c][1] = (c + 1) % n;
        }
        if (self_pair) G.cand[2][1] = G.cand[2][0];
        wgraph_finish(G, adj);
        return G;
    }
    std::vector<char> hub(n, 0);
    ivec hubs;
    for (int k = 0; k <= nlong; ++k) {  // the last one sits at long_thresh exactly
        int h = (7 + 3 * k) % n;
        while (!allowed(h) || hub[h]) h = (h + 1) % n;
        hub[h] = 1;
        hubs.push_back(h);
    }
    for (int k = 0; k <= nlong; ++k) {
        const int want = k == nlong ? kLongThresh : k == 0 ? 70 : k == 1 ? 33 : 17 + (k - 2) % 4;
        const int h = hubs[k];
        for (int t = 1; (int)adj[h].size() < want; ++t) {
            const int c = (int)((h + 1 + (uint64_t)t * 37) % n);
            if (allowed(c) && !hub[c] && (int)adj[c].size() < 9) add(h, c);
            if (t > 40 * n) setup_die("hub partners");
        }
    }
    // short rows: degrees around the 4-deep gather
    for (int r = 0; r < n && nnz < target; ++r) {
        if (!allowed(r) || hub[r]) continue;
        const int want = 1 + r % 9;
        for (int t = 0; t < 12 && (int)adj[r].size() < want; ++t) {
            const int c = (int)((r * 7 + 31 * t + 3) % n);
            if (c != r && allowed(c) && !hub[c] && (int)adj[c].size() < 9) add(r, c);
        }
        if (r % 97 == 3) add(r, r);
    }
    for (long tries = 0; nnz < target; ++tries) {
        const int a = (int)(rnd_l() % n), b = (int)(rnd_l() % n);
        if (a != b && allowed(a) && allowed(b) && !hub[a] && !hub[b] && (int)adj[a].size() < 14 && (int)adj[b].size() < 14) add(a, b);
        if (tries > 200L * target) setup_die("graph fill");
    }
    // candidates: an edge of the heaviest row, two more edges away from it
    const int h0 = hubs[0];
    G.cand[0][0] = adj[h0][0];
    for (int c : adj[h0])
        if (adj[c].size() > adj[G.cand[0][0]].size()) G.cand[0][0] = c;
    G.cand[0][1] = h0;
    int found = 1;
    for (int r = n / 3; r < n && found < 3; ++r)
        if (allowed(r) && !hub[r] && adj[r].size() >= 3 && adj[r][0] != r && r != G.cand[0][0]) {
            G.cand[found][0] = r;
            G.cand[found][1] = adj[r][0];
            ++found;
            r += n / 4;
        }
    if (found < 3) setup_die("candidates");
    if (self_pair) G.cand[2][1] = G.cand[2][0];
    wgraph_finish(G, adj);
    // the row classes the header names are there
    std::vector<char> has(128, 0);
    for (int r = 0; r < n; ++r) has[std::min(G.deg(r), 127)] = 1;
    for (int d : {0, 3, 4, 5, 7, 8, 9, kLongThresh})
        if (!has[d] && (nlong <= 3 || d == 0 || d == kLongThresh)) setup_die(fmt("graph %s has no row of %d entries", name, d));
    if (nlong > 0 && !(has[kLongThresh + 1] && has[33] && has[70])) setup_die(fmt("graph %s: long row classes", name));
    if ((nlong == 0) != G.lr.empty() || (nlong > 3 && (int)G.lr.size() <= kt::kRegLongCap)) setup_die(fmt("graph %s: n_long", name));
    return G;
}

static std::vector<WGraph> g_wgraphs;
static void wgraphs_init() {
    struct Spec {
        const char* name;
        int n, target, nlong;
        bool unit, self_pair;
        double wdiv = 4.0;
    };
    const std::vector<Spec> specs = {
        {"n2", 2, 0, 0, false, false},           {"n3", 3, 0, 0, true, true},
        {"n511", 511, 2200, 3, false, false},    {"n512", 512, 2200, 0, true, false},
        {"n513", 513, 2400, 3, true, true},      {"n1024", 1024, 4500, 0, false, false},
        {"n1025", 1025, 9000, 300, false, false, 16.0}, {"n2049", 2049, 9000, 3, false, false, 16.0},
        {"n3073", 3073, 12000, 0, false, true, 16.0},  {"n3585", 3585, 14000, 3, true, false},
        {"n4096a", 4096, 7400, 0, false, false}, {"n4096b", 4096, 20000, 3, false, false},
        {"n4096c", 4096, 46000, 3, true, false}, {"n4096d", 4096, 46000, 300, false, true},
        {"n4097", 4097, 16000, 3, false, false},
    };
    for (const Spec& S : specs) {
        if (g_small && strcmp(S.name, "n3") && strcmp(S.name, "n513") && strcmp(S.name, "n1025") && strcmp(S.name, "n4096a")) continue;
        g_wgraphs.push_back(make_wgraph(S.name, S.n, S.target, S.nlong, S.unit, S.self_pair, S.wdiv));
    }
}

static const double kWholeB[4] = {0.3, -1.0, -1.0, -0.2};  // column-major 2 x 2

// ---- long double reference of one candidate's run
struct WholeRef {
    std::vector<ld_t> xm;     // per step
    std::vector<ld_t> bound;  // per step, without the K factor: u rho sum|f'| and gamma sum|f|
    std::vector<ld_t> gterm;
    std::vector<ld_t> rnorm, rmin;  // |R|_F and min(|R11|, |R22|) per step
};

static void whole_ref(const WGraph& G, int ci_, int cj_, int fun, WholeRef& o) {
    const int n = G.n, it = G.it;
    lvec prev[2], cur[2] = {lvec(n, 0), lvec(n, 0)};
    ld_t R0[4] = {1, 0, 0, 1};  // row-major [R00 R01; R10 R11]
    cur[0][ci_] = 1;
    if (ci_ != cj_) {
        cur[1][cj_] = 1;
    } else {  // qr([e_i e_i]): LAPACK completes with e_1 (e_0 for i = 1); R = [1 1; 0 0] up to signs
        cur[1][ci_ == 1 ? 0 : ci_ == 0 ? 1 : 1] = 1;
        R0[1] = 1;
        R0[3] = 0;
    }
    const double* B = kWholeB;  // b00 b10 b01 b11
    const ld_t RB00 = R0[0] * B[0] + R0[1] * B[1], RB01 = R0[0] * B[2] + R0[1] * B[3];
    const ld_t RB10 = R0[3] * B[1], RB11 = R0[3] * B[3];
    const ld_t cm[4] = {RB00 * R0[0] + RB01 * R0[1], RB10 * R0[0] + RB11 * R0[1], RB01 * R0[3], RB11 * R0[3]};  // column-major
    auto dot = [&](const lvec& x, const lvec& y) {
        ld_t s = 0;
        for (int r = 0; r < n; ++r) s += x[r] * y[r];
        return s;
    };
    std::vector<ld_t> Dk, Rk;  // per step: D (a, b, c), R (r11, r12, r22)
    for (int j = 1; j <= it; ++j) {
        lvec w[2] = {lvec(n, 0), lvec(n, 0)};
        for (int s = 0; s < 2; ++s)
            for (int r = 0; r < n; ++r) {
                ld_t acc = 0;
                for (int k = G.rp[r]; k < G.rp[r + 1]; ++k) acc += (ld_t)G.va[k] * cur[s][G.ci[k]];
                w[s][r] = acc;
            }
        ld_t D[4];  // cur' A cur
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 2; ++k) D[2 * s + k] = dot(cur[k], w[s]);
        for (int pass = 0; pass < 2; ++pass)
            for (int s = 0; s < 2; ++s)
                for (const lvec* v : {&prev[0], &prev[1], &cur[0], &cur[1]}) {
                    if (v->empty()) continue;
                    const ld_t g = dot(*v, w[s]);
                    for (int r = 0; r < n; ++r) w[s][r] -= g * (*v)[r];
                }
        const ld_t r11 = sqrtl(dot(w[0], w[0]));
        if (r11 > 0)
            for (ld_t& x : w[0]) x /= r11;
        const ld_t r12 = dot(w[0], w[1]);
        for (int r = 0; r < n; ++r) w[1][r] -= r12 * w[0][r];
        const ld_t r22 = sqrtl(dot(w[1], w[1]));
        if (r22 > 0)
            for (ld_t& x : w[1]) x /= r22;
        Dk.push_back(D[0]);
        Dk.push_back(0.5L * (D[1] + D[2]));
        Dk.push_back(D[3]);
        Rk.push_back(r11);
        Rk.push_back(r12);
        Rk.push_back(r22);
        o.rnorm.push_back(sqrtl(r11 * r11 + r12 * r12 + r22 * r22));
        o.rmin.push_back(std::min(r11, r22));
        const int nn = 2 * j;
        lvec Gm((size_t)nn * nn, 0);
        for (int b = 0; b < j; ++b) {
            Gm[(size_t)(2 * b) * nn + 2 * b] = Dk[3 * b];
            Gm[(size_t)(2 * b + 1) * nn + 2 * b] = Gm[(size_t)(2 * b) * nn + 2 * b + 1] = Dk[3 * b + 1];
            Gm[(size_t)(2 * b + 1) * nn + 2 * b + 1] = Dk[3 * b + 2];
            if (b + 1 < j) {  // R_b at (2b+2.., 2b..), its transpose above
                const ld_t* R = &Rk[3 * b];
                Gm[(size_t)(2 * b + 2) * nn + 2 * b] = Gm[(size_t)(2 * b) * nn + 2 * b + 2] = R[0];
                Gm[(size_t)(2 * b + 2) * nn + 2 * b + 1] = Gm[(size_t)(2 * b + 1) * nn + 2 * b + 2] = R[1];
                Gm[(size_t)(2 * b + 3) * nn + 2 * b + 1] = Gm[(size_t)(2 * b + 1) * nn + 2 * b + 3] = R[2];
            }
        }
        lvec Tm = Gm;
        Tm[0] += cm[0];
        Tm[1] += 0.5L * (cm[1] + cm[2]);
        Tm[nn] += 0.5L * (cm[1] + cm[2]);
        Tm[nn + 1] += cm[3];
        ld_t rho = 0;
        for (const lvec* X : {&Gm, &Tm})
            for (int r = 0; r < nn; ++r) {
                ld_t s = 0;
                for (int q = 0; q < nn; ++q) s += fabsl((*X)[(size_t)r * nn + q]);
                rho = std::max(rho, s);
            }
        const lvec l1 = jacobi_eig<ld_t>(nn, Tm), l2 = jacobi_eig<ld_t>(nn, Gm);
        ld_t x = 0, sf = 0, sfp = 0;
        for (int i = 0; i < nn; ++i) {
            const ld_t f1 = fscalar<ld_t>(fun, l1[i]), f2 = fscalar<ld_t>(fun, l2[i]);
            x += f1 - f2;
            sf += fabsl(f1) + fabsl(f2);
            sfp += fabsl(fprime(fun, l1[i])) + fabsl(fprime(fun, l2[i]));
        }
        o.xm.push_back(x);
        o.bound.push_back(U * rho * sfp);
        o.gterm.push_back(gam(nn + 8) * sf);
        prev[0] = cur[0];
        prev[1] = cur[1];
        cur[0] = w[0];
        cur[1] = w[1];
    }
}

namespace host {
// the whole run of every candidate in fp64: qr(U) and CGS2 + Householder by
// the orth stand-in, the projections as launch_pair_eig's stand-in forms them,
// Jacobi, the lag-2 stop (kt_launch.h: launch_pair_fused)
static hipError_t pair_fused(int C, int n, const kt::CsrView& A, bool unit, const int* ii, const int* jj,
                             const double* B, int it, int fun, double tol, double* state) {
    g_whole_scope = true;
    for (int c = 0; c < C; ++c) {
        dvec V[3] = {dvec(2 * (size_t)n, 0.0), dvec(2 * (size_t)n, 0.0), dvec(2 * (size_t)n, 0.0)};
        dvec coef(CF_NCOEF), part(kt::pairs_part_doubles(n, 1, 1)), hist((size_t)it * 11);
        double rec0[11];
        V[0][2 * (size_t)ii[c]] = 1.0;
        V[0][2 * (size_t)jj[c] + 1] = 1.0;
        (void)pairs_orth(1, n, 1, nullptr, nullptr, V[0].data(), 2, coef.data(), part.data(), rec0, nullptr);
        const double R00 = rec0[8], R01 = mut("whole_cm_without_r12") ? 0.0 : rec0[9], R11 = rec0[10];
        const double RB00 = R00 * B[0] + R01 * B[1], RB01 = R00 * B[2] + R01 * B[3];
        const double RB10 = R11 * B[1], RB11 = R11 * B[3];
        const double cm[4] = {RB00 * R00 + RB01 * R01, RB10 * R00 + RB11 * R01, RB01 * R11, RB11 * R11};
        int prev = -1, cur = 0, w = 1, iter = it;
        double x0 = 0.0, x1 = 0.0, xm = 0.0;
        bool lucky = false;
        for (int j = 1; j <= it; ++j) {
            for (int r = 0; r < n; ++r) {
                double s0 = 0.0, s1 = 0.0;
                if (!(mut("whole_long_rows_skipped") && A.rp[r + 1] - A.rp[r] > A.long_thresh))
                    for (int k = A.rp[r]; k < A.rp[r + 1]; ++k) {
                        const double a = unit ? 1.0 : A.va[k];
                        s0 += a * V[cur][2 * (size_t)A.ci[k]];
                        s1 += a * V[cur][2 * (size_t)A.ci[k] + 1];
                    }
                V[w][2 * (size_t)r] = s0;
                V[w][2 * (size_t)r + 1] = s1;
            }
            double* h = &hist[(size_t)(j - 1) * 11];
            (void)pairs_orth(1, n, 1, prev >= 0 ? V[prev].data() : nullptr, V[cur].data(), V[w].data(), 2, coef.data(),
                       part.data(), h, nullptr);
            dvec Gm, Tm;
            place_projections(j, hist.data(), 11, cm, true, Gm, Tm);
            const dvec l1 = jacobi_eig<double>(2 * j, Tm), l2 = jacobi_eig<double>(2 * j, Gm);
            xm = 0.0;
            for (int k = 0; k < 2 * j; ++k) xm += fscalar<double>(fun, l1[k]) - fscalar<double>(fun, l2[k]);
            lucky = sqrt(h[8] * h[8] + h[9] * h[9] + h[10] * h[10]) < 1e-8;
            bool stop = false;
            if (j == 1) x0 = xm;
            else if (j == 2) x1 = xm;
            else if (fabs(xm - x0) < tol) stop = true;
            else {
                x0 = x1;
                x1 = xm;
            }
            if (stop || lucky || j == it) {
                iter = j;
                break;
            }
            const int freed = prev >= 0 ? prev : 3 - cur - w;
            prev = cur;
            cur = w;
            w = freed;
        }
        double* st = state + (size_t)c * PS_N;
        st[PS_XM] = xm;
        st[PS_ITER] = iter;
        st[PS_LUCKY] = lucky ? 1.0 : 0.0;
        st[PS_DONE] = 1.0;
    }
    g_whole_scope = false;
    return hipSuccess;
}
}  // namespace host

static bool wgraph_has_mid(const WGraph& G);
static void wgraphs_print() {
    if (g_wgraphs.empty()) wgraphs_init();
    for (size_t i = 0; i < g_wgraphs.size(); ++i) {
        const WGraph& G = g_wgraphs[i];
        printf("%s{\"graph\": \"%s\", \"n\": %d, \"nnz\": %d, \"n_long\": %d, \"unit\": %d, \"applies\": %d, \"rows\": %d, "
               "\"csr\": %d, \"spec\": %d, \"has_long\": %d, \"mid\": %d}",
               i ? ", " : "", G.name.c_str(), G.n, G.nnz(), (int)G.lr.size(), (int)G.unit, (int)G.applies, G.rows, G.csr,
               G.spec, (int)!G.lr.empty(), (int)wgraph_has_mid(G));
    }
}

static double g_r_whole = 0.0;

enum { WF_REG, WF_FUSED_BLK, WF_FUSED_DENSE, WF_DYN };
static const char* kWholeForm[] = {"default", "fused_blk", "fused_dense", "reg_dyn"};
enum { WT_NEVER, WT_ALWAYS, WT_MID };
static const char* kWholeTol[] = {"never", "always", "mid"};

struct WholeDev {  // one CSR on the device (or host) side
    kt::CsrView view;
    const int* dyn;
};
static WholeDev whole_upload(const WGraph& G, const ivec& rp, const ivec& ci, const dvec& va, const ivec& lr, int nnz,
                             int n_long_view) {
    WholeDev D;
    memset(&D.view, 0, sizeof D.view);
    ivec lrp = lr;
    lrp.resize(lr.size() + 4, ISENT);
    D.view.rp = up(rp);
    D.view.ci = up(ci);
    D.view.va = up(va);
    D.view.n = G.n;
    D.view.long_rows = up(lrp);
    D.view.n_long = n_long_view;
    D.view.long_thresh = kLongThresh;
    D.view.split_thresh = 64;
    D.dyn = up(ivec{nnz, (int)lr.size()});
    return D;
}

// The `mid` tolerance of a graph: 4 x one candidate's lag-2 difference at a
// step 4 <= J < it, the first for which that candidate stops at J and every
// decision of every candidate keeps a factor 4 from it.  Graphs without one
// have no `mid` cases (the enumeration, --count included, leaves them out).
static int whole_fun(const WGraph& G) { return G.n % 3 == 0 ? 2 : G.n % 3 == 1 ? 0 : 4; }  // cosh, exp, cos
struct MidTol {
    bool found = false;
    double tol = 0.0;
};
static const MidTol& mid_tol(const WGraph& G, int fun) {
    static std::map<std::string, MidTol> cache;
    auto hit = cache.find(G.name);
    if (hit != cache.end()) return hit->second;
    MidTol& m = cache[G.name];
    const int C = 3, it = G.it;
    std::vector<WholeRef> ref(C);
    for (int c = 0; c < C; ++c) whole_ref(G, G.cand[c][0], G.cand[c][1], fun, ref[c]);
    for (int c = 0; c < C && !m.found; ++c)
        for (int J = 4; J < it && !m.found; ++J) {
            const double cand_tol = (double)(4 * fabsl(ref[c].xm[J - 1] - ref[c].xm[J - 3]));
            bool ok = cand_tol > 0;
            for (int c2 = 0; c2 < C && ok; ++c2)
                for (int j = 3; j <= it && ok; ++j) {
                    const ld_t d = fabsl(ref[c2].xm[j - 1] - ref[c2].xm[j - 3]);
                    if (!(d <= cand_tol / 4 || d >= 4 * (ld_t)cand_tol)) ok = false;
                    if (d <= cand_tol / 4) break;  // stopped: later steps do not run
                }
            if (ok && fabsl(ref[c].xm[2] - ref[c].xm[0]) >= 4 * (ld_t)cand_tol) {
                m.tol = cand_tol;
                m.found = true;
            }
        }
    return m;
}

static bool wgraph_has_mid(const WGraph& G) { return mid_tol(G, whole_fun(G)).found; }

static void whole_case(const WGraph& G, int form, int tolmode, int fun) {
    if (tolmode == WT_MID && !mid_tol(G, fun).found) return;
    Case cs(G_WHOLE, fmt("%s_%s", kWholeForm[form], kWholeTol[tolmode]),
            fmt("graph=%s n=%d nnz=%d n_long=%d unit=%d it=%d fun=%d rows=%d csr=%d spec=%d", G.name.c_str(), G.n, G.nnz(),
                (int)G.lr.size(), (int)G.unit, G.it, fun, G.rows, G.csr, G.spec));
    if (g_list) return;
    const int C = 3, n = G.n, it = G.it;
    // the matrix of this case: the graph, or (reg_dyn) the graph with candidate 1's edge deleted
    ivec rp = G.rp, ci = G.ci, lr = G.lr;
    dvec va = G.va, vad = G.va_dev;
    WGraph E = G;  // the reference's matrix
    if (form == WF_DYN) {
        const int e1 = G.cand[1][0], e2 = G.cand[1][1];
        E.rp.assign(n + 1, 0);
        E.ci.clear();
        E.va.clear();
        E.va_dev.clear();
        E.lr.clear();
        for (int r = 0; r < n; ++r) {
            for (int k = G.rp[r]; k < G.rp[r + 1]; ++k) {
                if ((r == e1 && G.ci[k] == e2) || (r == e2 && G.ci[k] == e1)) continue;
                E.ci.push_back(G.ci[k]);
                E.va.push_back(G.va[k]);
                E.va_dev.push_back(G.va_dev[k]);
            }
            E.rp[r + 1] = (int)E.ci.size();
        }
        for (int r : G.lr)
            if (E.deg(r) > kLongThresh) E.lr.push_back(r);
        if (E.nnz() != G.nnz() - 2) setup_die("reg_dyn edit");
    }
    // reference runs (every step, no stop), then the tolerance and the decisions
    std::vector<WholeRef> ref(C);
    for (int c = 0; c < C; ++c) whole_ref(E, G.cand[c][0], G.cand[c][1], fun, ref[c]);
    const double tol = tolmode == WT_NEVER ? 0.0 : tolmode == WT_ALWAYS ? 1e300 : mid_tol(G, fun).tol;
    ivec xiter(C);
    std::vector<char> xlucky(C);
    for (int c = 0; c < C; ++c) {
        const WholeRef& R = ref[c];
        int iter = it;
        bool lucky = false;
        for (int j = 1; j <= it; ++j) {
            lucky = R.rnorm[j - 1] < 1e-8L;
            if (!(R.rnorm[j - 1] <= 0.25e-8L || R.rnorm[j - 1] >= 4e-8L)) cs.fail("lucky margin", c, (double)R.rnorm[j - 1], 1e-8, 0.0, INFINITY);
            bool stop = false;
            if (j >= 3) {
                const ld_t d = fabsl(R.xm[j - 1] - R.xm[j - 3]);
                stop = d < tol;
                if (!(d <= (ld_t)tol / 4 || d >= 4 * (ld_t)tol)) cs.fail("stop margin", c, (double)d, tol, 0.0, INFINITY);
            }
            if (stop || lucky || j == it) {
                iter = j;
                break;
            }
            // this record enters the next projection: keep condition
            if (!(R.rmin[j - 1] >= 1e-3L * E.rhoA)) cs.fail("keep condition: min(R11, R22) < 1e-3 rho(A)", c * 100 + j, (double)R.rmin[j - 1], (double)(1e-3L * E.rhoA), 0.0, INFINITY);
        }
        xiter[c] = iter;
        xlucky[c] = lucky;
    }
    ivec ii(C), jj(C);
    for (int c = 0; c < C; ++c) {
        ii[c] = G.cand[c][0];
        jj[c] = G.cand[c][1];
    }
    setenv("KT_PAIRS_REG", form == WF_FUSED_BLK || form == WF_FUSED_DENSE ? "0" : "1", 1);
    setenv("KT_PAIRS_DENSE_EIG", form == WF_FUSED_DENSE ? "1" : "0", 1);
    const dvec state0((size_t)C * PS_N + GUARD, SENT);
    dvec out[2], out_fused;
    for (int run = 0; run < (g_host ? 1 : 2); ++run) {
        g_work.off = 0;
        const int* dii = up(ii);
        const int* djj = up(jj);
        const double* dB = nullptr;  // B is read on the host
        (void)dB;
        double* dst = up(state0);
        double* dvec_ = up(dvec((size_t)C * 3 * n * 2 + GUARD, NAN));
        if (form == WF_DYN) {
            // the edited CSR in buffers of the first matrix's capacity; the LDS is sized by (nnz_max, first n_long)
            ivec ci2 = E.ci;
            dvec va2 = E.va_dev;
            ci2.resize(G.nnz(), ISENT);
            va2.resize(G.nnz(), NAN);
            const WholeDev D = whole_upload(G, E.rp, ci2, va2, E.lr, E.nnz(), (int)G.lr.size());
            if (g_host) LAUNCH(host::pair_fused(C, n, D.view, G.unit, dii, djj, kWholeB, it, fun, tol, dst));
            else LAUNCH(kt::launch_pair_reg_dyn(C, n, G.nnz(), D.view, G.unit, dii, djj, kWholeB, it, fun, tol, dst, D.dyn, nullptr));
            if (run == 0) {  // the contract: launch_pair_fused on that CSR, by bits
                const WholeDev F = whole_upload(G, E.rp, E.ci, E.va_dev, E.lr, E.nnz(), (int)E.lr.size());
                double* dst2 = up(state0);
                if (g_host) LAUNCH(host::pair_fused(C, n, F.view, G.unit, dii, djj, kWholeB, it, fun, tol, dst2));
                else LAUNCH(kt::launch_pair_fused(C, n, E.nnz(), F.view, G.unit, dii, djj, kWholeB, it, fun, tol, dvec_, nullptr, 0, dst2, nullptr));
                out_fused = down(dst2, state0.size());
            }
        } else {
            const WholeDev D = whole_upload(G, rp, ci, vad, lr, G.nnz(), (int)lr.size());
            if (g_host) LAUNCH(host::pair_fused(C, n, D.view, G.unit, dii, djj, kWholeB, it, fun, tol, dst));
            else LAUNCH(kt::launch_pair_fused(C, n, G.nnz(), D.view, G.unit, dii, djj, kWholeB, it, fun, tol, dvec_, nullptr, 0, dst, nullptr));
        }
        out[run] = down(dst, state0.size());
    }
    if (!g_host) cs.unchanged("second run differs", out[0], out[1]);
    if (form == WF_DYN) cs.unchanged("launch_pair_reg_dyn vs launch_pair_fused on the edited CSR", out_fused, out[0]);
    cs.unchanged("guard", state0, out[0], (size_t)C * PS_N);
    for (int c = 0; c < C; ++c) {
        const double* st = &out[0][(size_t)c * PS_N];
        const long ix = (long)c * PS_N;
        const int j = xiter[c];
        cs.bounded("Xm", ix + PS_XM, st[PS_XM], ref[c].xm[j - 1], (ld_t)K_WHOLE * ref[c].bound[j - 1] + ref[c].gterm[j - 1]);
        if (g_host && g_mut.empty() && ref[c].bound[j - 1] > 0)
            g_r_whole = std::max(g_r_whole, (double)((fabsl((ld_t)st[PS_XM] - ref[c].xm[j - 1]) - ref[c].gterm[j - 1]) / ref[c].bound[j - 1]));
        cs.same("iter", ix + PS_ITER, st[PS_ITER], (double)j);
        cs.same("lucky", ix + PS_LUCKY, st[PS_LUCKY], xlucky[c] ? 1.0 : 0.0);
        cs.same("done", ix + PS_DONE, st[PS_DONE], 1.0);
        for (int t : {0, 1, 6, 7}) cs.same("untouched slot", ix + t, st[t], SENT);
    }
}

static void grp_whole() {
    if (g_wgraphs.empty()) wgraphs_init();
    for (const WGraph& G : g_wgraphs) {
        const int fun = whole_fun(G);
        for (int form : {WF_REG, WF_FUSED_BLK, WF_FUSED_DENSE})
            for (int tolmode : {WT_NEVER, WT_ALWAYS, WT_MID}) whole_case(G, form, tolmode, fun);
        if (G.applies) whole_case(G, WF_DYN, WT_NEVER, fun);
    }
    setenv("KT_PAIRS_REG", "1", 1);
    setenv("KT_PAIRS_DENSE_EIG", "0", 1);
    if (g_host && !g_list && g_mut.empty()) fprintf(stderr, "pairs_check: r_whole = %.3f (K_whole = %g)\n", g_r_whole, K_WHOLE);
}

// ---------------------------------------------------------------------------
static const char* kMutations[] = {"eig_no_symmetrise",      "eig_cm_on_both",     "eig_drop_last_eigenvalue",
                                   "eig_lucky_r22_only",     "eig_stop_lag1",      "eig_done_not_frozen",
                                   "active_counts_done",     "edit_tie_takes_last", "edit_nan_wins",
                                   "edit_rp_shift_from_r1",  "edit_keeps_shortened_long_row",
                                   "edit_ranking_last_entry_lost", "orth_drop_last_row",
                                   "orth_row0_in_s1",        "orth_row1_in_s2",     "orth_no_tau0_branch",
                                   "orth_partials_stop_at_64", "orth_store_invalid_lane", "orth_ignores_skip",
                                   "whole_long_rows_skipped", "whole_cm_without_r12"};

int main(int argc, char** argv) {
    g_t0 = std::chrono::steady_clock::now();
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--host")) {
            g_host = true;
        } else if (!strncmp(argv[a], "--mutate=", 9)) {
            g_mut = argv[a] + 9;
        } else if (!strcmp(argv[a], "--count")) {
            g_list = g_host = true;
        } else if (!strcmp(argv[a], "--small")) {
            g_small = true;
        } else if (!strncmp(argv[a], "--group=", 8)) {
            for (int g = 0; g < NG; ++g)
                if (!strcmp(argv[a] + 8, g_groups[g].name)) g_only = g;
            if (g_only < 0) {
                fprintf(stderr, "pairs_check: unknown group %s\n", argv[a] + 8);
                return 2;
            }
        } else {
            fprintf(stderr, "usage: pairs_check [--host [--mutate=NAME]] [--count] [--group=NAME] [--small]\n");
            return 2;
        }
    }
    if (!g_mut.empty()) {
        bool known = false;
        for (const char* m : kMutations) known = known || g_mut == m;
        if (!known || !g_host || g_list) {
            fprintf(stderr, "pairs_check: --mutate needs --host and one of:");
            for (const char* m : kMutations) fprintf(stderr, " %s", m);
            fprintf(stderr, "\n");
            return 2;
        }
    }
    if (!g_host) {
        hipDeviceProp_t prop;
        HC(hipGetDeviceProperties(&prop, 0));
    }
    if (!g_list) {
        g_work.init((size_t)64 << 20);
        edit_graph_init();
    }
    void (*const groups[NG])() = {grp_select, grp_orth, grp_eig, grp_edit, grp_whole};
    for (int g = 0; g < NG; ++g) {
        if (g_only >= 0 && g != g_only) continue;
        const auto t0 = std::chrono::steady_clock::now();
        groups[g]();
        g_groups[g].seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    print_report(nullptr);
    long nfail = 0;
    for (int g = 0; g < NG; ++g) nfail += g_groups[g].nfail;
    return nfail ? 1 : 0;
}
