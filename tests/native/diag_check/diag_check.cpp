// diag_check -- the streaming kernels of kt_diag.hip (kt_diag_fun and
// kt_entries_fun) and the two streaming launchers of kt_adapt.hip that no other
// program calls (launch_weighted_sum_tab, launch_unit_start), called one by one
// through their kt::launch_* entry points (kt_launch.h) in every (P, KP) form a
// launcher's switch can select, each result compared with a host reference in
// long double (or in exact integers).
//
// Groups: qtz_sum, start, combine, finish, entries, d0, adapt_stream, contract.
// Three kinds of assertion (as block_check / sweep_check):
//   exact    small-integer inputs (Q, c, W, V, Y, G, H and the prior sums:
//            |v| <= 4, Q without zeros; signs +-1): every product and sum is
//            exact in fp64 in any order, with or without fma (each comparison
//            verifies that the sum of absolute terms stays below 2^52), so the
//            output must equal the integer reference.
//   bounded  standard-normal inputs against long double with componentwise
//            a-priori bounds, u = 2^-53, gamma_k = k u / (1 - k u); a sum whose
//            every term passes through at most k roundings is within gamma_k
//            times the sum of the absolute terms, in any order (adding an
//            exact zero is no rounding):
//     qtz + sum_parts   c[b, p] = sum_r Q[r, b] z[r, p]: z = +-1, the products
//                       are exact, n - 1 additions: gamma_n sum_r |Q[r, b]|.
//     sum_parts alone   gamma_nparts sum_g |part[g]|.
//     start, X          KP fmas and one subtraction:
//                       gamma_(KP+1) (1 + sum_b |Q[r, b]| |c[b, p]|).
//     start, norms      against the long double sum of the device's own X^2:
//                       one square, n - 1 additions: gamma_(n+1) sum X^2.
//     combine, y        dep = depth[p] fmas: gamma_dep ay, ay = sum_j |W||V|;
//                       a column cut at 0 is an exact zero.
//     combine, Q'y      the y chain, one product, n - 1 additions:
//                       gamma_(n+mdepth) sum_r |Q[r, b]| ay[r, p].
//     dsum (combine)    t = z y is exact; the P-term row sum and the += onto
//                       the prior value: every term passes through at most
//                       mdepth + (P - 1) + 1 roundings, the prior through one:
//                       gamma_(mdepth+P+1) (|prior| + sum_p ay).
//     dsum2             through the computed t: |t^ - t| <= g A with g the
//                       chain's gamma and A >= |t| the absolute sum, so
//                       |t^^2 - t^2| <= (2 g + g^2) A^2; one rounding of the
//                       square, P - 1 additions, the +=:
//                       sum_p (2 g + g^2) A_p^2
//                         + gamma_(P+2) (|prior| + (1 + g)^2 sum_p A_p^2).
//     finish            yt = y - Q c: KP fmas and a subtraction, g =
//                       gamma_(KP+1), A = |y| + sum_b |Q||c|; dsum:
//                       gamma_(KP+P+1) (|prior| + sum_p A_p); dsum2 as above.
//     entries           t = (z_i yt_j + z_j yt_i) / 2: the yt chain, one
//                       addition and the halving (counted, though exact):
//                       g = gamma_(KP+3), A = (A_i + A_j) / 2; esum:
//                       gamma_(KP+P+3) (|prior| + sum_p A_p); esum2 as dsum2.
//     d0                a = sum_c q g: k fmas; h: k fmas, one more fma each
//                       into b2; 2 a - b2 one rounding:
//                       gamma_(k+1) 2 sum_c |q g|
//                         + gamma_(2k+1) sum_bc |q_b H_bc q_c|.
//     e0                a: two rounded products, their sum, k additions, the
//                       final subtraction: gamma_(k+3) sum_c (|qi gj| + |gi qj|);
//                       b2: the h chain (k), product, sum, k additions, the
//                       subtraction: gamma_(2k+3) sum_bc (|qi_b H_bc qj_c| +
//                       |qj_b H_bc qi_c|) / 2.
//     weighted_sum_tab  m fmas: gamma_m sum_j |U_j||W_j|.
//            Nothing is tuned to the kernels and no constant is measured; each
//            group reports max_ratio, the largest error / bound it saw.
//   contract bit-for-bit statements the source makes (group contract, device
//            only; with --host they are counted and trivially true):
//     a  launch_diag_sum_parts adds in the documented order: lane l partials
//        l, l + 64, ..., then the xor butterfly at offsets 1, 2, ..., 32
//     b  launch_diag_start with KP = 0 writes the stream of launch_rademacher
//        on its live columns (the comment of probe_keys)
//     c  launch_diag_combine_y's Y is the KP > 0 form's Y on the same input
//     d  esum, esum2 and e0 of (i, j) and of (j, i) agree
//     e  a diagonal pair's esum equals launch_diag_finish's dsum of that row
//        from the same prior: t = (z yt + z yt) / 2 = z yt exactly and both
//        kernels reduce it with row_sum<P>.  Only esum is held to this: the
//        square t t feeds the first addition of row_sum, and whether those
//        two fuse is the compiler's choice in each kernel.
//     f  launch_weighted_sum_tab equals launch_weighted_sum on the same slots
//        laid out contiguously (k_weighted_sum: the same slot-order fma chain)
//     g  widths outside the switches (P in {3, 32}, KP in {2, 8}; KP = 0 for
//        qtz and finish) return hipErrorInvalidValue and leave the outputs
//        untouched (these run with --host too, against the stand-in's tables)
// Every output is pre-filled with a sentinel (or, where the kernel adds, a
// prior value) and followed by a guard region: Y, X, part (exactly grid K
// values), the sums and e0 leave no sentinel inside the documented extent and
// no change outside it.  Inputs carry NaN where the contract says they are not
// read: rows >= n of V, Q, Y, basis slots >= mdepth, the slots in [depth[p],
// mdepth) of a column with a shorter cut (and W there), columns [k, ld) of Q
// and G in d0 / e0, a whole slot after each chunk's last one.  On the device
// every case runs twice from the same initial state and the two runs must
// agree bit for bit ("no atomics, fixed order" is a claim of kt_diag.hip).
//
// Shapes: the launch_diag_* launchers take the grid, so small n reaches every
// loop path.  With RPB = 256 / max(P / 2, 1) rows per workgroup and trip:
// (n, grid) = (RPB - 3, diag_grid) one partly filled workgroup, (RPB, 1),
// (RPB + 1, 2), (7 RPB + 5, 3) three trips, a ragged last trip, idle rows.
// Seed 0xF1E2D3C4B5A69788, probe base 5000000007 (> 2^32); perm a shuffled
// bijection that is checked not to be an involution.  The only cases above a
// few MiB are the three grid-cap ones: entries at P = 16 with 4096 * 32 + 33
// pairs, e0 with 2048 * 256 + 77 pairs, d0 with n = 2048 * 256 + 300, and
// weighted_sum_tab with n nc = 4096 * 256 + 16.
//
// Planted defects (--host --mutate=NAME), each reported in its group only:
// qtz_drop_tail_row, qtz_dead_col_live, sum_parts_skip_64, start_no_projection,
// start_norm_from_z, combine_ignore_depth, combine_pair_depth,
// combine_dsum_by_row, combine_overwrite, finish_sign_by_row,
// entries_swap_signs, entries_dead_lane_adds (the pairs of a tail workgroup
// past npairs are added to: the guard changes), e0_half_missing,
// d0_row_major_H, wsum_tab_chunk_off_by_one, unit_start_oob_writes.
// d0_row_major_H reads H row-major with the leading dimension of Q and G: a
// plain transpose cannot be seen through d0 or e0, because q' H q = q' H' q.
//
//   diag_check                     run on the GPU
//   diag_check --host              the same cases with every device call
//                                  replaced by a plain fp64 host loop written
//                                  from the launchers' contract (no GPU)
//   diag_check --host --mutate=M   one deliberate defect in that stand-in
//   diag_check --count             the case counts, the form table and the
//                                  grid functions' values alone
//   --group=NAME runs one group; --small keeps the widths 1, 4 and 16 only
//
// Prints one JSON line; exit status 0 iff no case failed, 1 on failures, 3 on
// a HIP error (nothing is launched after it), 2 on bad usage.
// Build: make -C tests/native/diag_check (links the library's own objects).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../../krylov_robustness_amd/csrc/kt_launch.h"

namespace kt {
// kt_diag.hip's grid rule of launch_entries_accumulate (a plain host function
// of kt_diag.o that kt_launch.h does not list)
int entries_grid(int64_t npairs, int P);
void set_error(const std::string&) {}  // kt_dense.o's ABI edge; unused here
}  // namespace kt

typedef long double ld_t;
typedef std::vector<double> dvec;
typedef std::vector<int> ivec;
typedef std::vector<ld_t> lvec;

static bool g_host = false;
static bool g_list = false;  // --count: enumerate the cases, run nothing
static bool g_small = false;
static int g_only = -1;
static std::string g_mut;
static bool mut(const char* s) { return g_mut == s; }
static std::vector<int> kWidths = {1, 2, 4, 8, 16};

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
enum { G_QTZ, G_START, G_COMBINE, G_FINISH, G_ENTRIES, G_D0, G_ADAPT, G_CONTRACT, NG };
static Group g_groups[NG] = {{"qtz_sum"}, {"start"}, {"combine"},      {"finish"},
                             {"entries"}, {"d0"},    {"adapt_stream"}, {"contract"}};
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

// launcher forms: the enumeration below runs off this table
struct Form {
    const char* launcher;
    int P, KP;
    std::string reaches;
};
static std::vector<Form> g_forms;
static void forms_init() {
    struct L {
        const char *launcher, *kernel;
        bool k0, kpos;
    };
    static const L ls[] = {{"diag_qtz", "k_diag_qtz", false, true},
                           {"diag_start", "k_diag_start", true, true},
                           {"diag_combine", "k_diag_combine", true, true},
                           {"diag_combine_y", "k_diag_combine", true, false},
                           {"diag_finish", "k_diag_finish", false, true},
                           {"entries_accumulate", "k_entries_accumulate", true, true}};
    for (const L& l : ls)
        for (int P : {1, 2, 4, 8, 16})
            for (int KP : {0, 1, 4, 16}) {
                if (KP == 0 ? !l.k0 : !l.kpos) continue;
                const bool yonly = !l.kpos;
                g_forms.push_back({l.launcher, P, KP, fmt("%s<%d, %d%s>", l.kernel, P, KP, yonly ? ", true" : "")});
            }
}
static std::vector<const Form*> forms_of(const char* launcher) {
    std::vector<const Form*> v;
    for (const Form& f : g_forms)
        if (!strcmp(f.launcher, launcher) && std::find(kWidths.begin(), kWidths.end(), f.P) != kWidths.end())
            v.push_back(&f);
    return v;
}

static void print_report(const char* hip_err) {
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - g_t0).count();
    long nfail = 0;
    for (int g = 0; g < NG; ++g) nfail += g_groups[g].nfail;
    printf("{\"diag_check\": \"%s\", \"mode\": \"%s\", \"mutate\": \"%s\", \"wall_s\": %.3f, ",
           hip_err ? "HIP_ERROR" : (nfail ? "FAIL" : "ok"), g_list ? "count" : (g_host ? "host" : "device"),
           g_mut.c_str(), wall);
    if (hip_err) printf("\"hip_error\": \"%s\", ", hip_err);
    if (g_list) {
        printf("\"forms\": {");
        const char* last = "";
        for (const Form& f : g_forms) {
            if (strcmp(last, f.launcher)) printf("%s\"%s\": [", *last ? "], " : "", f.launcher);
            else printf(", ");
            printf("{\"P\": %d, \"KP\": %d, \"reaches\": \"%s\"}", f.P, f.KP, f.reaches.c_str());
            last = f.launcher;
        }
        printf("]}, \"grids\": {\"diag_grid\": [");
        static const int dg[][2] = {{0, 1},   {0, 16},   {1, 1},       {256, 1},     {257, 1},      {256, 2},
                                    {257, 2}, {129, 4},  {65, 8},      {32, 16},     {33, 16},      {50000, 16},
                                    {262144, 1}, {262145, 1}, {32736, 16}, {32768, 16}, {32769, 16}, {2000000000, 16}};
        for (size_t i = 0; i < sizeof dg / sizeof dg[0]; ++i)
            printf("%s[%d, %d, %d]", i ? ", " : "", dg[i][0], dg[i][1], kt::diag_grid(dg[i][0], dg[i][1]));
        printf("], \"entries_grid\": [");
        static const long long eg[][2] = {{0, 1},       {0, 16},      {1, 16},      {32, 16},          {33, 16},
                                          {257, 2},     {129, 4},     {65, 8},      {131040, 16},      {131072, 16},      {131073, 16},
                                          {1048576, 1}, {1048577, 1}, {5000000000LL, 16}};
        for (size_t i = 0; i < sizeof eg / sizeof eg[0]; ++i)
            printf("%s[%lld, %lld, %d]", i ? ", " : "", eg[i][0], eg[i][1], kt::entries_grid(eg[i][0], (int)eg[i][1]));
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
    fprintf(stderr, "diag_check: test setup: %s\n", msg.c_str());
    exit(2);
}

static uint64_t bits_of(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}

static const double SENT = -7.7777e77;
static const size_t GUARD = 67;
static const ld_t U = ldexpl(1.0L, -53);
static ld_t gam(ld_t k) { return k * U / (1.0L - k * U); }
static const ld_t kExactMax = ldexpl(1.0L, 52);

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
    // equal as numbers (exact arithmetic; +0 and -0 agree, NaN never does)
    void exact(const char* what, long idx, double got, double exp) {
        if (!(got == exp)) fail(what, idx, got, exp, 0.0, fabs(got - exp));
    }
    void same(const char* what, long idx, double got, double exp) {
        if (bits_of(got) != bits_of(exp)) fail(what, idx, got, exp, 0.0, INFINITY);
    }
    void bounded(const char* what, long idx, ld_t got, ld_t ref, ld_t bound) {
        const ld_t e = fabsl(got - ref);
        if (!(e <= bound)) {
            fail(what, idx, (double)got, (double)ref, (double)bound, (double)(e / bound));
        } else if (bound > 0.0L) {
            g.max_ratio = std::max(g.max_ratio, (double)(e / bound));
        }
    }
    // exact (integer inputs; mag = the sum of the absolute terms, which must
    // stay in the range where fp64 is exact) or bounded (normal inputs)
    void value(bool ex, const char* what, long idx, ld_t got, ld_t ref, ld_t bound, ld_t mag) {
        if (ex) {
            if (!(mag < kExactMax)) setup_die(fmt("%s %s: exact case leaves the fp64 integer range", name.c_str(), shape.c_str()));
            exact(what, idx, (double)got, (double)ref);
        } else {
            bounded(what, idx, got, ref, bound);
        }
    }
    // elements [0, count) hold no sentinel, elements from `count` on are unchanged
    void written(const char* what, const dvec& before, const dvec& after, size_t count) {
        for (size_t t = 0; t < count; ++t)
            if (bits_of(after[t]) == bits_of(SENT)) fail(what, (long)t, after[t], 0.0, 0.0, INFINITY);
        for (size_t t = count; t < before.size(); ++t) same("guard", (long)t, after[t], before[t]);
    }
    void unchanged(const char* what, const dvec& before, const dvec& after) {
        for (size_t t = 0; t < before.size(); ++t) same(what, (long)t, after[t], before[t]);
    }
    void repeat(const std::vector<dvec>& a, const std::vector<dvec>& b) {
        for (size_t k = 0; k < a.size(); ++k)
            for (size_t t = 0; t < a[k].size(); ++t)
                if (bits_of(a[k][t]) != bits_of(b[k][t]))
                    fail("second run differs", (long)t, b[k][t], a[k][t], 0.0, INFINITY);
    }
};

template <class F>
static std::vector<dvec> run_twice(Case& c, F exec) {
    std::vector<dvec> o = exec();
    if (!g_host) c.repeat(o, exec());
    return o;
}

// ---------------------------------------------------------------------------
// memory: one arena (device memory, or host memory with --host) used as a
// per-case stack
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

// ---------------------------------------------------------------------------
// data: blocks are slices of three pools made once (integers in [-4, 4],
// standard normals, integers +-1 .. +-4 without zero)
// ---------------------------------------------------------------------------
static uint64_t g_rng = 88172645463325252ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static double rnormal() {
    const double u1 = ((rnd() >> 11) + 1.0) * (1.0 / 9007199254740993.0);
    const double u2 = (rnd() >> 11) * (1.0 / 9007199254740992.0);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
enum Kind { INT4 = 0, NORMAL = 1 };
static const char* kind_name(int kind) { return kind == INT4 ? "exact" : "bounded"; }
static const size_t kPool = (size_t)1 << 20;
static dvec g_pool[3];
static size_t g_pos = 0;
static void pools_init() {
    for (dvec& p : g_pool) p.resize(kPool);
    for (size_t i = 0; i < kPool; ++i) {
        g_pool[0][i] = (double)((int)(rnd() % 9) - 4);
        g_pool[1][i] = rnormal();
        const int v = 1 + (int)(rnd() % 4);
        g_pool[2][i] = (rnd() & 1) ? (double)v : (double)-v;
    }
}
static dvec block(size_t count, int kind, bool nonzero = false) {
    const dvec& p = g_pool[kind == NORMAL ? 1 : (nonzero ? 2 : 0)];
    dvec v(count);
    for (size_t i = 0; i < count; ++i) v[i] = p[(g_pos + i) & (kPool - 1)];
    g_pos += count + 17;
    return v;
}
static dvec sentinels(size_t count) { return dvec(count + GUARD, SENT); }
// `count` values, then `pad` NaNs (input rows that must not be read)
static dvec nan_padded(dvec v, size_t pad) {
    v.resize(v.size() + pad, NAN);
    return v;
}
// prior values of a sum the kernel adds to, then the guard
static dvec priors(size_t count, int kind) {
    dvec v = block(count, kind);
    v.resize(count + GUARD, SENT);
    return v;
}

// splitmix64 and the probe sign of k_rademacher's comment: -1 where the top bit
// of splitmix64(key(seed, probe) + i) is set, key = splitmix64(splitmix64(seed)
// + probe), i the original row index
static uint64_t sm64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static const uint64_t kSeed = 0xF1E2D3C4B5A69788ull;
static const int64_t kBase = 5000000007LL;
static uint64_t probe_key(int p) { return sm64(sm64(kSeed) + (uint64_t)(kBase + p)); }
static double key_sign(uint64_t key, uint64_t i) { return (sm64(key + i) >> 63) ? -1.0 : 1.0; }
static double probe_sign(int p, uint64_t i) { return key_sign(probe_key(p), i); }

// a shuffled bijection of 0 .. n-1 that is not an involution (n >= 3)
static ivec make_perm(int n) {
    ivec p(n);
    for (int r = 0; r < n; ++r) p[r] = r;
    for (int i = n; i > 1; --i) std::swap(p[i - 1], p[rnd() % i]);
    bool invol = true;
    for (int r = 0; r < n; ++r) invol = invol && p[p[r]] == r;
    if (invol && n >= 3) std::rotate(p.begin(), p.begin() + 1, p.end());
    invol = true;
    for (int r = 0; r < n; ++r) invol = invol && p[p[r]] == r;
    if (invol && n >= 3) setup_die("perm is an involution");
    return p;
}

static int rpb_of(int P) { return 256 / std::max(P / 2, 1); }
struct Shape {
    int n, grid;
};
static std::vector<Shape> shapes_for(int P) {
    const int R = rpb_of(P);
    return {{R - 3, kt::diag_grid(R - 3, P)}, {R, kt::diag_grid(R, P)}, {R + 1, kt::diag_grid(R + 1, P)}, {7 * R + 5, 3}};
}
static std::vector<int> nc_list(int P) {
    std::vector<int> v{1};
    if (P - 1 > 1) v.push_back(P - 1);
    if (P > 1) v.push_back(P);
    return v;
}

// One sweep's rows: signs, deflation block, row order
static const int kPadRows = 3;
struct Sweep {
    int n, P, KP, nc;
    ivec perm;  // empty: natural order
    dvec Q;     // (n + kPadRows) x KP, the padding rows NaN
    uint64_t key[16];
    int orig(int r) const { return perm.empty() ? r : perm[r]; }
    double z(int r, int p) const { return p < nc ? key_sign(key[p], (uint64_t)orig(r)) : 0.0; }
    double q(int r, int b) const { return Q[(size_t)r * KP + b]; }
};
static Sweep make_sweep(int P, int KP, int n, int nc, bool perm, int kind) {
    Sweep S;
    S.n = n;
    S.P = P;
    S.KP = KP;
    S.nc = nc;
    if (perm) S.perm = make_perm(n);
    S.Q = nan_padded(block((size_t)n * std::max(KP, 1), kind, true), (size_t)kPadRows * std::max(KP, 1));
    for (int p = 0; p < 16; ++p) S.key[p] = probe_key(p);
    return S;
}
// c = Q'z in long double (KP x P), and sum_r |Q[r, b]| on the live columns
static void ref_qtz(const Sweep& S, lvec& c, lvec& a) {
    c.assign((size_t)std::max(S.KP, 1) * S.P, 0.0L);
    a.assign(c.size(), 0.0L);
    for (int r = 0; r < S.n; ++r)
        for (int b = 0; b < S.KP; ++b)
            for (int p = 0; p < S.nc; ++p) {
                c[b * S.P + p] += (ld_t)S.q(r, b) * (ld_t)S.z(r, p);
                a[b * S.P + p] += fabsl((ld_t)S.q(r, b));
            }
}

// ---------------------------------------------------------------------------
// the operations: the launcher, or its fp64 host stand-in written from
// kt_launch.h's contract (workgroup g owns the rows [g RPB, (g + 1) RPB) of
// every trip of grid RPB rows; its partial holds their sum)
// ---------------------------------------------------------------------------
static bool width_ok(int P) { return P == 1 || P == 2 || P == 4 || P == 8 || P == 16; }
static bool defl_ok(int KP) { return KP == 1 || KP == 4 || KP == 16; }

template <class F>
static void wg_rows(int g, int grid, int P, int n, F f) {
    const int R = rpb_of(P);
    for (int64_t rb = (int64_t)g * R; rb < n; rb += (int64_t)grid * R)
        for (int64_t r = rb; r < std::min<int64_t>(rb + R, n); ++r) f((int)r);
}

static hipError_t op_qtz(int P, int KP, int grid, int n, int nc, const int* perm, const double* Q, double* part) {
    if (!g_host) return kt::launch_diag_qtz(P, KP, grid, n, kSeed, kBase, nc, perm, Q, part, 0);
    if (!width_ok(P) || !defl_ok(KP)) return hipErrorInvalidValue;
    const bool drop = mut("qtz_drop_tail_row"), dead = mut("qtz_dead_col_live");
    for (int g = 0; g < grid; ++g) {
        dvec acc((size_t)KP * P, 0.0);
        wg_rows(g, grid, P, n, [&](int r) {
            if (drop && r == n - 1 && n % rpb_of(P)) return;
            const uint64_t i = perm ? perm[r] : r;
            for (int p = 0; p < P; ++p) {
                const double z = (p < nc || dead) ? probe_sign(p, i) : 0.0;
                for (int b = 0; b < KP; ++b) acc[b * P + p] += Q[(size_t)r * KP + b] * z;
            }
        });
        std::copy(acc.begin(), acc.end(), part + (size_t)g * KP * P);
    }
    return hipSuccess;
}

static hipError_t op_sum_parts(int nparts, int K, const double* part, double* out) {
    if (!g_host) return kt::launch_diag_sum_parts(nparts, K, part, out, 0);
    for (int i = 0; i < K; ++i) {
        double s = 0.0;
        for (int g = 0; g < nparts; ++g)
            if (!(mut("sum_parts_skip_64") && g == 64)) s += part[(size_t)g * K + i];
        out[i] = s;
    }
    return hipSuccess;
}

static hipError_t op_start(int P, int KP, int grid, int n, int nc, const int* perm, const double* Q, const double* c,
                           double* X, double* part) {
    if (!g_host) return kt::launch_diag_start(P, KP, grid, n, kSeed, kBase, nc, perm, Q, c, X, part, 0);
    if (!width_ok(P) || !(KP == 0 || defl_ok(KP))) return hipErrorInvalidValue;
    const bool noproj = mut("start_no_projection"), zn = mut("start_norm_from_z");
    for (int g = 0; g < grid; ++g) {
        dvec acc(P, 0.0);
        wg_rows(g, grid, P, n, [&](int r) {
            const uint64_t i = perm ? perm[r] : r;
            for (int p = 0; p < P; ++p) {
                const double z = p < nc ? probe_sign(p, i) : 0.0;
                double s = 0.0;
                for (int b = 0; b < KP; ++b) s += Q[(size_t)r * KP + b] * c[b * P + p];
                const double x = noproj ? z : z - s;
                X[(size_t)r * P + p] = x;
                acc[p] += zn ? z * z : x * x;
            }
        });
        std::copy(acc.begin(), acc.end(), part + (size_t)g * P);
    }
    return hipSuccess;
}

// KP = -1: launch_diag_combine_y
static hipError_t op_combine(int P, int KP, int grid, int n, int m, int mdepth, const double* V, int64_t sstride,
                             const double* W, const int* depth, const int* perm, const double* Q, double* Y,
                             double* part, double* dsum, double* dsum2) {
    if (!g_host) {
        if (KP < 0) return kt::launch_diag_combine_y(P, grid, n, m, mdepth, V, sstride, W, depth, Y, 0);
        return kt::launch_diag_combine(P, KP, grid, n, m, mdepth, V, sstride, W, depth, kSeed, kBase, perm, Q, Y, part,
                                       dsum, dsum2, 0);
    }
    if (!width_ok(P) || !(KP <= 0 || defl_ok(KP))) return hipErrorInvalidValue;
    const bool igd = mut("combine_ignore_depth"), pair = mut("combine_pair_depth");
    const bool byrow = mut("combine_dsum_by_row"), over = mut("combine_overwrite");
    for (int g = 0; g < grid; ++g) {
        dvec acc((size_t)std::max(KP, 1) * P, 0.0);
        wg_rows(g, grid, P, n, [&](int r) {
            const uint64_t i = perm ? perm[r] : r;
            double s1 = 0.0, s2 = 0.0;
            for (int p = 0; p < P; ++p) {
                int d = depth[p];
                if (igd) d = mdepth;
                if (pair && (p & 1)) d = depth[p - 1];
                double y = 0.0;
                for (int j = 0; j < d; ++j) y += W[j * P + p] * V[(int64_t)j * sstride + (int64_t)r * P + p];
                if (KP != 0) Y[(size_t)r * P + p] = y;
                for (int b = 0; b < KP; ++b) acc[b * P + p] += Q[(size_t)r * KP + b] * y;
                const double t = probe_sign(p, i) * y;
                s1 += t;
                s2 += t * t;
            }
            if (KP == 0) {
                const size_t at = byrow ? (size_t)r : (size_t)i;
                dsum[at] = over ? s1 : dsum[at] + s1;
                dsum2[at] = over ? s2 : dsum2[at] + s2;
            }
        });
        if (KP > 0) std::copy(acc.begin(), acc.end(), part + (size_t)g * KP * P);
    }
    return hipSuccess;
}

static hipError_t op_finish(int P, int KP, int grid, int n, const int* perm, const double* Q, const double* c,
                            const double* Y, double* dsum, double* dsum2) {
    if (!g_host) return kt::launch_diag_finish(P, KP, grid, n, kSeed, kBase, perm, Q, c, Y, dsum, dsum2, 0);
    if (!width_ok(P) || !defl_ok(KP)) return hipErrorInvalidValue;
    const bool byrow = mut("finish_sign_by_row");
    for (int g = 0; g < grid; ++g)
        wg_rows(g, grid, P, n, [&](int r) {
            const uint64_t i = perm ? perm[r] : r;
            double s1 = 0.0, s2 = 0.0;
            for (int p = 0; p < P; ++p) {
                double s = 0.0;
                for (int b = 0; b < KP; ++b) s += Q[(size_t)r * KP + b] * c[b * P + p];
                const double t = probe_sign(p, byrow ? (uint64_t)r : i) * (Y[(size_t)r * P + p] - s);
                s1 += t;
                s2 += t * t;
            }
            dsum[i] += s1;
            dsum2[i] += s2;
        });
    return hipSuccess;
}

static hipError_t op_entries(int P, int KP, int64_t npairs, const int* tab, const double* Q, const double* c,
                             const double* Y, double* esum, double* esum2) {
    if (!g_host) return kt::launch_entries_accumulate(P, KP, npairs, tab, kSeed, kBase, Q, c, Y, esum, esum2, 0);
    if (!width_ok(P) || !(KP == 0 || defl_ok(KP))) return hipErrorInvalidValue;
    const bool swap = mut("entries_swap_signs");
    uint64_t key[16];
    for (int p = 0; p < P; ++p) key[p] = probe_key(p);
    for (int64_t e = 0; e < npairs; ++e) {
        const int* pe = tab + 4 * e;
        double s1 = 0.0, s2 = 0.0;
        for (int p = 0; p < P; ++p) {
            double si = 0.0, sj = 0.0;
            for (int b = 0; b < KP; ++b) {
                si += Q[(size_t)pe[0] * KP + b] * c[b * P + p];
                sj += Q[(size_t)pe[1] * KP + b] * c[b * P + p];
            }
            const double yti = Y[(size_t)pe[0] * P + p] - si, ytj = Y[(size_t)pe[1] * P + p] - sj;
            const double zi = key_sign(key[p], (uint64_t)pe[2]), zj = key_sign(key[p], (uint64_t)pe[3]);
            const double t = swap ? 0.5 * (zi * yti + zj * ytj) : 0.5 * (zi * ytj + zj * yti);
            s1 += t;
            s2 += t * t;
        }
        esum[e] += s1;
        esum2[e] += s2;
    }
    if (mut("entries_dead_lane_adds")) {
        const int64_t ppb = rpb_of(P), end = std::min<int64_t>((npairs + ppb - 1) / ppb * ppb, npairs + (int64_t)GUARD);
        for (int64_t e = npairs; e < end; ++e) {
            esum[e] += 3.0e77;  // large enough to show on the guard's sentinel
            esum2[e] += 9.0e77;
        }
    }
    return hipSuccess;
}

static hipError_t op_e0(int64_t npairs, const int* tab, int k, const double* Q, const double* G, int ld,
                        const double* H, double* e0) {
    if (!g_host) return kt::launch_entries_e0(npairs, tab, k, Q, G, ld, H, e0, 0);
    const double half = mut("e0_half_missing") ? 1.0 : 0.5;
    for (int64_t e = 0; e < npairs; ++e) {
        const double* qi = Q + (size_t)tab[4 * e + 2] * ld;
        const double* qj = Q + (size_t)tab[4 * e + 3] * ld;
        const double* gi = G + (size_t)tab[4 * e + 2] * ld;
        const double* gj = G + (size_t)tab[4 * e + 3] * ld;
        double a = 0.0, b2 = 0.0;
        for (int c = 0; c < k; ++c) {
            a += qi[c] * gj[c] + gi[c] * qj[c];
            double hi = 0.0, hj = 0.0;
            for (int b = 0; b < k; ++b) {
                hi += qi[b] * H[b + c * k];
                hj += qj[b] * H[b + c * k];
            }
            b2 += hi * qj[c] + hj * qi[c];
        }
        e0[e] = a - half * b2;
    }
    return hipSuccess;
}

static hipError_t op_d0(int n, int k, const double* Q, const double* G, int ld, const double* H, double* d0) {
    if (!g_host) return kt::launch_diag_d0(n, k, Q, G, ld, H, d0, 0);
    const bool rowmajor = mut("d0_row_major_H");
    for (int r = 0; r < n; ++r) {
        const double* q = Q + (size_t)r * ld;
        const double* g = G + (size_t)r * ld;
        double a = 0.0, b2 = 0.0;
        for (int c = 0; c < k; ++c) {
            a += q[c] * g[c];
            double h = 0.0;
            for (int b = 0; b < k; ++b) h += q[b] * H[rowmajor ? b * ld + c : b + c * k];
            b2 += h * q[c];
        }
        d0[r] = 2.0 * a - b2;
    }
    return hipSuccess;
}

static hipError_t op_wsum_tab(int n, int m, int nc, const kt::SlotTab& tab, int spc, const double* W, double* Y,
                              int ldy) {
    if (!g_host) return kt::launch_weighted_sum_tab(n, m, nc, tab, spc, W, Y, ldy, 0);
    if (spc < 1 || m < 1 || (m + spc - 1) / spc > kt::kSlotTabChunks) return hipErrorInvalidValue;
    const bool off1 = mut("wsum_tab_chunk_off_by_one");
    const int64_t sstride = (int64_t)n * nc;
    for (int64_t t = 0; t < sstride; ++t) {
        const int c = (int)(t % nc);
        double s = 0.0;
        for (int j = 0; j < m; ++j) {
            const bool wrong = off1 && j == spc;  // the first slot of chunk 1 read past chunk 0's end
            const double* u = tab.chunk[wrong ? 0 : j / spc] + (int64_t)(wrong ? spc : j % spc) * sstride + t;
            s += *u * W[j * nc + c];
        }
        Y[(t / nc) * ldy + c] = s;
    }
    return hipSuccess;
}

static hipError_t op_unit_start(int n, int P, int nc, const int* pos, double* X, double* sc, double* k2s) {
    if (!g_host) return kt::launch_unit_start(n, P, nc, pos, X, sc, k2s, 0);
    if (n < 1 || P < 1 || P > 64 || nc < 0 || nc > P) return hipErrorInvalidValue;
    const bool oob = mut("unit_start_oob_writes");
    for (int c = 0; c < P; ++c) {
        const int r = c < nc ? pos[c] : -1;
        const bool ok = r >= 0 && (oob ? r <= n : r < n);
        if (ok) X[(size_t)r * P + c] = 1.0;
        sc[c] = ok ? 1.0 : 0.0;
        k2s[c] = ok ? 1.0 : 0.0;
    }
    return hipSuccess;
}

// sum of P squares of computed terms t^ with |t^ - t| <= ge A and |t| <= A,
// added to a prior value (the header's dsum2 bound)
static ld_t sq_bound(ld_t ge, const lvec& A, ld_t prior, int P) {
    ld_t s1 = 0.0L, s2 = 0.0L;
    for (ld_t a : A) {
        s1 += (2.0L * ge + ge * ge) * a * a;
        s2 += (1.0L + ge) * (1.0L + ge) * a * a;
    }
    return s1 + gam(P + 2) * (fabsl(prior) + s2);
}

// ---------------------------------------------------------------------------
// 1. qtz_sum
// ---------------------------------------------------------------------------
static void qtz_case(int P, int KP, Shape sh, int nc, bool perm, int kind) {
    Case c(G_QTZ, kind_name(kind), fmt("P=%d KP=%d n=%d grid=%d nc=%d perm=%d", P, KP, sh.n, sh.grid, nc, (int)perm));
    if (g_list) return;
    const Sweep S = make_sweep(P, KP, sh.n, nc, perm, kind);
    const size_t K = (size_t)KP * P;
    const std::vector<dvec> o = run_twice(c, [&]() {
        g_work.off = 0;
        const double* dQ = up(S.Q);
        const int* dperm = perm ? up(S.perm) : nullptr;
        double* dpart = up(sentinels(sh.grid * K));
        double* dout = up(sentinels(K));
        LAUNCH(op_qtz(P, KP, sh.grid, sh.n, nc, dperm, dQ, dpart));
        LAUNCH(op_sum_parts(sh.grid, (int)K, dpart, dout));
        return std::vector<dvec>{down(dpart, sh.grid * K + GUARD), down(dout, K + GUARD)};
    });
    c.written("part", sentinels(sh.grid * K), o[0], sh.grid * K);
    c.written("c", sentinels(K), o[1], K);
    lvec ref, a;
    ref_qtz(S, ref, a);
    for (int b = 0; b < KP; ++b)
        for (int p = 0; p < P; ++p) {
            const size_t t = (size_t)b * P + p;
            if (p >= nc) {
                c.exact("dead column", (long)t, o[1][t], 0.0);
                for (int g = 0; g < sh.grid; ++g) c.exact("dead column partial", (long)(g * K + t), o[0][g * K + t], 0.0);
            } else {
                c.value(kind == INT4, "c", (long)t, o[1][t], ref[t], gam(sh.n) * a[t], a[t]);
            }
        }
}

static void sum_parts_case(int nparts, int K, int kind) {
    Case c(G_QTZ, fmt("sum_parts_%s", kind_name(kind)), fmt("nparts=%d K=%d", nparts, K));
    if (g_list) return;
    const dvec part = nan_padded(block((size_t)nparts * K, kind), 8);
    const std::vector<dvec> o = run_twice(c, [&]() {
        g_work.off = 0;
        const double* dpart = up(part);
        double* dout = up(sentinels(K));
        LAUNCH(op_sum_parts(nparts, K, dpart, dout));
        return std::vector<dvec>{down(dout, K + GUARD)};
    });
    c.written("out", sentinels(K), o[0], K);
    for (int i = 0; i < K; ++i) {
        ld_t s = 0.0L, a = 0.0L;
        for (int g = 0; g < nparts; ++g) {
            s += (ld_t)part[(size_t)g * K + i];
            a += fabsl((ld_t)part[(size_t)g * K + i]);
        }
        c.value(kind == INT4, "out", i, o[0][i], s, gam(nparts) * a, a);
    }
}

static void grp_qtz() {
    for (const Form* f : forms_of("diag_qtz"))
        for (const Shape& sh : shapes_for(f->P))
            for (int nc : nc_list(f->P))
                for (int perm = 0; perm < 2; ++perm)
                    for (int kind : {INT4, NORMAL}) qtz_case(f->P, f->KP, sh, nc, perm, kind);
    for (int nparts : {1, 63, 64, 65, 1024})
        for (int K : {1, 2, 3, 4, 5, 256})
            for (int kind : {INT4, NORMAL}) sum_parts_case(nparts, K, kind);
}

// ---------------------------------------------------------------------------
// 2. start
// ---------------------------------------------------------------------------
// c as the driver passes it: the double of Q'z, dead columns zero
static dvec c_of(const Sweep& S) {
    lvec ref, a;
    ref_qtz(S, ref, a);
    dvec c(ref.size());
    for (size_t t = 0; t < c.size(); ++t) c[t] = (double)ref[t];
    return c;
}

static void start_case(int P, int KP, Shape sh, int nc, bool perm, int kind) {
    Case c(G_START, kind_name(kind), fmt("P=%d KP=%d n=%d grid=%d nc=%d perm=%d", P, KP, sh.n, sh.grid, nc, (int)perm));
    if (g_list) return;
    const Sweep S = make_sweep(P, KP, sh.n, nc, perm, kind);
    const int n = sh.n;
    const dvec cc = c_of(S);
    const std::vector<dvec> o = run_twice(c, [&]() {
        g_work.off = 0;
        const double* dQ = up(S.Q);
        const double* dc = up(nan_padded(cc, 4));
        const int* dperm = perm ? up(S.perm) : nullptr;
        double* dX = up(sentinels((size_t)n * P));
        double* dpart = up(sentinels((size_t)sh.grid * P));
        double* dout = up(sentinels(P));
        LAUNCH(op_start(P, KP, sh.grid, n, nc, dperm, KP ? dQ : nullptr, KP ? dc : nullptr, dX, dpart));
        LAUNCH(op_sum_parts(sh.grid, P, dpart, dout));
        return std::vector<dvec>{down(dX, (size_t)n * P + GUARD), down(dpart, (size_t)sh.grid * P + GUARD),
                                 down(dout, P + GUARD)};
    });
    c.written("X", sentinels((size_t)n * P), o[0], (size_t)n * P);
    c.written("part", sentinels((size_t)sh.grid * P), o[1], (size_t)sh.grid * P);
    c.written("norms", sentinels(P), o[2], P);
    for (int p = 0; p < P; ++p) {
        ld_t n2 = 0.0L;
        for (int r = 0; r < n; ++r) {
            const size_t t = (size_t)r * P + p;
            if (p >= nc) {
                c.exact("dead column", (long)t, o[0][t], 0.0);
                continue;
            }
            ld_t x = S.z(r, p), a = 1.0L;
            for (int b = 0; b < KP; ++b) {
                x -= (ld_t)S.q(r, b) * (ld_t)cc[b * P + p];
                a += fabsl((ld_t)S.q(r, b) * (ld_t)cc[b * P + p]);
            }
            c.value(kind == INT4, "X", (long)t, o[0][t], x, gam(KP + 1) * a, a);
            n2 += (ld_t)o[0][t] * (ld_t)o[0][t];
        }
        if (p >= nc) c.exact("dead column norm", p, o[2][p], 0.0);
        else c.value(kind == INT4, "norm", p, o[2][p], n2, gam(n + 1) * n2, n2);
    }
}

static void grp_start() {
    for (const Form* f : forms_of("diag_start"))
        for (const Shape& sh : shapes_for(f->P))
            for (int nc : nc_list(f->P))
                for (int perm = 0; perm < 2; ++perm)
                    for (int kind : {INT4, NORMAL}) start_case(f->P, f->KP, sh, nc, perm, kind);
}

// ---------------------------------------------------------------------------
// 3. combine
// ---------------------------------------------------------------------------
static const char* kPatName[6] = {"equal", "each", "pair", "one0", "all0", "below_m"};
static ivec depths_of(int P, int m, int pat) {
    ivec d(P);
    for (int p = 0; p < P; ++p) switch (pat) {
            case 0: d[p] = m; break;
            case 1: d[p] = m - p % (m + 1); break;
            case 2: d[p] = (p & 1) ? m - 1 : m; break;
            case 3: d[p] = p == P / 2 ? 0 : m; break;
            case 4: d[p] = 0; break;
            default: d[p] = std::max(m - 1 - (p & 1), 0); break;
        }
    return d;
}

// The basis, the weights and the reference y of one combine case
struct Basis {
    int n, P, m, mdepth;
    int64_t sstride;
    ivec depth;  // P entries, then garbage that must not be read
    dvec V, W;
    lvec y, ay;  // n x P
};
static Basis make_basis(int P, int n, int m, int pat, int kind) {
    Basis B;
    B.n = n;
    B.P = P;
    B.m = m;
    B.depth = depths_of(P, m, pat);
    B.mdepth = *std::max_element(B.depth.begin(), B.depth.end());
    B.sstride = (int64_t)n * P + 6;  // a gap of NaN between the slots (even: 16-byte pairs stay aligned)
    B.V.assign((size_t)(m * B.sstride), NAN);
    B.W.assign((size_t)m * P + 4, NAN);
    const dvec v = block((size_t)m * n * P, kind), w = block((size_t)m * P, kind, true);
    B.y.assign((size_t)n * P, 0.0L);
    B.ay.assign((size_t)n * P, 0.0L);
    for (int j = 0; j < m; ++j)
        for (int p = 0; p < P; ++p) {
            if (j >= B.depth[p]) continue;
            B.W[(size_t)j * P + p] = w[(size_t)j * P + p];
            for (int r = 0; r < n; ++r) {
                const double x = v[((size_t)j * n + r) * P + p];
                B.V[(size_t)(j * B.sstride) + (size_t)r * P + p] = x;
                B.y[(size_t)r * P + p] += (ld_t)w[(size_t)j * P + p] * (ld_t)x;
                B.ay[(size_t)r * P + p] += fabsl((ld_t)w[(size_t)j * P + p] * (ld_t)x);
            }
        }
    B.depth.resize(P + 4, 1 << 20);
    return B;
}

// KP = -1: launch_diag_combine_y
static void combine_case(int P, int KP, Shape sh, int m, int pat, bool perm, int kind) {
    Case c(G_COMBINE, kind_name(kind),
           fmt("%s P=%d KP=%d n=%d grid=%d m=%d depth=%s perm=%d", KP < 0 ? "combine_y" : "combine", P, std::max(KP, 0),
               sh.n, sh.grid, m, kPatName[pat], (int)perm));
    if (g_list) return;
    const int n = sh.n, KQ = std::max(KP, 0);
    const Sweep S = make_sweep(P, KQ, n, P, perm, kind);
    const Basis B = make_basis(P, n, m, pat, kind);
    const size_t K = (size_t)KQ * P;
    const dvec d1 = priors(n, kind), d2 = priors(n, kind);
    const bool ex = kind == INT4;
    const std::vector<dvec> o = run_twice(c, [&]() {
        g_work.off = 0;
        const double* dV = up(B.V);
        const double* dW = up(B.W);
        const int* ddepth = up(B.depth);
        const double* dQ = up(S.Q);
        const int* dperm = perm ? up(S.perm) : nullptr;
        double* dY = up(sentinels((size_t)n * P));
        double* dpart = up(sentinels(sh.grid * K));
        double* dout = up(sentinels(K));
        double* ds1 = up(d1);
        double* ds2 = up(d2);
        LAUNCH(op_combine(P, KP, sh.grid, n, m, B.mdepth, dV, B.sstride, dW, ddepth, dperm, KP > 0 ? dQ : nullptr, dY,
                          dpart, ds1, ds2));
        if (KP > 0) LAUNCH(op_sum_parts(sh.grid, (int)K, dpart, dout));
        return std::vector<dvec>{down(dY, (size_t)n * P + GUARD), down(dpart, sh.grid * K + GUARD), down(dout, K + GUARD),
                                 down(ds1, n + GUARD), down(ds2, n + GUARD)};
    });
    if (KP == 0) {
        c.unchanged("Y untouched", sentinels((size_t)n * P), o[0]);
        for (size_t t = n; t < d1.size(); ++t) {
            c.same("guard", (long)t, o[3][t], d1[t]);
            c.same("guard", (long)t, o[4][t], d2[t]);
        }
        for (int r = 0; r < n; ++r) {
            const int i = S.orig(r);
            ld_t s1 = d1[i], s2 = d2[i], a1 = fabsl((ld_t)d1[i]), a2 = fabsl((ld_t)d2[i]);
            lvec A(P);
            for (int p = 0; p < P; ++p) {
                const ld_t t = (ld_t)S.z(r, p) * B.y[(size_t)r * P + p];
                A[p] = B.ay[(size_t)r * P + p];
                s1 += t;
                s2 += t * t;
                a1 += A[p];
                a2 += A[p] * A[p];
            }
            if (B.mdepth == 0) {  // exact zeros were added
                c.same("dsum kept", i, o[3][i], d1[i]);
                c.same("dsum2 kept", i, o[4][i], d2[i]);
                continue;
            }
            c.value(ex, "dsum", i, o[3][i], s1, gam(B.mdepth + P + 1) * a1, a1);
            c.value(ex, "dsum2", i, o[4][i], s2, sq_bound(gam(B.mdepth), A, d2[i], P), a2);
        }
        return;
    }
    c.unchanged("dsum untouched", d1, o[3]);
    c.unchanged("dsum2 untouched", d2, o[4]);
    c.written("Y", sentinels((size_t)n * P), o[0], (size_t)n * P);
    for (int r = 0; r < n; ++r)
        for (int p = 0; p < P; ++p) {
            const size_t t = (size_t)r * P + p;
            c.value(ex, "Y", (long)t, o[0][t], B.y[t], gam(B.depth[p]) * B.ay[t], B.ay[t]);
        }
    if (KP < 0) {
        c.unchanged("part untouched", sentinels(0), o[1]);
        return;
    }
    c.written("part", sentinels(sh.grid * K), o[1], sh.grid * K);
    c.written("Q'y", sentinels(K), o[2], K);
    for (int b = 0; b < KP; ++b)
        for (int p = 0; p < P; ++p) {
            ld_t s = 0.0L, a = 0.0L;
            for (int r = 0; r < n; ++r) {
                s += (ld_t)S.q(r, b) * B.y[(size_t)r * P + p];
                a += fabsl((ld_t)S.q(r, b)) * B.ay[(size_t)r * P + p];
            }
            c.value(ex, "Q'y", b * P + p, o[2][b * P + p], s, gam(n + B.mdepth) * a, a);
        }
}

static void grp_combine() {
    for (const char* launcher : {"diag_combine", "diag_combine_y"})
        for (const Form* f : forms_of(launcher)) {
            const int KP = !strcmp(launcher, "diag_combine_y") ? -1 : f->KP;
            const std::vector<Shape> sh = shapes_for(f->P);
            for (int kind : {INT4, NORMAL}) {
                for (const Shape& s : sh)
                    for (int perm = 0; perm < (KP == 0 ? 2 : 1); ++perm) combine_case(f->P, KP, s, 9, 1, perm, kind);
                for (int m : {1, 7, 8, 9, 17})
                    for (int pat = 0; pat < 6; ++pat) combine_case(f->P, KP, sh[2], m, pat, true, kind);
            }
        }
    // the driver's maximum depth: 40 KiB of LDS at (16, 16)
    if (std::find(kWidths.begin(), kWidths.end(), 16) != kWidths.end())
        for (int kind : {INT4, NORMAL})
            for (int pat : {0, 1}) combine_case(16, 16, shapes_for(16)[2], 256, pat, true, kind);
}

// ---------------------------------------------------------------------------
// 4. finish
// ---------------------------------------------------------------------------
// Y and c of a finish / entries case: dead columns (>= nc) carry zeros
struct Tail {
    dvec Y, c;  // Y (n + kPadRows) x P with NaN padding rows; c KP x P
};
static Tail make_tail(int P, int KP, int n, int nc, int kind) {
    Tail T;
    T.Y = nan_padded(block((size_t)n * P, kind), (size_t)kPadRows * P);
    T.c = nan_padded(block((size_t)std::max(KP, 1) * P, kind), 4);
    for (int p = nc; p < P; ++p) {
        for (int r = 0; r < n; ++r) T.Y[(size_t)r * P + p] = 0.0;
        for (int b = 0; b < std::max(KP, 1); ++b) T.c[(size_t)b * P + p] = 0.0;
    }
    return T;
}
// yt[r, p] = Y - Q c in long double, and A = |Y| + sum |Q||c|
static void ref_yt(const Sweep& S, const Tail& T, int r, lvec& yt, lvec& A) {
    yt.assign(S.P, 0.0L);
    A.assign(S.P, 0.0L);
    for (int p = 0; p < S.P; ++p) {
        yt[p] = T.Y[(size_t)r * S.P + p];
        A[p] = fabsl(yt[p]);
        for (int b = 0; b < S.KP; ++b) {
            yt[p] -= (ld_t)S.q(r, b) * (ld_t)T.c[(size_t)b * S.P + p];
            A[p] += fabsl((ld_t)S.q(r, b) * (ld_t)T.c[(size_t)b * S.P + p]);
        }
    }
}

static void finish_case(int P, int KP, Shape sh, int nc, bool perm, int kind) {
    Case c(G_FINISH, kind_name(kind), fmt("P=%d KP=%d n=%d grid=%d nc=%d perm=%d", P, KP, sh.n, sh.grid, nc, (int)perm));
    if (g_list) return;
    const int n = sh.n;
    const Sweep S = make_sweep(P, KP, n, P, perm, kind);  // finish has no nc: every column has a sign
    const Tail T = make_tail(P, KP, n, nc, kind);
    const dvec d1 = priors(n, kind), d2 = priors(n, kind);
    const std::vector<dvec> o = run_twice(c, [&]() {
        g_work.off = 0;
        const double* dQ = up(S.Q);
        const double* dc = up(T.c);
        const double* dY = up(T.Y);
        const int* dperm = perm ? up(S.perm) : nullptr;
        double* ds1 = up(d1);
        double* ds2 = up(d2);
        LAUNCH(op_finish(P, KP, sh.grid, n, dperm, dQ, dc, dY, ds1, ds2));
        return std::vector<dvec>{down(ds1, n + GUARD), down(ds2, n + GUARD)};
    });
    for (size_t t = n; t < d1.size(); ++t) {
        c.same("guard", (long)t, o[0][t], d1[t]);
        c.same("guard", (long)t, o[1][t], d2[t]);
    }
    lvec yt, A;
    for (int r = 0; r < n; ++r) {
        const int i = S.orig(r);
        ref_yt(S, T, r, yt, A);
        ld_t s1 = d1[i], s2 = d2[i], a1 = fabsl((ld_t)d1[i]), a2 = fabsl((ld_t)d2[i]);
        for (int p = 0; p < P; ++p) {
            const ld_t t = (ld_t)S.z(r, p) * yt[p];
            s1 += t;
            s2 += t * t;
            a1 += A[p];
            a2 += A[p] * A[p];
        }
        c.value(kind == INT4, "dsum", i, o[0][i], s1, gam(KP + P + 1) * a1, a1);
        c.value(kind == INT4, "dsum2", i, o[1][i], s2, sq_bound(gam(KP + 1), A, d2[i], P), a2);
    }
}

static void grp_finish() {
    for (const Form* f : forms_of("diag_finish"))
        for (const Shape& sh : shapes_for(f->P))
            for (int nc : {f->P, f->P - 1})
                for (int perm = 0; perm < 2; ++perm)
                    for (int kind : {INT4, NORMAL})
                        if (nc >= 1) finish_case(f->P, f->KP, sh, nc, perm, kind);
}

// ---------------------------------------------------------------------------
// 5. entries
// ---------------------------------------------------------------------------
static const int kEntRows = 61;
// npairs x (r_i, r_j, i, j): every 7th pair diagonal, the next a repeat of the
// pair before it, the next that pair mirrored
static ivec make_tab(int64_t npairs, int n, const Sweep& S) {
    ivec tab((size_t)npairs * 4);
    int pi = 0, pj = 0;
    for (int64_t e = 0; e < npairs; ++e) {
        int ri = (int)(rnd() % n), rj = (int)(rnd() % n);
        if (e % 7 == 0) rj = ri;
        if (e % 7 == 4) ri = pi, rj = pj;
        if (e % 7 == 5) ri = pj, rj = pi;
        tab[4 * e] = ri;
        tab[4 * e + 1] = rj;
        tab[4 * e + 2] = S.orig(ri);
        tab[4 * e + 3] = S.orig(rj);
        pi = ri;
        pj = rj;
    }
    return tab;
}

static void entries_case(int P, int KP, int64_t npairs, int nc, int kind) {
    Case c(G_ENTRIES, kind_name(kind), fmt("accumulate P=%d KP=%d npairs=%lld nc=%d", P, KP, (long long)npairs, nc));
    if (g_list) return;
    const int n = kEntRows;
    const Sweep S = make_sweep(P, KP, n, P, true, kind);
    const Tail T = make_tail(P, KP, n, nc, kind);
    const ivec tab = make_tab(npairs, n, S);
    const dvec e1 = priors(npairs, kind), e2 = priors(npairs, kind);
    const std::vector<dvec> o = run_twice(c, [&]() {
        g_work.off = 0;
        const double* dQ = up(S.Q);
        const double* dc = up(T.c);
        const double* dY = up(T.Y);
        const int* dtab = up(tab);
        double* ds1 = up(e1);
        double* ds2 = up(e2);
        LAUNCH(op_entries(P, KP, npairs, dtab, KP ? dQ : nullptr, KP ? dc : nullptr, dY, ds1, ds2));
        return std::vector<dvec>{down(ds1, npairs + GUARD), down(ds2, npairs + GUARD)};
    });
    for (size_t t = npairs; t < e1.size(); ++t) {
        c.same("guard", (long)t, o[0][t], e1[t]);
        c.same("guard", (long)t, o[1][t], e2[t]);
    }
    std::vector<lvec> yt(n), A(n);
    for (int r = 0; r < n; ++r) ref_yt(S, T, r, yt[r], A[r]);
    lvec Ap(P);
    for (int64_t e = 0; e < npairs; ++e) {
        const int ri = tab[4 * e], rj = tab[4 * e + 1];
        ld_t s1 = e1[e], s2 = e2[e], a1 = fabsl((ld_t)e1[e]), a2 = fabsl((ld_t)e2[e]);
        for (int p = 0; p < P; ++p) {
            const ld_t t = 0.5L * ((ld_t)S.z(ri, p) * yt[rj][p] + (ld_t)S.z(rj, p) * yt[ri][p]);
            Ap[p] = 0.5L * (A[ri][p] + A[rj][p]);
            s1 += t;
            s2 += t * t;
            a1 += Ap[p];
            a2 += Ap[p] * Ap[p];
        }
        c.value(kind == INT4, "esum", (long)e, o[0][e], s1, gam(KP + P + 3) * a1, a1);
        c.value(kind == INT4, "esum2", (long)e, o[1][e], s2, sq_bound(gam(KP + 3), Ap, e2[e], P), a2);
    }
}

static const int kKLd[5][2] = {{1, 1}, {3, 4}, {4, 4}, {5, 16}, {16, 16}};
// Q, G: n x ld with NaN in the columns [k, ld) and in the padding rows; H: k x k
// column-major, then NaN up to 16 x 16
struct Defl {
    dvec Q, G, H;
};
static Defl make_defl(int n, int k, int ld, int kind) {
    Defl D;
    D.Q = nan_padded(block((size_t)n * ld, kind, true), (size_t)kPadRows * ld);
    D.G = nan_padded(block((size_t)n * ld, kind), (size_t)kPadRows * ld);
    for (int r = 0; r < n; ++r)
        for (int c = k; c < ld; ++c) D.Q[(size_t)r * ld + c] = D.G[(size_t)r * ld + c] = NAN;
    D.H = nan_padded(block((size_t)k * k, kind, true), 256 - (size_t)k * k);
    return D;
}

static void e0_case(int64_t npairs, int k, int ld, int kind) {
    Case c(G_ENTRIES, kind_name(kind), fmt("e0 npairs=%lld k=%d ld=%d", (long long)npairs, k, ld));
    if (g_list) return;
    const int n = kEntRows;
    const Sweep S = make_sweep(1, 0, n, 1, true, kind);  // for the row order alone
    const Defl D = make_defl(n, k, ld, kind);
    const ivec tab = make_tab(npairs, n, S);
    const std::vector<dvec> o = run_twice(c, [&]() {
        g_work.off = 0;
        const double* dQ = up(D.Q);
        const double* dG = up(D.G);
        const double* dH = up(D.H);
        const int* dtab = up(tab);
        double* de0 = up(sentinels(npairs));
        LAUNCH(op_e0(npairs, dtab, k, dQ, dG, ld, dH, de0));
        return std::vector<dvec>{down(de0, npairs + GUARD)};
    });
    c.written("e0", sentinels(npairs), o[0], npairs);
    for (int64_t e = 0; e < npairs; ++e) {
        const double* qi = D.Q.data() + (size_t)tab[4 * e + 2] * ld;
        const double* qj = D.Q.data() + (size_t)tab[4 * e + 3] * ld;
        const double* gi = D.G.data() + (size_t)tab[4 * e + 2] * ld;
        const double* gj = D.G.data() + (size_t)tab[4 * e + 3] * ld;
        ld_t a = 0.0L, aa = 0.0L, b2 = 0.0L, ab = 0.0L;
        for (int cc = 0; cc < k; ++cc) {
            a += (ld_t)qi[cc] * gj[cc] + (ld_t)gi[cc] * qj[cc];
            aa += fabsl((ld_t)qi[cc] * gj[cc]) + fabsl((ld_t)gi[cc] * qj[cc]);
            for (int b = 0; b < k; ++b) {
                const ld_t h = D.H[b + cc * k];
                b2 += (ld_t)qi[b] * h * qj[cc] + (ld_t)qj[b] * h * qi[cc];
                ab += fabsl((ld_t)qi[b] * h * qj[cc]) + fabsl((ld_t)qj[b] * h * qi[cc]);
            }
        }
        c.value(kind == INT4, "e0", (long)e, o[0][e], a - 0.5L * b2, gam(k + 3) * aa + gam(2 * k + 3) * 0.5L * ab, aa + ab);
    }
}

static void grp_entries() {
    for (const Form* f : forms_of("entries_accumulate")) {
        const int ppb = rpb_of(f->P);
        for (int64_t np : {1, ppb - 1, ppb, ppb + 1, 3 * ppb + 5})
            for (int nc : {f->P, f->P - 1})
                for (int kind : {INT4, NORMAL})
                    if (nc >= 1) entries_case(f->P, f->KP, np, nc, kind);
    }
    // the second trip past entries_grid's cap of 4096 workgroups
    if (std::find(kWidths.begin(), kWidths.end(), 16) != kWidths.end()) {
        const int64_t big = (int64_t)4096 * 32 + 33;
        entries_case(16, 0, big, 16, INT4);
        entries_case(16, 16, big, 16, INT4);
        entries_case(16, 4, big, 16, NORMAL);
    }
    for (auto& kl : kKLd)
        for (int64_t np : {1, 255, 256, 257, 3 * 256 + 5})
            for (int kind : {INT4, NORMAL}) e0_case(np, kl[0], kl[1], kind);
    e0_case((int64_t)2048 * 256 + 77, 1, 1, INT4);  // the second trip
}

// ---------------------------------------------------------------------------
// 6. d0
// ---------------------------------------------------------------------------
static void d0_case(int n, int k, int ld, int kind) {
    Case c(G_D0, kind_name(kind), fmt("n=%d k=%d ld=%d", n, k, ld));
    if (g_list) return;
    const Defl D = make_defl(n, k, ld, kind);
    const std::vector<dvec> o = run_twice(c, [&]() {
        g_work.off = 0;
        const double* dQ = up(D.Q);
        const double* dG = up(D.G);
        const double* dH = up(D.H);
        double* dd = up(sentinels(n));
        LAUNCH(op_d0(n, k, dQ, dG, ld, dH, dd));
        return std::vector<dvec>{down(dd, n + GUARD)};
    });
    c.written("d0", sentinels(n), o[0], n);
    for (int r = 0; r < n; ++r) {
        const double* q = D.Q.data() + (size_t)r * ld;
        const double* g = D.G.data() + (size_t)r * ld;
        ld_t a = 0.0L, aa = 0.0L, b2 = 0.0L, ab = 0.0L;
        for (int cc = 0; cc < k; ++cc) {
            a += (ld_t)q[cc] * g[cc];
            aa += fabsl((ld_t)q[cc] * g[cc]);
            for (int b = 0; b < k; ++b) {
                b2 += (ld_t)q[b] * D.H[b + cc * k] * q[cc];
                ab += fabsl((ld_t)q[b] * D.H[b + cc * k] * q[cc]);
            }
        }
        c.value(kind == INT4, "d0", r, o[0][r], 2.0L * a - b2, gam(k + 1) * 2.0L * aa + gam(2 * k + 1) * ab, 2.0L * aa + ab);
    }
}

static void grp_d0() {
    for (auto& kl : kKLd)
        for (int n : {1, 255, 256, 257})
            for (int kind : {INT4, NORMAL}) d0_case(n, kl[0], kl[1], kind);
    d0_case(2048 * 256 + 300, 1, 1, INT4);  // the second trip
}

// ---------------------------------------------------------------------------
// 7. adapt_stream
// ---------------------------------------------------------------------------
// The slots of a chunked basis: chunk q holds min(spc, m - q spc) slots of
// n nc values and then `tail` NaNs; the chunks are separate blocks of the
// arena, uploaded last chunk first.
struct Chunks {
    int n, m, nc, spc, nchunks;
    std::vector<dvec> chunk;
    dvec W;
    double u(int j, int64_t t) const { return chunk[j / spc][(size_t)(j % spc) * n * nc + t]; }
};
static Chunks make_chunks(int n, int m, int nc, int spc, int kind, bool big) {
    Chunks C;
    C.n = n;
    C.m = m;
    C.nc = nc;
    C.spc = spc;
    C.nchunks = (m + spc - 1) / spc;
    const size_t slot = (size_t)n * nc;
    for (int q = 0; q < C.nchunks; ++q)
        C.chunk.push_back(nan_padded(block((size_t)std::min(spc, m - q * spc) * slot, kind), big ? GUARD : slot));
    C.W = nan_padded(block((size_t)m * nc, kind, true), 4);
    return C;
}
static kt::SlotTab upload_chunks(const Chunks& C) {
    kt::SlotTab tab;
    for (const double*& p : tab.chunk) p = nullptr;
    for (int q = C.nchunks - 1; q >= 0; --q) tab.chunk[q] = up(C.chunk[q]);
    return tab;
}
// Y as launched: n x ldy of sentinels, then the guard
static dvec wsum_exec(const Chunks& C, int ldy, bool tabbed) {
    g_work.off = 0;
    const double* dW = up(C.W);
    double* dY = up(sentinels((size_t)C.n * ldy));
    if (tabbed) {
        const kt::SlotTab tab = upload_chunks(C);
        LAUNCH(op_wsum_tab(C.n, C.m, C.nc, tab, C.spc, dW, dY, ldy));
    } else {  // the same slots contiguously, for launch_weighted_sum (device only)
        dvec Uc;
        for (int j = 0; j < C.m; ++j)
            for (int64_t t = 0; t < (int64_t)C.n * C.nc; ++t) Uc.push_back(C.u(j, t));
        const double* dU = up(nan_padded(Uc, 8));
        LAUNCH(kt::launch_weighted_sum(C.n, C.m, C.nc, C.nc, dU, C.nc, (int64_t)C.n * C.nc, dW, dY, ldy, 0));
    }
    return down(dY, (size_t)C.n * ldy + GUARD);
}

static void wsum_case(int n, int m, int spc, int nc, int ldy, int kind, bool big) {
    Case c(G_ADAPT, kind_name(kind), fmt("weighted_sum_tab n=%d m=%d spc=%d nc=%d ldy=%d", n, m, spc, nc, ldy));
    if (g_list) return;
    const Chunks C = make_chunks(n, m, nc, spc, kind, big);
    const std::vector<dvec> o = run_twice(c, [&]() { return std::vector<dvec>{wsum_exec(C, ldy, true)}; });
    for (size_t t = (size_t)n * ldy; t < o[0].size(); ++t) c.same("guard", (long)t, o[0][t], SENT);
    for (int r = 0; r < n; ++r)
        for (int col = 0; col < ldy; ++col) {
            const size_t at = (size_t)r * ldy + col;
            if (col >= nc) {
                c.same("padding", (long)at, o[0][at], SENT);
                continue;
            }
            ld_t s = 0.0L, a = 0.0L;
            for (int j = 0; j < m; ++j) {
                const ld_t t = (ld_t)C.u(j, (int64_t)r * nc + col) * (ld_t)C.W[(size_t)j * nc + col];
                s += t;
                a += fabsl(t);
            }
            if (bits_of(o[0][at]) == bits_of(SENT)) c.fail("Y", (long)at, o[0][at], (double)s, 0.0, INFINITY);
            c.value(kind == INT4, "Y", (long)at, o[0][at], s, gam(m) * a, a);
        }
}

static void wsum_refused(int m, int spc, const char* why) {
    Case c(G_ADAPT, "refused", fmt("weighted_sum_tab m=%d spc=%d (%s)", m, spc, why));
    if (g_list) return;
    g_work.off = 0;
    const dvec U = block(64, NORMAL), W = block(64, NORMAL), Y0 = sentinels(32);
    const double* dU = up(U);
    const double* dW = up(W);
    double* dY = up(Y0);
    kt::SlotTab tab;
    for (const double*& p : tab.chunk) p = dU;
    const hipError_t e = op_wsum_tab(4, m, 2, tab, spc, dW, dY, 2);
    if (!g_host) {
        (void)hipGetLastError();
        HC(hipDeviceSynchronize());
    }
    if (e != hipErrorInvalidValue) c.fail("return code", 0, (double)e, (double)hipErrorInvalidValue, 0.0, INFINITY);
    c.unchanged("Y untouched", Y0, down(dY, Y0.size()));
}

static void unit_case(int n, int P, int nc, int variant) {
    static const char* vname[3] = {"distinct", "duplicates", "out_of_range"};
    Case c(G_ADAPT, "exact", fmt("unit_start n=%d P=%d nc=%d pos=%s", n, P, nc, vname[variant]));
    if (g_list) return;
    ivec pos(64);
    for (int col = 0; col < 64; ++col) {
        pos[col] = (col * 7 + 3) % n;  // the entries at and past nc: rows that a wrong kernel would mark
        if (col < nc && variant == 1) pos[col] = (col / 2 * 5 + 1) % n;
        if (col < nc && variant == 2) pos[col] = col % 3 == 0 ? -1 : (col % 3 == 1 ? n : (col * 7 + 3) % n);
    }
    dvec X0((size_t)n * P, 0.0);
    X0.resize(X0.size() + GUARD, SENT);
    const std::vector<dvec> o = run_twice(c, [&]() {
        g_work.off = 0;
        const int* dpos = up(pos);
        double* dX = up(X0);
        double* dsc = up(sentinels(P));
        double* dk2 = up(sentinels(P));
        LAUNCH(op_unit_start(n, P, nc, dpos, dX, dsc, dk2));
        return std::vector<dvec>{down(dX, X0.size()), down(dsc, P + GUARD), down(dk2, P + GUARD)};
    });
    dvec X = X0;
    for (int col = 0; col < P; ++col) {
        const bool ok = col < nc && pos[col] >= 0 && pos[col] < n;
        if (ok) X[(size_t)pos[col] * P + col] = 1.0;
        c.same("sc", col, o[1][col], ok ? 1.0 : 0.0);
        c.same("k2s", col, o[2][col], ok ? 1.0 : 0.0);
    }
    c.unchanged("X", X, o[0]);
    c.written("sc", sentinels(P), o[1], P);
    c.written("k2s", sentinels(P), o[2], P);
}

static void unit_refused(int n, int P, int nc) {
    Case c(G_ADAPT, "refused", fmt("unit_start n=%d P=%d nc=%d", n, P, nc));
    if (g_list) return;
    g_work.off = 0;
    const dvec X0 = sentinels(70 * 8), s0 = sentinels(70);
    const int* dpos = up(ivec(70, 0));
    double* dX = up(X0);
    double* dsc = up(s0);
    double* dk2 = up(s0);
    const hipError_t e = op_unit_start(n, P, nc, dpos, dX, dsc, dk2);
    if (!g_host) {
        (void)hipGetLastError();
        HC(hipDeviceSynchronize());
    }
    if (e != hipErrorInvalidValue) c.fail("return code", 0, (double)e, (double)hipErrorInvalidValue, 0.0, INFINITY);
    c.unchanged("X untouched", X0, down(dX, X0.size()));
    c.unchanged("sc untouched", s0, down(dsc, s0.size()));
    c.unchanged("k2s untouched", s0, down(dk2, s0.size()));
}

static const int kMSpc[5][2] = {{1, 1}, {8, 1}, {7, 3}, {24, 3}, {5, 8}};
static void grp_adapt() {
    for (auto& ms : kMSpc)
        for (int nc : {1, 3, 16})
            for (int n : {1, 300})
                for (int pad : {0, 3})
                    for (int kind : {INT4, NORMAL}) wsum_case(n, ms[0], ms[1], nc, nc + pad, kind, false);
    wsum_case(65537, 2, 1, 16, 16, INT4, true);  // n nc = 4096 * 256 + 16: the grid cap
    wsum_refused(3, 0, "spc < 1");
    wsum_refused(0, 2, "m < 1");
    wsum_refused(9, 1, "nine chunks");
    wsum_refused(17, 2, "nine chunks");
    for (int P : {1, 16, 64})
        for (int nc : {0, 1, P})
            for (int variant = 0; variant < 3; ++variant)
                for (int n : {1, 37}) unit_case(n, P, nc, variant);
    unit_refused(5, 65, 1);
    unit_refused(5, 16, 17);
    unit_refused(0, 16, 1);
    unit_refused(5, 16, -1);
}

// ---------------------------------------------------------------------------
// 8. contract
// ---------------------------------------------------------------------------
// a statement about the device code: counted, and trivially true with --host
#define DEVICE_ONLY(c) \
    if (g_list || g_host) return

static void same_all(Case& c, const char* what, const dvec& a, const dvec& b) {
    if (a.size() != b.size()) c.fail("sizes", 0, (double)a.size(), (double)b.size(), 0.0, INFINITY);
    else
        for (size_t t = 0; t < a.size(); ++t) c.same(what, (long)t, a[t], b[t]);
}

static void contract_sum_order(int nparts, int K) {
    Case c(G_CONTRACT, "a_sum_parts_order", fmt("nparts=%d K=%d", nparts, K));
    DEVICE_ONLY(c);
    const dvec part = nan_padded(block((size_t)nparts * K, NORMAL), 8);
    g_work.off = 0;
    const double* dpart = up(part);
    double* dout = up(sentinels(K));
    LAUNCH(op_sum_parts(nparts, K, dpart, dout));
    const dvec out = down(dout, K);
    for (int i = 0; i < K; ++i) {
        double s[64], t[64];
        for (int l = 0; l < 64; ++l) {
            s[l] = 0.0;
            for (int g = l; g < nparts; g += 64) s[l] += part[(size_t)g * K + i];
        }
        for (int off = 1; off < 64; off <<= 1) {
            for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ off];
            memcpy(s, t, sizeof s);
        }
        c.same("out", i, out[i], s[0]);
    }
}

static void contract_start_stream(int P, int nc, bool perm) {
    const Shape sh = shapes_for(P)[3];
    Case c(G_CONTRACT, "b_start_is_rademacher", fmt("P=%d n=%d grid=%d nc=%d perm=%d", P, sh.n, sh.grid, nc, (int)perm));
    DEVICE_ONLY(c);
    const ivec pm = make_perm(sh.n);
    g_work.off = 0;
    const int* dperm = perm ? up(pm) : nullptr;
    double* dX = up(sentinels((size_t)sh.n * P));
    double* dR = up(sentinels((size_t)sh.n * P));
    double* dpart = up(sentinels((size_t)sh.grid * P));
    LAUNCH(op_start(P, 0, sh.grid, sh.n, nc, dperm, nullptr, nullptr, dX, dpart));
    LAUNCH(kt::launch_rademacher(P, sh.n, kSeed, kBase, dperm, dR, 0));
    const dvec X = down(dX, (size_t)sh.n * P), R = down(dR, (size_t)sh.n * P);
    for (int r = 0; r < sh.n; ++r)
        for (int p = 0; p < nc; ++p) c.same("X", (long)r * P + p, X[(size_t)r * P + p], R[(size_t)r * P + p]);
}

static void contract_combine_y(int P, int KP) {
    const Shape sh = shapes_for(P)[2];
    Case c(G_CONTRACT, "c_combine_y_is_combine", fmt("P=%d KP=%d n=%d grid=%d m=9", P, KP, sh.n, sh.grid));
    DEVICE_ONLY(c);
    const Sweep S = make_sweep(P, KP, sh.n, P, false, NORMAL);
    const Basis B = make_basis(P, sh.n, 9, 1, NORMAL);
    dvec Y[2];
    for (int pass = 0; pass < 2; ++pass) {
        g_work.off = 0;
        const double* dV = up(B.V);
        const double* dW = up(B.W);
        const int* ddepth = up(B.depth);
        const double* dQ = up(S.Q);
        double* dY = up(sentinels((size_t)sh.n * P));
        double* dpart = up(sentinels((size_t)sh.grid * KP * P));
        LAUNCH(op_combine(P, pass ? -1 : KP, sh.grid, sh.n, 9, B.mdepth, dV, B.sstride, dW, ddepth, nullptr, dQ, dY, dpart,
                          nullptr, nullptr));
        Y[pass] = down(dY, (size_t)sh.n * P + GUARD);
    }
    same_all(c, "Y", Y[1], Y[0]);
}

// pairs (a, b), (b, a) side by side, then the diagonal pairs (r, r) of every row
static void contract_entries(int P, int KP) {
    Case c(G_CONTRACT, "d_e_entries_mirror_and_diagonal", fmt("P=%d KP=%d", P, KP));
    DEVICE_ONLY(c);
    const int n = kEntRows, nmir = 40;
    const Sweep S = make_sweep(P, KP, n, P, true, NORMAL);
    const Tail T = make_tail(P, KP, n, P, NORMAL);
    ivec tab;
    for (int e = 0; e < nmir; ++e) {
        const int a = (int)(rnd() % n), b = (int)(rnd() % n);
        for (int v : {a, b, S.orig(a), S.orig(b), b, a, S.orig(b), S.orig(a)}) tab.push_back(v);
    }
    for (int r = 0; r < n; ++r)
        for (int v : {r, r, S.orig(r), S.orig(r)}) tab.push_back(v);
    const int64_t npairs = 2 * nmir + n;
    dvec prior(npairs, 0.25);
    prior.resize(npairs + GUARD, SENT);
    g_work.off = 0;
    const double* dQ = up(S.Q);
    const double* dc = up(T.c);
    const double* dY = up(T.Y);
    const int* dtab = up(tab);
    const int* dperm = up(S.perm);
    double* ds1 = up(prior);
    double* ds2 = up(prior);
    double* dd1 = up(prior);
    double* dd2 = up(prior);
    LAUNCH(op_entries(P, KP, npairs, dtab, KP ? dQ : nullptr, KP ? dc : nullptr, dY, ds1, ds2));
    const dvec s1 = down(ds1, npairs), s2 = down(ds2, npairs);
    for (int e = 0; e < nmir; ++e) {
        c.same("esum of (j, i)", 2 * e + 1, s1[2 * e + 1], s1[2 * e]);
        c.same("esum2 of (j, i)", 2 * e + 1, s2[2 * e + 1], s2[2 * e]);
    }
    if (KP == 0) return;  // launch_diag_finish has no KP = 0 form
    LAUNCH(op_finish(P, KP, kt::diag_grid(n, P), n, dperm, dQ, dc, dY, dd1, dd2));
    const dvec d1 = down(dd1, n);
    for (int r = 0; r < n; ++r) c.same("diagonal esum vs finish dsum", r, s1[2 * nmir + r], d1[S.orig(r)]);
}

static void contract_e0(int k, int ld) {
    Case c(G_CONTRACT, "d_e0_mirror", fmt("k=%d ld=%d", k, ld));
    DEVICE_ONLY(c);
    const int n = kEntRows, nmir = 300;
    const Defl D = make_defl(n, k, ld, NORMAL);
    ivec tab;
    for (int e = 0; e < nmir; ++e) {
        const int a = (int)(rnd() % n), b = (int)(rnd() % n);
        for (int v : {b, a, a, b, a, b, b, a}) tab.push_back(v);
    }
    g_work.off = 0;
    const double* dQ = up(D.Q);
    const double* dG = up(D.G);
    const double* dH = up(D.H);
    const int* dtab = up(tab);
    double* de0 = up(sentinels(2 * nmir));
    LAUNCH(op_e0(2 * nmir, dtab, k, dQ, dG, ld, dH, de0));
    const dvec e0 = down(de0, 2 * nmir);
    for (int e = 0; e < nmir; ++e) c.same("e0 of (j, i)", 2 * e + 1, e0[2 * e + 1], e0[2 * e]);
}

static void contract_wsum(int m, int spc, int nc) {
    Case c(G_CONTRACT, "f_wsum_tab_is_wsum", fmt("n=300 m=%d spc=%d nc=%d", m, spc, nc));
    DEVICE_ONLY(c);
    const Chunks C = make_chunks(300, m, nc, spc, NORMAL, false);
    same_all(c, "Y", wsum_exec(C, nc + 3, true), wsum_exec(C, nc + 3, false));
}

// g: a width outside the switch: hipErrorInvalidValue, outputs untouched
static void refused_case(const char* launcher, int P, int KP) {
    Case c(G_CONTRACT, "g_refused_width", fmt("%s P=%d KP=%d", launcher, P, KP));
    if (g_list) return;
    const int n = 40, PP = 32, KK = 16;  // buffers wide enough for any form asked for
    g_work.off = 0;
    const dvec in = block((size_t)(n + 4) * PP * KK / 8, NORMAL), out0 = sentinels((size_t)n * PP);
    const double* din = up(in);
    const int* ddepth = up(ivec(PP, 2));
    const int* dtab = up(ivec(4 * n, 1));
    double* o1 = up(out0);
    double* o2 = up(out0);
    double* o3 = up(out0);
    hipError_t e = hipSuccess;
    if (!strcmp(launcher, "diag_qtz")) e = op_qtz(P, KP, 1, n, P, nullptr, din, o1);
    else if (!strcmp(launcher, "diag_start")) e = op_start(P, KP, 1, n, P, nullptr, din, din, o1, o2);
    else if (!strcmp(launcher, "diag_combine"))
        e = op_combine(P, KP, 1, n, 2, 2, din, (int64_t)n * PP, din, ddepth, nullptr, din, o1, o2, o3, o3);
    else if (!strcmp(launcher, "diag_combine_y"))
        e = op_combine(P, -1, 1, n, 2, 2, din, (int64_t)n * PP, din, ddepth, nullptr, nullptr, o1, o2, o3, o3);
    else if (!strcmp(launcher, "diag_finish")) e = op_finish(P, KP, 1, n, nullptr, din, din, din, o1, o2);
    else e = op_entries(P, KP, n, dtab, din, din, din, o1, o2);
    if (!g_host) {
        (void)hipGetLastError();  // a clean state for the next case
        HC(hipDeviceSynchronize());
    }
    if (e != hipErrorInvalidValue) c.fail("return code", 0, (double)e, (double)hipErrorInvalidValue, 0.0, INFINITY);
    c.unchanged("first output untouched", out0, down(o1, out0.size()));
    c.unchanged("second output untouched", out0, down(o2, out0.size()));
    c.unchanged("third output untouched", out0, down(o3, out0.size()));
}

static void grp_contract() {
    for (int nparts : {1, 63, 64, 65, 1024})
        for (int K : {1, 5}) contract_sum_order(nparts, K);
    for (int P : kWidths)
        for (int perm = 0; perm < 2; ++perm)
            for (int nc : {P, P - 1})
                if (nc >= 1) contract_start_stream(P, nc, perm);
    for (const Form* f : forms_of("diag_combine"))
        if (f->KP > 0) contract_combine_y(f->P, f->KP);
    for (const Form* f : forms_of("entries_accumulate")) contract_entries(f->P, f->KP);
    for (auto& kl : kKLd) contract_e0(kl[0], kl[1]);
    for (auto& ms : kMSpc)
        for (int nc : {1, 3, 16}) contract_wsum(ms[0], ms[1], nc);
    for (const char* launcher :
         {"diag_qtz", "diag_start", "diag_combine", "diag_combine_y", "diag_finish", "entries_accumulate"}) {
        const bool y = !strcmp(launcher, "diag_combine_y");
        for (int P : {3, 32}) refused_case(launcher, P, y ? 0 : 4);
        if (y) continue;
        for (int KP : {2, 8}) refused_case(launcher, 4, KP);
        if (!strcmp(launcher, "diag_qtz") || !strcmp(launcher, "diag_finish")) refused_case(launcher, 4, 0);
    }
}

// ---------------------------------------------------------------------------
static const char* kMutations[] = {"qtz_drop_tail_row",     "qtz_dead_col_live",   "sum_parts_skip_64",
                                   "start_no_projection",   "start_norm_from_z",   "combine_ignore_depth",
                                   "combine_pair_depth",    "combine_dsum_by_row", "combine_overwrite",
                                   "finish_sign_by_row",    "entries_swap_signs",  "entries_dead_lane_adds",
                                   "e0_half_missing",       "d0_row_major_H",      "wsum_tab_chunk_off_by_one",
                                   "unit_start_oob_writes"};

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
                fprintf(stderr, "diag_check: unknown group %s\n", argv[a] + 8);
                return 2;
            }
        } else {
            fprintf(stderr, "usage: diag_check [--host [--mutate=NAME]] [--count] [--group=NAME] [--small]\n");
            return 2;
        }
    }
    if (!g_mut.empty()) {
        bool known = false;
        for (const char* m : kMutations) known = known || g_mut == m;
        if (!known || !g_host) {
            fprintf(stderr, "diag_check: --mutate needs --host and one of:");
            for (const char* m : kMutations) fprintf(stderr, " %s", m);
            fprintf(stderr, "\n");
            return 2;
        }
    }
    if (g_small) kWidths = {1, 4, 16};
    forms_init();
    if (!g_host) {
        hipDeviceProp_t prop;
        HC(hipGetDeviceProperties(&prop, 0));
    }
    if (!g_list) {
        g_work.init((size_t)64 << 20);
        pools_init();
    }
    void (*const groups[NG])() = {grp_qtz, grp_start, grp_combine, grp_finish, grp_entries, grp_d0, grp_adapt, grp_contract};
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
