// expmv_check -- the expmv Taylor term kernels of kt_kernels.hip (k_expmv_begin,
// k_expmv_term, k_expmv_check, k_expmv_slot_check, k_expmv_step<P, FLAGS, SPLIT>,
// k_expmv_rows<P, FLAGS, CHECK>) and four small launchers that no other program
// calls (launch_sweep_scales, launch_gram_diag, launch_fill, launch_pair_start),
// called one by one through their kt::launch_* entry points (kt_launch.h), each
// result compared with a host reference in long double (or in exact integers).
//
// Groups: begin, unfused, step, stage, setup.
// Three kinds of assertion (as block_check / sweep_check / diag_check):
//   exact    b and F integers with |v| <= 8, unit weights or integer weights
//            with 1 <= |w| <= 2, mu in {0, 1, -2}, coef a power of two: every
//            product and sum is exact in fp64 in any order, with or without
//            fma, so the result must equal the reference by value.  The
//            reference (long double, 64-bit significand) verifies for every
//            element that the sum of the absolute terms, the new F and the
//            row sums, counted in units of the smallest power of two in play
//            (the product of the coefs so far), stay below 2^52; a case that
//            leaves that range is a failed case ("exact range"), with --host
//            too.  Multi-term stages use coef = 2^-4 or 2^-6 and degrees <= 40
//            for that reason.
//   bounded  standard-normal b, F and weights, mu, coef of order 1, against
//            long double, componentwise, u = 2^-53, gamma_k = k u / (1 - k u).
//            t = sum_i a_i x_i over a row of degree d is d fused or unfused
//            multiply-adds in some order: every term passes through at most d
//            roundings.  t - mu b is one more (an fma), coef times that one
//            more; mu b and the row sum share the roundings, so
//              |bout - ref| <= gamma_(d+2) |coef| (sum_i |a_i x_i| + |mu b|)
//            F' = fl(F + bout) adds one rounding of a sum whose size is at
//            most |F| + |coef| (sum_i |a_i x_i| + |mu b|):
//              |F' - ref| <= the above + u (|F| + |coef| (sum |a x| + |mu b|))
//            A row sum of nc absolute values (each within its bound e_c) is nc
//            additions: |fl(sum |got|) - sum |ref|| <= sum_c e_c + gamma_nc
//            (sum_c |ref_c| + sum_c e_c); max is 1-Lipschitz, so a maximum of
//            row sums is within the largest such per-row bound.
//            launch_sweep_scales: sqrt and the division are each allowed one
//            ulp (2 u relative, the device math library's documented worst
//            case): gamma_5 / sqrt(v).  Nothing is tuned to the kernels; each
//            group reports max_ratio, the largest error / bound it saw.
//            Bounded cases run with tol = 0, so no stop decision hangs on a
//            rounded number.
//   contract what the source states, bit for bit: forms 0, 1, 2 and 3 of
//            launch_expmv_step give identical F, bout columns < nc, active, mv
//            and slot maxima on the same input; forms 2 and 3 without task
//            lists are form 1; shuffled task lists give the bits of the
//            documented order; a stopped launch writes nothing; padding and
//            guards come back unchanged; refused arguments change nothing.
//
// Blocks: ld = P + 4 > P.  b input: columns < nc data, columns nc .. P-1 zero
// (the kernels gather P wide), columns >= P NaN.  b output: columns < nc
// sentinel, columns nc .. P-1 zero -- forms 0 and 1 write zeros there, forms 2
// and 3 must not write at all (a sentinel pad would not tell the two apart, a
// non-zero write does) -- columns >= P sentinel.  F: columns >= nc sentinel.
// A guard region follows every block, the partials and the state's slot words
// 2 .. 15.  With unit weights the device's value array holds NaN (never read).
// On the device every case runs twice from the same initial state and the
// two outputs, state block included, must agree bit for bit.
//
// CSR views: natural order, ascending columns, built here by the rules of
// build_csr (kt_runtime.cpp): long_rows = rows of degree > long_thresh (64),
// heaviest first and stable, the first n_heavy of them of degree >
// kExpmvCoopThresh; med_rows = rows with kMedThresh < degree <= long_thresh in
// row order; med_tasks / short_tasks = {row, beg, end, 0}, the short ones
// degree-descending (rows in order within a degree) inside windows of 4,096
// consecutive rows.  Matrices are not symmetric; with mu != 0 every non-empty
// row holds its diagonal entry.
//   classes  n = 600: degrees 0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65,
//            66, 127, 128, 129, 255, 256, 257, 300, 513, three rows each (rows
//            0 .. 22, 300 .. 322, 577 .. 599), the rest 0 .. 12; every width
//   nolong   n = 200, degrees <= 64;  nomed  n = 200, degrees <= 16 or 65 .. 90;
//   empty    n = 70, no entry (null long and medium lists)
//   tiny     n = 1, 2, 37;  ragged  n = 3 GPW + 1 short rows at each width
//   wrap     n = 8192, degree 1 but row 5000 (16), positive data: > 64
//            workgroups in every form, the maximum folded by workgroup >= 64
//   deep     (forms 2 and 3, P = 16 and P = 1; not with --small) sized from
//            expmv_rows_blocks so that the heavy, long, medium and short loops
//            of k_expmv_rows each make at least three trips (2.5 strides of
//            rows per class); the trip counts are asserted and reported
//   stage    n = 300, degrees 0 .. 15 and 18 .. 40 (no row of a degree that a
//            row-class defect of the step group touches), unit weights, nc = P
//
// Group stage: inf_norm, begin, terms k = 1 .. m ping-ponged as expmv_device
// does, the slot check after every term but the last in forms 1 and 2;
// after every launch active, mv, c1, c1s[], the three slot sets, F, both b
// blocks and the pinned host flag are compared with an exact reference state
// machine of expmv.m:71-92.  The reference alone decides which cases exist
// and a "coverage" case fails (with --host too) unless there are stops at
// terms 2, 3 and >= 4, a stage without stop, sharp pairs (tol_hi the smallest
// double with fl(tol nf) >= c1 + c2, tol_lo its predecessor) of which one has
// fl(tol_hi nf) == c1 + c2 exactly, and a two-stage run whose first stage's
// term maxima exceed every term maximum of the second.
//
// Planted defects (--host --mutate=NAME), each reported in its group only:
// short_skip_deg16, med_skip_deg17, long_drop_last_chain_entry, heavy_row_twice,
// mu_ignored_long, weights_ignored, pad_written_rows, f_pad_written (step);
// stop_strict_less, c1_wrong_parity, stale_slot_set (the next set is zeroed
// only by terms k <= 3), mv_counts_stopped_term, stopped_term_writes,
// hflag_before_stop (stage); begin_keeps_set1 (only the first nb slots are
// zeroed; begin); scales_nan_as_positive, pair_start_same_sign (setup).
//
// Measured (MI355X, device mode): wall 2.7 s (step 1.7 s, most of it the deep
// shape and its reference; the siblings take 2-3 s); cases begin 21, unfused
// 77, step 962, stage 41, setup 101; max_ratio begin 0, unfused 0.988, step
// 0.963, stage 0, setup 0.28 (a row of degree 0 or 1 has two or three
// roundings, so the bound is attained almost exactly there); grid of forms 2
// and 3: 1,024 workgroups, three trips of every loop at P = 16 and P = 1.
// --host 3.2 s on a CPU, --host --small --mutate=NAME 0.5 s.
//
//   expmv_check                     run on the GPU
//   expmv_check --host              the same cases with every device call
//                                   replaced by a plain fp64 host loop written
//                                   from the launchers' contract (no GPU)
//   expmv_check --host --mutate=M   one deliberate defect in that stand-in
//   expmv_check --count             the case counts and the form table alone
//   --group=NAME runs one group; --small keeps the widths 1, 4 and 16 and
//   leaves the deep shape and n = 70000 out
//
// Prints one JSON line; exit status 0 iff no case failed, 1 on failures, 3 on
// a HIP error (nothing is launched after it), 2 on bad usage.
// Build: make -C tests/native/expmv_check (links the library's own objects).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../krylov_robustness_amd/csrc/kt_launch.h"

namespace kt {
void set_error(const std::string&) {}  // kt_dense.o's ABI edge; unused here
}  // namespace kt

typedef long double ld_t;
typedef std::vector<double> dvec;
typedef std::vector<int> ivec;
typedef std::vector<ld_t> lvec;
using kt::ExpmvState;
using kt::kTermSlots;
using kt::kTermSlotStride;

static bool g_host = false;
static bool g_list = false;  // --count: enumerate the cases, run nothing
static bool g_small = false;
static int g_only = -1;
static std::string g_mut;
static bool mut(const char* s) { return g_mut == s; }
static std::vector<int> kWidths = {1, 2, 4, 8, 16, 32};
static const int kLongThresh = 64;   // kt_internal.h
static const int kHostResident = 1024;  // --host: the grid cap of forms 2 and 3 (4 x 256)

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
enum { G_BEGIN, G_UNFUSED, G_STEP, G_STAGE, G_SETUP, NG };
static Group g_groups[NG] = {{"begin"}, {"unfused"}, {"step"}, {"stage"}, {"setup"}};
static std::chrono::steady_clock::time_point g_t0;

static std::string fmt(const char* f, ...) {
    char buf[400];
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

// launch_expmv_step's forms: the step group's enumeration runs off this table
struct Form {
    int P, unit, form, mu0;
    std::string reaches;
    long cases = 0;
};
static std::vector<Form> g_forms;
static long g_fallback_cases = 0;
static void forms_init() {
    for (int P : {1, 2, 4, 8, 16, 32})
        for (int unit : {1, 0})
            for (int form = 0; form < 4; ++form)
                for (int mu0 : {1, 0}) {
                    std::string r;
                    if (form < 2) {
                        r = fmt("k_expmv_step<%d, %s, %s>", P, unit ? "KF_UNIT" : "0", form == 1 ? "true" : "false");
                    } else {
                        const char* fl = unit ? (mu0 ? "KF_UNIT | KF_MU0" : "KF_UNIT") : (mu0 ? "KF_MU0" : "0");
                        r = fmt("k_expmv_rows<%d, %s, %s>", P, fl, form == 3 ? "true" : "false");
                    }
                    g_forms.push_back({P, unit, form, mu0, r});
                }
}
static void form_hit(int P, bool unit, int form, double mu) {
    for (Form& f : g_forms)
        if (f.P == P && f.unit == (unit ? 1 : 0) && f.form == form && f.mu0 == (mu == 0.0 ? 1 : 0)) f.cases++;
}

struct Trips {
    int P = 0, grid = 0, heavy = 0, lng = 0, med = 0, shrt = 0;
};
static std::vector<Trips> g_trips;

static void print_report(const char* hip_err) {
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - g_t0).count();
    long nfail = 0;
    for (int g = 0; g < NG; ++g) nfail += g_groups[g].nfail;
    printf("{\"expmv_check\": \"%s\", \"mode\": \"%s\", \"mutate\": \"%s\", \"wall_s\": %.3f, ",
           hip_err ? "HIP_ERROR" : (nfail ? "FAIL" : "ok"), g_list ? "count" : (g_host ? "host" : "device"),
           g_mut.c_str(), wall);
    if (hip_err) printf("\"hip_error\": \"%s\", ", hip_err);
    if (g_list) {
        printf("\"forms\": {\"expmv_step\": [");
        for (size_t i = 0; i < g_forms.size(); ++i) {
            const Form& f = g_forms[i];
            printf("%s{\"P\": %d, \"unit\": %d, \"form\": %d, \"mu0\": %d, \"cases\": %ld, \"reaches\": \"%s\"}",
                   i ? ", " : "", f.P, f.unit, f.form, f.mu0, f.cases, f.reaches.c_str());
        }
        printf("], \"fallback\": [{\"form\": \"2, 3 without task lists\", \"cases\": %ld, \"reaches\": "
               "\"k_expmv_step<P, FLAGS, true>\"}]}, ",
               g_fallback_cases);
    }
    printf("\"trips\": [");
    for (size_t i = 0; i < g_trips.size(); ++i) {
        const Trips& t = g_trips[i];
        printf("%s{\"P\": %d, \"grid\": %d, \"heavy\": %d, \"long\": %d, \"medium\": %d, \"short\": %d}", i ? ", " : "",
               t.P, t.grid, t.heavy, t.lng, t.med, t.shrt);
    }
    printf("], \"groups\": {");
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
    fprintf(stderr, "expmv_check: test setup: %s\n", msg.c_str());
    exit(2);
}

static uint64_t bits_of(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}
static double from_bits(uint64_t b) {
    double x;
    memcpy(&x, &b, 8);
    return x;
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
    void fail(const std::string& what, long idx, double got, double exp, double bound, double sc = 0.0) {
        if (std::isnan(sc)) sc = INFINITY;
        if (!bad || sc > score) {
            worst = Fail{name, shape, what, idx, got, exp, bound};
            score = sc;
        }
        bad = true;
    }
    // equal as numbers (exact arithmetic; +0 and -0 agree, NaN never does)
    void exact(const std::string& what, long idx, double got, double exp) {
        if (!(got == exp)) fail(what, idx, got, exp, 0.0, fabs(got - exp));
    }
    void same(const std::string& what, long idx, double got, double exp) {
        if (bits_of(got) != bits_of(exp)) fail(what, idx, got, exp, 0.0, INFINITY);
    }
    void eqi(const std::string& what, long got, long exp) {
        if (got != exp) fail(what, 0, (double)got, (double)exp, 0.0, INFINITY);
    }
    void bounded(const std::string& what, long idx, ld_t got, ld_t ref, ld_t bound) {
        const ld_t e = fabsl(got - ref);
        if (!(e <= bound)) {
            fail(what, idx, (double)got, (double)ref, (double)bound, (double)(e / bound));
        } else if (bound > 0.0L) {
            g.max_ratio = std::max(g.max_ratio, (double)(e / bound));
        }
    }
    void value(bool ex, const std::string& what, long idx, double got, ld_t ref, ld_t bound) {
        if (ex) exact(what, idx, got, (double)ref);
        else bounded(what, idx, got, ref, bound);
    }
    void unchanged(const std::string& what, const dvec& before, const dvec& after) {
        for (size_t t = 0; t < before.size(); ++t) same(what, (long)t, after[t], before[t]);
    }
    void repeat(const std::vector<dvec>& a, const std::vector<dvec>& b) {
        if (a.size() != b.size()) fail("second run: another number of outputs", 0, (double)b.size(), (double)a.size(), 0.0, INFINITY);
        for (size_t k = 0; k < a.size() && k < b.size(); ++k)
            for (size_t t = 0; t < a[k].size(); ++t)
                if (bits_of(a[k][t]) != bits_of(b[k][t]))
                    fail(fmt("second run differs (output %d)", (int)k), (long)t, b[k][t], a[k][t], 0.0, INFINITY);
    }
};

// ---------------------------------------------------------------------------
// memory: one arena (device memory, or host memory with --host), a per-case stack
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
    T* up(const T* h, size_t count) {
        const size_t b = count * sizeof(T);
        T* p = (T*)(base + off);
        if (off + b > cap) setup_die("arena too small");
        off += (b + 255) / 256 * 256;
        if (b) {
            if (g_host) memcpy(p, h, b);
            else HC(hipMemcpy(p, h, b, hipMemcpyHostToDevice));
        }
        return p;
    }
};
static Arena g_work;
template <class T>
static T* up(const std::vector<T>& h) {
    return g_work.up(h.data(), h.size());
}
static ExpmvState* up_state(const ExpmvState& s) { return g_work.up(&s, 1); }
template <class T>
static void put(T* p, const T* h, size_t n) {
    if (g_host) memcpy(p, h, n * sizeof(T));
    else HC(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice));
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
static ExpmvState down_state(const ExpmvState* p) { return down(p, 1)[0]; }
static dvec state_words(const ExpmvState& s) {
    dvec w(sizeof(ExpmvState) / 8);
    memcpy(w.data(), &s, sizeof(ExpmvState));
    return w;
}

// the stop flag: pinned, device-mapped (a plain int with --host)
static int* g_hflag_host = nullptr;
static int* g_hflag_dev = nullptr;
static void hflag_init() {
    if (g_host) {
        static int word;
        g_hflag_host = g_hflag_dev = &word;
    } else {
        HC(hipHostMalloc((void**)&g_hflag_host, sizeof(int), hipHostMallocMapped));
        HC(hipHostGetDevicePointer((void**)&g_hflag_dev, g_hflag_host, 0));
    }
}
static int hflag_read() { return __atomic_load_n(g_hflag_host, __ATOMIC_ACQUIRE); }
static void hflag_write(int v) { __atomic_store_n(g_hflag_host, v, __ATOMIC_RELEASE); }

// ---------------------------------------------------------------------------
// data
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
enum Kind { EXACT = 0, NORMAL = 1, POSITIVE = 2 };
static const char* kind_name(int kind) { return kind == NORMAL ? "bounded" : "exact"; }
static const size_t kPool = (size_t)1 << 20;
static dvec g_pool[3];
static size_t g_pos = 0;
static void pools_init() {
    for (dvec& p : g_pool) p.resize(kPool);
    for (size_t i = 0; i < kPool; ++i) {
        g_pool[0][i] = (double)((int)(rnd() % 17) - 8);  // integers in [-8, 8]
        g_pool[1][i] = rnormal();
        g_pool[2][i] = (double)(1 + (int)(rnd() % 8));   // integers in [1, 8]
    }
}
static dvec block(size_t count, int kind) {
    const dvec& p = g_pool[kind];
    dvec v(count);
    for (size_t i = 0; i < count; ++i) v[i] = p[(g_pos + i) & (kPool - 1)];
    g_pos += count + 17;
    return v;
}
// an n x ld block + guard: columns < nc from `data` (n x nc), columns nc .. P-1
// `pad`, columns >= P and the guard `tail`
static dvec make_block(int n, int nc, int P, int ld, const dvec* data, double fill, double pad, double tail) {
    dvec v((size_t)n * ld + GUARD, tail);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < P && c < ld; ++c)
            v[(size_t)r * ld + c] = c < nc ? (data ? (*data)[(size_t)r * nc + c] : fill) : pad;
    return v;
}

// ---------------------------------------------------------------------------
// matrices and their views (the rules of build_csr restated)
// ---------------------------------------------------------------------------
struct Mat {
    std::string name;
    int n = 0, wkind = 0;  // weights: 0 unit, 1 integers +-1, +-2, 2 normal
    ivec rp, ci;
    dvec va;
    ivec long_rows, med_rows, med_tasks, short_tasks;
    int n_heavy = 0;
    int deg(int r) const { return rp[r + 1] - rp[r]; }
    int n_long() const { return (int)long_rows.size(); }
    int n_med() const { return (int)med_rows.size(); }
    int n_short() const { return (int)short_tasks.size() / 4; }
};
static bool g_build_always = false;  // the stage scenarios are built with --count too
static Mat build_mat(const std::string& name, ivec deg, int wkind, bool diag) {
    Mat m;
    m.name = name;
    m.n = (int)deg.size();
    m.wkind = wkind;
    if (g_list && !g_build_always) return m;
    const int n = m.n;
    m.rp.assign(n + 1, 0);
    for (int r = 0; r < n; ++r) m.rp[r + 1] = m.rp[r] + std::min(deg[r], n);
    m.ci.resize(m.rp[n]);
    m.va.resize(m.rp[n]);
    ivec cols;
    for (int r = 0; r < n; ++r) {
        const int d = m.deg(r);
        if (!d) continue;
        // d distinct columns: an arithmetic progression mod n from the row itself
        // (diag) or from a random column
        int step = 1 + (int)(rnd() % 7);
        if ((int64_t)d * step >= n) step = 1;
        const int s = diag ? r : (int)(rnd() % n);
        cols.resize(d);
        for (int j = 0; j < d; ++j) cols[j] = (int)(((int64_t)s + (int64_t)j * step) % n);
        std::sort(cols.begin(), cols.end());
        for (int j = 0; j < d; ++j) {
            m.ci[m.rp[r] + j] = cols[j];
            double w = 1.0;
            if (wkind == 1) {
                w = (double)(1 + (int)(rnd() % 2));
                if (rnd() & 1) w = -w;
            } else if (wkind == 2) {
                w = rnormal();
            }
            m.va[m.rp[r] + j] = w;
        }
    }
    for (int r = 0; r < n; ++r)
        if (m.deg(r) > kLongThresh) m.long_rows.push_back(r);
    std::stable_sort(m.long_rows.begin(), m.long_rows.end(), [&](int a, int b) { return m.deg(a) > m.deg(b); });
    for (int r : m.long_rows) m.n_heavy += m.deg(r) > kt::kExpmvCoopThresh;
    for (int r = 0; r < n; ++r)
        if (m.deg(r) > kt::kMedThresh && m.deg(r) <= kLongThresh) {
            m.med_rows.push_back(r);
            m.med_tasks.insert(m.med_tasks.end(), {r, m.rp[r], m.rp[r + 1], 0});
        }
    for (int w0 = 0; w0 < n; w0 += 4096) {
        const int w1 = std::min(n, w0 + 4096);
        for (int d = kt::kMedThresh; d >= 0; --d)
            for (int r = w0; r < w1; ++r)
                if (m.deg(r) == d) m.short_tasks.insert(m.short_tasks.end(), {r, m.rp[r], m.rp[r + 1], 0});
    }
    return m;
}

struct DevMat {
    kt::CsrView v;
    const int* med_rows;
    int n_med;
};
// variant 0: the documented lists, 1: no task lists (forms 2 and 3 fall back),
// 2: the short and medium task lists shuffled
static DevMat upload_mat(const Mat& m, bool unit, int variant) {
    ivec ci = m.ci;
    dvec va = m.va;
    if (unit) std::fill(va.begin(), va.end(), NAN);  // never read with unit weights
    if (ci.empty()) {
        ci.push_back(0);
        va.push_back(NAN);
    }
    ivec mt = m.med_tasks, st = m.short_tasks;
    if (variant == 2) {
        // the same permutation in every run of a case (which slot a workgroup
        // folds into follows the order, so the state's bits do too)
        uint64_t x = 0x2545F4914F6CDD1Dull;
        auto shuffle4 = [&x](ivec& t) {
            const int cnt = (int)t.size() / 4;
            for (int i = cnt; i > 1; --i) {
                x ^= x << 13, x ^= x >> 7, x ^= x << 17;
                const int j = (int)(x % i);
                for (int e = 0; e < 4; ++e) std::swap(t[4 * (i - 1) + e], t[4 * j + e]);
            }
        };
        shuffle4(mt);
        shuffle4(st);
    }
    // an empty list still needs a non-null pointer for forms 2 and 3 (never read)
    if (mt.empty()) mt.assign(4, 0);
    if (st.empty()) st.assign(4, 0);
    DevMat d;
    d.v = kt::CsrView{};
    d.v.rp = up(m.rp);
    d.v.ci = up(ci);
    d.v.va = up(va);
    d.v.n = m.n;
    d.v.long_rows = m.n_long() ? up(m.long_rows) : nullptr;
    d.v.n_long = m.n_long();
    d.v.long_thresh = kLongThresh;
    d.v.split_thresh = kt::kSplitThresh;
    d.v.short_tasks = variant == 1 ? nullptr : up(st);
    d.v.n_short = m.n_short();
    d.v.med_tasks = variant == 1 ? nullptr : up(mt);
    d.v.n_heavy = m.n_heavy;
    d.med_rows = m.n_med() ? up(m.med_rows) : nullptr;
    d.n_med = m.n_med();
    return d;
}

// ---------------------------------------------------------------------------
// the state block
// ---------------------------------------------------------------------------
static uint64_t seed_word(int set, int slot, int w) {
    if (w < 2) return bits_of(1.0 + set + slot / 64.0 + w * 0.25);
    return 0xABCD000000000000ull + (uint64_t)(set * 10000 + slot * 16 + w);
}
static ExpmvState seeded_state(int active, int mv) {
    ExpmvState s;
    memset(&s, 0, sizeof s);
    s.active = active;
    s.mv = mv;
    s.c1 = 6.5;
    s.c1s[0] = 2.5;
    s.c1s[1] = 3.5;
    for (int t = 0; t < 3; ++t)
        for (int i = 0; i < kTermSlots; ++i)
            for (int w = 0; w < kTermSlotStride; ++w) s.term_max[t][i][w] = seed_word(t, i, w);
    return s;
}
static void set_zero(ExpmvState& s, int set) {
    for (int i = 0; i < kTermSlots; ++i) s.term_max[set][i][0] = s.term_max[set][i][1] = 0ull;
}
static double set_max(const ExpmvState& s, int set, int w) {
    uint64_t m = 0;
    for (int i = 0; i < kTermSlots; ++i) m = std::max<uint64_t>(m, s.term_max[set][i][w]);
    return from_bits(m);
}
enum { SET_SEEDED = 0, SET_ZERO = 1, SET_MAX = 2 };
// one slot set against what it should hold; the words 2 .. 15 of a slot are never written
static void check_set(Case& c, const std::string& at, const ExpmvState& s, int set, int kind, bool ex, ld_t mb,
                      ld_t mf, ld_t bb, ld_t bf) {
    for (int i = 0; i < kTermSlots; ++i) {
        for (int w = 2; w < kTermSlotStride; ++w)
            if (s.term_max[set][i][w] != seed_word(set, i, w))
                c.fail(at + fmt(": set %d slot padding written", set), i * 16 + w, 0.0, 0.0, 0.0, INFINITY);
        for (int w = 0; w < 2; ++w) {
            const uint64_t got = s.term_max[set][i][w];
            if (kind == SET_SEEDED && got != seed_word(set, i, w))
                c.fail(at + fmt(": set %d changed", set), i * 16 + w, from_bits(got), from_bits(seed_word(set, i, w)), 0.0, INFINITY);
            if (kind == SET_ZERO && got != 0ull)
                c.fail(at + fmt(": set %d not zero", set), i * 16 + w, from_bits(got), 0.0, 0.0, INFINITY);
        }
    }
    if (kind == SET_MAX) {
        c.value(ex, at + fmt(": max |b| row sum in set %d", set), set, set_max(s, set, 0), mb, bb);
        c.value(ex, at + fmt(": max |F| row sum in set %d", set), set, set_max(s, set, 1), mf, bf);
    }
}

// ---------------------------------------------------------------------------
// the launchers, or their fp64 stand-ins written from kt_launch.h's contract
// ---------------------------------------------------------------------------
static void host_zero_next(ExpmvState* s, int k) {
    if (mut("stale_slot_set") && k >= 4) return;
    set_zero(*s, (k + 1) % 3);
}
static bool host_stop(double c1, double c2, double tol, double nf) {
    volatile double lhs = c1 + c2, rhs = tol * nf;
    return mut("stop_strict_less") ? lhs < rhs : lhs <= rhs;
}

static hipError_t op_inf_norm(int n, int nc, const double* X, int ldx, double* partial) {
    if (!g_host) return kt::launch_inf_norm(n, nc, X, ldx, partial, nullptr);
    const int nb = kt::inf_norm_blocks();
    for (int b = 0; b < nb; ++b) partial[b] = 0.0;
    for (int r = 0; r < n; ++r) {
        double s = 0.0;
        for (int c = 0; c < nc; ++c) s += fabs(X[(size_t)r * ldx + c]);
        double& p = partial[(r / 256) % nb];
        p = std::max(p, s);
    }
    return hipSuccess;
}

static hipError_t op_begin(const double* partial, int nb, ExpmvState* st) {
    if (!g_host) return kt::launch_expmv_begin(partial, nb, st, nullptr);
    double mx = 0.0;
    for (int i = 0; i < nb; ++i) mx = std::max(mx, partial[i]);
    st->c1 = mx;
    st->c1s[1] = mx;
    st->active = 1;
    const int nz = mut("begin_keeps_set1") ? std::min(nb, kTermSlots) : kTermSlots;
    for (int i = 0; i < nz; ++i) st->term_max[1][i][0] = st->term_max[1][i][1] = 0ull;
    return hipSuccess;
}

static int term_blocks(int n) {  // expmv_term_blocks restated
    const int b = (n + 255) / 256;
    return std::max(1, std::min(b, kt::inf_norm_blocks()));
}

static hipError_t op_term(int n, int nc, double mu, double coef, const double* Ab, double* b, double* F, int ld,
                          double* partial, const ExpmvState* st) {
    if (!g_host) return kt::launch_expmv_term(n, nc, mu, coef, Ab, b, F, ld, partial, st, nullptr);
    if (!st->active) return hipSuccess;
    const int nb = term_blocks(n);
    for (int i = 0; i < 2 * nb; ++i) partial[i] = 0.0;
    for (int r = 0; r < n; ++r) {
        double sb = 0.0, sf = 0.0;
        for (int c = 0; c < nc; ++c) {
            const size_t o = (size_t)r * ld + c;
            const double bn = coef * std::fma(-mu, b[o], Ab[o]);  // as launch_axpby(-mu, b, 1, Ab)
            const double f = F[o] + bn;
            b[o] = bn;
            F[o] = f;
            sb += fabs(bn);
            sf += fabs(f);
        }
        const int blk = (r / 256) % nb;
        partial[blk] = std::max(partial[blk], sb);
        partial[nb + blk] = std::max(partial[nb + blk], sf);
    }
    return hipSuccess;
}

static hipError_t op_check(int n, const double* partial, double tol, ExpmvState* st) {
    if (!g_host) return kt::launch_expmv_check(n, partial, tol, st, nullptr);
    if (!st->active) return hipSuccess;
    const int nb = term_blocks(n);
    double c2 = 0.0, nf = 0.0;
    for (int i = 0; i < nb; ++i) {
        c2 = std::max(c2, partial[i]);
        nf = std::max(nf, partial[nb + i]);
    }
    st->mv += 1;
    volatile double lhs = st->c1 + c2, rhs = tol * nf;
    if (lhs <= rhs) st->active = 0;
    else st->c1 = c2;
    return hipSuccess;
}

static hipError_t op_slot_check(ExpmvState* s, int k, double tol, int* hflag, int stage) {
    if (!g_host) return kt::launch_expmv_slot_check(s, k, tol, nullptr, hflag, stage);
    host_zero_next(s, k);
    if (!s->active) return hipSuccess;
    const double c1 = s->c1s[mut("c1_wrong_parity") ? (k + 1) & 1 : k & 1];
    const double c2 = set_max(*s, k % 3, 0), nf = set_max(*s, k % 3, 1);
    if (hflag && mut("hflag_before_stop")) *hflag = stage;
    if (host_stop(c1, c2, tol, nf)) {
        s->active = 0;
        if (hflag) *hflag = stage;
    } else {
        s->c1s[(k + 1) & 1] = c2;
    }
    return hipSuccess;
}

static hipError_t host_step(int P, bool unit, const kt::CsrView& M, const int* med_rows, int n_med, int nc, int ld,
                            double mu_in, double coef, double tol, int k, const double* bin, double* bout, double* F,
                            ExpmvState* s, int form, int* hflag, int stage) {
    if (P != 1 && P != 2 && P != 4 && P != 8 && P != 16 && P != 32) return hipErrorInvalidValue;
    if ((form == 2 || form == 3) && !(M.short_tasks && M.med_tasks)) form = 1;
    const bool fused = form == 0 || form == 3, rows = form >= 2;
    bool run = s->active != 0;
    if (run && fused && k > 1) {  // the check of term k - 1
        const double c1 = s->c1s[mut("c1_wrong_parity") ? k & 1 : (k - 1) & 1];
        const double c2 = set_max(*s, (k - 1) % 3, 0), nf = set_max(*s, (k - 1) % 3, 1);
        if (hflag && mut("hflag_before_stop")) *hflag = stage;
        if (host_stop(c1, c2, tol, nf)) {
            s->active = 0;
            if (hflag) *hflag = stage;
            run = false;
        } else {
            s->c1s[k & 1] = c2;
        }
    }
    if (!run) {
        if (mut("mv_counts_stopped_term")) s->mv += 1;
        if (!mut("stopped_term_writes")) return hipSuccess;
    } else {
        s->mv += 1;
        if (fused) host_zero_next(s, k);
    }
    // cls: 0 short, 1 medium, 2 long, 3 heavy
    auto row = [&](int r, int beg, int end, int cls) {
        const int d = end - beg;
        if (cls == 0 && d == 16 && mut("short_skip_deg16")) return;
        if (cls == 1 && d == 17 && mut("med_skip_deg17")) return;
        if (cls >= 2 && mut("long_drop_last_chain_entry")) end -= 1;
        const double mu = (cls >= 2 && mut("mu_ignored_long")) ? 0.0 : mu_in;
        double sb = 0.0, sf = 0.0;
        for (int c = 0; c < nc; ++c) {
            double t = 0.0;
            for (int q = beg; q < end; ++q) {
                const double a = (unit || mut("weights_ignored")) ? 1.0 : M.va[q];
                t += a * bin[(size_t)M.ci[q] * ld + c];
            }
            const size_t o = (size_t)r * ld + c;
            if (mu != 0.0) t = std::fma(-mu, bin[o], t);  // as launch_axpby(-mu, b, 1, Ab)
            const double bn = coef * t;
            const double f = F[o] + bn;
            bout[o] = bn;
            F[o] = f;
            sb += fabs(bn);
            sf += fabs(f);
        }
        for (int c = nc; c < P; ++c) {
            const size_t o = (size_t)r * ld + c;
            if (!rows) bout[o] = 0.0;
            else if (mut("pad_written_rows")) bout[o] = 1.0;
            if (mut("f_pad_written")) F[o] = 0.0;
        }
        if (run) {
            uint64_t* slot = (uint64_t*)s->term_max[k % 3][r % kTermSlots];
            slot[0] = std::max<uint64_t>(slot[0], bits_of(sb));
            slot[1] = std::max<uint64_t>(slot[1], bits_of(sf));
        }
    };
    if (!rows) {
        for (int i = 0; i < M.n_long; ++i) row(M.long_rows[i], M.rp[M.long_rows[i]], M.rp[M.long_rows[i] + 1], 2);
        for (int i = 0; i < n_med; ++i) row(med_rows[i], M.rp[med_rows[i]], M.rp[med_rows[i] + 1], 1);
        for (int r = 0; r < M.n; ++r)
            if (M.rp[r + 1] - M.rp[r] <= kt::kMedThresh) row(r, M.rp[r], M.rp[r + 1], 0);
    } else {
        for (int i = 0; i < M.n_heavy; ++i) row(M.long_rows[i], M.rp[M.long_rows[i]], M.rp[M.long_rows[i] + 1], 3);
        const int l0 = (mut("heavy_row_twice") && M.n_heavy > 0) ? M.n_heavy - 1 : M.n_heavy;
        for (int i = l0; i < M.n_long; ++i) row(M.long_rows[i], M.rp[M.long_rows[i]], M.rp[M.long_rows[i] + 1], 2);
        for (int i = 0; i < n_med; ++i) row(M.med_tasks[4 * i], M.med_tasks[4 * i + 1], M.med_tasks[4 * i + 2], 1);
        for (int i = 0; i < M.n_short; ++i)
            row(M.short_tasks[4 * i], M.short_tasks[4 * i + 1], M.short_tasks[4 * i + 2], 0);
    }
    return hipSuccess;
}
static hipError_t op_step(int P, bool unit, const DevMat& D, int nc, int ld, double mu, double coef, double tol, int k,
                          const double* bin, double* bout, double* F, ExpmvState* s, int form, int* hflag, int stage) {
    if (!g_host)
        return kt::launch_expmv_step(P, unit, D.v, D.med_rows, D.n_med, nc, ld, mu, coef, tol, k, bin, bout, F, s,
                                     nullptr, form, hflag, stage);
    return host_step(P, unit, D.v, D.med_rows, D.n_med, nc, ld, mu, coef, tol, k, bin, bout, F, s, form, hflag, stage);
}

// the grid of forms 2 and 3
static int rows_grid(int n_long, int n_med, int n_short) {
    const int tasks = n_long + n_med + (n_short + 7) / 8;
    if (!g_host) return kt::expmv_rows_blocks(tasks);
    return std::max(1, std::min(kHostResident, (tasks + 3) / 4));
}
static int gpw_of(int P) { return P >= 2 ? 64 / (P / 2) : 64; }  // short rows per wave

static hipError_t op_sweep_scales(const double* n2, int nc, int P, int mode, double* a, double* b) {
    if (!g_host) return kt::launch_sweep_scales(n2, nc, P, mode, a, b, nullptr);
    for (int t = 0; t < (mode ? 9 * P : P); ++t) {
        const int c = t % P, q = t / P;
        const double v = c < nc ? n2[c] : 0.0;
        const bool pos = mut("scales_nan_as_positive") ? !(v <= 0.0) : v > 0.0;
        const double s = pos ? 1.0 / sqrt(v) : 0.0;
        if (mode == 0) {
            a[t] = s;
            b[t] = pos ? v : 0.0;
        } else {
            a[t] = q == 0 ? s : (q == 6 ? 1.0 : 0.0);
        }
    }
    return hipSuccess;
}
static hipError_t op_gram_diag(const double* G, int ld, int nc, double* n2) {
    if (!g_host) return kt::launch_gram_diag(G, ld, nc, n2, nullptr);
    for (int c = 0; c < nc; ++c) n2[c] = G[c + (size_t)c * ld];
    return hipSuccess;
}
static hipError_t op_fill(double* x, int count, double v) {
    if (!g_host) return kt::launch_fill(x, count, v, nullptr);
    for (int t = 0; t < count; ++t) x[t] = v;
    return hipSuccess;
}
static hipError_t op_pair_start(int n, int P, int np, const int* pos, double* X, double* sc, double* k2s) {
    if (!g_host) return kt::launch_pair_start(n, P, np, pos, X, sc, k2s, nullptr);
    if (n < 2 || P < 2 || P > 64 || (P & 1) || np < 0 || 2 * np > P) return hipErrorInvalidValue;
    for (int c = 0; c < P; ++c) {
        const int p = c / 2;
        const int ri = p < np ? pos[2 * p] : -1, rj = p < np ? pos[2 * p + 1] : -1;
        const bool ok = ri >= 0 && ri < n && rj >= 0 && rj < n && ri != rj;
        if (ok) {
            X[(size_t)ri * P + c] = 1.0;
            X[(size_t)rj * P + c] = ((c & 1) && !mut("pair_start_same_sign")) ? -1.0 : 1.0;
        }
        sc[c] = ok ? 0.70710678118654752440 : 0.0;
        k2s[c] = ok ? 2.0 : 0.0;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// the reference of one term (long double) with the a-priori bounds
// ---------------------------------------------------------------------------
struct TermRef {
    lvec b, f, eb, ef;      // n x nc: values and bounds
    lvec sb, sf, esb, esf;  // per row: sums of |b|, |F| and their bounds
    ld_t mb = 0, mf = 0, emb = 0, emf = 0;  // maxima of the row sums, their bounds
    bool in_range = true;   // exact inputs: everything below 2^52 units
};
// bin, F: n x ld blocks; unit_in / unit_out: the power of two that every input /
// output value is a multiple of (exact kind)
static TermRef ref_term(const Mat& m, bool unit, int nc, int ld, double mu, double coef, const dvec& bin,
                        const dvec& F, ld_t unit_in = 1.0L, ld_t unit_out = 1.0L) {
    TermRef R;
    const int n = m.n;
    R.b.resize((size_t)n * nc);
    R.f = R.eb = R.ef = R.b;
    R.sb.assign(n, 0);
    R.sf = R.esb = R.esf = R.sb;
    for (int r = 0; r < n; ++r) {
        const int d = m.deg(r);
        ld_t seb = 0, sef = 0;
        for (int c = 0; c < nc; ++c) {
            ld_t t = 0, at = 0;
            for (int q = m.rp[r]; q < m.rp[r + 1]; ++q) {
                const ld_t a = unit ? 1.0L : (ld_t)m.va[q];
                const ld_t x = bin[(size_t)m.ci[q] * ld + c];
                t += a * x;
                at += fabsl(a * x);
            }
            const size_t o = (size_t)r * ld + c, i = (size_t)r * nc + c;
            t -= (ld_t)mu * bin[o];
            at += fabsl((ld_t)mu * bin[o]);
            const ld_t bn = (ld_t)coef * t, ab = fabsl((ld_t)coef) * at;
            R.b[i] = bn;
            R.f[i] = (ld_t)F[o] + bn;
            R.eb[i] = gam(d + 2) * ab;
            R.ef[i] = R.eb[i] + U * (fabsl((ld_t)F[o]) + ab);
            R.sb[r] += fabsl(bn);
            R.sf[r] += fabsl(R.f[i]);
            seb += R.eb[i];
            sef += R.ef[i];
            if (!(at < kExactMax * unit_in) || !(fabsl((ld_t)F[o]) + ab < kExactMax * unit_out)) R.in_range = false;
        }
        R.esb[r] = seb + gam(nc) * (R.sb[r] + seb);
        R.esf[r] = sef + gam(nc) * (R.sf[r] + sef);
        if (!(R.sb[r] < kExactMax * unit_out) || !(R.sf[r] < kExactMax * unit_out)) R.in_range = false;
        R.mb = std::max(R.mb, R.sb[r]);
        R.mf = std::max(R.mf, R.sf[r]);
        R.emb = std::max(R.emb, R.esb[r]);
        R.emf = std::max(R.emf, R.esf[r]);
    }
    return R;
}

// ---------------------------------------------------------------------------
// group begin
// ---------------------------------------------------------------------------
static void grp_begin() {
    for (int nb : {1, 63, 64, 255, 256, 257, 1000})
        for (int where = 0; where < 3; ++where) {
            Case c(G_BEGIN, "begin", fmt("nb=%d max_at=%s", nb, where == 0 ? "first" : where == 1 ? "last" : "middle"));
            if (g_list) continue;
            dvec part = block(nb, NORMAL);
            for (double& v : part) v = fabs(v);
            const int at = where == 0 ? 0 : where == 1 ? nb - 1 : nb / 2;
            part[at] = 11.0 + where;
            part.resize(nb + GUARD, NAN);  // not read past nb
            const ExpmvState s0 = seeded_state(where == 1 ? 7 : 0, 41);
            auto exec = [&]() {
                g_work.off = 0;
                double* dp = up(part);
                ExpmvState* ds = up_state(s0);
                LAUNCH(op_begin(dp, nb, ds));
                return std::vector<dvec>{state_words(down_state(ds))};
            };
            std::vector<dvec> o = exec();
            if (!g_host) c.repeat(o, exec());
            ExpmvState s;
            memcpy(&s, o[0].data(), sizeof s);
            c.same("c1", 0, s.c1, part[at]);
            c.same("c1s[1]", 0, s.c1s[1], part[at]);
            c.same("c1s[0] untouched", 0, s.c1s[0], s0.c1s[0]);
            c.eqi("active", s.active, 1);
            c.eqi("mv unchanged", s.mv, s0.mv);
            check_set(c, "after begin", s, 0, SET_SEEDED, true, 0, 0, 0, 0);
            check_set(c, "after begin", s, 1, SET_ZERO, true, 0, 0, 0, 0);
            check_set(c, "after begin", s, 2, SET_SEEDED, true, 0, 0, 0, 0);
        }
}

// ---------------------------------------------------------------------------
// group unfused: launch_expmv_term + launch_expmv_check
// ---------------------------------------------------------------------------
static void unfused_case(int n, int nc, double mu, int kind, bool stop, bool inactive) {
    const bool ex = kind == EXACT;
    const int ld = nc + 2, nb = term_blocks(n);
    const double coef = ex ? 0.5 : 0.8125, tol = ex && stop ? 1e9 : 0.0;
    Case c(G_UNFUSED, inactive ? "stopped" : kind_name(kind),
           fmt("n=%d nc=%d ld=%d mu=%g coef=%g tol=%g", n, nc, ld, mu, coef, tol));
    if (g_list) return;
    const dvec Abv = block((size_t)n * nc, kind), bv = block((size_t)n * nc, kind), Fv = block((size_t)n * nc, kind);
    const dvec Ab = make_block(n, nc, nc, ld, &Abv, 0, 0, NAN);
    const dvec b0 = make_block(n, nc, nc, ld, &bv, 0, 0, SENT), F0 = make_block(n, nc, nc, ld, &Fv, 0, 0, SENT);
    const dvec p0(2 * nb + GUARD, SENT);
    const ExpmvState s0 = seeded_state(inactive ? 0 : 1, 41);
    ExpmvState s1, s2;
    auto exec = [&]() {
        g_work.off = 0;
        double *dA = up(Ab), *db = up(b0), *dF = up(F0), *dp = up(p0);
        ExpmvState* ds = up_state(s0);
        LAUNCH(op_term(n, nc, mu, coef, dA, db, dF, ld, dp, ds));
        s1 = down_state(ds);
        const dvec p1 = down(dp, p0.size());
        LAUNCH(op_check(n, dp, tol, ds));
        s2 = down_state(ds);
        return std::vector<dvec>{down(db, b0.size()), down(dF, F0.size()), p1, down(dp, p0.size()), state_words(s1),
                                 state_words(s2)};
    };
    std::vector<dvec> o = exec();
    if (!g_host) c.repeat(o, exec());
    const dvec &b1 = o[0], &F1 = o[1], &p1 = o[2];
    c.unchanged("partial changed by the check", p1, o[3]);
    c.unchanged("state changed by the term", state_words(s0), o[4]);
    if (inactive) {
        c.unchanged("b written by a stopped term", b0, b1);
        c.unchanged("F written by a stopped term", F0, F1);
        c.unchanged("partial written by a stopped term", p0, p1);
        c.unchanged("state written by a stopped check", state_words(s0), o[5]);
        return;
    }
    // the reference: rows r with (r / 256) % nb == blk belong to partial[blk]
    lvec pb(nb, 0), pf(nb, 0), epb(nb, 0), epf(nb, 0);
    for (int r = 0; r < n; ++r) {
        ld_t sb = 0, sf = 0, seb = 0, sef = 0;
        for (int q = 0; q < nc; ++q) {
            const size_t o_ = (size_t)r * ld + q;
            const ld_t at = fabsl((ld_t)Ab[o_]) + fabsl((ld_t)mu * b0[o_]);
            const ld_t bn = (ld_t)coef * ((ld_t)Ab[o_] - (ld_t)mu * b0[o_]), f = (ld_t)F0[o_] + bn;
            // Ab is given: mu b (an fma) and coef are the two roundings: gamma_2
            const ld_t eb = gam(2) * fabsl((ld_t)coef) * at, ef = eb + U * (fabsl((ld_t)F0[o_]) + fabsl((ld_t)coef) * at);
            if (ex && !(at < kExactMax * 0.5L && fabsl((ld_t)F0[o_]) + at < kExactMax * 0.5L))
                c.fail("exact range", (long)o_, (double)at, 0.0, 0.0, INFINITY);
            c.value(ex, "b", (long)o_, b1[o_], bn, eb);
            c.value(ex, "F", (long)o_, F1[o_], f, ef);
            sb += fabsl(bn);
            sf += fabsl(f);
            seb += eb;
            sef += ef;
        }
        for (int q = nc; q < ld; ++q) {
            c.same("b padding", r, b1[(size_t)r * ld + q], SENT);
            c.same("F padding", r, F1[(size_t)r * ld + q], SENT);
        }
        const int blk = (r / 256) % nb;
        pb[blk] = std::max(pb[blk], sb);
        pf[blk] = std::max(pf[blk], sf);
        epb[blk] = std::max(epb[blk], seb + gam(nc) * (sb + seb));
        epf[blk] = std::max(epf[blk], sef + gam(nc) * (sf + sef));
    }
    for (size_t t = (size_t)n * ld; t < b0.size(); ++t) {
        c.same("b guard", (long)t, b1[t], SENT);
        c.same("F guard", (long)t, F1[t], SENT);
    }
    double c2 = 0.0, nf = 0.0;
    for (int i = 0; i < nb; ++i) {
        c.value(ex, "partial |b|", i, p1[i], pb[i], epb[i]);
        c.value(ex, "partial |F|", nb + i, p1[nb + i], pf[i], epf[i]);
        c2 = std::max(c2, p1[i]);
        nf = std::max(nf, p1[nb + i]);
    }
    for (size_t t = 2 * nb; t < p0.size(); ++t) c.same("partial guard", (long)t, p1[t], SENT);
    // the check: mv += 1; c1 + c2 <= tol nf ? active = 0 : c1 = c2, from the partials it was given
    ExpmvState e = s0;
    e.mv += 1;
    volatile double lhs = s0.c1 + c2, rhs = tol * nf;
    if (lhs <= rhs) e.active = 0;
    else e.c1 = c2;
    if (ex && stop && e.active) c.fail("setup: tol = 1e9 does not stop", 0, lhs, rhs, 0.0, INFINITY);
    c.unchanged("state after the check", state_words(e), o[5]);
}
static void grp_unfused() {
    int i = 0;
    for (int n : {1, 255, 256, 257, 1000, 70000}) {
        if (g_small && n == 70000) continue;
        for (int nc : {1, 3, 16})
            for (double mu : {0.0, i % 2 ? 1.0 : -2.0})
                for (int kind : {EXACT, NORMAL}) {
                    unfused_case(n, nc, kind == EXACT ? mu : mu * 0.37, kind, (i % 3) == 0, false);
                    ++i;
                }
    }
    for (int n : {1, 257, 1000})
        for (int nc : {1, 16}) {
            if (n == 257 && nc == 1) continue;
            unfused_case(n, nc, 1.0, EXACT, false, true);
        }
}

// ---------------------------------------------------------------------------
// group step: launch_expmv_step, one term per case
// ---------------------------------------------------------------------------
struct StepIn {
    const Mat* m;
    int P, nc, ld, k, kind;
    bool unit;
    double mu, coef;
    dvec bin, bout0, F0;
};
struct StepOut {
    dvec bout, F;
    ExpmvState st;
    hipError_t err;
};
static ExpmvState step_state(int form, int k) {
    ExpmvState s = seeded_state(1, 41);
    set_zero(s, k % 3);                                     // zeroed by the term before the last
    if (form == 1 || form == 2) set_zero(s, (k + 1) % 3);  // zeroed by the slot check of term k - 1
    return s;
}
static StepOut exec_step(const StepIn& in, int form, int variant, int P_arg, int seed_form = -1) {
    if (seed_form < 0) seed_form = form;
    g_work.off = 0;
    const DevMat D = upload_mat(*in.m, in.unit, variant);
    double *dbin = up(in.bin), *dbout = up(in.bout0), *dF = up(in.F0);
    ExpmvState* ds = up_state(step_state(seed_form, in.k));
    StepOut o;
    o.err = op_step(P_arg, in.unit, D, in.nc, in.ld, in.mu, in.coef, 0.0, in.k, dbin, dbout, dF, ds, form, nullptr, 0);
    if (o.err == hipErrorInvalidValue) {
        if (!g_host) (void)hipGetLastError();
    } else {
        HC(o.err);
    }
    if (!g_host) HC(hipDeviceSynchronize());
    o.bout = down(dbout, in.bout0.size());
    o.F = down(dF, in.F0.size());
    o.st = down_state(ds);
    return o;
}
static StepIn make_step_in(const Mat& m, int P, int nc, bool unit, double mu, int kind, int k) {
    StepIn in;
    in.m = &m;
    in.P = P;
    in.nc = nc;
    in.ld = P + 4;
    in.k = k;
    in.kind = kind;
    in.unit = unit;
    in.mu = mu;
    in.coef = kind == NORMAL ? -0.8125 : (k == 2 ? 2.0 : 0.5);
    if (g_list) return in;
    const dvec bv = block((size_t)m.n * nc, kind), Fv = block((size_t)m.n * nc, kind);
    in.bin = make_block(m.n, nc, P, in.ld, &bv, 0, 0.0, NAN);
    in.bout0 = make_block(m.n, nc, P, in.ld, nullptr, SENT, 0.0, SENT);
    in.F0 = make_block(m.n, nc, P, in.ld, &Fv, 0, SENT, SENT);
    return in;
}
static void check_step(Case& c, const StepIn& in, int form, const StepOut& o, const TermRef& R) {
    const bool ex = in.kind != NORMAL;
    const int n = in.m->n, nc = in.nc, P = in.P, ld = in.ld, k = in.k;
    if (ex && !R.in_range) c.fail("exact range", 0, 0.0, 0.0, 0.0, INFINITY);
    for (int r = 0; r < n; ++r) {
        for (int q = 0; q < ld; ++q) {
            const size_t t = (size_t)r * ld + q, i = (size_t)r * nc + q;
            if (q < nc) {
                c.value(ex, "bout", (long)t, o.bout[t], R.b[i], R.eb[i]);
                c.value(ex, "F", (long)t, o.F[t], R.f[i], R.ef[i]);
            } else {
                c.same(q < P ? "bout zero padding" : "bout padding", (long)t, o.bout[t], in.bout0[t]);
                c.same("F padding", (long)t, o.F[t], in.F0[t]);
            }
        }
    }
    for (size_t t = (size_t)n * ld; t < in.F0.size(); ++t) {
        c.same("bout guard", (long)t, o.bout[t], in.bout0[t]);
        c.same("F guard", (long)t, o.F[t], in.F0[t]);
    }
    const ExpmvState s0 = step_state(form, k);
    c.eqi("active", o.st.active, 1);
    c.eqi("mv", o.st.mv, s0.mv + 1);
    c.same("c1", 0, o.st.c1, s0.c1);
    const bool fused = form == 0 || form == 3;
    // the fused check of term k - 1 with tol = 0 does not stop and records c2
    const double c2 = set_max(s0, (k + 2) % 3, 0);
    c.same("c1s[k & 1]", 0, o.st.c1s[k & 1], fused && k > 1 ? c2 : s0.c1s[k & 1]);
    c.same("c1s[(k - 1) & 1]", 0, o.st.c1s[(k - 1) & 1], s0.c1s[(k - 1) & 1]);
    check_set(c, "after the term", o.st, k % 3, SET_MAX, ex, R.mb, R.mf, R.emb, R.emf);
    check_set(c, "after the term", o.st, (k + 1) % 3, SET_ZERO, ex, 0, 0, 0, 0);
    check_set(c, "after the term", o.st, (k + 2) % 3, SET_SEEDED, ex, 0, 0, 0, 0);
}
static std::vector<dvec> step_words(const StepOut& o) { return {o.bout, o.F, state_words(o.st)}; }
// forms 0 .. 3 agree on F, bout columns < nc, active, mv and the slot maxima
static void check_forms_agree(Case& c, const StepIn& in, const StepOut& a, const StepOut& b, bool whole) {
    const int n = in.m->n;
    for (int r = 0; r < n; ++r)
        for (int q = 0; q < (whole ? in.ld : in.nc); ++q) {
            const size_t t = (size_t)r * in.ld + q;
            c.same("bout differs between forms", (long)t, b.bout[t], a.bout[t]);
            c.same("F differs between forms", (long)t, b.F[t], a.F[t]);
        }
    c.eqi("active differs between forms", b.st.active, a.st.active);
    c.eqi("mv differs between forms", b.st.mv, a.st.mv);
    for (int w = 0; w < 2; ++w)
        c.same("slot maximum differs between forms", w, set_max(b.st, in.k % 3, w), set_max(a.st, in.k % 3, w));
}
static std::string step_shape_str(const StepIn& in, int form, const char* extra = "") {
    return fmt("mat=%s n=%d P=%d nc=%d ld=%d %s mu=%g coef=%g k=%d form=%d%s", in.m->name.c_str(), in.m->n, in.P, in.nc,
               in.ld, in.unit ? "unit" : "weighted", in.mu, in.coef, in.k, form, extra);
}
// one shape in the four forms (and, with `extras`, the fallback and the shuffled lists)
static void step_shape(const Mat& m, int P, int nc, bool unit, double mu, int kind, int k, bool extras,
                       int forms_mask = 15) {
    const StepIn in = make_step_in(m, P, nc, unit, mu, kind, k);
    TermRef R;
    if (!g_list) R = ref_term(m, unit, nc, in.ld, mu, in.coef, in.bin, in.F0, 1.0L, in.coef < 1.0 ? 0.5L : 1.0L);
    StepOut base[4];
    int first = -1;
    for (int form = 0; form < 4; ++form) {
        if (!(forms_mask >> form & 1)) continue;
        Case c(G_STEP, kind_name(kind), step_shape_str(in, form));
        form_hit(P, unit, form, mu);
        if (g_list) continue;
        base[form] = exec_step(in, form, 0, P);
        if (!g_host) c.repeat(step_words(base[form]), step_words(exec_step(in, form, 0, P)));
        check_step(c, in, form, base[form], R);
        if (first < 0) first = form;
        else check_forms_agree(c, in, base[first], base[form], false);
    }
    if (!extras) return;
    for (int form = 2; form < 4; ++form) {
        {
            Case c(G_STEP, "fallback", step_shape_str(in, form, " no_task_lists"));
            g_fallback_cases++;
            if (!g_list) {
                const StepOut o = exec_step(in, form, 1, P, 1);
                if (!g_host) c.repeat(step_words(o), step_words(exec_step(in, form, 1, P, 1)));
                check_step(c, in, 1, o, R);
                check_forms_agree(c, in, base[1], o, true);
                c.unchanged("state differs from form 1", state_words(base[1].st), state_words(o.st));
            }
        }
        {
            Case c(G_STEP, "task_order", step_shape_str(in, form, " shuffled_tasks"));
            if (!g_list) {
                const StepOut o = exec_step(in, form, 2, P);
                if (!g_host) c.repeat(step_words(o), step_words(exec_step(in, form, 2, P)));
                check_step(c, in, form, o, R);
                check_forms_agree(c, in, base[form], o, true);
            }
        }
    }
}
static void refused_case(const Mat& m, int P_arg, int form) {
    StepIn in = make_step_in(m, 16, 16, true, 0.0, EXACT, 1);
    Case c(G_STEP, "refused", step_shape_str(in, form, fmt(" P_arg=%d", P_arg).c_str()));
    if (g_list) return;
    const StepOut o = exec_step(in, form, 0, P_arg);
    if (o.err != hipErrorInvalidValue) c.fail("return code", 0, (double)o.err, (double)hipErrorInvalidValue, 0.0, INFINITY);
    c.unchanged("bout touched", in.bout0, o.bout);
    c.unchanged("F touched", in.F0, o.F);
    c.unchanged("state touched", state_words(step_state(form, 1)), state_words(o.st));
}

static ivec random_degs(int n, int lo, int hi) {
    ivec d(n);
    for (int& v : d) v = lo + (int)(rnd() % (hi - lo + 1));
    return d;
}
static ivec classes_degs() {
    static const int sp[] = {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 300, 513};
    const int ns = sizeof sp / sizeof sp[0], n = 600;
    ivec d = random_degs(n, 0, 12);
    for (int i = 0; i < ns; ++i) d[i] = d[300 + i] = d[n - ns + i] = sp[i];
    return d;
}

// the wrap shape: the workgroup that folds row `row` must have index >= 64
static void wrap_case(int form, int k) {
    const int n = 8192, row = 5000, P = 16;
    ivec d(n, 1);
    d[row] = 16;
    const Mat m = build_mat("wrap", d, 0, false);
    const StepIn in = make_step_in(m, P, P, true, 0.0, POSITIVE, k);
    Case c(G_STEP, "slot_wrap", step_shape_str(in, form));
    form_hit(P, true, form, 0.0);
    if (g_list) return;
    int grid, wg;
    if (form < 2) {
        grid = g_host ? m.n_long() + (m.n_med() + 3) / 4 + (n + 4 * gpw_of(P) - 1) / (4 * gpw_of(P))
                      : kt::expmv_step_blocks(n, P, m.n_long(), m.n_med());
        wg = m.n_long() + (m.n_med() + 3) / 4 + row / (4 * gpw_of(P));
    } else {
        grid = rows_grid(m.n_long(), m.n_med(), m.n_short());
        int t = 0;
        while (m.short_tasks[4 * t] != row) ++t;
        wg = ((t / gpw_of(P)) % (4 * grid)) / 4;
    }
    if (grid <= 64 || wg < 64) c.fail("setup: the maximum is not folded by a workgroup >= 64", wg, (double)grid, 65.0, 0.0, INFINITY);
    const TermRef R = ref_term(m, true, P, in.ld, 0.0, in.coef, in.bin, in.F0, 1.0L, 0.5L);
    if (!(R.sb[row] == R.mb && R.sf[row] == R.mf)) c.fail("setup: the marked row is not the maximum", row, 0.0, 0.0, 0.0, INFINITY);
    const StepOut o = exec_step(in, form, 0, P);
    if (!g_host) c.repeat(step_words(o), step_words(exec_step(in, form, 0, P)));
    check_step(c, in, form, o, R);
}

// the deep shape: every loop of k_expmv_rows makes at least three trips
static void deep_cases(int P) {
    // 2.5 strides of each class: workgroups (heavy), waves (long, medium), blocks of GPW short rows
    const int grid = g_list ? 1 : rows_grid(1 << 28, 0, 0), TW = 4 * grid, gpw = gpw_of(P);
    const int nh = 2 * grid + grid / 2 + 1, nl = 2 * TW + TW / 2 + 1, nm = nl, ns = (2 * TW + TW / 2) * gpw + 1;
    ivec d;
    if (!g_list) {
        d.reserve((size_t)nh + nl + nm + ns);
        // interleaved: one heavy, then 4 long, 4 medium and a run of short rows
        int h = 0, l = 0, me = 0, s = 0;
        while (h < nh || l < nl || me < nm || s < ns) {
            if (h < nh) d.push_back(257 + (h++ % 3));
            for (int i = 0; i < 4 && l < nl; ++i) d.push_back(65 + (l++ % 4));
            for (int i = 0; i < 4 && me < nm; ++i) d.push_back(17 + (me++ % 5));
            for (int i = 0; i < 4 * gpw && s < ns; ++i) d.push_back((s++ % 11) == 0 ? 9 + s % 8 : s % 3);
        }
    }
    struct V {
        int form, wkind, kind;
        double mu;
    };
    const V vs[] = {{2, 0, EXACT, 0.0}, {3, 0, EXACT, 0.0}, {3, 1, EXACT, 1.0}};
    Mat mats[2];
    for (int w = 0; w < 2; ++w) mats[w] = build_mat("deep", d, w, true);
    if (g_list) mats[0].n = mats[1].n = 0;
    int vi = 0;
    for (const V& v : vs) {
        const Mat& m = mats[v.wkind];
        const StepIn in = make_step_in(m, P, P, v.wkind == 0, v.mu, v.kind, 1 + vi++ % 3);
        Case c(G_STEP, "deep", g_list ? fmt("mat=deep P=%d form=%d", P, v.form) : step_shape_str(in, v.form));
        form_hit(P, v.wkind == 0, v.form, v.mu);
        if (g_list) continue;
        const int g = rows_grid(m.n_long(), m.n_med(), m.n_short());
        Trips t;
        t.P = P;
        t.grid = g;
        t.heavy = (m.n_heavy + g - 1) / g;
        t.lng = (m.n_long() - m.n_heavy + 4 * g - 1) / (4 * g);
        t.med = (m.n_med() + 4 * g - 1) / (4 * g);
        t.shrt = ((m.n_short() + gpw - 1) / gpw + 4 * g - 1) / (4 * g);
        if (v.form == 2) g_trips.push_back(t);
        if (t.heavy < 3 || t.lng < 3 || t.med < 3 || t.shrt < 3)
            c.fail("setup: a loop makes fewer than three trips", g, (double)std::min(std::min(t.heavy, t.lng), std::min(t.med, t.shrt)), 3.0, 0.0, INFINITY);
        const TermRef R = ref_term(m, in.unit, P, in.ld, in.mu, in.coef, in.bin, in.F0, 1.0L, 0.5L);
        const StepOut o = exec_step(in, v.form, 0, P);
        if (!g_host) c.repeat(step_words(o), step_words(exec_step(in, v.form, 0, P)));
        check_step(c, in, v.form, o, R);
    }
}

static void grp_step() {
    // class boundaries, every form of the table: widths x weights x mu x columns
    const ivec cd = g_list ? ivec(600, 0) : classes_degs();
    Mat classes[3];
    for (int w = 0; w < 3; ++w) classes[w] = build_mat("classes", cd, w, true);
    int i = 0;
    for (int P : kWidths) {
        ivec ncs = {1, P - 1, P};
        if (P == 32) ncs.push_back(17);
        std::sort(ncs.begin(), ncs.end());
        ncs.erase(std::unique(ncs.begin(), ncs.end()), ncs.end());
        for (int nc : ncs) {
            if (nc < 1) continue;
            for (int unit = 1; unit >= 0; --unit)
                for (int mz = 0; mz < 2; ++mz) {
                    const double mu_e = mz == 0 ? 0.0 : (i % 2 ? 1.0 : -2.0);
                    const int k = 1 + i % 3;
                    const bool extras = nc == P && unit == 1;
                    step_shape(classes[unit ? 0 : 1], P, nc, unit, mu_e, EXACT, k, extras);
                    step_shape(classes[unit ? 0 : 2], P, nc, unit, mu_e * 0.37, NORMAL, 1 + (i + 1) % 3, false);
                    ++i;
                }
        }
    }
    // no long rows, no medium rows, only empty rows; tiny and ragged sizes
    ivec dn = g_list ? ivec(200, 0) : random_degs(200, 0, 64), dm = g_list ? ivec(200, 0) : random_degs(200, 0, 16);
    if (!g_list) {
        dn[0] = 16, dn[1] = 17, dn[2] = 64, dn[199] = 64, dn[198] = 17;
        for (int r = 5; r < 200; r += 9) dm[r] = 65 + r % 26;
    }
    for (int P : kWidths) {
        const int gpw = gpw_of(P);
        for (int w = 0; w < 2; ++w) {
            const bool unit = w == 0;
            const double mu = w == 0 ? 0.0 : 1.0;
            const int k = 1 + (P + w) % 3;
            const Mat a = build_mat("nolong", dn, w, true), b = build_mat("nomed", dm, w, true),
                      e = build_mat("empty", ivec(70, 0), w, true);
            step_shape(a, P, P, unit, mu, EXACT, k, w == 0);
            step_shape(b, P, P, unit, mu, EXACT, k, false);
            step_shape(e, P, std::max(1, P - 1), unit, mu, EXACT, k, w == 0);
            for (int n : {1, 2, 37, 3 * gpw + 1}) {
                ivec d = g_list ? ivec(n, 0) : random_degs(n, 0, std::min(n, 16));
                if (!g_list && n == 37) d[20] = 20;
                if (!g_list && n <= 2) d[0] = n;
                const Mat t = build_mat(n == 3 * gpw + 1 ? "ragged" : "tiny", d, w, true);
                step_shape(t, P, P, unit, mu, EXACT, k, false);
            }
        }
    }
    for (int form = 0; form < 4; ++form) wrap_case(form, 1 + form % 3);
    if (!g_small)
        for (int P : {16, 1}) deep_cases(P);
    const Mat rm = build_mat("nolong", dn, 0, false);
    for (int form = 0; form < 4; ++form)
        for (int P : {3, 64}) refused_case(rm, P, form);
}

// ---------------------------------------------------------------------------
// group stage: the stop state machine
// ---------------------------------------------------------------------------
struct StageData {  // one stage of m terms on exact data, simulated in full
    int m = 0, nc = 0;
    double mu = 0, coef = 0;
    std::vector<dvec> b, F;  // b[k], F[k]: n x nc after term k (k = 0: the start)
    dvec c, nf;               // c[k] = norm(b_k, inf), nf[k] = norm(F_k, inf)
    bool in_range = true;
};
static StageData simulate(const Mat& A, int nc, double mu, double coef, int m, const dvec& b0, const dvec& F0,
                          ld_t unit0) {
    StageData S;
    S.m = m;
    S.nc = nc;
    S.mu = mu;
    S.coef = coef;
    S.b.push_back(b0);
    S.F.push_back(F0);
    auto norm = [&](const dvec& X) {
        double mx = 0;
        for (int r = 0; r < A.n; ++r) {
            double s = 0;
            for (int q = 0; q < nc; ++q) s += fabs(X[(size_t)r * nc + q]);
            mx = std::max(mx, s);
        }
        return mx;
    };
    S.c.push_back(norm(b0));
    S.nf.push_back(norm(F0));
    ld_t unit = unit0;
    for (int k = 1; k <= m; ++k) {
        const ld_t uo = unit * (ld_t)std::min(1.0, fabs(coef));
        const TermRef R = ref_term(A, true, nc, nc, mu, coef, S.b[k - 1], S.F[k - 1], unit, uo);
        S.in_range = S.in_range && R.in_range;
        dvec bk(R.b.size()), Fk(R.f.size());
        for (size_t t = 0; t < bk.size(); ++t) {
            bk[t] = (double)R.b[t];
            Fk[t] = (double)R.f[t];
        }
        S.b.push_back(bk);
        S.F.push_back(Fk);
        S.c.push_back((double)R.mb);
        S.nf.push_back((double)R.mf);
        unit = uo;
    }
    return S;
}
static bool ref_stop(const StageData& S, int k, double tol) {  // expmv.m:79-82 at term k
    volatile double lhs = S.c[k - 1] + S.c[k], rhs = tol * S.nf[k];
    return lhs <= rhs;
}
// the term whose check stops the stage; the last term's check is never made
static int stop_term(const StageData& S, double tol) {
    for (int k = 1; k < S.m; ++k)
        if (ref_stop(S, k, tol)) return k;
    return 0;
}
// tol_hi: the smallest double with fl(tol nf_j) >= c_(j-1) + c_j
static double tol_hi_of(const StageData& S, int j, bool* equal) {
    const double s = S.c[j - 1] + S.c[j], nf = S.nf[j];
    double t = s / nf;
    auto ge = [&](double x) {
        volatile double p = x * nf;
        return p >= s;
    };
    while (ge(t)) t = nextafter(t, 0.0);
    while (!ge(t)) t = nextafter(t, INFINITY);
    volatile double p = t * nf;
    *equal = p == s;
    return t;
}

struct Scenario {
    std::string name;
    int P = 16;
    double mu = 0;
    dvec b0;  // n x P
    // stage A, and (two-stage) stage B from A's F
    StageData A, B;
    double tolA = 0, tolB = 0;
    bool two = false;
};
static std::vector<Scenario> g_scen;
static bool g_cov_stop[3] = {false, false, false}, g_cov_equal = false, g_cov_nostop = false, g_cov_two = false,
            g_cov_range = true;
static Mat g_stage_mat[2];  // without / with the diagonal
static const int kStageN = 300, kStageM = 6;

static void build_scenarios() {
    // the same data in every mode and with any --group: its own stream and pool position
    const uint64_t rng_saved = g_rng;
    const size_t pos_saved = g_pos;
    g_rng = 0x9E3779B97F4A7C15ull;
    g_pos = 424243;
    g_build_always = true;
    ivec d = random_degs(kStageN, 0, 38);
    for (int& v : d)
        if (v == 16 || v == 17) v = 18 + v % 2 * 22;  // no degree that a row-class defect of `step` touches
    g_stage_mat[0] = build_mat("stage", d, 0, false);
    g_stage_mat[1] = build_mat("stage_diag", d, 0, true);
    const double coefA = 0.0625, coefB = 0.015625;
    struct T {
        int j, P;
        double mu;
    };
    const T targets[] = {{2, 16, 0.0}, {3, 16, 1.0}, {4, 4, -2.0}, {5, 1, 0.0}};
    for (const T& t : targets) {
        const Mat& A = g_stage_mat[t.mu != 0.0];
        Scenario best;
        bool have = false, have_eq = false;
        for (int seed = 0; seed < 200 && !have_eq; ++seed) {
            const dvec b0 = block((size_t)kStageN * t.P, EXACT);
            const StageData S = simulate(A, t.P, t.mu, coefA, kStageM, b0, b0, 1.0L);
            if (!S.in_range || S.nf[t.j] == 0.0) continue;
            bool eq;
            const double hi = tol_hi_of(S, t.j, &eq), lo = nextafter(hi, 0.0);
            if (stop_term(S, hi) != t.j) continue;  // an earlier term would stop first
            const int sl = stop_term(S, lo);
            if (sl != 0 && sl <= t.j) continue;
            if (have && !eq) continue;
            best = Scenario();
            best.name = fmt("stop%d", t.j);
            best.P = t.P;
            best.mu = t.mu;
            best.b0 = b0;
            best.A = S;
            best.tolA = hi;
            have = true;
            have_eq = eq;
        }
        if (!have) continue;
        g_cov_stop[std::min(t.j, 4) - 2] = true;
        g_cov_equal = g_cov_equal || have_eq;
        Scenario hi = best, lo = best;
        hi.name += have_eq ? "_sharp_hi_equal" : "_sharp_hi";
        lo.name += "_sharp_lo";
        lo.tolA = nextafter(best.tolA, 0.0);
        g_scen.push_back(hi);
        g_scen.push_back(lo);
    }
    {  // no stop: tol = 0
        Scenario s;
        s.name = "no_stop";
        s.P = 32;
        s.b0 = block((size_t)kStageN * s.P, EXACT);
        s.A = simulate(g_stage_mat[0], s.P, 0.0, coefA, kStageM, s.b0, s.b0, 1.0L);
        s.tolA = 0.0;
        g_cov_range = g_cov_range && s.A.in_range;
        g_cov_nostop = stop_term(s.A, 0.0) == 0;
        g_scen.push_back(s);
    }
    for (int seed = 0; seed < 200 && !g_cov_two; ++seed) {  // two stages on one state block
        Scenario s;
        s.name = "two_stages";
        s.P = 16;
        s.two = true;
        s.b0 = block((size_t)kStageN * s.P, EXACT);
        s.A = simulate(g_stage_mat[0], s.P, 0.0, coefA, kStageM, s.b0, s.b0, 1.0L);
        if (!s.A.in_range) continue;
        bool eq;
        s.tolA = tol_hi_of(s.A, 2, &eq);
        if (stop_term(s.A, s.tolA) != 2) continue;
        // stage B starts from b = F of the stopped stage A (two terms applied)
        s.B = simulate(g_stage_mat[0], s.P, 0.0, coefB, kStageM, s.A.F[2], s.A.F[2], ldexpl(1.0L, -8));
        if (!s.B.in_range || s.B.nf[3] == 0.0) continue;
        s.tolB = tol_hi_of(s.B, 3, &eq);
        if (stop_term(s.B, s.tolB) != 3) continue;
        double bmax = 0;
        for (int k = 1; k <= kStageM; ++k) bmax = std::max(bmax, s.B.c[k]);
        if (!(std::min(s.A.c[1], s.A.c[2]) > bmax)) continue;  // A's term maxima exceed all of B's
        g_cov_two = true;
        g_scen.push_back(s);
    }
    g_build_always = false;
    g_rng = rng_saved;
    g_pos = pos_saved;
}

struct Snap {
    std::string at;
    ExpmvState st;
    dvec F, B0, B1;
    int hflag;
};
struct Expect {
    int active, mv, hflag;
    double c1, c1s[2];
    int kind[3];
    double mb[3], mf[3];
    dvec F, B[2];
};
static void check_snap(Case& c, const Snap& s, const Expect& e) {
    c.eqi(s.at + ": active", s.st.active, e.active);
    c.eqi(s.at + ": mv", s.st.mv, e.mv);
    c.eqi(s.at + ": host flag", s.hflag, e.hflag);
    c.same(s.at + ": c1", 0, s.st.c1, e.c1);
    for (int i = 0; i < 2; ++i) c.same(s.at + fmt(": c1s[%d]", i), i, s.st.c1s[i], e.c1s[i]);
    for (int t = 0; t < 3; ++t) check_set(c, s.at, s.st, t, e.kind[t], true, e.mb[t], e.mf[t], 0, 0);
    for (size_t t = 0; t < e.F.size(); ++t) {
        if (!(s.F[t] == e.F[t]) && !(bits_of(s.F[t]) == bits_of(e.F[t]))) c.fail(s.at + ": F", (long)t, s.F[t], e.F[t], 0.0, INFINITY);
        if (!(s.B0[t] == e.B[0][t]) && !(bits_of(s.B0[t]) == bits_of(e.B[0][t])))
            c.fail(s.at + ": b block 0", (long)t, s.B0[t], e.B[0][t], 0.0, INFINITY);
        if (!(s.B1[t] == e.B[1][t]) && !(bits_of(s.B1[t]) == bits_of(e.B[1][t])))
            c.fail(s.at + ": b block 1", (long)t, s.B1[t], e.B[1][t], 0.0, INFINITY);
    }
}

// returns the state and blocks after the stage's last launch (`first`: those of
// the first form run, which every other form must equal bit for bit -- by then
// each form has recorded its decision; the slot sets are left out, since the
// forms with a slot check zero the next set one launch later)
static Snap stage_case(const Scenario& sc, int form, const Snap* first) {
    const int P = sc.P, nc = P, ld = P + 4, n = kStageN, m = kStageM;
    Case c(G_STAGE, sc.name,
           fmt("form=%d P=%d n=%d m=%d mu=%g tolA=%.17g%s", form, P, n, m, sc.mu, sc.tolA, sc.two ? fmt(" tolB=%.17g", sc.tolB).c_str() : ""));
    const Mat& A = g_stage_mat[sc.mu != 0.0];
    const bool split = form == 1 || form == 2;
    const dvec F0 = make_block(n, nc, P, ld, &sc.b0, 0, 0, SENT);
    const dvec B0 = make_block(n, nc, P, ld, &sc.b0, 0, 0, NAN), B1 = make_block(n, nc, P, ld, nullptr, SENT, 0, SENT);
    const ExpmvState s0 = seeded_state(0, 41);
    auto widen = [&](const dvec& X, const dvec& like) {  // n x nc values into a copy of the block `like`
        dvec v = like;
        for (int r = 0; r < n; ++r)
            for (int q = 0; q < nc; ++q) v[(size_t)r * ld + q] = X[(size_t)r * nc + q];
        return v;
    };
    // what the device does
    auto exec = [&]() {
        std::vector<Snap> tr;
        g_work.off = 0;
        const DevMat D = upload_mat(A, true, 0);
        double *dF = up(F0), *dB[2] = {up(B0), up(B1)};
        double* dpart = up(dvec(2 * kt::inf_norm_blocks() + GUARD, SENT));
        ExpmvState* ds = up_state(s0);
        hflag_write(-1);
        auto snap = [&](const std::string& at) {
            tr.push_back(Snap{at, down_state(ds), down(dF, F0.size()), down(dB[0], B0.size()), down(dB[1], B1.size()),
                              hflag_read()});
        };
        for (int stage = 1; stage <= (sc.two ? 2 : 1); ++stage) {
            const StageData& S = stage == 1 ? sc.A : sc.B;
            const double tol = stage == 1 ? sc.tolA : sc.tolB;
            if (stage == 2) {  // b = F (expmv_device's copy_cols), test plumbing
                const dvec Fh = down(dF, F0.size());
                dvec nb = B0;
                for (int r = 0; r < n; ++r)
                    for (int q = 0; q < nc; ++q) nb[(size_t)r * ld + q] = Fh[(size_t)r * ld + q];
                put(dB[0], nb.data(), nb.size());
            }
            LAUNCH(op_inf_norm(n, nc, dB[0], ld, dpart));
            LAUNCH(op_begin(dpart, kt::inf_norm_blocks(), ds));
            snap(fmt("stage %d begin", stage));
            int cur = 0;
            for (int k = 1; k <= m; ++k) {
                LAUNCH(op_step(P, true, D, nc, ld, S.mu, S.coef, tol, k, dB[cur], dB[1 - cur], dF, ds, form, g_hflag_dev,
                               stage));
                snap(fmt("stage %d term %d", stage, k));
                if (split && k < m) {
                    LAUNCH(op_slot_check(ds, k, tol, g_hflag_dev, stage));
                    snap(fmt("stage %d slot check %d", stage, k));
                }
                cur = 1 - cur;
            }
        }
        return tr;
    };
    std::vector<Snap> tr = exec();
    if (!g_host) {
        const std::vector<Snap> tr2 = exec();
        for (size_t i = 0; i < tr.size(); ++i) {
            c.repeat({state_words(tr[i].st), tr[i].F, tr[i].B0, tr[i].B1}, {state_words(tr2[i].st), tr2[i].F, tr2[i].B0, tr2[i].B1});
            c.eqi(tr[i].at + ": second run's host flag", tr2[i].hflag, tr[i].hflag);
        }
    }
    // what expmv.m:71-92 does
    Expect e;
    e.active = s0.active;
    e.mv = s0.mv;
    e.hflag = -1;
    e.c1 = s0.c1;
    e.c1s[0] = s0.c1s[0];
    e.c1s[1] = s0.c1s[1];
    for (int t = 0; t < 3; ++t) e.kind[t] = SET_SEEDED, e.mb[t] = e.mf[t] = 0;
    e.F = F0;
    e.B[0] = B0;
    e.B[1] = B1;
    size_t at = 0;
    auto next = [&]() {
        if (at < tr.size()) check_snap(c, tr[at], e);
        ++at;
    };
    for (int stage = 1; stage <= (sc.two ? 2 : 1); ++stage) {
        const StageData& S = stage == 1 ? sc.A : sc.B;
        const double tol = stage == 1 ? sc.tolA : sc.tolB;
        const int stop = stop_term(S, tol);
        if (!S.in_range) c.fail("exact range", stage, 0.0, 0.0, 0.0, INFINITY);
        if (stage == 2) e.B[0] = widen(S.b[0], B0);
        e.active = 1;
        e.c1 = e.c1s[1] = S.c[0];
        e.kind[1] = SET_ZERO;
        next();
        int cur = 0;
        auto term = [&](int k) {
            e.mv += 1;
            if (e.kind[k % 3] != SET_ZERO) c.fail("reference: term folds into a set that is not zero", k, 0.0, 0.0, 0.0, INFINITY);
            e.kind[k % 3] = SET_MAX;
            e.mb[k % 3] = S.c[k];
            e.mf[k % 3] = S.nf[k];
            e.B[1 - cur] = widen(S.b[k], e.B[1 - cur]);
            e.F = widen(S.F[k], e.F);
        };
        auto decide = [&](int j) {  // the check of term j, recorded by the launch that makes it
            if (j == stop) {
                e.active = 0;
                e.hflag = stage;
            } else {
                e.c1s[(j + 1) & 1] = S.c[j];
            }
        };
        for (int k = 1; k <= m; ++k) {
            if (split) {
                if (e.active) term(k);
                next();
                if (k < m) {
                    e.kind[(k + 1) % 3] = SET_ZERO;
                    if (e.active) decide(k);
                    next();
                }
            } else {
                if (e.active && k > 1) decide(k - 1);
                if (e.active) {
                    e.kind[(k + 1) % 3] = SET_ZERO;
                    term(k);
                }
                next();
            }
            cur = 1 - cur;
        }
    }
    if (at != tr.size()) c.fail("number of launches", 0, (double)tr.size(), (double)at, 0.0, INFINITY);
    const Snap& last = tr.back();
    if (first) {
        c.unchanged("F differs between forms", first->F, last.F);
        c.unchanged("b block 0 differs between forms", first->B0, last.B0);
        c.unchanged("b block 1 differs between forms", first->B1, last.B1);
        c.eqi("active differs between forms", last.st.active, first->st.active);
        c.eqi("mv differs between forms", last.st.mv, first->st.mv);
        c.eqi("host flag differs between forms", last.hflag, first->hflag);
        c.same("c1 differs between forms", 0, last.st.c1, first->st.c1);
        for (int i = 0; i < 2; ++i) c.same("c1s differs between forms", i, last.st.c1s[i], first->st.c1s[i]);
    }
    return last;
}

static void grp_stage() {
    // the scenario list is the reference's alone; --count needs it too (the
    // simulation is host arithmetic, nothing is launched)
    build_scenarios();
    {
        Case c(G_STAGE, "coverage", "the reference's scenarios");
        if (!g_cov_stop[0]) c.fail("no stage stops at term 2", 0, 0, 0, 0, INFINITY);
        if (!g_cov_stop[1]) c.fail("no stage stops at term 3", 0, 0, 0, 0, INFINITY);
        if (!g_cov_stop[2]) c.fail("no stage stops at a term >= 4", 0, 0, 0, 0, INFINITY);
        if (!g_cov_equal) c.fail("no sharp pair with fl(tol_hi nf) == c1 + c2", 0, 0, 0, 0, INFINITY);
        if (!g_cov_nostop || !g_cov_range) c.fail("no stage runs to m", 0, 0, 0, 0, INFINITY);
        if (!g_cov_two) c.fail("no two-stage run", 0, 0, 0, 0, INFINITY);
    }
    for (const Scenario& sc : g_scen) {
        Snap first;
        for (int form = 0; form < 4; ++form) {
            if (g_list) {
                Case c(G_STAGE, sc.name, fmt("form=%d", form));
                continue;
            }
            const Snap last = stage_case(sc, form, form ? &first : nullptr);
            if (form == 0) first = last;
        }
    }
}

// ---------------------------------------------------------------------------
// group setup: launch_sweep_scales, launch_gram_diag, launch_fill, launch_pair_start
// ---------------------------------------------------------------------------
static void scales_case(int mode, int P, int nc, int kind) {
    Case c(G_SETUP, kind_name(kind), fmt("sweep_scales mode=%d P=%d nc=%d", mode, P, nc));
    if (g_list) return;
    const bool ex = kind == EXACT;
    dvec n2(nc);
    for (int q = 0; q < nc; ++q) {
        const double v = ex ? ldexp(1.0, 2 * (int)(rnd() % 7) - 6) : fabs(rnormal()) + 0.01;  // exact: powers of 4
        n2[q] = q % 5 == 1 ? 0.0 : q % 5 == 2 ? -v : q % 5 == 3 ? NAN : v;
    }
    n2.resize(nc + GUARD, 1e300);  // not read past nc
    const size_t na = mode ? 9 * P : P;
    const dvec a0(na + GUARD, SENT), b0(P + GUARD, SENT);
    auto exec = [&]() {
        g_work.off = 0;
        double *dn = up(n2), *da = up(a0), *db = up(b0);
        LAUNCH(op_sweep_scales(dn, nc, P, mode, da, db));
        return std::vector<dvec>{down(da, a0.size()), down(db, b0.size())};
    };
    std::vector<dvec> o = exec();
    if (!g_host) c.repeat(o, exec());
    for (size_t t = 0; t < na; ++t) {
        const int q = (int)(t % P), slab = (int)(t / P);
        const double v = q < nc ? n2[q] : 0.0;
        const bool pos = v > 0.0;
        if (slab == 0) {
            const ld_t ref = pos ? 1.0L / sqrtl((ld_t)v) : 0.0L;
            if (pos) c.value(ex, "scale", (long)t, o[0][t], ref, gam(5) * ref);
            else c.same("scale of a non-positive norm", (long)t, o[0][t], 0.0);
        } else {
            c.same("coefficient block", (long)t, o[0][t], slab == 6 ? 1.0 : 0.0);
        }
        if (mode == 0) c.same("squared norm", (long)t, o[1][t], pos ? v : 0.0);
    }
    for (size_t t = na; t < a0.size(); ++t) c.same("guard", (long)t, o[0][t], SENT);
    for (size_t t = mode ? 0 : P; t < b0.size(); ++t) c.same("second output guard", (long)t, o[1][t], SENT);
}
static void gram_diag_case(int nc) {
    const int ld = nc + 3;
    Case c(G_SETUP, "exact", fmt("gram_diag nc=%d ld=%d", nc, ld));
    if (g_list) return;
    const dvec G = block((size_t)nc * ld, NORMAL), n0(nc + GUARD, SENT);
    auto exec = [&]() {
        g_work.off = 0;
        double *dG = up(G), *dn = up(n0);
        LAUNCH(op_gram_diag(dG, ld, nc, dn));
        return std::vector<dvec>{down(dn, n0.size())};
    };
    std::vector<dvec> o = exec();
    if (!g_host) c.repeat(o, exec());
    for (int q = 0; q < nc; ++q) c.same("diagonal", q, o[0][q], G[q + (size_t)q * ld]);
    for (size_t t = nc; t < n0.size(); ++t) c.same("guard", (long)t, o[0][t], SENT);
}
static void fill_case(int count) {
    Case c(G_SETUP, "exact", fmt("fill count=%d", count));
    if (g_list) return;
    const dvec x0(count + GUARD, SENT);
    const double v = -3.25;
    auto exec = [&]() {
        g_work.off = 0;
        double* dx = up(x0);
        LAUNCH(op_fill(dx, count, v));
        return std::vector<dvec>{down(dx, x0.size())};
    };
    std::vector<dvec> o = exec();
    if (!g_host) c.repeat(o, exec());
    for (int t = 0; t < count; ++t) c.same("value", t, o[0][t], v);
    for (size_t t = count; t < x0.size(); ++t) c.same("guard", (long)t, o[0][t], SENT);
}
// what: 0 distinct pairs, 1 with repeated pairs, 2 with out-of-range rows and i == j
static void pair_start_case(int n, int P, int np, int what, bool refused) {
    Case c(G_SETUP, refused ? "refused" : "exact",
           fmt("pair_start n=%d P=%d np=%d %s", n, P, np, what == 0 ? "distinct" : what == 1 ? "repeated" : "out_of_range"));
    if (g_list) return;
    const int nn = std::max(n, 2), PP = std::max(P, 2);
    ivec pos(2 * std::max(np, 0));
    for (int p = 0; p < np; ++p) {
        int i = (int)(rnd() % nn), j = (int)(rnd() % nn);
        if (i == j) j = (i + 1) % nn;
        if (what == 1 && p > 0 && p % 2) i = pos[2 * p - 2], j = pos[2 * p - 1];
        if (what == 2) {
            if (p % 4 == 0) i = -1;
            if (p % 4 == 1) j = nn + p;
            if (p % 4 == 2) j = i;
            if (p % 4 == 3 && p % 8 == 3) i = nn;
        }
        pos[2 * p] = i;
        pos[2 * p + 1] = j;
    }
    pos.resize(pos.size() + 8, 0);  // a benign tail (not read past 2 np)
    const dvec X0((size_t)nn * PP + GUARD, 0.0), s0(PP + GUARD, SENT);
    hipError_t err = hipSuccess;
    auto exec = [&]() {
        g_work.off = 0;
        int* dpos = up(pos);
        double *dX = up(X0), *dsc = up(s0), *dk = up(s0);
        err = op_pair_start(n, P, np, dpos, dX, dsc, dk);
        if (err == hipErrorInvalidValue) {
            if (!g_host) (void)hipGetLastError();
        } else {
            HC(err);
        }
        if (!g_host) HC(hipDeviceSynchronize());
        return std::vector<dvec>{down(dX, X0.size()), down(dsc, s0.size()), down(dk, s0.size())};
    };
    std::vector<dvec> o = exec();
    if (!g_host) c.repeat(o, exec());
    if (refused) {
        if (err != hipErrorInvalidValue) c.fail("return code", 0, (double)err, (double)hipErrorInvalidValue, 0.0, INFINITY);
        c.unchanged("X touched", X0, o[0]);
        c.unchanged("sc touched", s0, o[1]);
        c.unchanged("k2s touched", s0, o[2]);
        return;
    }
    dvec X = X0, sc = s0, k2 = s0;
    for (int q = 0; q < P; ++q) {
        const int p = q / 2, i = p < np ? pos[2 * p] : -1, j = p < np ? pos[2 * p + 1] : -1;
        const bool ok = i >= 0 && i < n && j >= 0 && j < n && i != j;
        if (ok) {
            X[(size_t)i * P + q] = 1.0;
            X[(size_t)j * P + q] = (q & 1) ? -1.0 : 1.0;
        }
        sc[q] = ok ? 0.70710678118654752440 : 0.0;
        k2[q] = ok ? 2.0 : 0.0;
    }
    c.unchanged("X", X, o[0]);
    c.unchanged("sc", sc, o[1]);
    c.unchanged("k2s", k2, o[2]);
}
static void grp_setup() {
    for (int mode = 0; mode < 2; ++mode)
        for (int P : {1, 16, 64, 128}) {
            ivec ncs = {0, 1, P - 1, P};
            std::sort(ncs.begin(), ncs.end());
            ncs.erase(std::unique(ncs.begin(), ncs.end()), ncs.end());
            for (int nc : ncs) scales_case(mode, P, nc, (nc + mode) % 2 ? NORMAL : EXACT);
            scales_case(mode, P, P, P % 2 ? NORMAL : EXACT);
            if (P > 1) scales_case(mode, P, P, NORMAL);
        }
    for (int nc : {1, 63, 64, 65, 128}) gram_diag_case(nc);
    for (int count : {1, 255, 256, 257, 100001}) fill_case(count);
    for (int P : {2, 4, 6, 16, 62, 64}) {
        ivec nps = {0, 1, P / 2 - 1, P / 2};
        std::sort(nps.begin(), nps.end());
        nps.erase(std::unique(nps.begin(), nps.end()), nps.end());
        for (int np : nps) {
            if (np < 0) continue;
            pair_start_case(50, P, np, 0, false);
            if (np >= 2) pair_start_case(50, P, np, 1, false);
            if (np >= 1) pair_start_case(P == 2 ? 2 : 50, P, np, 2, false);
        }
    }
    pair_start_case(1, 4, 1, 0, true);
    pair_start_case(50, 5, 2, 0, true);
    pair_start_case(50, 4, 3, 0, true);
    pair_start_case(50, 66, 2, 0, true);
}

// ---------------------------------------------------------------------------
static const char* kMutations[] = {"short_skip_deg16",   "med_skip_deg17",         "long_drop_last_chain_entry",
                                   "heavy_row_twice",    "mu_ignored_long",        "weights_ignored",
                                   "pad_written_rows",   "f_pad_written",          "stop_strict_less",
                                   "c1_wrong_parity",    "stale_slot_set",         "mv_counts_stopped_term",
                                   "stopped_term_writes", "hflag_before_stop",     "begin_keeps_set1",
                                   "scales_nan_as_positive", "pair_start_same_sign"};

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
                fprintf(stderr, "expmv_check: unknown group %s\n", argv[a] + 8);
                return 2;
            }
        } else {
            fprintf(stderr, "usage: expmv_check [--host [--mutate=NAME]] [--count] [--group=NAME] [--small]\n");
            return 2;
        }
    }
    if (!g_mut.empty()) {
        bool known = false;
        for (const char* m : kMutations) known = known || g_mut == m;
        if (!known || !g_host || g_list) {
            fprintf(stderr, "expmv_check: --mutate needs --host and one of:");
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
    pools_init();
    if (!g_list) {
        g_work.init((size_t)768 << 20);
        hflag_init();
    }
    void (*const groups[NG])() = {grp_begin, grp_unfused, grp_step, grp_stage, grp_setup};
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
