// sweep_check -- the sparse sweep passes of kt_kernels.hip called one by one
// through their kt::launch_* entry points (kt_launch.h), at all eight widths
// P = 1 .. 128 and in every flag form a launcher can select, each result
// compared with a host reference in long double (or in exact integers).
//
// Groups: probes, spmm_dot, spmm_block, lanczos_pass, lanczos_start,
// lanczos_first, quadform, coef, update, contract.
// Three kinds of assertion (as block_check):
//   exact    small-integer inputs (X, Yold: |v| <= 8; int16 tables in [-5, 5];
//            weights 1 or integers 1..4 that differ by position; g, a, b and
//            the scales in {0, +-1/2, +-1, +-2}): every product, row sum,
//            output and dot is exact in fp64 in any order, with or without
//            fma (check_exact_range() verifies the magnitudes), so the result
//            must equal the reference.
//   bounded  standard-normal inputs against a componentwise a-priori bound,
//            u = 2^-53, gamma_k = k u / (1 - k u): a row sum of d terms
//            gamma_d sum|a||x|; the epilogue three more roundings; a dot over
//            n rows gamma_(n + d + 4) times the sum of absolute products
//            (Out.Out, whose two factors both carry the row error:
//            gamma_(n + 2 d + 8)).  Nothing is tuned to the kernels; each
//            group reports max_ratio, the largest error / bound it saw.
//   contract bit-for-bit statements the source makes (group contract, device
//            only; with --host they are counted and trivially true).
// Output blocks and partial arrays are pre-filled with a sentinel and carry a
// guard region after the last element: no sentinel may remain inside the
// documented extent, and guard and padding must come back unchanged.  Input
// blocks with a leading dimension carry NaN padding.  On the device every
// case runs twice and the two outputs must agree bit for bit.
//
// Graphs (built here, symmetric pattern and weights, columns ascending):
//   A  n = 1103: short degrees 0 (the last row, a run of empty rows), 1, 3, 4,
//      5, 7, 8, 9, 16, 17, 33, 40, 50, 64; 24 long rows of 65 .. 80, 96, 97,
//      255, 256, 257, 320; diagonal entries first / in the middle / last in
//      their rows.  Launched with (spmm_grid(n, P, 1024) short blocks,
//      long_blocks_for(n_long, 512)) and with (3 short blocks, 1 long block).
//   B  n = 307 (less than one workgroup's rows at P = 1), no row above 64:
//      n_long = 0, launched with long_blocks = 0.
// long_rows: exactly the rows longer than long_thresh, heaviest first; lower:
// the index of the row's first entry with column >= r, complemented where it
// is the diagonal; chunk table: rows longer than split_thresh, heaviest first,
// in pieces of kChunkNnz (kt_runtime.cpp).  spmm_block also runs graph A with
// long_thresh = 32 < split_thresh = 64 (long-wave rows of 33 .. 64 beside the
// chunked ones).
//
// Launcher forms enumerated (flags argument -> template reached); --count
// prints the same table under "forms":
//   launch_spmm_dot            0, UNIT, NT, NT|UNIT, NTY|UNIT, NT|NTY|UNIT, MLP,
//                              MLP|UNIT, MLP|NTY|UNIT -> k_spmm_dot<that>;
//                              NT|MLP|UNIT (unsupported) -> k_spmm_dot<UNIT>
//   launch_spmm_block          0, UNIT, MLP, UNIT|MLP -> k_spmm_block<that>
//                              (+ k_spmm_combine with a chunk table)
//   launch_spmm_lanczos        0, UNIT, NTY, UNIT|NTY, SC1, UNIT|SC1 -> <that>;
//                              I16, I16|NTY, I16|SC1 -> <UNIT|I16[|NTY|SC1]>;
//                              Vn set: 0, UNIT, SC1, UNIT|SC1 -> <that|VB>;
//                              gate set: 0 -> <NTY|GATE>, UNIT -> <UNIT|NTY|GATE>,
//                              I16 -> <UNIT|I16|NTY|GATE>            (16 forms)
//   launch_spmm_lanczos_start  0, UNIT, NTY, UNIT|NTY, SC1, UNIT|SC1 -> <that>;
//                              I16 -> <UNIT|I16>
//   launch_spmm_lanczos_first  UNIT, UNIT|NTY, UNIT|SC1 -> <that>; gate set ->
//                              <UNIT|NTY|GATE>
//   launch_spmm_quadform       0, UNIT -> <that>; Vn set: 0, UNIT -> <that|VB>
// and, without a flags argument: launch_update (nt false / true), launch_ycoef
// (gate null -> k_ycoef<P>; gate set -> k_ycoef<P, true>, group contract),
// launch_coef_cgs2, launch_norm, launch_rademacher(_cols, _signs).
// Not covered on purpose: the expmv term kernels and the diag / entries
// kernels (kt_diag.hip).
//
//   sweep_check                     run on the GPU
//   sweep_check --host              the same cases with every device call
//                                   replaced by a plain fp64 host loop written
//                                   from the launchers' contract (no GPU)
//   sweep_check --host --mutate=M   one deliberate defect in that stand-in;
//                                   the matching group must report failures
//   sweep_check --count             the case counts and the form table alone
//   --group=NAME runs one group; --small keeps the widths 1, 4 and 32 only
//   (both for quick --mutate runs)
//
// Prints one JSON line; exit status 0 iff no case failed, 1 on failures, 3 on
// a HIP error (nothing is launched after it), 2 on bad usage.
// Build: make -C tests/native/sweep_check (links the library's own kt_kernels.o).
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
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../../krylov_robustness_amd/csrc/kt_launch.h"

typedef long double ld_t;
typedef std::vector<double> dvec;
typedef std::vector<int> ivec;

// the launchers' `flags` argument bits (kt_kernels.hip)
enum : int { F_NT = 1, F_UNIT = 2, F_MLP = 4, F_NTY = 8, F_SC1 = 16, F_I16 = 128 };

static bool g_host = false;
static bool g_list = false;  // --count: enumerate the cases, run nothing
static bool g_small = false; // --small: widths 1, 4 and 32 only (quick --mutate runs)
static int g_only = -1;      // --group=NAME: that group alone
static std::string g_mut;
static bool mut(const char* s) { return g_mut == s; }

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
enum { G_PROBES, G_DOT, G_BLOCK, G_PASS, G_START, G_FIRST, G_QUAD, G_COEF, G_UPDATE, G_CONTRACT, NG };
static Group g_groups[NG] = {{"probes"},        {"spmm_dot"}, {"spmm_block"}, {"lanczos_pass"}, {"lanczos_start"},
                             {"lanczos_first"}, {"quadform"}, {"coef"},       {"update"},       {"contract"}};
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
    const char* name;
    int flags;
    int mode;  // 0 plain, 1 Vn set (basis-forming), 2 gate set
    const char* reaches;
};
static const Form kForms[] = {
    {"spmm_dot", "0", 0, 0, "k_spmm_dot<0>"},
    {"spmm_dot", "UNIT", F_UNIT, 0, "k_spmm_dot<UNIT>"},
    {"spmm_dot", "NT", F_NT, 0, "k_spmm_dot<NT>"},
    {"spmm_dot", "NT|UNIT", F_NT | F_UNIT, 0, "k_spmm_dot<NT|UNIT>"},
    {"spmm_dot", "NTY|UNIT", F_NTY | F_UNIT, 0, "k_spmm_dot<NTY|UNIT>"},
    {"spmm_dot", "NT|NTY|UNIT", F_NT | F_NTY | F_UNIT, 0, "k_spmm_dot<NT|NTY|UNIT>"},
    {"spmm_dot", "MLP", F_MLP, 0, "k_spmm_dot<MLP>"},
    {"spmm_dot", "MLP|UNIT", F_MLP | F_UNIT, 0, "k_spmm_dot<MLP|UNIT>"},
    {"spmm_dot", "MLP|NTY|UNIT", F_MLP | F_NTY | F_UNIT, 0, "k_spmm_dot<MLP|NTY|UNIT>"},
    {"spmm_dot", "NT|MLP|UNIT(fallback)", F_NT | F_MLP | F_UNIT, 0, "k_spmm_dot<UNIT>"},
    {"spmm_block", "0", 0, 0, "k_spmm_block<0>"},
    {"spmm_block", "UNIT", F_UNIT, 0, "k_spmm_block<UNIT>"},
    {"spmm_block", "MLP", F_MLP, 0, "k_spmm_block<MLP>"},
    {"spmm_block", "UNIT|MLP", F_UNIT | F_MLP, 0, "k_spmm_block<UNIT|MLP>"},
    {"lanczos_pass", "0", 0, 0, "k_spmm_lanczos<0>"},
    {"lanczos_pass", "UNIT", F_UNIT, 0, "k_spmm_lanczos<UNIT>"},
    {"lanczos_pass", "NTY", F_NTY, 0, "k_spmm_lanczos<NTY>"},
    {"lanczos_pass", "UNIT|NTY", F_UNIT | F_NTY, 0, "k_spmm_lanczos<UNIT|NTY>"},
    {"lanczos_pass", "SC1", F_SC1, 0, "k_spmm_lanczos<SC1>"},
    {"lanczos_pass", "UNIT|SC1", F_UNIT | F_SC1, 0, "k_spmm_lanczos<UNIT|SC1>"},
    {"lanczos_pass", "I16", F_UNIT | F_I16, 0, "k_spmm_lanczos<UNIT|I16>"},
    {"lanczos_pass", "I16|NTY", F_UNIT | F_I16 | F_NTY, 0, "k_spmm_lanczos<UNIT|I16|NTY>"},
    {"lanczos_pass", "I16|SC1", F_UNIT | F_I16 | F_SC1, 0, "k_spmm_lanczos<UNIT|I16|SC1>"},
    {"lanczos_pass", "Vn:0", 0, 1, "k_spmm_lanczos<VB>"},
    {"lanczos_pass", "Vn:UNIT", F_UNIT, 1, "k_spmm_lanczos<UNIT|VB>"},
    {"lanczos_pass", "Vn:SC1", F_SC1, 1, "k_spmm_lanczos<SC1|VB>"},
    {"lanczos_pass", "Vn:UNIT|SC1", F_UNIT | F_SC1, 1, "k_spmm_lanczos<UNIT|SC1|VB>"},
    {"lanczos_pass", "gate:0", 0, 2, "k_spmm_lanczos<NTY|GATE>"},
    {"lanczos_pass", "gate:UNIT", F_UNIT, 2, "k_spmm_lanczos<UNIT|NTY|GATE>"},
    {"lanczos_pass", "gate:I16", F_UNIT | F_I16, 2, "k_spmm_lanczos<UNIT|I16|NTY|GATE>"},
    {"lanczos_start", "0", 0, 0, "k_spmm_lanczos_start<0>"},
    {"lanczos_start", "UNIT", F_UNIT, 0, "k_spmm_lanczos_start<UNIT>"},
    {"lanczos_start", "NTY", F_NTY, 0, "k_spmm_lanczos_start<NTY>"},
    {"lanczos_start", "UNIT|NTY", F_UNIT | F_NTY, 0, "k_spmm_lanczos_start<UNIT|NTY>"},
    {"lanczos_start", "SC1", F_SC1, 0, "k_spmm_lanczos_start<SC1>"},
    {"lanczos_start", "UNIT|SC1", F_UNIT | F_SC1, 0, "k_spmm_lanczos_start<UNIT|SC1>"},
    {"lanczos_start", "I16", F_UNIT | F_I16, 0, "k_spmm_lanczos_start<UNIT|I16>"},
    {"lanczos_first", "UNIT", F_UNIT, 0, "k_spmm_lanczos_first<UNIT>"},
    {"lanczos_first", "UNIT|NTY", F_UNIT | F_NTY, 0, "k_spmm_lanczos_first<UNIT|NTY>"},
    {"lanczos_first", "UNIT|SC1", F_UNIT | F_SC1, 0, "k_spmm_lanczos_first<UNIT|SC1>"},
    {"lanczos_first", "gate:UNIT", F_UNIT, 2, "k_spmm_lanczos_first<UNIT|NTY|GATE>"},
    {"quadform", "0", 0, 0, "k_spmm_quadform<0>"},
    {"quadform", "UNIT", F_UNIT, 0, "k_spmm_quadform<UNIT>"},
    {"quadform", "Vn:0", 0, 1, "k_spmm_quadform<VB>"},
    {"quadform", "Vn:UNIT", F_UNIT, 1, "k_spmm_quadform<UNIT|VB>"},
};
static std::vector<const Form*> forms_of(const char* launcher) {
    std::vector<const Form*> v;
    for (const Form& f : kForms)
        if (!strcmp(f.launcher, launcher)) v.push_back(&f);
    return v;
}

static void print_report(const char* hip_err) {
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - g_t0).count();
    long nfail = 0;
    for (int g = 0; g < NG; ++g) nfail += g_groups[g].nfail;
    printf("{\"sweep_check\": \"%s\", \"mode\": \"%s\", \"mutate\": \"%s\", \"wall_s\": %.3f, ",
           hip_err ? "HIP_ERROR" : (nfail ? "FAIL" : "ok"), g_list ? "count" : (g_host ? "host" : "device"),
           g_mut.c_str(), wall);
    if (hip_err) printf("\"hip_error\": \"%s\", ", hip_err);
    if (g_list) {
        printf("\"forms\": {");
        const char* last = "";
        for (const Form& f : kForms) {
            if (strcmp(last, f.launcher)) printf("%s\"%s\": [", *last ? "], " : "", f.launcher);
            else printf(", ");
            printf("{\"form\": \"%s\", \"flags\": %d, \"reaches\": \"%s\"}", f.name, f.flags, f.reaches);
            last = f.launcher;
        }
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
    fprintf(stderr, "sweep_check: test setup: %s\n", msg.c_str());
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
    // exact (integer inputs) or bounded (normal inputs)
    void value(bool ex, const char* what, long idx, ld_t got, ld_t ref, ld_t bound) {
        if (ex) exact(what, idx, (double)got, (double)ref);
        else bounded(what, idx, got, ref, bound);
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
// memory: two arenas (device memory, or host memory with --host): `keep` for
// the graphs and the input blocks (uploaded once), `work` as a per-case stack
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
static Arena g_keep, g_work;
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
template <class T>
static dvec to_d(const std::vector<T>& v) {
    return dvec(v.begin(), v.end());
}

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
static double rint8() { return (double)((int)(rnd() % 17) - 8); }
static double rnormal() {
    const double u1 = ((rnd() >> 11) + 1.0) * (1.0 / 9007199254740993.0);
    const double u2 = (rnd() >> 11) * (1.0 / 9007199254740992.0);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
enum Kind { INT8 = 0, NORMAL = 1 };
static const char* kind_name(int kind) { return kind == INT8 ? "exact" : "bounded"; }
static dvec block(size_t count, int kind) {
    dvec v(count);
    for (double& x : v) x = kind == INT8 ? rint8() : rnormal();
    return v;
}
static dvec sentinels(size_t count) { return dvec(count + GUARD, SENT); }

// splitmix64 and the probe sign of k_rademacher's comment: X[r, p] = -1 where
// the top bit of splitmix64(key(seed, probe) + i) is set, key = splitmix64(
// splitmix64(seed) + probe), i the original row index
static uint64_t sm64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static int probe_neg(uint64_t seed, int64_t probe, uint64_t i) {
    return (int)(sm64(sm64(sm64(seed) + (uint64_t)probe) + i) >> 63);
}
static const uint64_t kSeed = 20240607ull;
static const int64_t kProbeBase = 1000003;

// ---------------------------------------------------------------------------
// graphs
// ---------------------------------------------------------------------------
struct Tabs {  // long-row list and chunk table for one (long_thresh, split_thresh)
    int lt = 0, st = 0, dmax = 0;
    ivec lr, ckb, cke, spr, spf;
    const int *d_lr = nullptr, *d_ckb = nullptr, *d_cke = nullptr, *d_spr = nullptr, *d_spf = nullptr;
    int n_long() const { return (int)lr.size(); }
    int n_chunks() const { return (int)ckb.size(); }
    int n_split() const { return (int)spr.size(); }
};
struct Graph {
    const char* name;
    int n = 0, dmax = 0;
    ivec rp, ci, lower;
    dvec va;
    const int *d_rp = nullptr, *d_ci = nullptr, *d_lower = nullptr;
    const double* d_va = nullptr;
    Tabs t64, t32;
    int deg(int r) const { return rp[r + 1] - rp[r]; }
};

static void make_tabs(const Graph& G, int lt, int st, Tabs& T) {
    T.lt = lt;
    T.st = st;
    T.dmax = G.dmax;
    for (int r = 0; r < G.n; ++r)
        if (G.deg(r) > lt) T.lr.push_back(r);
    std::stable_sort(T.lr.begin(), T.lr.end(), [&](int a, int b) { return G.deg(a) > G.deg(b); });
    T.spf.assign(1, 0);
    for (int r : T.lr) {
        const int b = G.rp[r], e = G.rp[r + 1];
        if (e - b <= st) continue;
        T.spr.push_back(r);
        for (int k = b; k < e; k += kt::kChunkNnz) {
            T.ckb.push_back(k);
            T.cke.push_back(std::min(e, k + kt::kChunkNnz));
        }
        T.spf.push_back((int)T.ckb.size());
    }
    if (g_list) return;
    // never empty on the device side (a pointer into the arena either way)
    ivec lr = T.lr, ckb = T.ckb, cke = T.cke, spr = T.spr;
    for (ivec* v : {&lr, &ckb, &cke, &spr})
        if (v->empty()) v->push_back(0);
    T.d_lr = g_keep.up(lr);
    T.d_ckb = g_keep.up(ckb);
    T.d_cke = g_keep.up(cke);
    T.d_spr = g_keep.up(spr);
    T.d_spf = g_keep.up(T.spf);
}

// A symmetric graph with the stored row lengths len[r] (the diagonal entry of
// a row with diag[r] counts), by Havel-Hakimi on the off-diagonal degrees.
static void build_graph(Graph& G, const char* name, const ivec& len, std::vector<char> diag) {
    const int n = (int)len.size();
    G.name = name;
    G.n = n;
    ivec need(n);
    long total = 0;
    for (int r = 0; r < n; ++r) {
        if (len[r] == 0) diag[r] = 0;
        need[r] = len[r] - diag[r];
        total += need[r];
    }
    if (total & 1) {  // an even degree sum: move one filler row's diagonal
        for (int r = 0; r < n; ++r)
            if (len[r] == 2 || len[r] == 6) {
                diag[r] = !diag[r];
                need[r] = len[r] - diag[r];
                break;
            }
    }
    std::vector<ivec> adj(n);
    ivec tie(n);
    for (int r = 0; r < n; ++r) tie[r] = (int)(rnd() & 0xffff);
    std::vector<char> mark(n, 0);
    for (;;) {
        int r = -1;
        for (int q = 0; q < n; ++q)
            if (need[q] > 0 && (r < 0 || need[q] > need[r])) r = q;
        if (r < 0) break;
        for (int c : adj[r]) mark[c] = 1;
        ivec cand;
        for (int c = 0; c < n; ++c)
            if (c != r && need[c] > 0 && !mark[c]) cand.push_back(c);
        for (int c : adj[r]) mark[c] = 0;
        if ((int)cand.size() < need[r]) setup_die(fmt("graph %s: degree sequence not realised", name));
        std::sort(cand.begin(), cand.end(),
                  [&](int a, int b) { return need[a] != need[b] ? need[a] > need[b] : tie[a] < tie[b]; });
        for (int k = 0; k < need[r]; ++k) {
            adj[r].push_back(cand[k]);
            adj[cand[k]].push_back(r);
            need[cand[k]]--;
        }
        need[r] = 0;
    }
    G.rp.assign(n + 1, 0);
    for (int r = 0; r < n; ++r) {
        if (diag[r]) adj[r].push_back(r);
        std::sort(adj[r].begin(), adj[r].end());
        if ((int)adj[r].size() != len[r]) setup_die(fmt("graph %s: row %d has %d entries, wanted %d", name, r, (int)adj[r].size(), len[r]));
        G.rp[r + 1] = G.rp[r] + len[r];
        G.dmax = std::max(G.dmax, len[r]);
    }
    G.lower.resize(n);
    for (int r = 0; r < n; ++r) {
        for (int c : adj[r]) {
            G.ci.push_back(c);
            // symmetric integer weight 1..4 that varies along a row
            const uint64_t lo = std::min(r, c), hi = std::max(r, c);
            G.va.push_back(1.0 + (double)(sm64(lo * 65536 + hi) & 3));
        }
        const int* cb = G.ci.data() + G.rp[r];
        const int* ce = G.ci.data() + G.rp[r + 1];
        const int* it = std::lower_bound(cb, ce, r);
        const int k = (int)(it - G.ci.data());
        G.lower[r] = (it != ce && *it == r) ? ~k : k;
    }
    if (!g_list) {
        G.d_rp = g_keep.up(G.rp);
        G.d_ci = g_keep.up(G.ci);
        G.d_va = g_keep.up(G.va);
        G.d_lower = g_keep.up(G.lower);
    }
    make_tabs(G, 64, 64, G.t64);
    make_tabs(G, 32, 64, G.t32);
}

static void add(ivec& v, int deg, int count) {
    for (int k = 0; k < count; ++k) v.push_back(deg);
}

// the row lengths `want` at shuffled rows; the last row and rows [run0, run0 + run) empty
static void place(Graph& G, const char* name, int n, ivec want, int run0, int run, const ivec& fill) {
    ivec len(n, -1);
    len[n - 1] = 0;
    for (int r = run0; r < run0 + run; ++r) len[r] = 0;
    ivec rows;
    for (int r = 0; r < n; ++r)
        if (len[r] < 0) rows.push_back(r);
    for (size_t i = rows.size(); i > 1; --i) std::swap(rows[i - 1], rows[rnd() % i]);
    if (want.size() > rows.size()) setup_die("too many rows wanted");
    for (size_t i = 0; i < rows.size(); ++i) len[rows[i]] = i < want.size() ? want[i] : fill[i % fill.size()];
    std::vector<char> diag(n);
    for (int r = 0; r < n; ++r) diag[r] = (rnd() % 3) == 0;
    build_graph(G, name, len, diag);
}

static Graph g_A, g_B;

static bool has_deg(const Graph& G, int d) {
    for (int r = 0; r < G.n; ++r)
        if (G.deg(r) == d) return true;
    return false;
}

static void graphs_init() {
    ivec wa;
    add(wa, 65, 3);
    for (int d = 66; d <= 80; ++d) add(wa, d, 1);
    for (int d : {96, 97, 255, 256, 257, 320}) add(wa, d, 1);
    add(wa, 64, 4);
    for (int d : {50, 40, 33}) add(wa, d, 2);
    for (int d : {17, 16}) add(wa, d, 10);
    for (int d : {9, 8, 7}) add(wa, d, 20);
    for (int d : {5, 4}) add(wa, d, 30);
    for (int d : {3, 1}) add(wa, d, 40);
    add(wa, 0, 3);
    place(g_A, "A", 1103, wa, 500, 6, {2, 3, 4, 5, 6, 10, 12});
    ivec wb;
    add(wb, 64, 3);
    for (int d : {50, 40, 33}) add(wb, d, 1);
    for (int d : {17, 16}) add(wb, d, 5);
    for (int d : {9, 8, 7, 5, 4, 3, 1}) add(wb, d, 10);
    place(g_B, "B", 307, wb, 100, 3, {2, 3, 6});
    // what the cases rely on
    for (int d : {0, 1, 3, 4, 5, 7, 8, 9, 16, 17, 33, 64, 65, 96, 97, 255, 256, 257, 320})
        if (!has_deg(g_A, d)) setup_die(fmt("graph A lacks degree %d", d));
    for (int d : {0, 1, 3, 4, 5, 7, 8, 9, 16, 17, 64})
        if (!has_deg(g_B, d)) setup_die(fmt("graph B lacks degree %d", d));
    if (g_A.t64.n_long() < 20 || g_B.t64.n_long() != 0 || g_B.dmax != 64) setup_die("long-row counts");
    if (g_A.t32.n_long() <= g_A.t64.n_long() || g_A.t32.n_split() != g_A.t64.n_split()) setup_die("t32 tables");
    if (g_A.deg(g_A.n - 1) || g_A.deg(500) || g_A.deg(505) || g_B.deg(g_B.n - 1)) setup_die("empty rows");
    int first = 0, mid = 0, last = 0, long_diag = 0, long_nodiag = 0;
    for (int r = 0; r < g_A.n; ++r) {
        const int d = g_A.deg(r);
        if (g_A.lower[r] >= 0) {
            long_nodiag += d > 64;
            continue;
        }
        const int pos = ~g_A.lower[r] - g_A.rp[r];
        first += d > 1 && pos == 0;
        last += d > 1 && pos == d - 1;
        mid += pos > 0 && pos < d - 1;
        long_diag += d > 64;
    }
    if (!first || !mid || !last || !long_diag || !long_nodiag) setup_die("diagonal positions");
    // symmetric pattern and weights
    for (const Graph* G : {&g_A, &g_B})
        for (int r = 0; r < G->n; ++r)
            for (int k = G->rp[r]; k < G->rp[r + 1]; ++k) {
                const int c = G->ci[k];
                const int* cb = G->ci.data() + G->rp[c];
                const int* ce = G->ci.data() + G->rp[c + 1];
                const int* it = std::lower_bound(cb, ce, r);
                if (it == ce || *it != r || G->va[it - G->ci.data()] != G->va[k]) setup_die("graph not symmetric");
            }
    // the exact cases: every value is a multiple of 1/16 (products of halves)
    // below n outmax^2, outmax = 2 tmax + 32 with tmax = 4 * 8 * dmax
    const double tmax = 4.0 * 8.0 * g_A.dmax, outmax = 2.0 * tmax + 32.0;
    if (!(16.0 * g_A.n * outmax * outmax < 9007199254740992.0)) setup_die("exact cases leave the fp64 integer range");
}

// One launch shape of a graph: grid = short-row blocks + long-row blocks
struct Shape {
    const Graph* G;
    const Tabs* T;
    int grid, lb;
    const char* tag;
};
static std::vector<Shape> shapes_for(int P) {
    const int ga = kt::spmm_grid(g_A.n, P, 1024), la = kt::long_blocks_for(g_A.t64.n_long(), 512);
    return {{&g_A, &g_A.t64, ga + la, la, "A/full"},
            {&g_A, &g_A.t64, std::min(ga, 3) + 1, 1, "A/capped"},
            {&g_B, &g_B.t64, kt::spmm_grid(g_B.n, P, 1024), 0, "B"}};
}

// ---------------------------------------------------------------------------
// the input blocks of one (graph, P, kind), uploaded once
// ---------------------------------------------------------------------------
static const double kCoefG[7] = {1.0, -1.0, 0.5, 2.0, -0.5, -2.0, 0.0};
static const double kCoefA[7] = {0.5, -1.0, 0.0, 2.0, 1.0, -0.5, -2.0};
static const double kCoefB[7] = {1.0, -0.5, 2.0, 0.0, -1.0, 0.5, -2.0};
struct Inputs {
    int n, P, kind;
    double s0;
    dvec X, Yold, Vc, Vo, coef, sc, XT, Z;  // XT = s0 * (double)T, Z = the probes as +-1
    std::vector<int16_t> T;
    std::vector<uint32_t> S;
    const double *dX, *dYold, *dVc, *dVo, *dcoef, *dsc, *dXT;
    const int16_t* dT;
    const uint32_t* dS;
    const int* dgate;
};
static std::map<std::tuple<const Graph*, int, int>, Inputs> g_inputs;
static const Inputs& inputs(const Graph& G, int P, int kind) {
    const auto key = std::make_tuple(&G, P, kind);
    auto it = g_inputs.find(key);
    if (it != g_inputs.end()) return it->second;
    Inputs& I = g_inputs[key];
    const size_t np = (size_t)G.n * P;
    I.n = G.n;
    I.P = P;
    I.kind = kind;
    I.s0 = kind == INT8 ? 0.5 : 1.0 / sqrt((double)G.n);
    I.X = block(np, kind);
    I.Yold = block(np, kind);
    I.Vc = block(np, kind);
    I.Vo = block(np, kind);
    I.coef.resize(3 * P);
    I.sc.resize(P);
    for (int p = 0; p < P; ++p) {
        I.coef[p] = kind == INT8 ? kCoefG[p % 7] : rnormal();
        I.coef[P + p] = kind == INT8 ? kCoefA[p % 7] : rnormal();
        I.coef[2 * P + p] = kind == INT8 ? kCoefB[p % 7] : rnormal();
        I.sc[p] = kind == INT8 ? kCoefG[(p + 2) % 7] : rnormal();
    }
    I.T.resize(np);
    I.XT.resize(np);
    for (size_t t = 0; t < np; ++t) {
        I.T[t] = (int16_t)((int)(rnd() % 11) - 5);
        I.XT[t] = I.s0 * (double)I.T[t];
    }
    const int W = (P + 31) / 32;
    I.S.assign((size_t)G.n * W, 0u);
    I.Z.resize(np);
    for (int r = 0; r < G.n; ++r)
        for (int p = 0; p < P; ++p) {
            const int neg = probe_neg(kSeed, kProbeBase + p, (uint64_t)r);
            I.S[(size_t)r * W + p / 32] |= (uint32_t)neg << (p % 32);
            I.Z[(size_t)r * P + p] = neg ? -1.0 : 1.0;
        }
    I.dX = g_keep.up(I.X);
    I.dYold = g_keep.up(I.Yold);
    I.dVc = g_keep.up(I.Vc);
    I.dVo = g_keep.up(I.Vo);
    I.dcoef = g_keep.up(I.coef);
    I.dsc = g_keep.up(I.sc);
    I.dXT = g_keep.up(I.XT);
    I.dT = g_keep.up(I.T);
    I.dS = g_keep.up(I.S);
    I.dgate = g_keep.up(ivec{0, 1});  // two running words, one of them set: the gate is open
    return I;
}

// A X in long double, and sum |a||x| (per element), X with leading dimension ld
struct RefAX {
    std::vector<ld_t> t, ta;
};
static std::map<std::tuple<const Graph*, bool, const double*>, RefAX> g_refs;
static void refs_reset() { g_refs.clear(); }
static const RefAX& ref_ax(const Graph& G, bool unit, const dvec& X, int ld, int cols) {
    const auto key = std::make_tuple(&G, unit, X.data());
    auto it = g_refs.find(key);
    if (it != g_refs.end()) return it->second;
    RefAX& R = g_refs[key];
    R.t.assign((size_t)G.n * cols, 0.0L);
    R.ta.assign((size_t)G.n * cols, 0.0L);
    for (int r = 0; r < G.n; ++r)
        for (int k = G.rp[r]; k < G.rp[r + 1]; ++k) {
            const ld_t a = unit ? 1.0L : (ld_t)G.va[k];
            const double* x = X.data() + (size_t)G.ci[k] * ld;
            ld_t* t = R.t.data() + (size_t)r * cols;
            ld_t* ta = R.ta.data() + (size_t)r * cols;
            for (int p = 0; p < cols; ++p) {
                t[p] += a * (ld_t)x[p];
                ta[p] += a * fabsl((ld_t)x[p]);
            }
        }
    return R;
}

// ---------------------------------------------------------------------------
// the operations: the launcher, or its fp64 host stand-in.  The stand-ins are
// written from kt_launch.h's contract: one plain loop over the rows, the whole
// sum of a dot in block 0's partial slot and +0.0 in the others.
// ---------------------------------------------------------------------------
struct RowSum {  // stand-in defects of the row sum
    bool drop_last_mod4 = false, val_shift = false;
    int skip_deg = -1;
};
// out[p] = sum_{k0 <= k < k1} a_k X[col_k, p]
static void h_rowsum(const Graph& G, bool unit, const double* X, int ld, int cols, int k0, int k1, double* out,
                     const RowSum& m = RowSum()) {
    for (int p = 0; p < cols; ++p) out[p] = 0.0;
    for (int k = k0; k < k1; ++k) {
        const double a = unit ? 1.0 : G.va[(m.val_shift && k > 0) ? k - 1 : k];
        const double* x = X + (size_t)G.ci[k] * ld;
        for (int p = 0; p < cols; ++p) out[p] += a * x[p];
    }
}
static void h_store_part(double* part, int slots, int grid, const dvec& acc) {
    for (int s = 0; s < slots; ++s)
        for (int b = 0; b < grid; ++b) part[(size_t)s * grid + b] = b ? 0.0 : acc[s];
}

static hipError_t op_dot(const Shape& S, int P, int flags, const double* ucur, const double* sc, double* y, double* part) {
    const Graph& G = *S.G;
    if (!g_host)
        return kt::launch_spmm_dot(P, flags, S.grid, G.d_rp, G.d_ci, G.d_va, G.n, ucur, sc, y, part, S.T->d_lr,
                                   S.T->n_long(), S.T->lt, S.lb, 0);
    const bool unit = flags & F_UNIT;
    dvec acc(P, 0.0), t(P);
    for (int r = 0; r < G.n; ++r) {
        int k1 = G.rp[r + 1];
        if (mut("dot_drop_last_mod4") && G.deg(r) <= S.T->lt && G.deg(r) % 4 == 1) k1--;
        h_rowsum(G, unit, ucur, P, P, G.rp[r], k1, t.data());
        for (int p = 0; p < P; ++p) {
            const double yv = sc[p] * t[p];
            y[(size_t)r * P + p] = yv;
            acc[p] += (ucur[(size_t)r * P + p] * sc[p]) * yv;
        }
    }
    h_store_part(part, P, S.grid, acc);
    return hipSuccess;
}

// the epilogue of a y-form pass for one row: Out = g t - a x - b yold, the three dots
static void h_epilogue(int P, const double* coef, const double* t, const double* x, const double* yold, double* out,
                       dvec& acc) {
    for (int p = 0; p < P; ++p) {
        double u = coef[p] * t[p] - coef[P + p] * x[p];
        if (yold) u -= coef[2 * P + p] * yold[p];
        out[p] = u;
        acc[p] += x[p] * t[p];
        acc[P + p] += x[p] * u;
        acc[2 * P + p] += u * u;
    }
}
static void h_basis(int P, int bcols, size_t off, const double* coef, const double* x, const double* Vc,
                    const double* Vo, double* Vn, bool one_more) {
    const int hi = std::min(P, bcols + (one_more ? 1 : 0));
    for (int p = 0; p < hi; ++p) {
        double v = coef[p] * x[p] - coef[P + p] * Vc[off + p];
        if (Vo) v -= coef[2 * P + p] * Vo[off + p];
        Vn[off + p] = v;
    }
}

static hipError_t op_pass(const Shape& S, int P, int flags, const double* X, const void* Yold, double* Out,
                          const double* coef, double* part, const double* Vc, const double* Vo, double* Vn,
                          int bcols, double s0, const int* gate, int ngate) {
    const Graph& G = *S.G;
    if (!g_host)
        return kt::launch_spmm_lanczos(P, flags, S.grid, G.d_rp, G.d_ci, G.d_va, G.n, X, (const double*)Yold, Out,
                                       coef, part, S.T->d_lr, S.T->n_long(), S.T->lt, S.lb, 0, Vc, Vo, Vn, bcols,
                                       s0, gate, ngate);
    if (gate) {
        int run = 0;
        for (int k = 0; k < ngate; ++k) run |= gate[k];
        if (!run) return hipSuccess;
    }
    const bool unit = flags & (F_UNIT | F_I16), i16 = flags & F_I16;
    dvec acc(3 * P, 0.0), t(P), yo(P);
    for (int r = 0; r < G.n; ++r) {
        if (mut("pass_skip_long_plus1") && G.deg(r) == S.T->lt + 1) continue;
        const size_t off = (size_t)r * P;
        h_rowsum(G, unit, X, P, P, G.rp[r], G.rp[r + 1], t.data());
        const double* yp = nullptr;
        if (Yold && !mut("pass_no_yold")) {
            for (int p = 0; p < P; ++p)
                yo[p] = i16 ? s0 * (double)((const int16_t*)Yold)[off + p] : ((const double*)Yold)[off + p];
            yp = yo.data();
        }
        if (Vn) h_basis(P, bcols, off, coef, X + off, Vc, Vo, Vn, mut("vb_write_bcols"));
        h_epilogue(P, coef, t.data(), X + off, yp, Out + off, acc);
    }
    h_store_part(part, 3 * P, S.grid, acc);
    return hipSuccess;
}

static double h_sign(const uint32_t* Sg, int W, int r, int p, bool shifted) {
    const int b = shifted ? (p + 1) & 31 : p & 31;
    return ((Sg[(size_t)r * W + p / 32] >> b) & 1u) ? -1.0 : 1.0;
}
static hipError_t op_start(const Shape& S, int P, int flags, const uint32_t* Sg, double s0, void* Out, double* part) {
    const Graph& G = *S.G;
    if (!g_host)
        return kt::launch_spmm_lanczos_start(P, flags, S.grid, G.d_rp, G.d_ci, G.d_va, G.n, Sg, s0, (double*)Out,
                                             part, S.T->d_lr, S.T->n_long(), S.T->lt, S.lb, 0);
    const bool unit = flags & (F_UNIT | F_I16), i16 = flags & F_I16;
    const bool shift = mut("start_val_shift"), bit1 = mut("start_sign_bit_p1");
    const int W = (P + 31) / 32;
    dvec acc(3 * P, 0.0);
    for (int r = 0; r < G.n; ++r)
        for (int p = 0; p < P; ++p) {
            double sum = 0.0;
            for (int k = G.rp[r]; k < G.rp[r + 1]; ++k)
                sum += (unit ? 1.0 : G.va[(shift && k > 0) ? k - 1 : k]) * h_sign(Sg, W, G.ci[k], p, bit1);
            const double z = h_sign(Sg, W, r, p, false), u = s0 * sum;
            if (i16) ((int16_t*)Out)[(size_t)r * P + p] = (int16_t)(int)sum;
            else ((double*)Out)[(size_t)r * P + p] = u;
            acc[p] += z * sum;
            acc[P + p] += z * u;
            acc[2 * P + p] += u * u;
        }
    h_store_part(part, 3 * P, S.grid, acc);
    return hipSuccess;
}

static hipError_t op_first(const Shape& S, int P, int flags, const int16_t* T, double s0, double* Out,
                           const double* coef, double* part, const int* gate, int ngate) {
    const Graph& G = *S.G;
    if (!g_host)
        return kt::launch_spmm_lanczos_first(P, flags, S.grid, G.d_rp, G.d_ci, G.n, T, s0, Out, coef, part, S.T->d_lr,
                                             S.T->n_long(), S.T->lt, S.lb, 0, gate, ngate);
    dvec X((size_t)G.n * P), acc(3 * P, 0.0), t(P), c(coef, coef + 2 * P);
    for (size_t i = 0; i < X.size(); ++i) X[i] = s0 * (double)T[i];
    c.resize(3 * P, 0.0);
    if (mut("first_ignore_alpha"))
        for (int p = 0; p < P; ++p) c[P + p] = 0.0;
    for (int r = 0; r < G.n; ++r) {
        const size_t off = (size_t)r * P;
        h_rowsum(G, true, X.data(), P, P, G.rp[r], G.rp[r + 1], t.data());
        h_epilogue(P, c.data(), t.data(), X.data() + off, nullptr, Out + off, acc);
    }
    h_store_part(part, 3 * P, S.grid, acc);
    return hipSuccess;
}

static hipError_t op_quad(const Shape& S, int P, int flags, const double* X, const double* coef, double* part,
                          const double* Vc, const double* Vo, double* Vn, int bcols) {
    const Graph& G = *S.G;
    if (!g_host)
        return kt::launch_spmm_quadform(P, flags, S.grid, G.d_rp, G.d_ci, G.d_va, G.d_lower, G.n, X, coef, part,
                                        S.T->d_lr, S.T->n_long(), S.T->lt, S.lb, 0, Vc, Vo, Vn, bcols);
    const bool unit = flags & F_UNIT;
    dvec acc(3 * P, 0.0), s(P);
    for (int r = 0; r < G.n; ++r) {
        const size_t off = (size_t)r * P;
        const int lw = G.lower[r];
        int end = lw < 0 ? ~lw : lw;
        if (mut("quad_prefix_off_by_one") && end > G.rp[r]) end--;
        h_rowsum(G, unit, X, P, P, G.rp[r], end, s.data());
        const double arr = (lw < 0 && !mut("quad_no_diag")) ? (unit ? 1.0 : G.va[~lw]) : 0.0;
        if (Vn) h_basis(P, bcols, off, coef, X + off, Vc, Vo, Vn, mut("quad_vb_write_bcols"));
        for (int p = 0; p < P; ++p) acc[p] += X[off + p] * (2.0 * s[p] + arr * X[off + p]);
    }
    h_store_part(part, 3 * P, S.grid, acc);
    return hipSuccess;
}

// grid = chunk blocks + long blocks + short blocks
static hipError_t op_block(const Graph& G, const Tabs& T, int P, int flags, int grid, int lb, int cb, const double* X,
                           int ldx, double* Y, int ldy, double* ck_part, int slices, const int* skip) {
    if (!g_host) {
        const kt::CsrView V{G.d_rp, G.d_ci, G.d_va, G.n,      T.d_lr,  T.n_long(), T.lt,
                            T.st,   T.d_ckb, T.d_cke, T.n_chunks(), T.d_spr, T.d_spf,   T.n_split()};
        return kt::launch_spmm_block(P, flags, grid, V, X, ldx, Y, ldy, lb, cb, ck_part, 0, slices, skip);
    }
    if (skip && *skip == 0) return hipSuccess;
    const bool unit = flags & F_UNIT;
    dvec t(P);
    for (int s = 0; s < slices; ++s) {
        const double* Xs = X + (size_t)s * P;
        for (int r = 0; r < G.n; ++r) {
            if (G.deg(r) > T.st) continue;  // chunked below
            h_rowsum(G, unit, Xs, ldx, P, G.rp[r], G.rp[r + 1], t.data());
            for (int p = 0; p < P; ++p) Y[(size_t)r * ldy + s * P + p] = t[p];
        }
        double* part = ck_part + (size_t)s * T.n_chunks() * P;
        for (int i = 0; i < T.n_split(); ++i) {
            dvec sum(P, 0.0);
            const int c1 = T.spf[i + 1] - (mut("block_drop_last_chunk") ? 1 : 0);
            for (int c = T.spf[i]; c < T.spf[i + 1]; ++c) {
                h_rowsum(G, unit, Xs, ldx, P, T.ckb[c], T.cke[c], t.data());
                for (int p = 0; p < P; ++p) {
                    part[(size_t)c * P + p] = t[p];
                    if (c < c1) sum[p] += t[p];
                }
            }
            for (int p = 0; p < P; ++p) Y[(size_t)T.spr[i] * ldy + s * P + p] = sum[p];
        }
    }
    return hipSuccess;
}

static hipError_t op_update(int P, int grid, int n, const double* y, double* uprev, const double* ucur,
                            const double* sc, const double* sp, const double* coef, int first, double* part, bool nt,
                            double* rec, int bcols) {
    if (!g_host) return kt::launch_update(P, grid, n, y, uprev, ucur, sc, sp, coef, first, part, 0, nt, rec, bcols);
    const bool use_prev = !first || mut("update_reads_uprev_on_first");
    dvec acc(3 * P, 0.0);
    for (int r = 0; r < n; ++r)
        for (int p = 0; p < P; ++p) {
            const size_t off = (size_t)r * P + p;
            double u = y[off];
            if (use_prev) u -= (coef[p] * sp[p]) * uprev[off];
            u -= (coef[P + p] * sc[p]) * ucur[off];
            uprev[off] = u;
            if (rec && p < bcols) rec[(size_t)r * bcols + p] = u;
            acc[p] += u * u;
            acc[P + p] += y[off] * u;
            acc[2 * P + p] += ucur[off] * u;
        }
    h_store_part(part, 3 * P, grid, acc);
    return hipSuccess;
}

static hipError_t op_rademacher(int P, int n, uint64_t seed, int64_t base, const int* perm, double* X) {
    if (!g_host) return kt::launch_rademacher(P, n, seed, base, perm, X, 0);
    const bool noperm = mut("probes_ignore_perm");
    for (int r = 0; r < n; ++r)
        for (int p = 0; p < P; ++p)
            X[(size_t)r * P + p] = probe_neg(seed, base + p, (perm && !noperm) ? perm[r] : r) ? -1.0 : 1.0;
    return hipSuccess;
}
static hipError_t op_rademacher_cols(int n, int ncols, uint64_t seed, int64_t base, double* X, int ldx) {
    if (!g_host) return kt::launch_rademacher_cols(n, ncols, seed, base, X, ldx, 0);
    for (int r = 0; r < n; ++r)
        for (int p = 0; p < ncols; ++p) X[(size_t)r * ldx + p] = probe_neg(seed, base + p, r) ? -1.0 : 1.0;
    return hipSuccess;
}
static hipError_t op_signs(int P, int n, uint64_t seed, int64_t base, const int* perm, uint32_t* Sg) {
    if (!g_host) return kt::launch_rademacher_signs(P, n, seed, base, perm, Sg, 0);
    const int W = (P + 31) / 32;
    const bool noperm = mut("probes_ignore_perm");
    for (int r = 0; r < n; ++r)
        for (int w = 0; w < W; ++w) {
            uint32_t bits = 0;
            for (int b = 0; b < 32 && w * 32 + b < P; ++b)
                bits |= (uint32_t)probe_neg(seed, base + w * 32 + b, (perm && !noperm) ? perm[r] : r) << b;
            Sg[(size_t)r * W + w] = bits;
        }
    return hipSuccess;
}

// the sum of slot `slot`'s nblk partials (slot-major)
static double h_reduce(const double* partial, int nblk, int slot) {
    const int nb = mut("reduce_round_down_64") && nblk >= 64 ? nblk / 64 * 64 : nblk;
    double v = 0.0;
    for (int b = 0; b < nb; ++b) v += partial[(size_t)slot * nblk + b];
    return v;
}
static hipError_t op_coef_cgs2(int P, const double* partial, int nblk, int first, const double* k2s, const double* sc,
                               const double* sp, double* coef, double* t_alpha, double* t_up, double* hist) {
    if (!g_host) return kt::launch_coef_cgs2(P, partial, nblk, first, k2s, sc, sp, coef, t_alpha, t_up, hist, 0);
    for (int p = 0; p < P; ++p) {
        const double g1 = h_reduce(partial, nblk, p), s = sc[p];
        if (hist) hist[p] = s;
        const double G11 = s * s * k2s[p];
        double g0 = 0.0, G00 = 0.0, G01 = 0.0;
        if (!first) {
            g0 = s * k2s[P + p];
            G01 = sp[p] * s * k2s[2 * P + p];
            G00 = sp[p] * sp[p] * k2s[3 * P + p];
        }
        const double c0 = g0 + (g0 - (G00 * g0 + G01 * g1)), c1 = g1 + (g1 - (G01 * g0 + G11 * g1));
        coef[p] = t_up[p] = c0;
        coef[P + p] = t_alpha[p] = c1;
    }
    return hipSuccess;
}
static hipError_t op_norm(int P, const double* partial, int nblk, double* k2s, double* scale_next, double* t_low) {
    if (!g_host) return kt::launch_norm(P, partial, nblk, k2s, scale_next, t_low, 0);
    for (int p = 0; p < P; ++p) {
        const double r = h_reduce(partial, nblk, p), beta = sqrt(r);
        t_low[p] = beta;
        scale_next[p] = beta < 1e-8 ? 0.0 : 1.0 / beta;
        k2s[3 * P + p] = k2s[p];
        k2s[p] = r;
        k2s[P + p] = h_reduce(partial, nblk, P + p);
        k2s[2 * P + p] = h_reduce(partial, nblk, 2 * P + p);
    }
    return hipSuccess;
}
static hipError_t op_ycoef(int P, const double* partial, int nblk, int start, int last, double s0, double* ys,
                           double* t_alpha, double* t_up, double* t_low, double* guard, const int* gate = nullptr,
                           int ngate = 0) {
    if (!g_host)
        return kt::launch_ycoef(P, partial, nblk, start, last, s0, ys, t_alpha, t_up, t_low, guard, 0, gate, ngate);
    if (gate) {
        int run = 0;
        for (int k = 0; k < ngate; ++k) run |= gate[k];
        if (!run) return hipSuccess;
    }
    for (int p = 0; p < P; ++p) {
        const double d0 = h_reduce(partial, nblk, p), d1 = h_reduce(partial, nblk, P + p);
        const double d2 = h_reduce(partial, nblk, 2 * P + p);
        double an, bn, sq, g = 1.0;
        if (start) {
            an = d1 * s0;
            bn = 0.0;
            sq = d2 - an * an;
            ys[P + p] = ys[2 * P + p] = ys[4 * P + p] = 0.0;
            guard[p] = 1.0;
        } else {
            const double aj = ys[p], bj = ys[P + p], am1 = ys[2 * P + p], nyj = ys[3 * P + p], ydj = ys[4 * P + p];
            const double b1 = ys[5 * P + p];
            g = guard[p];
            an = (d0 - 2.0 * aj * nyj - 2.0 * bj * ydj + aj * aj * aj + 2.0 * aj * bj * bj + bj * bj * am1) / (b1 * b1);
            bn = b1;
            sq = d2 - an * an - b1 * b1;
            ys[P + p] = b1;
            ys[2 * P + p] = aj;
            ys[4 * P + p] = d1;
        }
        const double bnext = sqrt(sq > 0.0 ? sq : 0.0);
        ys[p] = an;
        ys[3 * P + p] = d2;
        ys[5 * P + p] = bnext;
        t_alpha[p] = an;
        t_up[p] = bn;
        t_low[p] = bnext;
        if (!last) {
            const double ratio = sq / d2;
            if (mut("ycoef_guard_overwrite")) guard[p] = ratio;
            else guard[p] = (ratio < g || ratio != ratio) ? ratio : g;
        }
        const double inv = (bnext > 0.0 && bnext < INFINITY) ? 1.0 / bnext : 0.0;
        ys[6 * P + p] = inv;
        ys[7 * P + p] = an * inv;
        ys[8 * P + p] = bn * inv;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// the y-form passes: run + check
// ---------------------------------------------------------------------------
static std::vector<int> kWidths = {1, 2, 4, 8, 16, 32, 64, 128};  // --small: {1, 4, 32}

// sum over the blocks of slot `slot`
static ld_t slot_sum(const dvec& part, int grid, int slot) {
    ld_t s = 0.0L;
    for (int b = 0; b < grid; ++b) s += (ld_t)part[(size_t)slot * grid + b];
    return s;
}

struct PassCfg {
    int flags = 0;
    int xsrc = 0;      // X: 0 the fp64 block, 1 XT = s0 * (double)T
    int ysrc = 0;      // Yold: 0 none, 1 the fp64 block, 2 the int16 table (F_I16), 3 XT as fp64
    int bcols = 0;     // > 0: Vn set
    bool vo = false;   // Vo set
    bool gate = false;
    bool inplace = false;  // Out over Yold (ysrc 1)
};
// {Out (+ guard), partial (+ guard), Vn (+ guard)}
static std::vector<dvec> run_pass(const Shape& S, const Inputs& I, const PassCfg& c) {
    const size_t np = (size_t)I.n * I.P;
    g_work.off = 0;
    dvec out0 = sentinels(np);
    if (c.inplace) std::copy(I.Yold.begin(), I.Yold.end(), out0.begin());
    double* dOut = up(out0);
    double* dpart = up(sentinels((size_t)3 * I.P * S.grid));
    double* dVn = up(sentinels(np));
    const void* dY = c.ysrc == 1 ? (c.inplace ? (const void*)dOut : (const void*)I.dYold)
                                 : c.ysrc == 2 ? (const void*)I.dT : c.ysrc == 3 ? (const void*)I.dXT : nullptr;
    LAUNCH(op_pass(S, I.P, c.flags, c.xsrc ? I.dXT : I.dX, dY, dOut, I.dcoef, dpart, c.bcols ? I.dVc : nullptr,
                   (c.bcols && c.vo) ? I.dVo : nullptr, c.bcols ? dVn : nullptr, c.bcols, I.s0,
                   c.gate ? I.dgate : nullptr, c.gate ? 2 : 0));
    return {down(dOut, np + GUARD), down(dpart, (size_t)3 * I.P * S.grid + GUARD), down(dVn, np + GUARD)};
}

// Out = g t - a x - b yold per element and the three dots, for X (fp64 block
// Xh), Yold values yo (nullptr: none); o = {Out, partial}
static void check_pass_out(Case& c, bool ex, const Shape& S, const Inputs& I, bool unit, const dvec& Xh, const dvec* yo,
                           const std::vector<dvec>& o) {
    const Graph& G = *S.G;
    const int P = I.P, n = I.n;
    const size_t np = (size_t)n * P;
    const RefAX& R = ref_ax(G, unit, Xh, P, P);
    c.written("Out", sentinels(np), o[0], np);
    c.written("partial", sentinels((size_t)3 * P * S.grid), o[1], (size_t)3 * P * S.grid);
    std::vector<ld_t> dot(3 * P, 0.0L), maj(3 * P, 0.0L);
    for (int r = 0; r < n; ++r) {
        const ld_t gk = gam((ld_t)G.deg(r) + 3);
        for (int p = 0; p < P; ++p) {
            const size_t t = (size_t)r * P + p;
            const ld_t g = I.coef[p], a = I.coef[P + p], b = I.coef[2 * P + p], x = Xh[t];
            ld_t ref = g * R.t[t] - a * x, m = fabsl(g) * R.ta[t] + fabsl(a * x);
            if (yo) {
                ref -= b * (ld_t)(*yo)[t];
                m += fabsl(b * (ld_t)(*yo)[t]);
            }
            c.value(ex, "Out", (long)t, o[0][t], ref, gk * m);
            dot[p] += x * R.t[t];
            maj[p] += fabsl(x) * R.ta[t];
            dot[P + p] += x * ref;
            maj[P + p] += fabsl(x) * m;
            dot[2 * P + p] += ref * ref;
            maj[2 * P + p] += m * m;
        }
    }
    const ld_t g1 = gam((ld_t)n + G.dmax + 4), g2 = gam((ld_t)n + 2 * G.dmax + 8);
    static const char* dn[3] = {"X.t", "X.Out", "Out.Out"};
    for (int s = 0; s < 3 * P; ++s)
        c.value(ex, dn[s / P], s, slot_sum(o[1], S.grid, s), dot[s], (s < 2 * P ? g1 : g2) * maj[s]);
}

// Vn = g X - a Vc - b Vo on the columns < bcols; the others keep their sentinel
static void check_basis(Case& c, bool ex, const Inputs& I, const dvec& Xh, bool vo, int bcols, const dvec& vn) {
    const int P = I.P;
    for (int r = 0; r < I.n; ++r)
        for (int p = 0; p < P; ++p) {
            const size_t t = (size_t)r * P + p;
            if (p >= bcols) {
                c.same("Vn beyond bcols", (long)t, vn[t], SENT);
                continue;
            }
            const ld_t g = I.coef[p], a = I.coef[P + p], b = I.coef[2 * P + p];
            ld_t ref = g * (ld_t)Xh[t] - a * (ld_t)I.Vc[t], m = fabsl(g * (ld_t)Xh[t]) + fabsl(a * (ld_t)I.Vc[t]);
            if (vo) {
                ref -= b * (ld_t)I.Vo[t];
                m += fabsl(b * (ld_t)I.Vo[t]);
            }
            if (bits_of(vn[t]) == bits_of(SENT)) c.fail("Vn not written", (long)t, vn[t], (double)ref, 0.0, INFINITY);
            c.value(ex, "Vn", (long)t, vn[t], ref, gam(3) * m);
        }
    for (size_t t = (size_t)I.n * P; t < vn.size(); ++t) c.same("Vn guard", (long)t, vn[t], SENT);
}

static int odd_below(int P) { return P >= 4 ? P / 2 + 1 : 1; }  // an odd bcols < P (P >= 4)

static void pass_case(const Shape& S, int P, int kind, const Form& f, bool has_old, int bcols, bool vo, bool inplace) {
    Case c(G_PASS, kind_name(kind),
           fmt("%s P=%d form=%s grid=%d long_blocks=%d yold=%d bcols=%d vo=%d inplace=%d", S.tag, P, f.name, S.grid,
               S.lb, (int)has_old, bcols, (int)vo, (int)inplace));
    if (g_list) return;
    const Inputs& I = inputs(*S.G, P, kind);
    PassCfg cfg;
    cfg.flags = f.flags;
    cfg.ysrc = (f.flags & F_I16) ? 2 : has_old ? 1 : 0;
    cfg.bcols = bcols;
    cfg.vo = vo;
    cfg.gate = f.mode == 2;
    cfg.inplace = inplace;
    auto o = run_twice(c, [&] { return run_pass(S, I, cfg); });
    const dvec* yo = cfg.ysrc == 2 ? &I.XT : cfg.ysrc == 1 ? &I.Yold : nullptr;
    check_pass_out(c, kind == INT8, S, I, f.flags & (F_UNIT | F_I16), I.X, yo, o);
    if (bcols) check_basis(c, kind == INT8, I, I.X, vo, bcols, o[2]);
    else c.unchanged("Vn", sentinels((size_t)I.n * P), o[2]);
}

static void grp_pass() {
    for (int P : kWidths) {
        refs_reset();
        for (const Shape& S : shapes_for(P))
            for (int kind = 0; kind < 2; ++kind)
                for (const Form* f : forms_of("lanczos_pass")) {
                    if (f->mode == 1) {  // basis-forming: Vo null / set, bcols 1, odd, P
                        ivec bc = {1, P};
                        if (P >= 4) bc.push_back(odd_below(P));
                        for (int b : bc)
                            for (int vo = 0; vo < 2; ++vo) pass_case(S, P, kind, *f, vo != 0, b, vo != 0, false);
                    } else if (f->flags & F_I16) {
                        pass_case(S, P, kind, *f, true, 0, false, false);
                    } else {
                        pass_case(S, P, kind, *f, false, 0, false, false);  // start mode
                        pass_case(S, P, kind, *f, true, 0, false, kind == NORMAL);
                    }
                }
    }
}

// {Out as doubles (+ guard), partial (+ guard)}
static std::vector<dvec> run_start(const Shape& S, const Inputs& I, int flags) {
    const size_t np = (size_t)I.n * I.P;
    g_work.off = 0;
    double* dpart = up(sentinels((size_t)3 * I.P * S.grid));
    dvec out;
    if (flags & F_I16) {
        int16_t* dT = up(std::vector<int16_t>(np + GUARD, (int16_t)-32123));
        LAUNCH(op_start(S, I.P, flags, I.dS, I.s0, dT, dpart));
        out = to_d(down(dT, np + GUARD));
    } else {
        double* dOut = up(sentinels(np));
        LAUNCH(op_start(S, I.P, flags, I.dS, I.s0, dOut, dpart));
        out = down(dOut, np + GUARD);
    }
    return {out, down(dpart, (size_t)3 * I.P * S.grid + GUARD)};
}

static void start_case(const Shape& S, int P, int kind, const Form& f) {
    Case c(G_START, kind_name(kind), fmt("%s P=%d form=%s grid=%d long_blocks=%d", S.tag, P, f.name, S.grid, S.lb));
    if (g_list) return;
    const Graph& G = *S.G;
    const Inputs& I = inputs(G, P, kind);
    const bool ex = kind == INT8, i16 = f.flags & F_I16;
    auto o = run_twice(c, [&] { return run_start(S, I, f.flags); });
    const size_t np = (size_t)G.n * P;
    const RefAX& R = ref_ax(G, f.flags & (F_UNIT | F_I16), I.Z, P, P);
    c.written("partial", sentinels((size_t)3 * P * S.grid), o[1], (size_t)3 * P * S.grid);
    for (size_t t = np; t < o[0].size(); ++t) c.same("Out guard", (long)t, o[0][t], i16 ? -32123.0 : SENT);
    std::vector<ld_t> dot(3 * P, 0.0L), maj(3 * P, 0.0L);
    const ld_t s0 = I.s0;
    for (int r = 0; r < G.n; ++r) {
        const ld_t gk = gam((ld_t)G.deg(r) + 1);
        for (int p = 0; p < P; ++p) {
            const size_t t = (size_t)r * P + p;
            const ld_t ref = s0 * R.t[t], m = fabsl(s0) * R.ta[t], z = I.Z[t];
            if (i16) {  // the integer row sums themselves (a sentinel never equals one: |sum| <= 320)
                c.exact("table", (long)t, o[0][t], (double)R.t[t]);
            } else {
                if (bits_of(o[0][t]) == bits_of(SENT)) c.fail("Out not written", (long)t, o[0][t], (double)ref, 0.0, INFINITY);
                c.value(ex, "Out", (long)t, o[0][t], ref, gk * m);
            }
            dot[p] += z * R.t[t];
            maj[p] += R.ta[t];
            dot[P + p] += z * ref;
            maj[P + p] += m;
            dot[2 * P + p] += ref * ref;
            maj[2 * P + p] += m * m;
        }
    }
    const ld_t g1 = gam((ld_t)G.n + G.dmax + 4), g2 = gam((ld_t)G.n + 2 * G.dmax + 8);
    static const char* dn[3] = {"z.Az", "z.Out", "Out.Out"};
    for (int s = 0; s < 3 * P; ++s)
        c.value(ex, dn[s / P], s, slot_sum(o[1], S.grid, s), dot[s], (s < 2 * P ? g1 : g2) * maj[s]);
}

static void grp_start() {
    for (int P : kWidths) {
        refs_reset();
        for (const Shape& S : shapes_for(P))
            for (int kind = 0; kind < 2; ++kind)
                for (const Form* f : forms_of("lanczos_start")) start_case(S, P, kind, *f);
    }
}

static std::vector<dvec> run_first(const Shape& S, const Inputs& I, int flags, bool gate) {
    const size_t np = (size_t)I.n * I.P;
    g_work.off = 0;
    double* dOut = up(sentinels(np));
    double* dpart = up(sentinels((size_t)3 * I.P * S.grid));
    LAUNCH(op_first(S, I.P, flags, I.dT, I.s0, dOut, I.dcoef, dpart, gate ? I.dgate : nullptr, gate ? 2 : 0));
    return {down(dOut, np + GUARD), down(dpart, (size_t)3 * I.P * S.grid + GUARD)};
}

static void grp_first() {
    for (int P : kWidths) {
        refs_reset();
        for (const Shape& S : shapes_for(P))
            for (int kind = 0; kind < 2; ++kind)
                for (const Form* f : forms_of("lanczos_first")) {
                    Case c(G_FIRST, kind_name(kind),
                           fmt("%s P=%d form=%s grid=%d long_blocks=%d", S.tag, P, f->name, S.grid, S.lb));
                    if (g_list) continue;
                    const Inputs& I = inputs(*S.G, P, kind);
                    auto o = run_twice(c, [&] { return run_first(S, I, f->flags, f->mode == 2); });
                    check_pass_out(c, kind == INT8, S, I, true, I.XT, nullptr, o);
                }
    }
}

static std::vector<dvec> run_quad(const Shape& S, const Inputs& I, int flags, int bcols, bool vo) {
    const size_t np = (size_t)I.n * I.P;
    g_work.off = 0;
    double* dpart = up(sentinels((size_t)3 * I.P * S.grid));
    double* dVn = up(sentinels(np));
    LAUNCH(op_quad(S, I.P, flags, I.dX, I.dcoef, dpart, bcols ? I.dVc : nullptr, (bcols && vo) ? I.dVo : nullptr,
                   bcols ? dVn : nullptr, bcols));
    return {down(dpart, (size_t)3 * I.P * S.grid + GUARD), down(dVn, np + GUARD)};
}

static void quad_case(const Shape& S, int P, int kind, const Form& f, int bcols, bool vo) {
    Case c(G_QUAD, kind_name(kind),
           fmt("%s P=%d form=%s grid=%d long_blocks=%d bcols=%d vo=%d", S.tag, P, f.name, S.grid, S.lb, bcols, (int)vo));
    if (g_list) return;
    const Graph& G = *S.G;
    const Inputs& I = inputs(G, P, kind);
    auto o = run_twice(c, [&] { return run_quad(S, I, f.flags, bcols, vo); });
    const RefAX& R = ref_ax(G, f.flags & F_UNIT, I.X, P, P);
    c.written("partial", sentinels((size_t)3 * P * S.grid), o[0], (size_t)3 * P * S.grid);
    const ld_t gk = gam((ld_t)G.n + G.dmax + 4);
    for (int p = 0; p < P; ++p) {
        ld_t q = 0.0L, m = 0.0L;  // X'AX from the full matrix; by symmetry the lower form's majorant is the same
        for (int r = 0; r < G.n; ++r) {
            q += (ld_t)I.X[(size_t)r * P + p] * R.t[(size_t)r * P + p];
            m += fabsl((ld_t)I.X[(size_t)r * P + p]) * R.ta[(size_t)r * P + p];
        }
        c.value(kind == INT8, "X'AX", p, slot_sum(o[0], S.grid, p), q, gk * m);
    }
    for (size_t t = (size_t)P * S.grid; t < (size_t)3 * P * S.grid; ++t) c.same("slabs 1, 2", (long)t, o[0][t], 0.0);
    if (bcols) check_basis(c, kind == INT8, I, I.X, vo, bcols, o[1]);
    else c.unchanged("Vn", sentinels((size_t)I.n * P), o[1]);
}

static void grp_quad() {
    for (int P : kWidths) {
        refs_reset();
        for (const Shape& S : shapes_for(P))
            for (int kind = 0; kind < 2; ++kind)
                for (const Form* f : forms_of("quadform")) {
                    if (f->mode != 1) {
                        quad_case(S, P, kind, *f, 0, false);
                        continue;
                    }
                    ivec bc = {1, P};
                    if (P >= 4) bc.push_back(odd_below(P));
                    for (int b : bc)
                        for (int vo = 0; vo < 2; ++vo) quad_case(S, P, kind, *f, b, vo != 0);
                }
    }
}

// ---------------------------------------------------------------------------
// spmm_dot
// ---------------------------------------------------------------------------
static std::vector<dvec> run_dot(const Shape& S, const Inputs& I, int flags) {
    const size_t np = (size_t)I.n * I.P;
    g_work.off = 0;
    double* dy = up(sentinels(np));
    double* dpart = up(sentinels((size_t)I.P * S.grid));
    LAUNCH(op_dot(S, I.P, flags, I.dX, I.dsc, dy, dpart));
    return {down(dy, np + GUARD), down(dpart, (size_t)I.P * S.grid + GUARD)};
}

static void dot_case(const Shape& S, int P, int kind, const Form& f) {
    Case c(G_DOT, kind_name(kind), fmt("%s P=%d form=%s grid=%d long_blocks=%d", S.tag, P, f.name, S.grid, S.lb));
    if (g_list) return;
    const Graph& G = *S.G;
    const Inputs& I = inputs(G, P, kind);
    const bool ex = kind == INT8;
    auto o = run_twice(c, [&] { return run_dot(S, I, f.flags); });
    const size_t np = (size_t)G.n * P;
    const RefAX& R = ref_ax(G, f.flags & F_UNIT, I.X, P, P);
    c.written("y", sentinels(np), o[0], np);
    c.written("partial", sentinels((size_t)P * S.grid), o[1], (size_t)P * S.grid);
    std::vector<ld_t> dot(P, 0.0L), maj(P, 0.0L);
    for (int r = 0; r < G.n; ++r) {
        const ld_t gk = gam((ld_t)G.deg(r) + 1);
        for (int p = 0; p < P; ++p) {
            const size_t t = (size_t)r * P + p;
            const ld_t s = I.sc[p], ref = s * R.t[t], m = fabsl(s) * R.ta[t];
            c.value(ex, "y", (long)t, o[0][t], ref, gk * m);
            dot[p] += s * (ld_t)I.X[t] * ref;
            maj[p] += fabsl(s * (ld_t)I.X[t]) * m;
        }
    }
    const ld_t g1 = gam((ld_t)G.n + G.dmax + 4);
    for (int p = 0; p < P; ++p) c.value(ex, "v.y", p, slot_sum(o[1], S.grid, p), dot[p], g1 * maj[p]);
}

static void grp_dot() {
    for (int P : kWidths) {
        refs_reset();
        for (const Shape& S : shapes_for(P))
            for (int kind = 0; kind < 2; ++kind)
                for (const Form* f : forms_of("spmm_dot")) dot_case(S, P, kind, *f);
    }
}

// ---------------------------------------------------------------------------
// spmm_block
// ---------------------------------------------------------------------------
// skipmode: 0 skip == nullptr, 1 *skip == 1, 2 *skip == 0 (nothing may be written)
static void block_case(const Graph& G, const Tabs& T, const char* tag, int P, int kind, const Form& f, int slices,
                       int skipmode, const dvec& X, int ldx) {
    const int gs = std::min(kt::spmm_grid(G.n, P, 1024), (T.lt == 32) ? 3 : 1024);
    const int lb = T.lt == 32 ? 1 : kt::long_blocks_for(T.n_long(), 512);
    const int cb = T.n_chunks() ? std::min((T.n_chunks() + 7) / 8, T.lt == 32 ? 2 : 512) : 0;
    const int grid = gs + lb + cb;
    Case c(G_BLOCK, kind_name(kind),
           fmt("%s P=%d form=%s grid=%d long_blocks=%d chunk_blocks=%d slices=%d skip=%d", tag, P, f.name, grid, lb, cb,
               slices, skipmode));
    if (g_list) return;
    const int ldy = 2 * P + 4;
    const size_t nck = (size_t)slices * T.n_chunks() * P;
    const dvec Y0((size_t)(G.n + 2) * ldy, SENT), ck0 = sentinels(nck);
    auto o = run_twice(c, [&] {
        g_work.off = 0;
        const double* dX = up(X);
        double* dY = up(Y0);
        double* dck = up(ck0);
        const int* dskip = skipmode ? up(ivec{skipmode == 1 ? 1 : 0}) : nullptr;
        LAUNCH(op_block(G, T, P, f.flags, grid, lb, cb, dX, ldx, dY, ldy, dck, slices, dskip));
        return std::vector<dvec>{down(dY, Y0.size()), down(dck, ck0.size())};
    });
    if (skipmode == 2) {
        c.unchanged("Y (skipped)", Y0, o[0]);
        c.unchanged("ck_part (skipped)", ck0, o[1]);
        return;
    }
    c.written("ck_part", ck0, o[1], nck);
    const RefAX& R = ref_ax(G, f.flags & F_UNIT, X, ldx, 2 * P);
    for (size_t t = 0; t < Y0.size(); ++t) {
        const int r = (int)(t / ldy), col = (int)(t % ldy);
        if (r >= G.n || col >= slices * P) {
            c.same("Y padding / guard", (long)t, o[0][t], SENT);
            continue;
        }
        if (bits_of(o[0][t]) == bits_of(SENT)) c.fail("Y not written", (long)t, o[0][t], 0.0, 0.0, INFINITY);
        const size_t q = (size_t)r * 2 * P + col;
        c.value(kind == INT8, "Y", (long)t, o[0][t], R.t[q], gam((ld_t)G.deg(r)) * R.ta[q]);
    }
}

static void grp_block() {
    for (int P : kWidths) {
        const int ldx = 2 * P + 2;  // even: a lane's 16-byte loads stay aligned
        for (int kind = 0; kind < 2; ++kind) {
            refs_reset();
            dvec XA((size_t)g_A.n * ldx, NAN), XB((size_t)g_B.n * ldx, NAN);
            if (!g_list) {
                for (int r = 0; r < g_A.n; ++r)
                    for (int p = 0; p < 2 * P; ++p) XA[(size_t)r * ldx + p] = kind == INT8 ? rint8() : rnormal();
                for (int r = 0; r < g_B.n; ++r)
                    for (int p = 0; p < 2 * P; ++p) XB[(size_t)r * ldx + p] = kind == INT8 ? rint8() : rnormal();
            }
            for (const Form* f : forms_of("spmm_block"))
                for (int slices = 1; slices <= 2; ++slices)
                    for (int skipmode = 0; skipmode < 3; ++skipmode) {
                        block_case(g_A, g_A.t64, "A/64-64", P, kind, *f, slices, skipmode, XA, ldx);
                        block_case(g_B, g_B.t64, "B", P, kind, *f, slices, skipmode, XB, ldx);
                    }
            // long_thresh 32 < split_thresh 64: long-wave rows of 33 .. 64 beside the chunked rows
            for (const Form* f : forms_of("spmm_block")) block_case(g_A, g_A.t32, "A/32-64", P, kind, *f, 2, 0, XA, ldx);
        }
    }
}

// ---------------------------------------------------------------------------
// update
// ---------------------------------------------------------------------------
static void update_case(const Graph& G, int grid, int P, int kind, int first, bool nt, int bcols) {
    Case c(G_UPDATE, kind_name(kind),
           fmt("n=%d P=%d grid=%d first=%d nt=%d bcols=%d", G.n, P, grid, first, (int)nt, bcols));
    if (g_list) return;
    const Inputs& I = inputs(G, P, kind);
    const bool ex = kind == INT8;
    const size_t np = (size_t)G.n * P;
    // y = X, u_cur = Vc, u_prev = Yold (first: never read, a sentinel block), sp = the b coefficients
    dvec up0 = sentinels(np);
    if (!first) std::copy(I.Yold.begin(), I.Yold.end(), up0.begin());
    const dvec rec0 = sentinels((size_t)G.n * bcols), part0 = sentinels((size_t)3 * P * grid);
    auto o = run_twice(c, [&] {
        g_work.off = 0;
        double* dup = up(up0);
        double* drec = up(rec0);
        double* dpart = up(part0);
        LAUNCH(op_update(P, grid, G.n, I.dX, dup, I.dVc, I.dsc, I.dcoef + 2 * P, I.dcoef, first, dpart, nt,
                         bcols ? drec : nullptr, bcols));
        return std::vector<dvec>{down(dup, up0.size()), down(drec, rec0.size()), down(dpart, part0.size())};
    });
    c.written("u_next", sentinels(np), o[0], np);
    c.written("partial", part0, o[2], (size_t)3 * P * grid);
    c.written("rec", rec0, o[1], (size_t)G.n * bcols);
    std::vector<ld_t> dot(3 * P, 0.0L), maj(3 * P, 0.0L);
    for (int r = 0; r < G.n; ++r)
        for (int p = 0; p < P; ++p) {
            const size_t t = (size_t)r * P + p;
            const ld_t a0 = first ? 0.0L : (ld_t)I.coef[p] * (ld_t)I.coef[2 * P + p];
            const ld_t a1 = (ld_t)I.coef[P + p] * (ld_t)I.sc[p], y = I.X[t], cv = I.Vc[t];
            ld_t ref = y - a1 * cv, m = fabsl(y) + fabsl(a1 * cv);
            if (!first) {
                ref -= a0 * (ld_t)I.Yold[t];
                m += fabsl(a0 * (ld_t)I.Yold[t]);
            }
            c.value(ex, "u_next", (long)t, o[0][t], ref, gam(4) * m);
            if (p < bcols) c.same("rec", (long)(r * bcols + p), o[1][(size_t)r * bcols + p], o[0][t]);
            dot[p] += ref * ref;
            maj[p] += m * m;
            dot[P + p] += y * ref;
            maj[P + p] += fabsl(y) * m;
            dot[2 * P + p] += cv * ref;
            maj[2 * P + p] += fabsl(cv) * m;
        }
    const ld_t g1 = gam((ld_t)G.n + 6), g2 = gam((ld_t)G.n + 10);
    static const char* dn[3] = {"u.u", "y.u", "u_cur.u"};
    for (int s = 0; s < 3 * P; ++s)
        c.value(ex, dn[s / P], s, slot_sum(o[2], grid, s), dot[s], (s < P ? g2 : g1) * maj[s]);
}

static void grp_update() {
    for (int P : kWidths)
        for (const Graph* G : {&g_A, &g_B})
            for (int kind = 0; kind < 2; ++kind)
                for (int first = 0; first < 2; ++first)
                    for (int nt = 0; nt < 2; ++nt) {
                        const int full = kt::spmm_grid(G->n, P, 1024);
                        ivec bc = {0, 1, P};
                        if (P >= 4) bc.push_back(odd_below(P));
                        for (int b : bc) update_case(*G, (b == 1) ? std::min(full, 3) : full, P, kind, first, nt != 0, b);
                    }
}

// ---------------------------------------------------------------------------
// probes
// ---------------------------------------------------------------------------
static void grp_probes() {
    const int n = g_A.n;
    ivec perm(n);
    for (int r = 0; r < n; ++r) perm[r] = r;
    for (int i = n; i > 1; --i) std::swap(perm[i - 1], perm[rnd() % i]);
    for (int P : kWidths)
        for (int wp = 0; wp < 2; ++wp) {
            Case c(G_PROBES, "rademacher_and_signs", fmt("n=%d P=%d perm=%d", n, P, wp));
            if (g_list) continue;
            const int W = (P + 31) / 32;
            const size_t np = (size_t)n * P;
            const std::vector<uint32_t> S0((size_t)n * W + GUARD, 0xdeadbeefu);
            auto o = run_twice(c, [&] {
                g_work.off = 0;
                const int* dperm = wp ? up(perm) : nullptr;
                double* dX = up(sentinels(np));
                uint32_t* dS = up(S0);
                LAUNCH(op_rademacher(P, n, kSeed, kProbeBase, dperm, dX));
                LAUNCH(op_signs(P, n, kSeed, kProbeBase, dperm, dS));
                return std::vector<dvec>{down(dX, np + GUARD), to_d(down(dS, S0.size()))};
            });
            c.written("X", sentinels(np), o[0], np);
            for (size_t t = (size_t)n * W; t < S0.size(); ++t) c.same("S guard", (long)t, o[1][t], (double)0xdeadbeefu);
            for (int r = 0; r < n; ++r)
                for (int w = 0; w < W; ++w) {
                    uint32_t ref = 0, fromx = 0;
                    for (int b = 0; b < 32 && w * 32 + b < P; ++b) {
                        const int p = w * 32 + b;
                        const int neg = probe_neg(kSeed, kProbeBase + p, wp ? perm[r] : r);
                        c.exact("X", (long)(r * P + p), o[0][(size_t)r * P + p], neg ? -1.0 : 1.0);
                        ref |= (uint32_t)neg << b;
                        fromx |= (uint32_t)(o[0][(size_t)r * P + p] == -1.0) << b;
                    }
                    // the packed word: the reference's bits, the fp64 block's bits, zero above P
                    c.exact("S", (long)(r * W + w), o[1][(size_t)r * W + w], (double)ref);
                    c.exact("S vs X", (long)(r * W + w), o[1][(size_t)r * W + w], (double)fromx);
                }
        }
    for (int ncols : {1, 37, 64}) {
        const int ldx = ncols + 3;
        Case c(G_PROBES, "rademacher_cols", fmt("n=%d ncols=%d ldx=%d", n, ncols, ldx));
        if (g_list) continue;
        const dvec X0((size_t)(n + 2) * ldx, SENT);
        auto o = run_twice(c, [&] {
            g_work.off = 0;
            double* dX = up(X0);
            LAUNCH(op_rademacher_cols(n, ncols, kSeed, kProbeBase, dX, ldx));
            return std::vector<dvec>{down(dX, X0.size())};
        });
        for (size_t t = 0; t < X0.size(); ++t) {
            const int r = (int)(t / ldx), p = (int)(t % ldx);
            if (r >= n || p >= ncols) c.same("X padding / guard", (long)t, o[0][t], SENT);
            else c.exact("X", (long)t, o[0][t], probe_neg(kSeed, kProbeBase + p, r) ? -1.0 : 1.0);
        }
    }
}

// ---------------------------------------------------------------------------
// coef: launch_coef_cgs2, launch_norm, launch_ycoef
// ---------------------------------------------------------------------------
static const int kNblk[8] = {1, 63, 64, 65, 2047, 2048, 2049, 4100};

// slot-major partials [slots][nblk]; kind INT8: integers, NORMAL: normals
static dvec make_partials(int slots, int nblk, int kind) {
    dvec v = sentinels((size_t)slots * nblk);
    for (size_t t = 0; t < (size_t)slots * nblk; ++t) v[t] = kind == INT8 ? rint8() : rnormal();
    return v;
}
static void slot_ref(const dvec& part, int nblk, int slot, ld_t& sum, ld_t& abs) {
    sum = abs = 0.0L;
    for (int b = 0; b < nblk; ++b) {
        sum += (ld_t)part[(size_t)slot * nblk + b];
        abs += fabsl((ld_t)part[(size_t)slot * nblk + b]);
    }
}

// The slab reduction through each of the three kernels, arranged so that the
// kernel's scalar step passes the sums on unchanged: norm stores r in k2s;
// cgs2 with first = 1 and ||u||^2 = 0 gives c1 = 2 g1; ycoef in ordinary mode
// with alpha_j = beta_j = 0, beta_{j+1} = 1 gives alpha = d0, ys[4] = d1,
// ys[3] = d2.  Integer partials: exact; normal partials: a term passes through
// at most nblk + 6 additions in any order of a 64-lane tree.
static void reduce_case(int P, int nblk, int kind, int which) {
    static const char* wn[3] = {"norm", "coef_cgs2", "ycoef"};
    Case c(G_COEF, fmt("reduce_%s_%s", wn[which], kind_name(kind)), fmt("P=%d nblk=%d", P, nblk));
    if (g_list) return;
    const bool ex = kind == INT8;
    const int slots = which == 1 ? P : 3 * P;
    dvec part = make_partials(slots, nblk, kind);
    if (which == 0)  // ||u||^2 >= 0
        for (int p = 0; p < P; ++p)
            for (int b = 0; b < nblk; ++b) part[(size_t)p * nblk + b] = fabs(part[(size_t)p * nblk + b]);
    dvec ys0 = sentinels(9 * P);
    for (int t = 0; t < 9 * P; ++t) ys0[t] = (t / P == 5) ? 1.0 : 0.0;
    dvec k2s0 = sentinels(4 * P);
    for (int t = 0; t < 4 * P; ++t) k2s0[t] = which == 0 ? (double)(t + 1) : (t < P ? 0.0 : NAN);
    const dvec one(P, 1.0), v0 = sentinels(P), c0 = sentinels(2 * P);
    auto o = run_twice(c, [&] {
        g_work.off = 0;
        const double* dpart = up(part);
        std::vector<dvec> r;
        if (which == 0) {
            double* dk = up(k2s0);
            double* dsn = up(v0);
            double* dlow = up(v0);
            LAUNCH(op_norm(P, dpart, nblk, dk, dsn, dlow));
            r = {down(dk, k2s0.size()), down(dsn, v0.size()), down(dlow, v0.size())};
        } else if (which == 1) {
            const double* dk = up(k2s0);
            const double* dsc = up(one);
            double* dcoef = up(c0);
            double* da = up(v0);
            double* du = up(v0);
            LAUNCH(op_coef_cgs2(P, dpart, nblk, 1, dk, dsc, nullptr, dcoef, da, du, nullptr));
            r = {down(dcoef, c0.size()), down(da, v0.size()), down(du, v0.size())};
        } else {
            double* dys = up(ys0);
            double* da = up(v0);
            double* du = up(v0);
            double* dl = up(v0);
            double* dg = up(dvec(P + GUARD, 0.25));
            LAUNCH(op_ycoef(P, dpart, nblk, 0, 1, 0.0, dys, da, du, dl, dg));
            r = {down(dys, ys0.size()), down(da, v0.size()), down(du, v0.size()), down(dl, v0.size())};
        }
        return r;
    });
    const ld_t gk = gam((ld_t)nblk + 6);
    for (int p = 0; p < P; ++p) {
        ld_t s[3], a[3];
        for (int q = 0; q < (which == 1 ? 1 : 3); ++q) slot_ref(part, nblk, q * P + p, s[q], a[q]);
        if (which == 0) {
            c.value(ex, "k2s[0]", p, o[0][p], s[0], gk * a[0]);
            c.value(ex, "k2s[1]", p, o[0][P + p], s[1], gk * a[1]);
            c.value(ex, "k2s[2]", p, o[0][2 * P + p], s[2], gk * a[2]);
            c.same("k2s[3] (rotated)", p, o[0][3 * P + p], k2s0[p]);
            c.bounded("t_low", p, o[2][p], sqrtl((ld_t)o[0][p]), U * sqrtl((ld_t)o[0][p]));
            const ld_t inv = 1.0L / sqrtl((ld_t)o[0][p]);
            if (o[0][p] >= 1.0) c.bounded("scale_next", p, o[1][p], inv, gam(2) * inv);
        } else if (which == 1) {
            c.value(ex, "coef[1] = 2 g1", p, o[0][P + p], 2.0L * s[0], 2.0L * gk * a[0]);
            c.exact("coef[0]", p, o[0][p], 0.0);
            c.same("t_alpha", p, o[1][p], o[0][P + p]);
            c.same("t_up", p, o[2][p], o[0][p]);
        } else {
            c.value(ex, "alpha = d0", p, o[1][p], s[0], gk * a[0]);
            c.value(ex, "ys[4] = d1", p, o[0][4 * P + p], s[1], gk * a[1]);
            c.value(ex, "ys[3] = d2", p, o[0][3 * P + p], s[2], gk * a[2]);
        }
    }
    if (which == 0) {
        c.written("k2s", k2s0, o[0], 4 * P);
        c.written("scale_next", v0, o[1], P);
        c.written("t_low", v0, o[2], P);
    } else if (which == 1) {
        c.written("coef", c0, o[0], 2 * P);
        c.written("t_alpha", v0, o[1], P);
        c.written("t_up", v0, o[2], P);
    } else {
        c.written("ys", ys0, o[0], 9 * P);
        for (int k = 1; k < 4; ++k) c.written("record", v0, o[k], P);
    }
}

// launch_coef_cgs2's scalar step (nblk = 1: g1 is the partial itself) against
// the documented expressions in long double; a term passes through at most 7
// roundings (gamma_8 times the sum of the terms' absolute values)
static void cgs2_formula_case(int P, int first, bool with_hist) {
    Case c(G_COEF, "cgs2_formula", fmt("P=%d first=%d hist=%d", P, first, (int)with_hist));
    if (g_list) return;
    const dvec part = make_partials(P, 1, NORMAL);
    dvec k2s = sentinels(4 * P), sc = block(P, NORMAL), sp = block(P, NORMAL);
    for (int t = 0; t < 4 * P; ++t) k2s[t] = (first && t >= P) ? NAN : rnormal();  // first: only ||u_cur||^2 is read
    if (first) std::fill(sp.begin(), sp.end(), NAN);
    const dvec v0 = sentinels(P), c0 = sentinels(2 * P);
    auto o = run_twice(c, [&] {
        g_work.off = 0;
        const double* dpart = up(part);
        const double* dk = up(k2s);
        const double* dsc = up(sc);
        const double* dsp = up(sp);
        double* dcoef = up(c0);
        double* da = up(v0);
        double* du = up(v0);
        double* dh = up(v0);
        LAUNCH(op_coef_cgs2(P, dpart, 1, first, dk, dsc, dsp, dcoef, da, du, with_hist ? dh : nullptr));
        return std::vector<dvec>{down(dcoef, c0.size()), down(da, v0.size()), down(du, v0.size()), down(dh, v0.size())};
    });
    c.written("coef", c0, o[0], 2 * P);
    c.written("t_alpha", v0, o[1], P);
    c.written("t_up", v0, o[2], P);
    if (with_hist) c.written("hist", v0, o[3], P);
    else c.unchanged("hist", v0, o[3]);
    for (int p = 0; p < P; ++p) {
        const ld_t g1 = part[p], s = sc[p], G11 = s * s * (ld_t)k2s[p];
        ld_t g0 = 0.0L, G00 = 0.0L, G01 = 0.0L;
        if (!first) {
            g0 = s * (ld_t)k2s[P + p];
            G01 = (ld_t)sp[p] * s * (ld_t)k2s[2 * P + p];
            G00 = (ld_t)sp[p] * (ld_t)sp[p] * (ld_t)k2s[3 * P + p];
        }
        const ld_t r0 = g0 + (g0 - (G00 * g0 + G01 * g1)), r1 = g1 + (g1 - (G01 * g0 + G11 * g1));
        const ld_t m0 = 2.0L * fabsl(g0) + fabsl(G00 * g0) + fabsl(G01 * g1);
        const ld_t m1 = 2.0L * fabsl(g1) + fabsl(G01 * g0) + fabsl(G11 * g1);
        c.bounded("coef[0]", p, o[0][p], r0, gam(8) * m0);
        c.bounded("coef[1]", p, o[0][P + p], r1, gam(8) * m1);
        c.same("t_alpha", p, o[1][p], o[0][P + p]);
        c.same("t_up", p, o[2][p], o[0][p]);
        if (with_hist) c.same("hist", p, o[3][p], sc[p]);
    }
}

// k_norm's threshold: beta < 1e-8 -> scale 0 (beta is still recorded)
static void norm_lucky_case(int P) {
    Case c(G_COEF, "norm_lucky_threshold", fmt("P=%d", P));
    if (g_list) return;
    dvec part = sentinels(3 * P);
    for (int p = 0; p < 3 * P; ++p) part[p] = p < P ? ((p & 1) ? 4e-16 : 1e-18) : 1.0;
    const dvec k2s0 = dvec(4 * P + GUARD, 2.0), v0 = sentinels(P);
    auto o = run_twice(c, [&] {
        g_work.off = 0;
        const double* dpart = up(part);
        double* dk = up(k2s0);
        double* dsn = up(v0);
        double* dlow = up(v0);
        LAUNCH(op_norm(P, dpart, 1, dk, dsn, dlow));
        return std::vector<dvec>{down(dsn, v0.size()), down(dlow, v0.size())};
    });
    c.written("scale_next", v0, o[0], P);
    c.written("t_low", v0, o[1], P);
    for (int p = 0; p < P; ++p) {
        const ld_t beta = sqrtl((ld_t)part[p]);
        c.bounded("t_low", p, o[1][p], beta, U * beta);
        if (p & 1) c.bounded("scale_next", p, o[0][p], 1.0L / beta, gam(2) / beta);
        else c.same("scale_next (lucky)", p, o[0][p], 0.0);
    }
}

// launch_ycoef's scalar step at nblk = 1 against the documented expressions in
// long double, the rounding errors propagated to first order with their
// second-order terms kept.  variant: 0 start, 1 ordinary, 2 last (guard left
// alone), 3 ordinary with guard below the ratio (the running minimum stays),
// 4 negative beta^2 (clamped: beta = 0, inv = 0), 5 start with 0 / 0 (NaN
// guard), 6 ordinary on a NaN guard (it sticks)
static void ycoef_formula_case(int P, int variant) {
    static const char* vn[] = {"ycoef_start", "ycoef_ordinary", "ycoef_last", "ycoef_guard_min",
                               "ycoef_negative_clamp", "ycoef_nan_ratio", "ycoef_nan_sticks"};
    Case c(G_COEF, vn[variant], fmt("P=%d", P));
    if (g_list) return;
    const int start = variant == 0 || variant == 5, last = variant == 2;
    const double s0 = 0.37;
    dvec part = sentinels(3 * P), ys0 = sentinels(9 * P), g0 = sentinels(P);
    for (int p = 0; p < P; ++p) {
        const double aj = rnormal(), bj = 0.5 + fabs(rnormal()), am1 = rnormal(), nyj = 1.0 + fabs(rnormal());
        const double ydj = rnormal(), b1 = 0.5 + fabs(rnormal());
        const double vals[9] = {aj, bj, am1, nyj, ydj, b1, NAN, NAN, NAN};
        for (int k = 0; k < 9; ++k) ys0[k * P + p] = start ? NAN : vals[k];
        part[p] = rnormal();
        part[P + p] = rnormal();
        // beta_next^2 = d2 - alpha^2 - beta^2: d2 chosen so that it is about 0.6 d2 (variant 4: negative)
        ld_t an;
        if (start) an = (ld_t)part[P + p] * s0;
        else an = ((ld_t)part[p] - 2.0L * aj * nyj - 2.0L * bj * ydj + (ld_t)aj * aj * aj + 2.0L * aj * bj * bj + (ld_t)bj * bj * am1) / ((ld_t)b1 * b1);
        const ld_t base = an * an + (start ? 0.0L : (ld_t)b1 * b1);
        part[2 * P + p] = variant == 4 ? (double)(0.5L * base) : (double)(2.5L * base + 1.0L);
        if (variant == 5) part[P + p] = part[2 * P + p] = 0.0;
        g0[p] = variant == 3 ? 0.25 : variant == 6 ? NAN : start ? SENT : 0.9;
    }
    const dvec v0 = sentinels(P);
    auto o = run_twice(c, [&] {
        g_work.off = 0;
        const double* dpart = up(part);
        double* dys = up(ys0);
        double* da = up(v0);
        double* du = up(v0);
        double* dl = up(v0);
        double* dg = up(g0);
        LAUNCH(op_ycoef(P, dpart, 1, start, last, s0, dys, da, du, dl, dg));
        return std::vector<dvec>{down(dys, ys0.size()), down(da, v0.size()), down(du, v0.size()), down(dl, v0.size()),
                                 down(dg, g0.size())};
    });
    c.written("ys", ys0, o[0], 9 * P);
    c.written("t_alpha", v0, o[1], P);
    c.written("t_up", v0, o[2], P);
    c.written("t_low", v0, o[3], P);
    for (size_t t = P; t < g0.size(); ++t) c.same("guard's guard", (long)t, o[4][t], SENT);
    const dvec& ys = o[0];
    for (int p = 0; p < P; ++p) {
        const ld_t d0 = part[p], d1 = part[P + p], d2 = part[2 * P + p];
        ld_t an, e_an, bn, b1sq;
        if (start) {
            an = d1 * (ld_t)s0;
            e_an = U * fabsl(an);
            bn = 0.0L;
            b1sq = 0.0L;
            c.same("ys[1]", p, ys[P + p], 0.0);
            c.same("ys[2]", p, ys[2 * P + p], 0.0);
            c.same("ys[4]", p, ys[4 * P + p], 0.0);
        } else {
            const ld_t aj = ys0[p], bj = ys0[P + p], am1 = ys0[2 * P + p], nyj = ys0[3 * P + p], ydj = ys0[4 * P + p];
            bn = ys0[5 * P + p];
            b1sq = bn * bn;
            const ld_t T[6] = {d0, -2.0L * aj * nyj, -2.0L * bj * ydj, aj * aj * aj, 2.0L * aj * bj * bj, bj * bj * am1};
            ld_t num = 0.0L, ab = 0.0L;
            for (ld_t t : T) {
                num += t;
                ab += fabsl(t);
            }
            an = num / b1sq;
            e_an = gam(11) * ab / b1sq;  // <= 3 products, 5 additions, beta^2 and the division per term
            c.same("ys[1] = beta_j+1", p, ys[P + p], ys0[5 * P + p]);
            c.same("ys[2] = alpha_j", p, ys[2 * P + p], ys0[p]);
            c.same("ys[4] = d1", p, ys[4 * P + p], part[P + p]);
        }
        c.bounded("alpha", p, ys[p], an, e_an);
        c.same("t_alpha", p, o[1][p], ys[p]);
        c.same("t_up", p, o[2][p], (double)bn);
        c.same("ys[3] = d2", p, ys[3 * P + p], part[2 * P + p]);
        c.same("t_low", p, o[3][p], ys[5 * P + p]);
        const ld_t sq = d2 - an * an - b1sq;
        const ld_t e_sq = gam(4) * (fabsl(d2) + an * an + b1sq) + (2.0L * fabsl(an) + e_an) * e_an;
        if (variant == 5) {  // 0 - 0: beta = 0, inv = 0, guard = 0 / 0
            c.same("beta_next", p, ys[5 * P + p], 0.0);
            c.same("inv", p, ys[6 * P + p], 0.0);
            if (!std::isnan(o[4][p])) c.fail("guard (0 / 0)", p, o[4][p], NAN, 0.0, INFINITY);
            continue;
        }
        const ld_t ratio = sq / d2, e_ratio = e_sq / fabsl(d2) + U * (fabsl(ratio) + e_sq / fabsl(d2));
        if (variant == 4) {
            c.same("beta_next (clamped)", p, ys[5 * P + p], 0.0);
            c.same("inv (clamped)", p, ys[6 * P + p], 0.0);
            c.exact("a next", p, ys[7 * P + p], 0.0);
            c.exact("b next", p, ys[8 * P + p], 0.0);
            c.bounded("guard (negative ratio)", p, o[4][p], ratio, e_ratio);
            continue;
        }
        const ld_t b = sqrtl(sq), e_b = e_sq / b + U * (b + e_sq / b);
        c.bounded("beta_next", p, ys[5 * P + p], b, e_b);
        const ld_t inv = 1.0L / b, e_inv = e_b / (b * (b - e_b)) + U / (b - e_b);
        c.bounded("inv", p, ys[6 * P + p], inv, e_inv);
        const ld_t hi7 = (fabsl(an) + e_an) * (inv + e_inv);
        c.bounded("a next", p, ys[7 * P + p], an * inv, hi7 - fabsl(an) * inv + U * hi7);
        c.bounded("b next", p, ys[8 * P + p], bn * inv, fabsl(bn) * e_inv + U * fabsl(bn) * (inv + e_inv));
        // the guard: ratio is about 0.6 by construction
        if (variant == 2) c.same("guard (last: left alone)", p, o[4][p], g0[p]);
        else if (variant == 3) c.same("guard (running minimum)", p, o[4][p], 0.25);
        else if (variant == 6) {
            if (!std::isnan(o[4][p])) c.fail("guard (NaN sticks)", p, o[4][p], NAN, 0.0, INFINITY);
        } else c.bounded("guard", p, o[4][p], ratio, e_ratio);
    }
}

static void grp_coef() {
    for (int P : kWidths) {
        for (int nblk : kNblk)
            for (int kind = 0; kind < 2; ++kind)
                for (int which = 0; which < 3; ++which) reduce_case(P, nblk, kind, which);
        for (int first = 0; first < 2; ++first)
            for (int h = 0; h < 2; ++h) cgs2_formula_case(P, first, h != 0);
        norm_lucky_case(P);
        for (int v = 0; v < 7; ++v) ycoef_formula_case(P, v);
    }
}

// ---------------------------------------------------------------------------
// contract: the bit-for-bit statements of kt_kernels.hip / kt_launch.h, on
// normal inputs (where a different evaluation order would show)
// ---------------------------------------------------------------------------
static void contract_case(const char* name, const Shape& S, int P, const std::string& what,
                          const std::function<std::vector<dvec>()>& a, const std::function<std::vector<dvec>()>& b,
                          size_t ncmp) {
    Case c(G_CONTRACT, name, fmt("%s P=%d %s", S.tag, P, what.c_str()));
    if (g_list || g_host) return;  // a statement about the device code
    const std::vector<dvec> oa = a(), ob = b();
    for (size_t k = 0; k < ncmp; ++k) {
        if (oa[k].size() != ob[k].size()) c.fail("sizes", (long)k, (double)oa[k].size(), (double)ob[k].size(), 0.0);
        else
            for (size_t t = 0; t < oa[k].size(); ++t)
                c.same(k == 0 ? "output" : k == 1 ? "partial" : "third output", (long)t, oa[k][t], ob[k][t]);
    }
}

static void grp_contract() {
    for (int P : kWidths) {
        const std::vector<Shape> shapes = shapes_for(P);
        for (const Shape& S : {shapes[0], shapes[2]}) {
            const Inputs* Ip = g_list ? nullptr : &inputs(*S.G, P, NORMAL);
            auto pass = [&, Ip](int flags, int xsrc, int ysrc, int bcols, bool gate) {
                return [=, &S]() {
                    PassCfg cfg;
                    cfg.flags = flags;
                    cfg.xsrc = xsrc;
                    cfg.ysrc = ysrc;
                    cfg.bcols = bcols;
                    cfg.vo = bcols > 0;
                    cfg.gate = gate;
                    return run_pass(S, *Ip, cfg);
                };
            };
            auto start = [&, Ip](int flags) { return [=, &S]() { return run_start(S, *Ip, flags); }; };
            auto first = [&, Ip](int flags, bool gate) { return [=, &S]() { return run_first(S, *Ip, flags, gate); }; };
            auto dot = [&, Ip](int flags) { return [=, &S]() { return run_dot(S, *Ip, flags); }; };
            // (a) NT, NTY and SC1 are cache hints
            static const int dotp[5][2] = {{F_NT, 0}, {F_NT | F_UNIT, F_UNIT}, {F_NTY | F_UNIT, F_UNIT},
                                           {F_NT | F_NTY | F_UNIT, F_UNIT}, {F_MLP | F_NTY | F_UNIT, F_MLP | F_UNIT}};
            for (auto& q : dotp) contract_case("a_cache_hints", S, P, fmt("spmm_dot %d vs %d", q[0], q[1]), dot(q[0]), dot(q[1]), 2);
            for (int u : {0, (int)F_UNIT})
                for (int h : {(int)F_NTY, (int)F_SC1}) {
                    contract_case("a_cache_hints", S, P, fmt("lanczos_pass %d vs %d", u | h, u), pass(u | h, 0, 1, 0, false),
                                  pass(u, 0, 1, 0, false), 2);
                    contract_case("a_cache_hints", S, P, fmt("lanczos_start %d vs %d", u | h, u), start(u | h), start(u), 2);
                }
            for (int h : {(int)F_NTY, (int)F_SC1}) {
                contract_case("a_cache_hints", S, P, fmt("lanczos_pass I16 %d vs plain", h),
                              pass(F_UNIT | F_I16 | h, 0, 2, 0, false), pass(F_UNIT | F_I16, 0, 2, 0, false), 2);
                contract_case("a_cache_hints", S, P, fmt("lanczos_first %d vs plain", h), first(F_UNIT | h, false),
                              first(F_UNIT, false), 2);
            }
            // (b) the first step on the table T is the ordinary step on X = s0 * (double)T
            contract_case("b_first_is_pass", S, P, "lanczos_first vs lanczos_pass(X = s0 T, UNIT, no Yold)",
                          first(F_UNIT, false), pass(F_UNIT, 1, 0, 0, false), 2);
            // (c) the I16 second step is the fp64 step with Yold = s0 * (double)T
            contract_case("c_i16_second_step", S, P, "lanczos_pass I16 vs UNIT with Yold = s0 T",
                          pass(F_UNIT | F_I16, 0, 2, 0, false), pass(F_UNIT, 0, 3, 0, false), 2);
            // (d) the fp64 start pass stores s0 * (double) of the I16 start pass's table; same partials
            contract_case("d_start_table", S, P, "lanczos_start UNIT vs s0 * table of I16", start(F_UNIT), [=, &S]() {
                std::vector<dvec> o = run_start(S, *Ip, F_UNIT | F_I16);
                for (size_t t = 0; t < (size_t)Ip->n * P; ++t) o[0][t] = Ip->s0 * o[0][t];
                for (size_t t = (size_t)Ip->n * P; t < o[0].size(); ++t) o[0][t] = SENT;
                return o;
            }, 2);
            // (e) a gated-open launch equals the ungated launch of the same form
            contract_case("e_gate_open", S, P, "lanczos_pass gate:0 vs NTY", pass(0, 0, 1, 0, true), pass(F_NTY, 0, 1, 0, false), 2);
            contract_case("e_gate_open", S, P, "lanczos_pass gate:UNIT vs UNIT|NTY", pass(F_UNIT, 0, 1, 0, true),
                          pass(F_UNIT | F_NTY, 0, 1, 0, false), 2);
            contract_case("e_gate_open", S, P, "lanczos_pass gate:I16 vs I16|NTY", pass(F_UNIT | F_I16, 0, 2, 0, true),
                          pass(F_UNIT | F_I16 | F_NTY, 0, 2, 0, false), 2);
            contract_case("e_gate_open", S, P, "lanczos_first gate vs UNIT|NTY", first(F_UNIT, true), first(F_UNIT | F_NTY, false), 2);
            // (f) forming the basis does not change Out or the partials
            for (int fl : {0, (int)F_UNIT, (int)F_SC1, (int)(F_UNIT | F_SC1)})
                contract_case("f_basis_keeps_out", S, P, fmt("lanczos_pass Vn:%d vs %d", fl, fl), pass(fl, 0, 1, P, false),
                              pass(fl, 0, 1, 0, false), 2);
            for (int fl : {0, (int)F_UNIT})
                contract_case("f_basis_keeps_out", S, P, fmt("quadform Vn:%d vs %d", fl, fl),
                              [=, &S]() { return run_quad(S, *Ip, fl, P, true); },
                              [=, &S]() { return run_quad(S, *Ip, fl, 0, false); }, 1);
        }
        // (e) for the coefficient step: the gated form of launch_ycoef with a running word set
        for (int start = 0; start < 2; ++start) {
            const int nblk = 130;
            auto ycoef = [=](bool gate) {
                return [=]() {
                    g_rng = 0x9E3779B97F4A7C15ull + (uint64_t)P * 2 + start;  // the same inputs for both launches
                    dvec part = make_partials(3 * P, nblk, NORMAL), ys = sentinels(9 * P);
                    for (int t = 0; t < 9 * P; ++t) ys[t] = 0.5 + fabs(rnormal());
                    for (int p = 0; p < P; ++p)
                        for (int b = 0; b < nblk; ++b) part[(size_t)(2 * P + p) * nblk + b] = 50.0 + fabs(part[(size_t)(2 * P + p) * nblk + b]);
                    g_work.off = 0;
                    const double* dpart = up(part);
                    double* dys = up(ys);
                    double* drec = up(sentinels(3 * P));
                    double* dg = up(dvec(P + GUARD, 0.75));
                    const int* dgate = up(ivec{0, 0, 4});
                    LAUNCH(op_ycoef(P, dpart, nblk, start, 0, 0.37, dys, drec, drec + P, drec + 2 * P, dg,
                                    gate ? dgate : nullptr, gate ? 3 : 0));
                    return std::vector<dvec>{down(dys, ys.size()), down(drec, 3 * P + GUARD), down(dg, P + GUARD)};
                };
            };
            contract_case("e_gate_open", shapes[0], P, fmt("ycoef gated vs ungated start=%d", start), ycoef(true), ycoef(false), 3);
        }
    }
}

// ---------------------------------------------------------------------------
static const char* kMutations[] = {"dot_drop_last_mod4", "pass_skip_long_plus1",  "start_val_shift",
                                   "pass_no_yold",       "quad_no_diag",          "quad_prefix_off_by_one",
                                   "block_drop_last_chunk", "ycoef_guard_overwrite", "reduce_round_down_64",
                                   "start_sign_bit_p1",  "vb_write_bcols",        "quad_vb_write_bcols",
                                   "first_ignore_alpha", "update_reads_uprev_on_first", "probes_ignore_perm"};

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
                fprintf(stderr, "sweep_check: unknown group %s\n", argv[a] + 8);
                return 2;
            }
        } else {
            fprintf(stderr, "usage: sweep_check [--host [--mutate=NAME]] [--count] [--group=NAME] [--small]\n");
            return 2;
        }
    }
    if (!g_mut.empty()) {
        bool known = false;
        for (const char* m : kMutations) known = known || g_mut == m;
        if (!known || !g_host) {
            fprintf(stderr, "sweep_check: --mutate needs --host and one of:");
            for (const char* m : kMutations) fprintf(stderr, " %s", m);
            fprintf(stderr, "\n");
            return 2;
        }
    }
    if (g_small) kWidths = {1, 4, 32};
    if (!g_host) {
        hipDeviceProp_t prop;
        HC(hipGetDeviceProperties(&prop, 0));
    }
    if (!g_list) {
        g_keep.init((size_t)96 << 20);
        g_work.init((size_t)32 << 20);
    }
    graphs_init();
    void (*const groups[NG])() = {grp_probes, grp_dot,  grp_block, grp_pass,   grp_start,
                                  grp_first,  grp_quad, grp_coef,  grp_update, grp_contract};
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
