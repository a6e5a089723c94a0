// block_check -- the block Gram-Schmidt and streaming kernels called one by
// one through their kt::launch_* entry points (kt_launch.h), each result
// compared with a host reference in long double (or in exact integers).
//
// Groups: gram, combine, chol_rinv, fro_colmax_scale, colbatch, streaming.
// Three kinds of assertion:
//   exact    small-integer inputs (|v| <= 8): every product and partial sum is
//            exact in fp64 in any order, with or without fma, so the result
//            must equal the reference (compared by value; the sign of a zero
//            sum is not pinned).  A dropped, doubled or misplaced term cannot
//            hide.
//   bounded  standard-normal inputs against a componentwise a-priori bound,
//            u = 2^-53, gamma_k = k u / (1 - k u); nothing is tuned to the
//            kernels.
//   contract pure moves and the documented evaluation orders, bit for bit.
// Input blocks have ld > columns with NaN in the padding; output blocks carry
// sentinels in their padding and in a guard region after the last element,
// which must come back unchanged.  On the device every case runs twice and
// the two outputs must agree bit for bit.
//
//   block_check                     run on the GPU
//   block_check --host              the same cases with every device call
//                                   replaced by a plain fp64 host loop (no GPU)
//   block_check --host --mutate=M   one deliberate defect in the host stand-in;
//                                   the matching group must report failures
//   block_check --count             the case counts alone (nothing is run)
//   --group=NAME runs one group; --small leaves out gram's n >= 8192 (both for
//   quick --mutate runs)
//
// Prints one JSON line; exit status 0 iff no case failed, 3 on a HIP error
// (nothing is launched after it), 2 on bad usage.
// Build: make -C tests/native/block_check (links the library's own objects).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../../krylov_robustness_amd/csrc/kt_launch.h"

typedef long double ld_t;
typedef std::vector<double> dvec;

static bool g_host = false;
static bool g_list = false;   // --count: enumerate the cases, run nothing
static bool g_small = false;  // --small: leave out gram's n >= 8192 (quick --mutate runs)
static int g_only = -1;       // --group=NAME: that group alone
static std::string g_mut;
static int g_num_cu = 256;  // --host: the MI355X's count, so both modes enumerate the same cases
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
    long cases, nfail;
    std::vector<Fail> fails;
    double seconds = 0.0, run_seconds = 0.0;  // the rest is input generation, references and checks
};
enum { G_GRAM, G_COMBINE, G_CHOL, G_FRO, G_COL, G_STREAM, NG };
static Group g_groups[NG] = {{"gram", 0, 0, {}},     {"combine", 0, 0, {}},  {"chol_rinv", 0, 0, {}},
                             {"fro_colmax_scale", 0, 0, {}}, {"colbatch", 0, 0, {}}, {"streaming", 0, 0, {}}};
static std::chrono::steady_clock::time_point g_t0;

static std::string fmt(const char* f, ...) {
    char buf[256];
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

static void print_report(const char* hip_err) {
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - g_t0).count();
    long nfail = 0;
    for (int g = 0; g < NG; ++g) nfail += g_groups[g].nfail;
    printf("{\"block_check\": \"%s\", \"mode\": \"%s\", \"mutate\": \"%s\", \"num_cu\": %d, \"wall_s\": %.3f, ",
           hip_err ? "HIP_ERROR" : (nfail ? "FAIL" : "ok"), g_list ? "count" : (g_host ? "host" : "device"), g_mut.c_str(), g_num_cu,
           wall);
    if (hip_err) printf("\"hip_error\": \"%s\", ", hip_err);
    printf("\"groups\": {");
    for (int g = 0; g < NG; ++g) {
        const Group& G = g_groups[g];
        printf("%s\"%s\": {\"cases\": %ld, \"seconds\": %.3f, \"run_seconds\": %.3f, \"failed_count\": %ld, \"failed\": [", g ? ", " : "",
               G.name, G.cases, G.seconds, G.run_seconds, G.nfail);
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
#define HC(x)                                     \
    do {                                          \
        hipError_t e_ = (x);                      \
        if (e_ != hipSuccess) hip_die(#x, e_);    \
    } while (0)
// a launcher call, then (device) the stream drained so that an error belongs to this case
#define LAUNCH(x)                                   \
    do {                                            \
        HC(x);                                      \
        if (!g_host) HC(hipDeviceSynchronize());    \
    } while (0)

static uint64_t bits_of(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}

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
        if (!(e <= bound)) fail(what, idx, (double)got, (double)ref, (double)bound, (double)(e / bound));
    }
    // everything of a (rows + guard) x ld block outside the live rows x cols is unchanged
    void untouched(const char* what, const dvec& before, const dvec& after, int64_t rows, int cols, int ld) {
        for (size_t t = 0; t < before.size(); ++t) {
            const int64_t r = (int64_t)(t / ld);
            const int c = (int)(t % ld);
            if (r < rows && c < cols) continue;
            same(what, (long)t, after[t], before[t]);
        }
    }
    // tight arrays: elements from `count` on are unchanged
    void guard(const char* what, const dvec& before, const dvec& after, size_t count) {
        for (size_t t = count; t < before.size(); ++t) same(what, (long)t, after[t], before[t]);
    }
    void repeat(const std::vector<dvec>& a, const std::vector<dvec>& b) {
        for (size_t k = 0; k < a.size(); ++k)
            for (size_t t = 0; t < a[k].size(); ++t)
                if (bits_of(a[k][t]) != bits_of(b[k][t])) fail("second run differs", (long)t, b[k][t], a[k][t], 0.0, INFINITY);
    }
};

static double g_run_s = 0.0;  // uploads, the operation under test (twice on the device), downloads
template <class F>
static std::vector<dvec> run_twice(Case& c, F exec) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<dvec> o = exec();
    if (!g_host) c.repeat(o, exec());
    g_run_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return o;
}

// ---------------------------------------------------------------------------
// memory: one arena (device memory, or host memory with --host), used as a stack
// ---------------------------------------------------------------------------
static char* g_arena = nullptr;
static size_t g_cap = 0, g_off = 0;
static void arena_init(size_t cap) {
    g_cap = cap;
    if (g_host) {
        g_arena = (char*)malloc(cap);
        if (!g_arena) exit(2);
    } else {
        HC(hipMalloc((void**)&g_arena, cap));
    }
}
static size_t arena_mark() { return g_off; }
static void arena_release(size_t m) { g_off = m; }
template <class T>
static T* up(const std::vector<T>& h) {
    const size_t b = h.size() * sizeof(T);
    T* p = (T*)(g_arena + g_off);
    if (g_off + b > g_cap) {
        fprintf(stderr, "block_check: arena too small\n");
        exit(2);
    }
    g_off += (b + 255) / 256 * 256;
    if (b) {
        if (g_host)
            memcpy(p, h.data(), b);
        else
            HC(hipMemcpy(p, h.data(), b, hipMemcpyHostToDevice));
    }
    return p;
}
template <class T>
static std::vector<T> down(const T* p, size_t n) {
    std::vector<T> h(n);
    if (n) {
        if (g_host)
            memcpy(h.data(), p, n * sizeof(T));
        else
            HC(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    }
    return h;
}
static dvec to_d(const std::vector<int>& v) { return dvec(v.begin(), v.end()); }

// ---------------------------------------------------------------------------
// data
// ---------------------------------------------------------------------------
static const double SENT = -7.7777e77;
static const size_t GUARD = 67;
static const ld_t U = ldexpl(1.0L, -53);
static ld_t gam(ld_t k) { return k * U / (1.0L - k * U); }

static uint64_t g_rng = 88172645463325252ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static double rint8() { return (double)((int)(rnd() % 17) - 8); }
// Two pools of 2^20 values, integers in [-8, 8] and standard normals
// (Box-Muller); blocks are filled with runs of a pool that start at random offsets.
static const size_t kPool = (size_t)1 << 20, kRun = 256;
static dvec g_pool[2];
enum Kind { INT8 = 0, NORMAL = 1 };
static void pool_init() {
    g_pool[INT8].resize(kPool);
    g_pool[NORMAL].resize(kPool);
    for (size_t i = 0; i < kPool; ++i) g_pool[INT8][i] = rint8();
    for (size_t i = 0; i < kPool; i += 2) {
        const double u1 = ((rnd() >> 11) + 1.0) * (1.0 / 9007199254740993.0);
        const double u2 = (rnd() >> 11) * (1.0 / 9007199254740992.0);
        const double r = sqrt(-2.0 * log(u1));
        g_pool[NORMAL][i] = r * cos(6.283185307179586 * u2);
        g_pool[NORMAL][i + 1] = r * sin(6.283185307179586 * u2);
    }
}
static void fill(double* dst, size_t count, int kind) {
    while (count) {
        const size_t m = std::min(count, kRun);
        memcpy(dst, g_pool[kind].data() + rnd() % (kPool - kRun), m * sizeof(double));
        dst += m;
        count -= m;
    }
}

// (rows + guard_rows) x ld, live rows x cols drawn from `kind`, everything else = pad
static dvec mk(int64_t rows, int cols, int ld, int kind, double pad, int guard_rows) {
    dvec v((size_t)(rows + guard_rows) * ld, pad);
    for (int64_t r = 0; r < rows; ++r) fill(v.data() + (size_t)r * ld, cols, kind);
    return v;
}
static dvec mk1(size_t count, int kind, size_t guard) {
    dvec v(count + guard, SENT);
    fill(v.data(), count, kind);
    return v;
}
static dvec sentinels(size_t count) { return dvec(count + GUARD, SENT); }

// The host work of the large cases (references, the gram stand-in) split over a
// few threads: f(r0, r1, t) takes rows [r0, r1) as part t (at most kMaxThreads
// parts of at least `grain` rows).
static const int kMaxThreads = 16;
template <class F>
static int par_rows(int64_t n, int64_t grain, F f) {
    const int hw = (int)std::thread::hardware_concurrency();
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(kMaxThreads, hw > 0 ? hw : 1), n / grain));
    if (T == 1) {
        f((int64_t)0, n, 0);
        return 1;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(f, n * t / T, n * (t + 1) / T, t);
    for (auto& x : th) x.join();
    return T;
}

// ---------------------------------------------------------------------------
// the operations: the launcher, or its fp64 host stand-in
// ---------------------------------------------------------------------------
static int64_t gram_rows_host(int64_t n) {
    const int64_t r = (n + 255) / 256;
    return r < 128 ? 128 : (r + 15) / 16 * 16;
}

static hipError_t op_gram(int64_t n, const double* X, int ldx, int px, const double* Y, int ldy, int py, double* part,
                          double* G) {
    if (!g_host) return kt::launch_gram_ts(n, X, ldx, px, Y, ldy, py, part, G, 0);
    const int64_t rows = gram_rows_host(n);
    const int S = (int)((n + rows - 1) / rows);
    const int64_t nn = mut("gram_drop_last_row") ? n - 1 : n;
    const bool skip32 = mut("gram_skip_col32");
    const size_t count = (size_t)px * py;
    const int Ssum = (mut("gram_drop_slab") && S > 1) ? S - 1 : S;
    par_rows(S, 16, [&](int64_t s0, int64_t s1, int) {  // the slabs are independent
        for (int64_t s = s0; s < s1; ++s) {
            double* slab = part + s * count;
            for (size_t t = 0; t < count; ++t) slab[t] = 0.0;
            const int64_t r1 = std::min<int64_t>(nn, (s + 1) * rows);
            for (int64_t r = s * rows; r < r1; ++r)
                for (int j = 0; j < py; ++j) {
                    const double y = Y[r * ldy + j];
                    double* col = slab + (size_t)j * px;
                    const double* xr = X + r * ldx;
                    for (int i = 0; i < px; ++i) col[i] += xr[i] * y;
                }
            if (skip32 && px > 32)
                for (int j = 0; j < py; ++j) slab[32 + (size_t)j * px] = 0.0;
        }
    });
    for (size_t t = 0; t < count; ++t) {
        double s = 0.0;
        for (int q = 0; q < Ssum; ++q) s += part[q * count + t];
        G[t] = s;
    }
    return hipSuccess;
}

static hipError_t op_combine(int64_t n, const double* X, int ldx, int px, const double* C, int q, double alpha,
                             double beta, double* Y, int ldy) {
    if (!g_host) return kt::launch_combine_ts(n, X, ldx, px, C, q, alpha, beta, Y, ldy, 0);
    if (n <= 0 || q <= 0) return hipSuccess;
    if (q > 32) {
        const double* x1 = X + (n - 1) * (int64_t)ldx + px;
        const double* y1 = Y + (n - 1) * (int64_t)ldy + q;
        if (X < y1 && Y < x1) return hipErrorInvalidValue;
    }
    const bool rowwise = mut("combine_inplace_rowwise"), nobeta = mut("combine_ignore_beta");
    dvec xr(px), acc(q), Ct((size_t)px * q);
    for (int i = 0; i < px; ++i)
        for (int j = 0; j < q; ++j) Ct[(size_t)i * q + j] = C[i + (size_t)j * px];
    for (int64_t r = 0; r < n; ++r) {
        for (int i = 0; i < px; ++i) xr[i] = X[r * ldx + i];
        if (!rowwise) {  // all of X's row first, then the stores
            std::fill(acc.begin(), acc.end(), 0.0);
            for (int i = 0; i < px; ++i)
                for (int j = 0; j < q; ++j) acc[j] += xr[i] * Ct[(size_t)i * q + j];
            for (int j = 0; j < q; ++j) {
                const double y0 = (beta == 0.0 || nobeta) ? 0.0 : beta * Y[r * ldy + j];
                Y[r * ldy + j] = y0 + alpha * acc[j];
            }
            continue;
        }
        for (int j = 0; j < q; ++j) {
            double acc = 0.0;
            for (int i = 0; i < px; ++i) acc += X[r * ldx + i] * C[i + (size_t)j * px];  // X read live: the defect
            const double y0 = (beta == 0.0 || nobeta) ? 0.0 : beta * Y[r * ldy + j];
            Y[r * ldy + j] = y0 + alpha * acc;
        }
    }
    return hipSuccess;
}

static hipError_t op_chol(int bs, const double* G, double shift_coef, double* R, double* Rinv, int* ok) {
    if (!g_host) return kt::launch_chol_rinv(bs, G, shift_coef, R, Rinv, ok, 0);
    if (bs < 1 || bs > 64) return hipErrorInvalidValue;
    dvec A(G, G + bs * bs), X((size_t)bs * bs, 0.0);
    double tr = 0.0;
    for (int i = 0; i < bs; ++i) tr += A[i + i * bs];
    const double shift = mut("chol_no_shift") ? 0.0 : shift_coef * tr;
    for (int i = 0; i < bs; ++i) A[i + i * bs] += shift;
    int okv = 1;
    for (int j = 0; j < bs; ++j) {
        const double d = A[j + j * bs];
        if (!(d > 0.0)) okv = 0;
        const double r = A[j + j * bs] = sqrt(d > 0.0 ? d : 1.0);
        for (int q = j + 1; q < bs; ++q) A[j + q * bs] /= r;
        for (int q = j + 1; q < bs; ++q)
            for (int p = j + 1; p <= q; ++p) A[p + q * bs] -= A[j + p * bs] * A[j + q * bs];
    }
    for (int t = 0; t < bs * bs; ++t) R[t] = (t % bs) <= (t / bs) ? A[t] : 0.0;
    if (mut("chol_below_diag") && bs >= 2) R[1] = 0.5;
    for (int c = 0; c < bs; ++c) {
        double* x = X.data() + c * bs;
        x[c] = 1.0 / A[c + c * bs];
        for (int i = c - 1; i >= 0; --i) {
            double sm = 0.0;
            for (int k = i + 1; k <= c; ++k) sm = fma(A[i + k * bs], x[k], sm);
            x[i] = -sm / A[i + i * bs];
        }
    }
    for (int t = 0; t < bs * bs; ++t) Rinv[t] = X[t];
    ok[0] = okv;
    return hipSuccess;
}

static hipError_t op_fro(int n, double* M, double* out, double* colsq) {
    if (!g_host) return kt::launch_fro_colmax_scale(n, M, out, colsq, 0);
    if (n <= 0) return hipSuccess;
    double f = 0.0, m = 0.0;
    for (int j = 0; j < n; ++j) {
        double c = 0.0;
        for (int i = 0; i < n; ++i) c += M[i + (size_t)j * n] * M[i + (size_t)j * n];
        colsq[j] = c;
        f += c;
        m = std::max(m, c);
    }
    out[0] = f;
    out[1] = m;
    if (!(f > 0.0)) return hipSuccess;
    const double inv = 1.0 / sqrt(f);
    for (size_t t = 0; t < (size_t)n * n; ++t) M[t] *= inv;
    return hipSuccess;
}

static hipError_t op_col_dots(int n, int P, int nb, int64_t vstride, const double* V, const double* W, int r_lo,
                              int num_cu, double* part, double* out, int rpb_lo) {
    if (!g_host) return kt::launch_col_dots(n, P, nb, vstride, V, W, r_lo, num_cu, part, out, 0, rpb_lo);
    const int lo = mut("col_dots_ignore_r_lo") ? 0 : r_lo;
    const int nrb = kt::col_nrb(n, num_cu, rpb_lo);
    for (int k = 0; k < nb; ++k) {
        double* o = out + k * P;
        for (int c = 0; c < P; ++c) o[c] = 0.0;
        for (int r = lo; r < n; ++r)
            for (int c = 0; c < P; ++c) o[c] += V[k * vstride + (int64_t)r * P + c] * W[(int64_t)r * P + c];
        for (int c = 0; c < P; ++c)
            for (int b = 0; b < nrb; ++b) part[((int64_t)k * P + c) * nrb + b] = b ? 0.0 : o[c];
    }
    return hipSuccess;
}

static hipError_t op_col_update(int n, int P, int nb, int64_t vstride, const double* V, const double* h, double* W) {
    if (!g_host) return kt::launch_col_update(n, P, nb, vstride, V, h, W, 0);
    for (int64_t t = 0; t < (int64_t)n * P; ++t) {
        double s = 0.0;
        for (int k = 0; k < nb; ++k) s += V[k * vstride + t] * h[k * P + t % P];
        W[t] -= s;
    }
    return hipSuccess;
}

static hipError_t op_col_householder(int n, int P, const double* s, double* W, double* Q, double* r) {
    if (!g_host) return kt::launch_col_householder(n, P, s, W, Q, r, 0);
    for (int c = 0; c < P; ++c) {
        const double alpha = W[c], xx = s[c];
        double beta = alpha, tau = 0.0, scal = 1.0;
        if (xx != 0.0) {
            beta = -copysign(hypot(alpha, sqrt(xx)), alpha);
            tau = (beta - alpha) / beta;
            scal = 1.0 / (alpha - beta);
        }
        for (int row = n - 1; row >= 0; --row)
            Q[(int64_t)row * P + c] = row == 0 ? 1.0 - tau : -tau * (W[(int64_t)row * P + c] * scal);
        r[c] = beta;
    }
    return hipSuccess;
}

static hipError_t op_col_select(int C, int P, const int* idx, double* X) {
    if (!g_host) return kt::launch_col_select(C, P, idx, X, 0);
    for (int c = 0; c < C; ++c) X[(int64_t)idx[c] * P + c] = 1.0;
    return hipSuccess;
}

static hipError_t op_weighted_sum(int n, int m, int P, int nc, const double* Uu, int ldu, int64_t sstride,
                                  const double* W, double* Y, int ldy) {
    if (!g_host) return kt::launch_weighted_sum(n, m, P, nc, Uu, ldu, sstride, W, Y, ldy, 0);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < nc; ++c) {
            double s = 0.0;
            for (int j = 0; j < m; ++j) s = fma(Uu[(int64_t)r * ldu + j * sstride + c], W[j * P + c], s);
            Y[(int64_t)r * ldy + c] = s;
        }
    return hipSuccess;
}

static hipError_t op_perm_rows(int n, int cols, const int* perm, int gather, const double* src, int lds, double* dst,
                               int ldd) {
    if (!g_host) return kt::launch_perm_rows(n, cols, perm, gather, src, lds, dst, ldd, 0);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < cols; ++c) {
            if (gather)
                dst[(int64_t)r * ldd + c] = src[(int64_t)perm[r] * lds + c];
            else
                dst[(int64_t)perm[r] * ldd + c] = src[(int64_t)r * lds + c];
        }
    return hipSuccess;
}

static hipError_t op_axpby(int n, int nc, double a, const double* X, int ldx, double b, double* Y, int ldy) {
    if (!g_host) return kt::launch_axpby(n, nc, a, X, ldx, b, Y, ldy, 0);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < nc; ++c) {
            const double y = b == 0.0 ? 0.0 : b * Y[(int64_t)r * ldy + c];
            Y[(int64_t)r * ldy + c] = fma(a, X[(int64_t)r * ldx + c], y);
        }
    return hipSuccess;
}

static hipError_t op_inf_norm(int n, int nc, const double* X, int ldx, double* partial) {
    if (!g_host) return kt::launch_inf_norm(n, nc, X, ldx, partial, 0);
    const int nb = kt::inf_norm_blocks();
    for (int b = 0; b < nb; ++b) partial[b] = 0.0;
    for (int r = 0; r < n; ++r) {
        double s = 0.0;
        for (int c = 0; c < nc; ++c) s += fabs(X[(int64_t)r * ldx + c]);
        double& p = partial[(r / 256) % nb];
        p = std::max(p, s);
    }
    return hipSuccess;
}

static hipError_t op_normest1_y(int n, const double* Y, const double* Sprev, double* S, double* partial) {
    if (!g_host) return kt::launch_normest1_y(n, Y, Sprev, S, partial, 0);
    const int nb = kt::normest1_blocks(n);
    for (int b = 0; b < 2 * nb; ++b) partial[b] = 0.0;
    for (int r = 0; r < n; ++r) {
        double s = Y[r] < 0.0 ? -1.0 : 1.0;
        if (mut("normest1_sign0") && Y[r] == 0.0) s = 0.0;
        const int b = (r / 256) % nb;
        partial[b] += fabs(Y[r]);
        partial[nb + b] += Sprev[r] * s;
        S[r] = s;
    }
    return hipSuccess;
}

static void absmax_merge(double& v, int& i, double v2, int i2, bool largest) {
    if (v2 > v || (v2 == v && (largest ? i2 > i : i2 < i))) {
        v = v2;
        i = i2;
    }
}

static hipError_t op_absmax_idx(int n, const double* Z, double* pval, int* pidx) {
    if (!g_host) return kt::launch_absmax_idx(n, Z, pval, pidx, 0);
    const int nb = kt::normest1_blocks(n);
    const bool largest = mut("absmax_tie_largest");
    for (int b = 0; b < nb; ++b) {
        pval[b] = -1.0;
        pidx[b] = largest ? -1 : INT_MAX;
    }
    for (int r = 0; r < n; ++r) {
        const int b = (r / 256) % nb;
        absmax_merge(pval[b], pidx[b], fabs(Z[r]), r, largest);
    }
    return hipSuccess;
}

static hipError_t op_gather_rows(int nr, int cols, const double* D, int ldd, const int64_t* rows, double* out) {
    if (!g_host) return kt::launch_gather_rows(nr, cols, D, ldd, rows, out, 0);
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < nr; ++r) out[(int64_t)c * nr + r] = D[rows[r] * ldd + c];
    return hipSuccess;
}
static hipError_t op_gather_elems(int64_t count, const double* D, const int64_t* off, double* out) {
    if (!g_host) return kt::launch_gather_elems(count, D, off, out, 0);
    for (int64_t t = 0; t < count; ++t) out[t] = D[off[t]];
    return hipSuccess;
}
static hipError_t op_scatter_elems(int64_t count, const int64_t* off, const double* val, double* D) {
    if (!g_host) return kt::launch_scatter_elems(count, off, val, D, 0);
    for (int64_t t = 0; t < count; ++t) D[off[t]] = val[t];
    return hipSuccess;
}

static hipError_t op_sum_slabs(int count, int S, const double* part, double* G) {
    if (!g_host) return kt::launch_sum_slabs(count, S, part, G, 0);
    for (int t = 0; t < count; ++t) {
        double s = 0.0;
        for (int q = 0; q < S; ++q) s += part[(int64_t)q * count + t];
        G[t] = s;
    }
    return hipSuccess;
}

static hipError_t op_poly4(int n, double beta, const double* in, double c0, double c1, const double* X1, double c2,
                           const double* X2, double c3, const double* X3, double* out, int batch) {
    if (!g_host) return kt::launch_poly4(n, beta, in, c0, c1, X1, c2, X2, c3, X3, out, 0, batch);
    const int64_t total = (int64_t)n * n;
    for (int64_t t = 0; t < total * batch; ++t) {
        const int64_t e = t % total;
        double v = (e % n == e / n) ? c0 : 0.0;
        v += c1 * X1[t];
        if (X2) v += c2 * X2[t];
        if (X3) v += c3 * X3[t];
        if (in) v += beta * in[t];
        out[t] = v;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// gram
// ---------------------------------------------------------------------------
// variant 0: X != Y integers (exact); 1: X != Y normal (bounded); 2: Y == X, one
// block of max(px, py) columns, integers; 3: X at column 3 of a wider block whose
// leading columns are NaN, normal
static void gram_case(int64_t n, int px, int py, int variant) {
    static const char* vn[] = {"exact", "bounded", "self_exact", "offset_bounded"};
    Case c(G_GRAM, vn[variant], fmt("n=%ld px=%d py=%d", (long)n, px, py));
    if (g_list) return;
    const int kind = (variant == 0 || variant == 2) ? INT8 : NORMAL;
    const int xoff = variant == 3 ? 3 : 0;
    const int wx = (variant == 2 ? std::max(px, py) : px) + xoff;
    const int ldx = wx + 3, ldy = variant == 2 ? ldx : py + 2;
    dvec X = mk(n, wx, ldx, kind, NAN, 0);
    for (int64_t r = 0; r < n; ++r)
        for (int k = 0; k < xoff; ++k) X[(size_t)r * ldx + k] = NAN;
    dvec Yv;
    if (variant != 2) Yv = mk(n, py, ldy, kind, NAN, 0);
    const dvec& Y = variant == 2 ? X : Yv;
    const int S = kt::gram_ts_chunks(n);
    const int64_t rows = gram_rows_host(n);
    if (S != (int)((n + rows - 1) / rows)) c.fail("gram_ts_chunks", 0, S, (double)((n + rows - 1) / rows), 0.0);
    const size_t count = (size_t)px * py;
    const dvec part0 = sentinels((size_t)S * count), G0 = sentinels(count);
    auto o = run_twice(c, [&] {
        arena_release(0);
        const double* dX = up(X);
        const double* dY = variant == 2 ? dX : up(Yv);
        double* dp = up(part0);
        double* dG = up(G0);
        LAUNCH(op_gram(n, dX + xoff, ldx, px, dY, ldy, py, dp, dG));
        return std::vector<dvec>{down(dG, G0.size()), down(dp, part0.size())};
    });
    c.guard("G guard", G0, o[0], count);
    c.guard("part guard", part0, o[1], (size_t)S * count);
    if (kind == INT8) {
        std::vector<int64_t> acc((size_t)kMaxThreads * count, 0);
        par_rows(n, 1024, [&](int64_t r0, int64_t r1, int th) {
            std::vector<int64_t> xi(px), loc(count, 0);  // thread-local sums (no shared cache lines)
            int64_t* ref = loc.data();
            for (int64_t r = r0; r < r1; ++r) {
                for (int i = 0; i < px; ++i) xi[i] = (int64_t)X[(size_t)r * ldx + xoff + i];
                for (int j = 0; j < py; ++j) {
                    const int64_t y = (int64_t)Y[(size_t)r * ldy + j];
                    int64_t* col = ref + (size_t)j * px;
                    for (int i = 0; i < px; ++i) col[i] += xi[i] * y;
                }
            }
            std::copy(loc.begin(), loc.end(), acc.begin() + (size_t)th * count);
        });
        for (size_t t = 0; t < count; ++t) {
            int64_t ref = 0;
            for (int th = 0; th < kMaxThreads; ++th) ref += acc[(size_t)th * count + t];
            c.exact("G", (long)t, o[0][t], (double)ref);
        }
    } else {
        // the sums in long double; sum |x||y| in fp64 (terms >= 0: relative error
        // <= gamma_(n+1)), inflated below so that it stays an upper bound
        std::vector<ld_t> racc((size_t)kMaxThreads * count, 0.0L);
        dvec aacc((size_t)kMaxThreads * count, 0.0);
        par_rows(n, 1024, [&](int64_t r0, int64_t r1, int th) {
            std::vector<ld_t> lref(count, 0.0L);  // thread-local sums
            dvec lab(count, 0.0);
            for (int64_t r = r0; r < r1; ++r)
                for (int j = 0; j < py; ++j) {
                    const double yd = Y[(size_t)r * ldy + j], ya = fabs(yd);
                    const ld_t y = yd;
                    const double* xr = X.data() + (size_t)r * ldx + xoff;
                    ld_t* ref = lref.data() + (size_t)j * px;
                    double* ab = lab.data() + (size_t)j * px;
                    for (int i = 0; i < px; ++i) ref[i] += (ld_t)xr[i] * y;
                    for (int i = 0; i < px; ++i) ab[i] += fabs(xr[i]) * ya;
                }
            std::copy(lref.begin(), lref.end(), racc.begin() + (size_t)th * count);
            std::copy(lab.begin(), lab.end(), aacc.begin() + (size_t)th * count);
        });
        std::vector<ld_t> ref(count, 0.0L), ab(count, 0.0L);
        for (int th = 0; th < kMaxThreads; ++th)
            for (size_t t = 0; t < count; ++t) {
                ref[t] += racc[(size_t)th * count + t];
                ab[t] += aacc[(size_t)th * count + t];
            }
        for (size_t t = 0; t < count; ++t) ab[t] *= 1.0L + 2.0L * gam((ld_t)n + 1);
        const ld_t g = gam((ld_t)n);
        for (size_t t = 0; t < count; ++t) c.bounded("G", (long)t, o[0][t], ref[t], g * ab[t]);
    }
}

static void grp_gram() {
    static const int pairs[12][2] = {{1, 1},   {2, 2},   {7, 3},   {16, 16}, {31, 33}, {32, 32},
                                     {33, 32}, {48, 48}, {64, 17}, {128, 2}, {129, 5}, {200, 48}};
    static const int64_t nsmall[] = {1, 3, 4, 31, 127, 128, 129, 1000};
    static const int64_t nbig[] = {8192, 32768, 32769, 40000};
    for (auto& p : pairs) {
        for (int64_t n : nsmall)
            for (int v = 0; v < 4; ++v) gram_case(n, p[0], p[1], v);
        if (p[0] <= 48 && !g_small)
            for (int64_t n : nbig)
                for (int v = 0; v < 3; ++v) gram_case(n, p[0], p[1], v);
    }
}

// ---------------------------------------------------------------------------
// combine
// ---------------------------------------------------------------------------
static const double kAB[3][2] = {{1.0, 0.0}, {-1.0, 1.0}, {0.5, -2.0}};

// mode 0: Y a separate block; 1: in place (Y == X, same ld, q == px)
static void combine_case(int64_t n, int px, int q, int ab, int kind, int mode) {
    const double alpha = kAB[ab][0], beta = kAB[ab][1];
    Case c(G_COMBINE, fmt("%s_%s", mode ? "inplace" : "separate", kind == INT8 ? "exact" : "bounded"),
           fmt("n=%ld px=%d q=%d alpha=%g beta=%g", (long)n, px, q, alpha, beta));
    if (g_list) return;
    const int ldx = px + 3, ldy = mode ? ldx : q + 2;
    const dvec X = mk(n, px, ldx, kind, NAN, mode ? 2 : 0);
    dvec Y0;
    if (!mode) {
        Y0 = mk(n, q, ldy, kind, SENT, 2);
        if (beta == 0.0)  // must be ignored
            for (int64_t r = 0; r < n; ++r)
                for (int j = 0; j < q; ++j) Y0[(size_t)r * ldy + j] = NAN;
    }
    const dvec& Yin = mode ? X : Y0;
    dvec C = mk1((size_t)px * q, kind, 0);
    auto o = run_twice(c, [&] {
        arena_release(0);
        double* dX = up(X);
        double* dY = mode ? dX : up(Y0);
        const double* dC = up(C);
        LAUNCH(op_combine(n, dX, ldx, px, dC, q, alpha, beta, dY, ldy));
        return std::vector<dvec>{down(dY, Yin.size())};
    });
    c.untouched("Y padding / guard", Yin, o[0], n, q, ldy);
    const ld_t g = gam((ld_t)px + 2);
    std::vector<ld_t> ref((size_t)n * q), bnd((size_t)n * q);
    par_rows(n, 256, [&](int64_t r0, int64_t r1, int) {
        for (int64_t r = r0; r < r1; ++r)
            for (int j = 0; j < q; ++j) {
                ld_t acc = 0.0L, aa = 0.0L;
                for (int i = 0; i < px; ++i) {
                    const ld_t p = (ld_t)X[(size_t)r * ldx + i] * (ld_t)C[i + (size_t)j * px];
                    acc += p;
                    aa += fabsl(p);
                }
                const ld_t by = beta == 0.0 ? 0.0L : (ld_t)beta * (ld_t)Yin[(size_t)r * ldy + j];
                ref[(size_t)r * q + j] = by + (ld_t)alpha * acc;
                bnd[(size_t)r * q + j] = g * (fabsl(by) + fabsl((ld_t)alpha) * aa);
            }
    });
    for (int64_t r = 0; r < n; ++r)
        for (int j = 0; j < q; ++j) {
            const double got = o[0][(size_t)r * ldy + j];
            if (kind == INT8)
                c.exact("Y", (long)(r * ldy + j), got, (double)ref[(size_t)r * q + j]);
            else
                c.bounded("Y", (long)(r * ldy + j), got, ref[(size_t)r * q + j], bnd[(size_t)r * q + j]);
        }
}

// q > 32 with Y overlapping X: hipErrorInvalidValue, nothing written
static void combine_overlap_case(int64_t n, int q, int yoff) {
    Case c(G_COMBINE, yoff ? "overlap_offset_rejected" : "overlap_alias_rejected", fmt("n=%ld px=%d q=%d", (long)n, q, q));
    if (g_list) return;
    const int ld = q + 3;
    const dvec X = mk(n, q, ld, NORMAL, NAN, 2);
    const dvec C = mk1((size_t)q * q, NORMAL, 0);
    arena_release(0);
    double* dX = up(X);
    const double* dC = up(C);
    const hipError_t e = op_combine(n, dX, ld, q, dC, q, 1.0, 0.0, dX + yoff, ld);
    if (e != hipErrorInvalidValue) {
        if (e != hipSuccess) hip_die("launch_combine_ts (overlap)", e);
        c.fail("return value", 0, (double)e, (double)hipErrorInvalidValue, 0.0);
    }
    if (!g_host) HC(hipDeviceSynchronize());
    const dvec after = down(dX, X.size());
    c.untouched("block", X, after, 0, 0, ld);
}

static void grp_combine() {
    static const int pxs[] = {1, 2, 32, 63, 64, 65, 130};
    static const int qs[] = {1, 7, 8, 9, 31, 32, 33, 48, 64};
    static const int64_t ns[] = {1, 63, 64, 65, 1000};
    for (int px : pxs)
        for (int q : qs)
            for (int64_t n : ns)
                for (int ab = 0; ab < 3; ++ab)
                    for (int kind = 0; kind < 2; ++kind) combine_case(n, px, q, ab, kind, 0);
    for (int px : {1, 2, 32})
        for (int64_t n : ns)
            for (int ab = 0; ab < 3; ++ab)
                for (int kind = 0; kind < 2; ++kind) combine_case(n, px, px, ab, kind, 1);
    for (int q : {33, 48, 64})
        for (int64_t n : {(int64_t)1, (int64_t)65})
            for (int yoff = 0; yoff < 2; ++yoff) combine_overlap_case(n, q, yoff);
}

// ---------------------------------------------------------------------------
// chol_rinv
// ---------------------------------------------------------------------------
// integer upper-triangular R0 with a power-of-two diagonal; G = R0' D R0
static void int_gram(int bs, const std::vector<int>& d, dvec& R0, dvec& G) {
    R0.assign((size_t)bs * bs, 0.0);
    for (int j = 0; j < bs; ++j)
        for (int i = 0; i <= j; ++i) R0[i + j * bs] = i == j ? (double)(1 << (rnd() % 4)) : rint8();
    G.assign((size_t)bs * bs, 0.0);
    for (int i = 0; i < bs; ++i)
        for (int j = 0; j < bs; ++j) {
            double s = 0.0;  // integers: exact
            for (int k = 0; k <= std::min(i, j); ++k) s += R0[k + i * bs] * d[k] * R0[k + j * bs];
            G[i + j * bs] = s;
        }
}

struct CholOut {
    dvec R, Rinv;
    int ok;
};
static CholOut chol_run(Case& c, int bs, const dvec& G, double shift_coef) {
    const size_t count = (size_t)bs * bs;
    const dvec R0 = sentinels(count);
    std::vector<int> ok0(1 + 8, -12345);
    auto o = run_twice(c, [&] {
        arena_release(0);
        const double* dG = up(G);
        double* dR = up(R0);
        double* dRi = up(R0);
        int* dok = up(ok0);
        LAUNCH(op_chol(bs, dG, shift_coef, dR, dRi, dok));
        return std::vector<dvec>{down(dR, R0.size()), down(dRi, R0.size()), to_d(down(dok, ok0.size()))};
    });
    c.guard("R guard", R0, o[0], count);
    c.guard("Rinv guard", R0, o[1], count);
    c.guard("ok guard", to_d(ok0), o[2], 1);
    return CholOut{o[0], o[1], (int)o[2][0]};
}

static void chol_case(int bs, bool with_shift, int kind) {
    const double shift_coef = with_shift ? 11.0 * (1e4 * bs + bs * (bs + 1.0)) * DBL_EPSILON : 0.0;
    Case c(G_CHOL, fmt("%s%s", kind == INT8 ? "integer" : "normal", with_shift ? "_shift" : ""),
           fmt("bs=%d shift_coef=%g", bs, shift_coef));
    if (g_list) return;
    dvec Rtrue, G;
    if (kind == INT8) {
        int_gram(bs, std::vector<int>(bs, 1), Rtrue, G);
    } else {  // G = X' X of a (3 bs + 5) x bs normal block (fp64 sums; G itself is the input)
        const int m = 3 * bs + 5;
        const dvec X = mk(m, bs, bs, NORMAL, 0.0, 0);
        G.assign((size_t)bs * bs, 0.0);
        for (int i = 0; i < bs; ++i)
            for (int j = i; j < bs; ++j) {
                double s = 0.0;
                for (int r = 0; r < m; ++r) s += X[(size_t)r * bs + i] * X[(size_t)r * bs + j];
                G[i + j * bs] = G[j + i * bs] = s;
            }
    }
    const CholOut o = chol_run(c, bs, G, shift_coef);
    if (o.ok != 1) c.fail("ok", 0, o.ok, 1, 0.0);
    ld_t tr = 0.0L;
    for (int i = 0; i < bs; ++i) tr += G[i + i * bs];
    const ld_t shift = (ld_t)shift_coef * tr;
    const ld_t g1 = gam((ld_t)bs + 1), g2 = gam((ld_t)bs);
    for (int j = 0; j < bs; ++j)
        for (int i = 0; i < bs; ++i) {
            const long t = i + j * bs;
            if (i > j) {
                if (!(o.R[t] == 0.0)) c.fail("R below the diagonal", t, o.R[t], 0.0, 0.0, INFINITY);
                if (!(o.Rinv[t] == 0.0)) c.fail("Rinv below the diagonal", t, o.Rinv[t], 0.0, 0.0, INFINITY);
            }
            if (kind == INT8 && !with_shift) c.exact("R", t, o.R[t], Rtrue[t]);
            ld_t s = 0.0L, a = 0.0L, s2 = 0.0L, a2 = 0.0L;
            for (int k = 0; k < bs; ++k) {
                const ld_t p = (ld_t)o.R[k + i * bs] * (ld_t)o.R[k + j * bs];
                s += p;
                a += fabsl(p);
                const ld_t p2 = (ld_t)o.R[i + k * bs] * (ld_t)o.Rinv[k + j * bs];
                s2 += p2;
                a2 += fabsl(p2);
            }
            c.bounded("R'R", t, s, (ld_t)G[t] + (i == j ? shift : 0.0L), g1 * a);
            c.bounded("R Rinv", t, s2, i == j ? 1.0L : 0.0L, g2 * a2);
        }
}

// pivot `pos` of the exact factorisation made negative (sign < 0) or zero (sign == 0)
static void chol_fail_case(int bs, int pos, int sign) {
    Case c(G_CHOL, sign ? "indefinite" : "singular", fmt("bs=%d pivot=%d", bs, pos));
    if (g_list) return;
    std::vector<int> d(bs, 1);
    d[pos] = sign;
    dvec Rtrue, G;
    int_gram(bs, d, Rtrue, G);
    const CholOut o = chol_run(c, bs, G, 0.0);
    if (o.ok != 0) c.fail("ok", 0, o.ok, 0, 0.0);
}

static void chol_invalid_case(int bs) {
    Case c(G_CHOL, "invalid_bs", fmt("bs=%d", bs));
    if (g_list) return;
    const dvec G(65 * 65, 1.0), R0 = sentinels(65 * 65);
    const std::vector<int> ok0(9, -12345);
    arena_release(0);
    const double* dG = up(G);
    double* dR = up(R0);
    double* dRi = up(R0);
    int* dok = up(ok0);
    const hipError_t e = op_chol(bs, dG, 0.0, dR, dRi, dok);
    if (e != hipErrorInvalidValue) {
        if (e != hipSuccess) hip_die("launch_chol_rinv (invalid bs)", e);
        c.fail("return value", 0, (double)e, (double)hipErrorInvalidValue, 0.0);
    }
    if (!g_host) HC(hipDeviceSynchronize());
    c.guard("R", R0, down(dR, R0.size()), 0);
    c.guard("Rinv", R0, down(dRi, R0.size()), 0);
    c.guard("ok", to_d(ok0), to_d(down(dok, ok0.size())), 0);
}

static void grp_chol() {
    for (int bs : {1, 2, 3, 17, 32, 63, 64})
        for (int sh = 0; sh < 2; ++sh)
            for (int kind = 0; kind < 2; ++kind) chol_case(bs, sh != 0, kind);
    for (int bs : {1, 3, 17, 64})
        for (int sign : {-1, 0}) {
            chol_fail_case(bs, 0, sign);
            if (bs > 1) chol_fail_case(bs, bs / 2, sign);
            if (bs > 1) chol_fail_case(bs, bs - 1, sign);
        }
    chol_invalid_case(0);
    chol_invalid_case(65);
}

// ---------------------------------------------------------------------------
// fro_colmax_scale
// ---------------------------------------------------------------------------
// variant 0: integers; 1: normal; 2: zero matrix; 3 / 4: the last column is the largest (integers / normal)
static void fro_case(int n, int variant) {
    static const char* vn[] = {"exact", "bounded", "zero", "last_col_exact", "last_col_bounded"};
    Case c(G_FRO, vn[variant], fmt("n=%d", n));
    if (g_list) return;
    const bool integer = variant == 0 || variant == 3;
    const size_t nn = (size_t)n * n;
    dvec M0 = variant == 2 ? dvec(nn + GUARD, SENT) : mk1(nn, integer ? INT8 : NORMAL, GUARD);
    if (variant == 2) std::fill(M0.begin(), M0.begin() + nn, 0.0);
    if (variant >= 3)
        for (int i = 0; i < n; ++i) M0[i + (size_t)(n - 1) * n] = (integer ? 9.0 + (i & 1) : 3.0 * M0[i + (size_t)(n - 1) * n] + 40.0);
    const dvec out0 = sentinels(2), cs0 = sentinels(n);
    auto o = run_twice(c, [&] {
        arena_release(0);
        double* dM = up(M0);
        double* dout = up(out0);
        double* dcs = up(cs0);
        LAUNCH(op_fro(n, dM, dout, dcs));
        return std::vector<dvec>{down(dM, M0.size()), down(dout, out0.size()), down(dcs, cs0.size())};
    });
    c.guard("M guard", M0, o[0], nn);
    c.guard("out guard", out0, o[1], 2);
    c.guard("colsq guard", cs0, o[2], n);
    ld_t f = 0.0L, m = 0.0L;
    int jmax = 0;
    for (int j = 0; j < n; ++j) {
        ld_t s = 0.0L;
        for (int i = 0; i < n; ++i) s += (ld_t)M0[i + (size_t)j * n] * (ld_t)M0[i + (size_t)j * n];
        f += s;
        if (s > m) {
            m = s;
            jmax = j;
        }
    }
    if (variant >= 3 && jmax != n - 1) c.fail("test setup: largest column", jmax, jmax, n - 1, 0.0);
    if (f == 0.0L) {  // nothing to scale by: M stays as it is
        c.exact("out[0]", 0, o[1][0], 0.0);
        c.exact("out[1]", 1, o[1][1], 0.0);
        for (size_t t = 0; t < nn; ++t) c.same("M unchanged", (long)t, o[0][t], M0[t]);
        return;
    }
    const ld_t g = gam((ld_t)n * n);
    if (integer) {
        c.exact("out[0]", 0, o[1][0], (double)f);
        c.exact("out[1]", 1, o[1][1], (double)m);
    } else {
        c.bounded("out[0]", 0, o[1][0], f, g * f);
        c.bounded("out[1]", 1, o[1][1], m, g * m);
    }
    const ld_t inv = 1.0L / sqrtl(f), rel = ((ld_t)n * n + 4) * U;
    for (size_t t = 0; t < nn; ++t) {
        const ld_t ref = (ld_t)M0[t] * inv;
        c.bounded("M scaled", (long)t, o[0][t], ref, rel * fabsl(ref));
    }
}

static void grp_fro() {
    for (int n : {1, 3, 63, 64, 65, 161, 225})
        for (int v = 0; v < 5; ++v) fro_case(n, v);
}

// ---------------------------------------------------------------------------
// colbatch
// ---------------------------------------------------------------------------
static void householder_case(int n, int P, int variant, bool inplace) {
    static const char* vn[] = {"random", "zero_tail", "alpha_zero", "alpha_negative"};
    Case c(G_COL, fmt("householder_%s_%s", vn[variant], inplace ? "inplace" : "outofplace"), fmt("n=%d P=%d", n, P));
    if (g_list) return;
    const size_t np = (size_t)n * P;
    dvec W0 = mk1(np, NORMAL, GUARD);
    for (int col = 0; col < P; ++col) {
        if (variant == 1) {
            for (int r = 1; r < n; ++r) W0[(size_t)r * P + col] = 0.0;
        }
        if (variant == 2) W0[col] = 0.0;
        if (variant == 3) W0[col] = -fabs(W0[col]) - 0.25;
    }
    dvec s((size_t)P);  // the tail's squared norm as fp64 data (k_col_dots supplies it in use)
    for (int col = 0; col < P; ++col) {
        ld_t a = 0.0L;
        for (int r = 1; r < n; ++r) a += (ld_t)W0[(size_t)r * P + col] * (ld_t)W0[(size_t)r * P + col];
        s[col] = (double)a;
    }
    const dvec Q0 = sentinels(np), r0 = sentinels(P);
    auto o = run_twice(c, [&] {
        arena_release(0);
        const double* ds = up(s);
        double* dW = up(W0);
        double* dQ = inplace ? dW : up(Q0);
        double* dr = up(r0);
        LAUNCH(op_col_householder(n, P, ds, dW, dQ, dr));
        return std::vector<dvec>{down(dQ, Q0.size()), down(dr, r0.size()), down(dW, W0.size())};
    });
    c.guard("Q guard", inplace ? W0 : Q0, o[0], np);
    c.guard("r guard", r0, o[1], P);
    if (!inplace) c.guard("W unchanged", W0, o[2], 0);
    for (int col = 0; col < P; ++col) {
        const ld_t alpha = W0[col], xx = s[col];
        ld_t beta = alpha, tau = 0.0L, scal = 1.0L;
        if (xx != 0.0L) {
            beta = -copysignl(hypotl(alpha, sqrtl(xx)), alpha);
            tau = (beta - alpha) / beta;
            scal = 1.0L / (alpha - beta);
        }
        const bool exact = s[col] == 0.0;  // tau = 0: Q = e1 and r = alpha exactly
        if (exact)
            c.exact("r (tau = 0)", col, o[1][col], W0[col]);
        else
            c.bounded("r", col, o[1][col], beta, 1e-12L * fabsl(beta));
        for (int r = 0; r < n; ++r) {
            const size_t t = (size_t)r * P + col;
            const ld_t ref = r == 0 ? 1.0L - tau : -tau * ((ld_t)W0[t] * scal);
            if (exact)
                c.exact("Q (tau = 0)", (long)t, o[0][t], r == 0 ? 1.0 : 0.0);
            else
                c.bounded("Q", (long)t, o[0][t], ref, 1e-12L);
        }
    }
}

static void col_select_case(int n, int P, int C) {
    Case c(G_COL, "col_select", fmt("n=%d P=%d C=%d", n, P, C));
    if (g_list) return;
    const size_t np = (size_t)n * P;
    dvec X0(np + GUARD, SENT);
    std::fill(X0.begin(), X0.begin() + np, 0.0);
    std::vector<int> idx(C);
    for (int k = 0; k < C; ++k) idx[k] = (int)(rnd() % n);
    auto o = run_twice(c, [&] {
        arena_release(0);
        const int* di = up(idx);
        double* dX = up(X0);
        LAUNCH(op_col_select(C, P, di, dX));
        return std::vector<dvec>{down(dX, X0.size())};
    });
    dvec ref = X0;
    for (int k = 0; k < C; ++k) ref[(size_t)idx[k] * P + k] = 1.0;
    for (size_t t = 0; t < ref.size(); ++t) c.same("X", (long)t, o[0][t], ref[t]);
}

static void grp_colbatch() {
    static const int Ps[] = {1, 2, 8, 32, 128};
    static const int ns[] = {1, 2, 31, 33, 1000, 5000};
    static const int nbs[] = {1, 2, 7};
    const int NBMAX = 7;
    for (int P : Ps)
        for (int n : ns) {
            const size_t np = (size_t)n * P;
            for (int kind = 0; kind < 2; ++kind) {
                // basis blocks vstride apart with NaN in the gaps
                const int64_t vstride = (int64_t)np + 5;
                dvec V, W;
                if (!g_list) {
                    V.assign((size_t)NBMAX * vstride, NAN);
                    W.resize(np);
                    for (int k = 0; k < NBMAX; ++k) fill(V.data() + k * vstride, np, kind);
                    fill(W.data(), np, kind);
                }
                // dot[lo][k * P + c] over rows >= lo, and the sums of |terms|
                std::vector<ld_t> dot[2], dab[2];
                for (int lo = 0; lo < 2 && !g_list; ++lo) {
                    dot[lo].assign((size_t)NBMAX * P, 0.0L);
                    dab[lo].assign((size_t)NBMAX * P, 0.0L);
                    for (int k = 0; k < NBMAX; ++k)
                        for (int r = lo; r < n; ++r)
                            for (int col = 0; col < P; ++col) {
                                const ld_t p = (ld_t)V[k * vstride + (size_t)r * P + col] * (ld_t)W[(size_t)r * P + col];
                                dot[lo][k * P + col] += p;
                                dab[lo][k * P + col] += fabsl(p);
                            }
                }
                arena_release(0);
                const double* dV = up(V);
                const double* dW = up(W);
                const size_t mark = arena_mark();
                const ld_t gn = gam((ld_t)n);
                for (int nb : nbs)
                    for (int r_lo = 0; r_lo < 2; ++r_lo)
                        for (int rpb_lo : {32, 64})
                            for (int ncu : {g_num_cu, 8}) {
                                Case c(G_COL, fmt("col_dots_%s", kind == INT8 ? "exact" : "bounded"),
                                       fmt("n=%d P=%d nb=%d r_lo=%d rpb_lo=%d num_cu=%s", n, P, nb, r_lo, rpb_lo,
                                           ncu == 8 ? "8" : "device"));
                                if (g_list) continue;
                                const int nrb = kt::col_nrb(n, ncu, rpb_lo);
                                const dvec part0 = sentinels((size_t)nb * P * nrb), out0 = sentinels((size_t)nb * P);
                                auto o = run_twice(c, [&] {
                                    arena_release(mark);
                                    double* dp = up(part0);
                                    double* dout = up(out0);
                                    LAUNCH(op_col_dots(n, P, nb, vstride, dV, dW, r_lo, ncu, dp, dout, rpb_lo));
                                    return std::vector<dvec>{down(dout, out0.size()), down(dp, part0.size())};
                                });
                                c.guard("out guard", out0, o[0], (size_t)nb * P);
                                c.guard("part guard", part0, o[1], (size_t)nb * P * nrb);
                                for (int t = 0; t < nb * P; ++t) {
                                    if (kind == INT8)
                                        c.exact("out", t, o[0][t], (double)dot[r_lo][t]);
                                    else
                                        c.bounded("out", t, o[0][t], dot[r_lo][t], gn * dab[r_lo][t]);
                                }
                            }
                for (int nb : nbs) {
                    Case c(G_COL, fmt("col_update_%s", kind == INT8 ? "exact" : "bounded"), fmt("n=%d P=%d nb=%d", n, P, nb));
                    if (g_list) continue;
                    const dvec h = mk1((size_t)nb * P, kind, 0);
                    dvec Wg(np + GUARD, SENT);
                    std::copy(W.begin(), W.end(), Wg.begin());
                    auto o = run_twice(c, [&] {
                        arena_release(mark);
                        const double* dh = up(h);
                        double* dWo = up(Wg);
                        LAUNCH(op_col_update(n, P, nb, vstride, dV, dh, dWo));
                        return std::vector<dvec>{down(dWo, Wg.size())};
                    });
                    c.guard("W guard", Wg, o[0], np);
                    const ld_t g = gam((ld_t)nb + 2);
                    for (size_t t = 0; t < np; ++t) {
                        ld_t s = 0.0L, a = 0.0L;
                        for (int k = 0; k < nb; ++k) {
                            const ld_t p = (ld_t)V[k * vstride + t] * (ld_t)h[k * P + t % P];
                            s += p;
                            a += fabsl(p);
                        }
                        if (kind == INT8)
                            c.exact("W", (long)t, o[0][t], (double)((ld_t)W[t] - s));
                        else
                            c.bounded("W", (long)t, o[0][t], (ld_t)W[t] - s, g * (fabsl((ld_t)W[t]) + a));
                    }
                }
            }
            for (int variant = 0; variant < 4; ++variant)
                for (int inplace = 0; inplace < 2; ++inplace) householder_case(n, P, variant, inplace != 0);
            col_select_case(n, P, 1);
            if (P > 1) col_select_case(n, P, P / 2 + 1);
            if (P > 1) col_select_case(n, P, P);
        }
}

// ---------------------------------------------------------------------------
// streaming
// ---------------------------------------------------------------------------
static const int kNs[] = {1, 255, 256, 257, 5000};
static const int kNcs[] = {1, 3, 32};

static void weighted_sum_cases(int n, int nc) {
    const int MMAX = 30, P = 32, ldu = nc + 1, ldy = nc + 2;
    const int64_t sstride = (int64_t)n * ldu;
    for (int kind = 0; kind < 2; ++kind) {
        dvec Uh, Wh;
        if (!g_list) {
            Uh.assign((size_t)MMAX * sstride, NAN);
            Wh.assign((size_t)MMAX * P, NAN);
        }
        for (int j = 0; j < MMAX && !g_list; ++j) {
            for (int r = 0; r < n; ++r) fill(Uh.data() + j * sstride + (size_t)r * ldu, nc, kind);
            fill(Wh.data() + j * P, nc, kind);
        }
        arena_release(0);
        const double* dU = up(Uh);
        const double* dW = up(Wh);
        const size_t mark = arena_mark();
        const dvec Y0 = g_list ? dvec() : mk(n, nc, ldy, NORMAL, SENT, 1);
        for (int m : {1, 7, 8, 9, 30}) {
            Case c(G_STREAM, fmt("weighted_sum_%s", kind == INT8 ? "exact" : "fma_chain"), fmt("n=%d nc=%d m=%d", n, nc, m));
            if (g_list) continue;
            auto o = run_twice(c, [&] {
                arena_release(mark);
                double* dY = up(Y0);
                LAUNCH(op_weighted_sum(n, m, P, nc, dU, ldu, sstride, dW, dY, ldy));
                return std::vector<dvec>{down(dY, Y0.size())};
            });
            c.untouched("Y padding / guard", Y0, o[0], n, nc, ldy);
            for (int r = 0; r < n; ++r)
                for (int col = 0; col < nc; ++col) {
                    const long t = (long)r * ldy + col;
                    if (kind == INT8) {
                        ld_t s = 0.0L;
                        for (int j = 0; j < m; ++j) s += (ld_t)Uh[j * sstride + (size_t)r * ldu + col] * (ld_t)Wh[j * P + col];
                        c.exact("Y", t, o[0][t], (double)s);
                    } else {  // the documented order: one fma per slot, slots ascending
                        double s = 0.0;
                        for (int j = 0; j < m; ++j) s = fma(Uh[j * sstride + (size_t)r * ldu + col], Wh[j * P + col], s);
                        c.same("Y", t, o[0][t], s);
                    }
                }
        }
    }
}

static std::vector<int> random_perm(int n) {
    std::vector<int> p(n);
    for (int i = 0; i < n; ++i) p[i] = i;
    for (int i = n - 1; i > 0; --i) std::swap(p[i], p[rnd() % (i + 1)]);
    return p;
}

static void perm_rows_case(int n, int cols, int gather) {
    Case c(G_STREAM, gather ? "perm_rows_gather" : "perm_rows_scatter", fmt("n=%d cols=%d", n, cols));
    if (g_list) return;
    const int lds = cols + 1, ldd = cols + 2;
    const dvec src = mk(n, cols, lds, NORMAL, NAN, 0), dst0 = mk(n, cols, ldd, NORMAL, SENT, 1);
    const std::vector<int> perm = random_perm(n);
    auto o = run_twice(c, [&] {
        arena_release(0);
        const int* dp = up(perm);
        const double* ds = up(src);
        double* dd = up(dst0);
        LAUNCH(op_perm_rows(n, cols, dp, gather, ds, lds, dd, ldd));
        return std::vector<dvec>{down(dd, dst0.size())};
    });
    c.untouched("dst padding / guard", dst0, o[0], n, cols, ldd);
    for (int r = 0; r < n; ++r)
        for (int col = 0; col < cols; ++col) {
            const size_t from = gather ? (size_t)perm[r] * lds + col : (size_t)r * lds + col;
            const size_t to = gather ? (size_t)r * ldd + col : (size_t)perm[r] * ldd + col;
            c.same("dst", (long)to, o[0][to], src[from]);
        }
}

static void axpby_case(int n, int nc, double a, double b) {
    Case c(G_STREAM, "axpby", fmt("n=%d nc=%d a=%g b=%g", n, nc, a, b));
    if (g_list) return;
    const int ldx = nc + 1, ldy = nc + 2;
    const dvec X = mk(n, nc, ldx, NORMAL, NAN, 0);
    dvec Y0 = mk(n, nc, ldy, NORMAL, SENT, 1);
    if (b == 0.0)  // Y must be ignored
        for (int r = 0; r < n; ++r)
            for (int col = 0; col < nc; ++col) Y0[(size_t)r * ldy + col] = NAN;
    auto o = run_twice(c, [&] {
        arena_release(0);
        const double* dX = up(X);
        double* dY = up(Y0);
        LAUNCH(op_axpby(n, nc, a, dX, ldx, b, dY, ldy));
        return std::vector<dvec>{down(dY, Y0.size())};
    });
    c.untouched("Y padding / guard", Y0, o[0], n, nc, ldy);
    for (int r = 0; r < n; ++r)
        for (int col = 0; col < nc; ++col) {
            const size_t t = (size_t)r * ldy + col;
            const double y = b == 0.0 ? 0.0 : b * Y0[t];
            c.same("Y", (long)t, o[0][t], fma(a, X[(size_t)r * ldx + col], y));
        }
}

static void inf_norm_case(int n, int nc, int kind) {
    Case c(G_STREAM, kind == INT8 ? "inf_norm_exact" : "inf_norm_bounded", fmt("n=%d nc=%d", n, nc));
    if (g_list) return;
    const int ldx = nc + 1, nb = kt::inf_norm_blocks();
    const dvec X = mk(n, nc, ldx, kind, NAN, 0), p0 = sentinels(nb);
    auto o = run_twice(c, [&] {
        arena_release(0);
        const double* dX = up(X);
        double* dp = up(p0);
        LAUNCH(op_inf_norm(n, nc, dX, ldx, dp));
        return std::vector<dvec>{down(dp, p0.size())};
    });
    c.guard("partial guard", p0, o[0], nb);
    double got = 0.0;
    for (int b = 0; b < nb; ++b) got = o[0][b] > got || std::isnan(o[0][b]) ? o[0][b] : got;
    ld_t ref = 0.0L;
    for (int r = 0; r < n; ++r) {
        ld_t s = 0.0L;
        for (int col = 0; col < nc; ++col) s += fabsl((ld_t)X[(size_t)r * ldx + col]);
        ref = std::max(ref, s);
    }
    if (kind == INT8)
        c.exact("max row sum", 0, got, (double)ref);
    else
        c.bounded("max row sum", 0, got, ref, gam((ld_t)nc) * ref);
}

static void normest1_case(int n, int kind) {
    Case c(G_STREAM, kind == INT8 ? "normest1_y_exact" : "normest1_y_bounded", fmt("n=%d", n));
    if (g_list) return;
    const int nb = kt::normest1_blocks(n);
    dvec Y = mk1(n, kind, 0), Sp(n);
    for (int r = 0; r < n; ++r) {
        if (r % 5 == 0) Y[r] = -0.0;
        if (r % 5 == 2) Y[r] = 0.0;
        if (r % 5 == 4) Y[r] = -fabs(Y[r]) - 1.0;
        Sp[r] = (rnd() & 1) ? 1.0 : -1.0;
    }
    const dvec S0 = sentinels(n), p0 = sentinels(2 * (size_t)nb);
    auto o = run_twice(c, [&] {
        arena_release(0);
        const double* dY = up(Y);
        const double* dSp = up(Sp);
        double* dS = up(S0);
        double* dp = up(p0);
        LAUNCH(op_normest1_y(n, dY, dSp, dS, dp));
        return std::vector<dvec>{down(dS, S0.size()), down(dp, p0.size())};
    });
    c.guard("S guard", S0, o[0], n);
    c.guard("partial guard", p0, o[1], 2 * (size_t)nb);
    ld_t a = 0.0L, d = 0.0L;
    for (int r = 0; r < n; ++r) {
        const double s = Y[r] < 0.0 ? -1.0 : 1.0;  // sign(+0) = sign(-0) = +1
        c.same("S", r, o[0][r], s);
        a += fabsl((ld_t)Y[r]);
        d += (ld_t)Sp[r] * s;
    }
    double ga = 0.0, gd = 0.0;  // integers (the sign dot always): exact in any order
    for (int b = 0; b < nb; ++b) {
        ga += o[1][b];
        gd += o[1][nb + b];
    }
    c.exact("sign dot", 1, gd, (double)d);
    if (kind == INT8)
        c.exact("sum |Y|", 0, ga, (double)a);
    else
        c.bounded("sum |Y|", 0, ga, a, gam((ld_t)n) * a);
}

// variant 0: normal data; 1: a tie inside one wave; 2: a tie between the most
// distant rows (two workgroups once n > 256), +big against -big; 3: all zeros
static void absmax_case(int n, int variant) {
    static const char* vn[] = {"random", "tie_in_wave", "tie_far_apart", "all_zero"};
    Case c(G_STREAM, fmt("absmax_idx_%s", vn[variant]), fmt("n=%d", n));
    if (g_list) return;
    const int nb = kt::normest1_blocks(n);
    dvec Z = mk1(n, NORMAL, 0);
    if (variant == 1) {
        const int a = std::min(n - 1, 70), b = std::min(n - 1, 75);
        Z[a] = 50.0;
        Z[b] = 50.0;
    } else if (variant == 2) {
        Z[n - 1] = 50.0;
        Z[n > 256 ? 10 : 0] = -50.0;
        if (n > 2) Z[n / 2] = 50.0;
    } else if (variant == 3) {
        for (int r = 0; r < n; ++r) Z[r] = (r & 1) ? -0.0 : 0.0;
    }
    const dvec pv0 = sentinels(nb);
    const std::vector<int> pi0((size_t)nb + 8, -12345);
    auto o = run_twice(c, [&] {
        arena_release(0);
        const double* dZ = up(Z);
        double* dv = up(pv0);
        int* di = up(pi0);
        LAUNCH(op_absmax_idx(n, dZ, dv, di));
        return std::vector<dvec>{down(dv, pv0.size()), to_d(down(di, pi0.size()))};
    });
    c.guard("pval guard", pv0, o[0], nb);
    c.guard("pidx guard", to_d(pi0), o[1], nb);
    double v = -1.0;
    int i = INT_MAX;
    for (int b = 0; b < nb; ++b) absmax_merge(v, i, o[0][b], (int)o[1][b], false);
    double rv = -1.0;
    int ri = 0;
    for (int r = 0; r < n; ++r)
        if (fabs(Z[r]) > rv) {
            rv = fabs(Z[r]);
            ri = r;
        }
    c.exact("max |Z|", 0, v, rv);
    c.exact("index", 1, i, ri);
}

static void poly4_case(int n, int batch, int nulls) {
    Case c(G_STREAM, "poly4_exact", fmt("n=%d batch=%d in=%d X2=%d X3=%d", n, batch, !(nulls & 1), !(nulls & 2), !(nulls & 4)));
    if (g_list) return;
    const size_t tot = (size_t)n * n * batch;
    const dvec in = mk1(tot, INT8, 0), X1 = mk1(tot, INT8, 0), X2 = mk1(tot, INT8, 0), X3 = mk1(tot, INT8, 0);
    const dvec out0 = sentinels(tot);
    const double beta = -3.0, c0 = 5.0, c1 = 2.0, c2 = -7.0, c3 = 4.0;
    auto o = run_twice(c, [&] {
        arena_release(0);
        const double* din = (nulls & 1) ? nullptr : up(in);
        const double* d1 = up(X1);
        const double* d2 = (nulls & 2) ? nullptr : up(X2);
        const double* d3 = (nulls & 4) ? nullptr : up(X3);
        double* dout = up(out0);
        LAUNCH(op_poly4(n, beta, din, c0, c1, d1, c2, d2, c3, d3, dout, batch));
        return std::vector<dvec>{down(dout, out0.size())};
    });
    c.guard("out guard", out0, o[0], tot);
    for (size_t t = 0; t < tot; ++t) {
        const size_t e = t % ((size_t)n * n);
        ld_t v = (e % n == e / n) ? c0 : 0.0;
        v += (ld_t)c1 * X1[t];
        if (!(nulls & 2)) v += (ld_t)c2 * X2[t];
        if (!(nulls & 4)) v += (ld_t)c3 * X3[t];
        if (!(nulls & 1)) v += (ld_t)beta * in[t];
        c.exact("out", (long)t, o[0][t], (double)v);
    }
}

static void sum_slabs_case(int count, int S, int kind) {
    Case c(G_STREAM, kind == INT8 ? "sum_slabs_exact" : "sum_slabs_sequential", fmt("count=%d S=%d", count, S));
    if (g_list) return;
    const dvec part = mk1((size_t)count * S, kind, 0), G0 = sentinels(count);
    auto o = run_twice(c, [&] {
        arena_release(0);
        const double* dp = up(part);
        double* dG = up(G0);
        LAUNCH(op_sum_slabs(count, S, dp, dG));
        return std::vector<dvec>{down(dG, G0.size())};
    });
    c.guard("G guard", G0, o[0], count);
    for (int t = 0; t < count; ++t) {
        double s = 0.0;  // the sequential sum, slab 0 first (exact for integers)
        for (int q = 0; q < S; ++q) s += part[(size_t)q * count + t];
        if (kind == INT8)
            c.exact("G", t, o[0][t], s);
        else
            c.same("G", t, o[0][t], s);
    }
}

static void gather_rows_case(int nD, int cols, int nr) {
    Case c(G_STREAM, "gather_rows", fmt("rows_of_D=%d cols=%d nr=%d", nD, cols, nr));
    if (g_list) return;
    const int ldd = cols + 1;
    const dvec D = mk(nD, cols, ldd, NORMAL, NAN, 0), out0 = sentinels((size_t)nr * cols);
    std::vector<int64_t> rows(nr);
    for (int r = 0; r < nr; ++r) rows[r] = (int64_t)(rnd() % nD);
    auto o = run_twice(c, [&] {
        arena_release(0);
        const double* dD = up(D);
        const int64_t* dr = up(rows);
        double* dout = up(out0);
        LAUNCH(op_gather_rows(nr, cols, dD, ldd, dr, dout));
        return std::vector<dvec>{down(dout, out0.size())};
    });
    c.guard("out guard", out0, o[0], (size_t)nr * cols);
    for (int col = 0; col < cols; ++col)
        for (int r = 0; r < nr; ++r)
            c.same("out", (long)col * nr + r, o[0][(size_t)col * nr + r], D[(size_t)rows[r] * ldd + col]);
}

static void elems_case(int count, int scatter) {
    Case c(G_STREAM, scatter ? "scatter_elems" : "gather_elems", fmt("count=%d", count));
    if (g_list) return;
    const size_t nD = 3 * (size_t)count + 5;
    const dvec D0 = mk1(nD, NORMAL, GUARD), val = mk1(count, NORMAL, 0), out0 = sentinels(count);
    std::vector<int64_t> off(count);
    const std::vector<int> perm = random_perm(count);
    for (int t = 0; t < count; ++t) off[t] = 3 * (int64_t)perm[t] + (int64_t)(rnd() % 3);  // distinct
    auto o = run_twice(c, [&] {
        arena_release(0);
        double* dD = up(D0);
        const int64_t* doff = up(off);
        const double* dval = up(val);
        double* dout = up(out0);
        if (scatter)
            LAUNCH(op_scatter_elems(count, doff, dval, dD));
        else
            LAUNCH(op_gather_elems(count, dD, doff, dout));
        return std::vector<dvec>{down(dD, D0.size()), down(dout, out0.size())};
    });
    dvec refD = D0, refo = out0;
    for (int t = 0; t < count; ++t) {
        if (scatter)
            refD[off[t]] = val[t];
        else
            refo[t] = D0[off[t]];
    }
    for (size_t t = 0; t < refD.size(); ++t) c.same("D", (long)t, o[0][t], refD[t]);
    for (size_t t = 0; t < refo.size(); ++t) c.same("out", (long)t, o[1][t], refo[t]);
}

static void grp_streaming() {
    for (int n : kNs) {
        for (int nc : kNcs) {
            weighted_sum_cases(n, nc);
            perm_rows_case(n, nc, 1);
            perm_rows_case(n, nc, 0);
            axpby_case(n, nc, 2.0, 0.0);
            axpby_case(n, nc, 0.5, -2.0);
            axpby_case(n, nc, -1.0, 1.0);
            inf_norm_case(n, nc, INT8);
            inf_norm_case(n, nc, NORMAL);
            gather_rows_case(n, nc, 1);
            gather_rows_case(n, nc, std::min(n, 300));
        }
        normest1_case(n, INT8);
        normest1_case(n, NORMAL);
        for (int v = 0; v < 4; ++v) absmax_case(n, v);
        elems_case(n, 0);
        elems_case(n, 1);
    }
    for (int n : {1, 5, 64})
        for (int batch : {1, 2})
            for (int nulls : {0, 1, 2, 4, 7}) poly4_case(n, batch, nulls);
    for (int S : {1, 2, 33})
        for (int count : {1, 255, 257})
            for (int kind = 0; kind < 2; ++kind) sum_slabs_case(count, S, kind);
}

// ---------------------------------------------------------------------------
static const char* kMutations[] = {"gram_drop_last_row", "gram_skip_col32",   "gram_drop_slab",       "combine_ignore_beta",
                                   "combine_inplace_rowwise", "chol_no_shift", "chol_below_diag", "col_dots_ignore_r_lo",
                                   "absmax_tie_largest", "normest1_sign0"};

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
                fprintf(stderr, "block_check: unknown group %s\n", argv[a] + 8);
                return 2;
            }
        } else {
            fprintf(stderr, "usage: block_check [--host [--mutate=NAME]] [--count] [--group=NAME] [--small]\n");
            return 2;
        }
    }
    if (!g_mut.empty()) {
        bool known = false;
        for (const char* m : kMutations) known = known || g_mut == m;
        if (!known || !g_host) {
            fprintf(stderr, "block_check: --mutate needs --host and one of:");
            for (const char* m : kMutations) fprintf(stderr, " %s", m);
            fprintf(stderr, "\n");
            return 2;
        }
    }
    if (!g_host) {
        hipDeviceProp_t prop;
        HC(hipGetDeviceProperties(&prop, 0));
        g_num_cu = prop.multiProcessorCount;
    }
    if (!g_list) {
        pool_init();
        arena_init((size_t)160 << 20);
    }
    void (*const groups[NG])() = {grp_gram, grp_combine, grp_chol, grp_fro, grp_colbatch, grp_streaming};
    for (int g = 0; g < NG; ++g) {
        if (g_only >= 0 && g != g_only) continue;
        const auto t0 = std::chrono::steady_clock::now();
        const double r0 = g_run_s;
        groups[g]();
        g_groups[g].run_seconds = g_run_s - r0;
        g_groups[g].seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    print_report(nullptr);
    long nfail = 0;
    for (int g = 0; g < NG; ++g) nfail += g_groups[g].nfail;
    return nfail ? 1 : 0;
}
