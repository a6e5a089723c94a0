// eig_check -- TEST INFRASTRUCTURE: the three launchers of kt_eigs.hip
// (kt_eigs_topk's streaming kernels) called one by one against exact
// references.  Prints one JSON line:
//   {"mode": "device"|"host", "groups": {"rotate": {"cases": N, "failed_count":
//    F, "failed": ["..."]}, "resid": ..., "start": ...}, "wall_s": s}
// plus "hip_error" when a HIP call failed (the run stops there).  Exit status
// 0: no failed case, 1: some, 2: HIP error.
//
//   eig_check          the cases on the device
//   eig_check --host   the same enumeration with plain host loops in place of
//                      the launches (tests/test_eigs_topk_host.py; the device
//                      test holds its case counts to this run's)
//
// rotate  V(:, 0:p) <- V(:, 0:mb) Y in place, integer V and Y (exact sums):
//         every output equals the product formed from the ORIGINAL row, the
//         columns p..mb-1 keep their values, the padding columns mb..ld-1 (NaN)
//         and the sentinel rows past n keep their bits.  Y is dense, so an
//         output stored before another output of its row had read its inputs
//         would show.  (No input column can hold NaN: every column feeds
//         every output.)
// resid   integer X, AX and theta: the three sums per column exactly; the
//         padding columns of both blocks are NaN and must not reach them
// start   the block is a function of (seed, ORIGINAL row, column): two
//         different perms give the same block once un-permuted, equal to the
//         host's splitmix64 stream; unmasked columns, padding and the rows
//         past n keep their sentinels
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

typedef std::vector<double> dvec;

static bool g_host = false;
static const char* g_hip_err = nullptr;
static const double SENT = -7.7777e77;
static const int GUARD_ROWS = 3;

struct Group {
    const char* name;
    int cases;
    std::vector<std::string> failed;
};
static Group g_groups[3] = {{"rotate", 0, {}}, {"resid", 0, {}}, {"start", 0, {}}};

static uint64_t g_rng = 88172645463325252ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static double rint_in(int a) { return (double)((int)(rnd() % (uint64_t)(2 * a + 1)) - a); }

static uint64_t bits_of(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}
static bool same_bits(double a, double b) { return bits_of(a) == bits_of(b); }

static bool hip_ok(hipError_t e) {
    if (e == hipSuccess) return true;
    if (!g_hip_err) g_hip_err = hipGetErrorString(e);
    return false;
}

// device copy of a host vector (host mode: the vector itself)
struct Buf {
    dvec h;
    double* d = nullptr;
    bool up() {
        if (g_host) {
            d = h.data();
            return true;
        }
        return hip_ok(hipMalloc((void**)&d, sizeof(double) * h.size())) &&
               hip_ok(hipMemcpy(d, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
    }
    bool down() {
        if (g_host) return true;
        return hip_ok(hipDeviceSynchronize()) &&
               hip_ok(hipMemcpy(h.data(), d, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    }
    ~Buf() {
        if (!g_host && d) (void)hipFree(d);
    }
};

// ---- host stand-ins -------------------------------------------------------
static uint64_t sm64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static double sign_of(uint64_t seed, uint64_t col, uint64_t i) {
    const uint64_t key = sm64(sm64(seed) + col);
    return (sm64(key + i) >> 63) ? -1.0 : 1.0;
}

static hipError_t op_start(int64_t n, uint64_t seed, int64_t col0, unsigned mask, bool ones_first, const int* perm,
                           double* X, int ldx) {
    if (!g_host) return kt::launch_eig_start(n, seed, col0, mask, ones_first, perm, X, ldx, nullptr);
    for (int64_t r = 0; r < n; ++r)
        for (int c = 0; c < 16; ++c)
            if (mask & (1u << c))
                X[r * ldx + c] = (ones_first && c == 0) ? 1.0 / sqrt((double)n)
                                                         : sign_of(seed, (uint64_t)(col0 + c), (uint64_t)(perm ? perm[r] : r));
    return hipSuccess;
}

static hipError_t op_rotate(int64_t n, int mb, int p, double* V, int ld, const double* Y) {
    if (!g_host) return kt::launch_eig_rotate(n, mb, p, V, ld, Y, nullptr);
    dvec row(mb);
    for (int64_t r = 0; r < n; ++r) {
        for (int k = 0; k < mb; ++k) row[k] = V[r * ld + k];
        for (int c = 0; c < p; ++c) {
            double s = 0.0;
            for (int k = 0; k < mb; ++k) s = fma(row[k], Y[k * p + c], s);
            V[r * ld + c] = s;
        }
    }
    return hipSuccess;
}

static hipError_t op_resid(int64_t n, int kp, const double* X, int ldx, const double* AX, int ldax,
                           const double* theta, double* part, double* out) {
    if (!g_host) return kt::launch_eig_resid(n, kp, X, ldx, AX, ldax, theta, part, out, nullptr);
    const int chunks = kt::eig_resid_chunks(n);
    for (int i = 0; i < 3 * kp; ++i) out[i] = 0.0;
    for (int ch = 0; ch < chunks; ++ch)
        for (int i = 0; i < kp; ++i) {
            double a = 0.0, b = 0.0, c = 0.0;
            for (int64_t r = (int64_t)ch * 512; r < n && r < (int64_t)(ch + 1) * 512; ++r) {
                const double x = X[r * ldx + i], d = AX[r * ldax + i] - theta[i] * x;
                a += d * d;
                b += x * x;
                c += x;
            }
            part[((size_t)ch * 3 + 0) * kp + i] = a;
            part[((size_t)ch * 3 + 1) * kp + i] = b;
            part[((size_t)ch * 3 + 2) * kp + i] = c;
            out[i] += a;
            out[kp + i] += b;
            out[2 * kp + i] += c;
        }
    return hipSuccess;
}

// ---- cases ----------------------------------------------------------------
static void report(int g, bool ok, const std::string& what) {
    g_groups[g].cases += 1;
    if (!ok) g_groups[g].failed.push_back(what);
}

static bool rotate_case(int64_t n, int mb, int p) {
    const int ld = mb + 2;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Buf V, Y;
    V.h.assign((size_t)(n + GUARD_ROWS) * ld, SENT);
    for (int64_t r = 0; r < n; ++r)
        for (int c = 0; c < ld; ++c) V.h[r * ld + c] = c < mb ? rint_in(4) : nan;
    Y.h.resize((size_t)mb * p);
    for (double& y : Y.h) y = rint_in(3);
    dvec expect = V.h;  // read into the expectation before the kernel touches V
    for (int64_t r = 0; r < n; ++r)
        for (int c = 0; c < p; ++c) {
            double s = 0.0;
            for (int k = 0; k < mb; ++k) s += V.h[r * ld + k] * Y.h[(size_t)k * p + c];
            expect[r * ld + c] = s;
        }
    if (!V.up() || !Y.up()) return false;
    if (!hip_ok(op_rotate(n, mb, p, V.d, ld, Y.d)) || !V.down()) return false;
    int64_t bad = -1;
    for (size_t i = 0; i < expect.size() && bad < 0; ++i)
        if (!same_bits(expect[i], V.h[i])) bad = (int64_t)i;
    char buf[160];
    snprintf(buf, sizeof buf, "rotate n=%lld mb=%d p=%d: first mismatch at row %lld col %lld", (long long)n, mb, p,
             (long long)(bad / ld), (long long)(bad % ld));
    report(0, bad < 0, buf);
    return true;
}

static bool resid_case(int64_t n, int kp) {
    const int ldx = kp + 2, ldax = kp + 4;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int chunks = kt::eig_resid_chunks(n);
    Buf X, AX, Th, Part, Out;
    X.h.assign((size_t)n * ldx, nan);
    AX.h.assign((size_t)n * ldax, nan);
    Th.h.resize(kp);
    for (double& t : Th.h) t = rint_in(2);
    dvec e((size_t)3 * kp, 0.0);
    for (int64_t r = 0; r < n; ++r)
        for (int i = 0; i < kp; ++i) {
            const double x = rint_in(3), y = rint_in(9);
            X.h[r * ldx + i] = x;
            AX.h[r * ldax + i] = y;
            const double d = y - Th.h[i] * x;
            e[i] += d * d;
            e[kp + i] += x * x;
            e[2 * kp + i] += x;
        }
    Part.h.assign((size_t)3 * kp * chunks + 16, SENT);
    Out.h.assign((size_t)3 * kp + 16, SENT);
    if (!X.up() || !AX.up() || !Th.up() || !Part.up() || !Out.up()) return false;
    if (!hip_ok(op_resid(n, kp, X.d, ldx, AX.d, ldax, Th.d, Part.d, Out.d)) || !Out.down() || !Part.down())
        return false;
    bool ok = true;
    for (int i = 0; i < 3 * kp; ++i) ok = ok && Out.h[i] == e[i];
    for (int i = 0; i < 16; ++i)
        ok = ok && same_bits(Out.h[3 * kp + i], SENT) && same_bits(Part.h[(size_t)3 * kp * chunks + i], SENT);
    for (size_t i = 0; i < (size_t)3 * kp * chunks; ++i) ok = ok && std::isfinite(Part.h[i]) && Part.h[i] != SENT;
    char buf[96];
    snprintf(buf, sizeof buf, "resid n=%lld kp=%d", (long long)n, kp);
    report(1, ok, buf);
    return true;
}

static std::vector<int> random_perm(int n) {
    std::vector<int> p(n);
    for (int i = 0; i < n; ++i) p[i] = i;
    for (int i = n - 1; i > 0; --i) std::swap(p[i], p[(int)(rnd() % (uint64_t)(i + 1))]);
    return p;
}

// one block (un-permuted: row perm[r] of the result is device row r)
static bool start_block(int64_t n, uint64_t seed, int64_t col0, unsigned mask, bool ones, const std::vector<int>* perm,
                        dvec& out, bool& untouched_ok) {
    const int ld = 18;
    Buf X;
    X.h.assign((size_t)(n + GUARD_ROWS) * ld, SENT);
    if (!X.up()) return false;
    int* dperm = nullptr;
    if (perm) {
        if (g_host) dperm = const_cast<int*>(perm->data());
        else if (!hip_ok(hipMalloc((void**)&dperm, sizeof(int) * n)) ||
                 !hip_ok(hipMemcpy(dperm, perm->data(), sizeof(int) * n, hipMemcpyHostToDevice)))
            return false;
    }
    const bool ran = hip_ok(op_start(n, seed, col0, mask, ones, dperm, X.d, ld)) && X.down();
    if (perm && !g_host) (void)hipFree(dperm);
    if (!ran) return false;
    out.assign((size_t)n * 16, 0.0);
    untouched_ok = true;
    for (int64_t r = 0; r < n + GUARD_ROWS; ++r)
        for (int c = 0; c < ld; ++c) {
            const double v = X.h[r * ld + c];
            if (r < n && c < 16 && (mask & (1u << c))) out[(size_t)(perm ? (*perm)[r] : r) * 16 + c] = v;
            else untouched_ok = untouched_ok && same_bits(v, SENT);
        }
    return true;
}

static bool start_case(int64_t n, uint64_t seed, int64_t col0, unsigned mask, bool ones) {
    const std::vector<int> p1 = random_perm((int)n), p2 = random_perm((int)n);
    dvec b0, b1, b2;
    bool u0, u1, u2;
    if (!start_block(n, seed, col0, mask, ones, nullptr, b0, u0) ||
        !start_block(n, seed, col0, mask, ones, &p1, b1, u1) || !start_block(n, seed, col0, mask, ones, &p2, b2, u2))
        return false;
    bool ok = u0 && u1 && u2;
    for (int64_t i = 0; i < n && ok; ++i)
        for (int c = 0; c < 16; ++c) {
            if (!(mask & (1u << c))) continue;
            const double e = (ones && c == 0) ? 1.0 / sqrt((double)n) : sign_of(seed, (uint64_t)(col0 + c), (uint64_t)i);
            ok = ok && same_bits(b0[i * 16 + c], e) && same_bits(b1[i * 16 + c], e) && same_bits(b2[i * 16 + c], e);
        }
    char buf[128];
    snprintf(buf, sizeof buf, "start n=%lld seed=%llu col0=%lld mask=%04x ones=%d", (long long)n,
             (unsigned long long)seed, (long long)col0, mask, (int)ones);
    report(2, ok, buf);
    return true;
}

static bool run_all() {
    const int rot_n[] = {1, 63, 64, 65, 257}, rot_mb[] = {32, 128}, rot_p[] = {16, 32, 48};
    for (int n : rot_n)
        for (int mb : rot_mb)
            for (int p : rot_p)
                if (p <= mb && !rotate_case(n, mb, p)) return false;
    const int res_n[] = {1, 127, 128, 129, 1000}, res_kp[] = {16, 32};
    for (int n : res_n)
        for (int kp : res_kp)
            if (!resid_case(n, kp)) return false;
    const int st_n[] = {1, 33, 1000};
    for (int n : st_n) {
        if (!start_case(n, 0, 0, 0xFFFFu, true)) return false;
        if (!start_case(n, 12345, 16, 0xFFFFu, false)) return false;
        if (!start_case(n, 7, 32, 0x0A5Bu, false)) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--host")) g_host = true;
        else {
            fprintf(stderr, "usage: eig_check [--host]\n");
            return 64;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    run_all();
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"mode\": \"%s\", ", g_host ? "host" : "device");
    if (g_hip_err) printf("\"hip_error\": \"%s\", ", g_hip_err);
    printf("\"groups\": {");
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
