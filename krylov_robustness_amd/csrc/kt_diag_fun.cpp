// kt_diag_fun.cpp -- kt_diag_fun: the deflated stochastic estimator of diag f(A)
// (compute_centrality.m:9-10 with f = exp).
//
// Per sweep of P probes, on the hubs-first CSR in its row order:
//   start    z' = z - Q (Q'z) and ||z'||^2 (k_diag_qtz, k_diag_start; z comes
//            from the counter RNG in registers, Q'z from workgroup partials
//            summed in a fixed order)
//   sweep    a y-form sweep that forms its own Lanczos basis (YBlockSweep with
//            `basis`); one whose cancellation guard trips, or that breaks
//            down, is redone whole by the explicit CGS2 sweep with its basis
//            (KT_SLQ_YFORM=0, the hot path's switch: every sweep explicit)
//   weights  host pool: ||z'|| f(T) e1 per column from its record, cut at a
//            lucky breakdown; the m x P table and the cuts go back
//   combine  one pass over the basis forms y, the partials of Q'y and (kdef
//            = 0) the row sums at once; with deflation a second pass over the
//            n x P block y alone forms z .* (y - Q (Q'y)) and the row sums
// The sweeps of a group run side by side on the sweep lanes; the combine and
// accumulate launches of all sweeps are queued on one stream in sweep order,
// so dsum and dsum2 do not depend on the lane count.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>

#include "kt_launch.h"
#include "kt_pool.h"
#include "kt_slq.h"

namespace kt {

namespace {

// one sweep lane's buffers (the lane's SweepBufs hold the sweep's own blocks)
struct DiagLane {
    DevMat basis;   // m slots of n x P
    DevMat x;       // z' (the sweep's start block); after the sweep, y
    DevBuf part;    // workgroup partials: grid x max(KP, 1) P
    DevBuf small;   // [c = Q'z or Q'y (KP P) | ||z'||^2 (P) | W (m P) | depth (P ints)]
    double *c = nullptr, *n2 = nullptr, *W = nullptr;
    int* depth = nullptr;
    hipStream_t st = nullptr;
};

// the deflation block's padded width
int defl_width(int64_t kdef) { return kdef == 0 ? 0 : kdef == 1 ? 1 : kdef <= 4 ? 4 : 16; }

void check_orthonormal(const double* Q, int64_t n, int k) {
    double worst = 0.0;
    for (int a = 0; a < k; ++a)
        for (int b = a; b < k; ++b) {
            const double* qa = Q + (size_t)a * n;
            const double* qb = Q + (size_t)b * n;
            double s = 0.0;
            for (int64_t i = 0; i < n; ++i) s += qa[i] * qb[i];
            const double e = std::fabs(s - (a == b ? 1.0 : 0.0));
            if (!(e <= worst)) worst = e;  // a NaN sticks
        }
    if (!(worst <= 1e-8)) fail(KT_ERR_ARG, "kt_diag_fun: the columns of Q are not orthonormal (max |Q'Q - I| > 1e-8)");
}

void diag_fun(kt_matrix_s* A, int fun, int m, uint64_t seed, int64_t probe_offset, int64_t nprobes, int block,
              int64_t kdef, const double* Q, double* dsum, double* dsum2, double* d0, double* sum_q,
              double* sum_q2) {
    if (fun < KT_FUN_EXP || fun > KT_FUN_SQRT) fail(KT_ERR_ARG, "unknown fun code");
    if (m < 1 || m > 256) fail(KT_ERR_ARG, "m must be in [1, 256]");
    if (nprobes < 1 || probe_offset < 0) fail(KT_ERR_ARG, "kt_diag_fun: nprobes >= 1 and probe_offset >= 0");
    if (block != 0 && !(block >= 1 && block <= 16 && (block & (block - 1)) == 0))
        fail(KT_ERR_ARG, "kt_diag_fun: block must be 0 or a power of two <= 16");
    if (kdef < 0 || kdef > 16) fail(KT_ERR_ARG, "kt_diag_fun: 0 <= kdef <= 16");
    if ((kdef == 0) != (Q == nullptr)) fail(KT_ERR_ARG, "kt_diag_fun: Q is NULL exactly when kdef == 0");
    if (!dsum) fail(KT_ERR_ARG, "kt_diag_fun: dsum is NULL");
    kt_context_s* ctx = A->ctx;
    Workspace& w = ctx->ws;
    if (w.slq_submitted != w.slq_collected)
        fail(KT_ERR_ARG, "kt_diag_fun: kt_slq_submit calls are outstanding on this context");
    if (sum_q) *sum_q = 0.0;
    if (sum_q2) *sum_q2 = 0.0;
    const int64_t n64 = A->n;
    if (n64 == 0) return;
    const int n = (int)n64, k = (int)kdef, KP = defl_width(kdef), P = block ? block : 16;
    if (k) check_orthonormal(Q, n64, k);
    KT_HIP(hipSetDevice(ctx->device));
    const DevCSR& M = hub_csr(A);
    const int* perm = M.perm;
    prof_recycle(ctx);

    // Q in original numbering (d0) and in the sweep's row order, n x KP row-major
    DevMat Qn, Qh;
    const double* Qs = nullptr;
    if (k) {
        Qn.alloc(ctx, n64, KP);
        upload_rows(A, Q, k, Qn.col(0), KP);
        // d0: G = f(A) Q by the column driver, H = Q'G, one streaming kernel
        DevMat Gn, d0d;
        Gn.alloc(ctx, n64, KP);
        lanczos_columns(A, Qn.col(0), KP, k, m, fun, nullptr, Gn.col(0), KP);
        const double* H = gram_device(ctx, n64, Qn.col(0), KP, k, Gn.col(0), KP, k);
        if (d0) {
            d0d.alloc(ctx, n64, 1, false);
            KT_HIP(launch_diag_d0(n, k, Qn.col(0), Gn.col(0), KP, H, d0d.col(0), ctx->stream));
            KT_HIP(hipMemcpyAsync(d0, d0d.col(0), sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (perm) {
            Qh.alloc(ctx, n64, KP, false);
            KT_HIP(launch_perm_rows(n, KP, perm, 1, Qn.col(0), KP, Qh.col(0), KP, ctx->stream));
            Qs = Qh.col(0);
        } else {
            Qs = Qn.col(0);
        }
        KT_HIP(hipStreamSynchronize(ctx->stream));
    } else if (d0) {
        std::fill(d0, d0 + n, 0.0);
    }

    const int64_t nsw = (nprobes + P - 1) / P;
    // KT_SLQ_LANES=L (<= 4), as the y-form sweeps of kt_slq_trace: 2 by default
    const char* le = getenv("KT_SLQ_LANES");
    const int lanes_env = le ? std::max(1, std::min(4, atoi(le))) : 2;
    int lanes = (int)std::max<int64_t>(1, std::min<int64_t>(nsw, lanes_env));
    const int grid = diag_grid(n, P), KK = std::max(KP, 1);
    std::vector<DiagLane> L(lanes);
    for (int l = 0; l < lanes; ++l) {
        DiagLane& d = L[l];
        try {
            d.basis.alloc(ctx, (int64_t)m * n64, P, false);
        } catch (const Status& s) {
            // a basis per lane in use: fewer lanes if the next one does not fit
            if (l == 0 || s.code != KT_ERR_ALLOC)
                fail(s.code, "kt_diag_fun: the Lanczos basis of one sweep (m n block doubles) does not fit: " + s.msg);
            lanes = l;
            L.resize(l);
            break;
        }
        d.x.alloc(ctx, n64, P, false);
        d.part.ensure(sizeof(double) * (size_t)grid * KK * P);
        d.small.ensure(sizeof(double) * ((size_t)KK * P + P + (size_t)m * P) + sizeof(int) * P);
        d.c = d.small.as<double>();
        d.n2 = d.c + (size_t)KK * P;
        d.W = d.n2 + P;
        d.depth = reinterpret_cast<int*>(d.W + (size_t)m * P);
        if (l && !ctx->aux_stream[l - 1])
            KT_HIP(hipStreamCreateWithFlags(&ctx->aux_stream[l - 1], hipStreamNonBlocking));
        d.st = l ? ctx->aux_stream[l - 1] : ctx->stream;
    }
    // the sums, alive for the call; added to in sweep order on ctx->stream
    DevMat acc;
    acc.alloc(ctx, 2 * n64, 1);
    double* dsum_d = acc.col(0);
    double* dsum2_d = dsum_d + n;
    // pinned, per lane: [record 3 m P | guard P | ||z'||^2 P | W m P | depth P ints]
    const size_t rec = (size_t)3 * m * P + P, per = rec + P + (size_t)m * P + P;
    PinnedBuf pin;
    pin.ensure(sizeof(double) * per * lanes);
    KT_HIP(hipStreamSynchronize(ctx->stream));  // the lanes read Q and the zeroed sums

    std::vector<double> qv((size_t)nprobes, 0.0);
    std::vector<std::vector<double>> hists(lanes);
    for (int64_t s0 = 0; s0 < nsw; s0 += lanes) {
        const int g = (int)std::min<int64_t>(lanes, nsw - s0);
        auto base_of = [&](int l) { return probe_offset + (s0 + l) * P; };
        auto live_of = [&](int l) { return (int)std::min<int64_t>(P, nprobes - (s0 + l) * P); };
        auto host_of = [&](int l) { return pin.as<double>() + per * l; };
        // start blocks and sweeps, the lanes' launches queued side by side
        std::vector<std::unique_ptr<YBlockSweep>> ys;
        std::vector<std::unique_ptr<ExplicitSweep>> ex;  // KT_SLQ_YFORM=0: every sweep explicit (the A/B)
        for (int l = 0; l < g; ++l) {
            DiagLane& d = L[l];
            const int nc = live_of(l);
            prof_begin(ctx, PROF_DIAG_START, d.st, P);
            if (KP) {
                KT_HIP(launch_diag_qtz(P, KP, grid, n, seed, base_of(l), nc, perm, Qs, d.part.as<double>(), d.st));
                KT_HIP(launch_diag_sum_parts(grid, KP * P, d.part.as<double>(), d.c, d.st));
            }
            KT_HIP(launch_diag_start(P, KP, grid, n, seed, base_of(l), nc, perm, Qs, d.c, d.x.col(0),
                                     d.part.as<double>(), d.st));
            KT_HIP(launch_diag_sum_parts(grid, P, d.part.as<double>(), d.n2, d.st));
            prof_end(ctx, PROF_DIAG_START, d.st);
            KT_HIP(hipMemcpyAsync(host_of(l) + rec, d.n2, sizeof(double) * P, hipMemcpyDeviceToHost, d.st));
            if (ctx->yform)
                ys.emplace_back(
                    new YBlockSweep(A, M, P, m, d.x.col(0), P, nc, d.n2, host_of(l), l, d.basis.col(0), nc));
            else
                ex.emplace_back(new ExplicitSweep(A, M, P, m, 0, 0, d.x.col(0), P, nc, d.n2, host_of(l), &d.basis,
                                                  &hists[l], l, P));
        }
        for (auto& y : ys) y->start();
        for (auto& e : ex) e->start();
        for (int j = 0; j < m; ++j) {
            for (auto& y : ys)
                if (j + 1 < m) y->step(j);
            for (auto& e : ex) e->step(j);
        }
        for (auto& y : ys) y->finish();
        for (auto& e : ex) e->finish();
        for (int l = 0; l < g; ++l) KT_HIP(hipStreamSynchronize(L[l].st));
        // a sweep with a guarded (or broken-down) column: redone whole by the
        // explicit sweep with its basis (slot j = u_j, n x P; v_j = s_j u_j)
        std::vector<char> explicit_basis(g, ctx->yform ? 0 : 1);
        for (int l = 0; l < g && ctx->yform; ++l) {
            double* R = host_of(l);
            const double* gd = R + (size_t)3 * m * P;
            const double* n2 = R + rec;
            bool bad = false;
            for (int c = 0; c < live_of(l); ++c) bad |= n2[c] > 0.0 && !(gd[c] >= kYformGuard);
            if (!bad) continue;
            DiagLane& d = L[l];
            lanczos_sweep(A, M, P, m, 0, 0, d.x.col(0), P, live_of(l), d.n2, R, &d.basis, &hists[l], l, P);
            KT_HIP(hipStreamSynchronize(d.st));
            explicit_basis[l] = 1;
            ctx->yform_redone += 1;
        }
        // per column on the host pool: the quadratic form and the basis weights
        std::vector<int> mdepth(g, 0);
        HostPool::get().run(g * P, [&](int t) {
            const int l = t / P, c = t % P;
            double* R = host_of(l);
            const double* n2 = R + rec;
            double* W = R + rec + P;
            int* dep = reinterpret_cast<int*>(W + (size_t)m * P);
            for (int j = 0; j < m; ++j) W[(size_t)j * P + c] = 0.0;
            dep[c] = 0;
            if (c >= live_of(l) || !(n2[c] > 0.0)) return;
            std::vector<double> al(m), off(m), fe1(m);
            const int steps = record_tridiag(R, m, P, c, al.data(), off.data());
            const double qd = tridiag_fun_e1(steps, al.data(), off.data(), fun, fe1.data());
            qv[(size_t)((s0 + l) * P + c)] = n2[c] * qd;
            const double nx = std::sqrt(n2[c]);
            for (int j = 0; j < steps; ++j)
                W[(size_t)j * P + c] = explicit_basis[l] ? nx * hists[l][(size_t)j * P + c] * fe1[j] : nx * fe1[j];
            dep[c] = steps;
        }, 4);
        // combine and accumulate, every sweep on ctx->stream in sweep order
        hipStream_t st = ctx->stream;
        for (int l = 0; l < g; ++l) {
            DiagLane& d = L[l];
            double* R = host_of(l);
            const int* dep = reinterpret_cast<const int*>(R + rec + P + (size_t)m * P);
            int md = 0;
            for (int c = 0; c < P; ++c) md = std::max(md, dep[c]);
            KT_HIP(hipMemcpyAsync(d.W, R + rec + P, sizeof(double) * (size_t)m * P + sizeof(int) * P,
                                  hipMemcpyHostToDevice, st));
            prof_begin(ctx, PROF_DIAG, st, P);
            KT_HIP(launch_diag_combine(P, KP, grid, n, m, md, d.basis.col(0), (int64_t)n * P, d.W, d.depth, seed,
                                       base_of(l), perm, Qs, d.x.col(0), d.part.as<double>(), dsum_d, dsum2_d, st));
            if (KP) {
                KT_HIP(launch_diag_sum_parts(grid, KP * P, d.part.as<double>(), d.c, st));
                KT_HIP(launch_diag_finish(P, KP, grid, n, seed, base_of(l), perm, Qs, d.c, d.x.col(0), dsum_d, dsum2_d,
                                          st));
            }
            prof_end(ctx, PROF_DIAG, st);
        }
        // the next group reuses the lanes' bases and the pinned blocks
        KT_HIP(hipStreamSynchronize(st));
    }
    KT_HIP(hipMemcpyAsync(dsum, dsum_d, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (dsum2) KT_HIP(hipMemcpyAsync(dsum2, dsum2_d, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    double s1 = 0.0, s2 = 0.0;
    for (int64_t p = 0; p < nprobes; ++p) {
        s1 += qv[p];
        s2 += qv[p] * qv[p];
    }
    if (sum_q) *sum_q = s1;
    if (sum_q2) *sum_q2 = s2;
}

}  // namespace

}  // namespace kt

extern "C" int kt_diag_fun(kt_matrix_t A, int fun, int m, uint64_t seed, int64_t probe_offset, int64_t nprobes,
                           int block, int64_t kdef, const double* Q, double* dsum, double* dsum2, double* d0,
                           double* sum_q, double* sum_q2) {
    try {
        if (!A) kt::fail(KT_ERR_ARG, "A is NULL");
        kt::diag_fun(A, fun, m, seed, probe_offset, nprobes, block, kdef, Q, dsum, dsum2, d0, sum_q, sum_q2);
    } catch (const kt::Status& s) {
        kt::set_error(s.msg);
        return s.code;
    } catch (const std::exception& e) {
        kt::set_error(e.what());
        return KT_ERR_ARG;
    }
    return KT_OK;
}
