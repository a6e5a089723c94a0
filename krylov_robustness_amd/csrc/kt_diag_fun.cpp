// kt_diag_fun.cpp -- kt_diag_fun: the deflated stochastic estimator of diag f(A)
// (compute_centrality.m:9-10 with f = exp).
//
// Per sweep of P probes, on the hubs-first CSR in its row order:
//   start    z' = z - Q (Q'z) and ||z'||^2 (k_diag_qtz, k_diag_start; z comes
//            from the counter RNG in registers, Q'z from workgroup partials
//            summed in a fixed order)
//   sweep    a y-form sweep that forms its own Lanczos basis (a block-seeded
//            YSweep with `basis`); one whose cancellation guard trips, or that
//            breaks down, is redone whole by the explicit CGS2 sweep with its basis
//            (KT_SLQ_YFORM=0, the hot path's switch: every sweep explicit)
//   weights  host pool: ||z'|| f(T) e1 per column from its record, cut at a
//            lucky breakdown; the m x P table and the cuts go back
//   combine  one pass over the basis forms y, the partials of Q'y and (kdef
//            = 0) the row sums at once; with deflation a second pass over the
//            n x P block y alone forms z .* (y - Q (Q'y)) and the row sums
// The sweeps of a group run side by side on the sweep lanes; the combine and
// accumulate launches of all sweeps are queued on one stream in sweep order,
// so dsum and dsum2 do not depend on the lane count.
//
// kt_entries_fun runs the same pipeline -- probe_sweeps below
// is the one driver -- with its own steps passed in: the combine stores y for
// every kdef, and k_entries_accumulate gathers the two rows of each pair.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>

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

void check_orthonormal(const std::string& who, const double* Q, int64_t n, int k) {
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
    if (!(worst <= 1e-8)) fail(KT_ERR_ARG, who + ": the columns of Q are not orthonormal (max |Q'Q - I| > 1e-8)");
}

// the deflation blocks once G and H are formed (kdef > 0): Qn, Gn n x KP
// row-major in original numbering, H k x k column-major, all on the device
struct DeflBlocks {
    int k, KP;
    const double *Qn, *Gn, *H;
};
// one sweep's combine inputs, its launches queued on st (= ctx->stream)
struct SweepOut {
    int P, KP, grid, n, m, md;
    const double* basis;  // m slots of n x P
    const double* W;      // m x P weights, then the P depths
    const int* depth;
    int64_t base;         // the sweep's first probe
    const int* perm;
    const double* Qs;     // Q in the sweep's row order
    double* c;            // KP x P: Q'y goes here
    double* Y;            // n x P
    double* part;
    hipStream_t st;
};
// The steps an estimator passes to probe_sweeps:
//   defl     once, with the deflation blocks, on ctx->stream (kdef > 0 only)
//   prepare  once, after the lanes' buffers are allocated and before the
//            stream sync ahead of the first sweep: the sums that live for the call
//   combine  per sweep in sweep order on ctx->stream: combine and accumulate
struct SweepSteps {
    std::function<void(const DeflBlocks&)> defl;
    std::function<void()> prepare;
    std::function<void(const SweepOut&)> combine;
};

void probe_sweeps(const std::string& who, kt_matrix_s* A, int fun, int m, uint64_t seed, int64_t probe_offset,
                  int64_t nprobes, int block, int64_t kdef, const double* Q, const SweepSteps& steps,
                  double* sum_q, double* sum_q2) {
    if (fun < KT_FUN_EXP || fun > KT_FUN_SQRT) fail(KT_ERR_ARG, "unknown fun code");
    if (m < 1 || m > 256) fail(KT_ERR_ARG, "m must be in [1, 256]");
    if (nprobes < 1 || probe_offset < 0) fail(KT_ERR_ARG, who + ": nprobes >= 1 and probe_offset >= 0");
    if (block != 0 && !(block >= 1 && block <= 16 && (block & (block - 1)) == 0))
        fail(KT_ERR_ARG, who + ": block must be 0 or a power of two <= 16");
    if (kdef < 0 || kdef > 16) fail(KT_ERR_ARG, who + ": 0 <= kdef <= 16");
    if ((kdef == 0) != (Q == nullptr)) fail(KT_ERR_ARG, who + ": Q is NULL exactly when kdef == 0");
    kt_context_s* ctx = A->ctx;
    Workspace& w = ctx->ws;
    if (w.slq_submitted != w.slq_collected)
        fail(KT_ERR_ARG, who + ": kt_slq_submit calls are outstanding on this context");
    if (sum_q) *sum_q = 0.0;
    if (sum_q2) *sum_q2 = 0.0;
    const int64_t n64 = A->n;
    if (n64 == 0) return;
    const int n = (int)n64, k = (int)kdef, KP = defl_width(kdef), P = block ? block : 16;
    if (k) check_orthonormal(who, Q, n64, k);
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
        DevMat Gn;
        Gn.alloc(ctx, n64, KP);
        lanczos_columns(A, Qn.col(0), KP, k, m, fun, nullptr, Gn.col(0), KP);
        const double* H = gram_device(ctx, n64, Qn.col(0), KP, k, Gn.col(0), KP, k);
        steps.defl(DeflBlocks{k, KP, Qn.col(0), Gn.col(0), H});
        if (perm) {
            Qh.alloc(ctx, n64, KP, false);
            KT_HIP(launch_perm_rows(n, KP, perm, 1, Qn.col(0), KP, Qh.col(0), KP, ctx->stream));
            Qs = Qh.col(0);
        } else {
            Qs = Qn.col(0);
        }
        KT_HIP(hipStreamSynchronize(ctx->stream));
    }

    const int64_t nsw = (nprobes + P - 1) / P;
    // KT_SLQ_LANES=L (<= 4), as the y-form sweeps of kt_slq_trace: 2 by default
    const int lanes_env = std::max(1, std::min(4, slq_lanes_env(2)));
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
                fail(s.code, who + ": the Lanczos basis of one sweep (m n block doubles) does not fit: " + s.msg);
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
        d.st = lane_stream(ctx, l);
    }
    // the sums, alive for the call; added to in sweep order on ctx->stream
    steps.prepare();
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
        SweepList grp;
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
                grp.emplace_back(new YSweep(A, M, P, m, d.x.col(0), P, nc, d.n2, host_of(l), l, d.basis.col(0), nc));
            else  // KT_SLQ_YFORM=0: every sweep explicit (the A/B)
                grp.emplace_back(new ExplicitSweep(A, M, P, m, 0, 0, d.x.col(0), P, nc, d.n2, host_of(l), &d.basis,
                                                   &hists[l], l, P));
        }
        run_sweeps(grp);
        for (int l = 0; l < g; ++l) KT_HIP(hipStreamSynchronize(L[l].st));
        // a sweep with a guarded (or broken-down) column: redone whole by the
        // explicit sweep with its basis (slot j = u_j, n x P; v_j = s_j u_j)
        std::vector<char> explicit_basis(g, ctx->yform ? 0 : 1);
        for (int l = 0; l < g && ctx->yform; ++l) {
            double* R = host_of(l);
            if (!guard_tripped(R, m, P, live_of(l), R + rec)) continue;
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
            const int steps = record_tridiag(R, m, m, P, c, al.data(), off.data());
            const double qd = tridiag_fun_e1(steps, al.data(), off.data(), fun, fe1.data());
            qv[(size_t)((s0 + l) * P + c)] = n2[c] * qd;
            basis_weights(steps, std::sqrt(n2[c]), fe1.data(), explicit_basis[l] ? hists[l].data() + c : nullptr, P,
                          W + c, P);
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
            steps.combine(SweepOut{P, KP, grid, n, m, md, d.basis.col(0), d.W, d.depth, base_of(l), perm, Qs, d.c,
                                   d.x.col(0), d.part.as<double>(), st});
        }
        // the next group reuses the lanes' bases and the pinned blocks
        KT_HIP(hipStreamSynchronize(st));
    }
    double s1 = 0.0, s2 = 0.0;
    for (int64_t p = 0; p < nprobes; ++p) {
        s1 += qv[p];
        s2 += qv[p] * qv[p];
    }
    if (sum_q) *sum_q = s1;
    if (sum_q2) *sum_q2 = s2;
}

void diag_fun(kt_matrix_s* A, int fun, int m, uint64_t seed, int64_t probe_offset, int64_t nprobes, int block,
              int64_t kdef, const double* Q, double* dsum, double* dsum2, double* d0, double* sum_q,
              double* sum_q2) {
    if (!dsum) fail(KT_ERR_ARG, "kt_diag_fun: dsum is NULL");
    kt_context_s* ctx = A->ctx;
    const int64_t n64 = A->n;
    const int n = (int)n64;
    DevMat acc, d0d;
    double *dsum_d = nullptr, *dsum2_d = nullptr;
    SweepSteps steps;
    steps.defl = [&](const DeflBlocks& b) {
        if (!d0) return;
        d0d.alloc(ctx, n64, 1, false);
        KT_HIP(launch_diag_d0(n, b.k, b.Qn, b.Gn, b.KP, b.H, d0d.col(0), ctx->stream));
        KT_HIP(hipMemcpyAsync(d0, d0d.col(0), sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    };
    // the sums, alive for the call; added to in sweep order on ctx->stream
    steps.prepare = [&]() {
        acc.alloc(ctx, 2 * n64, 1);
        dsum_d = acc.col(0);
        dsum2_d = dsum_d + n;
    };
    steps.combine = [&](const SweepOut& s) {
        prof_begin(ctx, PROF_DIAG, s.st, s.P);
        KT_HIP(launch_diag_combine(s.P, s.KP, s.grid, s.n, s.m, s.md, s.basis, (int64_t)s.n * s.P, s.W, s.depth, seed,
                                   s.base, s.perm, s.Qs, s.Y, s.part, dsum_d, dsum2_d, s.st));
        if (s.KP) {
            KT_HIP(launch_diag_sum_parts(s.grid, s.KP * s.P, s.part, s.c, s.st));
            KT_HIP(launch_diag_finish(s.P, s.KP, s.grid, s.n, seed, s.base, s.perm, s.Qs, s.c, s.Y, dsum_d, dsum2_d,
                                      s.st));
        }
        prof_end(ctx, PROF_DIAG, s.st);
    };
    probe_sweeps("kt_diag_fun", A, fun, m, seed, probe_offset, nprobes, block, kdef, Q, steps, sum_q, sum_q2);
    if (n64 == 0) return;
    if (!kdef && d0) std::fill(d0, d0 + n, 0.0);
    KT_HIP(hipMemcpyAsync(dsum, dsum_d, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (dsum2) KT_HIP(hipMemcpyAsync(dsum2, dsum2_d, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
}

void entries_fun(kt_matrix_s* A, int fun, int m, uint64_t seed, int64_t probe_offset, int64_t nprobes, int block,
                 int64_t kdef, const double* Q, int64_t npairs, const int64_t* ei, const int64_t* ej, double* esum,
                 double* esum2, double* e0, double* sum_q, double* sum_q2) {
    if (npairs < 1) fail(KT_ERR_ARG, "kt_entries_fun: npairs >= 1");
    if (!ei || !ej) fail(KT_ERR_ARG, "kt_entries_fun: ei or ej is NULL");
    if (!esum) fail(KT_ERR_ARG, "kt_entries_fun: esum is NULL");
    kt_context_s* ctx = A->ctx;
    const int64_t n64 = A->n;
    for (int64_t e = 0; e < npairs; ++e)
        if (ei[e] < 0 || ei[e] >= n64 || ej[e] < 0 || ej[e] >= n64)
            fail(KT_ERR_ARG, "kt_entries_fun: pair " + std::to_string(e) + " has an index outside [0, n)");
    // the pair table, the sums and e0, alive for the call
    DevMat tab, acc, e0d;
    double *esum_d = nullptr, *esum2_d = nullptr;
    // KT_ENTRIES_SORT=1 (the A/B of tests/perf/bench_entries.py): the table in
    // ascending r_i, table row t holding pair slot[t]; every pair still owns
    // its sums, so the results are the same bits
    const char* se = getenv("KT_ENTRIES_SORT");
    const bool sorted = se && atoi(se) != 0;
    std::vector<int64_t> slot;
    auto upload_table = [&]() {
        if (tab.ptr) return;
        // rows of the sweep's order through the inverse of the hub copy's perm
        const bool relabelled = hub_csr(A).perm != nullptr;
        std::vector<int32_t> h(4 * (size_t)npairs);
        auto row_of = [&](int64_t i) { return relabelled ? A->old2new[i] : (int32_t)i; };
        if (sorted) {
            slot.resize((size_t)npairs);
            for (int64_t e = 0; e < npairs; ++e) slot[e] = e;
            std::stable_sort(slot.begin(), slot.end(),
                             [&](int64_t a, int64_t b) { return row_of(ei[a]) < row_of(ei[b]); });
        }
        for (int64_t e = 0; e < npairs; ++e) {
            const int64_t src = sorted ? slot[e] : e;
            const int32_t i = (int32_t)ei[src], j = (int32_t)ej[src];
            h[4 * e + 0] = row_of(i);
            h[4 * e + 1] = row_of(j);
            h[4 * e + 2] = i;
            h[4 * e + 3] = j;
        }
        tab.alloc(ctx, 2 * npairs, 1, false);  // 16 bytes per pair
        KT_HIP(hipMemcpyAsync(tab.ptr, h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice, ctx->stream));
        KT_HIP(hipStreamSynchronize(ctx->stream));  // h goes out of scope
    };
    SweepSteps steps;
    steps.defl = [&](const DeflBlocks& b) {
        if (!e0) return;
        upload_table();
        e0d.alloc(ctx, npairs, 1, false);
        prof_begin(ctx, PROF_ENTRIES, ctx->stream, 0);
        KT_HIP(launch_entries_e0(npairs, tab.ptr, b.k, b.Qn, b.Gn, b.KP, b.H, e0d.col(0), ctx->stream));
        prof_end(ctx, PROF_ENTRIES, ctx->stream);
        KT_HIP(hipMemcpyAsync(e0, e0d.col(0), sizeof(double) * (size_t)npairs, hipMemcpyDeviceToHost, ctx->stream));
    };
    steps.prepare = [&]() {
        upload_table();
        acc.alloc(ctx, 2 * npairs, 1);
        esum_d = acc.col(0);
        esum2_d = esum_d + npairs;
    };
    steps.combine = [&](const SweepOut& s) {
        // y for every kdef (the combine's sums are kt_diag_fun's: not formed here)
        prof_begin(ctx, PROF_DIAG, s.st, s.P);
        if (s.KP) {
            KT_HIP(launch_diag_combine(s.P, s.KP, s.grid, s.n, s.m, s.md, s.basis, (int64_t)s.n * s.P, s.W, s.depth,
                                       seed, s.base, s.perm, s.Qs, s.Y, s.part, nullptr, nullptr, s.st));
            KT_HIP(launch_diag_sum_parts(s.grid, s.KP * s.P, s.part, s.c, s.st));
        } else {
            KT_HIP(launch_diag_combine_y(s.P, s.grid, s.n, s.m, s.md, s.basis, (int64_t)s.n * s.P, s.W, s.depth, s.Y,
                                         s.st));
        }
        prof_end(ctx, PROF_DIAG, s.st);
        prof_begin(ctx, PROF_ENTRIES, s.st, s.P);
        KT_HIP(launch_entries_accumulate(s.P, s.KP, npairs, tab.ptr, seed, s.base, s.Qs, s.c, s.Y, esum_d, esum2_d,
                                         s.st));
        prof_end(ctx, PROF_ENTRIES, s.st);
    };
    probe_sweeps("kt_entries_fun", A, fun, m, seed, probe_offset, nprobes, block, kdef, Q, steps, sum_q, sum_q2);
    if (!kdef && e0) std::fill(e0, e0 + npairs, 0.0);
    KT_HIP(hipMemcpyAsync(esum, esum_d, sizeof(double) * (size_t)npairs, hipMemcpyDeviceToHost, ctx->stream));
    if (esum2)
        KT_HIP(hipMemcpyAsync(esum2, esum2_d, sizeof(double) * (size_t)npairs, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    if (sorted) {
        std::vector<double> tmp((size_t)npairs);
        for (double* out : {esum, esum2, kdef ? e0 : nullptr}) {
            if (!out) continue;
            std::copy(out, out + npairs, tmp.begin());
            for (int64_t t = 0; t < npairs; ++t) out[slot[t]] = tmp[t];
        }
    }
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

extern "C" int kt_entries_fun(kt_matrix_t A, int fun, int m, uint64_t seed, int64_t probe_offset, int64_t nprobes,
                              int block, int64_t kdef, const double* Q, int64_t npairs, const int64_t* ei,
                              const int64_t* ej, double* esum, double* esum2, double* e0, double* sum_q,
                              double* sum_q2) {
    try {
        if (!A) kt::fail(KT_ERR_ARG, "A is NULL");
        kt::entries_fun(A, fun, m, seed, probe_offset, nprobes, block, kdef, Q, npairs, ei, ej, esum, esum2, e0,
                        sum_q, sum_q2);
    } catch (const kt::Status& s) {
        kt::set_error(s.msg);
        return s.code;
    } catch (const std::exception& e) {
        kt::set_error(e.what());
        return KT_ERR_ARG;
    }
    return KT_OK;
}
