// kt_slq.cpp -- the probe-Lanczos sweep engine and the hot-path entry point.
//
// One sweep = P independent single-vector Lanczos runs (one n x P block),
// m steps of four launches each (K1 spmm_dot, coef, K2 update, norm; see
// kt_kernels.hip).  The per-column recurrence coefficients (alpha, up, low)
// land in a host record; the host then solves the m x m tridiagonal
// eigenproblems (kt_dense.cpp, as the north star prescribes) and forms
//   q_c = ||x_c||^2 e1' f(T_c) e1,   T_c = (H + H')/2   (trace_fun_update.m:78-81)
// and, when the basis is recorded, f(A) x_c ~= ||x_c|| V_c f(T_c) e1.
// Sweeps are seeded either by the device Rademacher generator (kt_slq_trace,
// the Hutchinson hot path) or by a given device block (the Lanczos-f Afun
// of mc_trace, kt_mctrace.cpp).
#include "kt_slq.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <thread>

#include "kt_launch.h"
#include "kt_pool.h"

namespace kt {

int slq_auto_block(int64_t n, int64_t nprobes) {
    // Largest power-of-two P whose gathered n x P block (8nP bytes) stays
    // within ~160 MB, i.e. inside the 256 MiB Infinity Cache next to the CSR
    // stream; measured best on MI355X for n = 1M (P = 16) and n = 100k
    // (P = 128) -- profiles/r01_sweep.txt.
    int P = 128;
    while (P > 8 && (double)n * 8.0 * P > 160.0e6) P >>= 1;
    while (P > 1 && P / 2 >= nprobes) P >>= 1;
    // at least two sweeps, so the two sweep lanes overlap one sweep's small
    // coefficient launches and pass tails with the other's pass: config 2
    // (n = 100k, 128 probes) 150 evals/s at one P = 128 sweep, 168 at two
    // P = 64 sweeps (profiles/r02_er100k_sweep.txt)
    while (P > 16 && nprobes < 2 * P) P >>= 1;
    return P;
}

hipStream_t lane_stream(kt_context_s* ctx, int lane) {
    if (lane < 0 || lane > 3) fail(KT_ERR_ARG, "sweep lane out of range");
    if (lane && !ctx->aux_stream[lane - 1])
        KT_HIP(hipStreamCreateWithFlags(&ctx->aux_stream[lane - 1], hipStreamNonBlocking));
    return lane ? ctx->aux_stream[lane - 1] : ctx->stream;
}

SweepLane::SweepLane(kt_matrix_s* A, const DevCSR& M, int P, int lane)
    : st(lane_stream(A->ctx, lane)),
      grid(spmm_grid((int)A->n, P, A->ctx->num_cu * 4)),  // 4 row-group workgroups per CU
      lblocks(long_blocks_for(M.n_long, A->ctx->num_cu * 2)),
      grid1(grid + lblocks),
      blk_bytes(sizeof(double) * (size_t)A->n * P),
      w(A->ctx->ws.sweep[lane]) {}

void run_sweeps(const SweepList& sweeps) {
    int steps = 0;
    for (auto& s : sweeps) {
        s->start();
        steps = std::max(steps, s->nsteps());
    }
    for (int j = 0; j < steps; ++j)
        for (auto& s : sweeps)
            if (j < s->nsteps()) s->step(j);
    for (auto& s : sweeps) s->finish();
}

// Run one sweep.  rec_host receives [alpha | up | low][m][P].
// init: if seeded by RNG, `x` == nullptr; else x (device, n x ldx, ncols
// columns, their squared norms in the DEVICE array dnorms2) is copied into
// the sweep block.
ExplicitSweep::ExplicitSweep(kt_matrix_s* A_, const DevCSR& M_, int P_, int m_, uint64_t seed_, int64_t probe_base_,
                             const double* x_, int ldx_, int ncols_, const double* dnorms2_, double* rec_host_,
                             DevMat* basis_, std::vector<double>* scale_hist_, int lane_, int bcols_)
    : A(A_), M(M_), P(P_), m(m_), seed(seed_), probe_base(probe_base_), x(x_), ldx(ldx_), ncols(ncols_),
      dnorms2(dnorms2_), rec_host(rec_host_), basis(basis_), scale_hist(scale_hist_),
      bcols((bcols_ <= 0 || bcols_ > P_) ? P_ : bcols_), n((int)A_->n), L(A_, M_, P_, lane_) {
    SweepBufs& w = L.w;
    w.X0.ensure(L.blk_bytes);
    w.X1.ensure(L.blk_bytes);
    w.Y.ensure(L.blk_bytes);
    w.partial.ensure(sizeof(double) * (size_t)(L.grid1 + L.grid * 3) * P);
    w.k2s.ensure(sizeof(double) * 4 * P);
    w.coef.ensure(sizeof(double) * 2 * P);
    w.scales.ensure(sizeof(double) * 3 * P);
    w.trec.ensure(sizeof(double) * (size_t)3 * m * P);
    part1 = w.partial.as<double>();
    part2 = part1 + (size_t)L.grid1 * P;
    k2s = w.k2s.as<double>();
    coef = w.coef.as<double>();
    trec = w.trec.as<double>();
    Yb = w.Y.as<double>();
    ucur = w.X1.as<double>();
    uprev = w.X0.as<double>();
    sc = w.scales.as<double>();
    sp = sc + P;
    sn = sc + 2 * P;
}

void ExplicitSweep::start() {
    hipStream_t st = L.st;
    if (unit_pos) {
        KT_HIP(hipMemsetAsync(ucur, 0, L.blk_bytes, st));
        if (pair_start)
            KT_HIP(launch_pair_start(n, P, ncols / 2, unit_pos, ucur, sc, k2s, st));
        else
            KT_HIP(launch_unit_start(n, P, ncols, unit_pos, ucur, sc, k2s, st));
    } else if (!x) {
        KT_HIP(launch_rademacher(P, n, seed, probe_base, M.perm, ucur, st));
        KT_HIP(launch_fill(sc, P, 1.0 / std::sqrt((double)n), st));
        KT_HIP(launch_fill(k2s, P, (double)n, st));  // ||z||^2 = n
    } else {
        KT_HIP(hipMemsetAsync(ucur, 0, L.blk_bytes, st));
        KT_HIP(hipMemcpy2DAsync(ucur, sizeof(double) * P, x, sizeof(double) * ldx, sizeof(double) * ncols, (size_t)n,
                                hipMemcpyDeviceToDevice, st));
        // s_0 = 1/||x_c||, ||x_c||^2 from the device norms: no host round trip
        KT_HIP(launch_sweep_scales(dnorms2, ncols, P, 0, sc, k2s, st));
    }
    if (scale_hist) {
        scale_hist->assign((size_t)m * P, 0.0);
        hist_dev = &L.w.hist;
        hist_dev->ensure(sizeof(double) * (size_t)m * P);
    }
    // basis slot j (u_j's first bcols columns, n x bcols row-major) at
    // bbase + j n bcols: slot 0 copied from the start block, slot j + 1
    // stored by step j's K2 as it forms u_{j+1} (no copy pass per step)
    bbase = basis ? basis->col(0) : nullptr;
}

void ExplicitSweep::use_basis_chunks(std::vector<DevMat>* chunks_, int spc_) {
    chunks = chunks_;
    spc = spc_;
}

void ExplicitSweep::use_unit_start(const int* pos_dev) { unit_pos = pos_dev; }

void ExplicitSweep::use_pair_start(const int* pos_dev) {
    unit_pos = pos_dev;
    pair_start = true;
}

// basis slot j (nullptr: the sweep keeps no basis)
double* ExplicitSweep::slot(int j) {
    if (chunks) {
        const size_t k = (size_t)(j / spc);
        if (chunks->size() <= k) chunks->resize(k + 1);
        DevMat& cm = (*chunks)[k];
        if (!cm.ptr) cm.alloc(A->ctx, n, spc * bcols, false);  // every slot used is written by the sweep
        return cm.col(0) + (size_t)(j % spc) * n * bcols;
    }
    return bbase ? bbase + (size_t)j * n * bcols : nullptr;
}

void ExplicitSweep::step(int j) {
    kt_context_s* ctx = A->ctx;
    hipStream_t st = L.st;
    const int first = (j == 0), grid = L.grid, grid1 = L.grid1;
    if ((basis || chunks) && first)  // u_0 into slot 0
        KT_HIP(hipMemcpy2DAsync(slot(0), sizeof(double) * bcols, ucur, sizeof(double) * P, sizeof(double) * bcols,
                                (size_t)n, hipMemcpyDeviceToDevice, st));
    prof_begin(ctx, PROF_SPMM, st, P);
    KT_HIP(launch_spmm_dot(P, ctx->k1_flags | (A->unit_values ? 2 : 0), grid1, M.rowptr, M.col, M.val, n, ucur, sc, Yb,
                           part1, M.long_rows, M.n_long, A->long_thresh, L.lblocks, st));
    prof_end(ctx, PROF_SPMM, st);
    // the coefficient launch also records s_j (v_j = s_j u_j) for a basis sweep
    KT_HIP(launch_coef_cgs2(P, part1, grid1, first, k2s, sc, sp, coef, trec + (size_t)(0 * m + j) * P,
                            trec + (size_t)(1 * m + j) * P, hist_dev ? hist_dev->as<double>() + (size_t)j * P : nullptr,
                            st));
    prof_begin(ctx, PROF_UPDATE, st, P);
    double* rec = ((basis || chunks) && j + 1 < m) ? slot(j + 1) : nullptr;
    KT_HIP(launch_update(P, grid, n, Yb, uprev, ucur, sc, sp, coef, first, part2, st, ctx->k2_nt, rec, bcols));
    prof_end(ctx, PROF_UPDATE, st);
    KT_HIP(launch_norm(P, part2, grid, k2s, sn, trec + (size_t)(2 * m + j) * P, st));
    std::swap(ucur, uprev);  // uprev now holds u_{j+1}
    double* t = sp;
    sp = sc;
    sc = sn;
    sn = t;
}

void ExplicitSweep::finish() {
    KT_HIP(hipMemcpyAsync(rec_host, trec, sizeof(double) * (size_t)3 * m * P, hipMemcpyDeviceToHost, L.st));
    if (scale_hist)
        KT_HIP(hipMemcpyAsync(scale_hist->data(), hist_dev->ptr, sizeof(double) * (size_t)m * P,
                              hipMemcpyDeviceToHost, L.st));
}

void ExplicitSweep::finish(int rows) {
    if (rows <= 0) return;
    // the three record blocks' first `rows` rows, at the capacity's stride
    KT_HIP(hipMemcpy2DAsync(rec_host, sizeof(double) * (size_t)m * P, trec, sizeof(double) * (size_t)m * P,
                            sizeof(double) * (size_t)rows * P, 3, hipMemcpyDeviceToHost, L.st));
    if (scale_hist)
        KT_HIP(hipMemcpyAsync(scale_hist->data(), hist_dev->ptr, sizeof(double) * (size_t)rows * P,
                              hipMemcpyDeviceToHost, L.st));
}

void lanczos_sweep(kt_matrix_s* A, const DevCSR& M, int P, int m, uint64_t seed, int64_t probe_base,
                   const double* x, int ldx, int ncols, const double* dnorms2, double* rec_host,
                   DevMat* basis, std::vector<double>* scale_hist, int lane, int bcols) {
    SweepList one;
    one.emplace_back(
        new ExplicitSweep(A, M, P, m, seed, probe_base, x, ldx, ncols, dnorms2, rec_host, basis, scale_hist, lane, bcols));
    run_sweeps(one);
}

// y-form sweep: one fused pass + one coefficient launch per Lanczos step
// (kt_kernels.hip, k_spmm_lanczos / k_ycoef).  rec_host (pinned, or the call
// waits for the copy) receives [alpha | up | low][m][P] followed by guard[P].
// The block seed (the quadrature-only columns of mc_trace's Lanczos Afun,
// kt_mctrace.cpp; kt_diag_fun's sweeps): x (n x ldx, ncols columns, in M's row
// order, squared norms in the device array dnorms2) is normalised into the
// gathered table v_0 (zero columns stay zero), the pass in start mode forms
// y_0 = A v_0 with (g, a, b) = (1, 0, 0), then the same passes as the
// sign-seeded sweep (steps 0 .. m-2).
YSweep::YSweep(kt_matrix_s* A_, const DevCSR& M_, int P_, int m_, uint64_t seed_, int64_t probe_base_,
               double* rec_host_, int lane_, bool int0_, const int* gate_, int ngate_)
    : A(A_), M(M_), P(P_), m(m_), n((int)A_->n), rec_host(rec_host_), L(A_, M_, P_, lane_), seed(seed_),
      probe_base(probe_base_), int0(int0_), gate(gate_), ngate(ngate_) {
    s0 = 1.0 / std::sqrt((double)n);  // v_0 = z / ||z||, ||z||^2 = n
    setup();
}

YSweep::YSweep(kt_matrix_s* A_, const DevCSR& M_, int P_, int m_, const double* x_, int ldx_, int ncols_,
               const double* dnorms2_, double* rec_host_, int lane_, double* basis_, int bcols_)
    : A(A_), M(M_), P(P_), m(m_), n((int)A_->n), rec_host(rec_host_), L(A_, M_, P_, lane_), x(x_), ldx(ldx_),
      ncols(ncols_), dnorms2(dnorms2_), basis(basis_), bcols(basis_ ? bcols_ : 0) {
    if (!x) fail(KT_ERR_ARG, "y-form block sweep: x is NULL");
    if (ncols < 1 || ncols > P) fail(KT_ERR_ARG, "y-form block sweep: 1 <= ncols <= P");
    setup();
}

void YSweep::setup() {
    if (!M.lower) fail(KT_ERR_ARG, "y-form sweep: the CSR copy has no lower-prefix array");
    if (gate && basis) fail(KT_ERR_ARG, "y-form sweep: the gated form keeps no basis");
    if (int0 && x) fail(KT_ERR_ARG, "y-form sweep: the int16 start needs the sign seed");
    SweepBufs& w = L.w;
    const size_t blk_bytes = L.blk_bytes;
    // X1: the packed sign table and, in the compact form, y_0's int16 table
    // behind it (not in y_0's own slot Y: the second step stores y_2 there
    // while other rows still read y_0, and the two layouts' rows do not
    // coincide).  2nP bytes after <= 4n ceil(P/32): inside the block but for tiny n.
    const size_t t0_off = (sizeof(uint32_t) * (size_t)n * ((P + 31) / 32) + 127) & ~(size_t)127;
    w.X0.ensure(blk_bytes);
    w.X1.ensure(int0 ? std::max(blk_bytes, t0_off + sizeof(int16_t) * (size_t)n * P) : blk_bytes);
    w.Y.ensure(blk_bytes);
    w.partial.ensure(sizeof(double) * (size_t)3 * P * L.grid1);  // slot-major [3P][grid1]
    w.coef.ensure(sizeof(double) * 9 * P);
    w.trec.ensure(sizeof(double) * ((size_t)3 * m * P + P));
    part = w.partial.as<double>();
    ys = w.coef.as<double>();
    trec = w.trec.as<double>();
    guard = trec + (size_t)3 * m * P;
    flags = A->ctx->ky_flags | (A->unit_values ? 2 : 0);
    if (blk_bytes >= ((size_t)1 << 31)) flags &= ~16;  // sc1 buffer stores take 32-bit offsets
    Z = w.X1.as<uint32_t>();
    if (int0) T0 = reinterpret_cast<int16_t*>(w.X1.as<char>() + t0_off);
    V0 = basis ? slot(0) : w.X1.as<double>();
    Xc = w.Y.as<double>();   // y_j (compact form: y_0 is T0, this slot is first used for y_2)
    Yo = nullptr;            // y_{j-1} (none at j = 0)
    Ot = w.X0.as<double>();  // y_{j+1}
}

void YSweep::start() {
    kt_context_s* ctx = A->ctx;
    hipStream_t st = L.st;
    const int grid1 = L.grid1;
    if (x) {
        // ys: [1/||x_c|| (P) | 0 (5P) | start pass (g, a, b) = (1, 0, 0) (3P)], from
        // the device norms (no host round trip)
        KT_HIP(launch_sweep_scales(dnorms2, ncols, P, 1, ys, nullptr, st));
        KT_HIP(hipMemsetAsync(V0, 0, L.blk_bytes, st));
        KT_HIP(launch_weighted_sum(n, 1, P, ncols, x, ldx, 0, ys, V0, P, st));
        prof_begin(ctx, PROF_YBLOCK, st, P);
        KT_HIP(launch_spmm_lanczos(P, flags, grid1, M.rowptr, M.col, M.val, n, V0, nullptr, Xc, ys + 6 * P, part,
                                   M.long_rows, M.n_long, A->long_thresh, L.lblocks, st));
        prof_end(ctx, PROF_YBLOCK, st);
    } else {
        // probes as a packed sign table (n x ceil(P/32) words), gathered by the
        // start pass instead of an 8nP-byte fp64 block
        KT_HIP(launch_rademacher_signs(P, n, seed, probe_base, M.perm, Z, st));
        prof_begin(ctx, PROF_START, st, P);
        if (int0) ctx->int0_sweeps += 1;
        KT_HIP(launch_spmm_lanczos_start(P, flags | (int0 ? 128 : 0), grid1, M.rowptr, M.col, M.val, n, Z, s0,
                                         int0 ? reinterpret_cast<double*>(T0) : Xc, part, M.long_rows, M.n_long,
                                         A->long_thresh, L.lblocks, st));
        prof_end(ctx, PROF_START, st);
    }
    KT_HIP(launch_ycoef(P, part, grid1, 1, !gate && m == 1, s0, ys, rec_at(0, 0), rec_at(1, 0), rec_at(2, 0), guard,
                        st));
}

void YSweep::step(int j) {
    kt_context_s* ctx = A->ctx;
    hipStream_t st = L.st;
    const int grid1 = L.grid1, lblocks = L.lblocks, pslot = x ? PROF_YBLOCK : PROF_SPMM;
    prof_begin(ctx, pslot, st, P);
    // y_{m} is never used: alpha_{m-1} needs only X'A X (the resumable form
    // has no last pass: every row it writes is complete)
    const bool last = !gate && j + 2 == m;
    if (gate) ctx->auto_passes += 1;
    const double *vc = slot(j), *vo = j > 0 ? slot(j - 1) : nullptr;  // the basis slots (none: nullptr)
    double* vn = slot(j + 1);
    if (int0 && j == 0) {  // m >= 3: never the last pass; also timed alone in its own slot
        prof_begin(ctx, PROF_FIRST, st, P);
        KT_HIP(launch_spmm_lanczos_first(P, flags, grid1, M.rowptr, M.col, n, T0, s0, Ot, ys + 6 * P, part,
                                         M.long_rows, M.n_long, A->long_thresh, lblocks, st, gate, ngate));
        prof_end(ctx, PROF_FIRST, st);
    } else if (last)
        KT_HIP(launch_spmm_quadform(P, flags, grid1, M.rowptr, M.col, M.val, M.lower, n, Xc, ys + 6 * P, part,
                                    M.long_rows, M.n_long, A->long_thresh, lblocks, st, vc, vo, vn, bcols));
    else if (int0 && j == 1)  // Yold = y_0 from the int16 table
        KT_HIP(launch_spmm_lanczos(P, flags | 128, grid1, M.rowptr, M.col, M.val, n, Xc,
                                   reinterpret_cast<const double*>(T0), Ot, ys + 6 * P, part, M.long_rows,
                                   M.n_long, A->long_thresh, lblocks, st, nullptr, nullptr, nullptr, 0, s0, gate,
                                   ngate));
    else
        KT_HIP(launch_spmm_lanczos(P, flags, grid1, M.rowptr, M.col, M.val, n, Xc, Yo, Ot, ys + 6 * P, part,
                                   M.long_rows, M.n_long, A->long_thresh, lblocks, st, vc, vo, vn, bcols, 0.0, gate,
                                   ngate));
    prof_end(ctx, pslot, st);
    KT_HIP(launch_ycoef(P, part, grid1, 0, last, 0.0, ys, rec_at(0, j + 1), rec_at(1, j + 1), rec_at(2, j + 1),
                        guard, st, gate, ngate));
    Yo = Xc;  // y_{j+1} overwrites y_{j-1} from the next pass on
    Xc = Ot;
    Ot = Yo;
}

void YSweep::finish() {
    KT_HIP(hipMemcpyAsync(rec_host, trec, sizeof(double) * ((size_t)3 * m * P + P), hipMemcpyDeviceToHost, L.st));
}

void YSweep::finish(int rows) {
    // the three record blocks' first `rows` rows, at the capacity's stride, and the guard
    if (rows > 0)
        KT_HIP(hipMemcpy2DAsync(rec_host, sizeof(double) * (size_t)m * P, trec, sizeof(double) * (size_t)m * P,
                                sizeof(double) * (size_t)rows * P, 3, hipMemcpyDeviceToHost, L.st));
    KT_HIP(hipMemcpyAsync(rec_host + (size_t)3 * m * P, guard, sizeof(double) * P, hipMemcpyDeviceToHost, L.st));
}

void lanczos_sweep_y_block(kt_matrix_s* A, const DevCSR& M, int P, int m, const double* x, int ldx, int ncols,
                           const double* dnorms2, double* rec_host, int lane) {
    SweepList one;
    one.emplace_back(new YSweep(A, M, P, m, x, ldx, ncols, dnorms2, rec_host, lane));
    run_sweeps(one);
}

bool guard_tripped(const double* R, int m, int P, int live, const double* n2) {
    const double* g = R + (size_t)3 * m * P;
    for (int c = 0; c < live; ++c)
        if ((!n2 || n2[c] > 0.0) && !(g[c] >= kYformGuard)) return true;
    return false;
}

int record_tridiag(const double* R, int mcap, int d, int P, int c, double* al, double* off) {
    int steps = d;
    for (int j = 0; j < d; ++j)
        if (R[(size_t)(2 * mcap + j) * P + c] < 1e-8) {
            steps = j + 1;
            break;
        }
    for (int j = 0; j < steps; ++j) al[j] = R[(size_t)(0 * mcap + j) * P + c];
    for (int j = 0; j + 1 < steps; ++j)
        off[j] = 0.5 * (R[(size_t)(2 * mcap + j) * P + c] + R[(size_t)(1 * mcap + j + 1) * P + c]);
    return steps;
}

void basis_weights(int steps, double nx, const double* fe1, const double* hist, int P, double* W, int ldw) {
    for (int j = 0; j < steps; ++j) W[(size_t)j * ldw] = hist ? nx * hist[(size_t)j * P] * fe1[j] : nx * fe1[j];
}

int slq_lanes_env(int dflt) {
    const char* e = getenv("KT_SLQ_LANES");
    return e ? atoi(e) : dflt;
}

bool slq_int0_env() {
    const char* e = getenv("KT_SLQ_INT0");
    return !(e && e[0] == '0');
}

void lanczos_columns(kt_matrix_s* A, const double* X, int ldx, int ncols, int m, int fun,
                     double* quad, double* Y, int ldy) {
    // every column by the explicit sweep (P = pow2 >= ncols, <= 16);
    // KT_LC_YBASIS=1 (tests): the f(A) x columns by basis-forming y-form sweeps
    const char* e = getenv("KT_LC_YBASIS");
    const int yb = (e && e[0] == '1' && Y) ? ncols : 0;
    lanczos_columns_split(A, X, ldx, ncols, Y ? ncols : 0, ncols, m, fun, quad, Y, ldy, 0, 16, yb);
}

// Widths of the y-form sweeps for `cols` quadrature-only columns: sweeps of
// 16, the remainder at the power of two that holds it.  At config 4 the final
// mc_trace round's 20 columns as 16 + 4: 43.2 ms per trace_exp vs 44.8 with
// the remainder zero-padded to 16 (profiles/r05/sweep_plan_ab/; with the
// lanes queued step by step -- the padded form measured faster while the
// second lane was queued only after the whole first sweep).  The explicit
// sweep does not take narrow chunks: 10 + 30 columns as greedy power-of-two
// sweeps (8 + 2, 16 + 8 + 4 + 2) cost 53 ms.
// A smaller `chunk` cuts the columns into sweeps of `chunk` (the last one
// shorter), each at the power of two that holds it: {(columns, width)}.
// KT_LC_YMINP (A/B): the narrowest y-form sweep width (a remainder of 4
// columns padded to 8 or 16 instead of a 4-wide sweep).
static std::vector<std::pair<int, int>> quad_plan(int cols, int chunk = 16) {
    std::vector<std::pair<int, int>> wv;
    chunk = std::max(1, std::min(chunk, 16));
    const char* e = getenv("KT_LC_YMINP");
    const int pmin = e ? std::max(1, std::min(16, atoi(e))) : 1;
    for (int left = cols; left > 0; left -= chunk) {
        const int c = std::min(left, chunk);
        int P = 1;
        while (P < c || P < pmin) P <<= 1;
        wv.push_back({c, P});
    }
    return wv;
}

void lanczos_columns_split(kt_matrix_s* A, const double* X, int ldx, int ncols, int ny, int ne, int m, int fun,
                           double* quad, double* Y, int ldy, int px, int ychunk, int yb) {
    kt_context_s* ctx = A->ctx;
    const int64_t n = A->n;
    if (!Y) ny = 0;
    if (ny < 0 || ny > ne || ne > ncols) fail(KT_ERR_ARG, "lanczos_columns_split: 0 <= ny <= ne <= ncols");
    yb = std::max(0, std::min(yb, ny));
    // squared column norms on the device (the sweeps' start scales are formed
    // from them there); the host reads them with the sweep records
    ctx->ws.colnorm.ensure(sizeof(double) * ncols);
    double* dn2 = ctx->ws.colnorm.as<double>();
    KT_HIP(launch_gram_diag(gram_device(ctx, n, X, ldx, ncols, X, ldx, ncols), ncols, ncols, dn2, ctx->stream));
    // The sweeps run on the hubs-first CSR (equal-length neighbouring rows,
    // adjacent hub segments: the explicit K1 at P = 16 on the bench graph 264
    // -> ~210 us): the block is permuted into that row order on the way in
    // and f(A) x back out; quadratic forms are permutation invariant.
    const DevCSR& M = hub_csr(A);
    const int* perm = M.perm;
    DevMat Xh, Yh;
    const double* Xs = X;
    int ldxs = ldx;
    double* Ys = Y;
    int ldys = ldy;
    if (perm) {
        Xh.alloc(ctx, n, ncols, false);
        KT_HIP(launch_perm_rows((int)n, ncols, perm, 1, X, ldx, Xh.col(0), ncols, ctx->stream));
        Xs = Xh.col(0);
        ldxs = ncols;
        if (ny) {
            Yh.alloc(ctx, n, ny, false);
            Ys = Yh.col(0);
            ldys = ny;
        }
    }
    // Sweeps: columns [0, ne) by the explicit CGS2 sweep (P = px, or pow2 >=
    // ne capped at 16), the basis kept for the ny f(A)x columns among them;
    // columns [ne, ncols) -- quadratic forms only -- by y-form sweeps (no K2,
    // no basis; widths quad_plan).  All queued before the host waits, dealt
    // over the four lanes, so the device runs them side by side.
    struct Sw {
        int c0, nc, P, lane;
        bool yform;
        bool ybasis;  // a y-form sweep that also forms its Lanczos basis (KF_VB)
    };
    std::vector<Sw> sw;
    const char* ye = getenv("KT_LC_YFORM");  // 0: every column by the explicit sweep
    if (ye && ye[0] == '0') {
        ne = ncols;
        yb = 0;
    }
    int Pe = 1;
    while (Pe < ne - yb && Pe < 16) Pe <<= 1;
    if (px > 0) Pe = px;
    if (Pe > 32 || (Pe & (Pe - 1))) fail(KT_ERR_ARG, "lanczos_columns_split: sweep width must be a power of two <= 32");
    // sweeps dealt over the four lanes in order (basis-forming y-form, then
    // explicit, then forms-only y-form), so up to four run side by side; a
    // lane's later sweeps follow its earlier ones
    int k = 0;
    for (int c0 = 0; c0 < yb; c0 += 16) {
        const int c = std::min(16, yb - c0);
        int P = 1;
        while (P < c) P <<= 1;
        sw.push_back({c0, c, P, k++ % 4, true, true});
    }
    for (int c0 = yb; c0 < ne; c0 += Pe) sw.push_back({c0, std::min(Pe, ne - c0), Pe, k++ % 4, false, false});
    {
        int c0 = ne;
        for (const auto& cp : quad_plan(ncols - ne, ychunk)) {
            sw.push_back({c0, cp.first, cp.second, k++ % 4, true, false});
            c0 += cp.first;
        }
    }
    const size_t rec_max = (size_t)3 * m * 32 + 32;
    PinnedBuf& hr = ctx->ws.pin_colrec;
    hr.ensure(sizeof(double) * (rec_max * sw.size() + ncols));
    double* hn2 = hr.as<double>() + rec_max * sw.size();  // the norms, read after the sweeps
    KT_HIP(hipMemcpyAsync(hn2, dn2, sizeof(double) * ncols, hipMemcpyDeviceToHost, ctx->stream));
    // the aux lanes read the permuted block written on ctx->stream
    hipEvent_t ready = ctx->ws.colsplit_ev;
    if (!ready) {
        KT_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
        ctx->ws.colsplit_ev = ready;
    }
    KT_HIP(hipEventRecord(ready, ctx->stream));
    bool used[4] = {true, false, false, false};
    for (size_t i = 0; i < sw.size(); ++i) {
        const Sw& q = sw[i];
        if (used[q.lane]) continue;
        KT_HIP(hipStreamWaitEvent(lane_stream(ctx, q.lane), ready, 0));
        used[q.lane] = true;
    }
    // the explicit sweeps keep their bases (slot j: n x nyc); the basis-forming
    // y-form sweeps theirs as m slots of n x P (normalised vectors: no scale
    // history)
    std::vector<DevMat> bases(sw.size());
    std::vector<std::vector<double>> hists(sw.size());
    for (size_t i = 0; i < sw.size(); ++i) {
        const Sw& q = sw[i];
        if (q.ybasis) {
            bases[i].alloc(ctx, (int64_t)m * n, q.P, false);  // slot j = rows [j n, (j + 1) n)
            continue;
        }
        if (q.yform) continue;
        const int nyc = std::max(0, std::min(q.nc, ny - q.c0));
        if (nyc) bases[i].alloc(ctx, n, m * nyc, false);  // every slot is written by the sweep
    }
    // Queue the sweeps launch by launch across lanes (one sweep per lane at a
    // time: a lane's sweeps share its buffers), so every lane starts at once
    std::vector<int> next(4, 0);  // per lane: index into its sweeps
    std::vector<std::vector<int>> by_lane(4);
    for (size_t i = 0; i < sw.size(); ++i) by_lane[sw[i].lane].push_back((int)i);
    for (;;) {
        SweepList grp, ex;  // the y-form sweeps, then the explicit ones
        for (int l = 0; l < 4; ++l) {
            if (next[l] >= (int)by_lane[l].size()) continue;
            const int i = by_lane[l][next[l]++];
            const Sw& q = sw[i];
            double* R = hr.as<double>() + rec_max * i;
            if (q.yform) {
                grp.emplace_back(new YSweep(A, M, q.P, m, Xs + q.c0, ldxs, q.nc, dn2 + q.c0, R, q.lane,
                                            q.ybasis ? bases[i].col(0) : nullptr, q.nc));
            } else {
                const int nyc = std::max(0, std::min(q.nc, ny - q.c0));
                ex.emplace_back(new ExplicitSweep(A, M, q.P, m, 0, 0, Xs + q.c0, ldxs, q.nc, dn2 + q.c0, R,
                                                  nyc ? &bases[i] : nullptr, nyc ? &hists[i] : nullptr, q.lane,
                                                  nyc));
            }
        }
        for (auto& e : ex) grp.push_back(std::move(e));
        if (grp.empty()) break;
        run_sweeps(grp);
    }
    KT_HIP(hipStreamSynchronize(ctx->stream));
    for (int l = 1; l < 4; ++l)
        if (used[l]) KT_HIP(hipStreamSynchronize(ctx->aux_stream[l - 1]));
    const std::vector<double> norms2(hn2, hn2 + ncols);
    // a y-form column that tripped the cancellation guard (or broke down) is
    // redone by the explicit CGS2 sweep at the same width; only the tripped
    // columns take the redo's records, so a column's form never depends on
    // which columns share its sweep (mc_trace's world-size bit identity)
    // A basis-forming sweep with a tripped column is redone WHOLE by the
    // explicit sweep with its basis (its columns are f(A) x inputs, not
    // sharded forms): the sweep then takes the explicit path's records,
    // basis and scale history.
    std::vector<double> redo;
    std::vector<char> ex_basis(sw.size(), 0);  // the sweep's basis is the explicit layout
    for (size_t i = 0; i < sw.size(); ++i) ex_basis[i] = !sw[i].yform;
    for (size_t i = 0; i < sw.size(); ++i) {
        const Sw& q = sw[i];
        if (!q.yform) continue;
        double* R = hr.as<double>() + rec_max * i;
        const double* n2 = norms2.data() + q.c0;
        if (!guard_tripped(R, m, q.P, q.nc, n2)) continue;
        if (q.ybasis) {
            const int nyc = std::max(0, std::min(q.nc, ny - q.c0));
            DevMat eb;
            if (nyc) eb.alloc(ctx, n, m * nyc, false);
            lanczos_sweep(A, M, q.P, m, 0, 0, Xs + q.c0, ldxs, q.nc, dn2 + q.c0, R, nyc ? &eb : nullptr,
                          nyc ? &hists[i] : nullptr, 0, nyc);
            KT_HIP(hipStreamSynchronize(ctx->stream));
            bases[i] = std::move(eb);
            ex_basis[i] = 1;
            ctx->yform_redone += 1;
            continue;
        }
        redo.assign((size_t)3 * m * q.P, 0.0);
        lanczos_sweep(A, M, q.P, m, 0, 0, Xs + q.c0, ldxs, q.nc, dn2 + q.c0, redo.data(), nullptr, nullptr, 0);
        KT_HIP(hipStreamSynchronize(ctx->stream));
        for (int c = 0; c < q.nc; ++c) {
            if (!guard_tripped(R + c, m, q.P, 1, n2 + c)) continue;  // column c alone
            for (int row = 0; row < 3 * m; ++row) R[(size_t)row * q.P + c] = redo[(size_t)row * q.P + c];
        }
        ctx->yform_redone += 1;
    }
    // per column (one QL pass each, on the host pool): the quadrature and,
    // for the f(A) x columns, f(T) e1 -> the basis weights
    std::vector<int> nycs(sw.size()), col_sw, col_c;
    std::vector<std::vector<double>> Ws(sw.size());  // Y = sum_j u_j w_j, [j * nyc + c]
    for (size_t i = 0; i < sw.size(); ++i) {
        const Sw& q = sw[i];
        nycs[i] = (q.yform && !q.ybasis) ? 0 : std::max(0, std::min(q.nc, ny - q.c0));
        Ws[i].assign((size_t)m * std::max(nycs[i], 1), 0.0);
        for (int c = 0; c < q.nc; ++c) {
            col_sw.push_back((int)i);
            col_c.push_back(c);
        }
    }
    HostPool::get().run((int)col_sw.size(), [&](int t) {
        const int i = col_sw[t], c = col_c[t], nyc = nycs[i];
        const Sw& q = sw[i];
        const double* R = hr.as<double>() + rec_max * i;
        std::vector<double> al(m), off(m), fe1(m);
        const int steps = record_tridiag(R, m, m, q.P, c, al.data(), off.data());
        if (norms2[q.c0 + c] == 0.0) {
            if (quad) quad[q.c0 + c] = 0.0;
            return;
        }
        if (c >= nyc) {
            if (quad) quad[q.c0 + c] = norms2[q.c0 + c] * tridiag_quadrature(steps, al.data(), off.data(), fun);
            return;
        }
        const double qd = tridiag_fun_e1(steps, al.data(), off.data(), fun, fe1.data());
        if (quad) quad[q.c0 + c] = norms2[q.c0 + c] * qd;
        basis_weights(steps, std::sqrt(norms2[q.c0 + c]), fe1.data(), ex_basis[i] ? hists[i].data() + c : nullptr, q.P,
                      Ws[i].data() + c, nyc);
    }, 4);
    for (size_t i = 0; i < sw.size(); ++i) {
        const Sw& q = sw[i];
        const int nyc = nycs[i];
        const std::vector<double>& W = Ws[i];
        if (nyc) {
            DevBuf& dw = ctx->ws.small2;
            dw.ensure(sizeof(double) * W.size());
            KT_HIP(hipMemcpyAsync(dw.ptr, W.data(), sizeof(double) * W.size(), hipMemcpyHostToDevice, ctx->stream));
            // explicit basis: slot j = n x nyc; y-form basis: slot j = n x P
            const int ldu = ex_basis[i] ? nyc : q.P;
            KT_HIP(launch_weighted_sum((int)n, m, nyc, nyc, bases[i].col(0), ldu, (int64_t)n * ldu, dw.as<double>(),
                                       Ys + q.c0, ldys, ctx->stream));
            KT_HIP(hipStreamSynchronize(ctx->stream));
        }
    }
    if (perm && ny) KT_HIP(launch_perm_rows((int)n, ny, perm, 0, Ys, ldys, Y, ldy, ctx->stream));
}

// The adaptive depth.  Sweeps are always kAdaptP wide, so a
// column's recurrence does not depend on how many columns the call has; its
// depth is decided on the device from its own record and its values formed
// from that record truncated there.  The check of depth j + 1 is queued
// behind step j; every kAdaptPoll steps the sweep's count of running columns
// is copied to a pinned word behind an event, and the host reads the copy of
// the poll before (so kAdaptPoll steps stay queued) and stops queueing the
// sweep once it reads 0.  Steps queued past a column's depth are harmless.
// The f(A) x columns' basis grows in chunks of kAdaptSlots slots.
constexpr int kAdaptP = 16, kAdaptPoll = 4, kAdaptSlots = 32;

int lanczos_columns_adaptive(kt_matrix_s* A, const double* X, int ldx, int ncols, int ny, int m_max, double rtol,
                             int fun, double* quad, double* Y, int ldy, int* depth) {
    kt_context_s* ctx = A->ctx;
    const int64_t n = A->n;
    if (!Y) ny = 0;
    if (ncols < 1 || ny < 0 || ny > ncols) fail(KT_ERR_ARG, "lanczos_columns_adaptive: 0 <= ny <= ncols, ncols >= 1");
    if (m_max <= 0) m_max = kAdaptDefaultCap;
    if (m_max > kAdaptMaxCap) fail(KT_ERR_ARG, "the Lanczos depth cap must be at most 256");
    if (!(rtol > 0.0)) rtol = kAdaptRtol;
    const int m = m_max, P = kAdaptP;
    ctx->ws.colnorm.ensure(sizeof(double) * ncols);
    double* dn2 = ctx->ws.colnorm.as<double>();
    KT_HIP(launch_gram_diag(gram_device(ctx, n, X, ldx, ncols, X, ldx, ncols), ncols, ncols, dn2, ctx->stream));
    // the hubs-first CSR, the block permuted in and f(A) x back out, as
    // lanczos_columns_split does
    const DevCSR& M = hub_csr(A);
    const int* perm = M.perm;
    DevMat Xh, Yh;
    const double* Xs = X;
    int ldxs = ldx;
    double* Ys = Y;
    int ldys = ldy;
    if (perm) {
        Xh.alloc(ctx, n, ncols, false);
        KT_HIP(launch_perm_rows((int)n, ncols, perm, 1, X, ldx, Xh.col(0), ncols, ctx->stream));
        Xs = Xh.col(0);
        ldxs = ncols;
        if (ny) {
            Yh.alloc(ctx, n, ny, false);
            Ys = Yh.col(0);
            ldys = ny;
        }
    }
    const int nsw = (ncols + P - 1) / P;
    const size_t rec = (size_t)3 * m * P, stw = (size_t)P * kAdaptState;
    // pinned: per sweep its record and state block, then the norms
    PinnedBuf& hr = ctx->ws.pin_colrec;
    hr.ensure(sizeof(double) * ((rec + stw) * nsw + ncols));
    double* hn2 = hr.as<double>() + (rec + stw) * nsw;
    KT_HIP(hipMemcpyAsync(hn2, dn2, sizeof(double) * ncols, hipMemcpyDeviceToHost, ctx->stream));
    PinnedBuf& pw = ctx->ws.pin_adapt;  // the polled words: [lane][2]
    pw.ensure(sizeof(int) * 8);
    volatile int* polled = pw.as<int>();
    hipEvent_t ready = ctx->ws.colsplit_ev;
    if (!ready) {
        KT_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
        ctx->ws.colsplit_ev = ready;
    }
    KT_HIP(hipEventRecord(ready, ctx->stream));
    const int lanes = std::min(4, nsw);
    for (int l = 0; l < lanes; ++l) {
        if (l) {
            hipStream_t& as = ctx->aux_stream[l - 1];
            if (!as) KT_HIP(hipStreamCreateWithFlags(&as, hipStreamNonBlocking));
            KT_HIP(hipStreamWaitEvent(as, ready, 0));
        }
        for (auto& e : ctx->ws.adapt_ev[l])
            if (!e) KT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->ws.adapt_state[l].ensure(sizeof(double) * (stw + 1));
    }
    std::vector<std::vector<DevMat>> bases(nsw);  // per sweep: the basis chunks of its f(A) x columns
    std::vector<std::vector<double>> hists(nsw);
    std::vector<int> rows(nsw, 0);                // record rows written per sweep
    // one sweep per lane at a time, the lanes' sweeps queued step by step
    for (int s0 = 0; s0 < nsw; s0 += lanes) {
        const int g = std::min(lanes, nsw - s0);
        std::vector<std::unique_ptr<ExplicitSweep>> ex;
        std::vector<char> done(g, 0);
        for (int l = 0; l < g; ++l) {
            const int i = s0 + l, c0 = i * P, nc = std::min(P, ncols - c0);
            const int nyc = std::max(0, std::min(nc, ny - c0));
            double* R = hr.as<double>() + (rec + stw) * i;
            ex.emplace_back(new ExplicitSweep(A, M, P, m, 0, 0, Xs + c0, ldxs, nc, dn2 + c0, R, nullptr,
                                              nyc ? &hists[i] : nullptr, l, nyc));
            if (nyc) ex.back()->use_basis_chunks(&bases[i], kAdaptSlots);
            KT_HIP(hipMemsetAsync(ctx->ws.adapt_state[l].ptr, 0, sizeof(double) * (stw + 1), ex.back()->stream()));
            polled[2 * l] = polled[2 * l + 1] = 1;
        }
        for (auto& e : ex) e->start();
        int npoll = 0;
        for (int j = 0; j < m; ++j) {
            bool any = false;
            for (int l = 0; l < g; ++l) {
                if (done[l]) continue;
                any = true;
                const int i = s0 + l, c0 = i * P, nc = std::min(P, ncols - c0);
                const int nyc = std::max(0, std::min(nc, ny - c0));
                ExplicitSweep& e = *ex[l];
                e.step(j);
                rows[i] = j + 1;
                double* dst = ctx->ws.adapt_state[l].as<double>();
                int* dact = reinterpret_cast<int*>(dst + stw);
                // checks from two depths before the first decision (its two agreements)
                if (j + 1 >= kAdaptMinDepth - 2)
                    KT_HIP(launch_quad_check(e.device_record(), m, P, j + 1, nc, nyc, dn2 + c0, fun, rtol, dst, dact,
                                             e.stream()));
                if (j + 1 >= kAdaptMinDepth && (j + 1) % kAdaptPoll == 0) {
                    int* word = const_cast<int*>(polled) + 2 * l + (npoll & 1);
                    KT_HIP(hipMemcpyAsync(word, dact, sizeof(int), hipMemcpyDeviceToHost, e.stream()));
                    KT_HIP(hipEventRecord(ctx->ws.adapt_ev[l][npoll & 1], e.stream()));
                }
            }
            if (!any) break;
            if (j + 1 >= kAdaptMinDepth && (j + 1) % kAdaptPoll == 0) {
                // the poll before this one: its event has kAdaptPoll steps queued behind it
                if (npoll > 0)
                    for (int l = 0; l < g; ++l) {
                        if (done[l]) continue;
                        KT_HIP(hipEventSynchronize(ctx->ws.adapt_ev[l][(npoll - 1) & 1]));
                        if (polled[2 * l + ((npoll - 1) & 1)] == 0) done[l] = 1;
                    }
                ++npoll;
            }
        }
        for (int l = 0; l < g; ++l) {
            const int i = s0 + l;
            ex[l]->finish(rows[i]);
            KT_HIP(hipMemcpyAsync(hr.as<double>() + (rec + stw) * i + rec, ctx->ws.adapt_state[l].ptr,
                                  sizeof(double) * stw, hipMemcpyDeviceToHost, ex[l]->stream()));
        }
        // the lanes' buffers and state blocks are reused by the next group
        KT_HIP(hipStreamSynchronize(ctx->stream));
        for (int l = 1; l < g; ++l) KT_HIP(hipStreamSynchronize(ctx->aux_stream[l - 1]));
    }
    KT_HIP(hipStreamSynchronize(ctx->stream));
    const std::vector<double> norms2(hn2, hn2 + ncols);
    // per column on the host pool, at its own depth: the quadrature and, for
    // the f(A) x columns, f(T) e1 -> the basis weights
    std::vector<int> dep(ncols, 0);
    std::vector<char> cap(ncols, 0);
    std::vector<std::vector<double>> Ws(nsw);
    std::vector<int> nycs(nsw, 0);
    for (int i = 0; i < nsw; ++i) {
        const int c0 = i * P, nc = std::min(P, ncols - c0);
        nycs[i] = std::max(0, std::min(nc, ny - c0));
        Ws[i].assign((size_t)m * std::max(nycs[i], 1), 0.0);
    }
    HostPool::get().run(ncols, [&](int t) {
        const int i = t / P, c = t % P, nyc = nycs[i];
        const double* R = hr.as<double>() + (rec + stw) * i;
        const double* st = R + rec + (size_t)c * kAdaptState;
        if (norms2[t] == 0.0) {
            if (quad) quad[t] = 0.0;
            return;
        }
        // a column the device did not stop ran every row the sweep wrote
        const bool stopped = st[4] != 0.0;
        const int d = stopped ? (int)st[3] : rows[i];
        std::vector<double> al(d), off(d), fe1(d);
        const int steps = record_tridiag(R, m, d, P, c, al.data(), off.data());
        // unconverged at the cap, unless the record's last row is a lucky breakdown
        cap[t] = !stopped && !(R[(size_t)(2 * m + steps - 1) * P + c] < 1e-8);
        dep[t] = steps;
        if (c >= nyc) {
            if (quad) quad[t] = norms2[t] * tridiag_quadrature(steps, al.data(), off.data(), fun);
            return;
        }
        const double qd = tridiag_fun_e1(steps, al.data(), off.data(), fun, fe1.data());
        if (quad) quad[t] = norms2[t] * qd;
        basis_weights(steps, std::sqrt(norms2[t]), fe1.data(), hists[i].data() + c, P, Ws[i].data() + c, nyc);
    }, 4);
    for (int i = 0; i < nsw; ++i) {
        const int nyc = nycs[i], c0 = i * P;
        if (!nyc) continue;
        int mt = 1;
        for (int c = 0; c < nyc; ++c) mt = std::max(mt, dep[c0 + c]);
        SlotTab tab{};
        for (size_t k = 0; k < bases[i].size() && k < (size_t)kSlotTabChunks; ++k) tab.chunk[k] = bases[i][k].col(0);
        DevBuf& dw = ctx->ws.small2;
        dw.ensure(sizeof(double) * Ws[i].size());
        KT_HIP(hipMemcpyAsync(dw.ptr, Ws[i].data(), sizeof(double) * (size_t)mt * nyc, hipMemcpyHostToDevice,
                              ctx->stream));
        KT_HIP(launch_weighted_sum_tab((int)n, mt, nyc, tab, kAdaptSlots, dw.as<double>(), Ys + c0, ldys, ctx->stream));
        KT_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (perm && ny) KT_HIP(launch_perm_rows((int)n, ny, perm, 0, Ys, ldys, Y, ldy, ctx->stream));
    int ncap = 0, dmax = 0;
    for (int t = 0; t < ncols; ++t) {
        ncap += cap[t];
        dmax = std::max(dmax, dep[t]);
        if (depth) depth[t] = dep[t];
    }
    ctx->adapt_max_depth = std::max<int64_t>(ctx->adapt_max_depth, dmax);
    ctx->adapt_capped += ncap;
    return ncap;
}

// The node-removal columns: lanczos_columns_adaptive's
// driver -- sweeps kAdaptP wide, one per lane at a time, the check of depth
// j + 1 queued behind step j, the count of running columns polled every
// kAdaptPoll steps one poll behind -- for sweeps that start at unit vectors
// (k_unit_start, rows through the hub copy's permutation) and stop by
// k_node_check's lag-2 rule from depth 1 on.  The explicit CGS2 sweep: a hub's
// unit vector sits close to the dominant eigenvector, where the y-form's
// cancellation guard would trip.  The device decides depths; Xm comes from the
// host QL on the record cut at the column's depth, so a candidate's values
// depend on (A, node, tol, it, fun) alone.
//
// node_sweeps is that driver with the check as a parameter, shared with the
// bracket columns (§4.2i) and the pair columns (§4.2j): start(sweep, pos) picks
// the sweep's start block from its columns' rows (device, one per column);
// check(record, m, P, j, nc, state, active, stream)
// queues the stopping test of depth j on a lane; cut(t, d, alpha, off, beta_d)
// forms column t's values from its record cut at its depth d (alpha: d, off:
// d - 1 entries, beta_d the record's next off-diagonal), on the host pool.
namespace {

template <class Start, class Check, class Cut>
void node_sweeps(kt_matrix_s* A, int64_t ncand, const int64_t* nodes, int it, Start start, Check check, Cut cut) {
    kt_context_s* ctx = A->ctx;
    const int64_t n = A->n;
    if (ncand < 1) return;
    if (it < 1 || it > kAdaptMaxCap) fail(KT_ERR_ARG, "the Lanczos depth cap must be in [1, 256]");
    if (ncand > INT32_MAX - kAdaptP || n > INT32_MAX) fail(KT_ERR_ARG, "n and the candidate count must fit 32 bits");
    const int m = it, P = kAdaptP, ncols = (int)ncand;
    const DevCSR& M = hub_csr(A);
    const bool relabelled = M.perm != nullptr;
    std::vector<int> hpos((size_t)ncols);
    for (int c = 0; c < ncols; ++c) {
        if (nodes[c] < 0 || nodes[c] >= n) fail(KT_ERR_ARG, "node index out of range");
        hpos[c] = relabelled ? A->old2new[nodes[c]] : (int)nodes[c];
    }
    DevBuf& dposb = ctx->ws.node_pos;
    dposb.ensure(sizeof(int) * (size_t)ncols);
    const int* dpos = dposb.as<int>();
    KT_HIP(hipMemcpyAsync(dposb.ptr, hpos.data(), sizeof(int) * (size_t)ncols, hipMemcpyHostToDevice, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));  // the lanes read it; hpos may go
    const int nsw = (ncols + P - 1) / P;
    const size_t rec = (size_t)3 * m * P, stw = (size_t)P * kAdaptState;
    PinnedBuf& hr = ctx->ws.pin_colrec;  // per sweep its record and state block
    hr.ensure(sizeof(double) * (rec + stw) * nsw);
    PinnedBuf& pw = ctx->ws.pin_adapt;  // the polled words: [lane][2]
    pw.ensure(sizeof(int) * 8);
    volatile int* polled = pw.as<int>();
    const int lanes = std::min(4, nsw);
    for (int l = 0; l < lanes; ++l) {
        (void)lane_stream(ctx, l);
        for (auto& e : ctx->ws.adapt_ev[l])
            if (!e) KT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->ws.adapt_state[l].ensure(sizeof(double) * (stw + 1));
    }
    std::vector<int> rows(nsw, 0);  // record rows written per sweep
    int64_t steps_queued = 0;
    for (int s0 = 0; s0 < nsw; s0 += lanes) {
        const int g = std::min(lanes, nsw - s0);
        std::vector<std::unique_ptr<ExplicitSweep>> ex;
        std::vector<char> done(g, 0);
        for (int l = 0; l < g; ++l) {
            const int i = s0 + l, c0 = i * P, nc = std::min(P, ncols - c0);
            double* R = hr.as<double>() + (rec + stw) * i;
            ex.emplace_back(new ExplicitSweep(A, M, P, m, 0, 0, nullptr, 0, nc, nullptr, R, nullptr, nullptr, l, 0));
            start(*ex.back(), dpos + c0);
            KT_HIP(hipMemsetAsync(ctx->ws.adapt_state[l].ptr, 0, sizeof(double) * (stw + 1), ex.back()->stream()));
            polled[2 * l] = polled[2 * l + 1] = 1;
        }
        for (auto& e : ex) {
            prof_begin(ctx, PROF_NODES, e->stream(), P);
            e->start();
            prof_end(ctx, PROF_NODES, e->stream());
        }
        int npoll = 0;
        for (int j = 0; j < m; ++j) {
            bool any = false;
            for (int l = 0; l < g; ++l) {
                if (done[l]) continue;
                any = true;
                const int i = s0 + l, c0 = i * P, nc = std::min(P, ncols - c0);
                ExplicitSweep& e = *ex[l];
                e.step(j);
                ++steps_queued;
                rows[i] = j + 1;
                double* dst = ctx->ws.adapt_state[l].as<double>();
                int* dact = reinterpret_cast<int*>(dst + stw);
                prof_begin(ctx, PROF_NODES, e.stream(), P);
                KT_HIP(check(e.device_record(), m, P, j + 1, nc, dst, dact, e.stream()));
                prof_end(ctx, PROF_NODES, e.stream());
                if ((j + 1) % kAdaptPoll == 0) {
                    int* word = const_cast<int*>(polled) + 2 * l + (npoll & 1);
                    KT_HIP(hipMemcpyAsync(word, dact, sizeof(int), hipMemcpyDeviceToHost, e.stream()));
                    KT_HIP(hipEventRecord(ctx->ws.adapt_ev[l][npoll & 1], e.stream()));
                }
            }
            if (!any) break;
            if ((j + 1) % kAdaptPoll == 0) {
                // the poll before this one: its event has kAdaptPoll steps queued behind it
                if (npoll > 0)
                    for (int l = 0; l < g; ++l) {
                        if (done[l]) continue;
                        KT_HIP(hipEventSynchronize(ctx->ws.adapt_ev[l][(npoll - 1) & 1]));
                        if (polled[2 * l + ((npoll - 1) & 1)] == 0) done[l] = 1;
                    }
                ++npoll;
            }
        }
        for (int l = 0; l < g; ++l) {
            const int i = s0 + l;
            ex[l]->finish(rows[i]);
            KT_HIP(hipMemcpyAsync(hr.as<double>() + (rec + stw) * i + rec, ctx->ws.adapt_state[l].ptr,
                                  sizeof(double) * stw, hipMemcpyDeviceToHost, ex[l]->stream()));
        }
        // the lanes' buffers and state blocks are reused by the next group
        KT_HIP(hipStreamSynchronize(ctx->stream));
        for (int l = 1; l < g; ++l) KT_HIP(hipStreamSynchronize(ctx->aux_stream[l - 1]));
    }
    std::vector<int> dep(ncols, 0);
    HostPool::get().run(ncols, [&](int t) {
        const int i = t / P, c = t % P;
        const double* R = hr.as<double>() + (rec + stw) * i;
        const double* st = R + rec + (size_t)c * kAdaptState;
        // a column the device did not stop ran every row the sweep wrote: iter = it
        const int d = std::max(1, std::min(st[4] != 0.0 ? (int)st[3] : rows[i], rows[i]));
        std::vector<double> al(d), off(d);
        for (int k = 0; k < d; ++k) al[k] = R[(size_t)k * P + c];
        for (int k = 0; k + 1 < d; ++k)
            off[k] = 0.5 * (R[(size_t)(2 * m + k) * P + c] + R[(size_t)(1 * m + k + 1) * P + c]);
        cut(t, d, al.data(), off.data(), R[(size_t)(2 * m + d - 1) * P + c]);
        dep[t] = d;
    }, 4);
    ctx->nodes_sweeps = nsw;
    ctx->nodes_steps = steps_queued;
    ctx->nodes_max_depth = *std::max_element(dep.begin(), dep.end());
}

}  // namespace

void lanczos_nodes_adaptive(kt_matrix_s* A, int64_t ncand, const int64_t* nodes, double tol, int it, int fun,
                            double* Xm, int* iter, int* lucky) {
    node_sweeps(
        A, ncand, nodes, it, [](ExplicitSweep& e, const int* pos) { e.use_unit_start(pos); },
        [=](const double* trec, int m, int P, int j, int nc, double* state, int* active, hipStream_t st) {
            return launch_node_check(trec, m, P, j, nc, fun, tol, state, active, st);
        },
        [=](int t, int d, const double* al, const double* off, double beta_d) {
            Xm[t] = node_update_value(d, al, off, fun);
            if (iter) iter[t] = d;
            if (lucky) lucky[t] = beta_d < 1e-8 ? 1 : 0;
        });
}

// The bracket columns: node_sweeps with k_bracket_check.  The
// device decides depths; lo / hi come from the host rule (gauss_radau_sums) on
// the record cut at the column's depth, times exp(mu), and the flag from those
// values, so a column's results depend on (A, node, mu, rtol, it) alone.
void lanczos_nodes_bracket(kt_matrix_s* A, int64_t ncand, const int64_t* nodes, double mu, double rtol, int it,
                           double* lo, double* hi, int* iter, int* flag) {
    const double scale = std::exp(mu);
    node_sweeps(
        A, ncand, nodes, it, [](ExplicitSweep& e, const int* pos) { e.use_unit_start(pos); },
        [=](const double* trec, int m, int P, int j, int nc, double* state, int* active, hipStream_t st) {
            return launch_bracket_check(trec, m, P, j, nc, mu, rtol, state, active, st);
        },
        [=](int t, int d, const double* al, const double* off, double beta_d) {
            double l = 0.0, h = 0.0;
            int f = gauss_radau_sums(d, al, off, beta_d, mu, &l, &h);
            // the gap is judged on the values returned: a column the device stopped
            // on a gap the host sums miss by rounding reports 3 below the cap
            if (f == 0 && !(h - l <= rtol * l)) f = 3;
            lo[t] = l * scale;
            hi[t] = h * scale;
            if (iter) iter[t] = d;
            if (flag) flag[t] = f;
        });
}

// The pair columns: node_sweeps over 2 npairs columns, pair
// p's rows (i, j) at 2p and 2p + 1, with k_pair_start and k_pair_bracket_check.
// The device decides depths; each column's sums come from the host rule on its
// record cut at its own depth, and lo / hi / flag from pair_bracket_combine on
// those times exp(mu), so a pair's results depend on (A, i, j, mu, rtol, ftol,
// it) alone.
void lanczos_pairs_bracket(kt_matrix_s* A, int64_t npairs, const int64_t* ei, const int64_t* ej, double mu,
                           double rtol, double ftol, int it, double* lo, double* hi, int* iter, int* flag,
                           int* col_iter) {
    if (npairs < 1) return;
    if (npairs > (INT32_MAX - kAdaptP) / 2) fail(KT_ERR_ARG, "the pair count must fit 32 bits");
    const double scale = std::exp(mu);
    std::vector<int64_t> rows((size_t)2 * npairs);
    for (int64_t p = 0; p < npairs; ++p) {
        rows[2 * p] = ei[p];
        rows[2 * p + 1] = ej[p];
    }
    std::vector<double> L(rows.size()), U(rows.size());
    std::vector<int> kind(rows.size()), dep(rows.size());
    node_sweeps(
        A, 2 * npairs, rows.data(), it, [](ExplicitSweep& e, const int* pos) { e.use_pair_start(pos); },
        [=](const double* trec, int m, int P, int j, int nc, double* state, int* active, hipStream_t st) {
            return launch_pair_bracket_check(trec, m, P, j, nc, mu, rtol, ftol, state, active, st);
        },
        [&](int t, int d, const double* al, const double* off, double beta_d) {
            double l = 0.0, h = 0.0;
            kind[t] = gauss_radau_sums(d, al, off, beta_d, mu, &l, &h);
            L[t] = l * scale;
            U[t] = h * scale;
            dep[t] = d;
        });
    for (int64_t p = 0; p < npairs; ++p) {
        const size_t a = (size_t)2 * p;
        const int f = pair_bracket_combine(L[a], U[a], kind[a], L[a + 1], U[a + 1], kind[a + 1], rtol, ftol, &lo[p],
                                           &hi[p]);
        if (flag) flag[p] = f;
        if (iter) iter[p] = std::max(dep[a], dep[a + 1]);
        if (col_iter) {
            col_iter[a] = dep[a];
            col_iter[a + 1] = dep[a + 1];
        }
    }
}

static bool pow2_le128(int b) { return b >= 1 && b <= 128 && (b & (b - 1)) == 0; }

}  // namespace kt

using namespace kt;

extern "C" int kt_slq_plan(kt_matrix_t A, int64_t nprobes, int* block) {
    if (!A || !block || nprobes < 0) {
        kt::set_error("kt_slq_plan: bad argument");
        return KT_ERR_ARG;
    }
    *block = slq_auto_block(A->n, nprobes);
    return KT_OK;
}

namespace kt {

// The device half of kt_slq_trace: queue the sweeps (their record copies
// land in this call's host slot) and record one event per lane.  Returns the
// ticket; at most two calls may be outstanding per context.
static int slq_submit(kt_matrix_s* A, int fun, int m, uint64_t seed, int64_t probe_offset, int64_t nprobes,
                      int block) {
    if (fun < KT_FUN_EXP || fun > KT_FUN_SQRT) fail(KT_ERR_ARG, "unknown fun code");
    if (m < 1 || m > 256) fail(KT_ERR_ARG, "m must be in [1, 256]");
    if (nprobes < 0 || probe_offset < 0) fail(KT_ERR_ARG, "negative probe range");
    if (block != 0 && !pow2_le128(block)) fail(KT_ERR_ARG, "block must be 0 or a power of two <= 128");
    kt_context_s* ctx = A->ctx;
    Workspace& w = ctx->ws;
    if (w.slq_submitted - w.slq_collected >= 2)
        fail(KT_ERR_ARG, "kt_slq_submit: two calls already outstanding (collect one first)");
    const uint64_t ticket = w.slq_submitted;
    SlqPending& pd = w.slq_pend[ticket & 1];
    const int64_t n = A->n;
    pd.live = false;
    pd.A = A;
    pd.fun = fun;
    pd.m = m;
    pd.seed = seed;
    pd.offset = probe_offset;
    pd.nprobes = (n == 0) ? 0 : nprobes;
    pd.P = block ? block : slq_auto_block(n, std::max<int64_t>(nprobes, 1));
    pd.nsweeps = pd.nprobes ? (pd.nprobes + pd.P - 1) / pd.P : 0;
    // record per sweep: [alpha | up | low][m][P] (+ guard[P] in y-form)
    pd.rec = (size_t)3 * m * pd.P + pd.P;
    // KT_SLQ_LANES=L (<= 4): sweeps round-robin over L streams, so one
    // sweep's small launches (and, in the explicit sweep, its streaming K2)
    // overlap another sweep's gather-bound pass; measured best
    // (profiles/r01_yform_lanes.txt): 2 for the y-form pass, 3 for the
    // explicit K1/K2 sweep
    const int lanes_env = std::max(1, std::min(4, slq_lanes_env(ctx->yform ? 2 : 3)));
    pd.lanes = (int)std::max<int64_t>(1, std::min<int64_t>(pd.nsweeps, lanes_env));
    if (pd.nsweeps) {
        KT_HIP(hipSetDevice(ctx->device));
        PinnedBuf& hb = w.host_trec[ticket & 1];
        hb.ensure(sizeof(double) * pd.rec * pd.nsweeps);
        double* htrec = hb.as<double>();
        const DevCSR& H = hub_csr(A);
        const bool int0 = slq_int0_env() && int0_applies(A->unit_values, H.max_row, m);
        // profiling: the previous calls' events are folded in while this
        // call's sweeps run on the device
        prof_recycle(ctx);
        size_t prev_events[PROF_NSLOTS];
        for (int k = 0; k < PROF_NSLOTS; ++k) prev_events[k] = ctx->prof[k].used;
        // one sweep per lane at a time, the lanes' sweeps queued step by step
        // (launch by launch across the lanes, so every lane starts at once)
        for (int64_t s0 = 0; s0 < pd.nsweeps; s0 += pd.lanes) {
            const int g = (int)std::min<int64_t>(pd.lanes, pd.nsweeps - s0);
            SweepList grp;
            for (int l = 0; l < g; ++l) {
                const int64_t base = probe_offset + (s0 + l) * pd.P;
                double* R = htrec + pd.rec * (s0 + l);
                if (ctx->yform)
                    grp.emplace_back(new YSweep(A, H, pd.P, m, seed, base, R, l, int0));
                else
                    grp.emplace_back(
                        new ExplicitSweep(A, H, pd.P, m, seed, base, nullptr, 0, 0, nullptr, R, nullptr, nullptr, l, 0));
            }
            run_sweeps(grp);
        }
        for (int l = 0; l < pd.lanes; ++l) {
            if (!pd.done[l]) KT_HIP(hipEventCreateWithFlags(&pd.done[l], hipEventDisableTiming));
            KT_HIP(hipEventRecord(pd.done[l], l ? ctx->aux_stream[l - 1] : ctx->stream));
        }
        // (those may still be in flight when the previous submission is not
        // collected yet: wait for them -- this call's sweeps are queued already)
        prof_collect(ctx, prev_events, true);
    }
    pd.live = true;
    ++w.slq_submitted;
    return (int)(ticket & 0x7fffffff);
}

// The host half: wait for the call's sweeps (its lane events only, not work
// submitted after it), redo guarded sweeps with the explicit CGS2 sweep,
// host Gauss quadrature, sums.
static void slq_collect(kt_matrix_s* A, int ticket, double* sum_q, double* sum_q2, double* q) {
    kt_context_s* ctx = A->ctx;
    Workspace& w = ctx->ws;
    if (w.slq_collected == w.slq_submitted || (uint64_t)ticket != (w.slq_collected & 0x7fffffff))
        fail(KT_ERR_ARG, "kt_slq_collect: tickets must be collected once each, in submission order");
    SlqPending& pd = w.slq_pend[w.slq_collected & 1];
    const uint64_t slot = w.slq_collected & 1;
    // the record's n, CSR (guard redo) and lanes belong to the submitting
    // matrix: a call with another matrix is refused BEFORE the ticket is
    // consumed, so the caller can collect it with the right one; a ticket
    // whose matrix was destroyed (its sweeps drained) is consumed
    if (pd.live && pd.A && pd.A != A)
        fail(KT_ERR_ARG, "kt_slq_collect: the ticket was submitted with another matrix");
    ++w.slq_collected;
    if (!pd.live) fail(KT_ERR_ARG, "kt_slq_collect: the submission failed");
    pd.live = false;
    if (pd.A != A) fail(KT_ERR_ARG, "kt_slq_collect: the submitting matrix was destroyed");
    if (sum_q) *sum_q = 0.0;
    if (sum_q2) *sum_q2 = 0.0;
    if (pd.nprobes == 0) return;
    const int64_t n = A->n, nprobes = pd.nprobes;
    const int m = pd.m, P = pd.P, fun = pd.fun;
    const size_t rec = pd.rec;
    double* htrec = w.host_trec[slot].as<double>();
    KT_HIP(hipSetDevice(ctx->device));
    for (int l = 0; l < pd.lanes; ++l) KT_HIP(hipEventSynchronize(pd.done[l]));
    if (ctx->yform) {  // sweeps with a guarded probe are redone by the explicit CGS2 sweep
        const DevCSR& H = hub_csr(A);
        int64_t redone = 0;
        for (int64_t sw = 0; sw < pd.nsweeps; ++sw) {
            const int live = (int)std::min<int64_t>(P, nprobes - sw * P);
            if (!guard_tripped(htrec + rec * sw, m, P, live, nullptr)) continue;
            lanczos_sweep(A, H, P, m, pd.seed, pd.offset + sw * P, nullptr, 0, 0, nullptr, htrec + rec * sw,
                          nullptr, nullptr, 0);
            KT_HIP(hipStreamSynchronize(ctx->stream));
            ++redone;
        }
        ctx->yform_redone += redone;
    }
    // host Gauss quadrature, 16 probes per task on the persistent pool
    // (threads spawned and joined per call cost ~0.1-0.3 ms per call)
    std::vector<double> qv((size_t)nprobes);
    const int64_t chunk = 16;
    HostPool::get().run((int)((nprobes + chunk - 1) / chunk), [&](int t) {
        std::vector<double> al(m), off(m);
        const int64_t pb = t * chunk, pe = std::min<int64_t>(nprobes, pb + chunk);
        for (int64_t p = pb; p < pe; ++p) {
            const int steps = record_tridiag(htrec + rec * (p / P), m, m, P, (int)(p % P), al.data(), off.data());
            qv[p] = (double)n * tridiag_quadrature(steps, al.data(), off.data(), fun);
        }
    }, 4);
    double s1 = 0.0, s2 = 0.0;
    for (int64_t p = 0; p < nprobes; ++p) {
        s1 += qv[p];
        s2 += qv[p] * qv[p];
        if (q) q[p] = qv[p];
    }
    if (sum_q) *sum_q = s1;
    if (sum_q2) *sum_q2 = s2;
}

// ---- the error-controlled probe sweeps (kt_slq_trace_auto) ----
//
// The probe range of kt_slq_trace with each probe's depth chosen by the
// stopping rule of lanczos_columns_adaptive, on resumable y-form sweeps.  The
// check of depth j + 2 (k_quad_check_wide) is queued in the sweep's own stream
// behind step j, so a column's depth is the first depth at which the rule
// holds and the guard value it is judged by is the one it stopped with:
// neither depends on what the host saw or when.  Every kAutoPoll depths the
// sweep's running words are copied to a pinned ring slot behind an event; the
// host reads finished polls without waiting and waits only for the oldest
// when all kAutoRing slots are in flight, so at most
// kAutoPoll kAutoRing + 1 = 9 step passes are queued past the check that
// stopped a sweep's last column, and those are gated: they return at once.
// The lanes run independently: a lane whose sweep has stopped (or reached its
// last step) starts the call's next sweep at once.
//
// The y-form is measured to depth 100 (its Gram identities and guard,
// DESIGN.md §4.1): a y-form sweep runs to min(m_max, kAutoHorizon) rows; with
// columns still running there and m_max beyond, the whole sweep is handed to
// the explicit CGS2 sweep (RNG-seeded at the same P, the test after every
// step up to m_max), as is a sweep with a guarded column.
constexpr int kAutoHorizon = 100, kAutoPoll = 2, kAutoRing = 4, kAutoFirstCheck = kAdaptMinDepth - 2;

namespace {

// one lane's polls of its sweep's running words
struct AutoPoll {
    hipStream_t st = nullptr;
    const int* dwords = nullptr;  // device: ng running words
    volatile int* ring = nullptr;  // pinned: kAutoRing x kGateWordsMax
    hipEvent_t* ev = nullptr;
    int ng = 0, queued = 0, seen = 0;
    bool stopped = false;  // a finished poll read every word zero
    void reset(hipStream_t s, int words) {
        st = s;
        ng = words;
        queued = seen = 0;
        stopped = false;
    }
    // fold in the finished polls; with `room` wait for the oldest while every ring slot is in flight
    void observe(bool room) {
        while (seen < queued && !stopped) {
            const int slot = seen % kAutoRing;
            if (room && queued - seen >= kAutoRing) {
                KT_HIP(hipEventSynchronize(ev[slot]));
            } else {
                const hipError_t q = hipEventQuery(ev[slot]);
                if (q == hipErrorNotReady) {
                    (void)hipGetLastError();
                    return;
                }
                KT_HIP(q);
            }
            int any = 0;
            for (int k = 0; k < ng; ++k) any |= ring[slot * kGateWordsMax + k];
            ++seen;
            if (!any) stopped = true;
        }
    }
    void queue() {
        const int slot = queued % kAutoRing;
        KT_HIP(hipMemcpyAsync(const_cast<int*>(ring) + slot * kGateWordsMax, dwords, sizeof(int) * ng,
                              hipMemcpyDeviceToHost, st));
        KT_HIP(hipEventRecord(ev[slot], st));
        ++queued;
    }
};

// a lane's device block: [state P x kAdaptState | guard snapshot P | running words]
struct AutoDev {
    double* state = nullptr;
    double* gsnap = nullptr;
    int* words = nullptr;
    size_t bytes = 0;
};

AutoDev auto_dev(kt_context_s* ctx, int lane, int P) {
    AutoDev d;
    d.bytes = sizeof(double) * ((size_t)P * kAdaptState + P) + sizeof(int) * kGateWordsMax;
    ctx->ws.auto_state[lane].ensure(d.bytes);
    d.state = ctx->ws.auto_state[lane].as<double>();
    d.gsnap = d.state + (size_t)P * kAdaptState;
    d.words = reinterpret_cast<int*>(d.gsnap + P);
    return d;
}

// zero state, every live column group's word non-zero (running)
void auto_dev_reset(const AutoDev& d, int ng, hipStream_t st) {
    KT_HIP(hipMemsetAsync(d.state, 0, d.bytes, st));
    KT_HIP(hipMemsetAsync(d.words, 1, sizeof(int) * ng, st));
}

void auto_poll_bind(kt_context_s* ctx, int lane, AutoPoll& p) {
    PinnedBuf& pw = ctx->ws.pin_auto;
    pw.ensure(sizeof(int) * 4 * kAutoRing * kGateWordsMax);
    p.ring = pw.as<int>() + (size_t)lane * kAutoRing * kGateWordsMax;
    for (auto& e : ctx->ws.auto_ev[lane])
        if (!e) KT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    p.ev = ctx->ws.auto_ev[lane];
}

// One sweep of `live` probes by the explicit CGS2 sweep on lane 0 with the
// stopping test after every step, until its columns have all stopped or
// reached m rows.  R (host): [record 3 m P | guard P | state | guard snapshot];
// returns the record rows written.  Blocking.
int explicit_auto_sweep(kt_matrix_s* A, const DevCSR& H, int P, int m, int fun, double rtol, uint64_t seed,
                        int64_t base, int live, double* R) {
    kt_context_s* ctx = A->ctx;
    ExplicitSweep e(A, H, P, m, seed, base, nullptr, 0, 0, nullptr, R, nullptr, nullptr, 0, 0);
    hipStream_t st = e.stream();
    const int ng = (live + kWideCheckCols - 1) / kWideCheckCols;
    const AutoDev d = auto_dev(ctx, 0, P);
    AutoPoll poll;
    auto_poll_bind(ctx, 0, poll);
    poll.reset(st, ng);
    poll.dwords = d.words;
    auto_dev_reset(d, ng, st);
    e.start();
    int rows = 0;
    for (int j = 0; j < m; ++j) {
        poll.observe(false);
        if (poll.stopped) break;
        e.step(j);
        rows = j + 1;
        if (rows < kAutoFirstCheck) continue;
        prof_begin(ctx, PROF_CHECK, st, P);
        KT_HIP(launch_quad_check_wide(e.device_record(), m, P, rows, live, 0, nullptr, fun, rtol, d.state, d.words, st));
        prof_end(ctx, PROF_CHECK, st);
        if (rows % kAutoPoll == 0) {
            poll.observe(true);
            if (!poll.stopped) poll.queue();
        }
    }
    e.finish(rows);
    const size_t rec = (size_t)3 * m * P + P;
    KT_HIP(hipMemcpyAsync(R + rec, d.state, sizeof(double) * ((size_t)P * kAdaptState + P), hipMemcpyDeviceToHost,
                          st));
    KT_HIP(hipStreamSynchronize(st));
    return rows;
}

}  // namespace

static void slq_trace_auto(kt_matrix_s* A, int fun, int m_max, double rtol, uint64_t seed, int64_t probe_offset,
                           int64_t nprobes, int block, double* sum_q, double* sum_q2, double* q, int* depth,
                           int64_t* capped) {
    if (fun < KT_FUN_EXP || fun > KT_FUN_SQRT) fail(KT_ERR_ARG, "unknown fun code");
    if (m_max > kAdaptMaxCap) fail(KT_ERR_ARG, "the Lanczos depth cap must be at most 256");
    if (m_max <= 0) m_max = kAdaptDefaultCap;
    if (!(rtol > 0.0)) rtol = kAdaptRtol;
    if (nprobes < 0 || probe_offset < 0) fail(KT_ERR_ARG, "negative probe range");
    if (block != 0 && !pow2_le128(block)) fail(KT_ERR_ARG, "block must be 0 or a power of two <= 128");
    kt_context_s* ctx = A->ctx;
    Workspace& w = ctx->ws;
    if (w.slq_submitted != w.slq_collected)
        fail(KT_ERR_ARG, "kt_slq_trace_auto: kt_slq_submit calls are outstanding on this context");
    if (sum_q) *sum_q = 0.0;
    if (sum_q2) *sum_q2 = 0.0;
    if (capped) *capped = 0;
    const int64_t n = A->n;
    if (n == 0 || nprobes == 0) return;
    const int m = m_max, P = block ? block : slq_auto_block(n, nprobes);
    const int64_t nsw = (nprobes + P - 1) / P;
    const int hy = std::min(m, kAutoHorizon);  // rows a y-form sweep may reach
    // KT_SLQ_LANES=L (<= 4).  Default 4, where the fixed-depth y-form takes 2:
    // a lane spends about a third of its time in its one-workgroup check, which
    // only other lanes' passes can cover (the bench graph, 1,024 probes:
    // 2.0 / 2.9 / 3.4 / 3.5 evaluations/s at 1 / 2 / 3 / 4 lanes)
    const int lanes_env = std::max(1, std::min(4, slq_lanes_env(4)));
    const int lanes = (int)std::max<int64_t>(1, std::min<int64_t>(nsw, lanes_env));
    KT_HIP(hipSetDevice(ctx->device));
    const DevCSR& H = hub_csr(A);
    const bool int0 = slq_int0_env() && int0_applies(A->unit_values, H.max_row, hy);
    // pinned, per sweep: [record 3 m P | guard P | state P x 8 | guard snapshot P]
    const size_t rec = (size_t)3 * m * P + P, per = rec + (size_t)P * kAdaptState + P;
    w.pin_auto_rec.ensure(sizeof(double) * per * nsw);
    double* hrec = w.pin_auto_rec.as<double>();
    std::vector<int> rows((size_t)nsw, 0);
    auto live_of = [&](int64_t i) { return (int)std::min<int64_t>(P, nprobes - i * P); };
    prof_recycle(ctx);
    if (ctx->yform) {
        struct Lane {
            std::unique_ptr<YSweep> y;
            AutoPoll poll;
            AutoDev dev;
            int64_t sweep = -1;
            int j = 0;
        };
        std::vector<Lane> L(lanes);
        int64_t next = 0;
        for (int l = 0; l < lanes; ++l) {
            if (l && !ctx->aux_stream[l - 1])
                KT_HIP(hipStreamCreateWithFlags(&ctx->aux_stream[l - 1], hipStreamNonBlocking));
            L[l].dev = auto_dev(ctx, l, P);
            auto_poll_bind(ctx, l, L[l].poll);
            L[l].poll.dwords = L[l].dev.words;
        }
        auto begin = [&](int l) {
            Lane& s = L[l];
            s.y.reset();
            s.sweep = -1;
            if (next >= nsw) return;
            s.sweep = next++;
            const int ng = (live_of(s.sweep) + kWideCheckCols - 1) / kWideCheckCols;
            s.y.reset(new YSweep(A, H, P, m, seed, probe_offset + s.sweep * P, hrec + per * s.sweep, l, int0,
                                 s.dev.words, ng));
            s.poll.reset(s.y->stream(), ng);
            auto_dev_reset(s.dev, ng, s.y->stream());
            s.y->start();
            s.j = 0;
            rows[s.sweep] = 1;
        };
        auto end = [&](int l) {
            Lane& s = L[l];
            s.y->finish(rows[s.sweep]);
            KT_HIP(hipMemcpyAsync(hrec + per * s.sweep + rec, s.dev.state,
                                  sizeof(double) * ((size_t)P * kAdaptState + P), hipMemcpyDeviceToHost,
                                  s.y->stream()));
        };
        for (int l = 0; l < lanes; ++l) begin(l);
        // one launch group (step, check, poll) per lane in turn, so the lanes' work is queued side by side
        for (bool any = true; any;) {
            any = false;
            for (int l = 0; l < lanes; ++l) {
                Lane& s = L[l];
                if (s.sweep < 0) continue;
                any = true;
                s.poll.observe(false);
                if (s.poll.stopped || s.j + 1 >= hy) {
                    end(l);
                    begin(l);
                    continue;
                }
                s.y->step(s.j);
                const int d = s.j + 2;  // record rows complete after ordinary pass j
                rows[s.sweep] = d;
                ++s.j;
                if (d < kAutoFirstCheck) continue;
                hipStream_t st = s.y->stream();
                prof_begin(ctx, PROF_CHECK, st, P);
                KT_HIP(launch_quad_check_wide(s.y->device_record(), m, P, d, live_of(s.sweep), 0, nullptr, fun, rtol,
                                              s.dev.state, s.dev.words, st, s.y->device_guard(), kYformGuard,
                                              s.dev.gsnap));
                prof_end(ctx, PROF_CHECK, st);
                if (d % kAutoPoll == 0) {
                    s.poll.observe(true);
                    if (!s.poll.stopped) s.poll.queue();
                }
            }
        }
        KT_HIP(hipStreamSynchronize(ctx->stream));
        for (int l = 1; l < lanes; ++l) KT_HIP(hipStreamSynchronize(ctx->aux_stream[l - 1]));
    }
    // sweeps for the explicit path: all of them without the y-form; else the
    // guarded ones (counted as redone) and those still running at the horizon
    int64_t redone = 0;
    for (int64_t i = 0; i < nsw; ++i) {
        double* R = hrec + per * i;
        const int live = live_of(i);
        bool hand = !ctx->yform;
        if (ctx->yform) {
            const double* st = R + rec;
            const double* gs = st + (size_t)P * kAdaptState;
            const double* g = R + (size_t)3 * m * P;
            bool bad = false, running = false;
            for (int c = 0; c < live; ++c) {
                const bool stopped = st[(size_t)c * kAdaptState + 4] != 0.0;
                bad |= !((stopped ? gs[c] : g[c]) >= kYformGuard);
                running |= !stopped;
            }
            if (bad) ++redone;
            hand = bad || (running && hy < m);
        }
        if (hand) rows[i] = explicit_auto_sweep(A, H, P, m, fun, rtol, seed, probe_offset + i * P, live, R);
    }
    ctx->yform_redone += redone;
    // per probe on the host pool: its record truncated at its own depth
    std::vector<double> qv((size_t)nprobes);
    std::vector<int> dep((size_t)nprobes, 0);
    std::vector<char> cap((size_t)nprobes, 0);
    const int64_t chunk = 16;
    HostPool::get().run((int)((nprobes + chunk - 1) / chunk), [&](int t) {
        std::vector<double> al(m), off(m);
        const int64_t pb = t * chunk, pe = std::min<int64_t>(nprobes, pb + chunk);
        for (int64_t p = pb; p < pe; ++p) {
            const int64_t i = p / P;
            const int c = (int)(p % P);
            const double* R = hrec + per * i;
            const double* st = R + rec + (size_t)c * kAdaptState;
            // a column the device did not stop ran every row its sweep wrote
            const bool stopped = st[4] != 0.0;
            const int d = stopped ? (int)st[3] : rows[i];
            const int steps = record_tridiag(R, m, d, P, c, al.data(), off.data());
            cap[p] = !stopped && !(R[(size_t)(2 * m + steps - 1) * P + c] < 1e-8);
            dep[p] = steps;
            qv[p] = (double)n * tridiag_quadrature(steps, al.data(), off.data(), fun);
        }
    }, 4);
    double s1 = 0.0, s2 = 0.0;
    int64_t ncap = 0;
    int dmax = 0;
    for (int64_t p = 0; p < nprobes; ++p) {
        s1 += qv[p];
        s2 += qv[p] * qv[p];
        if (q) q[p] = qv[p];
        if (depth) depth[p] = dep[p];
        ncap += cap[p];
        dmax = std::max(dmax, dep[p]);
    }
    if (sum_q) *sum_q = s1;
    if (sum_q2) *sum_q2 = s2;
    if (capped) *capped = ncap;
    ctx->adapt_max_depth = std::max<int64_t>(ctx->adapt_max_depth, dmax);
    ctx->adapt_capped += ncap;
}

}  // namespace kt

#define KT_SLQ_TRY try {
#define KT_SLQ_CATCH                         \
    }                                        \
    catch (const kt::Status& s) {            \
        kt::set_error(s.msg);                \
        return s.code;                       \
    }                                        \
    catch (const std::exception& e) {        \
        kt::set_error(e.what());             \
        return KT_ERR_ARG;                   \
    }                                        \
    return KT_OK;

extern "C" int kt_slq_trace(kt_matrix_t A, int fun, int m, uint64_t seed, int64_t probe_offset,
                            int64_t nprobes, int block, double* sum_q, double* sum_q2, double* q) {
    KT_SLQ_TRY
    if (!A) fail(KT_ERR_ARG, "A is NULL");
    Workspace& w = A->ctx->ws;
    if (w.slq_submitted != w.slq_collected)
        fail(KT_ERR_ARG, "kt_slq_trace: kt_slq_submit calls are outstanding on this context");
    const int t = slq_submit(A, fun, m, seed, probe_offset, nprobes, block);
    slq_collect(A, t, sum_q, sum_q2, q);
    KT_SLQ_CATCH
}

extern "C" int kt_slq_submit(kt_matrix_t A, int fun, int m, uint64_t seed, int64_t probe_offset,
                             int64_t nprobes, int block, int* ticket) {
    KT_SLQ_TRY
    if (!A || !ticket) fail(KT_ERR_ARG, "NULL argument");
    *ticket = slq_submit(A, fun, m, seed, probe_offset, nprobes, block);
    KT_SLQ_CATCH
}

extern "C" int kt_slq_collect(kt_matrix_t A, int ticket, double* sum_q, double* sum_q2, double* q) {
    KT_SLQ_TRY
    if (!A) fail(KT_ERR_ARG, "A is NULL");
    slq_collect(A, ticket, sum_q, sum_q2, q);
    KT_SLQ_CATCH
}

extern "C" int kt_slq_trace_auto(kt_matrix_t A, int fun, int m_max, double rtol, uint64_t seed,
                                 int64_t probe_offset, int64_t nprobes, int block, double* sum_q, double* sum_q2,
                                 double* q, int* depth, int64_t* capped) {
    KT_SLQ_TRY
    if (!A) fail(KT_ERR_ARG, "A is NULL");
    slq_trace_auto(A, fun, m_max, rtol, seed, probe_offset, nprobes, block, sum_q, sum_q2, q, depth, capped);
    KT_SLQ_CATCH
}
